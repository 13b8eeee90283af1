"""Batch entry points (host buffers in, results out) and device-pointer entry points for callers that keep
their inputs resident in HBM (bench.py uses torch tensors only as device memory + stream plumbing)."""
import ctypes as C

from . import _native as N


def _c():
    return N.default_context()


def _moff(msg_offsets):
    """n + 1 byte offsets into the message buffer (messages of any length each), or None for msg_len bytes per item"""
    return None if msg_offsets is None else (C.c_uint64 * len(msg_offsets))(*msg_offsets)


def fast_aggregate_verify_batch(sigs, msgs, pks, n, k=None, pk_format=N.PK_COMPRESSED, msg_len=32, pk_offsets=None, ctx=None, msg_offsets=None):
    """n x AggregateSignature::fast_aggregate_verify (reference src/aggregates.rs:177-215).
    Returns (results: list[bool], status: list[int])."""
    ctx = ctx or _c()
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    off = None
    if pk_offsets is not None:
        off = (C.c_uint32 * len(pk_offsets))(*pk_offsets)
        k = 0
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch(ctx.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), N.cbuf(pks), pk_format,
                                                       off, n, k, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def fast_aggregate_verify_batch_indexed(table, sigs, msgs, key_idx, n, k=None, msg_len=32, offsets=None, ctx=None, msg_offsets=None):
    """The same over a resident key table: item i uses table entries key_idx[k*i : k*i+k] (or key_idx[offsets[i]:offsets[i+1]])."""
    ctx = ctx or table.ctx
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    idx = (C.c_uint32 * max(1, len(key_idx)))(*key_idx)
    off = None
    if offsets is not None:
        off = (C.c_uint32 * len(offsets))(*offsets)
        k = 0
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_indexed(ctx.handle, table.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), idx, off, n, k, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def _midx(msg_idx, n):
    if len(msg_idx) != n:
        raise ValueError("msg_idx must have n = %d entries, got %d" % (n, len(msg_idx)))
    return (C.c_uint32 * max(1, n))(*msg_idx)


def fast_aggregate_verify_batch_shared_msgs(sigs, msgs, n_msgs, msg_idx, pks, n, k=None, pk_format=N.PK_COMPRESSED, msg_len=32, pk_offsets=None, ctx=None,
                                            msg_offsets=None):
    """fast_aggregate_verify_batch over a LIST of n_msgs messages (msg_len bytes each, or msg_offsets of n_msgs + 1 entries): item i's message is message
    msg_idx[i]; every listed message is hashed once. Same (results, status) as fast_aggregate_verify_batch with the messages spelled out per item."""
    ctx = ctx or _c()
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    off = None
    if pk_offsets is not None:
        off = (C.c_uint32 * len(pk_offsets))(*pk_offsets)
        k = 0
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_shared_msgs(ctx.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), n_msgs, _midx(msg_idx, n),
                                                                   N.cbuf(pks), pk_format, off, n, k, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def fast_aggregate_verify_batch_indexed_shared_msgs(table, sigs, msgs, n_msgs, msg_idx, key_idx, n, k=None, msg_len=32, offsets=None, ctx=None, msg_offsets=None):
    """The same over a resident key table: keys by table index (as fast_aggregate_verify_batch_indexed), messages by list index."""
    ctx = ctx or table.ctx
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    idx = (C.c_uint32 * max(1, len(key_idx)))(*key_idx)
    off = None
    if offsets is not None:
        off = (C.c_uint32 * len(offsets))(*offsets)
        k = 0
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_indexed_shared_msgs(ctx.handle, table.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), n_msgs,
                                                                           _midx(msg_idx, n), idx, off, n, k, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def verify_batch_shared_msgs(sigs, msgs, n_msgs, msg_idx, pks, n, pk_format=N.PK_COMPRESSED, msg_len=32, ctx=None, msg_offsets=None):
    """verify_batch (n x Signature::verify) over a list of n_msgs messages: item i's message is message msg_idx[i]."""
    ctx = ctx or _c()
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    ctx.check(N.lib().mbls_verify_batch_shared_msgs(ctx.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), n_msgs, _midx(msg_idx, n), N.cbuf(pks),
                                                    pk_format, n, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def fast_aggregate_verify_batch_msgtable(msg_table, sigs, msg_idx, pks, n, k=None, pk_format=N.PK_COMPRESSED, pk_offsets=None, ctx=None):
    """fast_aggregate_verify_batch over a resident message table (N.MsgTable): item i's message is entry msg_idx[i]; nothing is hashed. Same (results, status)
    as fast_aggregate_verify_batch with the messages spelled out per item; an index that names no entry raises (MBLS_ERR_ARGUMENT)."""
    ctx = ctx or msg_table.ctx
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    off = None
    if pk_offsets is not None:
        off = (C.c_uint32 * len(pk_offsets))(*pk_offsets)
        k = 0
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_msgtable(ctx.handle, N.cbuf(sigs), msg_table.handle, _midx(msg_idx, n), N.cbuf(pks), pk_format, off, n, k, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def fast_aggregate_verify_batch_indexed_msgtable(table, msg_table, sigs, msg_idx, key_idx, n, k=None, offsets=None, ctx=None):
    """The same over a resident key table: keys by key-table index, messages by message-table index."""
    ctx = ctx or table.ctx
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    idx = (C.c_uint32 * max(1, len(key_idx)))(*key_idx)
    off = None
    if offsets is not None:
        off = (C.c_uint32 * len(offsets))(*offsets)
        k = 0
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_indexed_msgtable(ctx.handle, table.handle, N.cbuf(sigs), msg_table.handle, _midx(msg_idx, n), idx, off, n, k,
                                                                        res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def _bits(bits, bits_stride, n):
    bits = bytes(bits)
    if len(bits) != bits_stride * n:
        raise ValueError("bits must hold n = %d bitfields of bits_stride = %d bytes, got %d bytes" % (n, bits_stride, len(bits)))
    return N.cbuf(bits)


def fast_aggregate_verify_batch_committee(committees, sigs, msgs, cmt_idx, bits, bits_stride, n, msg_len=32, ctx=None, msg_offsets=None):
    """fast_aggregate_verify_batch over a committee table (N.CommitteeTable): item i's keys are the members of committee cmt_idx[i] whose bit is set in the
    bits_stride bytes at bits[bits_stride * i:] (SSZ bit order; bits at or above the committee's size are ignored). Same (results, status) as
    fast_aggregate_verify_batch_indexed with the selected members spelled out; a committee id that names nothing raises (MBLS_ERR_ARGUMENT)."""
    ctx = ctx or committees.ctx
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_committee(ctx.handle, committees.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets),
                                                                 _midx(cmt_idx, n), _bits(bits, bits_stride, n), bits_stride, n, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def fast_aggregate_verify_batch_committee_msgtable(committees, msg_table, sigs, msg_idx, cmt_idx, bits, bits_stride, n, ctx=None):
    """The same with the messages by message-table index."""
    ctx = ctx or committees.ctx
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_committee_msgtable(ctx.handle, committees.handle, N.cbuf(sigs), msg_table.handle, _midx(msg_idx, n),
                                                                          _midx(cmt_idx, n), _bits(bits, bits_stride, n), bits_stride, n, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def _span(cmt_id_lists, fields, bits_stride):
    """a list of id lists and one bitfield per item -> (ids, n_ids, absolute offsets, the fields padded to bits_stride bytes each)"""
    if len(cmt_id_lists) != len(fields):
        raise ValueError("one id list and one bitfield per item")
    ids, off = [], [0]
    for l in cmt_id_lists:
        ids.extend(l)
        off.append(len(ids))
    buf = bytearray()
    for f in fields:
        f = bytes(f)
        if len(f) > bits_stride:
            raise ValueError("a bitfield of %d bytes does not fit bits_stride = %d" % (len(f), bits_stride))
        buf += f + bytes(bits_stride - len(f))
    return (C.c_uint32 * max(1, len(ids)))(*ids), len(ids), (C.c_uint32 * len(off))(*off), N.cbuf(bytes(buf))


def fast_aggregate_verify_batch_committee_span(committees, sigs, msgs, cmt_id_lists, fields, bits_stride, msg_len=32, ctx=None, msg_offsets=None):
    """fast_aggregate_verify_batch over spans of committees (include/mbls.h, "committee spans"): item i names the committees cmt_id_lists[i] (at most
    N.SPAN_MAX_COMMITTEES) and fields[i] is ONE bitfield over their concatenated members (SSZ bit order; an Electra attestation's aggregation_bits; shorter fields
    are zero-padded to bits_stride bytes, a multiple of 4). Same (results, status) as fast_aggregate_verify_batch_indexed with the selected members spelled out in
    (segment, member) order; a malformed item raises (MBLS_ERR_ARGUMENT)."""
    ctx = ctx or committees.ctx
    n = len(cmt_id_lists)
    ids, n_ids, off, bits = _span(cmt_id_lists, fields, bits_stride)
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_committee_span(ctx.handle, committees.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), ids, n_ids,
                                                                      off, bits, bits_stride, n, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def fast_aggregate_verify_batch_committee_span_msgtable(committees, msg_table, sigs, msg_idx, cmt_id_lists, fields, bits_stride, ctx=None):
    """The same with the messages by message-table index."""
    ctx = ctx or committees.ctx
    n = len(cmt_id_lists)
    ids, n_ids, off, bits = _span(cmt_id_lists, fields, bits_stride)
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    ctx.check(N.lib().mbls_fast_aggregate_verify_batch_committee_span_msgtable(ctx.handle, committees.handle, N.cbuf(sigs), msg_table.handle, _midx(msg_idx, n), ids,
                                                                               n_ids, off, bits, bits_stride, n, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def set_committee_route(mode, ctx=None):
    """committee entries: N.CMT_ROUTE_AUTO (complement when eligible and cheaper), N.CMT_ROUTE_DIRECT, N.CMT_ROUTE_COMPLEMENT (whenever eligible)"""
    ctx = ctx or _c()
    ctx.check(N.lib().mbls_ctx_set_committee_route(ctx.handle, mode))


def verify_batch_msgtable(msg_table, sigs, msg_idx, pks, n, pk_format=N.PK_COMPRESSED, ctx=None):
    """verify_batch (n x Signature::verify) over a resident message table: item i's message is entry msg_idx[i]."""
    ctx = ctx or msg_table.ctx
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    ctx.check(N.lib().mbls_verify_batch_msgtable(ctx.handle, N.cbuf(sigs), msg_table.handle, _midx(msg_idx, n), N.cbuf(pks), pk_format, n, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def aggregate_signatures_batch(sigs96, n, k=None, offsets=None, ctx=None):
    """n x AggregateSignature::aggregate (reference src/aggregates.rs:100-106) -> (compressed sums, errs)"""
    ctx = ctx or _c()
    out, errs = N.outbuf(96 * n), N.outbuf(n)
    off = None
    if offsets is not None:
        off = (C.c_uint32 * len(offsets))(*offsets)
        k = 0
    ctx.check(N.lib().mbls_aggregate_signatures_batch(ctx.handle, N.cbuf(sigs96), off, n, k, out, errs))
    return bytes(out)[:96 * n], list(bytes(errs)[:n])


def aggregate_verify_batch(sigs, msgs, pks96, n, k=None, pair_offsets=None, msg_len=32, msg_offsets=None, ctx=None):
    """n x AggregateSignature::aggregate_verify (reference src/aggregates.rs:130-170): the (message, key) pairs of all items back to back;
    item i owns pairs [pair_offsets[i], pair_offsets[i+1]) or k each. Returns (results, status)."""
    ctx = ctx or _c()
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    off = None
    if (k is None) == (pair_offsets is None):
        raise ValueError("aggregate_verify_batch: give exactly one of k (pairs per item) and pair_offsets (n + 1 entries)")
    if pair_offsets is not None:
        if len(pair_offsets) != n + 1:
            raise ValueError("aggregate_verify_batch: pair_offsets must have n + 1 = %d entries, got %d" % (n + 1, len(pair_offsets)))
        if pair_offsets and not 0 <= pair_offsets[-1] <= 0xFFFFFFFF:
            raise ValueError("aggregate_verify_batch: pair indices are 32-bit")
        off = (C.c_uint32 * len(pair_offsets))(*pair_offsets)
        k = 0
    elif not 0 <= k * n <= 0xFFFFFFFF:
        raise ValueError("aggregate_verify_batch: pair indices are 32-bit")
    ctx.check(N.lib().mbls_aggregate_verify_batch(ctx.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), N.cbuf(pks96), off, k, n, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def verify_batch(sigs, msgs, pks, n, pk_format=N.PK_COMPRESSED, msg_len=32, ctx=None, msg_offsets=None):
    """n x Signature::verify (reference src/signature.rs:27-40)."""
    ctx = ctx or _c()
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    ctx.check(N.lib().mbls_verify_batch(ctx.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), N.cbuf(pks), pk_format, n, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def pk_decode_batch(data, n, in_format=N.PK_COMPRESSED, validate=True, ctx=None):
    ctx = ctx or _c()
    out, errs = N.outbuf(96 * n), N.outbuf(n)
    ctx.check(N.lib().mbls_pk_decode_batch(ctx.handle, N.cbuf(data), in_format, int(validate), n, out, errs))
    return bytes(out)[:96 * n], list(bytes(errs)[:n])


def pk_compress_batch(data96, n, ctx=None):
    ctx = ctx or _c()
    out, errs = N.outbuf(48 * n), N.outbuf(n)
    ctx.check(N.lib().mbls_pk_compress_batch(ctx.handle, N.cbuf(data96), n, out, errs))
    return bytes(out)[:48 * n], list(bytes(errs)[:n])


def sig_check_batch(data96, n, ctx=None):
    ctx = ctx or _c()
    errs, g2 = N.outbuf(n), N.outbuf(n)
    ctx.check(N.lib().mbls_sig_check_batch(ctx.handle, N.cbuf(data96), n, errs, g2))
    return list(bytes(errs)[:n]), [bool(x) for x in bytes(g2)[:n]]


def sign_batch(sks32, msgs, n, msg_len=32, ctx=None):
    ctx = ctx or _c()
    out = N.outbuf(96 * n)
    ctx.check(N.lib().mbls_sign_batch(ctx.handle, N.cbuf(sks32), N.cbuf(msgs), msg_len, n, out))
    return bytes(out)[:96 * n]


def sk_to_pk_batch(sks32, n, out_format=N.PK_COMPRESSED, ctx=None):
    ctx = ctx or _c()
    sz = 48 if out_format == N.PK_COMPRESSED else 96
    out = N.outbuf(sz * n)
    ctx.check(N.lib().mbls_sk_to_pk_batch(ctx.handle, N.cbuf(sks32), out_format, n, out))
    return bytes(out)[:sz * n]


def hash_to_g2_batch(msgs, n, msg_len=32, ctx=None, mode=0):
    """n x hash_to_curve_g2, compressed; mode 0: the stand-alone lane body, 1 / 2: the verification pipeline's message phase with one lane /
    one wave per item (include/mbls.h, mbls_hash_to_g2_batch_mode)"""
    ctx = ctx or _c()
    out = N.outbuf(96 * n)
    ctx.check(N.lib().mbls_hash_to_g2_batch_mode(ctx.handle, N.cbuf(msgs), msg_len, n, out, mode))
    return bytes(out)[:96 * n]


def map_to_g2_batch(u, n, mode=1, ctx=None):
    """test probe (include/mbls.h, mbls_map_to_g2_probe): hash_to_curve_g2 after hash_to_field on n pairs of field elements; u = a list of
    ((c0, c1), (c0, c1)) integer pairs (u0, u1) or 192 n packed bytes (u0.c0, u0.c1, u1.c0, u1.c1, 48 bytes big-endian each). mode 0: the
    compiled lane body, 1 / 2 / 3 as hash_to_g2_batch. n compressed points"""
    ctx = ctx or _c()
    if not isinstance(u, (bytes, bytearray)):
        u = b"".join(int(c).to_bytes(48, "big") for u0, u1 in u for c in (u0[0], u0[1], u1[0], u1[1]))
    if len(u) != 192 * n:
        raise ValueError("map_to_g2_batch takes 192 bytes per item")
    out = N.outbuf(96 * n)
    ctx.check(N.lib().mbls_map_to_g2_probe(ctx.handle, N.cbuf(u), n, out, mode))
    return bytes(out)[:96 * n]


MILLER_MODES = {"body": 0, "two_pair": 1, "one_pair": 2, "one_pair_lane_pair": 3, "miller1": 4, "smiller": 5}
FINAL_EXP_MODES = {"body": 0, "lane": 1, "lane_pair": 2, "vmfinal": 3}


def miller_probe(operands, n, mode, ctx=None):
    """test probe (include/mbls.h, mbls_miller_probe): the Miller loop of n items in the form `mode` names (MILLER_MODES); operands = 624 n packed bytes
    (apk X, Y, Z; sig x.c0, x.c1, y.c0, y.c1; H X.c0 .. Z.c1, 48 bytes big-endian each). 576 n bytes: the 12 coefficients of each value in the order of slot F"""
    ctx = ctx or _c()
    if len(operands) != 624 * n:
        raise ValueError("miller_probe takes 624 bytes per item")
    out = N.outbuf(576 * n)
    ctx.check(N.lib().mbls_miller_probe(ctx.handle, N.cbuf(operands), n, out, MILLER_MODES.get(mode, mode)))
    return bytes(out)[:576 * n]


def final_exp_probe(f, n, mode, ctx=None):
    """test probe (include/mbls.h, mbls_final_exp_probe): the final exponentiation of n elements of Fp12 (576 n packed bytes) in the form `mode` names
    (FINAL_EXP_MODES). (values: 576 n bytes, or None for the verdict-only form; is_one: n bools; lanes_equal: n bools for the lane-pair form, else None)"""
    ctx = ctx or _c()
    if len(f) != 576 * n:
        raise ValueError("final_exp_probe takes 576 bytes per item")
    mode = FINAL_EXP_MODES.get(mode, mode)
    out, bits = N.outbuf(576 * n), N.outbuf(n)
    ctx.check(N.lib().mbls_final_exp_probe(ctx.handle, N.cbuf(f), n, out, bits, mode))
    bits = bytes(bits)[:n]
    return (None if mode == 3 else bytes(out)[:576 * n], [bool(b & 1) for b in bits], [bool(b & 2) for b in bits] if mode == 2 else None)


def aggregate_public_keys_batch(pks, n, k=None, pk_format=N.PK_COMPRESSED, pk_offsets=None, ctx=None):
    ctx = ctx or _c()
    out = N.outbuf(96 * n)
    st = (C.c_uint32 * max(1, n))()
    off = None
    if pk_offsets is not None:
        off = (C.c_uint32 * len(pk_offsets))(*pk_offsets)
        k = 0
    ctx.check(N.lib().mbls_aggregate_public_keys_batch(ctx.handle, N.cbuf(pks), pk_format, off, n, k, out, st))
    return bytes(out)[:96 * n], list(st)[:n]


def fp_mul_batch(a48, b48, n, square=False, ctx=None, op=None):
    """field probe; op as in include/mbls.h (default: 1 if square else 0)"""
    ctx = ctx or _c()
    out = N.outbuf(48 * n)
    ctx.check(N.lib().mbls_fp_mul_batch(ctx.handle, N.cbuf(a48), N.cbuf(b48), n, out, int(square) if op is None else op))
    return bytes(out)[:48 * n]


def dform_probe_shape(op):
    """(input words, output words) per lane of probe `op` (include/mbls.h mbls_dform_probe)"""
    nin, nout = C.c_uint32(), C.c_uint32()
    if N.lib().mbls_dform_probe_shape(op, C.byref(nin), C.byref(nout)) != 0:
        raise ValueError("no such probe: %r" % (op,))
    return nin.value, nout.value


def dform_probe(op, words, n, ctx=None):
    """raw-register probe of a generated digit-form body: words = n_in * n unsigned 32-bit register contents, word-major (word w of lane i at w * n + i);
    returns the n_out * n register contents the probe stores, in the same layout"""
    ctx = ctx or _c()
    nin, nout = dform_probe_shape(op)
    if len(words) != nin * n:
        raise ValueError("probe %d takes %d words per lane" % (op, nin))
    src = (C.c_uint32 * max(1, nin * n))(*words)
    out = (C.c_uint32 * max(1, nout * n))()
    ctx.check(N.lib().mbls_dform_probe(ctx.handle, op, src, n, out))
    return list(out)[:nout * n]


def fp_mul_bench(n_lanes, iters, ctx=None):
    """Integer-ALU calibration: `iters` dependent Fp multiplications on each of n_lanes lanes -> elapsed ms."""
    ctx = ctx or _c()
    ms = C.c_float()
    ctx.check(N.lib().mbls_fp_mul_bench(ctx.handle, n_lanes, iters, C.byref(ms)))
    return ms.value


def verify_multiple_sets_device(d_sigs, d_pks, d_msgs, d_rands, n, k, pk_format=N.PK_COMPRESSED, msg_len=32, stream=None, ctx=None, d_result=None, d_status=None):
    """AggregateSignature::verify_multiple_aggregate_signatures (reference src/aggregates.rs:261-316) over n sets given by
    their k wire-format keys each, everything resident on the device (raw device pointers / ints). The C entry only enqueues: the bool
    arrives in the device byte d_result (and the OR of the sets' status bits in the device word d_status). Without d_result this wrapper
    provides both (torch tensors), synchronises and returns the bool."""
    ctx = ctx or _c()
    if d_result is not None:
        ctx.check(N.lib().mbls_verify_multiple_sets_device(ctx.handle, d_sigs, d_pks, pk_format, None, k, d_msgs, msg_len, None, d_rands, n,
                                                           d_result, d_status, stream))
        return None
    import torch
    res = torch.full((8,), 7, dtype=torch.uint8, device="cuda")
    ctx.check(N.lib().mbls_verify_multiple_sets_device(ctx.handle, d_sigs, d_pks, pk_format, None, k, d_msgs, msg_len, None, d_rands, n,
                                                       res.data_ptr(), None, stream))
    torch.cuda.synchronize()
    v = int(res[0].item())
    assert v in (0, 1)
    return bool(v)


def verify_multiple_sets_indexed_device(table, d_sigs, d_key_idx, d_msgs, d_rands, n, k, msg_len=32, stream=None, ctx=None, d_result=None, d_status=None, d_partial=None,
                                        d_offsets=None):
    """verify_multiple over sets named by indices into a resident KeyTable (raw device pointers). With d_result or d_partial the call only enqueues;
    without both it synchronises and returns the bool."""
    ctx = ctx or _c()
    f = N.lib().mbls_verify_multiple_sets_indexed_device
    if d_result is not None or d_partial is not None:
        ctx.check(f(ctx.handle, table.handle, d_sigs, d_key_idx, d_offsets, k, d_msgs, msg_len, None, d_rands, n, d_result, d_status, d_partial, stream))
        return None
    import torch
    res = torch.full((8,), 7, dtype=torch.uint8, device="cuda")
    ctx.check(f(ctx.handle, table.handle, d_sigs, d_key_idx, d_offsets, k, d_msgs, msg_len, None, d_rands, n, res.data_ptr(), d_status, None, stream))
    torch.cuda.synchronize()
    v = int(res[0].item())
    assert v in (0, 1)
    return bool(v)


def verify_multiple_partial_device(d_sigs, d_msgs, d_rands, n, d_partial, d_apks=None, d_pks=None, k=0, pk_format=N.PK_COMPRESSED, msg_len=32, stream=None, ctx=None):
    """One shard of a verify_multiple that is spread over several devices or processes (include/mbls.h): the shard's
    Miller product, signature sum and status bits as one N.VM_PARTIAL_BYTES record at the device address d_partial. Enqueues only."""
    ctx = ctx or _c()
    ctx.check(N.lib().mbls_verify_multiple_partial_device(ctx.handle, d_sigs, d_apks, d_pks, pk_format, None, k, d_msgs, msg_len, None, d_rands, n, d_partial, stream))


def verify_multiple_finish_device(d_partials, n_partials, d_result=None, d_status=None, stream=None, ctx=None):
    """The records of all shards (n_partials x N.VM_PARTIAL_BYTES at d_partials, the same order on every participant) -> the bool of the
    one-device call over the concatenated sets. With d_result the call only enqueues; without, it synchronises and returns the bool."""
    ctx = ctx or _c()
    if d_result is not None:
        ctx.check(N.lib().mbls_verify_multiple_finish_device(ctx.handle, d_partials, n_partials, d_result, d_status, stream))
        return None
    import torch
    res = torch.full((8,), 7, dtype=torch.uint8, device="cuda")
    ctx.check(N.lib().mbls_verify_multiple_finish_device(ctx.handle, d_partials, n_partials, res.data_ptr(), d_status, stream))
    torch.cuda.synchronize()
    v = int(res[0].item())
    assert v in (0, 1)
    return bool(v)


def multi_verify_multiple_aggregate_signatures(mctx, sigs, apks, msgs, rands, n, msg_len=32, msg_offsets=None):
    """verify_multiple_aggregate_signatures (reference src/aggregates.rs:261-316) sharded over the devices of a MultiContext: host buffers
    (sigs 96 B each, decoded aggregate keys 96 B each, messages, 64-bit scalars) -> bool"""
    r = (C.c_uint64 * max(1, n))(*rands)
    return bool(N.lib().mbls_multi_verify_multiple_aggregate_signatures(mctx.handle, N.cbuf(sigs), N.cbuf(apks), N.cbuf(msgs), msg_len, _moff(msg_offsets), r, n))


def multi_fast_aggregate_verify_batch(mctx, sigs, msgs, pks, n, k=None, pk_format=N.PK_COMPRESSED, msg_len=32, pk_offsets=None, msg_offsets=None):
    """fast_aggregate_verify_batch sharded over the devices of a MultiContext (include/mbls.h, mbls_multi_*)"""
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    off = None
    if pk_offsets is not None:
        off = (C.c_uint32 * len(pk_offsets))(*pk_offsets)
        k = 0
    mctx.check(N.lib().mbls_multi_fast_aggregate_verify_batch(mctx.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), N.cbuf(pks), pk_format,
                                                              off, n, k, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def multi_fast_aggregate_verify_bitmap(mctx, sigs, msgs, pks, n, k=None, pk_format=N.PK_COMPRESSED, msg_len=32, pk_offsets=None, msg_offsets=None):
    """The same with the results as ONE packed accept bitmap that every device of the handle ends up holding (all-gather between the devices: RCCL when
    mctx.rccl_active, host memory otherwise). -> (bits, status, words): bits[i] = item i accepted, words = the ceil(n / 64) bitmap words of the first device."""
    words = (C.c_uint64 * max(1, (n + 63) // 64))()
    st = (C.c_uint32 * max(1, n))()
    off = None
    if pk_offsets is not None:
        off = (C.c_uint32 * len(pk_offsets))(*pk_offsets)
        k = 0
    mctx.check(N.lib().mbls_multi_fast_aggregate_verify_bitmap(mctx.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), N.cbuf(pks), pk_format,
                                                               off, n, k, words, st))
    w = list(words)[:(n + 63) // 64]
    return [bool((w[i // 64] >> (i % 64)) & 1) for i in range(n)], list(st)[:n], w


def multi_verify_batch(mctx, sigs, msgs, pks, n, pk_format=N.PK_COMPRESSED, msg_len=32, msg_offsets=None):
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    mctx.check(N.lib().mbls_multi_verify_batch(mctx.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets), N.cbuf(pks), pk_format, n, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def multi_fast_aggregate_verify_batch_indexed(mctx, mtable, sigs, msgs, key_idx, n, k=None, msg_len=32, offsets=None, msg_offsets=None):
    res = N.outbuf(n)
    st = (C.c_uint32 * max(1, n))()
    idx = (C.c_uint32 * max(1, len(key_idx)))(*key_idx)
    off = None
    if offsets is not None:
        off = (C.c_uint32 * len(offsets))(*offsets)
        k = 0
    mctx.check(N.lib().mbls_multi_fast_aggregate_verify_batch_indexed(mctx.handle, mtable.handle, N.cbuf(sigs), N.cbuf(msgs), msg_len, _moff(msg_offsets),
                                                                      idx, off, n, k, res, st))
    return [bool(x) for x in bytes(res)[:n]], list(st)[:n]


def _boff(batch_offsets):
    return None if batch_offsets is None else (C.c_uint32 * len(batch_offsets))(*batch_offsets)


def verify_multiple_batches(sigs, apks, msgs, rands, n_sets, n_batches, batch_offsets=None, sets_per_batch=0, msg_len=32, msg_offsets=None, ctx=None):
    """n_batches x verify_multiple_aggregate_signatures (reference src/aggregates.rs:261-316) in ONE call (mbls_verify_multiple_batches): the sets of all
    batches back to back, batch b owning sets [batch_offsets[b], batch_offsets[b+1]) or sets_per_batch each; host buffers (signatures 96 B, decoded aggregate
    keys 96 B, messages, one nonzero 64-bit scalar per set). Returns (results: list[bool], status: list[int]), one entry per batch."""
    ctx = ctx or _c()
    res = N.outbuf(max(1, n_batches))
    st = (C.c_uint32 * max(1, n_batches))()
    r = None if rands is None else (C.c_uint64 * max(1, n_sets))(*rands)
    ctx.check(N.lib().mbls_verify_multiple_batches(ctx.handle, N.cbuf(sigs), N.cbuf(apks), N.cbuf(msgs), msg_len, _moff(msg_offsets), r, n_sets,
                                                   _boff(batch_offsets), sets_per_batch, n_batches, res, st))
    return [bool(x) for x in bytes(res)[:n_batches]], list(st)[:n_batches]


def verify_multiple_batches_device(d_sigs, d_msgs, d_rands, n_sets, n_batches, d_results, d_status=None, d_apks=None, d_pks=None, k=0, pk_format=N.PK_COMPRESSED,
                                   d_pk_offsets=None, msg_len=32, d_msg_offsets=None, d_batch_offsets=None, sets_per_batch=0, stream=None, ctx=None):
    """The same over device buffers (raw device pointers / ints): keys as one aggregate key per set (d_apks) or wire-format keys (d_pks, k or d_pk_offsets).
    Enqueues only: n_batches result bytes at d_results, n_batches status words at d_status (optional)."""
    ctx = ctx or _c()
    ctx.check(N.lib().mbls_verify_multiple_batches_device(ctx.handle, d_sigs, d_apks, d_pks, pk_format, d_pk_offsets, k, d_msgs, msg_len, d_msg_offsets, d_rands,
                                                          n_sets, d_batch_offsets, sets_per_batch, n_batches, d_results, d_status, stream))


def verify_multiple_batches_indexed_device(table, d_sigs, d_key_idx, d_msgs, d_rands, n_sets, n_batches, d_results, d_status=None, k=0, d_offsets=None, msg_len=32,
                                           d_msg_offsets=None, d_batch_offsets=None, sets_per_batch=0, stream=None, ctx=None):
    """The same over sets named by indices into a resident KeyTable (the deployment's form). Enqueues only."""
    ctx = ctx or table.ctx
    ctx.check(N.lib().mbls_verify_multiple_batches_indexed_device(ctx.handle, table.handle, d_sigs, d_key_idx, d_offsets, k, d_msgs, msg_len, d_msg_offsets, d_rands,
                                                                  n_sets, d_batch_offsets, sets_per_batch, n_batches, d_results, d_status, stream))


# ---- which sets of a rejected batch (include/mbls.h, mbls_verify_multiple_batches_locate*)
def verify_multiple_batches_locate(sigs, apks, msgs, rands, n_sets, n_batches, batch_offsets=None, sets_per_batch=0, msg_len=32, msg_offsets=None, ctx=None):
    """verify_multiple_batches, and in the same call one answer per SET (mbls_verify_multiple_batches_locate): every set of an accepted batch reads True (a passing
    batch is not examined), every set of a rejected batch reads what the one-set batch with its scalar returns. Returns (results, status, set_results,
    set_status): the first two per batch as verify_multiple_batches returns them, the last two per set."""
    ctx = ctx or _c()
    res = N.outbuf(max(1, n_batches))
    st = (C.c_uint32 * max(1, n_batches))()
    sres = N.outbuf(max(1, n_sets))
    sst = (C.c_uint32 * max(1, n_sets))()
    r = None if rands is None else (C.c_uint64 * max(1, n_sets))(*rands)
    ctx.check(N.lib().mbls_verify_multiple_batches_locate(ctx.handle, N.cbuf(sigs), N.cbuf(apks), N.cbuf(msgs), msg_len, _moff(msg_offsets), r, n_sets,
                                                          _boff(batch_offsets), sets_per_batch, n_batches, res, st, sres, sst))
    return [bool(x) for x in bytes(res)[:n_batches]], list(st)[:n_batches], [bool(x) for x in bytes(sres)[:n_sets]], list(sst)[:n_sets]


def verify_multiple_batches_locate_device(d_sigs, d_msgs, d_rands, n_sets, n_batches, d_results, d_set_results, d_status=None, d_set_status=None, d_apks=None,
                                          d_pks=None, k=0, pk_format=N.PK_COMPRESSED, d_pk_offsets=None, msg_len=32, d_msg_offsets=None, d_batch_offsets=None,
                                          sets_per_batch=0, stream=None, ctx=None):
    """The same over device buffers, as verify_multiple_batches_device: n_sets result bytes at d_set_results (required), n_sets status words at d_set_status
    (optional). Enqueues only."""
    ctx = ctx or _c()
    ctx.check(N.lib().mbls_verify_multiple_batches_locate_device(ctx.handle, d_sigs, d_apks, d_pks, pk_format, d_pk_offsets, k, d_msgs, msg_len, d_msg_offsets, d_rands,
                                                                 n_sets, d_batch_offsets, sets_per_batch, n_batches, d_results, d_status, d_set_results, d_set_status,
                                                                 stream))


def verify_multiple_batches_locate_indexed_device(table, d_sigs, d_key_idx, d_msgs, d_rands, n_sets, n_batches, d_results, d_set_results, d_status=None,
                                                  d_set_status=None, k=0, d_offsets=None, msg_len=32, d_msg_offsets=None, d_batch_offsets=None, sets_per_batch=0,
                                                  stream=None, ctx=None):
    """The same over sets named by indices into a resident KeyTable. Enqueues only."""
    ctx = ctx or table.ctx
    ctx.check(N.lib().mbls_verify_multiple_batches_locate_indexed_device(ctx.handle, table.handle, d_sigs, d_key_idx, d_offsets, k, d_msgs, msg_len, d_msg_offsets,
                                                                         d_rands, n_sets, d_batch_offsets, sets_per_batch, n_batches, d_results, d_status,
                                                                         d_set_results, d_set_status, stream))


# ---- verify_multiple over a shared message list: one Miller loop per message (include/mbls.h, mbls_verify_multiple*_shared_msgs)
def set_vm_grouping(mode, ctx=None):
    """routing of the entries below: 0 auto (grouped when 2 n_msgs <= n), 1 always one Miller loop per message, 2 never (every set gathers its message's point)"""
    ctx = ctx or _c()
    ctx.check(N.lib().mbls_ctx_set_vm_grouping(ctx.handle, mode))


plan_verify_multiple_shared_msgs = N.plan_verify_multiple_shared_msgs


def verify_multiple_shared_msgs(sigs, apks, msgs, n_msgs, msg_idx, rands, n, msg_len=32, msg_offsets=None, ctx=None):
    """verify_multiple_aggregate_signatures (reference src/aggregates.rs:261-316) over n sets whose messages are named by index in a LIST of n_msgs messages
    (msg_len bytes each, or msg_offsets of n_msgs + 1 entries); host buffers (signatures 96 B, decoded aggregate keys 96 B, one nonzero 64-bit scalar per set).
    Returns (bool, status word): what verify_multiple returns with set i's message spelled out."""
    ctx = ctx or _c()
    res = N.outbuf(1)
    st = C.c_uint32(0)
    r = None if rands is None else (C.c_uint64 * max(1, n))(*rands)
    ctx.check(N.lib().mbls_verify_multiple_shared_msgs(ctx.handle, N.cbuf(sigs), N.cbuf(apks), N.cbuf(msgs), msg_len, _moff(msg_offsets), n_msgs, _midx(msg_idx, n), r, n,
                                                       res, C.byref(st)))
    return bool(bytes(res)[0]), st.value


def verify_multiple_shared_msgs_rng(sigs, apks, msgs, n_msgs, msg_idx, n, draw, msg_len=32, msg_offsets=None, ctx=None):
    """The same with the reference's draw order (mbls_verify_multiple_shared_msgs_rng): draw(count) -> `count` nonzero scalars, called at most once, for the sets
    in front of the first signature outside G2. Returns the bool."""
    ctx = ctx or _c()
    res = N.outbuf(1)

    def source(_user, out, count):
        for i, v in enumerate(draw(int(count))):
            out[i] = v
    cb = N.SCALAR_SOURCE(source)
    ctx.check(N.lib().mbls_verify_multiple_shared_msgs_rng(ctx.handle, N.cbuf(sigs), N.cbuf(apks), N.cbuf(msgs), msg_len, _moff(msg_offsets), n_msgs, _midx(msg_idx, n), n,
                                                           res, cb, None))
    return bool(bytes(res)[0])


def verify_multiple_shared_msgs_device(d_sigs, d_apks, d_msgs, n_msgs, d_msg_idx, d_rands, n, d_result, d_status=None, msg_len=32, d_msg_offsets=None, stream=None, ctx=None):
    """The same over device buffers (raw device pointers / ints). Enqueues only: the bool at the device byte d_result, the status word at d_status (optional)."""
    ctx = ctx or _c()
    ctx.check(N.lib().mbls_verify_multiple_shared_msgs_device(ctx.handle, d_sigs, d_apks, d_msgs, msg_len, d_msg_offsets, n_msgs, d_msg_idx, d_rands, n, d_result, d_status,
                                                              stream))


def verify_multiple_sets_indexed_shared_msgs_device(table, d_sigs, d_key_idx, d_msgs, n_msgs, d_msg_idx, d_rands, n, d_result, d_status=None, k=0, d_offsets=None, msg_len=32,
                                                    d_msg_offsets=None, stream=None, ctx=None):
    """The same over sets named by indices into a resident KeyTable (the deployment's form). Enqueues only."""
    ctx = ctx or table.ctx
    ctx.check(N.lib().mbls_verify_multiple_sets_indexed_shared_msgs_device(ctx.handle, table.handle, d_sigs, d_key_idx, d_offsets, k, d_msgs, msg_len, d_msg_offsets, n_msgs,
                                                                           d_msg_idx, d_rands, n, d_result, d_status, stream))


# ---- which sets of a rejected call over a shared message list (include/mbls.h, mbls_verify_multiple*_shared_msgs_locate*)
plan_verify_multiple_shared_msgs_locate_workspace_items = N.plan_verify_multiple_shared_msgs_locate_workspace_items


def verify_multiple_shared_msgs_locate(sigs, apks, msgs, n_msgs, msg_idx, rands, n, msg_len=32, msg_offsets=None, ctx=None):
    """verify_multiple_shared_msgs, and in the same call one answer per SET (mbls_verify_multiple_shared_msgs_locate): every set of an accepted call reads True (a
    passing batch is not examined), every set of a rejected call reads what the one-set call with its scalar and its message spelled out returns. Returns
    (bool, status word, set_results, set_status)."""
    ctx = ctx or _c()
    res = N.outbuf(1)
    st = C.c_uint32(0)
    sres = N.outbuf(max(1, n))
    sst = (C.c_uint32 * max(1, n))()
    r = None if rands is None else (C.c_uint64 * max(1, n))(*rands)
    ctx.check(N.lib().mbls_verify_multiple_shared_msgs_locate(ctx.handle, N.cbuf(sigs), N.cbuf(apks), N.cbuf(msgs), msg_len, _moff(msg_offsets), n_msgs, _midx(msg_idx, n),
                                                              r, n, res, C.byref(st), sres, sst))
    return bool(bytes(res)[0]), st.value, [bool(x) for x in bytes(sres)[:n]], list(sst)[:n]


def verify_multiple_shared_msgs_locate_rng(sigs, apks, msgs, n_msgs, msg_idx, n, draw, msg_len=32, msg_offsets=None, ctx=None):
    """The same with the reference's draw order (mbls_verify_multiple_shared_msgs_locate_rng; draw as verify_multiple_shared_msgs_rng takes it). A set at or behind
    the first signature outside G2 has no scalar and reads False. Returns (bool, set_results, set_status)."""
    ctx = ctx or _c()
    res = N.outbuf(1)
    sres = N.outbuf(max(1, n))
    sst = (C.c_uint32 * max(1, n))()

    def source(_user, out, count):
        for i, v in enumerate(draw(int(count))):
            out[i] = v
    cb = N.SCALAR_SOURCE(source)
    ctx.check(N.lib().mbls_verify_multiple_shared_msgs_locate_rng(ctx.handle, N.cbuf(sigs), N.cbuf(apks), N.cbuf(msgs), msg_len, _moff(msg_offsets), n_msgs,
                                                                  _midx(msg_idx, n), n, res, sres, sst, cb, None))
    return bool(bytes(res)[0]), [bool(x) for x in bytes(sres)[:n]], list(sst)[:n]


def verify_multiple_shared_msgs_locate_device(d_sigs, d_apks, d_msgs, n_msgs, d_msg_idx, d_rands, n, d_result, d_set_results, d_status=None, d_set_status=None, msg_len=32,
                                              d_msg_offsets=None, stream=None, ctx=None):
    """The same over device buffers, as verify_multiple_shared_msgs_device: n result bytes at d_set_results (required), n status words at d_set_status (optional).
    Enqueues only."""
    ctx = ctx or _c()
    ctx.check(N.lib().mbls_verify_multiple_shared_msgs_locate_device(ctx.handle, d_sigs, d_apks, d_msgs, msg_len, d_msg_offsets, n_msgs, d_msg_idx, d_rands, n, d_result,
                                                                     d_status, d_set_results, d_set_status, stream))


def verify_multiple_sets_indexed_shared_msgs_locate_device(table, d_sigs, d_key_idx, d_msgs, n_msgs, d_msg_idx, d_rands, n, d_result, d_set_results, d_status=None,
                                                           d_set_status=None, k=0, d_offsets=None, msg_len=32, d_msg_offsets=None, stream=None, ctx=None):
    """The same over sets named by indices into a resident KeyTable. Enqueues only."""
    ctx = ctx or table.ctx
    ctx.check(N.lib().mbls_verify_multiple_sets_indexed_shared_msgs_locate_device(ctx.handle, table.handle, d_sigs, d_key_idx, d_offsets, k, d_msgs, msg_len, d_msg_offsets,
                                                                                  n_msgs, d_msg_idx, d_rands, n, d_result, d_status, d_set_results, d_set_status, stream))


# ---- verify_multiple over the resident message table, located per set (include/mbls.h, mbls_verify_multiple*_msgtable*): the sets' messages are entries of an
# N.MsgTable, named by table index; nothing is hashed. The stream, the multi-device handle, the shard form and wire-key sets take per-set messages only.
plan_verify_multiple_msgtable = N.plan_verify_multiple_msgtable
plan_verify_multiple_msgtable_workspace_items = N.plan_verify_multiple_msgtable_workspace_items
plan_verify_multiple_msgtable_locate_workspace_items = N.plan_verify_multiple_msgtable_locate_workspace_items


def _scalar_source(draw):
    """draw(count) -> `count` nonzero scalars, as the C callback the _rng entries take"""
    def source(_user, out, count):
        for i, v in enumerate(draw(int(count))):
            out[i] = v
    return N.SCALAR_SOURCE(source)


def verify_multiple_msgtable_device(msg_table, d_sigs, d_apks, d_msg_idx, d_rands, n, d_result, d_status=None, stream=None, ctx=None):
    """verify_multiple over device buffers with set i's message the entry d_msg_idx[i] of the resident table. Enqueues only: the bool at the device byte
    d_result, the status word at d_status (optional). An index at or above the table's size rejects its set (MBLS_ST_BAD_MSG_RANGE)."""
    ctx = ctx or msg_table.ctx
    ctx.check(N.lib().mbls_verify_multiple_msgtable_device(ctx.handle, d_sigs, d_apks, msg_table.handle, d_msg_idx, d_rands, n, d_result, d_status, stream))


def verify_multiple_sets_indexed_msgtable_device(table, msg_table, d_sigs, d_key_idx, d_msg_idx, d_rands, n, d_result, d_status=None, k=0, d_offsets=None, stream=None,
                                                 ctx=None):
    """The same over sets named by indices into a resident KeyTable: keys by key-table index, messages by message-table index. Enqueues only."""
    ctx = ctx or table.ctx
    ctx.check(N.lib().mbls_verify_multiple_sets_indexed_msgtable_device(ctx.handle, table.handle, d_sigs, d_key_idx, d_offsets, k, msg_table.handle, d_msg_idx, d_rands, n,
                                                                        d_result, d_status, stream))


def verify_multiple_msgtable_rng(msg_table, sigs, apks, msg_idx, n, draw, ctx=None):
    """Host buffers and the reference's draw order (mbls_verify_multiple_msgtable_rng; draw as verify_multiple_shared_msgs_rng takes it). An index that names no
    entry raises (MBLS_ERR_ARGUMENT). Returns the bool."""
    ctx = ctx or msg_table.ctx
    res = N.outbuf(1)
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_msgtable_rng(ctx.handle, N.cbuf(sigs), N.cbuf(apks), msg_table.handle, _midx(msg_idx, n), n, res, cb, None))
    return bool(bytes(res)[0])


def verify_multiple_msgtable_locate_device(msg_table, d_sigs, d_apks, d_msg_idx, d_rands, n, d_result, d_set_results, d_status=None, d_set_status=None, stream=None,
                                           ctx=None):
    """verify_multiple_msgtable_device, and in the same call one answer per SET: n result bytes at d_set_results (required), n status words at d_set_status
    (optional), with the semantics of verify_multiple_shared_msgs_locate_device. Enqueues only."""
    ctx = ctx or msg_table.ctx
    ctx.check(N.lib().mbls_verify_multiple_msgtable_locate_device(ctx.handle, d_sigs, d_apks, msg_table.handle, d_msg_idx, d_rands, n, d_result, d_status, d_set_results,
                                                                  d_set_status, stream))


def verify_multiple_sets_indexed_msgtable_locate_device(table, msg_table, d_sigs, d_key_idx, d_msg_idx, d_rands, n, d_result, d_set_results, d_status=None,
                                                        d_set_status=None, k=0, d_offsets=None, stream=None, ctx=None):
    """The same over sets named by indices into a resident KeyTable. Enqueues only."""
    ctx = ctx or table.ctx
    ctx.check(N.lib().mbls_verify_multiple_sets_indexed_msgtable_locate_device(ctx.handle, table.handle, d_sigs, d_key_idx, d_offsets, k, msg_table.handle, d_msg_idx,
                                                                               d_rands, n, d_result, d_status, d_set_results, d_set_status, stream))


def verify_multiple_msgtable_locate_rng(msg_table, sigs, apks, msg_idx, n, draw, ctx=None):
    """verify_multiple_msgtable_rng with one answer per set. A set at or behind the first signature outside G2 has no scalar and reads False. Returns
    (bool, set_results, set_status)."""
    ctx = ctx or msg_table.ctx
    res = N.outbuf(1)
    sres = N.outbuf(max(1, n))
    sst = (C.c_uint32 * max(1, n))()
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_msgtable_locate_rng(ctx.handle, N.cbuf(sigs), N.cbuf(apks), msg_table.handle, _midx(msg_idx, n), n, res, sres, sst, cb, None))
    return bool(bytes(res)[0]), [bool(x) for x in bytes(sres)[:n]], list(sst)[:n]


# ---- verify_multiple over committee bitfields and the resident message table (include/mbls.h, mbls_verify_multiple_committee_msgtable*): set i is the word
# cmt_idx[i] -- a committee id, or VM_SET_SINGLE_KEY | key-table index -- and bits_stride bytes of bitfield (not read for a single-key set). Routing and workspace
# are plan_verify_multiple_msgtable*, unchanged.
VM_SET_SINGLE_KEY = N.VM_SET_SINGLE_KEY


def verify_multiple_committee_msgtable_device(committees, msg_table, d_sigs, d_cmt_idx, d_bits, bits_stride, d_msg_idx, d_rands, n, d_result, d_status=None, stream=None,
                                              ctx=None):
    """verify_multiple_sets_indexed_msgtable_device with every set's signers named by committee and bitfield (or by one key index) over an N.CommitteeTable.
    Enqueues only: the bool at the device byte d_result, the status word at d_status (optional)."""
    ctx = ctx or committees.ctx
    ctx.check(N.lib().mbls_verify_multiple_committee_msgtable_device(ctx.handle, committees.handle, d_sigs, d_cmt_idx, d_bits, bits_stride, msg_table.handle, d_msg_idx,
                                                                     d_rands, n, d_result, d_status, stream))


def verify_multiple_committee_msgtable_locate_device(committees, msg_table, d_sigs, d_cmt_idx, d_bits, bits_stride, d_msg_idx, d_rands, n, d_result, d_set_results,
                                                     d_status=None, d_set_status=None, stream=None, ctx=None):
    """The same, and in the same call one answer per SET: n result bytes at d_set_results (required), n status words at d_set_status (optional). Enqueues only."""
    ctx = ctx or committees.ctx
    ctx.check(N.lib().mbls_verify_multiple_committee_msgtable_locate_device(ctx.handle, committees.handle, d_sigs, d_cmt_idx, d_bits, bits_stride, msg_table.handle,
                                                                            d_msg_idx, d_rands, n, d_result, d_status, d_set_results, d_set_status, stream))


def verify_multiple_committee_msgtable_rng(committees, msg_table, sigs, cmt_idx, bits, bits_stride, msg_idx, n, draw, ctx=None):
    """Host buffers and the reference's draw order (mbls_verify_multiple_committee_msgtable_rng; draw as verify_multiple_msgtable_rng takes it). A word or a message
    index that names nothing raises (MBLS_ERR_ARGUMENT). Returns the bool."""
    ctx = ctx or committees.ctx
    res = N.outbuf(1)
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_committee_msgtable_rng(ctx.handle, committees.handle, N.cbuf(sigs), _midx(cmt_idx, n), _bits(bits, bits_stride, n), bits_stride,
                                                                  msg_table.handle, _midx(msg_idx, n), n, res, cb, None))
    return bool(bytes(res)[0])


def verify_multiple_committee_msgtable_locate_rng(committees, msg_table, sigs, cmt_idx, bits, bits_stride, msg_idx, n, draw, ctx=None):
    """verify_multiple_committee_msgtable_rng with one answer per set. Returns (bool, set_results, set_status)."""
    ctx = ctx or committees.ctx
    res = N.outbuf(1)
    sres = N.outbuf(max(1, n))
    sst = (C.c_uint32 * max(1, n))()
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_committee_msgtable_locate_rng(ctx.handle, committees.handle, N.cbuf(sigs), _midx(cmt_idx, n), _bits(bits, bits_stride, n),
                                                                         bits_stride, msg_table.handle, _midx(msg_idx, n), n, res, sres, sst, cb, None))
    return bool(bytes(res)[0]), [bool(x) for x in bytes(sres)[:n]], list(sst)[:n]


# ---- many verify_multiple batches per call over committee bitfields and the resident message table (include/mbls.h,
# mbls_verify_multiple_batches_committee_msgtable*): the sets of the entries above, the batches of verify_multiple_batches*; one bool and one status word per batch,
# for _locate per set as well. Grouped route: one Miller loop per distinct (batch, table entry) pair.
plan_verify_multiple_batches_committee = N.plan_verify_multiple_batches_committee
VBG_MAX_SETS = N.VBG_MAX_SETS


def verify_multiple_batches_committee_msgtable_device(committees, msg_table, d_sigs, d_cmt_idx, d_bits, bits_stride, d_msg_idx, d_rands, n_sets, n_batches, d_results,
                                                      d_status=None, d_batch_offsets=None, sets_per_batch=0, max_groups=0, stream=None, ctx=None):
    """verify_multiple_batches_indexed_device with every set's signers named by committee and bitfield (or by one key index) and its message by an index into the
    resident table. max_groups: the caller's bound on the distinct (batch, entry) pairs of the call (0: none). Enqueues only: n_batches result bytes at d_results,
    n_batches status words at d_status (optional)."""
    ctx = ctx or committees.ctx
    ctx.check(N.lib().mbls_verify_multiple_batches_committee_msgtable_device(ctx.handle, committees.handle, d_sigs, d_cmt_idx, d_bits, bits_stride, msg_table.handle,
                                                                             d_msg_idx, d_rands, n_sets, d_batch_offsets, sets_per_batch, n_batches, max_groups,
                                                                             d_results, d_status, stream))


def verify_multiple_batches_committee_msgtable_locate_device(committees, msg_table, d_sigs, d_cmt_idx, d_bits, bits_stride, d_msg_idx, d_rands, n_sets, n_batches,
                                                             d_results, d_set_results, d_status=None, d_set_status=None, d_batch_offsets=None, sets_per_batch=0,
                                                             max_groups=0, stream=None, ctx=None):
    """The same, and in the same call one answer per SET, as verify_multiple_batches_locate_indexed_device gives it: n_sets result bytes at d_set_results
    (required), n_sets status words at d_set_status (optional). Enqueues only."""
    ctx = ctx or committees.ctx
    ctx.check(N.lib().mbls_verify_multiple_batches_committee_msgtable_locate_device(ctx.handle, committees.handle, d_sigs, d_cmt_idx, d_bits, bits_stride,
                                                                                    msg_table.handle, d_msg_idx, d_rands, n_sets, d_batch_offsets, sets_per_batch,
                                                                                    n_batches, max_groups, d_results, d_status, d_set_results, d_set_status, stream))


def verify_multiple_batches_committee_msgtable_rng(committees, msg_table, sigs, cmt_idx, bits, bits_stride, msg_idx, n_sets, n_batches, draw, batch_offsets=None,
                                                   sets_per_batch=0, ctx=None):
    """Host buffers and the draw order of verify_multiple_batches_rng (draw as verify_multiple_msgtable_rng takes it). A word or a message index that names
    nothing, or a batch table that is not sound, raises (MBLS_ERR_ARGUMENT). Returns list[bool], one per batch."""
    ctx = ctx or committees.ctx
    res = N.outbuf(max(1, n_batches))
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_batches_committee_msgtable_rng(ctx.handle, committees.handle, N.cbuf(sigs), _midx(cmt_idx, n_sets),
                                                                          _bits(bits, bits_stride, n_sets), bits_stride, msg_table.handle, _midx(msg_idx, n_sets), n_sets,
                                                                          _boff(batch_offsets), sets_per_batch, n_batches, res, cb, None))
    return [bool(x) for x in bytes(res)[:n_batches]]


def verify_multiple_batches_committee_msgtable_locate_rng(committees, msg_table, sigs, cmt_idx, bits, bits_stride, msg_idx, n_sets, n_batches, draw, batch_offsets=None,
                                                          sets_per_batch=0, ctx=None):
    """verify_multiple_batches_committee_msgtable_rng with one answer per set. Returns (results, set_results, set_status)."""
    ctx = ctx or committees.ctx
    res = N.outbuf(max(1, n_batches))
    sres = N.outbuf(max(1, n_sets))
    sst = (C.c_uint32 * max(1, n_sets))()
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_batches_committee_msgtable_locate_rng(ctx.handle, committees.handle, N.cbuf(sigs), _midx(cmt_idx, n_sets),
                                                                                 _bits(bits, bits_stride, n_sets), bits_stride, msg_table.handle,
                                                                                 _midx(msg_idx, n_sets), n_sets, _boff(batch_offsets), sets_per_batch, n_batches, res, sres,
                                                                                 sst, cb, None))
    return [bool(x) for x in bytes(res)[:n_batches]], [bool(x) for x in bytes(sres)[:n_sets]], list(sst)[:n_sets]


def vbg_group_probe(msg_idx, table_size, n_batches, batch_offsets=None, sets_per_batch=0, ctx=None):
    """test probe (mbls_vbg_group_probe): the grouping of the grouped route alone, on ANY batch table -> dict of lists: pos, status, pos_lo, pos_hi, head, entry
    (one word per set), count (per batch), off (n_batches + 1)"""
    ctx = ctx or _c()
    n = len(msg_idx)
    outs = [(C.c_uint32 * max(1, n))() for _ in range(6)]
    cnt, off = (C.c_uint32 * max(1, n_batches))(), (C.c_uint32 * (n_batches + 1))()
    ctx.check(N.lib().mbls_vbg_group_probe(ctx.handle, (C.c_uint32 * max(1, n))(*msg_idx), n, table_size, _boff(batch_offsets), sets_per_batch, n_batches, outs[0],
                                           outs[1], outs[2], outs[3], outs[4], outs[5], cnt, off))
    names = ("pos", "status", "pos_lo", "pos_hi", "head", "entry")
    d = {k: list(o)[:n] for k, o in zip(names, outs)}
    d["count"], d["off"] = list(cnt)[:n_batches], list(off)
    return d


# ---- verify_multiple over committee spans and the resident message table (include/mbls.h, mbls_verify_multiple_committee_span_msgtable*): set i names the ids
# cmt_ids[cmt_off[i] .. cmt_off[i + 1]) and one field over their concatenated members -- or is the one id VM_SET_SINGLE_KEY | key-table index, whose field is not read.
plan_verify_multiple_committee_span = N.plan_verify_multiple_committee_span


def set_vm_span_split(mode, ctx=None):
    """the key phase of the entries below: 0 auto (csrc/mbls_vcs.h vcs_split), else the lanes each of a set's two key lists is cut over: 1, 2, 4, 8 or 16"""
    ctx = ctx or _c()
    ctx.check(N.lib().mbls_ctx_set_vm_span_split(ctx.handle, mode))


def verify_multiple_committee_span_msgtable_device(committees, msg_table, d_sigs, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride, d_msg_idx, d_rands, n, d_result,
                                                   d_status=None, stream=None, ctx=None):
    """verify_multiple_sets_indexed_msgtable_device with every set's signers named by a span of committees and one field (or by one key index) over an
    N.CommitteeTable. Enqueues only: the bool at the device byte d_result, the status word at d_status (optional)."""
    ctx = ctx or committees.ctx
    ctx.check(N.lib().mbls_verify_multiple_committee_span_msgtable_device(ctx.handle, committees.handle, d_sigs, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride,
                                                                          msg_table.handle, d_msg_idx, d_rands, n, d_result, d_status, stream))


def verify_multiple_committee_span_msgtable_locate_device(committees, msg_table, d_sigs, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride, d_msg_idx, d_rands, n,
                                                          d_result, d_set_results, d_status=None, d_set_status=None, stream=None, ctx=None):
    """The same, and in the same call one answer per SET: n result bytes at d_set_results (required), n status words at d_set_status (optional). Enqueues only."""
    ctx = ctx or committees.ctx
    ctx.check(N.lib().mbls_verify_multiple_committee_span_msgtable_locate_device(ctx.handle, committees.handle, d_sigs, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits,
                                                                                 bits_stride, msg_table.handle, d_msg_idx, d_rands, n, d_result, d_status, d_set_results,
                                                                                 d_set_status, stream))


def verify_multiple_committee_span_msgtable_rng(committees, msg_table, sigs, cmt_id_lists, fields, bits_stride, msg_idx, draw, ctx=None):
    """Host buffers and the reference's draw order (mbls_verify_multiple_committee_span_msgtable_rng; draw as verify_multiple_msgtable_rng takes it): set i names the
    ids cmt_id_lists[i] with the field fields[i] (as fast_aggregate_verify_batch_committee_span takes them), or is [VM_SET_SINGLE_KEY | key index] with any field. A
    malformed set, a key index or a message index that names nothing raises (MBLS_ERR_ARGUMENT). Returns the bool."""
    ctx = ctx or committees.ctx
    n = len(cmt_id_lists)
    ids, n_ids, off, bits = _span(cmt_id_lists, fields, bits_stride)
    res = N.outbuf(1)
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_committee_span_msgtable_rng(ctx.handle, committees.handle, N.cbuf(sigs), ids, n_ids, off, bits, bits_stride, msg_table.handle,
                                                                       _midx(msg_idx, n), n, res, cb, None))
    return bool(bytes(res)[0])


def verify_multiple_committee_span_msgtable_locate_rng(committees, msg_table, sigs, cmt_id_lists, fields, bits_stride, msg_idx, draw, ctx=None):
    """verify_multiple_committee_span_msgtable_rng with one answer per set. Returns (bool, set_results, set_status)."""
    ctx = ctx or committees.ctx
    n = len(cmt_id_lists)
    ids, n_ids, off, bits = _span(cmt_id_lists, fields, bits_stride)
    res = N.outbuf(1)
    sres = N.outbuf(max(1, n))
    sst = (C.c_uint32 * max(1, n))()
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_committee_span_msgtable_locate_rng(ctx.handle, committees.handle, N.cbuf(sigs), ids, n_ids, off, bits, bits_stride,
                                                                              msg_table.handle, _midx(msg_idx, n), n, res, sres, sst, cb, None))
    return bool(bytes(res)[0]), [bool(x) for x in bytes(sres)[:n]], list(sst)[:n]


# ---- many verify_multiple batches per call over committee spans and the resident message table (include/mbls.h,
# mbls_verify_multiple_batches_committee_span_msgtable*): the sets of the span entries above, the batches and outputs of verify_multiple_batches_committee_msgtable*.
plan_verify_multiple_batches_committee_span = N.plan_verify_multiple_batches_committee_span


def verify_multiple_batches_committee_span_msgtable_device(committees, msg_table, d_sigs, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride, d_msg_idx, d_rands, n_sets,
                                                           n_batches, d_results, d_status=None, d_batch_offsets=None, sets_per_batch=0, max_groups=0, stream=None, ctx=None):
    """verify_multiple_batches_committee_msgtable_device with the sets of verify_multiple_committee_span_msgtable_device: one verdict per batch. Enqueues only."""
    ctx = ctx or committees.ctx
    ctx.check(N.lib().mbls_verify_multiple_batches_committee_span_msgtable_device(ctx.handle, committees.handle, d_sigs, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits,
                                                                                  bits_stride, msg_table.handle, d_msg_idx, d_rands, n_sets, d_batch_offsets,
                                                                                  sets_per_batch, n_batches, max_groups, d_results, d_status, stream))


def verify_multiple_batches_committee_span_msgtable_locate_device(committees, msg_table, d_sigs, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits, bits_stride, d_msg_idx, d_rands,
                                                                  n_sets, n_batches, d_results, d_set_results, d_status=None, d_set_status=None, d_batch_offsets=None,
                                                                  sets_per_batch=0, max_groups=0, stream=None, ctx=None):
    """The same, and in the same call one answer per SET: n_sets result bytes at d_set_results (required), n_sets status words at d_set_status (optional)."""
    ctx = ctx or committees.ctx
    ctx.check(N.lib().mbls_verify_multiple_batches_committee_span_msgtable_locate_device(ctx.handle, committees.handle, d_sigs, d_cmt_ids, n_cmt_ids, d_cmt_off, d_bits,
                                                                                         bits_stride, msg_table.handle, d_msg_idx, d_rands, n_sets, d_batch_offsets,
                                                                                         sets_per_batch, n_batches, max_groups, d_results, d_status, d_set_results,
                                                                                         d_set_status, stream))


def verify_multiple_batches_committee_span_msgtable_rng(committees, msg_table, sigs, cmt_id_lists, fields, bits_stride, msg_idx, n_batches, draw, batch_offsets=None,
                                                        sets_per_batch=0, ctx=None):
    """Host buffers and the draw order of verify_multiple_batches_committee_msgtable_rng; the sets as verify_multiple_committee_span_msgtable_rng takes them. A
    malformed set, a key or message index that names nothing, or a batch table that is not sound raises (MBLS_ERR_ARGUMENT). Returns list[bool], one per batch."""
    ctx = ctx or committees.ctx
    n = len(cmt_id_lists)
    ids, n_ids, off, bits = _span(cmt_id_lists, fields, bits_stride)
    res = N.outbuf(max(1, n_batches))
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_batches_committee_span_msgtable_rng(ctx.handle, committees.handle, N.cbuf(sigs), ids, n_ids, off, bits, bits_stride,
                                                                               msg_table.handle, _midx(msg_idx, n), n, _boff(batch_offsets), sets_per_batch, n_batches,
                                                                               res, cb, None))
    return [bool(x) for x in bytes(res)[:n_batches]]


def verify_multiple_batches_committee_span_msgtable_locate_rng(committees, msg_table, sigs, cmt_id_lists, fields, bits_stride, msg_idx, n_batches, draw, batch_offsets=None,
                                                               sets_per_batch=0, ctx=None):
    """verify_multiple_batches_committee_span_msgtable_rng with one answer per set. Returns (results, set_results, set_status)."""
    ctx = ctx or committees.ctx
    n = len(cmt_id_lists)
    ids, n_ids, off, bits = _span(cmt_id_lists, fields, bits_stride)
    res = N.outbuf(max(1, n_batches))
    sres = N.outbuf(max(1, n))
    sst = (C.c_uint32 * max(1, n))()
    cb = _scalar_source(draw)
    ctx.check(N.lib().mbls_verify_multiple_batches_committee_span_msgtable_locate_rng(ctx.handle, committees.handle, N.cbuf(sigs), ids, n_ids, off, bits, bits_stride,
                                                                                      msg_table.handle, _midx(msg_idx, n), n, _boff(batch_offsets), sets_per_batch,
                                                                                      n_batches, res, sres, sst, cb, None))
    return [bool(x) for x in bytes(res)[:n_batches]], [bool(x) for x in bytes(sres)[:n]], list(sst)[:n]
