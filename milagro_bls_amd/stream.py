"""Verification stream (include/mbls.h, "verification stream"): calls of any size are packed into full-round launches of the device entries.

    with VerifyStream(ctx, pk_format=PK_UNCOMPRESSED) as vs:
        t = vs.submit_device(d_sigs, d_msgs, d_pks, n, k, d_results, msg_len=32)       # device tensors or pointers
        h = vs.submit(sigs, msgs, pks, n, k, msg_len=32)                                # host bytes -> HostTicket
        vs.wait(t); results, status = h.result()

Over a resident message table (N.MsgTable) a call names its messages by table index:

    with VerifyStream(ctx, pk_format=PK_UNCOMPRESSED, msg_table=mt) as vs:
        t = vs.submit_device(d_sigs, d_msg_idx, d_pks, n, k, d_results)                 # uint32 indices where the messages were

Over a committee table (N.CommitteeTable) and a message table an item is a signature, a message index, a committee id and its SSZ bitfield:

    with VerifyStream(ctx, committees=ct, msg_table=mt, bits_stride=16) as vs:
        t = vs.submit_committee_device(d_sigs, d_msg_idx, d_cmt_idx, d_bits, bits_len, n, d_results)
        h = vs.submit_committee(sigs, msg_idx, cmt_idx, bits, bits_len, n)               # bits_len: per call, 1 .. bits_stride, any alignment

verify_multiple over the same two tables (vm=True): a call is one batch of sets, never split; a round is one call of
mbls_verify_multiple_batches_committee_msgtable_locate_device over every batch the round holds, answered per batch and per set:

    with VerifyStream(ctx, vm=True, committees=ct, msg_table=mt, bits_stride=16) as vs:
        t = vs.submit_vm_device(d_sigs, d_cmt_idx, d_bits, bits_len, d_msg_idx, d_rands, n_sets, d_result, set_results=d_set_results)
        ok, per_set = vs.submit_vm(sets, rng).result()                                   # the set tuples of verify_multiple_aggregate_signatures_committee
"""
import ctypes as C
from collections import deque

from . import _native as N


def _ptr(x):
    """device pointer of a torch tensor, an int or None"""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


def _host(x, dtype):
    """host input -> (object to keep alive, pointer): numpy arrays are passed in place, anything else is copied"""
    import numpy as np
    if isinstance(x, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(x) if not isinstance(x, bytes) else x, dtype=np.uint8)
    else:
        a = np.ascontiguousarray(np.asarray(x, dtype=dtype))
    return a, (a.ctypes.data if a.size else None)


def _offsets(seq, ctype):
    if seq is None:
        return None
    return (ctype * len(seq))(*[int(v) for v in seq])


class HostTicket:
    """a host submit: result() waits for the call and returns (results bytes, status list)"""

    def __init__(self, vs, ticket, res, st, n):
        self.vs, self.ticket, self._res, self._st, self.n = vs, ticket, res, st, n

    def result(self):
        self.vs.wait(self.ticket)
        return bytes(self._res)[:self.n], list(self._st)[:self.n]


class VmTicket:
    """a host verify_multiple submit: result() waits for the call and returns (bool, list[bool]): the batch, and which sets of a rejected batch are good"""

    def __init__(self, vs, ticket, res, st, sres, sst, n):
        self.vs, self.ticket, self._res, self._st, self._sres, self._sst, self.n = vs, ticket, res, st, sres, sst, n

    def result(self):
        self.vs.wait(self.ticket)
        return bool(bytes(self._res)[0]), [bool(x) for x in bytes(self._sres)[:self.n]]

    def status(self):
        """(the batch's status word, the sets' status words) of the completed call"""
        self.vs.wait(self.ticket)
        return int(self._st[0]), list(self._sst)[:self.n]


def _reference_scalar(rng):
    """one blinding scalar by the reference's rule (src/aggregates.rs:280-287): 8 random bytes, big-endian i64, absolute value, retry on zero"""
    r = 0
    while r == 0:
        r = abs(int.from_bytes(bytes(rng.getrandbits(8) for _ in range(8)), "big", signed=True)) & 0xFFFFFFFFFFFFFFFF
    return r


class VerifyStream:
    """One stream on one context: mode STREAM_FAST_AGGREGATE_VERIFY / STREAM_VERIFY; keys as pk_format bytes, or indices into `table` (a KeyTable); messages as bytes, or --
    msg_table given (a MsgTable) -- as uint32 indices into it: submit / submit_device then take the index array where they took the messages."""

    def __init__(self, ctx=None, mode=N.STREAM_FAST_AGGREGATE_VERIFY, pk_format=N.PK_UNCOMPRESSED, table=None, round_items=0, round_keys=0, round_msg_bytes=0,
                 depth=0, policy=N.STREAM_WORK_CONSERVING, msg_table=None, committees=None, bits_stride=0, vm=False):
        self.ctx = ctx or N.default_context()          # held: the stream is destroyed before its context
        self.table = table
        self.indexed = table is not None
        self._h = N.vp()
        o = N.StreamOpts(round_items, round_keys, round_msg_bytes, depth, policy)
        self.msg_table = msg_table                     # held: the stream is destroyed before its message table
        self.committees = committees                   # held likewise: a committee stream (submit_committee / submit_committee_device only)
        self.bits_stride = bits_stride
        self.vm = bool(vm)                             # a verify_multiple stream over committees= and msg_table= (submit_vm / submit_vm_device only)
        self._live = deque()                           # (ticket, buffers) kept alive until the call completes
        th = table.handle if table is not None else None
        if vm:
            if committees is None or msg_table is None or table is not None or mode != N.STREAM_FAST_AGGREGATE_VERIFY:
                raise ValueError("a verify_multiple stream runs over committees= and msg_table=: no key table of its own, no mode")
            rc = N.lib().mbls_stream_create_vm_committee(self.ctx.handle, committees.handle, msg_table.handle, bits_stride, C.byref(o), C.byref(self._h))
            if rc != N.OK:
                raise N.MblsError(rc, "mbls_stream_create_vm_committee: " + self.ctx.last_error())
            return
        if committees is not None:
            if msg_table is None or table is not None or mode != N.STREAM_FAST_AGGREGATE_VERIFY:
                raise ValueError("a committee stream is fast_aggregate_verify over committees= and msg_table=: no key table of its own, no other mode")
            rc = N.lib().mbls_stream_create_committee(self.ctx.handle, committees.handle, msg_table.handle, bits_stride, C.byref(o), C.byref(self._h))
            if rc != N.OK:
                raise N.MblsError(rc, "mbls_stream_create_committee: " + self.ctx.last_error())
            return
        if msg_table is not None:
            rc = N.lib().mbls_stream_create_msgtable(self.ctx.handle, mode, pk_format, th, msg_table.handle, C.byref(o), C.byref(self._h))
        else:
            rc = N.lib().mbls_stream_create(self.ctx.handle, mode, pk_format, th, C.byref(o), C.byref(self._h))
        if rc != N.OK:
            raise N.MblsError(rc, ("mbls_stream_create_msgtable: " if msg_table is not None else "mbls_stream_create: ") + self.ctx.last_error())
        self._live = deque()                           # (ticket, buffers) kept alive until the call completes

    def close(self):
        if self._h:
            N.lib().mbls_stream_destroy(self._h)
            self._h = N.vp()
            self._live.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def last_error(self):
        return N.lib().mbls_stream_last_error(self._h).decode()

    def check(self, rc):
        if rc != N.OK:
            raise N.MblsError(rc, self.last_error())

    def _keep(self, ticket, bufs):
        while self._live and N.lib().mbls_stream_query(self._h, self._live[0][0]) != N.PENDING:
            self._live.popleft()
        self._live.append((ticket, bufs))

    def submit_device(self, sigs, msgs, keys, n, k, results, msg_len=0, msg_offsets=None, pk_offsets=None, bitmap=None, status=None, stream=None):
        """device buffers (torch tensors or pointers); keys = key bytes, or uint32 table indices for a key-table stream; offsets are host sequences;
        stream: a torch stream or a raw hipStream_t -> ticket"""
        mo, po = _offsets(msg_offsets, C.c_uint64), _offsets(pk_offsets, C.c_uint32)
        hs = getattr(stream, "cuda_stream", stream)
        t = C.c_uint64(0)
        kp = _ptr(keys)
        if self.msg_table is not None:
            if msg_len or msg_offsets is not None:
                raise ValueError("a message-table stream takes uint32 message indices: no msg_len, no msg_offsets")
            self.check(N.lib().mbls_stream_submit_msgidx_device(self._h, _ptr(sigs), _ptr(msgs), None if self.indexed else kp, kp if self.indexed else None, po,
                                                                n, k, _ptr(results), _ptr(bitmap), _ptr(status), hs, C.byref(t)))
            self._keep(t.value, (po, sigs, msgs, keys, results, bitmap, status))
            return t.value
        self.check(N.lib().mbls_stream_submit_device(self._h, _ptr(sigs), _ptr(msgs), msg_len, mo, None if self.indexed else kp, kp if self.indexed else None, po,
                                                     n, k, _ptr(results), _ptr(bitmap), _ptr(status), hs, C.byref(t)))
        self._keep(t.value, (mo, po, sigs, msgs, keys, results, bitmap, status))
        return t.value

    def submit(self, sigs, msgs, keys, n, k, msg_len=0, msg_offsets=None, pk_offsets=None):
        """host bytes or numpy arrays (keys: key bytes, or uint32 table indices for a key-table stream; numpy arrays are read in place, when the
        call's round launches) -> HostTicket"""
        import numpy as np
        (sa, sp), (ma, mp) = _host(sigs, np.uint8), _host(msgs, np.uint32 if self.msg_table is not None else np.uint8)
        ka, kp = _host(keys, np.uint32 if self.indexed else np.uint8)
        mo, po = _offsets(msg_offsets, C.c_uint64), _offsets(pk_offsets, C.c_uint32)
        res, st = N.outbuf(n), (C.c_uint32 * max(1, n))()
        t = C.c_uint64(0)
        if self.msg_table is not None:
            if msg_len or msg_offsets is not None:
                raise ValueError("a message-table stream takes uint32 message indices: no msg_len, no msg_offsets")
            self.check(N.lib().mbls_stream_submit_msgidx(self._h, sp, mp, None if self.indexed else kp, kp if self.indexed else None, po, n, k, res, st, C.byref(t)))
            self._keep(t.value, (sa, ma, ka, po, res, st))
            return HostTicket(self, t.value, res, st, n)
        self.check(N.lib().mbls_stream_submit(self._h, sp, mp, msg_len, mo, None if self.indexed else kp, kp if self.indexed else None, po, n, k, res, st, C.byref(t)))
        self._keep(t.value, (sa, ma, ka, mo, po, res, st))
        return HostTicket(self, t.value, res, st, n)

    def submit_committee_device(self, sigs, msg_idx, cmt_idx, bits, bits_len, n, results, bitmap=None, status=None, stream=None):
        """a committee stream's device call: uint32 message-table indices and committee ids, n fields of bits_len bytes back to back (any address, any
        bits_len in 1 .. bits_stride) -> ticket"""
        hs = getattr(stream, "cuda_stream", stream)
        t = C.c_uint64(0)
        self.check(N.lib().mbls_stream_submit_committee_device(self._h, _ptr(sigs), _ptr(msg_idx), _ptr(cmt_idx), _ptr(bits), bits_len, n, _ptr(results), _ptr(bitmap),
                                                               _ptr(status), hs, C.byref(t)))
        self._keep(t.value, (sigs, msg_idx, cmt_idx, bits, results, bitmap, status))
        return t.value

    def submit_committee(self, sigs, msg_idx, cmt_idx, bits, bits_len, n):
        """the same from host memory (bits: any bytes-like or uint8 array of n * bits_len bytes) -> HostTicket"""
        import numpy as np
        (sa, sp), (ma, mp), (ca, cp), (ba, bp) = _host(sigs, np.uint8), _host(msg_idx, np.uint32), _host(cmt_idx, np.uint32), _host(bits, np.uint8)
        if ba.size != n * bits_len:
            raise ValueError("bits holds %d bytes, the call needs n * bits_len = %d" % (ba.size, n * bits_len))
        res, st = N.outbuf(n), (C.c_uint32 * max(1, n))()
        t = C.c_uint64(0)
        self.check(N.lib().mbls_stream_submit_committee(self._h, sp, mp, cp, bp, bits_len, n, res, st, C.byref(t)))
        self._keep(t.value, (sa, ma, ca, ba, res, st))
        return HostTicket(self, t.value, res, st, n)

    def submit_vm_device(self, sigs, cmt_idx, bits, bits_len, msg_idx, rands, n_sets, result, status=None, set_results=None, set_status=None, stream=None):
        """a verify_multiple stream's device call, one batch: n_sets signatures, set words (a committee id, or VM_SET_SINGLE_KEY | key index), fields of bits_len bytes
        back to back (any address, bits_len in 0 .. bits_stride; bits may be None for bits_len = 0), uint32 message indices and uint64 scalars from the caller;
        result: one byte, status: one word, set_results / set_status: n_sets of each (optional) -> ticket"""
        hs = getattr(stream, "cuda_stream", stream)
        t = C.c_uint64(0)
        self.check(N.lib().mbls_stream_submit_vm_device(self._h, _ptr(sigs), _ptr(cmt_idx), _ptr(bits), bits_len, _ptr(msg_idx), _ptr(rands), n_sets, _ptr(result),
                                                        _ptr(status), _ptr(set_results), _ptr(set_status), hs, C.byref(t)))
        self._keep(t.value, (sigs, cmt_idx, bits, msg_idx, rands, result, status, set_results, set_status))
        return t.value

    def submit_vm_arrays(self, sigs, cmt_idx, bits, bits_len, msg_idx, rands, n_sets):
        """the same from host memory, the scalars the caller's (uint64 array) -> VmTicket"""
        import numpy as np
        (sa, sp), (ca, cp), (ma, mp), (ra, rp) = _host(sigs, np.uint8), _host(cmt_idx, np.uint32), _host(msg_idx, np.uint32), _host(rands, np.uint64)
        ba, bp = (None, None) if bits is None else _host(bits, np.uint8)
        if (ba.size if ba is not None else 0) != n_sets * bits_len:
            raise ValueError("bits holds %d bytes, the call needs n_sets * bits_len = %d" % (ba.size if ba is not None else 0, n_sets * bits_len))
        res, st, sres, sst = N.outbuf(1), (C.c_uint32 * 1)(), N.outbuf(n_sets), (C.c_uint32 * max(1, n_sets))()
        t = C.c_uint64(0)
        self.check(N.lib().mbls_stream_submit_vm(self._h, sp, cp, bp, bits_len, mp, rp, n_sets, res, st, sres, sst, C.byref(t)))
        self._keep(t.value, (sa, ca, ba, ma, ra, res, st, sres, sst))
        return VmTicket(self, t.value, res, st, sres, sst, n_sets)

    def submit_vm(self, sets, rng):
        """one batch as AggregateSignature.verify_multiple_aggregate_signatures_committee takes it: sets (signature, committee_id, bits_bytes, message_index) or
        (signature, SingleKey(index), None, message_index) -> VmTicket, whose result() is (bool, list[bool]). One scalar per set is drawn from `rng` HERE, at
        submit, in set order, by the reference's rule (8 bytes, big-endian i64, absolute value, retry on zero). The one difference from the `_rng` entries:
        nothing is read back before the draw, so a batch with a signature outside G2 still consumes a scalar for every set (the `_rng` entries stop drawing at
        the first such signature, as the reference does). A field longer than bits_stride must be zero beyond it."""
        from .api import SingleKey
        import numpy as np
        sets = list(sets)
        if not sets:
            raise ValueError("a call holds at least one set")
        words, fields = [], []
        for s in sets:
            if isinstance(s[1], SingleKey):
                words.append(N.VM_SET_SINGLE_KEY | s[1].index); fields.append(b"")
            else:
                cid, field = int(s[1]), bytes(s[2])
                if not 0 <= cid < N.VM_SET_SINGLE_KEY:
                    raise ValueError("committee id out of range")
                if any(field[self.bits_stride:]):
                    raise ValueError("a bitfield names members beyond the stream's bits_stride")
                words.append(cid); fields.append(field[:self.bits_stride])
        bits_len = max(len(f) for f in fields)
        bits = b"".join(f.ljust(bits_len, b"\0") for f in fields)
        rands = np.array([_reference_scalar(rng) for _ in sets], dtype=np.uint64)
        return self.submit_vm_arrays(b"".join(s[0].point for s in sets), np.array(words, dtype=np.uint32), bits if bits_len else None, bits_len,
                                     np.array([int(s[3]) for s in sets], dtype=np.uint32), rands, len(sets))

    def flush(self):
        self.check(N.lib().mbls_stream_flush(self._h))

    def wait(self, ticket):
        self.check(N.lib().mbls_stream_wait(self._h, ticket))
        while self._live and self._live[0][0] <= ticket:
            self._live.popleft()

    def query(self, ticket):
        """OK / PENDING (or the call's error code)"""
        return N.lib().mbls_stream_query(self._h, ticket)

    def stats(self):
        s = N.StreamStats()
        self.check(N.lib().mbls_stream_get_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in N.StreamStats._fields_}
