"""Inputs for the shared-message-list tests (include/mbls.h, mbls_*_shared_msgs): items that really share messages -- one list, one index per item, signatures made
by the oracle over the message each item names -- with the rejection kinds of helpers.make_batch mixed in, the same items with their messages spelled out (what the
per-item entries take), and the oracle's verdicts. Messages may differ in length (the oracle's batch entries take one length per call: items are grouped by it)."""
import random

import helpers

ORDER = ["flip_msg", "wrong_key", "sig_not_in_g2", "sig_infinity", "apk_infinity", "bad_sig_bytes", "bad_pk_bytes"]
FLAG = {"sig_not_in_g2": 0x02, "apk_infinity": 0x08, "bad_sig_bytes": 0x01, "bad_pk_bytes": 0x04, "flip_msg": 0x40, "wrong_key": 0x40, "wrong_index": 0x40}
ST_BAD_MSG_RANGE = 0x100
ST_PAIRING_FAILED = 0x40


class Case:
    pass


def _by_length(msgs):
    groups = {}
    for i, m in enumerate(msgs):
        groups.setdefault(len(m), []).append(i)
    return groups


def _sign(sks, msgs, nthreads):
    """one signature per (secret key, message), messages of any length"""
    import orc
    out = [None] * len(msgs)
    for L, items in _by_length(msgs).items():
        s = orc.batch_sign(b"".join(sks[i].to_bytes(32, "big") for i in items), b"".join(msgs[i] for i in items), len(items), msg_len=L, nthreads=nthreads)
        for j, i in enumerate(items):
            out[i] = s[96 * j:96 * j + 96]
    return out


def build(n, k, msgs, idx, seed, fmt=1, signed_as=None, negatives=True, pool_n=32):
    """n items of k keys (fmt 0: 48-byte, 1: 96-byte) over the message list `msgs`; item i names message idx[i]. signed_as = {i: j}: item i's signature is over message j
    although its index names another (kind "wrong_index": the pairing check must fail). Negative kinds cycle over the other items with i % 4 == 3."""
    import orc
    nt = helpers.oracle_threads()
    rnd = random.Random(seed)
    signed_as = signed_as or {}
    pool = [rnd.randrange(1, helpers.R) for _ in range(pool_n)]
    sz = 48 if fmt == 0 else 96
    pkb = orc.batch_sk_to_pk(b"".join(s.to_bytes(32, "big") for s in pool), pool_n, fmt, nthreads=nt)
    pk = [pkb[sz * j:sz * j + sz] for j in range(pool_n)]
    idxs = [rnd.sample(range(pool_n), k) for _ in range(n)]
    aggs = [sum(pool[j] for j in ix) % helpers.R for ix in idxs]
    keys = [[pk[j] for j in ix] for ix in idxs]
    spelled = [msgs[j] for j in idx]                       # what item i's index names
    to_sign = list(spelled)                                # what item i's signature is over
    kinds = ["valid"] * n
    for i, j in signed_as.items():
        assert msgs[j] != msgs[idx[i]]
        to_sign[i] = msgs[j]; kinds[i] = "wrong_index"
    c = 0
    if negatives:
        for i in range(n):
            if i % 4 != 3 or i in signed_as:
                continue
            kind = ORDER[c % len(ORDER)]; c += 1
            if kind == "apk_infinity" and k < 2:
                kind = "flip_msg"
            kinds[i] = kind
            if kind == "flip_msg":                         # the signer saw another message than the one the list holds
                to_sign[i] = bytes([to_sign[i][0] ^ 1]) + to_sign[i][1:] if to_sign[i] else b"\x01"
    sigs = _sign(aggs, to_sign, nt)
    c = 0
    for i in range(n):
        kind = kinds[i]
        if kind in ("valid", "wrong_index", "flip_msg"):
            continue
        if kind == "wrong_key":
            keys[i][0] = pk[[j for j in range(pool_n) if j not in idxs[i]][0]]
        elif kind == "sig_not_in_g2":
            c += 1; sigs[i] = bytes.fromhex(helpers.load_vectors()["model"]["g2_subgroup_probes"][c % 3]["compressed"])
        elif kind == "sig_infinity":
            sigs[i] = helpers.G2_INF
        elif kind == "apk_infinity":
            e, partial = orc.aggregate_pks([orc.sk_to_pk(pool[j]) for j in idxs[i][:-1]])
            neg = orc.g1_mul(partial, helpers.R - 1)
            keys[i][-1] = orc.g1_compress(neg) if fmt == 0 else neg
        elif kind == "bad_sig_bytes":
            sigs[i] = bytes([sigs[i][0] & 0x7F]) + sigs[i][1:]
        elif kind == "bad_pk_bytes":
            keys[i][0] = bytes([0x80 if fmt == 0 else 0x00]) + b"\xff" * (sz - 1)
    cs = Case()
    cs.n, cs.k, cs.fmt, cs.n_msgs = n, k, fmt, len(msgs)
    cs.msgs, cs.idx, cs.spelled, cs.kinds = list(msgs), list(idx), spelled, kinds
    cs.sigs = b"".join(sigs); cs.pks = b"".join(b"".join(ks) for ks in keys)
    cs.expect = [kd == "valid" for kd in kinds]
    cs.uniform = len({len(m) for m in msgs}) <= 1
    cs.msg_len = len(msgs[0]) if msgs and cs.uniform else 0
    cs.list_bytes = b"".join(msgs)
    cs.list_offsets = [sum(len(m) for m in msgs[:j]) for j in range(len(msgs) + 1)]
    cs.spelled_bytes = b"".join(spelled)
    cs.spelled_offsets = [sum(len(m) for m in spelled[:i]) for i in range(n + 1)]
    return cs


def oracle(cs, verify=False):
    """the oracle's verdict per item on the spelled-out messages (fast_aggregate_verify, or Signature::verify for k = 1 with verify=True)"""
    import orc
    nt = helpers.oracle_threads()
    sz = 48 if cs.fmt == 0 else 96
    want = [None] * cs.n
    for L, items in _by_length(cs.spelled).items():
        s = b"".join(cs.sigs[96 * i:96 * i + 96] for i in items)
        m = b"".join(cs.spelled[i] for i in items)
        p = b"".join(cs.pks[sz * cs.k * i:sz * cs.k * (i + 1)] for i in items)
        if verify:
            assert cs.fmt == 0 and cs.k == 1
            w = orc.batch_verify(s, m, p, len(items), msg_len=L, nthreads=nt)
        else:
            w = orc.batch_fast_aggregate_verify(s, m, p, len(items), cs.k, cs.fmt, msg_len=L, nthreads=nt)
        for j, i in enumerate(items):
            want[i] = w[j]
    return want
