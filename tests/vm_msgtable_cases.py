"""Shared by tests/test_gpu_vm_msgtable.py and tests/test_gpu_vm_msgtable_locate.py: sets over a resident message table (two keys per set, messages of mixed
lengths including the empty one), the defects of the shared-message tests applied one at a time, the calls of the mbls_verify_multiple*_msgtable* entries with
canaries around their outputs, and the judges -- the existing entries on the spelled-out messages. Case, DevCase and the baselines are those of
tests/test_gpu_vm_shared_locate.py and tests/test_gpu_vm_shared_msgs.py, imported."""
import random

import numpy as np

import helpers
import orc
import test_gpu_vm_shared_locate as SL
import test_gpu_vm_shared_msgs as SM

REJECT_BATCH = SM.REJECT_BATCH
DEFECTS = SM.DEFECTS
ST_BAD_MSG_RANGE, ST_PAIRING_FAILED = 0x100, 0x40
N_SETS = SM.N_SETS
LENS = SL.RAGGED_LENS
NO_ENTRY = 0xFFFFFFFF
_SIGS = {}


def messages(seed, count):
    """count distinct messages of mixed lengths; entry 0 is the empty message"""
    rnd = random.Random(seed)
    out = []
    for j in range(count):
        ln = LENS[j % len(LENS)]
        out.append(b"" if j == 0 else rnd.randbytes(max(ln, 4)) if ln < 4 else rnd.randbytes(ln))
    assert len(set(out)) == count
    return out


def base_case(listed, idx, seed):
    """len(idx) <= 150 valid sets over `listed`: the module-wide keys of the shared-message tests (two per set), signatures made once per (set, message)"""
    sks, wire, apks = SM._keys(3000)
    n = len(idx)
    sigs = []
    for i, j in enumerate(idx):
        k = (i, listed[j])
        if k not in _SIGS:
            _SIGS[k] = orc.g2_compress(orc.sign(listed[j], (sks[i][0] + sks[i][1]) % helpers.R))
        sigs.append(_SIGS[k])
    rnd = random.Random(seed)
    return SL.Case(sigs, apks[:n], wire[:n], [rnd.randrange(1, 1 << 63) for _ in range(n)], listed, idx)


def with_defect(c, kind, i, probe):
    """a copy of c with defect `kind` on set i"""
    b = SL.Case(c.sigs, c.apks, c.wire, c.rands, c.listed, c.idx)
    other = (i + 1) % c.n
    if kind == "wrong_key":
        b.apks[i], b.wire[i] = c.apks[other], list(c.wire[other])
    elif kind == "swapped_sig":
        b.sigs[i] = c.sigs[other]
    elif kind == "inf_sig":
        b.sigs[i] = helpers.G2_INF
    elif kind in ("inf_key", "both_inf"):
        b.apks[i] = SL.G1_INF_U; b.wire[i] = [c.wire[i][0], orc.g1_mul(c.wire[i][0], helpers.R - 1)]
        if kind == "both_inf":
            b.sigs[i] = helpers.G2_INF
    elif kind == "not_in_g2":
        b.sigs[i] = probe
    elif kind == "undecodable":
        b.sigs[i] = bytes([c.sigs[i][0] & 0x7F]) + c.sigs[i][1:]
    elif kind == "zero_scalar":
        b.rands[i] = 0
    else:
        raise ValueError(kind)
    return b


def make_table(N, listed, capacity_hint=0, pieces=1):
    """a resident table holding `listed` in order, appended in `pieces` host appends"""
    mt = N.MsgTable(capacity_hint=capacity_hint)
    step = (len(listed) + pieces - 1) // pieces if listed else 1
    for a in range(0, len(listed), step):
        part = listed[a:a + step]
        assert mt.append(b"".join(part), len(part), msg_len=0, msg_offsets=SL._offsets(part)) == a
    assert len(mt) == len(listed)
    return mt


def bufs(n):
    import torch
    return (torch.full((8,), 7, dtype=torch.uint8, device="cuda:0"), torch.full((2,), -1, dtype=torch.int32, device="cuda:0"),
            torch.full((n + 8,), 7, dtype=torch.uint8, device="cuda:0"), torch.full((n + 2,), -1, dtype=torch.int32, device="cuda:0"))


def read(n, out, locate):
    """the outputs after the canary checks: 7 behind the result byte and behind set_results[n], -1 behind the status word and set_status[n]"""
    import torch
    torch.cuda.synchronize()
    res, st, sres, sst = out
    r = (int(res[0].item()), int(st[0].item()) & 0xFFFFFFFF)
    assert [int(x) for x in res.cpu().numpy()[1:]] == [7] * 7 and int(st[1].item()) == -1
    if not locate:
        assert [int(x) for x in sres.cpu().numpy()] == [7] * (n + 8)
        return r
    assert [int(x) for x in sres.cpu().numpy()[n:]] == [7] * 8 and [int(x) for x in sst.cpu().numpy()[n:]] == [-1, -1]
    return r + ([int(x) for x in sres.cpu().numpy()[:n]], [int(x) & 0xFFFFFFFF for x in sst.cpu().numpy()[:n]])


def enqueue_table(N, d, mt, locate, indexed=False, idx=None, stream=None):
    """one call of the device entry over the table under the context's current grouping mode; only enqueues -> the output buffers"""
    ctx = N.default_context()
    out = bufs(d.n)
    res, st, sres, sst = out
    idx = d.idx if idx is None else idx
    L = N.lib()
    tail = (res.data_ptr(), st.data_ptr()) + ((sres.data_ptr(), sst.data_ptr()) if locate else ()) + (stream,)
    common = (mt.handle, idx.data_ptr(), d.rands.data_ptr(), d.n)
    if indexed:
        f = L.mbls_verify_multiple_sets_indexed_msgtable_locate_device if locate else L.mbls_verify_multiple_sets_indexed_msgtable_device
        rc = f(ctx.handle, d.tab.handle, d.sigs.data_ptr(), d.key_idx.data_ptr(), None, 2, *common, *tail)
    else:
        f = L.mbls_verify_multiple_msgtable_locate_device if locate else L.mbls_verify_multiple_msgtable_device
        rc = f(ctx.handle, d.sigs.data_ptr(), d.apks.data_ptr(), *common, *tail)
    assert rc == 0, ctx.last_error()
    return out


def call_table(N, d, mt, mode, locate, indexed=False, idx=None):
    """-> (result, status[, set results, set status]) under grouping `mode`"""
    from milagro_bls_amd import batch
    ctx = N.default_context()
    batch.set_vm_grouping(mode, ctx)
    try:
        return read(d.n, enqueue_table(N, d, mt, locate, indexed, idx), locate)
    finally:
        batch.set_vm_grouping(0, ctx)


def judge_call(N, d):
    """the judge of the call's verdict: mbls_verify_multiple_aggregate_signatures_device on the same sets, each set's message spelled out, the same scalars"""
    return SM.run_ungrouped(N, d)


def dev_idx(values):
    return SL._dev(np.array(values, dtype=np.uint32))


def check_verdict(N, c, d, mt, modes=(1, 2, 0), indexed=(False, True), want=None):
    """result byte equal to the judge's, status word equal in the rejecting bits, under every mode and key form; -> the judge's (result, status)"""
    r0, s0 = judge_call(N, d)
    if want is not None:
        assert r0 == int(want), (r0, want)
    for mode in modes:
        for ix in indexed:
            r, s = call_table(N, d, mt, mode, False, ix)
            assert r == r0 and s & REJECT_BATCH == s0 & REJECT_BATCH, (mode, ix, r, hex(s), r0, hex(s0))
    return r0, s0


def check_located(N, c, d, mt, modes=(1, 2, 0), indexed=(False, True)):
    """the locate form: bool and word byte for byte the non-locate entry's under the same mode; every set of an accepted call 1; the sets of a rejected call
    what mbls_verify_multiple_batches_locate[_indexed]_device with one batch on the spelled-out messages gives them -> the reference's (result, set results, words)"""
    ref = {}
    for ix in indexed:
        ref[ix] = SL.one_batch_locate(N, d, ix)
        for mode in modes:
            r0, s0 = call_table(N, d, mt, mode, False, ix)
            res, st, sres, sst = call_table(N, d, mt, mode, True, ix)
            assert (res, st) == (r0, s0), (mode, ix, res, hex(st), r0, hex(s0))
            assert res == ref[ix][0], (mode, ix)
            if res:
                assert sres == [1] * c.n and not any(w & (ST_PAIRING_FAILED | REJECT_BATCH) for w in sst), (mode, ix)
            assert sres == ref[ix][1], (mode, ix, [(i, sres[i], ref[ix][1][i]) for i in range(c.n) if sres[i] != ref[ix][1][i]])
            assert sst == ref[ix][2], (mode, ix, [(i, hex(sst[i]), hex(ref[ix][2][i])) for i in range(c.n) if sst[i] != ref[ix][2][i]])
    return ref[indexed[0]]


# ------------------------------------------------------------------------------------------------ the shapes both files walk
def shape(name):
    """-> (listed, idx): the table's messages and the sets' indices"""
    rnd = random.Random(hash_name(name))
    n = N_SETS
    if name == "every_entry_of_12":
        listed = messages(11, 12)
        idx = list(range(12)) + [rnd.randrange(12) for _ in range(n - 12)]
        rnd.shuffle(idx)
    elif name == "sparse_9_of_2500":
        listed = messages(12, 2500)
        named = [0, 2499, 1200, 1201] + rnd.sample(range(1, 1200), 3) + rnd.sample(range(1202, 2499), 2)
        idx = named + [rnd.choice(named) for _ in range(n - len(named))]
        rnd.shuffle(idx)
    elif name == "one_entry_for_all":
        listed = messages(13, 7)
        idx = [3] * n
    elif name == "one_set_per_entry":
        listed = messages(14, n)
        idx = list(range(n)); rnd.shuffle(idx)
    elif name == "5_of_600":
        listed = messages(15, 600)
        named = [0, 599, 17, 300, 301]
        idx = named + [rnd.choice(named) for _ in range(n - len(named))]
        rnd.shuffle(idx)
    elif name == "20_of_20":
        listed = messages(16, 20)
        idx = list(range(20)) + [rnd.randrange(20) for _ in range(n - 20)]
    elif name == "20_of_40":
        listed = messages(17, 40)
        named = list(range(0, 40, 2))
        idx = named + [rnd.choice(named) for _ in range(n - 20)]
    elif name == "70_of_70":
        listed = messages(18, 70)
        idx = list(range(70)) + [rnd.randrange(70) for _ in range(n - 70)]
    else:
        raise ValueError(name)
    return listed, idx


def hash_name(name):
    return sum((i + 1) * b for i, b in enumerate(name.encode()))


SHAPES = ("every_entry_of_12", "sparse_9_of_2500", "one_entry_for_all", "one_set_per_entry")
_BUILT = {}


def built(N, name, indexed=True):
    """(case, device case, table) of a shape, once per session"""
    if name not in _BUILT:
        listed, idx = shape(name)
        c = base_case(listed, idx, hash_name(name))
        _BUILT[name] = (c, SL.DevCase(N, c, table=indexed), make_table(N, listed))
    return _BUILT[name]
