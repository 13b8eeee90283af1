"""What signing and sk -> pk LEAVE in device memory (include/mbls.h "SECRET KEYS ON THE DEVICE"), read back through the residue probe
(mbls_ctx_residue_regions / mbls_ctx_residue_read: every device allocation the context owns -- tests/test_secret_residue_cpu.py holds the list complete).

Differential, so no representation has to be known: on ONE fresh context the same call runs three times on the same messages and the same n -- secret keys
A, snapshot S1; keys B, snapshot S2; keys A again, snapshot S3. Never-written allocator garbage is the same in all three and cancels.
  premise  S1 == S3 everywhere (a byte that differs is nondeterminism this test cannot judge: it fails, named by region, slot, limb and item);
  claim    S1 == S2 everywhere, except that the staging buffer a host entry downloaded its result from may differ inside [0, out_bytes), where it must hold
           what the call returned. A difference is reported as (region, slot range, item ranges): the work list of the fix;
  wipes    what the header calls wiped reads zero in every snapshot: the staged keys, d_sksel (constant-time form) / d_skidx (variable-time form) and the
           wiped workspace slots of the call's items.
A_i and B_i differ in all four base-|x| digits of sk mod r and in every hexadecimal digit, so every lane's table, every selected record, every partial product
and every tree operand differs between the runs: a resting place cannot hide behind equal values.

Sizes: signing adds 4 n items in two tree levels, a level on lanes (k_g2_tree_d) iff it has more than MBLS_COOP_TREE_PAIRS = 2 048 pairs: n = 1, 3 (both levels
wave programs), 1 500 (3 000 pairs on lanes, then 1 500 on waves), 2 100 and 2 101 (both on lanes; an odd item count). sk -> pk: n = 1, 65, 130 (one and three
waves of k_sk_select, a key-sum wave with idle lanes). The context reserves what the call needs and no more (the largest snapshot is ~55 MB). Calls above one
chunk (65 536 signatures) are out of scope here: that workspace is 1.6 GB; the chunk loop reuses the items [0, 4 * chunk) that the final wipes cover.

Two controls show that the test can fail: two verify_multiple calls with different blinding scalars DO differ in workspace slots 25..30 (below), and a build
with one ws_wipe line of mbls_sign_batch_device removed fails the signing cases with that slot range named (done by hand for the change that added this
module: DESIGN section 6)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

X_ABS = 0xd201000000010000                 # |x|: sk mod r = a0 + a1 |x| + a2 |x|^2 + a3 |x|^3, one 64-bit multiplication per digit (k_sign_blind)
SLOT_TOTAL, LIMBS = 133, 12                # the workspace: row 12 * slot + limb of `cap` items, 4 bytes each
SEED = 0x7265736964756573
N_MAX = 2101
# the workspace slots the header calls wiped, [lo, hi): over items [0, 4 n) after signing, [0, n) after sk -> pk
WIPED_SIGN = ((3, 7), (25, 31), (43, 49), (49, 103))
WIPED_SKPK = ((0, 3),)
KEYREC_BYTES = 128


@pytest.fixture(scope="module")
def mb():
    import milagro_bls_amd  # noqa: F401
    from milagro_bls_amd import batch, _native
    _native.default_context()          # raises if the HIP library or the GPU is missing: no fallback
    return batch


@pytest.fixture
def ctx(mb):
    """a FRESH context per test: its allocations are exactly what the call under test reserves"""
    from milagro_bls_amd import _native
    c = _native.Context()
    yield c
    c.close()


def base_x_digits(sk):
    k = sk % helpers.R
    return [(k // X_ABS ** j) % X_ABS for j in range(4)]


@functools.lru_cache(maxsize=None)
def key_sets():
    """N_MAX pairs (A_i, B_i) of secret keys in [1, r) that differ in every hexadecimal digit and in all four base-|x| digits of sk mod r"""
    rnd = random.Random(SEED)
    A, B = [], []
    while len(A) < N_MAX:
        da = [rnd.randrange(7)] + [rnd.randrange(16) for _ in range(63)]              # top digit below 7: below r = 0x73ed...
        db = [(da[0] + rnd.randrange(1, 7)) % 7] + [(d + rnd.randrange(1, 16)) % 16 for d in da[1:]]
        a, b = int("".join("%x" % d for d in da), 16), int("".join("%x" % d for d in db), 16)
        if a == 0 or b == 0 or any(x == y for x, y in zip(base_x_digits(a), base_x_digits(b))):
            continue
        A.append(a); B.append(b)
    for a, b in zip(A, B):
        assert 0 < a < helpers.R and 0 < b < helpers.R
        ha, hb = "%064x" % a, "%064x" % b
        assert all(x != y for x, y in zip(ha, hb))
        assert all(x != y for x, y in zip(base_x_digits(a), base_x_digits(b)))
    # sk -> pk marks a key that has a digit 0 in its status word: among the first 65 pairs some differ in that, so the words differ unless they are wiped
    assert any(("0" in "%064x" % a) != ("0" in "%064x" % b) for a, b in zip(A[:65], B[:65]))
    return b"".join(a.to_bytes(32, "big") for a in A), b"".join(b.to_bytes(32, "big") for b in B)


def keys(n):
    a, b = key_sets()
    return a[:32 * n], b[:32 * n]


@functools.lru_cache(maxsize=None)
def messages():
    return random.Random(SEED + 1).randbytes(32 * N_MAX)


# ------------------------------------------------------------------------------------------------ snapshots and their differences
def snapshot(ctx):
    regions, cap = ctx.residue_regions()
    return cap, [(name, np.frombuffer(ctx.residue_read(i, 0, size), dtype=np.uint8)) for i, (name, size) in enumerate(regions)]


def runs(idx):
    """a sorted index array as a list of inclusive ranges"""
    if idx.size == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) > 1)
    lo = np.concatenate(([idx[0]], idx[cut + 1])); hi = np.concatenate((idx[cut], [idx[-1]]))
    return list(zip(lo.tolist(), hi.tolist()))


def ws_view(cap, a):
    assert a.size == SLOT_TOTAL * LIMBS * cap * 4
    return a.view(np.uint32).reshape(SLOT_TOTAL, LIMBS, cap)


def differences(s1, s2):
    """[(region, slot or None, limbs or None, ranges)]: for the workspace one entry per slot with the items (and the limbs) that differ, for every other region
    the byte ranges"""
    (cap1, r1), (cap2, r2) = s1, s2
    assert cap1 == cap2 and [(n, a.size) for n, a in r1] == [(n, a.size) for n, a in r2], "the context's allocations changed between the snapshots"
    out = []
    for (name, a), (_, b) in zip(r1, r2):
        if name == "d_w" and a.size:
            d = ws_view(cap1, a) != ws_view(cap1, b)
            per_slot = d.any(axis=1)
            for slot in np.flatnonzero(per_slot.any(axis=1)).tolist():
                out.append((name, slot, tuple(np.flatnonzero(d[slot].any(axis=1)).tolist()), runs(np.flatnonzero(per_slot[slot]))))
        else:
            idx = np.flatnonzero(a != b)
            if idx.size:
                out.append((name, None, None, runs(idx)))
    return out


def describe(diffs):
    """the work list: consecutive workspace slots that differ over the same items as one line"""
    lines, i = [], 0
    while i < len(diffs):
        name, slot, limbs, rg = diffs[i]
        j = i
        while slot is not None and j + 1 < len(diffs) and diffs[j + 1][0] == name and diffs[j + 1][1] == diffs[j][1] + 1 and diffs[j + 1][2:] == (limbs, rg):
            j += 1
        shown = ", ".join("%d..%d" % r for r in rg[:6]) + (" ... (%d ranges)" % len(rg) if len(rg) > 6 else "")
        if slot is None:
            lines.append("%s bytes %s" % (name, shown))
        else:
            lines.append("%s slots %d..%d limbs %s items %s" % (name, slot, diffs[j][1], "%d..%d" % (limbs[0], limbs[-1]) if len(limbs) > 1 else limbs[0], shown))
        i = j + 1
    return "\n  " + "\n  ".join(lines)


def region(snap, name):
    return dict(snap[1])[name]


def drop_staged_output(diffs, snaps, outs):
    """the one exception of the claim: ONE staging buffer may differ between the runs, inside [0, out_bytes) only, and there it holds what each call returned"""
    rest, seen = [], 0
    for d in diffs:
        name, _, _, rg = d
        nb = len(outs[0])
        if name.startswith("stage[") and rg[-1][1] < nb and all(region(s, name)[:nb].tobytes() == o for s, o in zip(snaps, outs)):
            seen += 1
            continue
        rest.append(d)
    assert seen <= 1
    return rest


def check_three_runs(ctx, call, n, items, wiped, host, out_bytes):
    """call(keys) -> the bytes the entry returned; the three runs, the premise, the claim and the documented wipes"""
    ka, kb = keys(n)
    snaps, outs = [], []
    for k in (ka, kb, ka):
        outs.append(call(k)); snaps.append(snapshot(ctx))
    assert len(outs[0]) == out_bytes and outs[0] == outs[2] and outs[0] != outs[1]
    for j in range(0, out_bytes, out_bytes // n):
        assert outs[0][j:j + out_bytes // n] != outs[1][j:j + out_bytes // n]
    premise = differences(snaps[0], snaps[2])
    assert not premise, "the same call on the same keys left different bytes (nondeterminism, not judged here):" + describe(premise)
    claim = differences(snaps[0], snaps[1])
    if host:
        claim = drop_staged_output(claim, snaps[:2], outs[:2])
    assert not claim, "device memory depends on the secret keys after the call returned:" + describe(claim)
    cap = snaps[0][0]
    assert cap >= items
    for s in snaps[:2]:
        w = ws_view(cap, region(s, "d_w"))
        for lo, hi in wiped:
            nz = np.flatnonzero(w[lo:hi, :, :items].any(axis=(0, 1)))
            assert nz.size == 0, "workspace slots %d..%d are not zero in items %s" % (lo, hi - 1, runs(nz)[:6])
        if host:
            assert region(s, "stage[0]").size >= 32 * n and not region(s, "stage[0]")[:32 * n].any(), "the staged secret keys are still there"
    return snaps


# ------------------------------------------------------------------------------------------------ the entries
def device_buffers(n, out_bytes):
    import torch
    dev = torch.device("cuda:0")
    return (torch.zeros(32 * n, dtype=torch.uint8, device=dev), torch.frombuffer(bytearray(messages()[:32 * n]), dtype=torch.uint8).to(dev),
            torch.zeros(out_bytes, dtype=torch.uint8, device=dev))


def put(d, data):
    import torch
    d.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8)); torch.cuda.synchronize()


def get(d):
    import torch
    torch.cuda.synchronize()
    return d.cpu().numpy().tobytes()


@pytest.mark.parametrize("n", [1, 3, 1500, 2100, 2101])
@pytest.mark.parametrize("variable_time", [0, 1], ids=["ct", "vt"])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_signing_leaves_nothing_of_the_keys(mb, ctx, entry, variable_time, n):
    from milagro_bls_amd import _native as N
    ctx.set_secret_ops(variable_time)
    msgs = messages()[:32 * n]
    if entry == "host":
        call = lambda k: mb.sign_batch(k, msgs, n, ctx=ctx)
    else:
        d_sk, d_msg, d_sig = device_buffers(n, 96 * n)

        def call(k):
            put(d_sk, k)
            ctx.check(N.lib().mbls_sign_batch_device(ctx.handle, d_sk.data_ptr(), d_msg.data_ptr(), 32, n, d_sig.data_ptr(), None))
            return get(d_sig)
    check_three_runs(ctx, call, n, 4 * n, WIPED_SIGN, entry == "host", 96 * n)


@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("fmt", [0, 1], ids=["pk48", "pk96"])
@pytest.mark.parametrize("variable_time", [0, 1], ids=["ct", "vt"])
@pytest.mark.parametrize("entry", ["host", "device"])
def test_sk_to_pk_leaves_nothing_of_the_keys(mb, ctx, entry, variable_time, fmt, n):
    from milagro_bls_amd import _native as N
    ctx.set_secret_ops(variable_time)
    out_bytes = (96 if fmt else 48) * n
    if entry == "host":
        call = lambda k: mb.sk_to_pk_batch(k, n, out_format=fmt, ctx=ctx)
    else:
        d_sk, _, d_pk = device_buffers(n, out_bytes)

        def call(k):
            put(d_sk, k)
            ctx.check(N.lib().mbls_sk_to_pk_batch_device(ctx.handle, d_sk.data_ptr(), fmt, n, d_pk.data_ptr(), None))
            return get(d_pk)
    snaps = check_three_runs(ctx, call, n, n, WIPED_SKPK, entry == "host", out_bytes)
    for s in snaps[:2]:
        # the key sum's status words: MBLS_ST_PK_INFINITY marks a key with a hexadecimal digit 0, so the words tell which keys have none
        assert not region(s, "d_status")[:4 * n].any()
        if variable_time:         # the hexadecimal digits of the keys
            assert region(s, "d_skidx").size >= 64 * 4 * n and not region(s, "d_skidx").any()
        else:                     # the multiples the keys' digits selected
            assert region(s, "d_sksel").size >= 64 * KEYREC_BYTES * n and not region(s, "d_sksel").any()


@pytest.mark.parametrize("variable_time", [0, 1], ids=["ct", "vt"])
@pytest.mark.parametrize("entry", ["sign", "pk_from_secret_key"])
def test_one_item_entries_leave_nothing_of_the_key(mb, ctx, entry, variable_time):
    from milagro_bls_amd import _native as N
    ctx.set_secret_ops(variable_time)
    msg = messages()[:32]
    out = (C.c_uint8 * 96)()

    def call(k):
        if entry == "sign":
            ctx.check(N.lib().mbls_sign(ctx.handle, N.cbuf(msg), 32, N.cbuf(k), 32, out))
        else:
            ctx.check(N.lib().mbls_pk_from_secret_key(ctx.handle, N.cbuf(k), 32, out))
        return bytes(out)
    snaps = check_three_runs(ctx, call, 1, 4 if entry == "sign" else 1, WIPED_SIGN if entry == "sign" else WIPED_SKPK, True, 96)
    if entry != "sign":
        for s in snaps[:2]:
            assert not region(s, "d_skidx" if variable_time else "d_sksel").any() and region(s, "d_skidx" if variable_time else "d_sksel").size


# ------------------------------------------------------------------------------------------------ control: the probe sees the workspace, and the rows it claims to
def test_control_blinding_scalars_show_in_slots_25_to_30(mb, ctx):
    """verify_multiple leaves [r_i] sig_i in slot S (25..30) of its items and wipes nothing (nothing there is secret): two calls on the same sets with different
    scalars MUST differ there -- and a third with the first scalars must not"""
    n = 6
    ka, _ = keys(n)
    msgs = messages()[:32 * n]
    sigs, apks = mb.sign_batch(ka, msgs, n, ctx=ctx), mb.sk_to_pk_batch(ka, n, out_format=1, ctx=ctx)
    rnd = random.Random(SEED + 2)
    ra = [rnd.getrandbits(64) | 1 for _ in range(n)]; rb = [(r ^ 0xaaaaaaaaaaaaaaaa) | 1 for r in ra]
    snaps = []
    for r in (ra, rb, ra):
        res, st = mb.verify_multiple_batches(sigs, apks, msgs, r, n, 1, sets_per_batch=n, ctx=ctx)
        assert res == [True] and st == [0]
        snaps.append(snapshot(ctx))
    assert not differences(snaps[0], snaps[2])
    diffs = differences(snaps[0], snaps[1])
    slots = {d[1] for d in diffs if d[0] == "d_w"}
    assert set(range(25, 31)) <= slots, describe(diffs)
