"""The Python model of the grouping of mbls_verify_multiple_batches_committee_msgtable* (milagro_bls_amd/csrc/mbls_vbg.h) and the cases the CPU harness
(tests/test_vm_batches_committee_cpu.py) and the GPU probe (tests/test_gpu_vm_batches_committee.py) are both held to, word for word."""
import random

NONE = 0xFFFFFFFF
SHARED = 0xFFFFFFFE
BAD_MSG = 0x100
CAP = 1024                      # MBLS_VBG_MAX_SETS


def ranges(n, B, spb=None, off=None):
    """batch b -> (lo, hi, range is sound); a faulty range is empty"""
    out = []
    for b in range(B):
        if off is None:
            lo, hi = spb * b, spb * b + spb
            out.append((lo, hi, hi <= n))
        else:
            lo, hi = off[b], off[b + 1]
            out.append((lo, hi, True) if lo <= hi <= n else (0, 0, False))
    return out


def set_map(n, B, off):
    """set -> the one batch with a sound range that claims it, SHARED for two or more, NONE for nobody"""
    m = [NONE] * n
    for b, (lo, hi, ok) in enumerate(ranges(n, B, off=off)):
        if ok:
            for j in range(lo, hi):
                m[j] = b if m[j] == NONE else SHARED
    return m


def model(idx, T, B, spb=None, off=None):
    """the arrays of k_vbg_group and the scan of the group counts, stated set by set"""
    n = len(idx)
    rg = ranges(n, B, spb, off)
    owner = set_map(n, B, off) if off is not None else None
    r = {k: [NONE] * n for k in ("pos", "pos_lo", "pos_hi", "head", "entry")}
    r["status"] = [0] * n
    r["count"] = [0] * B
    for b, (lo, hi, ok) in enumerate(rg):
        if not ok:
            continue
        mine = [j for j in range(lo, hi) if owner is None or owner[j] == b]
        for j in mine:
            if idx[j] >= T:
                r["status"][j] |= BAD_MSG
        if len(mine) != hi - lo:
            continue                                        # not sound: it joins nothing
        valid = [j for j in mine if idx[j] < T]
        if hi - lo > CAP:
            groups = [[j] for j in valid]                   # not grouped: every valid set a group of its own
        else:
            by_entry = {}
            for j in valid:
                by_entry.setdefault(idx[j], []).append(j)
            groups = sorted(by_entry.values(), key=lambda g: g[0])          # leader order
        start = lo
        for g, members in enumerate(groups):
            r["head"][lo + g], r["entry"][lo + g] = start, idx[members[0]]
            for rank, j in enumerate(members):
                r["pos"][j] = start + rank
                r["pos_lo"][start + rank], r["pos_hi"][start + rank] = start, start + len(members)
            start += len(members)
        r["count"][b] = len(groups)
    r["off"] = [0]
    for c in r["count"]:
        r["off"].append(r["off"][-1] + c)
    return r


def bound(n, B, T, spb, max_groups):
    """the host's bound on the groups; the T-per-batch term holds only where no batch can be larger than the cap (such a batch has one group per valid set)"""
    v = min(n, B * T) if (spb or n) <= CAP else n
    if spb:
        v = min(v, B * spb)
    if max_groups:
        v = min(v, max_groups)
    return v


def live(goff, B, bnd):
    """global group r < bnd -> its batch, or -1: no such group, or its batch overflows"""
    out = []
    for r in range(bnd):
        b = next((b for b in range(B) if goff[b] <= r < goff[b + 1]), None)
        out.append(-1 if b is None or goff[b + 1] > bnd else b)
    return out


def cases(big=True):
    """(idx, T, B, spb or None, off or None, max_groups). big=False leaves the cases around the cap out of the parametrised GPU runs that do not need them."""
    rnd = random.Random(20271)
    out = []
    sizes = [0, 1, 2, 63, 64, 65, 129] + ([CAP, CAP + 1] if big else [])
    # one batch of each size: all sets on one entry, all on distinct entries, a few entries, indices at and above T, T = 0
    for m in sizes:
        out.append(([5] * m, 9, 1, m, None, 0))
        out.append((rnd.sample(range(m + 7), m), m + 7, 1, m, None, 0))
        out.append(([rnd.randrange(4) for _ in range(m)], 4, 1, m, None, 0))
        out.append(([rnd.choice([0, 1, 2, 3, 4, 7, NONE]) for _ in range(m)], 4, 1, m, None, 0))
        out.append(([rnd.randrange(3) for _ in range(m)], 0, 1, m, None, 0))
    # all sizes as the ragged batches of one call, in a seeded order; the same with a promise that is too small for the batches at the end
    order = sizes[:]
    rnd.shuffle(order)
    off = [0]
    for m in order:
        off.append(off[-1] + m)
    idx = [rnd.randrange(6) for _ in range(off[-1])]
    exact = model(idx, 6, len(order), off=off)["off"][-1]
    out.append((idx, 6, len(order), None, off, 0))
    out.append((idx, 6, len(order), None, off, exact))
    out.append((idx, 6, len(order), None, off, max(1, exact // 2)))
    out.append((idx, 6, len(order), None, off, 1))
    # uniform layouts
    for spb, B in ((1, 40), (10, 13), (64, 3), (65, 2)):
        idx = [rnd.randrange(5) for _ in range(spb * B)]
        out.append((idx, 5, B, spb, None, 0))
        out.append((idx, 5, B, spb, None, 7))
    # faulty tables: backwards, overlapping, sets nobody covers, a range beyond n, everything at once
    n = 60
    idx = [rnd.choice([0, 1, 2, 9]) for _ in range(n)]
    for off in ([0, 20, 10, 30, 60], [0, 30, 20, 45, 60], [5, 20, 20, 50, 55], [0, 10, 70, 60, 60], [0, 40, 10, 50, 61], [0, 60, 0, 60, 60], [60, 0, 0, 0, 0]):
        out.append((idx, 3, 4, None, off, 0))
    return out
