"""verify_multiple over committee bitfields (mbls_verify_multiple_committee_msgtable[_locate]_device: a committee id and a bitfield, or one key index, per set; keys
and messages resident) against the entry it has to equal, mbls_verify_multiple_sets_indexed_msgtable[_locate]_device on the same sets with the signers spelled out
through a ragged offset table, measured in the same process on the same sets. Shapes: 2^16 sets over 512 committees of 128 members and 512 table entries at 100,
99, 90 and 50 % participation; 2^16 sets over one 512-member committee at 99 %; a gossip mix of two single-key sets per committee set (128 members, 99 %); and
1 024 sets over 8 table entries (128 members, 99 %). Device-resident inputs.
Every shape is measured in two forms. `rejected`: every 16th committee set (the j-th with j % 16 == 7) has one bit flipped against its signers, so the call must
answer 0 and the locate form must name exactly those sets -- both legs are rejected calls, so both sides run their _locate entry. `accepted`: the honest fields,
the plain entries on both sides, the call must answer 1.
Same timing method for every variant: a host clock around a window of repetitions that ends in a device synchronise, every shape warmed up, the variants alternated
inside every round, medians over the rounds with [min, max] beside them. Every result of every window is checked.
The output also carries `bench_vs_parent`: the ms_per_step of bench.py runs of the parent commit and of this tree, read from the two files of bench.py result
lines beside the output (bench_vm_committee_parent.jsonl, bench_vm_committee_this_tree.jsonl: one `bench.py --gpus 1 --steps 20 --warmup 5` line per run, taken
alternately); the block is left out where those files are absent.
usage: python scripts/vm_committee_throughput.py [OUT.json]   (default: profiles/vm_committee_throughput.json; VCT_ROUNDS, default 10)"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
from milagro_bls_amd import _native as N

lib = N.lib(); dev = torch.device("cuda:0")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vm_committee_throughput.json")
ROUNDS = int(os.environ.get("VCT_ROUNDS", "10"))
WINDOW_S = 0.2
SINGLE = N.VM_SET_SINGLE_KEY
ctx = N.default_context()
P = lambda t: t.data_ptr()
pool = bench.make_pool(bench.SEED)
POOL = len(pool)
limbs = np.array([[(sk >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for sk in pool], dtype=np.uint64)
d_pool_sk = torch.from_numpy(np.frombuffer(b"".join(s.to_bytes(32, "big") for s in pool), dtype=np.uint8).reshape(POOL, 32).copy()).to(dev)
d_pool_pk = torch.empty((POOL, 96), dtype=torch.uint8, device=dev)
ctx.check(lib.mbls_sk_to_pk_batch_device(ctx.handle, P(d_pool_sk), N.PK_UNCOMPRESSED, POOL, P(d_pool_pk), None))
table = N.KeyTable(ctx, capacity_hint=POOL)
d_errs = torch.zeros(POOL, dtype=torch.uint8, device=dev)
table.append_device(P(d_pool_pk), POOL, P(d_errs), pk_format=N.PK_UNCOMPRESSED, validate=False)
torch.cuda.synchronize(); assert int(d_errs.max().item()) == 0


def window(f, reps, clear):
    clear()
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def stat(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def measure(variants, clear, good, tag):
    reps, times = {}, {}
    for name, f in variants:
        window(f, 1, clear)
        est = window(f, 1, clear)
        assert good(), (tag, name)
        reps[name] = max(1, min(64, int(math.ceil(WINDOW_S / est))))
        times[name] = []
    for _ in range(ROUNDS):
        for name, f in variants:
            times[name].append(1e3 * window(f, reps[name], clear))
            assert good(), (tag, name)
    return {name: dict(stat(times[name]), reps_per_window=reps[name]) for name, _ in variants}


def committees_of(count, m, seed):
    """count committees of m distinct pool keys each (an odd stride from a random start)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, POOL, size=count, dtype=np.int64)
    s = rng.integers(0, POOL // 2, size=count, dtype=np.int64) * 2 + 1
    return (a[:, None] + np.arange(m, dtype=np.int64)[None, :] * s[:, None]) % POOL


def sets_of(members, percent, n, singles_per_committee_set, seed):
    """n sets: committee sets (exactly round(m percent / 100) signers each) with `singles_per_committee_set` single-key sets behind each. -> per set the descriptor
    word, the signers' secret key, the honest and the flipped bitfields, both spelled-out lists with their offsets, which sets are flipped"""
    count, m = members.shape
    rng = np.random.default_rng(seed)
    is_cmt = (np.arange(n) % (1 + singles_per_committee_set)) == 0
    nc = int(is_cmt.sum())
    cid = rng.integers(0, count, size=nc, dtype=np.int64)
    s = max(1, int(round(m * percent / 100.0)))
    order = np.argsort(rng.random((nc, m)), axis=1)
    signed = np.zeros((nc, m), dtype=bool)
    np.put_along_axis(signed, order[:, :s], True, axis=1)
    sk = np.zeros((n, 32), dtype=np.uint8)
    csk = np.zeros((nc, 32), dtype=np.uint8)
    for c0 in range(0, nc, 2048):
        agg = (limbs[members[cid[c0:c0 + 2048]]] * signed[c0:c0 + 2048, :, None]).sum(axis=1)
        for i in range(agg.shape[0]):
            v = sum(int(agg[i, j]) << (32 * j) for j in range(8)) % bench.R
            csk[c0 + i] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    sk[is_cmt] = csk
    key = rng.integers(0, POOL, size=n, dtype=np.int64)                 # the single-key sets' keys
    pool_sk = np.frombuffer(b"".join(x.to_bytes(32, "big") for x in pool), dtype=np.uint8).reshape(POOL, 32)
    sk[~is_cmt] = pool_sk[key[~is_cmt]]
    words = np.where(is_cmt, 0, SINGLE | key).astype(np.uint32)
    words[is_cmt] = cid.astype(np.uint32)
    named = signed.copy()
    flip = np.arange(7, nc, 16)
    pos = rng.integers(0, m, size=flip.size)
    named[flip, pos] ^= True
    expect = np.ones(n, dtype=np.uint8); expect[np.flatnonzero(is_cmt)[flip]] = 0
    out = {"words": words, "sk": sk, "expect": expect, "signers": s, "committee_sets": nc}
    for tag, sel in (("honest", signed), ("flipped", named)):
        bits_c = np.packbits(sel, axis=1, bitorder="little")             # SSZ bit order: member j is bit j & 7 of byte j >> 3
        stride = (bits_c.shape[1] + 3) // 4 * 4
        bits = np.zeros((n, stride), dtype=np.uint8)
        bits[is_cmt, :bits_c.shape[1]] = bits_c
        cnt = np.ones(n, dtype=np.int64); cnt[is_cmt] = sel.sum(axis=1)
        off = np.concatenate([[0], np.cumsum(cnt)])
        lists = np.zeros(int(off[-1]), dtype=np.int64)
        starts = off[:-1]
        lists[starts[~is_cmt]] = key[~is_cmt]
        flat = members[cid][sel]                                         # row-major: every committee set's named members in member order
        cstart = starts[is_cmt]; ccnt = cnt[is_cmt]
        lists[np.repeat(cstart, ccnt) + (np.arange(flat.size) - np.repeat(np.cumsum(ccnt) - ccnt, ccnt))] = flat
        out[tag] = (bits, stride, lists, off)
    return out


out = {"form": "device-resident inputs, keys and 32-byte messages resident; `rejected`: every 16th committee set has one bit flipped against its signers, _locate entries on both "
               "sides; `accepted`: honest fields, plain entries on both sides",
       "rounds": ROUNDS, "window_seconds": WINDOW_S,
       "timing": "host clock around a window of `reps` repetitions ending in a device synchronise; ms per repetition; median [min, max] over the rounds",
       "baseline": "mbls_verify_multiple_sets_indexed_msgtable[_locate]_device on the same sets, signers spelled out through a ragged offset table",
       "round_items": int(ctx.limits().round_items), "shapes": {}}
# (name, sets, members, committees, percent, single-key sets per committee set, table entries)
SHAPES = [("128_members/%d_percent" % p, 65536, 128, 512, p, 0, 512) for p in (100, 99, 90, 50)] + \
         [("512_members/99_percent", 65536, 512, 1, 99, 0, 512), ("gossip_mix_2_single_per_committee_set/128_members/99_percent", 65536, 128, 512, 99, 2, 512),
          ("1024_sets_over_8_entries/128_members/99_percent", 1024, 128, 512, 99, 0, 8)]
ctx.reserve(N.plan_verify_multiple_msgtable_locate_workspace_items(65536, 512, 0, 0, ctx.limits())); ctx.reserve_committee_items(65536, 512)
tables, msgtabs = {}, {}
for name, n, m, count, percent, singles, T in SHAPES:
    if (m, count) not in tables:
        members = committees_of(count, m, 31 + m)
        ct = N.CommitteeTable(table, capacity_hint=count)
        assert ct.append(members.reshape(-1).tolist(), list(range(0, count * m + 1, m))) == 0
        tables[(m, count)] = (members, ct)
    if T not in msgtabs:
        d_list = torch.from_numpy(np.random.default_rng(5 + T).integers(0, 256, size=(T, 32), dtype=np.uint8)).to(dev)
        mt = N.MsgTable(ctx, capacity_hint=T)
        assert mt.append_device(P(d_list), T, msg_len=32) == 0
        msgtabs[T] = (d_list, mt)
    members, ct = tables[(m, count)]; d_list, mt = msgtabs[T]
    rng = np.random.default_rng(9 + n + T)
    midx = rng.integers(0, T, size=n, dtype=np.int64)
    d_midx = torch.from_numpy(midx.astype(np.int32)).to(dev)
    d_signed_msgs = d_list[torch.from_numpy(midx).to(dev)].contiguous()
    S = sets_of(members, percent, n, singles, 100 * m + percent + singles)
    d_sk = torch.from_numpy(S["sk"]).to(dev)
    d_sigs = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    ctx.check(lib.mbls_sign_batch_device(ctx.handle, P(d_sk), P(d_signed_msgs), 32, n, P(d_sigs), None))
    d_words = torch.from_numpy(S["words"].view(np.int32)).to(dev)
    d_rands = torch.from_numpy(rng.integers(1, 1 << 63, size=n, dtype=np.int64)).to(dev)
    d_res = torch.zeros(1, dtype=torch.uint8, device=dev); d_sres = torch.zeros(n, dtype=torch.uint8, device=dev)
    expect = torch.from_numpy(S["expect"]).to(dev)
    route = "complement" if N.plan_committee_route(m, S["signers"]) else "direct"
    row = {"sets": n, "committee_sets": S["committee_sets"], "single_key_sets": n - S["committee_sets"], "members": m, "committees": count, "table_entries": T,
           "participation_percent": percent, "signers": S["signers"], "route": route, "flipped_sets": int((S["expect"] == 0).sum()),
           "grouping": {0: "per_set", 1: "grouped"}[N.plan_verify_multiple_msgtable(n, T, 0, 0, ctx.limits())["route"]]}
    for form, tag, locate in (("rejected", "flipped", True), ("accepted", "honest", False)):
        bits, stride, lists, off = S[tag]
        d_bits = torch.from_numpy(bits).to(dev)
        d_keys = torch.from_numpy(lists.astype(np.uint32).view(np.int32)).to(dev); d_off = torch.from_numpy(off.astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize()
        if locate:
            base = lambda: ctx.check(lib.mbls_verify_multiple_sets_indexed_msgtable_locate_device(ctx.handle, table.handle, P(d_sigs), P(d_keys), P(d_off), 0, mt.handle, P(d_midx),
                                                                                                  P(d_rands), n, P(d_res), None, P(d_sres), None, None))
            cmt = lambda: ctx.check(lib.mbls_verify_multiple_committee_msgtable_locate_device(ctx.handle, ct.handle, P(d_sigs), P(d_words), P(d_bits), stride, mt.handle, P(d_midx),
                                                                                              P(d_rands), n, P(d_res), None, P(d_sres), None, None))
            good = lambda: int(d_res.item()) == 0 and bool((d_sres == expect).all())
        else:
            base = lambda: ctx.check(lib.mbls_verify_multiple_sets_indexed_msgtable_device(ctx.handle, table.handle, P(d_sigs), P(d_keys), P(d_off), 0, mt.handle, P(d_midx),
                                                                                           P(d_rands), n, P(d_res), None, None))
            cmt = lambda: ctx.check(lib.mbls_verify_multiple_committee_msgtable_device(ctx.handle, ct.handle, P(d_sigs), P(d_words), P(d_bits), stride, mt.handle, P(d_midx),
                                                                                       P(d_rands), n, P(d_res), None, None))
            good = lambda: int(d_res.item()) == 1

        def clear():
            d_res.fill_(7); d_sres.fill_(7)
        variants = [("committee", cmt), ("indexed", base)]
        if route == "complement":                                   # the same entry held on the direct route: what k_vmc_expand costs on its own
            def direct():
                ctx.set_committee_route(N.CMT_ROUTE_DIRECT); cmt(); ctx.set_committee_route(N.CMT_ROUTE_AUTO)
            variants.append(("committee_forced_direct", direct))
        r = measure(variants, clear, good, (name, form))
        r["entries"] = "_locate" if locate else "plain"
        r["input_bytes_per_set"] = {"committee": 4 + stride, "indexed": round(4.0 * lists.size / n + 4, 1)}
        r["saved_vs_indexed_ms"] = round(r["indexed"]["ms_median"] - r["committee"]["ms_median"], 4)
        r["indexed_spread_ms"] = round(r["indexed"]["ms_max"] - r["indexed"]["ms_min"], 4)
        r["faster_beyond_indexed_spread"] = bool(r["saved_vs_indexed_ms"] > r["indexed_spread_ms"])
        r["slower_beyond_indexed_spread"] = bool(-r["saved_vs_indexed_ms"] > r["indexed_spread_ms"])
        row[form] = r
        print("%-62s %-8s %-10s  committee %8.3f ms [%.3f, %.3f]   indexed %8.3f ms [%.3f, %.3f]   saved %7.3f ms (spread %.3f)" % (
            name, form, route, r["committee"]["ms_median"], r["committee"]["ms_min"], r["committee"]["ms_max"], r["indexed"]["ms_median"], r["indexed"]["ms_min"],
            r["indexed"]["ms_max"], r["saved_vs_indexed_ms"], r["indexed_spread_ms"]), flush=True)
    out["shapes"][name] = row
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:                                      # (kept current shape by shape)
        json.dump(out, fh, indent=1); fh.write("\n")
for _, ct in tables.values():
    ct.close()
for _, mt in msgtabs.values():
    mt.close()
table.close()
# ---- bench.py against the parent commit: the result lines of the alternated runs, where they lie beside the output
lines = {}
for who in ("parent", "this_tree"):
    path = os.path.join(os.path.dirname(os.path.abspath(OUT)), "bench_vm_committee_%s.jsonl" % who)
    if os.path.exists(path):
        with open(path) as fh:
            lines[who] = [round(json.loads(l)["ms_per_step"], 4) for l in fh if l.strip()]
if len(lines) == 2:
    out["bench_vs_parent"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 5 of the parent commit and of this tree, alternated (full lines: bench_vm_committee_parent.jsonl, "
                                      "bench_vm_committee_this_tree.jsonl beside this file)",
                              "parent_ms_per_step": lines["parent"], "this_tree_ms_per_step": lines["this_tree"]}
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", OUT)
