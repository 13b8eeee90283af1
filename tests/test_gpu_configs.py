"""BASELINE.json configs at (or near) their stated sizes on the GPU, through size-independent properties: inputs are
signed on the device by the product's own kernels (bench.build_inputs), so every accepted item is a
sign -> aggregate -> verify round trip, every corrupted item must be rejected, and a subsample is pinned to the oracle."""
import ctypes as C

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import bench
    from milagro_bls_amd import _native as N
    ctx = N.default_context()
    return torch, bench, N, ctx


def test_config3_fast_aggregate_verify_128_keys_both_formats(env):
    # configs[2] AS NAMED: 2^16 items x 128 public keys in the 96-byte form the headline is measured on (26 ms of GPU time; building and signing the batch
    # on the device takes longer); the 48-byte wire form at 2^13 items (its decompression is 8 x the work per item)
    torch, bench, N, ctx = env
    dev = torch.device("cuda:0")
    for fmt in (N.PK_UNCOMPRESSED, N.PK_COMPRESSED):
        n, k = (1 << 16) if fmt == N.PK_UNCOMPRESSED else (1 << 13), 128
        d_sigs, d_msgs, d_pks, expect = bench.build_inputs(ctx, dev, n, k, fmt, rank=3)
        # outputs pre-filled with what no item may end with: a word the call leaves unwritten fails below
        d_res = torch.full((n,), 7, dtype=torch.uint8, device=dev); d_bm = torch.full((n // 64,), -1, dtype=torch.int64, device=dev)
        d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        ctx.check(N.lib().mbls_fast_aggregate_verify_batch_device(ctx.handle, d_sigs.data_ptr(), d_msgs.data_ptr(), 32, None, d_pks.data_ptr(), fmt, None,
                                                                  n, k, d_res.data_ptr(), d_bm.data_ptr(), d_st.data_ptr(), None))
        torch.cuda.synchronize()
        assert torch.equal(d_res.cpu(), expect)
        e = expect.numpy()
        assert (helpers.bitmap_bits(d_bm, n) == e).all()                # every bit of the bitmap, not only the results array
        # every rejected item carries its class's flag (msg bit, wrong key, infinity sig: pairing fails 0x40; sig not in G2 0x02; apk = infinity 0x08)
        # and no undefined bit; accepted items carry none (so no 0x5F rejection bit)
        helpers.check_status_classes(d_st.cpu().numpy(), e)
        # the oracle on a sample over the whole batch: wave edges, the tail, 8+ items of every rejection class (the 48-byte leg decompresses 128 keys per item)
        sel = sorted(set(helpers.sample_indices(n, seed=0x2c0 + fmt, count=1024 if fmt == N.PK_UNCOMPRESSED else 512)) | set(range(48)))
        assert len(sel) >= 512
        helpers.oracle_check_fav(d_sigs, d_msgs, d_pks, sel, k, fmt, expect, d_res)


def test_config4_verify_multiple_2_14_sets_128_keys(env):
    # configs[3]: verify_multiple_aggregate_signatures, 2^14 sets x 128 keys: all valid -> true, one corrupted set -> false
    torch, bench, N, ctx = env
    from milagro_bls_amd import batch
    dev = torch.device("cuda:0")
    n, k = 1 << 14, 128
    d_sigs, d_msgs, d_pks, expect = bench.build_inputs(ctx, dev, n, k, N.PK_UNCOMPRESSED, rank=4, negatives=False)
    g = torch.Generator(device="cpu"); g.manual_seed(7)
    rands = torch.randint(1, (1 << 62), (n,), dtype=torch.int64, generator=g).to(dev)
    args = (d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), rands.data_ptr(), n, k)
    assert batch.verify_multiple_sets_device(*args, pk_format=N.PK_UNCOMPRESSED) is True
    d_msgs[n // 3, 5] ^= 0x10
    assert batch.verify_multiple_sets_device(*args, pk_format=N.PK_UNCOMPRESSED) is False
    d_msgs[n // 3, 5] ^= 0x10
    assert batch.verify_multiple_sets_device(*args, pk_format=N.PK_UNCOMPRESSED) is True
    # a signature outside G2 anywhere in the batch -> false (reference src/aggregates.rs:274-276)
    probe = bytes.fromhex(helpers.load_vectors()["model"]["g2_subgroup_probes"][1]["compressed"])
    keep = d_sigs[n - 1].clone()
    d_sigs[n - 1] = torch.frombuffer(bytearray(probe), dtype=torch.uint8).to(dev)
    assert batch.verify_multiple_sets_device(*args, pk_format=N.PK_UNCOMPRESSED) is False
    d_sigs[n - 1] = keep
    # five kinds of corruption at seeded positions over the whole range: each -> false, the restored input -> true again
    rng = np.random.default_rng(0xc0f3)
    pos = [int(x) for x in rng.choice(n - 1, size=5, replace=False)]
    G2_INF = torch.frombuffer(bytearray(helpers.G2_INF), dtype=torch.uint8).to(dev)

    def spoiled(i, kind):
        if kind == "msg bit":
            d_msgs[i, int(rng.integers(32))] ^= 1 << int(rng.integers(8))
        elif kind == "swap":                                             # two neighbouring signatures swapped
            d_sigs[[i, i + 1]] = d_sigs[[i + 1, i]].clone()
        elif kind == "key":                                              # one key replaced by another pool key
            j = int(rng.integers(k))
            other = next(d_pks[(i + 1) % n, c].clone() for c in range(k) if not torch.equal(d_pks[(i + 1) % n, c], d_pks[i, j]))
            d_pks[i, j] = other
        elif kind == "zero scalar":
            rands[i] = 0
        elif kind == "infinity sig":
            d_sigs[i] = G2_INF

    for i, kind in zip(pos, ("msg bit", "swap", "key", "zero scalar", "infinity sig")):
        keep = [t.clone() for t in (d_sigs, d_msgs, d_pks, rands)]
        spoiled(i, kind)
        assert batch.verify_multiple_sets_device(*args, pk_format=N.PK_UNCOMPRESSED) is False, (i, kind)
        for t, v in zip((d_sigs, d_msgs, d_pks, rands), keep):
            t.copy_(v)
        assert batch.verify_multiple_sets_device(*args, pk_format=N.PK_UNCOMPRESSED) is True, (i, kind)
    # 64 sets at random indices against the oracle with the same blinding scalars: aggregate keys summed on the oracle, valid -> true, one
    # message bit flipped -> false, on both sides
    import orc
    m = 64
    sel = torch.from_numpy(np.sort(rng.choice(n, size=m, replace=False))).to(dev)
    s_sigs, s_msgs, s_pks, s_rands = d_sigs[sel].contiguous(), d_msgs[sel].contiguous(), d_pks[sel].contiguous(), rands[sel].contiguous()
    pk_rows = s_pks.cpu().numpy()
    sets = []
    for i in range(m):
        e, apk = orc.aggregate_pks([pk_rows[i, j].tobytes() for j in range(k)])
        assert e == 0
        sets.append((orc.g2_from_compressed(s_sigs[i].cpu().numpy().tobytes())[1], apk, s_msgs[i].cpu().numpy().tobytes()))
    rr = [int(x) for x in s_rands.cpu().tolist()]
    sub = (s_sigs.data_ptr(), s_pks.data_ptr(), s_msgs.data_ptr(), s_rands.data_ptr(), m, k)
    assert orc.verify_multiple(sets, rr) is True
    assert batch.verify_multiple_sets_device(*sub, pk_format=N.PK_UNCOMPRESSED) is True
    j = int(rng.integers(m))
    s_msgs[j, 0] ^= 1
    sets[j] = (sets[j][0], sets[j][1], s_msgs[j].cpu().numpy().tobytes())
    assert orc.verify_multiple(sets, rr) is False
    assert batch.verify_multiple_sets_device(*sub, pk_format=N.PK_UNCOMPRESSED) is False
    # the first sets of the batch, as before (the device call on a prefix of the same buffers)
    m = 6
    sets = []
    apks, _ = batch.aggregate_public_keys_batch(d_pks[:m].cpu().numpy().tobytes(), m, k, pk_format=N.PK_UNCOMPRESSED)
    for i in range(m):
        sets.append((orc.g2_from_compressed(d_sigs[i].cpu().numpy().tobytes())[1], apks[96 * i:96 * i + 96], d_msgs[i].cpu().numpy().tobytes()))
    rr = [int(x) for x in rands[:m].cpu().tolist()]
    assert orc.verify_multiple(sets, rr) is True
    assert batch.verify_multiple_sets_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), rands.data_ptr(), m, k, pk_format=N.PK_UNCOMPRESSED) is True


def test_bench_two_ranks_sharing_the_gpu_real_verifier():
    """bench.py's multi-rank path with the REAL verifier: two rank processes on this box's one GPU (MBLS_BENCH_SHARE_GPU=1: both on device 0, gathers through
    gloo because RCCL wants one rank per device) -- per-rank inputs, the bitmap gather inside the step, the gathered-bitmap check, MAX / MIN reductions, the
    launcher-free spawn -- and stdout carries exactly ONE line (libraries that print to the C stdout, like RCCL's banner, are kept off it)."""
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ, MBLS_BENCH_SHARE_GPU="1")
    p = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--items", "4096",
                        "--no-cpu-baseline", "--no-variants", "--full"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["bitmap_matches_expectation"] is True and len(d["ms_per_step_per_rank"]) == 2 and "share_gpu_test" in d
    # what makes a SCALE line check itself: the process group's own rank count against n_gpus and the time of the one collective, timed alone
    c = d["collective"]
    assert c["group_world_size"] == 2 and c["group_rank_count_matches_n_gpus"] is True and c["all_gather_ms_per_step"] > 0 and c["backend"] == "gloo"
    # one rank, with the in-process multi-device leg (it makes an RCCL communicator): still one line on stdout
    p = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--items", "4096", "--no-cpu-baseline", "--full"],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    d1 = json.loads(lines[0])
    assert len(lines) == 1 and d1["n_gpus"] == 1 and d1["collective"] is None
    assert d1["multi_legs_ok"] is True and all(l["ran"] and l["results_match"] for l in d1["multi_handle_leg"])
    k = d1["valu_issue"]["kernels"]["k_miller"]
    assert 0 < k["mac_frac"] < 1.0 and 0.5 < k["mac_share_of_valu"] < 0.8 and k["mac_peak"] > 0          # (4 096 items: not the kernels' operating point; the keys are what is checked)


def test_plain_bench_run_prints_the_headline_and_dumps_the_timed_outputs(tmp_path):
    """`bench.py` without --full: the headline line only (no leg beside the timed one), and --dump-outputs holds the verdicts and the bitmap of the last
    timed step as float32 -- every 16th item (i % 16 == 7) rejected, every other one accepted, as build_inputs constructs them"""
    import json
    import os
    import subprocess
    import sys
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--items", "4096",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["bitmap_matches_expectation"] is True
    assert d["unit"] == "fast_aggregate_verify/s" and d["higher_is_better"] is True and d["value"] > 0 and d["dtype"]
    assert not {"phase_ms", "variants", "other_configs", "valu_issue", "cpu_baseline", "multi_handle_leg"} & set(d)
    want = np.ones(4096, dtype=np.float32); want[7::16] = 0
    for name in ("results", "bitmap"):
        a = np.load(out / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, want), name


def test_bench_multi_device_leg_in_a_child_process():
    """the in-process multi-device legs over more than one device run in a child process with a time limit (bench.multi_leg_in_child): a hang or a crash
    there costs that leg, not the line. On this box: the child with two contexts on device 0 (host join), and what a child that cannot answer leaves behind."""
    import os
    import bench
    os.environ["MBLS_MULTI_LEG_DEVICES"] = "0,0"
    try:
        leg = bench.multi_leg_in_child(2, 2048, 4)
    finally:
        del os.environ["MBLS_MULTI_LEG_DEVICES"]
    assert leg.get("results_match") is True and leg["devices"] == [0, 0] and leg["items"] == 4096, leg
    assert leg["bitmap_gather"]["gathered_bitmap_matches"] is True
    gone = bench.multi_leg_in_child(2, 2048, 4, timeout_s=0.01)
    assert "error" in gone and "results_match" not in gone
