"""The generated digit-form leaves and passes ON THE GPU at the inputs their own generator admits: the cases of tests/dform_cases.py through the raw-register
probe kernel (mbls_dform_probe: one body per lane, raw int32 registers in, raw registers out). Every stored register must equal what tools/asm_sim.py computes
for the same instruction list -- integers and correctly rounded f32 operations, so there is no tolerance -- and the big-integer checks of the CPU test are applied
to the GPU's registers on their own, so that an interpreter error cannot excuse the kernel. Different case classes sit in neighbouring lanes of one wave (carries
are per-lane bits of a 64-bit mask on the hardware) and no launch fills its last wave."""
import pytest

import dform_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mb():
    from milagro_bls_amd import batch, _native
    _native.default_context()          # raises if the HIP library or the GPU is missing: no fallback
    return batch


def run_probe(mb, name, cs):
    """one launch: lane i runs case i; returns the stored registers per lane"""
    op, n = dc.OP[name], len(cs)
    nin, nout = mb.dform_probe_shape(op)
    assert (nin, nout) == (len(dc.OPS[op][1]), len(dc.OPS[op][2])), "the library was built from another probe list"
    flat = [0] * (nin * n)
    for i, c in enumerate(cs):
        flat[i::n] = c.words                      # word-major: word w of lane i at w * n + i
    out = mb.dform_probe(op, flat, n)
    return [out[i::n] for i in range(n)]


@pytest.mark.parametrize("name", list(dc.OP))
def test_probe_registers_equal_the_interpreter_and_the_big_integer_model(mb, name):
    cs = dc.cases(name)
    assert len(cs) % 64 != 0 and len(cs) > 64
    got = run_probe(mb, name, cs)
    want = dc.simulated(name)
    bad = [(i, cs[i]) for i in range(len(cs)) if got[i] != want[i]]
    if bad:
        i, c = bad[0]
        diff = [(dc.OPS[dc.OP[name]][2][w], hex(got[i][w]), hex(want[i][w])) for w in range(len(want[i])) if got[i][w] != want[i][w]]
        pytest.fail("%d of %d lanes differ from the interpreter; first: lane %d %r: (register, GPU, interpreter) %s" % (len(bad), len(cs), i, c, diff[:6]))
    for c, words in zip(cs, got):
        dc.check(c, words)


def test_probe_rejects_what_it_cannot_run(mb):
    with pytest.raises(ValueError):
        mb.dform_probe_shape(len(dc.OPS))
    with pytest.raises(ValueError):
        mb.dform_probe(0, [0] * 5, 1)
    assert mb.dform_probe(dc.OP["norm"], [], 0) == []
