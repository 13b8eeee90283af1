"""CommitteeTable::verify_multiple_aggregate_signatures_batches and its _locate form over SpanSet of include/milagro_bls.hpp: compiles and links against
libmbls_hip.so on the CPU; on the GPU a block's nine sets in four batches (one empty), one attestation with a wrong bit, give the bools and the generator state of
verify_multiple_aggregate_signatures_batches on the spelled-out keys and messages, and the bad set is located (tests/cpp/test_vm_batches_committee_span.cpp)."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "test_vm_batches_committee_span.cpp")


def build_exe(tmp_path):
    from milagro_bls_amd import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    exe = str(tmp_path / "test_vm_batches_committee_span")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(helpers.ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lmbls_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_vm_batches_committee_span_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_cpp_vm_batches_committee_span_four_batches_one_bad(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ verify_multiple batches committee span checks passed" in out.stdout
