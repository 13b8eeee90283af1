"""VerifyMultipleStream of include/milagro_bls.hpp (a verify_multiple stream over a CommitteeTable and a MessageTable): compiles and links against libmbls_hip.so on
the CPU; on the GPU three gossip batches -- aggregates mixed with single-key sets, single-key sets only, one wrong participation bit -- share one round and give the
bools and per-set answers of CommitteeTable::verify_multiple_aggregate_signatures_locate on each batch alone, the generator left where that method leaves it, and
what does not fit is refused (tests/cpp/test_stream_vm.cpp)."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "test_stream_vm.cpp")


def build_exe(tmp_path):
    from milagro_bls_amd import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    exe = str(tmp_path / "test_stream_vm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(helpers.ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lmbls_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_stream_vm_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_cpp_stream_vm_three_batches_in_one_round(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ verify_multiple stream checks passed" in out.stdout
