"""MessageTable, fast_aggregate_verify_batch_msgtable and the VerifyStream over a table of include/milagro_bls.hpp: compiles and links against libmbls_hip.so on
the CPU; on the GPU six items over a table of three messages, one with a wrong index, give the bools of one fast_aggregate_verify per item, directly and through a
stream (tests/cpp/test_msgtable.cpp)."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "test_msgtable.cpp")


def build_exe(tmp_path):
    from milagro_bls_amd import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    exe = str(tmp_path / "test_msgtable")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(helpers.ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lmbls_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_msgtable_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_cpp_msgtable_three_messages_one_wrong_index_direct_and_streamed(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ message table checks passed" in out.stdout
