"""fast_aggregate_verify_batch_shared_msgs of include/milagro_bls.hpp: compiles and links against libmbls_hip.so on the CPU; on the GPU six items over a list of
three messages, one with a wrong index, give the bools of one fast_aggregate_verify per item (tests/cpp/test_shared_msgs.cpp)."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "test_shared_msgs.cpp")


def build_exe(tmp_path):
    from milagro_bls_amd import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    exe = str(tmp_path / "test_shared_msgs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(helpers.ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lmbls_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_shared_msgs_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_cpp_shared_msgs_three_messages_one_wrong_index(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ shared message list checks passed" in out.stdout
