"""AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs of include/milagro_bls.hpp: compiles and links against libmbls_hip.so on the CPU; on the
GPU eight sets over three messages give the bool of verify_multiple_aggregate_signatures and draw as many bytes (tests/cpp/test_vm_shared_msgs.cpp)."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "test_vm_shared_msgs.cpp")


def build_exe(tmp_path):
    from milagro_bls_amd import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    exe = str(tmp_path / "test_vm_shared_msgs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(helpers.ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lmbls_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_vm_shared_msgs_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_cpp_vm_shared_msgs_same_bool_same_draws(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ shared message verify_multiple checks passed" in out.stdout
