"""AggregateSignature::verify_multiple_aggregate_signatures_shared_msgs_locate of include/milagro_bls.hpp: compiles and links against libmbls_hip.so on the CPU;
on the GPU nine sets over three messages with one bad set give false and exactly that set false, and the generator ends where the shared-message method leaves
it (tests/cpp/test_vm_shared_locate.cpp)."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "test_vm_shared_locate.cpp")


def build_exe(tmp_path):
    from milagro_bls_amd import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    exe = str(tmp_path / "test_vm_shared_locate")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(helpers.ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lmbls_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_vm_shared_locate_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_cpp_vm_shared_locate_one_bad_set(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ shared-message locate checks passed" in out.stdout
