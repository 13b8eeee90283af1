"""milagro_bls::VerifyStream (include/milagro_bls.hpp): compiles and links against libmbls_hip.so on the CPU; on the GPU it runs the reference's test
shapes through the stream and checks every item against the scalar API (tests/cpp/test_stream.cpp)."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "test_stream.cpp")


def build_exe(tmp_path):
    from milagro_bls_amd import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    exe = str(tmp_path / "test_stream")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(helpers.ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lmbls_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_stream_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_cpp_stream_against_the_scalar_api(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ stream checks passed" in out.stdout
