"""VerifyStream over a CommitteeTable and a MessageTable of include/milagro_bls.hpp: compiles and links against libmbls_hip.so on the CPU; on the GPU one mixed call --
complement and direct routes, nobody, a delimiter left in -- gives the bools of AggregateSignature::fast_aggregate_verify on the spelled-out members, a wrong bit and
what names nothing are rejections, shorter fields travel in a call of their own, and the table cannot outgrow the stride (tests/cpp/test_stream_committee.cpp)."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "test_stream_committee.cpp")


def build_exe(tmp_path):
    from milagro_bls_amd import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    exe = str(tmp_path / "test_stream_committee")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(helpers.ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lmbls_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_stream_committee_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_cpp_stream_committee_one_mixed_call(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ committee stream checks passed" in out.stdout
