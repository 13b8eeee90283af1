"""CommitteeTable::fast_aggregate_verify_spans of include/milagro_bls.hpp: compiles and links against libmbls_hip.so on the CPU; on the GPU five attestations over
spans of a four-committee table -- complement and direct segments mixed, a segment with nobody, the same committee twice, an empty span -- give the bools of
AggregateSignature::fast_aggregate_verify on the spelled-out members, a wrong bit is a rejection, and what names nothing throws (tests/cpp/test_committee_span.cpp)."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "test_committee_span.cpp")


def build_exe(tmp_path):
    from milagro_bls_amd import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    exe = str(tmp_path / "test_committee_span")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(helpers.ROOT, "include"), SRC, "-o", exe, "-L", libdir, "-lmbls_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_cpp_committee_span_compiles_and_links(tmp_path):
    assert os.path.exists(build_exe(tmp_path))


@pytest.mark.gpu
def test_cpp_committee_span_five_attestations_one_bad(tmp_path):
    out = subprocess.run([build_exe(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all C++ committee span checks passed" in out.stdout
