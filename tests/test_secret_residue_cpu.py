"""The residue probe (include/mbls.h, mbls_ctx_residue_regions / mbls_ctx_residue_read) must see EVERY device allocation a context owns: the tests of
tests/test_gpu_secret_residue.py can only hold the secret-key entries to what the probe lists. Here, without a GPU: struct mbls_ctx is parsed out of
csrc/mbls_kernels.hip, every member that is a device pointer (and the staging array, and every list of objects with device memory of their own) must be
named by the probe's region table or stand on the short exemption list below with its reason -- a new `d_...` member without a table line fails here."""
import os
import re

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "milagro_bls_amd", "csrc", "mbls_kernels.hip")

# member of struct mbls_ctx -> why the probe does not list it
EXEMPT = {
    "coop": "coop[]: host-side descriptors (pointers into d_coop, which is listed), no allocation of their own",
    "tables": "key tables are objects of their own (mbls_keytable); no secret-key entry touches them",
    "msgtables": "message tables are objects of their own (mbls_msgtable); no secret-key entry touches them",
    "committees": "committee tables are objects of their own (mbls_committees); no secret-key entry touches them",
}
# what a signing or sk -> pk call writes: never to be exempted, whatever the reason
NEVER_EXEMPT = ("d_w", "d_status", "d_scalar", "d_skidx", "d_sksel", "stage")


def struct_body(txt, name="mbls_ctx"):
    m = re.search(r"^struct %s \{\n(.*?)^\};" % name, txt, flags=re.S | re.M)
    assert m, "struct %s not found" % name
    return m.group(1)


def device_members(body):
    """the members of the struct that own (or describe) device memory: every pointer to bytes / words, the staging array, arrays of descriptor structs and
    vectors of objects"""
    body = re.sub(r"//[^\n]*", "", body)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    # struct { void* p; size_t cap; } stage[MBLS_N_STAGE]: one member, not a pointer called p
    for m in re.finditer(r"struct\s*\{[^}]*\*[^}]*\}\s*(\w+)\s*\[", body):
        out.append(m.group(1))
    body = re.sub(r"struct\s*\{[^}]*\}\s*\w+\s*\[[^\]]*\]\s*(=\s*\{\})?\s*;", "", body)
    for m in re.finditer(r"\b(?:u?int(?:8|16|32|64)_t|void|char|float|uint4)\s*\*+\s*(\w+)", body):
        out.append(m.group(1))
    for m in re.finditer(r"std::vector<[^>]*\*\s*>\s*(\w+)", body):
        out.append(m.group(1))
    for m in re.finditer(r"\bcoop_prog\s+(\w+)\s*\[", body):
        out.append(m.group(1))
    return out


def table_members(txt):
    """the members the probe's region table names: RESIDUE_REGION(member, bytes) lines of residue_table, and the staging array its loop walks"""
    m = re.search(r"static void residue_table\(.*?^\}", txt, flags=re.S | re.M)
    assert m, "residue_table not found"
    names = re.findall(r"RESIDUE_REGION\((\w+),", m.group(0))
    assert len(names) == len(set(names))
    if re.search(r"c->stage\[i\]\.p", m.group(0)):
        names.append("stage")
    return names


def uncovered(body, table):
    return [x for x in device_members(body) if x not in table and x not in EXEMPT]


def test_every_device_allocation_of_the_context_is_a_region_of_the_probe():
    txt = open(SRC).read()
    body, table = struct_body(txt), table_members(txt)
    members = device_members(body)
    # the parse found what the struct is known to hold (a regex that went blind would pass everything)
    for must in ("d_w", "d_status", "d_results", "d_scalar", "d_gtab", "d_skidx", "d_sksel", "d_keys_xy", "d_key_flags", "d_htab", "d_hflag", "d_hst", "d_hgrp", "d_vmap",
                 "d_cmt_list", "d_cmt_cnt", "d_cms_list", "d_cms_rec", "d_cms_park", "d_coop", "stage", "coop", "tables", "msgtables", "committees"):
        assert must in members, must
    assert "p" not in members and len(members) == len(set(members))
    assert not uncovered(body, table), "struct mbls_ctx members without a region of the residue probe: %s" % uncovered(body, table)
    # nothing stale either way: the table names members only, the exemptions name members only, and none of them is listed as well
    assert set(table) <= set(members), set(table) - set(members)
    assert set(EXEMPT) <= set(members) and not set(EXEMPT) & set(table)
    for name, why in EXEMPT.items():
        assert len(why) > 20 and "\n" not in why, name


def test_what_the_secret_key_entries_write_is_never_exempt():
    table = table_members(open(SRC).read())
    for name in NEVER_EXEMPT:
        assert name not in EXEMPT and name in table, name


@pytest.mark.parametrize("name,line", [("d_new", "    uint32_t* d_new = nullptr;              // a new scratch\n"),
                                       ("d_other", "    uint8_t* d_other = nullptr; uint64_t other_cap = 0;\n"),
                                       ("d_wide", "    uint64_t* d_wide = nullptr;\n"),
                                       ("stage2", "    struct { void* p; size_t cap; } stage2[4] = {};\n"),
                                       ("newtables", "    std::vector<struct mbls_newtable*> newtables;\n")])
def test_a_new_device_pointer_without_a_region_fails(name, line):
    """the check itself: a member added to the struct and forgotten in the table is reported by name"""
    txt = open(SRC).read()
    body, table = struct_body(txt), table_members(txt)
    assert uncovered(body + line, table) == [name]
    assert uncovered(body + line, table + [name]) == []


def test_the_probe_only_reads():
    """the two entries launch no kernel and write no device memory"""
    txt = open(SRC).read()
    for fn in ("mbls_ctx_residue_regions", "mbls_ctx_residue_read"):
        m = re.search(r'extern "C" int %s\(.*?^\}' % fn, txt, flags=re.S | re.M)
        assert m, fn
        code = m.group(0)
        assert "hipLaunchKernelGGL" not in code and "coop_run" not in code and "hipMemset" not in code and "HostToDevice" not in code and "hipMalloc" not in code
    read = re.search(r'extern "C" int mbls_ctx_residue_read\(.*?^\}', txt, flags=re.S | re.M).group(0)
    assert "mbls_lock" in read and read.index("hipDeviceSynchronize") < read.index("hipMemcpy(")
