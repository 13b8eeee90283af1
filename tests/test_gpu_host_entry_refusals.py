"""What the per-item verification entries refuse, and with which words: mbls_fast_aggregate_verify_batch / mbls_verify_batch / their `_indexed` forms, each with
per-item messages, a shared list (`_shared_msgs`) and a resident table (`_msgtable`), as host entries and as `_device` entries -- eighteen functions. Every call
below but the valid ones is refused before a kernel runs; the test pins the return code, the exact text of mbls_last_error, which refusal wins where two apply,
that the outputs are left alone, and that a valid call of the same entry succeeds right after (nothing of the refused call is left in flight). n = 4, k = 2."""
import ctypes as C
import random

import pytest

import shared_msgs_cases as smc

pytestmark = pytest.mark.gpu

P = "invalid argument: "
NULL_BUFFER = P + "null buffer"
NULL_KEYS = P + "null key buffer"
PK_FORMAT = P + "pk_format"
KEY_OFFSETS = P + "offsets must be non-decreasing"
MSG_OFFSETS = P + "msg_offsets must be non-decreasing, messages below 2^32 bytes"
NO_MESSAGE = P + "msg_idx names no message of the list"
NO_ENTRY = P + "msg_idx names no entry of the message table"
INDICES_32 = P + "message indices are 32-bit"
KEY_TABLE_CTX = P + "key table belongs to another context"
MSG_TABLE_CTX = P + "message table belongs to another context"
UNCHANGED = None          # the call returns MBLS_ERR_ARGUMENT and writes no text: mbls_last_error still gives the previous one

N_ITEMS, N_MSGS = 4, 5
IDX = [3, 0, 4, 3]
# key source: "fav" = wire keys, k per item (+ offsets); "verify" = one wire key per item; "table" = key-table indices. message source: "item", "list", "table".
ENTRIES = [(keys, msgs, device) for device in (False, True) for msgs in ("item", "list", "table") for keys in ("fav", "verify", "table")]


def entry_name(keys, msgs, device):
    return ("mbls_" + ("verify_batch" if keys == "verify" else "fast_aggregate_verify_batch") + ("_indexed" if keys == "table" else "") +
            {"item": "", "list": "_shared_msgs", "table": "_msgtable"}[msgs] + ("_device" if device else ""))


class World:
    def __init__(self):
        from milagro_bls_amd import _native as N
        self.N = N
        self.ctx = N.default_context()
        self.other = N.Context(0)
        rnd = random.Random(77)
        msgs = [rnd.randbytes(32) for _ in range(N_MSGS)]
        self.cs = smc.build(N_ITEMS, 2, msgs, IDX, seed=771, negatives=False)
        self.cv = smc.build(N_ITEMS, 1, msgs, IDX, seed=772, negatives=False)
        assert smc.oracle(self.cs) == self.cs.expect == [True] * N_ITEMS
        self.keytab = N.KeyTable(self.ctx, capacity_hint=8)
        assert self.keytab.append(self.cs.pks, 8, pk_format=1, validate=False)[0] == 0
        self.msgtab = N.MsgTable(self.ctx, capacity_hint=8)
        assert self.msgtab.append(b"".join(msgs), N_MSGS, msg_len=32) == 0
        self.foreign_keytab = N.KeyTable(self.other, capacity_hint=8)
        self.foreign_msgtab = N.MsgTable(self.other, capacity_hint=8)

    def close(self):
        for t in (self.keytab, self.msgtab, self.foreign_keytab, self.foreign_msgtab):
            t.close()
        self.other.close()

    def call(self, keys, msgs, device, **over):
        """the entry with valid arguments but for `over` -> (return code, results as the call left them)"""
        import torch
        N = self.N
        cs = self.cv if keys == "verify" else self.cs
        keep = []

        def put(v, ctype=None):
            """bytes, or a list of integers of the given ctypes type, as the entry takes them: a host array or a device pointer"""
            if v is None:
                return None
            host = N.cbuf(v) if ctype is None else (ctype * len(v))(*v)
            if device:
                host = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to("cuda:0")
            keep.append(host)
            return host.data_ptr() if device else host

        v = dict(keytab=self.keytab.handle, msgtab=self.msgtab.handle, sigs=cs.sigs, msgs=cs.list_bytes if msgs == "list" else cs.spelled_bytes, msg_len=32,
                 moff=None, n_msgs=N_MSGS, msg_idx=IDX, pks=cs.pks, fmt=1, key_idx=list(range(8)), off=None, res=[9] * N_ITEMS)
        v.update(over)
        a = [self.ctx.handle]
        if keys == "table":
            a.append(v["keytab"])
        a.append(put(v["sigs"]))
        if msgs == "table":
            a += [v["msgtab"], put(v["msg_idx"], C.c_uint32)]
        else:
            a += [put(v["msgs"]), v["msg_len"], put(v["moff"], C.c_uint64)]
            if msgs == "list":
                a += [v["n_msgs"], put(v["msg_idx"], C.c_uint32)]
        if keys == "table":
            a += [put(v["key_idx"], C.c_uint32), put(v["off"], C.c_uint32), N_ITEMS, cs.k]
        elif keys == "fav":
            a += [put(v["pks"]), v["fmt"], put(v["off"], C.c_uint32), N_ITEMS, cs.k]
        else:
            a += [put(v["pks"]), v["fmt"], N_ITEMS]
        a.append(put(v["res"], C.c_uint8))
        res = keep[-1] if v["res"] is not None else None
        if device:
            a += [put([0], C.c_uint64), put([0x7fffffff] * N_ITEMS, C.c_uint32), None]
        else:
            a.append(put([0x7fffffff] * N_ITEMS, C.c_uint32))
        rc = getattr(N.lib(), entry_name(keys, msgs, device))(*a)
        if device:
            torch.cuda.synchronize()
        return rc, None if res is None else (res.cpu().tolist() if device else list(res))

    def valid(self, keys, msgs, device):
        rc, res = self.call(keys, msgs, device)
        assert rc == self.N.OK, self.ctx.last_error()
        assert res == [1] * N_ITEMS


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def refusals(w, keys, msgs, device):
    """(what is wrong, the arguments that differ from the valid call's, the text mbls_last_error gives) for one entry"""
    key_arg = "key_idx" if keys == "table" else "pks"
    out = [("null signature buffer", dict(sigs=None), NULL_BUFFER),
           ("null key buffer", {key_arg: None}, NULL_BUFFER if device else NULL_KEYS),
           ("null result buffer", dict(res=None), NULL_BUFFER)]
    if keys != "table":
        out.append(("bad pk_format", dict(fmt=7), UNCHANGED if device else PK_FORMAT))
    if msgs == "list":
        out.append(("n_msgs above 2^32 - 1", dict(n_msgs=2 ** 32), INDICES_32))
        out.append(("n_msgs above 2^32 - 1 and a null signature buffer", dict(n_msgs=2 ** 32, sigs=None), INDICES_32))
    if keys == "table":
        out.append(("key table of another context", dict(keytab=w.foreign_keytab.handle), KEY_TABLE_CTX))
    if msgs == "table":
        out.append(("message table of another context", dict(msgtab=w.foreign_msgtab.handle), MSG_TABLE_CTX))
        if keys == "table":      # both tables foreign: the host entries look at the message table first, the device entries at the key table
            out.append(("both tables of another context", dict(keytab=w.foreign_keytab.handle, msgtab=w.foreign_msgtab.handle), KEY_TABLE_CTX if device else MSG_TABLE_CTX))
        elif device:             # the format is looked at before the table's owner
            out.append(("bad pk_format and a message table of another context", dict(fmt=7, msgtab=w.foreign_msgtab.handle), UNCHANGED))
    if device:                   # tables in device memory are not read by the host: their faults are per-item status bits, not refusals
        return out
    down = [0, 2, 1, 6, 8]
    if keys != "verify":
        out.append(("decreasing key offsets", dict(off=down), KEY_OFFSETS))
        if keys == "fav":
            out.append(("bad pk_format and decreasing key offsets", dict(fmt=7, off=down), PK_FORMAT))
        out.append(("decreasing key offsets and a null key buffer", {"off": down, key_arg: None}, KEY_OFFSETS))
    if msgs != "table":
        count = N_MSGS if msgs == "list" else N_ITEMS
        back = [0, 32, 24, 96, 128, 160][:count + 1]
        wide = [0] + [2 ** 32] * count
        out.append(("decreasing message offsets", dict(moff=back), MSG_OFFSETS))
        out.append(("a message offset step of 2^32", dict(moff=wide), MSG_OFFSETS))
        out.append(("decreasing message offsets and bad pk_format", dict(moff=back, fmt=7) if keys != "table" else dict(moff=back, off=down), MSG_OFFSETS))
    if msgs != "item":
        text = NO_MESSAGE if msgs == "list" else NO_ENTRY
        for bad in (N_MSGS, 0xFFFFFFFF):
            out.append(("message index %#x" % bad, dict(msg_idx=[3, 0, bad, 3]), text))
        out.append(("a message index that names nothing and bad pk_format", dict(msg_idx=[3, 0, N_MSGS, 3], **({"fmt": 7} if keys != "table" else {"off": down})), text))
        if msgs == "list":
            out.append(("decreasing message offsets and a message index that names nothing", dict(moff=[0, 32, 24, 96, 128, 160], msg_idx=[3, 0, N_MSGS, 3]), MSG_OFFSETS))
    return out


@pytest.mark.parametrize("keys,msgs,device", ENTRIES, ids=[entry_name(*e) for e in ENTRIES])
def test_refusals_of_one_entry(world, keys, msgs, device):
    N = world.N
    world.valid(keys, msgs, device)
    for what, over, text in refusals(world, keys, msgs, device):
        before = world.ctx.last_error()
        rc, res = world.call(keys, msgs, device, **over)
        assert rc == N.ERR_ARGUMENT, what
        assert world.ctx.last_error() == (before if text is UNCHANGED else text), what
        assert res is None or res == [9] * N_ITEMS, what
        world.valid(keys, msgs, device)
