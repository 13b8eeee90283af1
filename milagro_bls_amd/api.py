"""Host-side mirror of the reference's public API (reference src/lib.rs:17-22) over the C ABI of
libmbls_hip.so: same type and method names, argument meaning and error behaviour, so that the parity tests
read like the reference's own tests. Every numeric operation runs in the HIP kernels (no CPU arithmetic
here apart from SecretKey's HKDF key derivation, which the reference also does on the host, src/keys.rs:45-77).

    reference                                   here
    ---------                                   ----
    SecretKey / PublicKey / Keypair             src/keys.rs:28-204
    Signature                                   src/signature.rs:9-51
    AggregatePublicKey / AggregateSignature     src/aggregates.rs:17-334
    AmclError                                   amcl::errors::AmclError (src/amcl_utils.rs:11)
"""
import ctypes as C
import hashlib
import hmac
import os

from . import _native as N

G1_BYTES = 48            # reference src/lib.rs:20
G2_BYTES = 96
SECRET_KEY_BYTES = 32
CURVE_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
KEY_SALT = b"BLS-SIG-KEYGEN-SALT-"   # reference src/keys.rs:24
L = 48                                # reference src/keys.rs:26
_G2_INFINITY = bytes([0xC0]) + bytes(95)


class AmclError(Exception):
    """Mirror of the AmclError variants the reference uses."""
    InvalidG1Size = N.ERR_INVALID_G1_SIZE
    InvalidG2Size = N.ERR_INVALID_G2_SIZE
    InvalidPoint = N.ERR_INVALID_POINT
    AggregateEmptyPoints = N.ERR_AGGREGATE_EMPTY_POINTS
    InvalidSecretKeySize = N.ERR_INVALID_SECRET_KEY_SIZE
    InvalidSecretKeyRange = N.ERR_INVALID_SECRET_KEY_RANGE
    _NAMES = {1: "InvalidG1Size", 2: "InvalidG2Size", 3: "InvalidPoint", 4: "AggregateEmptyPoints",
              5: "InvalidSecretKeySize", 6: "InvalidSecretKeyRange"}

    def __init__(self, code):
        super().__init__(self._NAMES.get(code, "DeviceError(%d)" % code))
        self.code = code

    def __eq__(self, other):
        return isinstance(other, AmclError) and other.code == self.code

    def __hash__(self):
        return hash(self.code)


def hkdf_extract(salt, ikm):
    """HKDF-Extract with SHA-256 (RFC 5869 section 2.2; amcl HASH256::hkdf_extract, reference src/keys.rs:62)"""
    return hmac.new(bytes(salt) if salt else bytes(32), bytes(ikm), hashlib.sha256).digest()


def hkdf_expand(prk, info, length):
    """HKDF-Expand with SHA-256 (RFC 5869 section 2.3; amcl HASH256::hkdf_extend, reference src/keys.rs:67)"""
    okm, t, i = b"", b"", 1
    while len(okm) < length:
        t = hmac.new(prk, t + bytes(info) + bytes([i]), hashlib.sha256).digest()
        okm += t
        i += 1
    return okm[:length]


def _ctx():
    return N.default_context()


def _raise(rc):
    if rc != N.OK:
        if rc >= N.ERR_DEVICE:
            raise N.MblsError(rc, _ctx().last_error())
        raise AmclError(rc)


class SecretKey:
    """reference src/keys.rs:28-113. Host-only object; the scalar is sent to the GPU only for signing."""

    def __init__(self, x):
        self._x = int(x)

    @classmethod
    def random(cls, rng=None):
        ikm = os.urandom(32) if rng is None else bytes(rng.getrandbits(8) for _ in range(32))
        return cls.key_generate(ikm, b"")

    @classmethod
    def key_generate(cls, ikm, key_info=b""):
        """KeyGenerate, reference src/keys.rs:45-77 (HKDF-SHA256 with the salt-rehash loop)."""
        if len(ikm) < 32:
            raise AmclError(AmclError.InvalidSecretKeySize)
        sk, salt = 0, KEY_SALT
        while sk == 0:
            salt = hashlib.sha256(salt).digest()
            prk = hkdf_extract(salt, bytes(ikm) + b"\x00")
            okm = hkdf_expand(prk, bytes(key_info) + bytes([0, L]), L)
            sk = int.from_bytes(okm, "big") % CURVE_ORDER
        return cls(sk)

    @classmethod
    def from_bytes(cls, data):
        """reference src/keys.rs:80-82, error cases pinned by tests at src/keys.rs:285-297."""
        data = bytes(data)
        if len(data) != SECRET_KEY_BYTES:
            raise AmclError(AmclError.InvalidSecretKeySize)
        x = int.from_bytes(data, "big")
        if x == 0 or x >= CURVE_ORDER:
            raise AmclError(AmclError.InvalidSecretKeyRange)
        return cls(x)

    def as_bytes(self):
        return self._x.to_bytes(SECRET_KEY_BYTES, "big")

    def as_raw(self):
        return self._x

    def __eq__(self, other):
        return isinstance(other, SecretKey) and self.as_bytes() == other.as_bytes()


class PublicKey:
    """reference src/keys.rs:116-187. `point` is the 96-byte uncompressed form (amcl's layout is private)."""

    def __init__(self, point):
        self.point = bytes(point)

    @classmethod
    def from_secret_key(cls, sk):
        out = N.outbuf(96)
        _raise(N.lib().mbls_pk_from_secret_key(_ctx().handle, N.cbuf(sk.as_bytes()), 32, out))
        return cls(bytes(out))

    @classmethod
    def from_bytes(cls, data):
        out = N.outbuf(96)
        _raise(N.lib().mbls_pk_from_bytes(_ctx().handle, N.cbuf(data), len(data), out))
        return cls(bytes(out))

    @classmethod
    def from_bytes_unchecked(cls, data):
        out = N.outbuf(96)
        _raise(N.lib().mbls_pk_from_bytes_unchecked(_ctx().handle, N.cbuf(data), len(data), out))
        return cls(bytes(out))

    @classmethod
    def from_uncompressed_bytes(cls, data):
        out = N.outbuf(96)
        _raise(N.lib().mbls_pk_from_uncompressed_bytes(_ctx().handle, N.cbuf(data), len(data), out))
        return cls(bytes(out))

    def as_bytes(self):
        out = N.outbuf(48)
        _raise(N.lib().mbls_pk_as_bytes(_ctx().handle, N.cbuf(self.point), out))
        return bytes(out)

    def as_uncompressed_bytes(self):
        return self.point

    def key_validate(self):
        return bool(N.lib().mbls_pk_key_validate(_ctx().handle, N.cbuf(self.point)))

    def is_infinity(self):
        return self.point[0] == 0x40

    def __eq__(self, other):
        return isinstance(other, PublicKey) and self.point == other.point


class Keypair:
    """reference src/keys.rs:189-204."""

    def __init__(self, sk, pk):
        self.sk, self.pk = sk, pk

    @classmethod
    def random(cls, rng=None):
        sk = SecretKey.random(rng)
        return cls(sk, PublicKey.from_secret_key(sk))


class Signature:
    """reference src/signature.rs:9-51. `point` is the 96-byte compressed form."""

    def __init__(self, point):
        self.point = bytes(point)

    @classmethod
    def new(cls, msg, sk):
        out = N.outbuf(96)
        _raise(N.lib().mbls_sign(_ctx().handle, N.cbuf(msg), len(msg), N.cbuf(sk.as_bytes()), 32, out))
        return cls(bytes(out))

    def verify(self, msg, pk):
        return bool(N.lib().mbls_verify(_ctx().handle, N.cbuf(self.point), N.cbuf(msg), len(msg), N.cbuf(pk.point)))

    @classmethod
    def from_bytes(cls, data):
        out = N.outbuf(96)
        _raise(N.lib().mbls_sig_from_bytes(_ctx().handle, N.cbuf(data), len(data), out))
        return cls(bytes(out))

    def as_bytes(self):
        return self.point

    def __eq__(self, other):
        return isinstance(other, Signature) and self.point == other.point


class AggregatePublicKey:
    """reference src/aggregates.rs:17-78."""

    def __init__(self, point):
        self.point = bytes(point)

    @classmethod
    def aggregate(cls, keys):
        if len(keys) == 0:
            raise AmclError(AmclError.AggregateEmptyPoints)
        out = N.outbuf(96)
        _raise(N.lib().mbls_aggregate_public_keys(_ctx().handle, N.cbuf(b"".join(k.point for k in keys)), len(keys), out))
        return cls(bytes(out))

    into_aggregate = aggregate

    @classmethod
    def from_public_key(cls, key):
        return cls(key.point)

    def add(self, public_key):
        out = N.outbuf(96)
        _raise(N.lib().mbls_aggregate_public_key_add(_ctx().handle, N.cbuf(self.point), N.cbuf(public_key.point), out))
        self.point = bytes(out)

    def add_aggregate(self, other):
        self.add(other)

    def is_infinity(self):
        return self.point[0] == 0x40

    def __eq__(self, other):
        return isinstance(other, AggregatePublicKey) and self.point == other.point



class SingleKey:
    """In a set of verify_multiple_aggregate_signatures_committee: the set is signed by ONE key, entry `index` of the key table the committees are bound to (a
    selection proof, an aggregator's signature, an unaggregated attestation)."""
    __slots__ = ("index",)

    def __init__(self, index):
        index = int(index)
        if not 0 <= index < N.VM_SET_SINGLE_KEY:
            raise ValueError("a key index has 31 bits")
        self.index = index


def _reference_draw(rng, failed):
    """The scalar source of the verify_multiple methods: src/aggregates.rs:280-287 -- 8 random bytes, big-endian i64, absolute value, retry on zero --, for the sets
    the reference's loop reaches a draw for. An exception must not unwind through the C frames: the batch fails (zero scalars) and the caller raises failed[0]."""
    def draw(_user, out, count):
        try:
            for i in range(count):
                r = 0
                while r == 0:
                    v = int.from_bytes(bytes(rng.getrandbits(8) for _ in range(8)), "big", signed=True)
                    r = abs(v) & 0xFFFFFFFFFFFFFFFF
                out[i] = r
        except BaseException as e:
            failed.append(e)
            for i in range(count):
                out[i] = 0
    return draw


class AggregateSignature:
    """reference src/aggregates.rs:83-334."""

    def __init__(self, point=_G2_INFINITY):
        self.point = bytes(point)

    @classmethod
    def new(cls):
        return cls(_G2_INFINITY)

    @classmethod
    def aggregate(cls, signatures):
        """reference src/aggregates.rs:100-106: one batched launch (segmented G2 sum) instead of one addition per call"""
        signatures = list(signatures)
        if not signatures:
            return cls.new()
        out, errs = N.outbuf(96), N.outbuf(1)
        _raise(N.lib().mbls_aggregate_signatures_batch(_ctx().handle, N.cbuf(b"".join(s.point for s in signatures)), None, 1, len(signatures), out, errs))
        _raise(bytes(errs)[0])
        return cls(bytes(out))

    @classmethod
    def from_signature(cls, signature):
        return cls(signature.point)

    def clone(self):
        return AggregateSignature(self.point)

    def add(self, signature):
        out = N.outbuf(96)
        _raise(N.lib().mbls_aggregate_signature_add(_ctx().handle, N.cbuf(self.point), N.cbuf(signature.point), out))
        self.point = bytes(out)

    def add_aggregate(self, other):
        self.add(other)

    def aggregate_verify(self, msgs, public_keys):
        lens = (C.c_size_t * max(1, len(msgs)))(*[len(m) for m in msgs])
        return bool(N.lib().mbls_aggregate_verify(_ctx().handle, N.cbuf(self.point), N.cbuf(b"".join(msgs)), lens, len(msgs),
                                                   N.cbuf(b"".join(k.point for k in public_keys)), len(public_keys)))

    def fast_aggregate_verify(self, msg, public_keys):
        return bool(N.lib().mbls_fast_aggregate_verify(_ctx().handle, N.cbuf(self.point), N.cbuf(msg), len(msg),
                                                        N.cbuf(b"".join(k.point for k in public_keys)), len(public_keys)))

    def fast_aggregate_verify_pre_aggregated(self, msg, aggregate_public_key):
        return bool(N.lib().mbls_fast_aggregate_verify_pre_aggregated(_ctx().handle, N.cbuf(self.point), N.cbuf(msg), len(msg),
                                                                       N.cbuf(aggregate_public_key.point)))

    @staticmethod
    def verify_multiple_aggregate_signatures(rng, signature_sets, devices=None):
        """reference src/aggregates.rs:261-316. devices (optional, not in the reference): a _native.MultiContext -- the sets are then cut into one shard per device
        (mbls_multi_verify_multiple_aggregate_signatures_rng: same bool, same draws). `rng` must offer getrandbits (random.Random); the blinding scalars
        are drawn exactly as at :280-287: 8 random bytes, big-endian i64, absolute value, retry on zero -- and IN THE REFERENCE'S ORDER: its loop
        tests set i's signature for the subgroup (:272-275) before it draws rand[i], and returns at the first signature outside G2, so a rejected
        batch leaves the caller's generator where the reference would (mbls_verify_multiple_aggregate_signatures_rng tests the signatures first and
        asks for the scalars of the sets in front of the first bad one only). Messages may have any lengths (`&[u8]` per set in the reference): one buffer + an offset table."""
        sets = list(signature_sets)
        if not sets:
            return bool(N.lib().mbls_verify_multiple_aggregate_signatures(_ctx().handle, None, None, None, 0, None, None, 0))
        failed = []
        draw = _reference_draw(rng, failed)
        offs = [0]
        for s in sets:
            offs.append(offs[-1] + len(s[2]))
        moff = (C.c_uint64 * len(offs))(*offs)
        cb = N.SCALAR_SOURCE(draw)
        entry, handle = ((N.lib().mbls_verify_multiple_aggregate_signatures_rng, _ctx().handle) if devices is None else
                         (N.lib().mbls_multi_verify_multiple_aggregate_signatures_rng, devices.handle))
        ok = bool(entry(handle, N.cbuf(b"".join(s[0].point for s in sets)), N.cbuf(b"".join(s[1].point for s in sets)),
                        N.cbuf(b"".join(bytes(s[2]) for s in sets)), 0, moff, len(sets), cb, None))
        if failed:
            raise failed[0]
        return ok

    @staticmethod
    def verify_multiple_aggregate_signatures_shared_msgs(rng, signature_sets):
        """Not in the reference: verify_multiple_aggregate_signatures(rng, signature_sets) -- the same (signature, aggregate_public_key, message) sets, the same
        bool, `rng` left in the same state -- for batches whose sets share messages (a slot's gossip: tens of thousands of sets over a few hundred signing
        roots). The messages are deduplicated here by their bytes, and ONE call (mbls_verify_multiple_shared_msgs_rng) hashes each distinct message once and,
        where it pays, walks one Miller loop per message instead of one per set. The scalars are drawn as there, in the reference's order."""
        return AggregateSignature._vm_shared(rng, signature_sets, False)

    @staticmethod
    def verify_multiple_aggregate_signatures_shared_msgs_locate(rng, signature_sets):
        """verify_multiple_aggregate_signatures_shared_msgs, and in the same call (mbls_verify_multiple_shared_msgs_locate_rng) which sets of a rejected call are
        the bad ones. Returns (bool, list[bool]). Every set of an accepted call reads True -- a passing batch is not examined set by set. A set of a rejected
        call reads what the one-set call with its scalar returns; a set at or behind the first signature outside G2 has no scalar (the reference never draws
        one) and reads False. The messages are deduplicated as there, and `rng` is left exactly where that method leaves it."""
        return AggregateSignature._vm_shared(rng, signature_sets, True)

    @staticmethod
    def _vm_shared(rng, signature_sets, locate):
        sets = list(signature_sets)
        if not sets:
            return (True, []) if locate else True
        failed = []
        draw = _reference_draw(rng, failed)
        index, listed, idx = {}, [], []
        for s in sets:
            m = bytes(s[2])
            if m not in index:
                index[m] = len(listed)
                listed.append(m)
            idx.append(index[m])
        offs = [0]
        for m in listed:
            offs.append(offs[-1] + len(m))
        moff = (C.c_uint64 * len(offs))(*offs)
        midx = (C.c_uint32 * len(idx))(*idx)
        cb = N.SCALAR_SOURCE(draw)
        res = N.outbuf(1)
        ctx = _ctx()
        S, A, M = N.cbuf(b"".join(s[0].point for s in sets)), N.cbuf(b"".join(s[1].point for s in sets)), N.cbuf(b"".join(listed))
        if locate:
            sres = N.outbuf(len(sets))
            rc = N.lib().mbls_verify_multiple_shared_msgs_locate_rng(ctx.handle, S, A, M, 0, moff, len(listed), midx, len(sets), res, sres, None, cb, None)
        else:
            rc = N.lib().mbls_verify_multiple_shared_msgs_rng(ctx.handle, S, A, M, 0, moff, len(listed), midx, len(sets), res, cb, None)
        ctx.check(rc)
        if failed:
            raise failed[0]
        if not locate:
            return bool(bytes(res)[0])
        return bool(bytes(res)[0]), [bool(x) for x in bytes(sres)[:len(sets)]]

    @staticmethod
    def verify_multiple_aggregate_signatures_msgtable(rng, signature_sets, table):
        """Not in the reference: verify_multiple_aggregate_signatures over sets (signature, aggregate_public_key, message_index) whose messages are entries of a
        resident message table (_native.MsgTable): the same bool as that method on the spelled-out messages and `rng` left in the same state, with nothing
        hashed in the call (mbls_verify_multiple_msgtable_rng). An index that names no entry of the table raises."""
        return AggregateSignature._vm_msgtable(rng, signature_sets, table, False)

    @staticmethod
    def verify_multiple_aggregate_signatures_msgtable_locate(rng, signature_sets, table):
        """verify_multiple_aggregate_signatures_msgtable, and in the same call (mbls_verify_multiple_msgtable_locate_rng) which sets of a rejected call are the bad
        ones. Returns (bool, list[bool]) with the semantics of verify_multiple_aggregate_signatures_shared_msgs_locate."""
        return AggregateSignature._vm_msgtable(rng, signature_sets, table, True)

    @staticmethod
    def _vm_msgtable(rng, signature_sets, table, locate):
        sets = list(signature_sets)
        if not sets:
            return (True, []) if locate else True
        failed = []
        cb = N.SCALAR_SOURCE(_reference_draw(rng, failed))
        midx = (C.c_uint32 * len(sets))(*[int(s[2]) for s in sets])
        res = N.outbuf(1)
        ctx = table.ctx
        S, A = N.cbuf(b"".join(s[0].point for s in sets)), N.cbuf(b"".join(s[1].point for s in sets))
        if locate:
            sres = N.outbuf(len(sets))
            rc = N.lib().mbls_verify_multiple_msgtable_locate_rng(ctx.handle, S, A, table.handle, midx, len(sets), res, sres, None, cb, None)
        else:
            rc = N.lib().mbls_verify_multiple_msgtable_rng(ctx.handle, S, A, table.handle, midx, len(sets), res, cb, None)
        ctx.check(rc)
        if failed:
            raise failed[0]
        if not locate:
            return bool(bytes(res)[0])
        return bool(bytes(res)[0]), [bool(x) for x in bytes(sres)[:len(sets)]]

    @staticmethod
    def verify_multiple_aggregate_signatures_committee(rng, signature_sets, committees, table):
        """Not in the reference: verify_multiple_aggregate_signatures over a gossip batch whose keys are resident (mbls_verify_multiple_committee_msgtable_rng). A set
        is (signature, committee_id, bits_bytes, message_index) -- the aggregate over the members of committee `committee_id` of `committees`
        (_native.CommitteeTable) whose bit is set, SSZ bit order, bits at or above the committee's size ignored -- or (signature, SingleKey(index), None,
        message_index): one key of the key table the committees are bound to. Messages are entries of `table` (_native.MsgTable). The same bool as
        verify_multiple_aggregate_signatures on the spelled-out aggregate keys and messages, `rng` left in the same state. A committee id, key index or message
        index that names nothing raises."""
        return AggregateSignature._vm_committee(rng, signature_sets, committees, table, False)

    @staticmethod
    def verify_multiple_aggregate_signatures_committee_locate(rng, signature_sets, committees, table):
        """verify_multiple_aggregate_signatures_committee, and in the same call (mbls_verify_multiple_committee_msgtable_locate_rng) which sets of a rejected call
        are the bad ones. Returns (bool, list[bool]) with the semantics of verify_multiple_aggregate_signatures_shared_msgs_locate."""
        return AggregateSignature._vm_committee(rng, signature_sets, committees, table, True)

    @staticmethod
    def _vm_committee(rng, signature_sets, committees, table, locate):
        sets = list(signature_sets)
        if not sets:
            return (True, []) if locate else True
        stride = max(4, (committees.max_members + 31) // 32 * 4)
        words, fields = [], []
        for s in sets:
            if isinstance(s[1], SingleKey):
                words.append(N.VM_SET_SINGLE_KEY | s[1].index)
                fields.append(bytes(stride))
            else:
                cid, field = int(s[1]), bytes(s[2])
                if not 0 <= cid < N.VM_SET_SINGLE_KEY:
                    raise ValueError("committee id out of range")
                if len(field) > stride and any(field[stride:]):
                    raise ValueError("a bitfield names members beyond the table's largest committee")
                words.append(cid)
                fields.append(field[:stride].ljust(stride, b"\0"))
        failed = []
        cb = N.SCALAR_SOURCE(_reference_draw(rng, failed))
        cidx = (C.c_uint32 * len(sets))(*words)
        midx = (C.c_uint32 * len(sets))(*[int(s[3]) for s in sets])
        res = N.outbuf(1)
        ctx = committees.ctx
        S, B = N.cbuf(b"".join(s[0].point for s in sets)), N.cbuf(b"".join(fields))
        if locate:
            sres = N.outbuf(len(sets))
            rc = N.lib().mbls_verify_multiple_committee_msgtable_locate_rng(ctx.handle, committees.handle, S, cidx, B, stride, table.handle, midx, len(sets), res, sres,
                                                                           None, cb, None)
        else:
            rc = N.lib().mbls_verify_multiple_committee_msgtable_rng(ctx.handle, committees.handle, S, cidx, B, stride, table.handle, midx, len(sets), res, cb, None)
        ctx.check(rc)
        if failed:
            raise failed[0]
        if not locate:
            return bool(bytes(res)[0])
        return bool(bytes(res)[0]), [bool(x) for x in bytes(sres)[:len(sets)]]

    @staticmethod
    def verify_multiple_aggregate_signatures_committee_span(rng, signature_sets, committees, table):
        """Not in the reference: verify_multiple_aggregate_signatures over a block's sets (mbls_verify_multiple_committee_span_msgtable_rng). A set is
        (signature, committee_ids, field_bytes, message_index) -- the aggregate over the selected members of the committees `committee_ids` (at most 64) of
        `committees` (_native.CommitteeTable), `field_bytes` ONE bitfield over their concatenated members (an Electra attestation's aggregation_bits; SSZ bit order,
        bits at or above the members' total ignored) -- or (signature, SingleKey(index), None, message_index). Messages are entries of `table` (_native.MsgTable).
        The same bool as verify_multiple_aggregate_signatures on the spelled-out aggregate keys and messages, `rng` left in the same state. A malformed set, a key
        index or a message index that names nothing raises."""
        return AggregateSignature._vm_committee_span(rng, signature_sets, committees, table, False)

    @staticmethod
    def verify_multiple_aggregate_signatures_committee_span_locate(rng, signature_sets, committees, table):
        """verify_multiple_aggregate_signatures_committee_span, and in the same call (mbls_verify_multiple_committee_span_msgtable_locate_rng) which sets of a
        rejected call are the bad ones. Returns (bool, list[bool]) with the semantics of verify_multiple_aggregate_signatures_shared_msgs_locate."""
        return AggregateSignature._vm_committee_span(rng, signature_sets, committees, table, True)

    @staticmethod
    def _vm_committee_span(rng, signature_sets, committees, table, locate):
        sets = list(signature_sets)
        if not sets:
            return (True, []) if locate else True
        id_lists, fields = [], []
        for s in sets:
            if isinstance(s[1], SingleKey):
                id_lists.append([N.VM_SET_SINGLE_KEY | s[1].index])
                fields.append(b"")
            else:
                ids = [int(x) for x in s[1]]
                if any(not 0 <= x < N.VM_SET_SINGLE_KEY for x in ids):
                    raise ValueError("committee id out of range")
                id_lists.append(ids)
                fields.append(bytes(s[2]))
        stride = max(4, (max(len(f) for f in fields) + 3) // 4 * 4)
        n = len(sets)
        ids = (C.c_uint32 * max(1, sum(map(len, id_lists))))(*[x for l in id_lists for x in l])
        off = (C.c_uint32 * (n + 1))(*([0] + [sum(map(len, id_lists[:i + 1])) for i in range(n)]))
        failed = []
        cb = N.SCALAR_SOURCE(_reference_draw(rng, failed))
        midx = (C.c_uint32 * n)(*[int(s[3]) for s in sets])
        res = N.outbuf(1)
        ctx = committees.ctx
        S, B = N.cbuf(b"".join(s[0].point for s in sets)), N.cbuf(b"".join(f.ljust(stride, b"\0") for f in fields))
        n_ids = sum(map(len, id_lists))
        if locate:
            sres = N.outbuf(n)
            rc = N.lib().mbls_verify_multiple_committee_span_msgtable_locate_rng(ctx.handle, committees.handle, S, ids, n_ids, off, B, stride, table.handle, midx, n, res,
                                                                                sres, None, cb, None)
        else:
            rc = N.lib().mbls_verify_multiple_committee_span_msgtable_rng(ctx.handle, committees.handle, S, ids, n_ids, off, B, stride, table.handle, midx, n, res, cb, None)
        ctx.check(rc)
        if failed:
            raise failed[0]
        if not locate:
            return bool(bytes(res)[0])
        return bool(bytes(res)[0]), [bool(x) for x in bytes(sres)[:n]]

    @staticmethod
    def verify_multiple_aggregate_signatures_batches(rng, batches):
        """Not in the reference: what calling verify_multiple_aggregate_signatures(rng, batch) once per batch, in order, returns -- as ONE call on the GPU
        (mbls_verify_multiple_batches_rng), which costs about what one such call costs. `batches`: an iterable of iterables of
        (signature, aggregate_public_key, message). Returns list[bool], one per batch; a bad batch rejects itself and nothing else. The scalars are drawn as
        above and in the order the per-batch calls would draw them (for every batch, the sets in front of its first signature outside G2), so `rng` is left
        exactly where those calls would leave it."""
        return AggregateSignature._vm_batches(rng, batches, False)

    @staticmethod
    def verify_multiple_aggregate_signatures_batches_locate(rng, batches):
        """verify_multiple_aggregate_signatures_batches, and in the same call (mbls_verify_multiple_batches_locate_rng) which sets of the rejected batches are the
        bad ones. Returns (list[bool], list[list[bool]]): one bool per batch as above, and per batch one bool per set. Every set of an accepted batch reads
        True -- a passing batch is not examined set by set: the batch check is the statement verify_multiple makes. A set of a rejected batch reads what the
        one-set batch with its scalar returns; a set at or behind the batch's first signature outside G2 has no scalar (the reference never draws one) and
        reads False. `rng` is left exactly where verify_multiple_aggregate_signatures_batches leaves it."""
        return AggregateSignature._vm_batches(rng, batches, True)

    @staticmethod
    def _vm_batches(rng, batches, locate):
        batches = [list(b) for b in batches]
        if not batches:
            return ([], []) if locate else []
        sets = [s for b in batches for s in b]
        boffs = [0]
        for b in batches:
            boffs.append(boffs[-1] + len(b))
        failed = []
        draw = _reference_draw(rng, failed)
        offs = [0]
        for s in sets:
            offs.append(offs[-1] + len(s[2]))
        moff = (C.c_uint64 * len(offs))(*offs)
        boff = (C.c_uint32 * len(boffs))(*boffs)
        res = N.outbuf(len(batches))
        cb = N.SCALAR_SOURCE(draw)
        ctx = _ctx()
        S, A, M = N.cbuf(b"".join(s[0].point for s in sets)), N.cbuf(b"".join(s[1].point for s in sets)), N.cbuf(b"".join(bytes(s[2]) for s in sets))
        if locate:
            sres = N.outbuf(max(1, len(sets)))
            if not sets:
                C.memset(sres, 1, 1)
            rc = N.lib().mbls_verify_multiple_batches_locate_rng(ctx.handle, S, A, M, 0, moff, len(sets), boff, 0, len(batches), res, sres, None, cb, None)
        else:
            rc = N.lib().mbls_verify_multiple_batches_rng(ctx.handle, S, A, M, 0, moff, len(sets), boff, 0, len(batches), res, cb, None)
        if failed:
            raise failed[0]
        ctx.check(rc)
        out = [bool(x) for x in bytes(res)[:len(batches)]]
        if not locate:
            return out
        per_set = [bool(x) for x in bytes(sres)[:len(sets)]]
        return out, [per_set[boffs[b]:boffs[b + 1]] for b in range(len(batches))]

    @staticmethod
    def verify_multiple_aggregate_signatures_committee_batches(rng, batches, committees, table):
        """Not in the reference: verify_multiple_aggregate_signatures_committee once per batch, in order, as ONE call on the GPU
        (mbls_verify_multiple_batches_committee_msgtable_rng). `batches`: an iterable of iterables of the sets that method takes. Returns list[bool], one per
        batch; a bad batch rejects itself and nothing else. Inside a batch the sets that name one table entry share one Miller loop. `rng` is left exactly where
        verify_multiple_aggregate_signatures_batches leaves it on the spelled-out sets. A committee id, key index or message index that names nothing raises."""
        return AggregateSignature._vm_committee_batches(rng, batches, committees, table, False)

    @staticmethod
    def verify_multiple_aggregate_signatures_committee_batches_locate(rng, batches, committees, table):
        """verify_multiple_aggregate_signatures_committee_batches, and in the same call (mbls_verify_multiple_batches_committee_msgtable_locate_rng) which sets of
        the rejected batches are the bad ones. Returns (list[bool], list[list[bool]]) with the semantics of verify_multiple_aggregate_signatures_batches_locate."""
        return AggregateSignature._vm_committee_batches(rng, batches, committees, table, True)

    @staticmethod
    def _vm_committee_batches(rng, batches, committees, table, locate):
        batches = [list(b) for b in batches]
        if not batches:
            return ([], []) if locate else []
        sets = [s for b in batches for s in b]
        boffs = [0]
        for b in batches:
            boffs.append(boffs[-1] + len(b))
        stride = max(4, (committees.max_members + 31) // 32 * 4)
        words, fields = [], []
        for s in sets:
            if isinstance(s[1], SingleKey):
                words.append(N.VM_SET_SINGLE_KEY | s[1].index)
                fields.append(bytes(stride))
            else:
                cid, field = int(s[1]), bytes(s[2])
                if not 0 <= cid < N.VM_SET_SINGLE_KEY:
                    raise ValueError("committee id out of range")
                if len(field) > stride and any(field[stride:]):
                    raise ValueError("a bitfield names members beyond the table's largest committee")
                words.append(cid)
                fields.append(field[:stride].ljust(stride, b"\0"))
        n = len(sets)
        failed = []
        cb = N.SCALAR_SOURCE(_reference_draw(rng, failed))
        cidx = (C.c_uint32 * max(1, n))(*words)
        midx = (C.c_uint32 * max(1, n))(*[int(s[3]) for s in sets])
        boff = (C.c_uint32 * len(boffs))(*boffs)
        res = N.outbuf(len(batches))
        ctx = committees.ctx
        S, B = N.cbuf(b"".join(s[0].point for s in sets)), N.cbuf(b"".join(fields))
        if locate:
            sres = N.outbuf(max(1, n))
            if not sets:
                C.memset(sres, 1, 1)
            rc = N.lib().mbls_verify_multiple_batches_committee_msgtable_locate_rng(ctx.handle, committees.handle, S, cidx, B, stride, table.handle, midx, n, boff, 0,
                                                                                   len(batches), res, sres, None, cb, None)
        else:
            rc = N.lib().mbls_verify_multiple_batches_committee_msgtable_rng(ctx.handle, committees.handle, S, cidx, B, stride, table.handle, midx, n, boff, 0,
                                                                            len(batches), res, cb, None)
        if failed:
            raise failed[0]
        ctx.check(rc)
        out = [bool(x) for x in bytes(res)[:len(batches)]]
        if not locate:
            return out
        per_set = [bool(x) for x in bytes(sres)[:n]]
        return out, [per_set[boffs[b]:boffs[b + 1]] for b in range(len(batches))]

    @staticmethod
    def verify_multiple_aggregate_signatures_committee_span_batches(rng, batches, committees, table):
        """Not in the reference: verify_multiple_aggregate_signatures_committee_span once per batch (per block), in order, as ONE call on the GPU
        (mbls_verify_multiple_batches_committee_span_msgtable_rng). `batches`: an iterable of iterables of the sets that method takes. Returns list[bool], one per
        batch; a bad batch rejects itself and nothing else. `rng` is left exactly where verify_multiple_aggregate_signatures_batches leaves it on the spelled-out
        sets. A malformed set, a key index or a message index that names nothing raises."""
        return AggregateSignature._vm_committee_span_batches(rng, batches, committees, table, False)

    @staticmethod
    def verify_multiple_aggregate_signatures_committee_span_batches_locate(rng, batches, committees, table):
        """verify_multiple_aggregate_signatures_committee_span_batches, and in the same call (mbls_verify_multiple_batches_committee_span_msgtable_locate_rng) which
        sets of the rejected batches are the bad ones. Returns (list[bool], list[list[bool]]) with the semantics of
        verify_multiple_aggregate_signatures_batches_locate."""
        return AggregateSignature._vm_committee_span_batches(rng, batches, committees, table, True)

    @staticmethod
    def _vm_committee_span_batches(rng, batches, committees, table, locate):
        batches = [list(b) for b in batches]
        if not batches:
            return ([], []) if locate else []
        sets = [s for b in batches for s in b]
        boffs = [0]
        for b in batches:
            boffs.append(boffs[-1] + len(b))
        id_lists, fields = [], []
        for s in sets:
            if isinstance(s[1], SingleKey):
                id_lists.append([N.VM_SET_SINGLE_KEY | s[1].index])
                fields.append(b"")
            else:
                ids = [int(x) for x in s[1]]
                if any(not 0 <= x < N.VM_SET_SINGLE_KEY for x in ids):
                    raise ValueError("committee id out of range")
                id_lists.append(ids)
                fields.append(bytes(s[2]))
        stride = max(4, (max([len(f) for f in fields] + [0]) + 3) // 4 * 4)
        n = len(sets)
        n_ids = sum(map(len, id_lists))
        ids = (C.c_uint32 * max(1, n_ids))(*[x for l in id_lists for x in l])
        off = (C.c_uint32 * (n + 1))(*([0] + [sum(map(len, id_lists[:i + 1])) for i in range(n)]))
        failed = []
        cb = N.SCALAR_SOURCE(_reference_draw(rng, failed))
        midx = (C.c_uint32 * max(1, n))(*[int(s[3]) for s in sets])
        boff = (C.c_uint32 * len(boffs))(*boffs)
        res = N.outbuf(len(batches))
        ctx = committees.ctx
        S, B = N.cbuf(b"".join(s[0].point for s in sets)), N.cbuf(b"".join(f.ljust(stride, b"\0") for f in fields))
        if locate:
            sres = N.outbuf(max(1, n))
            if not sets:
                C.memset(sres, 1, 1)
            rc = N.lib().mbls_verify_multiple_batches_committee_span_msgtable_locate_rng(ctx.handle, committees.handle, S, ids, n_ids, off, B, stride, table.handle, midx, n,
                                                                                        boff, 0, len(batches), res, sres, None, cb, None)
        else:
            rc = N.lib().mbls_verify_multiple_batches_committee_span_msgtable_rng(ctx.handle, committees.handle, S, ids, n_ids, off, B, stride, table.handle, midx, n, boff, 0,
                                                                                 len(batches), res, cb, None)
        if failed:
            raise failed[0]
        ctx.check(rc)
        out = [bool(x) for x in bytes(res)[:len(batches)]]
        if not locate:
            return out
        per_set = [bool(x) for x in bytes(sres)[:n]]
        return out, [per_set[boffs[b]:boffs[b + 1]] for b in range(len(batches))]

    @classmethod
    def from_bytes(cls, data):
        out = N.outbuf(96)
        _raise(N.lib().mbls_sig_from_bytes(_ctx().handle, N.cbuf(data), len(data), out))
        return cls(bytes(out))

    def as_bytes(self):
        return self.point

    def __eq__(self, other):
        return isinstance(other, AggregateSignature) and self.point == other.point
