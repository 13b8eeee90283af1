"""ctypes loader for libmbls_hip.so. There is no CPU fallback: if the HIP library is missing, or no GPU
is present when a context is created, this raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MBLS_LIB", os.path.join(HERE, "libmbls_hip.so"))

# error codes (include/mbls.h)
OK = 0
ERR_INVALID_G1_SIZE = 1
ERR_INVALID_G2_SIZE = 2
ERR_INVALID_POINT = 3
ERR_AGGREGATE_EMPTY_POINTS = 4
ERR_INVALID_SECRET_KEY_SIZE = 5
ERR_INVALID_SECRET_KEY_RANGE = 6
ERR_DEVICE = 100
ERR_ARGUMENT = 101
PENDING = 102                   # mbls_stream_query: the call is not done
PK_COMPRESSED, PK_UNCOMPRESSED = 0, 1
RESIDUE_NAME_BYTES = 16           # MBLS_RESIDUE_NAME_BYTES
VM_PARTIAL_BYTES = 896          # include/mbls.h MBLS_VM_PARTIAL_BYTES
N_PHASES = 6
PHASE_NAMES = ("aggregate", "sig", "hash", "miller", "final", "pack")

_lib = None

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
vp = C.c_void_p
class Limits(C.Structure):
    """include/mbls.h mbls_limits"""
    _fields_ = [(n, C.c_uint64) for n in ("round_items", "coop_max_items", "coop_hash_max_items", "coop_pack_min_items", "coop_pack_max_items", "coop_hash_pack_min_items",
                                          "split_max_items", "fork_max_items", "hash2_max_items", "tracks_min_rest", "tracks_side_max")]


class PassPlan(C.Structure):
    """include/mbls.h mbls_pass_plan"""
    _fields_ = [(n, C.c_uint64) for n in ("first_item", "items", "workspace_first", "workspace_items")] + \
               [(n, C.c_uint32) for n in ("track", "stage", "pairing", "message", "front", "sig_subgroup_from_miller_loop")]


class BatchPlan(C.Structure):
    """include/mbls.h mbls_batch_plan"""
    _fields_ = [("mode", C.c_uint32), ("n_passes", C.c_uint32), ("passes", PassPlan * 3)]


PAIRING_WAVE, PAIRING_LANE, PAIRING_LANES2, PAIRING_LANES4, PAIRING_WAVE_X2 = 0, 1, 2, 4, 5
MESSAGE_LANE, MESSAGE_LANES2, MESSAGE_WAVE, MESSAGE_WAVE_X4 = 1, 2, 3, 4
FRONT_IN_A_ROW, FRONT_MESSAGE_BESIDE, FRONT_ALL_BESIDE = 0, 1, 2
BATCH_ONE_PASS, BATCH_ROUNDS_THEN_REST, BATCH_ROUND_BESIDE_REST, BATCH_TWO_HALVES = 0, 1, 2, 3


def default_limits(round_items=65536):
    """the library's default routing limits for a device whose round is round_items lanes (pure: no GPU)"""
    L = Limits()
    lib().mbls_default_limits(round_items, C.byref(L))
    return L


def plan_batch(n, limits=None):
    """what mbls_fast_aggregate_verify_batch_device would do with n items under `limits` (pure: no GPU) -> (mode, [pass dicts])"""
    L = limits if limits is not None else default_limits()
    b = BatchPlan()
    rc = lib().mbls_plan_batch(C.byref(L), n, C.byref(b))
    if rc != OK:
        raise MblsError(rc, "mbls_plan_batch")
    return b.mode, [{f: getattr(b.passes[i], f) for f, _ in PassPlan._fields_} for i in range(b.n_passes)]


def plan_workspace_items(n, k, split_layout=True, limits=None):
    """workspace items the plan of n items of k keys needs (pure: no GPU); split_layout: uniform 96-byte keys or key-table indices"""
    L = limits if limits is not None else default_limits()
    return int(lib().mbls_plan_workspace_items(C.byref(L), n, k, 1 if split_layout else 0))


def plan_locate_workspace_items(n_sets, n_batches, limits=None):
    """workspace items a mbls_verify_multiple_batches_locate* call of n_sets sets in n_batches batches reserves (pure: no GPU)"""
    L = limits if limits is not None else default_limits()
    return int(lib().mbls_plan_locate_workspace_items(C.byref(L), n_sets, n_batches))


class SharedMsgsPlan(C.Structure):
    """include/mbls.h mbls_shared_msgs_plan"""
    _fields_ = [("batch", BatchPlan), ("list_message", C.c_uint32), ("list_pieces", C.c_uint32), ("list_piece_items", C.c_uint64), ("list_workspace_items", C.c_uint64),
                ("table_entries", C.c_uint64)]


MESSAGE_GATHER = 5


def plan_batch_shared_msgs(n, n_msgs, limits=None):
    """what the *_shared_msgs entries would do with n items over a list of n_msgs messages under `limits` (pure: no GPU) -> (mode, [pass dicts], list dict)"""
    L = limits if limits is not None else default_limits()
    sp = SharedMsgsPlan()
    rc = lib().mbls_plan_batch_shared_msgs(C.byref(L), n, n_msgs, C.byref(sp))
    if rc != OK:
        raise MblsError(rc, "mbls_plan_batch_shared_msgs")
    b = sp.batch
    return (b.mode, [{f: getattr(b.passes[i], f) for f, _ in PassPlan._fields_} for i in range(b.n_passes)],
            {f: getattr(sp, f) for f in ("list_message", "list_pieces", "list_piece_items", "list_workspace_items", "table_entries")})


def plan_shared_msgs_workspace_items(n, n_msgs, k, split_layout=True, limits=None):
    """workspace items a *_shared_msgs call of n items of k keys over n_msgs messages reserves (pure: no GPU)"""
    L = limits if limits is not None else default_limits()
    return int(lib().mbls_plan_shared_msgs_workspace_items(C.byref(L), n, n_msgs, k, 1 if split_layout else 0))


class VmSharedMsgsPlan(C.Structure):
    """include/mbls.h mbls_vm_shared_msgs_plan"""
    _fields_ = [(n, C.c_uint32) for n in ("route", "list_message", "list_pieces", "miller", "tree_levels", "chains_beside", "sig_lane_pairs", "reserved")] + \
               [(n, C.c_uint64) for n in ("list_piece_items", "list_workspace_items", "table_entries", "miller_items", "miller_rounds", "miller_rest_items",
                                          "workspace_items")]


VM_ROUTE_PER_SET, VM_ROUTE_GROUPED = 0, 1
VM_GROUPING_AUTO, VM_GROUPING_ALWAYS, VM_GROUPING_NEVER = 0, 1, 2


def plan_verify_multiple_shared_msgs(n, n_msgs, mode=0, limits=None):
    """what the verify_multiple*_shared_msgs entries would do with n sets over a list of n_msgs messages under `limits` and grouping mode (pure: no GPU) -> dict"""
    L = limits if limits is not None else default_limits()
    vp_ = VmSharedMsgsPlan()
    rc = lib().mbls_plan_verify_multiple_shared_msgs(C.byref(L), n, n_msgs, mode, C.byref(vp_))
    if rc != OK:
        raise MblsError(rc, "mbls_plan_verify_multiple_shared_msgs")
    return {f: getattr(vp_, f) for f, _ in VmSharedMsgsPlan._fields_ if f != "reserved"}


def plan_verify_multiple_shared_msgs_locate_workspace_items(n, n_msgs, mode=0, limits=None):
    """workspace items a mbls_verify_multiple*_shared_msgs_locate* call of n sets over n_msgs messages reserves under grouping `mode` (pure: no GPU)"""
    L = limits if limits is not None else default_limits()
    return int(lib().mbls_plan_verify_multiple_shared_msgs_locate_workspace_items(C.byref(L), n, n_msgs, mode))


def plan_verify_multiple_shared_msgs_workspace_items(n, n_msgs, mode=0, limits=None):
    """workspace items such a call reserves (pure: no GPU; 0 for arguments the plan refuses)"""
    L = limits if limits is not None else default_limits()
    return int(lib().mbls_plan_verify_multiple_shared_msgs_workspace_items(C.byref(L), n, n_msgs, mode))


def plan_verify_multiple_msgtable(n, table_size, named=0, mode=0, limits=None):
    """what the verify_multiple*_msgtable entries would do with n sets over a resident table of table_size entries of which `named` distinct ones are named
    (0: not known -- the device entries) under `limits` and grouping mode (pure: no GPU) -> dict"""
    L = limits if limits is not None else default_limits()
    vp_ = VmSharedMsgsPlan()
    rc = lib().mbls_plan_verify_multiple_msgtable(C.byref(L), n, table_size, named, mode, C.byref(vp_))
    if rc != OK:
        raise MblsError(rc, "mbls_plan_verify_multiple_msgtable")
    return {f: getattr(vp_, f) for f, _ in VmSharedMsgsPlan._fields_ if f != "reserved"}


def plan_verify_multiple_msgtable_workspace_items(n, table_size, named=0, mode=0, limits=None):
    """workspace items such a call reserves (pure: no GPU; 0 for arguments the plan refuses)"""
    L = limits if limits is not None else default_limits()
    return int(lib().mbls_plan_verify_multiple_msgtable_workspace_items(C.byref(L), n, table_size, named, mode))


def plan_verify_multiple_msgtable_locate_workspace_items(n, table_size, named=0, mode=0, limits=None):
    """workspace items a mbls_verify_multiple*_msgtable_locate* call reserves (pure: no GPU)"""
    L = limits if limits is not None else default_limits()
    return int(lib().mbls_plan_verify_multiple_msgtable_locate_workspace_items(C.byref(L), n, table_size, named, mode))


class VmBatchesCommitteePlan(C.Structure):
    """include/mbls.h mbls_vm_batches_committee_plan"""
    _fields_ = [("route", C.c_int32), ("miller", C.c_int32), ("tree_levels", C.c_uint32), ("product_levels", C.c_uint32), ("bound", C.c_uint64),
                ("miller_items", C.c_uint64), ("workspace_items", C.c_uint64)]


VBG_MAX_SETS = 1024              # include/mbls.h MBLS_VBG_MAX_SETS: a batch with more sets is not grouped
VBG_NONE = 0xFFFFFFFF


def plan_verify_multiple_batches_committee(n_sets, n_batches, sets_per_batch=0, table_size=0, max_groups=0, mode=0, locate=False, limits=None):
    """what the verify_multiple_batches_committee_msgtable entries would do with n_sets sets in n_batches batches (sets_per_batch 0: a ragged device-side table)
    over a resident table of table_size entries under the caller's bound max_groups (0: none), `limits` and grouping mode (pure: no GPU) -> dict"""
    L = limits if limits is not None else default_limits()
    vp_ = VmBatchesCommitteePlan()
    rc = lib().mbls_plan_verify_multiple_batches_committee(C.byref(L), n_sets, n_batches, sets_per_batch, table_size, max_groups, mode, 1 if locate else 0, C.byref(vp_))
    if rc != OK:
        raise MblsError(rc, "mbls_plan_verify_multiple_batches_committee")
    return {f: getattr(vp_, f) for f, _ in VmBatchesCommitteePlan._fields_}


class StreamOpts(C.Structure):
    """include/mbls.h mbls_stream_opts (0 = default)"""
    _fields_ = [("round_items", C.c_uint64), ("round_keys", C.c_uint64), ("round_msg_bytes", C.c_uint64), ("depth", C.c_uint32), ("policy", C.c_uint32)]


class StreamStats(C.Structure):
    """include/mbls.h mbls_stream_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("calls", "items", "pieces", "rounds", "full_rounds", "split_calls", "gathered_bytes")]


class StreamCallShape(C.Structure):
    """include/mbls.h mbls_stream_call_shape"""
    _fields_ = [("n", C.c_uint64), ("k", C.c_uint32), ("msg_len", C.c_uint32), ("pk_offsets", u32p), ("msg_offsets", u64p), ("flush_after", C.c_uint32)]


class StreamPiece(C.Structure):
    """include/mbls.h mbls_stream_piece"""
    _fields_ = [(n, C.c_uint64) for n in ("call", "first", "items", "round", "round_first")]


STREAM_FAST_AGGREGATE_VERIFY, STREAM_VERIFY = 0, 1
STREAM_WORK_CONSERVING, STREAM_FULL_ROUNDS = 0, 1


def stream_cut(calls, round_items, round_keys, round_msg_bytes):
    """how a verification stream cuts a sequence of calls into rounds (pure: no GPU) -> [piece dicts]. calls: dicts with n and optionally k, msg_len,
    pk_offsets, msg_offsets (sequences) and flush_after (a launch is forced after the call)"""
    o = StreamOpts(round_items, round_keys, round_msg_bytes, 1, STREAM_FULL_ROUNDS)
    shapes = (StreamCallShape * max(1, len(calls)))()
    keep = []
    for i, c in enumerate(calls):
        s = shapes[i]
        s.n, s.k, s.msg_len, s.flush_after = c["n"], c.get("k", 0), c.get("msg_len", 0), int(bool(c.get("flush_after", 0)))
        if c.get("pk_offsets") is not None:
            a = (C.c_uint32 * len(c["pk_offsets"]))(*c["pk_offsets"]); keep.append(a); s.pk_offsets = C.cast(a, u32p)
        if c.get("msg_offsets") is not None:
            a = (C.c_uint64 * len(c["msg_offsets"]))(*c["msg_offsets"]); keep.append(a); s.msg_offsets = C.cast(a, u64p)
    cnt = C.c_uint64(0)
    rc = lib().mbls_stream_cut(C.byref(o), shapes, len(calls), None, 0, C.byref(cnt))
    if rc != OK:
        raise MblsError(rc, "mbls_stream_cut")
    out = (StreamPiece * max(1, cnt.value))()
    rc = lib().mbls_stream_cut(C.byref(o), shapes, len(calls), out, cnt.value, C.byref(cnt))
    if rc != OK:
        raise MblsError(rc, "mbls_stream_cut")
    return [{f: getattr(out[i], f) for f, _ in StreamPiece._fields_} for i in range(cnt.value)]


def stream_cut_vm(call_sets, round_items, flush_after=None):
    """how a verify_multiple stream cuts a sequence of calls (one batch each, never split) into rounds (pure: no GPU) -> [piece dicts]. call_sets: the sets per
    call; flush_after: None or one flag per call (a launch is forced after the call)"""
    o = StreamOpts(round_items, 0, 0, 1, STREAM_FULL_ROUNDS)
    n = len(call_sets)
    sets = (C.c_uint64 * max(1, n))(*call_sets)
    fl = None if flush_after is None else (C.c_uint32 * max(1, n))(*[int(bool(f)) for f in flush_after])
    out = (StreamPiece * max(1, n))()
    cnt = C.c_uint64(0)
    rc = lib().mbls_stream_cut_vm(C.byref(o), sets, fl, n, out, n, C.byref(cnt))
    if rc != OK:
        raise MblsError(rc, "mbls_stream_cut_vm")
    return [{f: getattr(out[i], f) for f, _ in StreamPiece._fields_} for i in range(cnt.value)]


# mbls_scalar_source (include/mbls.h): void draw(void* user, uint64_t* out, uint64_t count)
SCALAR_SOURCE = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64)
SIGNATURES = {
    "mbls_ctx_create": (C.c_int, [C.POINTER(vp), C.c_int]),
    "mbls_ctx_destroy": (None, [vp]),
    "mbls_ctx_reserve": (C.c_int, [vp, C.c_uint64]),
    "mbls_ctx_reserve_keys": (C.c_int, [vp, C.c_uint64]),
    "mbls_ctx_set_coop_max_items": (C.c_int, [vp, C.c_uint64]),
    "mbls_ctx_set_coop_hash_max_items": (C.c_int, [vp, C.c_uint64]),
    "mbls_ctx_set_coop_packing": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint64]),
    "mbls_ctx_set_round_items": (C.c_int, [vp, C.c_uint64]),
    "mbls_ctx_reset_tuning": (C.c_int, [vp]),
    "mbls_ctx_set_lane_shaping": (C.c_int, [vp, C.c_uint64, C.c_uint64]),
    "mbls_ctx_set_tracks": (C.c_int, [vp, C.c_uint64, C.c_uint64]),
    "mbls_ctx_set_secret_ops": (C.c_int, [vp, C.c_int]),
    "mbls_default_limits": (None, [C.c_uint64, vp]),
    "mbls_ctx_get_limits": (C.c_int, [vp, vp]),
    "mbls_plan_batch": (C.c_int, [vp, C.c_uint64, vp]),
    "mbls_plan_workspace_items": (C.c_uint64, [vp, C.c_uint64, C.c_uint32, C.c_int]),
    "mbls_last_error": (C.c_char_p, [vp]),
    "mbls_fast_aggregate_verify_batch_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_verify_batch_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_int, C.c_uint64, vp, vp, vp, vp]),
    "mbls_verify_batch": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_int, C.c_uint64, vp, vp]),
    "mbls_aggregate_verify_batch": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp]),
    "mbls_aggregate_verify_batch_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp, vp]),
    "mbls_keytable_create": (C.c_int, [vp, C.c_uint64, C.POINTER(vp)]),
    "mbls_keytable_destroy": (None, [vp]),
    "mbls_keytable_size": (C.c_uint64, [vp]),
    "mbls_keytable_append": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), vp]),
    "mbls_keytable_append_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), vp, vp]),
    "mbls_keytable_get": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp, vp]),
    "mbls_fast_aggregate_verify_batch_indexed_device": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch_indexed": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_ctx_reserve_msgs": (C.c_int, [vp, C.c_uint64]),
    "mbls_plan_batch_shared_msgs": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp]),
    "mbls_plan_shared_msgs_workspace_items": (C.c_uint64, [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int]),
    "mbls_fast_aggregate_verify_batch_shared_msgs_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch_shared_msgs": (C.c_int, [vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_verify_batch_shared_msgs_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_int, C.c_uint64, vp, vp, vp, vp]),
    "mbls_verify_batch_shared_msgs": (C.c_int, [vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_int, C.c_uint64, vp, vp]),
    "mbls_fast_aggregate_verify_batch_indexed_shared_msgs_device": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch_indexed_shared_msgs": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_msgtable_create": (C.c_int, [vp, C.c_uint64, C.POINTER(vp)]),
    "mbls_msgtable_destroy": (None, [vp]),
    "mbls_msgtable_size": (C.c_uint64, [vp]),
    "mbls_msgtable_append": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mbls_msgtable_append_device": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64), vp]),
    "mbls_msgtable_get": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp, vp]),
    "mbls_msgtable_clear": (C.c_int, [vp]),
    "mbls_fast_aggregate_verify_batch_msgtable_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch_msgtable": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_verify_batch_msgtable_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_uint64, vp, vp, vp, vp]),
    "mbls_verify_batch_msgtable": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_uint64, vp, vp]),
    "mbls_fast_aggregate_verify_batch_indexed_msgtable_device": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch_indexed_msgtable": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_committees_create": (C.c_int, [vp, vp, C.c_uint64, C.POINTER(vp)]),
    "mbls_committees_destroy": (None, [vp]),
    "mbls_committees_count": (C.c_uint64, [vp]),
    "mbls_committees_clear": (C.c_int, [vp]),
    "mbls_committees_max_members": (C.c_uint32, [vp]),
    "mbls_committees_append": (C.c_int, [vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mbls_committees_get": (C.c_int, [vp, C.c_uint64, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mbls_ctx_set_committee_route": (C.c_int, [vp, C.c_int]),
    "mbls_plan_committee_route": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.c_int]),
    "mbls_ctx_reserve_committee_items": (C.c_int, [vp, C.c_uint64, C.c_uint32]),
    "mbls_fast_aggregate_verify_batch_committee_device": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch_committee": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp]),
    "mbls_fast_aggregate_verify_batch_committee_msgtable_device": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch_committee_msgtable": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp]),
    "mbls_fast_aggregate_verify_batch_committee_span_device": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_uint64, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch_committee_span": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_uint64, vp, vp]),
    "mbls_fast_aggregate_verify_batch_committee_span_msgtable_device": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_uint64, vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify_batch_committee_span_msgtable": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_uint64, vp, vp]),
    "mbls_ctx_reserve_committee_span_items": (C.c_int, [vp, C.c_uint64, C.c_uint32]),
    "mbls_plan_committee_span": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mbls_aggregate_signatures_batch": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_aggregate_signatures_batch_device": (C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint64, vp, vp, vp]),
    "mbls_pk_from_bytes": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "mbls_pk_from_bytes_unchecked": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "mbls_pk_from_uncompressed_bytes": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "mbls_pk_as_bytes": (C.c_int, [vp, vp, vp]),
    "mbls_pk_key_validate": (C.c_int, [vp, vp]),
    "mbls_pk_from_secret_key": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "mbls_sig_from_bytes": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "mbls_sign": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, vp]),
    "mbls_verify": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "mbls_aggregate_public_keys": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "mbls_aggregate_public_key_add": (C.c_int, [vp, vp, vp, vp]),
    "mbls_aggregate_signature_add": (C.c_int, [vp, vp, vp, vp]),
    "mbls_fast_aggregate_verify": (C.c_int, [vp, vp, vp, C.c_size_t, vp, C.c_size_t]),
    "mbls_fast_aggregate_verify_pre_aggregated": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "mbls_aggregate_verify": (C.c_int, [vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t]),
    "mbls_verify_multiple_aggregate_signatures": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_size_t]),
    "mbls_verify_multiple_aggregate_signatures_device": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_aggregate_signatures_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_size_t, SCALAR_SOURCE, vp]),
    "mbls_verify_multiple_sets_device": (C.c_int, [vp, vp, vp, C.c_int, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_sets_indexed_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp]),
    "mbls_verify_multiple_partial_device": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp]),
    "mbls_verify_multiple_finish_device": (C.c_int, [vp, vp, C.c_uint64, vp, vp, vp]),
    "mbls_ctx_set_vm_grouping": (C.c_int, [vp, C.c_int]),
    "mbls_plan_verify_multiple_shared_msgs": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_int, vp]),
    "mbls_plan_verify_multiple_shared_msgs_workspace_items": (C.c_uint64, [vp, C.c_uint64, C.c_uint64, C.c_int]),
    "mbls_verify_multiple_shared_msgs_device": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_sets_indexed_shared_msgs_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_shared_msgs": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp]),
    "mbls_verify_multiple_shared_msgs_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp, SCALAR_SOURCE, vp]),
    "mbls_verify_multiple_batches_device": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_batches_indexed_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_batches": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, vp]),
    "mbls_verify_multiple_batches_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, SCALAR_SOURCE, vp]),
    "mbls_plan_verify_multiple_shared_msgs_locate_workspace_items": (C.c_uint64, [vp, C.c_uint64, C.c_uint64, C.c_int]),
    "mbls_verify_multiple_shared_msgs_locate_device": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, vp, vp]),
    "mbls_verify_multiple_sets_indexed_shared_msgs_locate_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp,
                                                                              vp, vp, vp]),
    "mbls_verify_multiple_shared_msgs_locate": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, vp]),
    "mbls_verify_multiple_shared_msgs_locate_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, SCALAR_SOURCE, vp]),
    "mbls_plan_verify_multiple_msgtable": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, vp]),
    "mbls_plan_verify_multiple_msgtable_workspace_items": (C.c_uint64, [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]),
    "mbls_plan_verify_multiple_msgtable_locate_workspace_items": (C.c_uint64, [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]),
    "mbls_verify_multiple_msgtable_device": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_sets_indexed_msgtable_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_msgtable_rng": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, vp, SCALAR_SOURCE, vp]),
    "mbls_verify_multiple_msgtable_locate_device": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp]),
    "mbls_verify_multiple_sets_indexed_msgtable_locate_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp]),
    "mbls_verify_multiple_msgtable_locate_rng": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp, SCALAR_SOURCE, vp]),
    "mbls_verify_multiple_committee_msgtable_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_committee_msgtable_locate_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp]),
    "mbls_verify_multiple_committee_msgtable_rng": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, SCALAR_SOURCE, vp]),
    "mbls_verify_multiple_committee_msgtable_locate_rng": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, SCALAR_SOURCE, vp]),
    "mbls_verify_multiple_committee_span_msgtable_device": (C.c_int, [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_committee_span_msgtable_locate_device": (C.c_int, [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp]),
    "mbls_verify_multiple_committee_span_msgtable_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, SCALAR_SOURCE, vp]),
    "mbls_verify_multiple_committee_span_msgtable_locate_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, SCALAR_SOURCE, vp]),
    "mbls_ctx_set_vm_span_split": (C.c_int, [vp, C.c_int]),
    "mbls_plan_verify_multiple_span": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "mbls_plan_verify_multiple_batches_committee": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_int, vp]),
    "mbls_verify_multiple_batches_committee_msgtable_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp,
                                                                         vp, vp]),
    "mbls_verify_multiple_batches_committee_msgtable_locate_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64,
                                                                                vp, vp, vp, vp, vp]),
    "mbls_verify_multiple_batches_committee_msgtable_rng": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, SCALAR_SOURCE, vp]),
    "mbls_verify_multiple_batches_committee_msgtable_locate_rng": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, vp, vp,
                                                                             SCALAR_SOURCE, vp]),
    "mbls_plan_verify_multiple_batches_committee_span": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_int, vp,
                                                                   C.POINTER(C.c_uint32)]),
    "mbls_verify_multiple_batches_committee_span_msgtable_device": (C.c_int, [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint32,
                                                                              C.c_uint64, C.c_uint64, vp, vp, vp]),
    "mbls_verify_multiple_batches_committee_span_msgtable_locate_device": (C.c_int, [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint32,
                                                                                     C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp]),
    "mbls_verify_multiple_batches_committee_span_msgtable_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp,
                                                                           SCALAR_SOURCE, vp]),
    "mbls_verify_multiple_batches_committee_span_msgtable_locate_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32,
                                                                                  C.c_uint64, vp, vp, vp, SCALAR_SOURCE, vp]),
    "mbls_vbg_group_probe": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mbls_plan_locate_workspace_items": (C.c_uint64, [vp, C.c_uint64, C.c_uint64]),
    "mbls_verify_multiple_batches_locate_device": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, vp,
                                                             vp, vp, vp]),
    "mbls_verify_multiple_batches_locate_indexed_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, vp,
                                                                     vp, vp, vp]),
    "mbls_verify_multiple_batches_locate": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, vp, vp, vp]),
    "mbls_verify_multiple_batches_locate_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, vp, vp, SCALAR_SOURCE, vp]),
    "mbls_multi_verify_multiple_aggregate_signatures": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_size_t]),
    "mbls_multi_verify_multiple_aggregate_signatures_rng": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, C.c_size_t, SCALAR_SOURCE, vp]),
    "mbls_pk_decode_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_uint64, vp, vp]),
    "mbls_pk_compress_batch": (C.c_int, [vp, vp, C.c_uint64, vp, vp]),
    "mbls_sig_check_batch": (C.c_int, [vp, vp, C.c_uint64, vp, vp]),
    "mbls_sign_batch": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint64, vp]),
    "mbls_sign_batch_device": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp]),
    "mbls_sk_to_pk_batch": (C.c_int, [vp, vp, C.c_int, C.c_uint64, vp]),
    "mbls_sk_to_pk_batch_device": (C.c_int, [vp, vp, C.c_int, C.c_uint64, vp, vp]),
    "mbls_hash_to_g2_batch": (C.c_int, [vp, vp, C.c_uint32, C.c_uint64, vp]),
    "mbls_hash_to_g2_batch_mode": (C.c_int, [vp, vp, C.c_uint32, C.c_uint64, vp, C.c_int]),
    "mbls_aggregate_public_keys_batch": (C.c_int, [vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_fp_mul_batch": (C.c_int, [vp, vp, vp, C.c_uint64, vp, C.c_int]),
    "mbls_map_to_g2_probe": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_int]),
    "mbls_miller_probe": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_int]),
    "mbls_final_exp_probe": (C.c_int, [vp, vp, C.c_uint64, vp, vp, C.c_int]),
    "mbls_dform_probe_shape": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mbls_dform_probe": (C.c_int, [vp, C.c_int, vp, C.c_uint64, vp]),
    "mbls_ctx_residue_regions": (C.c_int, [vp, vp, vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "mbls_ctx_residue_read": (C.c_int, [vp, C.c_uint32, C.c_uint64, C.c_uint64, vp]),
    "mbls_fp_mul_bench": (C.c_int, [vp, C.c_uint64, C.c_uint32, C.POINTER(C.c_float)]),
    "mbls_valu_bench": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "mbls_multi_create": (C.c_int, [C.POINTER(vp), C.POINTER(C.c_int), C.c_int]),
    "mbls_multi_destroy": (None, [vp]),
    "mbls_multi_device_count": (C.c_int, [vp]),
    "mbls_multi_last_error": (C.c_char_p, [vp]),
    "mbls_multi_context": (vp, [vp, C.c_int]),
    "mbls_multi_reserve": (C.c_int, [vp, C.c_uint64]),
    "mbls_multi_rccl_active": (C.c_int, [vp]),
    "mbls_multi_exchange_note": (C.c_char_p, [vp]),
    "mbls_multi_fast_aggregate_verify_bitmap": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_multi_device_bitmap": (vp, [vp, C.c_int]),
    "mbls_multi_fast_aggregate_verify_batch": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_multi_verify_batch": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_int, C.c_uint64, vp, vp]),
    "mbls_multi_keytable_create": (C.c_int, [vp, C.c_uint64, C.POINTER(vp)]),
    "mbls_multi_keytable_destroy": (None, [vp]),
    "mbls_multi_keytable_size": (C.c_uint64, [vp]),
    "mbls_multi_keytable_replica": (vp, [vp, C.c_int]),
    "mbls_multi_keytable_append": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), vp]),
    "mbls_multi_fast_aggregate_verify_batch_indexed": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp]),
    "mbls_stream_create": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.POINTER(vp)]),
    "mbls_stream_destroy": (None, [vp]),
    "mbls_stream_last_error": (C.c_char_p, [vp]),
    "mbls_stream_submit_device": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "mbls_stream_submit": (C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.POINTER(C.c_uint64)]),
    "mbls_stream_create_msgtable": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(vp)]),
    "mbls_stream_submit_msgidx_device": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "mbls_stream_submit_msgidx": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.POINTER(C.c_uint64)]),
    "mbls_stream_create_committee": (C.c_int, [vp, vp, vp, C.c_uint32, vp, C.POINTER(vp)]),
    "mbls_stream_submit_committee_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "mbls_stream_submit_committee": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, vp, vp, C.POINTER(C.c_uint64)]),
    "mbls_stream_flush": (C.c_int, [vp]),
    "mbls_stream_wait": (C.c_int, [vp, C.c_uint64]),
    "mbls_stream_query": (C.c_int, [vp, C.c_uint64]),
    "mbls_stream_get_stats": (C.c_int, [vp, vp]),
    "mbls_stream_cut": (C.c_int, [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mbls_stream_create_vm_committee": (C.c_int, [vp, vp, vp, C.c_uint32, vp, C.POINTER(vp)]),
    "mbls_stream_submit_vm_device": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "mbls_stream_submit_vm": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "mbls_stream_cut_vm": (C.c_int, [vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mbls_enable_phase_timing": (C.c_int, [vp, C.c_int]),
    "mbls_last_phase_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
}


class MblsError(RuntimeError):
    def __init__(self, code, what=""):
        super().__init__("mbls error %d %s" % (code, what))
        self.code = code


def lib():
    """Load libmbls_hip.so (raises if it has not been built: there is no fallback)."""
    global _lib
    if _lib is None:
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / HSA runtime. Two HIP runtimes in one process
        # do not coexist (the second one finds no GPU), so when torch is installed it is imported first: our
        # library's NEEDED libamdhip64.so.7 then resolves to the copy torch already loaded. Set MBLS_STANDALONE=1
        # to skip this and run against /opt/rocm's runtime alone.
        if os.environ.get("MBLS_STANDALONE", "0") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libmbls_hip.so not built: run `python -m milagro_bls_amd.build` (HIP extension is mandatory)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(l, name)
            f.restype = res
            f.argtypes = args
        _lib = l
    return _lib


class Context:
    """One mbls_ctx per GPU."""

    def __init__(self, device_id=0):
        self._h = vp()
        rc = lib().mbls_ctx_create(C.byref(self._h), device_id)
        if rc != OK:
            raise MblsError(rc, "mbls_ctx_create failed (no MI355X / HIP device available?)")

    def close(self):
        if self._h:
            lib().mbls_ctx_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def last_error(self):
        return lib().mbls_last_error(self._h).decode()

    def check(self, rc):
        if rc != OK:
            raise MblsError(rc, self.last_error())

    def reserve(self, n):
        self.check(lib().mbls_ctx_reserve(self._h, n))

    def reserve_msgs(self, n_msgs):
        """the table of hashed points for message lists of up to n_msgs messages (the *_shared_msgs entries)"""
        self.check(lib().mbls_ctx_reserve_msgs(self._h, n_msgs))

    def reserve_committee_items(self, max_items, max_members):
        """the scratch of the committee entries for batches of up to max_items items over committees of up to max_members members"""
        self.check(lib().mbls_ctx_reserve_committee_items(self._h, max_items, max_members))

    def reserve_committee_span_items(self, max_items, max_item_members):
        """the scratch of the committee-span entries for batches of up to max_items items whose list regions take max_item_members words each"""
        self.check(lib().mbls_ctx_reserve_committee_span_items(self._h, max_items, max_item_members))

    def set_committee_route(self, mode):
        """committee entries: CMT_ROUTE_AUTO / CMT_ROUTE_DIRECT / CMT_ROUTE_COMPLEMENT"""
        self.check(lib().mbls_ctx_set_committee_route(self._h, mode))

    def set_coop_max_items(self, n):
        """batches up to n items take the one-wave-per-item pairing check (0: never)"""
        self.check(lib().mbls_ctx_set_coop_max_items(self._h, n))

    def set_coop_hash_max_items(self, n):
        self.check(lib().mbls_ctx_set_coop_hash_max_items(self._h, n))

    def set_lane_shaping(self, split_max_items, fork_max_items):
        """one-lane path below a full round: two lanes per item in the Miller phase up to split_max_items, front phases side by side up to fork_max_items"""
        self.check(lib().mbls_ctx_set_lane_shaping(self._h, split_max_items, fork_max_items))

    def set_tracks(self, min_rest_items, side_max_items=16384):
        """batches of q rounds + r items with r >= min_rest_items: the last round and the remainder on two tracks side by side -- the remainder beside the round
        up to side_max_items, two equal halves above (min_rest_items = 0: never)"""
        self.check(lib().mbls_ctx_set_tracks(self._h, min_rest_items, side_max_items))

    def limits(self):
        """the context's current routing limits (setters and environment applied)"""
        L = Limits()
        self.check(lib().mbls_ctx_get_limits(self._h, C.byref(L)))
        return L

    def set_secret_ops(self, variable_time):
        """False (default): signing / sk -> pk look their tables up by scan + selection (constant-time access); True: by key-dependent address (throw-away keys only)"""
        self.check(lib().mbls_ctx_set_secret_ops(self._h, int(bool(variable_time))))

    def residue_regions(self):
        """test probe (include/mbls.h, mbls_ctx_residue_regions): ([(name, bytes)] of every device allocation the context owns, in the table's order; the
        workspace's capacity in items)"""
        cnt, cap = C.c_uint32(0), C.c_uint64(0)
        self.check(lib().mbls_ctx_residue_regions(self._h, None, None, 0, C.byref(cnt), C.byref(cap)))
        names = C.create_string_buffer(RESIDUE_NAME_BYTES * cnt.value)
        sizes = (C.c_uint64 * cnt.value)()
        self.check(lib().mbls_ctx_residue_regions(self._h, names, sizes, cnt.value, C.byref(cnt), C.byref(cap)))
        raw = names.raw
        return [(raw[RESIDUE_NAME_BYTES * i:RESIDUE_NAME_BYTES * (i + 1)].split(b"\0", 1)[0].decode(), int(sizes[i])) for i in range(cnt.value)], int(cap.value)

    def residue_read(self, region, offset, nbytes):
        """test probe (mbls_ctx_residue_read): bytes [offset, offset + nbytes) of region `region` (an index of residue_regions) once the device has drained"""
        out = (C.c_uint8 * max(1, nbytes))()
        self.check(lib().mbls_ctx_residue_read(self._h, region, offset, nbytes, out))
        return bytes(memoryview(out)[:nbytes])

    def reset_tuning(self):
        """every routing parameter (engine crossovers, packing, round, lane shaping) back to the library's defaults"""
        self.check(lib().mbls_ctx_reset_tuning(self._h))

    def set_round_items(self, items):
        """items per round of the one-lane kernels (0: the device's CUs x 4 x 64); a batch's remainder above whole rounds is routed on its own"""
        self.check(lib().mbls_ctx_set_round_items(self._h, items))

    def set_coop_packing(self, pairing_min_items, pairing_max_items, hash_min_items):
        """pairing_min < n <= pairing_max: two items per wave in the pairing check; n > hash_min: four per wave in the message phase"""
        self.check(lib().mbls_ctx_set_coop_packing(self._h, pairing_min_items, pairing_max_items, hash_min_items))


class KeyTable:
    """Resident table of decoded public keys in HBM (include/mbls.h, mbls_keytable_*): decode once, verify by index."""

    def __init__(self, ctx=None, capacity_hint=0):
        self.ctx = ctx or default_context()
        self._h = vp()
        self.ctx.check(lib().mbls_keytable_create(self.ctx.handle, capacity_hint, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().mbls_keytable_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return int(lib().mbls_keytable_size(self._h))

    def append(self, pks, n, pk_format=PK_COMPRESSED, validate=True):
        """-> (first_index, errs): errs[i] = OK / ERR_* as PublicKey::from_bytes[_unchecked] / from_uncompressed_bytes would return"""
        first = C.c_uint64(0)
        errs = outbuf(n)
        self.ctx.check(lib().mbls_keytable_append(self._h, cbuf(pks), pk_format, int(validate), n, C.byref(first), errs))
        return int(first.value), list(bytes(errs)[:n])

    def append_device(self, d_pks, n, d_errs, pk_format=PK_COMPRESSED, validate=True, stream=None):
        first = C.c_uint64(0)
        self.ctx.check(lib().mbls_keytable_append_device(self._h, d_pks, pk_format, int(validate), n, C.byref(first), d_errs, stream))
        return int(first.value)

    def get(self, first, n=1):
        out, errs = outbuf(96 * n), outbuf(n)
        self.ctx.check(lib().mbls_keytable_get(self._h, first, n, out, errs))
        return bytes(out)[:96 * n], list(bytes(errs)[:n])


class MsgTable:
    """Resident table of hashed messages in HBM (include/mbls.h, mbls_msgtable_*): hash once, verify by index in any call or stream."""

    def __init__(self, ctx=None, capacity_hint=0):
        self.ctx = ctx or default_context()
        self._h = vp()
        self.ctx.check(lib().mbls_msgtable_create(self.ctx.handle, capacity_hint, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().mbls_msgtable_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return int(lib().mbls_msgtable_size(self._h))

    def append(self, msgs, n, msg_len=32, msg_offsets=None):
        """n messages of msg_len bytes each, or msgs[msg_offsets[j]:msg_offsets[j+1]] (n + 1 offsets) -> first_index"""
        first = C.c_uint64(0)
        off = None if msg_offsets is None else (C.c_uint64 * len(msg_offsets))(*msg_offsets)
        self.ctx.check(lib().mbls_msgtable_append(self._h, cbuf(msgs), msg_len, off, n, C.byref(first)))
        return int(first.value)

    def append_device(self, d_msgs, n, msg_len=32, d_msg_offsets=None, stream=None):
        """device pointers; enqueues only (a bad range becomes a flagged entry) -> first_index"""
        first = C.c_uint64(0)
        self.ctx.check(lib().mbls_msgtable_append_device(self._h, d_msgs, msg_len, d_msg_offsets, n, C.byref(first), stream))
        return int(first.value)

    def get(self, first, n=1):
        """-> (96-byte compressed points of n entries, errs): errs[i] = ERR_ARGUMENT for a flagged entry"""
        out, errs = outbuf(96 * n), outbuf(n)
        self.ctx.check(lib().mbls_msgtable_get(self._h, first, n, out, errs))
        return bytes(out)[:96 * n], list(bytes(errs)[:n])

    def clear(self):
        """size back to 0, capacity kept; refused while a stream bound to the table has calls that have not completed"""
        self.ctx.check(lib().mbls_msgtable_clear(self._h))


COMMITTEE_MAX_MEMBERS = 2048    # include/mbls.h MBLS_COMMITTEE_MAX_MEMBERS
CMT_ROUTE_AUTO, CMT_ROUTE_DIRECT, CMT_ROUTE_COMPLEMENT = 0, 1, 2
VM_SET_SINGLE_KEY = 0x80000000   # mbls_verify_multiple_committee_msgtable*: a set under one key of the key table (the low 31 bits are its index)


def plan_committee_route(m, s, eligible=True, mode=CMT_ROUTE_AUTO):
    """the route an item with s of the m members of a committee selected takes under `mode` (pure: no GPU) -> True: complement, False: direct"""
    rc = lib().mbls_plan_committee_route(m, s, int(bool(eligible)), mode)
    if rc not in (0, 1):
        raise MblsError(rc, "mbls_plan_committee_route")
    return bool(rc)


SPAN_MAX_COMMITTEES = 64        # include/mbls.h MBLS_SPAN_MAX_COMMITTEES


def plan_committee_span(sizes, eligible, bits, mode=CMT_ROUTE_AUTO):
    """what the span kernel decides for one item (pure: no GPU): segment t has sizes[t] members and is eligible[t]; `bits` is the item's field (bytes, SSZ bit
    order) -> (complement mask: bit t set when segment t takes the complement route, entries of the direct list, entries of the missing list)"""
    q = len(sizes)
    if len(eligible) != q:
        raise ValueError("one eligible flag per segment")
    bits = bytes(bits)
    for s in sizes:
        if not 0 <= s <= 0xFFFFFFFF:
            raise ValueError("segment sizes are uint32")
    sz = (C.c_uint32 * max(1, q))(*sizes)
    el = (C.c_uint8 * max(1, q))(*[1 if e else 0 for e in eligible])
    mask, nd, nm = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    rc = lib().mbls_plan_committee_span(sz, el, q, cbuf(bits) if bits else None, len(bits), mode, C.byref(mask), C.byref(nd), C.byref(nm))
    if rc != 0:
        raise MblsError(rc, "mbls_plan_committee_span")
    return int(mask.value), int(nd.value), int(nm.value)


VM_SPAN_SPLITS = (0, 1, 2, 4, 8, 16)      # mbls_ctx_set_vm_span_split: 0 auto


def plan_verify_multiple_committee_span(n, table_size, stride_words, locate=False, split_mode=0, limits=None):
    """verify_multiple over committee spans (pure: no GPU): n sets over a message table of table_size entries, regions of stride_words words (min(8 * bits_stride,
    64 * the table's largest committee)) -> (split factor P of the key phase, workspace items the call reserves)"""
    L = limits if limits is not None else default_limits()
    split, items = C.c_uint32(0), C.c_uint64(0)
    rc = lib().mbls_plan_verify_multiple_span(C.byref(L), n, table_size, stride_words, int(bool(locate)), split_mode, C.byref(split), C.byref(items))
    if rc != 0:
        raise MblsError(rc, "mbls_plan_verify_multiple_span")
    return int(split.value), int(items.value)


def plan_verify_multiple_batches_committee_span(n_sets, n_batches, sets_per_batch=0, table_size=0, max_groups=0, mode=0, locate=False, stride_words=1, split_mode=0,
                                                limits=None):
    """the verify_multiple_batches_committee_span_msgtable entries (pure: no GPU): plan_verify_multiple_batches_committee's dict for the same arguments with
    workspace_items raised by the partial sums of the split key phase, and the split factor P (stride_words as plan_verify_multiple_committee_span takes it)
    -> (dict, P)"""
    L = limits if limits is not None else default_limits()
    vp_, split = VmBatchesCommitteePlan(), C.c_uint32(0)
    rc = lib().mbls_plan_verify_multiple_batches_committee_span(C.byref(L), n_sets, n_batches, sets_per_batch, table_size, max_groups, mode, 1 if locate else 0,
                                                                stride_words, split_mode, C.byref(vp_), C.byref(split))
    if rc != OK:
        raise MblsError(rc, "mbls_plan_verify_multiple_batches_committee_span")
    return {f: getattr(vp_, f) for f, _ in VmBatchesCommitteePlan._fields_}, int(split.value)


class CommitteeTable:
    """Resident table of committees over a KeyTable (include/mbls.h, mbls_committees_*): ordered member lists with their cached key sums; verify by
    committee id and participation bits. Destroy it before its key table."""

    def __init__(self, keytable, capacity_hint=0, ctx=None):
        self.ctx = ctx or keytable.ctx
        self.keytable = keytable
        self._h = vp()
        self.ctx.check(lib().mbls_committees_create(self.ctx.handle, keytable.handle, capacity_hint, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().mbls_committees_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return int(lib().mbls_committees_count(self._h))

    @property
    def max_members(self):
        """the size of the largest committee the table holds: 8 * bits_stride must cover it"""
        return int(lib().mbls_committees_max_members(self._h))

    def append(self, key_idx, offsets):
        """committees key_idx[offsets[c]:offsets[c+1]], c = 0 .. len(offsets) - 2 -> first_id"""
        if len(offsets) < 1:
            raise ValueError("offsets must have one entry more than there are committees (at least one)")
        first = C.c_uint64(0)
        idx = (C.c_uint32 * max(1, len(key_idx)))(*key_idx)
        off = (C.c_uint32 * len(offsets))(*offsets)
        self.ctx.check(lib().mbls_committees_append(self._h, idx, off, len(offsets) - 1, C.byref(first)))
        return int(first.value)

    def get(self, cid):
        """-> (the committee's full key sum as 96 uncompressed bytes, member count, eligible)"""
        out, m, el = outbuf(96), C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(lib().mbls_committees_get(self._h, cid, out, C.byref(m), C.byref(el)))
        return bytes(out)[:96], int(m.value), bool(el.value)

    def clear(self):
        """count back to 0 (blocks until everything enqueued over the table has finished); the next append starts at id 0"""
        self.ctx.check(lib().mbls_committees_clear(self._h))


class MultiContext:
    """Several GPUs behind one handle (include/mbls.h, mbls_multi_*): contiguous shards, one context and one host thread per device."""

    def __init__(self, device_ids):
        ids = (C.c_int * len(device_ids))(*device_ids)
        self._h = vp()
        rc = lib().mbls_multi_create(C.byref(self._h), ids, len(device_ids))
        if rc != OK:
            raise MblsError(rc, "mbls_multi_create failed")

    def close(self):
        if self._h:
            lib().mbls_multi_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return int(lib().mbls_multi_device_count(self._h))

    def check(self, rc):
        if rc != OK:
            raise MblsError(rc, lib().mbls_multi_last_error(self._h).decode())

    def reserve(self, n):
        self.check(lib().mbls_multi_reserve(self._h, n))

    @property
    def rccl_active(self):
        """True: the handle's exchange steps (accept bitmap, verify_multiple's partial records) are RCCL all-gathers between the devices"""
        return bool(lib().mbls_multi_rccl_active(self._h))

    @property
    def exchange_note(self):
        return lib().mbls_multi_exchange_note(self._h).decode()


class MultiKeyTable:
    """A key table replicated on every device of a MultiContext (same indices everywhere)."""

    def __init__(self, mctx, capacity_hint=0):
        self.m = mctx
        self._h = vp()
        mctx.check(lib().mbls_multi_keytable_create(mctx.handle, capacity_hint, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().mbls_multi_keytable_destroy(self._h)
            self._h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return int(lib().mbls_multi_keytable_size(self._h))

    def append(self, pks, n, pk_format=PK_COMPRESSED, validate=True):
        first = C.c_uint64(0)
        errs = outbuf(n)
        self.m.check(lib().mbls_multi_keytable_append(self._h, cbuf(pks), pk_format, int(validate), n, C.byref(first), errs))
        return int(first.value), list(bytes(errs)[:n])


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("MBLS_DEVICE", "0")))
    return _default_ctx


def cbuf(data):
    """bytes -> ctypes buffer (kept alive by the caller)."""
    data = bytes(data)
    return (C.c_uint8 * max(1, len(data))).from_buffer_copy(data if data else b"\0")


def outbuf(n):
    return (C.c_uint8 * max(1, n))()
