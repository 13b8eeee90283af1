"""The routing of the shared-message entries as data (include/mbls.h: mbls_plan_batch_shared_msgs, mbls_plan_shared_msgs_workspace_items -- pure functions, no GPU):
the items' plan is mbls_plan_batch's with every message phase a gather, and the list is hashed in the form ITS size asks for. The entries act on the same function
(verify_device calls plan_shared), so what is asserted here is what the GPU runs; tests/test_gpu_shared_msgs.py compares results."""
import pytest

from milagro_bls_amd import _native as N

R = 65536
FIELDS = ("first_item", "items", "workspace_first", "workspace_items", "track", "stage", "pairing", "front", "sig_subgroup_from_miller_loop")


def shared(n, n_msgs, L=None):
    mode, passes, lst = N.plan_batch_shared_msgs(n, n_msgs, L)
    mode0, passes0 = N.plan_batch(n, L)
    # the items' plan: mbls_plan_batch's own, field by field, except the message phase
    assert mode == mode0 and len(passes) == len(passes0)
    for p, q in zip(passes, passes0):
        assert [p[f] for f in FIELDS] == [q[f] for f in FIELDS]
        assert p["message"] == N.MESSAGE_GATHER and q["message"] != N.MESSAGE_GATHER
    assert lst["table_entries"] == n_msgs + 1
    return mode, passes, lst


@pytest.mark.parametrize("n_msgs,form,pieces,piece,ws", [
    (1, N.MESSAGE_WAVE, 1, 1, 1),
    (768, N.MESSAGE_WAVE, 1, 768, 768),                  # coop_hash_pack_min_items: still one message per wave
    (769, N.MESSAGE_WAVE_X4, 1, 769, 769),
    (3584, N.MESSAGE_WAVE_X4, 1, 3584, 3584),            # coop_hash_max_items: the wave engine's last size
    (3585, N.MESSAGE_LANES2, 1, 3585, 2 * 3585),         # above it: lane pairs, two workspace items per message
    (20480, N.MESSAGE_LANES2, 1, 20480, 2 * 20480), (20481, N.MESSAGE_LANE, 1, 20481, 20481),
    (R, N.MESSAGE_LANE, 1, R, R),                        # n_msgs = n: today's k_hash, plus export and gather
])
def test_list_hash_of_a_full_round_of_items(n_msgs, form, pieces, piece, ws):
    mode, passes, lst = shared(R, n_msgs)
    assert mode == N.BATCH_ONE_PASS and passes[0]["pairing"] == N.PAIRING_LANE
    assert (lst["list_message"], lst["list_pieces"], lst["list_piece_items"], lst["list_workspace_items"]) == (form, pieces, piece, ws)
    # the call reserves the larger of the items' plan and the list's items
    assert N.plan_shared_msgs_workspace_items(R, n_msgs, 128) == max(R, ws)


def test_the_form_follows_the_list_not_the_items():
    for n in (1, 3, 130, 5121, 40000, R, R + 1, 73728, 3 * R):
        assert shared(n, 300)[2]["list_message"] == N.MESSAGE_WAVE
        assert shared(n, 30000)[2]["list_message"] == N.MESSAGE_LANE
    # more messages than items: the workspace follows the list
    assert N.plan_shared_msgs_workspace_items(3, 70, 2) == 70 and N.plan_workspace_items(3, 2) == 3
    assert N.plan_shared_msgs_workspace_items(3, 70, 128) == 70 and N.plan_shared_msgs_workspace_items(10, 70, 128) == 90     # eight-lane key sum: 9 n items
    # an empty list: nothing to hash, only the empty message's entry
    lst = shared(5, 0)[2]
    assert (lst["list_message"], lst["list_pieces"], lst["list_piece_items"], lst["list_workspace_items"], lst["table_entries"]) == (0, 0, 0, 0, 1)


def test_lists_above_a_round_are_hashed_in_pieces_of_a_round():
    lst = shared(10, R + 1)[2]
    assert (lst["list_message"], lst["list_pieces"], lst["list_piece_items"], lst["list_workspace_items"]) == (N.MESSAGE_LANE, 2, R, R)
    lst = shared(10, 3 * R)[2]
    assert (lst["list_pieces"], lst["list_piece_items"]) == (3, R)
    L = N.default_limits(64)                                # what the GPU test with rounds of 64 sees: 70 messages = 64 + 6
    lst = shared(3, 70, L)[2]
    assert (lst["list_message"], lst["list_pieces"], lst["list_piece_items"], lst["list_workspace_items"]) == (N.MESSAGE_WAVE, 2, 64, 64)
    L.coop_max_items = 0; L.coop_hash_max_items = 0         # the 'lanes' engine: 2 x 64 lanes would be two rounds, so one lane per message
    lst = shared(3, 70, L)[2]
    assert (lst["list_message"], lst["list_pieces"], lst["list_workspace_items"]) == (N.MESSAGE_LANE, 2, 64)


def test_plans_of_several_passes_gather_in_every_pass():
    mode, ps, lst = shared(65537, 300)
    assert mode == N.BATCH_ROUNDS_THEN_REST and [(p["first_item"], p["items"]) for p in ps] == [(0, R), (R, 1)]
    mode, ps, lst = shared(73728, 300)
    assert mode == N.BATCH_ROUND_BESIDE_REST and [(p["first_item"], p["items"], p["track"], p["workspace_first"]) for p in ps] == [(0, R, 0, 0), (R, 8192, 1, R)]
    assert lst["list_message"] == N.MESSAGE_WAVE and lst["list_workspace_items"] == 300
    assert N.plan_shared_msgs_workspace_items(73728, 300, 128) == N.plan_workspace_items(73728, 128) == R + 2 * 8192
    mode, ps, lst = shared(100000, 4096)
    assert mode == N.BATCH_TWO_HALVES and lst["list_message"] == N.MESSAGE_LANES2


def test_argument_errors():
    import ctypes as C
    L = N.default_limits(R); sp = N.SharedMsgsPlan()
    assert N.lib().mbls_plan_batch_shared_msgs(C.byref(L), 0, 5, C.byref(sp)) == N.ERR_ARGUMENT
    assert N.lib().mbls_plan_batch_shared_msgs(None, 5, 5, C.byref(sp)) == N.ERR_ARGUMENT
    assert N.lib().mbls_plan_batch_shared_msgs(C.byref(L), 5, 5, None) == N.ERR_ARGUMENT
    assert N.plan_shared_msgs_workspace_items(0, 5, 2) == 0


# mbls_plan_batch itself is unchanged: the rows of tests/test_plan_cpu.py's table (n, pairing, message, front, workspace items per item), as literals
PLAN_BATCH_TABLE = [
    (1, 0, 3, 2, 1), (768, 0, 3, 2, 1), (769, 0, 4, 2, 1), (1024, 0, 4, 2, 1), (1025, 5, 4, 2, 1), (2048, 5, 4, 2, 1), (2049, 0, 4, 2, 1), (3584, 0, 4, 2, 1),
    (3585, 0, 2, 2, 2), (5120, 0, 2, 2, 2), (5121, 4, 2, 2, 2), (16384, 4, 2, 2, 2), (16385, 2, 2, 1, 2), (20480, 2, 2, 1, 2), (20481, 2, 1, 1, 2), (32768, 2, 1, 1, 2),
    (32769, 1, 1, 1, 1), (49152, 1, 1, 1, 1), (49153, 1, 1, 0, 1), (65536, 1, 1, 0, 1), (131072, 1, 1, 0, 1),
]


def test_plan_batch_is_what_it_was():
    import ctypes as C
    for n, pairing, message, front, ws in PLAN_BATCH_TABLE:
        mode, ps = N.plan_batch(n)
        assert mode == N.BATCH_ONE_PASS and len(ps) == 1
        p = ps[0]
        assert (p["first_item"], p["items"], p["workspace_first"], p["workspace_items"], p["track"], p["stage"]) == (0, n, 0, ws * n, 0, 0)
        assert (p["pairing"], p["message"], p["front"], p["sig_subgroup_from_miller_loop"]) == (pairing, message, front, 1 if n > 5120 else 0)
    # the structure keeps its size and layout (the new plan embeds it): 8 + 3 x 56 bytes, unused passes zeroed
    assert C.sizeof(N.BatchPlan) == 176 and C.sizeof(N.PassPlan) == 56
    b = N.BatchPlan(); C.memset(C.byref(b), 0xFF, C.sizeof(b))
    L = N.default_limits(R)
    assert N.lib().mbls_plan_batch(C.byref(L), R + 3584, C.byref(b)) == N.OK
    raw = bytes(b)
    assert raw[8 + 2 * 56:] == bytes(56)
    want = [(0, R, 0, R, 0, 0, 1, 1, 0, 1), (R, 3584, R, 7168, 1, 0, 4, 2, 2, 1)]
    got = [tuple(getattr(b.passes[i], f) for f, _ in N.PassPlan._fields_) for i in range(2)]
    assert (b.mode, b.n_passes, got) == (N.BATCH_ROUND_BESIDE_REST, 2, want)
