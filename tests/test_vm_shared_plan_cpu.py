"""mbls_plan_verify_multiple_shared_msgs through the built library (pure: no GPU): the route, the form of the list hash, the Miller items, the tree levels and the
workspace of the shared-message verify_multiple at every boundary -- n_msgs around the auto condition 2 n_msgs <= n, n around coop_max_items / 2, half a round,
a round and a round + 1 -- in the three grouping modes, against the rules as include/mbls.h states them."""
import ctypes as C

import pytest

from milagro_bls_amd import _native as N


def limits(round_items=65536):
    return N.default_limits(round_items)


def expect(L, n, M, mode):
    grouped = mode == 1 or (mode == 0 and 2 * M <= n)
    _mode, _passes, lst = N.plan_batch_shared_msgs(n, M, L)           # the list hash is the one the per-item shared-message entries plan
    items = (M or 1) if grouped else n
    e = dict(route=N.VM_ROUTE_GROUPED if grouped else N.VM_ROUTE_PER_SET, miller_items=items, **lst)
    e["tree_levels"] = (0 if n <= 1 else (n - 1).bit_length()) if grouped else 0
    sets = (max(n, items) + n) if grouped else n                      # sets and Miller items in front, the n positions behind both
    e["workspace_items"] = max(sets, lst["list_workspace_items"])
    e["chains_beside"] = int(2 * n <= L.round_items)
    e["sig_lane_pairs"] = int(2 * n <= L.coop_max_items)
    R = L.round_items
    if 2 * items <= L.coop_max_items:
        e.update(miller=N.PAIRING_WAVE, miller_rounds=0, miller_rest_items=items)
    else:
        full = (items // R) * R if items > R else 0
        rest = items - full
        e.update(miller=N.PAIRING_LANES2 if (rest and 2 * rest <= R) else N.PAIRING_LANE, miller_rounds=full // R, miller_rest_items=rest)
    return e


def sizes(L):
    base = [L.coop_max_items // 2, L.round_items // 2, L.round_items, L.round_items + 1]
    return sorted({b + d for b in base for d in (-1, 0, 1)} | {1, 2, 3})


@pytest.mark.parametrize("round_items", [65536, 64, 4096])
def test_plan_at_every_boundary(round_items):
    L = limits(round_items)
    seen = set()
    for n in sizes(L):
        for M in sorted({0, 1, n // 2, n // 2 + 1, n, n + 1}):
            for mode in (0, 1, 2):
                got = N.plan_verify_multiple_shared_msgs(n, M, mode, L)
                want = expect(L, n, M, mode)
                assert got == want, (n, M, mode, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
                assert N.plan_verify_multiple_shared_msgs_workspace_items(n, M, mode, L) == want["workspace_items"]
                seen.add((got["route"], got["miller"], got["chains_beside"], got["sig_lane_pairs"], got["miller_rounds"] > 0))
    # the boundaries are where the plan changes: both routes, all three Miller forms, both shapes of the chains, a Miller phase above a round
    # (a round of 64 lies below coop_max_items / 2: its Miller phases leave the waves only above a round, for whole rounds + a lane-pair remainder)
    assert {s[0] for s in seen} == {0, 1} and {s[1] for s in seen} == {N.PAIRING_WAVE, N.PAIRING_LANES2} | ({N.PAIRING_LANE} if round_items > 64 else set())
    assert {s[2] for s in seen} == {0, 1} and any(s[4] for s in seen)


def test_auto_condition_and_modes():
    L = limits()
    for n in (2, 3, 100, 101, 65536):
        assert N.plan_verify_multiple_shared_msgs(n, n // 2, 0, L)["route"] == N.VM_ROUTE_GROUPED
        assert N.plan_verify_multiple_shared_msgs(n, n // 2 + 1, 0, L)["route"] == N.VM_ROUTE_PER_SET
        assert N.plan_verify_multiple_shared_msgs(n, n + 1, 1, L)["route"] == N.VM_ROUTE_GROUPED
        assert N.plan_verify_multiple_shared_msgs(n, 1, 2, L)["route"] == N.VM_ROUTE_PER_SET
    # an empty list still walks one Miller item (infinite key, H of the empty message); more messages than sets put the positions behind the Miller items
    p = N.plan_verify_multiple_shared_msgs(10, 0, 1, L)
    assert p["miller_items"] == 1 and p["table_entries"] == 1 and p["list_pieces"] == 0 and p["workspace_items"] == 20
    assert N.plan_verify_multiple_shared_msgs(10, 13, 1, L)["workspace_items"] == 23
    # a list above a round is hashed in pieces of a round, and its Miller phase is cut at rounds
    p = N.plan_verify_multiple_shared_msgs(3 * 65536, 65536 + 100, 1, L)
    assert (p["list_pieces"], p["list_piece_items"], p["miller_rounds"], p["miller_rest_items"], p["miller"]) == (2, 65536, 1, 100, N.PAIRING_LANES2)


def test_refused_arguments():
    L = limits()
    out = N.VmSharedMsgsPlan()
    f = N.lib().mbls_plan_verify_multiple_shared_msgs
    assert f(C.byref(L), 0, 4, 0, C.byref(out)) == N.ERR_ARGUMENT
    assert f(C.byref(L), 8, 4, 3, C.byref(out)) == N.ERR_ARGUMENT
    assert f(C.byref(L), 8, 4, -1, C.byref(out)) == N.ERR_ARGUMENT
    assert f(None, 8, 4, 0, C.byref(out)) == N.ERR_ARGUMENT
    assert f(C.byref(L), 8, 4, 0, None) == N.ERR_ARGUMENT
    assert N.plan_verify_multiple_shared_msgs_workspace_items(0, 4, 0, L) == 0
    assert N.plan_verify_multiple_shared_msgs_workspace_items(8, 4, 7, L) == 0
