"""CPU checks of mbls_plan_verify_multiple_msgtable (include/mbls.h): the routing of verify_multiple over a resident message table as a pure function, at every
boundary of its rule -- bound = named when the host has counted the named entries, min(n, table size) otherwise; auto groups when 2 bound <= n;
miller_items = max(bound, 1); the Miller form follows miller_items; the workspace is what the call reserves."""
import pytest

from milagro_bls_amd import _native as N

P = N.plan_verify_multiple_msgtable
WS = N.plan_verify_multiple_msgtable_workspace_items
LWS = N.plan_verify_multiple_msgtable_locate_workspace_items


def levels(n):
    return 0 if n <= 1 else (n - 1).bit_length()


def model(L, n, T, named, mode):
    """the rule as include/mbls.h states it"""
    bound = named if named else min(n, T)
    grouped = True if mode == 1 else False if mode == 2 else 2 * bound <= n
    m = max(bound, 1) if grouped else n
    pbase = max(n, max(bound, 1))
    ws = pbase + n if grouped else n
    R = L.round_items
    if 2 * m <= L.coop_max_items:
        form, rounds, rest = N.PAIRING_WAVE, 0, m
    else:
        full = (m // R) * R if m > R else 0
        rest = m - full
        rounds = full // R
        form = N.PAIRING_LANES2 if rest and 2 * rest <= R else N.PAIRING_LANE
    return dict(route=N.VM_ROUTE_GROUPED if grouped else N.VM_ROUTE_PER_SET, miller_items=m, miller=form, miller_rounds=rounds, miller_rest_items=rest,
                tree_levels=levels(n) if grouped else 0, workspace_items=ws, chains_beside=1 if 2 * n <= R else 0, sig_lane_pairs=1 if 2 * n <= L.coop_max_items else 0,
                list_message=0, list_pieces=0, list_piece_items=0, list_workspace_items=0, table_entries=0), (ws + (2 * n if grouped else n))


def check(L, n, T, named, mode):
    want, lws = model(L, n, T, named, mode)
    got = P(n, T, named, mode, limits=L)
    assert got == want, (n, T, named, mode, got, want)
    assert WS(n, T, named, mode, limits=L) == want["workspace_items"]
    assert LWS(n, T, named, mode, limits=L) == lws
    return got


def test_auto_condition_on_both_sides():
    L = N.default_limits()
    # 2 bound == n groups, 2 bound == n + 1 does not -- through the table's size (device entries) and through the count (host entries)
    assert check(L, 150, 75, 0, 0)["route"] == N.VM_ROUTE_GROUPED
    assert check(L, 149, 75, 0, 0)["route"] == N.VM_ROUTE_PER_SET
    assert check(L, 150, 5000, 75, 0)["route"] == N.VM_ROUTE_GROUPED
    assert check(L, 149, 5000, 75, 0)["route"] == N.VM_ROUTE_PER_SET
    # the bound of a device entry is min(n, T): a table smaller than the call bounds it
    assert check(L, 150, 12, 0, 0)["miller_items"] == 12
    assert check(L, 10, 12, 0, 0)["route"] == N.VM_ROUTE_PER_SET


def test_named_not_known_against_counted_in_a_large_table():
    """T >> n: the device form cannot know that few entries are named and goes per set; the host form has counted them and groups"""
    L = N.default_limits()
    dev = check(L, 150, 2500, 0, 0)
    host = check(L, 150, 2500, 9, 0)
    assert dev["route"] == N.VM_ROUTE_PER_SET and dev["miller_items"] == 150 and dev["workspace_items"] == 150
    assert host["route"] == N.VM_ROUTE_GROUPED and host["miller_items"] == 9 and host["workspace_items"] == 300
    forced = check(L, 150, 2500, 0, 1)
    assert forced["route"] == N.VM_ROUTE_GROUPED and forced["miller_items"] == 150 and forced["workspace_items"] == 300
    big = check(L, 1 << 16, 1 << 16, 512, 0)
    assert big["route"] == N.VM_ROUTE_GROUPED and big["miller_items"] == 512
    assert check(L, 1 << 16, 1 << 16, 0, 0)["route"] == N.VM_ROUTE_PER_SET


def test_miller_form_follows_the_miller_items():
    L = N.default_limits()
    L.coop_max_items = 40
    L.round_items = 100
    n = 1000
    assert check(L, n, 5000, 20, 1)["miller"] == N.PAIRING_WAVE                  # 2 m == coop_max_items
    p = check(L, n, 5000, 21, 1)                                                 # 2 m == coop_max_items + 2: lane pairs (half a round or less)
    assert p["miller"] == N.PAIRING_LANES2 and p["miller_rounds"] == 0 and p["miller_rest_items"] == 21
    assert check(L, n, 5000, 50, 1)["miller"] == N.PAIRING_LANES2                # 2 m == round
    assert check(L, n, 5000, 51, 1)["miller"] == N.PAIRING_LANE                  # above half a round: one lane per pair
    p = check(L, n, 5000, 100, 1)                                                # exactly a round: not cut
    assert p["miller_rounds"] == 0 and p["miller_rest_items"] == 100 and p["miller"] == N.PAIRING_LANE
    p = check(L, n, 5000, 101, 1)                                                # one past a round: the round, then one item on a lane pair
    assert p["miller_rounds"] == 1 and p["miller_rest_items"] == 1 and p["miller"] == N.PAIRING_LANES2
    p = check(L, n, 5000, 0, 2)                                                  # per set: the sets are the Miller items
    assert p["miller_items"] == n and p["miller_rounds"] == 10 and p["miller_rest_items"] == 0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_modes_and_edges(mode):
    L = N.default_limits()
    for n, T, named in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (7, 0, 0), (150, 1, 0), (150, 150, 0), (150, 600, 5), (33, 2500, 33), (4096, 1 << 20, 64)):
        p = check(L, n, T, named, mode)
        assert p["route"] == (N.VM_ROUTE_GROUPED if mode == 1 else N.VM_ROUTE_PER_SET if mode == 2 else p["route"])
        assert p["miller_items"] >= 1


def test_refused_arguments():
    L = N.default_limits()
    with pytest.raises(N.MblsError):
        P(0, 10, 0, 0, limits=L)
    with pytest.raises(N.MblsError):
        P(10, 10, 0, 3, limits=L)
    assert WS(0, 10, 0, 0, limits=L) == 0 and LWS(10, 10, 0, 5, limits=L) == 0
