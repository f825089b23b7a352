"""The crafted states of the route batch (tests/route_states.py) without a device: every state's edge check, from the Python restatement alone; the
host referee frx_route_plan_levels_batch against the restatement on every state it accepts - every point bit for bit, every status, level count and offset
equal; the offsets that begin behind unused waypoints through the C entry; the neighbours of ends outside the map; and the refusals of the short and empty
routes that only the device form takes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import route_reference as rr  # noqa: E402
import route_states as rs  # noqa: E402

STATES = rs.all_states()
HOST = [s for s in STATES if not s.extra.get("device_only")]
DEVICE_ONLY = [s for s in STATES if s.extra.get("device_only")]


@pytest.mark.parametrize("s", STATES, ids=[s.label for s in STATES])
def test_every_state_sits_on_its_edge(s):
    s.check(s)


def test_the_sample_counts_cover_the_chunk_ends():
    """the counts are asserted edge by edge in the states' checks; here: that the set is the one the chunks of 64 ask for"""
    counts = {c for _, _, c in rs.SAMPLE_EDGES}
    assert {61, 63, 64, 65, 256} <= counts and any(c > 256 and c % rs.WAVE == 1 for c in counts)
    m = rr.Map((0.0, 0.0, 0.0), (16, 3, 3), 0.1, np.zeros(144, np.int8))
    a, b = rr.centre((1, 1, 1), m.origin, m.res), rr.centre((13, 1, 1), m.origin, m.res)
    assert rr.edge_samples(a, b) == 60 and round(1.2 / 0.02) + 1 == 61                              # the accumulation, not len / 0.02 + 1
    assert len(DEVICE_ONLY) == 2 and [s.extra["refused"] for s in DEVICE_ONLY] == [False, True]


def assert_equal(got, want, label):
    for k in ("route_status", "leg_status", "levels", "max_level_cells"):
        assert list(got[k]) == list(want[k]), (label, k, list(got[k]), list(want[k]))
    assert len(got["paths"]) == len(want["paths"])
    for r, (a, b) in enumerate(zip(got["paths"], want["paths"])):
        assert rr.same_bits(a, b), (label, "route", r)
    assert list(got["path_off"]) == [0] + list(np.cumsum([len(p) for p in want["paths"]])), label
    assert got["need"] == want["need"], label


@pytest.mark.parametrize("s", HOST, ids=[s.label for s in HOST])
def test_the_host_referee_equals_the_restatement(frx, s):
    vm = frx.VoxelMap(s.origin, s.dim, s.res, s.cells)
    want = rr.route_batch(rs.omap(s), s.routes, **s.caps)
    if "lead" in s.extra:
        off, pts = rs.pack(s)
        assert off[0] == s.extra["lead"] > 0
        rc, got = rs.c_batch(frx, vm, "frx_route_plan_levels_batch", off, pts, s.caps, want["need"])
        assert rc == 0
        assert rr.same_bits(got["path"], vm.route_batch_host(s.routes, **s.caps)["path"])           # and the same batch packed from 0
    else:
        got = vm.route_batch_host(s.routes, **s.caps)
        assert got["fits"] == (s.caps.get("cap_total") is None or want["need"] <= s.caps["cap_total"])
    assert_equal(got, want, s.label)


def test_the_neighbours_of_ends_outside_are_as_without_them(frx):
    s = next(s for s in STATES if "neighbours" in s.extra)
    vm = frx.VoxelMap(s.origin, s.dim, s.res, s.cells)
    got, alone = vm.route_batch_host(s.routes, **s.caps), vm.route_batch_host(s.extra["alone"], **s.caps)
    for k, r in s.extra["neighbours"].items():
        assert rr.same_bits(got["paths"][r], alone["paths"][k]) and got["route_status"][r] == 0
    bad = [r for r in range(len(s.routes)) if r not in s.extra["neighbours"].values()]
    assert sorted(int(v) for v in got["leg_status"] if v) == [rr.START] * len(bad) + [rr.GOAL] * len(bad)   # every end outside: status 1 or 2
    for r in bad:
        assert got["route_status"][r] == 1 and rr.same_bits(got["paths"][r], s.routes[r][[0, -1]])


@pytest.mark.parametrize("s", DEVICE_ONLY, ids=[s.label for s in DEVICE_ONLY])
def test_the_host_forms_refuse_short_and_empty_routes(frx, s):
    vm = frx.VoxelMap(s.origin, s.dim, s.res, s.cells)
    off, pts = rs.pack(s)
    for entry in ("frx_route_plan_levels_batch", "frx_route_plan_batch"):                           # the blocking form refuses before it looks for a device
        rc, got = rs.c_batch(frx, vm, entry, off, pts, s.caps, 4096)
        assert rc == -1 and b"fewer than 2 waypoints" in frx.lib().frx_last_error(), entry
        assert (got["route_status"] == -7).all() and (got["path_off"] == -7).all()                  # nothing written
    with pytest.raises(frx.FrxError) as e:
        vm.route_batch_host(s.routes, **s.caps)
    assert e.value.code == -1
