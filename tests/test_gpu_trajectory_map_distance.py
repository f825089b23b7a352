"""frx_trajectory_map_distance on the device against the numpy restatement (tests/map_distance_reference.py): all four fields exactly on every piece the
restatement calls decision-safe (at least 95 % of them), the crafted cases, bit identity between the device form, the blocking form and a replayed graph, both
kinds of handle, and the loop it closes with frx_trajectory_clearance on a field that frx_map_esdf_device built from a marked cloud."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_states as cs  # noqa: E402
import map_distance_reference as mr  # noqa: E402
from test_gpu_trajectory_sample import DevBuf, hip  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
PAD = 64
LAYOUTS = [(1,), (7,), (8, 9), (65, 1, 7)]
INTERVALS = (1, 5, 64, 65)                                                # M + 1 = 2, 6, a wave + 1, a wave + 2 samples
# the Zhangjiajie volume x in [-35, 35], y in [-10, 390], z in [0, 2.8] (scenario.make_gates) with a margin, at half a metre: about a million cells
ORIGIN, DIM, RES = (-40.13, -15.21, -0.67), (160, 820, 8), 0.5           # (an origin that puts no round coordinate on a cell border)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def pool(frx, sc):
    """130 pieces of two candidates at the initial guess, the map, a field with ties in it, and the restatement's rows per M: computed once, shared, unchanged"""
    cands = sc.make_batch(0, 2, 65, 16)
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=8)
    T, Cf = prob.forward(prob.initial_guess())
    T = np.array(T, dtype=np.float64); Cf = np.array(Cf, dtype=np.float64).reshape(-1, 3)
    vmap = frx.VoxelMap(ORIGIN, DIM, RES)
    rng = np.random.default_rng(11)
    field = rng.integers(0, 24, vmap.cells.size) / 8.0                    # few values: equal minima along a piece, the lower j must win
    ref = {}
    for M in INTERVALS:
        rows, safe = mr.pieces(T, Cf, M, ORIGIN, DIM, RES, field)
        rows.setflags(write=False); safe.setflags(write=False)
        ref[M] = (rows, safe)
        print(f"M = {M}: {safe.sum()} of {len(safe)} pieces decision-safe")
        assert safe.mean() >= 0.95, (M, safe.mean())                      # the restatement alone: at most 5 % of the pieces are left out
    for a in (T, Cf, field):
        a.setflags(write=False)
    yield dict(prob=prob, T=T, Cf=Cf, vmap=vmap, field=field, ref=ref)
    prob.close()


def device_rows(frx, prob, T, Cf, vmap, field, M, stream=0, launch=None):
    P = prob.P
    host = np.full(4 * P + PAD, SENTINEL)
    bufs = [DevBuf(np.ascontiguousarray(T)), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(np.ascontiguousarray(field)), DevBuf(host)]
    try:
        def call():
            prob.trajectory_map_distance_device(bufs[0].p, bufs[1].p, vmap.device_struct(), bufs[2].p, bufs[3].p, M, stream)
        (launch or (lambda f: f()))(call)
        got = bufs[3].get(host)
        assert (got[4 * P:] == SENTINEL).all()
        return got[:4 * P].reshape(-1, 4)
    finally:
        for d in bufs:
            d.close()


def assert_rows(got, rows, safe, T, off, margin):
    assert same(got["piece"][safe], rows[safe]), np.argwhere(bits(got["piece"]) != bits(rows))[:8]
    assert safe.mean() >= 0.95, safe.mean()
    mine = mr.fold(got["piece"], T, off, margin)                          # the host fold, from the device's own rows: exact
    assert same(got["cand"], mine[0]) and np.array_equal(got["flags"], mine[1])


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda n: "P%d" % sum(n))
def test_exact_on_ragged_batches(frx, sc, pool, layout):
    P = sum(layout)
    T, Cf = pool["T"][:P], pool["Cf"][:6 * P]
    off = np.concatenate([[0], np.cumsum(layout)])
    prob = cs.handle(frx, dict(sc.ZHANGJIAJIE), list(layout))
    try:
        for M in INTERVALS:
            rows, safe = pool["ref"][M]
            rows, safe = rows[:P], safe[:P]
            got = prob.trajectory_map_distance(T, Cf, pool["vmap"], pool["field"], margin=0.5, intervals=M)
            assert got["piece"].shape == (P, 4) and got["cand"].shape == (len(layout), 4) and got["flags"].dtype == np.uint32
            assert np.array_equal(got["dist"], got["cand"][:, 0]) and np.array_equal(got["outside"], got["cand"][:, 3])
            assert_rows(got, rows, safe, T, off, 0.5)
            dev = device_rows(frx, prob, T, Cf, pool["vmap"], pool["field"], M)
            assert same(dev, got["piece"])
            again = prob.trajectory_map_distance(T, Cf, pool["vmap"], pool["field"], margin=0.5, intervals=M)
            assert same(again["piece"], got["piece"]) and same(again["cand"], got["cand"])
    finally:
        prob.close()


def test_a_handle_with_variables_and_pieces_in_other_batches(frx, pool):
    """frx_problem_create's handle serves the screen too, and a piece's row does not depend on the batch around it"""
    M = 65
    rows, safe = pool["ref"][M]
    got = pool["prob"].trajectory_map_distance(pool["T"], pool["Cf"], pool["vmap"], pool["field"], margin=1.0, intervals=M)
    assert_rows(got, rows, safe, pool["T"], list(pool["prob"].piece_off), 1.0)
    assert same(device_rows(frx, pool["prob"], pool["T"], pool["Cf"], pool["vmap"], pool["field"], M), got["piece"])


def test_graph_replay_is_bit_identical(frx, sc, pool):
    P = 17
    T, Cf = pool["T"][:P], pool["Cf"][:6 * P]
    prob = cs.handle(frx, dict(sc.ZHANGJIAJIE), [8, 9])
    H = hip()
    st, graph, exe, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
    assert H.hipStreamCreate(C.byref(st)) == 0
    try:
        want = prob.trajectory_map_distance(T, Cf, pool["vmap"], pool["field"], intervals=64)["piece"]

        def launch(call):
            assert H.hipStreamBeginCapture(st, 0) == 0
            call()
            assert H.hipStreamEndCapture(st, C.byref(graph)) == 0
            assert H.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 1
            assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
            for _ in range(2):
                assert H.hipGraphLaunch(exe, st) == 0 and H.hipStreamSynchronize(st) == 0
        assert same(device_rows(frx, prob, T, Cf, pool["vmap"], pool["field"], 64, stream=st.value, launch=launch), want)
        assert same(device_rows(frx, prob, T, Cf, pool["vmap"], pool["field"], 64, stream=st.value), want)
    finally:
        if exe.value:
            H.hipGraphExecDestroy(exe)
        if graph.value:
            H.hipGraphDestroy(graph)
        H.hipStreamDestroy(st)
        prob.close()


def test_crafted_cases(frx, sc):
    """A small map over [0, 4) x [0, 2) x [0, 1) at a quarter of a metre; straight pieces along x at the centre of a row of cells, so every cell is known"""
    vmap = frx.VoxelMap([0.0, 0.0, 0.0], (16, 8, 4), 0.25)
    field = (np.arange(vmap.cells.size) % 7 + 1).astype(np.float64)
    y, z = 0.875, 0.375                                                   # cells cy = 3, cz = 1: dyadic, the centres of their cells
    inside = cs.line_piece((0.125, y, z), (3.875, y, z), 1.0)             # samples at the centres of 16 cells for M = 15
    outside = cs.line_piece((5.125, y, z), (9.125, y, z), 1.0)               # wholly outside
    crossing = cs.line_piece((3.125, y, z), (4.875, y, z), 1.0)           # M = 7: cells 12..15, then four samples outside
    bad = inside.copy(); bad[5, 1] = np.nan                               # a NaN coefficient: every sample is not a number, so outside
    T = np.ones(4)
    Cf = np.concatenate([inside, outside, crossing, bad])
    prob = cs.handle(frx, dict(sc.ZHANGJIAJIE), [1, 1, 1, 1])
    try:
        base = 16 * (3 + 8 * 1)
        got = prob.trajectory_map_distance(T, Cf, vmap, field, margin=1.5, intervals=15)
        ref, safe = mr.pieces(T, Cf, 15, vmap.origin, vmap.dim, vmap.res, field)
        assert safe.all() and same(got["piece"], ref)
        f = field[base:base + 16]
        j = int(np.argmin(f))                                             # the first of the equal minima
        assert tuple(got["piece"][0]) == (f.min(), (1.0 / 15) * j, float(base + j), 0.0)
        assert tuple(got["piece"][1]) == (np.inf, -1.0, -1.0, 16.0) and tuple(got["piece"][3]) == (np.inf, -1.0, -1.0, 16.0)
        assert got["flags"][0] == frx.MAPDIST_FLAG_BELOW and got["flags"][1] == got["flags"][3] == frx.MAPDIST_FLAG_OUTSIDE | frx.MAPDIST_FLAG_NONFINITE
        got7 = prob.trajectory_map_distance(T, Cf, vmap, field, margin=0.0, intervals=7)
        f = field[base + 12:base + 16]
        assert tuple(got7["piece"][2]) == (f.min(), (1.0 / 7) * int(np.argmin(f)), float(base + 12 + int(np.argmin(f))), 4.0)
        assert got7["flags"][2] == frx.MAPDIST_FLAG_OUTSIDE
        # a NaN field value beats every number, the first of two wins, and it reaches the candidate and its flag
        fn = field.copy(); fn[base + 9] = np.nan; fn[base + 4] = np.nan
        gn = prob.trajectory_map_distance(T, Cf, vmap, fn, margin=0.0, intervals=15)
        assert np.isnan(gn["piece"][0, 0]) and tuple(gn["piece"][0, 1:]) == ((1.0 / 15) * 4, float(base + 4), 0.0)
        assert gn["flags"][0] == frx.MAPDIST_FLAG_NONFINITE and same(gn["piece"][1:], got["piece"][1:])
        assert same(device_rows(frx, prob, T, Cf, vmap, fn, 15), gn["piece"])
        # candidates without pieces, first, in the middle and last: the device form's rows through the fold
        rows = device_rows(frx, prob, T, Cf, vmap, field, 15)
        off = [0, 0, 2, 2, 4, 4]
        cand, flags = frx.map_distance_fold(rows, T, off, 1.5)
        rc, rf = mr.fold(rows, T, off, 1.5)
        assert same(cand, rc) and np.array_equal(flags, rf) and flags[0] == flags[2] == flags[4] == 0 and (cand[[0, 2, 4]] == 0).all()
        assert tuple(cand[1, :3]) == tuple(got["piece"][0, :3]) and cand[1, 3] == 16.0                 # the first piece wins, OUTSIDE is summed
        assert tuple(cand[3, :3]) == tuple(got["piece"][2, :3]) and cand[3, 3] == got["piece"][2, 3] + 16.0
    finally:
        prob.close()


def test_closing_the_loop_with_the_clearance(frx, sc):
    """The map is marked from a cloud on the device, pos comes from frx_map_esdf_device, every sample lies inside the map: per piece the screen's DIST and the
    clearance's FRX_CLEAR_DIST at the same M differ by at most sqrt(3) res + 1e-9 - a sample and a cloud point each lie within (sqrt(3) / 2) res of their
    cell's centre, and pos is the distance between those centres."""
    rng = np.random.default_rng(21)
    origin, dim, res = (-1.0, -2.0, 0.0), (60, 40, 20), 0.25              # 15 x 10 x 5 m
    lo, hi = np.array(origin), np.array(origin) + res * np.array(dim)
    obs = rng.uniform(lo + 1e-6, hi - 1e-6, (500, 3))
    P, M = 12, 32
    way = rng.uniform(lo + 0.5, hi - 0.5, (P + 1, 3))
    T = rng.uniform(0.8, 2.0, P)
    Cf = np.concatenate([cs.line_piece(way[k], way[k + 1], T[k]) for k in range(P)])
    vmap = frx.VoxelMap(origin, dim, res)
    n = vmap.cells.size
    bufs = dict(cells=DevBuf(np.zeros(n, np.int8)), pts=DevBuf(obs.reshape(-1)), cnt=DevBuf(np.zeros(1, np.int32)),
                work=DevBuf(np.zeros(frx.map_esdf_workspace(dim) // 4, np.int32)), pos=DevBuf(np.zeros(n)), T=DevBuf(T), C=DevBuf(Cf.reshape(-1)), rows=DevBuf(np.zeros(4 * P)))
    params = dict(sc.ZHANGJIAJIE)
    params.update(cs.LOOSE)
    prob = cs.handle(frx, params, [P])
    try:
        ms = vmap.device_struct(bufs["cells"].p)
        frx.map_mark_cloud_device(ms, bufs["cells"].p, len(obs), bufs["pts"].p, bufs["cnt"].p)
        frx.map_esdf_device(ms, bufs["pos"].p, 0, 0, bufs["work"].p)
        prob.trajectory_map_distance_device(bufs["T"].p, bufs["C"].p, ms, bufs["pos"].p, bufs["rows"].p, M)
        rows = bufs["rows"].get(np.zeros(4 * P)).reshape(-1, 4)
        assert int(bufs["cnt"].get(np.zeros(1, np.int32))[0]) == len(obs)
        assert (rows[:, 3] == 0).all() and np.isfinite(rows).all()
        clear = prob.trajectory_clearance(T, Cf, obs, M)["piece"]
        gap = np.abs(clear[:, 1] - rows[:, 0])
        print(f"closing the loop: largest |CLEAR_DIST - DIST| {gap.max():.4f} m, bound {np.sqrt(3.0) * res + 1e-9:.4f} m")
        assert (gap <= np.sqrt(3.0) * res + 1e-9).all(), (gap, clear[:, 1], rows[:, 0])
        # and the blocking form on the downloaded field gives the device form's bits
        pos = bufs["pos"].get(np.zeros(n))
        assert same(prob.trajectory_map_distance(T, Cf, vmap, pos, intervals=M)["piece"], rows)
    finally:
        prob.close()
        for d in bufs.values():
            d.close()
