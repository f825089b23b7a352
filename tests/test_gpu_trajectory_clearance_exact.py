"""frx_trajectory_clearance_exact on the device: bit for bit against the float64 restatement (tests/clear_exact_reference.py) for ragged batches and clouds
each side of a wave and of a chunk; the same bits under every packing (chunk size, cull on or off, the forms, a graph replay, the batch, the kind of handle);
the crafted states of tests/clear_exact_states.py; the collision the dense form steps over; the dense form at 256 and 16 384 intervals; the cull's counts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_exact_reference as cx  # noqa: E402
import clear_exact_states as xs  # noqa: E402
import clear_reference as clr  # noqa: E402
from test_gpu_trajectory_check import TOL  # noqa: E402
from test_gpu_trajectory_contain import DevBuf, differ, offsets, penalty_handle, same  # noqa: E402
from test_gpu_trajectory_sample import hip  # noqa: E402

pytestmark = pytest.mark.gpu

KAPPA = 16
# pieces per candidate x the clouds every batch meets: 1, 63, 64, 65 (each side of a wave), 129 (two tiles and one point), 1025 (one point into a second chunk)
CLOUDS = (1, 63, 64, 65, 129, 1025)
CASES = [((1,), CLOUDS), ((7,), CLOUDS), ((8, 9), CLOUDS), ((65, 1, 7), CLOUDS)]
SENTINEL = -7.0
_REF = {}


@pytest.fixture(scope="module")
def pool(frx, sc):
    """130 pieces of two candidates at the initial guess and after about 30 iterations, with their corridor cells: computed once, shared, left unchanged"""
    params = sc.ZHANGJIAJIE
    cands = sc.make_batch(0, 2, 65, 16)
    prob = frx.Problem(cands, params, qd_intervals=KAPPA)
    assert prob.P == prob.Pc == 130
    polys = [h for c in cands for h in c.h_polys]
    x0 = prob.initial_guess()
    T0, C0 = prob.forward(x0)
    res = prob.optimize(params["opt_rel_tol"], x0=x0, max_iterations=30)
    states = {}
    for name, (T, Cf) in (("initial", (T0, C0)), ("optimised", (res["T"], res["C"]))):
        T = np.array(T, dtype=np.float64); Cf = np.array(Cf, dtype=np.float64).reshape(-1, 3)
        T.setflags(write=False); Cf.setflags(write=False)
        states[name] = (T, Cf)
    yield prob, cands, polys, states
    prob.close()


def reference(states, state, P, n_obs, params):
    """(T, Cf, cloud, rows) of the pool's first P pieces against n_obs points near their paths: the restatement, computed once per (state, P, n_obs)"""
    key = (state, P, n_obs)
    if key not in _REF:
        T, Cf = np.ascontiguousarray(states[state][0][:P]), np.ascontiguousarray(states[state][1][:6 * P])
        cloud = xs.near_cloud(np.random.default_rng(1000 * P + n_obs), T, Cf, n_obs)
        counts = []
        ref = cx.rows(T, Cf, cloud, params, True, counts)
        assert (np.array(counts)[:, 0] >= 1).all()                      # survivors exist
        for a in (T, Cf, cloud, ref):
            a.setflags(write=False)
        _REF[key] = (T, Cf, cloud, ref)
    return _REF[key]


def assert_rows(got, ref, T, piece_off):
    bad = differ(got["piece"], ref)
    assert len(bad) == 0, (bad[:8], got["piece"][bad[:4, 0]], ref[bad[:4, 0]])
    cref = cx.reduce_candidates(ref, T, piece_off)
    assert same(got["cand"], cref), (got["cand"], cref)
    assert np.array_equal(got["flags"], cx.flags_of(cref, piece_off)), (got["flags"], cx.flags_of(cref, piece_off))


def device_rows(h, T, Cf, obs, force=0, stream=0, launch=None):
    """The piece rows of the device form; rows and workspace are pre-filled with a sentinel and nothing is written behind either at the size the workspace
    query reports.  launch(call) runs the enqueueing call (default: directly)."""
    P, n = h.P, len(obs)
    nbytes = h.trajectory_clearance_exact_workspace(n)
    assert nbytes == xs.workspace_bytes(P, n, force) and nbytes > 0, (nbytes, P, n, force)
    host = np.full(P * 6 + 64, SENTINEL); whost = np.full(nbytes // 8 + 64, SENTINEL)
    bufs = [DevBuf(np.ascontiguousarray(T)), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(np.ascontiguousarray(obs).reshape(-1)), DevBuf(whost), DevBuf(host)]
    try:
        def call():
            h.trajectory_clearance_exact_device(bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value, n, bufs[3].ptr.value, bufs[4].ptr.value, stream)
        (launch or (lambda f: f()))(call)
        got, work = bufs[4].get(host), bufs[3].get(whost)
        assert (got[P * 6:] == SENTINEL).all() and (work[nbytes // 8:] == SENTINEL).all()
        counts = h.clear_exact_counts()                                  # (the workspace is still alive)
        return got[:P * 6].reshape(-1, 6), counts
    finally:
        for d in bufs:
            d.close()


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_bit_identical_to_the_restatement_for_ragged_batches(frx, sc, pool, state):
    """batches of 1, 7, 8 + 9 and 65 + 1 + 7 pieces against clouds of 1 .. 1025 points within 2 m of their paths"""
    params = sc.ZHANGJIAJIE
    _, _, polys, states = pool
    for piece_n, clouds in CASES:
        P = sum(piece_n)
        h = penalty_handle(frx, sc, piece_n, polys[:P])
        try:
            for n_obs in clouds:
                T, Cf, cloud, ref = reference(states, state, P, n_obs, params)
                got = h.trajectory_clearance_exact(T, Cf, cloud)
                assert got["piece"].shape == (P, 6) and got["cand"].shape == (len(piece_n), 6) and got["flags"].dtype == np.uint32
                assert_rows(got, ref, T, offsets(piece_n))
                assert np.array_equal(got["ell"], got["cand"][:, 0]) and np.array_equal(got["i_dist"], got["cand"][:, 5])
                surv, ell = h.clear_exact_counts()
                assert (surv >= 1).all() and (ell >= 1).all() and (ell <= surv).all() and (surv <= n_obs).all(), (piece_n, n_obs, surv, ell)
        finally:
            h.close()


@pytest.mark.parametrize("state", ["initial", "optimised"])
def test_every_packing_gives_the_same_bits(frx, sc, pool, state):
    """chunks of 64 and 128 points, the cull on or off, the blocking and the device form, a replay in a captured graph, a candidate alone or in the batch, a
    planning handle or a penalty handle: the restatement's bits every time"""
    params = sc.ZHANGJIAJIE
    prob, cands, polys, states = pool
    piece_n = (8, 9)
    P, n_obs = 17, 129
    T, Cf, cloud, ref = reference(states, state, P, n_obs, params)
    off = offsets(piece_n)
    h = penalty_handle(frx, sc, piece_n, polys[:P])
    try:
        want = h.trajectory_clearance_exact(T, Cf, cloud)
        assert_rows(want, ref, T, off)
        base = h.clear_exact_counts()
        # (chunks of 1 point: 129 chunks a piece, so the lanes that read the chunks' bounds and fold their partials take a second stride)
        for chunk, cull in ((64, True), (128, True), (1, True), (0, False), (64, False), (128, False)):
            h.set_clear_exact(chunk, cull)
            assert xs.chunks(P, n_obs, chunk)[1] == (1 if chunk == 0 else -(-n_obs // chunk))
            got = h.trajectory_clearance_exact(T, Cf, cloud)
            assert same(got["piece"], want["piece"]) and same(got["cand"], want["cand"]) and np.array_equal(got["flags"], want["flags"]), (chunk, cull)
            surv, ell = h.clear_exact_counts()
            if not cull:
                assert (surv == n_obs).all() and (ell == n_obs).all()   # every point a survivor, every task run
            dev, counts = device_rows(h, T, Cf, cloud, chunk)
            assert same(dev, want["piece"]), (chunk, cull)
            assert np.array_equal(counts[0], surv) and np.array_equal(counts[1], ell)
            cand, flags = frx.clearance_exact_fold(dev, T, off)
            assert same(cand, want["cand"]) and np.array_equal(flags, want["flags"])
        assert (base[0] < n_obs).any()                                   # the cull left points out
        # a replay in a captured graph: three kernel nodes when the cloud is split, two when it is not
        H = hip()
        for chunk, nodes in ((0, 2), (64, 3)):
            h.set_clear_exact(chunk, True)
            st, graph, exe, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
            assert H.hipStreamCreate(C.byref(st)) == 0
            try:
                def launch(call):
                    assert H.hipStreamBeginCapture(st, 0) == 0
                    call()
                    assert H.hipStreamEndCapture(st, C.byref(graph)) == 0
                    assert H.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == nodes
                    assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
                    for _ in range(2):
                        assert H.hipGraphLaunch(exe, st) == 0 and H.hipStreamSynchronize(st) == 0
                assert same(device_rows(h, T, Cf, cloud, chunk, stream=st.value, launch=launch)[0], want["piece"])
            finally:
                if exe.value:
                    H.hipGraphExecDestroy(exe)
                if graph.value:
                    H.hipGraphDestroy(graph)
                H.hipStreamDestroy(st)
        h.set_clear_exact(0, True)
    finally:
        h.close()
    # the second candidate alone on its own handle
    solo = penalty_handle(frx, sc, (9,), polys[8:17])
    try:
        r = solo.trajectory_clearance_exact(T[8:], Cf[48:], cloud)
        assert same(r["piece"], want["piece"][8:]) and same(r["cand"][0], want["cand"][1]) and r["flags"][0] == want["flags"][1]
    finally:
        solo.close()
    # the planning handle of the whole pool and a penalty handle of its layout: the same bits, and the first 17 rows are the restatement's
    Tp, Cp = states[state]
    a = prob.trajectory_clearance_exact(Tp, Cp, cloud)
    assert same(a["piece"][:P], ref)
    pen = penalty_handle(frx, sc, np.diff(prob.piece_off), polys)
    try:
        b = pen.trajectory_clearance_exact(Tp, Cp, cloud)
    finally:
        pen.close()
    assert same(a["piece"], b["piece"]) and same(a["cand"], b["cand"]) and np.array_equal(a["flags"], b["flags"])
    assert same(a["cand"], cx.reduce_candidates(a["piece"], Tp, prob.piece_off))


def test_crafted_states(frx, sc):
    """every crafted state on a handle of its own: the restatement's bits, the closed forms and the flags - and the same bits with one point a chunk and with
    the cull off (thrust zero at one end of a piece: the far point at index 0 ties at NaN and must win under every one of them)"""
    for name, st in xs.crafted(sc.ZHANGJIAJIE).items():
        h = xs.handle(frx, st["params"], st["counts"])
        try:
            got = h.trajectory_clearance_exact(st["T"], st["C"], st["obs"])
            for chunk, cull in ((1, True), (2, True), (0, False), (1, False)):
                h.set_clear_exact(chunk, cull)
                alt = h.trajectory_clearance_exact(st["T"], st["C"], st["obs"])
                assert same(alt["piece"], got["piece"]) and same(alt["cand"], got["cand"]) and np.array_equal(alt["flags"], got["flags"]), (name, chunk, cull)
        finally:
            h.close()
        off = offsets(st["counts"])
        assert_rows(got, cx.rows(st["T"], st["C"], st["obs"], st["params"]), st["T"], off)
        for r, e in zip(got["piece"], st["expect"]):
            if isinstance(e, str):
                assert np.isnan(r).all(), (name, r)
            else:
                assert not xs.expectation_failures(r, e), (name, xs.expectation_failures(r, e), r)
        if st["cand"] is not None:
            assert not xs.expectation_failures(got["cand"][0], st["cand"]), (name, got["cand"][0])
        fl = int(got["flags"][0])
        assert fl & st["set"] == st["set"] and fl & st["clear"] == 0, (name, fl)


def test_the_collision_the_dense_form_steps_over(frx, sc):
    """A 4 m piece flown at 10 m/s past a cloud point 0.9 eh beside the path at a third of it.  The dense form at 2 intervals samples the ends and the middle:
    ELL >= 1, no flag.  The exact form reports ELL = 0.9 at T / 3 and FRX_CLEAR_FLAG_COLLISION."""
    st = xs.crafted(sc.ZHANGJIAJIE)["a_beside"]
    h = xs.handle(frx, st["params"], [1])
    try:
        dense = h.trajectory_clearance(st["T"], st["C"], st["obs"], 2)
        exact = h.trajectory_clearance_exact(st["T"], st["C"], st["obs"])
    finally:
        h.close()
    assert dense["ell"][0] >= 1.0 and dense["flags"][0] == 0, dense["cand"]
    assert abs(exact["ell"][0] - 0.9) <= 1e-12 and abs(exact["t_ell"][0] - xs.T_RACE / 3) <= 1e-12 and exact["i_ell"][0] == 1
    assert exact["flags"][0] == frx.CLEAR_FLAG_COLLISION


def test_against_the_dense_form(frx, sc, pool):
    """The optimised 8 + 9 pieces against their 129 points, dense at 256 and 16 384 intervals.  The exact minimum cannot exceed a sample's value but by rounding:
    how much is measured HERE, on the CPU, between the two restatements (tests/clear_reference.py and tests/clear_exact_reference.py) on these very inputs, and
    asserted at 8 x the worst seen (0 where the exact value is never above); TOL max(1, value) is added for the device's dense rows against their own
    restatement, as tests/test_gpu_trajectory_clearance.py holds them.  And the finer dense run is never further from the exact value than the coarser one."""
    params = sc.ZHANGJIAJIE
    _, _, polys, states = pool
    piece_n, P = (8, 9), 17
    T, Cf, cloud, ref = reference(states, "optimised", P, 129, params)
    h = penalty_handle(frx, sc, piece_n, polys[:P])
    try:
        exact = h.trajectory_clearance_exact(T, Cf, cloud)["piece"]
        dense = {M: h.trajectory_clearance(T, Cf, cloud, M)["piece"] for M in (256, 16384)}
    finally:
        h.close()
    assert same(exact, ref)
    worst = 0.0
    for M in (256, 16384):
        dref = clr.clear_pieces(T, Cf, cloud, params, M)
        worst = max(worst, float((ref[:, :2] - dref[:, :2]).max()))
    bound = 8.0 * max(worst, 0.0)
    print("exact above dense between the restatements by at most", worst, "-> bound", bound)
    for M in (256, 16384):
        over = exact[:, :2] - dense[M][:, :2]
        print("M", M, "device: exact - dense in", float(over.min()), float(over.max()))
        assert (over <= bound + TOL * np.maximum(1.0, np.abs(dense[M][:, :2]))).all(), (M, over.max(), bound)
    assert (dense[16384][:, :2] - exact[:, :2] <= dense[256][:, :2] - exact[:, :2]).all()


def test_counts_on_a_spread_cloud(frx, sc, pool):
    """4 096 points spread over the scenario's whole bounding box: every piece keeps at least one survivor and fewer than the cloud holds.  No fraction is
    asserted; the printed one is that of this one synthetic scenario."""
    prob, _, _, states = pool
    T, Cf = states["optimised"]
    cloud = xs.spread_cloud(np.random.default_rng(77), T, Cf, 4096)
    got = prob.trajectory_clearance_exact(T, Cf, cloud)
    surv, ell = prob.clear_exact_counts()
    print(f"spread cloud of 4096 points, {prob.P} pieces: survivors per piece mean {surv.mean():.1f} max {surv.max()}, degree-21 tasks per piece mean {ell.mean():.1f} "
          f"max {ell.max()} ({surv.mean() / 4096:.4f} and {ell.mean() / 4096:.4f} of the cloud)")
    assert np.isfinite(got["piece"]).all()
    assert (surv >= 1).all() and (ell >= 1).all() and (surv < 4096).all()


def test_argument_errors_on_a_live_handle(frx, sc, pool):
    prob, _, _, states = pool
    T, Cf = states["initial"]
    L = frx.lib()
    t, c = np.ascontiguousarray(T), np.ascontiguousarray(Cf).reshape(-1)
    o = np.zeros((5, 3)) + 3.0
    piece = np.full(6 * prob.P, SENTINEL); cand = np.full(6 * prob.B, SENTINEL); nb = C.c_size_t(77)
    a = [prob.h, t.ctypes.data, c.ctypes.data, 5, o.ctypes.data, piece.ctypes.data, cand.ctypes.data, None]
    for k, v in ((1, None), (2, None), (4, None), (6, None), (3, 0), (3, -1), (3, (1 << 24) + 1)):
        b = list(a); b[k] = v
        assert L.frx_trajectory_clearance_exact(*b) == -1, (k, v)
    assert L.frx_trajectory_clearance_exact_device(prob.h, a[1], a[2], 5, a[4], None, a[5], None) == -1 and b"work_dev" in L.frx_last_error()
    assert L.frx_trajectory_clearance_exact_workspace(prob.h, 0, C.byref(nb)) == -1 and nb.value == 77
    assert (piece == SENTINEL).all() and (cand == SENTINEL).all()
    with pytest.raises(ValueError):
        prob.trajectory_clearance_exact(T[:1], Cf, o)
    with pytest.raises(ValueError):
        prob.trajectory_clearance_exact(T, Cf, o[:, :2])
    a[5] = None                                                          # piece_out and flags may be NULL
    assert L.frx_trajectory_clearance_exact(*a) == 0
    assert same(cand.reshape(-1, 6), prob.trajectory_clearance_exact(T, Cf, o)["cand"])
