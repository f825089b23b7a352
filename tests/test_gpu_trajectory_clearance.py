"""frx_trajectory_clearance on the device against the numpy restatement (tests/clear_reference.py): values to the TOL of
test_gpu_trajectory_check, whatever is stated as exact (ties, indices, worst_t, flags, NaN placement, bit-identity between forms, runs, batches
and splits of the cloud) with ==; and the loop it closes with frx_trajectory_check on cells that frx_line_segment_dilate built."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_reference as clr  # noqa: E402
import clear_states as cs  # noqa: E402
from test_gpu_trajectory_check import TOL, close  # noqa: E402
from test_gpu_trajectory_sample import DevBuf, hip  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
PAD = 4 * 64                                                           # sentinel doubles behind the rows and behind the workspace


def device_rows(prob, T, Cf, obs, M, stream=0, launch=None):
    """The piece rows of the device form; rows and workspace are pre-filled with a sentinel and nothing is written behind either at the size the
    workspace query reports.  launch(call) runs the enqueueing call (default: directly)."""
    P, n = prob.P, len(obs)
    nbytes = prob.trajectory_clearance_workspace(n, M)
    chunk, nch = cs.chunks(P, n, getattr(prob, "_forced_chunk", 0))
    assert nbytes == (32 * P * nch if nch > 1 else 0), (nbytes, P, nch)
    host = np.full(P * 4 + PAD, SENTINEL); whost = np.full(nbytes // 8 + PAD, SENTINEL)
    bufs = [DevBuf(np.ascontiguousarray(T)), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(np.ascontiguousarray(obs).reshape(-1)), DevBuf(whost), DevBuf(host)]
    Td, Cd, Od, Wd, out = bufs
    try:
        def call():
            prob.trajectory_clearance_device(Td.p, Cd.p, Od.p, n, Wd.p, out.p, M, stream)
        (launch or (lambda f: f()))(call)
        got, work = out.get(host), Wd.get(whost)
        assert (got[P * 4:] == SENTINEL).all() and (work[nbytes // 8:] == SENTINEL).all()
        assert nch == 1 or not (work[:nbytes // 8] == SENTINEL).any()
        return got[:P * 4].reshape(-1, 4)
    finally:
        for d in bufs:
            d.close()


def force(prob, points):
    prob.set_clear_chunk(points)
    prob._forced_chunk = points


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("piece", "cand", "flags"))


def assert_agrees(got, T, Cf, obs, params, M, piece_off):
    ref = clr.clear_pieces(T, Cf, obs, params, M)
    ok = close(got["piece"][:, :2], ref[:, :2])
    assert ok.all(), (M, np.argwhere(~ok)[:5], got["piece"][~ok.all(axis=1)][:2], ref[~ok.all(axis=1)][:2])
    # the reported worst sample attains the minimum: recompute it where the device says it is
    ell, g = clr.params_of(params)
    Cp = np.asarray(Cf).reshape(-1, 6, 3)
    for k in range(len(T)):
        step = T[k] / M
        j = int(round(got["piece"][k, 2] / step)); i = int(got["piece"][k, 3])
        assert 0 <= j <= M and got["piece"][k, 2] == step * j and 0 <= i < len(obs) and got["piece"][k, 3] == i, (k, got["piece"][k])
        q = clr.piece_q_r(Cp[k], float(T[k]), M, obs[i:i + 1], ell, g)["q"]
        assert abs(np.sqrt(q[j, 0]) - ref[k, 0]) <= TOL * max(1.0, abs(ref[k, 0])), (k, j, i, np.sqrt(q[j, 0]), ref[k, 0])
    cref = clr.reduce_candidates(ref, T, piece_off)
    assert close(got["cand"][:, :2], cref[:, :2]).all()
    mine = clr.reduce_candidates(got["piece"], T, piece_off)             # the host reduction, from the device's own rows: exact
    assert np.array_equal(got["cand"], mine) and np.array_equal(got["flags"], clr.flags_of(mine))
    return ref


def random_case(frx, sc, P, n_obs, seed=0):
    rng = np.random.default_rng(100 * P + n_obs + seed)
    T, Cf = cs.quintics(rng, P)
    params = dict(sc.ZHANGJIAJIE)
    params.update(cs.LOOSE)
    counts = cs.counts_of(P)
    return cs.handle(frx, params, counts), params, T, Cf, cs.cloud(rng, n_obs), np.concatenate([[0], np.cumsum(counts)])


@pytest.mark.parametrize("P", [1, 2, 5])
def test_agrees_with_numpy(frx, sc, P):
    """M = 1 and each side of the sample tile (= a wave); the cloud short of a wave's registers."""
    prob, params, T, Cf, obs, off = random_case(frx, sc, P, 300)
    try:
        for M in (1, cs.TILE - 2, cs.TILE - 1, cs.TILE, 2 * cs.TILE + 1):     # M + 1 = 2, tile - 1, tile, tile + 1, two tiles + 2 samples
            got = prob.trajectory_clearance(T, Cf, obs, M)
            assert got["piece"].shape == (P, 4) and got["cand"].shape == (len(off) - 1, 4) and got["flags"].dtype == np.uint32
            assert np.array_equal(got["ell"], got["cand"][:, 0]) and np.array_equal(got["worst_i"], got["cand"][:, 3])
            assert_agrees(got, T, Cf, obs, params, M, off)
            assert same(got, prob.trajectory_clearance(T, Cf, obs, M))
            assert np.array_equal(device_rows(prob, T, Cf, obs, M), got["piece"])
    finally:
        prob.close()


@pytest.mark.parametrize("n_obs", [1, 63, 64, 65, 255, 256, 257, cs.PASS - 1, cs.PASS, cs.PASS + 1, 2 * cs.PASS + 3])
def test_cloud_sizes(frx, sc, n_obs):
    """Each side of a wave, of a slot of registers and of a pass; past one pass a lone piece's cloud is split (chunks of one pass), a batch's is not
    when forced into one chunk of several passes."""
    prob, params, T, Cf, obs, off = random_case(frx, sc, 2, n_obs)
    try:
        assert cs.chunks(2, n_obs)[1] == -(-n_obs // cs.PASS)
        got = prob.trajectory_clearance(T, Cf, obs, 5)
        assert_agrees(got, T, Cf, obs, params, 5, off)
        assert np.array_equal(device_rows(prob, T, Cf, obs, 5), got["piece"])
        force(prob, n_obs)                                                # one chunk: as many passes as the cloud needs
        assert np.array_equal(device_rows(prob, T, Cf, obs, 5), got["piece"]) and same(got, prob.trajectory_clearance(T, Cf, obs, 5))
    finally:
        prob.close()


def test_each_side_of_a_chunk_and_every_split_gives_the_same_bits(frx, sc):
    prob, params, T, Cf, obs, off = random_case(frx, sc, 5, 257)
    try:
        M = 9
        force(prob, 100)
        for n in (99, 100, 101):                                          # one chunk short, exactly one, one point into the second
            assert cs.chunks(5, n, 100)[1] == (1 if n <= 100 else 2)
            got = prob.trajectory_clearance(T, Cf, obs[:n], M)
            assert_agrees(got, T, Cf, obs[:n], params, M, off)
            assert np.array_equal(device_rows(prob, T, Cf, obs[:n], M), got["piece"])
        force(prob, 0)
        want = prob.trajectory_clearance(T, Cf, obs, M)
        assert_agrees(want, T, Cf, obs, params, M, off)
        for pts in (257, 1000, 256, 129, 128, 100, 64, 7, 1):             # one chunk, a chunk larger than the cloud, many, sizes that do not divide 257
            force(prob, pts)
            assert same(want, prob.trajectory_clearance(T, Cf, obs, M)), pts
            assert np.array_equal(device_rows(prob, T, Cf, obs, M), want["piece"]), pts
    finally:
        prob.close()


def test_split_for_few_pieces_and_not_for_many(frx, sc):
    """The same cloud of 1030 points: split in two for one piece (2048 workgroups wanted), whole for 1100 pieces; a piece's row is the same in both."""
    rng = np.random.default_rng(8)
    P, n = 1100, cs.PASS + 6
    T, Cf = cs.quintics(rng, P)
    obs = cs.cloud(rng, n)
    params = dict(sc.ZHANGJIAJIE)
    params.update(cs.LOOSE)
    counts = [22] * 50                                                    # (many short candidates)
    big, one = cs.handle(frx, params, counts), cs.handle(frx, params, [1])
    try:
        assert cs.chunks(P, n) == (n, 1) and cs.chunks(1, n) == (cs.PASS, 2)
        assert big.trajectory_clearance_workspace(n, 3) == 0 and one.trajectory_clearance_workspace(n, 3) == 32 * 2
        got = big.trajectory_clearance(T, Cf, obs, 3)
        pick = np.array([0, 1, 549, 550, 777, 1099])
        ref = clr.clear_pieces(T[pick], Cf.reshape(-1, 6, 3)[pick].reshape(-1, 3), obs, params, 3)
        assert close(got["piece"][pick, :2], ref[:, :2]).all() and np.array_equal(got["piece"][pick, 3], ref[:, 3])
        assert np.array_equal(got["cand"], clr.reduce_candidates(got["piece"], T, np.concatenate([[0], np.cumsum(counts)])))
        assert np.array_equal(device_rows(big, T, Cf, obs, 3), got["piece"])
        for q in (0, 777):
            solo = one.trajectory_clearance(T[q:q + 1], Cf[6 * q:6 * q + 6], obs, 3)
            assert np.array_equal(solo["piece"][0], got["piece"][q])
            assert np.array_equal(device_rows(one, T[q:q + 1], Cf[6 * q:6 * q + 6], obs, 3)[0], got["piece"][q])
    finally:
        big.close(); one.close()


def test_both_kinds_of_handle_and_a_piece_alone(frx, sc):
    """A handle with variables (frx_problem_create) serves the check too; a one-piece handle gives the bits of the same piece inside the batch."""
    cands = sc.make_batch(1, 3, 16, 4)
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=8)
    try:
        T, Cf = prob.forward(prob.initial_guess())
        rng = np.random.default_rng(2)
        lo, hi = Cf.reshape(-1, 6, 3)[:, 0].min(axis=0) - 2.0, Cf.reshape(-1, 6, 3)[:, 0].max(axis=0) + 2.0
        obs = rng.uniform(lo, hi, (700, 3))
        got = prob.trajectory_clearance(T, Cf, obs, 40)
        assert_agrees(got, T, Cf, obs, sc.ZHANGJIAJIE, 40, list(prob.piece_off))
        assert np.array_equal(device_rows(prob, T, Cf, obs, 40), got["piece"])
        for q in (0, prob.P - 1):
            solo = cs.handle(frx, dict(sc.ZHANGJIAJIE), [1])
            try:
                r = solo.trajectory_clearance(T[q:q + 1], Cf[6 * q:6 * q + 6], obs, 40)
                assert np.array_equal(r["piece"][0], got["piece"][q])
            finally:
                solo.close()
    finally:
        prob.close()


def test_exact_ties(frx, sc):
    params = cs.exact_params(sc.ZHANGJIAJIE)
    # a duplicated cloud point: the lower i; far enough apart in the cloud to sit in other slots, lanes, waves and chunks
    line = cs.line_piece((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1.0)
    n = 600
    obs = np.tile(np.array([[9.0, 0.0, 0.0]]), (n, 1)) + np.arange(n)[:, None] * np.array([[0.0, 0.125, 0.0]])
    near = np.array([0.375, 1.0, 0.0])                                   # equidistant from the samples j = 1 and 2 of M = 4: the lower j
    prob = cs.handle(frx, params, [1])
    try:
        for a, b in ((3, 5), (3, 70), (3, 259), (130, 599), (0, 256)):
            o = obs.copy()
            o[a] = near; o[b] = near
            for pts in (0, 600, 64, 7):
                force(prob, pts)
                got = prob.trajectory_clearance(np.array([1.0]), line, o, 4)
                assert tuple(got["piece"][0]) == (np.sqrt(0.0625 + 4.0), np.sqrt(0.015625 + 1.0), 0.25, float(a)), (a, b, pts, got["piece"][0])
                assert same(got, dict(piece=device_rows(prob, np.array([1.0]), line, o, 4), cand=got["cand"], flags=got["flags"]))
            assert tuple(got["cand"][0]) == tuple(got["piece"][0]) and got["flags"][0] == 0
        # a body that stands still ties on every sample: j = 0
        force(prob, 0)
        got = prob.trajectory_clearance(np.array([1.0]), cs.still_piece((0.0, 0.0, 0.0)), obs, 200)
        assert tuple(got["piece"][0]) == (18.0, 9.0, 0.0, 0.0)
    finally:
        prob.close()
    # a duplicated piece in two candidates: identical rows, and the candidate names the first of equal pieces
    rng = np.random.default_rng(12)
    T, Cf = cs.quintics(rng, 5)
    T[4] = T[1]; Cf[24:30] = Cf[6:12]
    T[2] = T[1]; Cf[12:18] = Cf[6:12]
    cloud = cs.cloud(rng, 400) * 0.25                                    # (close by: piece 1 is the nearest of its candidate)
    prob = cs.handle(frx, params, [3, 2])
    try:
        got = prob.trajectory_clearance(T, Cf, cloud, 20)
        assert np.array_equal(got["piece"][1], got["piece"][4]) and np.array_equal(got["piece"][1], got["piece"][2])
        assert_agrees(got, T, Cf, cloud, params, 20, [0, 3, 5])
        if got["piece"][1, 0] < got["piece"][0, 0]:
            assert got["cand"][0, 2] == T[0] + got["piece"][1, 2]
    finally:
        prob.close()


def test_nan_order(frx, sc):
    params = dict(sc.ZHANGJIAJIE)
    params.update(cs.LOOSE)
    rng = np.random.default_rng(13)
    T, Cf = cs.quintics(rng, 7)
    obs = cs.cloud(rng, 300)
    prob = cs.handle(frx, params, [3, 4])
    try:
        clean = prob.trajectory_clearance(T, Cf, obs, 33)
        assert np.isfinite(clean["piece"]).all() and not (clean["flags"] & frx.CLEAR_FLAG_NONFINITE).any()
        # a NaN in a later piece: its candidate is NaN from there, with the prefix of durations; the other candidate keeps its bits
        bad = Cf.copy()
        bad[6 * 5 + 4, 1] = np.nan                                        # piece 5 = the third of candidate 1
        got = prob.trajectory_clearance(T, bad, obs, 33)
        assert np.isnan(got["piece"][5, :2]).all() and got["piece"][5, 2] == 0.0 and got["piece"][5, 3] == 0.0
        keep = np.arange(7) != 5
        assert np.array_equal(got["piece"][keep], clean["piece"][keep])
        assert np.array_equal(got["cand"][0], clean["cand"][0]) and got["flags"][0] == clean["flags"][0]
        assert np.isnan(got["cand"][1, :2]).all() and got["cand"][1, 2] == (T[3] + T[4]) + 0.0 and got["cand"][1, 3] == 0.0
        assert got["flags"][1] == frx.CLEAR_FLAG_NONFINITE
        assert np.array_equal(device_rows(prob, T, bad, obs, 33), got["piece"], equal_nan=True)
        # NaN cloud points at 6 and 3: every piece reports the lower index at its first sample, under every split
        o = obs.copy()
        o[6, 2] = np.nan; o[3, 0] = np.nan
        for pts in (0, 300, 5, 4, 1):
            force(prob, pts)
            got = prob.trajectory_clearance(T, Cf, o, 33)
            assert np.isnan(got["piece"][:, :2]).all() and (got["piece"][:, 2] == 0.0).all() and (got["piece"][:, 3] == 3.0).all(), (pts, got["piece"])
            assert np.isnan(got["cand"][:, :2]).all() and (got["cand"][:, 2] == 0.0).all() and (got["cand"][:, 3] == 3.0).all()
            assert (got["flags"] == frx.CLEAR_FLAG_NONFINITE).all()
            assert np.array_equal(device_rows(prob, T, Cf, o, 33), got["piece"], equal_nan=True)
        # a non-finite duration
        force(prob, 0)
        Tb = T.copy(); Tb[0] = np.inf
        got = prob.trajectory_clearance(Tb, Cf, obs, 33)
        assert got["flags"][0] & frx.CLEAR_FLAG_NONFINITE and np.array_equal(got["piece"][3:], clean["piece"][3:]) and np.array_equal(got["cand"][1], clean["cand"][1])
    finally:
        prob.close()


def test_graph_capture(frx, sc):
    """The device form is pure launches: captured on a caller stream it is two kernel nodes when the cloud is split, one when it is not, and
    replaying the graph gives the bits of the blocking form."""
    prob, params, T, Cf, obs, off = random_case(frx, sc, 5, 700)
    H = hip()
    try:
        for pts, nodes in ((0, 1), (100, 2)):
            force(prob, pts)
            want = prob.trajectory_clearance(T, Cf, obs, 70)["piece"]
            st, graph, exe, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
            assert H.hipStreamCreate(C.byref(st)) == 0
            try:
                def launch(call):
                    assert H.hipStreamBeginCapture(st, 0) == 0                                 # hipStreamCaptureModeGlobal
                    call()
                    assert H.hipStreamEndCapture(st, C.byref(graph)) == 0
                    assert H.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == nodes
                    assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
                    for _ in range(2):
                        assert H.hipGraphLaunch(exe, st) == 0 and H.hipStreamSynchronize(st) == 0
                assert np.array_equal(device_rows(prob, T, Cf, obs, 70, stream=st.value, launch=launch), want)
            finally:
                if exe.value:
                    H.hipGraphExecDestroy(exe)
                if graph.value:
                    H.hipGraphDestroy(graph)
                H.hipStreamDestroy(st)
    finally:
        prob.close()


def test_flags_on_both_sides_of_one(frx, sc):
    """grav_acc = 8 and semi-axes 1/2, 1/8: R = I exactly, so a point at exactly e0 on the axis gives ELL = 1 (free) and one ulp inside gives
    the double below 1 (collision)."""
    params = cs.exact_params(sc.ZHANGJIAJIE)
    prob = cs.handle(frx, params, [1])
    try:
        far = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 2.0]])
        c, T = cs.still_piece((0.0, 0.0, 0.0)), np.array([1.0])
        for o, e in (((0.5, 0.0, 0.0), 0.5), ((0.0, -0.5, 0.0), 0.5), ((0.0, 0.0, 0.125), 0.125)):
            got = prob.trajectory_clearance(T, c, np.vstack([far, [o]]), 8)
            assert tuple(got["cand"][0]) == (1.0, e, 0.0, 2.0) and got["flags"][0] == 0, (o, got["cand"][0])
            inside = np.array(o) * (np.nextafter(e, 0.0) / e)             # one ulp towards the centre
            got = prob.trajectory_clearance(T, c, np.vstack([far, [inside]]), 8)
            assert got["cand"][0, 0] == np.nextafter(1.0, 0.0) and got["flags"][0] == frx.CLEAR_FLAG_COLLISION, (o, got["cand"][0])
            assert_agrees(got, T, c, np.vstack([far, [inside]]), params, 8, [0, 1])
    finally:
        prob.close()


def test_closing_the_loop(frx, sc):
    """Cells of frx_line_segment_dilate hold no cloud point in their interior: wherever the device's check puts the body inside its cell, the
    device's clearance finds no cloud point inside the body.  1e-9 stands for the rsqrt_fast frame both kernels share."""
    st = cs.loop_state(frx, sc.ZHANGJIAJIE)
    prob = cs.handle(frx, st["params"], st["counts"], st["polys"])
    try:
        chk = prob.trajectory_check(st["T"], st["Cf"], cs.LOOP_M)["piece"]
        got = prob.trajectory_clearance(st["T"], st["Cf"], st["obs"], cs.LOOP_M)
        inside = chk[:, 0] <= 0.0
        print(f"closing the loop: {inside.sum()} of {len(inside)} pieces inside their cells, smallest ELL among them {got['piece'][inside, 0].min():.6f}, "
              f"smallest ELL of all {got['piece'][:, 0].min():.6f}")
        assert 2 * inside.sum() >= len(inside) and 2 * st["inside"].sum() >= len(inside)
        assert (got["piece"][inside, 0] >= 1.0 - 1e-9).all(), got["piece"][:, 0]
        assert_agrees(got, st["T"], st["Cf"], st["obs"], st["params"], cs.LOOP_M, [0, len(inside)])
    finally:
        prob.close()


def test_argument_errors_on_a_live_handle(frx, sc):
    prob, params, T, Cf, obs, off = random_case(frx, sc, 2, 50)
    try:
        assert isinstance(prob, frx.PenaltyProblem)
        L = frx.lib()
        t, c, o = np.ascontiguousarray(T), np.ascontiguousarray(Cf).reshape(-1), np.ascontiguousarray(obs)
        piece, cand, fl, nb = np.full(8, SENTINEL), np.full(4, SENTINEL), np.full(1, 77, np.uint32), C.c_size_t(77)
        a = [prob.h, t.ctypes.data, c.ctypes.data, 16, 50, o.ctypes.data, piece.ctypes.data, cand.ctypes.data, fl.ctypes.data]
        for k, v in ((1, None), (2, None), (5, None), (7, None), (3, 0), (3, -1), (3, 16385), (4, 0), (4, -3), (4, (1 << 24) + 1)):
            b = list(a); b[k] = v
            assert L.frx_trajectory_clearance(*b) == -1, (k, v)
            d = [prob.h, b[1], b[2], b[3], b[4], b[5], None, b[6], None]
            if k != 7:
                assert L.frx_trajectory_clearance_device(*d) == -1, (k, v)
            if k in (3, 4):
                assert L.frx_trajectory_clearance_workspace(prob.h, b[3], b[4], C.byref(nb)) == -1
        assert L.frx_trajectory_clearance_device(prob.h, a[1], a[2], 16, 50, a[5], None, None, None) == -1
        assert L.frx_trajectory_clearance_workspace(prob.h, 16, 50, None) == -1
        force(prob, 10)                                                   # scratch is asked for, none given
        assert L.frx_trajectory_clearance_device(prob.h, a[1], a[2], 16, 50, a[5], None, a[6], None) == -1 and b"work_dev" in L.frx_last_error()
        assert (piece == SENTINEL).all() and (cand == SENTINEL).all() and fl[0] == 77 and nb.value == 77
        with pytest.raises(ValueError):
            prob.trajectory_clearance(T[:1], Cf, obs, 16)
        with pytest.raises(ValueError):
            prob.trajectory_clearance(T, Cf, obs[:, :2], 16)
        force(prob, 0)
        got = prob.trajectory_clearance(T, Cf, obs, 16)                    # piece_out and flags may be NULL
        only = np.zeros(4 * (len(off) - 1))
        assert L.frx_trajectory_clearance(prob.h, t.ctypes.data, c.ctypes.data, 16, 50, o.ctypes.data, None, only.ctypes.data, None) == 0
        assert np.array_equal(only.reshape(-1, 4), got["cand"])
    finally:
        prob.close()
