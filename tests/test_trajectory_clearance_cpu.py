"""frx_trajectory_clearance without a device: the entry points exist, bad arguments are refused before any device work, the launch rule restated
in tests/clear_states.py is the library's, and the numpy restatement the GPU tests compare against (tests/clear_reference.py) gives the
hand-checkable answers and agrees with the ellipsoid distance of frx_line_segment_dilate."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_reference as cr  # noqa: E402
import clear_reference as clr  # noqa: E402
import clear_states as cs  # noqa: E402


def test_entry_points_are_exported(frx):
    L = C.CDLL(frx.LIB_PATH)
    for name in ("frx_trajectory_clearance", "frx_trajectory_clearance_workspace", "frx_trajectory_clearance_device"):
        assert hasattr(L, name) and name in frx.ABI_SYMBOLS
    assert hasattr(L, "frx_debug_set_clear_chunk") and "frx_debug_set_clear_chunk" in frx.DEBUG_SYMBOLS
    assert frx.CLEAR_FIELDS == clr.FIELDS and frx.CLEAR_MAX_POINTS == 1 << 24
    assert (frx.CLEAR_FLAG_COLLISION, frx.CLEAR_FLAG_NONFINITE) == (clr.FLAG_COLLISION, clr.FLAG_NONFINITE)
    assert (frx.CLEAR_TILE, frx.CLEAR_PASS) == (cs.TILE, cs.PASS)
    for name in ("trajectory_clearance", "trajectory_clearance_device", "trajectory_clearance_workspace"):
        assert hasattr(frx.Problem, name) and getattr(frx.PenaltyProblem, name) is getattr(frx.Problem, name)


def test_invalid_arguments(frx):
    L = frx.lib()
    T = np.zeros(1); Cf = np.zeros(18); out = np.zeros(4); fl = np.zeros(1, np.uint32); obs = np.zeros(3); nb = C.c_size_t(77)
    t, c, o, f, b = T.ctypes.data, Cf.ctypes.data, out.ctypes.data, fl.ctypes.data, obs.ctypes.data
    assert L.frx_trajectory_clearance(None, t, c, 16, 1, b, o, o, f) == -1
    assert L.frx_trajectory_clearance_device(None, t, c, 16, 1, b, None, o, None) == -1
    assert L.frx_trajectory_clearance_workspace(None, 16, 1, C.byref(nb)) == -1
    # a handle-shaped placeholder: the arguments are refused before the handle is ever read
    fake = C.create_string_buffer(64)
    h = C.cast(fake, C.c_void_p)
    assert L.frx_trajectory_clearance(h, None, c, 16, 1, b, o, o, f) == -1
    assert L.frx_trajectory_clearance(h, t, None, 16, 1, b, o, o, f) == -1
    assert L.frx_trajectory_clearance(h, t, c, 16, 1, None, o, o, f) == -1
    assert L.frx_trajectory_clearance(h, t, c, 16, 1, b, o, None, f) == -1
    assert L.frx_trajectory_clearance_device(h, None, c, 16, 1, b, None, o, None) == -1
    assert L.frx_trajectory_clearance_device(h, t, None, 16, 1, b, None, o, None) == -1
    assert L.frx_trajectory_clearance_device(h, t, c, 16, 1, None, None, o, None) == -1
    assert L.frx_trajectory_clearance_device(h, t, c, 16, 1, b, None, None, None) == -1
    assert L.frx_trajectory_clearance_workspace(h, 16, 1, None) == -1
    for bad in (0, -1, 16385):
        assert L.frx_trajectory_clearance(h, t, c, bad, 1, b, o, o, f) == -1
        assert b"intervals" in L.frx_last_error()
        assert L.frx_trajectory_clearance_device(h, t, c, bad, 1, b, None, o, None) == -1
        assert L.frx_trajectory_clearance_workspace(h, bad, 1, C.byref(nb)) == -1
    for bad in (0, -1, (1 << 24) + 1):
        assert L.frx_trajectory_clearance(h, t, c, 16, bad, b, o, o, f) == -1
        assert b"n_obs" in L.frx_last_error()
        assert L.frx_trajectory_clearance_device(h, t, c, 16, bad, b, None, o, None) == -1
        assert L.frx_trajectory_clearance_workspace(h, 16, bad, C.byref(nb)) == -1
    assert L.frx_debug_set_clear_chunk(None, 4) == -1
    assert not fake.raw.strip(b"\0") and nb.value == 77 and not out.any()      # nothing was written


def test_launch_rule():
    """The split of the cloud: whole passes, 2048 workgroups wanted, one chunk when the pieces alone reach that."""
    assert cs.chunks(1, 1) == (1, 1) and cs.chunks(1, 1024) == (1024, 1) and cs.chunks(1, 1025) == (1024, 2)
    assert cs.chunks(1, 2500) == (1024, 3) and cs.chunks(1000, 2500) == (2048, 2) and cs.chunks(1100, 2500) == (2500, 1) and cs.chunks(2048, 2500) == (2500, 1) and cs.chunks(5000, 2500) == (2500, 1)
    assert cs.chunks(64, 65536) == (2048, 32) and cs.chunks(2048, 65536) == (65536, 1) and cs.chunks(32768, 65536) == (65536, 1)
    assert cs.chunks(3, 100, 7) == (7, 15) and cs.chunks(3, 100, 100) == (100, 1) and cs.chunks(3, 100, 1000) == (100, 1)


def test_hover_on_a_principal_axis_is_exactly_one():
    params = dict(horiz_half_len=0.5, vert_half_len=0.15, grav_acc=9.81)
    ell, g = clr.params_of(params)
    at = np.zeros(3)                                                      # (at the origin o - p is the semi-axis itself, bit for bit)
    c = cs.still_piece(at)
    for axis in range(3):
        for sign in (1.0, -1.0):
            o = at.copy()
            o[axis] += sign * ell[axis]
            far = at + np.array([3.0, 4.0, 0.0])
            row = clr.piece_row(c, 1.0, 4, np.array([far, o, far]), ell, g)
            assert row[0] == 1.0 and row[1] == ell[axis] and row[2] == 0.0 and row[3] == 1.0, (axis, sign, row)
    # exactly 1 where the arithmetic is exact, and a point one ulp inside is inside
    p = cs.exact_params(params)
    ell, g = clr.params_of(p)
    row = clr.piece_row(cs.still_piece((0.0, 0.0, 0.0)), 1.0, 4, np.array([[0.5, 0.0, 0.0]]), ell, g)
    assert row[0] == 1.0 and row[1] == 0.5
    row = clr.piece_row(cs.still_piece((0.0, 0.0, 0.0)), 1.0, 4, np.array([[np.nextafter(0.5, 0.0), 0.0, 0.0]]), ell, g)
    assert row[0] < 1.0
    cand = clr.reduce_candidates(np.array([row]), np.array([1.0]), [0, 1])
    assert clr.flags_of(cand)[0] == clr.FLAG_COLLISION


def test_tilted_body_gives_the_rotated_answer():
    """Constant acceleration a = (g, 0, 0): h = (g, 0, g), zB = (1, 0, 1) / sqrt 2, yB = e2, xB = (1, 0, -1) / sqrt 2."""
    g = 9.81
    ell = (0.5, 0.4, 0.15)
    c = np.zeros((6, 3))
    c[2] = (0.5 * g, 0.0, 0.0)                                            # p = (g / 2) s^2 e1
    r2 = np.sqrt(0.5)
    xB, yB, zB = np.array([r2, 0.0, -r2]), np.array([0.0, 1.0, 0.0]), np.array([r2, 0.0, r2])
    M, T = 4, 1.0
    s = (T / M) * np.arange(M + 1)
    pos = np.stack([0.5 * g * s ** 2, 0 * s, 0 * s], axis=1)
    # on the tilted axes at the semi-axis length from the sample at j = 2, j = 3 and j = 0: ELL = 1 there, attained first at the lowest of them
    obs = np.array([pos[2] + ell[2] * zB, pos[3] - ell[0] * xB, pos[0] + ell[1] * yB, pos[4] + 2.0 * zB])
    v = clr.piece_q_r(c, T, M, obs, ell, g)
    assert v["q"][2, 0] == pytest.approx(1.0, abs=1e-14) and v["q"][3, 1] == pytest.approx(1.0, abs=1e-14) and v["q"][0, 2] == pytest.approx(1.0, abs=1e-14)
    assert v["q"][4, 3] == pytest.approx((2.0 / ell[2]) ** 2, rel=1e-14)
    # an untilted body would see the first point at (r2 ell2 / e0)^2 + (r2 ell2 / e2)^2: the frame matters
    flat = clr.q_r(pos[2:3], np.eye(3)[None], ell, obs[:1])[0][0, 0]
    assert flat == pytest.approx((r2 * ell[2] / ell[0]) ** 2 + 0.5, rel=1e-14) and abs(flat - 1.0) > 0.4
    row = clr.piece_row(c, T, M, obs, ell, g)
    assert row[0] == pytest.approx(np.sqrt(v["q"].min()), abs=0) and row[0] == pytest.approx(1.0, abs=1e-13)
    j, i = divmod(int(np.argmin(v["q"].reshape(-1))), 4)
    assert row[2] == s[j] and row[3] == float(i)


def test_order_and_reduction_rules():
    """NaN first, then the smaller value, then the lower j, then the lower i; the candidate names its first piece and sums the prefix."""
    p = cs.exact_params(dict(horiz_half_len=0.5, vert_half_len=0.15, grav_acc=9.81))
    ell, g = clr.params_of(p)
    c = cs.line_piece((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1.0)
    obs = np.array([[9.0, 0.0, 0.0], [0.375, 1.0, 0.0], [0.375, 1.0, 0.0]])        # equidistant from the samples j = 1 and 2 of M = 4; a duplicate
    row = clr.piece_row(c, 1.0, 4, obs, ell, g)
    assert row[0] == np.sqrt(0.0625 + 4.0) and row[2] == 0.25 and row[3] == 1.0 and row[1] == np.sqrt(0.125 ** 2 + 1.0)
    bad = obs.copy()
    bad[2, 1] = np.nan
    nrow = clr.piece_row(c, 1.0, 4, bad, ell, g)
    assert np.isnan(nrow[0]) and np.isnan(nrow[1]) and nrow[2] == 0.0 and nrow[3] == 2.0
    rows = np.array([row, row, nrow, nrow])
    cand = clr.reduce_candidates(rows, np.array([1.0, 2.0, 4.0, 8.0]), [0, 2, 4])
    assert cand[0, 0] == row[0] and cand[0, 2] == 0.25 and cand[0, 3] == 1.0
    assert np.isnan(cand[1, 0]) and np.isnan(cand[1, 1]) and cand[1, 2] == 0.0 and cand[1, 3] == 2.0
    cand = clr.reduce_candidates(rows, np.array([1.0, 2.0, 4.0, 8.0]), [0, 4])
    assert np.isnan(cand[0, 0]) and cand[0, 2] == 3.0 and cand[0, 3] == 2.0
    assert tuple(clr.flags_of(cand)) == (clr.FLAG_NONFINITE,)
    assert tuple(clr.flags_of(np.array([[1.0, 2.0, 0.0, 0.0], [np.nextafter(1.0, 0.0), 2.0, 0.0, 0.0]]))) == (0, clr.FLAG_COLLISION)


def test_agrees_with_the_ellipsoid_of_line_segment_dilate(frx):
    """ELL^2 is the square of decomp_util's Ellipsoid::dist |C^-1 (o - d)| for the body ellipsoid C = R E: taken on the ellipsoids that
    frx_line_segment_dilate returns (ell_C, ell_d), whose axes and frame are read off C."""
    rng = np.random.default_rng(21)
    for k in range(6):
        p1 = rng.uniform(-3, 3, 3); p2 = p1 + rng.normal(0, 1, 3) * np.array([2.0, 2.0, 0.5])
        obs = 0.5 * (p1 + p2) + rng.normal(0, 1.2, (60, 3))
        _, Cm, d = frx.line_segment_dilate(p1, p2, np.array([4.0, 4.0, 2.5]), obs)
        w, V = np.linalg.eigh(0.5 * (Cm + Cm.T))                          # C = V diag(w) V^T: semi-axes w along the columns of V
        q, _ = clr.q_r(d[None], V[None], w, obs)
        dist = np.linalg.norm(np.linalg.solve(Cm, (obs - d).T), axis=0)
        assert np.abs(q[0] - dist ** 2).max() <= 1e-11 * (dist ** 2).max(), (k, np.abs(q[0] - dist ** 2).max())
        assert np.sqrt(q[0].min()) >= 1.0 - 1e-9                          # the cell's ellipsoid holds no cloud point


def test_closing_the_loop_state(frx, sc):
    """At least half of the pieces lie inside their cells by check_reference, and on those the restatement finds no cloud point inside the body."""
    st = cs.loop_state(frx, sc.ZHANGJIAJIE)
    assert len(st["obs"]) >= 1025 and max(h.shape[1] for h in st["polys"]) <= 500
    assert 2 * st["inside"].sum() >= len(st["T"]), (st["inside"], st["params"]["horiz_half_len"])
    rows = cr.check_pieces(st["T"], st["Cf"], st["polys"], st["params"], cs.LOOP_M)
    assert np.array_equal(rows[:, 0] <= 0.0, st["inside"])
    clear = clr.clear_pieces(st["T"], st["Cf"], st["obs"], st["params"], cs.LOOP_M)
    assert (clear[st["inside"], 0] >= 1.0).all(), clear[:, 0]
    assert np.isfinite(clear).all() and (clear[:, 1] >= clear[:, 0] * st["params"]["vert_half_len"] * (1 - 1e-12)).all()
