"""frx_trajectory_check without a device: the entry points exist, bad arguments are refused before any device work, and the numpy restatement
the GPU tests compare against (tests/check_reference.py) agrees with the reference's exact maxima (Trajectory::getMaxVelRate / getMaxAccRate)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_reference as cr  # noqa: E402


def test_entry_points_are_exported(frx):
    L = C.CDLL(frx.LIB_PATH)
    assert hasattr(L, "frx_trajectory_check") and hasattr(L, "frx_trajectory_check_device")
    assert "frx_trajectory_check" in frx.ABI_SYMBOLS and "frx_trajectory_check_device" in frx.ABI_SYMBOLS
    assert frx.CHECK_FIELDS == cr.FIELDS and frx.CHECK_MAX_INTERVALS == 16384


def test_invalid_arguments(frx):
    L = frx.lib()
    T = np.zeros(1); Cf = np.zeros(18); out = np.zeros(8); fl = np.zeros(1, np.uint32)
    t, c, o, f = T.ctypes.data, Cf.ctypes.data, out.ctypes.data, fl.ctypes.data
    assert L.frx_trajectory_check(None, t, c, 16, o, o, f) == -1
    assert L.frx_trajectory_check_device(None, t, c, 16, o, None) == -1
    # a handle-shaped placeholder: the arguments are refused before the handle is ever read
    fake = C.create_string_buffer(64)
    h = C.cast(fake, C.c_void_p)
    assert L.frx_trajectory_check(h, None, c, 16, o, o, f) == -1
    assert L.frx_trajectory_check(h, t, None, 16, o, o, f) == -1
    assert L.frx_trajectory_check(h, t, c, 16, o, None, f) == -1
    assert L.frx_trajectory_check_device(h, None, c, 16, o, None) == -1
    assert L.frx_trajectory_check_device(h, t, None, 16, o, None) == -1
    assert L.frx_trajectory_check_device(h, t, c, 16, None, None) == -1
    for bad in (0, -1, 16385):
        assert L.frx_trajectory_check(h, t, c, bad, o, o, f) == -1
        assert b"intervals" in L.frx_last_error()
        assert L.frx_trajectory_check_device(h, t, c, bad, o, None) == -1
    assert not fake.raw.strip(b"\0")                    # nothing was written through it


def _optimised(sc, ob, sid, N, gates):
    cand = sc.make_candidate(sid, N, gates)
    r = ob.Oracle(cand, sc.ZHANGJIAJIE, qd_intervals=8).optimize(1e-6, max_iterations=80)
    return cand, r["T"], r["C"]


def test_numpy_reference_brackets_the_exact_maxima(sc, ob):
    """At M = 2048 the sampled maxima of speed and acceleration lie within (1 - 1e-5, 1 + 1e-12) of the reference's root-finder maxima."""
    if ob.ref_traj() is None:
        pytest.skip("oracle/_ref/libref_traj.so not built (reference tree absent)")
    rng = np.random.default_rng(11)
    trajs = [_optimised(sc, ob, sid, 10, 2)[1:] for sid in (2, 5)]
    trajs.append((rng.uniform(0.2, 2.0, 4), rng.normal(0, 1, (24, 3))))       # random quintics as well
    for T, Cf in trajs:
        pl = ob.piece_layout(Cf)
        box = np.concatenate([np.vstack([np.eye(3), 1e3 * np.ones((3, 3))]), np.vstack([-np.eye(3), -1e3 * np.ones((3, 3))])], axis=1)
        rows = cr.check_pieces(T, Cf, [box] * len(T), sc.ZHANGJIAJIE, 2048)
        for i in range(len(T)):
            exact = np.zeros(2)
            ob.ref_traj().ref_piece_max_rates(float(T[i]), np.ascontiguousarray(pl[i].reshape(-1)), exact)
            for got, ex in ((rows[i, 1], exact[0]), (rows[i, 5], exact[1])):
                assert ex * (1 - 1e-5) <= got <= ex * (1 + 1e-12), (i, got, ex)
        out3 = np.zeros(3)
        ob.ref_traj().ref_traj_max_rates(len(T), np.ascontiguousarray(T), np.ascontiguousarray(pl.reshape(-1)), out3)
        cand = cr.reduce_candidates(rows, T, [0, len(T)])
        assert out3[0] * (1 - 1e-5) <= cand[0, 1] <= out3[0] * (1 + 1e-12)
        assert out3[1] * (1 - 1e-5) <= cand[0, 5] <= out3[1] * (1 + 1e-12)


def test_numpy_reference_definitions():
    """Hand-checkable cases of the restatement: hover at a point, a straight constant-velocity line, the corridor reach of the ellipsoid."""
    params = dict(horiz_half_len=0.5, vert_half_len=0.15, grav_acc=9.81)
    ell, g = cr.params_of(params)
    box = np.concatenate([np.vstack([np.eye(3), np.ones((3, 3))]), np.vstack([-np.eye(3), -np.ones((3, 3))])], axis=1)   # |x|, |y|, |z| <= 1
    c = np.zeros((6, 3)); c[1] = (0.5, 0.0, 0.0)                          # x = 0.5 s
    r = cr.piece_row(c, 1.0, 4, box, ell, g)
    # level flight: zB = e3, the body's reach along x is the horizontal half-length; worst at s = 1 against face 0 (x <= 1)
    assert r[0] == pytest.approx(0.5 + 0.5 - 1.0, abs=1e-15) and r[6] == 1.0 and r[7] == 0.0
    assert r[1] == 0.5 and r[2] == r[3] == 9.81 and r[4] == 0.0 and r[5] == 0.0
    c[0] = (0.0, 0.0, 0.9)                                                 # 0.9 + 0.15 past z <= 1 at every sample: first sample, face 2
    r = cr.piece_row(c, 1.0, 4, box, ell, g)
    assert r[0] == pytest.approx(0.05, abs=1e-15) and r[6] == 0.0 and r[7] == 2.0
    cand = cr.reduce_candidates(np.array([r, r]), np.array([1.0, 2.0]), [0, 2])
    assert cand[0, 7] == 0.0 and cand[0, 6] == 0.0
    rows = np.array([r, r]); rows[1, 0] = np.nan
    cand = cr.reduce_candidates(rows, np.array([1.0, 2.0]), [0, 2])
    assert np.isnan(cand[0, 0]) and cand[0, 7] == 1.0 and cand[0, 6] == 1.0
    fl = cr.flags_of(cand, dict(vel_max=14.0, thr_acc_min=5.0, thr_acc_max=12.0, body_rate_max=3.8))
    assert fl[0] == 32
