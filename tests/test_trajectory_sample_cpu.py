"""frx_trajectory_sample without a device: the entry points exist, bad arguments are refused before any device work, and the numpy restatement
the GPU tests compare against (tests/sample_reference.py) agrees with the wire-format sampler (frx_msg_sample, pinned to the reference's
trajectory.hpp by tests/test_next_rows.py), with the geometry of its own attitude and body rates, and with the check's body rate."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_reference as cr  # noqa: E402
import sample_reference as sr  # noqa: E402

G = 9.81


def test_entry_points_are_exported(frx):
    L = C.CDLL(frx.LIB_PATH)
    assert hasattr(L, "frx_trajectory_sample") and hasattr(L, "frx_trajectory_sample_device")
    assert "frx_trajectory_sample" in frx.ABI_SYMBOLS and "frx_trajectory_sample_device" in frx.ABI_SYMBOLS
    assert frx.SAMPLE_FIELDS == sr.FIELDS == 20 and frx.SAMPLE_VIEWS == sr.VIEWS


def test_invalid_arguments(frx):
    L = frx.lib()
    T = np.zeros(1); Cf = np.zeros(18); out = np.zeros(40); tm = np.zeros(2)
    t, c, o = T.ctypes.data, Cf.ctypes.data, out.ctypes.data
    assert L.frx_trajectory_sample(None, t, c, 2, 0.0, 0.0, None, o) == -1
    assert L.frx_trajectory_sample_device(None, t, c, 2, 0.0, 0.0, None, o, None) == -1
    # a handle-shaped placeholder: the arguments are refused before the handle is ever read
    fake = C.create_string_buffer(64)
    h = C.cast(fake, C.c_void_p)
    for fn, extra in ((L.frx_trajectory_sample, ()), (L.frx_trajectory_sample_device, (None,))):
        assert fn(h, None, c, 2, 0.0, 0.0, None, o, *extra) == -1
        assert fn(h, t, None, 2, 0.0, 0.0, None, o, *extra) == -1
        assert fn(h, t, c, 2, 0.0, 0.0, None, None, *extra) == -1
        for S in (0, -1):
            assert fn(h, t, c, S, 0.0, 0.01, None, o, *extra) == -1 and b"n_samples" in L.frx_last_error()
            assert fn(h, t, c, S, 0.0, 0.0, tm.ctypes.data, o, *extra) == -1
        assert fn(h, t, c, 1, 0.0, 0.0, None, o, *extra) == -1 and b"dt == 0" in L.frx_last_error()    # spread over the duration: S >= 2
        for t0, dt in ((0.0, -0.01), (0.0, -np.inf), (0.0, np.nan), (0.0, np.inf), (np.nan, 0.01), (np.inf, 0.0), (-np.inf, 0.01)):
            assert fn(h, t, c, 8, t0, dt, None, o, *extra) == -1 and b"dt" in L.frx_last_error(), (t0, dt)
    assert not fake.raw.strip(b"\0")                    # nothing was written through it


def _trajectories(sc, ob):
    """Two optimised trajectories of the CPU oracle and one of random quintics."""
    out = []
    for sid in (2, 5):
        r = ob.Oracle(sc.make_candidate(sid, 10, 2), sc.ZHANGJIAJIE, qd_intervals=8).optimize(1e-6, max_iterations=80)
        out.append((np.asarray(r["T"]), np.asarray(r["C"])))
    rng = np.random.default_rng(3)
    out.append((rng.uniform(0.2, 2.0, 5), rng.normal(0, 1, (30, 3))))
    return out


def _interior_times(T, rng, n=60):
    """Times at least 1e-3 s away from every knot and both ends."""
    cum = sr.prefix_sums(T)
    i = rng.integers(0, len(T), n)
    return cum[i] + 1e-3 + rng.uniform(0.0, 1.0, n) * (T[i] - 2e-3)


def test_flat_state_agrees_with_msg_sample(frx, sc, ob):
    rng = np.random.default_rng(0)
    for T, Cf in _trajectories(sc, ob):
        msg = frx.traj_to_msg(T, Cf)
        t = _interior_times(T, rng)
        rows = sr.sample_candidate(T, Cf, t, G)
        for k, tk in enumerate(t):
            for got, sl in zip(frx.msg_sample(msg, float(tk)), ("pos", "vel", "acc", "jerk")):
                want = rows[k, sr.VIEWS[sl]]
                assert np.all(np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want))), (sl, tk, got, want)


def test_quaternion_rebuilds_the_frame(sc, ob):
    rng = np.random.default_rng(1)
    for T, Cf in _trajectories(sc, ob):
        t = _interior_times(T, rng)
        rows = sr.sample_candidate(T, Cf, t, G)
        q = rows[:, sr.VIEWS["quat"]]
        assert np.all(np.abs(np.linalg.norm(q, axis=1) - 1.0) <= 1e-12) and np.all(q[:, 0] >= 0.0)
        _, R, _ = sr.frame(rows[:, sr.VIEWS["acc"]], G)
        assert np.abs(sr.quat_to_R(q) - R).max() <= 1e-12
    # this frame has R00 = |(0, zB.z, -zB.y)| >= 0 >= R11, R22 when zB.z < 0 and trace >= R00, R11, R22 when zB.z >= 0: the trace and R00 branches
    # are the ones that occur; accelerations in every direction reach both, and zB = e2 ties the trace with R00 (= 1)
    acc = np.concatenate([np.random.default_rng(4).normal(0.0, 30.0, (4000, 3)), [[0.0, 30.0, -G], [0.0, 0.0, -20.0]]])
    _, R, _ = sr.frame(acc, G)
    q = sr.quaternion(R)
    assert np.all(np.abs(np.linalg.norm(q, axis=1) - 1.0) <= 1e-12) and np.all(q[:, 0] >= 0.0) and np.abs(sr.quat_to_R(q) - R).max() <= 1e-12
    tr = np.trace(R, axis1=1, axis2=2)
    assert (tr >= R[:, 0, 0]).any() and (tr < R[:, 0, 0]).any() and tr[-2] == R[-2, 0, 0] == 1.0


def test_body_rates_are_the_derivative_of_the_frame(sc, ob):
    """omega (body frame) matches the central difference R^T (R(t + d) - R(t - d)) / (2 d) to about 1e-6 relative."""
    rng = np.random.default_rng(2)
    d = 1e-5
    for T, Cf in _trajectories(sc, ob):
        t = _interior_times(T, rng, 40)
        rows = sr.sample_candidate(T, Cf, t, G)
        Rp = sr.quat_to_R(sr.sample_candidate(T, Cf, t + d, G)[:, sr.VIEWS["quat"]])
        Rm = sr.quat_to_R(sr.sample_candidate(T, Cf, t - d, G)[:, sr.VIEWS["quat"]])
        R = sr.quat_to_R(rows[:, sr.VIEWS["quat"]])
        W = np.einsum("nji,njk->nik", R, (Rp - Rm) / (2 * d))                   # R^T R' = [omega]x
        num = np.stack([W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]], axis=1)
        om = rows[:, sr.VIEWS["omega"]]
        scale = max(1.0, np.abs(om).max())
        assert np.abs(num - om).max() <= 1e-6 * scale, np.abs(num - om).max()
        assert np.abs(W + W.transpose(0, 2, 1)).max() <= 1e-6 * scale             # (a rotation's derivative: skew)


def test_body_rate_is_the_checks(sc, ob):
    """|omega_xy| is the quantity frx_trajectory_check limits (its restatement, tests/check_reference.py), at the check's own samples."""
    box = np.concatenate([np.vstack([np.eye(3), 1e3 * np.ones((3, 3))]), np.vstack([-np.eye(3), -1e3 * np.ones((3, 3))])], axis=1)
    M = 64
    for T, Cf in _trajectories(sc, ob):
        Cp = Cf.reshape(-1, 6, 3)
        for i in range(len(T)):
            chk = cr.piece_samples(Cp[i], float(T[i]), M, box, (0.5, 0.5, 0.15), G)
            rows = sr.sample_candidate(T[i:i + 1], Cp[i], chk["s"], G)
            bdr = np.linalg.norm(rows[:, 17:19], axis=1)
            assert np.all(np.abs(bdr - chk["body_rate"]) <= 1e-12 * np.maximum(1.0, chk["body_rate"]))
            assert np.all(np.abs(rows[:, 12] - chk["thrust"]) <= 1e-12 * chk["thrust"])


def test_time_rules(frx, sc, ob):
    """Knot times stay in the earlier piece (traj_server's rule), times before the start give the start, times past the end hold the end
    (where traj_server extrapolates the last piece), NaN gives a row of NaN."""
    T, Cf = _trajectories(sc, ob)[0]
    cum = sr.prefix_sums(T)
    i, s = sr.locate(T, cum[1:])
    assert np.array_equal(i, np.arange(len(T))) and np.array_equal(s, cum[1:] - cum[:-1])
    i, s = sr.locate(T, [0.0, -0.0, -1.0, -np.inf, cum[-1], cum[-1] + 3.0, np.inf])
    assert np.array_equal(i, [0, 0, 0, 0, len(T) - 1, len(T) - 1, len(T) - 1]) and np.array_equal(s[:4], [0, 0, 0, 0])
    rows = sr.sample_candidate(T, Cf, [0.0, -1.0, cum[-1], cum[-1] + 3.0, np.inf, np.nan] + list(cum[1:-1]), G)
    assert np.array_equal(rows[1], rows[0]) and np.array_equal(rows[3], rows[2]) and np.array_equal(rows[4], rows[2])
    assert np.isnan(rows[5]).all() and np.isfinite(rows[:5]).all() and np.isfinite(rows[6:]).all()
    msg = frx.traj_to_msg(T, Cf)
    for k, tk in enumerate(cum[1:-1]):
        for got, sl in zip(frx.msg_sample(msg, float(tk)), ("pos", "vel", "acc", "jerk")):
            want = rows[6 + k, sr.VIEWS[sl]]
            assert np.all(np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want))), (sl, k)
    p_end = frx.msg_sample(msg, float(cum[-1]))[0]
    p_past = frx.msg_sample(msg, float(cum[-1] + 3.0))[0]
    assert np.allclose(p_end, rows[2, :3], rtol=0, atol=1e-9) and not np.allclose(p_past, rows[3, :3], rtol=0, atol=1e-3)
    # the time modes: t0 + s dt, and S points over the duration (the last one the end: clamped where s (total / (S - 1)) rounds past it)
    assert np.array_equal(sr.sample_times(T, 5, 0.25, -0.5), -0.5 + np.arange(5) * 0.25)
    tt = sr.sample_times(T, 7)
    assert tt[0] == 0.0 and abs(tt[-1] - cum[-1]) <= 4e-16 * cum[-1]
