"""States of the exact clearance certificate (frx_trajectory_clearance_exact, frx_clear_exact_kernel.hpp) - test infrastructure, not a test module.

  crafted states   straight constant-velocity pieces of length L flown in T at hover thrust (a = 0, zB = e3), so that q = (dx^2 + dy^2) / eh^2 + dz^2 / ev^2 and
                   every minimum has a closed form; a piece in free fall; a handle whose ellipsoid is a sphere.  Each state: dict(params, T (N,), C (6N, 3),
                   obs (n, 3), expect (per piece: field -> value, or "nan"), cand (field -> value or None), set / clear (flag bits of the candidate)).
  clouds           near_cloud: points within `reach` metres of a point on the batch's paths; spread_cloud: points over the batch's bounding box.
  chunks           the launch rule (cloud_split of frx_traj_host.hpp with the constants of frx_device.hpp) restated.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clear_states import LOOSE, handle, line_piece  # noqa: E402,F401

CHUNK, TARGET_WGS, PARTIAL = 1024, 1024, 10
FLAG_COLLISION, FLAG_NONFINITE = 1, 2
FIELDS = ("ell", "dist", "t_ell", "i_ell", "t_dist", "i_dist")
NAN_ = float("nan")
L_RACE, T_RACE, Z = 4.0, 0.4, 1.5                                        # a racing piece: 4 m at 10 m/s


def chunks(P, n_obs, force=0):
    """(points per chunk, chunks per piece) of an exact clearance launch."""
    c = force
    if force <= 0:
        want = TARGET_WGS // P if P < TARGET_WGS else 1
        c = -(-n_obs // want)
        c = -(-c // CHUNK) * CHUNK
    return min(c, n_obs), -(-n_obs // c)


def workspace_bytes(P, n_obs, force=0):
    return 8 * PARTIAL * P * chunks(P, n_obs, force)[1]


def straight(n=1, L=L_RACE, T=T_RACE, z=Z):
    """n consecutive straight pieces along x from the origin's height z: (T (n,), C (6n, 3))"""
    return np.full(n, T), np.concatenate([line_piece((k * L, 0.0, z), ((k + 1) * L, 0.0, z), T) for k in range(n)])


def loose(base, **kw):
    p = dict(base)
    p.update(LOOSE)
    p.update(kw)
    return p


def crafted(base):
    p = loose(base)
    eh, ev, g = p["horiz_half_len"], p["vert_half_len"], p["grav_acc"]
    L, T, z = L_RACE, T_RACE, Z
    far = [L / 2, 30.0, z]
    st = {}
    T1, C1 = straight(1)
    y0 = 0.9 * eh
    st["a_beside"] = dict(params=p, T=T1, C=C1, obs=np.array([far, [L / 3, y0, z]]),
                          expect=[dict(ell=0.9, dist=y0, t_ell=T / 3, i_ell=1, t_dist=T / 3, i_dist=1)], cand=dict(ell=0.9, t_ell=T / 3), set=FLAG_COLLISION, clear=FLAG_NONFINITE)
    st["a_beside_below"] = dict(params=p, T=T1, C=C1, obs=np.array([[L / 3, -1.25 * eh, z], far]),
                                expect=[dict(ell=1.25, dist=1.25 * eh, t_ell=T / 3, i_ell=0, t_dist=T / 3, i_dist=0)], cand=None, set=0, clear=FLAG_COLLISION | FLAG_NONFINITE)
    s = 1.5
    st["b_above"] = dict(params=p, T=T1, C=C1, obs=np.array([far, far, [L / 3, 0.0, z + s * ev]]),
                         expect=[dict(ell=s, dist=s * ev, t_ell=T / 3, i_ell=2, t_dist=T / 3, i_dist=2)], cand=dict(ell=s), set=0, clear=FLAG_COLLISION | FLAG_NONFINITE)
    # the nearest point in metres is not the nearest in the ellipsoid's measure: 0.4 m above (q = (0.4 / ev)^2) against 0.6 m beside (q = (0.6 / eh)^2)
    st["b_two_measures"] = dict(params=p, T=T1, C=C1, obs=np.array([[L / 4, 0.0, z + 0.4], [3 * L / 4, 0.6, z]]),
                                expect=[dict(ell=0.6 / eh, dist=0.4, t_ell=3 * T / 4, i_ell=1, t_dist=T / 4, i_dist=0)], cand=None, set=0, clear=FLAG_COLLISION | FLAG_NONFINITE)
    st["c_on_the_path"] = dict(params=p, T=T1, C=C1, obs=np.array([far, [L / 4, 0.0, z]]),
                               expect=[dict(ell=(0.0, 1e-7), dist=(0.0, 1e-7), i_ell=1, i_dist=1, t_ell=(T / 4, 1e-6), t_dist=(T / 4, 1e-6))], cand=None,
                               set=FLAG_COLLISION, clear=FLAG_NONFINITE)
    T2, C2 = straight(2)
    st["d_knot"] = dict(params=p, T=T2, C=C2, obs=np.array([[L, 0.75, z], [L / 2, 40.0, z]]),
                        expect=[dict(ell=0.75 / eh, dist=0.75, t_ell=T, i_ell=0, t_dist=T, i_dist=0), dict(ell=0.75 / eh, dist=0.75, t_ell=0.0, i_ell=0, t_dist=0.0, i_dist=0)],
                        cand=dict(ell=0.75 / eh, dist=0.75, t_ell=T, t_dist=T), set=0, clear=FLAG_COLLISION | FLAG_NONFINITE)
    fall = np.zeros((6, 3))
    fall[0] = (0.0, 0.0, z); fall[1] = (2.0, 0.0, 1.0); fall[2] = (0.0, 0.0, -0.5 * g)
    st["e_free_fall"] = dict(params=p, T=np.array([0.5]), C=fall, obs=np.array([[0.5, 1.0, z], [0.0, 9.0, z]]),
                             expect=[dict(ell=NAN_, i_ell=0, t_ell=0.0, i_dist=0)], cand=dict(ell=NAN_), set=FLAG_NONFINITE, clear=0)
    # thrust zero at the start only (a = -g e3 there, then 6 t e3): q = NaN at tau = 0 for EVERY point, so the points tie and the lowest index wins - the far one
    start = fall.copy()
    start[3] = (0.0, 0.0, 1.0)
    st["e_zero_thrust_at_the_start"] = dict(params=p, T=np.array([0.5]), C=start, obs=np.array([[0.0, 90.0, z], [0.5, 1.0, z]]),
                                            expect=[dict(ell=NAN_, i_ell=0, t_ell=0.0, i_dist=1)], cand=dict(ell=NAN_), set=FLAG_NONFINITE, clear=0)
    # thrust zero at the end only, with numbers that make it exact: g = 8, T = 1/2, a(t) = (-11 + 6 t) e3, so wh(1) = (-0.75 + 0.75) e3 = 0
    end = fall.copy()
    end[2] = (0.0, 0.0, -5.5); end[3] = (0.0, 0.0, 1.0)
    st["e_zero_thrust_at_the_end"] = dict(params=loose(base, grav_acc=8.0), T=np.array([0.5]), C=end, obs=np.array([[0.0, 90.0, z], [0.5, 1.0, z], [0.4, 1.2, z]]),
                                          expect=[dict(ell=NAN_, i_ell=0, t_ell=0.5)], cand=dict(ell=NAN_), set=FLAG_NONFINITE, clear=0)
    ps = loose(base, vert_half_len=eh)
    st["f_sphere"] = dict(params=ps, T=T1, C=C1, obs=np.array([[L / 3, 0.6, z + 0.8], far]),
                          expect=[dict(ell=1.0 / eh, dist=1.0, t_ell=T / 3, i_ell=0, t_dist=T / 3, i_dist=0)], cand=None, set=0, clear=FLAG_COLLISION | FLAG_NONFINITE)
    bad = C1.copy()
    bad[3, 1] = np.inf
    st["g_not_finite"] = dict(params=p, T=np.array([T, T, -1.0]), C=np.concatenate([C1, bad, C1]), obs=np.array([[L / 3, 1.0, z]]),
                              expect=[dict(ell=1.0 / eh, dist=1.0), "nan", "nan"], cand=dict(ell=NAN_, dist=NAN_), set=FLAG_NONFINITE, clear=0)
    for s_ in st.values():
        s_["counts"] = [len(s_["T"])]
    return st


def expectation_failures(row, expect, tol=1e-9):
    """deviations of a row from a crafted state's closed-form values: expect maps a field name to a value (compared to tol max(1, |value|); an int exactly)
    or to a (value, tol) pair"""
    bad = []
    for name, val in expect.items():
        t = tol
        if isinstance(val, tuple):
            val, t = val
        got = row[FIELDS.index(name)]
        if isinstance(val, int):
            ok = got == val
        else:
            ok = (val != val and got != got) or abs(got - val) <= t * max(1.0, abs(val))
        if not ok:
            bad.append((name, float(got), val))
    return bad


def positions(T, Cf, piece, tau):
    """p(tau T) of the pieces `piece` (arrays)"""
    Cp = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    t = (np.asarray(tau) * np.asarray(T)[piece])[:, None]
    return sum(Cp[piece, k] * t ** k for k in range(6))


def near_cloud(rng, T, Cf, n, reach=2.0):
    """n points, each within `reach` metres of a point on one of the batch's paths"""
    P = len(T)
    piece = rng.integers(0, P, n)
    at = positions(T, Cf, piece, rng.uniform(0.0, 1.0, n))
    d = rng.normal(0.0, 1.0, (n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.ascontiguousarray(at + d * rng.uniform(0.05, reach, n)[:, None])


def spread_cloud(rng, T, Cf, n, margin=1.0):
    """n points over the bounding box of the batch's knots, grown by margin"""
    Cp = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    ends = np.concatenate([Cp[:, 0], positions(T, Cf, np.arange(len(T)), np.ones(len(T)))])
    return rng.uniform(ends.min(axis=0) - margin, ends.max(axis=0) + margin, (n, 3))
