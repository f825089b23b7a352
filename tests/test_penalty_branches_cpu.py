"""Every branch of the penalty integrand (frx_math.hpp: penalty_sample), in its host build (tests/hostcheck), against the oracle on
branch-isolated states (tests/penalty_states.py), and the oracle's own analytic gradient against central differences of its cost where
each branch is live.  Errors are normalised per state and per piece, never over a gradient that mixes terms of different size."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import penalty_states as ps  # noqa: E402
from test_hostcheck import _load_hostcheck  # noqa: E402

TOL = 1e-10


@pytest.fixture(scope="module")
def hc():
    return _load_hostcheck()


@pytest.fixture(scope="module")
def states(sc, ob):
    out = ps.limit_states(sc, ob, 8, iterate=0) + ps.limit_states(sc, ob, 8, iterate=15) + ps.corridor_states(sc, ob, 16) + ps.corridor_states(sc, ob, 8)
    for s in out:
        s.name += f"/k{s.kappa}"
        ps.check(s, sc.ZHANGJIAJIE)
    return out


def pc_vector(p):
    return np.array([p["horiz_half_len"], p["horiz_half_len"], p["vert_half_len"], p["safe_margin"], p["vel_max"], p["thr_acc_min"],
                     p["thr_acc_max"], p["body_rate_max"], p["grav_acc"], *p["penalty_pvtb"]])


def oracle_penalty(ob, sc, s, b):
    o = ob.Oracle(s.cands[b], sc.ZHANGJIAJIE, qd_intervals=s.kappa, **s.override)
    o.set_abscissa_mode(False)
    off = s.piece_off
    return o.penalty(s.T[off[b]:off[b + 1]], s.C[6 * off[b]:6 * off[b + 1]])


def host_penalty(hc, sc, s, b):
    c = s.cands[b]
    h_off, h_rec, _, _ = c.packed()
    hr = h_rec.reshape(-1, 6).copy()
    hr[:, :3] /= np.linalg.norm(hr[:, :3], axis=1)[:, None]
    off = s.piece_off
    N = c.coarse_n
    out = np.zeros(20 * N)
    hc.hostcheck_penalty(N, s.kappa, np.ascontiguousarray(s.T[off[b]:off[b + 1]]), np.ascontiguousarray(s.C[6 * off[b]:6 * off[b + 1]].reshape(-1)),
                         h_off, np.ascontiguousarray(hr.reshape(-1)), pc_vector(s.params(sc.ZHANGJIAJIE)), 0, out)
    out = out.reshape(-1, 20)
    return out[:, 0].sum(), out[:, 1].copy(), out[:, 2:].reshape(-1, 3)


def compare(name, got, ref, tol, T):
    """(cost, gdT (N,), gdC (6N, 3)) against the oracle: cost relative; per piece the gradient in the piece's own time unit (T gdT, gdC_k / T^k)
    relative to its largest entry; a piece whose oracle block is exactly zero must be exactly zero, and a piece the oracle sees active must not be."""
    cost, gdT, gdC = got
    c_ref, gT_ref, gC_ref = ref
    assert abs(cost - c_ref) <= tol * abs(c_ref), f"{name}: cost {cost!r} vs {c_ref!r}"
    N = gT_ref.size
    worst = 0.0
    for i in range(N):
        sk = T[i] ** np.arange(6)[:, None]
        g = np.concatenate([[gdT[i] * T[i]], (gdC[6 * i:6 * i + 6] / sk).ravel()])
        g_ref = np.concatenate([[gT_ref[i] * T[i]], (gC_ref[6 * i:6 * i + 6] / sk).ravel()])
        if not g_ref.any():
            assert not g.any(), f"{name} piece {i}: inactive in the oracle, {g} here"
            continue
        assert g.any(), f"{name} piece {i}: active in the oracle, all zero here"
        err = np.abs(g - g_ref).max() / np.abs(g_ref).max()
        worst = max(worst, err)
        assert err <= tol, f"{name} piece {i}: gradient differs by {err:.2e} of its largest entry"
    return worst


def test_states_activate_the_terms_they_claim(states):
    """The builders' self-checks have run (fixture); here the counts are reported and the coverage the suite relies on is pinned."""
    names = set()
    for s in states:
        print(f"{s.name:28s} terms {'+'.join(s.terms):44s} active samples {s.counts}")
        names.add(s.name.split("@")[0].split("/")[0])
    assert {"corridor", "speed", "thrust_min", "thrust_max", "body_rate", "all", "corridor_face", "corridor_edge", "corridor_corner", "corridor_K",
            "corridor_guard"} <= names
    assert max(s.counts["max_faces"] for s in states) >= 3
    ks = {K for s in states if s.name.startswith("corridor_K") for K in (h.shape[1] for h in s.cands[0].h_polys)}
    assert {K % 4 for K in ks} == {0, 1, 2, 3} and min(ks) == 1 and max(ks) >= 40


def test_hostcheck_matches_oracle_on_every_branch(hc, sc, ob, states):
    for s in states:
        for b in range(len(s.cands)):
            off = s.piece_off
            compare(f"{s.name} cand {b}", host_penalty(hc, sc, s, b), oracle_penalty(ob, sc, s, b), TOL, s.T[off[b]:off[b + 1]])


def test_guard_band_pieces_are_active_exactly_where_the_oracle_says(hc, sc, ob):
    """The pre-reject (d0 < -emax (1 + 2^-20) skips the full test) must never drop a half-space the full test would flag: pieces at sd = 2^-22,
    d0 = -emax + 2^-22, are active; their signed distance is exact in both implementations, so the values agree to rounding."""
    s = ps.guard_state(sc, 8)
    ps.check(s, sc.ZHANGJIAJIE)
    ref = oracle_penalty(ob, sc, s, 0)
    active = np.array([np.any(ref[1][i]) or np.any(ref[2][6 * i:6 * i + 6]) for i in range(ref[1].size)])
    assert list(active) == [True, True, False, False, True, True, True]
    compare(s.name, host_penalty(hc, sc, s, 0), ref, 1e-13, s.T)


def _fd_check(name, fn, T, Cf, tol=1e-6):
    """Central differences of cost = fn(T, C) against its gradient (gdT, gdC): per piece, relative to the piece's largest scaled entry."""
    cost, gdT, gdC = fn(T, Cf)
    assert cost > 0.0
    N = T.size
    fdT, fdC = np.zeros(N), np.zeros_like(Cf)
    for i in range(N):
        h = 1e-6 * T[i]
        Tp, Tm = T.copy(), T.copy(); Tp[i] += h; Tm[i] -= h
        fdT[i] = (fn(Tp, Cf)[0] - fn(Tm, Cf)[0]) / (2 * h)
        for k in range(6):
            for d in range(3):
                r = 6 * i + k
                hc_ = 1e-6 / T[i] ** k
                Cp, Cm = Cf.copy(), Cf.copy(); Cp[r, d] += hc_; Cm[r, d] -= hc_
                fdC[r, d] = (fn(T, Cp)[0] - fn(T, Cm)[0]) / (2 * hc_)
    for i in range(N):
        sc_k = T[i] ** np.arange(6)[:, None]                                       # d cost / d c_k in the piece's own time unit
        g = np.concatenate([[gdT[i] * T[i]], (gdC[6 * i:6 * i + 6] / sc_k).ravel()])
        f = np.concatenate([[fdT[i] * T[i]], (fdC[6 * i:6 * i + 6] / sc_k).ravel()])
        if not g.any():
            continue
        err = np.abs(g - f).max() / np.abs(g).max()
        assert err <= tol, f"{name} piece {i}: finite differences differ by {err:.2e} of the largest entry"


def test_oracle_gradient_matches_finite_differences_on_every_branch(sc, ob):
    for s in ps.small_states(sc, ob):
        ps.check(s, sc.ZHANGJIAJIE, min_samples=2)
        o = ob.Oracle(s.cands[0], sc.ZHANGJIAJIE, qd_intervals=s.kappa, **s.override)
        o.set_abscissa_mode(False)
        _fd_check(s.name, o.penalty, s.T, s.C)
