"""Branch-isolated states of the penalty integrand (frx_math.hpp: penalty_sample) - test infrastructure, not a test module.

The scenario generator's states leave most branches of the integrand cold: with the stock limits almost no sample touches a corridor face or
falls below the thrust minimum.  A State here is (parameter override, candidates, T, C[, x]) chosen so that a named set of the five penalty
terms fires and the others cannot, built in two ways:

  limit overrides   every limit but the one under test relaxed beyond reach (RELAXED, and a negative safe margin for the corridor), the one
                    under test set from the state's own samples so that about a third of them violate it;
  corridor states   the pieces' constant coefficients c0 shifted so that chosen faces sit at a chosen signed distance at one sample, the
                    polytopes padded with redundant half-spaces (outside the cell's vertices: the V-polytopes stay valid) to set K per piece,
                    and exact-arithmetic pieces on both sides of the pre-reject guard d0 = -max(ell) (1 + 2^-20).

check() counts, with check_reference.piece_samples, the active samples of every term and fails unless each intended term has enough of them
and every other term has none, so that a change of the scenario generator makes the tests fail instead of going vacuous.
Sample abscissae are s = (T / kappa) j, the device's form (oracle.set_abscissa_mode(False)).
"""
import os
import sys
from dataclasses import dataclass, field

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_reference as cr  # noqa: E402

TERMS = ("corridor", "speed", "thrust_min", "thrust_max", "body_rate")
LIMIT_OF = {"speed": "vel_max", "thrust_min": "thr_acc_min", "thrust_max": "thr_acc_max", "body_rate": "body_rate_max"}
RELAXED = dict(vel_max=1e4, thr_acc_min=0.0, thr_acc_max=1e4, body_rate_max=1e4)
NO_CORRIDOR = dict(safe_margin=-10.0)          # every signed distance of a trajectory inside (or near) its corridor is far below zero


@dataclass
class State:
    name: str
    cands: list
    override: dict
    kappa: int
    T: np.ndarray                              # (P,) durations of every piece of the batch
    C: np.ndarray                              # (6P, 3) coefficients, row = power
    terms: tuple                               # the terms the state means to activate
    x: list = None                             # per candidate: the decision vector T and C came from (limit states only)
    min_faces: int = 1                         # corridor: some sample must touch this many faces at once
    counts: dict = field(default_factory=dict)

    @property
    def piece_off(self):
        return np.concatenate([[0], np.cumsum([c.coarse_n for c in self.cands])]).astype(int)

    def params(self, base):
        p = dict(base)
        p.update(self.override)
        return p


def activity(state, base):
    """Per piece of the batch: dict(term -> bool array over the kappa + 1 samples), and 'faces' = corridor faces active per sample."""
    p = state.params(base)
    ell, g = cr.params_of(p)
    polys = [h for c in state.cands for h in c.h_polys]
    out = []
    for i, h in enumerate(polys):
        v = cr.piece_samples(state.C[6 * i:6 * i + 6], float(state.T[i]), state.kappa, h, ell, g)
        faces = (v["corridor"] + p["safe_margin"] > 0.0).sum(axis=1)
        out.append(dict(corridor=faces > 0, faces=faces, speed=v["speed"] > p["vel_max"], thrust_min=v["thrust"] < p["thr_acc_min"],
                        thrust_max=v["thrust"] > p["thr_acc_max"], body_rate=v["body_rate"] > p["body_rate_max"]))
    return out


def check(state, base, min_samples=3):
    """The state's self-check: active-sample counts per term (stored in state.counts and returned)."""
    act = activity(state, base)
    counts = {t: int(sum(a[t].sum() for a in act)) for t in TERMS}
    counts["max_faces"] = int(max(a["faces"].max() for a in act))
    state.counts = counts
    for t in TERMS:
        if t in state.terms:
            assert counts[t] >= min_samples, f"{state.name}: term {t} has {counts[t]} active samples, at least {min_samples} needed ({counts})"
        else:
            assert counts[t] == 0, f"{state.name}: term {t} is meant to be inactive but has {counts[t]} active samples ({counts})"
    if "corridor" in state.terms:
        assert counts["max_faces"] >= state.min_faces, f"{state.name}: no sample touches {state.min_faces} faces at once ({counts})"
    return counts


def _samples(cands, T, C, kappa, params):
    ell, g = cr.params_of(params)
    polys = [h for c in cands for h in c.h_polys]
    vs = [cr.piece_samples(C[6 * i:6 * i + 6], float(T[i]), kappa, h, ell, g) for i, h in enumerate(polys)]
    return {k: np.concatenate([v[k] for v in vs]) for k in ("speed", "thrust", "body_rate")}


def limit_states(sc, ob, kappa, iterate=0, scenario=31, N=16, gates=4, B=2, corridor_margin=0.6, quantile=0.3):
    """Limit-override states on B candidates of an obstacle scenario at the oracle's L-BFGS iterate `iterate` (stock parameters): one per
    term, each alone, and 'all' with the five together.  The limit under test is the sample quantile that leaves `quantile` of the samples
    in violation; the corridor is switched on by the raised safe margin."""
    base = sc.ZHANGJIAJIE
    cands = [sc.make_candidate(scenario, N, gates, perturb_id=b, obstacles=True) for b in range(B)]
    xs, Ts, Cs = [], [], []
    for c in cands:
        o = ob.Oracle(c, base, qd_intervals=kappa)
        o.set_abscissa_mode(False)
        x0 = o.initial_guess()
        x = x0 if iterate == 0 else o.optimize(1e-6, max_iterations=iterate, x0=x0)["x"]
        T, _, Cf = o.forward(x)
        xs.append(x); Ts.append(T); Cs.append(Cf)
    T, C = np.concatenate(Ts), np.concatenate(Cs)
    s = _samples(cands, T, C, kappa, base)
    tight = dict(vel_max=float(np.quantile(s["speed"], 1.0 - quantile)), thr_acc_min=float(np.quantile(s["thrust"], quantile)),
                 thr_acc_max=float(np.quantile(s["thrust"], 1.0 - quantile)), body_rate_max=float(np.quantile(s["body_rate"], 1.0 - quantile)))
    states = []
    for t in TERMS:
        if t == "corridor":
            over = dict(RELAXED, safe_margin=corridor_margin)
        else:
            over = dict(RELAXED, **NO_CORRIDOR)
            over[LIMIT_OF[t]] = tight[LIMIT_OF[t]]
        states.append(State(f"{t}@it{iterate}", cands, over, kappa, T, C, (t,), x=xs))
    states.append(State(f"all@it{iterate}", cands, dict(tight, safe_margin=corridor_margin), kappa, T, C, TERMS, x=xs))
    return states


# ---- constructed corridor states ----
def _redundant(rng, verts, count, gap=2.0):
    """`count` half-spaces (6 x count, column = (unit normal, point)) that hold every vertex of the cell `gap` metres inside."""
    cols = []
    for _ in range(count):
        n = np.array([rng.normal(), rng.normal(), rng.normal()])
        n /= np.linalg.norm(n)
        cols.append(np.concatenate([n, n * ((n @ verts).max() + gap)]))
    return np.array(cols).T.reshape(6, -1)


def _unit(h):
    return h[:3] / np.linalg.norm(h[:3], axis=0)


def _shift_to_faces(c, T, kappa, h, faces, targets, params, j_star=None):
    """c0 += delta so that the faces' signed distances (margin included) equal `targets` at sample j_star (default: each face's worst sample,
    for a single face; sample 0 for several)."""
    ell, g = cr.params_of(params)
    v = cr.piece_samples(c, T, kappa, h, ell, g)
    sd = v["corridor"] + params["safe_margin"]
    n = _unit(h)[:, faces].T                                                    # (F, 3)
    if len(faces) == 1:
        delta = n[0] * (targets[0] - sd[:, faces[0]].max())
    else:
        j = 0 if j_star is None else j_star
        delta = np.linalg.lstsq(n, np.asarray(targets) - sd[j, faces], rcond=None)[0]
    c = c.copy()
    c[0] += delta
    return c


def _base_pieces(sc, ob, scenario, N, gates, kappa):
    cand = sc.make_candidate(scenario, N, gates)
    o = ob.Oracle(cand, sc.ZHANGJIAJIE, qd_intervals=kappa)
    T, _, Cf = o.forward(o.initial_guess())
    return cand, T, Cf


def _corridor_state(sc, ob, name, kappa, scenario, N, gates, K_of, faces_of, targets_of, min_faces=1, seed=0):
    """Pieces of a scenario's initial guess, each shifted onto faces_of(i) of its own cell; the cell padded to K_of(i) half-spaces with the
    active faces LAST (K < 8: box faces dropped - a penalty-only geometry, the V-polytopes are the unpadded cell's)."""
    params = dict(sc.ZHANGJIAJIE, **RELAXED)
    cand, T, Cf = _base_pieces(sc, ob, scenario, N, gates, kappa)
    rng = sc.SplitMix64(7001 + seed)
    polys, C = [], Cf.copy()
    for i, h in enumerate(cand.h_polys):
        faces = list(faces_of(i))
        K = K_of(i)
        rest = [k for k in range(h.shape[1]) if k not in faces]
        hu = h.copy(); hu[:3] = _unit(h)
        if K >= h.shape[1]:
            hp = np.concatenate([hu[:, rest], _redundant(rng, cand.v_polys[2 * i], K - h.shape[1]), hu[:, faces]], axis=1)
        else:
            hp = np.concatenate([hu[:, rest[:K - len(faces)]], hu[:, faces]], axis=1)
        fpos = list(range(K - len(faces), K))
        C[6 * i:6 * i + 6] = _shift_to_faces(Cf[6 * i:6 * i + 6], float(T[i]), kappa, hp, fpos, targets_of(i), params)
        polys.append(hp)
    c2 = sc.Candidate(cand.ini_state, cand.fin_state, polys, cand.v_polys, cand.gates)
    return State(name, [c2], dict(RELAXED), kappa, T, C, ("corridor",), min_faces=min_faces)


def guard_state(sc, kappa):
    """Pieces that move in the y-z plane only with h = (0, 0, 8) (grav_acc = 8, no acceleration): xB = e_x, zB = e_z exactly, and the face
    n = e_x has |E R^T n| = max(ell) = 0.5 at every sample.  With safe_margin = 1/16 and dyadic offsets the signed distance is EXACT in every
    implementation: sd = 0.5625 - px.  Pieces on both sides of the pre-reject guard: sd = +2^-22 and +2^-23 (d0 inside the guard band
    (-emax (1 + 2^-20), -emax (1 - 2^-20)): active), -2^-22 and -2^-22 - 2^-23 (inactive), +2^-10 and +0.03 (d0 = -0.47, active)."""
    sds = [2.0 ** -22, 2.0 ** -23, -(2.0 ** -22), -(2.0 ** -22) - 2.0 ** -23, 2.0 ** -10, 0.03, 2.0 ** -22]
    margin = 0.0625
    polys, Cs, Ts = [], [], []
    for i, sd in enumerate(sds):
        px = 0.5625 - sd
        cols = [((1.0, 0, 0), (px, 0, 0)), ((-1.0, 0, 0), (-2.0, 0, 0)), ((0, 1.0, 0), (0, 8.0, 0)), ((0, -1.0, 0), (0, -4.0, 0)),
                ((0, 0, 1.0), (0, 0, 4.0)), ((0, 0, -1.0), (0, 0, -4.0))]
        if i == len(sds) - 1:                                              # the same face behind three others: K = 9, second chunk
            cols = cols[1:4] + [((0.6, 0.8, 0), (0, 8.0, 0)), ((0.6, -0.8, 0), (0, -4.0, 0))] + cols[4:] + [cols[0], ((-0.6, 0.8, 0), (0, 8.0, 0))]
        polys.append(np.array([np.concatenate([n, p]) for n, p in cols], dtype=np.float64).T)
        c = np.zeros((6, 3))
        c[0] = (0.0, -2.0 + 0.5 * i, 0.25 * i - 1.0)
        c[1] = (0.0, 1.0 + 0.25 * i, 0.0)
        Cs.append(c); Ts.append(0.5)
    v_polys = []
    for i in range(len(polys)):
        v_polys.append(sc.enumerate_vertices(polys[i]))
        if i + 1 < len(polys):
            v_polys.append(sc.enumerate_vertices(np.concatenate([polys[i], polys[i + 1]], axis=1)))
    ini = np.zeros((3, 3)); ini[:, 0] = Cs[0][0]
    fin = np.zeros((3, 3)); fin[:, 0] = Cs[-1][0] + 0.5 * Cs[-1][1]
    cand = sc.Candidate(ini, fin, polys, v_polys)
    return State("corridor_guard", [cand], dict(RELAXED, safe_margin=margin, grav_acc=8.0), kappa, np.array(Ts), np.concatenate(Cs), ("corridor",))


K_LIST = [1, 2, 3, 5, 6, 7, 9, 11, 12, 13, 14, 15, 17, 19, 22, 26, 31, 36, 39, 40]      # every residue mod 4, 1 .. 40


def corridor_states(sc, ob, kappa):
    """The constructed corridor states: one face per piece at sd 1e-4 .. 1e-2; edges (two faces at one sample); corners (three); K per piece
    over K_LIST with the active face the last record; and the pre-reject guard."""
    N = 8
    tg = np.geomspace(1e-4, 1e-2, N)
    return [
        _corridor_state(sc, ob, "corridor_face", kappa, 21, N, 2, lambda i: 8 + (i % 4), lambda i: [0], lambda i: [tg[i]]),
        _corridor_state(sc, ob, "corridor_edge", kappa, 22, N, 2, lambda i: 10, lambda i: [0, 7], lambda i: [tg[i], 2e-3], min_faces=2, seed=1),
        _corridor_state(sc, ob, "corridor_corner", kappa, 23, N, 2, lambda i: 13, lambda i: [0, 3, 7], lambda i: [3e-3, tg[i], 2e-3], min_faces=3, seed=2),
        _corridor_state(sc, ob, "corridor_K", kappa, 24, len(K_LIST), 5, lambda i: K_LIST[i], lambda i: [i % 2], lambda i: [1e-3 * (1 + i % 5)], seed=3),
        guard_state(sc, kappa),
    ]


def big_K_state(sc, ob, kappa, K=260):
    """corridor_K's geometry with one piece of K half-spaces: enough corridor records per workgroup that the large-batch integrator's four-wave
    workgroup no longer fits a CU's LDS and the launch steps down to fewer waves (frx_api.cpp: pen_lds)."""
    Ks = list(K_LIST)
    Ks[7] = K
    return _corridor_state(sc, ob, "corridor_bigK", kappa, 24, len(Ks), 5, lambda i: Ks[i], lambda i: [i % 2], lambda i: [1e-3 * (1 + i % 5)], seed=3)


def small_states(sc, ob, kappa=8, N=4):
    """One small state (N pieces) per term for finite differences: the limit terms from the limit overrides on a scenario's initial guess, the
    corridor from one face per piece."""
    st = [s for s in limit_states(sc, ob, kappa, iterate=0, scenario=41, N=N, gates=0, B=1) if s.terms != TERMS and s.terms != ("corridor",)]
    tg = np.geomspace(1e-3, 1e-2, N)
    st.append(_corridor_state(sc, ob, "corridor_small", kappa, 42, N, 0, lambda i: 9, lambda i: [0] if i % 2 else [0, 7], lambda i: [tg[i]] + [3e-3] * (i % 2 == 0)))
    return st


TIGHT = dict(vel_max=6.0, thr_acc_min=9.3, thr_acc_max=10.3, body_rate_max=0.8)   # every limit tight at once (whole optimisations)
