"""Independent numpy restatement of the clearance check against the obstacle cloud (frx_trajectory_clearance, include/frx.h) - test
infrastructure, not a test module.  Written from the header's rules; the frame comes from sample_reference.frame (the restatement the sampler
and the check are tested against), every point is brute-forced:

  s_j = (T / M) * j, j = 0..M                                       (step first, then multiplied, as check_reference does)
  p = c^T (1, s, .., s^5);  h = acc + gAcc e3;  R = [xB yB zB](h)   (sample_reference.flat_state / frame)
  u = o_i - p;  q = (xB.u / e0)^2 + (yB.u / e1)^2 + (zB.u / e2)^2;  r = u.u
  row = (sqrt(min q), sqrt(min r), s_j, i) of the first (j, i) in lexicographic order that attains min q; a NaN q first of all
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_reference as sr  # noqa: E402

FIELDS = ("ell", "dist", "worst_t", "worst_i")
FLAG_COLLISION, FLAG_NONFINITE = 1, 2


def params_of(params):
    ell = (params["horiz_half_len"], params["horiz_half_len"], params["vert_half_len"])
    return ell, params["grav_acc"]


def q_r(p, R, ell, obs):
    """q (S, n) and r (S, n) of the bodies at p (S, 3) with frames R (S, 3, 3; columns xB, yB, zB) and semi-axes ell against obs (n, 3)."""
    u = np.asarray(obs, dtype=np.float64)[None, :, :] - np.asarray(p, dtype=np.float64)[:, None, :]      # the difference first
    d = np.einsum("sik,sni->snk", R, u) / np.asarray(ell, dtype=np.float64)[None, None, :]               # (axis_k . u) / e_k
    return (d ** 2).sum(axis=2), (u ** 2).sum(axis=2)


def piece_q_r(c, T, M, obs, ell, g_acc):
    """dict(s (M + 1,), q (M + 1, n), r (M + 1, n)) of one piece: c (6, 3) coefficients, row k = power k."""
    c = np.asarray(c, dtype=np.float64).reshape(6, 3)
    step = T / M
    s = step * np.arange(M + 1, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pos, _, acc, _ = sr.flat_state(np.broadcast_to(c, (M + 1, 6, 3)), s)
        _, R, _ = sr.frame(acc, g_acc)
        q, r = q_r(pos, R, ell, obs)
    return dict(s=s, q=q, r=r)


def piece_row(c, T, M, obs, ell, g_acc):
    v = piece_q_r(c, T, M, obs, ell, g_acc)
    q, r = v["q"], v["r"]
    nanm = np.isnan(q)
    flat = int(np.argmax(nanm.reshape(-1))) if nanm.any() else int(np.argmin(q.reshape(-1)))      # first occurrence in (j, i) order
    j, i = divmod(flat, q.shape[1])
    return np.array([np.sqrt(q[j, i]), np.nan if np.isnan(r).any() else np.sqrt(r.min()), v["s"][j], float(i)])


def clear_pieces(T, Cf, obs, params, M):
    """Rows (P, 4) of a batch: T (P,), Cf (6P, 3), obs (n, 3)."""
    ell, g = params_of(params)
    Cf = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    return np.array([piece_row(Cf[i], float(T[i]), M, obs, ell, g) for i in range(len(T))])


def reduce_candidates(rows, T, piece_off):
    """Candidate rows (B, 4) from piece rows: the first NaN piece, else the first piece with the smallest ell; worst_t from the candidate's start
    (durations summed left to right); dist a NaN-propagating min."""
    out = []
    for b in range(len(piece_off) - 1):
        r = rows[piece_off[b]:piece_off[b + 1]]
        t = np.asarray(T[piece_off[b]:piece_off[b + 1]], dtype=np.float64)
        nanm = np.isnan(r[:, 0])
        k = int(np.argmax(nanm)) if nanm.any() else int(np.argmin(r[:, 0]))
        start = 0.0
        for q in range(k):
            start += t[q]
        out.append([r[k, 0], np.nan if np.isnan(r[:, 1]).any() else r[:, 1].min(), start + r[k, 2], r[k, 3]])
    return np.array(out)


def flags_of(cand):
    f = np.zeros(len(cand), np.uint32)
    with np.errstate(invalid="ignore"):
        f |= np.where(cand[:, 0] < 1.0, FLAG_COLLISION, 0).astype(np.uint32)
        f |= np.where(~np.isfinite(cand).all(axis=1), FLAG_NONFINITE, 0).astype(np.uint32)
    return f
