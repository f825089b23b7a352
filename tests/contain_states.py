"""Crafted candidates for frx_trajectory_contain - test infrastructure, not a test module.  Every state is one candidate: durations T (N,),
coefficients C (N, 6, 3) (row k = power k), the 6 x K polytope of every piece (columns: outer normal, point), the slack it is judged with, what it is there
for and, where the numbers are known in closed form, the expected fields of every piece row and of the candidate row.

The states are written for the body eh = 0.5, ev = 0.15 under g = 9.81 (scenario.ZHANGJIAJIE); `crafted` asserts that."""
import math

import numpy as np

CORRIDOR, NONFINITE = 1, 32


def face(n, p):
    return np.concatenate([np.asarray(n, dtype=np.float64), np.asarray(p, dtype=np.float64)])


# faces |x|, |y|, |z| <= 50: every state's polytope is bounded, and the body never comes near these six
FAR_BOX = [face((1, 0, 0), (50, 0, 0)), face((0, 1, 0), (0, 50, 0)), face((0, 0, 1), (0, 0, 50)),
           face((-1, 0, 0), (-50, 0, 0)), face((0, -1, 0), (0, -50, 0)), face((0, 0, -1), (0, 0, -50))]


def poly(*faces, first=False):
    """FAR_BOX plus the given faces, behind it (indices 6..) or in front of it (first: the given face's point becomes the block's origin)"""
    cols = (list(faces) + FAR_BOX) if first else (FAR_BOX + list(faces))
    return np.array(cols).T.copy()


def _piece(T, **rows):
    c = np.zeros((6, 3))
    for k, v in rows.items():
        c[int(k[1:])] = v
    return float(T), c


def _state(pieces, polys, expect, cand, slack=0.0, set=0, clear=0):
    return dict(T=np.array([p[0] for p in pieces]), C=np.array([p[1] for p in pieces]), polys=list(polys), slack=slack, expect=list(expect), cand=cand,
                set=set, clear=clear)


def ring_faces(n, centre, radius):
    """n vertical faces tangent to a cylinder round `centre`"""
    out = []
    for i in range(n):
        phi = 2.0 * math.pi * (i + 0.5) / n
        d = np.array([math.cos(phi), math.sin(phi), 0.0])
        out.append(face(d, np.asarray(centre, dtype=np.float64) + radius * d))
    return out


def crafted(params):
    """dict name -> state"""
    eh, ev, g = params["horiz_half_len"], params["vert_half_len"], params["grav_acc"]
    assert (eh, ev, g) == (0.5, 0.15, 9.81)
    out = {}
    level = _piece(2.0, c0=(0.0, 0.0, 1.0), c1=(1.0, 0.0, 0.0))           # level flight along x at 1 m/s: h = g e3, zB = e3
    # (a) into n = (1, 0, 0) at x = 1.25: zB.n = 0, the reach is eh; sd = t - 1.25 + 0.5
    e = dict(n_contact=1, outside=1.25, t_exit=0.75, t_enter=2.0, k_exit=6, centre=0.75, t_centre=2.0, k_centre=6)
    out["a_level_into_x_face"] = _state([level], [poly(face((1, 0, 0), (1.25, 0, 0)))], [e], dict(e, k_exit=0, k_centre=0), set=CORRIDOR, clear=NONFINITE)
    # (b) a climb at 0.5 m/s into n = (0, 0, 1) at z = 1.6: the reach is ev; sd = 1 + t / 2 - 1.6 + 0.15
    climb = _piece(2.0, c0=(0.0, 0.0, 1.0), c1=(0.0, 0.0, 0.5))
    e = dict(n_contact=1, outside=1.1, t_exit=0.9, t_enter=2.0, k_exit=6, centre=0.4, t_centre=2.0, k_centre=6)
    out["b_climb_into_z_face"] = _state([climb], [poly(face((0, 0, 1), (0, 0, 1.6)))], [e], dict(e, k_exit=0, k_centre=0), set=CORRIDOR, clear=NONFINITE)
    # (c) level flight into a tilted normal (sin th, 0, cos th) through (1, 0, 1): the reach is sqrt(eh^2 + Delta cos^2 th); sd = sin th (t - 1) + reach
    th = 0.6
    r = math.sqrt(eh * eh + (ev * ev - eh * eh) * math.cos(th) ** 2)
    tc = 1.0 - r / math.sin(th)
    e = dict(n_contact=1, outside=2.0 - tc, t_exit=tc, t_enter=2.0, k_exit=6, centre=math.sin(th), t_centre=2.0, k_centre=6)
    out["c_tilted_normal"] = _state([level], [poly(face((math.sin(th), 0, math.cos(th)), (1.0, 0, 1.0)))], [e], dict(e, k_exit=0, k_centre=0), set=CORRIDOR,
                                    clear=NONFINITE)
    # (d) constant lateral acceleration (g, 0, 0): zB = (1, 0, 1) / sqrt 2, the reach against n = (1, 0, 0) is sqrt((eh^2 + ev^2) / 2); contact at t = 0.6
    r = math.sqrt((eh * eh + ev * ev) / 2.0)
    X = r + 0.5 * g * 0.36
    e = dict(n_contact=1, outside=0.4, t_exit=0.6, t_enter=1.0, k_exit=6, centre=0.5 * g - X, t_centre=1.0, k_centre=6)
    out["d_lateral_acceleration"] = _state([_piece(1.0, c0=(0.0, 0.0, 1.0), c2=(0.5 * g, 0.0, 0.0))], [poly(face((1, 0, 0), (X, 0, 0)))], [e],
                                           dict(e, k_exit=0, k_centre=0), set=CORRIDOR, clear=NONFINITE)
    # (e) out and back: z = 1 + t (2 - t) against z <= 1.9 (a_z = -2: zB = e3, the reach is ev); past the face for 0.5 < t < 1.5
    hop = _piece(2.0, c0=(0.0, 0.0, 1.0), c1=(0.0, 0.0, 2.0), c2=(0.0, 0.0, -1.0))
    e = dict(n_contact=2, outside=1.0, t_exit=0.5, t_enter=1.5, k_exit=6, centre=0.1, t_centre=1.0, k_centre=6)
    out["e_out_and_back"] = _state([hop], [poly(face((0, 0, 1), (0, 0, 1.9)))], [e], dict(e, k_exit=0, k_centre=0), set=CORRIDOR, clear=NONFINITE)
    # (f) the body is outside at the start: x = -t against x <= 0.25, sd = 0.25 - t
    back = _piece(2.0, c0=(0.0, 0.0, 1.0), c1=(-1.0, 0.0, 0.0))
    e = dict(n_contact=1, outside=0.25, t_exit=0.0, t_enter=0.25, k_exit=6, centre=-0.25, t_centre=0.0, k_centre=6)
    out["f_outside_at_the_start"] = _state([back], [poly(face((1, 0, 0), (0.25, 0, 0)))], [e], dict(e, k_exit=0, k_centre=0), set=CORRIDOR, clear=NONFINITE)
    # (g) far faces only: every face is skipped; CENTRE is the nearest of them, x <= 50 at the piece's end
    e = dict(n_contact=0, outside=0.0, t_exit=-1.0, t_enter=-1.0, k_exit=-1, centre=-48.0, t_centre=2.0, k_centre=0)
    out["g_far_faces"] = _state([level], [poly()], [e], dict(e, k_centre=0), set=0, clear=CORRIDOR | NONFINITE)
    # (g2) far faces in free fall: h = 0, the attitude is undefined and sd is not a number - but no attitude reaches a face 48 m away: the skip rule certifies it
    # (nearest: z <= 50 at the start, where z = 1)
    e = dict(n_contact=0, outside=0.0, t_exit=-1.0, t_enter=-1.0, k_exit=-1, centre=-49.0, t_centre=0.0, k_centre=2)
    out["g2_far_faces_in_free_fall"] = _state([_piece(0.5, c0=(0.0, 0.0, 1.0), c1=(1.0, 0.0, 0.0), c2=(0.0, 0.0, -0.5 * g))], [poly()], [e],
                                              dict(e, k_centre=0), set=0, clear=CORRIDOR | NONFINITE)
    # (h) z = 1 + A t (1 - t) (t - 1/2)^2, A = 0.64, against z <= 1.155: two bulges of 0.01 between the nodes 0, 1/2, 1 of a check at M = 2, which reads
    # sd = -0.005 at all three.  With s = t - 1/2: A (s^2 / 4 - s^4) = 0.005, four contacts at s = -+s_hi, -+s_lo
    A = 0.64
    disc = math.sqrt(0.0625 - 4.0 * 0.005 / A)
    s_hi, s_lo = math.sqrt((0.25 + disc) / 2.0), math.sqrt((0.25 - disc) / 2.0)
    bulge = _piece(1.0, c0=(0.0, 0.0, 1.0), c1=(0.0, 0.0, 0.25 * A), c2=(0.0, 0.0, -1.25 * A), c3=(0.0, 0.0, 2.0 * A), c4=(0.0, 0.0, -A))
    e = dict(n_contact=4, outside=2.0 * (s_hi - s_lo), t_exit=0.5 - s_hi, t_enter=0.5 - s_lo, k_exit=6, centre=0.01 - 0.155, k_centre=6)
    out["h_between_the_nodes"] = _state([bulge], [poly(face((0, 0, 1), (0, 0, 1.155)))], [e], dict(e, k_exit=0, k_centre=0), set=CORRIDOR, clear=NONFINITE)
    # (i) a knot on a contact: d = -1 + tau / 2 on the first piece, -1 / 2 + tau / 2 on the second, the face first in its block so that its record is exact:
    # F is Q_0 (3/4 - tau + tau^2 / 4) with an exact root at tau = 1, then Q_0 (-tau / 2 + tau^2 / 4) with an exact root at tau = 0, which is dropped
    k0 = _piece(1.0, c0=(0.25, 0.0, 1.0), c1=(0.5, 0.0, 0.0))
    k1 = _piece(1.0, c0=(0.75, 0.0, 1.0), c1=(0.5, 0.0, 0.0))
    kp = poly(face((1, 0, 0), (1.25, 0, 0)), first=True)
    e0 = dict(n_contact=1, outside=0.0, t_exit=-1.0, t_enter=-1.0, k_exit=-1, centre=-0.5, t_centre=1.0, k_centre=0)
    e1 = dict(n_contact=0, outside=1.0, t_exit=0.0, t_enter=1.0, k_exit=0, centre=0.0, t_centre=1.0, k_centre=0)
    out["i_knot_on_a_contact"] = _state([k0, k1], [kp, kp], [e0, e1], dict(n_contact=1, outside=1.0, t_exit=1.0, t_enter=2.0, k_exit=1, centre=0.0,
                                                                            t_centre=2.0, k_centre=1), set=CORRIDOR, clear=NONFINITE)
    # (j) slack 0.125 is the face of (a) moved in by 0.125: contact at t = 0.625
    e = dict(n_contact=1, outside=1.375, t_exit=0.625, t_enter=2.0, k_exit=6, centre=0.875, t_centre=2.0, k_centre=6)
    out["j_slack"] = _state([level], [poly(face((1, 0, 0), (1.25, 0, 0)))], [e], dict(e, k_exit=0, k_centre=0), slack=0.125, set=CORRIDOR, clear=NONFINITE)
    out["j_face_moved"] = _state([level], [poly(face((1, 0, 0), (1.125, 0, 0)))], [e], dict(e, k_exit=0, k_centre=0), set=CORRIDOR, clear=NONFINITE)
    # (k) the causes of an all-NaN row between two good pieces: a NaN coefficient, T = inf, T = 0, T < 0; the candidate's row is poisoned, its flag set
    bad = []
    for T, poke in ((0.7, True), (np.inf, False), (0.0, False), (-0.5, False)):
        c = np.array(level[1], copy=True)
        if poke:
            c[4, 1] = np.nan
        bad.append((T, c))
    lp = poly(face((1, 0, 0), (1.25, 0, 0)))
    ea = out["a_level_into_x_face"]["expect"][0]
    out["k_nan_causes"] = _state([level] + bad + [level], [lp] * 6, [ea, "nan", "nan", "nan", "nan", ea], None, set=NONFINITE, clear=0)
    # (l) 70 faces: the far box, a ring of 63 faces 3 m from the path's start, and the face of (a) last, at k = 69 - beyond one stride of 64 lanes
    e = dict(n_contact=1, outside=1.25, t_exit=0.75, t_enter=2.0, k_exit=69, centre=0.75, t_centre=2.0, k_centre=69)
    big = poly(*(ring_faces(63, (0.0, 0.0, 1.0), 3.5) + [face((1, 0, 0), (1.25, 0, 0))]))
    assert big.shape == (6, 70)
    out["l_seventy_faces"] = _state([level], [big], [e], dict(e, k_exit=0, k_centre=0), set=CORRIDOR, clear=NONFINITE)
    return out
