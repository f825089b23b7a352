"""Gate frames for scenario candidates and crafted states for frx_trajectory_gates - test infrastructure, not a test module.  A state is one
candidate: T (N,), C (N, 6, 3) (row k = power k), gates (G, 9) in the order they are to be flown, per gate what the row must hold in closed form
("nan": all ten NaN), and the flag bits that must be set / clear.  Every crafted input is a double written exactly (halves, quarters, sixteenths, the
parameters' own g and g / 2)."""
import numpy as np

MISSED, REPEAT, ORDER, NONFINITE = 1, 2, 4, 8


def frame_gates(centres, polyline, half_u, half_v):
    """Records (n, 9) for gate centres that are interior vertices 1 .. n of `polyline`: the normal along the bisector of the two legs that meet at the centre,
    ev the vertical made orthogonal to it, eu = ev x n (so that a x b points along the normal), half extents half_u and half_v"""
    out = []
    for k, c in enumerate(np.asarray(centres, dtype=np.float64)):
        d0, d1 = polyline[k + 1] - polyline[k], polyline[k + 2] - polyline[k + 1]
        n = d0 / np.linalg.norm(d0) + d1 / np.linalg.norm(d1)
        n /= np.linalg.norm(n)
        ev = np.array([0.0, 0.0, 1.0]) - n[2] * n
        ev /= np.linalg.norm(ev)
        eu = np.cross(ev, n)
        out.append(np.concatenate([c, half_u * eu, half_v * ev]))
    return np.array(out)


def candidate_gates(cand, half_u=1.0, half_v=0.75):
    """the gates of a scenario.Candidate (start -> gates -> goal is the polyline its corridor follows)"""
    poly = np.vstack([cand.ini_state[:, 0], cand.gates, cand.fin_state[:, 0]])
    return frame_gates(cand.gates, poly, half_u, half_v)


def _gate(c, wu, wv):
    """axis-aligned: eu = +x, ev = -z, so n = +y"""
    return np.array([c[0], c[1], c[2], wu, 0.0, 0.0, 0.0, 0.0, -wv])


def _cand(T, *pieces):
    C = np.zeros((len(pieces), 6, 3))
    for i, rows in enumerate(pieces):
        for k, v in rows.items():
            C[i, int(k[1:])] = v
    return np.array(T, dtype=np.float64), C


def crafted(params, long_n=130):
    """long_n: pieces of state (k) (a handle holds candidates of up to 128 pieces: the device tests pass 128)"""
    g, e0, e2 = params["grav_acc"], params["horiz_half_len"], params["vert_half_len"]
    out = {}

    def add(name, TC, gates, expect, set=0, clear=0):
        out[name] = dict(T=TC[0], C=TC[1], gates=np.array(gates, dtype=np.float64).reshape(-1, 9), expect=expect, set=set, clear=clear)

    line = dict(c0=(0.0, 0.0, 1.0), c1=(0.0, 2.0, 0.0))                  # y = 2 t at hover attitude: xB = x, yB = y, zB = z
    # (a) through the centre: the reach is the semi-axis itself (sqrt(x x) == x in binary arithmetic)
    add("a_centre", _cand([2.0], line), [_gate((0.0, 2.0, 1.0), 1.0, 0.5)],
        [dict(n_cross=1, n_pass=1, margin=(min(1.0 - e0, 0.5 - e2), 0.0), time=(1.0, 0.0), piece=0, u=(0.0, 0.0), v=(0.0, 0.0), reach_u=(e0, 0.0), reach_v=(e2, 0.0),
              normal_speed=(2.0, 0.0))], clear=MISSED | REPEAT | ORDER | NONFINITE)
    # (b) offset in u
    add("b_offset", _cand([2.0], dict(c0=(0.25, 0.0, 1.0), c1=(0.0, 2.0, 0.0))), [_gate((0.0, 2.0, 1.0), 1.0, 0.5)],
        [dict(n_cross=1, n_pass=1, margin=(min(1.0 - 0.25 - e0, 0.5 - e2), 0.0), u=(0.25, 0.0), time=(1.0, 0.0))], clear=MISSED | REPEAT | ORDER | NONFINITE)
    # (c) y = 4 t - t^2 meets the plane y = 3 at t = 1 and t = 3, outside the opening both times (x = 2.5, then 1.5): the nearer miss is the later one
    arc = dict(c1=(0.0, 4.0, 0.0), c2=(0.0, -1.0, 0.0))
    add("c_outside", _cand([4.0], dict(c0=(3.0, 0.0, 1.0), c1=(-0.5, 4.0, 0.0), c2=(0.0, -1.0, 0.0))), [_gate((0.0, 3.0, 1.0), 1.0, 0.5)],
        [dict(n_cross=2, n_pass=0, margin=1.0 - 1.5 - e0, u=1.5, time=3.0, piece=0, normal_speed=-2.0)], set=MISSED, clear=REPEAT | ORDER | NONFINITE)
    # (d) out and back through the opening (x = 0.25, then 0: the later passage has the larger margin); the earlier one is reported
    add("d_out_and_back", _cand([4.0], dict(c0=(0.375, 0.0, 1.0), c1=(-0.125, 4.0, 0.0), c2=(0.0, -1.0, 0.0))), [_gate((0.0, 3.0, 1.0), 1.0, 0.5)],
        [dict(n_cross=2, n_pass=2, margin=1.0 - 0.25 - e0, u=0.25, time=1.0, piece=0, normal_speed=2.0)], set=REPEAT, clear=MISSED | ORDER | NONFINITE)
    # (e) a knot exactly on the plane: tau = 1 of piece 0 and tau = 0 of piece 1 are both exact roots; it counts once, for piece 0
    add("e_knot_on_plane", _cand([1.0, 1.0], line, dict(c0=(0.0, 2.0, 1.0), c1=(0.0, 2.0, 0.0))), [_gate((0.0, 2.0, 1.0), 1.0, 0.5)],
        [dict(n_cross=1, n_pass=1, piece=0, time=(1.0, 0.0), normal_speed=(2.0, 0.0))], clear=MISSED | REPEAT | ORDER | NONFINITE)
    # (f) an exact touch: y = 4 t - t^2 reaches 4 at t = 2 and turns; f = -4 (2 tau - 1)^2 is exactly 0 at its critical point
    add("f_touch", _cand([4.0], dict(c0=(0.0, 0.0, 1.0), **arc)), [_gate((0.0, 4.0, 1.0), 1.0, 0.5)],
        [dict(n_cross=1, n_pass=1, time=(2.0, 0.0), normal_speed=(0.0, 0.0), u=(0.0, 0.0))], clear=MISSED | REPEAT | ORDER | NONFINITE)
    # (g) constant lateral acceleration (g, 0, 0): h = (g, 0, g), the body is rolled 45 degrees about y and reaches sqrt((e0^2 + e2^2) / 2) along x
    tilt = dict(c0=(0.0, 0.0, 1.0), c1=(0.0, 2.0, 0.0), c2=(g / 2.0, 0.0, 0.0))
    ru = float(np.sqrt((e0 * e0 + e2 * e2) / 2.0))
    add("g_tilt", _cand([2.0], tilt), [_gate((g / 2.0, 2.0, 1.0), 1.0, 0.5)],
        [dict(n_cross=1, n_pass=1, reach_u=(ru, 1e-15), reach_v=(ru, 1e-15), u=(0.0, 0.0), margin=0.5 - ru, time=(1.0, 0.0))], clear=MISSED | REPEAT | ORDER | NONFINITE)
    # ... and a gate narrower than the body is wide (2 x 7/16 < 2 e0) that passes only because of the tilt
    assert 0.4375 < e0 and 0.4375 - ru > 0.0
    add("g_narrow", _cand([2.0], tilt), [_gate((g / 2.0, 2.0, 1.0), 0.4375, 0.5)],
        [dict(n_cross=1, n_pass=1, margin=0.4375 - ru, reach_u=(ru, 1e-15))], clear=MISSED | REPEAT | ORDER | NONFINITE)
    # (h) two gates flown in the wrong order; and two gates passed at the same instant (strictly increasing is asked for)
    far, near = _gate((0.0, 6.0, 1.0), 1.0, 0.5), _gate((0.0, 2.0, 1.0), 1.0, 0.5)
    add("h_wrong_order", _cand([4.0], line), [far, near], [dict(n_pass=1, time=(3.0, 0.0)), dict(n_pass=1, time=(1.0, 0.0))], set=ORDER, clear=MISSED | REPEAT | NONFINITE)
    add("h_same_instant", _cand([4.0], line), [near, near], [dict(n_pass=1, time=(1.0, 0.0)), dict(n_pass=1, time=(1.0, 0.0))], set=ORDER, clear=MISSED | REPEAT | NONFINITE)
    add("h_right_order", _cand([4.0], line), [near, far], [dict(n_pass=1, time=(1.0, 0.0)), dict(n_pass=1, time=(3.0, 0.0))], clear=ORDER | MISSED | REPEAT | NONFINITE)
    # (i) what makes a row all NaN: a NaN coefficient, T = 0 (in a piece the crossing is not in), a NaN gate, a gate of zero extent
    two = (line, dict(c0=(0.0, 2.0, 1.0), c1=(0.0, 2.0, 0.0)))
    T, C = _cand([1.0, 1.0], *two)
    C[1, 4, 1] = np.nan
    add("i_nan_coefficient", (T, C), [_gate((0.0, 1.0, 1.0), 1.0, 0.5)], ["nan"], set=NONFINITE, clear=MISSED | REPEAT | ORDER)
    add("i_zero_duration", _cand([1.0, 0.0], *two), [_gate((0.0, 1.0, 1.0), 1.0, 0.5)], ["nan"], set=NONFINITE, clear=MISSED | REPEAT | ORDER)
    bad = _gate((0.0, 1.0, 1.0), 1.0, 0.5)
    bad[1] = np.nan
    add("i_nan_gate", _cand([1.0, 1.0], *two), [bad, _gate((0.0, 3.0, 1.0), 1.0, 0.5)], ["nan", dict(n_cross=1, n_pass=1, time=(1.5, 0.0), piece=1)],
        set=NONFINITE, clear=MISSED | REPEAT | ORDER)
    add("i_zero_extent", _cand([1.0, 1.0], *two), [_gate((0.0, 1.0, 1.0), 1.0, 0.5), _gate((0.0, 3.0, 1.0), 0.0, 0.5)],
        [dict(n_cross=1, n_pass=1, time=(0.5, 0.0), piece=0), "nan"], set=NONFINITE, clear=MISSED | REPEAT | ORDER)
    # (k) long_n pieces of y = k / 2 + t, T = 1 / 2 each; the only crossing is in the last piece (130: the third stride of the kernel's walk)
    last = long_n - 1
    add("k_last_of_%d" % long_n, _cand([0.5] * long_n, *[dict(c0=(0.0, 0.5 * k, 1.0), c1=(0.0, 1.0, 0.0)) for k in range(long_n)]),
        [_gate((0.0, 0.5 * last + 0.25, 1.0), 1.0, 0.5)],
        [dict(n_cross=1, n_pass=1, piece=last, time=(0.5 * last + 0.25, 0.0), normal_speed=(1.0, 0.0), margin=(min(1.0 - e0, 0.5 - e2), 0.0))],
        clear=MISSED | REPEAT | ORDER | NONFINITE)
    return out


def random_gates(rng, T, c6, n, inner=0.0):
    """n gates for one piece, each through a random point of the piece (so that it is crossed; inner > 0 keeps the point that share of T away from the piece's
    ends) with a random frame and half extents in [0.3, 2]"""
    c6 = np.asarray(c6, dtype=np.float64).reshape(6, 3)
    out = []
    for _ in range(n):
        t = rng.uniform(inner * T, (1.0 - inner) * T)
        p = sum(c6[k] * t ** k for k in range(6))
        Q, _ = np.linalg.qr(rng.normal(0.0, 1.0, (3, 3)))
        wu, wv = rng.uniform(0.3, 2.0, 2)
        c = p + Q[:, 0] * rng.uniform(-1.0, 1.0) * wu + Q[:, 1] * rng.uniform(-1.0, 1.0) * wv
        out.append(np.concatenate([c, wu * Q[:, 0], wv * Q[:, 1]]))
    return np.array(out)
