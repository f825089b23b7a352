"""Crafted pieces for frx_trajectory_extrema - test infrastructure, not a test module.  Every state is one quintic piece
(T, c (6, 3), row k = power k) with what it is there for and, where the numbers are known in closed form, the expected (value, local time) of a field."""
import numpy as np

KAPPA = 16                                                               # quadrature intervals of the handle the states are judged on


def _piece(T, **rows):
    c = np.zeros((6, 3))
    for k, v in rows.items():
        c[int(k[1:])] = v
    return float(T), c


def crafted(params, kappa=KAPPA):
    """dict name -> dict(T, c, expect {field: (value, time)}, flag bits that must be set / clear in a candidate made of this piece alone)"""
    g, vmax, thr_min = params["grav_acc"], params["vel_max"], params["thr_acc_min"]
    out = {}
    # (a) constant velocity (3, -4, 0): frx_traj_max_rates reports 0 (the reference's early-out); the ends are candidates here
    T, c = _piece(2.0, c0=(0.0, 0.0, 1.0), c1=(3.0, -4.0, 0.0))
    out["a_constant_velocity"] = dict(T=T, c=c, expect=dict(speed=(5.0, 0.0), acc=(0.0, 0.0), thrust_min=(g, 0.0), thrust_max=(g, 0.0), body_rate=(0.0, 0.0)),
                                      set=0, clear=2 | 4 | 8 | 16 | 32)
    # (b) a cubic stored as a quintic: c4 = c5 = 0, leading zeros of every critical polynomial are stripped
    T, c = _piece(0.9, c0=(0.2, -0.1, 1.0), c1=(1.5, -0.7, 0.3), c2=(-2.0, 1.1, 0.4), c3=(0.3, 0.2, -1.5))
    out["b_cubic_as_quintic"] = dict(T=T, c=c, expect={}, set=0, clear=32)
    # (c) monotone speed v_x = 1 + t on [0, 2]: no interior root, the maximum is the end tau = 1
    T, c = _piece(2.0, c1=(1.0, 0.0, 0.0), c2=(0.5, 0.0, 0.0))
    out["c_monotone"] = dict(T=T, c=c, expect=dict(speed=(3.0, 2.0), acc=(1.0, 0.0)), set=0, clear=2 | 32)
    # (d) v = (1 - t^2, 0, 0), T = 1: d/dtau |wv|^2 = 4 tau (tau^2 - 1) has exact roots at BOTH ends (fa == 0, fb == 0, out.back())
    T, c = _piece(1.0, c1=(1.0, 0.0, 0.0), c3=(-1.0 / 3.0, 0.0, 0.0))
    out["d_roots_at_both_ends"] = dict(T=T, c=c, expect=dict(speed=(1.0, 0.0), acc=(2.0, 1.0)), set=0, clear=2 | 32)
    # (e) v_x = 1 + (t - 1/2)^3: a double root of the critical polynomial that is no extremum; the maximum 1.125 is at the end
    T, c = _piece(1.0, c1=(0.875, 0.0, 0.0), c2=(0.375, 0.0, 0.0), c3=(-0.5, 0.0, 0.0), c4=(0.25, 0.0, 0.0))
    out["e_double_root"] = dict(T=T, c=c, expect=dict(speed=(1.125, 1.0)), set=0, clear=2 | 32)
    # (f) v_x = 1 - ((t - 1/2)^2 - 1/16)^2: two equal interior maxima 1 at t = 1/4 and 3/4
    T, c = _piece(1.0, c1=(247.0 / 256.0, 0.0, 0.0), c2=(3.0 / 16.0, 0.0, 0.0), c3=(-11.0 / 24.0, 0.0, 0.0), c4=(0.5, 0.0, 0.0), c5=(-0.2, 0.0, 0.0))
    out["f_two_equal_maxima"] = dict(T=T, c=c, expect=dict(speed=(1.0, None)), set=0, clear=2 | 32)
    # (g) between the nodes: v_x = vmax + 0.01 - q (t - T / (2 kappa))^2, the nodes 0 and T / kappa both read vmax - 0.01
    T = 1.0
    ts = T / (2 * kappa)
    q = 0.02 / ts ** 2
    T, c = _piece(T, c1=(vmax + 0.01 - q * ts ** 2, 0.0, 0.0), c2=(q * ts, 0.0, 0.0), c3=(-q / 3.0, 0.0, 0.0))
    out["g_speed_between_nodes"] = dict(T=T, c=c, expect=dict(speed=(vmax + 0.01, ts)), set=2, clear=32)
    # (h) the same for the thrust: a_x = a_y = 0, |h| = a_z + g = thr_min - 0.01 + q (t - ts)^2 dips below thr_min between the first two nodes
    a0 = thr_min - g - 0.01 + q * ts ** 2
    T, c = _piece(T, c1=(1.0, 0.0, 0.0), c2=(0.0, 0.0, a0 / 2.0), c3=(0.0, 0.0, -2.0 * q * ts / 6.0), c4=(0.0, 0.0, q / 12.0))
    out["h_thrust_between_nodes"] = dict(T=T, c=c, expect=dict(thrust_min=(thr_min - 0.01, ts)), set=4, clear=32)
    # (i) a = (0, 0, -g): h = 0 on the whole piece - thrust 0, the body rate 0 / 0
    T, c = _piece(0.8, c1=(1.0, 0.0, 0.0), c2=(0.0, 0.0, -g / 2.0))
    out["i_free_fall"] = dict(T=T, c=c, expect=dict(thrust_min=(0.0, 0.0), thrust_max=(0.0, 0.0), body_rate=(np.nan, 0.0)), set=4 | 32, clear=2 | 8)
    # (k) v_x = 1 - t^2 (1 - t)^2, T = 1: equal maxima 1 at BOTH ends, and both ends are exact roots of the critical polynomial (integer coefficients, found by
    # fa == 0 and fb == 0).  The candidates are (0, .., 1, 0, 1): the root at 0 stands first and wins the tie.  The only thing the fa == 0 branch can ever add is
    # that root at tau = 0; without it the root at 1 stands before the end 0 and the reported time moves to T
    T, c = _piece(1.0, c0=(0.0, 0.0, 1.0), c1=(1.0, 0.0, 0.0), c3=(-1.0 / 3.0, 0.0, 0.0), c4=(0.5, 0.0, 0.0), c5=(-0.2, 0.0, 0.0))
    out["k_equal_maxima_at_both_ends"] = dict(T=T, c=c, expect=dict(speed=(1.0, 0.0)), set=0, clear=2 | 32)
    return out


def bad_pieces(rng):
    """(j) four pieces whose rows are all NaN: a NaN coefficient, T = inf, T = 0, T < 0"""
    out = []
    for T, poke in ((0.7, True), (np.inf, False), (0.0, False), (-0.5, False)):
        c = rng.normal(0.0, 1.0, (6, 3))
        if poke:
            c[4, 1] = np.nan
        out.append((T, c))
    return out


def random_quintics(rng, n):
    """n random quintics with all six coefficient rows non-zero and T in [0.05, 3]"""
    return [(float(rng.uniform(0.05, 3.0)), rng.normal(0.0, 1.0, (6, 3))) for _ in range(n)]
