"""frx_trajectory_clearance_exact without a device: the symbols and argument errors, the host fold against the restatement, the restatement
(tests/clear_exact_reference.py) against closed forms on crafted states and against an independent long-double sampler, and the cull: rows with it on and
off are the same bits."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_exact_reference as cx  # noqa: E402
import clear_exact_states as xs  # noqa: E402
import extrema_states as es  # noqa: E402

INVALID_ARG, NO_DEVICE = -1, -2
# The restatement's minimum of q or r of a (piece, point) pair against the long-double sampler's, as a fraction of the SCALE of the pair: what rounding is
# relative to where u = o - p cancels.  scale_r = 3 (max_d (|o_d| + sum_k |w_k[d]|))^2 bounds every term of u.u, scale_q = scale_r / min(eh, ev)^2.
# "Never above": in exact arithmetic the minimum over the candidates cannot exceed a sample.  In double arithmetic the restatement's value carries the
# rounding of its own evaluation, so a literal "not above" fails by rounding alone; what is asserted is 8 x the worst excess seen, the rule of the other side.
# How far it may lie BELOW: both find the same minimum and the same rounding separates them (the sampler's golden section ends within a flat of the long
# double's precision and its result is rounded to a double).  Measured here on the 360 pairs of the two tests below, as fractions of the scale: above by at
# most 6.4e-17 on the random quintics and 6.6e-17 on the optimised candidate, below by at most 3.5e-17 and 6.1e-17; each asserted at 8 x the worst seen.
MEASURED_ABOVE, MEASURED_BELOW = 6.6e-17, 6.1e-17
ABOVE_BOUND, BELOW_BOUND = 8 * MEASURED_ABOVE, 8 * MEASURED_BELOW


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and not ((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))).any()


def test_symbols_and_argument_errors_come_before_the_device(frx):
    L = frx.lib()
    for name in ("frx_trajectory_clearance_exact", "frx_trajectory_clearance_exact_workspace", "frx_trajectory_clearance_exact_device", "frx_clearance_exact_fold"):
        assert name in frx.ABI_SYMBOLS and hasattr(L, name)
    for name in ("frx_debug_set_clear_exact", "frx_debug_clear_exact_counts"):
        assert name in frx.DEBUG_SYMBOLS and hasattr(L, name)
    assert frx.CLEAR_EXACT_FIELDS == cx.FIELDS == xs.FIELDS and len(frx.CLEAR_EXACT_FIELDS) == 6
    nb = C.c_size_t(77)
    h = 8                                                                # never read: these checks come first
    for k in (0, 1, 2, 4, 6):                                            # handle, T, C, obs, cand_out; piece_out and flags may be NULL
        args = [h, 8, 8, 5, 8, 8, 8, 8]
        args[k] = None
        assert L.frx_trajectory_clearance_exact(*args) == INVALID_ARG, k
    for k in (0, 1, 2, 4, 5, 6):                                         # handle, T, C, obs, work, rows
        args = [h, 8, 8, 5, 8, 8, 8, None]
        args[k] = None
        assert L.frx_trajectory_clearance_exact_device(*args) == INVALID_ARG, k
    for n in (0, -4, (1 << 24) + 1):
        assert L.frx_trajectory_clearance_exact(h, 8, 8, n, 8, 8, 8, 8) == INVALID_ARG
        assert L.frx_trajectory_clearance_exact_device(h, 8, 8, n, 8, 8, 8, None) == INVALID_ARG
        assert L.frx_trajectory_clearance_exact_workspace(h, n, C.byref(nb)) == INVALID_ARG
    assert L.frx_trajectory_clearance_exact_workspace(None, 5, C.byref(nb)) == INVALID_ARG
    assert L.frx_trajectory_clearance_exact_workspace(h, 5, None) == INVALID_ARG
    assert L.frx_debug_set_clear_exact(None, 0, 1) == INVALID_ARG and L.frx_debug_clear_exact_counts(None, 8, 8) == INVALID_ARG
    if L.frx_device_count() < 1:
        assert L.frx_trajectory_clearance_exact(h, 8, 8, 5, 8, None, 8, None) == NO_DEVICE
        assert L.frx_trajectory_clearance_exact_device(h, 8, 8, 5, 8, 8, 8, None) == NO_DEVICE
        assert L.frx_trajectory_clearance_exact_workspace(h, 5, C.byref(nb)) == NO_DEVICE
    assert nb.value == 77
    buf = np.zeros(64)
    off = np.array([0, 1], np.int32)
    d, o = buf.ctypes.data, off.ctypes.data
    assert L.frx_clearance_exact_fold(0, o, d, d, d, d) == INVALID_ARG
    assert L.frx_clearance_exact_fold(1, None, d, d, d, d) == INVALID_ARG
    assert L.frx_clearance_exact_fold(1, o, None, d, d, d) == INVALID_ARG
    assert L.frx_clearance_exact_fold(1, o, d, None, d, d) == INVALID_ARG
    assert L.frx_clearance_exact_fold(2, np.array([0, 2, 1], np.int32).ctypes.data, d, d, d, d) == INVALID_ARG
    assert L.frx_clearance_exact_fold(1, np.array([-1, 1], np.int32).ctypes.data, d, d, d, d) == INVALID_ARG
    assert L.frx_clearance_exact_fold(1, o, d, d, None, None) == 0       # nothing asked for: nothing done


def _row(ell, dist, t_ell=0.25, i_ell=3.0, t_dist=0.5, i_dist=4.0, nan=False):
    r = np.array([ell, dist, t_ell, i_ell, t_dist, i_dist])
    if nan:
        r[:] = np.nan
    return r


def test_fold_against_the_restatement(frx):
    """made-up piece rows: a tie between pieces keeps the earlier one (with ITS time and point), each of the two minima has its own piece, a NaN row takes
    both and stays, candidates without pieces keep their rows, either output may be NULL"""
    cands = [
        [_row(1.5, 0.7), _row(1.25, 0.9, 0.1, 7.0, 0.2, 8.0), _row(1.25, 0.7, 0.3, 1.0, 0.4, 2.0)],    # ELL: piece 1 before its tie in 2; DIST: piece 0 before 2
        [_row(0.5, 0.2)],                                                                              # a collision
        [],
        [_row(2.0, 1.0), _row(0.0, 0.0, nan=True), _row(0.1, 0.05)],                                   # NaN takes and stays
        [_row(np.nan, 0.4, 0.0, 2.0), _row(3.0, 0.3)],                                                 # free fall: ELL NaN, DIST goes on
        [],
    ]
    rows = np.array([r for c in cands for r in c])
    off = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int32)
    T = np.linspace(0.5, 1.75, len(rows))
    want = cx.reduce_candidates(rows, T, off)
    wf = cx.flags_of(want, off)
    assert wf.tolist() == [0, 1, 0, 2, 2, 0]
    assert tuple(want[0]) == (1.25, 0.7, T[0] + 0.1, 7.0, 0.0 + 0.5, 4.0)
    assert np.isnan(want[3, [0, 1]]).all() and np.isnan(want[3, 2]) and tuple(want[4, 1:]) == (0.3, 0.0, 2.0, T[off[4]] + 0.5, 4.0)
    cand, flags = frx.clearance_exact_fold(rows, T, off)
    assert same(cand, want) and np.array_equal(flags, wf), (cand, want, flags, wf)
    L = frx.lib()
    c2 = np.full((len(cands), 6), -3.0); f2 = np.full(len(cands), 77, np.uint32)
    assert L.frx_clearance_exact_fold(len(cands), off.ctypes.data, T.ctypes.data, rows.ctypes.data, c2.ctypes.data, None) == 0
    assert same(c2[[0, 1, 3, 4]], want[[0, 1, 3, 4]]) and (c2[[2, 5]] == -3.0).all()
    assert L.frx_clearance_exact_fold(len(cands), off.ctypes.data, T.ctypes.data, rows.ctypes.data, None, f2.ctypes.data) == 0
    assert np.array_equal(f2, wf)


def crafted_failures(st, cull=True):
    rows = cx.rows(st["T"], st["C"], st["obs"], st["params"], cull)
    bad = []
    for i, (r, e) in enumerate(zip(rows, st["expect"])):
        if isinstance(e, str):
            bad += [] if np.isnan(r).all() else [(i, "nan", r.tolist())]
        else:
            bad += [(i,) + b for b in xs.expectation_failures(r, e)]
    cand = cx.reduce_candidates(rows, st["T"], [0, len(rows)])
    if st["cand"] is not None:
        bad += [("cand",) + b for b in xs.expectation_failures(cand[0], st["cand"])]
    fl = int(cx.flags_of(cand)[0])
    if fl & st["set"] != st["set"] or fl & st["clear"]:
        bad.append(("flags", fl, st["set"], st["clear"]))
    return bad, rows, cand


def test_crafted_states_against_their_closed_forms(frx, sc):
    """a point beside the straight piece: DIST = |y0|, ELL = |y0| / eh at T / 3; above it: ELL = s; on the path: 0 and 0; a nearest point at a knot: both
    neighbours report it and the fold keeps the earlier; free fall: ELL NaN, DIST finite, NONFINITE; a sphere: ELL = DIST / eh - and with the cull off the
    same bits"""
    for name, st in xs.crafted(sc.ZHANGJIAJIE).items():
        bad, rows, cand = crafted_failures(st)
        print(name, rows.tolist(), bad)
        assert not bad, (name, bad)
        c2, f2 = frx.clearance_exact_fold(rows, st["T"], [0, len(rows)])
        assert same(c2, cand) and np.array_equal(f2, cx.flags_of(cand)), name
        assert same(crafted_failures(st, cull=False)[1], rows), name
    ff = crafted_failures(xs.crafted(sc.ZHANGJIAJIE)["e_free_fall"])[1][0]
    assert np.isnan(ff[cx.ELL]) and np.isfinite(ff[cx.DIST]) and ff[cx.DIST] > 0.0


def _compare(pairs, params):
    """pairs of (T, c (6, 3), o): the restatement's min q and min r of the point against the sampler's.  Returns (worst below, worst above) as fractions of
    the pair's scale"""
    eh, ev, g = params["horiz_half_len"], params["vert_half_len"], params["grav_acc"]
    below = above = 0.0
    for T, c, o in pairs:
        pc = cx.setup(T, c, g, eh, ev)
        _, Sp, m = cx.point_polys(pc, o)
        mr, _ = cx.dist_task(pc, o, Sp)
        mq, _ = cx.ell_task(pc, o, Sp, m)
        sq, sr = cx.sample_min(c, T, o, (eh, eh, ev), g)
        scale = 3.0 * max(abs(o[d]) + sum(abs(pc["w"][k][d]) for k in range(6)) for d in range(3)) ** 2
        for mine, theirs, sc_ in ((mq, sq, scale / min(eh, ev) ** 2), (mr, sr, scale)):
            assert theirs > 0.0 and mine > 0.0
            d = (theirs - mine) / sc_
            below, above = max(below, d), max(above, -d)
    return below, above


def _cull_on_and_off(groups, params):
    """groups of (T (n,), Cf (6n, 3), cloud): the rows with the cull on and off are the same bits"""
    for T, Cf, cloud in groups:
        on, off = cx.rows(T, Cf, cloud, params, True), cx.rows(T, Cf, cloud, params, False)
        assert same(on, off), (on, off)


def test_restatement_against_the_long_double_sampler_on_random_quintics(sc):
    """60 random quintics (tilted: |a| of the order of g) x 3 random points within 2 m of the path"""
    params = sc.ZHANGJIAJIE
    rng = np.random.default_rng(23)
    pairs = []
    for T, c in es.random_quintics(np.random.default_rng(11), 60):
        for _ in range(3):
            ts = rng.uniform(0.0, T)
            d = rng.normal(0.0, 1.0, 3)
            pairs.append((T, c, list(np.array([ts ** k for k in range(6)]) @ c + d / np.linalg.norm(d) * rng.uniform(0.1, 2.0))))
    below, above = _compare(pairs, params)
    print("pairs", len(pairs), "restatement below the sampler by at most", below, "above by at most", above)
    assert above <= ABOVE_BOUND and below <= BELOW_BOUND
    _cull_on_and_off([(np.array([pairs[i][0]]), pairs[i][1], np.array([p[2] for p in pairs[i:i + 3]])) for i in range(0, len(pairs), 3)], params)   # each piece against its own three points


def test_restatement_against_the_long_double_sampler_on_an_optimised_candidate(sc, ob):
    """an oracle-optimised 12-piece candidate (scenario 2 after 80 iterations) against a random cloud round its path: 15 points a piece"""
    params = sc.ZHANGJIAJIE
    cand = sc.make_candidate(2, 12, 3)
    r = ob.Oracle(cand, params, qd_intervals=8).optimize(1e-6, max_iterations=80)
    T, Cp = np.asarray(r["T"]), np.asarray(r["C"]).reshape(-1, 6, 3)
    cloud = xs.near_cloud(np.random.default_rng(31), T, Cp.reshape(-1, 3), 15)
    pairs = [(float(T[i]), Cp[i], list(o)) for i in range(len(T)) for o in cloud]
    below, above = _compare(pairs, params)
    print("pairs", len(pairs), "restatement below the sampler by at most", below, "above by at most", above)
    assert above <= ABOVE_BOUND and below <= BELOW_BOUND
    _cull_on_and_off([(T, Cp.reshape(-1, 3), cloud)], params)          # the candidate against its cloud


def test_the_cull_never_changes_a_row(sc):
    """random tilted quintics against a cloud near them, the same cloud pushed at least 1 km away, and the cloud with one point that is not finite: the rows
    with the cull on and off are the same bits, and the cull leaves work out"""
    params = xs.loose(sc.ZHANGJIAJIE)
    rng = np.random.default_rng(41)
    quint = es.random_quintics(np.random.default_rng(12), 4)
    T = np.array([q[0] for q in quint]); Cf = np.concatenate([q[1] for q in quint])
    near = xs.near_cloud(rng, T, Cf, 40)
    far = near + np.array([1000.0, 0.0, 300.0])
    for kind in ("nan", "inf"):
        bad = near.copy()
        bad[17, 1] = np.nan if kind == "nan" else np.inf
        for name, cloud in (("near", near), ("far", far), (kind, bad)):
            if kind == "inf" and name != "inf":
                continue
            cnt = []
            on = cx.rows(T, Cf, cloud, params, True, cnt)
            off = cx.rows(T, Cf, cloud, params, False)
            assert same(on, off), (name, on, off)
            ran = np.array(cnt)
            print(name, "survivors, DIST, ELL tasks per piece", ran.tolist())
            assert (ran[:, 0] >= 1).all() and (ran[:, 2] >= 1).all()
            if name in ("near", "far"):
                assert np.isfinite(on).all() and ran[:, 2].sum() < len(T) * len(cloud)
            else:
                assert np.isnan(on[:, cx.ELL]).all() and (on[:, cx.I_ELL] == 17).all()
            if name == "far":
                assert (on[:, cx.DIST] >= 1000.0).all()
