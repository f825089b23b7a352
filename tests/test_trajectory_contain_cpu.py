"""frx_trajectory_contain without a device: the symbols and argument errors of the three entries, the host-only fold (frx_contain_fold) against the restatement,
and the restatement (tests/contain_reference.py) against closed forms, planted errors and an independent long-double sampler.  The device kernel is held to
the restatement bit for bit in tests/test_gpu_trajectory_contain.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contain_reference as cn  # noqa: E402
import contain_states as cs  # noqa: E402
import extrema_states as es  # noqa: E402

INVALID_ARG, NO_DEVICE = -1, -2
FACE_SEED = 5                                                            # seed of the random faces of the sampler comparison
CONTACT_BOUND = 1e-11                                                    # |sd| <= CONTACT_BOUND S at a contact, S = sum_k |d_k|


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and not ((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))).any()


def test_symbols_and_argument_errors_come_before_the_device(frx):
    L = frx.lib()
    for name in ("frx_trajectory_contain", "frx_trajectory_contain_device", "frx_contain_fold"):
        assert name in frx.ABI_SYMBOLS and hasattr(L, name)
    assert frx.CONTAIN_FIELDS == cn.FIELDS and len(frx.CONTAIN_FIELDS) == 8
    h = 8                                                                # never read: these checks come first
    for k in (0, 1, 2, 5):                                               # handle, T, C, cand_out; piece_out and flags may be NULL
        args = [h, 8, 8, 0.0, 8, 8, 8]
        args[k] = None
        assert L.frx_trajectory_contain(*args) == INVALID_ARG, k
    for k in (0, 1, 2, 4):
        args = [h, 8, 8, 0.0, 8, None]
        args[k] = None
        assert L.frx_trajectory_contain_device(*args) == INVALID_ARG, k
    for bad in (np.nan, np.inf, -np.inf):
        assert L.frx_trajectory_contain(h, 8, 8, bad, 8, 8, 8) == INVALID_ARG
        assert L.frx_trajectory_contain_device(h, 8, 8, bad, 8, None) == INVALID_ARG
    if L.frx_device_count() < 1:
        assert L.frx_trajectory_contain(h, 8, 8, 0.0, None, 8, None) == NO_DEVICE
        assert L.frx_trajectory_contain_device(h, 8, 8, 0.0, 8, None) == NO_DEVICE
    buf = np.zeros(64)
    off = np.array([0, 1], np.int32)
    d, o = buf.ctypes.data, off.ctypes.data
    assert L.frx_contain_fold(0, o, d, d, d, d) == INVALID_ARG
    assert L.frx_contain_fold(1, None, d, d, d, d) == INVALID_ARG
    assert L.frx_contain_fold(1, o, None, d, d, d) == INVALID_ARG
    assert L.frx_contain_fold(1, o, d, None, d, d) == INVALID_ARG
    assert L.frx_contain_fold(2, np.array([0, 2, 1], np.int32).ctypes.data, d, d, d, d) == INVALID_ARG
    assert L.frx_contain_fold(1, np.array([-1, 1], np.int32).ctypes.data, d, d, d, d) == INVALID_ARG
    assert L.frx_contain_fold(1, o, d, d, None, None) == 0               # nothing asked for: nothing done


def test_debug_fold_rows_keeps_its_three_kinds(frx):
    """the containment fold has its own entry: kind 3 of frx_debug_fold_rows stays an error"""
    buf = np.zeros(64)
    off = np.array([0, 1], np.int32)
    assert frx.lib().frx_debug_fold_rows(3, 1, off.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None) == INVALID_ARG


def _row(n, outside, ex=None, centre=(-0.5, 0.25, 3.0), nan=False):
    r = np.array([n, outside] + (list(ex) if ex else [-1.0, -1.0, -1.0]) + list(centre))
    if nan:
        r[:] = np.nan
    return r


def test_contain_fold_against_the_restatement(frx):
    """made-up piece rows: ties of OUTSIDE and CENTRE keep the first piece, a NaN row takes every field and stays, the exit group comes from the first piece
    that has one, candidates without pieces keep their rows, either output may be NULL"""
    cands = [
        [_row(2, 0.5, (0.25, 0.75, 4.0)), _row(0, 0.0), _row(2, 0.5, (0.1, 0.6, 2.0), centre=(-0.5, 0.5, 1.0))],      # ties: first piece's OUTSIDE and CENTRE
        [_row(0, 0.0), _row(0, 0.0, centre=(-0.25, 0.5, 2.0))],                                                       # inside: no flag
        [],
        [_row(0, 0.0), _row(1, 0.25, (0.5, 1.0, 7.0)), _row(1, 0.75, (0.0, 0.75, 1.0), centre=(0.5, 0.0, 0.0))],      # the exit of the second piece, not the third
        [_row(1, 0.5, (0.0, 0.5, 0.0)), _row(0, 0.0, nan=True), _row(3, 2.0, (0.1, 0.2, 1.0), centre=(9.0, 0.0, 0.0))],   # NaN takes and stays; the exit stays the first
        [_row(0, 0.0, nan=True), _row(1, 0.5, (0.0, 0.5, 0.0))],                                                      # NaN first: the exit group is NaN too
        [],
    ]
    rows = np.array([r for c in cands for r in c])
    off = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int32)
    T = np.linspace(0.5, 1.75, len(rows))
    want = cn.reduce_candidates(rows, T, off)
    wf = cn.flags_of(want, off)
    assert wf.tolist() == [1, 0, 0, 1, 1 | 32, 32, 0]
    assert want[0, cn.T_EXIT] == 0.25 and want[0, cn.K_EXIT] == 0 and want[0, cn.T_CENTRE] == 0.25 and want[0, cn.K_CENTRE] == 0 and want[0, cn.N_CONTACT] == 4
    assert want[3, cn.K_EXIT] == 1 and want[3, cn.T_EXIT] == T[off[3]] + 0.5 and want[3, cn.OUTSIDE] == 0.75 and want[3, cn.K_CENTRE] == 2
    assert want[4, cn.T_EXIT] == 0.0 and np.isnan(want[4, [cn.N_CONTACT, cn.OUTSIDE, cn.CENTRE]]).all() and want[4, cn.K_CENTRE] == 1
    assert np.isnan(want[5, cn.T_EXIT]) and want[5, cn.K_EXIT] == 0
    cand, flags = frx.contain_fold(rows, T, off)
    assert same(cand, want) and np.array_equal(flags, wf), (cand, want, flags, wf)
    L = frx.lib()
    c2 = np.full((len(cands), 8), -3.0); f2 = np.full(len(cands), 77, np.uint32)
    assert L.frx_contain_fold(len(cands), off.ctypes.data, T.ctypes.data, rows.ctypes.data, c2.ctypes.data, None) == 0
    assert same(c2[[0, 1, 3, 4, 5]], want[[0, 1, 3, 4, 5]]) and (c2[[2, 6]] == -3.0).all()          # a candidate without pieces leaves its row as it is
    assert L.frx_contain_fold(len(cands), off.ctypes.data, T.ctypes.data, rows.ctypes.data, None, f2.ctypes.data) == 0
    assert np.array_equal(f2, wf)


def crafted_failures(st, params, variant=None):
    """what a (possibly planted) restatement gets wrong on one crafted state"""
    N = len(st["T"])
    rows = cn.rows(st["T"], st["C"], [0, N], st["polys"], params, st["slack"], variant)
    bad = []
    for i, (r, e) in enumerate(zip(rows, st["expect"])):
        if isinstance(e, str):
            bad += [] if np.isnan(r).all() else [(i, "nan", r.tolist())]
        else:
            bad += [(i,) + b for b in cn.expectation_failures(r, e)]
    cand = cn.reduce_candidates(rows, st["T"], [0, N])
    if st["cand"] is not None:
        bad += [("cand",) + b for b in cn.expectation_failures(cand[0], st["cand"])]
    fl = int(cn.flags_of(cand)[0])
    if fl & st["set"] != st["set"] or fl & st["clear"]:
        bad.append(("flags", fl, st["set"], st["clear"]))
    return bad, rows, cand


def test_crafted_states_against_their_closed_forms(frx, sc):
    for name, st in cs.crafted(sc.ZHANGJIAJIE).items():
        bad, rows, cand = crafted_failures(st, sc.ZHANGJIAJIE)
        print(name, rows.tolist(), bad)
        assert not bad, (name, bad)
        c2, f2 = frx.contain_fold(rows, st["T"], [0, len(rows)])
        assert same(c2, cand) and np.array_equal(f2, cn.flags_of(cand)), name


def test_slack_is_the_face_moved(sc):
    """a face pulled in by slack against the face moved by as much: the same contacts, to rounding"""
    st = cs.crafted(sc.ZHANGJIAJIE)
    a = crafted_failures(st["j_slack"], sc.ZHANGJIAJIE)[1]
    b = crafted_failures(st["j_face_moved"], sc.ZHANGJIAJIE)[1]
    assert np.abs(a - b).max() <= 1e-12 and a[0, cn.N_CONTACT] == b[0, cn.N_CONTACT] == 1


@pytest.mark.parametrize("variant", ["keep_far", "no_skip", "left_end", "keep_tau0"])
def test_planted_errors_fail_on_the_crafted_states(sc, variant):
    """keep_far fails on (a) ... (the far side's contact is counted too), no_skip on g2 (sd is not a number in free fall: without the skip the far faces
    count as left), left_end on (a) ... (sd at a contact is zero to rounding, at the piece's start it is the start's), keep_tau0 on (i) (the knot is
    counted twice)."""
    failing = [name for name, st in cs.crafted(sc.ZHANGJIAJIE).items() if crafted_failures(st, sc.ZHANGJIAJIE, variant)[0]]
    print(variant, failing)
    assert failing, f"planted error {variant!r} passes on every crafted state"


def _compare(pairs, params):
    """pairs of (T, c (6, 3), normal, point): the restatement's contacts and intervals of the face against the sampler.  Returns (pairs, left out, contacts,
    worst |sd| / S at a contact)"""
    eh, ev, g, margin = params["horiz_half_len"], params["vert_half_len"], params["grav_acc"], params["safe_margin"]
    ell = (eh, eh, ev)
    left_out = contacts = 0
    worst = 0.0
    for i, (T, c, normal, point) in enumerate(pairs):
        hp = np.concatenate([normal, point])[:, None]
        org, recs = cn.face_records(hp, margin)
        w, wh, Q = cn.normalised(T, c, g)
        r = cn.face_result(w, wh, Q, T, org, recs[0][0], recs[0][1], True, eh, ev, margin, 0.0)
        s = cn.sample_pair(c, T, normal, point, ell, g)
        if s["doubtful"]:
            left_out += 1
            continue
        assert len(r["contacts"]) == s["changes"], (i, r, s)
        contacts += len(r["contacts"])
        S = cn.scale(c, T, normal, point)
        if r["contacts"]:
            sd, d = cn.sample_sd(c, [np.longdouble(tau) * np.longdouble(T) for tau in r["contacts"]], normal, point, ell, g)
            worst = max(worst, float(np.abs(sd).max()) / S)
            assert (np.abs(sd) <= CONTACT_BOUND * S).all() and (d < 0).all(), (i, sd, S)
        if r["intervals"]:
            mids = [0.5 * (np.longdouble(a) + np.longdouble(b)) * np.longdouble(T) for a, b, _ in r["intervals"]]
            sd, _ = cn.sample_sd(c, mids, normal, point, ell, g)
            for (a, b, outside), v in zip(r["intervals"], sd):
                assert (v > 0) == outside, (i, a, b, outside, float(v))
        else:                                                            # a skipped face: the sampler never sees the body past it
            assert r["skipped"] and s["changes"] == 0
    return len(pairs), left_out, contacts, worst


def test_restatement_against_the_long_double_sampler_on_random_quintics(sc):
    """300 random quintics with three random faces through the path each (unit normal, face point = p(t*) + n U(-0.7, 0.7)): 900 pairs.  N_CONTACT of the
    face equals the sampler's count of sign changes of sd over 20 001 long-double samples in physical time; every interval's midpoint has the sign the
    restatement gave it (sd > 0 exactly where it says outside); at each contact the long-double |sd| <= 1e-11 S, S = sum_k |d_k|, and d < 0.  A pair is left
    out only where the sampler itself sees a near-tangency (a local extremum of |sd| below 1e-6) or a sign change within two steps of an end; at most 2 %
    may be.  Observed with FACE_SEED = 5: see the printed line (contacts, left out, worst |sd| / S)."""
    params = sc.ZHANGJIAJIE
    rng = np.random.default_rng(FACE_SEED)
    pairs = []
    for T, c in es.random_quintics(np.random.default_rng(11), 300):
        for _ in range(3):
            n = rng.normal(0.0, 1.0, 3)
            n /= np.linalg.norm(n)
            ts = rng.uniform(0.0, T)
            p = np.array([ts ** k for k in range(6)]) @ c + n * rng.uniform(-0.7, 0.7)
            pairs.append((T, c, n, p))
    n, left_out, contacts, worst = _compare(pairs, params)
    print("pairs", n, "left out", left_out, "contacts", contacts, "worst |sd| / S", worst)
    assert n == 900 and left_out <= 0.02 * n and contacts > 300


def test_restatement_against_the_long_double_sampler_on_optimised_candidates(sc, ob):
    """oracle-optimised 12-piece candidates (scenarios 2, 6 and 11 after 80 iterations, scenario 6 after 5 as well) against the faces of their own
    corridors: every (piece, face) pair by the same comparison"""
    params = sc.ZHANGJIAJIE
    pairs = []
    for sid, iters in ((2, 80), (6, 80), (11, 80), (6, 5)):
        cand = sc.make_candidate(sid, 12, 3)
        r = ob.Oracle(cand, params, qd_intervals=8).optimize(1e-6, max_iterations=iters)
        T, Cp = np.asarray(r["T"]), np.asarray(r["C"]).reshape(-1, 6, 3)
        for i, hp in enumerate(cand.h_polys):
            for k in range(hp.shape[1]):
                pairs.append((float(T[i]), Cp[i], hp[:3, k] / np.linalg.norm(hp[:3, k]), hp[3:, k]))
    n, left_out, contacts, worst = _compare(pairs, params)
    print("pairs", n, "left out", left_out, "contacts", contacts, "worst |sd| / S", worst)
    assert n >= 300 and left_out <= 0.02 * n
