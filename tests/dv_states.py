"""States and command sequences for k_lbfgs_pre / k_lbfgs_post (driven through frx.dv_round, held by dv_reference.compare): synthetic ragged batches under
the library's own geometry, and real (x_k, g_k) sequences harvested from the CPU oracle.  The same driver runs the device (GPU tests) or the long-double
model itself (CPU tests: the sequences, the driver and the comparator are exercised without a device)."""
import ctypes as C
import functools

import numpy as np

import dv_reference as ref
from dv_reference import DV_ADVANCE, DV_EVAL, DV_INIT, DV_RESTORE, DV_TRIAL

# vector lengths of a batch, and the ((E, W, PF, BLK), hs) the library takes for its longest vector
BATCHES = {
    "one_wave": ([128, 1, 2, 3, 127, 65], ((2, 1, 16, 4), 128)),           # E = 2, one wave, full rows; a half-filled last thread; a one-element vector
    "headline": ([641, 640, 7, 513, 1, 322], ((6, 2, 8, 4), 656)),         # tight row of 656 on a 768 shape
    "one_slab": ([513, 512, 9, 1], ((2, 5, 16, 4), 528)),                  # one slab of pairs, half its threads clamped, tight 528 on 640
    "tight_4x5": ([1153, 1152, 3, 641], ((4, 5, 8, 4), 1168)),             # a 4 x 5 shape with tight rows
    "full_e8": ([2048, 1025, 5], ((8, 4, 4, 4), 2048)),                    # E = 8, an exactly full shape
}
EXPERIMENTAL = {"blk1": (4, 3, 8, 1), "blk2": (4, 3, 8, 2), "e2_blk1": (2, 6, 16, 1)}     # the geometries the launcher instantiates beside the library's choice
EXPERIMENTAL_NS = [641, 7, 130]

_NAN = float("nan")


def memories(PF):
    return [1, 3, PF - 1, PF, PF + 1]


def new_state(frx, ns, m, geom, hs, rng):
    """A state for vectors of lengths ns: the first candidate starts at an odd offset, every array has a sentinel tail (NaN, or -77 for the flags) behind what
    the batch owns, the vectors hold finite noise, the history is zero as a plan starts it, gt[..][3] (never used) is a sentinel as well."""
    B = len(ns)
    xoff = np.zeros(B + 1, np.int32); xoff[0] = 3; xoff[1:] = 3 + np.cumsum(ns)
    nv = int(xoff[-1]) + 5
    st = dict(geom=tuple(geom), hs=int(hs), m=int(m), xoff=xoff)
    for k in ref.VEC:
        v = np.full(nv, _NAN); v[xoff[0]:xoff[-1]] = rng.uniform(-1.0, 1.0, int(xoff[-1] - xoff[0])); st[k] = v
    nh = B * m * hs
    for k in ("S", "Y"):
        v = np.zeros(nh + 37); v[nh:] = _NAN; st[k] = v
    st["ys"] = np.concatenate([np.zeros(B * m), np.full(3, _NAN)])
    gt = np.zeros(4 * B * m + 6); gt[3:4 * B * m:4] = -12345.678; gt[4 * B * m:] = _NAN; st["gt"] = gt
    res = np.zeros(B + 2, frx.DV_RESULT)
    res.view(np.float64)[:] = rng.uniform(1.0, 2.0, 8 * (B + 2))                 # stale results: what no bit of a command asks for must stay
    st["res"] = res
    pieces = [[1, 100, 65, 64, 300, 7][b % 6] for b in range(B)]                 # fine pieces per candidate: fewer and more than a workgroup has threads
    poff = np.zeros(B + 1, np.int32); poff[0] = 2; poff[1:] = 2 + np.cumsum(pieces)
    st["poff"] = poff
    st["pflags"] = np.full(int(poff[-1]) + 4, -77, np.int32)
    st["dflags"] = np.full(B + 3, -77, np.int32)
    return st


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def synthetic_rounds(frx, st, rng, advances):
    """Rounds (cmd, f) of ONE launch each with mixed commands; the generator writes the evaluation's part - the accepted point (x, g) of a candidate about to
    advance - into st before it yields.  Candidate b starts b rounds late (idle until then), evaluates its start point with DV_EVAL alone, starts with INIT,
    then advances `advances` times; twice on the way a rejected trial follows an advance (TRIAL alone at a step that is not 1).  Candidate 0 then fails a line
    search: one more trial and a RESTORE while its neighbours advance.  Who is finished stays idle.  Scales per candidate: gradients 1e-6 .. 1e6, steps 1 .. 1e-8."""
    B = len(st["xoff"]) - 1; m = st["m"]
    sg = 10.0 ** np.linspace(-6.0, 6.0, B) if B > 1 else np.array([1.0])
    ss = 10.0 ** np.linspace(0.0, -8.0, B) if B > 1 else np.array([1e-3])
    plans = []
    for b in range(B):
        p = [0] * b + [DV_EVAL, DV_EVAL | DV_INIT | DV_TRIAL]
        retry_at = {2 + b % 3, m + 2}                                     # a rejected trial early, and one after the history has wrapped
        for k in range(advances):
            p.append(DV_EVAL | DV_ADVANCE | DV_TRIAL)
            if k in retry_at:
                p.append(DV_EVAL | DV_TRIAL)
        if b == 0:
            p += [DV_EVAL | DV_TRIAL, DV_RESTORE]
        plans.append(p)
    rounds = max(len(p) for p in plans) + 1                               # (one last round in which everybody is idle)
    k_adv = [0] * B
    for r in range(rounds):
        cmd = np.zeros(B, frx.DV_COMMAND)
        for b in range(B):
            fl = plans[b][r] if r < len(plans[b]) else 0
            lo, hi = int(st["xoff"][b]), int(st["xoff"][b + 1]); n = hi - lo
            cmd[b]["flags"] = fl
            cmd[b]["step"] = 1.0 if fl & (DV_INIT | DV_ADVANCE) else (0.37 if fl & DV_TRIAL else 0.0)
            if fl & DV_INIT:
                st["x"][lo:hi] = rng.uniform(-1.0, 1.0, n); st["g"][lo:hi] = sg[b] * rng.uniform(-0.5, 0.5, n)
                cmd[b]["step"] = 1.0 / max(np.sqrt(st["g"][lo:hi] @ st["g"][lo:hi]), 1e-300)
            if fl & DV_ADVANCE:                                           # the accepted point: a step that correlates with the gradient change, so y.s > 0 mostly
                k = k_adv[b]; k_adv[b] += 1
                sx = 0.1 * ss[b] * rng.uniform(-0.5, 0.5, n)
                st["x"][lo:hi] = st["xp"][lo:hi] + sx
                st["g"][lo:hi] = st["gp"][lo:hi] + 3.0 * (sg[b] / ss[b]) * sx + 0.05 * sg[b] * rng.uniform(-0.5, 0.5, n)
                cmd[b]["slot"] = k % m; cmd[b]["newest"] = k % m; cmd[b]["bound"] = min(k + 1, m)
            elif fl & (DV_TRIAL | DV_RESTORE) and not fl & DV_INIT:       # the gradient a rejected trial left behind
                st["g"][lo:hi] = sg[b] * rng.uniform(-0.5, 0.5, n)
        yield cmd, rng.uniform(-1e3, 1e3, B)


def drive(st, rounds, execute, d_tol=1e-9, stats=None, after_round=None):
    """Runs the rounds on st, handing every returned state back in; after each the comparator and the table check.  execute(st, cmd, f) works in place.
    after_round(r, cmd, st): further checks of the caller, returns a list of violations.  Returns every violation found, with its round."""
    B = len(st["xoff"]) - 1
    track = [(0, 0)] * B
    bad = []
    for r, (cmd, f) in enumerate(rounds):
        before = copy_state(st)
        execute(st, cmd, f)
        found = ref.compare(before, cmd, f, st, d_tol=d_tol, stats=stats)
        for b in range(B):
            if int(cmd[b]["flags"]) & DV_ADVANCE and not int(cmd[b]["flags"]) & DV_RESTORE:
                track[b] = (int(cmd[b]["slot"]), int(cmd[b]["bound"]))
            elif int(cmd[b]["flags"]) & DV_INIT and not int(cmd[b]["flags"]) & DV_RESTORE:
                track[b] = (0, 0)
        found += ref.check_tables(st, track)
        if after_round is not None:
            found += after_round(r, cmd, st)
        bad += [f"round {r} (flags {[int(c) for c in cmd['flags']]}): {t}" for t in found]
        if len(bad) > 20:
            break
    return bad


# ---- harvested histories -------------------------------------------------------------------------------------------------------------------------------

HEADLINE = dict(cands=[(0, 64, 16, False)], kappa=16, m=128, iterations=300)                               # n = 633; 2 m + 40 = 296 accepted steps at least
RAGGED = dict(cands=[(4, 64, 16, True), (7, 12, 3, True), (62, 2, 0, False)], kappa=16, m=8, iterations=40)   # n = 839, 139, 9 under (2, 7, 16, 4): m <= PF


@functools.lru_cache(maxsize=None)
def harvest(sid, N, gates, obstacles, kappa, m, iterations):
    """The points the CPU oracle's L-BFGS (history m, otherwise the planner's parameters) accepts from the initial guess on: dict(n, x [K+1][n], g [K+1][n],
    f [K+1], step [K]: step[k] leads from point k to point k+1, evaluated: every point the solver evaluated, index: where the accepted ones sit in it)."""
    from fast_racing_amd import scenario as sc
    from oracle import binding as ob
    cand = sc.make_candidate(sid, N, gates, obstacles=obstacles)
    o = ob.Oracle(cand, sc.ZHANGJIAJIE, qd_intervals=kappa)
    L = ob.lib()
    pm = ob.lbfgs_params(mem_size=m, past=3, g_epsilon=1e-16, min_step=1e-32, delta=1e-12, max_iterations=iterations)
    x = o.initial_guess(); fx = C.c_double()
    cap = 64 * iterations + 64
    tf = np.zeros(cap); ts = np.zeros(cap); tl = np.zeros(cap, np.int32); cnt = C.c_int()
    L.orc_trace_begin(o.h, cap)
    L.orc_lbfgs_run(o.n, x, C.byref(fx), L.orc_objective_fnptr(), o.h, pm, cap, tf, ts, tl, C.byref(cnt))
    pts = np.zeros((cap, o.n))
    pts = pts[:L.orc_trace_get(o.h, pts.ctypes.data, cap)].copy()
    K = cnt.value
    assert K <= cap and len(pts) < cap, f"harvest: the trace was cut at {cap} entries ({K} iterations, {len(pts)} evaluated points)"
    index = np.concatenate([[0], np.cumsum(tl[:K])])                     # the accepted points sit at the cumulative line-search counts
    assert index[-1] < len(pts), f"harvest: {len(pts)} evaluated points recorded, the line-search counts ask for {index[-1] + 1}"
    xs = pts[index]
    fg = [o.objective(xk) for xk in xs]
    return dict(n=o.n, x=xs, g=np.array([q[1] for q in fg]), f=np.array([q[0] for q in fg]), f_solver=tf[:K].copy(), step=ts[:K].copy(), evaluated=pts, index=index,
                oracle=o)


def harvested(spec):
    return [harvest(*c, spec["kappa"], spec["m"], spec["iterations"]) for c in spec["cands"]]


def harvested_rounds(frx, st, seqs):
    """Open-loop replay of the harvested sequences: round 0 INIT at (x_0, g_0), round k ADVANCE at the accepted (x_k, g_k), each with the trial at the step the
    solver accepted next; a candidate whose sequence has ended is idle."""
    B = len(seqs); m = st["m"]
    for r in range(max(len(s["step"]) for s in seqs) + 1):
        cmd = np.zeros(B, frx.DV_COMMAND); f = np.zeros(B)
        for b, s in enumerate(seqs):
            K = len(s["step"])
            if r > K:
                continue
            lo, hi = int(st["xoff"][b]), int(st["xoff"][b + 1])
            st["x"][lo:hi] = s["x"][r]; st["g"][lo:hi] = s["g"][r]
            fl = DV_EVAL | (DV_INIT if r == 0 else DV_ADVANCE)
            if r < K:
                fl |= DV_TRIAL; cmd[b]["step"] = s["step"][r]; f[b] = s["f"][r + 1]
            cmd[b]["flags"] = fl
            if r > 0:
                cmd[b]["slot"] = cmd[b]["newest"] = (r - 1) % m; cmd[b]["bound"] = min(r, m)
        yield cmd, f


def next_point_check(seqs, tol=1e-9):
    """after_round for drive: the trial point of round r reproduces the oracle's accepted point r + 1 to `tol` (relative, max-norm)."""
    def check(r, cmd, st):
        bad = []
        for b, s in enumerate(seqs):
            if int(cmd[b]["flags"]) & DV_TRIAL:
                lo, hi = int(st["xoff"][b]), int(st["xoff"][b + 1])
                err = ref.rel_max(st["x"][lo:hi], s["x"][r + 1])
                if not err <= tol:
                    bad.append(f"cand {b}: trial point is {err:.3e} from the oracle's accepted point {r + 1}")
        return bad
    return check


def _lanes_dot(a, b):
    """a . b summed like a wave would: 64 partial sums over strided elements, then those."""
    p = a * b
    full = p.size // 64 * 64
    lanes = p[:full].reshape(-1, 64).sum(axis=0) if full else np.zeros(64, p.dtype)
    lanes[:p.size - full] += p[full:]
    return lanes.sum()


@functools.lru_cache(maxsize=None)
def reference_error(sid, N, gates, obstacles, kappa, m, iterations):
    """What a plain double two-loop recursion loses on the harvested states: worst relative max-norm error against long double over the sequence, the worse of two
    summation orders (numpy's sum of products; 64 strided partial sums).  Returns (worst, worst of order 1, worst of order 2)."""
    s = harvest(sid, N, gates, obstacles, kappa, m, iterations)
    n, K = s["n"], len(s["step"])
    S = np.zeros((m, n)); Y = np.zeros((m, n))
    w = [0.0, 0.0]
    for k in range(1, K + 1):
        j = (k - 1) % m
        S[j] = s["x"][k] - s["x"][k - 1]; Y[j] = s["g"][k] - s["g"][k - 1]
        d_ld = ref.two_loop(S, Y, s["g"][k], j, min(k, m), m, n)
        for i, dot in enumerate((None, _lanes_dot)):
            w[i] = max(w[i], ref.rel_max(ref.two_loop(S, Y, s["g"][k], j, min(k, m), m, n, dtype=np.float64, dot=dot), d_ld))
    return max(w), w[0], w[1]
