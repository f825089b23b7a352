"""The commands of the device-vector L-BFGS (fast-racing_amd/csrc/frx_lbfgs.hpp: DvCommand / DvResult, k_lbfgs_pre and k_lbfgs_post of
frx_lbfgs_kernels.hpp) restated in numpy.longdouble on the state frx.dv_round works on, and the comparator that holds a device round against it.

State (a dict, see frx.dv_round): geom (E, W, PF, BLK), hs, m, xoff; packed x, g, xp, gp, d; S, Y [B][m][hs]; ys [B][m]; gt [B][m][4] with
gt[j][k-1] = s_j . y_{j+k}; res (DV_RESULT records); optionally poff, dflags, pflags.  Arrays may be longer than the batch needs (sentinel tails).

What is exact and what is bounded (compare):
  bit for bit   INIT: d = -g, xp = x, gp = g.  ADVANCE: row `slot` of S = x - xp and of Y = g - gp (one double subtraction each), zero from n to hs, xp = x,
                gp = g.  RESTORE: x = xp, g = gp.  dflags / pflags = the command's flags.  res.f = f.  Everything else, sentinel tails included, unchanged.
  derived       every dot product (ys[slot], the new gt entries, dginit against the device's own d, dg / xx / gg) against the long-double one by
                n 2^-52 sum |a_i b_i|: any summation order, with or without FMA, stays below n u sum |a_i b_i| (1 + O(n u)) with u = 2^-53.
                TRIAL: |x_i - (xp_i + step d_i)| <= 2^-52 (|step d_i| + |xp_i|): one rounding (FMA) or two (product, then sum).
  by tolerance  the direction d of an ADVANCE against the long-double two-loop recursion (lbfgs.hpp:1381-1411) over the rows the device stored, relative max-norm.
"""
import copy

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
DV_EVAL, DV_INIT, DV_ADVANCE, DV_TRIAL, DV_RESTORE = 1, 2, 4, 8, 16
VEC = ("x", "g", "xp", "gp", "d")


def ld_dot(a, b):
    """(sum a_i b_i, sum |a_i b_i|) in long double."""
    p = np.asarray(a, LD) * np.asarray(b, LD)
    return p.sum(), np.abs(p).sum()


def two_loop(Sb, Yb, g, newest, bound, m, n, dtype=LD, dot=None):
    """d = -H g by the reference's two-loop recursion (lbfgs.hpp:1381-1411) over history rows Sb, Yb [m][>= n]; y.s and y.y are formed from the rows in
    `dtype` as well.  dot(a, b): the summation to use (default: numpy's sum of the products)."""
    if dot is None:
        dot = lambda a, b: (a * b).sum()
    S = np.asarray(Sb[:, :n], dtype); Y = np.asarray(Yb[:, :n], dtype)
    d = -np.asarray(g, dtype)
    alpha = np.zeros(m, dtype)
    j = (newest + 1) % m
    ys = np.zeros(m, dtype)
    for _ in range(bound):
        j = (j + m - 1) % m
        ys[j] = dot(Y[j], S[j])
        alpha[j] = dot(S[j], d) / ys[j]
        d = d - alpha[j] * Y[j]
    d = d * (ys[newest] / dot(Y[newest], Y[newest]))
    for _ in range(bound):
        beta = dot(Y[j], d) / ys[j]
        d = d + (alpha[j] - beta) * S[j]
        j = (j + 1) % m
    return d


def rel_max(a, ref):
    ref = np.asarray(ref, LD)
    den = np.abs(ref).max() if ref.size else LD(0)
    num = np.abs(np.asarray(a, LD) - ref).max() if ref.size else LD(0)
    if not np.isfinite(num):
        return float("inf")
    return float(num / den) if den > 0 else (0.0 if num == 0 else float("inf"))


def hist(st, name, b):
    """candidate b's [m][hs] block of S or Y (a view)."""
    m, hs = st["m"], st["hs"]
    return st[name][b * m * hs:(b + 1) * m * hs].reshape(m, hs)


def row_of_age(slot, a, m):
    return (slot - a) % m


def apply(st, cmd, f=None):
    """One round of the model, IN PLACE: what k_lbfgs_pre does with cmd[B], then k_lbfgs_post when f[B] is given.  Values the device rounds in an order of
    its own are computed in long double and rounded once."""
    m, hs, BLK = st["m"], st["hs"], st["geom"][3]
    B = len(st["xoff"]) - 1
    for b in range(B):
        c = cmd[b]; fl = int(c["flags"])
        lo, hi = int(st["xoff"][b]), int(st["xoff"][b + 1]); n = hi - lo
        if st.get("dflags") is not None:
            st["dflags"][b] = fl
        if st.get("poff") is not None:
            st["pflags"][st["poff"][b]:st["poff"][b + 1]] = fl
        x, g, xp, gp, d = (st[k][lo:hi] for k in VEC)
        if fl & DV_RESTORE:                                            # lbfgs.hpp:1287-1288; nothing else happens in such a round
            x[:] = xp; g[:] = gp
        elif fl & (DV_INIT | DV_ADVANCE | DV_TRIAL):
            if fl & DV_INIT:
                d[:] = -g; xp[:] = x; gp[:] = g
                st["res"]["dginit"][b] = float(ld_dot(g, d)[0])
            elif fl & DV_ADVANCE:
                slot, bound = int(c["slot"]), int(c["bound"])
                Sb, Yb = hist(st, "S", b), hist(st, "Y", b)
                Sb[slot, :n] = x - xp; Sb[slot, n:] = 0.0
                Yb[slot, :n] = g - gp; Yb[slot, n:] = 0.0
                st["ys"][b * m + slot] = float(ld_dot(Yb[slot, :n], Sb[slot, :n])[0])
                if BLK > 1:
                    for k in range(1, min(3, bound - 1) + 1):
                        j = row_of_age(slot, k, m)
                        st["gt"][(b * m + j) * 4 + k - 1] = float(ld_dot(Sb[j, :n], Yb[slot, :n])[0])
                d[:] = two_loop(Sb, Yb, g, slot, bound, m, n).astype(np.float64)
                xp[:] = x; gp[:] = g
                st["res"]["dginit"][b] = float(ld_dot(g, d)[0])
            if fl & DV_TRIAL:
                x[:] = (np.asarray(xp, LD) + LD(c["step"]) * np.asarray(d, LD)).astype(np.float64)
        if f is not None and fl & DV_EVAL:
            r = st["res"]
            r["f"][b] = f[b]; r["dg"][b] = float(ld_dot(g, d)[0]); r["xx"][b] = float(ld_dot(x, x)[0]); r["gg"][b] = float(ld_dot(g, g)[0])
    return st


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def compare(before, cmd, f, after, d_tol=1e-9, stats=None):
    """Holds `after` (the device's state after one round on `before` with cmd, f) to the rules in the module's text.  Returns the list of violations (empty:
    the round stands).  d_tol: the direction's tolerance, one number or one per candidate.  stats (a dict, optional): "d_err" collects the direction error of every ADVANCE as (candidate, relative error)."""
    bad = []
    m, hs, BLK = before["m"], before["hs"], before["geom"][3]
    B = len(before["xoff"]) - 1
    exp = {k: (v.copy() if isinstance(v, np.ndarray) else copy.copy(v)) for k, v in before.items()}      # what is exact is built here; what is bounded is taken over from `after` once it has passed

    def dot_ok(what, b, got, a_, b_, n):
        ref, mag = ld_dot(a_, b_)
        err = abs(LD(got) - ref)
        if not err <= LD(n) * EPS * mag:
            bad.append(f"cand {b}: {what} = {got!r} is {float(err):.3e} from the long-double {float(ref)!r}, bound {float(LD(n) * EPS * mag):.3e}")

    for b in range(B):
        c = cmd[b]; fl = int(c["flags"])
        lo, hi = int(before["xoff"][b]), int(before["xoff"][b + 1]); n = hi - lo
        if exp.get("dflags") is not None:
            exp["dflags"][b] = fl
        if exp.get("poff") is not None:
            exp["pflags"][exp["poff"][b]:exp["poff"][b + 1]] = fl
        ex, eg, exp_, egp, ed = (exp[k][lo:hi] for k in VEC)
        ax, ag, axp, agp, ad = (after[k][lo:hi] for k in VEC)
        if fl & DV_RESTORE:
            ex[:] = exp_; eg[:] = egp
        elif fl & (DV_INIT | DV_ADVANCE | DV_TRIAL):
            if fl & DV_INIT:
                ed[:] = -eg; exp_[:] = ex; egp[:] = eg
                dot_ok("dginit (INIT)", b, after["res"]["dginit"][b], eg, ad, n)
                exp["res"]["dginit"][b] = after["res"]["dginit"][b]
            elif fl & DV_ADVANCE:
                slot, bound = int(c["slot"]), int(c["bound"])
                Sb, Yb = hist(exp, "S", b), hist(exp, "Y", b)
                Sb[slot, :n] = ex - exp_; Sb[slot, n:] = 0.0
                Yb[slot, :n] = eg - egp; Yb[slot, n:] = 0.0
                aS, aY = hist(after, "S", b), hist(after, "Y", b)
                rows_ok = _same(aS, Sb) and _same(aY, Yb)
                dot_ok(f"ys[{slot}]", b, after["ys"][b * m + slot], aY[slot, :n], aS[slot, :n], n)
                exp["ys"][b * m + slot] = after["ys"][b * m + slot]
                if BLK > 1:
                    for k in range(1, min(3, bound - 1) + 1):
                        j = row_of_age(slot, k, m); at = (b * m + j) * 4 + k - 1
                        dot_ok(f"gt[{j}][{k - 1}] = s_{j} . y_{slot}", b, after["gt"][at], aS[j, :n], aY[slot, :n], n)
                        exp["gt"][at] = after["gt"][at]
                if rows_ok:                                             # (rows that differ are reported below, bit for bit; a direction from them would say nothing)
                    ref = two_loop(aS, aY, eg, slot, bound, m, n)
                    err = rel_max(ad, ref)
                    if stats is not None:
                        stats.setdefault("d_err", []).append((b, err))
                    tol = d_tol[b] if np.ndim(d_tol) else d_tol
                    if not err <= tol:
                        bad.append(f"cand {b}: direction of the advance into slot {slot} (bound {bound}, n {n}) is {err:.3e} from the long-double recursion, tolerance {tol:.3e}")
                ed[:] = ad
                exp_[:] = ex; egp[:] = eg
                dot_ok("dginit (ADVANCE)", b, after["res"]["dginit"][b], eg, ad, n)
                exp["res"]["dginit"][b] = after["res"]["dginit"][b]
            if fl & DV_TRIAL:
                step = LD(c["step"])
                sd = step * np.asarray(ed, LD); ref = np.asarray(exp_, LD) + sd
                off = np.abs(np.asarray(ax, LD) - ref); lim = EPS * (np.abs(sd) + np.abs(np.asarray(exp_, LD)))
                w = np.flatnonzero(~(off <= lim))
                if w.size:
                    i = int(w[0])
                    bad.append(f"cand {b}: trial point element {i} of {n}: {ax[i]!r} is {float(off[i]):.3e} from xp + step d = {float(ref[i])!r}, bound {float(lim[i]):.3e} ({w.size} elements)")
                ex[:] = ax
        if f is not None and fl & DV_EVAL:
            r = after["res"]
            exp["res"]["f"][b] = f[b]
            dot_ok("dg", b, r["dg"][b], ag, ad, n); dot_ok("xx", b, r["xx"][b], ax, ax, n); dot_ok("gg", b, r["gg"][b], ag, ag, n)
            for k in ("dg", "xx", "gg"):
                exp["res"][k][b] = r[k][b]
    for k in VEC + ("S", "Y", "ys", "gt", "res", "dflags", "pflags"):
        if exp.get(k) is None:
            continue
        if not _same(exp[k], after[k]):
            ea, aa = exp[k], after[k]
            if k == "res":
                ea, aa = ea.view(np.float64), aa.view(np.float64)
            if ea.shape != aa.shape:
                bad.append(f"{k}: came back with {aa.shape} elements, went with {ea.shape}")
                continue
            w = np.flatnonzero((_bits(ea).reshape(ea.size, -1) != _bits(aa).reshape(aa.size, -1)).any(axis=1))
            bad.append(f"{k}: {w.size} elements differ bit for bit from what the commands allow, first at {describe(before, k, int(w[0]))}: "
                       f"expected {ea.reshape(-1)[w[0]]!r}, got {aa.reshape(-1)[w[0]]!r}")
    return bad


def describe(st, k, i):
    """Where element i of array k lies: candidate, row, position."""
    B = len(st["xoff"]) - 1; m, hs = st["m"], st["hs"]
    if k in VEC:
        if i < st["xoff"][0] or i >= st["xoff"][B]:
            return f"{k}[{i}] (outside every candidate: sentinel)"
        b = int(np.searchsorted(st["xoff"], i, side="right")) - 1
        return f"{k}[{i}] = candidate {b} element {i - int(st['xoff'][b])} of {int(st['xoff'][b + 1] - st['xoff'][b])}"
    if k in ("S", "Y"):
        if i >= B * m * hs:
            return f"{k}[{i}] (behind the history: sentinel)"
        b, r = divmod(i, m * hs); j, e = divmod(r, hs)
        return f"{k}[{i}] = candidate {b} row {j} element {e} (n = {int(st['xoff'][b + 1] - st['xoff'][b])}, hs = {hs})"
    if k == "ys":
        return f"ys[{i}] = candidate {i // m} slot {i % m}" if i < B * m else f"ys[{i}] (sentinel)"
    if k == "gt":
        return f"gt[{i}] = candidate {i // (4 * m)} slot {(i // 4) % m} entry {i % 4}" if i < 4 * B * m else f"gt[{i}] (sentinel)"
    if k == "res":
        return f"res[{i // 8}].{('f', 'dg', 'xx', 'gg', 'dginit', 'pad0', 'pad1', 'pad2')[i % 8]}"
    return f"{k}[{i}]"


def check_tables(st, track, stats=None):
    """The tables hold what the next advance will read: for candidate b with `bound` pairs, the newest in slot `newest` (track[b] = (newest, bound), bound 0:
    no pair yet), ys of every pair and gt[row(a)][k-1] = s_{age a} . y_{age a-k} for a = 1 .. bound-1, k = 1 .. min(3, a), by the dot-product bound, on the rows
    as they stand; every row zero from n to hs."""
    bad = []
    m, hs, BLK = st["m"], st["hs"], st["geom"][3]
    for b, (newest, bound) in enumerate(track):
        n = int(st["xoff"][b + 1] - st["xoff"][b])
        Sb, Yb = hist(st, "S", b), hist(st, "Y", b)
        if Sb[:, n:].any() or Yb[:, n:].any():
            bad.append(f"cand {b}: a history row is not zero from n = {n} to hs = {hs}")
        if bound < 1:
            continue
        rows = (newest - np.arange(bound)) % m                           # by age
        Sa, Ya = np.asarray(Sb[rows, :n], LD), np.asarray(Yb[rows, :n], LD)
        for k in range(0, (min(3, bound - 1) if BLK > 1 else 0) + 1):    # k = 0: y.s of every pair; k >= 1: s_{age a} . y_{age a-k}, a = k .. bound-1
            p = Sa[k:] * Ya[:bound - k]
            refv, mag = p.sum(axis=1), np.abs(p).sum(axis=1)
            got = st["ys"][b * m + rows] if k == 0 else st["gt"][(b * m + rows[k:]) * 4 + k - 1]
            for a in np.flatnonzero(~(np.abs(np.asarray(got, LD) - refv) <= LD(n) * EPS * mag)):
                j = int(rows[a + k])
                bad.append(f"cand {b}: {'ys[%d]' % j if k == 0 else 'gt[%d][%d]' % (j, k - 1)} (age {a + k}) = {got[a]!r}, the rows give {float(refv[a])!r}")
    return bad
