"""Hand-made piece rows for the host fold of frx_trajectory_check / _extrema / _clearance (fast-racing_amd/csrc/frx_traj_fold.hpp): three candidates of
1, 2 and 4 pieces.  tests/test_trajectory_fold_cpu.py folds them through frx_debug_fold_rows and through the Python restatements;
tests/hostcheck/fold_rows_main.cpp folds the same rows from the text file that `python tests/fold_cases.py FILE` writes."""
import sys

import numpy as np

POFF = [0, 1, 3, 7]
# durations whose sums depend on the order: (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)
T = np.array([0.7, 1.3, 0.45, 0.1, 0.2, 0.3, 0.9])
LIMITS = dict(vel_max=6.0, thr_acc_min=2.0, thr_acc_max=18.0, body_rate_max=3.5)
LIMITS4 = np.array([LIMITS["vel_max"], LIMITS["thr_acc_min"], LIMITS["thr_acc_max"], LIMITS["body_rate_max"]])
NAN, INF = float("nan"), float("inf")

# per kind: name, fields of a row, (lo, hi) of every folded field - inside the limits, so that a base row raises no flag -, which of them fold as a minimum,
# and the flag limits as (field, limit, side the flag lies on, bit)
KINDS = {
    0: dict(name="check", fields=8, ranges=[(-1.0, -0.1), (1.0, 5.0), (3.0, 8.0), (9.0, 15.0), (0.5, 3.0), (1.0, 9.0)], mins=(2,),
            limits=[(0, 0.0, +1, 1), (1, LIMITS["vel_max"], +1, 2), (2, LIMITS["thr_acc_min"], -1, 4), (3, LIMITS["thr_acc_max"], +1, 8),
                    (4, LIMITS["body_rate_max"], +1, 16)], nonfinite=32),
    1: dict(name="extrema", fields=10, ranges=[(1.0, 5.0), (1.0, 9.0), (3.0, 8.0), (9.0, 15.0), (0.5, 3.0)], mins=(2,),
            limits=[(0, LIMITS["vel_max"], +1, 2), (2, LIMITS["thr_acc_min"], -1, 4), (3, LIMITS["thr_acc_max"], +1, 8),
                    (4, LIMITS["body_rate_max"], +1, 16)], nonfinite=32),
    2: dict(name="clearance", fields=4, ranges=[(1.5, 4.0), (0.3, 2.0)], mins=(0, 1), limits=[(0, 1.0, -1, 1)], nonfinite=2),
}


def base_rows(kind):
    """Finite rows, all different, inside every limit; the carried fields are local times in [0, T] (and a small integer in the last field of kinds 0, 2)."""
    k = KINDS[kind]
    rows = np.zeros((len(T), k["fields"]))
    for gp in range(len(T)):
        for f in range(k["fields"]):
            frac = ((gp * 37 + f * 21 + 11) % 64) / 64.0
            if f < len(k["ranges"]):
                lo, hi = k["ranges"][f]
                rows[gp, f] = lo + (hi - lo) * frac
            else:
                rows[gp, f] = T[gp] * frac
        if kind in (0, 2):
            rows[gp, -1] = float((gp * 5 + 2) % 7)
    return rows


def piece(b, local):
    return POFF[b] + local


def cases(kind):
    """(name, rows) of every case of one kind"""
    k = KINDS[kind]
    base = base_rows(kind)
    out = [("base", base)]

    def put(name, edits):
        r = base.copy()
        for gp, f, v in edits:
            r[gp, f] = v
        out.append((name, r))

    for f in range(k["fields"]):
        # a NaN in the first, a middle and the last piece (the single piece is all three)
        put(f"nan_first_f{f}", [(piece(0, 0), f, NAN), (piece(1, 0), f, NAN), (piece(2, 0), f, NAN)])
        put(f"nan_middle_f{f}", [(piece(2, 1), f, NAN)])
        put(f"nan_middle2_f{f}", [(piece(2, 2), f, NAN)])
        put(f"nan_last_f{f}", [(piece(1, 1), f, NAN), (piece(2, 3), f, NAN)])
        # a later NaN against a running one
        put(f"nan_twice_f{f}", [(piece(1, 0), f, NAN), (piece(1, 1), f, NAN), (piece(2, 1), f, NAN), (piece(2, 3), f, NAN)])
        # non-finite values of either kind and sign
        put(f"inf_f{f}", [(piece(0, 0), f, INF), (piece(1, 1), f, -INF), (piece(2, 2), f, INF)])
        put(f"neg_inf_f{f}", [(piece(2, 1), f, -INF)])
    for f, (lo, hi) in enumerate(k["ranges"]):
        worst = lo - 0.25 if f in k["mins"] else hi + 0.25
        # two pieces tied for the worst value: the first wins
        put(f"tie_13_f{f}", [(piece(2, 1), f, worst), (piece(2, 3), f, worst), (piece(1, 0), f, worst), (piece(1, 1), f, worst)])
        put(f"tie_23_f{f}", [(piece(2, 2), f, worst), (piece(2, 3), f, worst)])
        put(f"tie_all_f{f}", [(gp, f, worst) for gp in range(len(T))])
        # the worst in the last piece: its time rides on the prefix of three durations
        put(f"worst_last_f{f}", [(piece(2, 3), f, worst), (piece(1, 1), f, worst)])
    for f, limit, side, _ in k["limits"]:
        past = np.nextafter(limit, side * INF)
        # exactly at the limit, and the next double past it: in the single piece, the second of two and the third of four
        put(f"at_limit_f{f}", [(piece(0, 0), f, limit), (piece(1, 1), f, limit), (piece(2, 2), f, limit)])
        put(f"past_limit_f{f}", [(piece(0, 0), f, past), (piece(1, 1), f, past), (piece(2, 2), f, past)])
        put(f"at_and_past_f{f}", [(piece(0, 0), f, limit), (piece(1, 1), f, past), (piece(2, 2), f, limit)])
    return out


def expected_flags_at_limits(kind, name):
    """flag words the limit cases must give, written down independently of any fold: {case name: (flags of the three candidates)}"""
    for f, _, _, bit in KINDS[kind]["limits"]:
        if name == f"at_limit_f{f}":
            return (0, 0, 0)
        if name == f"past_limit_f{f}":
            return (bit, bit, bit)
        if name == f"at_and_past_f{f}":
            return (0, bit, 0)
    return None


def dump(path):
    """Text file of every case: `kind B P`, then poff, T, the limits and the rows, doubles as C hexadecimal literals (nan and inf by name)"""
    with open(path, "w") as fh:
        for kind in KINDS:
            for _, rows in cases(kind):
                fh.write(f"{kind} {len(POFF) - 1} {len(T)}\n")
                fh.write(" ".join(str(v) for v in POFF) + "\n")
                for arr in (T, LIMITS4, rows.reshape(-1)):
                    fh.write(" ".join(float(v).hex() for v in arr) + "\n")


if __name__ == "__main__":
    dump(sys.argv[1])
