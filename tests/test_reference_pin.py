"""PIN of the CPU oracle against the reference's OWN code.

oracle/_ref/libref_gcopter.so is the reference's CPU path — se3gcopter_cpu.hpp, trajectory.hpp, geoutils.hpp, sdlp.hpp,
quickhull.hpp, lbfgs.hpp — compiled unmodified from /root/reference against oracle/eigen_shim (a minimal stand-in for the
Eigen API those headers use; Eigen itself is not installed).  The restatement in oracle/gcopter_oracle.cpp must reproduce
it on identical inputs: initial guess, forward map, penalty integrator, and the full L-BFGS callback (f, grad)."""
import os

import numpy as np
import pytest

REFPIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin_cases.npz")


def rel(a, b, floor=0.0):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), floor, 1e-300))


@pytest.fixture(scope="module")
def have_ref(ob):
    if ob.ref_gcopter() is None:
        pytest.skip("oracle/_ref/libref_gcopter.so not built (needs /root/reference at build time)")
    return True


CASES = [(0, 16, 4, 8, False, {}), (3, 32, 8, 16, True, {}), (5, 12, 3, 48, False, {}), (7, 10, 2, 8, True, dict(rho=0.0, total_t=7.0, c2_diffeo=0)),
         (8, 10, 2, 8, False, dict(rho=0.0, total_t=7.0, c2_diffeo=1)), (9, 6, 1, 8, False, dict(c2_diffeo=0)),
         (0, 64, 16, 16, False, {}), (2, 64, 16, 16, True, {})]          # the headline geometry (BASELINE.json configs[2]): K_i = 8, and K_i = 8 ... 14


def reference_outputs(o, r):
    """What the pin compares, taken from the reference handle r: dimensions, initial guess, and at three points (the initial guess, the oracle's
    iterates after 30 and 300 iterations from it) the objective, the forward map and the penalty integrator at the reference's own (T, C)."""
    x0 = r.initial_guess()
    pts = [x0, o.optimize(1e-6, max_iterations=30, x0=x0)["x"], o.optimize(1e-6, max_iterations=300, x0=x0)["x"]]
    rows = []
    for x in pts:
        fr, gr = r.objective(x)                                     # SE3GCOPTER::objectiveFunc itself
        Tr, Cr = r.forward(x)                                       # forwardT/P + MINCO_S3::generate (banded LU)
        cr, gtr, gcr = r.penalty(Tr, Cr)                            # MINCO_S3::addTimeIntPenalty
        rows.append((fr, gr, Tr, Cr, cr, gtr, gcr))
    out = {"dims": np.array([r.coarse_n, r.fine_n, r.dim_t, r.dim_p]), "x0": x0, "pts": np.array(pts)}
    out.update({k: np.array([row[j] for row in rows]) for j, k in enumerate(("f", "g", "T", "C", "pen", "pen_gT", "pen_gC"))})
    return out


@pytest.mark.parametrize("sid,N,gates,kappa,obst,over", CASES)
def test_oracle_reproduces_the_reference_cpu_path(sc, ob, sid, N, gates, kappa, obst, over):
    cand = sc.make_candidate(sid, N, gates, obstacles=obst)
    o = ob.Oracle(cand, sc.ZHANGJIAJIE, qd_intervals=kappa, **over)
    if ob.ref_gcopter() is not None:
        ref = reference_outputs(o, ob.Reference(cand, sc.ZHANGJIAJIE, override_vs=True, qd_intervals=kappa, **over))
    else:                                                           # no reference tree to build it from: its outputs at these inputs, recorded
        i = CASES.index((sid, N, gates, kappa, obst, over))         # by tests/golden/make_refpin.py
        d = np.load(REFPIN)
        ref = {k.split("_", 1)[1]: d[k] for k in d.files if k.startswith(f"{i}_")}
    assert (o.coarse_n, o.fine_n, o.dim_t, o.dim_p) == tuple(int(v) for v in ref["dims"])
    assert rel(o.initial_guess(), ref["x0"]) < 1e-13                # setInitial + backwardT + backwardP (nested L-BFGS)
    for j, x in enumerate(ref["pts"]):
        fo, go = o.objective(x)
        assert abs(fo - ref["f"][j]) <= 1e-12 * abs(ref["f"][j])
        assert rel(go, ref["g"][j], abs(ref["f"][j])) < 1e-9
        To, Po, Co = o.forward(x)
        assert rel(To, ref["T"][j]) < 1e-14 and rel(Co, ref["C"][j]) < 1e-10
        co, gto, gco = o.penalty(ref["T"][j], ref["C"][j])
        assert abs(co - ref["pen"][j]) <= 1e-11 * max(abs(ref["pen"][j]), 1e-300)
        assert rel(gto, ref["pen_gT"][j]) < 1e-10 and rel(gco, ref["pen_gC"][j]) < 1e-10


def test_reference_against_itself_shows_the_path_sensitivity(have_ref, sc, ob):
    """The reference's optimize() and the oracle's — whose objective agrees with it to 1e-14 — end 5e-3 apart in the
    coefficients at the stock tolerance: the 1e-6 contract on optimised coefficients is not a property independent runs
    of the REFERENCE ALGORITHM have; both reach the same objective level."""
    cand = sc.make_candidate(0, 16, 4)
    o = ob.Oracle(cand, sc.ZHANGJIAJIE, qd_intervals=8)
    r = ob.Reference(cand, sc.ZHANGJIAJIE, override_vs=True, qd_intervals=8)
    ro = o.optimize(1e-6); rr = r.optimize(1e-6)
    spread = rel(ro["C"], rr["C"])
    fo = o.objective(ro["x"])[0]
    # objective of the reference's final trajectory, evaluated by mapping its (T, C) through the penalty + jerk + rho*T terms
    pen, _, _ = o.penalty(rr["T"], rr["C"])
    fr = rr["jerk_cost"] + pen + sc.ZHANGJIAJIE["rho"] * rr["T"].sum()
    print(f"coefficient spread {spread:.2e}; objective oracle {fo:.6f} reference {fr:.6f}")
    assert 1e-6 < spread < 5e-2                                     # documented: far above 1e-6, yet the same optimum
    assert abs(fo - fr) <= 5e-3 * fr


def test_reference_vertex_enumeration_agrees_with_the_generator(have_ref, sc, ob):
    """f1 row preview: geoutils::enumerateVs (Seidel LP + polar-dual quickhull, se3gcopter_cpu.hpp:1031-1074) finds the same
    vertex SETS as the generator's brute-force enumeration; only the order (hence v0) differs."""
    cand = sc.make_candidate(4, 12, 3, obstacles=True)
    r = ob.Reference(cand, sc.ZHANGJIAJIE, override_vs=False, qd_intervals=8)
    for m, V in enumerate(cand.v_polys):
        Vr = r.vpoly(m)
        assert Vr.shape == V.shape
        a = V.T[np.lexsort((V[2], V[1], V[0]))]; b = Vr.T[np.lexsort((np.round(Vr[2], 6), np.round(Vr[1], 6), np.round(Vr[0], 6)))]
        d = np.abs(a[:, None, :] - b[None, :, :]).max(axis=2).min(axis=1)      # every generator vertex has a reference twin
        assert d.max() < 1e-6
