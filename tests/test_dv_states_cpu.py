"""The states, the long-double model and the comparator behind test_gpu_dv_commands.py, checked where there is no device: the layout the states rest on, the
harvested sequences' coherence, the model against the reference solver's iterates, the error of a plain double recursion (from which the device's margin is
taken), and planted errors the comparator has to catch."""
import numpy as np
import pytest

import dv_reference as ref
import dv_states as dvs
from dv_reference import DV_ADVANCE


def test_layout_query_gives_the_geometry_the_states_are_written_for(frx):
    for name, (ns, want) in dvs.BATCHES.items():
        assert frx.dv_layout(max(ns)) == want, name
        assert frx.dv_layout(max(ns), tight=False) == (want[0], 64 * want[0][0] * want[0][1]), name
    for name, geom in dvs.EXPERIMENTAL.items():
        assert frx.dv_layout(max(dvs.EXPERIMENTAL_NS), geom) == (geom, 656), name
    with pytest.raises(frx.FrxError):
        frx.dv_layout(4097)                                             # longer than any shape (8 waves x 8 doubles)
    with pytest.raises(frx.FrxError):
        frx.dv_layout(769, (4, 3, 8, 1))


def _model_run(frx, ns, m, geom, hs, seed, record=None):
    rng = np.random.default_rng(seed)
    st = dvs.new_state(frx, ns, m, geom, hs, rng)

    def execute(s, cmd, f):
        before = dvs.copy_state(s) if record is not None else None
        ref.apply(s, cmd, f)
        if record is not None:
            record.append((before, cmd.copy(), f.copy(), dvs.copy_state(s)))
    stats = {}
    bad = dvs.drive(st, dvs.synthetic_rounds(frx, st, rng, 2 * m + 3), execute, stats=stats)
    return bad, stats


@pytest.mark.parametrize("name", list(dvs.BATCHES))
def test_model_passes_its_own_comparator_on_every_synthetic_sequence(frx, name):
    """The sequences, the driver and the comparator as the device test runs them, on the model: no violation, and every class of command occurs."""
    ns, (geom, hs) = dvs.BATCHES[name]
    for m in (1, 3, geom[2] + 1):
        rec = []
        bad, stats = _model_run(frx, ns, m, geom, hs, seed=m, record=rec)
        assert not bad, "\n".join(bad[:5])
        flags = {int(fl) for _, cmd, _, _ in rec for fl in cmd["flags"]}
        assert {0, 1, 1 | 2 | 8, 1 | 4 | 8, 1 | 8, 16} <= flags
        assert m == 1 or any(len({(int(c["slot"]), int(c["bound"])) for c in cmd if c["flags"] & DV_ADVANCE}) > 1 for _, cmd, _, _ in rec)   # slot and bound differ inside a launch
        assert len(stats["d_err"]) == len(ns) * (2 * m + 3) and max(e for _, e in stats["d_err"]) < 1e-15    # (the model against itself: one rounding)


def _first(rec, pred):
    for before, cmd, f, after in rec:
        for b in range(len(cmd)):
            if pred(before, cmd, b):
                return before, cmd, f, dvs.copy_state(after), b
    raise AssertionError("no such round in the sequence")


def test_comparator_catches_planted_errors(frx):
    ns, (geom, hs) = dvs.BATCHES["headline"]
    m = 3
    rec = []
    bad, _ = _model_run(frx, ns, m, geom, hs, seed=11, record=rec)
    assert not bad
    adv = lambda bound_min=1, slot=None: (lambda st, cmd, b: cmd[b]["flags"] & DV_ADVANCE and cmd[b]["bound"] >= bound_min and (slot is None or cmd[b]["slot"] == slot)
                                          and st["xoff"][b + 1] - st["xoff"][b] > 1)
    span = lambda st, b: (int(st["xoff"][b]), int(st["xoff"][b + 1]))

    def run(case):
        before, cmd, f, after = case[:4]
        return ref.compare(before, cmd, f, after)

    # the last element left out of a dot product
    case = _first(rec, adv()); before, cmd, f, after, b = case
    lo, hi = span(before, b); slot = int(cmd[b]["slot"])
    assert not run(case)
    after["ys"][b * m + slot] = float(ref.ld_dot(ref.hist(after, "Y", b)[slot, :hi - lo - 1], ref.hist(after, "S", b)[slot, :hi - lo - 1])[0])
    assert any("ys[" in t for t in run(case))
    # a gt entry left stale after its row was overwritten
    case = _first(rec, lambda st, cmd, b: adv(bound_min=m, slot=0)(st, cmd, b) and st["gt"][(b * m + ref.row_of_age(0, 1, m)) * 4] != 0.0)
    before, cmd, f, after, b = case
    at = (b * m + ref.row_of_age(0, 1, m)) * 4
    assert before["gt"][at] != after["gt"][at] and before["gt"][at] != 0.0
    after["gt"][at] = before["gt"][at]
    assert any("gt[" in t for t in run(case))
    # a history row written one slot late at the wrap
    case = _first(rec, adv(bound_min=m, slot=m - 1)); before, cmd, f, after, b = case
    aS, bS = ref.hist(after, "S", b), ref.hist(before, "S", b)
    aS[0] = aS[m - 1]; aS[m - 1] = bS[m - 1]
    assert any(t.startswith("S:") for t in run(case))
    # a row's tail non-zero
    case = _first(rec, adv()); before, cmd, f, after, b = case
    lo, hi = span(before, b)
    ref.hist(after, "Y", b)[int(cmd[b]["slot"]), hi - lo] = 1e-300
    assert any(t.startswith("Y:") for t in run(case))
    assert ref.check_tables(after, [(int(cmd[q]["slot"]), 0) for q in range(len(ns))])
    # xp not updated on ADVANCE
    case = _first(rec, adv()); before, cmd, f, after, b = case
    lo, hi = span(before, b)
    after["xp"][lo:hi] = before["xp"][lo:hi]
    assert any(t.startswith("xp:") for t in run(case))
    # an idle candidate's d touched
    case = _first(rec, lambda st, cmd, b: cmd[b]["flags"] == 0); before, cmd, f, after, b = case
    lo, hi = span(before, b)
    after["d"][hi - 1] = np.nextafter(after["d"][hi - 1], np.inf)
    assert any(t.startswith("d:") for t in run(case))
    # pflags short by one piece
    case = _first(rec, lambda st, cmd, b: cmd[b]["flags"] != 0 and st["pflags"][st["poff"][b + 1] - 1] != cmd[b]["flags"] and st["poff"][b + 1] - st["poff"][b] > 64)
    before, cmd, f, after, b = case
    after["pflags"][before["poff"][b + 1] - 1] = before["pflags"][before["poff"][b + 1] - 1]
    assert any(t.startswith("pflags:") for t in run(case))
    # and what the comparator does not look at bit for bit is still held: a direction off by 1e-8, a trial point off by an ulp too many, a stale result overwritten
    case = _first(rec, adv(bound_min=2)); before, cmd, f, after, b = case
    lo, hi = span(before, b)
    after["d"][lo:hi] *= 1.0 + 1e-8
    assert any("direction" in t for t in run(case))
    case = _first(rec, lambda st, cmd, b: cmd[b]["flags"] == 1 | 8); before, cmd, f, after, b = case
    lo, hi = span(before, b)
    after["x"][lo] += 4.0 * np.spacing(abs(after["x"][lo]) + abs(0.37 * after["d"][lo]))
    assert any("trial point" in t for t in run(case))
    after = dvs.copy_state(case[3]); after["res"]["dginit"][b] = 0.0
    assert any(t.startswith("res:") for t in ref.compare(before, cmd, f, after))


SPECS = {"headline": dvs.HEADLINE, "ragged": dvs.RAGGED}


@pytest.mark.parametrize("name", list(SPECS))
def test_harvested_sequences_are_coherent_and_the_model_reproduces_the_solver(frx, name):
    """The harvested (x_k, g_k) are the solver's own: the objective at them equals its trace bit for bit; and the model driven by ADVANCE + TRIAL at the solver's
    steps reproduces the next accepted point to 1e-9 all the way (which also says that `step` and the accepted points belong together)."""
    spec = SPECS[name]
    seqs = dvs.harvested(spec)
    for s in seqs:
        K = len(s["step"])
        assert K >= 2 * spec["m"] + 3 and (name != "headline" or K >= 2 * 128 + 40), K
        assert np.array_equal(s["f"][1:], s["f_solver"])                # bit for bit
        assert s["index"][-1] < len(s["evaluated"])
    assert [s["n"] for s in seqs] == {"headline": [633], "ragged": [839, 139, 9]}[name]
    ns = [s["n"] for s in seqs]
    geom, hs = frx.dv_layout(max(ns))
    assert spec["m"] <= geom[2] or name == "headline"
    st = dvs.new_state(frx, ns, spec["m"], geom, hs, np.random.default_rng(1))
    bad = dvs.drive(st, dvs.harvested_rounds(frx, st, seqs), lambda s, c, f: ref.apply(s, c, f), after_round=dvs.next_point_check(seqs))
    assert not bad, "\n".join(bad[:5])


@pytest.mark.parametrize("name", list(SPECS))
def test_reference_error_of_a_plain_double_recursion(name):
    """What the device's margin on the harvested sequences is taken from (16 times this): a double two-loop recursion in two summation orders against long double."""
    spec = SPECS[name]
    for c in spec["cands"]:
        worst, a, b = dvs.reference_error(*c, spec["kappa"], spec["m"], spec["iterations"])
        print(f"{name} candidate {c}: double recursion vs long double, worst over the sequence {worst:.3e} (numpy order {a:.3e}, 64 strided partial sums {b:.3e})")
        assert 0.0 < worst < 1e-9 / 16                                   # (otherwise the margin would be no sharper than the project's 1e-9)


def test_round_entry_refuses_what_would_leave_the_arrays(frx):
    """frx_debug_dv_round checks, before it touches a device, everything a launch would index with: a row stride that is neither the tight nor the full row of
    the batch, arrays shorter than the batch needs, an ADVANCE whose slot or bound lies outside the history, an empty candidate, poff beyond pflags."""
    ns, (geom, hs) = dvs.BATCHES["one_slab"]
    m = 3

    def refused(change, pattern):
        st = dvs.new_state(frx, ns, m, geom, hs, np.random.default_rng(0))
        cmd = np.zeros(len(ns), frx.DV_COMMAND)
        change(st, cmd)
        with pytest.raises(frx.FrxError, match=pattern) as e:
            frx.dv_round(st, cmd)
        assert e.value.code in (-1, -5)

    refused(lambda st, cmd: st.update(hs=hs - 16), "neither the tight nor the full row")
    refused(lambda st, cmd: st.update(hs=hs + 16), "neither the tight nor the full row")
    refused(lambda st, cmd: st.update(S=st["S"][:len(ns) * m * hs - 1].copy(), Y=st["Y"][:len(ns) * m * hs - 1].copy()), "shorter than the batch needs")
    refused(lambda st, cmd: [st.update({k: st[k][:st["xoff"][-1] - 1].copy()}) for k in ref.VEC], "shorter than the batch needs")
    refused(lambda st, cmd: st.update(gt=st["gt"][:4 * len(ns) * m - 1].copy()), "shorter than the batch needs")
    refused(lambda st, cmd: st.update(res=st["res"][:len(ns) - 1].copy()), "shorter than the batch needs")

    def bad_slot(st, cmd):
        cmd[1]["flags"] = DV_ADVANCE; cmd[1]["slot"] = m; cmd[1]["bound"] = 1
    refused(bad_slot, "slot or bound outside")

    def bad_bound(st, cmd):
        cmd[2]["flags"] = DV_ADVANCE; cmd[2]["slot"] = 0; cmd[2]["bound"] = m + 1
    refused(bad_bound, "slot or bound outside")

    def empty(st, cmd):
        st["xoff"][2] = st["xoff"][1]
    refused(empty, "at least one variable")
    refused(lambda st, cmd: st.update(pflags=st["pflags"][:st["poff"][-1] - 1].copy()), "pflags shorter")
    refused(lambda st, cmd: st.update(geom=(8, 1, 4, 4)), "too long for the geometry")
    refused(lambda st, cmd: st.update(m=513), "bad dv round argument")
    refused(lambda st, cmd: st.update(geom=(2, 5, 32, 4)), "no such k_lbfgs_pre geometry")
    refused(lambda st, cmd: st.update(geom=(2, 5, 16, 8)), "no such k_lbfgs_pre geometry")
