"""k_lbfgs_pre and k_lbfgs_post command by command against the long-double model (dv_reference): one launch per round through frx.dv_round on state the test
owns, the returned state handed back in, and after every round every buffer of every candidate held bit for bit, by a derived bound or by tolerance (the rules
are in dv_reference's text; the states and sequences in dv_states)."""
import numpy as np
import pytest

import dv_states as dvs

pytestmark = pytest.mark.gpu


def _device(frx):
    def execute(st, cmd, f):
        try:
            frx.dv_round(st, cmd, f)
        except frx.FrxError as e:
            if e.code in (-3, -6):                                      # FRX_ERR_HIP, FRX_ERR_ALLOC: a launch the device refused or lost - nothing more is started on it
                pytest.exit(f"frx_debug_dv_round failed on the device, the session ends here: {e}", returncode=3)
            raise                                                       # (refused before the device was touched: this test's own failure)
    return execute


def _worst(stats, B):
    w = [0.0] * B
    for b, e in stats.get("d_err", []):
        w[b] = max(w[b], e)
    return w


@pytest.mark.parametrize("name,mi", [(name, mi) for name in dvs.BATCHES for mi in range(5)])
def test_synthetic_ragged_batches_command_by_command(frx, name, mi):
    """Ragged batches under the geometry of their longest vector, candidates at different steps inside one launch, idle / EVAL-only / TRIAL-only / RESTORE
    neighbours, m in {1, 3, PF-1, PF, PF+1}, 2 m + 3 advances (every slot overwritten twice), data scaled over twelve decades from candidate to candidate."""
    ns, (geom, hs) = dvs.BATCHES[name]
    assert frx.dv_layout(max(ns)) == (geom, hs)
    m = dvs.memories(geom[2])[mi]
    rng = np.random.default_rng(1000 * mi + len(name))
    st = dvs.new_state(frx, ns, m, geom, hs, rng)
    stats = {}
    bad = dvs.drive(st, dvs.synthetic_rounds(frx, st, rng, 2 * m + 3), _device(frx), d_tol=1e-9, stats=stats)
    print(f"{name} m={m} geometry {geom} hs={hs}: worst direction error per candidate {['%.2e' % e for e in _worst(stats, len(ns))]}")
    assert not bad, "\n".join(bad[:8])
    assert len(stats["d_err"]) == len(ns) * (2 * m + 3)


# m over {1, 3, PF-1, PF, PF+1} on tight rows as for the main batches (m = 1, 3: fewer pairs than the look-ahead, every other visit a pad; PF-1, PF: V1 just above
# and at bound), and the full row 64 W E once per geometry
@pytest.mark.parametrize("name,mi,tight", [(name, mi, True) for name in dvs.EXPERIMENTAL for mi in range(5)] + [(name, 4, False) for name in dvs.EXPERIMENTAL])
def test_experimental_geometries_command_by_command(frx, name, mi, tight):
    """The geometries the launcher instantiates beside the library's choice (one and two pairs per reduction) on one short batch."""
    geom = dvs.EXPERIMENTAL[name]
    ns = dvs.EXPERIMENTAL_NS
    g2, hs = frx.dv_layout(max(ns), geom, tight=tight)
    assert g2 == geom and hs == (656 if tight else 768)
    m = dvs.memories(geom[2])[mi]
    rng = np.random.default_rng(hs + 10 * geom[3] + mi)
    st = dvs.new_state(frx, ns, m, geom, hs, rng)
    stats = {}
    bad = dvs.drive(st, dvs.synthetic_rounds(frx, st, rng, 2 * m + 3), _device(frx), d_tol=1e-9, stats=stats)
    print(f"{name} {geom} hs={hs} m={m}: worst direction error per candidate {['%.2e' % e for e in _worst(stats, len(ns))]}")
    assert not bad, "\n".join(bad[:8])
    assert len(stats["d_err"]) == len(ns) * (2 * m + 3)


# the blocked recursion (BLK = 4: the library's choice) and, where a geometry with one pair per reduction holds the vectors, the sequential one beside it: should the
# blocked form ever miss the margin, the second row says whether the rearranged algebra or a defect did it
@pytest.mark.parametrize("name,geom", [("headline", None), ("headline", (4, 3, 8, 1)), ("ragged", None)])
def test_harvested_histories_command_by_command(frx, name, geom):
    """Real (x_k, g_k) sequences of the CPU oracle's L-BFGS replayed open loop: the same exact and derived checks, the direction against the long-double
    recursion within 16 times what a plain double recursion loses on these very states (dv_states.reference_error, measured here in two summation orders; the
    factor covers the blocked form's rearranged algebra, whose rounding nobody has analysed), and every trial point within 1e-9 of the oracle's next accepted
    point.  Measured on an MI355X (worst over the sequence, device / margin): see DESIGN.md, "Device-vector commands, pinned"."""
    spec = {"headline": dvs.HEADLINE, "ragged": dvs.RAGGED}[name]
    seqs = dvs.harvested(spec)
    ns = [s["n"] for s in seqs]
    geom, hs = frx.dv_layout(max(ns), geom)
    margin = [16.0 * dvs.reference_error(*c, spec["kappa"], spec["m"], spec["iterations"])[0] for c in spec["cands"]]
    st = dvs.new_state(frx, ns, spec["m"], geom, hs, np.random.default_rng(2))
    stats = {}
    bad = dvs.drive(st, dvs.harvested_rounds(frx, st, seqs), _device(frx), d_tol=margin, stats=stats, after_round=dvs.next_point_check(seqs, 1e-9))
    worst = _worst(stats, len(ns))
    print(f"{name} {geom} hs={hs} m={spec['m']}, {[len(s['step']) for s in seqs]} accepted steps: device direction error {['%.3e' % e for e in worst]}, "
          f"margin (16 x double recursion) {['%.3e' % e for e in margin]}")
    assert not bad, "\n".join(bad[:8])
    assert len(stats["d_err"]) == sum(len(s["step"]) for s in seqs)
