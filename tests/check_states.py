"""Edge states of the dense feasibility check (frx_trajectory_check, frx_check_kernel.hpp) - test infrastructure, not a test module.

The launcher's geometry rule (frx_device_check.hip: check_geometry), restated here as geometry(M, Kmax):

  lpp  lanes per piece: the smallest power of two >= M + 1, clamped to 2 .. 64;
       then doubled while ppw (19 + 4 (Kmax + 1)) > 2048 doubles of LDS per wave, ppw = 64 / lpp pieces per wave;
  refused when even ppw = 1 does not fit: Kmax <= 506 fits (2047 doubles), 507 does not (2051).

A workgroup is four waves, so 4 ppw pieces.  Every State names the (lpp, ppw) class it is built for and asserts, with geometry(), that it
still hits it; the builders assert with check_reference that a state has the property it exists for, so that a state that has drifted
fails here and not silently in a GPU test.

  packing states   random quintics over random durations, candidates of 1 .. 9 pieces, every piece's polytope of another K than its
                   neighbour's; per lpp class P = 1, ppw - 1, ppw + 1, 4 ppw - 1, 4 ppw + 1 pieces (a partial first wave, a second wave of one
                   piece followed by waves of none, a second workgroup) and M that fills the group, leaves it short, or (lpp = 64) strides.
                   K is drawn from 1 .. min(40, k_cap(lpp)): more half-spaces than k_cap(lpp) would let the LDS rule raise lpp, and the
                   classes lpp = 2 and 4 would never be reached from M (k_cap = 10 and 26).
  LDS states       the same quintics with one polytope padded to Kmax by redundant half-spaces (penalty_states._redundant): the LDS rule,
                   not M, sets lpp.  Every threshold of the rule: Kmax = 11 | 26, 27 | 58, 59 | 122, 123 | 250, 251 | 506.
  tie states       dyadic pieces in a box that lists its nearest face twice, bit for bit (k = 1 and k = 4), with grav_acc = 8,
                   vert_half_len = 1/8 and safe_margin = 1/16: zB = e3 and every corridor value exact in any arithmetic.
  flag states      one (T, Cf) and limit overrides derived from its reference candidate rows: no bit, each bit alone, all five, and the two
                   sides of equality for every comparison.
"""
import os
import sys
from dataclasses import dataclass, field

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_reference as cr  # noqa: E402
from penalty_states import _redundant  # noqa: E402

WAVE_LDS_CAP = 2048                                # doubles of LDS per wave
WAVES = 4                                          # waves per workgroup
LOOSE = dict(vel_max=1e4, thr_acc_min=0.0, thr_acc_max=1e4, body_rate_max=1e4)
EXACT = dict(grav_acc=8.0, vert_half_len=0.125, horiz_half_len=0.5, safe_margin=0.0625)
TIE_M = (1, 7, 63, 200)


def wave_lds(ppw, Kmax):
    return ppw * (19 + 4 * (Kmax + 1))


def geometry(M, Kmax):
    """(lpp, ppw) of a check at M intervals on a handle whose largest polytope has Kmax half-spaces; None = the launch is refused."""
    lpp = 2
    while lpp < M + 1 and lpp < 64:
        lpp *= 2
    while lpp < 64 and wave_lds(64 // lpp, Kmax) > WAVE_LDS_CAP:
        lpp *= 2
    if wave_lds(64 // lpp, Kmax) > WAVE_LDS_CAP:
        return None
    return lpp, 64 // lpp


def k_cap(lpp):
    """The largest Kmax at which the LDS rule leaves 64 / lpp pieces in a wave."""
    return (WAVE_LDS_CAP // (64 // lpp) - 19) // 4 - 1


@dataclass
class State:
    name: str
    counts: list                               # pieces per candidate
    piece_poly: list                           # index into polys per piece
    polys: list                                # 6 x K H-polytopes, column = (outer normal, point)
    override: dict                             # parameter overrides of the handle
    T: np.ndarray                              # (P,)
    Cf: np.ndarray                             # (6P, 3), row = power
    Ms: tuple                                  # interval counts the state is meant for
    lpp: int = 0                               # the class it hits at every M of Ms (0: not a geometry state)
    expect: dict = field(default_factory=dict)

    @property
    def P(self):
        return int(sum(self.counts))

    @property
    def piece_off(self):
        return np.concatenate([[0], np.cumsum(self.counts)]).astype(int)

    @property
    def piece_polys(self):
        return [self.polys[i] for i in self.piece_poly]

    @property
    def Kmax(self):
        return max(h.shape[1] for h in self.piece_polys)

    def params(self, base):
        p = dict(base)
        p.update(self.override)
        return p

    def reference(self, base, M):
        """(piece rows, candidate rows, flags) of the numpy restatement."""
        p = self.params(base)
        rows = cr.check_pieces(self.T, self.Cf, self.piece_polys, p, M)
        cand = cr.reduce_candidates(rows, self.T, self.piece_off)
        return rows, cand, cr.flags_of(cand, p)


# ---- packing ----
M_OF = {2: (1,), 4: (3, 2), 8: (7, 5), 16: (15, 11), 32: (31, 20), 64: (63, 40, 65, 127, 129)}    # fills the group, short of it, strides
K_POOL = (1, 2, 3, 5, 6, 7, 9, 11, 12, 14, 17, 19, 22, 26, 31, 36, 39)


def packing_counts(ppw):
    return sorted({1, ppw - 1, ppw + 1, 4 * ppw - 1, 4 * ppw + 1} - {0})


def _random_poly(rng, K):
    """K half-spaces in general position: normals of any length (the library normalises), points anywhere on their planes."""
    n = rng.normal(size=(3, K))
    n /= np.linalg.norm(n, axis=0)
    p = n * rng.uniform(0.5, 5.0, K) + np.cross(n.T, rng.normal(size=(K, 3))).T
    return np.concatenate([n * rng.uniform(0.5, 2.0, K), p], axis=0)


def _quintics(rng, P):
    """Random quintics over random durations: the distributions of test_gpu_trajectory_sample.test_ragged_batch."""
    return rng.uniform(0.05, 0.4, P), rng.normal(0.0, 2.0, (6 * P, 3))


def _split(rng, P):
    """Candidates of 1 .. 9 pieces that sum to P."""
    counts = []
    while sum(counts) < P:
        counts.append(int(min(rng.integers(1, 10), P - sum(counts))))
    return counts


def _neighbours_differ(rng, P, n_polys, first):
    idx = [first]
    while len(idx) < P:
        i = int(rng.integers(0, n_polys))
        if i != idx[-1]:
            idx.append(i)
    return idx


def _assert_class(st):
    ppw = 64 // st.lpp
    for M in st.Ms:
        assert geometry(M, st.Kmax) == (st.lpp, ppw), f"{st.name}: M = {M}, Kmax = {st.Kmax} gives {geometry(M, st.Kmax)}, not lpp = {st.lpp}"
    assert all(1 <= c <= 9 for c in st.counts) and len(st.T) == st.P and st.Cf.shape == (6 * st.P, 3)
    K = [h.shape[1] for h in st.piece_polys]
    assert all(K[i] != K[i + 1] for i in range(st.P - 1)), f"{st.name}: two neighbouring pieces have the same K"
    if ppw > 1 and st.P > 9:
        assert any(o % ppw for o in st.piece_off[1:-1]), f"{st.name}: no candidate boundary inside a wave"


def packing_state(lpp, P, seed=0):
    """P pieces whose lpp comes from M alone (every M of M_OF[lpp])."""
    rng = np.random.default_rng(1000 * lpp + 10 * P + seed)
    Ks = [k for k in K_POOL if k < min(40, k_cap(lpp))] + [min(40, k_cap(lpp))]
    polys = [_random_poly(rng, K) for K in Ks]
    T, Cf = _quintics(rng, P)
    st = State(f"M-lpp{lpp}-ppw{64 // lpp}-P{P}", _split(rng, P), _neighbours_differ(rng, P, len(polys), len(polys) - 1), polys, dict(LOOSE), T, Cf,
               M_OF[lpp], lpp)
    _assert_class(st)
    for M in st.Ms:
        assert geometry(M, 1)[0] == lpp                                   # M alone asks for this class
    return st


def packing_cases():
    """(lpp, P) of every packing state."""
    return [(lpp, P) for lpp in (2, 4, 8, 16, 32, 64) for P in packing_counts(64 // lpp)]


# ---- LDS-forced packing ----
LDS_CASES = ((11, (1,)), (26, (1,)), (27, (1,)), (40, (1, 3)), (58, (1,)), (59, (1,)), (122, (1,)), (123, (1,)), (250, (1,)), (251, (1,)), (260, (1,)),
             (506, (1, 64)))
BOX_HALF = 3.0


def _box(half, centre=(0.0, 0.0, 0.0)):
    """x, y, z <= centre + half and >= centre - half as columns (outer normal, point)."""
    c = np.asarray(centre, dtype=np.float64)
    return np.concatenate([np.vstack([np.eye(3), np.diag(c + half)]), np.vstack([-np.eye(3), np.diag(c - half)])], axis=1)


def padded_box(rng, K):
    """The box |x|, |y|, |z| <= BOX_HALF with K - 6 redundant half-spaces behind it: K half-spaces, the same feasible set."""
    assert K >= 6
    box = _box(BOX_HALF)
    if K == 6:
        return box
    verts = BOX_HALF * np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64).T
    red = _redundant(rng, verts, K - 6)
    assert (np.einsum("ik,ikv->kv", red[:3], verts[:, None, :] - red[3:, :, None]) < -1.0).all()      # every vertex well inside every added face
    return np.concatenate([box, red], axis=1)


def lds_state(Kmax, Ms, seed=0):
    """4 ppw + 1 pieces, one polytope of Kmax half-spaces among small ones: lpp is what the LDS rule leaves."""
    geo = geometry(Ms[0], Kmax)
    assert geo is not None
    lpp, ppw = geo
    rng = np.random.default_rng(77000 + 10 * Kmax + seed)
    P = 4 * ppw + 1
    polys = [_random_poly(rng, K) for K in (1, 5, 7, 10) if K < Kmax] + [padded_box(rng, Kmax)]
    idx = _neighbours_differ(rng, P, len(polys) - 1, 0)
    idx[1] = idx[-1] = len(polys) - 1                                      # the large block inside the first wave and alone in the last
    T, Cf = _quintics(rng, P)
    st = State(f"LDS-Kmax{Kmax}-lpp{lpp}-ppw{ppw}", _split(rng, P), idx, polys, dict(LOOSE), T, Cf, tuple(Ms), lpp)
    assert st.Kmax == Kmax
    _assert_class(st)
    forced = [M for M in Ms if geometry(M, 1)[0] < lpp]
    assert Ms[0] in forced, f"{st.name}: M = {Ms[0]} reaches lpp = {lpp} on its own"
    return st


# ---- ties ----
def tie_box(z_face=1.25):
    """|x|, |y| <= 4, -4 <= z <= z_face, the face z <= z_face listed at k = 1 and again, bit for bit, at k = 4."""
    cols = [((1.0, 0, 0), (4.0, 0, 0)), ((0, 0, 1.0), (0, 0, z_face)), ((0, 1.0, 0), (0, 4.0, 0)), ((-1.0, 0, 0), (-4.0, 0, 0)),
            ((0, 0, 1.0), (0, 0, z_face)), ((0, -1.0, 0), (0, -4.0, 0)), ((0, 0, -1.0), (0, 0, -4.0))]
    h = np.array([np.concatenate([n, p]) for n, p in cols], dtype=np.float64).T
    assert h[:, 1].tobytes() == h[:, 4].tobytes()
    return h


def _const_piece(pos, vel=(0.0, 0.0, 0.0)):
    c = np.zeros((6, 3))
    c[0] = pos
    c[1] = vel
    return c


def _assert_tie(st, base, piece=0, value=-0.125):
    """Columns k = 1 and k = 4 of the reference's sample matrix: equal bits, constant along j, above every other column at every sample."""
    ell, g = cr.params_of(st.params(base))
    for M in st.Ms:
        v = cr.piece_samples(st.Cf[6 * piece:6 * piece + 6], float(st.T[piece]), M, st.piece_polys[piece], ell, g)["corridor"]
        assert (v[:, 1] == value).all() and (v[:, 4] == value).all(), (st.name, M, v[:, [1, 4]])
        others = np.delete(v, [1, 4], axis=1)
        assert (others < value).all(), (st.name, M, others.max())
        row = cr.piece_row(st.Cf[6 * piece:6 * piece + 6], float(st.T[piece]), M, st.piece_polys[piece], ell, g)
        assert row[0] == value and row[6] == 0.0 and row[7] == 1.0


def tie_state(moving, base):
    """One piece at z = 1 under the duplicated face z <= 1.25: reach 1 - 1.25 + 1/8 = -1/8 on both copies at every sample.  moving: a straight
    constant-velocity line parallel to that face; the side faces stay below -1/8 (x <= 0.75: 0.75 - 4 + 0.5)."""
    c = _const_piece((0.25, 0.5, 1.0), (0.5, 0.25, 0.0) if moving else (0.0, 0.0, 0.0))
    st = State("tie-line" if moving else "tie-point", [1], [0], [tie_box()], dict(LOOSE, **EXACT), np.array([1.0]), c, TIE_M)
    _assert_tie(st, base)
    st.expect = dict(value=-0.125, worst_t=0.0, worst_k=1.0)
    return st


def _two_candidates(special, other_z=0.5):
    """Candidate 0: eight constant pieces at z = other_z but for `special` {local index: (6, 3) coefficients}; candidate 1: three more."""
    T = np.array([0.5, 0.25, 1.0, 0.5, 2.0, 1.0, 0.25, 0.5, 1.0, 0.5, 0.25])
    C = [special.get(i, _const_piece((0.125 * i, -0.25 * i, other_z))) for i in range(8)] + [_const_piece((1.0, 1.0, 0.25 * i)) for i in range(3)]
    return [8, 3], T, np.concatenate(C)


def duplicate_piece_state(base):
    """Pieces 2 and 5 of candidate 0 are bit-identical copies of the tie piece and the worst of it: the candidate row names piece 2."""
    tie = _const_piece((0.25, 0.5, 1.0))
    counts, T, Cf = _two_candidates({2: tie, 5: tie.copy()})
    st = State("tie-pieces", counts, [0] * 11, [tie_box()], dict(LOOSE, **EXACT), T, Cf, TIE_M)
    assert Cf[12:18].tobytes() == Cf[30:36].tobytes()
    _assert_tie(st, base, piece=2)
    _assert_tie(st, base, piece=5)
    for M in st.Ms:
        rows, cand, flags = st.reference(base, M)
        assert rows[2, 0] == rows[5, 0] == -0.125 and (np.delete(rows[:8, 0], [2, 5]) < -0.125).all()
        assert cand[0, 0] == -0.125 and cand[0, 7] == 2.0 and cand[0, 6] == 0.75 and not flags.any()
    st.expect = dict(candidate=0, value=-0.125, worst_k=2.0, worst_t=0.75)                # 0.5 + 0.25 + local time 0
    return st


def nan_order_state(base):
    """One NaN coefficient (c5.x: every derivative of every sample carries it) in pieces 3 and 6 of candidate 0."""
    bad = _const_piece((0.25, 0.5, 1.0))
    bad[5, 0] = np.nan
    counts, T, Cf = _two_candidates({3: bad, 6: bad.copy()})
    st = State("nan-pieces", counts, [0] * 11, [tie_box()], dict(LOOSE, **EXACT), T, Cf, TIE_M)
    for M in st.Ms:
        rows, cand, flags = st.reference(base, M)
        for q in (3, 6):
            assert np.isnan(rows[q, :6]).all() and rows[q, 6] == 0.0 and rows[q, 7] == 0.0
        assert np.isfinite(np.delete(rows, [3, 6], axis=0)).all()
        assert np.isnan(cand[0, :6]).all() and cand[0, 7] == 3.0 and cand[0, 6] == 1.75 and flags[0] == 32      # 0.5 + 0.25 + 1.0
        assert np.isfinite(cand[1]).all() and flags[1] == 0
    st.expect = dict(candidate=0, nan_pieces=(3, 6), worst_k=3.0, worst_t=1.75, flags=(32, 0))
    return st


# ---- flags ----
FLAG_M = 37
LIMIT_BIT = (("vel_max", 1, 2, -1), ("thr_acc_min", 2, 4, +1), ("thr_acc_max", 3, 8, -1), ("body_rate_max", 4, 16, -1))   # name, field, bit, violating side
WIDE, NARROW = 1e3, 0.01                                                  # half-sizes of the box nothing reaches / everything leaves


def flag_base_state():
    rng = np.random.default_rng(5)
    counts = [3, 4]
    T, Cf = _quintics(rng, 7)
    return State("flags-none", counts, [0] * 7, [_box(WIDE)], dict(LOOSE), T, Cf, (FLAG_M,))


def flag_states(base):
    """{name: State}: 'none', one state per bit alone, 'all'.  Limits at half (twice, for the thrust minimum) the value of the candidate
    that is nearest to them in the reference's rows, so that every candidate violates; the box of half-size NARROW is left by every candidate."""
    st0 = flag_base_state()
    _, cand, flags = st0.reference(base, FLAG_M)
    assert not flags.any() and (cand[:, 0] < -1.0).all()
    st0.expect = dict(flags=(0, 0))
    tight = dict(vel_max=0.5 * cand[:, 1].min(), thr_acc_min=2.0 * cand[:, 2].max(), thr_acc_max=0.5 * cand[:, 3].min(),
                 body_rate_max=0.5 * cand[:, 4].min())
    out = {"none": st0}
    for name, _, bit, _ in LIMIT_BIT:
        over = dict(LOOSE)
        over[name] = float(tight[name])
        out[name] = State(f"flags-{name}", st0.counts, st0.piece_poly, st0.polys, over, st0.T, st0.Cf, st0.Ms, expect=dict(flags=(bit, bit)))
    out["corridor"] = State("flags-corridor", st0.counts, st0.piece_poly, [_box(NARROW)], dict(LOOSE), st0.T, st0.Cf, st0.Ms, expect=dict(flags=(1, 1)))
    out["all"] = State("flags-all", st0.counts, st0.piece_poly, [_box(NARROW)], {k: float(v) for k, v in tight.items()}, st0.T, st0.Cf, st0.Ms,
                       expect=dict(flags=(31, 31)))
    for st in out.values():
        assert tuple(st.reference(base, FLAG_M)[2]) == st.expect["flags"], (st.name, st.reference(base, FLAG_M)[2])
    return out


def strict_states(cand_row):
    """For each limit: (State with the limit EQUAL to cand_row's value - the bit stays clear, State with np.nextafter of it on the violating
    side - the bit is set), for candidate 0 of the flag state.  cand_row: candidate 0's row as the implementation under test reports it
    (the comparison is on its own value: an implementation that differs from another in the last bit is still strict or not)."""
    st0 = flag_base_state()
    out = []
    for name, f, bit, side in LIMIT_BIT:
        v = float(cand_row[f])
        pair = []
        for lim, fires in ((v, False), (float(np.nextafter(v, side * np.inf)), True)):
            over = dict(LOOSE)
            over[name] = lim
            pair.append(State(f"strict-{name}-{'past' if fires else 'equal'}", st0.counts, st0.piece_poly, st0.polys, over, st0.T, st0.Cf, st0.Ms,
                              expect=dict(bit=bit, fires=fires)))
        out.append(tuple(pair))
    return out


def corridor_zero_states(base):
    """The tie-point piece (z = 1, zB = e3, vertical half-length 1/8) with the duplicated face through the ellipsoid's top, z <= 1.125: the
    reach is 1 - 1.125 + 0.125 = 0.0 exactly (every operand dyadic, the margin 1/16 subtracted at create and added back in the kernel
    exactly): bit 1 stays clear.  With the face one ulp lower the reach is 2^-52 and the bit is set."""
    out = []
    for z_face, reach in ((1.125, 0.0), (float(np.nextafter(1.125, -np.inf)), 2.0 ** -52)):
        st = State(f"strict-corridor-{'past' if reach else 'equal'}", [1], [0], [tie_box(z_face)], dict(LOOSE, **EXACT), np.array([1.0]),
                   _const_piece((0.25, 0.5, 1.0)), TIE_M, expect=dict(bit=1, fires=reach > 0.0, value=reach, worst_k=1.0, worst_t=0.0))
        _assert_tie(st, base, value=reach)
        for M in st.Ms:
            _, cand, flags = st.reference(base, M)
            assert cand[0, 0] == reach and flags[0] == (1 if reach else 0)
        out.append(st)
    return tuple(out)
