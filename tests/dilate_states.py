"""States of the corridor cell kernel (dilate_cell in frx_corridor_kernels.hpp, behind frx_dilate_batch and frx_corridor_generate_batch) at its compaction,
order and capacity edges - test infrastructure, not a test module.

  size_state(n)      one segment, n cloud points, n in 1, 2, 255, 256, 257, 511, 512, 513, 1025: the points alternate in cloud order between the local box and
                     far outside it (so the prefix offsets of the compaction are not the chunk starts), point 0 is in the box (thread 0's count matters) and
                     the LAST point is the closest to the segment: it is a contact point of the cell, so a kernel that loses it gives another cell.
  count_state(M)     M candidates in the box: 0 (300 points, all outside: six box planes), 1, 255, 256, 257 - the 256-lane stride of the scans - and
                     4095, 4096, 4097 around the kernel's candidate buffer: some thirty points near the segment, the rest on a thin ray that starts outside the
                     initial sphere and leads away from it (the tangent plane at its first point cuts nearly all the others: at most 90 tangent planes, checked
                     with the host form), padded with outside points to 4200.
  order_state(k)     seeded clouds of 40, 200 and 1000 points around a generic segment, a vertical segment (the degenerate branch of the box) and a segment
                     with a zero box (every cloud point is a candidate); at least 8 tangent planes each.
  four_contacts(sw)  segment (-1,0,0)-(1,0,0), offset 0: R = I and the initial shape is the unit sphere.  (0,+-1/2,0) and (0,0,+-1/2) are at distance 1/2 then,
                     1 in every later shape, exactly, whatever is fused (all products are by 0, 1, 2 or 1/2) - PROVIDED (0,+1/2,0) stands first in the cloud:
                     the roll towards it is atan2(0, 1/2) = 0, while a roll of pi/2 or pi has an inexact cosine or sine.  It stands first in both orders; sw
                     swaps (0,-1/2,0) and (0,0,-1/2).  Compacted positions 37, 38, 102, 358: lanes 37 and 38 of wave 0 (the shuffle fold), lane 38 of wave 1
                     (the fold over red[]), and 358 = 102 + 256, the same lane one stride later (the lane loop).  The filler is farther than 0.6 from the axis.
                     An ellipsoid-stage tie is NOT built on purpose: two candidates tied as closest force a circular section, so either winner gives the same
                     ellipsoid (here: which of (0,0,+-1/2) fixes the third axis).  Only the tangent planes' order shows who won.
  duplicate_pair()   the 1000-point order cloud with one contact point moved to the front, and the same cloud with a bit-for-bit copy of that point appended
                     (more than 256 candidates later): the copy lies ON the first copy's plane, n.(q - c) = 0 exactly, and leaves with it.
  plane_caps()       cap_planes = K and K - 1 for a cell with a box (the `np + 6 > cap_planes` branch) and one with a zero box (`np >= cap_planes`).
  batch()            5 segments in one cloud, segment 2 the M = 4097 state, its neighbours cells 100 m apart.
  chain_worlds()     2-point paths over the M = 4096 / 4097 clouds with a far neighbour path.

Every state handed out is decision-safe, by the restatement (dilate_reference.py) in float64 AND in longdouble with the same order of contact points:
  box_margin >= 1e-6; every arg-min gap >= 1e-6 except inside a DECLARED group - an intended exact tie (gap exactly 0.0; tie_ok) or the contact group of the
  final ellipsoid: the `group` candidates at distance 1 +- 1e-9 in the final metric (the points that fixed its axes), which the polyhedron loop takes first and
  whose order among themselves the headers leave to rounding; the in / out decisions of the ellipsoid loops and the cuts of the polyhedron loop keep 1e-6 too
  (shell_margin, cut_margin; the four-contact states are exempt from the first: their arithmetic is exact).  The seeds below were chosen on the CPU so that
  this holds; a seed that fails is replaced, not tolerated.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dilate_reference as dr  # noqa: E402

BBOX = np.array([4.0, 4.0, 2.5])
SAFE = 1e-6
PCAP = 4096                                                       # candidate points of a cell (frx_batch.cpp, frx_device.hpp: CHAIN_PCAP)
SIZES = [1, 2, 255, 256, 257, 511, 512, 513, 1025]
COUNTS = [0, 1, 255, 256, 257, 4095, 4096, 4097]
BIG_PLANES = 90                                                   # tangent planes of an M ~ 4096 state: cap_planes = 96 holds
TIE_AT = [37, 38, 102, 358]
MAP_HEIGHT, MAX_SEG = 3.0, 4.0

_cache = {}


def _frame(p1, p2):
    n, _ = dr.box_planes(p1, p2, BBOX)
    return n[2], n[0], n[4]                                       # along, sideways, upwards (u, h, v)


def _far(rng, p1, p2, n):
    """n points clearly outside the local box (12-20 m from the midpoint; the box's corners are nearer than 8)"""
    w = rng.normal(0, 1, (n, 3)); w /= np.linalg.norm(w, axis=1, keepdims=True)
    return 0.5 * (p1 + p2) + w * rng.uniform(12.0, 20.0, (n, 1))


def _seg_dist(q, p1, p2):
    t = np.clip((q - p1) @ (p2 - p1) / ((p2 - p1) @ (p2 - p1)), 0, 1)
    return np.linalg.norm(q - (p1 + t * (p2 - p1)))


def _boxed(rng, p1, p2, n, clear=0.7):
    """n points clearly inside the local box (0.5 / 0.5 / 0.3 m from its faces), none closer than `clear` to the segment"""
    u, h, v = _frame(p1, p2); L = np.linalg.norm(p2 - p1); out = []
    while len(out) < n:
        q = p1 + u * rng.uniform(-3.5, L + 3.5) + h * rng.uniform(-3.5, 3.5) + v * rng.uniform(-2.2, 2.2)
        if _seg_dist(q, p1, p2) > clear:
            out.append(q)
    return np.array(out).reshape(-1, 3)


def _scatter(rng, p1, p2, n, spread, clear=0.35):
    """n points scattered around the segment (in and out of the box as they fall), none closer than `clear` to it"""
    u = (p2 - p1) / np.linalg.norm(p2 - p1); L = np.linalg.norm(p2 - p1); out = []
    while len(out) < n:
        q = p1 + u * rng.uniform(-2.0, L + 2.0) + rng.normal(0, spread, 3)
        if _seg_dist(q, p1, p2) > clear:
            out.append(q)
    return np.array(out)


def _interleave(inside, outside):
    """cloud order: inside[0], outside[0], inside[1], outside[1], ... and what is left of the longer one"""
    out = []
    for k in range(max(len(inside), len(outside))):
        if k < len(inside): out.append(inside[k])
        if k < len(outside): out.append(outside[k])
    return np.array(out).reshape(-1, 3)


def make(name, p1, p2, bbox, obs, tie_ok=False, exact=False, want_M=None):
    """the state, self-checked: SimpleNamespace(name, p1, p2, bbox, obs, ref = the float64 restatement, M, group, tie_ok, K)"""
    p1, p2, bbox = np.asarray(p1, float), np.asarray(p2, float), np.asarray(bbox, float)
    obs = np.ascontiguousarray(np.asarray(obs, float).reshape(-1, 3))
    ref = dr.dilate_cell(p1, p2, bbox, obs)
    refl = dr.dilate_cell(p1, p2, bbox, obs, dtype=np.longdouble)
    M = len(ref.cand)
    assert want_M is None or M == want_M, (name, M, want_M)
    group = 0 if exact else int((np.abs(ref.dist_final - 1.0) <= 1e-9).sum())
    assert ref.box_margin >= SAFE and refl.box_margin >= SAFE, (name, ref.box_margin)
    assert np.array_equal(ref.cand, refl.cand), name
    # the same decisions in both precisions: the same contact points in the same order, the group as a set
    assert len(ref.order) == len(refl.order) and ref.order[group:] == refl.order[group:] and sorted(ref.order[:group]) == sorted(refl.order[:group]), name
    if group:                                                     # the group is what the polyhedron loop takes first, and nothing else is near the shell
        assert sorted(c for c, _ in ref.order[:group]) == np.flatnonzero(np.abs(ref.dist_final - 1.0) <= 1e-9).tolist(), name
    for r in (ref, refl):
        pick = 0
        for g, st in zip(r.gaps, r.gap_stage):
            in_group = st == "poly" and pick < group - 1
            pick += st == "poly"
            assert g >= SAFE or in_group or (tie_ok and g == 0.0), (name, st, pick, g)
        assert r.cut_margin >= SAFE, (name, "cut", r.cut_margin)
        assert exact or r.shell_margin >= SAFE, (name, "shell", r.shell_margin)
    return SimpleNamespace(name=name, p1=p1, p2=p2, bbox=bbox, obs=obs, ref=ref, M=M, group=group, tie_ok=tie_ok, K=ref.H.shape[1])


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


# ---- how a cell is compared with the restatement ---------------------------------------------------------------------------------------------------------------
def _canon(H):
    key = np.round(H / 1e-6).astype(np.int64)
    return H[:, np.lexsort(key[::-1])]


def plane_difference(H, st):
    """largest difference between the records H (6 x K) and the state's restatement IN EMISSION ORDER; the first st.group records - the declared contact group -
    are compared as a set"""
    Hr = st.ref.H
    assert H.shape == Hr.shape, (st.name, H.shape, Hr.shape)
    g = st.group
    worst = np.abs(_canon(H[:, :g]) - _canon(Hr[:, :g])).max() if g else 0.0
    return max(worst, np.abs(H[:, g:] - Hr[:, g:]).max()) if H.shape[1] > g else worst


def contact_indices(H, st):
    """cloud index of every tangent plane's contact point (the FIRST bit-equal cloud point), -1 when it is no cloud point"""
    n_tan = H.shape[1] - (6 if np.linalg.norm(st.bbox) != 0 else 0)
    out = []
    for k in range(n_tan):
        hit = np.flatnonzero((st.obs == H[3:, k][None]).all(axis=1))
        out.append(int(hit[0]) if len(hit) else -1)
    return out


def assert_order(H, st):
    got = contact_indices(H, st); want = [c for _, c in st.ref.order]
    g = st.group
    assert -1 not in got, (st.name, got)
    assert got[g:] == want[g:] and sorted(got[:g]) == sorted(want[:g]), (st.name, got, want)


# ---- cloud size ------------------------------------------------------------------------------------------------------------------------------------------------
SIZE_P1, SIZE_P2 = np.array([1.3, -0.7, 1.1]), np.array([3.6, 1.2, 1.5])
SIZE_SEED = {1: 0, 2: 0, 255: 0, 256: 0, 257: 0, 511: 0, 512: 0, 513: 0, 1025: 0}


def size_state(n):
    def build():
        rng = np.random.default_rng(1000 + 10 * n + SIZE_SEED[n])
        u, h, v = _frame(SIZE_P1, SIZE_P2)
        near = 0.5 * (SIZE_P1 + SIZE_P2) + 0.45 * (np.cos(0.7) * h + np.sin(0.7) * v)
        n_in = (n - 1 + 1) // 2                                    # even cloud indices below n - 1
        obs = _interleave(_boxed(rng, SIZE_P1, SIZE_P2, n_in), _far(rng, SIZE_P1, SIZE_P2, n - 1 - n_in))
        obs = np.vstack([obs, near[None]])
        st = make(f"size{n}", SIZE_P1, SIZE_P2, BBOX, obs)
        assert len(st.obs) == n and n - 1 in [c for _, c in st.ref.order[:st.group]]     # the last cloud point fixed an axis: a contact
        assert n == 1 or (0 in st.ref.cand and st.M == n_in + 1)
        return st
    return _cached(("size", n), build)


# ---- candidate count -------------------------------------------------------------------------------------------------------------------------------------------
COUNT_P1, COUNT_P2 = np.array([-2.0, 0.4, 1.4]), np.array([0.6, 1.9, 1.0])
COUNT_SEED = {0: 0, 1: 0, 255: 0, 256: 0, 257: 0}
BIG_SEED, BIG_NEAR, BIG_N = 0, 30, 4200


def _big_cloud(M):
    rng = np.random.default_rng(7000 + BIG_SEED)
    u, h, v = _frame(COUNT_P1, COUNT_P2)
    near = _boxed(rng, COUNT_P1, COUNT_P2, BIG_NEAR, clear=0.6)
    n_ray = PCAP + 1 - BIG_NEAR
    s = rng.uniform(0.0, 1.2, n_ray)
    ray = 0.5 * (COUNT_P1 + COUNT_P2) + h * (2.6 + s)[:, None] + u * rng.normal(0, 0.03, (n_ray, 1)) + v * rng.normal(0, 0.03, (n_ray, 1))
    inside = np.vstack([near, ray])[rng.permutation(PCAP + 1)][:M]     # 4095 and 4096 drop the last one or two of 4097's candidates
    far = _far(rng, COUNT_P1, COUNT_P2, BIG_N - M)
    # the outside points stand at regular distances in the cloud, the first at index 1
    step = M // len(far)
    out, k = [], 0
    for i, q in enumerate(inside):
        out.append(q)
        if i % step == 0 and k < len(far):
            out.append(far[k]); k += 1
    out += list(far[k:])
    return np.array(out)


def count_state(M):
    def build():
        if M >= PCAP - 1:
            obs = _big_cloud(M)
            assert len(obs) == BIG_N > PCAP + 1
            st = make(f"count{M}", COUNT_P1, COUNT_P2, BBOX, obs, want_M=M)
            assert st.K - 6 <= BIG_PLANES, (M, st.K)
            return st
        rng = np.random.default_rng(3000 + 10 * M + COUNT_SEED[M])
        n_out = 300 if M == 0 else M + 3
        return make(f"count{M}", COUNT_P1, COUNT_P2, BBOX, _interleave(_boxed(rng, COUNT_P1, COUNT_P2, M), _far(rng, COUNT_P1, COUNT_P2, n_out)), want_M=M)
    return _cached(("count", M), build)


def host_planes_within_cap(frx, st):
    """the host form's own count for an M ~ 4096 state (the condition under which cap_planes = 96 holds)"""
    H, _, _ = frx.line_segment_dilate(st.p1, st.p2, st.bbox, st.obs)
    return H.shape[1] - 6 <= BIG_PLANES and H.shape[1] == st.K


# ---- order -----------------------------------------------------------------------------------------------------------------------------------------------------
ORDER = [  # (seed, n_obs, spread, p1, p2, bbox)
    (4, 40, 1.0, [0.5, -1.0, 1.2], [2.9, 0.8, 1.7], BBOX),
    (0, 200, 2.0, [-3.0, 2.0, 0.6], [-3.0, 2.0, 2.9], BBOX),              # vertical
    (0, 1000, 3.0, [4.0, 4.5, 1.0], [1.5, 6.0, 1.6], np.zeros(3)),        # zero box: every cloud point is a candidate
]


def order_state(k, shift=None):
    def build():
        seed, n, spread, p1, p2, bbox = ORDER[k]
        p1, p2 = np.array(p1), np.array(p2)
        obs = _scatter(np.random.default_rng(5000 + 100 * k + seed), p1, p2, n, spread)
        if shift is not None:
            p1, p2, obs = p1 + shift, p2 + shift, obs + shift
        st = make(f"order{k}" + ("" if shift is None else "+shift"), p1, p2, bbox, obs)
        n_tan = st.K - (6 if np.linalg.norm(bbox) != 0 else 0)
        assert n_tan >= 8 and np.linalg.norm(p2 - p1) < MAX_SEG, (k, n_tan)
        return st
    return _cached(("order", k, None if shift is None else tuple(shift)), build)


# ---- exact ties ------------------------------------------------------------------------------------------------------------------------------------------------
TIE_P1, TIE_P2 = np.array([-1.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])
TIE_SEED, TIE_FILL = 0, 520
FOUR = np.array([[0.0, 0.5, 0.0], [0.0, -0.5, 0.0], [0.0, 0.0, 0.5], [0.0, 0.0, -0.5]])


def four_contacts(swapped, frx=None):
    """the four-contact state; swapped: (0,-1/2,0) and (0,0,-1/2) change places in the cloud.  st.four = the four in cloud order.  With frx the host form's record
    order is checked too."""
    def build():
        rng = np.random.default_rng(9000 + TIE_SEED)
        fill = []
        while len(fill) < TIE_FILL:
            q = np.array([rng.uniform(-4.5, 4.5), rng.uniform(-3.5, 3.5), rng.uniform(-2.2, 2.2)])
            if np.hypot(q[1], q[2]) > 0.6:
                fill.append(q)
        four = FOUR[[0, 3, 2, 1]] if swapped else FOUR.copy()
        inside = list(fill)
        for pos, q in zip(TIE_AT, four):
            inside.insert(pos, q)
        inside = np.array(inside); far = _far(rng, TIE_P1, TIE_P2, len(inside) // 2)
        obs = []
        for i, q in enumerate(inside):                             # an outside point after every second candidate
            obs.append(q)
            if i % 2 == 1: obs.append(far[i // 2])
        st = make("four" + ("-swapped" if swapped else ""), TIE_P1, TIE_P2, BBOX, np.array(obs), tie_ok=True, exact=True, want_M=TIE_FILL + 4)
        st.four = four
        assert [c for c, _ in st.ref.order[:4]] == TIE_AT and np.array_equal(st.ref.H[3:, :4].T, four)
        assert np.array_equal(st.ref.H[:3, :4].T, 2.0 * four)       # the normals are the axes, exactly
        assert (st.ref.gaps[:1] == 0.0).all() and (st.ref.dist_final[TIE_AT] == 1.0).all()
        return st
    st = _cached(("four", swapped), build)
    if frx is not None:
        H, _, _ = frx.line_segment_dilate(st.p1, st.p2, st.bbox, st.obs)
        assert H.shape == st.ref.H.shape and np.array_equal(H[3:, :4].T, st.four), "the host form's record order does not follow the cloud order"
    return st


def duplicate_pair():
    """(state without the duplicate, state with it): the contact point of the first tangent plane behind the contact group stands at cloud index 0, its copy at the
    end, more than 256 candidates later"""
    def build():
        base = order_state(2)
        c = base.ref.order[base.group][1]
        obs = base.obs.copy(); obs[[0, c]] = obs[[c, 0]]
        a = make("single", base.p1, base.p2, base.bbox, obs)
        b = make("duplicate", base.p1, base.p2, base.bbox, np.vstack([obs, obs[:1]]), tie_ok=True)
        assert a.ref.order[a.group] == (0, 0) and b.M == a.M + 1 and b.ref.cand[-1] == len(obs) and b.M - 1 >= 256
        assert b.K == a.K and np.array_equal(a.ref.H, b.ref.H) and a.ref.order == b.ref.order
        return a, b
    return _cached("dup", build)


# ---- capacity of planes ----------------------------------------------------------------------------------------------------------------------------------------
def plane_caps():
    """[(state, K)]: cap_planes = K must succeed, K - 1 must refuse; the first has a box (np + 6 > cap_planes), the second is the same segment and cloud with a
    zero box (np >= cap_planes)"""
    def build():
        a = order_state(0)
        b = make("order0-nobox", a.p1, a.p2, np.zeros(3), a.obs)
        assert a.K - 1 >= 6 and b.K - 1 >= 6                        # frx_dilate_batch takes no cap_planes below 6
        return [(a, a.K), (b, b.K)]
    return _cached("caps", build)


# ---- batch and chain -------------------------------------------------------------------------------------------------------------------------------------------
SHIFTS = [np.array([100.0, 0.0, 0.0]), np.array([0.0, 100.0, 0.0]), np.array([-100.0, 0.0, 0.0]), np.array([0.0, -100.0, 0.0])]


def batch():
    """(states [5], cloud): segment 2 is the M = 4097 state; the others are order states 0, 1, 1, 0 moved 100 m away in four directions, so that every segment's
    box holds its own points only (the zero-box order state would take the whole union as candidates); one cloud, the union in the order 0, 1, 2, 3, 4"""
    def build():
        big = count_state(PCAP + 1)
        parts = [order_state(0, SHIFTS[0]), order_state(1, SHIFTS[1]), big, order_state(1, SHIFTS[2]), order_state(0, SHIFTS[3])]
        cloud = np.ascontiguousarray(np.vstack([s.obs for s in parts]))
        out = []
        for s in parts:                                            # the same cells over the union (checked: same candidates, so the same restatement)
            t = make(s.name + "@batch", s.p1, s.p2, s.bbox, cloud, want_M=s.M)
            assert t.K == s.K and np.array_equal(t.ref.H, s.ref.H)
            out.append(t)
        return out, cloud
    return _cached("batch", build)


def chain_world(frx, M):
    """(paths [2], cloud): path 0 = the two end points of count_state(M)'s segment, path 1 = order state 0 moved 100 m away; the cloud holds both.  Self-checked:
    the host chain forms exactly one cell for either path (for path 0 only when M <= 4096 matters to the device; the host has no such limit)."""
    def build():
        big, nb = count_state(M), order_state(0, SHIFTS[0])
        cloud = np.ascontiguousarray(np.vstack([big.obs, nb.obs]))
        paths = [np.stack([big.p1, big.p2]), np.stack([nb.p1, nb.p2])]
        for p in paths:
            assert np.linalg.norm(p[1] - p[0]) < MAX_SEG
            assert len(frx.corridor_generate(p, cloud, BBOX, MAP_HEIGHT, MAX_SEG)) == 1
        assert len(dr.candidates(big.p1, big.p2, BBOX, cloud)[0]) == M
        return paths, cloud
    return _cached(("chain", M), build)


def all_parity_states():
    """every cloud-size, candidate-count (M <= 4096) and order state"""
    return [size_state(n) for n in SIZES] + [count_state(M) for M in COUNTS if M <= PCAP] + [order_state(k) for k in range(3)]
