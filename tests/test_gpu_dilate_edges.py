"""dilate_cell (frx_corridor_kernels.hpp) on the device, through both of its kernels - k_dilate (frx_dilate_batch) and k_corridor_chain
(frx_corridor_generate_batch) - on the decision-safe states of tests/dilate_states.py, against the plain numpy restatement of tests/dilate_reference.py:
records IN EMISSION ORDER (modulo the declared contact group) within 1e-9, ellipsoid within 1e-9, centre within 1e-12, every contact point bit-equal to the
cloud point the restatement names; exact ties in cloud order with ==; the cell's own promise on the device's output; and both capacities at their edges.
The largest launch is 5 workgroups.  Nothing here reads the reference tree.

Which mutation of the kernel each group catches, argued from the code:
  * `i < bi` turned into `i > bi`, the tie rule of the block-wide arg-min, in
      - the shuffle fold: the four contacts stand at compacted positions 37 and 38 (lanes 37, 38 of wave 0).  Tied at distance exactly 1, wave 0 would hand
        on 38 instead of 37: the first record is (0,-1/2,0) instead of (0,1/2,0) -> test_exact_ties_come_out_in_cloud_order;
      - the fold over red[]: position 102 is lane 38 of wave 1.  Once 37 is gone the tie of 38 / 102 / 358 is between wave 0 and wave 1: the second record
        becomes the point at 102 -> the same test;
      - the lane loop: 358 = 102 + 256 is the same lane one stride later.  As written the clause is dead there - i ascends, so `i < bi` never holds once bi is
        set, and dropping it changes nothing - but flipped it prefers the later index at a tie: the third record becomes the point at 358 -> the same test,
        and only a state with two tied candidates on ONE lane can see it.
    (The duplicate state cannot see any of the three: whichever copy wins, the record holds the same bits.  It is there for the filter `n.(q - c) < 0` at
    exactly 0: a `<= 0` would keep the second copy alive and give it a plane of its own -> test_a_duplicate_changes_nothing, by plane count.)
  * the prefix scan started at cnt[1] (cnt[0] keeps thread 0's count mine_0 instead of 0): every other thread's offset and M lose mine_0, and thread 0 writes
    its candidates at mine_0.. on top of its neighbours' or past M.  Cloud point 0 is in the box in every size state and in count1: at size1 and count1 it is the
    only candidate and M becomes 0 (six box planes); at size2 thread 1 puts the near point into slot 0, M is 1 and point 0 - a tangent plane of its own - lies
    past it -> test_matches_the_restatement_in_emission_order[size1, size2, count1], by plane count.
  * `chunk` rounded down (n_obs / 256): 0 at n_obs = 1, 2, 255 (no candidate at all: six box planes), and at 257, 511, 513, 1025 the tail n_obs - 256 chunk is
    never read; the last cloud point is the nearest one -> the same size cases.  At 256 and 512 the mutant is equivalent (n_obs is a multiple of 256).
  * `M > pcap` turned into `M >= pcap`: count4096 refuses -> test_matches_the_restatement_in_emission_order[count4096], test_4096_candidates_fit_and_4097_do_not
    and test_chain_at_the_candidate_capacity.  Turned into `M > pcap + 1`, 4097 candidates would be written into a 4096-point buffer; the 4097 cases ask for the refusal.
  * `np + 6 > cap_planes` off by one: `>=` refuses cap_planes = K; `np + 5 >` accepts K - 1 -> test_plane_capacity_is_exact (with a box); the zero-box state
    holds `np >= cap_planes` in the same way.
  * a wave left out of the fold over red[] (w2 < 3): candidates on lanes 192-255 never win.  The size states from 511 on, the count states from 255 on and order
    state 2 hold contact points there (test_dilate_states_cpu.py: test_the_states_reach_every_wave) -> parity, by contact index.
None of the six is an equivalent mutant of the kernel as a whole; two are equivalent on part of the input (chunk at multiples of 256; the lane loop's clause
when dropped rather than flipped).

Every parity case prints its device - restatement differences (planes, ellipsoid, centre); the worst of them are kept in DESIGN.md, section 3.13.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dilate_reference as dr  # noqa: E402
import dilate_states as ds  # noqa: E402
from test_gpu_corridor_batch import assert_same_corridor  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, TOL_D = 1e-9, 1e-12
ERR_CAPACITY = -5                                                            # FRX_ERR_CAPACITY (include/frx.h)

_cells = {}


def device_cell(frx, st, cap_planes=96):
    """(H, C, d) of the state's cell by k_dilate; one launch per state and module"""
    key = (st.name, cap_planes)
    if key not in _cells:
        _cells[key], = frx.dilate_batch(st.p1[None], st.p2[None], st.bbox, st.obs, cap_planes=cap_planes)
    return _cells[key]


PARITY = [f"size{n}" for n in ds.SIZES] + [f"count{M}" for M in ds.COUNTS if M <= ds.PCAP] + [f"order{k}" for k in range(3)]


def _state(name):
    if name.startswith("size"): return ds.size_state(int(name[4:]))
    if name.startswith("count"): return ds.count_state(int(name[5:]))
    return ds.order_state(int(name[5:]))


@pytest.mark.parametrize("name", PARITY)
def test_matches_the_restatement_in_emission_order(frx, name):
    st = _state(name)
    H, Cm, d = device_cell(frx, st)
    assert H.shape[1] == st.K, (name, H.shape[1], st.K)
    dh, dc, dd = ds.plane_difference(H, st), np.abs(Cm - st.ref.C).max(), np.abs(d - st.ref.d).max()
    print(f"{name}: M {st.M}, {st.K} records, device - restatement: planes {dh:.2e} ellipsoid {dc:.2e} centre {dd:.2e}")
    assert dh < TOL and dc < TOL and dd < TOL_D, (name, dh, dc, dd)
    ds.assert_order(H, st)                                                   # every contact point is a cloud point, bit for bit, and the one the restatement names


def test_exact_ties_come_out_in_cloud_order(frx):
    for swapped in (False, True):
        st = ds.four_contacts(swapped, frx)
        H, Cm, d = device_cell(frx, st)
        assert H.shape[1] == st.K
        assert np.array_equal(H[3:, :4].T, st.four), (swapped, H[3:, :4].T)  # == : the four contacts in THIS cloud's order
        assert np.array_equal(H[:3, :4].T, 2.0 * st.four) and np.array_equal(Cm, np.diag([1.0, 0.5, 0.5]))      # the state's arithmetic is exact
        assert ds.plane_difference(H, st) < TOL
        ds.assert_order(H, st)
    a, b = ds.four_contacts(False), ds.four_contacts(True)
    assert np.array_equal(device_cell(frx, a)[0][3:, 1], device_cell(frx, b)[0][3:, 3])        # the swap moved the records with the points


def test_a_duplicate_changes_nothing(frx):
    a, b = ds.duplicate_pair()
    Ha, Ca, da = device_cell(frx, a)
    Hb, Cb, db = device_cell(frx, b)
    assert np.array_equal(Ha, Hb) and np.array_equal(Ca, Cb) and np.array_equal(da, db)
    assert ds.plane_difference(Hb, b) < TOL
    ds.assert_order(Hb, b)


def test_device_cells_keep_the_cells_promise(frx):
    """reference-free, on the device's own output: no candidate more than 1e-9 inside all planes, none with | C^-1 (q - d) | < 1 - 1e-9, the segment inside"""
    a, b = ds.duplicate_pair()
    for st in [_state(n) for n in PARITY] + [ds.four_contacts(False), ds.four_contacts(True), a, b]:
        H, Cm, d = device_cell(frx, st)
        deep, in_ell, seg = dr.unsafe_points(H, Cm, d, st.p1, st.p2, st.bbox, st.obs, tol=TOL)
        assert deep == 0 and in_ell == 0 and seg <= TOL, (st.name, deep, in_ell, seg)


def _refused(frx, st, cap_planes, text):
    with pytest.raises(frx.FrxError) as e:
        frx.dilate_batch(st.p1[None], st.p2[None], st.bbox, st.obs, cap_planes=cap_planes)
    assert e.value.code == ERR_CAPACITY and text in str(e.value), str(e.value)


def test_4096_candidates_fit_and_4097_do_not(frx):
    st = ds.count_state(ds.PCAP)
    H, Cm, d = device_cell(frx, st)
    assert H.shape[1] == st.K and ds.plane_difference(H, st) < TOL and np.abs(Cm - st.ref.C).max() < TOL
    _refused(frx, ds.count_state(ds.PCAP + 1), 96, "more than 4096 obstacle points")


def test_plane_capacity_is_exact(frx):
    for st, K in ds.plane_caps():                                            # with a box: np + 6 > cap_planes; zero box: np >= cap_planes
        H, Cm, d = device_cell(frx, st, cap_planes=K)
        assert H.shape[1] == K and ds.plane_difference(H, st) < TOL
        ds.assert_order(H, st)
        _refused(frx, st, K - 1, "more half-spaces than cap_planes")


def _raw_batch(frx, sts, cloud, cap_planes=96):
    """frx_dilate_batch itself, so that the buffers survive an error: (rc, n_planes, records [S][cap][6], C [S][9], d [S][3]).  Only the first n_planes[s] records
    of a row are defined (include/frx.h): the call copies the whole device buffer back, so what lies behind them is not the caller's fill."""
    S = len(sts)
    p1 = np.ascontiguousarray(np.concatenate([s.p1 for s in sts])); p2 = np.ascontiguousarray(np.concatenate([s.p2 for s in sts]))
    npl = np.full(S, -77, np.int32); rec = np.full(S * cap_planes * 6, -7.0); Cm = np.full(S * 9, -7.0); d = np.full(S * 3, -7.0)
    rc = frx.lib().frx_dilate_batch(0, S, p1, p2, np.ascontiguousarray(ds.BBOX), len(cloud), cloud.ctypes.data, 0.0, cap_planes, npl, rec, Cm, d)
    return rc, npl, rec.reshape(S, cap_planes, 6), Cm.reshape(S, 9), d.reshape(S, 3)


def test_a_refused_segment_leaves_its_neighbours_rows_valid(frx):
    """include/frx.h: on FRX_ERR_CAPACITY n_planes marks the refused segments (-1 / -2) and every other segment's rows are what the call gives without them"""
    sts, cloud = ds.batch()
    rc, npl, rec, Cm, d = _raw_batch(frx, sts, cloud)
    assert rc == ERR_CAPACITY and b"4096 obstacle points" in frx.lib().frx_last_error()
    assert npl[2] == -1
    others = [0, 1, 3, 4]
    rc4, npl4, rec4, Cm4, d4 = _raw_batch(frx, [sts[i] for i in others], cloud)
    assert rc4 == 0
    for k, i in enumerate(others):
        assert npl[i] == npl4[k] == sts[i].K, (i, npl[i], npl4[k], sts[i].K)
        assert np.array_equal(rec[i, :npl[i]], rec4[k, :npl4[k]]) and np.array_equal(Cm[i], Cm4[k]) and np.array_equal(d[i], d4[k])
        assert ds.plane_difference(rec[i, :npl[i]].T, sts[i]) < TOL


def test_chain_at_the_candidate_capacity(frx):
    paths, cloud = ds.chain_world(frx, ds.PCAP)
    got, st = frx.corridor_generate_batch(paths[:1], cloud, ds.BBOX, ds.MAP_HEIGHT, ds.MAX_SEG)
    assert st.tolist() == [0] and len(got[0]) == 1
    assert_same_corridor(got[0], frx.corridor_generate(paths[0], cloud, ds.BBOX, ds.MAP_HEIGHT, ds.MAX_SEG), "M = 4096")
    big = ds.count_state(ds.PCAP)                                            # the same candidates, so the same restatement - in emission order
    assert ds.plane_difference(got[0][0][:, :-2], big) < TOL
    # the largest LDS layout: at cap_planes = 512 the records start right behind cnt[]
    wide, stw = frx.corridor_generate_batch(paths[:1], cloud, ds.BBOX, ds.MAP_HEIGHT, ds.MAX_SEG, cap_planes=512)
    assert stw.tolist() == [0] and len(wide[0]) == 1 and np.array_equal(wide[0][0], got[0][0])
    # one more candidate: the path is refused, a neighbour far from it is unchanged bit for bit
    paths7, cloud7 = ds.chain_world(frx, ds.PCAP + 1)
    got7, st7 = frx.corridor_generate_batch(paths7, cloud7, ds.BBOX, ds.MAP_HEIGHT, ds.MAX_SEG)
    assert st7.tolist() == [frx.CHAIN_BOX_POINTS, 0] and got7[0] == [] and len(got7[1]) == 1
    alone, sta = frx.corridor_generate_batch(paths7[1:], cloud7, ds.BBOX, ds.MAP_HEIGHT, ds.MAX_SEG)
    assert sta.tolist() == [0] and len(alone[0]) == 1 and np.array_equal(alone[0][0], got7[1][0])
    assert ds.plane_difference(got7[1][0][:, :-2], ds.order_state(0, ds.SHIFTS[0])) < TOL


@pytest.mark.parametrize("k", range(3))
def test_both_kernels_form_the_same_bits(frx, k):
    """k_dilate's cell of segment p1-p2 == the first (only) cell of k_corridor_chain for the 2-point path p1, p2: the same dilate_cell with offset 0"""
    st = ds.order_state(k)
    H, _, _ = device_cell(frx, st)
    (cells,), status = frx.corridor_generate_batch([np.stack([st.p1, st.p2])], st.obs, st.bbox, ds.MAP_HEIGHT, ds.MAX_SEG)
    assert status.tolist() == [0] and len(cells) == 1
    chain = cells[0]
    assert np.array_equal(chain[:, -2:], np.array([[0, 0, 1, 0, 0, ds.MAP_HEIGHT], [0, 0, -1, 0, 0, 0]], float).T)      # ceiling, then floor
    assert np.array_equal(chain[:, :-2], H)
