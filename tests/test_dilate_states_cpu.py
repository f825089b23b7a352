"""The states of tests/dilate_states.py and the restatement of tests/dilate_reference.py, on the CPU: every builder runs with its self-checks, the restatement
agrees with the library's host form (frx_line_segment_dilate) on every state IN EMISSION ORDER modulo the declared groups - 1e-9 on planes and ellipsoid, 1e-12
on the centre, the tolerances of test_next_rows.py - and, where oracle/_ref/libref_decomp.so is built, with the reference's own LineSegment3D::dilate; its
float64 and longdouble decisions are equal; and the cell it forms keeps the cell's promise (no candidate inside all planes, none inside the ellipsoid, the
segment inside)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dilate_reference as dr  # noqa: E402
import dilate_states as ds  # noqa: E402

TOL, TOL_D = 1e-9, 1e-12


def _states(frx):
    a, b = ds.duplicate_pair()
    return (ds.all_parity_states() + [ds.count_state(ds.PCAP + 1), ds.four_contacts(False, frx), ds.four_contacts(True, frx), a, b]
            + [s for s, _ in ds.plane_caps()] + ds.batch()[0])


def test_every_builder_runs_and_is_what_it_claims(frx):
    sts = _states(frx)
    assert len(sts) == len(ds.SIZES) + len(ds.COUNTS) + 3 + 2 + 2 + 2 + 5
    for n in ds.SIZES:
        st = ds.size_state(n)
        chunk = -(-n // 256); owners = -(-n // chunk)                          # the kernel's chunks: thread t owns [t chunk, (t + 1) chunk)
        assert len(st.obs) == n and n - 1 in st.ref.cand and 0 in st.ref.cand
        if n == 257:
            assert chunk == 2 and owners == 129 and n - (owners - 1) * chunk == 1     # thread 128 holds the single last point, threads 129.. start past the end
        if n == 513:
            assert chunk == 3 and owners == 171                                 # (513 = 171 x 3: the last owner holds a full chunk; 85 threads hold none)
        if n == 1025:
            assert chunk == 5 and owners == 205
    for M in ds.COUNTS:
        st = ds.count_state(M)
        assert st.M == M and (M < ds.PCAP - 1 or len(st.obs) > ds.PCAP + 1)
        if M >= ds.PCAP - 1:
            assert ds.host_planes_within_cap(frx, st)
    assert ds.count_state(0).K == 6 and len(ds.count_state(0).obs) == 300
    for (st, K) in ds.plane_caps():
        assert K == st.K
    sts5, cloud = ds.batch()
    assert len(sts5) == 5 and sts5[2].M == ds.PCAP + 1 and all(s.obs is not None and len(s.obs) == len(cloud) for s in sts5)
    for M in (ds.PCAP, ds.PCAP + 1):
        paths, cloud = ds.chain_world(frx, M)
        assert len(paths) == 2 and len(cloud) > M


def test_swapping_two_tied_points_swaps_their_planes(frx):
    a, b = ds.four_contacts(False, frx), ds.four_contacts(True, frx)
    assert np.array_equal(a.four, ds.FOUR) and np.array_equal(b.four, ds.FOUR[[0, 3, 2, 1]])
    assert np.array_equal(a.ref.H[:, 4:], b.ref.H[:, 4:]) and np.array_equal(a.ref.C, b.ref.C)
    assert np.array_equal(a.ref.C, np.diag([1.0, 0.5, 0.5]))
    for st in (a, b):                                                           # the host form, bit for bit: the state's arithmetic is exact
        H, Cm, d = frx.line_segment_dilate(st.p1, st.p2, st.bbox, st.obs)
        assert np.array_equal(H[:, :4], st.ref.H[:, :4]) and np.array_equal(Cm, st.ref.C)


def test_the_duplicate_changes_nothing(frx):
    a, b = ds.duplicate_pair()
    Ha, Ca, _ = frx.line_segment_dilate(a.p1, a.p2, a.bbox, a.obs)
    Hb, Cb, _ = frx.line_segment_dilate(b.p1, b.p2, b.bbox, b.obs)
    assert np.array_equal(Ha, Hb) and np.array_equal(Ca, Cb)
    ds.assert_order(Hb, b)                                                      # the first copy (cloud index 0) is the contact, not the one at the end


def test_restatement_matches_the_host_form_in_emission_order(frx, ob):
    worst = [0.0, 0.0, 0.0]
    for st in _states(frx):
        H, Cm, d = frx.line_segment_dilate(st.p1, st.p2, st.bbox, st.obs)
        dh, dc, dd = ds.plane_difference(H, st), np.abs(Cm - st.ref.C).max(), np.abs(d - st.ref.d).max()
        assert dh < TOL and dc < TOL and dd < TOL_D, (st.name, dh, dc, dd)
        ds.assert_order(H, st)
        worst = [max(worst[0], dh), max(worst[1], dc), max(worst[2], dd)]
        if ob.ref_decomp() is not None:                                         # the reference's own decomp_util
            Hr, Cr, dref = ob.ref_line_segment_dilate(st.p1, st.p2, st.bbox, st.obs)
            assert ds.plane_difference(Hr, st) < TOL and np.abs(Cr - st.ref.C).max() < TOL and np.abs(dref - st.ref.d).max() < TOL_D, st.name
            ds.assert_order(Hr, st)
    print(f"restatement vs host form, worst: planes {worst[0]:.2e} ellipsoid {worst[1]:.2e} centre {worst[2]:.2e}")


def test_float64_and_longdouble_make_the_same_decisions(frx):
    for st in _states(frx):
        rl = dr.dilate_cell(st.p1, st.p2, st.bbox, st.obs, dtype=np.longdouble)
        g = st.group
        assert rl.order[g:] == st.ref.order[g:] and sorted(rl.order[:g]) == sorted(st.ref.order[:g]), st.name
        assert np.array_equal(rl.cand, st.ref.cand)
        assert ds.plane_difference(np.asarray(rl.H, dtype=np.float64), st) < TOL and np.abs(np.asarray(rl.C, dtype=np.float64) - st.ref.C).max() < TOL


def test_the_restatement_keeps_the_cells_promise(frx):
    for st in _states(frx):
        deep, in_ell, seg = dr.unsafe_points(st.ref.H, st.ref.C, st.ref.d, st.p1, st.p2, st.bbox, st.obs)
        assert deep == 0 and in_ell == 0 and seg <= TOL, (st.name, deep, in_ell, seg)


def test_the_promise_check_sees_a_broken_cell():
    """unsafe_points is itself a check: a cell with one tangent plane dropped, or an ellipsoid blown up, must be reported"""
    st = ds.order_state(1)
    last = st.K - 7                                                             # the last tangent plane: its contact point was inside all earlier ones
    assert dr.unsafe_points(np.delete(st.ref.H, last, axis=1), st.ref.C, st.ref.d, st.p1, st.p2, st.bbox, st.obs)[0] >= 1
    assert dr.unsafe_points(st.ref.H, 1.5 * st.ref.C, st.ref.d, st.p1, st.p2, st.bbox, st.obs)[1] >= 1
    moved = st.ref.H.copy(); moved[3:, 0] = st.ref.d - 0.01 * moved[:3, 0]      # a plane 1 cm beyond the midpoint
    assert dr.unsafe_points(moved, st.ref.C, st.ref.d, st.p1, st.p2, st.bbox, st.obs)[2] > 1e-3


def test_the_states_reach_every_wave():
    """contact points on every wave's lanes (compacted position mod 256) and behind the first stride of the scans, so that a wave left out of a fold shows"""
    pos = [c for st in ds.all_parity_states() for c, _ in st.ref.order]
    assert {(c % 256) // 64 for c in pos} == {0, 1, 2, 3} and max(pos) >= 256
    for st in ds.all_parity_states():
        print(st.name, sorted({(c % 256) // 64 for c, _ in st.ref.order}))
