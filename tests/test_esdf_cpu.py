"""frx_map_esdf on the host against the numpy referee (tests/esdf_reference.py), bit for bit; the referee against the definition; the verdicts and the scratch
of the device form, answered without a device; the fold of the screen (frx_map_distance_fold) against its numpy restatement; and the argument rules, all of
which come before the search for a device."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esdf_reference as er  # noqa: E402
import esdf_states as es  # noqa: E402
import map_distance_reference as mr  # noqa: E402
from conftest import has_gpu  # noqa: E402

KEYS = ("pos", "neg", "all")


def test_the_referee_is_the_definition_on_small_maps():
    rng = np.random.default_rng(1)
    for trial in range(60):
        dim = tuple(int(v) for v in rng.integers(1, 9, 3))
        cells = rng.choice(np.array([-1, 0, 0, 100], np.int8), dim[0] * dim[1] * dim[2]) if trial % 5 else np.full(dim[0] * dim[1] * dim[2], (-1, 0, 100)[trial % 3], np.int8)
        a, b = er.fields(cells, dim, 0.1), er.fields(cells, dim, 0.1, er.brute_squared)
        for k in KEYS + ("d2_occ", "d2_free"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (dim, k)


def test_host_equals_the_referee_on_every_state(frx):
    both_kinds = 0
    for label, dim, res, cells in es.all_states():
        ref = er.fields(cells, dim, res)
        m = frx.VoxelMap([0.0, 0.0, 0.0], dim, res, cells)
        got = m.esdf()
        for k in KEYS:
            assert er.same_bits(got[k], ref[k]), (label, k, np.flatnonzero(got[k].view(np.uint64) != ref[k].view(np.uint64))[:5])
        for drop in KEYS:                                                 # each output NULL in turn: the others keep their bits
            part = m.esdf([k for k in KEYS if k != drop])
            assert set(part) == set(KEYS) - {drop} and all(er.same_bits(part[k], ref[k]) for k in part), (label, drop)
        for k in KEYS:
            assert er.same_bits(m.esdf([k])[k], ref[k]), (label, k)
        both_kinds += bool(np.isfinite(ref["pos"]).all() and np.isfinite(ref["neg"]).all() and (ref["neg"] > 0).any() and (ref["pos"] > 0).any())
    assert both_kinds >= 40
    # the stated outcomes without a site: +inf, -inf where only neg is infinite, the plain quiet NaN where both are
    full = frx.VoxelMap([0, 0, 0], (3, 2, 2), 0.5, np.full(12, 100, np.int8)).esdf()
    assert (full["pos"] == 0).all() and np.isposinf(full["neg"]).all() and np.isneginf(full["all"]).all()
    unknown = frx.VoxelMap([0, 0, 0], (3, 2, 2), 0.5, np.full(12, -1, np.int8)).esdf()
    assert np.isposinf(unknown["pos"]).all() and np.isposinf(unknown["neg"]).all() and (unknown["all"].view(np.uint64) == 0x7FF8000000000000).all()
    empty = frx.VoxelMap([0, 0, 0], (3, 2, 2), 0.5).esdf()
    assert np.isposinf(empty["pos"]).all() and (empty["neg"] == 0).all() and np.isposinf(empty["all"]).all()


def test_pos_is_rounded_before_the_sum(frx):
    """res sqrt(v) + (-neg + res) in one fused multiply-add differs from the stated two roundings somewhere on these maps; the library gives the stated ones."""
    rng = np.random.default_rng(3)
    differs = 0
    for res in (0.1, 0.3, 0.7):
        cells = rng.choice(np.array([-1, -1, -1, -1, -1, -1, 0, 100], np.int8), 40 * 9 * 3)   # unknown cells are where pos > 0 and neg > 0 at once
        ref = er.fields(cells, (40, 9, 3), res)
        got = frx.VoxelMap([0, 0, 0], (40, 9, 3), res, cells).esdf()
        assert er.same_bits(got["all"], ref["all"])
        inside = np.flatnonzero(ref["neg"] > 0)[:400]
        for o, n in zip(ref["d2_occ"][inside], ref["neg"][inside]):
            tail = -float(n) + res                                            # the parenthesis, rounded
            fused = float(Fraction(res) * Fraction(float(np.sqrt(np.float64(o)))) + Fraction(tail))   # one rounding of the exact sum: what a fused multiply-add gives
            differs += fused != res * float(np.sqrt(np.float64(o))) + tail
    assert differs >= 1


def dims_grid():
    vals = (-1, 0, 1, 2, 255, 256, 257, 4096, es.LIMIT, es.LIMIT + 1, es.MAX_DIM, es.MAX_DIM + 1)
    return [(a, b, c) for a in vals for b in vals for c in vals]


def test_verdicts_and_workspace_over_a_grid_of_dims(frx):
    L = frx.lib()
    for dim in dims_grid():
        d = (C.c_int * 3)(*dim)
        n = C.c_size_t(77)
        rc = L.frx_map_esdf_workspace(d, C.byref(n))
        cells = dim[0] * dim[1] * dim[2]
        if min(dim) <= 0:
            want = -1
        elif dim[0] > es.LIMIT or dim[1] > es.MAX_DIM or dim[2] > es.MAX_DIM or cells > 2 ** 31 - 1:
            want = -5
        else:
            want = 0
        assert rc == want, (dim, rc, want)
        assert n.value == (4 * (4 * cells + dim[0] + 1 + 2 * dim[0] * dim[1]) if want == 0 else 77), (dim, n.value)
    assert frx.map_esdf_workspace((700, 4000, 28)) == 4 * (4 * 700 * 4000 * 28 + 701 + 2 * 700 * 4000)          # the 0.1 m volume: inside the limits
    assert frx.map_esdf_workspace((4096, 4096, 127)) > 0
    assert L.frx_map_esdf_workspace(None, C.byref(C.c_size_t())) == -1 and L.frx_map_esdf_workspace((C.c_int * 3)(1, 1, 1), None) == -1


def test_argument_errors_come_before_the_device(frx):
    L = frx.lib()
    ok = frx.VoxelMap([0, 0, 0], (4, 3, 2), 0.1)
    out = np.full(24, -7.0)
    o = out.ctypes.data
    one = C.c_void_p(8)                                                   # a non-NULL address nobody reads: the argument rules come first
    S = frx.VoxelMapStruct

    def st(dim=(4, 3, 2), res=0.1, cells=ok.cells.ctypes.data):
        return S((C.c_double * 3)(0, 0, 0), (C.c_int * 3)(*dim), res, cells)
    bad = [(st(res=0.0), -1), (st(res=-1.0), -1), (st(res=float("nan")), -1), (st(dim=(0, 3, 2)), -1), (st(dim=(4, -1, 2)), -1), (st(cells=None), -1),
           (st(dim=(es.LIMIT + 1, 1, 1)), -5), (st(dim=(1, es.MAX_DIM + 1, 1)), -5), (st(dim=(1, 1, es.MAX_DIM + 1)), -5), (st(dim=(es.LIMIT, es.MAX_DIM, 17)), -5)]
    for s, want in bad:
        assert L.frx_map_esdf(C.byref(s), o, o, o) == want
        assert L.frx_map_esdf_device(C.byref(s), one, one, one, one, None) == want
        assert L.frx_map_esdf_on_device(0, C.byref(s), o, o, o) == want
    good = st()
    assert L.frx_map_esdf(None, o, o, o) == -1 and L.frx_map_esdf(C.byref(good), None, None, None) == -1
    assert L.frx_map_esdf_device(None, one, one, one, one, None) == -1 and L.frx_map_esdf_device(C.byref(good), None, None, None, one, None) == -1
    assert L.frx_map_esdf_device(C.byref(good), one, one, one, None, None) == -1 and b"work_dev" in L.frx_last_error()
    assert L.frx_map_esdf_on_device(0, None, o, o, o) == -1 and L.frx_map_esdf_on_device(0, C.byref(good), None, None, None) == -1
    for args in ((None, one, 1, one, one), (good, None, 1, one, one), (good, one, -1, one, one), (good, one, 1, None, one), (good, one, 1, one, None),
                 (st(res=0.0), one, 1, one, one), (st(dim=(4, 0, 2)), one, 1, one, one), (st(dim=(65536, 65536, 1)), one, 1, one, one)):
        s = C.byref(args[0]) if args[0] is not None else None
        assert L.frx_map_mark_cloud_device(s, *args[1:], None) == -1, args[1:]
    assert (out == -7.0).all()
    # the fold and the screen: no handle, so every rule that needs none
    z = np.zeros(8); off = np.array([0, 1], np.int32)
    assert L.frx_map_distance_fold(0, off.ctypes.data, z.ctypes.data, z.ctypes.data, 0.0, z.ctypes.data, None) == -1
    assert L.frx_map_distance_fold(1, None, z.ctypes.data, z.ctypes.data, 0.0, z.ctypes.data, None) == -1
    assert L.frx_map_distance_fold(1, off.ctypes.data, z.ctypes.data, z.ctypes.data, float("nan"), z.ctypes.data, None) == -1
    assert L.frx_map_distance_fold(1, np.array([1, 0], np.int32).ctypes.data, z.ctypes.data, z.ctypes.data, 0.0, z.ctypes.data, None) == -1
    assert L.frx_trajectory_map_distance(None, o, o, 8, C.byref(good), o, 0.0, o, o, None) == -1
    assert L.frx_trajectory_map_distance_device(None, one, one, 8, C.byref(good), one, one, None) == -1


@pytest.mark.skipif(has_gpu(), reason="checks the no-device behaviour")
def test_device_forms_report_the_missing_device(frx):
    L = frx.lib()
    m = frx.VoxelMap([0, 0, 0], (4, 3, 2), 0.1)
    one = C.c_void_p(8)
    assert L.frx_map_esdf_device(C.byref(m._s), one, one, one, one, None) == -2
    assert L.frx_map_mark_cloud_device(C.byref(m._s), one, 0, None, one, None) == -2
    with pytest.raises(frx.FrxError, match="no HIP device") as e:
        m.esdf_on_device()
    assert e.value.code == -2


def random_rows(rng, P):
    rows = np.stack([rng.choice([0.0, 0.1, 0.25, 0.25, 1.5, np.inf, np.nan, -0.5], P), rng.uniform(0.0, 1.0, P), rng.integers(0, 1000, P).astype(float),
                     rng.integers(0, 4, P).astype(float)], axis=1)
    none = rng.random(P) < 0.2                                            # pieces with no sample inside the map
    rows[none] = [np.inf, -1.0, -1.0, 9.0]
    return rows


def test_fold_against_numpy(frx):
    rng = np.random.default_rng(5)
    for trial in range(200):
        B = int(rng.integers(1, 7))
        counts = rng.integers(0, 5, B)                                    # candidates without pieces among them: first, in the middle, last
        if trial == 0:
            counts = np.array([0, 3, 0, 2, 0])
            B = 5
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        P = int(off[-1])
        T = rng.uniform(0.3, 2.0, P)
        rows = random_rows(rng, P)
        margin = float(rng.choice([0.0, 0.25, 0.2, np.inf, -np.inf]))
        cand, flags = frx.map_distance_fold(rows, T, off, margin)
        rc, rf = mr.fold(rows, T, off, margin)
        assert np.array_equal(cand.view(np.uint64), rc.view(np.uint64)) and np.array_equal(flags, rf), (trial, off, rows, cand, rc, flags, rf)
    # the stated cases by hand
    rows = np.array([[0.5, 0.1, 7.0, 0.0], [np.nan, 0.2, 8.0, 1.0], [np.nan, 0.3, 9.0, 0.0], [0.25, 0.0, 3.0, 2.0], [0.25, 0.4, 4.0, 0.0], [np.inf, -1.0, -1.0, 5.0]])
    T = np.array([1.0, 2.0, 4.0, 1.0, 1.0, 1.0])
    cand, flags = frx.map_distance_fold(rows, T, [0, 3, 5, 5, 6], 0.25)
    assert np.isnan(cand[0, 0]) and tuple(cand[0, 1:]) == (1.0 + 0.2, 8.0, 1.0) and flags[0] == frx.MAPDIST_FLAG_OUTSIDE | frx.MAPDIST_FLAG_NONFINITE
    assert tuple(cand[1]) == (0.25, 0.0, 3.0, 2.0) and flags[1] == frx.MAPDIST_FLAG_OUTSIDE                      # the earlier of equal pieces; 0.25 is not below 0.25
    assert tuple(cand[2]) == (0.0, 0.0, 0.0, 0.0) and flags[2] == 0                                              # no pieces: the row stays, no flag
    assert tuple(cand[3]) == (np.inf, -1.0, -1.0, 5.0) and flags[3] == frx.MAPDIST_FLAG_OUTSIDE | frx.MAPDIST_FLAG_NONFINITE
    assert frx.map_distance_fold(rows, T, [0, 3, 5, 5, 6], 0.2500001)[1][1] == frx.MAPDIST_FLAG_OUTSIDE | frx.MAPDIST_FLAG_BELOW


@pytest.mark.parametrize("k", [0, 1])
def test_pinned_to_the_reference_itself(frx, k):
    """tests/golden/refpin_esdf_*.npz: the three buffers MapUtil<3>::updateESDF3d itself left on two maps that hold both kinds of site (recorded by
    scripts/esdf_ref_record.cpp).  Data only; bit for bit."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"refpin_esdf_{k}.npz"))
    cells = g["cells"]
    assert (cells > 0).any() and (cells == 0).any() and (cells == -1).any()
    got = frx.VoxelMap([0.0, 0.0, 0.0], g["dim"], float(g["res"]), cells).esdf()
    ref = er.fields(cells, g["dim"], float(g["res"]))
    for key in KEYS:
        assert er.same_bits(got[key], g[key]) and er.same_bits(ref[key], g[key]), key
    assert (g["neg"] > float(g["res"])).any() == (k == 1) and ((g["pos"] > 0) & (g["neg"] > 0)).any()
