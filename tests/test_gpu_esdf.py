"""frx_map_esdf_device and frx_map_mark_cloud_device against their host forms, bit for bit (uint64 / int8): on every crafted map (tests/esdf_states.py) twice
in a row, on a caller's stream, captured into a graph and replayed, with each output NULL; the blocking form; the cloud sizes at the edges of a wave; and the
chain cloud -> mark -> field on the device against the same chain on the host."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esdf_reference as er  # noqa: E402
import esdf_states as es  # noqa: E402
from test_gpu_trajectory_sample import DevBuf, hip  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("pos", "neg", "all")
SENTINEL = -7.0
PAD = 64                                                                  # sentinel doubles behind every output, sentinel ints behind the scratch


@pytest.fixture(scope="module")
def host(frx):
    """frx_map_esdf of every state: computed once, shared, left unchanged"""
    out = {}
    for label, dim, res, cells in es.all_states():
        f = frx.VoxelMap([0.0, 0.0, 0.0], dim, res, cells).esdf()
        for v in f.values():
            v.setflags(write=False)
        out[label] = f
    return out


def device_fields(frx, dim, res, cells, keys=KEYS, stream=0, launch=None, repeat=1):
    """The named fields from the device form; outputs and scratch are pre-filled with a sentinel and nothing is written behind either at the size the
    workspace query reports.  launch(call) runs the enqueueing call (default: directly), `repeat` times into the same buffers."""
    n = int(np.prod(dim))
    nbytes = frx.map_esdf_workspace(dim)
    assert nbytes == 4 * (4 * n + dim[0] + 1 + 2 * dim[0] * dim[1])
    whost = np.full(nbytes // 4 + PAD, -7, np.int32)
    ohost = np.full(n + PAD, SENTINEL)
    bufs = {"cells": DevBuf(np.ascontiguousarray(cells, dtype=np.int8)), "work": DevBuf(whost)}
    for k in keys:
        bufs[k] = DevBuf(ohost)
    try:
        ms = frx.VoxelMap([0.0, 0.0, 0.0], dim, res).device_struct(bufs["cells"].p)

        def call():
            frx.map_esdf_device(ms, *[bufs[k].p if k in keys else 0 for k in KEYS], bufs["work"].p, stream)
        out = None
        for _ in range(repeat):
            (launch or (lambda f: f()))(call)
            got = {k: bufs[k].get(ohost) for k in keys}
            assert all((g[n:] == SENTINEL).all() for g in got.values()) and (bufs["work"].get(whost)[nbytes // 4:] == -7).all()
            got = {k: g[:n] for k, g in got.items()}
            assert out is None or all(er.same_bits(out[k], got[k]) for k in keys)               # run to run
            out = got
        return out
    finally:
        for d in bufs.values():
            d.close()


def assert_same(got, want, label):
    for k in got:
        assert er.same_bits(got[k], want[k]), (label, k, np.flatnonzero(got[k].view(np.uint64) != want[k].view(np.uint64))[:5])


def test_every_state_twice_in_a_row(frx, host):
    for label, dim, res, cells in es.all_states():
        assert_same(device_fields(frx, dim, res, cells, repeat=2), host[label], label)


def test_every_state_on_a_callers_stream(frx, host):
    H = hip()
    st = C.c_void_p()
    assert H.hipStreamCreate(C.byref(st)) == 0
    try:
        for label, dim, res, cells in es.all_states():
            assert_same(device_fields(frx, dim, res, cells, stream=st.value), host[label], label)
    finally:
        H.hipStreamDestroy(st)


def test_every_state_captured_and_replayed(frx, host):
    """pure launches: five kernel nodes, and a replay gives the host's bits"""
    H = hip()
    st = C.c_void_p()
    assert H.hipStreamCreate(C.byref(st)) == 0
    try:
        for label, dim, res, cells in es.all_states():
            graph, exe, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
            try:
                def launch(call):
                    assert H.hipStreamBeginCapture(st, 0) == 0                                 # hipStreamCaptureModeGlobal
                    call()
                    assert H.hipStreamEndCapture(st, C.byref(graph)) == 0
                    assert H.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 5
                    assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
                    for _ in range(2):
                        assert H.hipGraphLaunch(exe, st) == 0 and H.hipStreamSynchronize(st) == 0
                assert_same(device_fields(frx, dim, res, cells, stream=st.value, launch=launch), host[label], label)
            finally:
                if exe.value:
                    H.hipGraphExecDestroy(exe)
                if graph.value:
                    H.hipGraphDestroy(graph)
    finally:
        H.hipStreamDestroy(st)


def test_every_state_with_each_output_null(frx, host):
    for label, dim, res, cells in es.all_states():
        for drop in KEYS:
            keys = tuple(k for k in KEYS if k != drop)
            assert_same(device_fields(frx, dim, res, cells, keys=keys), host[label], (label, drop))
        for k in KEYS:
            assert_same(device_fields(frx, dim, res, cells, keys=(k,)), host[label], (label, k))


def test_blocking_form_and_the_line_limit(frx, host):
    for label, dim, res, cells in es.all_states():
        m = frx.VoxelMap([0.0, 0.0, 0.0], dim, res, cells)
        assert_same(m.esdf_on_device(), host[label], label)
        assert_same(m.esdf_on_device(("neg",)), host[label], label)
    one_more = frx.VoxelMap([0.0, 0.0, 0.0], (es.LIMIT + 1, 1, 1), 0.1)
    with pytest.raises(frx.FrxError) as e:
        one_more.esdf_on_device()
    assert e.value.code == -5
    with pytest.raises(frx.FrxError) as e:
        frx.map_esdf_workspace((es.LIMIT + 1, 1, 1))
    assert e.value.code == -5


# ---- the cloud ----
DIM, RES, ORIGIN = (20, 13, 7), 0.1, (-1.0, -0.65, 0.25)


def cloud(rng, n):
    """points in a box a cell wider than the map on every side (so some are outside), every fourth on a cell border, a few far away"""
    lo = np.array(ORIGIN) - RES
    hi = np.array(ORIGIN) + RES * (np.array(DIM) + 1)
    p = rng.uniform(lo, hi, (n, 3))
    k = rng.integers(-1, np.array(DIM) + 2, (n, 3))
    border = np.array(ORIGIN) + RES * k                                  # on a border to within a rounding: either cell, the same one on host and device
    p[::4, 0] = border[::4, 0]; p[1::8, 1] = border[1::8, 1]; p[2::8, 2] = border[2::8, 2]
    if n >= 8:
        p[5] = (1e6, 0.0, 0.5); p[6] = (0.0, -1e6, 0.5)
    return np.ascontiguousarray(p)


def mark_on_device(frx, start, pts, stream=0):
    m = frx.VoxelMap(ORIGIN, DIM, RES)
    pad = np.full(PAD, 55, np.int8)
    bufs = [DevBuf(np.concatenate([start, pad])), DevBuf(pts.reshape(-1) if len(pts) else np.zeros(3)), DevBuf(np.array([-9, 77], np.int32))]
    try:
        frx.map_mark_cloud_device(m.device_struct(), bufs[0].p, len(pts), bufs[1].p if len(pts) else 0, bufs[2].p, stream)
        cells = bufs[0].get(np.concatenate([start, pad])); cnt = bufs[2].get(np.zeros(2, np.int32))
        assert (cells[len(start):] == 55).all() and cnt[1] == 77
        return cells[:len(start)], int(cnt[0])
    finally:
        for d in bufs:
            d.close()


@pytest.mark.parametrize("n_pts", [0, 1, 63, 64, 65, 1000])
def test_mark_cloud_equals_the_host(frx, n_pts):
    rng = np.random.default_rng(n_pts)
    start = rng.choice(np.array([-1, 0, 0, 3], np.int8), int(np.prod(DIM)))
    pts = cloud(rng, n_pts)
    m = frx.VoxelMap(ORIGIN, DIM, RES, start.copy())
    inside = m.mark_cloud(pts)
    cells, cnt = mark_on_device(frx, start, pts)
    assert np.array_equal(cells, m.cells) and cnt == inside
    assert n_pts < 63 or (0 < inside < n_pts and (m.cells == 100).sum() > 0)                   # points inside and points outside
    again = mark_on_device(frx, start, pts)
    assert np.array_equal(again[0], cells) and again[1] == cnt


def test_cloud_to_field_on_the_device_equals_the_host_chain(frx):
    rng = np.random.default_rng(9)
    pts = cloud(rng, 300)
    m = frx.VoxelMap(ORIGIN, DIM, RES)
    m.mark_cloud(pts)
    want = m.esdf()
    n = int(np.prod(DIM))
    nbytes = frx.map_esdf_workspace(DIM)
    bufs = dict(cells=DevBuf(np.zeros(n, np.int8)), pts=DevBuf(pts.reshape(-1)), cnt=DevBuf(np.zeros(1, np.int32)), work=DevBuf(np.zeros(nbytes // 4, np.int32)),
                pos=DevBuf(np.zeros(n)), neg=DevBuf(np.zeros(n)), all=DevBuf(np.zeros(n)))
    H = hip()
    st = C.c_void_p()
    assert H.hipStreamCreate(C.byref(st)) == 0
    try:
        ms = m.device_struct(bufs["cells"].p)
        frx.map_mark_cloud_device(ms, bufs["cells"].p, len(pts), bufs["pts"].p, bufs["cnt"].p, st.value)       # one stream, no synchronisation in between
        frx.map_esdf_device(ms, bufs["pos"].p, bufs["neg"].p, bufs["all"].p, bufs["work"].p, st.value)
        assert H.hipStreamSynchronize(st) == 0
        assert np.array_equal(bufs["cells"].get(m.cells), m.cells)
        assert_same({k: bufs[k].get(want[k]) for k in KEYS}, want, "chain")
    finally:
        H.hipStreamDestroy(st)
        for d in bufs.values():
            d.close()
