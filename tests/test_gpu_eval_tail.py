"""The tail of the one-launch evaluation (k_eval_cluster, frx_eval_kernel.hpp): thread 0 of a cluster's leader stores f and the tag of the completed evaluation
(`done`) from inside the adjoint, right behind the objective's sum - no workgroup barrier, no load of the global status word in front of them; whether a wait for
the penalty partials ended without them comes out of a word in the leader's LDS.  Checked here, through the public Problem API with the cluster form on: the values
at the smallest shapes where the tail can go wrong, the tags over evaluations that follow each other on a stream without a synchronisation, the verdict of an
expired wait, and the sticky status word of an earlier launch."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-10           # one launch against three stage launches, per candidate: |g1 - g3|max <= 1e-10 max(|g3|max, |f3|) - the bound of tests/test_gpu_parity.py for these two forms
FRX_ERR_TIMEOUT = -7       # include/frx.h

_hip = None


def hip():
    """The HIP runtime libfrx.so itself uses."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so.7")
        for name in ("hipMalloc", "hipMemcpy", "hipFree", "hipStreamCreate", "hipStreamDestroy", "hipStreamSynchronize", "hipStreamBeginCapture", "hipStreamEndCapture",
                     "hipGraphInstantiate", "hipGraphLaunch", "hipGraphExecDestroy", "hipGraphDestroy", "hipDeviceSynchronize"):
            getattr(_hip, name).restype = C.c_int
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
        _hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.c_void_p]
        _hip.hipGraphInstantiate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        _hip.hipGraphLaunch.argtypes = [C.c_void_p, C.c_void_p]
        for name in ("hipStreamDestroy", "hipStreamSynchronize", "hipGraphExecDestroy", "hipGraphDestroy", "hipFree"):
            getattr(_hip, name).argtypes = [C.c_void_p]
    return _hip


class DevBuf:
    def __init__(self, host):
        self.host = np.ascontiguousarray(host, dtype=np.float64)
        self.ptr = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.ptr), C.c_size_t(self.host.nbytes)) == 0
        assert hip().hipMemcpy(self.ptr, self.host.ctypes.data, self.host.nbytes, 1) == 0   # hipMemcpyHostToDevice

    @property
    def p(self):
        return self.ptr.value

    def get(self):
        out = np.empty_like(self.host)
        assert hip().hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2) == 0              # hipMemcpyDeviceToHost (the caller has synchronised)
        return out

    def close(self):
        if self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = None


class Stream:
    def __init__(self):
        self.st = C.c_void_p()
        assert hip().hipStreamCreate(C.byref(self.st)) == 0

    def sync(self):
        assert hip().hipStreamSynchronize(self.st) == 0

    def close(self):
        hip().hipStreamDestroy(self.st)


# pieces per candidate, samples per piece: one waypoint and one active knot | the first shape whose lane shifts carry data | unequal candidates | the full wave
SHAPES = {"one_waypoint": ((2,), 8), "first_lane_shift": ((3,), 16), "unequal": ((5, 3, 4), 16), "full_wave": ((64, 64), 16)}
_handles = {}


def handle(frx, sc, name):
    """One handle per shape for the whole module, with its point and the values of the one-launch form there (computed once, never changed)."""
    if name not in _handles:
        pieces, kappa = SHAPES[name]
        cands = [sc.make_candidate(0, n, n // 4 if n >= 8 else 0, perturb_id=b) for b, n in enumerate(pieces)]   # (short candidates: one gate 4 m per piece ahead)
        prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=kappa)
        x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
        fused = prob.eval_fused()
        f, g = prob.objective(x) if fused else (None, None)
        _handles[name] = (prob, x, f, g, fused)
    prob, x, f, g, fused = _handles[name]
    if not fused:
        pytest.skip("the cluster form does not apply to this handle")
    assert prob.eval_fused() == fused
    return prob, x, f, g


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for prob, *_ in _handles.values():
        prob.close()
    _handles.clear()


@pytest.mark.parametrize("name", list(SHAPES))
def test_values_against_the_three_stage_form(frx, sc, name):
    prob, x, f, g = handle(frx, sc, name)
    prob.set_eval_fused(False)
    try:
        f3, g3 = prob.objective(x)
    finally:
        prob.set_eval_fused(True)
    assert np.all(np.isfinite(f)) and np.array_equal(f, f3)
    for b in range(prob.B):
        sl = slice(prob.x_off[b], prob.x_off[b + 1])
        err, scale = np.abs(g[sl] - g3[sl]).max(), max(np.abs(g3[sl]).max(), abs(f3[b]))
        print(f"{name} candidate {b}: gradient differs by {err:.3e}, scale {scale:.3e}")
        assert err <= GRAD_TOL * scale, (name, b)
    f1, g1 = prob.objective(x)                                       # and the cluster form again behind the stage launches: the same bits as before
    assert np.array_equal(f1, f) and np.array_equal(g1, g)


def test_tags_hold_over_evaluations_without_a_synchronisation(frx, sc):
    """Five evaluations at five points back to back on one stream, nothing on the host between them: each leaves what the same call leaves with a synchronisation
    behind it.  A `done` stored before its evaluation's partials are in, or an f stored by the wrong evaluation, shows here."""
    prob, x, _, _ = handle(frx, sc, "full_wave")
    xs = [x + 2e-3 * k * np.cos(np.arange(prob.NX) + k) for k in range(5)]
    st = Stream()
    xd = [DevBuf(v) for v in xs]
    fd = [[DevBuf(np.zeros(prob.B)) for _ in xs] for _ in range(2)]
    gd = [[DevBuf(np.zeros(prob.NX)) for _ in xs] for _ in range(2)]
    try:
        for k in range(5):                                           # the reference: a synchronisation after every call
            prob.objective_device(xd[k].p, fd[0][k].p, gd[0][k].p, st.st.value)
            st.sync()
        for k in range(5):
            prob.objective_device(xd[k].p, fd[1][k].p, gd[1][k].p, st.st.value)
        st.sync()
        prob.eval_status()
        assert prob.eval_fused() > 0
        want = [(fd[0][k].get(), gd[0][k].get()) for k in range(5)]
        for k in range(5):
            assert np.all(np.isfinite(want[k][0])) and np.abs(want[k][1]).max() > 0
            assert np.array_equal(fd[1][k].get(), want[k][0]) and np.array_equal(gd[1][k].get(), want[k][1]), k
        assert not np.array_equal(want[0][0], want[4][0])            # five different points
    finally:
        for b in xd + fd[0] + fd[1] + gd[0] + gd[1]:
            b.close()
        st.close()


def _expired_handle(frx, sc, monkeypatch):
    monkeypatch.setenv("FRX_EVAL_TIMEOUT_MS", "5")                   # (the injected mode below bounds the leaders' waits at 50 us by itself)
    cands = [sc.make_candidate(0, 5, 0, perturb_id=b) for b in range(2)]
    prob = frx.Problem(cands, sc.ZHANGJIAJIE, qd_intervals=16)
    if not prob.eval_fused():
        prob.close()
        pytest.skip("the cluster form does not apply to this handle")
    x = prob.initial_guess() + 1e-3 * np.sin(np.arange(prob.NX))
    return prob, x, prob.objective(x)


def test_verdict_of_an_expired_wait(frx, sc, monkeypatch):
    """The injected mode: the members leave at once and the leaders' bounded waits for the partials expire by design.  Every f is NaN, the blocking entry reports
    FRX_ERR_TIMEOUT, frx_eval_status returns the code once, and the next evaluation in the normal mode gives the values from before."""
    prob, x, (f_ok, g_ok) = _expired_handle(frx, sc, monkeypatch)
    st, xd, fd, gd = Stream(), DevBuf(x), DevBuf(np.zeros(prob.B)), DevBuf(np.zeros(prob.NX))
    try:
        assert np.all(np.isfinite(f_ok))
        prob.set_eval_fused(2)
        prob.objective_device(xd.p, fd.p, gd.p, st.st.value)
        st.sync()
        assert np.all(np.isnan(fd.get()))
        with pytest.raises(frx.FrxError) as ei:
            prob.eval_status()
        assert ei.value.code == FRX_ERR_TIMEOUT
        prob.eval_status()                                           # cleared
        prob.set_eval_fused(2)
        with pytest.raises(frx.FrxError) as ei:
            prob.objective(x)
        assert ei.value.code == FRX_ERR_TIMEOUT and "expired" in str(ei.value)
        prob.set_eval_fused(1)
        assert prob.eval_fused() > 0
        f1, g1 = prob.objective(x)
        assert np.array_equal(f1, f_ok) and np.array_equal(g1, g_ok)
    finally:
        for b in (xd, fd, gd):
            b.close()
        st.close()
        prob.close()


def test_sticky_status_word_of_an_earlier_launch(frx, sc, monkeypatch):
    """After an expired evaluation and before anybody has cleared the status word, a further launch of the cluster form - a replay of a graph captured while all was
    well: the launcher itself would go to the stage kernels - evaluates nothing and answers NaN for every candidate."""
    prob, x, (f_ok, g_ok) = _expired_handle(frx, sc, monkeypatch)
    H = hip()
    st, xd, fd, gd = Stream(), DevBuf(x), DevBuf(np.zeros(prob.B)), DevBuf(np.zeros(prob.NX))
    graph, exe = C.c_void_p(), C.c_void_p()
    try:
        assert H.hipStreamBeginCapture(st.st, 0) == 0                # hipStreamCaptureModeGlobal
        prob.objective_device(xd.p, fd.p, gd.p, st.st.value)
        assert H.hipStreamEndCapture(st.st, C.byref(graph)) == 0
        assert H.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        assert H.hipGraphLaunch(exe, st.st) == 0
        st.sync()
        assert np.array_equal(fd.get(), f_ok) and np.array_equal(gd.get(), g_ok)
        prob.set_eval_fused(2)
        prob.objective_device(xd.p, fd.p, gd.p, st.st.value)         # expires
        st.sync()
        assert np.all(np.isnan(fd.get()))
        assert H.hipMemcpy(fd.ptr, f_ok.ctypes.data, f_ok.nbytes, 1) == 0
        t0 = time.perf_counter()
        assert H.hipGraphLaunch(exe, st.st) == 0
        st.sync()
        print(f"replay against the sticky word: {1e3 * (time.perf_counter() - t0):.2f} ms")
        assert np.all(np.isnan(fd.get()))
        with pytest.raises(frx.FrxError) as ei:
            prob.eval_status()
        assert ei.value.code == FRX_ERR_TIMEOUT
        prob.set_eval_fused(1)
        assert H.hipGraphLaunch(exe, st.st) == 0                     # the word is clear again: the same graph evaluates
        st.sync()
        assert np.array_equal(fd.get(), f_ok) and np.array_equal(gd.get(), g_ok)
    finally:
        if exe.value:
            H.hipGraphExecDestroy(exe)
        if graph.value:
            H.hipGraphDestroy(graph)
        for b in (xd, fd, gd):
            b.close()
        st.close()
        prob.close()
