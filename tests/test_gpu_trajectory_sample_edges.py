"""frx_trajectory_sample at the edges of its tiling and of its attitude branches, against tests/sample_reference.py (assert_rows and TOL of
test_gpu_trajectory_sample).

The launcher's rule (frx_device_sample.hip: launch_sample), restated as passes_rule(B, S): a workgroup takes `passes` tiles of 256 consecutive
samples of one candidate; passes starts at 4 and is halved while B x ceil(tiles / passes) < 2048 workgroups, tiles = ceil(S / 256); a
candidate has chunks = ceil(tiles / passes) workgroups.  A wave owns 64 rows of a tile and leaves the pass loop at its first tile that
starts at or past S; a tile that straddles S is stored up to row S - 1.
  B = 2048, S = 300    passes 4, 1 chunk: pass 1 holds the partial tile 256 .. 299, passes 2 and 3 break
  B = 2048, S = 1281   passes 4, 2 chunks: the second chunk's pass 1 holds one row (1280), then it breaks
  B = 2047, S = 700    passes 2, 2 chunks (2047 < 2048 <= 2 x 2047: the only way to two passes is three or four tiles and B in 1024 .. 2047)
  B = 2047, S = 300    passes 1 by the same rule (2047 x 1 < 2048 at four and at two passes), S = 1281: passes 4
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_reference as sr  # noqa: E402
from test_gpu_trajectory_sample import DevBuf, G, assert_rows  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
PAD = 64                                                              # sentinel doubles behind a device output
BOX = np.concatenate([np.vstack([np.eye(3), 1e3 * np.ones((3, 3))]), np.vstack([-np.eye(3), -1e3 * np.ones((3, 3))])], axis=1)


def passes_rule(B, S):
    """(passes, chunks) of a launch."""
    tiles = (S + 255) // 256
    passes = 4
    while passes > 1 and B * ((tiles + passes - 1) // passes) < 2048:
        passes //= 2
    return passes, (tiles + passes - 1) // passes


def device_rows(prob, T, Cf, S, times=None, **kw):
    """Rows of the device form and the PAD doubles behind them, the whole buffer pre-filled with a sentinel."""
    n = prob.B * S * 20
    host = np.full(n + PAD, SENTINEL)
    bufs = [DevBuf(T), DevBuf(np.ascontiguousarray(Cf).reshape(-1)), DevBuf(host)]
    if times is not None:
        bufs.append(DevBuf(times))
        kw["times_ptr"] = bufs[3].p
    try:
        prob.trajectory_sample_device(bufs[0].p, bufs[1].p, bufs[2].p, S, **kw)
        out = bufs[2].get(host)
    finally:
        for d in bufs:
            d.close()
    return out[:n].reshape(prob.B, S, 20), out[n:]


@pytest.fixture(scope="module")
def ragged(frx, sc):
    counts = [1, 3, 64, 65, 7]
    prob = frx.PenaltyProblem(sc.ZHANGJIAJIE, counts, [0] * sum(counts), [BOX], qd_intervals=8)
    rng = np.random.default_rng(17)
    T = rng.uniform(0.05, 0.4, prob.P)
    Cf = rng.normal(0.0, 2.0, (6 * prob.P, 3))
    yield prob, T, Cf
    prob.close()


@pytest.mark.parametrize("S", [2, 63, 64, 65, 255, 256, 257, 513])
def test_tile_edges(ragged, S):
    """One wave short of, at and past its 64 rows; one tile short of, at and past its 256; two tiles and a row (513: B = 5, so one pass each)."""
    prob, T, Cf = ragged
    assert passes_rule(prob.B, S)[0] == 1
    got = prob.trajectory_sample(T, Cf, S)["rows"]
    assert_rows(got, sr.sample_batch(T, Cf, prob.piece_off, S, G))
    dev, pad = device_rows(prob, T, Cf, S)
    assert np.array_equal(dev, got) and (pad == SENTINEL).all()


def test_one_sample(ragged):
    """S = 1 exists in the dt and times forms only: every candidate's tile holds one row."""
    prob, T, Cf = ragged
    times = np.array([[0.03], [0.2], [3.0], [1e9], [np.nan]])
    for kw in (dict(dt=0.25, t0=0.07), dict(times=times)):
        got = prob.trajectory_sample(T, Cf, 1, **kw)["rows"]
        assert got.shape == (prob.B, 1, 20)
        assert_rows(got, sr.sample_batch(T, Cf, prob.piece_off, 1, G, **kw))
        dev, pad = device_rows(prob, T, Cf, 1, **kw)
        assert np.array_equal(dev, got, equal_nan=True) and (pad == SENTINEL).all()


@pytest.fixture(scope="module")
def many(frx, sc):
    """2048 one-piece candidates - the smallest batch for which the launcher keeps four passes - and its first 2047."""
    rng = np.random.default_rng(23)
    T = rng.uniform(0.05, 0.4, 2048)
    Cf = rng.normal(0.0, 2.0, (6 * 2048, 3))
    probs = {B: frx.PenaltyProblem(sc.ZHANGJIAJIE, [1] * B, [0] * B, [BOX], qd_intervals=8) for B in (2048, 2047)}
    yield probs, T, Cf
    for p in probs.values():
        p.close()


# (the largest case holds 2048 x 1281 x 20 doubles = 420 MB on the device and on the host: the size the break after a partial tile in a
# workgroup's second chunk needs at four passes)
@pytest.mark.parametrize("B,S,passes,chunks", [(2048, 300, 4, 1), (2048, 1281, 4, 2), (2047, 700, 2, 2), (2047, 300, 1, 2), (2047, 1281, 4, 2)],
                         ids=["B2048-S300-passes4", "B2048-S1281-passes4", "B2047-S700-passes2", "B2047-S300-passes1", "B2047-S1281-passes4"])
def test_several_passes_per_workgroup(many, B, S, passes, chunks):
    probs, T, Cf = many
    prob = probs[B]
    assert passes_rule(B, S) == (passes, chunks) and prob.B == B
    T, Cf = T[:B], Cf[:6 * B]
    rows = prob.trajectory_sample(T, Cf, S)["rows"]
    assert rows.shape == (B, S, 20) and np.isfinite(rows).all()
    pick = sorted(set(np.random.default_rng(S).choice(B, 24, replace=False)) | {0, B - 1})
    assert_rows(rows[pick], sr.sample_batch(T, Cf, prob.piece_off, S, G, cands=pick))


# ---- attitude branches ----
S_ATT = 33                                                            # t = s / 32, s = 0 .. 32: exact times over pieces of one second
ATTITUDES = (                                                          # name, acceleration at t = 0, jerk
    ("up", (0.0, 0.0, 0.0), (0.5, -0.25, 0.125)),                      # zB = e3 exactly at t = 0
    ("tilted", (3.0, -2.0, 1.0), (1.0, 1.0, -1.0)),
    ("horizontal", (4.0, 3.0, -G), (0.5, 0.25, 0.0)),                  # zB.z = 0 exactly throughout: the trace ties with R00
    ("below", (2.0, -3.0, -1.5 * G), (1.0, 0.5, -2.0)),                # zB.z < 0: the R00 branch
    ("down", (0.0, 0.0, -2.0 * G), (0.5, 0.25, 0.0)),                  # zB = -e3 exactly at t = 0
)
DEGENERATE = (("plus_e1", (5.0, 0.0, -G), (1.0, 0.0, 0.0)), ("minus_e1", (-5.0, 0.0, -G), (-1.0, 0.0, 0.0)))   # |(0, zB.z, -zB.y)| = 0 throughout


def attitude_batch(cases):
    """One one-piece candidate per case: p0 and v0 arbitrary, c2 = a / 2, c3 = j / 6.  Counts the quaternion branches of the restatement."""
    rng = np.random.default_rng(29)
    Cf = np.zeros((6 * len(cases), 3))
    for i, (_, a, j) in enumerate(cases):
        Cf[6 * i] = rng.normal(0.0, 2.0, 3)
        Cf[6 * i + 1] = rng.normal(0.0, 2.0, 3)
        Cf[6 * i + 2] = np.array(a) / 2.0
        Cf[6 * i + 3] = np.array(j) / 6.0
    T = np.ones(len(cases))
    off = np.arange(len(cases) + 1)
    ref = sr.sample_batch(T, Cf, off, S_ATT, G, dt=1.0 / 32.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        _, R, m = sr.frame(ref[..., 6:9].reshape(-1, 3), G)
    R00, R11, R22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    tr = R00 + R11 + R22
    k0 = (tr >= R00) & (tr >= R11) & (tr >= R22)
    k1 = ~k0 & (R00 >= R11) & (R00 >= R22)
    k2 = ~k0 & ~k1 & (R11 >= R22)
    k3 = ~k0 & ~k1 & ~k2 & np.isfinite(tr)
    counts = dict(trace=int(k0.sum()), R00=int(k1.sum()), R11=int(k2.sum()), R22=int(k3.sum()), tie=int((k0 & (tr == R00)).sum()))
    return T, Cf, off, ref, counts, R.reshape(len(cases), S_ATT, 3, 3)


def test_attitude_branches(frx, sc):
    T, Cf, off, ref, counts, R = attitude_batch(ATTITUDES)
    assert counts["trace"] >= 2 * S_ATT and counts["R00"] >= 2 * S_ATT and counts["R11"] == 0 and counts["R22"] == 0, counts
    assert counts["tie"] >= S_ATT                                     # (the horizontal piece: trace = R00 at every sample)
    assert np.array_equal(R[0, 0, :, 2], [0.0, 0.0, 1.0]) and np.array_equal(R[4, 0, :, 2], [0.0, 0.0, -1.0]) and (R[2, :, 2, 2] == 0.0).all()
    assert (R[3, :, 2, 2] < 0.0).all() and np.isfinite(ref).all()
    n = len(ATTITUDES)
    prob = frx.PenaltyProblem(sc.ZHANGJIAJIE, [1] * n, [0] * n, [BOX], qd_intervals=8)
    try:
        got = prob.trajectory_sample(T, Cf, S_ATT, dt=1.0 / 32.0)["rows"]
    finally:
        prob.close()
    assert_rows(got, ref)
    assert (got[..., 13] >= 0.0).all() and np.abs(np.linalg.norm(got[..., 13:17], axis=2) - 1.0).max() <= 1e-12
    assert np.abs(got[..., 17:20]).max() > 0.01                       # (the body rates are not trivially zero)


def test_degenerate_frame(frx, sc):
    """zB = +/- e1: the frame's yB = (0, zB.z, -zB.y) / 0 does not exist.  The quaternion and the body rates are not numbers, exactly where
    the restatement's are not; the flat outputs and the thrust are, and the other candidates' rows are bit for bit those of a batch without
    the degenerate ones."""
    cases = ATTITUDES[:2] + DEGENERATE[:1] + ATTITUDES[2:] + DEGENERATE[1:]
    T, Cf, off, ref, _, _ = attitude_batch(cases)
    deg = [2, len(cases) - 1]
    keep = [i for i in range(len(cases)) if i not in deg]
    assert np.isfinite(ref[keep]).all() and np.isfinite(ref[deg][..., :13]).all() and np.isnan(ref[deg][..., 13:]).all()
    n = len(cases)
    prob = frx.PenaltyProblem(sc.ZHANGJIAJIE, [1] * n, [0] * n, [BOX], qd_intervals=8)
    clean = frx.PenaltyProblem(sc.ZHANGJIAJIE, [1] * len(keep), [0] * len(keep), [BOX], qd_intervals=8)
    try:
        got = prob.trajectory_sample(T, Cf, S_ATT, dt=1.0 / 32.0)["rows"]
        rows = np.concatenate([Cf[6 * i:6 * i + 6] for i in keep])
        alone = clean.trajectory_sample(T[keep], rows, S_ATT, dt=1.0 / 32.0)["rows"]
    finally:
        prob.close()
        clean.close()
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    assert_rows(got, ref)
    assert np.array_equal(got[keep], alone)
