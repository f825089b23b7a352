"""States of the clearance check against the obstacle cloud (frx_trajectory_clearance, frx_clear_kernel.hpp) - test infrastructure, not a test
module.

The kernel's launch rule (frx_traj_host.hpp: cloud_split with the constants of frx_device.hpp), restated here as chunks(P, n_obs, force): the cloud is split into chunks of whole
passes of PASS = 1024 points so that P x chunks reaches 2048 workgroups (one chunk when P alone does); force > 0 = that many points per chunk.
A workgroup holds TILE = 64 sample states at a time.

  random states    random quintics over random durations, candidates of uneven length, a cloud around the origin.
  exact states     grav_acc = 8, horiz_half_len = 1/2, vert_half_len = 1/8 and pieces of zero acceleration: zB = e3, R = I exactly in the
                   device's frame arithmetic (rsqrt of 64 and of 1 are exact) and dyadic points make every q exact, so ties are ties.
  loop state       a random cloud, frx_line_segment_dilate cells along a polyline, one straight constant-velocity piece per segment, and an
                   ellipsoid shrunk until at least half of the pieces lie inside their cells by check_reference.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_reference as cr  # noqa: E402

TILE, PASS, TARGET_WGS = 64, 1024, 2048
LOOSE = dict(vel_max=1e4, thr_acc_min=0.0, thr_acc_max=1e4, body_rate_max=1e4)
EXACT = dict(grav_acc=8.0, vert_half_len=0.125, horiz_half_len=0.5, safe_margin=0.0625)
BOX = np.concatenate([np.vstack([np.eye(3), 50.0 * np.eye(3)]), np.vstack([-np.eye(3), -50.0 * np.eye(3)])], axis=1)    # |x|, |y|, |z| <= 50


def chunks(P, n_obs, force=0):
    """(points per chunk, chunks per piece) of a clearance launch."""
    c = force
    if force <= 0:
        want = TARGET_WGS // P if P < TARGET_WGS else 1
        c = -(-n_obs // want)
        c = -(-c // PASS) * PASS
    return min(c, n_obs), -(-n_obs // c)


def quintics(rng, P):
    """Random pieces with |a| well below g: T (P,), Cf (6P, 3)."""
    T = rng.uniform(0.4, 1.6, P)
    C = rng.normal(0.0, 1.0, (P, 6, 3)) * np.array([2.0, 1.0, 0.4, 0.2, 0.1, 0.05])[None, :, None]
    return T, C.reshape(-1, 3)


def cloud(rng, n):
    return rng.uniform(-6.0, 6.0, (n, 3))


def counts_of(P):
    """Uneven candidates: P = 1 -> [1], 2 -> [2], 5 -> [2, 3] (a ragged two-candidate batch), else halves."""
    return [P] if P < 3 else [P // 2, P - P // 2]


def handle(frx, params, counts, polys=None):
    """A PenaltyProblem of sum(counts) pieces; every piece in the wide box unless polys (one per piece) are given."""
    P = int(sum(counts))
    if polys is None:
        return frx.PenaltyProblem(params, counts, [0] * P, [BOX], qd_intervals=8)
    return frx.PenaltyProblem(params, counts, list(range(P)), polys, qd_intervals=8)


def exact_params(base):
    p = dict(base)
    p.update(LOOSE)
    p.update(EXACT)
    return p


def still_piece(at):
    """A piece that stays at `at`: level attitude."""
    c = np.zeros((6, 3))
    c[0] = at
    return c


def line_piece(a, b, T):
    """A straight constant-velocity piece from a to b in T: level attitude."""
    c = np.zeros((6, 3))
    c[0] = a
    c[1] = (np.asarray(b, dtype=np.float64) - np.asarray(a, dtype=np.float64)) / T
    return c


def loop_state(frx, base, seed=4, n_obs=1500, n_seg=12):
    """dict(params, T, Cf, obs, polys, inside): the closing-the-loop state.  inside[i]: check_reference puts piece i inside its cell at LOOP_M."""
    rng = np.random.default_rng(seed)
    obs = np.concatenate([rng.uniform(-1.0, 25.0, (n_obs, 1)), rng.uniform(-6.0, 6.0, (n_obs, 1)), rng.uniform(0.0, 5.0, (n_obs, 1))], axis=1)
    way = np.stack([np.linspace(0.0, 24.0, n_seg + 1), 2.0 * np.sin(np.linspace(0.0, 5.0, n_seg + 1)), 2.5 + 0.8 * np.cos(np.linspace(0.0, 7.0, n_seg + 1))], axis=1)
    obs = obs[np.array([np.min(np.linalg.norm(way - o, axis=1)) > 0.6 for o in obs])]       # keep the waypoints themselves free
    bbox = np.array([2.0, 2.0, 1.0])
    polys = [frx.line_segment_dilate(way[k], way[k + 1], bbox, obs)[0] for k in range(n_seg)]
    T = np.full(n_seg, 1.5)
    Cf = np.concatenate([line_piece(way[k], way[k + 1], T[k]) for k in range(n_seg)])
    params = dict(base)
    params.update(LOOSE)
    scale = 1.0
    while True:                                                         # shrink the ellipsoid until at least half of the pieces fit
        params.update(horiz_half_len=0.5 * scale, vert_half_len=0.15 * scale)
        rows = cr.check_pieces(T, Cf, polys, params, LOOP_M)
        inside = rows[:, 0] <= 0.0
        if 2 * inside.sum() >= n_seg or scale < 1e-3:
            break
        scale *= 0.5
    return dict(params=params, T=T, Cf=Cf, obs=np.ascontiguousarray(obs), polys=polys, inside=inside, counts=[n_seg])


LOOP_M = 32
