"""Generates tests/golden/refpin_extrema_max_rates.npz: Piece::getMaxVelRate / getMaxAccRate of the REFERENCE (oracle/_ref/libref_traj.so, its
trajectory.hpp + root_finder.hpp compiled unmodified) on 200 random quintics - all six coefficient rows non-zero, so the reference never reports its 0
for a constant magnitude - with T in [0.05, 3].  Data only: T (200,), C (200, 6, 3) as frx_optimize lays coefficients out, max_vel, max_acc (200,).
tests/test_gpu_trajectory_extrema.py holds frx_trajectory_extrema's SPEED and ACC against them.  Run from the repo root after build():
    python tests/golden/make_extrema_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import binding as ob  # noqa: E402
import extrema_states as es  # noqa: E402

SEED, COUNT = 20261019, 200


def main():
    if ob.ref_traj() is None:
        raise SystemExit("oracle/_ref/libref_traj.so not built: nothing to record")
    pieces = es.random_quintics(np.random.default_rng(SEED), COUNT)
    T = np.array([t for t, _ in pieces])
    Cp = np.array([c for _, c in pieces])
    assert (np.abs(Cp).max(axis=2) > 0).all()
    pl = ob.piece_layout(Cp.reshape(-1, 3))
    mv, ma = np.zeros(COUNT), np.zeros(COUNT)
    for i in range(COUNT):
        out = np.zeros(2)
        ob.ref_traj().ref_piece_max_rates(float(T[i]), np.ascontiguousarray(pl[i].reshape(-1)), out)
        mv[i], ma[i] = out
    assert (mv > 0).all() and (ma > 0).all()
    path = os.path.join(ROOT, "tests", "golden", "refpin_extrema_max_rates.npz")
    np.savez_compressed(path, T=T, C=Cp, max_vel=mv, max_acc=ma)
    print(f"wrote {path}: {COUNT} pieces, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
