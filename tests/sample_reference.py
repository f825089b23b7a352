"""Independent numpy restatement of batched trajectory sampling (frx_trajectory_sample, include/frx.h) - test infrastructure, not a test module.
Written from the header's rules and the reference's flatness map (se3gcopter_cpu.hpp:260-299), not from the kernel's arithmetic:

  cum[0] = 0, cum[i + 1] = cum[i] + T[i] (left to right); t clamped to [0, cum[N]]; piece = first i with t <= cum[i + 1]; s = t - cum[i]
  pos / vel / acc / jer = d^m/ds^m of c^T (1, s, .., s^5)                                          (CPU.hpp:253-263)
  h = acc + gAcc e3;  zB = h / |h|;  yB = normalise(0, zB_z, -zB_y);  xB = yB x zB;  R = [xB yB zB]     (normalizeFDF, CPU.hpp:265-276)
  quaternion (w, x, y, z) of R: branch on the largest of (trace, R00, R11, R22), the earlier on a tie, then w >= 0
  omega = (-(yB.j), xB.j, -(xB_y dzB_z - xB_z dzB_y) / |(0, zB_z, -zB_y)|) with the first two over |h|, dzB = (j - zB (zB.j)) / |h|
"""
import numpy as np

FIELDS = 20
VIEWS = dict(pos=slice(0, 3), vel=slice(3, 6), acc=slice(6, 9), jerk=slice(9, 12), thrust=12, quat=slice(13, 17), omega=slice(17, 20))


def prefix_sums(T):
    cum = np.zeros(len(T) + 1)
    acc = 0.0
    for i, d in enumerate(np.asarray(T, dtype=np.float64)):
        acc = acc + float(d)
        cum[i + 1] = acc
    return cum


def sample_times(T, n_samples, dt=0.0, t0=0.0):
    """The times of the two modes without a times array, as the header defines them (products and sums rounded as written)."""
    s = np.arange(n_samples, dtype=np.float64)
    if dt > 0.0:
        return t0 + s * dt
    return s * (prefix_sums(T)[-1] / (n_samples - 1))


def locate(T, t):
    """(piece index, local time) of every time in t."""
    cum = prefix_sums(T)
    t = np.array(t, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        t = np.where(t < 0.0, 0.0, t)
        t = np.where(t > cum[-1], cum[-1], t)
    # first i with t <= cum[i + 1] (cum is non-decreasing); NaN sorts past the end and lands in the last piece
    i = np.minimum(np.searchsorted(cum[1:], t, side="left"), len(T) - 1)
    return i, t - cum[i]


def flat_state(c, s):
    """pos, vel, acc, jer (each (n, 3)) of the quintics c (n, 6, 3), row k = power k, at local times s (n,)."""
    s = np.asarray(s, dtype=np.float64)
    one, z = np.ones_like(s), np.zeros_like(s)
    betas = (np.stack([one, s, s ** 2, s ** 3, s ** 4, s ** 5], axis=1),
             np.stack([z, one, 2.0 * s, 3.0 * s ** 2, 4.0 * s ** 3, 5.0 * s ** 4], axis=1),
             np.stack([z, z, 2.0 * one, 6.0 * s, 12.0 * s ** 2, 20.0 * s ** 3], axis=1),
             np.stack([z, z, z, 6.0 * one, 24.0 * s, 60.0 * s ** 2], axis=1))
    return [np.einsum("nk,nkd->nd", b, c) for b in betas]


def frame(acc, g_acc):
    """|h| (n,), R (n, 3, 3) with columns xB, yB, zB, and |(0, zB_z, -zB_y)| (n,)."""
    h = np.array(acc, dtype=np.float64)
    h[:, 2] += g_acc
    thr = np.linalg.norm(h, axis=1)
    zB = h / thr[:, None]
    u = np.stack([np.zeros(len(h)), zB[:, 2], -zB[:, 1]], axis=1)
    m = np.linalg.norm(u, axis=1)
    yB = u / m[:, None]
    xB = np.cross(yB, zB)
    return thr, np.stack([xB, yB, zB], axis=2), m


def quaternion(R):
    """(n, 4) unit quaternions (w, x, y, z), Hamilton, R(q) = R, by the header's branch rule and sign."""
    R00, R01, R02 = R[:, 0, 0], R[:, 0, 1], R[:, 0, 2]
    R10, R11, R12 = R[:, 1, 0], R[:, 1, 1], R[:, 1, 2]
    R20, R21, R22 = R[:, 2, 0], R[:, 2, 1], R[:, 2, 2]
    tr = R00 + R11 + R22
    # the largest of (trace, R00, R11, R22), the earlier one on a tie
    k0 = (tr >= R00) & (tr >= R11) & (tr >= R22)
    k1 = ~k0 & (R00 >= R11) & (R00 >= R22)
    k2 = ~k0 & ~k1 & (R11 >= R22)
    r = np.sqrt(np.select([k0, k1, k2], [1.0 + tr, 1.0 + R00 - R11 - R22, 1.0 + R11 - R00 - R22], 1.0 + R22 - R00 - R11))
    f = 0.5 / r
    wx, wy, wz = (R21 - R12) * f, (R02 - R20) * f, (R10 - R01) * f
    xy, xz, yz = (R01 + R10) * f, (R02 + R20) * f, (R12 + R21) * f
    q = np.stack([np.select([k0, k1, k2], [0.5 * r, wx, wy], wz),
                  np.select([k0, k1, k2], [wx, 0.5 * r, xy], xz),
                  np.select([k0, k1, k2], [wy, xy, 0.5 * r], yz),
                  np.select([k0, k1, k2], [wz, xz, yz], 0.5 * r)], axis=1)
    return np.where((q[:, 0] < 0.0)[:, None], -q, q)


def quat_to_R(q):
    """(n, 3, 3) rotation matrices of unit quaternions (w, x, y, z), Hamilton convention."""
    w, x, y, z = (q[:, i] for i in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def body_rates(R, jer, thr, m):
    xB, yB, zB = R[:, :, 0], R[:, :, 1], R[:, :, 2]
    zj = np.einsum("nd,nd->n", zB, jer)
    dzB = (jer - zB * zj[:, None]) / thr[:, None]
    wx = -np.einsum("nd,nd->n", yB, jer) / thr
    wy = np.einsum("nd,nd->n", xB, jer) / thr
    wz = -(xB[:, 1] * dzB[:, 2] - xB[:, 2] * dzB[:, 1]) / m
    return np.stack([wx, wy, wz], axis=1)


def sample_candidate(T, Cf, t, g_acc):
    """Rows (len(t), 20) of one candidate: T (N,), Cf (6N, 3) or (18N,), times from its start."""
    T = np.asarray(T, dtype=np.float64)
    C = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    i, s = locate(T, t)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pos, vel, acc, jer = flat_state(C[i], s)
        thr, R, m = frame(acc, g_acc)
        q = quaternion(R)
        om = body_rates(R, jer, thr, m)
    return np.concatenate([pos, vel, acc, jer, thr[:, None], q, om], axis=1)


def sample_batch(T, Cf, piece_off, n_samples, g_acc, dt=0.0, t0=0.0, times=None, cands=None):
    """Rows (len(cands), S, 20) of the candidates `cands` (default: all) of a batch, in any of the three time modes."""
    Cp = np.asarray(Cf, dtype=np.float64).reshape(-1, 18)
    cands = range(len(piece_off) - 1) if cands is None else cands
    out = []
    for b in cands:
        sl = slice(piece_off[b], piece_off[b + 1])
        t = times[b] if times is not None else sample_times(T[sl], n_samples, dt, t0)
        out.append(sample_candidate(T[sl], Cp[sl], t, g_acc))
    return np.array(out)
