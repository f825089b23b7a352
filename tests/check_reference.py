"""Independent numpy restatement of the dense feasibility certificate (frx_trajectory_check, include/frx.h) - test infrastructure, not a test
module.  Written from the reference's penalty integrand (se3gcopter_cpu.hpp:240-330, 347-398), not from the library's kernel arithmetic:

  s_j = (T / M) * j, j = 0..M                                      (step first, then multiplied: the penalty's abscissa form)
  beta_m = d^m/ds^m (1, s, .., s^5);  pos / vel / acc / jer = c^T beta_0..3        (CPU.hpp:253-263)
  h = acc + gAcc e3;  zB = h / |h|;  yB = normalise(0, zB_z, -zB_y);  xB = yB x zB;  R = [xB yB zB]      (normalizeFDF, CPU.hpp:265-276)
  fThr = |h|;  bdr = R^T jer / fThr;  xyBdr = (-bdr_y, bdr_x, 0)                    (CPU.hpp:281-291)
  corridor: n.(pos - p) + |(R^T n) .* ellipsoid|, normals normalised as setup() does (CPU.hpp:1114-1116, 322-325), no safeMargin
"""
import numpy as np

FIELDS = ("corridor", "speed", "thrust_min", "thrust_max", "body_rate", "acc", "worst_t", "worst_k")


def piece_samples(c, T, M, hpoly, ell, g_acc):
    """Per-sample values of one piece: dict(s, corridor (M+1, K), speed, thrust, body_rate, acc), every array over the M + 1 samples.
    c: (6, 3) coefficients (row k = power k), hpoly: 6 x K columns (outer normal, point)."""
    c = np.asarray(c, dtype=np.float64).reshape(6, 3)
    step = T / M
    s = step * np.arange(M + 1, dtype=np.float64)
    one, z = np.ones_like(s), np.zeros_like(s)
    beta0 = np.stack([one, s, s ** 2, s ** 3, s ** 4, s ** 5], axis=1)
    beta1 = np.stack([z, one, 2.0 * s, 3.0 * s ** 2, 4.0 * s ** 3, 5.0 * s ** 4], axis=1)
    beta2 = np.stack([z, z, 2.0 * one, 6.0 * s, 12.0 * s ** 2, 20.0 * s ** 3], axis=1)
    beta3 = np.stack([z, z, z, 6.0 * one, 24.0 * s, 60.0 * s ** 2], axis=1)
    pos, vel, acc, jer = beta0 @ c, beta1 @ c, beta2 @ c, beta3 @ c
    h = acc.copy()
    h[:, 2] += g_acc
    fThr = np.linalg.norm(h, axis=1)
    zB = h / fThr[:, None]
    czB = np.stack([z, zB[:, 2], -zB[:, 1]], axis=1)
    yB = czB / np.linalg.norm(czB, axis=1)[:, None]
    xB = np.cross(yB, zB)
    R = np.stack([xB, yB, zB], axis=2)                                   # R[:, :, 0] = xB ...
    rotTrDotJer = np.einsum("sij,si->sj", R, jer)
    bdr = rotTrDotJer / fThr[:, None]
    xyBdr = np.stack([-bdr[:, 1], bdr[:, 0], z], axis=1)
    H = np.asarray(hpoly, dtype=np.float64)
    n = H[:3] / np.linalg.norm(H[:3], axis=0)                            # (3, K)
    p = H[3:]
    RtN = np.einsum("sij,ik->sjk", R, n)                                 # (M+1, 3, K): R^T n_k
    eNorm = np.linalg.norm(RtN * np.asarray(ell, dtype=np.float64)[None, :, None], axis=1)
    dist = np.einsum("ik,sik->sk", n, pos[:, :, None] - p[None, :, :])
    return dict(s=s, corridor=dist + eNorm, speed=np.linalg.norm(vel, axis=1), thrust=fThr,
                body_rate=np.linalg.norm(xyBdr, axis=1), acc=np.linalg.norm(acc, axis=1))


def piece_row(c, T, M, hpoly, ell, g_acc):
    """The eight fields of one piece (FRX_CHECK_* order).  NaN anywhere in a field's samples makes the field NaN; the worst corridor sample is
    the first (j, then k) that attains the maximum, a NaN one first of all."""
    v = piece_samples(c, T, M, hpoly, ell, g_acc)
    cor = v["corridor"]
    nanm = np.isnan(cor)
    flat = int(np.argmax(nanm.reshape(-1))) if nanm.any() else int(np.argmax(cor.reshape(-1)))    # argmax: first occurrence in (j, k) order
    j, k = divmod(flat, cor.shape[1])

    def mx(a):
        return np.nan if np.isnan(a).any() else a.max()

    def mn(a):
        return np.nan if np.isnan(a).any() else a.min()
    return np.array([mx(cor), mx(v["speed"]), mn(v["thrust"]), mx(v["thrust"]), mx(v["body_rate"]), mx(v["acc"]), v["s"][j], float(k)])


def params_of(params):
    ell = (params["horiz_half_len"], params["horiz_half_len"], params["vert_half_len"])
    return ell, params["grav_acc"]


def check_pieces(T, Cf, polys, params, M):
    """Rows (P, 8) of a batch: T (P,), Cf (6P, 3), polys: the 6 x K H-polytope of every piece."""
    ell, g = params_of(params)
    Cf = np.asarray(Cf, dtype=np.float64).reshape(-1, 6, 3)
    return np.array([piece_row(Cf[i], float(T[i]), M, polys[i], ell, g) for i in range(len(T))])


def reduce_candidates(rows, T, piece_off):
    """Candidate rows (B, 8) from piece rows: max (min for thrust_min) in piece order, NaN propagating; worst_t from the candidate's start,
    worst_k = local index of the first piece with the worst corridor value."""
    out = []
    for b in range(len(piece_off) - 1):
        r = rows[piece_off[b]:piece_off[b + 1]]
        t = np.asarray(T[piece_off[b]:piece_off[b + 1]], dtype=np.float64)
        row = np.empty(8)
        for f in (0, 1, 3, 4, 5):
            row[f] = np.nan if np.isnan(r[:, f]).any() else r[:, f].max()
        row[2] = np.nan if np.isnan(r[:, 2]).any() else r[:, 2].min()
        nanm = np.isnan(r[:, 0])
        i = int(np.argmax(nanm)) if nanm.any() else int(np.argmax(r[:, 0]))
        start = 0.0
        for q in range(i):
            start += t[q]
        row[6] = start + r[i, 6]
        row[7] = float(i)
        out.append(row)
    return np.array(out)


def flags_of(cand, params):
    """Flag bits per candidate (FRX_CHECK_FLAG_*), no slack."""
    f = np.zeros(len(cand), np.uint32)
    with np.errstate(invalid="ignore"):
        f |= np.where(cand[:, 0] > 0.0, 1, 0).astype(np.uint32)
        f |= np.where(cand[:, 1] > params["vel_max"], 2, 0).astype(np.uint32)
        f |= np.where(cand[:, 2] < params["thr_acc_min"], 4, 0).astype(np.uint32)
        f |= np.where(cand[:, 3] > params["thr_acc_max"], 8, 0).astype(np.uint32)
        f |= np.where(cand[:, 4] > params["body_rate_max"], 16, 0).astype(np.uint32)
        f |= np.where(~np.isfinite(cand).all(axis=1), 32, 0).astype(np.uint32)
    return f
