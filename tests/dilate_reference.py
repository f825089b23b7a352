"""Plain numpy restatement of ONE corridor cell, LineSegment3D::dilate(offset) of decomp_util - test infrastructure, not a test module.

Sequential, one segment, no lanes and no chunks; it does not call the library.  The steps, with the reference's lines:
  local box        line_segment.h:47-85    six planes around the segment (none when the box is zero)
  set_obs          decomp_base.h:33-38     the cloud points with n.(q - p) <= 1e-10 for all six, in cloud order: the candidates
  find_ellipsoid   line_segment.h:136-211  a sphere on the segment; the two short axes shrink together, rolled towards the closest candidate inside, until
                                           none is inside; then the third axis starts again from its old length and shrinks alone
  find_polyhedron  decomp_base.h:63-83     the closest remaining candidate in the ellipsoid's metric gives the tangent plane there; everything with
                                           n.(q - c) >= 0 leaves; until nothing remains
  box planes appended                      line_segment.h:31-35
Every arg-min is np.argmin: the first of the minima in cloud order (ellipsoid.h:39-50 keeps the first with `<`).

The ellipsoid is { C u + d : |u| <= 1 } with C = R diag(a) R^T, R a rotation; its inverse is formed as R diag(1 / a) R^T, not by inverting C, so that the
metric does not share the library's cofactor formula.  dtype is np.float64 or np.longdouble.
"""
import numpy as np

EPS = 1e-10                                                       # decomp_basis/data_type.h:129


class Cell(dict):
    __getattr__ = dict.__getitem__


def _rotation_from_direction(v, T):
    """R = Rz(yaw) Ry(pitch): takes e_x to the direction of v, zero roll (geometric_utils.h:27-35)"""
    pitch = np.arctan2(-v[2], np.hypot(v[0], v[1])); yaw = np.arctan2(v[1], v[0])
    cp, sp, cy, sy = np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    return np.array([[cy * cp, -sy, cy * sp], [sy * cp, cy, sy * sp], [-sp, T(0), cp]], dtype=T)


def _roll_about_x(roll, T):
    c, s = np.cos(roll), np.sin(roll)
    return np.array([[T(1), T(0), T(0)], [T(0), c, -s], [T(0), s, c]], dtype=T)


def box_planes(p1, p2, bbox, dtype=np.float64):
    """(n [6][3], p [6][3]) of the local box, or two empty arrays when the box is zero"""
    T = dtype
    p1, p2, bbox = (np.asarray(x, dtype=T) for x in (p1, p2, bbox))
    if np.sqrt((bbox * bbox).sum()) == 0:
        return np.zeros((0, 3), T), np.zeros((0, 3), T)
    u = p2 - p1; u = u / np.sqrt((u * u).sum())
    h = np.array([u[1], -u[0], T(0)], dtype=T)
    if np.sqrt((h * h).sum()) == 0:
        h = np.array([-1, 0, 0], dtype=T)
    h = h / np.sqrt((h * h).sum())
    v = np.array([u[1] * h[2] - u[2] * h[1], u[2] * h[0] - u[0] * h[2], u[0] * h[1] - u[1] * h[0]], dtype=T)
    n = np.stack([h, -h, u, -u, v, -v])
    p = np.stack([p1 + h * bbox[1], p1 - h * bbox[1], p2 + u * bbox[0], p1 - u * bbox[0], p1 + v * bbox[2], p1 - v * bbox[2]])
    return n, p


def candidates(p1, p2, bbox, obs, dtype=np.float64):
    """(cloud indices of the points set_obs keeps, box_margin = smallest | n.(q - p) - 1e-10 | over all cloud points and box planes)"""
    obs = np.asarray(obs, dtype=dtype).reshape(-1, 3)
    n, p = box_planes(p1, p2, bbox, dtype)
    if len(n) == 0 or len(obs) == 0:
        return np.arange(len(obs)), np.inf
    sd = ((obs[:, None, :] - p[None]) * n[None]).sum(axis=2)      # [n_obs][6]
    return np.flatnonzero(~(sd > dtype(EPS)).any(axis=1)), float(np.abs(sd - dtype(EPS)).min())


def dilate_cell(p1, p2, bbox, obs, offset=0.0, dtype=np.float64):
    """One cell.  Returns Cell(H 6 x K in emission order, C 3x3, d, order [(candidate index, cloud index)] of the tangent planes' contact points, gaps and
    gap_stage (for every arg-min taken, in the order taken: runner-up distance minus chosen distance - inf when one point was left, 0 at an exact tie -
    and 'a1' / 'a2' / 'poly' for the loop that took it), box_margin, cand (cloud index of every candidate), dist_final (every candidate's distance in the
    final ellipsoid's metric), shell_margin (smallest | 1 - dist - 1e-10 | and | dist - 1 | over the in / out decisions of the ellipsoid loops, the points
    that fixed an axis left out: they sit on the boundary by construction), cut_margin (smallest | n.(q - c) | over the polyhedron loop's decisions, q == c
    bit for bit left out))."""
    T = dtype
    p1, p2 = np.asarray(p1, dtype=T), np.asarray(p2, dtype=T)
    obs = np.asarray(obs, dtype=T).reshape(-1, 3)
    cand, box_margin = candidates(p1, p2, bbox, obs, T)
    Q = obs[cand]; M = len(Q)
    one, eps = T(1), T(EPS)
    gaps, stage = [], []

    def shape(R, a):
        return (R * a[None]) @ R.T, (R * (one / a)[None]) @ R.T

    def dist(Cinv, pts):
        u = (pts - d[None]) @ Cinv.T
        return np.sqrt((u * u).sum(axis=1))

    def argmin_live(dd, live, which):
        idx = np.flatnonzero(live)
        k = int(np.argmin(dd[idx]))                                # first of the minima
        rest = np.delete(dd[idx], k)
        gaps.append(float(rest.min() - dd[idx][k]) if len(rest) else np.inf); stage.append(which)
        return int(idx[k])

    # ---- find_ellipsoid ----
    diff = p1 - p2
    f = np.sqrt((diff * diff).sum()) / 2
    a = np.array([f + T(offset), f, f], dtype=T)
    if a[0] > 0:
        a = a * (a[1] / a[0])
    Ri = _rotation_from_direction(p2 - p1, T); Rf = Ri
    d = (p1 + p2) / 2
    C, Cinv = shape(Ri, a)
    fixed = np.zeros(M, bool)                                      # points that fixed an axis
    shell = [np.inf]
    dd = dist(Cinv, Q)
    in0 = dd <= 1
    shell.append(np.abs(dd - one).min() if M else np.inf)
    live = in0.copy()
    while live.any():                                              # the two short axes together
        ic = argmin_live(dd, live, "a1")
        p = Ri.T @ (Q[ic] - d)
        Rf = Ri @ _roll_about_x(np.arctan2(p[2], p[1]), T)
        p = Rf.T @ (Q[ic] - d)
        if p[0] < a[0]:
            a[1] = np.abs(p[1]) / np.sqrt(one - (p[0] / a[0]) ** 2)
        C, Cinv = shape(Rf, np.array([a[0], a[1], a[1]], dtype=T))
        dd = dist(Cinv, Q)
        fixed[ic] = True
        m = live & ~fixed
        if m.any():
            shell.append(np.abs(one - dd[m] - eps).min())
        live = live & (one - dd > eps)
    C, Cinv = shape(Rf, a)                                         # the third axis from its old length
    dd = dist(Cinv, Q)
    m = in0 & ~fixed
    if m.any():
        shell.append(np.abs(dd[m] - one).min())
    live = in0 & (dd <= 1)
    while live.any():
        ic = argmin_live(dd, live, "a2")
        p = Rf.T @ (Q[ic] - d)
        r = one - (p[0] / a[0]) ** 2 - (p[1] / a[1]) ** 2
        if r > eps:
            a[2] = np.abs(p[2]) / np.sqrt(r)
        C, Cinv = shape(Rf, a)
        dd = dist(Cinv, Q)
        fixed[ic] = True
        m = live & ~fixed
        if m.any():
            shell.append(np.abs(one - dd[m] - eps).min())
        live = live & (one - dd > eps)
    # ---- find_polyhedron ----
    dist_final = dist(Cinv, Q)
    W = Cinv @ Cinv.T
    live = np.ones(M, bool)
    normals, points, order, cut = [], [], [], [np.inf]
    while live.any():
        ic = argmin_live(dist_final, live, "poly")
        c = Q[ic]
        n = W @ (c - d); n = n / np.sqrt((n * n).sum())
        normals.append(n); points.append(c); order.append((ic, int(cand[ic])))
        sd = (Q - c[None]) @ n
        m = live & ~(Q == c[None]).all(axis=1)
        if m.any():
            cut.append(np.abs(sd[m]).min())
        live = live & (sd < 0)
    bn, bp = box_planes(p1, p2, bbox, T)
    N = np.concatenate([np.array(normals, dtype=T).reshape(-1, 3), bn]); P = np.concatenate([np.array(points, dtype=T).reshape(-1, 3), bp])
    return Cell(H=np.concatenate([N, P], axis=1).T.copy(), C=C, d=d, order=order, gaps=np.array(gaps, dtype=np.float64), gap_stage=stage,
                box_margin=box_margin, cand=cand, dist_final=dist_final, shell_margin=float(min(shell)), cut_margin=float(min(cut)))


# ---- the cell's own promise, on anybody's output -------------------------------------------------------------------------------------------------------------
def unsafe_points(H, C, d, p1, p2, bbox, obs, tol=1e-9):
    """(number of candidates more than tol inside ALL planes of H, number of candidates with | C^-1 (q - d) | < 1 - tol, largest n.(x - p) over the planes for
    x = p1, p2 and the midpoint).  A cell keeps its promise when this is (0, 0, <= tol)."""
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
    cand, _ = candidates(p1, p2, bbox, obs)
    Q = obs[cand]
    H = np.asarray(H, dtype=np.float64)
    seg = np.stack([np.asarray(p1, float), np.asarray(p2, float), 0.5 * (np.asarray(p1, float) + np.asarray(p2, float))])
    worst_seg = float(np.einsum("dk,ndk->nk", H[:3], seg[:, :, None] - H[3:][None]).max()) if H.shape[1] else -np.inf
    if len(Q) == 0:
        return 0, 0, worst_seg
    sd = np.einsum("dk,ndk->nk", H[:3], Q[:, :, None] - H[3:][None])     # [M][K]
    deep = int((sd < -tol).all(axis=1).sum()) if H.shape[1] else len(Q)
    u = (Q - np.asarray(d, float)[None]) @ np.linalg.inv(np.asarray(C, dtype=np.float64)).T
    return deep, int((np.sqrt((u * u).sum(axis=1)) < 1 - tol).sum()), worst_seg
