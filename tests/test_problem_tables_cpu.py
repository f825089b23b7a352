"""What frx_problem_create decides on the host (fast-racing_amd/csrc/frx_problem_tables.hpp and the sizes and choices of frx_launch_forms.hpp), in its host build
(tests/hostcheck): create asks these functions, so what is pinned here is what every kernel reads.  The tables are checked against a numpy restatement of the
reference's rules (CPU.hpp:1003-1029 gridMesh, 1049 the [v0, v_r - v0] form, 1116 the normalisation, 1129-1152 the index maps, 325/328 the signed distance), written
here with the reference's idxVs / idxHs and not from the C++; the geometry against closed forms and the kernels' own carve-ups, listed below.  No GPU."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hostcheck import _load_hostcheck  # noqa: E402

OK, INVALID_ARG, EMPTY_POLYTOPE = 0, -1, -4
TABLES_OK, TABLES_COARSE_N, TABLES_NO_HALFSPACES, TABLES_NO_VERTICES = range(4)
BAND_W = 13
LDS = 160 * 1024
INT_TABLES = ("poff", "coff", "xoff", "boff", "cvoff", "dimT", "piece_hbeg", "piece_K", "piece_coarse", "piece_iv", "coarse_iv", "coarse_fbeg", "wp_vbeg", "wp_nv", "wp_xbeg")
DBL_TABLES = ("hrec", "horg", "vrec", "head", "tail", "hblk")
SCALARS = ("P", "Pc", "NX", "Kmax", "maxN", "maxCN", "sumKfine", "maxXb", "maxVb")


@pytest.fixture(scope="module")
def hc():
    H = _load_hostcheck()
    ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    lp = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    H.hostcheck_problem_tables_fill.restype = C.c_int
    H.hostcheck_problem_tables_fill.argtypes = [C.c_double] * 4 + [C.c_int, ip, dp, dp, ip, dp, ip, dp, C.POINTER(C.c_int), ip]
    H.hostcheck_problem_tables_get.restype = C.c_longlong
    H.hostcheck_problem_tables_get.argtypes = [C.c_int, C.c_void_p, C.c_longlong]
    H.hostcheck_launch_geometry.restype = None
    H.hostcheck_launch_geometry.argtypes = [ip, C.c_int, lp]
    H.hostcheck_knot_threads.restype = C.c_int
    H.hostcheck_knot_threads.argtypes = [C.c_int]
    H.hostcheck_pcr_steps.restype = C.c_int
    H.hostcheck_pcr_steps.argtypes = [C.c_int]
    H.hostcheck_penalty_waves.restype = None
    H.hostcheck_penalty_waves.argtypes = [C.c_int] * 5 + [ip]
    H.hostcheck_eval_cluster_admitted.restype = C.c_int
    H.hostcheck_eval_cluster_admitted.argtypes = [C.c_int] * 6
    H.hostcheck_eval_solo_choice.restype = None
    H.hostcheck_eval_solo_choice.argtypes = [C.c_int] * 4 + [ip]
    return H


# ---- crafted batches ----
GRID_RES, MARGIN, VEL_MAX = 1.5, 0.25, 4.0


def _candidate(rng, Ks, intervals, nvs):
    """One candidate of len(Ks) coarse pieces.  Ks[i] half-spaces of polytope i, with normals of every length but 1; nvs[m] vertices of V-polytope m (2 cN - 1 of
    them); the overlap polytopes and the final position are placed so that gridMesh gives `intervals`: the centres lie (intervals[i] - 0.5) cells apart."""
    cN = len(Ks)
    assert len(intervals) == cN and len(nvs) == 2 * cN - 1
    ini, fin = rng.uniform(-2.0, 2.0, 9), rng.uniform(-2.0, 2.0, 9)
    h_polys = []
    for K in Ks:
        rec = np.empty((K, 6))
        rec[:, :3] = rng.uniform(-1.0, 1.0, (K, 3)) + 3.0 * np.eye(3)[np.arange(K) % 3]
        rec[:, :3] *= rng.uniform(0.05, 40.0, (K, 1))                       # |n| from 0.1 to over 100
        rec[:, 3:] = rng.uniform(-15.0, 15.0, (K, 3))
        h_polys.append(rec)
    v_polys, at = [], ini[:3].copy()
    for m in range(2 * cN - 1):
        if m % 2 == 1:                                                      # the overlap of cells i and i + 1: its centre is the next mesh point
            d = rng.normal(size=3)
            target = at + d / np.linalg.norm(d) * (intervals[m // 2] - 0.5) * GRID_RES
            v = target + rng.uniform(-0.3, 0.3, (nvs[m], 3))
            k = nvs[m] - 1
            if k > 0:                                                       # move the last vertex so that sum(v_r - v0) / (1 + k) + v0 is the target
                rest = v[1:-1] - v[0]
                v[-1] = v[0] + (target - v[0]) * (1.0 + k) - rest.sum(axis=0)
            else:
                v[0] = target
            at = target
        else:
            v = at + rng.uniform(-0.5, 0.5, (nvs[m], 3))
        v_polys.append(v)
    d = rng.normal(size=3)
    fin[:3] = at + d / np.linalg.norm(d) * (intervals[-1] - 0.5) * GRID_RES
    return dict(ini=ini, fin=fin, h=h_polys, v=v_polys, intervals=list(intervals))


def _the_batch():
    rng = np.random.default_rng(7)
    return [
        _candidate(rng, [5], [3], [4]),                                     # coarse_n = 1, three intervals: two within-cell waypoints, no overlap
        _candidate(rng, [1, 40, 3], [1, 1, 1], [3, 2, 5, 1, 4]),            # every coarse piece one interval: overlap waypoints only; K = 1 beside K = 40; a one-vertex overlap
        _candidate(rng, [6, 2, 9, 4], [2, 1, 3, 1], [4, 3, 2, 6, 5, 3, 7]),  # both kinds of waypoint
        _candidate(rng, [7, 12], [1, 4], [2, 8, 3]),
        _candidate(rng, [3], [1], [5]),                                     # one piece: no waypoint, and with the fixed total time no variable at all
    ]


def _pack(cands):
    coarse_n = np.array([len(c["h"]) for c in cands], np.int32)
    ini = np.ascontiguousarray(np.concatenate([c["ini"] for c in cands]))
    fin = np.ascontiguousarray(np.concatenate([c["fin"] for c in cands]))
    hs = [h for c in cands for h in c["h"]]
    vs = [v for c in cands for v in c["v"]]
    h_off = np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.int32)
    v_off = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int32)
    h_rec = np.ascontiguousarray(np.concatenate([h.reshape(-1) for h in hs] + [np.zeros(6)]))
    v_rec = np.ascontiguousarray(np.concatenate([v.reshape(-1) for v in vs] + [np.zeros(3)]))
    return coarse_n, ini, fin, h_off, h_rec, v_off, v_rec


def _fill(hc, cands, soft, packed=None):
    coarse_n, ini, fin, h_off, h_rec, v_off, v_rec = packed if packed is not None else _pack(cands)
    why, scal = C.c_int(-1), np.full(9, -1, np.int32)
    rc = hc.hostcheck_problem_tables_fill(1000.0 if soft else 0.0, GRID_RES, VEL_MAX, MARGIN, len(coarse_n), coarse_n, ini, fin, h_off, h_rec, v_off, v_rec, C.byref(why), scal)
    got = dict(zip(SCALARS, (int(v) for v in scal)))
    for which, name in enumerate(INT_TABLES + DBL_TABLES):
        n = hc.hostcheck_problem_tables_get(which, None, -1)
        out = np.zeros(max(n, 1), np.int32 if which < len(INT_TABLES) else np.float64)
        assert hc.hostcheck_problem_tables_get(which, out.ctypes.data_as(C.c_void_p), n) == n
        got[name] = out[:n]
    return rc, why.value, got


# ---- the restatement ----
def _restate(cands, soft):
    """The reference's setup() per candidate (its cfgVs, intervals, idxVs, idxHs, dimFreeT, dimFreeP), then what the kernels are documented to read (DevProblem,
    frx_device.hpp): per piece the polytope of idxHs, per waypoint the polytope of idxVs and where its variables start, per candidate the running offsets."""
    t = {k: [] for k in INT_TABLES + DBL_TABLES}
    for k in ("poff", "coff", "xoff", "boff", "cvoff"):
        t[k] = [0]
    n_hrec = n_vrec = 0
    Kmax = sumK = 0
    per_piece_poly = []                                                     # global polytope index of every fine piece
    polys = []                                                              # (origin, records [K][4]) of every polytope of the batch
    for c in cands:
        cN = len(c["h"])
        cfgVs = [np.vstack([v[:1], v[1:] - v[0]]) for v in c["v"]]          # CPU.hpp:1049
        intervals, cur = [], c["ini"][:3].copy()                            # gridMesh
        for i in range(cN):
            last = cur
            if i < cN - 1:
                V = cfgVs[2 * i + 1]
                k = len(V) - 1
                cur = V[1:].sum(axis=0) / (1.0 + k) + V[0]
            else:
                cur = c["fin"][:3]
            n = int(np.ceil(np.linalg.norm(cur - last) / GRID_RES))
            intervals.append(n if n > 0 else 1)
        assert intervals == c["intervals"], "the batch is what its comment says"
        fineN = sum(intervals)
        idxVs, idxHs = [], []                                               # CPU.hpp:1129-1152
        for i in range(cN):
            for j in range(intervals[i]):
                if j < intervals[i] - 1:
                    idxVs.append(2 * i)
                elif i < cN - 1:
                    idxVs.append(2 * i + 1)
                idxHs.append(i)
        assert len(idxVs) == fineN - 1 and len(idxHs) == fineN
        dimT = cN if soft else cN - 1
        dimP = sum(len(cfgVs[m]) - 1 for m in idxVs)
        p0, c0, x0 = t["poff"][-1], t["coff"][-1], t["xoff"][-1]
        # the polytopes: unit normals and c = n.(p_k - org) - margin, org the point of the first half-space
        hbeg = []
        for rec in c["h"]:
            hbeg.append(n_hrec)
            nn = np.sqrt(rec[:, 0] * rec[:, 0] + rec[:, 1] * rec[:, 1] + rec[:, 2] * rec[:, 2])
            n0, n1, n2 = rec[:, 0] / nn, rec[:, 1] / nn, rec[:, 2] / nn
            org = rec[0, 3:]
            cc = n0 * (rec[:, 3] - org[0]) + n1 * (rec[:, 4] - org[1]) + n2 * (rec[:, 5] - org[2]) - MARGIN
            r4 = np.stack([n0, n1, n2, cc], axis=1)
            t["hrec"].append(r4.reshape(-1)); t["horg"].append(org)
            polys.append((org, r4))
            n_hrec += len(rec)
            Kmax = max(Kmax, len(rec))
        fbeg = np.concatenate([[0], np.cumsum(intervals)])[:-1]
        t["coarse_iv"] += intervals
        t["coarse_fbeg"] += [p0 + int(f) for f in fbeg]
        for i in idxHs:
            t["piece_hbeg"].append(hbeg[i]); t["piece_K"].append(len(c["h"][i])); t["piece_coarse"].append(c0 + i); t["piece_iv"].append(intervals[i])
            per_piece_poly.append(c0 + i)
            sumK += len(c["h"][i])
        x = x0 + dimT
        for m in idxVs:
            t["wp_vbeg"].append(n_vrec); t["wp_nv"].append(len(cfgVs[m])); t["wp_xbeg"].append(x)
            t["vrec"].append(cfgVs[m].reshape(-1))
            n_vrec += len(cfgVs[m])
            x += len(cfgVs[m]) - 1
        assert x == x0 + dimT + dimP
        t["dimT"].append(dimT)
        t["poff"].append(p0 + fineN); t["coff"].append(c0 + cN); t["xoff"].append(x0 + dimT + dimP); t["boff"].append(t["boff"][-1] + 6 * fineN * BAND_W)
        t["cvoff"].append(n_vrec)
        t["head"].append(c["ini"]); t["tail"].append(c["fin"])
    hblk = np.zeros((len(per_piece_poly), Kmax + 1, 4))
    for gp, m in enumerate(per_piece_poly):
        org, r4 = polys[m]
        hblk[gp, 0, :3] = org; hblk[gp, 0, 3] = len(r4)
        hblk[gp, 1:1 + len(r4)] = r4
    t["hblk"] = [hblk.reshape(-1)]
    out = {}
    for k in INT_TABLES:
        out[k] = np.array(t[k], np.int32)
    for k in DBL_TABLES:
        out[k] = np.concatenate(t[k]) if t[k] else np.zeros(0)
    nx = np.diff(out["xoff"]); nv = np.diff(out["cvoff"]); fine = np.diff(out["poff"])
    out.update(P=int(out["poff"][-1]), Pc=int(out["coff"][-1]), NX=int(out["xoff"][-1]), Kmax=Kmax, maxN=int(fine.max()), maxCN=int(np.diff(out["coff"]).max()),
               sumKfine=sumK, maxXb=max(1, int(nx.max())), maxVb=max(3, 3 * int(nv.max())))
    return out


def _assert_tables(got, want):
    for k in SCALARS:
        assert got[k] == want[k], k
    for k in INT_TABLES:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in DBL_TABLES:                                                    # bit for bit: the same operations in the same order on float64
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (k, np.abs(got[k] - want[k]).max())


BATCHES = {"B5": (0, 1, 2, 3, 4), "B1_mixed": (2,), "B1_one_piece": (4,), "B1_coarse1": (0,), "B2_reversed": (3, 1)}


@pytest.mark.parametrize("soft", (True, False), ids=("softT", "fixedT"))
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_tables_against_the_restatement(hc, name, soft):
    all5 = _the_batch()
    cands = [all5[i] for i in BATCHES[name]]
    rc, why, got = _fill(hc, cands, soft)
    assert (rc, why) == (OK, TABLES_OK)
    want = _restate(cands, soft)
    _assert_tables(got, want)
    # what the crafted batch is there to exercise
    assert np.array_equal(got["dimT"], [len(c["h"]) - (0 if soft else 1) for c in cands])
    if name == "B5":
        assert got["Kmax"] == 40 and 1 in got["piece_K"] and got["hblk"].size == got["P"] * 41 * 4
        assert list(np.diff(got["poff"])) == [3, 3, 7, 5, 1] and got["wp_nv"].size == got["P"] - 5
        assert got["maxVb"] == 3 * max(np.diff(got["cvoff"])) and 1 in got["wp_nv"]
    if name == "B1_one_piece":
        assert got["wp_nv"].size == 0 and got["vrec"].size == 0 and got["maxVb"] == 3 and got["maxXb"] == 1 and got["NX"] == (1 if soft else 0)


def test_the_padding_of_hblk_is_zero_and_the_normals_are_unit(hc):
    rc, why, got = _fill(hc, _the_batch(), True)
    assert rc == OK
    blk = got["hblk"].reshape(got["P"], 41, 4)
    for gp in range(got["P"]):
        K = int(got["piece_K"][gp])
        assert blk[gp, 0, 3] == K and not blk[gp, 1 + K:].any()
        assert np.abs(np.linalg.norm(blk[gp, 1:1 + K, :3], axis=1) - 1.0).max() < 1e-15
        assert blk[gp, 1, 3] == -MARGIN                                    # the first half-space's point is the origin


def test_the_refusals(hc):
    cands = _the_batch()
    packed = list(_pack(cands))
    bad = packed[0].copy(); bad[3] = 0
    rc, why, _ = _fill(hc, cands, True, [bad] + packed[1:])
    assert (rc, why) == (INVALID_ARG, TABLES_COARSE_N)
    # an H-polytope without half-spaces: the second polytope of candidate 2
    h_off = packed[3].copy(); k = 1 + 3 + 1
    h_off[k + 1:] -= h_off[k + 1] - h_off[k]
    rc, why, _ = _fill(hc, cands, True, packed[:3] + [h_off] + packed[4:])
    assert (rc, why) == (INVALID_ARG, TABLES_NO_HALFSPACES)
    # a V-polytope without vertices, in candidate 3: refused as such - but behind the half-space refusal of candidate 2, and in front of a coarse_n of candidate 4,
    # candidate after candidate as create met them
    v_off = packed[5].copy(); m = 1 + 5 + 7 + 1
    v_off[m + 1:] -= v_off[m + 1] - v_off[m]
    rc, why, _ = _fill(hc, cands, True, packed[:5] + [v_off] + packed[6:])
    assert (rc, why) == (EMPTY_POLYTOPE, TABLES_NO_VERTICES)
    rc, why, _ = _fill(hc, cands, True, packed[:3] + [h_off, packed[4], v_off, packed[6]])
    assert (rc, why) == (INVALID_ARG, TABLES_NO_HALFSPACES)
    bad4 = packed[0].copy(); bad4[4] = -2
    rc, why, _ = _fill(hc, cands, True, [bad4] + packed[1:5] + [v_off, packed[6]])
    assert (rc, why) == (EMPTY_POLYTOPE, TABLES_NO_VERTICES)
    bad0 = packed[0].copy(); bad0[0] = 0
    rc, why, _ = _fill(hc, cands, True, [bad0] + packed[1:3] + [h_off, packed[4], v_off, packed[6]])
    assert (rc, why) == (INVALID_ARG, TABLES_COARSE_N)


# ---- the geometry ----
MAXN = (1, 2, 3, 64, 65, 66, 128, 129, 256, 257)


def _knot_fwd_doubles(nt, maxCN, maxXb, maxVb, steps):
    """forward_knot_body's carve-up (frx_kernels.hpp), array after array"""
    return sum([36 * nt,                     # rowbuf
                3 * (nt + 1) * 3,            # KP, KV, KA
                nt,                          # Tf
                maxCN,                       # Tc
                maxXb,                       # xs
                maxVb,                       # vs
                (steps * 8 + 5) * nt])       # pwf


def _knot_bwd_doubles(nt, maxCN, maxXb, maxVb, steps):
    """the backward_knot bodies' carve-up, 256 threads: red holds 2 (nthr >> 6) + 2"""
    return sum([36 * nt, 3 * (nt + 1) * 3,
                nt, nt,                      # Tf, gT
                maxCN,                       # gCo
                2 * (256 >> 6) + 2,          # red
                maxXb, maxVb,                # xs, vs
                (steps * 8 + 5) * nt,        # pw
                maxXb])                      # dsv


def _geometry(hc, maxN, maxCN, Kmax, P, maxXb, maxVb, kappa, simds, forced=0):
    out = np.zeros(16, np.int64)
    hc.hostcheck_launch_geometry(np.array([maxN, maxCN, Kmax, P, maxXb, maxVb, kappa, simds], np.int32), forced, out)
    names = ("lpp", "ppw", "pen_w", "ppg", "lds_fwd", "lds_bwd", "lds_pen", "lds_pen2", "solver", "knot_threads", "pcr_steps", "lds_kfwd", "lds_kbwd", "refusal", "banded_ok", "maxXb")
    return dict(zip(names, (int(v) for v in out)))


def test_knot_threads_and_pcr_steps(hc):
    for maxN in MAXN:
        assert hc.hostcheck_knot_threads(maxN) == 64 * -(-maxN // 64), maxN
        # the reduction doubles its stride until it covers the maxN - 1 interior knots: ceil(log2(maxN - 1)), none up to two pieces
        assert hc.hostcheck_pcr_steps(maxN) == (0 if maxN <= 2 else (maxN - 2).bit_length()), maxN
    assert [hc.hostcheck_pcr_steps(n) for n in MAXN] == [0, 0, 1, 6, 6, 7, 7, 7, 8, 8]


def test_lds_sizes_and_the_capacity_verdict(hc):
    """Over the grid: every size is the sum of its kernel's carve-up; create refuses exactly where the knot system passes 256 threads or 160 KiB, the banded-LU
    pair becomes unavailable exactly where its sizes pass 160 KiB, and neither moves the other."""
    seen = set()
    for maxN, maxCNf, maxXb, maxVb in itertools.product(MAXN, (0, 1), (1, 640, 2900, 3000, 6000), (3, 2700, 9000)):
        maxCN = maxN if maxCNf else 1
        g = _geometry(hc, maxN, maxCN, 8, 4 * maxN, maxXb, maxVb, 16, 1024)
        nt, steps = 64 * -(-maxN // 64), (0 if maxN <= 2 else (maxN - 2).bit_length())
        assert (g["knot_threads"], g["pcr_steps"], g["solver"], g["maxXb"]) == (nt, steps, 0, maxXb)
        assert g["lds_kfwd"] == 8 * _knot_fwd_doubles(nt, maxCN, maxXb, maxVb, steps)
        assert g["lds_kbwd"] == 8 * _knot_bwd_doubles(nt, maxCN, maxXb, maxVb, steps)
        # k_forward: band | rhs | Tf | Tc; k_backward: band | gd | cL | Tf | gT | gCo
        fwd = 8 * (6 * maxN * BAND_W + 6 * maxN * 3 + maxN + maxCN)
        bwd = 8 * (6 * maxN * BAND_W + 2 * 6 * maxN * 3 + 2 * maxN + maxCN)
        assert (g["lds_fwd"], g["lds_bwd"]) == (fwd, bwd)
        knot_refused = nt > 256 or g["lds_kbwd"] > LDS
        assert g["refusal"] == (1 if knot_refused else 0), (maxN, maxXb, maxVb)
        assert g["banded_ok"] == (0 if fwd > LDS or bwd > LDS else 1)
        seen.add((knot_refused, nt > 256, bool(g["banded_ok"])))
    # (a candidate the banded pair cannot hold - 179 pieces and more - needs three waves of knot rows, which pass 160 KiB by themselves: no handle is created there)
    assert seen == {(True, True, False), (True, False, True), (True, False, False), (False, False, True)}
    # the banded pair's own edge: k_backward's 8 (116 N + 1) bytes pass 163840 behind N = 176 (k_forward's 8 (98 N + 1) much later)
    assert [_geometry(hc, N, 1, 8, N, 1, 3, 16, 1024)["banded_ok"] for N in (175, 176, 177, 178)] == [1, 1, 0, 0]
    assert 8 * (116 * 176 + 1) <= LDS < 8 * (116 * 177 + 1)
    # the knot kernels' own edge at one wave of rows: 8 (2949 + 2 maxXb + 1 + 3 + 10 + (6 * 8 + 5) * 64) bytes at 64 pieces
    base = _knot_bwd_doubles(64, 1, 0, 3, 6)
    x_fit = (LDS // 8 - base) // 2
    assert _geometry(hc, 64, 1, 8, 64, x_fit, 3, 16, 1024)["refusal"] == 0 and _geometry(hc, 64, 1, 8, 64, x_fit + 1, 3, 16, 1024)["refusal"] == 1
    # the penalty workgroup alone: one wave of one piece with more half-spaces than a CU holds
    k_fit = (LDS // 8 - 3 * 19 - 64 * 21) // (3 * 4) - 1
    assert _geometry(hc, 4, 1, k_fit, 4, 1, 3, 16, 1024)["refusal"] == 0 and _geometry(hc, 4, 1, k_fit + 1, 4, 1, 3, 16, 1024)["refusal"] == 2


def _pen_bytes(ppg, Kmax, waves, per_lane=21):
    return 8 * (ppg * 19 + ppg * (Kmax + 1) * 4 + 64 * waves * per_lane)


def _waves(hc, lpp, Kmax, P, simds, forced=0):
    out = np.zeros(2, np.int32)
    hc.hostcheck_penalty_waves(lpp, Kmax, P, simds, forced, out)
    assert out[1] == 64 * out[0] // lpp
    return int(out[0])


def test_penalty_waves(hc):
    simds = 1024
    for lpp in (17, 49):
        ppw = 64 // lpp
        # lane utilisation of w waves: whole pieces only.  17: 51/64, 119/128, 187/192, 255/256 -> four; 49: 49/64, 98/128, 147/192 (equal: the fewest), 245/256 -> four
        util = {w: (64 * w // lpp) * lpp / (64.0 * w) for w in (1, 2, 3, 4)}
        assert max(util, key=util.get) == 4
        fits, beyond = simds * ppw, simds * ppw + 1                        # pieces: one wave per piece-group still fits the SIMDs / no longer
        assert _waves(hc, lpp, 8, fits, simds) == 1 and _waves(hc, lpp, 8, beyond, simds) == 4
        for forced in (1, 2, 3, 4):
            assert _waves(hc, lpp, 8, fits, simds, forced) == forced and _waves(hc, lpp, 8, beyond, simds, forced) == forced
        for forced in (0, 5, -1):
            assert _waves(hc, lpp, 8, beyond, simds, forced) == 4
    assert 49 / 64 == 98 / 128 == 147 / 192
    # among equals the fewest waves: at 49 lanes per piece one, two and three waves tie and none of them is picked over four; where every count ties
    # (32 or 64 lanes per piece: no lane idle at any count) it is one wave.  33 lanes per piece (33/64, 99/128, 165/192, 231/256): no tie, four win
    assert _waves(hc, 32, 8, 10 ** 6, simds) == 1 and _waves(hc, 64, 8, 10 ** 6, simds) == 1
    assert _waves(hc, 33, 8, 10 ** 6, simds) == 4
    # Kmax = 260 at kappa = 16 (tests/test_gpu_penalty_branches.py): four waves' fifteen blocks pass 160 KiB, three waves' eleven fit
    assert _pen_bytes(15, 260, 4) > LDS >= _pen_bytes(11, 260, 3)
    assert _waves(hc, 17, 260, 10 ** 6, simds) == 3 and _waves(hc, 17, 260, 10 ** 6, simds, 4) == 3 and _waves(hc, 17, 260, 10 ** 6, simds, 2) == 2
    g = _geometry(hc, 16, 16, 260, 10 ** 6, 100, 300, 16, simds)
    assert (g["pen_w"], g["ppg"], g["lds_pen"], g["lds_pen2"], g["refusal"]) == (3, 11, _pen_bytes(11, 260, 3), 0, 0)
    # the two-phase form's size exists with four waves and one sample per lane only
    g = _geometry(hc, 16, 16, 8, 10 ** 6, 100, 300, 16, simds)
    assert (g["lpp"], g["ppw"], g["pen_w"], g["ppg"], g["lds_pen2"]) == (17, 3, 4, 15, _pen_bytes(15, 8, 4, 11))
    assert _geometry(hc, 16, 16, 8, 100, 100, 300, 16, simds)["lds_pen2"] == 0                        # one wave
    g = _geometry(hc, 16, 16, 8, 10 ** 6, 100, 300, 100, simds)                                       # kappa + 1 > 64: 64 lanes per piece, a lane walks over samples
    assert (g["lpp"], g["ppw"], g["lds_pen2"]) == (64, 1, 0)
    # every step of the step-down, at a forced four: the largest count whose block fits
    for Kmax in (8, 200, 260, 400, 700, 1400):
        want = next((w for w in (4, 3, 2) if _pen_bytes(64 * w // 17, Kmax, w) <= LDS), 1)
        assert _waves(hc, 17, Kmax, 10 ** 6, simds, 4) == want, Kmax


def test_one_launch_admission(hc):
    cus, G = 256, 8
    adm = hc.hostcheck_eval_cluster_admitted
    for B, fits in ((cus // G, True), (cus // G + 1, False)):               # B G = cus and cus + G
        for ch, ranks, ndev in itertools.product((0, ord("0"), ord("1"), ord("2")), (1, 8, 9), (1, 8)):
            want = fits and ch != ord("0") and (ranks <= ndev or ch == ord("1"))
            assert adm(G, B, cus, ch, ranks, ndev) == int(want), (B, ch, ranks, ndev)
    assert adm(1, cus, cus, 0, 1, 1) == 1 and adm(1, cus + 1, cus, 0, 1, 1) == 0 and adm(1, cus + 1, cus, ord("1"), 1, 1) == 0   # B G = cus, cus + 1
    assert adm(0, 1, cus, ord("1"), 1, 1) == 0                              # the geometry does not apply
    assert adm(40, 60000000, cus, 0, 1, 1) == 0                             # B G beyond 2^31


def test_solo_thresholds(hc):
    def choice(lds_solo, ch=0, lo=0, hi=0):
        out = np.zeros(3, np.int32)
        hc.hostcheck_eval_solo_choice(lds_solo, ch, lo, hi, out)
        return tuple(int(v) for v in out)
    assert choice(1) == (1, 384, 512) and choice(0) == (0, 384, 512)
    assert choice(1, ord("0")) == (0, 384, 512) and choice(1, ord("1")) == (2, 384, 512) and choice(0, ord("1")) == (0, 384, 512) and choice(1, ord("7")) == (1, 384, 512)
    assert choice(1, 0, 100) == (1, 100, 512) and choice(1, 0, 0, 2000) == (1, 384, 2000) and choice(1, ord("1"), 7, 9) == (2, 7, 9)
    assert choice(1, 0, -5, -1) == (1, 384, 512)
