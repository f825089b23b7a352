// What frx_problem_create decides on the host before its first HIP call: the descriptor tables the kernels read (the reference's index maps, CPU.hpp:1116 and
// 1129-1152, expanded per piece, per coarse piece and per waypoint) and the launch geometry that follows from their maxima.  Plain C++: no HIP and no getenv, so
// create (frx_api.cpp) and the CPU-side checks (tests/test_problem_tables_cpu.py, tests/hostcheck/problem_tables_main.cpp) ask the same functions.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/frx.h"
#include "frx_device.hpp"
#include "frx_host_setup.hpp"
#include "frx_launch_forms.hpp"

namespace frx {

// ---- the descriptor tables ----
struct ProblemTables {
    std::vector<int> poff, coff, xoff, boff, cvoff;          // [B + 1] fine pieces, coarse pieces, variables, band doubles, waypoint-vertex records
    std::vector<int> dimT;                                    // [B] durations among a candidate's variables: cN with the soft total time, cN - 1 with the fixed one
    std::vector<int> piece_hbeg, piece_K, piece_coarse, piece_iv;   // [P]
    std::vector<int> coarse_iv, coarse_fbeg;                  // [Pc]
    std::vector<int> wp_vbeg, wp_nv, wp_xbeg;                 // per waypoint, candidate after candidate
    std::vector<double> hrec;                                 // per half-space {unit normal, n.(p_k - org) - margin}, coarse piece after coarse piece
    std::vector<double> horg;                                 // [Pc][3] polytope origin = point of its first half-space
    std::vector<double> vrec;                                 // waypoint vertices [v0, v_r - v0] in waypoint order, contiguous per candidate
    std::vector<double> head, tail;                           // [B][9]
    std::vector<double> hblk;                                 // [P][Kmax + 1][4]: {origin, K}, the K records, zero padded - one contiguous, index-free read per piece in k_penalty
    int P = 0, Pc = 0, NX = 0, Kmax = 0, maxN = 0, maxCN = 0, sumKfine = 0;
    int maxXb = 1, maxVb = 3;                                 // per-candidate maxima: variables, waypoint-vertex doubles
};

enum TablesRefusal { TABLES_OK, TABLES_COARSE_N, TABLES_NO_HALFSPACES, TABLES_NO_VERTICES };

// Fills the tables of a batch, candidate after candidate: the host description of candidate b (host_cand_init into cand[b]: V-polytopes as [v0, v_r - v0], gridMesh,
// waypoint index map, clipped boundary speeds), then its rows while that description is still in cache - describing the whole batch first and tabulating it in a
// second pass costs 3 ms of 12 at 512 candidates of 64 pieces.  Returns FRX_OK or the code of the first refusal met in that order; *why names it.
inline int problem_tables_fill(const frx_config &cfg, bool softT, int B, const int *coarse_n, const double *ini_state, const double *fin_state, const int *h_off,
                               const double *h_rec, const int *v_off, const double *v_rec, std::vector<HostCand> &cand, ProblemTables &t, TablesRefusal *why) {
    cand.resize(B);
    t = ProblemTables();
    t.poff.assign(B + 1, 0); t.coff.assign(B + 1, 0); t.xoff.assign(B + 1, 0); t.boff.assign(B + 1, 0); t.cvoff.assign(B + 1, 0);
    t.dimT.assign(B, 0);
    t.head.assign(ini_state, ini_state + 9 * (size_t)B); t.tail.assign(fin_state, fin_state + 9 * (size_t)B);
    int hpoly = 0, vpoly = 0;                     // running polytope indices into h_off / v_off
    for (int b = 0; b < B; b++) {
        const int cN = coarse_n[b];
        if (cN < 1) { *why = TABLES_COARSE_N; return FRX_ERR_INVALID_ARG; }
        HostCand &hc = cand[b];
        if (host_cand_init(hc, cfg, softT, cN, ini_state + 9 * (size_t)b, fin_state + 9 * (size_t)b, v_off + vpoly, v_rec) != FRX_OK) { *why = TABLES_NO_VERTICES; return FRX_ERR_EMPTY_POLYTOPE; }
        t.cvoff[b] = (int)(t.vrec.size() / 3);
        // index maps (CPU.hpp:1129-1152), expanded into per-piece / per-waypoint device descriptors
        const int gp0 = t.poff[b], gc0 = t.coff[b];
        int offset = 0;
        int xcur = t.xoff[b] + hc.dimT;
        for (int i = 0; i < cN; i++) {
            const int hb = h_off[hpoly + i], K = h_off[hpoly + i + 1] - hb;
            if (K < 1) { *why = TABLES_NO_HALFSPACES; return FRX_ERR_INVALID_ARG; }
            const int hbeg_dev = (int)(t.hrec.size() / 4);
            const double *org = h_rec + 6 * (size_t)hb + 3;              // polytope origin = point of its first half-space
            t.horg.push_back(org[0]); t.horg.push_back(org[1]); t.horg.push_back(org[2]);
            for (int k = 0; k < K; k++) {                                // normalise outer normals, CPU.hpp:1116
                const double *rec = h_rec + 6 * (size_t)(hb + k);
                const double nn = std::sqrt(rec[0] * rec[0] + rec[1] * rec[1] + rec[2] * rec[2]);
                const double n0 = rec[0] / nn, n1 = rec[1] / nn, n2 = rec[2] / nn;
                t.hrec.push_back(n0); t.hrec.push_back(n1); t.hrec.push_back(n2);
                // n.(pos - p_k) + margin = n.(pos - org) - c   with   c = n.(p_k - org) - margin   (CPU.hpp:325,328)
                t.hrec.push_back(n0 * (rec[3] - org[0]) + n1 * (rec[4] - org[1]) + n2 * (rec[5] - org[2]) - cfg.safe_margin);
            }
            t.Kmax = std::max(t.Kmax, K);
            t.coarse_iv.push_back(hc.intervals[i]);
            t.coarse_fbeg.push_back(gp0 + offset);
            for (int j = 0; j < hc.intervals[i]; j++) {
                int vm = -1;
                if (j < hc.intervals[i] - 1) vm = 2 * i;
                else if (i < cN - 1) vm = 2 * i + 1;
                if (vm >= 0) {
                    const int nv = (int)(hc.cfgVs[vm].size() / 3);
                    t.wp_vbeg.push_back((int)(t.vrec.size() / 3)); t.wp_nv.push_back(nv); t.wp_xbeg.push_back(xcur);
                    t.vrec.insert(t.vrec.end(), hc.cfgVs[vm].begin(), hc.cfgVs[vm].end());   // waypoint order, contiguous per candidate
                    xcur += nv - 1;
                }
                t.piece_hbeg.push_back(hbeg_dev); t.piece_K.push_back(K); t.piece_coarse.push_back(gc0 + i); t.piece_iv.push_back(hc.intervals[i]);
                t.sumKfine += K;
                offset++;
            }
        }
        hpoly += cN;
        vpoly += 2 * cN - 1;
        t.dimT[b] = hc.dimT;
        t.poff[b + 1] = gp0 + hc.fineN;
        t.coff[b + 1] = gc0 + cN;
        t.xoff[b + 1] = t.xoff[b] + hc.dimT + hc.dimP;
        t.boff[b + 1] = t.boff[b] + 6 * hc.fineN * FRX_BAND_W;
        t.maxN = std::max(t.maxN, hc.fineN);
        t.maxCN = std::max(t.maxCN, cN);
    }
    t.cvoff[B] = (int)(t.vrec.size() / 3);
    t.P = t.poff[B]; t.Pc = t.coff[B]; t.NX = t.xoff[B];
    for (int b = 0; b < B; b++) {
        t.maxXb = std::max(t.maxXb, t.xoff[b + 1] - t.xoff[b]);
        t.maxVb = std::max(t.maxVb, 3 * (t.cvoff[b + 1] - t.cvoff[b]));
    }
    // per-piece corridor blocks, padded to Kmax
    const int hs = (t.Kmax + 1) * 4;
    t.hblk.assign((size_t)t.P * hs, 0.0);
    for (int gp = 0; gp < t.P; gp++) {
        double *blk = &t.hblk[(size_t)gp * hs];
        const int gc = t.piece_coarse[gp], K = t.piece_K[gp];
        blk[0] = t.horg[3 * (size_t)gc]; blk[1] = t.horg[3 * (size_t)gc + 1]; blk[2] = t.horg[3 * (size_t)gc + 2]; blk[3] = (double)K;
        std::memcpy(blk + 4, &t.hrec[4 * (size_t)t.piece_hbeg[gp]], sizeof(double) * 4 * K);
    }
    *why = TABLES_OK;
    return FRX_OK;
}

// ---- the launch geometry ----
// The environment of frx_problem_create as read once per handle (create_switches_from_env, frx_api.cpp); the defaults are the unset variables.
struct CreateSwitches {
    int penalty_waves = 0;                      // FRX_PENALTY_WAVES: 1..4 waves per workgroup of k_penalty
    char eval_fused = 0;                        // FRX_EVAL_FUSED, first character: '0' never the one-launch evaluation, '1' also on a device that local ranks share
    int local_ranks = 1;                        // FRX_LOCAL_RANKS, else LOCAL_WORLD_SIZE: processes of this node
    char eval_solo = 0;                         // FRX_EVAL_SOLO, first character: '0' never, '1' always
    int solo_min_B = 0, solo_max_B = 0;         // FRX_EVAL_SOLO_MIN_B / _MAX_B: > 0 moves the threshold
    double eval_timeout_ms = 0.0;               // FRX_EVAL_TIMEOUT_MS: > 0 bounds every wait inside the one-launch evaluation
    bool setup_timing = false;                  // FRX_SETUP_TIMING set
};

// Everything of LaunchGeom that is arithmetic on the tables' maxima: lanes and pieces per wave, the penalty workgroup, every LDS size of the stage kernels.  The
// one-launch and the solo form (ev_G / lds_ev, lds_solo) need the kernels' layout headers: eval_cluster_geometry and eval_solo_geometry fill them behind this.
inline void launch_geometry_fill(LaunchGeom &ge, const ProblemTables &t, int qd_intervals, int simds, int forced_waves) {
    const int spp = qd_intervals + 1;
    ge.maxN = t.maxN; ge.maxCN = t.maxCN; ge.Kmax = t.Kmax; ge.maxXb = t.maxXb; ge.maxVb = t.maxVb;
    ge.lpp = std::min(spp, 64);
    ge.ppw = 64 / ge.lpp;
    const PenaltyWaves pw = penalty_waves(ge.lpp, t.Kmax, t.P, simds, forced_waves);
    ge.pen_w = pw.pen_w; ge.ppg = pw.ppg;
    ge.lds_fwd = banded_fwd_lds_bytes(t.maxN, t.maxCN);
    ge.lds_bwd = banded_bwd_lds_bytes(t.maxN, t.maxCN);
    ge.lds_pen = pen_wg_bytes(ge.ppg, t.Kmax, ge.pen_w, 21);
    // large batches (four-wave workgroups), one sample per lane: the two-phase form of the integrator (k_penalty_lat2) - half the transpose buffer, four waves per SIMD
    ge.lds_pen2 = (ge.pen_w == 4 && spp <= 64) ? pen_wg_bytes(ge.ppg, t.Kmax, ge.pen_w, 11) : 0;
    ge.solver = SOLVER_KNOT_PCR;
    ge.knot_threads = knot_threads(t.maxN);
    ge.pcr_steps = pcr_steps(t.maxN);
    ge.lds_kfwd = knot_fwd_lds_bytes(ge.knot_threads, t.maxCN, t.maxXb, t.maxVb, ge.pcr_steps);
    ge.lds_kbwd = knot_bwd_lds_bytes(ge.knot_threads, t.maxCN, t.maxXb, t.maxVb, ge.pcr_steps);
}

} // namespace frx
