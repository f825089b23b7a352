// TEST INFRASTRUCTURE: a stand-alone host program around fast-racing_amd/csrc/frx_problem_tables.hpp and the geometry functions of frx_launch_forms.hpp, meant for
// a sanitizer build (make problem_tables_san).  It carries the table loop and the geometry block frx_problem_create had before the header existed - the code it
// replaced, on a plain struct in place of the handle and with the environment and the device's figures as arguments - and compares the new functions with it over
// random batches: every table, offset, maximum and size must be equal, the doubles bit for bit.  Exit status 0 and no sanitizer report is the result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <random>
#include <string>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_problem_tables.hpp"

using namespace frx;

// ---- the code it replaced ----
struct OldHandle {
    int B = 0, P = 0, Pc = 0, NX = 0, Kmax = 0, maxN = 0, maxCN = 0, sumKfine = 0;
    bool softT = true;
    std::vector<HostCand> cand;
    std::vector<int> poff, coff, xoff, boff, dimT;
    LaunchGeom geo = {};
    bool banded_ok = true;
    int eval_fused = 0, eval_fused_G = 0, eval_solo = 0, eval_solo_min_B = 0, eval_solo_max_B = 0;
    // what create kept in locals
    std::vector<int> piece_hbeg, piece_K, piece_coarse, piece_iv, coarse_iv, coarse_fbeg, wp_vbeg, wp_nv, wp_xbeg, cvoff;
    std::vector<double> hrec, horg, vrec, head, tail, hblk;
    int maxXb = 1, maxVb = 3;
};
enum { OLD_OK, OLD_COARSE_N, OLD_NO_VERTICES, OLD_NO_HALFSPACES, OLD_KNOT_CAPACITY, OLD_PENALTY_CAPACITY };

static int old_tables(OldHandle *p, const frx_config *cfg, int B, const int *coarse_n, const double *ini_state, const double *fin_state, const int *h_off,
                      const double *h_rec, const int *v_off, const double *v_rec) {
    p->B = B;
    p->softT = cfg->rho > 0;                                             // CPU.hpp:1097
    p->cand.resize(B);
    p->poff.assign(B + 1, 0); p->coff.assign(B + 1, 0); p->xoff.assign(B + 1, 0); p->boff.assign(B + 1, 0);
    p->dimT.assign(B, 0);

    std::vector<int> &piece_hbeg = p->piece_hbeg, &piece_K = p->piece_K, &piece_coarse = p->piece_coarse, &piece_iv = p->piece_iv, &coarse_iv = p->coarse_iv,
                     &coarse_fbeg = p->coarse_fbeg, &wp_vbeg = p->wp_vbeg, &wp_nv = p->wp_nv, &wp_xbeg = p->wp_xbeg, &cvoff = p->cvoff;
    cvoff.assign(B + 1, 0);
    std::vector<double> &hrec = p->hrec, &horg = p->horg, &vrec = p->vrec;
    p->head.assign(ini_state, ini_state + 9 * (size_t)B); p->tail.assign(fin_state, fin_state + 9 * (size_t)B);
    int hpoly = 0, vpoly = 0;                     // running polytope indices into h_off / v_off
    for (int b = 0; b < B; b++) {
        frx::HostCand &hc = p->cand[b];
        const int cN = coarse_n[b];
        if (cN < 1) return OLD_COARSE_N;
        // host description: V-polytopes as [v0, v_r - v0], gridMesh, waypoint index map, clipped boundary speeds (frx_host_setup.hpp)
        if (frx::host_cand_init(hc, *cfg, p->softT, cN, ini_state + 9 * (size_t)b, fin_state + 9 * (size_t)b, v_off + vpoly, v_rec) != FRX_OK) return OLD_NO_VERTICES;
        cvoff[b] = (int)(vrec.size() / 3);
        // index maps (CPU.hpp:1129-1152), expanded into per-piece / per-waypoint device descriptors
        const int gp0 = p->poff[b], gc0 = p->coff[b];
        int offset = 0;
        int xcur = p->xoff[b] + hc.dimT;
        for (int i = 0; i < cN; i++) {
            const int hb = h_off[hpoly + i], K = h_off[hpoly + i + 1] - hb;
            if (K < 1) return OLD_NO_HALFSPACES;
            const int hbeg_dev = (int)(hrec.size() / 4);
            const double *org = h_rec + 6 * (size_t)hb + 3;              // polytope origin = point of its first half-space
            horg.push_back(org[0]); horg.push_back(org[1]); horg.push_back(org[2]);
            for (int k = 0; k < K; k++) {                                // normalise outer normals, CPU.hpp:1116
                const double *rec = h_rec + 6 * (size_t)(hb + k);
                const double nn = std::sqrt(rec[0] * rec[0] + rec[1] * rec[1] + rec[2] * rec[2]);
                const double n0 = rec[0] / nn, n1 = rec[1] / nn, n2 = rec[2] / nn;
                hrec.push_back(n0); hrec.push_back(n1); hrec.push_back(n2);
                // n.(pos - p_k) + margin = n.(pos - org) - c   with   c = n.(p_k - org) - margin   (CPU.hpp:325,328)
                hrec.push_back(n0 * (rec[3] - org[0]) + n1 * (rec[4] - org[1]) + n2 * (rec[5] - org[2]) - cfg->safe_margin);
            }
            p->Kmax = std::max(p->Kmax, K);
            coarse_iv.push_back(hc.intervals[i]);
            coarse_fbeg.push_back(gp0 + offset);
            for (int j = 0; j < hc.intervals[i]; j++) {
                int vm = -1;
                if (j < hc.intervals[i] - 1) vm = 2 * i;
                else if (i < cN - 1) vm = 2 * i + 1;
                if (vm >= 0) {
                    const int nv = (int)(hc.cfgVs[vm].size() / 3);
                    wp_vbeg.push_back((int)(vrec.size() / 3)); wp_nv.push_back(nv); wp_xbeg.push_back(xcur);
                    vrec.insert(vrec.end(), hc.cfgVs[vm].begin(), hc.cfgVs[vm].end());   // waypoint order, contiguous per candidate
                    xcur += nv - 1;
                }
                piece_hbeg.push_back(hbeg_dev); piece_K.push_back(K); piece_coarse.push_back(gc0 + i); piece_iv.push_back(hc.intervals[i]);
                p->sumKfine += K;
                offset++;
            }
        }
        hpoly += cN;
        vpoly += 2 * cN - 1;
        p->dimT[b] = hc.dimT;
        p->poff[b + 1] = gp0 + hc.fineN;
        p->coff[b + 1] = gc0 + cN;
        p->xoff[b + 1] = p->xoff[b] + hc.dimT + hc.dimP;
        p->boff[b + 1] = p->boff[b] + 6 * hc.fineN * FRX_BAND_W;
        p->maxN = std::max(p->maxN, hc.fineN);
        p->maxCN = std::max(p->maxCN, cN);
    }
    cvoff[B] = (int)(vrec.size() / 3);
    p->P = p->poff[B]; p->Pc = p->coff[B]; p->NX = p->xoff[B];
    int maxXb = 1, maxVb = 3;
    for (int b = 0; b < B; b++) {
        maxXb = std::max(maxXb, p->xoff[b + 1] - p->xoff[b]);
        maxVb = std::max(maxVb, 3 * (cvoff[b + 1] - cvoff[b]));
    }
    p->maxXb = maxXb; p->maxVb = maxVb;
    {
        // per-piece corridor blocks, padded to Kmax: one contiguous, index-free read per piece in k_penalty
        const int hs = (p->Kmax + 1) * 4;
        std::vector<double> hblk((size_t)p->P * hs, 0.0);
        for (int gp = 0; gp < p->P; gp++) {
            double *blk = &hblk[(size_t)gp * hs];
            const int gc = piece_coarse[gp], K = piece_K[gp];
            blk[0] = horg[3 * (size_t)gc]; blk[1] = horg[3 * (size_t)gc + 1]; blk[2] = horg[3 * (size_t)gc + 2]; blk[3] = (double)K;
            std::memcpy(blk + 4, &hrec[4 * (size_t)piece_hbeg[gp]], sizeof(double) * 4 * K);
        }
        p->hblk.swap(hblk);
    }
    return OLD_OK;
}

// the environment and the device as the block met them: a variable is a string or null; G stands for eval_cluster_geometry's answer, lds_solo for eval_solo_geometry's
struct OldEnv { const char *penalty_waves, *eval_fused, *local_ranks, *local_world_size, *eval_solo, *solo_min_B, *solo_max_B; int cus, ndev, G; size_t lds_solo; };

static int old_geometry(OldHandle *p, const frx_config *cfg, int B, const OldEnv &env) {
    const int maxXb = p->maxXb, maxVb = p->maxVb, ndev = env.ndev;
    // launch geometry + LDS budgets
    const int spp = cfg->qd_intervals + 1;
    frx::LaunchGeom &ge = p->geo;
    ge.maxN = p->maxN; ge.maxCN = p->maxCN; ge.Kmax = p->Kmax;
    ge.lpp = std::min(spp, 64);
    ge.ppw = 64 / ge.lpp;
    {
        int best_w = 1; double best_u = 0.0;
        for (int w = 1; w <= 4; w++) {
            const double u = (double)((64 * w) / ge.lpp * ge.lpp) / (64.0 * w);
            if (u > best_u + 1e-9) { best_u = u; best_w = w; }
        }
        int simds = 1024;
        simds = 4 * env.cus;
        if ((p->P + ge.ppw - 1) / ge.ppw <= simds) best_w = 1;
        if (const char *pw = env.penalty_waves) { const int w = std::atoi(pw); if (w >= 1 && w <= 4) best_w = w; }
        while (best_w > 1 && frx::pen_wg_bytes((64 * best_w) / ge.lpp, p->Kmax, best_w, 21) > (size_t)160 * 1024) best_w--;
        ge.pen_w = best_w; ge.ppg = (64 * best_w) / ge.lpp;
    }
    ge.lds_fwd = sizeof(double) * ((size_t)6 * p->maxN * (FRX_BAND_W + 3) + p->maxN + p->maxCN);
    ge.lds_bwd = sizeof(double) * ((size_t)6 * p->maxN * (FRX_BAND_W + 6) + 2 * (size_t)p->maxN + p->maxCN);
    ge.lds_pen = frx::pen_wg_bytes(ge.ppg, p->Kmax, ge.pen_w, 21);
    ge.lds_pen2 = (ge.pen_w == 4 && spp <= 64) ? frx::pen_wg_bytes(ge.ppg, p->Kmax, ge.pen_w, 11) : 0;
    ge.solver = frx::SOLVER_KNOT_PCR;
    ge.knot_threads = 64 * ((p->maxN + 63) / 64);
    {
        const size_t nt = ge.knot_threads;
        ge.maxXb = maxXb; ge.maxVb = maxVb;
        ge.pcr_steps = 0;
        for (int s = 1; s < p->maxN - 1; s <<= 1) ge.pcr_steps++;
        ge.lds_kfwd = sizeof(double) * (36 * nt + 9 * (nt + 1) + nt + p->maxCN + maxXb + maxVb + (size_t)(ge.pcr_steps * 8 + 5) * nt);
        ge.pcr_steps = 0;
        for (int s = 1; s < p->maxN - 1; s <<= 1) ge.pcr_steps++;
        ge.lds_kbwd = sizeof(double) * (36 * nt + 9 * (nt + 1) + 2 * nt + p->maxCN + 2 * 4 + 2 + 2 * maxXb + maxVb + (size_t)(ge.pcr_steps * 8 + 5) * nt);
    }
    {   // one launch per evaluation when every cluster of the batch gets its CUs at once
        int cus = 256;
        cus = env.cus;
        const char *ef = env.eval_fused;
        const int G = env.G;
        ge.ev_G = G; ge.lds_ev = G ? 4096 : 0;
        int ranks = 1;
        if (const char *e = env.local_ranks) ranks = std::max(1, std::atoi(e));
        else if (const char *e2 = env.local_world_size) ranks = std::max(1, std::atoi(e2));
        const bool shared_device = ranks > ndev && !(ef && ef[0] == '1');
        if (!G || (long long)B * G > cus || (ef && ef[0] == '0') || shared_device) { ge.ev_G = 0; ge.lds_ev = 0; }
        p->eval_fused_G = ge.ev_G; p->eval_fused = ge.ev_G ? 1 : 0;
        ge.lds_solo = env.lds_solo;
        p->eval_solo = ge.lds_solo ? 1 : 0; p->eval_solo_min_B = 384; p->eval_solo_max_B = 512;
        if (const char *es = env.eval_solo) { if (es[0] == '0') p->eval_solo = 0; else if (es[0] == '1' && ge.lds_solo) p->eval_solo = 2; }
        if (const char *mb = env.solo_min_B) { const int v = std::atoi(mb); if (v > 0) p->eval_solo_min_B = v; }
        if (const char *mb = env.solo_max_B) { const int v = std::atoi(mb); if (v > 0) p->eval_solo_max_B = v; }
    }
    const size_t lds_cap = 160 * 1024;
    if (ge.knot_threads > 256 || ge.lds_kbwd > lds_cap) return OLD_KNOT_CAPACITY;
    // the banded-LU cross-check kernels need the whole band in LDS; fall back to "unavailable" instead of failing create
    p->banded_ok = !(ge.lds_bwd > lds_cap || ge.lds_fwd > lds_cap);
    if (!p->banded_ok) { ge.lds_fwd = ge.lds_bwd = 1024; }
    if (ge.lds_pen > lds_cap) return OLD_PENALTY_CAPACITY;
    return OLD_OK;
}

// ---- the new functions, put together as frx_problem_create puts them together ----
static CreateSwitches switches_of(const OldEnv &env) {
    CreateSwitches s;
    if (const char *e = env.penalty_waves) s.penalty_waves = std::atoi(e);
    if (const char *e = env.eval_fused) s.eval_fused = e[0];
    if (const char *e = env.local_ranks) s.local_ranks = std::max(1, std::atoi(e));
    else if (const char *e2 = env.local_world_size) s.local_ranks = std::max(1, std::atoi(e2));
    if (const char *e = env.eval_solo) s.eval_solo = e[0];
    if (const char *e = env.solo_min_B) s.solo_min_B = std::atoi(e);
    if (const char *e = env.solo_max_B) s.solo_max_B = std::atoi(e);
    return s;
}
static int new_geometry(OldHandle *p, const ProblemTables &tb, const frx_config *cfg, int B, const OldEnv &env) {
    const CreateSwitches sw = switches_of(env);
    LaunchGeom &ge = p->geo;
    launch_geometry_fill(ge, tb, cfg->qd_intervals, 4 * env.cus, sw.penalty_waves);
    ge.ev_G = env.G; ge.lds_ev = env.G ? 4096 : 0;
    if (!eval_cluster_admitted(env.G, B, env.cus, sw.eval_fused, sw.local_ranks, env.ndev)) { ge.ev_G = 0; ge.lds_ev = 0; }
    p->eval_fused_G = ge.ev_G; p->eval_fused = ge.ev_G ? 1 : 0;
    ge.lds_solo = env.lds_solo;
    const SoloChoice solo = eval_solo_choice(ge.lds_solo != 0, sw.eval_solo, sw.solo_min_B, sw.solo_max_B);
    p->eval_solo = solo.eval_solo; p->eval_solo_min_B = solo.min_B; p->eval_solo_max_B = solo.max_B;
    const GeomVerdict v = geometry_verdict(ge.knot_threads, ge.lds_kbwd, ge.lds_fwd, ge.lds_bwd, ge.lds_pen);
    if (v.refusal == GEOM_KNOT_CAPACITY) return OLD_KNOT_CAPACITY;
    if (v.refusal == GEOM_PENALTY_CAPACITY) return OLD_PENALTY_CAPACITY;
    p->banded_ok = v.banded_ok;
    if (!p->banded_ok) { ge.lds_fwd = ge.lds_bwd = 1024; }
    return OLD_OK;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static bool same_geometry(const OldHandle &a, const OldHandle &b, bool whole) {
    const LaunchGeom &g = a.geo, &h = b.geo;
    bool ok = g.maxN == h.maxN && g.maxCN == h.maxCN && g.Kmax == h.Kmax && g.lpp == h.lpp && g.ppw == h.ppw && g.pen_w == h.pen_w && g.ppg == h.ppg && g.lds_pen == h.lds_pen &&
              g.lds_pen2 == h.lds_pen2 && g.solver == h.solver && g.knot_threads == h.knot_threads && g.lds_kfwd == h.lds_kfwd && g.lds_kbwd == h.lds_kbwd && g.maxXb == h.maxXb &&
              g.maxVb == h.maxVb && g.pcr_steps == h.pcr_steps && g.ev_G == h.ev_G && g.lds_ev == h.lds_ev && g.lds_solo == h.lds_solo && a.eval_fused == b.eval_fused &&
              a.eval_fused_G == b.eval_fused_G && a.eval_solo == b.eval_solo && a.eval_solo_min_B == b.eval_solo_min_B && a.eval_solo_max_B == b.eval_solo_max_B;
    // (a refused handle is deleted: whether its banded sizes had been replaced by then is nothing anybody sees)
    return ok && (!whole || (a.banded_ok == b.banded_ok && g.lds_fwd == h.lds_fwd && g.lds_bwd == h.lds_bwd));
}

int main(int argc, char **argv) {
    const int batches = argc > 1 ? std::atoi(argv[1]) : 4000;
    std::mt19937_64 rng(20240607);
    auto ri = [&](int lo, int hi) { return (int)(lo + rng() % (unsigned long long)(hi - lo + 1)); };
    auto pick = [&](std::initializer_list<int> l) { return *(l.begin() + ri(0, (int)l.size() - 1)); };
    auto rd = [&](double lo, double hi) { return lo + (hi - lo) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); };
    static const char *const waves[] = {nullptr, "0", "1", "2", "3", "4", "5", "x"};
    static const char *const chars[] = {nullptr, "", "0", "1", "2"};
    static const char *const ranks[] = {nullptr, "0", "1", "2", "8", "9"};
    static const char *const bounds[] = {nullptr, "0", "-3", "1", "200", "4096"};
    int bad = 0, tables[6] = {0, 0, 0, 0, 0, 0}, geoms[6] = {0, 0, 0, 0, 0, 0};
    for (int it = 0; it < batches; it++) {
        const int B = ri(1, 8);
        frx_config cfg = {};
        cfg.rho = ri(0, 1) ? 1000.0 : 0.0; cfg.total_t = 10.0; cfg.grid_res = rd(0.5, 4.0); cfg.qd_intervals = pick({8, 16, 48, 63, 64, 100});
        cfg.vel_max = rd(1.0, 20.0); cfg.safe_margin = rd(0.0, 0.5);
        // one batch in a hundred carries each refusal somewhere
        const int spoil = ri(0, 99) < 3 ? ri(1, 3) : 0, spoil_b = ri(0, B - 1);
        std::vector<int> coarse_n(B), h_off(1, 0), v_off(1, 0);
        std::vector<double> ini(9 * (size_t)B), fin(9 * (size_t)B), h_rec, v_rec;
        for (int b = 0; b < B; b++) {
            const int cN = coarse_n[b] = (spoil == 1 && b == spoil_b) ? ri(-1, 0) : ri(1, 6);
            for (int q = 0; q < 9; q++) { ini[9 * b + q] = rd(-3.0, 3.0); fin[9 * b + q] = rd(-3.0, 3.0); }
            double at[3] = {ini[9 * b], ini[9 * b + 1], ini[9 * b + 2]};
            for (int i = 0; i < std::max(cN, 0); i++) {
                int K = ri(0, 9) ? ri(1, 12) : ri(13, 48);
                if (spoil == 3 && b == spoil_b && i == cN - 1) K = 0;
                for (int k = 0; k < K; k++) for (int q = 0; q < 6; q++) h_rec.push_back(q < 3 ? rd(-5.0, 5.0) + (q == k % 3 ? 6.0 : 0.0) : rd(-20.0, 20.0));
                h_off.push_back(h_off.back() + K);
            }
            for (int m = 0; m < 2 * cN - 1; m++) {
                // the overlap polytopes lie up to five grid cells apart: intervals 1..5 (and the last one as far as the final state happens to be)
                if (m & 1) { const double step = rd(0.01, 5.0) * cfg.grid_res; at[ri(0, 2)] += step; }
                int nv = ri(1, 9);
                if (spoil == 2 && b == spoil_b && m == ri(0, 2 * cN - 2)) nv = 0;
                for (int a = 0; a < nv; a++) for (int q = 0; q < 3; q++) v_rec.push_back(at[q] + rd(-0.2, 0.2));
                v_off.push_back(v_off.back() + nv);
            }
            if (cN >= 1 && ri(0, 1)) for (int q = 0; q < 3; q++) fin[9 * b + q] = at[q] + rd(0.0, 2.0) * cfg.grid_res;
        }
        h_rec.resize(h_rec.size() + 6, 0.0); v_rec.resize(v_rec.size() + 3, 0.0);       // (never empty: the pointers below are those of real arrays)

        OldHandle old;
        const int rc_old = old_tables(&old, &cfg, B, coarse_n.data(), ini.data(), fin.data(), h_off.data(), h_rec.data(), v_off.data(), v_rec.data());
        std::vector<HostCand> cand;
        ProblemTables tb;
        TablesRefusal why;
        const int rc_new = problem_tables_fill(cfg, cfg.rho > 0, B, coarse_n.data(), ini.data(), fin.data(), h_off.data(), h_rec.data(), v_off.data(), v_rec.data(), cand, tb, &why);
        const int want_why[4] = {TABLES_OK, TABLES_COARSE_N, TABLES_NO_VERTICES, TABLES_NO_HALFSPACES};
        const int want_rc[4] = {FRX_OK, FRX_ERR_INVALID_ARG, FRX_ERR_EMPTY_POLYTOPE, FRX_ERR_INVALID_ARG};
        tables[rc_old]++;
        if ((int)why != want_why[rc_old] || rc_new != want_rc[rc_old]) { bad++; std::printf("batch %d: refusal %d against %d (code %d)\n", it, (int)why, rc_old, rc_new); continue; }
        if (rc_old != OLD_OK) continue;
        const bool tables_ok = same(tb.poff, old.poff) && same(tb.coff, old.coff) && same(tb.xoff, old.xoff) && same(tb.boff, old.boff) && same(tb.cvoff, old.cvoff) &&
            same(tb.dimT, old.dimT) && same(tb.piece_hbeg, old.piece_hbeg) && same(tb.piece_K, old.piece_K) && same(tb.piece_coarse, old.piece_coarse) &&
            same(tb.piece_iv, old.piece_iv) && same(tb.coarse_iv, old.coarse_iv) && same(tb.coarse_fbeg, old.coarse_fbeg) && same(tb.wp_vbeg, old.wp_vbeg) &&
            same(tb.wp_nv, old.wp_nv) && same(tb.wp_xbeg, old.wp_xbeg) && same(tb.hrec, old.hrec) && same(tb.horg, old.horg) && same(tb.vrec, old.vrec) &&
            same(tb.head, old.head) && same(tb.tail, old.tail) && same(tb.hblk, old.hblk) && tb.P == old.P && tb.Pc == old.Pc && tb.NX == old.NX && tb.Kmax == old.Kmax &&
            tb.maxN == old.maxN && tb.maxCN == old.maxCN && tb.sumKfine == old.sumKfine && tb.maxXb == old.maxXb && tb.maxVb == old.maxVb;
        if (!tables_ok) { bad++; std::printf("batch %d: the tables differ\n", it); continue; }

        // the geometry of this batch, and of the same batch with its maxima moved to the edges of the knot kernels and the penalty workgroup
        for (int edge = 0; edge < 4; edge++) {
            ProblemTables te = tb;                // (only the maxima are read)
            OldHandle oe; oe.P = old.P; oe.maxN = old.maxN; oe.maxCN = old.maxCN; oe.Kmax = old.Kmax; oe.maxXb = old.maxXb; oe.maxVb = old.maxVb;
            if (edge) {
                te.maxN = oe.maxN = pick({1, 2, 3, 63, 64, 65, 66, 100, 127, 128, 129, 255, 256, 257});
                te.maxCN = oe.maxCN = ri(1, te.maxN);
                te.Kmax = oe.Kmax = edge == 2 ? ri(200, 1400) : ri(1, 48);
                te.P = oe.P = ri(te.maxN, 8 * te.maxN) * (edge == 3 ? 64 : 1);
                te.maxXb = oe.maxXb = ri(1, 12 * te.maxN); te.maxVb = oe.maxVb = 3 * ri(1, 9 * te.maxN);
            }
            OldEnv env = {waves[ri(0, 7)], chars[ri(0, 4)], ranks[ri(0, 5)], ranks[ri(0, 5)], chars[ri(0, 4)], bounds[ri(0, 5)], bounds[ri(0, 5)], pick({8, 64, 256, 304}),
                          ri(1, 8), ri(0, 3) ? ri(1, 40) : 0, ri(0, 2) ? (size_t)ri(1, 160) * 1024 : 0};
            const int Bg = edge ? ri(1, 600) : B;
            OldHandle ne;
            const int g_old = old_geometry(&oe, &cfg, Bg, env), g_new = new_geometry(&ne, te, &cfg, Bg, env);
            geoms[g_old]++;
            if (g_old != g_new || !same_geometry(oe, ne, g_old == OLD_OK)) { bad++; std::printf("batch %d, edge %d: the geometry differs (%d against %d)\n", it, edge, g_new, g_old); }
        }
    }
    std::printf("%d batches: %d with tables, %d coarse_n, %d vertex and %d half-space refusals; geometries: %d fit, %d knot and %d penalty refusals; %d disagreements with the code it replaced\n",
                batches, tables[OLD_OK], tables[OLD_COARSE_N], tables[OLD_NO_VERTICES], tables[OLD_NO_HALFSPACES], geoms[OLD_OK], geoms[OLD_KNOT_CAPACITY], geoms[OLD_PENALTY_CAPACITY], bad);
    return bad ? 1 : 0;
}
