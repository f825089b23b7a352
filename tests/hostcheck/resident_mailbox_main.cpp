// TEST INFRASTRUCTURE - the host's side of the resident kernel's mailbox protocol (fast-racing_amd/csrc/frx_resident_mailbox.hpp) without a device: a plain
// std::thread plays the clusters over ordinary host memory.  It reads each command word, executes the command on a host emulation of the device vectors (the
// loops of hostcheck_lbfgs_dv, on a small quadratic per candidate), answers with the result and the command's sequence number, and honours DV_NEXT and DV_QUIT.
// tests/test_resident_mailbox_cpu.py drives hostcheck_resident_mailbox_case through libhostcheck.so; built alone (make resident_mailbox_san) the same cases run
// under the address and undefined-behaviour sanitizers.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_resident_mailbox.hpp"

namespace rmb {

typedef unsigned long long u64;

// one candidate's vectors as the device would hold them, and its objective f(x) = sum_i a_i (x_i - c_i)^2 / 2
struct Emu {
    int n = 0, m = 0;
    std::vector<double> a, c, x, g, xp, gp, d, S, Y, ys, al;
    double res[5] = {0, 0, 0, 0, 0};                                   // f, dg, xx, gg, dginit (the last one stays until the next INIT / ADVANCE)
    void init(int n_, int m_, int seed) {
        n = n_; m = m_;
        a.resize(n); c.resize(n); x.assign(n, 0.0); g.assign(n, 0.0); xp = gp = d = g;
        S.assign((size_t)m * n, 0.0); Y = S; ys.assign(m, 0.0); al = ys;
        for (int i = 0; i < n; i++) { a[i] = 1.0 + 0.37 * ((i * 7 + seed * 3) % 11); c[i] = 0.25 * ((i * 5 + seed) % 9) - 1.0; x[i] = 0.5 * ((i + 2 * seed) % 5); }
    }
    double dot(const double *p, const double *q) const { double s = 0.; for (int i = 0; i < n; ++i) s += p[i] * q[i]; return s; }
    void axpy(double *y, const double *v, double k) const { for (int i = 0; i < n; ++i) y[i] += k * v[i]; }
    void exec(int flags, int slot, int bound, double step) {
        if (flags & frx::DV_RESTORE) { x = xp; g = gp; return; }
        if (flags & frx::DV_INIT) { for (int i = 0; i < n; ++i) d[i] = -g[i]; xp = x; gp = g; res[4] = dot(gp.data(), d.data()); }
        if (flags & frx::DV_ADVANCE) {
            double *se = &S[(size_t)slot * n], *ye = &Y[(size_t)slot * n];
            for (int i = 0; i < n; ++i) { se[i] = x[i] - xp[i]; ye[i] = g[i] - gp[i]; }
            const double y_s = dot(ye, se), y_y = dot(ye, ye);
            ys[slot] = y_s;
            for (int i = 0; i < n; ++i) d[i] = -g[i];
            int j = (slot + 1) % m;
            for (int it = 0; it < bound; ++it) { j = (j + m - 1) % m; al[j] = dot(&S[(size_t)j * n], d.data()) / ys[j]; axpy(d.data(), &Y[(size_t)j * n], -al[j]); }
            for (int i = 0; i < n; ++i) d[i] *= y_s / y_y;
            for (int it = 0; it < bound; ++it) { const double beta = dot(&Y[(size_t)j * n], d.data()) / ys[j]; axpy(d.data(), &S[(size_t)j * n], al[j] - beta); j = (j + 1) % m; }
            xp = x; gp = g; res[4] = dot(gp.data(), d.data());
        }
        if (flags & frx::DV_TRIAL) { x = xp; axpy(x.data(), d.data(), step); }
        if (flags & frx::DV_EVAL) {
            double f = 0.0;
            for (int i = 0; i < n; ++i) { const double r = x[i] - c[i]; f += 0.5 * a[i] * r * r; g[i] = a[i] * r; }
            res[0] = f; res[1] = dot(g.data(), d.data()); res[2] = dot(x.data(), x.data()); res[3] = dot(g.data(), g.data());
        }
    }
};

inline frx_lbfgs_params params() { frx_lbfgs_params pm; frx::lbfgs_defaults(pm); pm.mem_size = 4; pm.max_iterations = 60; return pm; }
inline int cand_n(int b) { return 6 + b % 3; }

// a candidate's plan with nobody between the solver and the vectors, up to `rounds` commands (< 0: to its end)
struct Solo { int status, iters, evals; double value; };
inline Solo solo(frx::SolverDV &sv, frx::DvCommand &cmd, Emu &e, long rounds) {
    for (long r = 0; cmd.flags != 0 && (rounds < 0 || r < rounds); r++) {
        const frx::DvCommand c = cmd;
        e.exec(c.flags, c.slot, c.bound, c.step);
        if (c.flags & frx::DV_EVAL) { frx::DvResult res; std::memcpy(&res, e.res, sizeof(e.res)); sv.feed(res); } else cmd.flags = 0;
    }
    return {sv.status(), sv.iterations(), sv.evaluations(), sv.value()};
}

enum { NORMAL = 0, INVALID = 1, TAKEOVER = 2, GIVES_UP = 3, SILENT_LEFT = 4, SILENT_TIMEOUT = 5 };

// the clusters: what a command word carries is all they know (flags, slot, pair count; the step from the second word)
struct Clusters {
    int S; volatile u64 *hc, *hr; size_t cs2;
    std::vector<Emu> *emu; std::vector<int> cand;                      // the candidate each cluster is bound to
    int odd = -1, odd_mode = NORMAL;                                   // cluster `odd` gives up on its second command / never answers
    std::vector<int> quits, ncmd, next_seen;                           // per cluster: DV_QUIT words, commands; per candidate: DV_NEXT words that named it
    void run() {
        std::vector<u64> last(S, 0);
        int left = S;
        while (left > 0)
            for (int k = 0; k < S; k++) {
                const u64 w = hc[cs2 * k];
                if ((w >> 32) == last[k]) continue;
                std::atomic_thread_fence(std::memory_order_acquire);
                if (quits[k] == 0 && (w >> 32) != last[k] + 1) { quits[k] = -1000; left--; last[k] = w >> 32; continue; }   // a sequence number was skipped
                last[k] = w >> 32;
                const int flags = (int)(w & 0xFF), slot = (int)((w >> 8) & 0xFFF), bound = (int)((w >> 20) & 0xFFF);
                if (flags & frx::DV_QUIT) { if (quits[k]++ == 0) left--; continue; }
                ncmd[k]++;
                if (k == odd && odd_mode != GIVES_UP) continue;                                                // silent
                if (k == odd && ncmd[k] == 2) { hr[8 * k + 7] = ~0ull; continue; }
                if (flags & frx::DV_NEXT) { cand[k] = slot | (bound << 12); next_seen[cand[k]]++; }
                else {
                    double step;
                    std::memcpy(&step, (const void *)(hc + cs2 * k + 1), sizeof(double));
                    Emu &e = (*emu)[cand[k]];
                    e.exec(flags, slot, bound, step);
                    std::memcpy((void *)(hr + 8 * k), e.res, sizeof(e.res));
                }
                std::atomic_thread_fence(std::memory_order_release);
                hr[8 * k + 7] = last[k];
            }
    }
};

} // namespace rmb

// One case.  S clusters, B candidates, nsrv service threads; mode / arg: NORMAL; INVALID: candidate arg has no variables; TAKEOVER: the S candidates
// 1, 3, 5, .. continue after arg commands each with nobody in between; GIVES_UP / SILENT_LEFT / SILENT_TIMEOUT: cluster arg writes ~0 on its second command / never
// answers with the "kernel has left" probe true / false.  Out: status, iters, evals [B] (-77 where nothing was recorded), objective [B], solo4 [B][4]: the same plan
// with nobody in between (status, iters, evals, objective), next_seen [B], quits [S].  Returns the abort code.
extern "C" int hostcheck_resident_mailbox_case(int S, int B, int nsrv, int mode, int arg, double timeout_ms, int cmd_stride, int *status, int *iters, int *evals,
                                               double *objective, double *solo4, int *next_seen, int *quits) {
    using namespace rmb;
    const frx_lbfgs_params pm = params();
    std::vector<int> xoff(B + 1, 0);
    for (int b = 0; b < B; b++) xoff[b + 1] = xoff[b] + (mode == INVALID && b == arg ? 0 : cand_n(b));
    std::vector<Emu> emu(B), emu_solo(B);
    for (int b = 0; b < B; b++) {
        const int n = xoff[b + 1] - xoff[b];
        emu[b].init(n, pm.mem_size, b); emu_solo[b].init(n, pm.mem_size, b);
        frx::SolverDV sv; frx::DvCommand cmd;
        sv.start(n, pm, &cmd);
        const Solo s = solo(sv, cmd, emu_solo[b], -1);
        solo4[4 * b] = s.status; solo4[4 * b + 1] = s.iters; solo4[4 * b + 2] = s.evals; solo4[4 * b + 3] = s.value;
        status[b] = iters[b] = evals[b] = -77; objective[b] = -77.0;
    }
    const size_t cs2 = 2 * (size_t)cmd_stride;
    std::vector<u64> cmd_words(cs2 * S, 0), res_words((size_t)8 * S, 0);
    frx::ResidentMailbox mb(S, B, xoff.data(), pm, cmd_words.data(), res_words.data(), cmd_stride, {status, iters, evals, objective, nullptr});
    Clusters cl{S, cmd_words.data(), res_words.data(), cs2, &emu, std::vector<int>(S), -1, NORMAL, std::vector<int>(S, 0), std::vector<int>(S, 0), std::vector<int>(B, 0)};
    if (mode >= GIVES_UP) { cl.odd = arg; cl.odd_mode = mode; }
    if (mode == TAKEOVER) {
        std::vector<int> cand; std::vector<frx::SolverDV> svs(S); std::vector<frx::DvCommand> cmds(S);
        for (int k = 0; k < S; k++) {
            cand.push_back(2 * k + 1); cl.cand[k] = 2 * k + 1;
            svs[k].start(cand_n(2 * k + 1), pm, &cmds[k]);
            (void)solo(svs[k], cmds[k], emu[2 * k + 1], arg);
        }
        mb.start_takeover(cand, svs);
    } else {
        for (int k = 0; k < S; k++) cl.cand[k] = k;
        mb.start();
    }
    std::thread device([&] { cl.run(); });
    mb.post_first();
    {
        std::vector<std::thread> helpers;
        auto serve = [&](int tid) { (void)mb.serve(tid, nsrv, timeout_ms, 0, [mode] { return mode == SILENT_LEFT; }); };
        for (int tid = 1; tid < nsrv; tid++) helpers.emplace_back(serve, tid);
        serve(0);
        for (auto &h : helpers) h.join();
    }
    mb.quit_all();
    device.join();
    for (int b = 0; b < B; b++) next_seen[b] = cl.next_seen[b];
    for (int k = 0; k < S; k++) quits[k] = cl.quits[k];
    return mb.abort_code();
}

#ifndef HOSTCHECK_LIBRARY
// the cases of tests/test_resident_mailbox_cpu.py with their checks, as a program of its own (the sanitizer build)
static int check(const char *name, int S, int B, int nsrv, int mode, int arg, double timeout_ms, int stride, int want_abort) {
    std::vector<int> status(B), iters(B), evals(B), next_seen(B), quits(S);
    std::vector<double> objective(B), solo4(4 * (size_t)B);
    const int abort_code = hostcheck_resident_mailbox_case(S, B, nsrv, mode, arg, timeout_ms, stride, status.data(), iters.data(), evals.data(), objective.data(), solo4.data(), next_seen.data(), quits.data());
    int bad = abort_code != want_abort;
    for (int k = 0; k < S; k++) bad += quits[k] != 1;
    for (int b = 0; b < B && want_abort == 0; b++) {
        const bool ran = mode != rmb::TAKEOVER || (b % 2 == 1 && b < 2 * S);
        if (!ran) { bad += status[b] != -77; continue; }
        bad += status[b] != (int)solo4[4 * b] || iters[b] != (int)solo4[4 * b + 1] || evals[b] != (int)solo4[4 * b + 2] || objective[b] != solo4[4 * b + 3];
        bad += next_seen[b] != (mode != rmb::TAKEOVER && b >= S ? 1 : 0);
    }
    std::printf("%-40s abort %d %s\n", name, abort_code, bad ? "FAILED" : "ok");
    return bad;
}
int main() {
    int bad = 0;
    bad += check("one cluster, one candidate", 1, 1, 1, rmb::NORMAL, 0, 2000.0, 4, 0);
    bad += check("queue, one service thread", 2, 5, 1, rmb::NORMAL, 0, 2000.0, 4, 0);
    bad += check("queue, two service threads", 2, 5, 2, rmb::NORMAL, 0, 2000.0, 4, 0);
    bad += check("queue, command stride 1", 2, 5, 2, rmb::NORMAL, 0, 2000.0, 1, 0);
    bad += check("first candidate invalid", 2, 5, 1, rmb::INVALID, 0, 2000.0, 4, 0);
    bad += check("queued candidate invalid", 2, 5, 2, rmb::INVALID, 3, 2000.0, 4, 0);
    bad += check("take-over after 3 commands", 2, 5, 1, rmb::TAKEOVER, 3, 2000.0, 4, 0);
    bad += check("a cluster gives up", 2, 5, 1, rmb::GIVES_UP, 1, 2000.0, 4, 1);
    bad += check("silent cluster, kernel has left", 2, 5, 1, rmb::SILENT_LEFT, 1, 2000.0, 4, 1);   // (one thread: the probe is thread 0's, while it still has a cluster waiting)
    bad += check("silent cluster, host deadline", 2, 5, 1, rmb::SILENT_TIMEOUT, 0, 50.0, 4, 2);
    return bad ? 1 : 0;
}
#endif
