// The host's side of the resident round kernel's mailbox protocol (frx_round_kernel.hpp: RoundCmd, RoundRes): one SolverDV per cluster, its commands posted the
// moment the cluster's result arrives, the work queue (DV_NEXT) and the quit hand-shake.  Plain C++ over two arrays of 64-bit words - no HIP - so the driver
// (frx_optimize.cpp) runs it over mapped host memory against the device and tests/hostcheck/resident_mailbox_main.cpp over ordinary memory against a thread.
#pragma once
#include <atomic>
#include <chrono>
#include <cstring>
#include <vector>

#include "frx_lbfgs.hpp"
#include "frx_resident_plan.hpp"

namespace frx {

class ResidentMailbox {
public:
    // Host state per CLUSTER, one cache-line-aligned slot each and a CONTIGUOUS range of slots per service thread: with the state in
    // parallel arrays and candidate b served by thread b % nsrv (round 2), every line of `seq`, `waiting`, `cmd` and the solvers was
    // written by all threads - two service threads answered SLOWER than one (leader's wait for a command at 32 candidates: median
    // 8-16 us with two threads, 4-8 us with one, 2-4 us at 8 candidates; profiles/r03_hostwait_probe.jsonl) and more threads bought nothing.
    // A slot holds the solver of the candidate its cluster is working on; with more candidates than clusters (S < B) a slot whose
    // candidate is finished takes the next one of the batch (`next_cand`) and tells the cluster with DV_NEXT.
    struct alignas(128) Slot { SolverDV sv; DvCommand cmd; unsigned long long seq = 0; long ncmd = 0; int cand = -1; char waiting = 0, quit_sent = 0, switching = 0; };
    // where a finished plan is recorded, [B] each (status required); trace (optional): {flags, step, f, dg, dginit, xx, gg} per evaluation of candidate 0
    struct Out { int *status, *iters, *evals; double *objective; std::vector<double> *trace; };
    struct ServeStats { long scans = 0; double busy_ms = 0.0; };

    // cmd: [S] x 2 cmd_stride words (word, step), res: [S] x 8 words (f, dg, xx, gg, dginit, -, -, seq); xoff: [B + 1] offsets of the candidates' vectors
    ResidentMailbox(int S_, int B_, const int *xoff_, const frx_lbfgs_params &pm_, volatile unsigned long long *cmd, volatile unsigned long long *res, int cmd_stride, Out out_)
        : S(S_), B(B_), xoff(xoff_), pm(pm_), hc(cmd), hr(res), cs2(2 * (size_t)cmd_stride), out(out_), slot_(S_), next_cand(S_) {}

    // a plan from its start: cluster k begins with candidate k, the others wait in the queue
    void start() {
        for (int k = 0; k < S; k++) { slot_[k].cand = k; slot_[k].sv.start(xoff[k + 1] - xoff[k], pm, &slot_[k].cmd); }
    }
    // a take-over: cluster k continues candidate cand[k] with the solver the per-stage rounds drove (the pending command comes along); nobody is handed a further candidate
    void start_takeover(const std::vector<int> &cand, const std::vector<SolverDV> &sv) {
        next_cand.store(B);
        for (int k = 0; k < S; k++) { slot_[k].cand = cand[k]; slot_[k].sv = sv[k]; slot_[k].sv.rebind(&slot_[k].cmd); }
    }
    // once the kernel is launched: every cluster's first command (invalid parameters - nothing to run - hand the cluster on at once)
    void post_first() {
        for (int k = 0; k < S; k++) {
            if (slot_[k].cmd.flags != 0) { post(k, slot_[k].cmd.flags, slot_[k].cmd.slot, slot_[k].cmd.bound, slot_[k].cmd.step); slot_[k].waiting = 1; }
            else hand_over(k);
        }
    }

    void post(int k, int flags, int slot, int bound, double step) {
        std::memcpy((void *)(hc + cs2 * k + 1), &step, sizeof(double));
        std::atomic_thread_fence(std::memory_order_release);
        ++slot_[k].seq;
        hc[cs2 * k] = round_command_word(slot_[k].seq, flags, slot, bound, step);
        slot_[k].ncmd++;
    }
    void record(int k) {                                                             // the finished plan of slot k's candidate (the point itself is read from the device at the end)
        const int b = slot_[k].cand;
        out.status[b] = slot_[k].sv.status();
        if (out.iters) out.iters[b] = slot_[k].sv.iterations();
        if (out.evals) out.evals[b] = slot_[k].sv.evaluations();
        if (out.objective) out.objective[b] = slot_[k].sv.value();
    }
    // slot k's candidate is finished (or had nothing to run): the next candidate of the batch for its cluster, or DV_QUIT.  Returns true
    // while the slot has work.
    bool hand_over(int k) {
        record(k);
        const int nb = next_cand.load(std::memory_order_relaxed) < B ? next_cand.fetch_add(1) : B;
        if (nb >= B) { post(k, DV_QUIT, 0, 0, 0.0); slot_[k].quit_sent = 1; slot_[k].waiting = 0; return false; }   // this cluster leaves the chip
        slot_[k].cand = nb;
        slot_[k].sv.start(xoff[nb + 1] - xoff[nb], pm, &slot_[k].cmd);
        post(k, DV_NEXT, nb & 0xFFF, nb >> 12, 0.0);                                 // the cluster re-binds and answers with the command's sequence number
        slot_[k].switching = 1; slot_[k].waiting = 1;
        return true;
    }

    // Mailbox service: thread tid serves the clusters [S tid / nsrv, S (tid + 1) / nsrv) until each has been told to quit or the plan is aborted.  The clusters
    // of a batch run in near lock-step, so their results arrive together and a thread's k-th mailbox waits for the k - 1 before it.
    // kernel_left(): has the kernel gone?  Asked by thread 0 alone, every 16384 idle scans.
    template <class KernelLeft> ServeStats serve(int tid, int nsrv, double timeout_ms, int scan_pause, KernelLeft &&kernel_left) {
        using clk = std::chrono::steady_clock;
        auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
        ServeStats st;
        int mine = 0;
        long nscan = 0;
        const int lo = (int)((long)S * tid / nsrv), hi = (int)((long)S * (tid + 1) / nsrv);      // this thread's clusters
        for (int k = lo; k < hi; k++) mine += slot_[k].waiting ? 1 : 0;
        auto t_last = clk::now();
        while (mine > 0 && abort_.load(std::memory_order_relaxed) == 0) {
            bool progress = false;
            nscan++;
            for (int k = lo; k < hi; k++) {
                if (!slot_[k].waiting) continue;
                const unsigned long long rs = hr[8 * k + 7];
                if (rs == ~0ull) { abort_.store(1); break; }                            // the device gave up on this cluster
                if (rs != slot_[k].seq) continue;
                std::atomic_thread_fence(std::memory_order_acquire);
                progress = true;
                const auto th = clk::now();
                DvCommand &c = slot_[k].cmd;
                if (slot_[k].switching) slot_[k].switching = 0;                         // the cluster is on its new candidate: c holds the first command of that plan (SolverDV::start)
                else if (c.flags & DV_EVAL) {
                    DvResult r;
                    std::memcpy(&r, (const void *)(hr + 8 * k), 5 * sizeof(double));
                    if (out.trace && slot_[k].cand == 0) { const double row[7] = {(double)c.flags, c.step, r.f, r.dg, r.dginit, r.xx, r.gg}; out.trace->insert(out.trace->end(), row, row + 7); }
                    if (slot_[k].sv.saw_nonfinite(r.f)) slot_[k].sv.give_up(LBERR_ROUNDING); else slot_[k].sv.feed(r);
                } else c.flags = 0;                                                     // a RESTORE has been executed
                if (c.flags != 0) post(k, c.flags, c.slot, c.bound, c.step);
                else if (!hand_over(k)) mine--;
                st.busy_ms += ms_since(th);
            }
            if (progress) t_last = clk::now();
            else if (ms_since(t_last) > timeout_ms) abort_.store(2);
            else {
                // a kernel that has LEFT while clusters still wait (start-up census failed: the grid did not fit next to another
                // process's work; a device fault) will never answer: notice it instead of sitting out the whole timeout
                if (tid == 0 && (nscan & 0x3FFF) == 0 && kernel_left()) {
                    bool answered = true;
                    for (int k = 0; k < S; k++) if (slot_[k].waiting && hr[8 * k + 7] != slot_[k].seq) answered = false;
                    if (!answered) abort_.store(1);
                }
                for (int q = 0; q <= scan_pause; q++) __builtin_ia32_pause();
            }
        }
        st.scans = nscan;
        return st;
    }
    // after the service: DV_QUIT for every cluster that has not been told yet (an aborted plan)
    void quit_all() { for (int k = 0; k < S; k++) if (!slot_[k].quit_sent) { post(k, DV_QUIT, 0, 0, 0.0); slot_[k].quit_sent = 1; } }

    int abort_code() const { return abort_.load(); }                                 // 0, 1 = the device gave up, 2 = no result within the timeout
    long busiest() const { long n = 0; for (const Slot &s : slot_) n = std::max(n, s.ncmd); return n; }   // commands of the busiest cluster (S < B: over all the candidates it took)
    const Slot &slot(int k) const { return slot_[k]; }

private:
    const int S, B;
    const int *xoff;
    const frx_lbfgs_params pm;
    volatile unsigned long long *hc, *hr;
    const size_t cs2;
    Out out;
    std::vector<Slot> slot_;
    std::atomic<int> next_cand;
    std::atomic<int> abort_{0};
};

} // namespace frx
