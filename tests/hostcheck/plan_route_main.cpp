// TEST INFRASTRUCTURE: the route of a plan (fast-racing_amd/csrc/frx_plan_route.hpp) against drivers played from a script.  Two uses:
//  - included by hostcheck.cpp (HOSTCHECK_LIBRARY): hostcheck_plan_route and the decisions as integers, for tests/test_plan_route_cpu.py;
//  - a stand-alone host program meant for a sanitizer build (make plan_route_san && ./plan_route_san): the route and the ladder frx_optimize carried before the
//    header existed, copied below and adapted only to call the scripted drivers, over a few thousand random scripts; calls, arrays, counters and stats must agree.
//    Exit status 0 and no sanitizer report is the result.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_plan_route.hpp"

namespace plan_route_check {

// What the drivers do at their k-th call, whichever of the two it is: the code they return, the device status a resident call leaves, every candidate's verdict,
// who is still running when a per-stage call hands over (rc 2), and the four times of a call that ran.
struct Script {
    int B; const int *xoff; int n_calls;
    const int *rc; const unsigned *dev; const int *status; const unsigned char *hand; const double *times;
    int cap;                                  // what capacity() answers; negative: the device cannot be asked
};
constexpr int LOG_HEAD = 4;                   // a log row: kind (0 resident, 1 per stage), take passed, its capacity, its not_before, then only[b] (-1: no `only`);
                                              // beside it in `found`: the first element of every candidate's x as the call found it

struct ScriptedPaths {
    const Script &s; frx::PlanArrays out; frx::PlanCounters c; frx::PlanTimes *times;
    unsigned dev_status = 0;
    int k = 0, cap_asked = 0, err_code = 0;
    std::string err;
    std::vector<int> log;
    std::vector<double> found;
    ScriptedPaths(const Script &s_, const frx::PlanArrays &out_, const frx::PlanCounters &c_, frx::PlanTimes *times_) : s(s_), out(out_), c(c_), times(times_) {}

    void note(int kind, const std::vector<char> *only, const frx::TakeOver *take) {
        log.push_back(kind); log.push_back(take != nullptr); log.push_back(take ? take->capacity : 0); log.push_back(take ? (int)take->not_before : 0);
        for (int b = 0; b < s.B; b++) { log.push_back(only ? (*only)[b] : -1); found.push_back(out.x[s.xoff[b]]); }
    }
    // a result that names the call and the candidate it belongs to
    void write(int b) {
        for (int i = s.xoff[b]; i < s.xoff[b + 1]; i++) out.x[i] = 1000.0 * (k + 1) + b + 0.001 * (i - s.xoff[b]);
        out.status[b] = s.status[(size_t)k * s.B + b];
        if (out.iters) out.iters[b] = 100 * (k + 1) + b;
        if (out.evals) out.evals[b] = 200 * (k + 1) + b;
        if (out.objective) out.objective[b] = 0.5 + 10.0 * (k + 1) + b;
    }
    void ran() { const double *t = s.times + 4 * (size_t)k; *times = {t[0], t[1], t[2], t[3]}; }

    int resident(frx::TakeOver *take) {
        note(0, nullptr, take);
        if (k >= s.n_calls) return -99;                                  // the script has no such call
        c.resident_used = 0; c.resident_failed = 0; dev_status = s.dev[k];
        const int rc = s.rc[k];
        if (rc < 0) { k++; return rc; }
        if (rc != 0) {                                                   // given up: a plan from its start has cleared the verdicts and may have moved x
            if (!take) for (int b = 0; b < s.B; b++) { out.status[b] = 0; for (int i = s.xoff[b]; i < s.xoff[b + 1]; i++) out.x[i] = -1.0; }
            k++;
            return 1;
        }
        int n = 0;
        for (int q = 0; q < (take ? (int)take->cand.size() : s.B); q++) {
            const int b = take ? take->cand[q] : q;
            write(b); n++;
            if (out.status[b] < 0 && out.status[b] != frx::LBERR_MAXIMUMITERATION) c.resident_failed++;
        }
        ran();
        c.resident_used = 7 + k; c.resident_clusters = n;
        for (int q = 0; q < 4; q++) c.spec_counts[q] = 10ull * (k + 1) + q;
        k++;
        return 0;
    }
    int per_stage(const std::vector<char> *only, frx::TakeOver *take) {
        note(1, only, take);
        if (k >= s.n_calls) return -99;
        const int rc = s.rc[k];
        if (rc < 0 || rc == 1) { k++; return rc; }                       // (1: nothing has been touched)
        bool handed = false;
        for (int b = 0; b < s.B && rc == 2 && take; b++) handed = handed || ((!only || (*only)[b]) && s.hand[(size_t)k * s.B + b]);
        ran();
        for (int b = 0; b < s.B; b++) {
            if (only && !(*only)[b]) continue;
            if (handed && s.hand[(size_t)k * s.B + b]) { take->cand.push_back(b); take->sv.emplace_back(); take->newest.push_back(0); take->bound.push_back(0); take->f_last.push_back(0.0); continue; }
            write(b);
        }
        if (handed) take->spent = *times;
        k++;
        return handed ? 2 : 0;
    }
    unsigned device_status() const { return dev_status; }
    int capacity() { cap_asked++; return s.cap; }
    int fail(int code, const char *text) { err_code = code; err = text; return code; }
};

// sw7: FRX_LBFGS=host, FRX_RESIDENT=0, FRX_RESIDENT_RETRY's first character (-1 unset), FRX_TAKEOVER=0, FRX_RESIDENT_QUEUE=0, then two spare
inline frx::PlanSwitches switches(const int *sw7) {
    frx::PlanSwitches sw;
    sw.lbfgs_host = sw7[0] != 0; sw.resident_off = sw7[1] != 0; sw.resident_retry = sw7[2]; sw.takeover_off = sw7[3] != 0; sw.resident_queue_off = sw7[4] != 0;
    return sw;
}

} // namespace plan_route_check

#ifdef HOSTCHECK_LIBRARY
// handle7: lbfgs_mode, resident_mode, resident_retry, takeover_at, solver, knot_threads, mem_size.  counters10 (in: what an earlier plan left; out): resident_used,
// resident_retried, resident_failed, resident_clusters, taken_over, spec_counts[4], device status.  log: rows of 4 + B ints (plan_route_check::LOG_HEAD), at most
// log_cap of them, `found` [log_cap][B] beside them; made3: calls made, times capacity() was asked, the code handed to fail().  Returns what plan_route returns.
extern "C" int hostcheck_plan_route(const int *sw7, const int *handle7, int B, const int *xoff, int cap, int n_calls, const int *rc, const unsigned *dev, const int *status,
                                    const unsigned char *hand, const double *times, double *x, int *st, int *iters, int *evals, double *objective, long long *counters10,
                                    double *stats4, int *log, double *found, int log_cap, int *made3, char *err_text, int err_cap) {
    using namespace plan_route_check;
    const Script s{B, xoff, n_calls, rc, dev, status, hand, times, cap};
    int ci[5]; unsigned long long spec[4];
    for (int q = 0; q < 5; q++) ci[q] = (int)counters10[q];
    for (int q = 0; q < 4; q++) spec[q] = (unsigned long long)counters10[5 + q];
    frx::PlanTimes tm{stats4[0], stats4[1], stats4[2], stats4[3]};
    const frx::PlanArrays out{x, st, iters, evals, objective};
    ScriptedPaths paths(s, out, {ci[0], ci[1], ci[2], ci[3], ci[4], spec}, &tm);
    paths.dev_status = (unsigned)counters10[9];
    const int ret = frx::plan_route({switches(sw7), handle7[0], handle7[1], handle7[2], handle7[3], handle7[4], handle7[5], handle7[6], B, xoff[B], xoff}, out,
                                    {ci[0], ci[1], ci[2], ci[3], ci[4], spec}, tm, paths);
    for (int q = 0; q < 5; q++) counters10[q] = ci[q];
    for (int q = 0; q < 4; q++) counters10[5 + q] = (long long)spec[q];
    counters10[9] = paths.dev_status;
    stats4[0] = tm.ms; stats4[1] = tm.ms_dev; stats4[2] = tm.ms_host; stats4[3] = tm.rounds;
    const int rows = (int)paths.log.size() / (LOG_HEAD + B);
    std::memcpy(log, paths.log.data(), sizeof(int) * (size_t)std::min(rows, log_cap) * (LOG_HEAD + B));
    std::memcpy(found, paths.found.data(), sizeof(double) * (size_t)std::min(rows, log_cap) * B);
    made3[0] = rows; made3[1] = paths.cap_asked; made3[2] = paths.err_code;
    if (err_cap > 0) { std::strncpy(err_text, paths.err.c_str(), (size_t)err_cap - 1); err_text[err_cap - 1] = 0; }
    return ret;
}
extern "C" int hostcheck_retry_mode(int first_char, int handle_retry) { return frx::retry_mode(first_char, handle_retry); }
extern "C" int hostcheck_wants_retry(int status, int mode) { return frx::wants_retry(status, mode); }
extern "C" int hostcheck_resident_first(const int *sw7, int resident_mode, long takeover_at) { return frx::resident_first(plan_route_check::switches(sw7), resident_mode, takeover_at); }
extern "C" int hostcheck_wants_device_vectors(const int *sw7, int lbfgs_mode) { return frx::wants_device_vectors(plan_route_check::switches(sw7), lbfgs_mode); }
extern "C" int hostcheck_skip_inactive(int sw_skip, int B) { return frx::skip_inactive(sw_skip, B); }
// out3: capacity, not_before, whether the capacity was asked for
extern "C" void hostcheck_takeover_rule(const int *sw7, int resident_mode, int gave_up, int solver, int knot_threads, int mem_size, int min_n, int cap, int B, long takeover_at, long *out3) {
    int asked = 0;
    const frx::TakeOverRule r = frx::takeover_rule(plan_route_check::switches(sw7), resident_mode, gave_up != 0, solver, knot_threads, mem_size, min_n, B, takeover_at, [&] { asked++; return cap; });
    out3[0] = r.capacity; out3[1] = r.not_before; out3[2] = asked;
}
// geom: FRX_DV_GEOM as set, null: unset.  out4: E, W, PF, BLK
extern "C" void hostcheck_dv_pre_geometry(int maxXb, const char *geom, int *out4) {
    frx::PlanSwitches sw;
    if (geom) { sw.dv_geom_set = true; sw.dv_geom = geom; }
    const frx::DvPreGeometry g = frx::dv_pre_geometry(maxXb, sw);
    out4[0] = g.E; out4[1] = g.W; out4[2] = g.PF; out4[3] = g.BLK;
}
#else

#include <map>
#include <random>

namespace parent {
// ---- what the copied ladder finds where frx_optimize found the handle, the environment and the two drivers ----
using plan_route_check::ScriptedPaths;
struct frx_lbfgs_params_t { int mem_size; };
struct Problem {
    int B, NX; std::vector<int> xoff;
    int lbfgs_mode, resident_mode, resident_retry; long takeover_at;
    struct { int solver, knot_threads, maxXb; } geo;
    int device = 0, taken_over = 0, resident_used = 0, resident_retried = 0, resident_failed = 0, resident_clusters = 0;
    unsigned resident_status = 0;
    unsigned long long spec_counts[4] = {0, 0, 0, 0};
    double stats[4] = {0, 0, 0, 0};
    ScriptedPaths *paths = nullptr;
};
struct TakeOver {
    int capacity = 0; long not_before = 1;
    std::vector<int> cand;
    double ms = 0.0, ms_dev = 0.0, ms_host = 0.0; long rounds = 0;
};
static std::map<std::string, std::string> g_env;
static const char *fake_getenv(const char *name) { auto it = g_env.find(name); return it == g_env.end() ? nullptr : it->second.c_str(); }
namespace frx_ {
using ::frx::LBERR_MAXIMUMITERATION; using ::frx::LBERR_INCREASEGRADIENT; using ::frx::SOLVER_KNOT_PCR;
static bool env_is(const char *name, char ch) { const char *e = fake_getenv(name); return e && e[0] == ch; }
static bool env_off(const char *name) { return env_is(name, '0'); }
static int g_cap = 0;
static int resident_capacity(int, int) { return g_cap; }
}
struct hipDeviceProp_t { int multiProcessorCount = 0; };
constexpr int hipSuccess = 0;
static int hipGetDeviceProperties(hipDeviceProp_t *, int) { return frx_::g_cap >= 0 ? hipSuccess : 1; }
// the drivers: the scripted ones, on the handle's stats
template <class F> static int on_stats(Problem *p, F &&call) {
    frx::PlanTimes t{p->stats[0], p->stats[1], p->stats[2], p->stats[3]};
    p->paths->times = &t;
    const int rc = call();
    p->stats[0] = t.ms; p->stats[1] = t.ms_dev; p->stats[2] = t.ms_host; p->stats[3] = t.rounds;
    p->resident_status = p->paths->dev_status;
    return rc;
}
template <class F> static int with_take(TakeOver *take, F &&call) {
    if (!take) return call(nullptr);
    frx::TakeOver t;
    t.capacity = take->capacity; t.not_before = take->not_before; t.cand = take->cand;
    t.sv.resize(t.cand.size()); t.newest.resize(t.cand.size()); t.bound.resize(t.cand.size()); t.f_last.resize(t.cand.size());
    const int rc = call(&t);
    take->cand = t.cand; take->ms = t.spent.ms; take->ms_dev = t.spent.ms_dev; take->ms_host = t.spent.ms_host; take->rounds = (long)t.spent.rounds;
    return rc;
}
static int optimize_resident(Problem *p, const frx_lbfgs_params_t &, double *, int *, int *, int *, double *, TakeOver *take = nullptr) {
    return on_stats(p, [&] { return with_take(take, [&](frx::TakeOver *t) { return p->paths->resident(t); }); });
}
static int optimize_device_vectors(Problem *p, const frx_lbfgs_params_t &, double *, int *, int *, int *, double *, const std::vector<char> *only = nullptr, TakeOver *take = nullptr) {
    return on_stats(p, [&] { return with_take(take, [&](frx::TakeOver *t) { return p->paths->per_stage(only, t); }); });
}
static int fail(Problem *p, int code, const char *text) { return p->paths->fail(code, text); }

// ---- frx_optimize from its want_device_vectors line to the line that chose between finish_optimize (0) and the host-vector plan (1), as it stood ----
#define frx frx_
static int ladder(Problem *p, const frx_lbfgs_params_t *params, double *x, double *objective, int *status, int *iters, int *evals) {
    const bool want_device_vectors = !frx::env_is("FRX_LBFGS", 'h') && p->lbfgs_mode != 1;
    int rc_dv = 1;
    p->taken_over = 0;
    if (want_device_vectors) {
        const bool resident_off = frx::env_off("FRX_RESIDENT");
        p->resident_used = 0; p->resident_retried = 0;
        p->resident_failed = 0; p->resident_clusters = 0; for (auto &q : p->spec_counts) q = 0;
        const std::vector<double> x_start(x, x + p->NX);
        const char *rt_env = fake_getenv("FRX_RESIDENT_RETRY");
        const int retry_mode = rt_env ? (rt_env[0] == '0' ? 0 : rt_env[0] == 't' ? 2 : 1) : (p->resident_retry != 0 ? 1 : 2);   // 2 = targeted (default)
        auto wants_retry = [&](int st) { return st < 0 && st != frx::LBERR_MAXIMUMITERATION && (retry_mode == 1 || (retry_mode == 2 && st == frx::LBERR_INCREASEGRADIENT)); };
        auto retry_increase_gradient = [&](const std::vector<int> *scope) -> int {
            std::vector<char> again(p->B, 0);
            int n_again = 0;
            if (scope) { for (int b : *scope) if (wants_retry(status[b])) { again[b] = 1; n_again++; } }
            else for (int b = 0; b < p->B; b++) if (wants_retry(status[b])) { again[b] = 1; n_again++; }
            if (n_again == 0) return 0;
            const std::vector<double> x_res(x, x + p->NX);
            std::vector<int> st_res(status, status + p->B), it_res, ev_res;
            std::vector<double> obj_res;
            if (iters) it_res.assign(iters, iters + p->B);
            if (evals) ev_res.assign(evals, evals + p->B);
            if (objective) obj_res.assign(objective, objective + p->B);
            for (int b = 0; b < p->B; b++) if (again[b]) std::copy(x_start.begin() + p->xoff[b], x_start.begin() + p->xoff[b + 1], x + p->xoff[b]);
            const int used = p->resident_used, taken = p->taken_over;
            const double t_res[4] = {p->stats[0], p->stats[1], p->stats[2], p->stats[3]};
            const int rc2 = optimize_device_vectors(p, *params, x, status, iters, evals, objective, &again);
            if (rc2 < 0) return rc2;
            if (rc2 != 0) {
                std::copy(x_res.begin(), x_res.end(), x);
                std::copy(st_res.begin(), st_res.end(), status);
                if (iters) std::copy(it_res.begin(), it_res.end(), iters);
                if (evals) std::copy(ev_res.begin(), ev_res.end(), evals);
                if (objective) std::copy(obj_res.begin(), obj_res.end(), objective);
                n_again = 0;
            }
            p->resident_used = used; p->taken_over = taken; p->resident_retried += n_again;
            if (rc2 == 0) p->stats[0] += t_res[0]; else p->stats[0] = t_res[0];
            if (scope) { for (int q = 1; q < 4; q++) p->stats[q] = (rc2 == 0 ? p->stats[q] : 0.0) + t_res[q]; }
            return 0;
        };
        bool resident_gave_up = false;
        if (!resident_off && p->resident_mode != 0 && p->takeover_at <= 0) {
            rc_dv = optimize_resident(p, *params, x, status, iters, evals, objective);
            resident_gave_up = rc_dv != 0 && p->resident_status != 0;
            if (rc_dv < 0) return rc_dv;
            if (rc_dv != 0) std::copy(x_start.begin(), x_start.end(), x);
            else {
                const int rc_retry = retry_increase_gradient(nullptr);
                if (rc_retry < 0) return rc_retry;
            }
        }
        if (rc_dv != 0) {
            TakeOver take;
            {
                const bool wanted = !frx::env_off("FRX_TAKEOVER") && !resident_off && !frx::env_off("FRX_RESIDENT_QUEUE") && p->resident_mode != 0 && !resident_gave_up;
                hipDeviceProp_t prop;
                if (wanted && p->geo.solver == frx::SOLVER_KNOT_PCR && p->geo.knot_threads == 64 && params->mem_size == 128 && hipGetDeviceProperties(&prop, p->device) == hipSuccess) {
                    bool fits = true;
                    for (int b = 0; b < p->B; b++) fits = fits && p->xoff[b + 1] - p->xoff[b] >= 2 * params->mem_size;
                    const int cap = frx::resident_capacity(p->geo.maxXb, prop.multiProcessorCount);   // what optimize_resident will hold when they are handed over
                    if (fits && cap >= 1 && p->B > cap) take.capacity = cap;
                    if (p->takeover_at > 0) { take.not_before = p->takeover_at; if (fits && cap >= 1 && p->B <= cap) take.capacity = cap; }   // (tests: a small batch hands over after so many rounds)
                }
            }
            rc_dv = optimize_device_vectors(p, *params, x, status, iters, evals, objective, nullptr, take.capacity > 0 ? &take : nullptr);
            if (rc_dv < 0) return rc_dv;
            if (rc_dv == 2) {
                const double ms_ps = take.ms, dev_ps = take.ms_dev, host_ps = take.ms_host;
                const long rounds_ps = take.rounds;
                const int rc3 = optimize_resident(p, *params, x, status, iters, evals, objective, &take);
                if (rc3 < 0) return rc3;
                if (rc3 == 0) {
                    p->taken_over = (int)take.cand.size();
                    p->stats[0] += ms_ps; p->stats[1] += dev_ps; p->stats[2] += host_ps; p->stats[3] += (double)rounds_ps;
                    const int rc_retry = retry_increase_gradient(&take.cand);
                    if (rc_retry < 0) return rc_retry;
                } else {
                    std::vector<char> again(p->B, 0);
                    for (int c : take.cand) { again[c] = 1; std::copy(x_start.begin() + p->xoff[c], x_start.begin() + p->xoff[c + 1], x + p->xoff[c]); }
                    const int rc4 = optimize_device_vectors(p, *params, x, status, iters, evals, objective, &again);
                    if (rc4 != 0) return rc4 < 0 ? rc4 : fail(p, FRX_ERR_HIP, "per-stage path unavailable after a failed take-over");
                    p->resident_used = 0;
                    p->stats[0] += ms_ps; p->stats[1] += dev_ps; p->stats[2] += host_ps; p->stats[3] += (double)rounds_ps;
                }
                rc_dv = 0;
            }
        }
    }
    if (rc_dv == 0) return 0;
    return 1;
}
#undef frx
} // namespace parent

// everything a plan leaves behind, to compare the two
struct Left {
    int ret = 0;
    std::vector<double> x, objective; std::vector<int> status, iters, evals, log; std::vector<double> found;
    long long counters[10] = {0}; double stats[4] = {0}; int k = 0, err_code = 0; std::string err;
    bool operator==(const Left &o) const {
        return ret == o.ret && x == o.x && objective == o.objective && status == o.status && iters == o.iters && evals == o.evals && log == o.log && found == o.found &&
               std::memcmp(counters, o.counters, sizeof(counters)) == 0 && std::memcmp(stats, o.stats, sizeof(stats)) == 0 && k == o.k && err_code == o.err_code && err == o.err;
    }
};

int main() {
    using namespace plan_route_check;
    std::mt19937 rng(20261020);
    auto pick = [&](std::initializer_list<int> v) { return *(v.begin() + rng() % v.size()); };
    const int codes[7] = {0, 0, 3, frx::LBERR_INCREASEGRADIENT, frx::LBERR_MINIMUMSTEP, frx::LBERR_MAXIMUMITERATION, frx::LBERR_ROUNDING};
    int bad = 0, n = 0, seen[4] = {0, 0, 0, 0}, retried = 0, handed = 0, refused = 0;
    for (int trial = 0; trial < 20000; trial++) {
        const int B = pick({1, 2, 3, 5, 9}), n_calls = 5;
        std::vector<int> xoff(B + 1, 0);
        for (int b = 0; b < B; b++) xoff[b + 1] = xoff[b] + pick({255, 256, 256, 257, 300, 300, 641, 641});
        const int NX = xoff[B];
        std::vector<int> rc(n_calls), status((size_t)n_calls * B);
        std::vector<unsigned> dev(n_calls);
        std::vector<unsigned char> hand((size_t)n_calls * B);
        std::vector<double> times(4 * (size_t)n_calls);
        for (int k = 0; k < n_calls; k++) {
            rc[k] = pick({0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2, -6});
            dev[k] = (unsigned)pick({0, 0, 5});
            for (int b = 0; b < B; b++) { status[(size_t)k * B + b] = codes[rng() % 7]; hand[(size_t)k * B + b] = rng() % 2; }
            for (int q = 0; q < 4; q++) times[4 * k + q] = std::ldexp(1.0, 4 * k + q);
        }
        // mostly the settings under which every stretch of the route is open; each switch and each refusal of the take-over rule now and then
        const int sw7[7] = {pick({0, 0, 0, 0, 0, 0, 0, 1}), pick({0, 0, 0, 0, 0, 1}), pick({-1, -1, '0', '1', 't', 'x'}), pick({0, 0, 0, 0, 0, 0, 0, 1}), pick({0, 0, 0, 0, 0, 0, 0, 1}), 0, 0};
        const int handle7[7] = {pick({0, 0, 0, 0, 0, 0, 0, 1}), pick({0, 1, 1, 1, 1, 2}), pick({0, 1}), pick({0, 0, 3}), pick({0, 0, 0, 0, 0, 0, 0, 1}), pick({64, 64, 64, 64, 64, 64, 64, 128}),
                                pick({128, 128, 128, 128, 128, 128, 128, 127})};
        const int cap = pick({-1, 0, 1, 2, 2, 8, 8, 32});
        const bool optional = rng() % 4 != 0;
        const Script s{B, xoff.data(), n_calls, rc.data(), dev.data(), status.data(), hand.data(), times.data(), cap};
        Left got[2];
        for (int side = 0; side < 2; side++) {                               // 0: the route; 1: the ladder, the scripted drivers on its handle's fields
            Left &L = got[side];
            L.x.resize(NX); L.status.assign(B, 77); L.iters.assign(B, 78); L.evals.assign(B, 79); L.objective.assign(B, 80.0);
            for (int i = 0; i < NX; i++) L.x[i] = 0.25 * i;
            parent::Problem p;                                               // (what an earlier plan left: in the counters, the stats and the device status)
            p.B = B; p.NX = NX; p.xoff = xoff; p.lbfgs_mode = handle7[0]; p.resident_mode = handle7[1]; p.resident_retry = handle7[2]; p.takeover_at = handle7[3];
            p.geo = {handle7[4], handle7[5], 641};
            p.resident_used = 91; p.resident_retried = 92; p.resident_failed = 93; p.resident_clusters = 94; p.taken_over = 95;
            for (int q = 0; q < 4; q++) p.spec_counts[q] = 96 + q;
            frx::PlanTimes tm{-1.0, -2.0, -3.0, -4.0};
            const frx::PlanArrays out{L.x.data(), L.status.data(), optional ? L.iters.data() : nullptr, optional ? L.evals.data() : nullptr, optional ? L.objective.data() : nullptr};
            const frx::PlanCounters counters{p.resident_used, p.resident_retried, p.resident_failed, p.resident_clusters, p.taken_over, p.spec_counts};
            ScriptedPaths paths(s, out, counters, &tm);
            paths.dev_status = 9;
            if (side == 0) {
                L.ret = frx::plan_route({switches(sw7), handle7[0], handle7[1], handle7[2], handle7[3], handle7[4], handle7[5], handle7[6], B, NX, xoff.data()}, out, counters, tm, paths);
            } else {
                parent::g_env.clear();
                if (sw7[0]) parent::g_env["FRX_LBFGS"] = "host";
                if (sw7[1]) parent::g_env["FRX_RESIDENT"] = "0";
                if (sw7[2] >= 0) parent::g_env["FRX_RESIDENT_RETRY"] = std::string(1, (char)sw7[2]);
                if (sw7[3]) parent::g_env["FRX_TAKEOVER"] = "0";
                if (sw7[4]) parent::g_env["FRX_RESIDENT_QUEUE"] = "0";
                parent::frx_::g_cap = cap;
                p.stats[0] = tm.ms; p.stats[1] = tm.ms_dev; p.stats[2] = tm.ms_host; p.stats[3] = tm.rounds;
                p.resident_status = 9; p.paths = &paths;
                const parent::frx_lbfgs_params_t pm{handle7[6]};
                L.ret = parent::ladder(&p, &pm, out.x, out.objective, out.status, out.iters, out.evals);
                tm = {p.stats[0], p.stats[1], p.stats[2], p.stats[3]};
            }
            const long long left[10] = {p.resident_used, p.resident_retried, p.resident_failed, p.resident_clusters, p.taken_over, (long long)p.spec_counts[0], (long long)p.spec_counts[1],
                                        (long long)p.spec_counts[2], (long long)p.spec_counts[3], paths.dev_status};
            std::memcpy(L.counters, left, sizeof(left));
            L.stats[0] = tm.ms; L.stats[1] = tm.ms_dev; L.stats[2] = tm.ms_host; L.stats[3] = tm.rounds;
            L.log = paths.log; L.found = paths.found; L.k = paths.k; L.err_code = paths.err_code; L.err = paths.err;
        }
        const bool device_vectors = !sw7[0] && handle7[0] != 1;
        n++;
        if (!(got[0] == got[1])) { if (!bad) std::printf("trial %d: the route and the ladder disagree (returns %d, %d; calls %d, %d)\n", trial, got[0].ret, got[1].ret, got[0].k, got[1].k); bad++; }
        seen[got[0].ret < 0 ? 2 : got[0].ret] ++;
        retried += device_vectors && got[0].counters[1] > 0; handed += device_vectors && got[0].counters[4] > 0; refused += got[0].err_code != 0;
    }
    std::printf("%d random scripts: %d disagreements; %d plans stood, %d fell back to host vectors, %d ended with an error; %d retried, %d handed over, %d refused twice\n",
                n, bad, seen[0], seen[1], seen[2], retried, handed, refused);
    return bad || !seen[0] || !seen[1] || !seen[2] || !retried || !handed || !refused ? 1 : 0;
}
#endif
