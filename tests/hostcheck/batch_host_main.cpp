// TEST INFRASTRUCTURE - what the handle-less batch entries decide on the host (fast-racing_amd/csrc/frx_batch_host.hpp), two ways:
//  - included by hostcheck.cpp (HOSTCHECK_LIBRARY): the functions behind plain C signatures, for tests/test_batch_host_cpu.py;
//  - a program of its own (make batch_host_san): the task list and pack_slots over a few thousand random small inputs against straightforward restatements,
//    under the address and undefined-behaviour sanitizers.  Host code only; never loaded into Python with a sanitizer and never run on a GPU machine.
// The library's frx::set_error lives in frx_api.cpp, beside the handle; here it records the text for hostcheck_batch_last_error.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_batch_host.hpp"

namespace { thread_local std::string g_batch_error; }
namespace frx { int set_error(int code, const std::string &msg) { g_batch_error = msg; return code; } }

#ifdef HOSTCHECK_LIBRARY
extern "C" const char *hostcheck_batch_last_error() { return g_batch_error.c_str(); }
// the argument rules, then the tasks: returns the rules' code, or the number of tasks (4 ints each, copied when they fit cap_tasks)
extern "C" long long hostcheck_enum_tasks(int B, const int *coarse_n, const int *h_off, int *tasks, long long cap_tasks) {
    long long n_poly = 0;
    g_batch_error.clear();
    if (int rc = frx::enum_csr_args("hostcheck", B, coarse_n, h_off, &n_poly)) return rc;
    const std::vector<int> t = frx::enum_tasks(B, coarse_n, h_off);
    if ((long long)(t.size() / 4) <= cap_tasks) std::copy(t.begin(), t.end(), tasks);
    return (long long)(t.size() / 4);
}
extern "C" int hostcheck_pack_slots(int W, int n, const int *count, long long widest, const double *stage, int used, double *rec, int *off) {
    return frx::pack_slots(W, n, count, (size_t)widest, stage, used, rec, off);
}
// 1 = the capacity holds the need of the n counts; *need unclipped, *reported what the entry writes to *n_rec / *n_vert
extern "C" int hostcheck_need_fits(int n, const int *count, int cap, long long *need, int *reported) {
    *need = frx::slots_need(n, count);
    return frx::need_fits(*need, cap, reported);
}
extern "C" int hostcheck_voxel_map_args(const int *dim, double res, const void *cells, int need_cells) {
    frx_voxel_map m = {};
    for (int i = 0; i < 3; i++) m.dim[i] = dim[i];
    m.res = res; m.cells = (const signed char *)cells;
    g_batch_error.clear();
    return frx::voxel_map_args(&m, "hostcheck", need_cells != 0);
}
#else
namespace {
// the task list as the entry's documentation states it, task by task, with none of the library's two passes
std::vector<int> tasks_restated(int B, const std::vector<int> &cn, const std::vector<int> &off) {
    std::vector<int> out;
    int poly = 0;
    auto task = [&](int b0, int k0, int b1, int k1) {
        if (k0 == 0) { k0 = k1; b1 = 0; k1 = 0; }
        out.push_back(b0); out.push_back(k0 == 0 ? -1 : k0); out.push_back(b1); out.push_back(k1);
    };
    for (int b = 0; b < B; b++)
        for (int i = 0; i < cn[b]; i++, poly++) {
            task(off[poly], off[poly + 1] - off[poly], 0, 0);
            if (i + 1 < cn[b]) task(off[poly], off[poly + 1] - off[poly], off[poly + 1], off[poly + 2] - off[poly + 1]);
        }
    return out;
}
} // namespace

int main() {
    std::mt19937 rng(20250117u);
    auto below = [&](int n) { return (int)(rng() % (unsigned)n); };
    long long bad = 0, n_tasks = 0, n_rows = 0;
    for (int it = 0; it < 4000; it++) {
        // ---- the task list: 1..5 candidates of 1..4 cells of 0..5 planes (a third of the cells empty), h_off[0] from 0 to 3 ----
        const int B = 1 + below(5);
        std::vector<int> cn(B), off(1, below(4));
        for (int b = 0; b < B; b++) { cn[b] = 1 + below(4); for (int i = 0; i < cn[b]; i++) off.push_back(off.back() + (below(3) ? 1 + below(5) : 0)); }
        long long n_poly = 0;
        if (frx::enum_csr_args("san", B, cn.data(), off.data(), &n_poly) != FRX_OK || n_poly + 1 != (long long)off.size()) bad++;
        const std::vector<int> got = frx::enum_tasks(B, cn.data(), off.data());
        if (got != tasks_restated(B, cn, off) || (long long)got.size() != 4 * (2 * n_poly - B)) bad++;
        n_tasks += (long long)got.size() / 4;
        // a refusal of each kind on the same batch
        const int at = below(B);
        std::vector<int> cn_bad = cn; cn_bad[at] = -below(2);
        if (frx::enum_csr_args("san", B, cn_bad.data(), off.data(), &n_poly) != FRX_ERR_INVALID_ARG || g_batch_error.find("coarse_n[" + std::to_string(at) + "]") == std::string::npos) bad++;
        std::vector<int> off_bad = off; const int m = below((int)off.size() - 1); off_bad[m + 1] = off_bad[m] - 1;
        if (off_bad[0] >= 0 && (frx::enum_csr_args("san", B, cn.data(), off_bad.data(), &n_poly) != FRX_ERR_INVALID_ARG || g_batch_error.find("polytope " + std::to_string(m)) == std::string::npos)) bad++;
        // ---- pack_slots: two groups behind one another, staged at exactly their widest count, into records of exactly the need ----
        const int W = below(2) ? 3 : 6;
        std::vector<double> rec, want;
        std::vector<int> offs(1, 0), want_off(1, 0);
        std::vector<std::vector<int>> counts(2);
        std::vector<std::vector<double>> stages(2);
        std::vector<size_t> widest(2, 0);
        for (int g = 0; g < 2; g++) {
            const int n = 1 + below(6);
            for (int t = 0; t < n; t++) { counts[g].push_back(below(3) ? below(5) : 0); widest[g] = std::max<size_t>(widest[g], counts[g][t]); }
            stages[g].resize((size_t)W * widest[g] * n);
            for (double &v : stages[g]) v = (double)rng();
            for (int t = 0; t < n; t++) {
                want.insert(want.end(), stages[g].begin() + W * widest[g] * t, stages[g].begin() + W * (widest[g] * t + counts[g][t]));
                want_off.push_back(want_off.back() + counts[g][t]);
            }
        }
        rec.resize(want.size());
        offs.resize(want_off.size());
        int used = 0, poly = 0;
        for (int g = 0; g < 2; g++) {
            used = frx::pack_slots(W, (int)counts[g].size(), counts[g].data(), widest[g], stages[g].data(), used, rec.data(), offs.data() + poly);
            poly += (int)counts[g].size();
        }
        int reported = -1;
        if (rec != want || offs != want_off || used != want_off.back() || !frx::need_fits(frx::slots_need((int)counts[0].size(), counts[0].data()) + frx::slots_need((int)counts[1].size(), counts[1].data()), used, &reported) || reported != used) bad++;
        n_rows += used;
    }
    std::printf("batch_host_san: 4000 random inputs, %lld tasks, %lld packed rows, %lld disagreements\n", n_tasks, n_rows, bad);
    return bad ? 1 : 0;
}
#endif
