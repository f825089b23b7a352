// TEST INFRASTRUCTURE - what the trajectory entries decide on the host (fast-racing_amd/csrc/frx_traj_host.hpp), two ways:
//  - included by hostcheck.cpp (HOSTCHECK_LIBRARY) behind batch_host_main.cpp, whose frx::set_error and error text it shares: the functions behind plain C
//    signatures, for tests/test_traj_host_cpu.py;
//  - a program of its own (make traj_host_san): cloud_split against the two ladders it replaced, the offsets rule and the carve-ups against straightforward
//    restatements, over random inputs and the edges, under the address and undefined-behaviour sanitizers.  Host code only; never loaded into Python with a
//    sanitizer and never run on a GPU machine.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_device.hpp"
#include "../../fast-racing_amd/csrc/frx_traj_host.hpp"

#ifdef HOSTCHECK_LIBRARY
// {CLEAR_PASS, CLEAR_TARGET_WGS, CLEAR_EXACT_CHUNK, CLEAR_EXACT_TARGET_WGS}: what the two call sites of cloud_split pass
extern "C" void hostcheck_cloud_constants(int *out4) { out4[0] = frx::CLEAR_PASS; out4[1] = frx::CLEAR_TARGET_WGS; out4[2] = frx::CLEAR_EXACT_CHUNK; out4[3] = frx::CLEAR_EXACT_TARGET_WGS; }
extern "C" int hostcheck_cloud_split(int P, int n_obs, int force, int unit, int target_wgs, int *out2) { return frx::cloud_split(P, n_obs, force, unit, target_wgs, out2, out2 + 1); }
extern "C" int hostcheck_offsets_args(const char *what, int B, const int *off, int from_zero) { g_batch_error.clear(); return frx::offsets_args(what, B, off, from_zero != 0); }
extern "C" int hostcheck_intervals_arg(int intervals) { g_batch_error.clear(); return frx::intervals_arg(intervals); }
extern "C" int hostcheck_cloud_points_arg(int n_obs) { g_batch_error.clear(); return frx::cloud_points_arg(n_obs); }
extern "C" int hostcheck_sample_time_args(int n_samples, double t0, double dt, int have_times) { g_batch_error.clear(); return frx::sample_time_args(n_samples, t0, dt, have_times != 0); }
extern "C" int hostcheck_sample_rows_arg(int B, int n_samples, unsigned long long *n_out) {
    size_t n = *n_out;
    g_batch_error.clear();
    const int rc = frx::sample_rows_arg(B, n_samples, &n);
    *n_out = n;
    return rc;
}
// kind 0: carve_clear(a = n_rows, b = n_obs, c = n_work); 1: carve_gates(a = n_gates, b = B); 2: carve_sample(a = n_out, b = have_times); 3: carve_mapdist(a = n_rows, dim)
extern "C" void hostcheck_carve(int kind, unsigned long long a, unsigned long long b, unsigned long long c, const int *dim, unsigned long long *out3) {
    const frx::Carve at = kind == 0 ? frx::carve_clear((size_t)a, (int)b, (size_t)c) : kind == 1 ? frx::carve_gates((int)a, (int)b)
                        : kind == 2 ? frx::carve_sample((size_t)a, b != 0) : frx::carve_mapdist((size_t)a, dim);
    out3[0] = at.second; out3[1] = at.third; out3[2] = at.total;
}
#else
namespace { std::string g_error; }
namespace frx { int set_error(int code, const std::string &msg) { g_error = msg; return code; } }

namespace {
using frx::CLEAR_PASS; using frx::CLEAR_TARGET_WGS; using frx::CLEAR_EXACT_CHUNK; using frx::CLEAR_EXACT_TARGET_WGS;
// ---- the ladder being replaced: the two functions as frx_device.hpp carried them ----
inline int clear_geometry(int P, int n_obs, int force, int *chunk, int *nchunks) {
    long long c = force;
    if (force <= 0) {
        const long long want = P < CLEAR_TARGET_WGS ? CLEAR_TARGET_WGS / P : 1;
        c = ((long long)n_obs + want - 1) / want;
        c = (c + CLEAR_PASS - 1) / CLEAR_PASS * CLEAR_PASS;
    }
    const long long nc = ((long long)n_obs + c - 1) / c;
    if ((long long)P * nc > 0x7fffffffLL) return 0;
    *chunk = (int)(c < n_obs ? c : n_obs); *nchunks = (int)nc;
    return 1;
}
inline int clear_exact_geometry(int P, int n_obs, int force, int *chunk, int *nchunks) {
    long long c = force;
    if (force <= 0) {
        const long long want = P < CLEAR_EXACT_TARGET_WGS ? CLEAR_EXACT_TARGET_WGS / P : 1;
        c = ((long long)n_obs + want - 1) / want;
        c = (c + CLEAR_EXACT_CHUNK - 1) / CLEAR_EXACT_CHUNK * CLEAR_EXACT_CHUNK;
    }
    const long long nc = ((long long)n_obs + c - 1) / c;
    if ((long long)P * nc > 0x7fffffffLL) return 0;
    *chunk = (int)(c < n_obs ? c : n_obs); *nchunks = (int)nc;
    return 1;
}

// 0 when cloud_split says what both old functions say (verdict, and chunk and nchunks where accepted; untouched outputs where refused)
int split_disagrees(int P, int n_obs, int force) {
    int bad = 0;
    for (int exact = 0; exact < 2; exact++) {
        int want[2] = {-5, -6}, got[2] = {-5, -6};
        const int ok_want = exact ? clear_exact_geometry(P, n_obs, force, &want[0], &want[1]) : clear_geometry(P, n_obs, force, &want[0], &want[1]);
        const int ok_got = exact ? frx::cloud_split(P, n_obs, force, CLEAR_EXACT_CHUNK, CLEAR_EXACT_TARGET_WGS, &got[0], &got[1])
                                 : frx::cloud_split(P, n_obs, force, CLEAR_PASS, CLEAR_TARGET_WGS, &got[0], &got[1]);
        if (ok_want != ok_got || want[0] != got[0] || want[1] != got[1]) {
            std::printf("cloud_split(%d, %d, %d)%s: %d (%d, %d), the old function %d (%d, %d)\n", P, n_obs, force, exact ? " exact" : "", ok_got, got[0], got[1], ok_want, want[0], want[1]);
            bad++;
        }
    }
    return bad;
}

// the offsets rule, restated: the first refusal in the order first entry, then each step
std::string offsets_restated(const std::string &what, const std::vector<int> &off, bool from_zero) {
    if (from_zero && off[0] != 0) return what + "[0] must be 0";
    if (!from_zero && off[0] < 0) return what + "[0] must be >= 0";
    for (size_t b = 0; b + 1 < off.size(); b++)
        if (off[b + 1] < off[b]) return what + " must not fall (candidate " + std::to_string(b) + ")";
    return "";
}
} // namespace

int main() {
    std::mt19937_64 rng(20250611u);
    auto below = [&](long long n) { return (long long)(rng() % (unsigned long long)n); };
    long long bad = 0, n_split = 0, n_refused = 0;
    // ---- cloud_split: the edges, then random (P, n_obs, force) ----
    const int Ps[] = {1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 100000}, Ns[] = {1, 1023, 1024, 1025, 4097, FRX_CLEAR_MAX_POINTS};
    for (int P : Ps)
        for (int n : Ns) {
            const int forces[] = {0, 1, 7, 1024, n, n + 1, -3};
            for (int f : forces) { bad += split_disagrees(P, n, f); n_split++; }
        }
    for (int P : {127, 128, 129, 0x7fffffff}) { bad += split_disagrees(P, FRX_CLEAR_MAX_POINTS, 1); n_split++; }   // P x nchunks across 2^31 - 1
    for (int it = 0; it < 200000; it++) {
        const int P = 1 + (int)(below(4) ? below(5000) : below(0x7fffffff)), n = 1 + (int)(below(3) ? below(20000) : below(FRX_CLEAR_MAX_POINTS));
        const int f = below(2) ? 0 : below(8) ? 1 + (int)below(n + 1) : -(int)below(5);
        bad += split_disagrees(P, n, f); n_split++;
        int c = 0, nc = 0;
        if (!frx::cloud_split(P, n, f, CLEAR_PASS, CLEAR_TARGET_WGS, &c, &nc)) n_refused++;
        else if (c < 1 || c > n || (long long)c * nc < n || (long long)c * (nc - 1) >= n) { std::printf("cloud_split(%d, %d, %d): %d chunks of %d do not tile the cloud\n", P, n, f, nc, c); bad++; }
    }
    // ---- the offsets rule: random walks, some broken in one place, under every name in use ----
    const char *names[] = {"frx_contain_fold: piece_off", "frx_clearance_exact_fold: piece_off", "frx_map_distance_fold: piece_off", "gate_off"};
    long long n_off = 0, n_off_refused = 0;
    for (int it = 0; it < 20000; it++) {
        const int B = 1 + (int)below(6), k = (int)below(4);
        const bool from_zero = k == 3;
        std::vector<int> off(1, below(3) ? 0 : (int)below(5) - 2);
        for (int b = 0; b < B; b++) off.push_back(off.back() + (below(6) ? (int)below(4) : -1 - (int)below(3)));
        const std::string want = offsets_restated(names[k], off, from_zero);
        g_error.clear();
        const int rc = frx::offsets_args(names[k], B, off.data(), from_zero);
        if (rc != (want.empty() ? FRX_OK : FRX_ERR_INVALID_ARG) || g_error != want) { std::printf("offsets_args: \"%s\" (%d), restated \"%s\"\n", g_error.c_str(), rc, want.c_str()); bad++; }
        n_off++; n_off_refused += !want.empty();
    }
    // ---- the carve-ups: each part begins where the one before it ends ----
    for (int it = 0; it < 20000; it++) {
        const size_t n_rows = (size_t)below(1 << 20), n_work = below(2) ? 0 : (size_t)below(1ll << 34);
        const int n_obs = 1 + (int)below(FRX_CLEAR_MAX_POINTS), n_gates = 1 + (int)below(1 << 20), B = 1 + (int)below(1 << 16);
        const int dim[3] = {1 + (int)below(1290), 1 + (int)below(1290), 1 + (int)below(1290)};
        const size_t n_out = (size_t)FRX_SAMPLE_FIELDS * (size_t)below(1ll << 30);
        frx::Carve at = frx::carve_clear(n_rows, n_obs, n_work);
        if (at.second != n_rows || at.third != n_rows + 3 * (size_t)n_obs || at.total != n_rows + 3 * (size_t)n_obs + n_work) bad++;
        at = frx::carve_gates(n_gates, B);
        const size_t off_doubles = (sizeof(int) * ((size_t)B + 1) + sizeof(double) - 1) / sizeof(double);
        if (at.second != 10 * (size_t)n_gates || at.third != 19 * (size_t)n_gates || at.total != 19 * (size_t)n_gates + off_doubles) bad++;
        at = frx::carve_sample(n_out, false);
        if (at.second != n_out || at.third != n_out || at.total != n_out) bad++;
        at = frx::carve_sample(n_out, true);
        if (at.second != n_out || at.third != n_out + n_out / 20 || at.total != at.third || at.second % 2) bad++;
        at = frx::carve_mapdist(n_rows, dim);
        if (at.second != n_rows || at.third != n_rows + (size_t)dim[0] * (size_t)dim[1] * (size_t)dim[2] || at.total != at.third) bad++;
    }
    std::printf("traj_host_san: %lld splits (%lld refused), %lld offset walks (%lld refused), 20000 carve-ups, %lld disagreements\n", n_split, n_refused, n_off, n_off_refused, bad);
    return bad ? 1 : 0;
}
#endif
