// Where the host side of a plan runs: this plan's share of the host CPUs (the mailbox threads of a resident plan SPIN for its whole length), the CPUs of the
// NUMA node a device hangs on, and the scope that keeps a thread there.  Host-only translation unit (g++).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>

#include <pthread.h>
#include <sched.h>
#include <unistd.h>
#include <sys/syscall.h>

#include "../../include/frx.h"
#include "../../include/frx_debug.h"
#include "frx_handle.hpp"

namespace frx {

static std::atomic<int> g_extra_plans{0};                 // plans of this process that run next to the caller's (frx_multi: shards - 1)
void concurrent_plans_hint(int delta) { g_extra_plans.fetch_add(delta, std::memory_order_relaxed); }
// CPUs the process may use: the affinity mask, cut by the cgroup's CPU quota (v2: cpu.max "quota period"; v1: cpu.cfs_quota_us / cpu.cfs_period_us)
double host_cpu_budget() {
    double cpus = (double)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) == 0 && CPU_COUNT(&allowed) > 0) cpus = std::min(cpus, (double)CPU_COUNT(&allowed));
    auto read2 = [](const char *path, double &a, double &b) -> int {
        FILE *f = std::fopen(path, "r");
        if (!f) return 0;
        char t0[64] = {0}, t1[64] = {0};
        const int n = std::fscanf(f, "%63s %63s", t0, t1);
        std::fclose(f);
        if (n >= 1 && std::strcmp(t0, "max") == 0) return -1;            // no quota
        if (n >= 1) a = std::atof(t0);
        if (n >= 2) b = std::atof(t1);
        return n;
    };
    double q = 0.0, per = 0.0;
    const int n2 = read2("/sys/fs/cgroup/cpu.max", q, per);
    if (n2 == 2 && q > 0.0 && per > 0.0) cpus = std::min(cpus, q / per);
    else if (n2 == 0) {
        double q1 = 0.0, p1 = 0.0, dummy = 0.0;
        if (read2("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", q1, dummy) >= 1 && read2("/sys/fs/cgroup/cpu/cpu.cfs_period_us", p1, dummy) >= 1 && q1 > 0.0 && p1 > 0.0)
            cpus = std::min(cpus, q1 / p1);
    }
    if (const char *e = std::getenv("FRX_HOST_CPUS")) { const double v = std::atof(e); if (v > 0.0) cpus = v; }   // (tests, experiments)
    return std::max(1.0, cpus);
}
//  The budget is divided by the node's ranks only when they SHARE it: a launcher that pins every rank to its own CPU subset (the affinity mask is
// smaller than the online set) has made the division already - dividing again left large batches with one mailbox thread where S / 16 were measured to help.
// FRX_LOCAL_RANKS states the divisor explicitly and is always honoured.
static int share_of(int extra_plans) {
    int ranks = 1;
    if (const char *e = std::getenv("FRX_LOCAL_RANKS")) ranks = std::max(1, std::atoi(e));
    else if (const char *e2 = std::getenv("LOCAL_WORLD_SIZE")) {
        ranks = std::max(1, std::atoi(e2));
        cpu_set_t allowed;
        CPU_ZERO(&allowed);
        const long online = sysconf(_SC_NPROCESSORS_ONLN);
        if (ranks > 1 && sched_getaffinity(0, sizeof(allowed), &allowed) == 0 && online > 0 && (long)CPU_COUNT(&allowed) * ranks <= online) ranks = 1;   // pinned per rank
    }
    const int plans = ranks * (1 + std::max(0, extra_plans));
    return std::max(1, (int)(host_cpu_budget() / plans));
}
int host_cpu_share() { return share_of(g_extra_plans.load(std::memory_order_relaxed)); }
// mailbox service threads of a resident plan with S clusters (the caller included): one per sixteen clusters, at most four, and at most share - 1
static int mailbox_threads_for(int S, int extra_plans) { return std::max(1, std::min(std::max(1, std::min(4, S / 16)), share_of(extra_plans) - 1)); }
int mailbox_threads(int S) { return mailbox_threads_for(S, g_extra_plans.load(std::memory_order_relaxed)); }

static bool device_numa_cpus_uncached(int device, cpu_set_t *out) {
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, sizeof(bdf), device) != hipSuccess) return false;
    for (char *c = bdf; *c; c++) *c = (char)std::tolower(*c);
    int node = -1;
    { const std::string p = std::string("/sys/bus/pci/devices/") + bdf + "/numa_node"; if (FILE *f = std::fopen(p.c_str(), "r")) { if (std::fscanf(f, "%d", &node) != 1) node = -1; std::fclose(f); } }
    if (node < 0) return false;
    std::string list;
    { const std::string p = "/sys/devices/system/node/node" + std::to_string(node) + "/cpulist"; if (FILE *f = std::fopen(p.c_str(), "r")) { char buf[4096] = {0}; if (std::fgets(buf, sizeof(buf), f)) list = buf; std::fclose(f); } }
    if (list.empty()) return false;
    cpu_set_t allowed, want;
    CPU_ZERO(&allowed); CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return false;
    for (size_t i = 0; i < list.size();) {                                   // "0-63,128-191"
        if (!std::isdigit((unsigned char)list[i])) { i++; continue; }
        size_t j = i; int a = 0; while (j < list.size() && std::isdigit((unsigned char)list[j])) a = 10 * a + (list[j++] - '0');
        int b = a;
        if (j < list.size() && list[j] == '-') { j++; b = 0; while (j < list.size() && std::isdigit((unsigned char)list[j])) b = 10 * b + (list[j++] - '0'); }
        for (int c = a; c <= b && c < CPU_SETSIZE; c++) if (CPU_ISSET(c, &allowed)) CPU_SET(c, &want);
        i = j;
    }
    if (CPU_COUNT(&want) < 2) return false;                                 // nothing (or a single CPU) of that node is ours: leave the threads where they are
    *out = want;
    return true;
}
// CPUs of the NUMA node the device hangs on (sysfs: the PCI function's numa_node, the node's cpulist), intersected with what the process may use.
// The mailbox threads of a resident plan are kept there: with the threads on the OTHER socket of a two-socket box every command the device reads
// and every result it writes crosses the socket interconnect and its cache-coherence traffic (measured, 32 candidates: 28.2-28.9 us per round with
// the process on the device's node, 30.6-32.5 on the other one; waits for the host's confirmation: p90 2.3 against 6.9 us - profiles/r04_numa.txt).
//  looked up once per device and process - two sysfs reads and a PCI query are not something to do while a resident kernel's clusters
// already spin; a change of the process's affinity mask after the first plan on a device is not followed
bool device_numa_cpus(int device, cpu_set_t *out) {
    struct Entry { bool ok; cpu_set_t set; };
    static std::mutex lock;
    static std::map<int, Entry> cache;
    std::lock_guard<std::mutex> g(lock);
    auto it = cache.find(device);
    if (it == cache.end()) { Entry e; e.ok = device_numa_cpus_uncached(device, &e.set); it = cache.emplace(device, e).first; }
    if (it->second.ok) *out = it->second.set;
    return it->second.ok;
}

NumaScope::NumaScope(int device) {
    cpu_set_t want;
    if (env_off("FRX_NUMA") || env_off("FRX_NUMA_ALLOC") || !device_numa_cpus(device, &want)) return;   // FRX_NUMA_ALLOC=0: allocations where the caller happens to run (round 5's behaviour, for A/B)
    if (pthread_getaffinity_np(pthread_self(), sizeof(saved), &saved) != 0) return;
    active = pthread_setaffinity_np(pthread_self(), sizeof(want), &want) == 0;
}
NumaScope::~NumaScope() { if (active) (void)pthread_setaffinity_np(pthread_self(), sizeof(saved), &saved); }

} // namespace frx

extern "C" {

int frx_debug_host_cpu_share(int clusters, int extra_plans, double *budget, int *share, int *mailbox_threads) {
    // (computed from the arguments - the process-wide count of concurrent plans is not touched while real plans may be running)
    if (budget) *budget = frx::host_cpu_budget();
    if (share) *share = frx::share_of(extra_plans);
    if (mailbox_threads) *mailbox_threads = frx::mailbox_threads_for(std::max(1, clusters), extra_plans);
    return FRX_OK;
}

// Diagnostic (bench, scripts/r06/mode_probe.py): where the resident plan's mailboxes live.  out4 = {NUMA node of the command mailbox's first page, of the result
// mailbox's first page (move_pages query; -1: no resident plan yet or not available), NUMA node the device hangs on (sysfs; -1: unknown), CPU the caller runs on}.
int frx_debug_mailbox_numa(const frx_problem *p, int *out4) {
    if (!p || !out4) return fail(FRX_ERR_INVALID_ARG, "null argument");
    auto node_of = [](const void *ptr) -> int {
        if (!ptr) return -1;
        void *page = (void *)((uintptr_t)ptr & ~(uintptr_t)4095);
        int status = -1;
        const long rc = syscall(SYS_move_pages, 0, 1UL, &page, (const int *)nullptr, &status, 0);
        return rc == 0 ? status : -1;
    };
    out4[0] = node_of(p->h_rcmd.p); out4[1] = node_of(p->h_rres.p);
    out4[2] = -1;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, sizeof(bdf), p->device) == hipSuccess) {
        for (char *c = bdf; *c; c++) *c = (char)std::tolower(*c);
        const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/numa_node";
        if (FILE *f = std::fopen(path.c_str(), "r")) { int node = -1; if (std::fscanf(f, "%d", &node) == 1) out4[2] = node; std::fclose(f); }
    }
    out4[3] = sched_getcpu();
    return FRX_OK;
}

} // extern "C"
