// hipcc translation unit: batched sampling of trajectories with their SE(3) outputs (frx_sample_kernel.hpp) and its launcher.
#include <hip/hip_runtime.h>

#include "frx_device.hpp"
#include "frx_sample_kernel.hpp"

namespace frx {

static constexpr int SAMPLE_MAX_PASSES = 4;            // 256-sample passes per workgroup: the prefix sums are paid once per 160 KB of rows
static constexpr int SAMPLE_MIN_WORKGROUPS = 2048;     // fewer passes while the grid would hold fewer workgroups (256 CUs, 3 resident each)
static constexpr size_t SAMPLE_LDS_CAP = 65536;        // the default dynamic-LDS limit of a launch

int sample_fits(int maxN) { return sample_lds_bytes(maxN) <= SAMPLE_LDS_CAP; }

int launch_sample(const DevProblem &dp, int maxN, const double *T, const double *C, int S, double t0, double dt, const double *times, double *out,
                  void *stream) {
    if (S < 1 || !sample_fits(maxN)) return (int)hipErrorInvalidValue;
    const long long tiles = (S + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    int passes = SAMPLE_MAX_PASSES;
    while (passes > 1 && dp.B * ((tiles + passes - 1) / passes) < SAMPLE_MIN_WORKGROUPS) passes >>= 1;
    const long long chunks = (tiles + passes - 1) / passes, blocks = dp.B * chunks;
    if (blocks > (1ll << 24) - 1) return (int)hipErrorInvalidConfiguration;    // (a grid dimension holds at most 2^32 work-items)
    hipLaunchKernelGGL(k_traj_sample, dim3((unsigned)blocks), dim3(SAMPLE_THREADS), sample_lds_bytes(maxN), (hipStream_t)stream, dp.poff, dp.pc.gAcc,
                       T, C, S, t0, dt, times, out, (int)chunks, passes);
    return (int)hipGetLastError();
}

} // namespace frx
