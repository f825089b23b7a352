// hipcc translation unit of the vertex enumeration: k_enumerate (one workgroup per polytope), k_slots_to_tasks (the corridor generator's slots as tasks) and
// their launchers (frx_enumerate_kernel.hpp).
#include <hip/hip_runtime.h>

#include "frx_enumerate_kernel.hpp"
#include "frx_device.hpp"

namespace frx {

static_assert((int)ENUM_MAX_PLANES == (int)HV_MAX_PLANES && (int)ENUM_MIN_CAP_V == (int)HV_MIN_CAP_V && (int)ENUM_MAX_CAP_V == (int)HV_MAX_CAP_V, "frx_device.hpp and the kernel agree");

// accepted keys and points (48 bytes an entry) and the rank permutation (4): 26 KB at the largest cap_v, beside 20.2 KB of static LDS - under the 64 KB a
// kernel gets without asking, so no function attribute is set and a launch is the launch alone
size_t enumerate_lds_bytes(int cap_v) { return (size_t)52 * cap_v; }

int launch_enumerate(const EnumLaunch &e, void *stream) {
    if (e.n_tasks < 1 || e.cap_v < HV_MIN_CAP_V || e.cap_v > HV_MAX_CAP_V) return (int)hipErrorInvalidValue;
    EnumArgs a;
    a.tasks = e.tasks; a.h_rec = e.h_rec; a.n_tasks = e.n_tasks; a.cap_v = e.cap_v; a.v_slot = e.v_slot; a.nv = e.nv; a.status = e.status;
    hipLaunchKernelGGL(k_enumerate, dim3(e.n_tasks), dim3(256), enumerate_lds_bytes(e.cap_v), (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_slots_to_tasks(int n_paths, int cap_polys, int cap_planes, const int *cell_planes, const int *n_polys, int *tasks, void *stream) {
    if (n_paths < 1 || cap_polys < 1 || cap_planes < 1) return (int)hipErrorInvalidValue;
    const long long n = (long long)n_paths * (2 * (long long)cap_polys - 1);
    if (n > 0x7fffffffLL || (long long)n_paths * cap_polys * cap_planes > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_slots_to_tasks, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_paths, cap_polys, cap_planes, cell_planes, n_polys, tasks);
    return (int)hipGetLastError();
}

} // namespace frx
