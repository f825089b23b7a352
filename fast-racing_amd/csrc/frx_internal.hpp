// Private glue between the translation units of libfrx.so (not part of the C ABI).
#pragma once
#include <string>

#include "../../include/frx.h"

namespace frx {
// records the text frx_last_error() returns on this thread and hands `code` back (frx_api.cpp)
int set_error(int code, const std::string &msg);
// the one refusal of every entry that finds no device to run on
inline int no_device() { return set_error(FRX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)"); }
// argument rules of the voxel map's distance field (frx_search.cpp; the verdict is esdf_plan's, frx_esdf_plan.hpp): FRX_OK, or the status `who` returns
int esdf_map_args(const struct ::frx_voxel_map *map, const char *who);
// Host CPU budget of a resident plan (frx_host_cpus.cpp): CPUs the process may use (affinity mask and cgroup quota), and this plan's share of them
// when `LOCAL_WORLD_SIZE` ranks of a node and the other shards of a frx_multi job (concurrent_plans_hint: +n before, -n after) spin next to it.
double host_cpu_budget();
int host_cpu_share();
void concurrent_plans_hint(int delta);
}
