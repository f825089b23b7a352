// hipcc translation unit of the corridor kernels: cells of a batch of segments (k_dilate, frx_corridor_kernels.hpp), whole corridors of a batch of paths
// (k_corridor_chain, frx_chain_kernel.hpp; both run the same dilate_cell) and their launchers.
#include <hip/hip_runtime.h>

#include "frx_chain_kernel.hpp"
#include "frx_device.hpp"

namespace frx {

size_t dilate_lds_bytes(int pcap) { return sizeof(double) * ((size_t)3 * pcap + 32 + 36 + 16) + sizeof(int) * ((size_t)2 * pcap + 257 + 3); }
int launch_dilate(const DilateLaunch &d, void *stream) {
    DilateArgs a;
    a.p1 = d.p1; a.p2 = d.p2; a.obs = d.obs; a.bbox[0] = d.bbox[0]; a.bbox[1] = d.bbox[1]; a.bbox[2] = d.bbox[2]; a.offset = d.offset;
    a.S = d.S; a.n_obs = d.n_obs; a.cap_planes = d.cap_planes; a.pcap = d.pcap;
    a.n_planes = d.n_planes; a.h_rec = d.h_rec; a.ell_C = d.ell_C; a.ell_d = d.ell_d;
    const size_t lds = dilate_lds_bytes(d.pcap);
    if (const int e = raise_lds_limit((const void *)k_dilate, lds)) return e;
    hipLaunchKernelGGL(k_dilate, dim3(d.S), dim3(256), lds, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

size_t chain_lds_bytes(int pcap, int cap_planes) {
    return sizeof(double) * ((size_t)3 * pcap + 32 + 36 + 16 + ((size_t)2 * pcap + 257 + 3 + 1) / 2 + (size_t)6 * cap_planes) + sizeof(int) * 4;
}

static DevVoxelMap to_map(const ChainLaunch &c) {
    DevVoxelMap m;
    for (int i = 0; i < 3; i++) { m.origin[i] = c.map_origin[i]; m.dim[i] = c.map_dim[i]; }
    m.res = c.map_res; m.cells = c.map_cells;
    return m;
}

int launch_chain(const ChainLaunch &c, void *stream) {
    if (c.n_paths < 1 || c.n_obs < 0 || c.cap_polys < 1 || c.cap_planes < 8 || c.cap_planes > CHAIN_MAX_PLANES || c.pcap < 1) return (int)hipErrorInvalidValue;
    const size_t lds = chain_lds_bytes(c.pcap, c.cap_planes);
    if (lds > (size_t)160 * 1024) return (int)hipErrorInvalidValue;
    ChainArgs a;
    a.path_off = c.path_off; a.path = c.path; a.obs = c.obs; a.map = to_map(c);
    for (int i = 0; i < 3; i++) a.bbox[i] = c.bbox[i];
    a.map_height = c.map_height; a.max_seg = c.max_seg;
    a.n_paths = c.n_paths; a.n_obs = c.n_obs; a.cap_polys = c.cap_polys; a.cap_planes = c.cap_planes; a.pcap = c.pcap;
    a.h_slot = c.h_slot; a.cell_planes = c.cell_planes; a.n_polys = c.n_polys; a.status = c.status;
    // The function's limit is raised to the whole LDS, never to one launch's need: launches of different cap_planes may be in flight side by side.  Later calls -
    // a capture among them - are the launch alone.
    if (const int e = raise_lds_limit((const void *)k_corridor_chain, (size_t)160 * 1024)) return e;
    hipLaunchKernelGGL(k_corridor_chain, dim3(c.n_paths), dim3(256), lds, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_map_blocked_pairs(const ChainLaunch &map_of, int n, const double *a, const double *b, int *out, void *stream) {
    if (n < 1 || !map_of.map_cells) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_map_blocked_pairs, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, to_map(map_of), n, a, b, out);
    return (int)hipGetLastError();
}

} // namespace frx
