// What the distance field of a voxel map (frx_map_esdf*, include/frx.h) decides before anything runs: whether a grid is accepted, how much scratch the device
// form needs, and the launch geometry of each pass.  Pure functions of the three dimensions: plain C++, no HIP, no environment - shared by the entries
// (frx_batch.cpp), the launcher (frx_device_esdf.hip), the host referee's argument check (frx_search.cpp), a stand-alone host program
// (tests/hostcheck/esdf_main.cpp); the CPU tests read its verdict and bytes through frx_map_esdf_workspace.
#pragma once
#include <cstddef>

namespace frx {

enum { ESDF_MAX_DIM = 16384,             // cells along y or z: 3 dim^2 stays inside 31 bits, so a squared distance is an int and INT_MAX is free for "no site"
       ESDF_MAX_LINE = 8192,             // cells along x: the x pass keeps a whole line of both site sets in LDS, 8 bytes a cell, inside the 64 KiB a launch gets unasked
       ESDF_THREADS = 256,               // workgroup of every pass
       ESDF_INF = 0x7fffffff };          // squared distance of a cell whose line (so far) holds no site

enum EsdfVerdict { ESDF_FITS = 0, ESDF_INVALID = 1, ESDF_CAPACITY = 2 };

struct EsdfPlan {
    EsdfVerdict verdict;
    long long cells, columns;            // nx ny nz, nx ny
    size_t work_bytes;                   // four int arrays of `cells` (dz^2 and dz^2 + dy^2 towards occupied and towards free cells), nx + 1 flag words, then two int
                                         // arrays of `columns` (per (x, y) column the distance along y to the nearest column with an occupied / a free cell)
    size_t flag_off, ydist_off;          // where the flag words and the column distances begin, in ints
    unsigned grid_flags, grid_z, grid_ycol, grid_y, grid_x;   // workgroups of ESDF_THREADS lanes: flag words / columns / x rows / cells, each in a flat range; one per x line
    unsigned lds_x;                      // dynamic LDS of the x pass, bytes
};

// dim[i] <= 0: invalid.  A y or z above ESDF_MAX_DIM, an x above ESDF_MAX_LINE or more than 2^31 - 1 cells: capacity.
inline EsdfPlan esdf_plan(const int *dim) {
    EsdfPlan p{};
    if (!dim || dim[0] <= 0 || dim[1] <= 0 || dim[2] <= 0) { p.verdict = ESDF_INVALID; return p; }
    p.verdict = ESDF_CAPACITY;
    if (dim[0] > ESDF_MAX_LINE || dim[1] > ESDF_MAX_DIM || dim[2] > ESDF_MAX_DIM) return p;
    p.columns = (long long)dim[0] * dim[1];
    p.cells = p.columns * dim[2];
    if (p.cells > 0x7fffffffLL) return p;
    p.verdict = ESDF_FITS;
    p.flag_off = 4 * (size_t)p.cells;
    p.ydist_off = p.flag_off + (size_t)dim[0] + 1;
    p.work_bytes = sizeof(int) * (p.ydist_off + 2 * (size_t)p.columns);
    p.grid_flags = (unsigned)((dim[0] + 1 + ESDF_THREADS - 1) / ESDF_THREADS);
    p.grid_z = (unsigned)((p.columns + ESDF_THREADS - 1) / ESDF_THREADS);
    p.grid_ycol = (unsigned)((dim[0] + ESDF_THREADS - 1) / ESDF_THREADS);
    p.grid_y = (unsigned)((p.cells + ESDF_THREADS - 1) / ESDF_THREADS);
    p.grid_x = (unsigned)((long long)dim[1] * dim[2]);
    p.lds_x = (unsigned)(2 * sizeof(int) * (size_t)dim[0]);
    return p;
}

} // namespace frx
