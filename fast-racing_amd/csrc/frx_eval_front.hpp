// The front record of the one-launch evaluation (k_eval_cluster<.., FR>, frx_eval_kernel.hpp): what a workgroup needs from the handle's offset tables before it can
// issue its first operand loads, per candidate, in ONE 64-byte line.  Through the tables themselves the kernel's entry is a chain of dependent first touches
// (poff -> coff / xoff / cvoff -> the per-piece tables -> ...); with the record a workgroup reads its candidate's line next to the leading lines of the argument block
// and issues every load of the front behind one wait.  Constant for the life of a handle: written at create from the host copies of the tables, uploaded once.
// Plain C++, no HIP: included by the kernel header and by the host (frx_api.cpp, tests/hostcheck/eval_front_main.cpp).
#pragma once
#include <cstddef>

namespace frx {

struct alignas(64) EvalFront {
    int p0, N;                                // first fine piece (poff[b]) and piece count
    int c0, cN;                               // first coarse piece (coff[b]) and count
    int x0, nx;                               // first variable (xoff[b]) and count
    int nT;                                   // tau of this candidate: x[x0, x0 + nT) - cN with the soft total time, cN - 1 with the fixed one
    int cv0, nvd;                             // first waypoint-vertex record (cvoff[b]) and the DOUBLES of the candidate's records (3 per vertex)
    int wbase;                                // p0 - b: the candidate's first row of the waypoint tables (wp_nv, wp_vbeg, wp_xbeg)
    int ntasks;                               // wave-tasks of the members: ceil(N / ppw)
    int pad[5];
};
static_assert(sizeof(EvalFront) == 64 && alignof(EvalFront) == 64, "one record, one line");

// the B records from the host copies of the offset tables ([B + 1] each); ppw: pieces per wave-task of the handle's geometry
inline void eval_front_fill(int B, const int *poff, const int *coff, const int *xoff, const int *cvoff, bool soft, int ppw, EvalFront *out) {
    for (int b = 0; b < B; b++) {
        EvalFront r = {};
        r.p0 = poff[b]; r.N = poff[b + 1] - poff[b];
        r.c0 = coff[b]; r.cN = coff[b + 1] - coff[b];
        r.x0 = xoff[b]; r.nx = xoff[b + 1] - xoff[b];
        r.nT = soft ? r.cN : r.cN - 1;
        r.cv0 = cvoff[b]; r.nvd = 3 * (cvoff[b + 1] - cvoff[b]);
        r.wbase = r.p0 - b;
        r.ntasks = (r.N + ppw - 1) / ppw;
        out[b] = r;
    }
}

} // namespace frx
