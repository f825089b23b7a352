// Host side of the gate passage certificate (frx_trajectory_gates, include/frx.h): gate records from corner poses and the flag words from gate
// rows.  Plain C++: no HIP and no handle, so the blocking entry (frx_traj.cpp), a caller of the _device form and a host-only program share this one implementation.
#pragma once
#include <cmath>

#include "../../include/frx.h"

namespace frx {

inline double gate_norm3(const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// n gates of four corners each (corners [n][4][3], in order round the opening) -> records {c, a, b} ([n][9]); fit ([n][2]) may be NULL:
// {a.b / (|a| |b|), max_i |corner_i - (c -/+ a -/+ b)|}, the corners of the record taken in the same order round the opening
inline void gate_from_corners(int n, const double *corners, double *gates, double *fit) {
    for (int i = 0; i < n; i++) {
        const double *c0 = corners + 12 * (size_t)i, *c1 = c0 + 3, *c2 = c0 + 6, *c3 = c0 + 9;
        double *c = gates + 9 * (size_t)i, *a = c + 3, *b = c + 6;
        for (int d = 0; d < 3; d++) {
            c[d] = (((c0[d] + c1[d]) + c2[d]) + c3[d]) / 4.0;            // the reference's sum (se3_node_cpu.cpp:44-61), then the mean
            a[d] = ((c1[d] - c0[d]) + (c2[d] - c3[d])) / 4.0;
            b[d] = ((c3[d] - c0[d]) + (c2[d] - c1[d])) / 4.0;
        }
        if (!fit) continue;
        fit[2 * i] = (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]) / (gate_norm3(a) * gate_norm3(b));
        const double su[4] = {-1.0, 1.0, 1.0, -1.0}, sv[4] = {-1.0, -1.0, 1.0, 1.0};
        double worst = 0.0;
        for (int q = 0; q < 4; q++) {
            double r[3];
            for (int d = 0; d < 3; d++) r[d] = c0[3 * q + d] - ((c[d] + su[q] * a[d]) + sv[q] * b[d]);
            const double e = gate_norm3(r);
            if (e > worst || e != e) worst = e;
        }
        fit[2 * i + 1] = worst;
    }
}

// flag words of the B candidates from their gate rows: candidate b owns the rows gate_off[b] .. gate_off[b + 1] - 1, in the order the gates are to be flown
inline void gate_flags(int B, const int *gate_off, const double *rows, unsigned *flags) {
    for (int b = 0; b < B; b++) {
        unsigned f = 0u;
        double last = -INFINITY;
        for (int g = gate_off[b]; g < gate_off[b + 1]; g++) {
            const double *r = rows + (size_t)FRX_GATE_FIELDS * g;
            if (r[FRX_GATE_N_PASS] == 0.0) f |= FRX_GATE_FLAG_MISSED;
            if (r[FRX_GATE_N_PASS] > 1.0) f |= FRX_GATE_FLAG_REPEAT;
            if (r[FRX_GATE_N_PASS] > 0.0) {                              // the row names this gate's first passage
                if (!(r[FRX_GATE_TIME] > last)) f |= FRX_GATE_FLAG_ORDER;
                last = r[FRX_GATE_TIME];
            }
            for (int k = 0; k < FRX_GATE_FIELDS; k++)
                if (r[k] != r[k]) f |= FRX_GATE_FLAG_NONFINITE;
        }
        flags[b] = f;
    }
}

} // namespace frx
