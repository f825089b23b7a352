// Piece rows -> candidate rows and flag words of frx_trajectory_check / _extrema / _clearance / _clearance_exact / _contain / _map_distance (include/frx.h documents the rows).  Plain C++: no HIP
// and no handle, so the blocking entries (frx_traj.cpp), frx_debug_fold_rows, frx_contain_fold and a host-only program share this one implementation.
//
// One shape: the candidates b = 0..B-1 own the pieces poff[b]..poff[b+1]-1 of T[] and of rows[] (piece rows, FIELDS doubles each), folded in piece order;
// a time is counted from the candidate's start on the prefix of durations summed left to right.  limits = {vel_max, thr_acc_min, thr_acc_max,
// body_rate_max}, compared with no slack.  cand_out ([B][FIELDS]) and flags ([B]) may each be NULL.  A candidate without pieces leaves its row as it is.
#pragma once
#include <cmath>

#include "../../include/frx.h"
#include "frx_math.hpp"

namespace frx {

// The walk the three folds share.  Candidate b's row o (the caller's, or a scratch row when cand_out is NULL) takes its pieces in order through
// merge(o, piece row r, local piece index k, t0 = the piece's start from the candidate's); then flags[b] = bits(o) | `nonfinite` if a field of o is not finite.
template <int FIELDS, class Merge, class Bits>
inline void fold_rows(int B, const int *poff, const double *T, const double *rows, double *cand_out, unsigned *flags, unsigned nonfinite, Merge merge, Bits bits) {
    for (int b = 0; b < B; b++) {
        double own[FIELDS] = {0.0};
        double *o = cand_out ? cand_out + (size_t)FIELDS * b : own;
        double t0 = 0.0;
        for (int gp = poff[b]; gp < poff[b + 1]; gp++) { merge(o, rows + (size_t)FIELDS * gp, gp - poff[b], t0); t0 += T[gp]; }
        if (!flags) continue;
        flags[b] = bits(o);
        for (int f = 0; f < FIELDS; f++)
            if (!std::isfinite(o[f])) flags[b] |= nonfinite;
    }
}
// the four limits, which the check's and the extrema's rows hold in different fields
inline unsigned fold_limit_bits(double speed, double thr_min, double thr_max, double body_rate, const double *limits) {
    return (speed > limits[0] ? FRX_CHECK_FLAG_SPEED : 0u) | (thr_min < limits[1] ? FRX_CHECK_FLAG_THRUST_MIN : 0u) |
           (thr_max > limits[2] ? FRX_CHECK_FLAG_THRUST_MAX : 0u) | (body_rate > limits[3] ? FRX_CHECK_FLAG_BODY_RATE : 0u);
}

// check: max (min for THRUST_MIN), NaN propagating; the worst reach keeps the first piece that attains it (a NaN counts as the worst), with its time
inline void fold_check(int B, const int *poff, const double *T, const double *rows, const double *limits, double *cand_out, unsigned *flags) {
    fold_rows<FRX_CHECK_FIELDS>(B, poff, T, rows, cand_out, flags, FRX_CHECK_FLAG_NONFINITE,
        [](double *o, const double *r, int k, double t0) {
            const double a = o[FRX_CHECK_CORRIDOR], c = r[FRX_CHECK_CORRIDOR];
            if (k == 0 || (a == a && (c > a || c != c))) { o[FRX_CHECK_WORST_T] = k ? t0 + r[FRX_CHECK_WORST_T] : r[FRX_CHECK_WORST_T]; o[FRX_CHECK_WORST_K] = (double)k; }
            for (int f = 0; f < 6; f++) o[f] = k == 0 ? r[f] : f == FRX_CHECK_THRUST_MIN ? nan_min(o[f], r[f]) : nan_max(o[f], r[f]);
        },
        [limits](const double *o) {
            return (o[FRX_CHECK_CORRIDOR] > 0.0 ? FRX_CHECK_FLAG_CORRIDOR : 0u) |
                   fold_limit_bits(o[FRX_CHECK_SPEED], o[FRX_CHECK_THRUST_MIN], o[FRX_CHECK_THRUST_MAX], o[FRX_CHECK_BODY_RATE], limits);
        });
}

// extrema: per field the value with its time; a later piece replaces on strict > (< for THRUST_MIN) or when it is not a number, and a field that is not a
// number stays
inline void fold_extrema(int B, const int *poff, const double *T, const double *rows, const double *limits, double *cand_out, unsigned *flags) {
    fold_rows<FRX_EXTREMA_FIELDS>(B, poff, T, rows, cand_out, flags, FRX_CHECK_FLAG_NONFINITE,
        [](double *o, const double *r, int k, double t0) {
            for (int f = 0; f < 5; f++) {
                const double a = o[f], c = r[f];
                const bool better = f == FRX_EXTREMA_THRUST_MIN ? c < a : c > a;
                if (k == 0 || (a == a && (better || c != c))) { o[f] = c; o[5 + f] = t0 + r[5 + f]; }
            }
        },
        [limits](const double *o) {
            return fold_limit_bits(o[FRX_EXTREMA_SPEED], o[FRX_EXTREMA_THRUST_MIN], o[FRX_EXTREMA_THRUST_MAX], o[FRX_EXTREMA_BODY_RATE], limits);
        });
}

// clearance: the kernel's order on (ELL, piece) - NaN beats any number, then the smaller value, then the earlier piece - with its time and point; DIST is
// a NaN-propagating min.  The limits play no part.
inline void fold_clearance(int B, const int *poff, const double *T, const double *rows, const double *, double *cand_out, unsigned *flags) {
    fold_rows<FRX_CLEAR_FIELDS>(B, poff, T, rows, cand_out, flags, FRX_CLEAR_FLAG_NONFINITE,
        [](double *o, const double *r, int k, double t0) {
            const double a = o[FRX_CLEAR_ELL], c = r[FRX_CLEAR_ELL];
            if (k == 0 || (a == a && (c < a || c != c))) {
                o[FRX_CLEAR_ELL] = c; o[FRX_CLEAR_WORST_T] = k ? t0 + r[FRX_CLEAR_WORST_T] : r[FRX_CLEAR_WORST_T]; o[FRX_CLEAR_WORST_I] = r[FRX_CLEAR_WORST_I];
            }
            o[FRX_CLEAR_DIST] = k == 0 ? r[FRX_CLEAR_DIST] : nan_min(o[FRX_CLEAR_DIST], r[FRX_CLEAR_DIST]);
        },
        [](const double *o) { return o[FRX_CLEAR_ELL] < 1.0 ? FRX_CLEAR_FLAG_COLLISION : 0u; });
}

// exact clearance: ELL and DIST each under the kernel's order on (value, piece) - NaN beats any number, then the smaller value, then the earlier piece - each
// with its own time and point
inline void fold_clearance_exact(int B, const int *poff, const double *T, const double *rows, double *cand_out, unsigned *flags) {
    fold_rows<FRX_CLEAR_EXACT_FIELDS>(B, poff, T, rows, cand_out, flags, FRX_CLEAR_FLAG_NONFINITE,
        [](double *o, const double *r, int k, double t0) {
            const int val[2] = {FRX_CLEAR_EXACT_ELL, FRX_CLEAR_EXACT_DIST}, tm[2] = {FRX_CLEAR_EXACT_T_ELL, FRX_CLEAR_EXACT_T_DIST},
                      pt[2] = {FRX_CLEAR_EXACT_I_ELL, FRX_CLEAR_EXACT_I_DIST};
            for (int f = 0; f < 2; f++) {
                const double a = o[val[f]], c = r[val[f]];
                if (k == 0 || (a == a && (c < a || c != c))) { o[val[f]] = c; o[tm[f]] = t0 + r[tm[f]]; o[pt[f]] = r[pt[f]]; }
            }
        },
        [](const double *o) { return o[FRX_CLEAR_EXACT_ELL] < 1.0 ? FRX_CLEAR_FLAG_COLLISION : 0u; });
    if (!flags) return;
    for (int b = 0; b < B; b++)
        if (poff[b + 1] == poff[b]) flags[b] = 0u;                       // (a row nobody wrote says nothing: ELL = 0 in it is no collision)
}

// map distance: the kernel's order on (DIST, piece) - a value that is not a number first, then the smaller value, then the earlier piece - with its time (-1,
// no sample inside the map, stays -1) and cell; OUTSIDE summed.  A candidate without pieces gets no flag.
inline void fold_map_distance(int B, const int *poff, const double *T, const double *rows, double margin, double *cand_out, unsigned *flags) {
    fold_rows<FRX_MAPDIST_FIELDS>(B, poff, T, rows, cand_out, flags, FRX_MAPDIST_FLAG_NONFINITE,
        [](double *o, const double *r, int k, double t0) {
            const double a = o[FRX_MAPDIST_DIST], c = r[FRX_MAPDIST_DIST];
            if (k == 0 || (a == a && (c < a || c != c))) {
                o[FRX_MAPDIST_DIST] = c; o[FRX_MAPDIST_WORST_CELL] = r[FRX_MAPDIST_WORST_CELL];
                o[FRX_MAPDIST_WORST_T] = r[FRX_MAPDIST_WORST_CELL] >= 0.0 ? t0 + r[FRX_MAPDIST_WORST_T] : -1.0;
            }
            o[FRX_MAPDIST_OUTSIDE] = k == 0 ? r[FRX_MAPDIST_OUTSIDE] : o[FRX_MAPDIST_OUTSIDE] + r[FRX_MAPDIST_OUTSIDE];
        },
        [margin](const double *o) {
            return (o[FRX_MAPDIST_DIST] < margin ? FRX_MAPDIST_FLAG_BELOW : 0u) | (o[FRX_MAPDIST_OUTSIDE] > 0.0 ? FRX_MAPDIST_FLAG_OUTSIDE : 0u);
        });
    if (!flags) return;
    for (int b = 0; b < B; b++)
        if (poff[b + 1] == poff[b]) flags[b] = 0u;                       // (a row nobody wrote says nothing: DIST = 0 in it is below no margin)
}

// contain: N_CONTACT summed; OUTSIDE and CENTRE maxima in piece order (strict > replaces, a value that is not a number takes the field and stays); the
// T_EXIT group from the first piece whose T_EXIT is not -1 (an excursion, or a row that is not a number); K_EXIT and K_CENTRE become the local piece index
inline void fold_contain(int B, const int *poff, const double *T, const double *rows, double *cand_out, unsigned *flags) {
    fold_rows<FRX_CONTAIN_FIELDS>(B, poff, T, rows, cand_out, flags, FRX_CHECK_FLAG_NONFINITE,
        [](double *o, const double *r, int k, double t0) {
            o[FRX_CONTAIN_N_CONTACT] = k == 0 ? r[FRX_CONTAIN_N_CONTACT] : o[FRX_CONTAIN_N_CONTACT] + r[FRX_CONTAIN_N_CONTACT];
            const double a = o[FRX_CONTAIN_OUTSIDE], c = r[FRX_CONTAIN_OUTSIDE];
            if (k == 0 || (a == a && (c > a || c != c))) o[FRX_CONTAIN_OUTSIDE] = c;
            if (k == 0) { o[FRX_CONTAIN_T_EXIT] = -1.0; o[FRX_CONTAIN_T_ENTER] = -1.0; o[FRX_CONTAIN_K_EXIT] = -1.0; }
            if (o[FRX_CONTAIN_T_EXIT] == -1.0 && r[FRX_CONTAIN_T_EXIT] != -1.0) {
                o[FRX_CONTAIN_T_EXIT] = t0 + r[FRX_CONTAIN_T_EXIT]; o[FRX_CONTAIN_T_ENTER] = t0 + r[FRX_CONTAIN_T_ENTER]; o[FRX_CONTAIN_K_EXIT] = (double)k;
            }
            const double a2 = o[FRX_CONTAIN_CENTRE], c2 = r[FRX_CONTAIN_CENTRE];
            if (k == 0 || (a2 == a2 && (c2 > a2 || c2 != c2))) {
                o[FRX_CONTAIN_CENTRE] = c2; o[FRX_CONTAIN_T_CENTRE] = t0 + r[FRX_CONTAIN_T_CENTRE]; o[FRX_CONTAIN_K_CENTRE] = (double)k;
            }
        },
        [](const double *o) { return o[FRX_CONTAIN_T_EXIT] >= 0.0 ? FRX_CHECK_FLAG_CORRIDOR : 0u; });
    if (!flags) return;
    for (int b = 0; b < B; b++)
        if (poff[b + 1] == poff[b]) flags[b] = 0u;                       // (a row nobody wrote says nothing: T_EXIT = 0 in it is no excursion)
}

} // namespace frx
