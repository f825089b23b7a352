// TEST INFRASTRUCTURE: a stand-alone host program around fast-racing_amd/csrc/frx_traj_fold.hpp, meant for a sanitizer build (make fold_rows_san).
// It folds every case of the text file `python tests/fold_cases.py FILE` writes - with both outputs, with the candidate rows alone and with the flags
// alone, into buffers of exactly the size the header promises - and two cases of its own: a batch whose last candidate has no pieces, and B = 1.
// Exit status 0 and no sanitizer report is the result; the numbers are checked by tests/test_trajectory_fold_cpu.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_traj_fold.hpp"

using Fold = void (*)(int, const int *, const double *, const double *, const double *, double *, unsigned *);
static const Fold FOLD[3] = {frx::fold_check, frx::fold_extrema, frx::fold_clearance};
static const int FIELDS[3] = {FRX_CHECK_FIELDS, FRX_EXTREMA_FIELDS, FRX_CLEAR_FIELDS};

// every array on the heap at its exact size, so that a read or write past an end is reported
static int fold_all_ways(int kind, int B, const std::vector<int> &poff, const std::vector<double> &T, const std::vector<double> &rows, const double *limits) {
    const size_t nc = (size_t)B * FIELDS[kind];
    std::unique_ptr<double[]> cand(new double[nc]), cand2(new double[nc]);
    std::unique_ptr<unsigned[]> flags(new unsigned[B]), flags2(new unsigned[B]);
    std::unique_ptr<double[]> lim(new double[4]);
    std::memcpy(lim.get(), limits, sizeof(double) * 4);
    for (size_t i = 0; i < nc; i++) cand[i] = cand2[i] = -7.0;
    FOLD[kind](B, poff.data(), T.data(), rows.data(), lim.get(), cand.get(), flags.get());
    FOLD[kind](B, poff.data(), T.data(), rows.data(), lim.get(), cand2.get(), nullptr);
    FOLD[kind](B, poff.data(), T.data(), rows.data(), lim.get(), nullptr, flags2.get());
    FOLD[kind](B, poff.data(), T.data(), rows.data(), lim.get(), nullptr, nullptr);
    if (std::memcmp(cand.get(), cand2.get(), sizeof(double) * nc) != 0) return 1;
    for (int b = 0; b < B; b++)
        if (poff[b + 1] > poff[b] && flags[b] != flags2[b]) return 1;       // (a candidate without pieces has no row of its own to flag)
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASES.txt\n", argv[0]); return 2; }
    FILE *fh = std::fopen(argv[1], "r");
    if (!fh) { std::perror(argv[1]); return 2; }
    int kind, B, P, n_cases = 0, bad = 0;
    while (std::fscanf(fh, "%d %d %d", &kind, &B, &P) == 3) {
        if (kind < 0 || kind > 2 || B < 1 || P < 0) { std::fprintf(stderr, "case %d: bad header\n", n_cases); return 2; }
        std::vector<int> poff(B + 1);
        std::vector<double> T(P), rows((size_t)P * FIELDS[kind]);
        double limits[4];
        bool ok = true;
        for (int &v : poff) ok &= std::fscanf(fh, "%d", &v) == 1;
        for (double &v : T) ok &= std::fscanf(fh, "%lf", &v) == 1;
        for (double &v : limits) ok &= std::fscanf(fh, "%lf", &v) == 1;
        for (double &v : rows) ok &= std::fscanf(fh, "%lf", &v) == 1;
        if (!ok || poff[0] != 0 || poff[B] != P) { std::fprintf(stderr, "case %d: bad body\n", n_cases); return 2; }
        bad += fold_all_ways(kind, B, poff, T, rows, limits);
        n_cases++;
    }
    std::fclose(fh);
    if (n_cases == 0) { std::fprintf(stderr, "no cases in %s\n", argv[1]); return 2; }

    const double limits[4] = {6.0, 2.0, 18.0, 3.5};
    for (kind = 0; kind < 3; kind++) {
        const int F = FIELDS[kind];
        // three candidates of 2, 1 and 0 pieces: the last one owns nothing
        std::vector<double> T = {0.5, 0.25, 1.5}, rows((size_t)3 * F);
        for (size_t i = 0; i < rows.size(); i++) rows[i] = 0.125 * (double)(i % 11) + 1.0;
        bad += fold_all_ways(kind, 3, {0, 2, 3, 3}, T, rows, limits);
        // B = 1, one piece and three
        bad += fold_all_ways(kind, 1, {0, 1}, T, rows, limits);
        bad += fold_all_ways(kind, 1, {0, 3}, T, rows, limits);
        n_cases += 3;
    }
    std::printf("%d cases folded, %d disagreements between the output forms\n", n_cases, bad);
    return bad ? 1 : 0;
}
