// TEST INFRASTRUCTURE: a stand-alone host program around fast-racing_amd/csrc/frx_eval_front.hpp, meant for a sanitizer build (tests/test_eval_front_cpu.py compiles it with
// -fsanitize=address,undefined and runs it; host code only, never loaded into Python).  It builds the offset tables of a few batches the way frx_problem_create does,
// fills the front records from them and compares every field of every record with the table expression k_eval_cluster and forward_knot_body use without the record.
// Exit status 0 and no sanitizer report is the result.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../fast-racing_amd/csrc/frx_eval_front.hpp"

using namespace frx;

static int check_batch(const std::vector<int> &pieces, bool soft, int ppw, int *fields) {
    const int B = (int)pieces.size();
    // tables at their exact sizes on the heap, so that a read past B + 1 entries is reported
    std::unique_ptr<int[]> poff(new int[B + 1]), coff(new int[B + 1]), xoff(new int[B + 1]), cvoff(new int[B + 1]);
    poff[0] = coff[0] = xoff[0] = cvoff[0] = 0;
    for (int b = 0; b < B; b++) {
        const int N = pieces[b];
        const int cN = (N + 1) / 2 + (b % 2);                                   // coarse pieces: any count in [1, N] will do, and it differs between neighbours
        const int cNc = cN < 1 ? 1 : (cN > N ? N : cN);
        int nv = 0;
        for (int w = 0; w < N - 1; w++) nv += 8 + (w + b) % 5;                  // vertices per waypoint polytope
        const int nxi = nv - (N - 1);                                           // one barycentric variable less than vertices per waypoint
        poff[b + 1] = poff[b] + N;
        coff[b + 1] = coff[b] + cNc;
        xoff[b + 1] = xoff[b] + (soft ? cNc : cNc - 1) + nxi;
        cvoff[b + 1] = cvoff[b] + nv;
    }
    std::unique_ptr<EvalFront[]> rec(new EvalFront[B]);
    eval_front_fill(B, poff.get(), coff.get(), xoff.get(), cvoff.get(), soft, ppw, rec.get());
    int bad = 0;
    for (int b = 0; b < B; b++) {
        const EvalFront &r = rec[b];
        bad += (reinterpret_cast<uintptr_t>(&r) & 63u) != 0;                    // every record on a line of its own
        // the kernel's own expressions (frx_eval_kernel.hpp, forward_knot_body in frx_kernels.hpp)
        const int p0 = poff[b], N = poff[b + 1] - p0;
        const int c0 = coff[b], cN = coff[b + 1] - c0;
        const int x0 = xoff[b], nx = xoff[b + 1] - x0;
        const int nT = soft ? cN : cN - 1;
        const int v0 = cvoff[b], nvd = 3 * (cvoff[b + 1] - v0);
        const int ntasks = (N + ppw - 1) / ppw;
        bad += r.p0 != p0; bad += r.N != N; bad += r.c0 != c0; bad += r.cN != cN; bad += r.x0 != x0; bad += r.nx != nx; bad += r.nT != nT;
        bad += r.cv0 != v0; bad += r.nvd != nvd; bad += r.wbase != p0 - b; bad += r.ntasks != ntasks;
        for (int q = 0; q < 5; q++) bad += r.pad[q] != 0;
        *fields += 16;
    }
    return bad;
}

int main() {
    static_assert(sizeof(EvalFront) == 64, "record size");
    static_assert(alignof(EvalFront) == 64, "record alignment");
    static_assert(offsetof(EvalFront, ntasks) == 40 && offsetof(EvalFront, pad) == 44, "eleven integers, then padding");
    const std::vector<std::vector<int>> batches = {{64}, {64, 7, 9, 3, 2}, {2}, {3}, {64, 5, 12, 3, 33, 64, 8, 2, 17}};
    int bad = 0, fields = 0, records = 0;
    for (const auto &pieces : batches)
        for (int soft = 0; soft < 2; soft++)
            for (int ppw : {3, 7, 1}) { bad += check_batch(pieces, soft != 0, ppw, &fields); records += (int)pieces.size(); }
    {   // nT in both layers on one table: cN with the soft total time, cN - 1 with the fixed one
        const int poff[2] = {0, 5}, coff[2] = {0, 4}, xoff[2] = {0, 20}, cvoff[2] = {0, 40};
        EvalFront a, f;
        eval_front_fill(1, poff, coff, xoff, cvoff, true, 3, &a);
        eval_front_fill(1, poff, coff, xoff, cvoff, false, 3, &f);
        bad += a.nT != 4 || f.nT != 3 || a.cN != 4 || f.cN != 4 || a.ntasks != 2 || a.nvd != 120;
        fields += 6;
    }
    std::printf("%d records, %d fields compared, %d disagreements with the table expressions\n", records, fields, bad);
    return bad ? 1 : 0;
}
