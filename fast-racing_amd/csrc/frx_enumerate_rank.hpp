// The rank order of the vertex enumeration's plane triples and plane pairs in plain C++: lane t of window r0 of k_enumerate
// (frx_enumerate_kernel.hpp) works on the triple of rank r0 + t, and its verdict loop on the pair of rank p.  Integer arithmetic only, no floating-point root:
// two binary searches over closed-form counts.  tests/hostcheck/enumerate_rank_main.cpp runs every rank of every K it names against the nested loops under
// the sanitizers; the kernel includes this file as it stands.
#pragma once

// what the kernel calls as well
#if defined(__HIPCC__)
#define FRX_RANK_HD __host__ __device__ __forceinline__
#else
#define FRX_RANK_HD inline
#endif

namespace frx {

FRX_RANK_HD int hv_c3(int n) { return n * (n - 1) * (n - 2) / 6; }             // C(n, 3), n <= 256: below 2^24
FRX_RANK_HD int hv_before(int m, int i) { return i * (2 * m - i - 1) / 2; }    // pairs (p < q) of m elements with p < i

// the triple of rank r in the lexicographic order of a < b < c < K
FRX_RANK_HD void hv_unrank(int K, int r, int &a, int &b, int &c) {
    const int tot = hv_c3(K);
    int lo = 0, hi = K - 3;                                            // largest a with (triples whose first index is below a) <= r
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tot - hv_c3(K - mid) <= r) lo = mid; else hi = mid - 1; }
    a = lo;
    const int r1 = r - (tot - hv_c3(K - a)), m = K - a - 1;
    lo = 0; hi = m - 2;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (hv_before(m, mid) <= r1) lo = mid; else hi = mid - 1; }
    b = a + 1 + lo;
    c = b + 1 + (r1 - hv_before(m, lo));
}
FRX_RANK_HD void hv_unrank_pair(int K, int r, int &a, int &b) {
    int lo = 0, hi = K - 2;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (hv_before(K, mid) <= r) lo = mid; else hi = mid - 1; }
    a = lo;
    b = a + 1 + (r - hv_before(K, lo));
}

} // namespace frx
