// TEST INFRASTRUCTURE: a stand-alone host program around fast-racing_amd/csrc/frx_enumerate_rank.hpp, meant for a sanitizer build (make enumerate_rank_san).
// For every K in 3 ... 96 and K in {127, 128, 129, 191, 192, 193, 255, 256} it walks the three nested loops a < b < c < K and the two nested loops a < b < K
// and asks hv_unrank / hv_unrank_pair for the triple / pair of the running rank; hv_c3(K) and the pair count must equal the number of steps.  The same searches
// are restated here in 64-bit integers, which records the largest magnitude any product, sum or difference reaches: it must stay below 2^31, the range of the
// int the header (and the kernel) computes in - beside the sanitizer, which ends the program at a signed overflow.
// Prints "N triples, M pairs, D disagreements"; exit status 0 and no sanitizer report is the result.
#include <cstdio>

#include "../../fast-racing_amd/csrc/frx_enumerate_rank.hpp"

using namespace frx;
typedef long long i64;

static i64 g_max = 0;
static i64 see(i64 v) { const i64 m = v < 0 ? -v : v; if (m > g_max) g_max = m; return v; }
static i64 w_c3(i64 n) { return see(see(see(n * (n - 1)) * (n - 2)) / 6); }
static i64 w_before(i64 m, i64 i) { return see(see(i * see(see(2 * m - i) - 1)) / 2); }

// hv_unrank and hv_unrank_pair once more, every intermediate seen
static void w_unrank(i64 K, i64 r, i64 &a, i64 &b, i64 &c) {
    const i64 tot = w_c3(K);
    i64 lo = 0, hi = see(K - 3);
    while (lo < hi) { const i64 mid = see(lo + hi + 1) >> 1; if (see(tot - w_c3(see(K - mid))) <= r) lo = mid; else hi = see(mid - 1); }
    a = lo;
    const i64 r1 = see(r - see(tot - w_c3(see(K - a)))), m = see(K - a - 1);
    lo = 0; hi = see(m - 2);
    while (lo < hi) { const i64 mid = see(lo + hi + 1) >> 1; if (w_before(m, mid) <= r1) lo = mid; else hi = see(mid - 1); }
    b = see(a + 1 + lo);
    c = see(see(b + 1) + see(r1 - w_before(m, lo)));
}
static void w_unrank_pair(i64 K, i64 r, i64 &a, i64 &b) {
    i64 lo = 0, hi = see(K - 2);
    while (lo < hi) { const i64 mid = see(lo + hi + 1) >> 1; if (w_before(K, mid) <= r) lo = mid; else hi = see(mid - 1); }
    a = lo;
    b = see(see(a + 1) + see(r - w_before(K, lo)));
}

static i64 n_triples = 0, n_pairs = 0, n_bad = 0;

static void bad(const char *what, int K, i64 r, int a, int b, int c, i64 x, i64 y, i64 z) {
    if (n_bad++ < 20) std::printf("%s K=%d rank=%lld: loops (%d, %d, %d), got (%lld, %lld, %lld)\n", what, K, r, a, b, c, x, y, z);
}

static void run(int K) {
    int r = 0;
    for (int a = 0; a < K - 2; a++)
        for (int b = a + 1; b < K - 1; b++)
            for (int c = b + 1; c < K; c++, r++) {
                int x = -1, y = -1, z = -1;
                hv_unrank(K, r, x, y, z);
                if (x != a || y != b || z != c) bad("hv_unrank", K, r, a, b, c, x, y, z);
                i64 wx = -1, wy = -1, wz = -1;
                w_unrank(K, r, wx, wy, wz);
                if (wx != a || wy != b || wz != c) bad("64-bit restatement", K, r, a, b, c, wx, wy, wz);
                n_triples++;
            }
    if (hv_c3(K) != r) bad("hv_c3", K, r, 0, 0, 0, hv_c3(K), 0, 0);
    see((i64)r + 255);                                                  // the rank of the last lane of the kernel's last window
    int p = 0;
    for (int a = 0; a < K - 1; a++)
        for (int b = a + 1; b < K; b++, p++) {
            int x = -1, y = -1;
            hv_unrank_pair(K, p, x, y);
            if (x != a || y != b) bad("hv_unrank_pair", K, p, a, b, 0, x, y, 0);
            i64 wx = -1, wy = -1;
            w_unrank_pair(K, p, wx, wy);
            if (wx != a || wy != b) bad("64-bit pair restatement", K, p, a, b, 0, wx, wy, 0);
            n_pairs++;
        }
    if (hv_before(K, K - 1) != p || K * (K - 1) / 2 != p) bad("pair count", K, p, 0, 0, 0, hv_before(K, K - 1), K * (K - 1) / 2, 0);
    see((i64)p + 255);
}

int main() {
    for (int K = 3; K <= 96; K++) run(K);
    const int more[] = {127, 128, 129, 191, 192, 193, 255, 256};
    for (int K : more) run(K);
    if (g_max >= (1LL << 31)) { std::printf("an intermediate reaches %lld, beyond int\n", g_max); n_bad++; }
    std::printf("largest intermediate %lld\n", g_max);
    std::printf("%lld triples, %lld pairs, %lld disagreements\n", n_triples, n_pairs, n_bad);
    return n_bad ? 1 : 0;
}
