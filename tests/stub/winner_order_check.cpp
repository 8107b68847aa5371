// Stand-alone check of sketchy_amd/csrc/skx_winner_order.hpp (plain C++, no HIP): the global order of winner-takes-all breadth -- the
// larger containment covered / max(len, 1) as an exact fraction, then the larger covered, then the lower index -- and the rank per padded
// genome built from it.  Against a brute-force comparison of the two fractions in 128-bit integers: tie-rich inputs (few distinct values),
// len = 0, covered and len near 2^32 - 1 (products near 2^64), and padded layouts of one and several species whose padding entries hold
// garbage.  Built and run by tests/test_winners_cpu.py (with -fsanitize=address,undefined).  Prints "<checks> checks, <n> failures".
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "skx_winner_order.hpp"

static long n_checks = 0, n_fail = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        ++n_checks;                                                              \
        if (!(c)) { ++n_fail; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } \
    } while (0)

typedef unsigned __int128 u128;

// -1: g first, +1: h first (g != h: never 0)
static int brute(uint32_t cov_g, uint32_t len_g, uint32_t g, uint32_t cov_h, uint32_t len_h, uint32_t h) {
    const u128 lg = len_g ? len_g : 1, lh = len_h ? len_h : 1;
    const u128 a = (u128)cov_g * lh, b = (u128)cov_h * lg;  // cov_g / lg ? cov_h / lh
    if (a != b) return a > b ? -1 : 1;
    if (cov_g != cov_h) return cov_g > cov_h ? -1 : 1;
    return g < h ? -1 : 1;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

// every pair of the values, both ways
static void pairs(const std::vector<uint32_t>& cov, const std::vector<uint32_t>& len) {
    const uint32_t n = (uint32_t)cov.size();
    for (uint32_t g = 0; g < n; ++g) {
        CHECK(!skx::winner_precedes(cov[g], len[g], g, cov[g], len[g], g));  // (irreflexive)
        for (uint32_t h = 0; h < n; ++h) {
            if (g == h) continue;
            const bool gh = skx::winner_precedes(cov[g], len[g], g, cov[h], len[h], h);
            CHECK(gh == (brute(cov[g], len[g], g, cov[h], len[h], h) < 0));
            CHECK(gh != skx::winner_precedes(cov[h], len[h], h, cov[g], len[g], g));  // (total: exactly one of the two)
        }
    }
}

// a padded layout: species of the given sizes, each starting on a multiple of 512
static void layout(const std::vector<uint32_t>& sizes, uint32_t cov_kinds, uint32_t len_kinds, bool huge) {
    std::vector<uint32_t> g0, pad_of, len;
    uint32_t g = 0;
    for (uint32_t n : sizes) {
        g0.push_back(g);
        for (uint32_t i = 0; i < n; ++i) pad_of.push_back(g + i);
        g += (n + 511u) / 512u * 512u;
    }
    const uint32_t n_pad = g, n = (uint32_t)pad_of.size();
    std::vector<uint32_t> cov_pad(n_pad);
    for (uint32_t p = 0; p < n_pad; ++p) cov_pad[p] = 0xDEAD0000u + rnd() % 7u;  // (padding: garbage the construction must not read as a genome)
    std::vector<uint32_t> cov(n);
    for (uint32_t i = 0; i < n; ++i) {
        len.push_back(huge ? 0xFFFFFFFFu - rnd() % len_kinds : rnd() % len_kinds);  // (len = 0 occurs)
        cov[i] = huge ? 0xFFFFFFFFu - rnd() % cov_kinds : rnd() % cov_kinds;
        cov_pad[pad_of[i]] = cov[i];
    }
    std::vector<uint32_t> order, rank;
    skx::winner_ranks((uint32_t)sizes.size(), sizes.data(), g0.data(), cov_pad.data(), len.data(), n_pad, order, rank);
    CHECK(order.size() == n && rank.size() == n_pad);
    if (order.size() != n || rank.size() != n_pad) return;
    std::vector<uint32_t> seen(n, 0), real_of(n_pad, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < n; ++i) real_of[pad_of[i]] = i;
    for (uint32_t p = 0; p < n_pad; ++p) {
        if (real_of[p] == 0xFFFFFFFFu) { CHECK(rank[p] == 0xFFFFFFFFu); continue; }
        CHECK(rank[p] < n);
        if (rank[p] < n) { ++seen[rank[p]]; CHECK(order[rank[p]] == real_of[p]); }
    }
    for (uint32_t i = 0; i < n; ++i) CHECK(seen[i] == 1);  // (a permutation of 0 .. n - 1)
    for (uint32_t i = 0; i + 1 < n; ++i) CHECK(brute(cov[order[i]], len[order[i]], order[i], cov[order[i + 1]], len[order[i + 1]], order[i + 1]) < 0);
    if (n <= 200)
        for (uint32_t a = 0; a < n; ++a)
            for (uint32_t b = 0; b < n; ++b)
                if (a != b) CHECK((rank[pad_of[a]] < rank[pad_of[b]]) == (brute(cov[a], len[a], a, cov[b], len[b], b) < 0));
}

int main() {
    // the rules one by one
    CHECK(skx::winner_precedes(2, 4, 5, 1, 4, 0));    // larger containment, whatever the index
    CHECK(skx::winner_precedes(2, 4, 5, 1, 2, 0));    // 2/4 == 1/2: the larger covered
    CHECK(!skx::winner_precedes(1, 2, 0, 2, 4, 5));
    CHECK(skx::winner_precedes(3, 9, 1, 3, 9, 2));    // all equal: the lower index
    CHECK(skx::winner_precedes(0, 0, 1, 0, 7, 2));    // 0/1 == 0/7, covered equal: the index
    CHECK(skx::winner_precedes(1, 0, 9, 1, 2, 0));    // len = 0 counts as 1: 1/1 > 1/2
    // products near 2^64: 64 bits hold them, and neighbours still differ
    const uint32_t M = 0xFFFFFFFFu;
    CHECK(skx::winner_precedes(M, M - 1, 1, M, M, 0));          // M / (M - 1) > M / M
    CHECK(skx::winner_precedes(M, M, 1, M - 1, M, 0));          // M / M > (M - 1) / M
    CHECK(skx::winner_precedes(M - 1, M - 1, 1, M - 2, M - 1, 0));
    CHECK(skx::winner_precedes(M, M, 0, M - 1, M - 1, 1));      // 1 == 1: the larger covered
    CHECK(!skx::winner_precedes(M - 1, M, 0, M, M, 1));
    {
        std::vector<uint32_t> cov, len;
        for (uint32_t c : {0u, 1u, 2u, 3u, 6u, 48u, M - 2, M - 1, M})
            for (uint32_t l : {0u, 1u, 2u, 3u, 4u, 48u, 96u, M - 2, M - 1, M}) { cov.push_back(c); len.push_back(l); }
        pairs(cov, len);   // (covered > len does not occur in the library; the order is defined for it all the same)
        cov.clear(); len.clear();
        for (int i = 0; i < 120; ++i) { cov.push_back(rnd() % 4u); len.push_back(rnd() % 3u); }          // tie-rich
        pairs(cov, len);
        cov.clear(); len.clear();
        for (int i = 0; i < 120; ++i) { cov.push_back(M - rnd() % 5u); len.push_back(M - rnd() % 5u); }  // near 2^32 - 1
        pairs(cov, len);
    }
    for (const auto& sizes : std::vector<std::vector<uint32_t>>{{1}, {2}, {64}, {1300}, {1, 513, 64}, {70, 600, 3}, {512, 512}}) {
        layout(sizes, 3, 2, false);     // almost everything tied: rules two and three decide
        layout(sizes, 29, 49, false);   // the range of the small test designs, len = 0 included
        layout(sizes, 1u << 20, 1u << 20, false);
        layout(sizes, 6, 6, true);      // products near 2^64
    }
    printf("%ld checks, %ld failures\n", n_checks, n_fail);
    return n_fail ? 1 : 0;
}
