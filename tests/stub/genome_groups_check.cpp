// Stand-alone check of sketchy_amd/csrc/skx_genome_groups.hpp (plain C++, no HIP): a caller's list of genomes -> the aligned groups of 64
// padded genomes that hold one of them.  Against a brute-force real2pad built here from the same layout: one species of 1 genome, one of
// 1300, three of 1, 513 and 64 (each starting on a 512 boundary); lists that are empty, one genome, every genome reversed, duplicates, the
// last genome of each species with the first of the next, and an out-of-range entry first, in the middle and last (the FIRST offender is
// reported).  Built and run by tests/test_genome_groups_cpu.py (with -fsanitize=address,undefined).  Prints "<checks> checks, <n> failures".
#include <stdint.h>
#include <stdio.h>

#include <set>
#include <vector>

#include "skx_genome_groups.hpp"

static long n_checks = 0, n_fail = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        ++n_checks;                                                              \
        if (!(c)) { ++n_fail; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } \
    } while (0)

struct Layout {
    std::vector<uint32_t> real0, g0, real2pad;
    explicit Layout(const std::vector<uint32_t>& sizes) {
        uint32_t r = 0, g = 0;
        for (uint32_t n : sizes) {
            real0.push_back(r); g0.push_back(g);
            for (uint32_t i = 0; i < n; ++i) real2pad.push_back(g + i);
            r += n; g += (n + 511u) / 512u * 512u;
        }
    }
    uint32_t n_genomes() const { return (uint32_t)real2pad.size(); }
};

// a list without an offender: n comes back, the groups are the brute-force set, ascending
static void good(const Layout& L, const std::vector<uint32_t>& list) {
    std::vector<uint32_t> got;
    const uint32_t n = (uint32_t)list.size();
    CHECK(skx::genome_groups((uint32_t)L.real0.size(), L.real0.data(), L.g0.data(), L.n_genomes(), list.data(), n, got) == n);
    std::set<uint32_t> want;
    for (uint32_t x : list) want.insert(L.real2pad[x] / 64u);
    CHECK(got == std::vector<uint32_t>(want.begin(), want.end()));
    for (uint32_t x : list) {  // (every requested genome lies in a listed group)
        bool in = false;
        for (uint32_t g : got) in = in || L.real2pad[x] / 64u == g;
        CHECK(in);
    }
}
static void bad(const Layout& L, const std::vector<uint32_t>& list, uint32_t first) {
    std::vector<uint32_t> got;
    CHECK(skx::genome_groups((uint32_t)L.real0.size(), L.real0.data(), L.g0.data(), L.n_genomes(), list.data(), (uint32_t)list.size(), got) == first);
}

int main() {
    const std::vector<std::vector<uint32_t>> layouts = {{1}, {1300}, {1, 513, 64}};
    for (const auto& sizes : layouts) {
        const Layout L(sizes);
        const uint32_t n = L.n_genomes();
        good(L, {});
        for (uint32_t x = 0; x < n; ++x) good(L, {x});
        std::vector<uint32_t> rev;
        for (uint32_t x = n; x-- > 0;) rev.push_back(x);
        good(L, rev);
        good(L, {n - 1, 0, n - 1, 0, n / 2, n / 2, n - 1});
        std::vector<uint32_t> edges;  // the last genome of each species and the first of the next
        for (size_t sp = 0; sp + 1 < sizes.size(); ++sp) { edges.push_back(L.real0[sp + 1] - 1); edges.push_back(L.real0[sp + 1]); }
        edges.push_back(n - 1);
        good(L, edges);
        for (uint32_t off : {n, n + 1, 0xFFFFFFFFu}) {
            bad(L, {off}, 0);
            bad(L, {off, 0, n - 1}, 0);
            bad(L, {0, off, n - 1}, 1);
            bad(L, {0, n - 1, off}, 2);
            bad(L, {0, off, n - 1, off + 0u, n}, 1);  // (two offenders: the first one)
            std::vector<uint32_t> longer = rev;
            longer[rev.size() / 2] = off;
            bad(L, longer, (uint32_t)rev.size() / 2);
        }
    }
    printf("%ld checks, %ld failures\n", n_checks, n_fail);
    return n_fail ? 1 : 0;
}
