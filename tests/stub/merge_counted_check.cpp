// formats.hpp's merge_counted (two ascending rows with counts -> the first s values of their union, counts of equal values added,
// saturating) against a std::map reference, over a few thousand random pairs of rows of every shape: disjoint, identical,
// interleaved, a cut that falls on a shared value, counts that saturate.  Stand-alone: tests/test_sketch_counts_cpu.py compiles it
// with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

#include "formats.hpp"

using Row = std::pair<std::vector<uint64_t>, std::vector<uint32_t>>;

static int failures = 0;

static void check(const Row& a, const Row& b, size_t s, const char* what) {
    std::map<uint64_t, uint64_t> ref;
    for (size_t i = 0; i < a.first.size(); ++i) ref[a.first[i]] += a.second[i];
    for (size_t i = 0; i < b.first.size(); ++i) ref[b.first[i]] += b.second[i];
    std::vector<uint64_t> want; std::vector<uint32_t> want_counts;
    for (const auto& kv : ref) {
        if (want.size() == s) break;
        want.push_back(kv.first);
        want_counts.push_back(kv.second > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)kv.second);
    }
    std::vector<uint64_t> out{1, 2, 3}; std::vector<uint32_t> out_counts{9};  // (stale content must go)
    sketchy::merge_counted(a.first.data(), a.second.data(), a.first.size(), b.first.data(), b.second.data(), b.first.size(), s, out, out_counts);
    if (out != want || out_counts != want_counts) {
        std::fprintf(stderr, "FAIL %s: |a| = %zu, |b| = %zu, s = %zu: %zu values (want %zu)\n", what, a.first.size(), b.first.size(), s, out.size(), want.size());
        ++failures;
    }
}

int main() {
    std::mt19937_64 rng(12345);
    auto count = [&](bool big) -> uint32_t {
        if (big) return 0xFFFFFFFFu - (uint32_t)(rng() % 3);                 // saturates with anything >= 3
        return (rng() % 8 == 0) ? (uint32_t)(rng() % 0xFFFFFFFFull) + 1u : (uint32_t)(rng() % 100) + 1u;
    };
    // a row of n distinct ascending values drawn from [0, span), counts >= 1
    auto row = [&](size_t n, uint64_t span, bool big) {
        std::map<uint64_t, uint32_t> m;
        while (m.size() < n) m.emplace(rng() % span, count(big));
        Row r;
        for (const auto& kv : m) { r.first.push_back(kv.first); r.second.push_back(kv.second); }
        return r;
    };
    size_t n_cases = 0;
    for (int it = 0; it < 4000; ++it) {
        const size_t na = rng() % 40, nb = rng() % 40;
        const bool big = it % 5 == 0;
        Row a = row(na, 64 + rng() % 200, big), b;
        const char* what = "";
        switch (it % 4) {
        case 0: {  // disjoint: b above a, below a, or on the odd values while a is on the even ones
            what = "disjoint";
            b = row(nb, 64 + rng() % 200, big);
            const uint64_t mode = rng() % 3;
            if (mode == 2) { for (auto& v : a.first) v = 2 * v; for (auto& v : b.first) v = 2 * v + 1; }
            else for (auto& v : (mode ? a.first : b.first)) v += 1000;
            break;
        }
        case 1: what = "identical"; b = a; for (auto& c : b.second) c = count(big); break;
        case 2: what = "interleaved"; b = row(nb, 64 + rng() % 200, big); break;  // (small span: many shared values)
        default: {  // a cut that falls on a shared value: s = position of a value both rows hold, and one more
            what = "cut on a shared value";
            b = row(nb, 64 + rng() % 200, big);
            if (!a.first.empty()) {
                const size_t i = rng() % a.first.size();
                std::map<uint64_t, uint32_t> m;
                for (size_t j = 0; j < b.first.size(); ++j) m[b.first[j]] = b.second[j];
                m[a.first[i]] = count(big);
                b = Row();
                for (const auto& kv : m) { b.first.push_back(kv.first); b.second.push_back(kv.second); }
                std::map<uint64_t, int> u;
                for (auto v : a.first) u[v]; for (auto v : b.first) u[v];
                size_t pos = 0;
                for (const auto& kv : u) { if (kv.first == a.first[i]) break; ++pos; }
                check(a, b, pos, what); check(a, b, pos + 1, what); n_cases += 2;
            }
            break;
        }
        }
        const size_t total = a.first.size() + b.first.size();
        for (size_t s : {(size_t)1, total / 2 + 1, total, total + 5, (size_t)(rng() % (total + 1)) + 1}) { check(a, b, s, what); ++n_cases; }
    }
    // saturation, spelled out
    check({{5}, {0xFFFFFFFFu}}, {{5}, {0xFFFFFFFFu}}, 4, "saturation");
    check({{5, 9}, {0xFFFFFFFEu, 7}}, {{5, 9}, {1, 8}}, 4, "saturation");
    check({{5}, {0xFFFFFFFEu}}, {{5}, {2}}, 1, "saturation");
    check({{}, {}}, {{}, {}}, 3, "empty");
    std::printf("%zu cases, %d failures\n", n_cases + 4, failures);
    return failures ? 1 : 0;
}
