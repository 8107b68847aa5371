// The global order of winner-takes-all breadth (skx_stream_winners): genome g precedes genome h when its containment covered / len is the
// larger one as an exact fraction, then when its covered is the larger one (Mash's tie rule), then when g < h.  A seen hash is credited to
// the first of its holders in this order; the device needs it as rank[padded genome] = position in the order.  Plain C++ (no HIP):
// tests/test_winners_cpu.py compiles this header alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace skx {

// g, h: global genome indices (species concatenated, the caller's order); len = col_len, lifted hashes included, 0 taken as 1.
// The products are below 2^64 for every pair of u32.
inline bool winner_precedes(uint32_t cov_g, uint32_t len_g, uint32_t g, uint32_t cov_h, uint32_t len_h, uint32_t h) {
    const uint64_t a = (uint64_t)cov_g * std::max<uint32_t>(len_h, 1u), b = (uint64_t)cov_h * std::max<uint32_t>(len_g, 1u);
    if (a != b) return a > b;
    if (cov_g != cov_h) return cov_g > cov_h;
    return g < h;
}

// covered_pad [n_pad]: the counts in PADDED order (species sp's genomes at sp_g0[sp] ..., sp_n[sp] of them; global index = species one after
// the other); col_len [n_genomes] in global order.  rank_pad [n_pad] = position of the genome in the order, 0xFFFFFFFF for padding genomes;
// order [n_genomes] = the global indices, first to last.
inline void winner_ranks(uint32_t n_species, const uint32_t* sp_n, const uint32_t* sp_g0, const uint32_t* covered_pad,
                         const uint32_t* col_len, uint32_t n_pad, std::vector<uint32_t>& order, std::vector<uint32_t>& rank_pad) {
    struct Key { uint32_t cov, len, g, pad; };  // (sorted by value: the comparator touches nothing else)
    std::vector<Key> keys;
    for (uint32_t sp = 0; sp < n_species; ++sp)
        for (uint32_t i = 0; i < sp_n[sp]; ++i) {
            const uint32_t g = (uint32_t)keys.size();
            keys.push_back(Key{covered_pad[sp_g0[sp] + i], col_len[g], g, sp_g0[sp] + i});
        }
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return winner_precedes(a.cov, a.len, a.g, b.cov, b.len, b.g); });
    const uint32_t n = (uint32_t)keys.size();
    order.resize(n);
    rank_pad.assign(n_pad, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < n; ++i) { order[i] = keys[i].g; rank_pad[keys[i].pad] = i; }
}

}  // namespace skx
