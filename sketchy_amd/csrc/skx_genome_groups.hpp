// A list of genomes as the caller numbers them (species concatenated) -> the aligned groups of 64 PADDED genomes that hold one of them,
// the unit of work of the per-genome queries of a stream's statistics (skx_stream_coverage_rows, skx_stream_depth_rows).  Plain C++ (no
// HIP): tests/test_genome_groups_cpu.py compiles this header alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace skx {

// sp_real0[sp] / sp_g0[sp]: first genome of species sp in the caller's order / in padded order (both ascending, sp_real0[0] = 0).
// Returns n and leaves the groups ascending, each once -- or the index of the first entry outside 0 .. n_genomes - 1 (groups: unspecified).
inline uint32_t genome_groups(uint32_t n_species, const uint32_t* sp_real0, const uint32_t* sp_g0, uint32_t n_genomes, const uint32_t* genomes,
                              uint32_t n, std::vector<uint32_t>& groups) {
    groups.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (genomes[i] >= n_genomes) return i;
        uint32_t sp = 0;
        while (sp + 1 < n_species && genomes[i] >= sp_real0[sp + 1]) ++sp;
        groups[i] = (sp_g0[sp] + (genomes[i] - sp_real0[sp])) / 64u;
    }
    std::sort(groups.begin(), groups.end());
    groups.erase(std::unique(groups.begin(), groups.end()), groups.end());
    return n;
}

}  // namespace skx
