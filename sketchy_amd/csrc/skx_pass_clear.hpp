// What a deferred pass zero-fills (or 0xFF-fills) before its front half runs: ONE table of ranges, handed to pass_clear_kernel by
// value.  Plain C++ (no HIP): the table is put together on the host and tests/test_pass_clear_cpu.py compiles this header alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace skx {

constexpr unsigned kClearRangesMax = 40;   // 16 whole arrays + 8 batch slots each of the row counts and the rare-row map, and a few to spare
constexpr unsigned kClearSlotsMax = 8;     // (= kPassBatchesMax; skx_kernels.hpp asserts it)
constexpr unsigned kExtentWhole = 0xFFFFFFFFu;  // a slot's extent when nothing is known about it (fresh allocation, reset, failed pass)

struct ClearRange {
    void* p;                 // 4-byte aligned
    unsigned long long bytes;  // a multiple of 4
    unsigned fill;           // 0x00 or 0xFF, every byte
};
struct PassClear {
    unsigned n = 0;
    ClearRange r[kClearRangesMax];
    // the per-batch counters of the compact matrices' rare rows: nqc[i * nqc_stride] = nqc_start, the words between them 0
    unsigned* nqc = nullptr;
    unsigned nqc_words = 0, nqc_stride = 1, nqc_start = 0;
    // the compact matrices of batch slots [0, n_b) (or mqc == NULL: not this pass): rows [0, ext[i]) of each of a slot's n_grp_c
    // groups -- every row of the slots in whole_mask
    unsigned long long* mqc = nullptr;
    unsigned long long* rowany_c = nullptr;
    const unsigned* ext = nullptr;
    unsigned n_b = 0, n_grp_c = 0, rows_c = 0, whole_mask = 0;
};

// one range; false when the table is full (the caller then falls back to a memset of its own: never silently dropped)
inline bool clear_add(PassClear& pc, void* p, size_t bytes, unsigned fill = 0u) {
    if (bytes == 0) return true;
    if (pc.n >= kClearRangesMax || (bytes & 3u) || ((uintptr_t)p & 3u)) return false;
    pc.r[pc.n++] = ClearRange{p, (unsigned long long)bytes, fill};
    return true;
}

// The rows a batch slot's last use could have dirtied, per slot of an array of [slots][stride] u32 (d_rowcnt, smap).  An extent
// describes the LAST use and is cleared at the NEXT: everything beyond it is clean then, whatever the order of large and small
// passes.  kExtentWhole: the whole slot (hipMalloc memory is not zero).
struct SlotExtents {
    unsigned rows[kClearSlotsMax];
    SlotExtents() { whole(); }
    void whole() { for (unsigned i = 0; i < kClearSlotsMax; ++i) rows[i] = kExtentWhole; }
    // this pass writes rows [0, nq_rows) of slots [0, n_b)
    void used(unsigned n_b, unsigned nq_rows) { for (unsigned i = 0; i < n_b && i < kClearSlotsMax; ++i) rows[i] = nq_rows; }
};
// ... as 1D ranges: rows [0, min(extent, stride)) of slots [0, n_b), one range per slot with anything to clear
inline bool clear_add_slots(PassClear& pc, unsigned* base, size_t stride, const SlotExtents& ext, unsigned n_b) {
    for (unsigned i = 0; i < n_b && i < kClearSlotsMax; ++i) {
        const size_t rows = ext.rows[i] < stride ? ext.rows[i] : stride;
        if (!clear_add(pc, base + (size_t)i * stride, rows * 4u)) return false;
    }
    return true;
}

}  // namespace skx
