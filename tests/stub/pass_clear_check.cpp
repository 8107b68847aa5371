// Stand-alone check of sketchy_amd/csrc/skx_pass_clear.hpp (plain C++, no HIP): the table of ranges a deferred pass hands to
// pass_clear_kernel.  For the extreme batch counts, row strides and row extents: every range lies inside its array, no two ranges
// overlap, each slot is cleared exactly as far as its LAST use could have dirtied it, and a full table is refused, not truncated.
// Built and run by tests/test_pass_clear_cpu.py (with -fsanitize=address,undefined).  Prints "<checks> checks, <n> failures".
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "skx_pass_clear.hpp"

static long n_checks = 0, n_fail = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        ++n_checks;                                                              \
        if (!(c)) { ++n_fail; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } \
    } while (0)

struct Buf { unsigned char* p; size_t bytes; };

static void inside_and_disjoint(const skx::PassClear& pc, const std::vector<Buf>& bufs) {
    std::vector<std::pair<const unsigned char*, const unsigned char*>> iv;
    for (unsigned k = 0; k < pc.n; ++k) {
        const unsigned char* a = (const unsigned char*)pc.r[k].p;
        const unsigned char* e = a + pc.r[k].bytes;
        CHECK(pc.r[k].bytes > 0 && pc.r[k].bytes % 4 == 0 && ((size_t)a & 3u) == 0);
        bool in = false;
        for (const Buf& b : bufs) in = in || (a >= b.p && e <= b.p + b.bytes);
        CHECK(in);
        iv.push_back({a, e});
    }
    std::sort(iv.begin(), iv.end());
    for (size_t i = 1; i < iv.size(); ++i) CHECK(iv[i - 1].second <= iv[i].first);
}

int main() {
    const unsigned strides[] = {1, 64, 192, 65536 + 128, 1037056 + 128};
    for (unsigned stride : strides) {
        std::vector<unsigned> rowcnt((size_t)skx::kClearSlotsMax * stride), smap((size_t)skx::kClearSlotsMax * stride);
        const std::vector<Buf> bufs = {{(unsigned char*)rowcnt.data(), rowcnt.size() * 4}, {(unsigned char*)smap.data(), smap.size() * 4}};
        skx::SlotExtents e_cnt, e_map;  // (fresh: nothing known -- whole slots)
        // a sequence of passes of every size: n_b batches, rows [0, nq_rows) each
        const unsigned nbs[] = {8, 1, 8, 3, 0, 8}, rows_of[] = {stride, 1, stride / 2 + 1, 0, 7, stride};
        unsigned dirty[skx::kClearSlotsMax];  // what a slot really holds (model): rows its last use wrote, or everything
        for (unsigned& d : dirty) d = stride;
        for (int pass = 0; pass < 6; ++pass) {
            const unsigned n_b = nbs[pass], nq_rows = std::min(rows_of[pass], stride);
            skx::PassClear pc;
            CHECK(skx::clear_add_slots(pc, rowcnt.data(), stride, e_cnt, n_b));
            CHECK(skx::clear_add_slots(pc, smap.data(), stride, e_map, n_b));
            CHECK(pc.n <= 2 * n_b);
            inside_and_disjoint(pc, bufs);
            // every slot of the pass is cleared as far as it is dirty: ranges come in slot order, the row counts first
            unsigned k = 0;
            for (int arr = 0; arr < 2; ++arr)
                for (unsigned i = 0; i < n_b; ++i) {
                    if (dirty[i] == 0) continue;  // (nothing to clear: no range)
                    const unsigned* base = (arr ? smap.data() : rowcnt.data()) + (size_t)i * stride;
                    CHECK(k < pc.n && pc.r[k].p == (void*)base && pc.r[k].bytes == (unsigned long long)dirty[i] * 4 && pc.r[k].fill == 0);
                    ++k;
                }
            CHECK(k == pc.n);
            e_cnt.used(n_b, nq_rows); e_map.used(n_b, nq_rows);
            for (unsigned i = 0; i < n_b; ++i) dirty[i] = nq_rows;
        }
        // after a regrow / reset / failed pass: whole slots again
        e_cnt.whole();
        skx::PassClear pc;
        CHECK(skx::clear_add_slots(pc, rowcnt.data(), stride, e_cnt, skx::kClearSlotsMax));
        CHECK(pc.n == skx::kClearSlotsMax);
        for (unsigned i = 0; i < pc.n; ++i) CHECK(pc.r[i].bytes == (unsigned long long)stride * 4);
        inside_and_disjoint(pc, bufs);
    }
    {   // the table: zero-length ranges take no entry, misaligned ones and the entry past the last are refused
        skx::PassClear pc;
        unsigned w[64];
        CHECK(skx::clear_add(pc, w, 0) && pc.n == 0);
        CHECK(!skx::clear_add(pc, (unsigned char*)w + 2, 8) && pc.n == 0);
        CHECK(!skx::clear_add(pc, w, 6) && pc.n == 0);
        CHECK(skx::clear_add(pc, w, 8, 0xFFu) && pc.n == 1 && pc.r[0].fill == 0xFFu);
        for (unsigned i = 1; i < skx::kClearRangesMax; ++i) CHECK(skx::clear_add(pc, w + i, 4));
        CHECK(pc.n == skx::kClearRangesMax && !skx::clear_add(pc, w, 4) && pc.n == skx::kClearRangesMax);
        // what a pass of eight batches with every row class puts into it fits: 14 whole arrays + 2 x 8 slots
        CHECK(14 + 2 * skx::kClearSlotsMax <= skx::kClearRangesMax);
    }
    printf("%ld checks, %ld failures\n", n_checks, n_fail);
    return n_fail ? 1 : 0;
}
