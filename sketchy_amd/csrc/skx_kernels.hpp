// skx_kernels.hpp -- launch wrappers of the gfx950 kernels (skx_kernels.hip).  Internal to libsketchy_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <stdlib.h>

#include "skx_pass_clear.hpp"

namespace skx {
typedef unsigned long long u64;
typedef unsigned int u32;

// Experiment / test knobs: environment variables that pick a kernel variant, a stream arrangement, a pass size or -- the
// profiling aids SKX_SCAN_ABLATE and SKX_NO_FILTER -- change what the kernels compute.  They exist only in the
// -DSKX_EXPERIMENTS build (sketchy_amd/libsketchy_hip_exp.so, used by tests/ and tools/ through SKX_LIB_PATH); the
// product library reads no environment variable at all.
inline const char* knob(const char* name) {
#ifdef SKX_EXPERIMENTS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

constexpr int kSketchCap = 2048;   // k-mers per read the one-wave-per-read sketcher holds in LDS
constexpr u32 kSegLen = 64;        // reads per ranking segment
constexpr int kRankWords = 8;      // genome words (x64 genomes) per ranking wave = one 64-byte sector of Mq per pair

// Species: several reference collections share one matrix, each padded to whole rank groups (512 genomes); every species
// has its own ranking.  Device arrays: g0[sp] first padded genome index, n[sp] real genomes, of_grp[rank group] species.
struct Species { const u32* g0; const u32* n; const u32* of_grp; u32 n_sp; };

// reference upload: src / eff_len start at the chunk's first genome, which sits at padded index pad_base
void launch_ref_tile(hipStream_t st, const u64* src, const u32* eff_len, u64* dst, u32 s, u32 pad_base, u32 g_count);
void launch_band_bounds(hipStream_t st, const u64* mat, u32 s, u32 n_tiles, u32 rb, u32 n_bands, u64* lo, u64* hi);

// Long reads of a production batch are split over waves (skx_kernels.hip, "long reads: split over waves"): device tables
// built by launch_batch_check and consumed by launch_sketch.  Capacities: a read is long beyond long_read_split() raw
// bytes and takes ceil(length / kSketchCap) segment slots, so a batch of at most B bases needs at most
// B / long_read_split() + 1 list entries and 5 B / (4 kSketchCap) + 1 slots (the caller sizes them from max_batch_bases).
struct LongReads {
    u32* list;     // [long_cap] read index
    u32* seg0;     // [long_cap] first segment slot of the read
    u32* seg_tab;  // [segs_cap] position in `list` of the read a segment slot belongs to
    u32* seg_cnt;  // [segs_cap] hashes the segment kept
    u64* seg_h;    // [segs_cap][long_read_seg_slots()]
    u32 segs_cap, long_cap;
};
u32 long_read_split();
u32 long_read_seg_slots();
u32 pool_row_fixed();  // entries of a read's fixed slot at the start of the row pool
u32 chk_words();  // u32 words of a `chk` block: 16 flags / counters + the row pool's bump counters (one cache line each)

// k-mer prefilter (k = 16): a two-probe blocked Bloom table over the 2-bit code of the CANONICAL k-mer, holding every
// k-mer whose MurmurHash3 value passes the reference's membership filter (<= max_ref and bit set) -- built once per
// reference by enumerating all 4^16 / 2 canonical 16-mers (~10 ms of VALU work on an MI355X).  A read with at most s k-mer
// windows cannot be truncated (its sketch is ALL its distinct hashes), so only k-mers that can end up as (read, hash) pairs
// matter: the sketcher looks every window up in this table (one 4-byte gather) and runs murmur3 only on the survivors,
// compacted through the wave's LDS -- ~30 instead of ~100 VALU instructions per 64 windows.  Exact: the table has no
// false negatives; false positives are hashed and then dropped by the in-range / membership tests as before.
struct KmerFilter { const u32* words; u32 shift; };  // word = (code * kKmerMix) >> shift; bits (m & 31), ((m >> 5) & 31)
// count (pass 1) / insert (pass 2) the canonical 16-mers whose hash passes (max_ref, filt); *n_keys accumulates in pass 1
void launch_kmer_filter_build(hipStream_t st, u64 seed, u64 max_ref, const u64* filt, u32 filt_shift, u32* n_keys /* pass 1 */,
                              u32* words /* pass 2, zeroed */, u32 shift);

// sketching: every read of the batch, any length -- one wave per read (256 hash slots, then 2048 for the reads that
// overflow); what still does not fit (and, for full sketches, every read with more than kSketchCap k-mers) is left on the
// device-side list `big` for launch_sketch_block (one block per read).  `retry` / `big`: [0] = count, zero on entry.
// n_bases: bytes the caller vouches for from offsets[0] on; a read reaching outside is skipped and flagged in chk[6]
// (chk may be NULL).  long_reads (production batches, with chk): the tables launch_batch_check filled for this batch.
// Returns the launch status (it also opts the big-LDS kernels in, once per device).
hipError_t launch_sketch(hipStream_t st, const uint8_t* bases, const u64* offsets, u32 n_reads, u32 k, u64 seed, u32 s,
                         u64 max_ref, bool inrange_only, u64* out_sk, u32 sk_stride, u32* out_len, u32* out_cnt_in,
                         const u64* filt /* membership filter applied in inrange_only mode, or NULL */, u32 filt_shift,
                         u32* retry /* [1 + n_reads] */, u32* big /* [1 + n_reads] */, u64 n_bases, u32* chk,
                         int leave_room /* 0 no, 1 a scan overlaps the start, 2 a scan runs beside most of it */, bool packed = false,
                         const LongReads* long_reads = nullptr, const KmerFilter* kmer_filter = nullptr /* production, k = 16 */,
                         int phase = 3 /* production batches: 1 = the main kernel only, 2 = only the list walks behind it, 3 = both */,
                         u32 pool_cap = 0 /* sk_stride == 0 (production): out_sk is a pool of this many entries, out_len receives
                                             every row's start, chk[6] |= 4 on overflow */,
                         u32 pool_fixed = 0 /* its first entries: pool_row_fixed() per read, taken without reservation */);
// the block sketcher for the n_big reads launch_sketch left on `big` (big[1 ..]); the caller reads the count back first
hipError_t launch_sketch_block(hipStream_t st, const uint8_t* bases, const u64* offsets, const u32* big, u32 n_big, u32 k, u64 seed,
                               u32 s, u64 max_ref, bool inrange_only, u64* out_sk, u32 sk_stride, u32* out_len, u32* out_cnt_in,
                               const u64* filt, u32 filt_shift, bool packed = false, u32* chk = nullptr, u32 pool_cap = 0,
                               u32 pool_fixed = 0);
// exclusive scan of n counts (out[i] = sum of in[0..i)); bsum: [ceil(n / 1024)] scratch
void launch_count_scan(hipStream_t st, const u32* in, u32* out, u32 n, u32* bsum);

// Rare-hash index of a reference (skx_kernels.hip, "rare-hash index"): open-addressing table over the distinct reference hashes
// (key, all-ones = empty; mask = slots - 1), cnt = genomes that hold the hash, off = start of its genome list in post (padded genome
// indices) -- or 0xFFFFFFFF for a hash held by more genomes than the policy "rare_hash_genomes": those stay with the scan.
struct RareIndex { const u64* key; const u32* off; const u32* cnt; const u32* post; u32 mask;
                   // long lists (more than 8 genomes) also as BIT ROWS: mlong[lid][n_gw] u64, bit g of a row = genome g holds the hash;
                   // lid[key slot] = row (0xFFFFFFFF: none), lslot[row] = key slot.  NULL when there was no room for the rows.
                   const u64* mlong = nullptr; const u32* lid = nullptr; const u32* lslot = nullptr; u32 n_gw = 0;
                   // ... and the same bits TRANSPOSED: mlongT[genome][n_lw] u64, bit r of a genome's row = bit row r holds the genome
                   // (n_lw = ceil(rows / 64) words; NULL when there was no room): which of a batch's long-list rows meet a candidate is
                   // then an AND of the candidate's row with the batch's row mask, not a walk over every row (launch_cand_hit)
                   const u64* mlongT = nullptr; u32 n_lw = 0;
                   // ... and most long lists as (pattern, exceptions) (round 6; skx_kernels.hip, "long lists as (pattern, exceptions)"):
                   // prec[bit row][pat_record_words()] = {pattern or 0xFFFFFFFF, n, n x (genome | not-on-the-list << 31)}; pat_rep[pattern] =
                   // the bit row whose list IS the pattern; pm[word of 64 patterns][n_pad] the patterns' bits in M's layout; d_npat[0] = n_pat
                   const u32* prec = nullptr; const u32* pat_rep = nullptr; const u64* pm = nullptr; const u32* d_npat = nullptr; u32 n_pat = 0;
                   // the STATIC dense dictionary (round 6): qs[0 .. n_sd) = every hash the scan can be asked for (held by more genomes than
                   // the index lists, + the lifted hashes), ascending; a pass's dense rows are ITS rows (launch_classify); NULL: per-pass dictionaries
                   // (several species: the species' sorted segments one after the other, each starting on a multiple of 64 rows, padded with
                   // all-ones; srow[key slot] = the hash's row; the lifted hashes sorted in the tail [tail0, n_sd))
                   const u64* qs = nullptr; u32 n_sd = 0; const u32* srow = nullptr; u32 tail0 = 0; };
void launch_collect_dense(hipStream_t st, const u64* key, const u32* off, u64 slots, u64* out, u32* out_slot, u32* n, u32 cap);
void launch_window_seg(hipStream_t st, const u64* lo, const u64* hi, u32 n_bt, u32 n_tiles, const u64* q, const u32* seg, const u32* grp_sp, u32* win);
// pattern rows of a pass: hist[b][hist_stride] = occurrences of every pattern among batch b's pairs, gain_x[b][n_pad] += / -= the rows'
// counts at their exceptions (wrapping), nprow[b] (one counter per batch, like LongRows::nlrow) rows listed from the END of lrow[b]
struct PatRows { u32* hist; u32 hist_stride; u32* gain_x; u32* nprow; };
void launch_list_sig(hipStream_t st, const u32* lslot, u32 n_long, const u32* off, const u32* cnt, const u32* post, u32* sig, u64* content);
void launch_pat_exceptions(hipStream_t st, const u64* mlong, u32 n_gw, u32 n_long, const u32* pat_of, const u32* pat_rep, u32* prec, u32* n_done);
void launch_pat_matrix(hipStream_t st, const u64* mlong, const u32* pat_rep, u32 n_pat, u32 n_gw, u64* pm, u32 n_pad);
u32 pat_record_words();
u32 pat_words_max();  // genome words of a compact problem the pattern path handles (more species than that: the stream does not use the patterns)
// long-list rows of a pass, per batch: lrow[b][i] = {bit row, sparse row of the pass's matrix} (nlrow[b] of them, lrow_stride apart)
struct LongRows { uint2* lrow; u32* nlrow; u32 lrow_stride; u64* inb = nullptr; u32 n_lw = 0; };  // inb[b][n_lw] (or NULL; zero on entry): bit r = bit row r is on batch b's list  // (nlrow: one counter per batch, pass_counter_bytes() in all)
u32 pass_counter_bytes();  // size of the per-batch counter arrays of a pass (nlrow, nqc: one cache line per batch)
void launch_mlong_build(hipStream_t st, const u32* lslot, u32 n_long, const u32* off, const u32* cnt, const u32* post, u64* mlong, u32 n_gw);
// gain_l[b][g] (zero on entry) += sum over batch b's long-list rows of cnt x bit: bit-sliced counters over the rows' 64-bit words
void launch_gain_long(hipStream_t st, const LongRows& lr, const RareIndex& ri, const u32* n_d, const u32* cnt, u32 row_stride, u32 n_b, u32 n_pad,
                      u32* gain_l, u32 walk_scale = 1);
// the candidates of every batch by genome word: cw[b][w] their bits, cbase[b][w] the slot of the word's first one, cwl[b][.] / ncwl[b] the
// words that hold any (cw, ncwl zero on entry; cbase all-ones)
void launch_mlong_transpose(hipStream_t st, const u64* mlong, u32 n_long, u32 n_gw, u64* mlongT, u32 n_lw);
// hit[b][n_lw] (zero on entry) |= (row of candidate g in the transposed bit rows) & inb[b], for every candidate of every batch: the
// long-list rows of batch b that hold any of its candidates -- cand_long_kernel then only looks at those
void launch_cand_hit(hipStream_t st, const u32* cand, u32 n_pad_c, u32 n_b, const u32* bad, const RareIndex& ri, const u64* inb, u64* hit);
void launch_cand_words(hipStream_t st, const u32* cand, u32 n_pad_c, u32 n_b, u32 n_gw, u64* cw, u32* cbase, u32* cwl, u32* ncwl);
void launch_cand_long(hipStream_t st, const LongRows& lr, const RareIndex& ri, const u32* n_d, const u64* cw, const u32* cbase, const u32* cwl,
                      const u32* ncwl, u32 n_pad_c, u32* bad, u32 n_b, u32* nqc, u32* smap, u32 smap_stride, u64* mqc, size_t mqc_stride,
                      u32 rows_c, u64* rowany_c, u32 rowany_stride, u32* grp_any_c, u32 n_grp_c, u32 walk_scale = 1, const u64* hit = nullptr /* launch_cand_hit's, or NULL: every listed row is tested */);
// build, two passes over the tiled matrix (n_elems = n_tiles * s * 256): count (key / cnt zeroed: all-ones / 0; *overflow raised when
// the table is too small), then -- offsets from the counts, cursor zeroed -- fill
void launch_rare_count(hipStream_t st, const u64* mat, u64 n_elems, u64* key, u32* cnt, u32 mask, u32* overflow,
                       u64* spmask = nullptr /* [slots], zero on entry: bit sp = a genome of species sp holds the key */, const u32* grp_sp = nullptr, u32 s = 0);
void launch_rare_fill(hipStream_t st, const u64* mat, u64 n_elems, u32 s, const u64* key, const u32* off, u32* cursor, u32* post, u32 mask);
// a pass's dictionary split into the hashes the scan looks for (qd ascending, n_d[0] of them: rows [0, n_d[0]) of the bit matrix)
// and the others (n_d[1]; rows from n_d[2] on, sslot[2 i], [2 i + 1] = start and length of row i's genome list); qrow[position in q] = row.
// q_bound: host's upper bound of *n_q (sizes the grids); qinfo / qloc: [q_bound] scratch; bsum: [q_bound / 1024 + 1] scratch;
// h_words (page-locked, or NULL): [0] = *n_q, [1] = n_d[0]
void launch_classify(hipStream_t st, const u64* q, const u32* n_q, u32 q_bound, const RareIndex& ri, u32* qinfo, u32* qloc, u32* bsum,
                     u64* qd, u32* n_d, u32* qrow, u32* sslot, u32* h_words);
// bits of the rows behind the dense ones, from the genome lists: atomicOr into m_bits (and *m_dirty = 1)
// the rare rows straight into the group-major matrix (rows n_d[2] .. of Mq, their words of rowany, grp_any): references with bit rows
// for every list longer than 8 genomes (RareIndex::mlong) -- then M holds the dense rows only and launch_transpose_bits is given n_d + 2
// ext = {row stride, clean rows} of the buffer set's (Mq, rowany) pair (device; see rare_to_mq_kernel): read, then brought up to date
void launch_rare_to_mq(hipStream_t st, const u32* sslot, const u32* n_d, const RareIndex& ri, u64* mq, u32 nq_rows, u32 n_pad, u64* rowany,
                       u32* grp_any, u32 rows_bound, const u32* only_if, u32* ext);
u32 mq_any_stride();  // the stride value of arrays that were zeroed at allocation (clean under any stride)
void launch_sparse_fill(hipStream_t st, const u32* sslot, const u32* n_d, const RareIndex& ri, u64* m_bits, u32 n_pad, u32* m_dirty,
                        u32 rows_bound, const u32* only_if = nullptr /* device flag: run only when it is non-zero */);
// n_d = {dense rows, other rows, first other row (dense rows rounded up to 64), rows in all} -- what launch_classify leaves; for a
// reference without the index: everything dense, rows = positions in q
void launch_nd_from_nq(hipStream_t st, const u32* n_q, u32* n_d, u32* h_words);

// ---- the table without the ranking, and the candidates of a batch (skx_kernels.hip, "the table without the ranking")
static const u32 kPassBatchesMax = 8;          // batches of a pass (stream_coalesce)
static const u32 kCandCap = 1024;              // candidates per species the compact ranking takes (two rank groups)
static const u32 kCandRows = 131072;           // rows of a compact bit matrix (dense rows + the rare rows some candidate holds)
struct PassBatches { u32 n; u32 p_off[kPassBatchesMax + 1]; };  // pairs [p_off[b], p_off[b + 1]) of the pass's lists are batch b's
// every "zero on entry" below, for a whole deferred pass, in one launch: the ranges of pc (skx_pass_clear.hpp), the nqc counters' start
// values, the compact matrices up to the rows their last use dirtied (ext[], which launch_cand_publish writes)
static_assert(kClearSlotsMax == kPassBatchesMax, "one extent per batch slot");
void launch_pass_clear(hipStream_t st, const PassClear& pc);
u32 pass_counter_stride();  // u32 words between two per-batch counters (pass_counter_bytes() in all)
// cnt[b][row] (zero on entry; row_stride entries per batch) = occurrences of the row among batch b's pairs
void launch_pass_hist(hipStream_t st, const u32* pair_q, const PassBatches& pb, u32* cnt, u32 row_stride);
// gain[b][g] (zero on entry) += sum over rows of cnt[b][row] * (row's bit for g): dense rows from m_bits (BEFORE the transpose
// re-zeroes it), the others from the genome lists (ri / sslot, or NULL)
// gain_s (zero on entry, [n_b][n_pad] entries gain_sparse_stride() words apart): the rare rows' part
// op (or NULL): scratch for the counts as the int8 operand of the matrix product (gain_operand_kernel writes it, gain_dense_mfma_kernel
// reads it, both inside this call) -- frag: gain_operand_bytes(words_cap) bytes, 16-byte aligned; pairs: [words_cap].  Nothing of it
// is cleared or kept between calls.  Without it, with m_int, or with more than words_cap words of rows: the bit-by-bit kernel.
struct GainOperand { void* frag; u32* pairs; u32 words_cap; };
size_t gain_operand_bytes(u32 words_cap);
bool gain_dense_by_bits();  // experiments build, SKX_GAIN_MFMA=0: the bit-by-bit kernel for every call (A/B baseline)
void launch_gain_dense(hipStream_t st, const u64* m_bits, const u64* m_int /* or NULL */, u32 n_pad, const u32* n_d, u32 rows_bound, const u32* cnt,
                       u32 row_stride, u32 n_b, u32* gain, const u32* segw = nullptr /* [2 n_sp] word range of every species' rows (static dictionary) */,
                       const u32* grp_sp = nullptr, const GainOperand* op = nullptr);
// (lr: also lists the rows with a bit row per batch, nlrow zero on entry; walk_scale: multiplies the workgroups of the list walk --
// a pass with nothing beside it may fill the chip)
// (pr: the rows whose list is pattern + exceptions add to hist / gain_x and are listed for launch_cand_pat_map; hist, gain_x, nprow zero on entry)
void launch_gain_sparse(hipStream_t st, const u32* n_d, u32 rows_bound, const u32* cnt, u32 row_stride, u32 n_b, u32 n_pad, u32* gain_s,
                        const u32* sslot, const RareIndex& ri, const LongRows* lr, u32 walk_scale, const PatRows* pr = nullptr);
// pattern rows of the compact problems: nqc starts at n_pat rounded up to 64 (the mapped rows come behind the patterns' rows: PassClear::nqc_start);
// launch_cand_pat_rows: row n_d[2] + p of mqc[b] = pattern p at batch b's candidates, pcw[b][p][n_grp_c * 8] the same words;
// launch_cand_pat_map: smap of every listed pattern row -> its pattern's row, or a new row (pattern's words with the exceptions that are
// candidates flipped)
void launch_cand_pat_rows(hipStream_t st, const RareIndex& ri, const u32* n_d, const u32* candmask, const u32* candslot, u32 n_pad, u32* bad, u32 n_b,
                          u64* pcw, u64* mqc, size_t mqc_stride, u32 rows_c, u64* rowany_c, u32 rowany_stride, u32* grp_any_c, u32 n_grp_c);
void launch_cand_pat_map(hipStream_t st, const LongRows& lr, const PatRows& pr, const RareIndex& ri, const u32* n_d, const u32* candmask,
                         const u32* candslot, u32 n_pad, u32* bad, u32 n_b, u32* nqc, u32* smap, u32 smap_stride, const u64* pcw, u64* mqc,
                         size_t mqc_stride, u32 rows_c, u64* rowany_c, u32 rowany_stride, u32* grp_any_c, u32 n_grp_c, u32 rows_bound, u32 walk_scale = 1);
u32 gain_sparse_stride();
// tab[0] = prev, tab[b + 1] = tab[b] + gain[b]   ([n_b + 1][n_pad])
void launch_pass_tables(hipStream_t st, const u64* prev, const u32* gain, const u32* gain_s /* or NULL */, const u32* gain_l /* or NULL */, u32 n_b,
                        u32 n_pad, u64* tab);
// per (batch, species): the genomes whose value at the end of the batch reaches the top_k-th best value at its start, in reference
// order: cand[(b n_sp + sp) cap + i], candslot[b][g] (0xFFFFFFFF: none), tabc[b][sp cap + i] start values, ncand[b n_sp + sp],
// bad[b] (zero on entry) |= 1 when a species has more than cap
// candmask[g] (zero on entry) |= 1 << b for every candidate g of batch b
void launch_cand_select(hipStream_t st, const u64* tab, u32 n_pad, const Species& sp, u32 n_b, u32 top_k, u32 cap, u32* cand, u32* candslot,
                        u64* tabc, u32* ncand, u32* bad, u32* candmask);
// candidates a batch would have had (t0 / t1: the table before / after it): the largest count over the species -> h_out[0], seq -> h_out[1]
void launch_cand_count(hipStream_t st, const u64* t0, const u64* t1, const Species& sp, u32 top_k, u32* h_out, u32 seq);
// mc[b][w][c] = m_bits[w][cand[b][c]] (dense words; n_pad_c = n_sp * cap columns, words_c words per batch)
void launch_cand_gather_m(hipStream_t st, const u64* m_bits, const u64* m_int /* or NULL */, u32 n_pad, const u32* n_d, u32 rows_bound, const u32* cand,
                          u32 n_pad_c, const u32* bad, u32 n_b, u64* mc, u32 words_c);
// rare rows of the compact problems: rows behind the dense ones for the hashes some candidate holds (nqc[b] of them, smap[b][.]),
// their bits into mqc[b] / rowany_c[b] / grp_any_c[b] (all zero on entry); bad[b] |= 2 when they do not fit rows_c
void launch_cand_sparse(hipStream_t st, const u32* sslot, const u32* n_d, u32 rows_bound, const RareIndex& ri, const u32* candmask,
                        const u32* candslot, u32 n_pad, u32* bad, u32 n_b, u32* nqc, u32* smap, u32 smap_stride, u64* mqc, size_t mqc_stride,
                        u32 rows_c, u64* rowany_c, u32 rowany_stride, u32* grp_any_c, u32 n_grp_c, u32 walk_scale = 1);
// mode[b] = 1 compact / 0 everything, *any_full, nqc_total[b] = rows of the compact problem; h_pub (page-locked): [b] mode,
// [8 + b] largest candidate count, [16] any_full, [18] = n_b, [17] = seq (written last)
void launch_cand_publish(hipStream_t st, const u32* bad, u32 force_full, const u32* ncand, const u32* nqc, const u32* n_d, u32 n_b, u32 n_sp,
                         u32 rows_c, u32* mode, u32* any_full, u32* nqc_total, u32* h_pub, u32 seq,
                         u32* ext = nullptr /* [n_b] rows of mqc[b] this pass dirtied (passes that filled the compact matrices) */);
void launch_m_clear(hipStream_t st, u64* m_bits, u64* m_int /* or NULL */, u32 n_pad, const u32* n_d, const u32* any_full);
void launch_cand_pair_rows(hipStream_t st, const u32* pair_q, u32 n_pairs, const u32* n_d, const u32* smap, u32 rows_c, u32* pair_qc);
void launch_cand_rows_back(hipStream_t st, u32* out_idx, u32 n_reads, u32 n_sp, u32 top_k, const u32* cand, u32 cap, const u32* g0);
// consensus genotypes of finished index rows: out[row][sp][f] = the code most of codes[g0[sp] + idx[row][sp][j]][f], j < top_k, carry;
// ties go to the smallest code.  Rows [first_row, first_row + n_rows) of idx [.][n_sp][top_k] and out [.][n_sp][n_feat];
// codes [n_code_rows][n_feat] (table rows past the end are clamped to it); 1 <= top_k <= kConsensusTopMax.
// One thread per output value; more than 2^31 of them go out as several launches.
constexpr u32 kConsensusTopMax = 64;
void launch_consensus_rows(hipStream_t st, const u32* idx, u64 first_row, u64 n_rows, u32 n_sp, u32 top_k, const u32* g0, const u32* codes,
                           u32 n_feat, u32* out, u32 n_code_rows);
// Change points of finished rows (skx_stream_bind_changes, skx_changes_rows): rows [.][width] u32, 1 <= width <= kChangeWidthMax.
//   flags   flag[r] = (r == 0) || rows[r] != rows[r - 1] for r in [ra, rb): one u32 per row, written by exactly one lane, so launches over
//           disjoint [ra, rb) of one batch share nothing.  Row ra - 1 (ra > 0) must be complete in the stream's order.
//   events  behind the flags of ALL n rows: an exclusive scan of the flags (pos, launch_count_scan's two kernels; bsum: one word per 1024
//           rows), then every flagged row r with pos[r] < cap writes ev_read[pos] = r and copies its rows of idx (w_idx u32), sum (w_idx
//           u64) and codes (w_codes u32) to entry pos of the optional ev_* arrays; *n_events = number of flags (not capped).  Entries from
//           min(n_events, cap) on are not touched.  n >= 1.
constexpr u32 kChangeWidthMax = 4096;
void launch_change_flags(hipStream_t st, const u32* rows, u32 width, u32 ra, u32 rb, u32* flag);
void launch_change_events(hipStream_t st, const u32* flag, u32* pos, u32* bsum, u32 n, u32 cap, u32* n_events, u32* ev_read,
                          const u32* idx, const u64* sum, u32 w_idx, u32* ev_idx, u64* ev_sum, const u32* codes, u32 w_codes, u32* ev_codes);
// Species call of finished rows (skx_stream_bind_call, skx_stream_bind_call_changes, skx_call_rows): for the rows r in [ra, rb) of
// idx / sum [.][n_sp][top_k] (and codes [.][n_sp][n_feat] or NULL) the species c(r) = lowest sp with the largest sum[r][sp][0], to
// call_sp[r], and -- each optional -- that species' rows compact: call_idx / call_sum [.][top_k], call_codes [.][n_feat],
// key [.][1 + (key_codes ? n_feat : top_k)] = {c(r), index row | codes}, the rows launch_change_flags compares.  Plain loads and stores,
// one writer per element, launches over disjoint [ra, rb) share nothing.  n_sp, top_k >= 1.
void launch_species_call(hipStream_t st, const u32* idx, const u64* sum, const u32* codes, u32 ra, u32 rb, u32 n_sp, u32 top_k, u32 n_feat,
                         u32* call_sp, u32* call_idx, u64* call_sum, u32* call_codes, u32* key, bool key_codes);
// behind launch_change_events over the key: ev_sp[pos[r]] = call_sp[r] for every flagged r < n with pos[r] < cap
void launch_call_species_gather(hipStream_t st, const u32* flag, const u32* pos, u32 n, u32 cap, const u32* call_sp, u32* ev_sp);

// dictionary
// qrow (launch_classify) != NULL: pair_q receives ROWS of the bit matrix instead of positions in q
void launch_pair_q(hipStream_t st, const u64* pair_h, u32 n_pairs, const u64* q, const u32* n_q, u32* pair_q, const u32* qrow /* or NULL */,
                   const u32* bbase, const u32* btot, u64 max_ref /* launch_dict_rest's, of the same pass */);
// Dictionary of a pass, in two steps.  (1) launch_dict_insert gathers the pairs of reads [r_begin, r_end) (pair_h, pair_r)
// and inserts every pair hash into the hash set -- one wave per read, no knowledge of the pair count needed: it can be
// queued right behind the sketcher; if the reads have more than pair_cap pairs it does nothing.  (2) launch_dict_rest
// turns the set into q / n_q, the sorted distinct dictionary, and empties it.
// ht: hash set of ht_slots (power of two, >= 2 x pairs) u64, all-ones between passes; slot_off: [ht_slots] scratch;
// bcount: [dict_buckets()] zero between passes; bbase: [dict_buckets()]; btot: [129]; ctr: [4] zero between passes
// (ctr[1]: the all-ones hash was seen, ctr[2]: distinct keys inserted so far)
// base: device words whose sum is the number of pairs already in the lists (a batch sharing the pass of the batches before it:
// their pair counts are only known on the device when this is queued)
static const int kPairBaseMax = 7;
struct PairBase { const u32* p[kPairBaseMax] = {}; };
void launch_dict_insert(hipStream_t st, const u64* sk, u32 sk_stride, const u32* poff, u32 r_begin, u32 r_end, u32 p_base,
                        u64* pair_h, u32* pair_r, u64* ht, u32 ht_slots, u32* ctr, u32 pair_cap,
                        const u32* row_off = nullptr /* sk_stride == 0: row r starts at sk + row_off[r] */,
                        PairBase base = PairBase());
void launch_dict_rest(hipStream_t st, u64* ht, u32 ht_slots, u64 max_ref, u32* slot_off, u32* bcount, u32* bbase, u32* btot,
                      u32* ctr, u64* q, u32* n_q);
u32 dict_buckets();
void launch_window(hipStream_t st, const u64* lo, const u64* hi, u32 n_bt, const u64* q, const u32* n_q, u32* win,
                   u32* h_nq /* page-locked host word that receives *n_q, or NULL */);
void launch_exceptions(hipStream_t st, const u32* exc_g, const u64* exc_h, u32 n_exc, const u64* q, const u32* n_q,
                       u64* m_bits, u32 n_pad, u32* m_dirty /* raised when a bit was set, or NULL */, const u32* qrow = nullptr,
                       u32 row0 = 0 /* q[0]'s row */, u32 n_fixed = 0 /* n_q == NULL: entries of q */);

// scan + transpose
// lean: scan_lean_kernel (sparse dictionaries: every production pass) -- every (band, tile) block ORs the words of its slice into
// m_bits when its band is done (one coalesced atomicOr per non-zero word) and raises *m_dirty; !lean: scan_kernel variants into
// m_bits / m_int.  Experiments build only: hbuf != NULL with into_m == false = round 3's slab form (every block stores its words
// into its own slab hbuf[(band * n_tiles + tile) * scan_lean_words() * 256 ...]; scan_lean_wants_slabs() says whether a knob asks
// for it, and the stream then allocates the slabs).
bool scan_lean_applies(u32 n_bands, bool split, bool big_table);
u32 scan_lean_words();
bool scan_lean_wants_slabs();
bool scan_lean_into_m();
// (experiments build: the profiling aid SKX_SCAN_ABLATE is set -- the scan of the static dense dictionary then takes the ablated kernels
// too, like a per-pass dictionary's; the product library: false)
bool scan_ablated();
// run > 0: scan_run_kernel -- one workgroup per `run` consecutive bands of a tile, results OR-ed into m_bits (no slabs, no hbuf);
// windows of up to scan_run_cap() entries in one pass over the rows
u32 scan_run_cap();
void launch_scan(hipStream_t st, const u64* mat, u32 s, u32 n_tiles, u32 rb, u32 n_bands, const u64* q, const u32* win,
                 u64* m_bits, u64* m_int, u32 n_pad, bool big_table, bool lean, u64* hbuf, u32* m_dirty, bool into_m = true, u32 run = 0, bool big_slices = false);
u32 scan_lean_cap(bool big);  // entries of a (band, tile) slice the lean kernel's one-pass probe holds (big: the instance for passes with large slices)
// wb[w * n_tiles + t] = (first | last << 16) band of tile t whose slice can reach query word w (first > last: none)
// lo != NULL: also computes the windows (launch_window's work) first: one launch instead of two in front of the scan
void launch_word_bands(hipStream_t st, u32* win, u32 n_tiles, u32 n_bands, const u32* n_q, u32* wb, const u64* lo = nullptr,
                       const u64* hi = nullptr, const u64* q = nullptr, u32* h_nq = nullptr);
// also re-zeroes m_bits / m_int; words beyond *n_q are skipped; grp_any[rank group] (zero on entry) receives the number of
// query rows that hold a bit for some genome of the group -- the ranking kernels skip groups with none (grp_any arguments
// below) and compact the pairs of groups with few (rowany)
// hbuf != NULL: also ORs the lean kernel's slabs in (wb from launch_word_bands, win = the windows) and reads m_bits only
// when *m_dirty != 0
void launch_transpose_bits(hipStream_t st, u64* m_bits, u64* m_int, u32 n_pad, u32 n_words, u64* mq,
                           const u32* n_q, u32* grp_any, const u64* hbuf, const u32* wb, const u32* win, u32 n_tiles,
                           const u32* m_dirty, u64 nq_est /* the host's estimate of the dictionary size: sizes the grid */,
                           u64* rowany /* [rank groups][n_words]: bit r of word w = row 64 w + r holds a bit in the group; or NULL */,
                           const u32* only_if = nullptr /* device flag: run only when it is non-zero */,
                           bool keep_m = false /* do NOT re-zero m_bits (static dense rows kept for later passes: policy reuse_membership) */);
// chk[0..5], [9] (zero on entry): non-monotonic marker, long-read count, offsets[0], offsets[n_reads], segment count;
// long_reads != NULL: also lists the batch's long reads and their segments (chk[6] |= 2 if they do not fit the tables)
void launch_batch_check(hipStream_t st, const u64* offsets, u32 n_reads, u64 n_bases, u32* chk, u32* cnt_tail /* zeroed */,
                        const LongReads* long_reads);
// h_pub (page-locked host memory, 16 words): [0..7] = chk (then zeroed, as is retry[0]), [8] = *total_pairs, [15] = seq last
// ([7] = number of reads the block sketcher took; `big` is re-armed like `retry`)
// [10] = distinct keys in the hash set dict_ctr belongs to (the speculative gather's |Q|; 0xFFFFFFFF without dict_ctr)
// n <= 64 words, device memory -> page-locked (coherent) host memory, written by a kernel: never blocks the queueing thread
// (reads AND zeroes d_src: a counter block that is published once per use needs no memset of its own)
void launch_store_host_words(hipStream_t st, u32* h_dst, u32* d_src, u32 n);
void launch_publish(hipStream_t st, u32* chk, u32* retry, u32* big, const u32* total_pairs, u32* h_pub, u32 seq,
                    const u32* dict_ctr /* counters of the set the speculative gather filled, or NULL */);
// membership filter over the union of the reference hashes (blocked Bloom filter, skx_common.hpp: filter_mask / filter_hit);
// count != NULL: `words` is a plain bitmap over v >> shift instead and *count receives the bits newly set (distinct values)
void launch_filter_build(hipStream_t st, const u64* vals, u64 n, u32 shift, u64* words, bool markers_are_values,
                         unsigned long long* count = nullptr);
void launch_filter_apply(hipStream_t st, u64* sk, u32 sk_stride, u32* cnt, u32 n_reads, const u64* bits, u32 shift);

// ranking
void launch_seg_sum(hipStream_t st, const u32* pair_q, const u32* poff, u32 p_base, u32 r_begin, u32 n_reads,
                    u32 seg_len, const u64* mq, u32 n_pad, u32 nq_rows, u32* inc, const u32* grp_any,
                    u32* csum_raw /* [ceil(n_seg / 16)][n_pad] chunk sums, zero on entry; NULL: not wanted */,
                    const u64* rowany /* of launch_transpose_bits, or NULL */, const u32* n_q, const Species& sp,
                    const u64* gmax = nullptr /* != NULL: only the (chunk, rank group)s that can hold a candidate (launch_seg_prefix part 1) */,
                    const u64* lead_val = nullptr);
// the chunk sums alone (csum_raw zero on entry): a workgroup per (rank group, chunk), one extraction per quarter chunk
void launch_chunk_sum(hipStream_t st, const u32* pair_q, const u32* poff, u32 p_base, u32 r_begin, u32 n_reads,
                      const u64* mq, u32 n_pad, u32 nq_rows, const u32* grp_any, u32* csum_raw, const u64* rowany, const u32* n_q,
                      const Species& sp);
// prune_top_k > 0 (1..rank_topk_fast_max()): also find the first prune_top_k genomes as each chunk of 16 segments begins
// (leader [n_chunks * k], lead_val [n_chunks]) and every half rank group's best value per chunk boundary (gmax
// [(n_chunks + 1) * n_pad / 256]); start values are then only written for (chunk, group)s that can hold a candidate.
// part: 0 = everything; 1 = what needs only the chunk sums; 2 = what needs the per-segment increments (after part 1)
void launch_seg_prefix(hipStream_t st, const u32* inc, u32 n_seg, u32 n_pad, const Species& sp, const u64* cum_in, u64* cum_out,
                       u32* rel /* [n_seg][n_pad]: segment start values minus cum_in */, u32* csum, u32* csum_raw, u32 prune_top_k,
                       u32* leader /* [n_chunks * n_sp * k] */, u64* lead_val /* [n_chunks * n_sp] */, u64* gmax,
                       u64* part_sum, u32* part_idx /* [n_chunks * n_sp * rank_leader_parts() * k] scratch */,
                       const u32* grp_any, unsigned char* live /* [n_seg][n_pad / 64], pruned rankings only; else NULL */,
                       u64* lead_seg /* [n_seg][n_sp] scratch */, int part = 0,
                       u32* live_ctr = nullptr /* [2], pruned rankings: += (chunk, half group)s that can hold a candidate / tested (a sample) */,
                       hipEvent_t ev_table = nullptr /* recorded right behind chunk_prefix: cum_out is complete (parts 0 and 1) */);
u32 rank_leader_parts();
void launch_rank_seg(hipStream_t st, const u32* pair_q, const u32* pair_r, const u32* poff, u32 p_base, u32 r_begin,
                     u32 n_reads, u32 seg_len, const u64* mq, u32 n_pad, u32 nq_rows, const Species& sp, const u64* cum_in,
                     const u32* rel, u32 top_k, u64* cand_sum, u32* cand_idx, const u32* grp_any);
void launch_rank_seg_top1(hipStream_t st, const u32* pair_q, const u32* pair_r, const u32* poff, u32 p_base, u32 r_begin,
                          u32 n_reads, const u64* mq, u32 n_pad, u32 nq_rows, const Species& sp, const u64* cum_in,
                          const u32* rel, u64* best_sum, u32* best_idx, const u32* inc, const u32* leader, const u64* gmax,
                          const u64* lead_val, const u32* grp_any, const unsigned char* live, unsigned char* has,
                          const u64* rowany /* of launch_transpose_bits, or NULL */, const u32* n_q);
// 2 <= top_k <= rank_topk_fast_max(): pruned, one wave per (rank group, segment);
// cand_sum / cand_idx[(r * n_grp + grp) * top_k + j]
void launch_rank_seg_topk(hipStream_t st, const u32* pair_q, const u32* pair_r, const u32* poff, u32 p_base, u32 r_begin,
                          u32 n_reads, const u64* mq, u32 n_pad, u32 nq_rows, const Species& sp, const u64* cum_in,
                          const u32* rel, u32 top_k, u64* cand_sum, u32* cand_idx, const u32* inc, const u32* leader,
                          const u64* gmax, const u64* lead_val, const u32* grp_any, const unsigned char* live, unsigned char* has);
u32 rank_topk_fast_max();
// rows come out per (read, species) with genome indices local to the species: out[((out_r0 + r) * n_sp + sp) * top_k + j]
void launch_top1_merge(hipStream_t st, const u64* best_sum, const u32* best_idx, u32 n_reads, u32* out_idx, u64* out_sum,
                       u32 out_r0, const Species& sp, const unsigned char* has, u32 n_grp);
// n_units candidates-units per read (rank groups: per_grp = 1; genome words: per_grp = kRankWords)
void launch_topk_merge(hipStream_t st, const u64* cand_sum, const u32* cand_idx, u32 n_reads, u32 n_units, u32 per_grp,
                       u32 top_k, u32* out_idx, u64* out_sum, u32 out_r0, const Species& sp, const unsigned char* has /* [segments][rank groups] of the pruned kernels, or NULL */);
void launch_rank_table(hipStream_t st, const u64* cum, const Species& sp, u32 top_k, u32* out_idx /* [n_sp][top_k] */, u64* out_sum);
// n_real real genomes (species concatenated); real2pad[g] = padded index
void launch_shared_debug(hipStream_t st, const u32* pair_q, const u32* poff, u32 p_base, u32 r_begin, u32 n_reads,
                         const u64* mq, u32 nq_rows, u32 n_real, const u32* real2pad, u32* shared, u32 out_r0);
// per (row, species) the first top_k of (count desc, index asc) over the species' real genomes of cnt[n_rows][n_pad] (padded counts:
// launch_seg_sum with seg_len = 1); bound >= every count; top_idx / top_val [n_rows][n_sp][top_k], indices local to the species;
// 1 <= top_k <= min(kRowTopkMax, smallest species)
constexpr u32 kRowTopkMax = 64;
void launch_row_topk(hipStream_t st, const u32* cnt, u32 n_rows, u32 n_pad, const Species& sp, u32 top_k, u32 bound, u32* top_idx, u32* top_val);
// the same for rows ranked in ONE species with one genome each left out (skx_ref_neighbours): row r = the first top_k genomes of `species`
// other than excl0 + r; top_idx / top_val [n_rows][top_k]; 1 <= top_k <= min(kRowTopkMax, genomes of the species - 1)
void launch_row_topk_excl(hipStream_t st, const u32* cnt, u32 n_rows, u32 n_pad, const Species& sp, u32 species, u32 excl0, u32 top_k, u32 bound,
                          u32* top_idx, u32* top_val);
// genomes [p0, p0 + cnt) (padded indices) of the resident matrix [n_tiles][s][256] as query rows [cnt][row_stride] (row_stride >= s):
// ascending, zero-padded, the genome's lifted hashes (exc_g ascending, a genome's hashes descending) appended in ascending order;
// len [cnt] = entries of each row.  Two launches on st.
void launch_ref_rows(hipStream_t st, const u64* mat, u32 s, u32 p0, u32 cnt, const u32* exc_g, const u64* exc_h, u32 n_exc, u64* rows,
                     u32 row_stride, u32* len);
// out[n_rows][n_real] = cnt[row][real2pad[g]]
void launch_unpad_rows(hipStream_t st, const u32* cnt, u32 n_rows, u32 n_pad, u32 n_real, const u32* real2pad, u32* out);
void launch_add_table(hipStream_t st, u64* cum, const u64* add, u32 n_real, const u32* real2pad);
void launch_gather_table(hipStream_t st, const u64* cum, u64* out, u32 n_real, const u32* real2pad);
// ---- breadth of a stream (skx_kernels.hip, "breadth of a stream").  seen: one bit per key-table slot + two for the lifted hashes,
// (kt_slots + 2 + 31) / 32 words.  launch_seen_mark: behind launch_classify of the same pass, same stream (q, n_q, q_bound, qinfo: its).
void launch_seen_mark(hipStream_t st, const u64* q, const u32* n_q, u32 q_bound, const u32* qinfo, u32* seen, u32 kt_slots);
// covered[p] += seen hashes of padded genome p, for the genomes of the aligned 64-genome groups groups[0 .. n_groups) (NULL: groups
// 0 .. n_groups - 1, the whole table); covered [n_pad], zero on entry for those genomes
void launch_coverage_walk(hipStream_t st, const u64* mat, u32 s, const u32* groups, u32 n_groups, const u64* key, u32 mask, const u32* seen,
                          const u32* exc_g, const u64* exc_h, u32 n_exc, u32* covered);
// out_x[i] = x[real2pad[genomes ? genomes[i] : i]], i < n, for the per-genome results of the breadth and depth walks; an output that is
// NULL is not wanted.  wide[p] = covered[p], p < n_pad (for launch_rank_table)
void launch_genome_gather(hipStream_t st, const u32* covered, const u32* median, const u64* total, const u32* real2pad, const u32* genomes,
                          u32 n, u32* out_cov, u32* out_med, u64* out_tot);
void launch_coverage_widen(hipStream_t st, const u32* covered, u32 n_pad, u64* wide);
// ---- winner-takes-all breadth (skx_kernels.hip, "Winner-takes-all breadth").  rank [n_pad]: a padded genome's position in the global
// order (skx_winner_order.hpp), 0xFFFFFFFF for padding genomes; win: one u32 per bit of `seen`, same indices.
// launch_winner_mark: the whole table (groups 0 .. n_groups - 1); win all-ones on entry, afterwards the lowest rank among the holders of
// every seen hash.  launch_winner_count, behind it on the same stream: won[p] += seen hashes of padded genome p with win == rank[p], for
// the genomes of groups[0 .. n_groups) (NULL: the whole table); won [n_pad], zero on entry for those genomes
void launch_winner_mark(hipStream_t st, const u64* mat, u32 s, u32 n_groups, const u64* key, u32 mask, const u32* seen, const u32* exc_g,
                        const u64* exc_h, u32 n_exc, const u32* rank, u32* win);
void launch_winner_count(hipStream_t st, const u64* mat, u32 s, const u32* groups, u32 n_groups, const u64* key, u32 mask, const u32* seen,
                         const u32* exc_g, const u64* exc_h, u32 n_exc, const u32* rank, const u32* win, u32* won);
// ---- depth of a stream (skx_kernels.hip, "depth of a stream").  depth: one u32 per bit of `seen`, same indices, saturating.
// launch_depth_mark: behind launch_pair_q of the same pass, same stream (pair_h, q, n_q, bbase, btot: its; qinfo: its launch_classify's);
// tmp [>= q_bound] is zero on entry and zero again afterwards.
void launch_depth_mark(hipStream_t st, const u64* pair_h, u32 n_pairs, const u64* q, const u32* n_q, u32 q_bound, const u32* qinfo,
                       const u32* bbase, const u32* btot, u64 max_ref, u32* tmp, u32* depth, u32 kt_slots);
// per padded genome of the groups groups[0 .. n_groups) (NULL: groups g0 .. g0 + n_groups - 1): covered += counters > 0, total += their sum,
// vmax = their maximum (all three zero on entry), median = the lower median of the counters > 0; vals: scratch of depth_vals_per_group(s)
// u32 per group of the launch
inline size_t depth_vals_per_group(u32 s) { return ((size_t)s + 2u) * 64u; }
void launch_depth_walk(hipStream_t st, const u64* mat, u32 s, const u32* groups, u32 g0, u32 n_groups, const u64* key, u32 mask,
                       const u32* depth, const u32* exc_g, const u64* exc_h, u32 n_exc, u32* covered, u64* total, u32* vmax, u32* median,
                       u32* vals);
// *n += indices with a counter > 0 (zero on entry); hashes / counts [cap] take the first cap of them (hashes == NULL: count only)
void launch_depth_export(hipStream_t st, const u64* key, const u32* depth, u64 kt_slots, u64* hashes, u32* counts, u64 cap,
                         unsigned long long* n);
// depth[hash's index] = sat(+ counts[i]), its seen bit set where counts[i] > 0; *n_unknown += entries that are no key (zero on entry)
void launch_depth_import(hipStream_t st, const u64* hashes, const u32* counts, u64 n, const u64* key, u32 mask, u32* depth, u32* seen,
                         unsigned long long* n_unknown);
// ---- composition of a stream (skx_kernels.hip, "composition of a stream").  spmask: one u64 per key-table slot, bit sp = some genome of
// species sp holds the key; zero on entry of launch_species_mask, which walks the whole table (groups 0 .. n_groups - 1).
void launch_species_mask(hipStream_t st, const u64* mat, u32 s, u32 n_groups, const u64* key, u32 mask, Species sp, u64* spmask);
// behind launch_pair_q of the same pass, same stream (inputs as launch_depth_mark's): qmask [>= q_bound] = the species mask of every distinct
// hash of the pass (spmask == NULL: one species, a found slot has mask 1) ...
void launch_comp_qmask(hipStream_t st, const u64* q, const u32* n_q, u32 q_bound, const u32* qinfo, const u64* spmask, u32 kt_slots,
                       u64* qmask);
// ... and, per batch of the pass (pair_h: its part of the pass's pair hashes; read i < n_reads has the pairs [poff[i] - p_base,
// poff[i + 1] - p_base) of it): reads [n_sp + 2] += its reads per class, pairs [n_sp] += their hits per species.  comp_count_prepare:
// once per device before the first launch with that many species (above 31 the kernel has to ask for its LDS)
hipError_t comp_count_prepare(u32 n_sp);
void launch_comp_count(hipStream_t st, const u64* pair_h, const u32* poff, u32 p_base, u32 n_reads, const u64* q, const u32* n_q,
                             u32 q_bound, const u32* bbase, const u32* btot, u64 max_ref, const u64* qmask, u32 n_sp, u32 min_hits, u64* reads,
                             u64* pairs);
void launch_comp_add(hipStream_t st, u64* ctr, u32 n);  // *ctr += n

// ---- pooled sketches (skx_kernels.hip, "pooled sketches"): the bottom-s distinct hashes of the union of a group's rows
// One round of the segmented merge tree: items[i] = {left row, partner row or 0xFFFFFFFF (no partner: the row is copied)}; rows are
// `stride` entries apart in src / dst (two buffers of the same geometry), lengths in src_len / dst_len; dst row `left` receives at
// most s values and may extend over the slots of the rows of its subtree.
void launch_pool_merge_round(hipStream_t st, const uint2* items, u32 n_items, const u64* src, const u32* src_len, u64* dst, u32* dst_len,
                             u32 stride, u32 s);
// dst[0 .. *dst_len) = first s distinct values of a[0 .. *na) U b[0 .. *nb) (ascending rows, device lengths)
void launch_pool_merge_one(hipStream_t st, const u64* a, const u32* na, const u64* b, const u32* nb, u64* dst, u32* dst_len, u32 s);
// out[g][s] (zero-padded), out_len[g] for n_groups groups: desc[g] = {first row, rows} -- the pooled row of a group of `rows` rows sits
// at its first row in buffer (ceil(log2(rows)) & 1); rows = 0: empty group; first row = 0xFFFFFFFF: the row is acc[0 .. *acc_len)
void launch_pool_gather(hipStream_t st, const uint2* desc, u32 n_groups, const u64* buf0, const u64* buf1, const u32* len0, const u32* len1,
                        u32 stride, const u64* acc, const u32* acc_len, u64* out, u32* out_len, u32 s);
// valid[r] = windows of k retained bases of record r that are all A/C/G/T/U (the sketchers' normalisation), duplicates counted
void launch_pool_valid_kmers(hipStream_t st, const uint8_t* bases, const u64* offsets, u32 n_records, u32 k, u64* valid);
// out[i] = sum of v[seg[i].x .. seg[i].x + seg[i].y)
void launch_pool_seg_sum(hipStream_t st, const u64* v, const uint2* seg, u32 n_seg, u64* out);
// k-mer abundance counts (skx_sketch_groups_counts).  seg[i] = {first row, rows, offset of the segment's counters in `counts` (low,
// high word)}: the segments tile the slice's n_records records in order; a segment's root row sits where launch_pool_gather finds
// it and its counters (zero on entry, min(s, stride * rows) of them) receive, per position of the root row, the valid k-mer
// windows of the segment's records whose canonical hash is that value.  offsets[0] = 0, offsets[n_records] = n_bases <= 2^32 - 1.
void launch_pool_count(hipStream_t st, const uint8_t* bases, const u64* offsets, u32 n_records, u64 n_bases, u32 k, u64 seed, const uint4* seg,
                       u32 n_seg, const u64* buf0, const u64* buf1, const u32* len0, const u32* len1, u32 stride, u32 s, u32* counts);
// launch_pool_merge_one with counts: the counts of a value both rows hold are added (saturating), the cut at s drops counts too
void launch_pool_merge_one_counted(hipStream_t st, const u64* a, const u32* ca, const u32* na, const u64* b, const u32* cb, const u32* nb, u64* dst,
                                   u32* dst_cnt, u32* dst_len, u32 s);
// launch_pool_gather + out_cnt[g][s] (zero-padded): desc[g] = {first row, rows, offset of the row's counters (low, high word)}
void launch_pool_gather_counted(hipStream_t st, const uint4* desc, u32 n_groups, const u64* buf0, const u64* buf1, const u32* len0, const u32* len1,
                                u32 stride, const u32* counts, const u64* acc, const u32* acc_cnt, const u32* acc_len, u64* out, u32* out_cnt,
                                u32* out_len, u32 s);

}  // namespace skx
