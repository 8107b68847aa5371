/*
 * sketchy_hip.h -- C ABI of libsketchy_hip.so: the MI355X (gfx950) implementation of
 * sketchy's streaming read-vs-reference MinHash path.
 *
 * The reference (esteinig/sketchy v0.6.0) has no FFI/plugin interface; it is one Rust
 * binary.  The boundary below sits exactly at the seam its hot loop uses internally
 * (paths are under the reference tree):
 *
 *   skx_ref_create         <- the in-RAM reference collection `Vec<Sketch>` returned by
 *                             Sketchy::_read_sketch (src/sketchy.rs:497-536) and consumed at
 *                             :337-339; k / seed / s are the sketch params of :82, :520-527
 *   skx_stream_create      <- state of Sketchy::_sum_of_shared_hashes (src/sketchy.rs:326-327):
 *                             `sum_of_shared_hashes: Vec<u64>` + read counter; `top` is
 *                             PredictConfig::top (src/sketchy.rs:43-50)
 *   skx_stream_push        <- one or more iterations of the loop body src/sketchy.rs:328-354:
 *                             create_sketcher/process/to_vec (:331-335, finch MashSketcher),
 *                             N x _common_hashes (:337-341, :419-459), stable sort (:348),
 *                             first `top` rows (:391)
 *   skx_stream_table[_add] <- read / seed `sum_of_shared_hashes` (:326, :341)
 *   skx_common_hashes      <- Sketchy::_common_hashes (src/sketchy.rs:419-459) for sketch
 *                             collections (the `shared` all-pairs use at :251-261)
 *   skx_rank_sketches      <- the tail of Sketchy::_shared_hashes (src/sketchy.rs:304-312): shared hashes against every
 *                             genome, stable sort, first `top` rows -- for many pooled sketches in one call
 *   skx_ref_neighbours     <- no counterpart: the same tail for every genome of the resident reference against the others of its species
 *   skx_predict_groups     <- all of Sketchy::_shared_hashes (src/sketchy.rs:281-315) for many samples: pool, count, rank
 *   skx_stream_bind_changes / skx_changes_rows <- no counterpart: the reference prints every read's rows (:348-349, :391-399); these
 *                             report only the reads at which what it would print (indices or consensus) differs from the read before
 *   skx_stream_bind_call / skx_stream_bind_call_changes / skx_call_rows <- no counterpart: the reference ranks against one file; these
 *                             say which of the resident species the sample is after every read, with that species' rows alone
 *   skx_stream_enable_coverage / skx_stream_coverage[_rows|_rank] <- no counterpart: the reference keeps sums only; these say how many of
 *                             a genome's own sketch hashes the reads have shared at least once (containment, as `mash screen` reports it)
 *   skx_stream_winners[_rows|_rank] <- no counterpart: the breadth with every seen hash credited to ONE genome, the best of its
 *                             holders (`mash screen -w`): a clone tree's thousands of copies of one lineage stop outranking a second strain
 *   skx_stream_enable_depth / skx_stream_depth[_rows|_count|_export|_import] <- no counterpart: how OFTEN each of a genome's hashes was
 *                             shared (the median multiplicity of `mash screen`), and the counters as portable (hash, count) pairs
 *   skx_stream_enable_composition / skx_stream_composition <- no counterpart: reads per resident species, ambiguous and unclassified,
 *                             each read classified by its own sketch's hits per species
 *   skx_sketch_reads       <- finch SketchScheme::{process,to_vec} as called at :331-335
 *   skx_sketch_groups      <- finch SketchScheme::{process x many, to_vec}: ONE sketcher fed several records -- all reads of an
 *                             offline `predict` (src/sketchy.rs:291-302), all contigs of a genome file in `sketch` (:473-478)
 *   skx_sketch_groups_counts <- the same + KmerCount.count of every sketch hash (:302, :480-488): Mash's counts32
 *
 * Conventions: every function returns 0 (SKX_OK) or a negative SKX_ERR_* code and never
 * throws; skx_last_error() returns a thread-local message for the last failure.  Handles
 * are opaque and owned by the library.  Host buffers are caller-owned and only borrowed for
 * the duration of the call.  A stream handle is driven by one host thread at a time (the
 * reference loop is single-threaded); different handles may be used from different threads.
 * There is NO CPU fallback: with no usable gfx950 device every entry point that needs one
 * fails with SKX_ERR_NO_DEVICE.
 */
#ifndef SKETCHY_HIP_H
#define SKETCHY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKX_OK 0
#define SKX_ERR_INVALID (-1)      /* bad argument (NULL, k out of range, top > n_genomes ...) */
#define SKX_ERR_NO_DEVICE (-2)    /* no HIP device / device index out of range */
#define SKX_ERR_HIP (-3)          /* a HIP runtime call failed; see skx_last_error() */
#define SKX_ERR_UNSORTED (-4)     /* a reference column is not strictly ascending */
#define SKX_ERR_CAPACITY (-5)     /* batch exceeds the capacity given at skx_stream_create */
#define SKX_ERR_COMM (-6)         /* RCCL failure */
#define SKX_ERR_UNSUPPORTED (-7)  /* parameter combination outside what the kernels support */

#define SKX_MAX_K 32u             /* k-mer length 1..32 (sketchy default 16, src/cli.rs:39-41) */
#define SKX_MAX_TOP 64u           /* rows ranked per read (sketchy default 1, src/cli.rs:118-119) */
#define SKX_MAX_SPECIES 64u       /* reference collections resident together in one skx_ref */
#define SKX_MAX_FEATURES 64u      /* genotype columns of a reference's genotype table (skx_ref_set_genotypes) */
/* largest entry skx_stream_table_add leaves in the running table (see there): 2^54 - 1 */
#define SKX_MAX_TABLE_SUM ((1ull << 54) - 1)

typedef struct skx_ref skx_ref;
typedef struct skx_stream skx_stream;
typedef struct skx_comm skx_comm;

/* ---- library / device ------------------------------------------------------------- */
const char *skx_last_error(void);
const char *skx_version(void);
int skx_device_count(void);
/* name (<= name_cap bytes), number of CUs and bytes of device memory of `device` */
int skx_device_info(int device, char *name, size_t name_cap, int *compute_units, uint64_t *total_mem);
/* PCI address of `device` as "domain:bus:device.function" (>= 13 bytes): what a host that feeds the device from page-locked
 * memory looks up under /sys/bus/pci/devices/<id>/ (numa_node, local_cpulist) to keep its threads on the device's NUMA node */
int skx_device_pci_bus_id(int device, char *bus_id, size_t cap);

/*
 * Process-wide policies, consulted when a reference or a stream is CREATED (no effect on existing handles, never on
 * results -- only on memory and speed).  Names:
 *   "kmer_prefilter"  0 off (default) / 1 on / 2 on when its table fits 32 KB: for k = 16, skx_ref_create also builds a Bloom
 *                     table over the canonical 16-mers whose hash can meet the reference (every 4^16 / 2 of them is hashed
 *                     once, ~10 ms on an MI355X; 8 table bits per key); the production sketcher then hashes only the windows
 *                     of a read that pass it (reads with at most s windows -- longer ones can be truncated and take the plain
 *                     loop).  Rows, tables and debug outputs are identical either way.  One gather per window: it pays only
 *                     while the table sits in the L1 caches (a 16 KB table: +10 % reads/s; 128 KB: -10 %; 8 MB: -50 %), i.e.
 *                     for references with a few thousand distinct hashes -- not for a species-wide collection.
 *   "filter_bits_per_hash"  table bits of the membership filter per DISTINCT reference hash, 4..4096 (default 32: ~0.03 % of
 *                     the read hashes no genome holds get through and cost an all-zero row each; 32 MB at 40 000 S. aureus-like
 *                     genomes x 10 000 hashes, which share all but ~6e6 of their 4e8 hashes).
 *   "stream_query_rows"  rows of a pass's bit matrices = distinct query hashes one pass can hold; 0 (default) = 65 536, never
 *                     fewer than one read can need (s).  A batch (or pair of batches) with more distinct in-range hashes is
 *                     cut into several passes.  The bit matrices take rows x n_genomes / 8 bytes, three times.
 *   "stream_coalesce" 1 .. 8 (default 8): how many batches of skx_stream_enqueue_device / skx_stream_submit (there: at most 4)
 *                     may share one scoring pass (see skx_stream_enqueue_device).  n batches per pass divide the scans of the
 *                     reference per read by n (C2, 98 304-read batches: 77 / 97 / 111 / 116 M reads/s at 1 / 2 / 4 / 8) at
 *                     the cost of up to n - 1 more batches of latency and n + 1 copies of the per-batch sketch rows (25 MB
 *                     each at C2).  A group whose pairs or distinct hashes turn out too many for one pass is processed
 *                     batch by batch, and the stream forms smaller groups from then on.
 *   "rank_lanes"      1 .. 4 (default 2): the rankings of the batches that share a pass run as chains on this many HIP streams,
 *                     each with its own scratch (the table a batch starts from is all a chain needs of the one before it: it waits
 *                     for that chain's second kernel, not for its end).  C2, 20 batches from a fresh table: 131 M reads/s on one
 *                     lane, 134 M on two, 129-131 M on three / four; ~0.6 GB of scratch per lane at C2, 2.3 GB at C4.
 *   "rare_hash_genomes"  0 (no rare-hash index) .. 2^20 (default 1024): see skx_ref_rare_index.
 *   "reuse_membership"  0 (default) / 1: references with a static dense dictionary (skx_ref_static_dense) -- the bits the scan finds
 *                     for them depend on the reference alone.  0: every scoring pass streams the reference once (8 x stride x genomes
 *                     bytes: the pass SURVEY 8(d)'s roofline figure is defined on).  1: a stream scans the reference once per buffer set
 *                     and keeps the rows; later passes read the 52 MB (C2) of kept bits instead of the 3.2 GB of hashes.
 *   "comm_timeout_ms" 0 (default: no watchdog) .. 86 400 000: skx_comm_create (ncclCommInitRank) and skx_stream_allreduce
 *                     (ncclAllReduce + its stream synchronisation) block for ever when a peer never arrives.  With a
 *                     timeout set, a call that has not returned in time prints which rank was stuck in what to stderr and
 *                     ends the PROCESS with exit code SKX_COMM_TIMEOUT_EXIT -- a hung collective cannot be cancelled, and a
 *                     rank that exits lets the launcher tear the job down.  Consulted at every call (not at creation).
 * Unknown names fail with SKX_ERR_INVALID.
 */
#define SKX_COMM_TIMEOUT_EXIT 86
int skx_set_option(const char *name, uint64_t value);
int skx_get_option(const char *name, uint64_t *value);

/* ---- reference sketch collection, resident in HBM --------------------------------- */
/*
 * hashes: genome g's ascending distinct 64-bit hashes at [g*stride, g*stride + col_len[g]), col_len[g] <= stride.
 * k, seed, s are the sketch parameters reads are sketched with (src/sketchy.rs:331): the reference takes them from the
 * FIRST sketch of the collection -- s := number of hashes of sketch 0 (src/sketchy.rs:82, :520-527) -- while the other
 * sketches of a collection may be longer or shorter and are still intersected in full (:425-438).  So `s` (read sketch
 * size) and `stride` (capacity of a column = the longest sketch) are separate; a host mirroring the reference passes
 * s = col_len[0].  The library keeps its own device copy (a tiled, rank-major stride x N matrix); `hashes` may be
 * freed after the call.
 */
int skx_ref_create(skx_ref **out, int device, uint32_t k, uint64_t seed, uint32_t s, uint32_t stride, uint32_t n_genomes,
                   const uint64_t *hashes, const uint32_t *col_len);
/*
 * Several reference collections ("species": one sketch file each, src/sketchy.rs:81-82) resident together and scored
 * in ONE pass per batch.  The reference binary takes one sketch file per `predict` run, so a multi-species deployment
 * runs one predict per species over the same reads; here every read is sketched once and scanned against all of them,
 * and every species keeps its own running table and its own (sum desc, index asc) ranking.  All collections share
 * k, seed, s (the read sketch depends on them) and the column stride.  hashes[sp] / col_len[sp] are laid out as for
 * skx_ref_create.
 * Everywhere below, "n_genomes" of such a reference is the total over its species and genome-indexed arrays
 * (running table, per_read_shared, skx_common_hashes) hold the species one after the other; ranked rows come per
 * species, with genome indices local to the species.
 */
int skx_ref_create_multi(skx_ref **out, int device, uint32_t k, uint64_t seed, uint32_t s, uint32_t stride, uint32_t n_species,
                         const uint32_t *n_genomes, const uint64_t *const *hashes, const uint32_t *const *col_len);
int skx_ref_n_genomes(const skx_ref *ref, uint32_t *n_genomes);
int skx_ref_n_species(const skx_ref *ref, uint32_t *n_species);
int skx_ref_species_genomes(const skx_ref *ref, uint32_t species, uint32_t *n_genomes);
/* read sketch size and column stride the reference was created with */
int skx_ref_sketch_size(const skx_ref *ref, uint32_t *s, uint32_t *stride);
/* k-mer prefilter of the reference: keys it holds (0: none was built) and the bytes of its table */
int skx_ref_kmer_filter(const skx_ref *ref, uint64_t *n_keys, uint64_t *table_bytes);
/*
 * Rare-hash index of the reference (policy "rare_hash_genomes", default 1024, 0 = none): the distinct hashes of the collection
 * (n_keys), how many of them at most that many genomes hold (n_rare_keys), the entries of their genome lists (n_postings) and the
 * device memory of the whole index.  A pass looks its rare query hashes up there instead of asking the scan for them (the scan's
 * dictionary then holds the hashes many genomes share); results are the same with and without it.  All zero: none was built.
 */
int skx_ref_rare_index(const skx_ref *ref, uint64_t *n_keys, uint64_t *n_rare_keys, uint64_t *n_postings, uint64_t *bytes);
/*
 * ... and how its long genome lists (more than 8 genomes) are stored: n_long_lists of them have a bit row over the genomes;
 * n_pattern_lists of those are ALSO written as one of n_patterns shared patterns plus at most 14 exceptions (the lineage-level hashes
 * of a clonal collection: "the lineage's strains minus the odd one") -- a pass adds such rows up per pattern instead of per row; bytes =
 * the device memory of the records and the pattern matrix.  Exact either way; all zero: no bit rows / no patterns.
 */
int skx_ref_patterns(const skx_ref *ref, uint64_t *n_long_lists, uint64_t *n_patterns, uint64_t *n_pattern_lists, uint64_t *bytes);
/*
 * The static dense dictionary: with the rare-hash index the scan is only ever asked for hashes held by more genomes than the index
 * lists, and which hashes those are depends on the reference alone -- n_hashes of them (0 with *is_static set: every hash is rare,
 * nothing is ever scanned for).  Their rows of the bit matrix are fixed, a pass needs no dictionary sort or windows for them, and its
 * scan is queued with its first batch's sketch instead of behind its dictionary.  *is_static = 0: per-pass dictionaries (no index, too
 * many dense hashes for the scan kernel's slices, or long lists without bit rows).
 */
int skx_ref_static_dense(const skx_ref *ref, int *is_static, uint64_t *n_hashes);
/* bytes of reference hashes one scoring pass streams from HBM (8*stride*n_genomes) */
int skx_ref_pass_bytes(const skx_ref *ref, uint64_t *bytes);
/*
 * Genotype table of the reference, for consensus calls on the device (Sketchy::_print_results' consensus branch,
 * src/sketchy.rs:365-388: every genotype column called by majority over the `top` best genomes).
 * codes[g][f], uint32, n_features in 1..SKX_MAX_FEATURES; g runs over all genomes of the reference, species one after the other, as
 * in every genome-indexed array of this header.  Two genomes have the same value in column f iff their codes in column f are equal;
 * what the codes stand for is the host's business.
 * CONSENSUS of one ranked row (top_k genome indices of one species) in column f: the code that occurs most often among the top_k
 * genomes' codes in that column.  TIES GO TO THE SMALLEST CODE.  (The reference takes max_by over a HashMap: which of several tied
 * values it prints is unspecified.  A host that numbers every column's distinct strings in byte-wise sorted order gets the
 * lexicographically smallest tied string -- what a std::map walked in order, first maximum kept, gives.)  top_k may be even here.
 * Consensus output everywhere: codes_out[row][species][n_features] (uint32).
 * skx_ref_set_genotypes uploads the table (the library keeps its own copy, freed with the reference).  Once per reference, before any
 * stream of it binds a consensus output: a second call fails with SKX_ERR_INVALID, so no stream ever sees the table change under it.
 * NULL pointers, n_features of 0 or above SKX_MAX_FEATURES: SKX_ERR_INVALID, before the device is touched.
 */
int skx_ref_set_genotypes(skx_ref *ref, uint32_t n_features, const uint32_t *codes); /* [n_genomes][n_features], host */
int skx_ref_n_features(const skx_ref *ref, uint32_t *n_features);                    /* 0: no table */
void skx_ref_destroy(skx_ref *ref);

/* ---- streaming predictor ----------------------------------------------------------- */
/*
 * top_k: rows ranked after every read (per species), 0..min(genomes of the smallest species, SKX_MAX_TOP)
 * (0 = no per-read ranking, table only).  max_batch_reads / max_batch_bases bound one skx_stream_push call.
 */
int skx_stream_create(skx_stream **out, const skx_ref *ref, uint32_t top_k, uint32_t max_batch_reads,
                      uint64_t max_batch_bases);
/*
 * Consume n_reads reads: read r is the raw (un-normalised) ASCII bytes bases[offsets[r] .. offsets[r+1]).
 * Outputs are optional (NULL to skip), caller-allocated host arrays:
 *   topk_idx [n_reads][n_species][top_k]  genome indices (within the species) after that read, order =
 *                                         (cumulative sum desc, index asc); n_species = 1 for skx_ref_create
 *   topk_sum [n_reads][n_species][top_k]  the cumulative sums of those genomes after that read (exact while every entry of the
 *                                         table is below 2^55 - 1: skx_stream_table_add)
 *   per_read_shared [n_reads][n_genomes]  this read's shared-hash count per genome (parity/debug)
 *   sketches [n_reads][s], sketch_len [n_reads]  the read's bottom-s sketch, ascending (parity/debug)
 * Synchronous: on return the running table includes these reads.
 */
int skx_stream_push(skx_stream *st, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                    uint32_t *topk_idx, uint64_t *topk_sum, uint32_t *per_read_shared, uint64_t *sketches,
                    uint32_t *sketch_len);
/*
 * Same, with every pointer a DEVICE pointer on the stream's device (bench path: inputs already
 * resident in HBM; only the optional topk outputs are produced).  Asynchronous on the stream's
 * HIP stream except for the library's own internal synchronisation points; call
 * skx_stream_sync() before reading the outputs.
 */
int skx_stream_push_device(skx_stream *st, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                           uint64_t n_bases, uint32_t *d_topk_idx, uint64_t *d_topk_sum);
/*
 * skx_stream_push_device in two halves, so that consecutive batches overlap on the device without the host in between:
 * the call queues the sketch of THIS batch first, then waits for the published summary of the batch(es) enqueued before
 * and queues their scan / ranking passes.  (skx_stream_push_device does both halves of one batch in one call: the sketch
 * stream then idles while the host queues the passes -- ~0.25 ms per 98,304-read batch, measured.)
 * With the option "stream_coalesce" = n (default 8) up to n batches enqueued back to back SHARE one pass -- one dictionary
 * of their distinct hashes, one scan of the reference, one transpose, then one ranking each, in order -- when their pairs
 * and distinct hashes together fit a pass; otherwise each takes its own.  The back half of a group is queued by the call
 * that opens the next group (behind that batch's sketch), or by the flush.
 * Consequences: rows of batch i are written by work queued during one of the calls i + 1 .. i + n; an error found in batch i (offsets
 * not monotonic, a read outside n_bases) is returned by one of those calls or by the flush -- batches enqueued BEFORE the
 * faulty one are processed, the faulty one and those enqueued after it (up to the call that reports the error) are
 * dropped.  d_bases / d_offsets of a batch must stay untouched until skx_stream_sync() (or any other flushing entry
 * point followed by a synchronisation).  skx_stream_flush() queues the outstanding half; every other entry point of the
 * stream (sync, table, rank, push, reset, stats ...) flushes first.  Rows and table are those of skx_stream_push_device
 * on the same batches in the same order (src/sketchy.rs:328-354 is sequential over reads).
 */
int skx_stream_enqueue_device(skx_stream *st, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n_reads,
                              uint64_t n_bases, uint32_t *d_topk_idx, uint64_t *d_topk_sum);
int skx_stream_flush(skx_stream *st);
/*
 * 4-bit packed input (optional; the reference reads ASCII FASTX: src/sketchy.rs:328-333 -- this is a wire format for
 * hosts that feed the device over PCIe, where a 98 304-read batch of 1.5 kb reads is 147 MB of ASCII and the copy,
 * not the kernels, bounds a host-fed stream).  After skx_stream_set_packed_input(st, 1) every entry point of the stream
 * takes `bases` as two bases per byte, low nibble first, codes 0..3 = A C G T(U), any other value = a retained
 * non-ACGT byte (N, IUPAC, '-': breaks k-mers exactly as in the ASCII path); whitespace does not exist in this format.
 * `offsets` (and n_bases / max_batch_bases) count BASES, i.e. nibbles of the stream; a read may start on an odd
 * nibble.  skx_pack_bases() is the matching host-side packer: it appends the normalised bases of `ascii[0..n)`
 * (whitespace dropped) at nibble position `nibble_pos` of `packed` and returns the new position.  Rows, tables and
 * debug outputs are those of the same reads given as ASCII.
 */
int skx_stream_set_packed_input(skx_stream *st, int on);
uint64_t skx_pack_bases(const uint8_t *ascii, uint64_t n, uint8_t *packed, uint64_t nibble_pos);
/* the same up to the first line feed of ascii[0..n): packs what lies in front of it, *consumed = bytes taken, the line feed
 * included (n when there is none) -- a FASTX parser finds the end of a sequence line and packs it in one pass over its bytes */
uint64_t skx_pack_line(const uint8_t *ascii, uint64_t n, uint8_t *packed, uint64_t nibble_pos, uint64_t *consumed);
int skx_stream_sync(skx_stream *st);
/*
 * Host-fed pipeline.  skx_stream_submit() queues a batch from PAGE-LOCKED host buffers (skx_host_alloc; bases, offsets
 * and the optional row arrays) and returns without waiting for it: the host-to-device copy of batch i+1 runs on its
 * own stream into another staging slot (three; up to nine when batches share passes, "stream_coalesce" >= 2: each holds a batch's
 * bases, offsets and rows on the device) while batch i is sketched, scanned and ranked.  Processing lags one call
 * behind submission (submit(i) starts the copy of batch i, then runs batch i-1 through the kernels), so a single host
 * thread keeps the copy engine and the kernels busy at the same time -- what needletail's reader plus the loop of
 * src/sketchy.rs:328-354 would look like with the device in between.  Rows of batch `ticket` ([n_reads][n_species]
 * [top_k], as skx_stream_push) are in its arrays once skx_stream_wait(st, ticket) or skx_stream_drain(st) has returned;
 * the input buffers may be reused after the NEXT submit has returned (or after wait / drain).  Results are those of
 * the same batches pushed with skx_stream_push in the same order.  Do not interleave with skx_stream_push[_device]
 * without a drain in between.
 * Errors: a batch that turns out to be faulty (offsets not monotonic ...) makes the submit that hands it to the kernels -- or a
 * later wait / drain -- fail; batches submitted BEFORE it are processed and their rows delivered, the faulty one and those
 * submitted after it (up to the failing call, the failing call's own batch included) are dropped, and skx_stream_wait on a
 * dropped ticket fails instead of returning rows that were never written.
 * skx_stream_wait(ticket) on a batch that still waits for the partners of its group closes the group early (a pass for fewer
 * batches): a host that wants full groups waits for a ticket only once nine younger ones have been submitted -- by then the
 * batch is through and the call returns at once (sketchy_amd/host/sketchy_host.cpp does exactly that).
 */
int skx_stream_submit(skx_stream *st, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                      uint32_t *topk_idx, uint64_t *topk_sum, uint64_t *ticket);
int skx_stream_wait(skx_stream *st, uint64_t ticket);
int skx_stream_drain(skx_stream *st);
/*
 * Consensus codes of a batch (see skx_ref_set_genotypes): binds codes_out [n_reads][n_species][n_features] for the NEXT batch handed
 * to skx_stream_push, _push_device, _enqueue_device or _submit.  ONE-SHOT: that call consumes the binding whether it succeeds or
 * fails; a batch call with nothing bound behaves as if this function did not exist and writes no codes anywhere.
 * codes_out is the kind of memory the entry point's other outputs are: host for skx_stream_push, device for skx_stream_push_device /
 * skx_stream_enqueue_device, page-locked host for skx_stream_submit; the codes are valid whenever that entry point's rows are.  They
 * are computed on the device behind the batch's ranking (same queue) from the rows the batch returns, which are the same with and
 * without a binding.
 * A bound batch call fails with SKX_ERR_INVALID, before any device work and with the binding consumed, unless: the reference has a
 * genotype table; the stream has top_k >= 1; for the two _device entry points, d_topk_idx is non-NULL (the stream's own fallback row
 * buffer is shared by enqueued batches whose rankings run side by side: the vote would race with the next batch's ranking).
 * skx_stream_push and skx_stream_submit keep a device copy of their rows anyway: with a consensus bound they may be given NULL for
 * topk_idx and topk_sum, and then only codes travel back.
 * Device scratch for codes (the stream's own buffer for pushes, one per staging slot for submits) is allocated by the first bound
 * push / submit: streams that never bind pay nothing.
 */
int skx_stream_bind_consensus(skx_stream *st, uint32_t *codes_out);
/*
 * Change points of a batch: only the reads whose call differs from the previous read's, as a short event list.  (The reference prints
 * `top` lines after EVERY read, src/sketchy.rs:348-349, :391-399; nearly all of them repeat the read before.)
 * The CALL of read r of a batch is its ranked index row topk_idx[r] (n_species x top_k; sums are no part of it: they move with nearly
 * every read) or, in codes mode (ev_codes != NULL), its consensus codes [n_species][n_features] (skx_ref_set_genotypes: meaning, tie rule).
 * Read r is a change point iff r == 0 or call(r) != call(r - 1) in any element; the events of a batch are its change points in
 * ascending order.  STATELESS PER BATCH: read 0 of every batch is an event and nothing is compared across batches on the device -- the
 * rankings of enqueued batches run side by side, and a carried "last row" would make every batch wait for the end of the one before.
 * A caller chaining batches compares the first event of a batch with the last call it kept: one row compare on the host.
 * Binds, for the NEXT batch handed to skx_stream_push, _push_device, _enqueue_device or _submit (ONE-SHOT, consumed by that call
 * whether it succeeds or fails, exactly like skx_stream_bind_consensus):
 *   n_events [1]                          change points of the batch, NOT capped: n_events > cap says the list is truncated (the
 *                                         batch's full rows are still there if they were asked for)
 *   ev_read  [cap]                        batch-local read ordinals, ascending
 *   ev_idx   [cap][n_species][top_k]      optional: topk_idx of those reads
 *   ev_sum   [cap][n_species][top_k]      optional: topk_sum of those reads
 *   ev_codes [cap][n_species][n_features] optional: their consensus codes; non-NULL selects codes mode
 * The first min(n_events, cap) entries are written, nothing else is touched.  The arrays are the kind of memory the entry point's other
 * outputs are (host / device / page-locked host) and valid whenever that call's rows are.  An empty batch gives n_events = 0.
 * Codes mode works with or without a consensus output bound for the same batch; the vote goes to the scratch the consensus binding uses.
 * With a binding, skx_stream_push and skx_stream_submit may be given NULL for topk_idx and topk_sum: then only events travel back.
 * A bound batch call fails with SKX_ERR_INVALID, before any device work and with the binding consumed, when the stream has top_k == 0,
 * when a _device entry point is given d_topk_idx == NULL (as for consensus), or in codes mode without a genotype table.
 * cap == 0, a NULL stream, NULL n_events or ev_read: SKX_ERR_INVALID here.
 * Found on the device behind the ranking (same queue): a flag per read, an exclusive scan, a gather.  Scratch -- a flag and
 * a position per read, the event arrays of pushes and submits -- is allocated by the first bound batch; a stream that never binds
 * launches nothing and allocates nothing for this, and its rows and table are what they were.
 */
int skx_stream_bind_changes(skx_stream *st, uint32_t cap, uint32_t *n_events, uint32_t *ev_read, uint32_t *ev_idx, uint64_t *ev_sum,
                            uint32_t *ev_codes);
/*
 * Species call of a batch: for a reference of several species, which species the sample is after every read, and that species' rows
 * alone.  (The reference binary ranks against one file; a sample of unknown species is run once per file and the outputs are compared.)
 * For a stream with top_k >= 1 over a reference of n_species >= 1, after read r of a batch:
 *   lead[r][sp] = topk_sum[r][sp][0], the running sum of species sp's best genome.  All species share s, so the sums are comparable;
 *                 nothing is normalised.
 *   c(r)        = the SMALLEST sp whose lead[r][sp] is the maximum over the species: a table of zeros calls species 0, and two species
 *                 holding the same genomes call the lower one.
 *   call(r)     = (c(r), topk_idx[r][c(r)][0..top_k), topk_sum[r][c(r)][0..top_k)) and, with a genotype table, the consensus codes
 *                 [n_features] of species c(r) (skx_ref_set_genotypes: meaning, tie rule).
 * skx_stream_bind_call binds, for the NEXT batch handed to skx_stream_push, _push_device, _enqueue_device or _submit (ONE-SHOT, consumed
 * by that call whether it succeeds or fails, like skx_stream_bind_consensus):
 *   call_species [n_reads]              c(r); required
 *   call_idx     [n_reads][top_k]       optional: the called species' index row (genome indices local to that species)
 *   call_sum     [n_reads][top_k]       optional: its sums
 *   call_codes   [n_reads][n_features]  optional: its consensus codes
 * skx_stream_bind_call_changes binds, likewise, the CALL CHANGE POINTS of the batch: read r is one iff r == 0, or c(r) != c(r - 1), or the
 * compared part of the call differs in any element -- the index row, or in codes mode (ev_codes != NULL) the codes; sums are never
 * compared.  STATELESS PER BATCH exactly as skx_stream_bind_changes: read 0 of every batch is an event, nothing is carried across
 * batches on the device, the caller compares a batch's first event with the last call it kept.
 *   n_events   [1]                  call change points of the batch, NOT capped; required
 *   ev_read    [cap]                batch-local read ordinals, ascending; required
 *   ev_species [cap]                c of those reads; required
 *   ev_idx     [cap][top_k]         optional: their index rows
 *   ev_sum     [cap][top_k]         optional: their sums
 *   ev_codes   [cap][n_features]    optional: their codes; non-NULL selects codes mode
 * The first min(n_events, cap) entries are written, nothing else is touched.  An empty batch gives n_events = 0.
 * The two bindings are independent of each other and of the consensus and changes bindings: a batch may have all four.  Output memory
 * is the kind the entry point's other outputs are (host / device / page-locked host) and valid whenever that call's rows are.  With a
 * call bound, skx_stream_push and skx_stream_submit may be given NULL for topk_idx and topk_sum: then only the call travels back,
 * 1 + top_k values per read instead of n_species x top_k.
 * A bound batch call fails with SKX_ERR_INVALID, before any device work and with the binding consumed, when the stream has top_k == 0,
 * when call_codes or ev_codes is given and the reference has no genotype table, or when a _device entry point is given
 * d_topk_idx == NULL or d_topk_sum == NULL (the lead needs the sums, and the stream's fallback rows are shared between chains).
 * NULL stream, NULL required pointer, cap == 0: SKX_ERR_INVALID here.
 * Selected on the device behind the ranking, on the queue that ranked the batch, once its rows are final (and voted on, when codes
 * are wanted; the vote goes to the scratch the consensus binding uses): one kernel per pass writes the species, the compact rows and a
 * compare key {species, index row | codes}; the events are the change points of that key (flags, scan, gather: DESIGN.md 4).
 * Scratch -- compact rows, key, flags and positions, event arrays; per stream for pushes, per staging slot for submits -- is allocated
 * by the first bound batch; a stream that never binds launches nothing and allocates nothing for this, and its rows and table are what
 * they were.
 */
int skx_stream_bind_call(skx_stream *st, uint32_t *call_species, uint32_t *call_idx, uint64_t *call_sum, uint32_t *call_codes);
int skx_stream_bind_call_changes(skx_stream *st, uint32_t cap, uint32_t *n_events, uint32_t *ev_read, uint32_t *ev_species,
                                 uint32_t *ev_idx, uint64_t *ev_sum, uint32_t *ev_codes);
/* running sum-of-shared-hashes table, u64[n_genomes] (host) */
int skx_stream_table(skx_stream *st, uint64_t *cum);
/*
 * cum[g] += add[g]: resume from a checkpoint, or offset a shard by the totals of earlier shards.
 * The table is u64, but rows (topk_idx, topk_sum, skx_stream_rank) and table are exact only while every entry is below 2^55 - 1:
 * for 2 <= top_k <= 16 the ranking orders genomes by a 64-bit key that holds sum + 1 in 55 bits.  So this call refuses
 * (SKX_ERR_INVALID, table and stream left as they were) any add that would take an entry above SKX_MAX_TABLE_SUM = 2^54 - 1.  The
 * 2^54 in between is more than a stream can add: at s = 10 000 shared hashes per read it is 1.8e12 reads.
 */
int skx_stream_table_add(skx_stream *st, const uint64_t *add);
/* zero the table and the read counter */
int skx_stream_reset(skx_stream *st);
/* reads consumed so far (the reference's `read` counter minus one, src/sketchy.rs:327/:350) */
int skx_stream_reads(const skx_stream *st, uint64_t *n_reads);
/*
 * Counters for tuning / reporting (no effect on results): out[0] (read, hash) pairs of the last push, [1] scoring
 * passes it took, [2] distinct query hashes of the most recent dictionary, [3] reads sketched by the block sketcher so
 * far, [4] passes so far, [5] of those with the lean scan kernel, [6] pair capacity of a pass, [7] rank groups (512 genomes)
 * that received any bit in the most recent pass, [8] long reads (more than 8192 bases) whose sketch was split over several
 * wavefronts so far, [9] the segments they were cut into, [10] batches that were sketched a second time because their rows
 * did not fit the stream's row pool (it grows to fit), [11] passes that served SEVERAL enqueued batches (option
 * "stream_coalesce"), [12] groups of enqueued batches that turned out too large for one pass together (or held an error) and were
 * processed one by one -- the stream forms smaller groups after that, [13] rows (distinct query hashes) the bit matrices of a
 * pass hold right now, [14] how often they grew because a batch held more distinct hashes than that (only without a
 * "stream_query_rows" policy; at most a quarter of the free device memory is taken), [15] of the most recent dictionary ([2]) the
 * hashes the scan looked for (all of them without a rare-hash index, skx_ref_rare_index; else those many genomes hold), [16] batches
 * whose per-read ranking ran on their CANDIDATES only (the genomes whose value at the end of the batch reaches the top-th best
 * value at its start: at most 1024 per species), [17] batches ranked on every genome.  Waits for the stream's queued work.
 */
#define SKX_N_STATS 18
int skx_stream_stats(skx_stream *st, uint64_t *out, uint32_t n_out);
/* rank the CURRENT table: first top_k of (sum desc, index asc) per species; idx/sum are host arrays [n_species][top_k] */
int skx_stream_rank(skx_stream *st, uint32_t top_k, uint32_t *idx, uint64_t *sum);
/*
 * Breadth of a stream (no counterpart in the reference binary; what `mash screen` reports for a read set).  The running table is a sum:
 * it grows with depth and counts repeats.  The breadth of genome g is
 *   covered[g] = |{ h in column g : some read pushed so far has h in its bottom-s sketch }|
 * -- truncation to s first, membership second, as for the sums.  covered[g] <= col_len[g] and <= table[g]; it never decreases, saturates at
 * col_len[g], does not depend on how the reads are cut into batches, and covered[g] / col_len[g] is a containment in [0, 1] that compares
 * across species and sketch sizes.
 * skx_stream_enable_coverage gives the stream its SEEN set: one bit per distinct hash of the reference (per slot of the rare-hash index's key
 * table, plus one each for 0xFFFFFFFFFFFFFFFE and 0xFFFFFFFFFFFFFFFF), zeroed.  The set belongs to the stream: streams on one reference are
 * independent.  From then on every scoring pass of the stream marks its distinct query hashes that some genome holds (one small kernel behind
 * the pass's dictionary; nothing of the table, the gains or the ranking is involved, rows and table are what they were).
 *   SKX_ERR_INVALID      the stream has taken reads already (skx_stream_reads > 0): enable first, or after skx_stream_reset
 *   SKX_ERR_UNSUPPORTED  the reference has no rare-hash index (policy "rare_hash_genomes" = 0): nothing gives a query hash a persistent
 *                        identity there.  The stream is left exactly as it was and goes on working.
 *   a second call on an enabled stream: SKX_OK, nothing changes
 * skx_stream_reset clears the set and keeps coverage enabled; skx_stream_table_add and skx_stream_allreduce do not touch it (the sets of
 * several ranks are not combined); skx_stream_destroy frees it.  A stream that never enables coverage allocates and launches nothing for it.
 * The three queries flush pending batches (as skx_stream_table), wait for the marks of every queued pass and COUNT THEN: breadth is
 * queried, not streamed per read.  A query walks the resident matrix against the set -- the columns of the genomes asked for, one probe of
 * the key table per hash -- so _rows of a few genomes costs a fraction of the whole table:
 *   skx_stream_coverage       covered [n_genomes] (host), species one after the other
 *   skx_stream_coverage_rows  covered [n] for the global genome indices genomes[0..n) (any order, repeats allowed); n == 0: SKX_OK
 *   skx_stream_coverage_rank  per species the first top_k of (covered desc, index asc): idx / covered [n_species][top_k], indices local to
 *                             the species; top_k in 1..smallest species, independent of the stream's own top_k
 * SKX_ERR_INVALID: a stream that never enabled coverage; and, before the device is touched, a NULL argument, an index >= n_genomes, top_k
 * out of range.
 */
int skx_stream_enable_coverage(skx_stream *st);
int skx_stream_coverage(skx_stream *st, uint32_t *covered);
int skx_stream_coverage_rows(skx_stream *st, const uint32_t *genomes, uint32_t n, uint32_t *covered);
int skx_stream_coverage_rank(skx_stream *st, uint32_t top_k, uint32_t *idx, uint32_t *covered);
/*
 * Winner-takes-all breadth (`mash screen -w`; one round, as Mash does).  covered[g] credits a seen hash to every genome that holds it, so
 * in a clone tree the top of a ranking by covered is one lineage listed many times.  Here every seen hash is credited once:
 *   order      one global order over all genomes of the resident reference, all species together.  g precedes h when
 *              covered[g] * max(len[h], 1) > covered[h] * max(len[g], 1) (the larger containment, exact, in 64 bits; len = col_len, lifted
 *              hashes included); when the products are equal, covered[g] > covered[h]; when those are equal too, g < h (global indices)
 *   winner(x)  for every seen reference hash x, lifted ones included: the first genome in this order among the genomes that hold x
 *   won[g]     = number of seen hashes of g's column whose winner is g
 * Integer, exact, independent of how the reads were cut into batches.  won[g] <= covered[g]; the sum of won over all genomes is the
 * number of distinct seen hashes some genome holds (skx_stream_depth_count on a stream with depth); the first genome of the order has
 * won == covered; a reference whose genomes share nothing has won == covered everywhere.  The order comes from the plain covered and is
 * not iterated.
 * Nothing is enabled separately: the queries need skx_stream_enable_coverage, recompute everything from the seen set (so skx_stream_reset,
 * _table_add, _allreduce and _depth_import need no special handling), and a stream that never asks allocates and launches nothing for
 * them.  The first query allocates its scratch -- one uint32_t per bit of the seen set, two per padded genome --, skx_stream_destroy frees
 * it.  A query flushes pending batches, counts the whole table, brings the counts to the host for ONE sort of n_genomes keys, sends the
 * ranks back, and walks the matrix twice more: every holder of a hash can be its winner, so the marking walk always covers the whole
 * table, whatever is asked for; only the final count is restricted to the genomes of a list.
 *   skx_stream_winners       covered / won [n_genomes] (host), species one after the other; either may be NULL
 *   skx_stream_winners_rows  the same for the global genome indices genomes[0..n) (any order, repeats allowed); n == 0: SKX_OK
 *   skx_stream_winners_rank  per species the first top_k of (won desc, index asc): idx / won [n_species][top_k], indices local to the
 *                            species; top_k as in skx_stream_coverage_rank
 * SKX_ERR_INVALID: a stream that never enabled coverage; and, before the device is touched, a NULL stream, list or (_rank) output, an
 * index >= n_genomes (the outputs are untouched), top_k out of range.
 */
int skx_stream_winners(skx_stream *st, uint32_t *covered, uint32_t *won);
int skx_stream_winners_rows(skx_stream *st, const uint32_t *genomes, uint32_t n, uint32_t *covered, uint32_t *won);
int skx_stream_winners_rank(skx_stream *st, uint32_t top_k, uint32_t *idx, uint32_t *won);
/*
 * Depth of a stream (no counterpart in the reference binary; the median-multiplicity column of `mash screen`).  Breadth says whether a
 * genome is there, not how deep: a containment of 0.95 reads the same from 40 reads and from 4 million, and a contaminant seen once per
 * hash reads the same as the main strain seen fifty times per hash.
 *   depth[h] = number of reads pushed so far whose bottom-s sketch holds reference hash h
 * -- truncation to s first, as for covered; a read's sketch holds a hash once, so a read counts once per hash; repeats of a read count
 * again (depth, unlike breadth, grows with them).  One uint32_t per distinct hash of the reference, at the indices of the seen set's bits
 * (per slot of the key table, plus the two lifted hashes); it SATURATES at 2^32 - 1 and stays there.
 * skx_stream_enable_depth has the preconditions and errors of skx_stream_enable_coverage (before the first read or after a reset:
 * SKX_ERR_INVALID otherwise; no rare-hash index: SKX_ERR_UNSUPPORTED, stream untouched; second call: SKX_OK) and enables coverage too when
 * it is not on yet.  Every scoring pass then also counts its (read, hash) pairs per hash and adds them, clamped, to the counters.  Rows,
 * table and coverage are what they were.  skx_stream_reset zeroes the counters and keeps depth enabled; skx_stream_table_add and
 * skx_stream_allreduce do not touch them; skx_stream_destroy frees them.  A stream that never enables depth allocates and launches nothing.
 * The queries flush and count then, as the coverage queries do; indices, order, n == 0 and the error for an index out of range are those of
 * skx_stream_coverage / _rows.  Each output may be NULL:
 *   covered[g] = hashes of genome g's column with depth > 0: identical to skx_stream_coverage
 *   total[g]   = sum of the stored (clamped) counters over g's hashes: equal to skx_stream_table's entry as long as nothing saturated and
 *                neither skx_stream_table_add nor skx_stream_depth_import was used
 *   median[g]  = LOWER median of the counters of g's covered hashes: the element at index (covered - 1) / 2 of their ascending order, 0
 *                when covered == 0.  Integer and exact.  (Mash averages the two middle values of an even count; this library does not.)
 * The first query allocates a scratch of at most 256 MiB (one uint32_t per hash of the genomes of one launch); the table is walked in
 * chunks of as many 64-genome groups as fit.
 * Portable state.  The key table is filled by atomic insertion: its slot layout differs between two builds of one reference, so the
 * counters travel as (hash, count):
 *   skx_stream_depth_count   *n = distinct reference hashes with depth > 0, lifted ones included
 *   skx_stream_depth_export  those entries, order unspecified; *n is their number (not capped), hashes / counts [cap] take the first
 *                            min(*n, cap)
 *   skx_stream_depth_import  adds counts[i], clamped, to the counter of hashes[i] and marks the hash seen when counts[i] > 0; entries
 *                            naming one hash twice add up; an entry whose hash is no hash of this reference is skipped and counted in
 *                            *n_unknown (may be NULL).  Allowed at any time on a stream with depth: on a fresh stream it resumes a
 *                            checkpoint, on top of reads it merges another rank's shard.  The running table is not touched (use
 *                            skx_stream_table_add for the sums); after an import total[g] and the table differ.
 * SKX_ERR_INVALID: a stream that never enabled depth; a NULL stream, list or count pointer.
 */
int skx_stream_enable_depth(skx_stream *st);
int skx_stream_depth(skx_stream *st, uint32_t *covered, uint32_t *median, uint64_t *total);
int skx_stream_depth_rows(skx_stream *st, const uint32_t *genomes, uint32_t n, uint32_t *covered, uint32_t *median, uint64_t *total);
int skx_stream_depth_count(skx_stream *st, uint64_t *n);
int skx_stream_depth_export(skx_stream *st, uint64_t *hashes, uint32_t *counts, uint64_t cap, uint64_t *n);
int skx_stream_depth_import(skx_stream *st, const uint64_t *hashes, const uint32_t *counts, uint64_t n, uint64_t *n_unknown);
/*
 * Composition of a stream (no counterpart in the reference binary).  Every other number a stream returns describes the sample as a whole;
 * the species call names ONE species for the sample.  This says what the sample is made of: how many reads came from each resident
 * species, counted read by read from the read's OWN sketch -- a 3 % contaminant stays 3 %.
 * For every read r pushed after skx_stream_enable_composition(st, min_hits), with K_r its bottom-s sketch (truncation first, as everywhere):
 *   hits[r][sp] = |{h in K_r : some genome of species sp holds h inside its col_len}|
 * A hash held by two species counts for both.  The lifted values 0xFF..FE and 0xFF..FF count for nobody: no read hashes to them.
 * With best = max over sp of hits[r][sp] the read falls into exactly one class:
 *   best < min_hits                  unclassified (reads without a valid k-mer and reads whose hashes nobody holds are here)
 *   one species attains best         that species
 *   several species attain best      ambiguous -- there is NO lowest-index tie rule: a tie is not credited to anybody
 * The stream keeps, as uint64_t:
 *   reads[n_species + 2]  reads per species, then ambiguous, then unclassified; their sum is the reads pushed since enable or reset,
 *                         whichever entry point brought them and however a batch was cut into passes or shared one
 *   pairs[n_species]      pairs[sp] += hits[r][sp] for every read, whatever its class
 * With one species reads[0] is the number of reads that hit the reference at least min_hits times (the on-target reads).
 * skx_stream_enable_composition has the preconditions and errors of skx_stream_enable_depth (before the first read or after a reset:
 * SKX_ERR_INVALID otherwise; no rare-hash index: SKX_ERR_UNSUPPORTED, stream untouched); min_hits == 0: SKX_ERR_INVALID; a second call
 * with the same min_hits: SKX_OK, with another: SKX_ERR_INVALID; more than 64 species: SKX_ERR_UNSUPPORTED.  It needs neither coverage nor
 * depth and changes neither.  The first stream that enables it on a reference of several species builds that reference's species masks
 * (one uint64_t per distinct reference hash, one walk over the resident matrix); they are kept with the skx_ref and freed with it.  Every
 * scoring pass then classifies its reads on the device.  Rows, table, coverage and depth are what they were.  skx_stream_reset zeroes the
 * counters and keeps composition enabled; skx_stream_table_add, skx_stream_allreduce and skx_stream_depth_import do not touch them (the
 * counters are additive: ranks add theirs on the host); skx_stream_destroy frees them.  A stream that never enables composition allocates
 * and launches nothing.
 * skx_stream_composition flushes as the coverage queries do and copies the counters; either output may be NULL.
 * SKX_ERR_INVALID: a NULL stream; a stream that never enabled composition.
 */
int skx_stream_enable_composition(skx_stream *st, uint32_t min_hits);
int skx_stream_composition(skx_stream *st, uint64_t *reads /* [n_species + 2] or NULL */, uint64_t *pairs /* [n_species] or NULL */);
void skx_stream_destroy(skx_stream *st);

/*
 * Per-stage device time, measured with HIP events on the stream's own HIP stream when enabled.
 * Stages: 0 sketch (+ membership filter), 1 dictionary (distinct query hashes, windows), 2 reference scan (the roofline kernel),
 * 3 bit-matrix transpose, 4 rank (segment sums, prefix, per-read top-k, merge).
 */
#define SKX_N_STAGES 5
/* enabled: 0 off, 1 every stage, 2 only stage 2 (two event records per pass instead of twelve: ~2 % of a step) */
int skx_stream_set_profiling(skx_stream *st, int enabled);
/* ms[SKX_N_STAGES] accumulated milliseconds, launches[SKX_N_STAGES] timed intervals; resets the counters */
int skx_stream_profile(skx_stream *st, double *ms, uint64_t *launches);
/*
 * The reference scan ALONE on the device: `reps` launches back to back behind a synchronisation, their average in milliseconds.
 * (References with a static dense dictionary -- the hashes the scan can be asked for are a property of the reference; see
 * skx_ref_static_dense -- have their scans queued beside the sketches of the batches they serve, so no other entry point times one
 * by itself.)  SKX_ERR_INVALID for a stream that builds its scan's dictionary per pass.
 */
int skx_stream_scan_alone(skx_stream *st, uint32_t reps, double *ms_avg);

/* ---- stand-alone operators (parity / `shared` subcommand) --------------------------- */
/* sketch n_reads reads with (k, seed, s); outputs as in skx_stream_push (host arrays) */
int skx_sketch_reads(int device, uint32_t k, uint64_t seed, uint32_t s, const uint8_t *bases,
                     const uint64_t *offsets, uint32_t n_reads, uint64_t *sketches, uint32_t *sketch_len);
/* finch SketchScheme::{process x many, to_vec}: ONE sketcher per group of records (src/sketchy.rs:291-302, :473-478).
 * Group g = records [group_first[g], group_first[g+1]); group_first[0] = 0, group_first[n_groups] = n_records, non-decreasing.
 * sketches [n_groups][s] ascending distinct, zero-padded; sketch_len [n_groups];
 * valid_kmers [n_groups] (optional, NULL to skip): windows of k bases that are all A/C/G/T/U after normalisation, duplicates counted.
 * The per-record rows never leave the device: they are reduced there (a segmented merge tree) and n_groups x s hashes
 * come back.  Any number of records: beyond 2 GiB of per-record rows (or 1 GiB of bases) the call works in slices. */
int skx_sketch_groups(int device, uint32_t k, uint64_t seed, uint32_t s, const uint8_t *bases, const uint64_t *offsets,
                      uint32_t n_records, const uint32_t *group_first, uint32_t n_groups,
                      uint64_t *sketches, uint32_t *sketch_len, uint64_t *valid_kmers);
/* skx_sketch_groups + the abundance of every sketch hash: finch's KmerCount.count (src/sketchy.rs:302, :480-488), what its Mash
 * writer stores in `counts32`.  counts [n_groups][s], REQUIRED: counts[g][j] = valid k-mer windows (as valid_kmers counts them,
 * duplicates included) over all records of group g whose canonical hash is sketches[g][j]; 0 for j >= sketch_len[g]; saturating at
 * 0xFFFFFFFF (the true multiplicity: the width of finch's own counter is not pinned).  Independent of the order of records.
 * Every other argument, check and result as skx_sketch_groups; counts == NULL is SKX_ERR_INVALID.  The device walks a slice's bases
 * once more against the slice-local pooled rows and adds the counts of equal hashes wherever rows meet: exact. */
int skx_sketch_groups_counts(int device, uint32_t k, uint64_t seed, uint32_t s, const uint8_t *bases, const uint64_t *offsets,
                             uint32_t n_records, const uint32_t *group_first, uint32_t n_groups, uint64_t *sketches,
                             uint32_t *sketch_len, uint64_t *valid_kmers, uint32_t *counts);
/*
 * common[q][g] = |query sketch q  intersect  reference genome g|  (src/sketchy.rs:419-438) for
 * n_query ascending sketches laid out like skx_ref_create's input (row stride q_stride).
 * Any 64-bit value is an ordinary hash, in the reference and in a query: 0xFFFFFFFFFFFFFFFE and 0xFFFFFFFFFFFFFFFF (which the
 * library keeps outside its matrix, as exceptions) count for exactly the genomes that hold that very value -- a query's ...FE shares
 * nothing with a reference that holds only ...FF, and the other way round.
 */
int skx_common_hashes(const skx_ref *ref, const uint64_t *query, const uint32_t *query_len, uint32_t n_query,
                      uint32_t q_stride, uint32_t *common);
/* Sketchy::_shared_hashes' tail (src/sketchy.rs:304-312) for many query sketches at once: per query and species the first
 * top_k genomes of (shared desc, index asc), index local to the species.  Queries laid out as for skx_common_hashes (hashes
 * >= 0xFFFFFFFFFFFFFFFE in a query behave as they do there).
 * top_idx / top_shared: host arrays [n_query][n_species][top_k]; common: optional [n_query][n_genomes] (NULL to skip),
 * the counts the rows were taken from.  top_k: 1 .. min(genomes of the smallest species, SKX_MAX_TOP).
 * The counts stay on the device (a bit-sliced counter over the pass's bit matrix, then one selection per (query, species) that
 * reads its row a number of times independent of top_k): n_query x n_species x top_k rows come back.
 * Errors (all found before any device work): NULL required pointer / top_k out of range SKX_ERR_INVALID, a query row that is
 * not strictly ascending SKX_ERR_UNSORTED.  n_query == 0: SKX_OK, nothing is touched. */
int skx_rank_sketches(const skx_ref *ref, const uint64_t *query, const uint32_t *query_len, uint32_t n_query, uint32_t q_stride,
                      uint32_t top_k, uint32_t *top_idx, uint32_t *top_shared, uint32_t *common);
/* records -> one pooled sketch per group (as skx_sketch_groups, with the reference's k, seed, s and device) -> rows as above.
 * top_idx / top_shared: [n_groups][n_species][top_k].  sketches / sketch_len / valid_kmers: optional (NULL to skip), as in
 * skx_sketch_groups.  Works in chunks of groups: the pooled rows pass through at most 256 MiB of host memory.
 * n_groups == 0: SKX_OK, nothing is touched. */
int skx_predict_groups(const skx_ref *ref, const uint8_t *bases, const uint64_t *offsets, uint32_t n_records,
                       const uint32_t *group_first, uint32_t n_groups, uint32_t top_k,
                       uint32_t *top_idx, uint32_t *top_shared, uint64_t *sketches, uint32_t *sketch_len, uint64_t *valid_kmers);
/* Consensus codes (skx_ref_set_genotypes: semantics, tie rule) of ranked rows on the host: idx [n_rows][n_species][top_k] as returned
 * by skx_rank_sketches, skx_predict_groups, skx_stream_rank or any push; codes_out [n_rows][n_species][n_features].  Rows need not
 * hold distinct genomes.  Works in chunks: at most 64 MiB of rows are on the device at a time.
 * Errors (all found before any device work): NULL argument, top_k outside 1..SKX_MAX_TOP, no genotype table on the reference, an
 * index >= its species' genome count: SKX_ERR_INVALID.  n_rows == 0: SKX_OK, nothing is touched. */
int skx_consensus_rows(const skx_ref *ref, const uint32_t *idx, uint64_t n_rows, uint32_t top_k, uint32_t *codes_out);
/* Leave-one-out neighbours of the resident reference (no counterpart in the reference binary; the question its "Sketch validation"
 * section asks): for every genome g of [first, first + count) of `species` (indices local to the species) the first top_k genomes OF
 * THE SAME SPECIES OTHER THAN g in (shared hashes desc, index asc) order, shared = |column g  intersect  column h| by plain set
 * intersection (src/sketchy.rs:425-438; hashes >= 0xFFFFFFFFFFFFFFFE count like any other) -- what offline `predict` of g's own sketch
 * would print against a reference that lacks g.  g is left out INSIDE the selection: it ties with every duplicate of itself and with
 * every genome that contains its sketch, and among ties the lower index wins, so g need not be among the first top_k + 1 rows of a
 * plain ranking (a caller taking it out afterwards has to look for it), and at top_k = SKX_MAX_TOP there is no top_k + 1 to ask for.
 * nb_idx / nb_shared: host arrays [count][top_k].  codes_out: optional [count][n_features], the consensus of each row's neighbours
 * (skx_ref_set_genotypes: semantics, tie rule), voted on the device; non-NULL without a genotype table is SKX_ERR_INVALID.
 * top_k: 1 .. min(genomes of the species - 1, SKX_MAX_TOP).
 * The query rows never exist on the host: a kernel rebuilds them from the resident matrix and the exception list, in chunks of at most
 * 256 MiB of rows; the counting and the selection are skx_rank_sketches' (every species is counted, the species' own segment is ranked).
 * Errors (all found before any device work): NULL required pointer, species out of range, first + count beyond the species, top_k out of
 * range: SKX_ERR_INVALID.  count == 0: SKX_OK, nothing is touched. */
int skx_ref_neighbours(const skx_ref *ref, uint32_t species, uint32_t first, uint32_t count, uint32_t top_k,
                       uint32_t *nb_idx, uint32_t *nb_shared, uint32_t *codes_out);

/* The same operator alone on rows the caller holds (host): the change points of n_rows rows of `width` u32 each, row 0 included.
 * ev_row [cap] receives the first min(n_events, cap) of them (row indices, ascending; nothing past them is touched), *n_events their
 * number, not capped.  Works in chunks: at most 64 MiB of rows are on the device at a time; a chunk's first row is compared with the
 * previous chunk's last row on the host.  width outside 1..4096 (SKX_MAX_SPECIES x SKX_MAX_TOP) or a NULL argument: SKX_ERR_INVALID
 * before the device is touched.  n_rows == 0: SKX_OK, n_events = 0. */
int skx_changes_rows(int device, const uint32_t *rows, uint64_t n_rows, uint32_t width, uint64_t cap, uint64_t *n_events,
                     uint64_t *ev_row);

/* The species call (skx_stream_bind_call: definitions, tie rule) alone on rows the caller holds (host): idx / sum
 * [n_rows][n_species][top_k], codes [n_rows][n_species][n_features] or NULL.  call_species [n_rows] receives c(r); call_idx / call_sum
 * [n_rows][top_k] and call_codes [n_rows][n_features], each optional, the called species' rows.  Works in chunks: at most 64 MiB of
 * input rows are on the device at a time.  All found before the device is touched, SKX_ERR_INVALID: NULL idx, sum or call_species;
 * n_species outside 1..SKX_MAX_SPECIES; top_k outside 1..SKX_MAX_TOP; exactly one of codes and call_codes; n_features outside
 * 1..SKX_MAX_FEATURES when codes is given.  n_rows == 0: SKX_OK, nothing is touched. */
int skx_call_rows(int device, const uint32_t *idx, const uint64_t *sum, const uint32_t *codes, uint64_t n_rows, uint32_t n_species,
                  uint32_t top_k, uint32_t n_features, uint32_t *call_species, uint32_t *call_idx, uint64_t *call_sum,
                  uint32_t *call_codes);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI --------------------------------- */
#define SKX_COMM_ID_BYTES 128
int skx_comm_unique_id(uint8_t id[SKX_COMM_ID_BYTES]);                 /* rank 0; broadcast it out of band */
int skx_comm_create(skx_comm **out, int device, int rank, int n_ranks, const uint8_t id[SKX_COMM_ID_BYTES]);
/* ranks of the communicator as RCCL reports them (ncclCommCount) */
int skx_comm_n_ranks(const skx_comm *comm, int *n_ranks);
/* in-place sum of the running tables of all ranks' streams (u64, exact); keeping the sum over ranks of every entry below 2^55 - 1
 * (see skx_stream_table_add) is the caller's: nothing is checked here */
int skx_stream_allreduce(skx_stream *st, skx_comm *comm);
void skx_comm_destroy(skx_comm *comm);

/* ---- raw device buffers (so a host without a HIP binding can stage inputs in HBM) ---- */
int skx_dev_malloc(int device, void **d_ptr, size_t bytes);
int skx_dev_free(int device, void *d_ptr);
int skx_dev_upload(int device, void *d_dst, const void *h_src, size_t bytes);
int skx_dev_download(int device, void *h_dst, const void *d_src, size_t bytes);
int skx_dev_synchronize(int device);
/* free / total bytes of device memory (hipMemGetInfo): what a host sizing several streams per GPU looks at */
int skx_dev_mem_info(int device, uint64_t *free_bytes, uint64_t *total_bytes);
/* page-locked host memory for batch buffers handed to skx_stream_push / skx_sketch_reads: the H2D copy then runs at
 * full PCIe rate and asynchronously (what a double-buffered FASTX front-end wants; needletail's reader in
 * src/sketchy.rs:89-92 has no counterpart, the reference never leaves the host) */
int skx_host_alloc(int device, void **h_ptr, size_t bytes);
int skx_host_free(int device, void *h_ptr);

#ifdef __cplusplus
}
#endif
#endif /* SKETCHY_HIP_H */
