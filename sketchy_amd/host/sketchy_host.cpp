// sketchy_host.cpp -- C++ host above the C ABI, mirroring the reference's interface for the predict path
// (Rust is unavailable in this image; the reference is compiled code, so the host is C++).
//
//   sketchy::PredictConfig            src/sketchy.rs:43-50
//   Sketchy::predict                  src/sketchy.rs:66-124   (reference + genotypes + FASTX, header line, mode switch)
//   Sketchy::_sum_of_shared_hashes    src/sketchy.rs:317-356  (streaming: rows after every read)  -> skx_stream_push
//   Sketchy::_shared_hashes           src/sketchy.rs:281-315  (offline: one pooled sketch per input) -> skx_sketch_groups + skx_rank_sketches
//   Sketchy::_print_results           src/sketchy.rs:358-402  (rows / consensus)
//   Sketchy::shared                   src/sketchy.rs:238-279                                       -> skx_common_hashes
//   Sketchy::info (names only)        src/sketchy.rs:172-208
//   Sketchy::check                    src/sketchy.rs:212-236
//   Sketchy::sketch + _sketch_files   src/sketchy.rs:128-167, :465-494  (genome files -> Mash .msh)      -> skx_sketch_groups
// Command line: the reference's flag names and defaults (src/cli.rs:25-132).
//
// Streaming (`predict -s`) runs as a pipeline of four stages (the reference reads, scores and prints one record at a time
// on one thread, src/sketchy.rs:328-354):
//   parse   N threads: an uncompressed input file is mapped and cut at record boundaries into chunks of ~batch reads; a
//           thread parses its chunk and PACKS the bases as it goes (4 bits each, skx_pack_bases) into a page-locked slot.
//           gzip input and stdin are parsed by one thread (the stream is sequential), everything behind it is the same
//   device  one thread: skx_stream_submit, in file order -- the copy of batch i + 1 overlaps the kernels of batch i, up to
//           four batches share one scan of the reference (include/sketchy_hip.h)
//   format  M threads: the rows of a finished batch as text (src/sketchy.rs:389-400)
//   write   in file order, by whichever format thread completes the next batch
// Rows are the reference's, byte for byte; what changes is who does what when.
// --changes (not in the reference): of those rows only read 1 and the reads whose lines, the shared_hashes column aside, differ from the
// read before -- the library lists every batch's change points (skx_stream_bind_changes), format turns those into text, write drops a
// batch's first block when the batch before ended with the same call.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <exception>
#include <iostream>
#include <map>
#include <mutex>
#include <optional>
#include <sched.h>
#include <thread>

#include "formats.hpp"
#include "sketchy_hip.h"

// The pooled entry point is referenced WEAKLY: a library without it (the stub of the sanitizer build, tests/stub) leaves the
// address null and the host pools the per-record rows of skx_sketch_reads itself; libsketchy_hip.so always has it.
extern "C" int skx_sketch_groups(int device, uint32_t k, uint64_t seed, uint32_t s, const uint8_t* bases, const uint64_t* offsets,
                                 uint32_t n_records, const uint32_t* group_first, uint32_t n_groups, uint64_t* sketches,
                                 uint32_t* sketch_len, uint64_t* valid_kmers) __attribute__((weak));
// ... so is its counted form (`sketch --counts`: the abundance of every sketch hash, Mash's counts32): a library without it cannot
// fill the list, and --counts says so instead of writing a file without counts.
extern "C" int skx_sketch_groups_counts(int device, uint32_t k, uint64_t seed, uint32_t s, const uint8_t* bases, const uint64_t* offsets,
                                        uint32_t n_records, const uint32_t* group_first, uint32_t n_groups, uint64_t* sketches,
                                        uint32_t* sketch_len, uint64_t* valid_kmers, uint32_t* counts) __attribute__((weak));
// ... and so is the device-side ranking of many pooled sketches: without it the host takes skx_common_hashes' counts and sorts.
extern "C" int skx_rank_sketches(const skx_ref* ref, const uint64_t* query, const uint32_t* query_len, uint32_t n_query, uint32_t q_stride,
                                 uint32_t top_k, uint32_t* top_idx, uint32_t* top_shared, uint32_t* common) __attribute__((weak));
// ... and the consensus calls on the device (genotype table as codes on the reference, one code per column and read back instead of
// rows): without them --consensus votes over rows on the host, as before.
extern "C" int skx_ref_set_genotypes(skx_ref* ref, uint32_t n_features, const uint32_t* codes) __attribute__((weak));
extern "C" int skx_consensus_rows(const skx_ref* ref, const uint32_t* idx, uint64_t n_rows, uint32_t top_k, uint32_t* codes_out) __attribute__((weak));
extern "C" int skx_stream_bind_consensus(skx_stream* st, uint32_t* codes_out) __attribute__((weak));
// ... and the leave-one-out neighbours of the resident reference (`neighbours`): without it the host intersects the file's sketches itself.
extern "C" int skx_ref_neighbours(const skx_ref* ref, uint32_t species, uint32_t first, uint32_t count, uint32_t top_k, uint32_t* nb_idx,
                                  uint32_t* nb_shared, uint32_t* codes_out) __attribute__((weak));
// ... and the per-batch event list (`predict -s --changes`): without it the host finds the change points itself, over every read's rows.
extern "C" int skx_stream_bind_changes(skx_stream* st, uint32_t cap, uint32_t* n_events, uint32_t* ev_read, uint32_t* ev_idx, uint64_t* ev_sum,
                                       uint32_t* ev_codes) __attribute__((weak));
// ... and what `predict` with several -r stands on: the species resident together, the species call of a stream and of rows the host
// holds.  There is no host route around these: without them several -r end with a message that names what is missing.
extern "C" int skx_ref_create_multi(skx_ref** out, int device, uint32_t k, uint64_t seed, uint32_t s, uint32_t stride, uint32_t n_species,
                                    const uint32_t* n_genomes, const uint64_t* const* hashes, const uint32_t* const* col_len) __attribute__((weak));
extern "C" int skx_stream_bind_call(skx_stream* st, uint32_t* call_species, uint32_t* call_idx, uint64_t* call_sum, uint32_t* call_codes) __attribute__((weak));
extern "C" int skx_stream_bind_call_changes(skx_stream* st, uint32_t cap, uint32_t* n_events, uint32_t* ev_read, uint32_t* ev_species,
                                            uint32_t* ev_idx, uint64_t* ev_sum, uint32_t* ev_codes) __attribute__((weak));
extern "C" int skx_call_rows(int device, const uint32_t* idx, const uint64_t* sum, const uint32_t* codes, uint64_t n_rows, uint32_t n_species,
                             uint32_t top_k, uint32_t n_features, uint32_t* call_species, uint32_t* call_idx, uint64_t* call_sum,
                             uint32_t* call_codes) __attribute__((weak));
// ... and the breadth of a stream (`screen`).  No host route either: the seen set lives on the device, beside the stream.
extern "C" int skx_stream_enable_coverage(skx_stream* st) __attribute__((weak));
extern "C" int skx_stream_coverage(skx_stream* st, uint32_t* covered) __attribute__((weak));
extern "C" int skx_stream_table(skx_stream* st, uint64_t* cum) __attribute__((weak));  // (`screen` is the host's only reader of the table)
// ... and its depth (`screen --depth`): the counters live beside the seen set
extern "C" int skx_stream_enable_depth(skx_stream* st) __attribute__((weak));
extern "C" int skx_stream_depth_rows(skx_stream* st, const uint32_t* genomes, uint32_t n, uint32_t* covered, uint32_t* median, uint64_t* total)
    __attribute__((weak));
// ... and the breadth with every seen hash credited to one sketch (`screen --winner-take-all`): the winner is a property of each hash
extern "C" int skx_stream_winners(skx_stream* st, uint32_t* covered, uint32_t* won) __attribute__((weak));
// ... and what the read set is made of (`composition`): every read is classified on the device, beside the stream
extern "C" int skx_stream_enable_composition(skx_stream* st, uint32_t min_hits) __attribute__((weak));
extern "C" int skx_stream_composition(skx_stream* st, uint64_t* reads, uint64_t* pairs) __attribute__((weak));

namespace sketchy {

struct PredictConfig { size_t top = 1, limit = 0; bool stream = false, consensus = false, header = false;
                       // (not in the reference: print only the reads at which the call changes, see sum_of_shared_hashes)
                       bool changes = false;
                       // (not in the reference: how the streaming pipeline is run, and whether it says how fast it was)
                       size_t threads = 0; bool timing = false, pin = false; };

struct SketchyError : std::runtime_error { using std::runtime_error::runtime_error; };
// a command line that asks for something the inputs cannot give (found only once they are read): exit status 2, as usage errors
struct UsageError : SketchyError { using SketchyError::SketchyError; };

// (not in the reference) `neighbours`: rows, one consensus line per genome, or one line per genotype column
struct NeighboursConfig { size_t top = 1; bool consensus = false, summary = false, header = false; };

static void hip_check(int rc, const char* what) {
    if (rc != SKX_OK) throw SketchyError(std::string(what) + ": " + skx_last_error());
}

class Sketchy {
  public:
    explicit Sketchy(int device = 0, size_t batch_reads = 16384) : device_(device), batch_(batch_reads) {}

    // fastx: the inputs (none: stdin).  Offline mode takes several: every path is one sample, its block of rows is what a run on that
    // file alone prints, in input order (the header once); streaming takes one.
    void predict(const std::vector<std::string>& fastx, const std::string& reference, const std::string& genotypes,
                 const PredictConfig& config, std::ostream& out) {
        if (config.stream && fastx.size() > 1) throw SketchyError("--stream takes one input");
        if (config.consensus && config.top % 2 != 1)  // src/sketchy.rs:74-79
            throw SketchyError("--top must be an odd number when using --consensus");
        const auto sketches = read_sketch(reference);
        if (sketches.empty()) throw SketchyError("reference sketch file holds no sketches");
        const auto geno = read_genotypes(genotypes);
        for (const auto& s : sketches)  // the reference panics on a missing name (geno_map[&name], :308/:345)
            if (!geno.map.count(s.name)) throw SketchyError("reference sketch " + s.name + " has no row in the genotype table");
        if (config.top > sketches.size()) throw SketchyError("--top exceeds the number of reference sketches");
        if (config.header) out << "reads\tsketch_id\tshared_hashes\t" << geno.header << "\n";  // :99-101
        Ref ref(sketches, device_);
        cons_ = ConsensusTable();
        if (config.consensus) set_consensus_table(sketches, ref, geno, config);
        if (config.stream) sum_of_shared_hashes(fastx.empty() ? std::string("-") : fastx[0], sketches, ref, geno, config, out);
        else shared_hashes(fastx.empty() ? std::vector<std::string>{"-"} : fastx, sketches, ref, geno, config, out);
    }

    // `predict` with several -r (not in the reference, which takes one file and is run once per species): reference i goes with table i,
    // all of them are resident together (skx_ref_create_multi), every read is sketched once, and after every read ONE species is
    // called -- the lowest whose best genome has the largest sum (skx_stream_bind_call) -- whose rows or consensus are printed with
    // the species' name (the file's name without directory and .msh) in a second field.
    void predict_multi(const std::vector<std::string>& fastx, const std::vector<std::string>& references, const std::vector<std::string>& genotypes,
                       const PredictConfig& config, std::ostream& out) {
        if (config.stream && fastx.size() > 1) throw SketchyError("--stream takes one input");
        if (config.consensus && config.top % 2 != 1) throw SketchyError("--top must be an odd number when using --consensus");
        if (config.threads || config.timing || config.pin)  // (call_stream runs on this thread alone and keeps no timings)
            std::fprintf(stderr, "sketchy-hip: warning: -j, --timing and --pin have no effect with several -r\n");
        // (nothing is read and nothing is printed before the library is known to have what this mode stands on)
        auto need = [](bool have, const char* name) {
            if (!have) throw SketchyError(std::string("several -r need ") + name + ", which the loaded libsketchy_hip does not export");
        };
        need(skx_ref_create_multi != nullptr, "skx_ref_create_multi");
        if (config.stream) need(skx_stream_bind_call != nullptr, "skx_stream_bind_call");
        if (config.stream && config.changes) need(skx_stream_bind_call_changes != nullptr, "skx_stream_bind_call_changes");
        if (!config.stream) { need(skx_call_rows != nullptr, "skx_call_rows"); need(skx_rank_sketches != nullptr, "skx_rank_sketches"); }
        if (config.consensus) { need(skx_ref_set_genotypes != nullptr, "skx_ref_set_genotypes"); need(skx_consensus_rows != nullptr, "skx_consensus_rows"); }
        if (references.size() > SKX_MAX_SPECIES) throw UsageError("at most " + std::to_string(SKX_MAX_SPECIES) + " references can be resident together");
        std::vector<Species> species(references.size());
        std::vector<std::vector<Sketch>> all;
        size_t smallest = (size_t)-1;
        for (size_t i = 0; i < references.size(); ++i) {
            Species& sp = species[i];
            auto sketches = read_sketch(references[i]);
            if (sketches.empty()) throw SketchyError("reference sketch file " + references[i] + " holds no sketches");
            sp.geno = read_genotypes(genotypes[i]);
            for (const auto& s : sketches)
                if (!sp.geno.map.count(s.name)) throw SketchyError("reference sketch " + s.name + " has no row in the genotype table " + genotypes[i]);
            const auto slash = references[i].find_last_of('/');
            sp.name = slash == std::string::npos ? references[i] : references[i].substr(slash + 1);
            if (sp.name.size() > 4 && sp.name.compare(sp.name.size() - 4, 4, ".msh") == 0) sp.name.resize(sp.name.size() - 4);
            const Sketch &a = all.empty() ? sketches[0] : all[0][0], &b = sketches[0];
            if (a.kmer_length != b.kmer_length || a.hash_seed != b.hash_seed || a.hashes.size() != b.hashes.size())
                throw UsageError("references " + references[0] + " and " + references[i] + " do not agree in k-mer size, seed and the size of their first sketch (" +
                                 std::to_string(a.kmer_length) + "/" + std::to_string(a.hash_seed) + "/" + std::to_string(a.hashes.size()) + " and " +
                                 std::to_string(b.kmer_length) + "/" + std::to_string(b.hash_seed) + "/" + std::to_string(b.hashes.size()) + ")");
            smallest = std::min(smallest, sketches.size());
            all.push_back(std::move(sketches));
        }
        if (config.top < 1 || config.top > smallest || config.top > SKX_MAX_TOP)
            throw UsageError("--top must be between 1 and the number of sketches of the smallest reference = " + std::to_string(std::min<size_t>(smallest, SKX_MAX_TOP)));
        // consensus: every (species, column) has its own dictionary of distinct strings in byte-wise sorted order; tables narrower than
        // the widest are padded with code 0, and only a species' own columns are printed
        size_t nfeat = 0;
        std::vector<uint32_t> codes;
        if (config.consensus) {
            for (size_t i = 0; i < species.size(); ++i) {
                Species& sp = species[i];
                sp.nfeat = sp.geno.map.at(all[i][0].name).size();
                for (const auto& s : all[i])
                    if (sp.geno.map.at(s.name).size() != sp.nfeat) throw UsageError("genotype table " + genotypes[i] + " is ragged: --consensus with several -r needs as many columns in every row");
                if (sp.nfeat < 1 || sp.nfeat > SKX_MAX_FEATURES)
                    throw UsageError("genotype table " + genotypes[i] + " has " + std::to_string(sp.nfeat) + " columns: --consensus with several -r takes 1 to " + std::to_string(SKX_MAX_FEATURES));
                nfeat = std::max(nfeat, sp.nfeat);
            }
            size_t total = 0, g0 = 0;
            for (const auto& sk : all) total += sk.size();
            codes.assign(total * nfeat, 0);
            for (size_t i = 0; i < species.size(); ++i) {
                Species& sp = species[i];
                for (size_t j = 0; j < sp.nfeat; ++j) {
                    std::map<std::string, uint32_t> rank;
                    for (const auto& s : all[i]) rank.emplace(sp.geno.map.at(s.name)[j], 0u);
                    std::vector<std::string> vals;
                    for (auto& kv : rank) { kv.second = (uint32_t)vals.size(); vals.push_back(kv.first); }
                    for (size_t g = 0; g < all[i].size(); ++g) codes[(g0 + g) * nfeat + j] = rank.at(sp.geno.map.at(all[i][g].name)[j]);
                    sp.values.push_back(std::move(vals));
                }
                g0 += all[i].size();
            }
        } else {
            for (size_t i = 0; i < species.size(); ++i)
                for (const auto& s : all[i]) {
                    species[i].mid.push_back("\t" + species[i].name + "\t" + s.name + "\t");
                    species[i].tail.push_back("\t" + join_tab(species[i].geno.map.at(s.name)) + "\n");
                }
        }
        if (config.header)
            for (const auto& sp : species) out << "reads\t" << sp.name << "\tsketch_id\tshared_hashes\t" << sp.geno.header << "\n";
        Ref ref(all, device_);
        if (config.consensus) hip_check(skx_ref_set_genotypes(ref.h, (uint32_t)nfeat, codes.data()), "genotype table");
        if (config.stream) call_stream(fastx.empty() ? std::string("-") : fastx[0], species, ref, nfeat, config, out);
        else call_offline(fastx.empty() ? std::vector<std::string>{"-"} : fastx, species, ref, nfeat, config, out);
    }

    // `sketchy shared`: every reference x query pair, "ref query common" (src/sketchy.rs:251-276)
    void shared(const std::string& reference, const std::string& query, std::ostream& out) {
        const auto refs = read_sketch(reference), qs = read_sketch(query);
        if (refs.empty() || qs.empty()) throw SketchyError("empty sketch file");
        Ref ref(refs, device_);
        uint32_t stride = 1;
        for (const auto& q : qs) stride = std::max<uint32_t>(stride, (uint32_t)q.hashes.size());
        std::vector<uint64_t> flat(qs.size() * (size_t)stride, 0);
        std::vector<uint32_t> len(qs.size());
        for (size_t i = 0; i < qs.size(); ++i) {
            std::copy(qs[i].hashes.begin(), qs[i].hashes.end(), flat.begin() + i * stride);
            len[i] = (uint32_t)qs[i].hashes.size();
        }
        std::vector<uint32_t> common(qs.size() * refs.size());
        hip_check(skx_common_hashes(ref.h, flat.data(), len.data(), (uint32_t)qs.size(), stride, common.data()), "shared");
        for (size_t r = 0; r < refs.size(); ++r)
            for (size_t q = 0; q < qs.size(); ++q) {
                if (refs[r].kmer_length != qs[q].kmer_length || refs[r].hash_seed != qs[q].hash_seed)
                    throw SketchyError("reference (" + refs[r].name + ") does not match query (" + qs[q].name + ")");
                out << refs[r].name << " " << qs[q].name << " " << common[q * refs.size() + r] << "\n";
            }
    }

    // `sketchy check` (src/sketchy.rs:212-236): the per-row identifier comparison builds an error and discards it
    // (:219-228), so only the size check has an effect -- kept that way
    void check(const std::string& reference, const std::string& genotypes, std::ostream& out) {
        const auto sk = read_sketch(reference);
        const auto geno = read_genotypes(genotypes);
        if (sk.size() != geno.rows) throw SketchyError("reference sketch and genotype table must have the same length");
        out << "ok\n";
    }

    // `neighbours` (not in the reference; the question of its "Sketch validation" section asked directly): for every sketch of the file,
    // in file order, the `top` OTHER sketches that share the most hashes with it -- (shared desc, file order asc), what offline predict of
    // the genome's own sketch prints against a reference that lacks it -- as rows, as one consensus line per genome (-c), or as one
    // "column correct total" line per genotype column (-S): correct = genomes whose own string is the consensus of their neighbours.
    // The rows (and with a genotype table the consensus codes) come from skx_ref_neighbours.  A library without it (tests/stub) has no
    // counts to give either -- the host then intersects the file's sketches itself (src/sketchy.rs:425-438, all pairs: for files of test
    // size), sorts stably with the genome itself skipped and votes over the rows as print_results does.  Both ways print the same bytes.
    void neighbours(const std::string& reference, const std::string& genotypes, const NeighboursConfig& config, std::ostream& out) {
        const auto sketches = read_sketch(reference);
        const size_t n = sketches.size(), top = config.top;
        if (n < 2) throw SketchyError("neighbours needs a reference of at least two sketches");
        if (top < 1 || top > n - 1) throw UsageError("--top must be between 1 and the number of reference sketches - 1 = " + std::to_string(n - 1));
        const bool with_geno = !genotypes.empty();
        Genotypes geno;
        if (with_geno) {
            geno = read_genotypes(genotypes);
            for (const auto& s : sketches)
                if (!geno.map.count(s.name)) throw SketchyError("reference sketch " + s.name + " has no row in the genotype table");
        }
        Ref ref(sketches, device_);
        std::vector<uint32_t> idx(n * top), shared(n * top), codes;
        cons_ = ConsensusTable();
        const bool want_call = config.consensus || config.summary;
        if (skx_ref_neighbours && top <= SKX_MAX_TOP) {
            if (want_call) { PredictConfig pc; pc.top = top; set_consensus_table(sketches, ref, geno, pc); }
            if (cons_.on) codes.resize(n * cons_.nfeat);
            hip_check(skx_ref_neighbours(ref.h, 0, 0, (uint32_t)n, (uint32_t)top, idx.data(), shared.data(), cons_.on ? codes.data() : nullptr), "neighbours");
        } else {
            std::vector<uint32_t> common(n), order;
            for (size_t g = 0; g < n; ++g) {
                const auto& a = sketches[g].hashes;
                order.clear();
                for (size_t h = 0; h < n; ++h) {
                    const auto& b = sketches[h].hashes;
                    uint32_t c = 0;
                    for (size_t i = 0, j = 0; i < a.size() && j < b.size();) {
                        if (a[i] < b[j]) ++i; else if (b[j] < a[i]) ++j; else { ++c; ++i; ++j; }
                    }
                    common[h] = c;
                    if (h != g) order.push_back((uint32_t)h);
                }
                std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return common[x] > common[y]; });
                for (size_t j = 0; j < top; ++j) { idx[g * top + j] = order[j]; shared[g * top + j] = common[order[j]]; }
            }
        }
        // the call of genome g's neighbours, one string per genotype column
        auto call_of = [&](size_t g) {
            if (!cons_.on) return vote(sketches, geno, idx.data() + g * top, top);
            std::vector<std::string> call;
            for (size_t j = 0; j < cons_.nfeat; ++j) call.push_back(cons_.values[j][codes[g * cons_.nfeat + j]]);
            return call;
        };
        if (config.summary) {
            const auto columns = split_tab(geno.header);
            std::vector<size_t> correct(columns.size(), 0);
            for (size_t g = 0; g < n; ++g) {
                const auto call = call_of(g);
                const auto& own = geno.map.at(sketches[g].name);
                for (size_t j = 0; j < columns.size(); ++j) correct[j] += j < call.size() && j < own.size() && call[j] == own[j] ? 1 : 0;
            }
            for (size_t j = 0; j < columns.size(); ++j) out << columns[j] << "\t" << correct[j] << "\t" << n << "\n";
            return;
        }
        if (config.header) out << "sketch_id\tneighbour_id\tshared_hashes" << (with_geno ? "\t" + geno.header : std::string()) << "\n";
        for (size_t g = 0; g < n; ++g) {
            if (config.consensus) { out << sketches[g].name << "\t-\t-\t" << join_tab(call_of(g)) << "\n"; continue; }
            for (size_t j = 0; j < top; ++j) {
                const auto& name = sketches[idx[g * top + j]].name;
                out << sketches[g].name << "\t" << name << "\t" << shared[g * top + j];
                if (with_geno) out << "\t" << join_tab(geno.map.at(name));
                out << "\n";
            }
        }
    }

    // `screen` (not in the reference; what `mash screen` answers): how much of every reference sketch is in the read set.  All reads go
    // through one table-only stream (top_k = 0: no per-read ranking) with coverage enabled; then, per sketch, covered = its hashes that
    // some read shared, containment = covered / its own size, and the running sum from the table.  The `top` best by containment
    // (ties: the sketch earlier in the file) are printed.  One reference only: several -r are not built.
    // depth: also the median multiplicity of the printed sketches (the lower median of how many reads shared each covered hash), from
    // skx_stream_depth_rows of the TOP rows; identity: Mash screen's containment^(1/k), computed here.
    // winners (`mash screen -w`): every seen hash is credited to ONE sketch, the best of its holders (skx_stream_winners); the rows are
    // then ordered by won / size (ties: the larger plain containment, then the sketch earlier in the file), two columns -- won and
    // winner_containment -- follow shared_hashes, and the identity is taken from the winner containment, as Mash does.
    void screen(const std::string& fastx, const std::string& reference, const std::string& genotypes, size_t top, size_t limit, bool header,
                std::ostream& out, bool depth = false, bool identity = false, bool winners = false) {
        if (winners && !skx_stream_winners) throw UsageError("screen --winner-take-all needs skx_stream_winners, which the loaded libsketchy_hip does not export");
        if (depth && !skx_stream_enable_depth) throw UsageError("screen --depth needs skx_stream_enable_depth, which the loaded libsketchy_hip does not export");
        if (depth && !skx_stream_depth_rows) throw UsageError("screen --depth needs skx_stream_depth_rows, which the loaded libsketchy_hip does not export");
        // there is no host route to the number: a library without the entry points ends here, before anything is read
        if (!skx_stream_enable_coverage) throw SketchyError("screen needs skx_stream_enable_coverage, which the loaded libsketchy_hip does not export");
        if (!skx_stream_coverage) throw SketchyError("screen needs skx_stream_coverage, which the loaded libsketchy_hip does not export");
        if (!skx_stream_table) throw SketchyError("screen needs skx_stream_table, which the loaded libsketchy_hip does not export");
        const auto sketches = read_sketch(reference);
        const size_t n = sketches.size();
        if (n == 0) throw SketchyError("reference sketch file holds no sketches");
        if (top < 1 || top > n) throw UsageError("--top must be between 1 and the number of reference sketches = " + std::to_string(n));
        const bool with_geno = !genotypes.empty();
        Genotypes geno;
        if (with_geno) {
            geno = read_genotypes(genotypes);
            for (const auto& s : sketches)
                if (!geno.map.count(s.name)) throw SketchyError("reference sketch " + s.name + " has no row in the genotype table");
        }
        Ref ref(sketches, device_);
        const uint64_t max_bases = 1ull << 28;
        skx_stream* st = nullptr;
        hip_check(skx_stream_create(&st, ref.h, 0, (uint32_t)batch_, max_bases), "stream");
        std::vector<uint32_t> covered(n), order(n), median(depth ? top : 0), won(winners ? n : 0);
        std::vector<uint64_t> sum(n);
        for (size_t g = 0; g < n; ++g) order[g] = (uint32_t)g;
        auto size_of = [&](uint32_t g) { return (uint64_t)sketches[g].hashes.size(); };
        try {
            hip_check(skx_stream_enable_coverage(st), "screen");
            if (depth) hip_check(skx_stream_enable_depth(st), "screen");
            FastxReader reader(fastx);
            Batch b; std::string seq;
            size_t reads = 0;
            auto flush = [&]() {
                if (b.n() == 0) return;
                hip_check(skx_stream_push(st, b.bases.data(), b.offsets.data(), (uint32_t)b.n(), nullptr, nullptr, nullptr, nullptr, nullptr), "screen");
                b.clear();
            };
            while (reader.next(seq)) {
                if (b.n() && b.bases.size() + seq.size() > max_bases) flush();
                b.add(seq); ++reads;
                if (b.n() == batch_) flush();
                if (reads == limit) break;
            }
            flush();
            if (winners) hip_check(skx_stream_winners(st, covered.data(), won.data()), "screen");
            else hip_check(skx_stream_coverage(st, covered.data()), "screen");
            hip_check(skx_stream_table(st, sum.data()), "screen");
            // by containment = covered / size, compared as fractions (exact); an empty sketch contains nothing
            auto more_of = [&](const std::vector<uint32_t>& v, uint32_t x, uint32_t y) {
                return (uint64_t)v[x] * std::max<uint64_t>(size_of(y), 1) > (uint64_t)v[y] * std::max<uint64_t>(size_of(x), 1);
            };
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
                if (winners && (more_of(won, x, y) || more_of(won, y, x))) return more_of(won, x, y);
                return more_of(covered, x, y);
            });
            if (depth) hip_check(skx_stream_depth_rows(st, order.data(), (uint32_t)top, nullptr, median.data(), nullptr), "screen");
        } catch (...) {
            skx_stream_destroy(st);
            throw;
        }
        skx_stream_destroy(st);
        if (header)
            out << "sketch_id\tcovered\tsketch_size\tcontainment\tshared_hashes" << (winners ? "\twon\twinner_containment" : "")
                << (depth ? "\tmedian_multiplicity" : "") << (identity ? "\tidentity" : "")
                << (with_geno ? "\t" + geno.header : std::string()) << "\n";
        char buf[32];
        for (size_t j = 0; j < top; ++j) {
            const uint32_t g = order[j];
            const double containment = size_of(g) ? (double)covered[g] / (double)size_of(g) : 0.0;
            std::snprintf(buf, sizeof buf, "%.6f", containment);
            out << sketches[g].name << "\t" << covered[g] << "\t" << size_of(g) << "\t" << buf << "\t" << sum[g];
            const double won_containment = winners && size_of(g) ? (double)won[g] / (double)size_of(g) : 0.0;
            if (winners) {
                std::snprintf(buf, sizeof buf, "%.6f", won_containment);
                out << "\t" << won[g] << "\t" << buf;
            }
            if (depth) out << "\t" << median[j];
            if (identity) {
                std::snprintf(buf, sizeof buf, "%.6f", std::pow(winners ? won_containment : containment, 1.0 / (double)std::max<uint32_t>(sketches[g].kmer_length, 1u)));
                out << "\t" << buf;
            }
            if (with_geno) out << "\t" << join_tab(geno.map.at(sketches[g].name));
            out << "\n";
        }
    }

    // `composition` (not in the reference): what the read set is made of.  The references -- one species each, named by the file without
    // directory and .msh as in `predict` with several -r -- are resident together, all reads go through one table-only stream with
    // composition enabled (skx_stream_enable_composition), and every read is one species' (the one its own sketch shares the most hashes
    // with, at least min_hits), ambiguous (several species tie) or unclassified.  One line per reference -- species reads fraction pairs,
    // fraction = reads / all reads, pairs = hashes the reads shared with the species -- then the lines ambiguous and unclassified.
    // The files must agree in k-mer size and seed; the reads are sketched with the size of the first file's first sketch.
    void composition(const std::string& fastx, const std::vector<std::string>& references, uint32_t min_hits, size_t limit, bool header,
                     std::ostream& out) {
        // (there is no host route to the numbers: a library without the entry points ends here, before anything is read)
        auto need = [](bool have, const char* name) {
            if (!have) throw UsageError(std::string("composition needs ") + name + ", which the loaded libsketchy_hip does not export");
        };
        need(skx_stream_enable_composition != nullptr, "skx_stream_enable_composition");
        need(skx_stream_composition != nullptr, "skx_stream_composition");
        need(skx_ref_create_multi != nullptr, "skx_ref_create_multi");
        if (references.size() > SKX_MAX_SPECIES) throw UsageError("at most " + std::to_string(SKX_MAX_SPECIES) + " references can be resident together");
        std::vector<std::string> names;
        std::vector<std::vector<Sketch>> all;
        for (const auto& path : references) {
            auto sketches = read_sketch(path);
            if (sketches.empty()) throw SketchyError("reference sketch file " + path + " holds no sketches");
            const auto slash = path.find_last_of('/');
            std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
            if (name.size() > 4 && name.compare(name.size() - 4, 4, ".msh") == 0) name.resize(name.size() - 4);
            names.push_back(name);
            const Sketch &a = all.empty() ? sketches[0] : all[0][0], &b = sketches[0];
            if (a.kmer_length != b.kmer_length || a.hash_seed != b.hash_seed)
                throw UsageError("references " + references[0] + " and " + path + " do not agree in k-mer size and seed (" + std::to_string(a.kmer_length) +
                                 "/" + std::to_string(a.hash_seed) + " and " + std::to_string(b.kmer_length) + "/" + std::to_string(b.hash_seed) + ")");
            all.push_back(std::move(sketches));
        }
        Ref ref(all, device_);
        const size_t n_sp = all.size();
        const uint64_t max_bases = 1ull << 28;
        skx_stream* st = nullptr;
        hip_check(skx_stream_create(&st, ref.h, 0, (uint32_t)batch_, max_bases), "stream");
        std::vector<uint64_t> reads(n_sp + 2), pairs(n_sp);
        try {
            hip_check(skx_stream_enable_composition(st, min_hits), "composition");
            FastxReader reader(fastx);
            Batch b; std::string seq;
            size_t n = 0;
            auto flush = [&]() {
                if (b.n() == 0) return;
                hip_check(skx_stream_push(st, b.bases.data(), b.offsets.data(), (uint32_t)b.n(), nullptr, nullptr, nullptr, nullptr, nullptr), "composition");
                b.clear();
            };
            while (reader.next(seq)) {
                if (b.n() && b.bases.size() + seq.size() > max_bases) flush();
                b.add(seq); ++n;
                if (b.n() == batch_) flush();
                if (n == limit) break;
            }
            flush();
            hip_check(skx_stream_composition(st, reads.data(), pairs.data()), "composition");
        } catch (...) {
            skx_stream_destroy(st);
            throw;
        }
        skx_stream_destroy(st);
        uint64_t total = 0;
        for (uint64_t r : reads) total += r;
        if (header) out << "species\treads\tfraction\tpairs\n";
        char buf[32];
        for (size_t i = 0; i < n_sp + 2; ++i) {
            std::snprintf(buf, sizeof buf, "%.6f", total ? (double)reads[i] / (double)total : 0.0);
            out << (i < n_sp ? names[i] : i == n_sp ? std::string("ambiguous") : std::string("unclassified")) << "\t" << reads[i] << "\t" << buf << "\t";
            if (i < n_sp) out << pairs[i]; else out << "-";
            out << "\n";
        }
    }

    void info(const std::string& input, bool params, std::ostream& out) {
        const auto sk = read_sketch(input);
        if (sk.empty()) throw SketchyError("empty sketch file");
        if (params) { out << "type=mash sketch_size=" << sk[0].hashes.size() << " kmer_size=" << sk[0].kmer_length << " seed=" << sk[0].hash_seed << "\n"; return; }
        for (const auto& s : sk) out << s.name << " " << s.seq_length << " " << s.hashes.size() << "\n";
    }

    // `sketchy sketch` (src/sketchy.rs:128-167; _sketch_files :465-494): one Mash sketch per input FILE over all of its
    // records (k-mers never span records), name = file name (:484).  Whole files are batched, several per call, one group of
    // records per file: the device sketches every record (genomes take the block-per-read + segmented-sort path), pools the
    // rows of a group and counts its valid k-mers (skx_sketch_groups) -- one row of s hashes per file comes back.  A file
    // larger than a batch is cut at record boundaries and its per-batch rows are merged here.
    // want_counts (--counts): every hash's abundance as well (skx_sketch_groups_counts), written as the references' counts32; the
    // per-batch rows of a large file are merged with their counts (merge_counted).
    void sketch(const std::vector<std::string>& files, const std::string& output, size_t sketch_size, uint32_t kmer, uint64_t seed,
                bool want_counts = false) {
        const auto dot = output.rfind('.');
        const std::string ext = dot == std::string::npos ? "" : output.substr(dot + 1);
        if (ext == "fsh") throw SketchyError("Finch scaled sketches (.fsh) are outside the accelerated path");
        if (ext != "msh") throw SketchyError("output sketch file must have Mash (.msh) or Finch (.fsh) extension");  // :573-600
        if (sketch_size < 1) throw SketchyError("sketch size must be at least 1");
        if (sketch_size > 0xFFFFFFFFull) throw SketchyError("sketch size must fit 32 bits");
        if (kmer < 1 || kmer > SKX_MAX_K) throw SketchyError("k-mer size must be between 1 and " + std::to_string(SKX_MAX_K));
        if (seed > 0xFFFFFFFFull) throw SketchyError("the Mash format stores a 32-bit hash seed");
        if (want_counts && !skx_sketch_groups_counts)
            throw SketchyError("--counts needs skx_sketch_groups_counts, which the loaded libsketchy_hip does not export");
        constexpr size_t kBatchBases = 1ull << 30, kBatchRecords = 1ull << 22;
        std::vector<Sketch> out(files.size());
        Batch b; std::string seq;
        std::vector<uint32_t> first, len; std::vector<size_t> owner;  // group g of the batch = records [first[g], first[g + 1]) of file owner[g]
        std::vector<uint64_t> rows, valid, merged;
        std::vector<uint32_t> counts, merged_counts;
        auto flush = [&]() {
            if (owner.empty()) return;
            first.push_back((uint32_t)b.n());
            pool_groups(b, first, kmer, seed, (uint32_t)sketch_size, true, rows, len, valid, want_counts ? &counts : nullptr);
            for (size_t g = 0; g < owner.size(); ++g) {
                Sketch& sk = out[owner[g]];
                const uint64_t* row = rows.data() + g * sketch_size;
                sk.num_valid_kmers += valid[g];  // [UPSTREAM-RECALL] finch: k-mers pushed to the sketcher
                if (want_counts) {
                    const uint32_t* cnt = counts.data() + g * sketch_size;
                    if (sk.hashes.empty()) { sk.hashes.assign(row, row + len[g]); sk.counts.assign(cnt, cnt + len[g]); continue; }
                    merge_counted(sk.hashes.data(), sk.counts.data(), sk.hashes.size(), row, cnt, len[g], sketch_size, merged, merged_counts);
                    sk.hashes.swap(merged); sk.counts.swap(merged_counts);
                    continue;
                }
                if (sk.hashes.empty()) { sk.hashes.assign(row, row + len[g]); continue; }
                merged.clear();
                std::set_union(sk.hashes.begin(), sk.hashes.end(), row, row + len[g], std::back_inserter(merged));
                if (merged.size() > sketch_size) merged.resize(sketch_size);
                sk.hashes.swap(merged);
            }
            b.clear(); first.clear(); owner.clear();
        };
        for (size_t fi = 0; fi < files.size(); ++fi) {
            const auto& file = files[fi];
            FastxReader reader(file);
            Sketch& sk = out[fi];
            const auto slash = file.find_last_of('/');
            sk.name = slash == std::string::npos ? file : file.substr(slash + 1);
            sk.kmer_length = kmer; sk.hash_seed = seed;
            if (b.bases.size() >= kBatchBases) flush();
            owner.push_back(fi); first.push_back((uint32_t)b.n());
            while (reader.next(seq)) {
                sk.seq_length += seq.size();                       // [UPSTREAM-RECALL] finch: total bases of the records
                if (seq.size() >= (1ull << 32)) throw SketchyError("a record of " + file + " exceeds 4 Gbases");
                if (b.n() && (b.bases.size() + seq.size() > kBatchBases || b.n() >= kBatchRecords)) {
                    flush();
                    owner.push_back(fi); first.push_back(0);  // the file goes on in the next batch
                }
                b.add(seq);
            }
        }
        flush();
        write_mash_file(output, out, kmer, (uint32_t)seed);
    }
    // windows of k bases that are all A/C/G/T/U (any case), as needletail's normalize + canonical_kmers see them
    static uint64_t count_valid_kmers(const uint8_t* seq, size_t len, uint32_t k) {
        uint64_t n = 0; uint32_t run = 0;
        for (size_t i = 0; i < len; ++i) {
            const unsigned char c = seq[i];
            if (c == ' ' || c == '\t' || c == '\r' || c == '\n') continue;
            const unsigned char u = c & 0xDF;
            run = (u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'U') ? run + 1 : 0;
            if (run >= k) ++n;
        }
        return n;
    }

    static std::vector<Sketch> read_sketch(const std::string& path) {  // src/sketchy.rs:497-536
        const auto dot = path.rfind('.');
        const std::string ext = dot == std::string::npos ? "" : path.substr(dot + 1);
        if (ext == "msh") return read_mash_file(path);
        if (ext == "fsh") throw SketchyError("Finch scaled sketches (.fsh) are outside the accelerated path");
        throw SketchyError("reference sketch file must have Mash (.msh) or Finch (.fsh) extension");
    }

  private:
    struct Ref {  // the reference collection on the device
        skx_ref* h = nullptr; uint32_t k = 0, s = 0; uint64_t seed = 0;
        Ref(const std::vector<Sketch>& sk, int device) {
            k = sk[0].kmer_length; seed = sk[0].hash_seed;
            s = (uint32_t)sk[0].hashes.size();       // src/sketchy.rs:82 / :520-527: read sketch size := |sketch 0|
            uint32_t stride = s;
            for (const auto& x : sk) stride = std::max<uint32_t>(stride, (uint32_t)x.hashes.size());
            if (stride == 0) throw SketchyError("reference sketches are empty");
            std::vector<uint64_t> flat((size_t)stride * sk.size(), ~0ull);
            std::vector<uint32_t> len(sk.size());
            for (size_t g = 0; g < sk.size(); ++g) {
                std::copy(sk[g].hashes.begin(), sk[g].hashes.end(), flat.begin() + g * (size_t)stride);
                len[g] = (uint32_t)sk[g].hashes.size();
            }
            stride_ = stride;
            // columns may be longer than sketch 0; the read sketch size stays s (reference behaviour)
            if (s == 0) throw SketchyError("the first reference sketch is empty (it defines the read sketch size)");
            hip_check(skx_ref_create(&h, device, k, seed, s, stride, (uint32_t)sk.size(), flat.data(), len.data()), "reference upload");
        }
        // several files resident together (skx_ref_create_multi); the caller has checked that they agree in k, seed and |sketch 0|
        Ref(const std::vector<std::vector<Sketch>>& species, int device) {
            k = species[0][0].kmer_length; seed = species[0][0].hash_seed; s = (uint32_t)species[0][0].hashes.size();
            uint32_t stride = s;
            for (const auto& sk : species)
                for (const auto& x : sk) stride = std::max<uint32_t>(stride, (uint32_t)x.hashes.size());
            if (s == 0) throw SketchyError("the first reference sketch is empty (it defines the read sketch size)");
            std::vector<std::vector<uint64_t>> flat(species.size());
            std::vector<std::vector<uint32_t>> len(species.size());
            std::vector<uint32_t> n_genomes;
            std::vector<const uint64_t*> hp;
            std::vector<const uint32_t*> lp;
            for (size_t sp = 0; sp < species.size(); ++sp) {
                const auto& sk = species[sp];
                flat[sp].assign((size_t)stride * sk.size(), ~0ull);
                len[sp].resize(sk.size());
                for (size_t g = 0; g < sk.size(); ++g) {
                    std::copy(sk[g].hashes.begin(), sk[g].hashes.end(), flat[sp].begin() + g * (size_t)stride);
                    len[sp][g] = (uint32_t)sk[g].hashes.size();
                }
                n_genomes.push_back((uint32_t)sk.size()); hp.push_back(flat[sp].data()); lp.push_back(len[sp].data());
            }
            stride_ = stride;
            hip_check(skx_ref_create_multi(&h, device, k, seed, s, stride, (uint32_t)species.size(), n_genomes.data(), hp.data(), lp.data()),
                      "reference upload");
        }
        ~Ref() { skx_ref_destroy(h); }
        uint32_t stride_ = 0;
    };

    // --consensus on the device: every genotype column as a dictionary of its distinct strings in byte-wise sorted order (the order
    // of the std::map print_results votes in), a genome's code = its string's rank.  The library's tie rule -- the smallest code --
    // is then print_results' "first maximum of the map": the same bytes come out.
    struct ConsensusTable {
        bool on = false;
        size_t nfeat = 0, line_cap = 0;                // columns; bytes a line can take
        std::vector<std::vector<std::string>> values;  // [column][code]
    } cons_;
    void set_consensus_table(const std::vector<Sketch>& sketches, Ref& ref, const Genotypes& geno, const PredictConfig& config) {
        if (!skx_ref_set_genotypes || !skx_consensus_rows || !skx_stream_bind_consensus) return;  // (a library without them)
        if (config.top < 1 || config.top > SKX_MAX_TOP) return;
        const size_t nfeat = geno.map.at(sketches[0].name).size();
        if (nfeat < 1 || nfeat > SKX_MAX_FEATURES) return;
        std::vector<const std::vector<std::string>*> rows;
        for (const auto& sk : sketches) {
            rows.push_back(&geno.map.at(sk.name));
            if (rows.back()->size() != nfeat) return;  // (a ragged table: print_results decides what that means)
        }
        ConsensusTable t;
        t.nfeat = nfeat; t.line_cap = 32;
        std::vector<uint32_t> codes(rows.size() * nfeat);
        for (size_t j = 0; j < nfeat; ++j) {
            std::map<std::string, uint32_t> rank;
            for (const auto* r : rows) rank.emplace((*r)[j], 0u);
            std::vector<std::string> vals;
            size_t longest = 0;
            for (auto& kv : rank) { kv.second = (uint32_t)vals.size(); vals.push_back(kv.first); longest = std::max(longest, kv.first.size()); }
            for (size_t g = 0; g < rows.size(); ++g) codes[g * nfeat + j] = rank.at((*rows[g])[j]);
            t.values.push_back(std::move(vals));
            t.line_cap += longest + 1;
        }
        hip_check(skx_ref_set_genotypes(ref.h, (uint32_t)nfeat, codes.data()), "genotype table");
        t.on = true;
        cons_ = std::move(t);
    }
    // "<read>\t-\t-\t<call>\t...\n" from one read's codes; p has line_cap bytes of room
    char* put_consensus_line(char* p, size_t read, const uint32_t* codes) const {
        p = put_u64(p, read);
        memcpy(p, "\t-\t-\t", 5); p += 5;
        for (size_t j = 0; j < cons_.nfeat; ++j) {
            const std::string& v = cons_.values[j][codes[j]];
            memcpy(p, v.data(), v.size()); p += v.size();
            *p++ = j + 1 < cons_.nfeat ? '\t' : '\n';
        }
        return p;
    }

    struct Batch { std::vector<uint8_t> bases; std::vector<uint64_t> offsets{0}; size_t n() const { return offsets.size() - 1; }
                   void add(const std::string& seq) { bases.insert(bases.end(), seq.begin(), seq.end()); offsets.push_back(bases.size()); }
                   void clear() { bases.clear(); offsets.assign(1, 0); } };

    // One pooled bottom-s row per group of the batch's records (group g = records [first[g], first[g + 1])): rows [groups][s]
    // zero-padded, their lengths and -- want_valid -- the groups' valid k-mer windows.
    // counts (or NULL): the hashes' abundances [groups][s] as well; the caller has made sure the library has the counted entry point
    void pool_groups(const Batch& b, const std::vector<uint32_t>& first, uint32_t k, uint64_t seed, uint32_t s, bool want_valid,
                     std::vector<uint64_t>& rows, std::vector<uint32_t>& len, std::vector<uint64_t>& valid, std::vector<uint32_t>* counts = nullptr) {
        const size_t ng = first.size() - 1;
        rows.assign(ng * (size_t)s, 0); len.assign(ng, 0); valid.assign(ng, 0);
        if (counts) {
            counts->assign(ng * (size_t)s, 0);
            hip_check(skx_sketch_groups_counts(device_, k, seed, s, b.bases.data(), b.offsets.data(), (uint32_t)b.n(), first.data(), (uint32_t)ng,
                                               rows.data(), len.data(), want_valid ? valid.data() : nullptr, counts->data()), "sketch");
            return;
        }
        if (skx_sketch_groups) {
            hip_check(skx_sketch_groups(device_, k, seed, s, b.bases.data(), b.offsets.data(), (uint32_t)b.n(), first.data(), (uint32_t)ng,
                                        rows.data(), len.data(), want_valid ? valid.data() : nullptr), "sketch");
            return;
        }
        // a library without the pooled entry point: one row per record (at most 2^24 row entries per call), merged here
        const size_t step = std::max<size_t>(1, (1ull << 24) / s);
        std::vector<uint64_t> sk, pooled, merged; std::vector<uint32_t> sl;
        for (size_t g = 0; g < ng; ++g) {
            pooled.clear();
            for (size_t r0 = first[g]; r0 < first[g + 1]; r0 += step) {
                const size_t n = std::min<size_t>(step, first[g + 1] - r0);
                sk.assign(n * (size_t)s, 0); sl.assign(n, 0);
                hip_check(skx_sketch_reads(device_, k, seed, s, b.bases.data(), b.offsets.data() + r0, (uint32_t)n, sk.data(), sl.data()), "sketch");
                for (size_t r = 0; r < n; ++r) {
                    merged.clear();
                    std::set_union(pooled.begin(), pooled.end(), sk.begin() + r * s, sk.begin() + r * s + sl[r], std::back_inserter(merged));
                    if (merged.size() > s) merged.resize(s);
                    pooled.swap(merged);
                    if (want_valid) valid[g] += count_valid_kmers(b.bases.data() + b.offsets[r0 + r], b.offsets[r0 + r + 1] - b.offsets[r0 + r], k);
                }
            }
            std::copy(pooled.begin(), pooled.end(), rows.begin() + g * (size_t)s);
            len[g] = (uint32_t)pooled.size();
        }
    }

    // ---- streaming pipeline
    // one batch travelling parse -> device -> format and back: page-locked (skx_host_alloc) packed bases, offsets (in bases),
    // rows.  Slot i % n_slots carries chunk i: a parser waits for its slot to come back from the batch n_slots chunks before --
    // which only depends on OLDER chunks, so the ring cannot deadlock.
    struct Slot {
        uint8_t* packed = nullptr; uint64_t* offsets = nullptr; uint32_t* idx = nullptr; uint64_t* sum = nullptr;
        uint32_t* cons = nullptr;  // consensus on the device: [reads][columns] codes instead of rows
        // --changes with a library that lists a batch's change points: {n_events}, [cap] read ordinals, their rows or codes
        uint32_t *ev_n = nullptr, *ev_read = nullptr, *ev_idx = nullptr, *ev_codes = nullptr; uint64_t* ev_sum = nullptr;
        size_t n = 0, first_read = 1;
        // what did not fit the slot (a chunk with far more / longer reads than the first records promised): heap batches the
        // device thread sends through its spill slot, one by one (rare, slow, correct)
        struct Extra { std::vector<uint8_t> packed; std::vector<uint64_t> offsets{0}; };
        std::vector<Extra> extra;
        int state = 0;           // 0 free, 1 parsed
        bool last = false;       // the input ended in (or before) this chunk
    };
    static unsigned usable_threads() {
        unsigned n = std::max(1u, std::thread::hardware_concurrency());
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min<unsigned>(n, (unsigned)CPU_COUNT(&set));
        std::ifstream f("/sys/fs/cgroup/cpu.max");  // (the container's quota: hardware_concurrency reports the machine)
        std::string quota; long long period = 0;
        if (f >> quota >> period && quota != "max" && period > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, atoll(quota.c_str()) / period));
        return std::max(1u, n);
    }
    // --pin: keep the process on CPUs next to the device -- the first `want` of /sys/bus/pci/devices/<device>/local_cpulist.  The
    // parser threads fill page-locked buffers the device's DMA engines read, and on a two-socket box threads float over both
    // sockets.  Off by default: measured on the MI355X boxes (2 x EPYC 9575F, `predict -s` at C2) what matters more is that the
    // parsers sit next to the INPUT's pages -- 26 M reads/s with the whole job (the writer of the file included) on either
    // socket, 22 M floating, 18-22 M with only this process pinned to the device's node while the file's pages lay elsewhere.
    // Returns how many CPUs the process was confined to (0: nothing was changed).
    static unsigned pin_near_device(int device, unsigned want) {
        char bus[64] = {0};
        if (skx_device_pci_bus_id(device, bus, sizeof bus) != SKX_OK) return 0;
        std::string id(bus);
        for (auto& c : id) c = (char)tolower((unsigned char)c);
        std::ifstream f("/sys/bus/pci/devices/" + id + "/local_cpulist");
        std::string list;
        if (!(f >> list) || list.empty()) return 0;
        cpu_set_t allowed, set;
        if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return 0;
        CPU_ZERO(&set);
        unsigned n = 0;
        size_t i = 0;
        while (i < list.size() && n < want) {  // "0-63,128-191"
            size_t j = list.find(',', i);
            if (j == std::string::npos) j = list.size();
            const std::string part = list.substr(i, j - i);
            const size_t dash = part.find('-');
            const long a = atol(part.c_str()), b = dash == std::string::npos ? a : atol(part.c_str() + dash + 1);
            for (long c = a; c <= b && n < want; ++c)
                if (c >= 0 && c < CPU_SETSIZE && CPU_ISSET((int)c, &allowed)) { CPU_SET((int)c, &set); ++n; }
            i = j + 1;
        }
        if (n < 2 || sched_setaffinity(0, sizeof set, &set) != 0) return 0;
        return n;
    }
    static char* put_u64(char* p, uint64_t v) {  // decimal, no terminator; returns the end
        char tmp[24]; int n = 0;
        do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (n) *p++ = tmp[--n];
        return p;
    }

    // ---- several references: the species call
    struct Species {
        std::string name;  // the reference file's name without directory and .msh
        Genotypes geno;
        std::vector<std::string> mid, tail;            // rows: per genome "\t<species>\t<sketch>\t" and "\t<genotype columns>\n"
        size_t nfeat = 0;                              // consensus: the table's own columns ...
        std::vector<std::vector<std::string>> values;  // ... and their dictionaries [column][code]
    };
    // the text of one read's call: `top` row lines of the called species, or its consensus line (codes: padded to the widest table;
    // only the species' own columns are printed)
    static void put_call(std::string& text, const std::vector<Species>& species, const PredictConfig& config, size_t read, uint32_t sp,
                         const uint32_t* idx, const uint64_t* sum, const uint32_t* codes) {
        char num[48];
        const Species& s = species[sp];
        if (config.consensus) {
            text.append(num, (size_t)(put_u64(num, read) - num));
            text += '\t'; text += s.name; text += "\t-\t-";
            for (size_t j = 0; j < s.nfeat; ++j) { text += '\t'; text += s.values[j][codes[j]]; }
            text += '\n';
            return;
        }
        for (size_t t = 0; t < config.top; ++t) {
            text.append(num, (size_t)(put_u64(num, read) - num));
            text += s.mid[idx[t]];
            text.append(num, (size_t)(put_u64(num, sum[t]) - num));
            text += s.tail[idx[t]];
        }
    }
    // what --changes compares: everything the call prints but the read number and the sums
    static void call_key(std::string& key, const std::vector<Species>& species, const PredictConfig& config, uint32_t sp, const uint32_t* idx,
                         const uint32_t* codes) {
        key.assign(reinterpret_cast<const char*>(&sp), 4);
        if (config.consensus) { key.append(reinterpret_cast<const char*>(codes), species[sp].nfeat * 4); return; }
        for (size_t t = 0; t < config.top; ++t) { key += species[sp].mid[idx[t]]; key += species[sp].tail[idx[t]]; }
    }

    // streaming with several references: batches of -b reads through skx_stream_submit with the call bound and NO full rows -- 1 + top
    // values per read come back instead of species x top -- over a ring of page-locked slots, in file order on this thread (the parse
    // and format thread pools of the single-reference stream are not wired to this path).  --changes binds the call's event list
    // (4 096 entries per batch) and formats events only; a batch with more than that is formatted from its full call, which is
    // therefore bound to every batch in this mode too: 1 + top values per read still come back beside the events (an overflowing
    // batch cannot be asked for again -- the table has moved on).  A block is dropped when its printed call -- species included --
    // is the one printed last, across batches as within them.
    void call_stream(const std::string& path, const std::vector<Species>& species, Ref& ref, size_t nfeat, const PredictConfig& config,
                     std::ostream& out) {
        const size_t cap_reads = std::max<size_t>(1, batch_), cap_bases = std::max<size_t>(1u << 20, cap_reads * 1600), top = config.top;
        constexpr size_t kRing = 10;  // (one more than the batches the library holds between submit and rows: a wait returns at once)
        constexpr size_t kChangesCap = 4096;
        const size_t chg_cap = std::min(kChangesCap, cap_reads);
        skx_stream* st = nullptr;
        hip_check(skx_stream_create(&st, ref.h, (uint32_t)top, (uint32_t)cap_reads, cap_bases), "stream");
        struct Guard { skx_stream* s; ~Guard() { skx_stream_destroy(s); } } guard{st};
        struct CSlot {
            uint8_t* bases = nullptr; uint64_t* offsets = nullptr;
            uint32_t *sp = nullptr, *idx = nullptr, *codes = nullptr; uint64_t* sum = nullptr;
            uint32_t *ev_n = nullptr, *ev_read = nullptr, *ev_sp = nullptr, *ev_idx = nullptr, *ev_codes = nullptr; uint64_t* ev_sum = nullptr;
            size_t n = 0, first_read = 1; uint64_t ticket = 0; bool busy = false;
        };
        std::vector<CSlot> slots(kRing);
        struct SlotGuard { std::vector<CSlot>& s; int dev; ~SlotGuard() { for (auto& x : s) for (void* p : {(void*)x.bases, (void*)x.offsets, (void*)x.sp, (void*)x.idx, (void*)x.codes, (void*)x.sum, (void*)x.ev_n, (void*)x.ev_read, (void*)x.ev_sp, (void*)x.ev_idx, (void*)x.ev_codes, (void*)x.ev_sum}) if (p) skx_host_free(dev, p); } } sguard{slots, device_};
        auto pinned = [&](size_t bytes, const char* what) { void* p = nullptr; hip_check(skx_host_alloc(device_, &p, std::max<size_t>(bytes, 8)), what); return p; };
        for (auto& sl : slots) {
            sl.bases = static_cast<uint8_t*>(pinned(cap_bases, "batch buffer"));
            sl.offsets = static_cast<uint64_t*>(pinned((cap_reads + 1) * 8, "batch buffer"));
            sl.sp = static_cast<uint32_t*>(pinned(cap_reads * 4, "call buffer"));
            if (config.consensus) sl.codes = static_cast<uint32_t*>(pinned(cap_reads * nfeat * 4, "call buffer"));
            else { sl.idx = static_cast<uint32_t*>(pinned(cap_reads * top * 4, "call buffer")); sl.sum = static_cast<uint64_t*>(pinned(cap_reads * top * 8, "call buffer")); }
            if (config.changes) {
                sl.ev_n = static_cast<uint32_t*>(pinned(4, "event buffer"));
                sl.ev_read = static_cast<uint32_t*>(pinned(chg_cap * 4, "event buffer"));
                sl.ev_sp = static_cast<uint32_t*>(pinned(chg_cap * 4, "event buffer"));
                if (config.consensus) sl.ev_codes = static_cast<uint32_t*>(pinned(chg_cap * nfeat * 4, "event buffer"));
                else { sl.ev_idx = static_cast<uint32_t*>(pinned(chg_cap * top * 4, "event buffer")); sl.ev_sum = static_cast<uint64_t*>(pinned(chg_cap * top * 8, "event buffer")); }
            }
        }
        std::string text, key, prev_key;
        bool have_prev = false;
        // a finished batch as text, in file order
        auto emit = [&](CSlot& sl) {
            hip_check(skx_stream_wait(st, sl.ticket), "wait");
            sl.busy = false;
            text.clear();
            const bool events = config.changes && *sl.ev_n <= chg_cap;
            const size_t m = events ? *sl.ev_n : sl.n;
            for (size_t c = 0; c < m; ++c) {
                const size_t r = events ? sl.ev_read[c] : c;
                const uint32_t sp = events ? sl.ev_sp[c] : sl.sp[r];
                const uint32_t* ri = config.consensus ? nullptr : (events ? sl.ev_idx + c * top : sl.idx + r * top);
                const uint64_t* rs = config.consensus ? nullptr : (events ? sl.ev_sum + c * top : sl.sum + r * top);
                const uint32_t* rc = config.consensus ? (events ? sl.ev_codes + c * nfeat : sl.codes + r * nfeat) : nullptr;
                if (config.changes) {
                    call_key(key, species, config, sp, ri, rc);
                    if (have_prev && key == prev_key) continue;
                    prev_key = key; have_prev = true;
                }
                put_call(text, species, config, sl.first_read + r, sp, ri, rs, rc);
            }
            out.write(text.data(), (std::streamsize)text.size());
        };
        FastxReader reader(path);
        std::string seq;
        bool more = true, carried = false;  // carried: seq holds a record that did not fit the batch before
        size_t fed = 0, submitted = 0;
        while (more) {
            CSlot& sl = slots[submitted % kRing];
            if (sl.busy) emit(sl);
            size_t n = 0, bases = 0;
            sl.offsets[0] = 0;
            while (n < cap_reads && (!config.limit || fed + n < config.limit)) {
                if (!carried && !(more = reader.next(seq))) break;
                if (seq.size() > cap_bases) throw SketchyError("a record exceeds the batch buffer (" + std::to_string(cap_bases) + " bases): raise --batch");
                carried = bases + seq.size() > cap_bases;
                if (carried) break;
                memcpy(sl.bases + bases, seq.data(), seq.size());
                bases += seq.size();
                sl.offsets[++n] = bases;
            }
            if (config.limit && fed + n >= config.limit) more = false;  // src/sketchy.rs:350-353
            if (n == 0) break;
            sl.n = n; sl.first_read = fed + 1;
            hip_check(skx_stream_bind_call(st, sl.sp, sl.idx, sl.sum, sl.codes), "bind call");
            if (config.changes) hip_check(skx_stream_bind_call_changes(st, (uint32_t)chg_cap, sl.ev_n, sl.ev_read, sl.ev_sp, sl.ev_idx, sl.ev_sum, sl.ev_codes), "bind call changes");
            hip_check(skx_stream_submit(st, sl.bases, sl.offsets, (uint32_t)n, nullptr, nullptr, &sl.ticket), "submit");
            sl.busy = true;
            fed += n; ++submitted;
        }
        for (size_t k = 0; k < kRing; ++k) {  // what is still in the ring, oldest first
            CSlot& o = slots[(submitted + k) % kRing];
            if (o.busy) emit(o);
        }
        out.flush();
    }

    // offline with several references: one pooled sketch per sample, ranked against every species in one call (skx_rank_sketches is
    // multi-species already), the species selected by skx_call_rows with shared hashes as the sums
    void call_offline(const std::vector<std::string>& paths, const std::vector<Species>& species, Ref& ref, size_t nfeat,
                      const PredictConfig& config, std::ostream& out) {
        const size_t n = paths.size(), n_sp = species.size(), top = config.top;
        std::vector<std::vector<uint64_t>> pooled(n);
        std::vector<size_t> reads(n, 0);
        pool_samples(paths, ref, config, pooled, reads);
        size_t stride = 1;
        for (const auto& p : pooled) stride = std::max(stride, p.size());
        std::vector<uint64_t> flat(n * stride, 0);
        std::vector<uint32_t> plen(n);
        for (size_t f = 0; f < n; ++f) { std::copy(pooled[f].begin(), pooled[f].end(), flat.begin() + f * stride); plen[f] = (uint32_t)pooled[f].size(); }
        std::vector<uint32_t> idx(n * n_sp * top), shared(n * n_sp * top), codes;
        hip_check(skx_rank_sketches(ref.h, flat.data(), plen.data(), (uint32_t)n, (uint32_t)stride, (uint32_t)top, idx.data(), shared.data(), nullptr), "rank");
        std::vector<uint64_t> sums(shared.begin(), shared.end());
        if (config.consensus) {
            codes.resize(n * n_sp * nfeat);
            hip_check(skx_consensus_rows(ref.h, idx.data(), n, (uint32_t)top, codes.data()), "consensus");
        }
        std::vector<uint32_t> c_sp(n), c_idx(n * top), c_codes(config.consensus ? n * nfeat : 0);
        std::vector<uint64_t> c_sum(n * top);
        hip_check(skx_call_rows(device_, idx.data(), sums.data(), config.consensus ? codes.data() : nullptr, n, (uint32_t)n_sp, (uint32_t)top,
                                (uint32_t)nfeat, c_sp.data(), c_idx.data(), c_sum.data(), config.consensus ? c_codes.data() : nullptr), "call");
        std::string text;
        for (size_t f = 0; f < n; ++f)
            put_call(text, species, config, reads[f], c_sp[f], c_idx.data() + f * top, c_sum.data() + f * top, config.consensus ? c_codes.data() + f * nfeat : nullptr);
        out.write(text.data(), (std::streamsize)text.size());
    }

    // streaming mode
    void sum_of_shared_hashes(const std::string& path, const std::vector<Sketch>& sketches, Ref& ref, const Genotypes& geno,
                              const PredictConfig& config, std::ostream& out) {
        using clock = std::chrono::steady_clock;
        const auto t_begin = clock::now();
        MappedFile map;
        // (a BGZF file -- gzip members with their sizes in the header -- is inflated by all threads at once and then cut and parsed
        // like an uncompressed one; plain gzip is one sequential stream)
        const bool mapped = map.open(path) || map.open_bgzf(path, config.threads ? (unsigned)config.threads : std::min(usable_threads(), 22u));
        const double open_s = std::chrono::duration<double>(clock::now() - t_begin).count();  // mapping the input (BGZF: inflating all of it)
        if (mapped && map.inflated() && !map.eof_marker)
            fprintf(stderr, "sketchy-hip: warning: %s does not end with BGZF's end-of-file block (truncated at a block boundary?)\n", path.c_str());
        const char *fbegin = mapped ? map.data() : nullptr, *fend = mapped ? map.data() + map.size() : nullptr;
        bool fastq = false;
        size_t chunk_bytes = 0;
        std::vector<size_t> cuts;  // chunk i = [cuts[i], cuts[i + 1]) of the mapped file
        const size_t want_reads = std::max<size_t>(1, batch_);
        // Threads: every parser / formatter thread owns a page-locked slot (~100 MB at the default batch of 65 536 x 1.5 kb FASTQ), and the
        // front-end saturates at 12-16 parsers (tools/frontend_rate.sh) -- an unrestricted 256-thread host must not page-lock 27 GB before
        // its first read.  Without -j: at most kAutoThreads; with -j: what was asked for, the parsers still capped at kMaxParsers.
        constexpr unsigned kAutoThreads = 22, kMaxParsers = 32;
        const unsigned hw = config.threads ? (unsigned)config.threads : std::min(usable_threads(), kAutoThreads);
        const unsigned n_format = std::max(1u, std::min(4u, hw / 4));
        const unsigned n_parse = mapped ? std::min(kMaxParsers, std::max(1u, hw > n_format + 2 ? hw - n_format - 2 : 1u)) : 1u;
        const unsigned pinned = config.pin ? pin_near_device(device_, std::max(hw, 2u)) : 0u;
        if (mapped) {
            const char* p = fbegin;
            while (p < fend && (*p == '\n' || *p == '\r')) ++p;
            if (p < fend && *p != '@' && *p != '>') throw SketchyError("input is neither FASTA nor FASTQ");
            fastq = p < fend && *p == '@';
            // bytes per record from the first records; chunks of ~batch records, cut at record boundaries
            size_t n0 = 0; const char* q = p;
            while (q < fend && n0 < 64) { const char* nx = next_record_start(fbegin, q + 1, fend, fastq); ++n0; q = nx; }
            const size_t per = n0 ? std::max<size_t>(4, (size_t)(q - p) / n0) : 4;
            chunk_bytes = std::max<size_t>(64, per * want_reads);
            cuts.push_back((size_t)(p - fbegin));
            while (cuts.back() < map.size()) {
                // (the first chunks grow from 1 / n_parse of a batch to a whole one: the parser threads all start at once, and with
                // equal chunks they would all hand over their first batch at the same moment, a whole chunk's parse time in)
                const size_t k = cuts.size() - 1;
                const size_t this_chunk = k < n_parse ? std::max<size_t>(64, chunk_bytes * (k + 1) / n_parse) : chunk_bytes;
                const size_t nominal = cuts.back() + this_chunk;
                const size_t nx = nominal >= map.size() ? map.size() : (size_t)(next_record_start(fbegin, fbegin + nominal, fend, fastq) - fbegin);
                cuts.push_back(std::max(nx, cuts.back() + 1));
            }
        } else {
            chunk_bytes = std::max<size_t>(64, (size_t)3200 * want_reads);  // (what a batch may hold: reads x a long-read-ish record)
        }
        const size_t cap_reads = 2 * want_reads + 64;            // a slot's reads ...
        size_t cap_bases = std::max<size_t>(chunk_bytes, 1u << 16);  // ... and bases: a chunk holds fewer bases than bytes, so a mapped
        for (size_t i = 0; i + 1 < cuts.size(); ++i) cap_bases = std::max(cap_bases, cuts[i + 1] - cuts[i]);  // chunk always fits
        if (cap_bases >= (1ull << 32) - 64) throw SketchyError("a record of the input exceeds what one batch can hold (4 Gbases)");
        const size_t n_chunks = mapped ? cuts.size() - 1 : (size_t)-1;

        constexpr size_t kInFlight = 9;  // batches the library holds between submit and rows (its staging slots: 2 x 4 + 1)
        const size_t n_slots = kInFlight + n_parse + n_format + 2;

        skx_stream* st = nullptr;
        hip_check(skx_stream_create(&st, ref.h, (uint32_t)config.top, (uint32_t)cap_reads, cap_bases), "stream");
        struct Guard { skx_stream* s; ~Guard() { skx_stream_destroy(s); } } guard{st};
        hip_check(skx_stream_set_packed_input(st, 1), "packed input");

        std::vector<Slot> slots(n_slots + 1);  // (+ the device thread's spill slot)
        struct SlotGuard { std::vector<Slot>& s; int dev; ~SlotGuard() { for (auto& x : s) { for (void* p : {(void*)x.packed, (void*)x.offsets, (void*)x.idx, (void*)x.sum, (void*)x.cons, (void*)x.ev_n, (void*)x.ev_read, (void*)x.ev_idx, (void*)x.ev_sum, (void*)x.ev_codes}) if (p) skx_host_free(dev, p); } } } sguard{slots, device_};
        const bool dev_cons = config.consensus && cons_.on;  // one code per column and read comes back, no rows
        const size_t rows_cap = dev_cons ? 0 : cap_reads * config.top;
        // --changes: the library lists the change points of every batch (skx_stream_bind_changes; one per batch, the first read always
        // among them) and the formatters turn only those into text.  kChangesCap entries per batch: the near-tie stream of the tests
        // changes its top-64 row at 24 % of its reads and its top-1 row at 2 %, a sample that has found its strain a handful of times
        // per million -- 4 096 holds a quarter of a 16 384-read batch and costs top x 12 bytes x 4 096 (3 MB at top 64) of page-locked
        // memory per slot.  A batch with more change points than that is filtered on the host from its full rows, which therefore keep
        // coming back; so is every batch of a library without the entry point.
        constexpr size_t kChangesCap = 4096;
        const size_t chg_cap = std::min(kChangesCap, cap_reads);
        const bool dev_chg = config.changes && skx_stream_bind_changes;
        for (auto& sl : slots) {
            void* p = nullptr;
            hip_check(skx_host_alloc(device_, &p, cap_bases / 2 + 64), "batch buffer"); sl.packed = static_cast<uint8_t*>(p);
            hip_check(skx_host_alloc(device_, &p, (cap_reads + 1) * 8), "batch buffer"); sl.offsets = static_cast<uint64_t*>(p);
            hip_check(skx_host_alloc(device_, &p, std::max<size_t>(rows_cap, 1) * 4), "row buffer"); sl.idx = static_cast<uint32_t*>(p);
            hip_check(skx_host_alloc(device_, &p, std::max<size_t>(rows_cap, 1) * 8), "row buffer"); sl.sum = static_cast<uint64_t*>(p);
            if (dev_cons) { hip_check(skx_host_alloc(device_, &p, cap_reads * cons_.nfeat * 4), "consensus buffer"); sl.cons = static_cast<uint32_t*>(p); }
            if (dev_chg && &sl != &slots[n_slots]) {  // (the spill slot's batches are filtered from their full rows)
                hip_check(skx_host_alloc(device_, &p, 4), "event buffer"); sl.ev_n = static_cast<uint32_t*>(p);
                hip_check(skx_host_alloc(device_, &p, chg_cap * 4), "event buffer"); sl.ev_read = static_cast<uint32_t*>(p);
                if (dev_cons) { hip_check(skx_host_alloc(device_, &p, chg_cap * cons_.nfeat * 4), "event buffer"); sl.ev_codes = static_cast<uint32_t*>(p); }
                else {
                    hip_check(skx_host_alloc(device_, &p, chg_cap * config.top * 4), "event buffer"); sl.ev_idx = static_cast<uint32_t*>(p);
                    hip_check(skx_host_alloc(device_, &p, chg_cap * config.top * 8), "event buffer"); sl.ev_sum = static_cast<uint64_t*>(p);
                }
            }
        }
        Slot& spill = slots[n_slots];

        std::mutex mu;  // slot states, queues, the error
        std::condition_variable cv_parsed, cv_free, cv_format;
        std::exception_ptr error;
        bool stop = false;  // an error, or the limit was reached: nobody starts anything new
        auto fail_with = [&](std::exception_ptr e) { std::lock_guard<std::mutex> l(mu); if (!error) error = e; stop = true; cv_parsed.notify_all(); cv_free.notify_all(); cv_format.notify_all(); };

        // ---- stage 1: parse + pack
        // record sink of one chunk: the slot while it has room, heap batches behind it
        auto parse_into = [&](Slot& sl, auto&& walk) {
            sl.n = 0; sl.extra.clear(); sl.offsets[0] = 0;
            uint64_t pos = 0;              // nibbles written to the current target
            bool in_extra = false;
            auto cur_packed = [&]() -> uint8_t* { return in_extra ? sl.extra.back().packed.data() : sl.packed; };
            size_t open_len = 0;           // bases of the record being assembled (multi-line FASTA)
            walk([&](const char* piece, size_t len, bool last_piece) {
                // room for the record's next piece?  (a record that alone exceeds a batch cannot be scored by this stream)
                const size_t n_now = in_extra ? sl.extra.back().offsets.size() - 1 : sl.n;
                if (open_len + len > cap_bases) throw SketchyError("a record exceeds the batch buffer (" + std::to_string(cap_bases) + " bases): raise --batch");
                if (pos + len > cap_bases || (open_len == 0 && n_now >= cap_reads)) {
                    // move on to a fresh heap batch; the open record's pieces so far move with it
                    Slot::Extra e; e.packed.assign(cap_bases / 2 + 64, 0);
                    const uint64_t rec0 = pos - open_len;
                    if (open_len) {  // re-pack the open record's nibbles at the front of the new batch
                        const uint8_t* src = cur_packed();
                        for (uint64_t i = 0; i < open_len; ++i) {
                            const uint8_t c = (uint8_t)((src[(rec0 + i) >> 1] >> (4 * ((rec0 + i) & 1))) & 0xF);
                            uint8_t& b = e.packed[i >> 1];
                            b = (i & 1) ? (uint8_t)((b & 0x0F) | (c << 4)) : c;
                        }
                    }
                    sl.extra.push_back(std::move(e));
                    in_extra = true; pos = open_len;
                }
                pos = skx_pack_bases(reinterpret_cast<const uint8_t*>(piece), len, cur_packed(), pos);
                open_len += len;
                if (last_piece) {
                    // (whitespace inside a piece is dropped by the packer: the offset is what was really written)
                    if (in_extra) sl.extra.back().offsets.push_back(pos);
                    else sl.offsets[++sl.n] = pos;
                    open_len = 0;
                }
            });
        };
        // a chunk of the mapped file [a, b): one pass per sequence line -- skx_pack_line finds its end and packs it.  The slot
        // cannot run out of BASES (it holds as many as the longest chunk has bytes); when it runs out of READS the rest of the
        // chunk goes to heap batches, each with the same room.  Errors are FastxReader's, at the same records.
        auto parse_mapped = [&](Slot& sl, const char* a, const char* b) {
            sl.n = 0; sl.extra.clear(); sl.offsets[0] = 0;
            uint8_t* target = sl.packed;
            uint64_t pos = 0;
            size_t n_here = 0;
            auto begin_record = [&] {
                if (n_here < cap_reads) return;
                Slot::Extra e; e.packed.assign(cap_bases / 2 + 64, 0);
                sl.extra.push_back(std::move(e));
                target = sl.extra.back().packed.data(); pos = 0; n_here = 0;
            };
            auto end_record = [&] {
                if (sl.extra.empty()) sl.offsets[++sl.n] = pos; else sl.extra.back().offsets.push_back(pos);
                ++n_here;
            };
            auto lf = [&](const char* q) { return static_cast<const char*>(memchr(q, '\n', (size_t)(b - q))); };
            const char* p = a;
            size_t stride = 0;  // length of the previous record
            static const bool guess_next = !getenv("SKETCHY_HIP_NO_PREFETCH");  // (measurement aid, like SKETCHY_HIP_NO_POPULATE)
            while (p < b) {
                if (*p == '\n' || *p == '\r') { ++p; continue; }
                if (fastq) {
                    if (*p != '@') throw SketchyError("input is neither FASTA nor FASTQ");
                    // The quality line is skipped, so every record starts with cache misses the hardware prefetcher cannot see
                    // coming: the byte that ends this record, the next header, the first lines of its sequence.  Records of one
                    // file mostly have one length (short-read instruments: exactly), so the previous record's length says where
                    // they are: requested now, they arrive while this record's sequence is packed.  A wrong guess costs five
                    // useless prefetches.
                    if (stride && guess_next && (size_t)(b - p) > stride + 320) {
                        const char* nx = p + stride;
                        for (int i = -64; i < 320; i += 64) __builtin_prefetch(nx + i, 0, 1);
                    }
                    const char* const rec0 = p;
                    const char* e0 = lf(p);
                    if (!e0 || e0 + 1 >= b) throw SketchyError("truncated FASTQ record");
                    const char* s0 = e0 + 1;
                    begin_record();
                    uint64_t used = 0;
                    const uint64_t pos1 = skx_pack_line(reinterpret_cast<const uint8_t*>(s0), (uint64_t)(b - s0), target, pos, &used);
                    if (used == 0 || s0[used - 1] != '\n') throw SketchyError("malformed FASTQ record (no '+' line)");
                    const char* plus = s0 + used;
                    if (plus >= b || *plus != '+') throw SketchyError("malformed FASTQ record (no '+' line)");
                    const char* e2 = (plus + 1 < b && plus[1] == '\n') ? plus + 1 : lf(plus);
                    if (!e2 || e2 + 1 >= b) throw SketchyError("truncated FASTQ record");
                    const char* q0 = e2 + 1;
                    const size_t line = (size_t)used - 1;  // (the quality line is as long as the sequence line: a byte test, not a scan)
                    const char* e3 = ((size_t)(b - q0) > line && q0[line] == '\n') ? q0 + line : lf(q0);
                    pos = pos1;
                    end_record();
                    p = e3 ? e3 + 1 : b;
                    stride = (size_t)(p - rec0);
                } else {
                    if (*p != '>') throw SketchyError("input is neither FASTA nor FASTQ");
                    const char* e0 = lf(p);
                    const char* q = e0 ? e0 + 1 : b;
                    begin_record();
                    while (q < b && *q != '>') {
                        uint64_t used = 0;
                        pos = skx_pack_line(reinterpret_cast<const uint8_t*>(q), (uint64_t)(b - q), target, pos, &used);
                        q += used;
                    }
                    end_record();
                    p = q;
                }
            }
        };
        std::atomic<size_t> next_chunk{0};
        std::vector<std::thread> parsers;
        std::vector<size_t> slot_gen(n_slots, 0);  // chunks a slot has carried so far: slot s is free for chunk c when slot_gen[s] == c / n_slots
        auto wait_slot = [&](size_t c) -> Slot* {
            const size_t s = c % n_slots;
            std::unique_lock<std::mutex> l(mu);
            cv_free.wait(l, [&] { return stop || (slots[s].state == 0 && slot_gen[s] == c / n_slots); });
            return stop ? nullptr : &slots[s];
        };
        auto publish = [&](Slot& sl, bool last) { { std::lock_guard<std::mutex> l(mu); sl.state = 1; sl.last = last; } cv_parsed.notify_all(); };
        if (mapped) {
            for (unsigned t = 0; t < n_parse; ++t)
                parsers.emplace_back([&] {
                    try {
                        for (;;) {
                            const size_t c = next_chunk.fetch_add(1);
                            if (c >= n_chunks) {
                                if (c == n_chunks) { Slot* sl = wait_slot(c); if (sl) { sl->n = 0; sl->extra.clear(); publish(*sl, true); } }  // the end marker
                                return;
                            }
                            Slot* sl = wait_slot(c);
                            if (!sl) return;
                            const char *a = fbegin + cuts[c], *b = fbegin + cuts[c + 1];
                            if (!getenv("SKETCHY_HIP_NO_POPULATE")) map.prefetch(cuts[c], cuts[c + 1]);  // (the chunk's pages in one call instead of a fault every 4 KB)
                            parse_mapped(*sl, a, b);
                            publish(*sl, false);
                        }
                    } catch (...) { fail_with(std::current_exception()); }
                });
        } else {
            parsers.emplace_back([&] {  // gzip / stdin: one sequential reader, batches of `batch_` reads
                try {
                    FastxReader reader(path);
                    std::string seq;
                    bool more = true;
                    for (size_t c = 0; more; ++c) {
                        Slot* sl = wait_slot(c);
                        if (!sl) return;
                        size_t bases = 0, n = 0;
                        parse_into(*sl, [&](auto&& emit) {
                            while (n < want_reads && bases < cap_bases / 2 && (more = reader.next(seq))) { emit(seq.data(), seq.size(), true); ++n; bases += seq.size(); }
                        });
                        if (!more && sl->n == 0 && sl->extra.empty()) { publish(*sl, true); return; }
                        publish(*sl, false);
                        if (!more) { Slot* e = wait_slot(c + 1); if (e) { e->n = 0; e->extra.clear(); publish(*e, true); } return; }
                    }
                } catch (...) { fail_with(std::current_exception()); }
            });
        }

        // ---- stage 3 + 4: rows as text, written in order
        struct Job { Slot* sl = nullptr; size_t seq = 0, n = 0, first_read = 1; uint64_t ticket = 0; std::vector<uint32_t> idx, cons; std::vector<uint64_t> sum;
                     bool events = false; /* the slot holds the batch's event list */ };
        std::deque<Job> format_q;
        bool format_closed = false;
        // seq -> text, waiting for its turn.  --changes: the text opens with the block of the batch's FIRST read (first_len bytes), which
        // the writer drops when that read's call (first_key) is the call the batch before ended with (last_key)
        struct Done { std::string text, first_key, last_key; size_t first_len = 0; };
        std::map<size_t, Done> done_text;
        std::string prev_key; bool have_prev = false;
        size_t next_write = 0;
        std::mutex write_mu;
        std::vector<std::string> mid, tail;  // per reference sketch: "\t<name>\t" and "\t<genotype columns>\n"
        if (!config.consensus)
            for (const auto& sk : sketches) { mid.push_back("\t" + sk.name + "\t"); tail.push_back("\t" + join_tab(geno.map.at(sk.name)) + "\n"); }
        // --changes, rows: two genomes print the same lines (but for the sums) iff they share name and genotype -- line_class[g]
        std::vector<uint32_t> line_class;
        if (config.changes && !config.consensus) {
            std::map<std::string, uint32_t> seen;
            for (size_t g = 0; g < sketches.size(); ++g) line_class.push_back(seen.emplace(mid[g] + tail[g], (uint32_t)g).first->second);
        }
        auto release_slot = [&](Slot* sl) { { std::lock_guard<std::mutex> l(mu); sl->state = 0; slot_gen[(size_t)(sl - slots.data())] += 1; } cv_free.notify_all(); };
        std::vector<std::thread> formatters;
        for (unsigned t = 0; t < n_format; ++t)
            formatters.emplace_back([&] {
                try {
                    for (;;) {
                        Job job;
                        {
                            std::unique_lock<std::mutex> l(mu);
                            cv_format.wait(l, [&] { return !format_q.empty() || format_closed || (bool)error; });
                            if (format_q.empty()) return;
                            job = std::move(format_q.front()); format_q.pop_front();
                        }
                        const uint32_t* idx = job.sl ? job.sl->idx : job.idx.data();
                        const uint64_t* sum = job.sl ? job.sl->sum : job.sum.data();
                        std::string text;
                        Done done;
                        if (config.changes) {
                            // the reads whose call may differ from the call before them: the library's events, or every read
                            const uint32_t* codes = dev_cons ? (job.sl ? job.sl->cons : job.cons.data()) : nullptr;
                            const bool events = job.events && *job.sl->ev_n <= chg_cap;
                            const size_t m = events ? *job.sl->ev_n : job.n;
                            std::string key, last, block;
                            std::ostringstream os;
                            for (size_t c = 0; c < m; ++c) {
                                const size_t r = events ? job.sl->ev_read[c] : c;
                                const uint32_t* ri = events ? (dev_cons ? nullptr : job.sl->ev_idx + c * config.top) : (dev_cons ? nullptr : idx + r * config.top);
                                const uint64_t* rs = events ? (dev_cons ? nullptr : job.sl->ev_sum + c * config.top) : (dev_cons ? nullptr : sum + r * config.top);
                                const uint32_t* rc = dev_cons ? (events ? job.sl->ev_codes + c * cons_.nfeat : codes + r * cons_.nfeat) : nullptr;
                                block.clear();
                                if (dev_cons) {
                                    key.assign(reinterpret_cast<const char*>(rc), cons_.nfeat * 4);
                                } else if (config.consensus) {  // (a library without the vote: the line itself, behind the read number)
                                    os.str(std::string());
                                    print_results(sketches, geno, ri, rs, job.first_read + r, config, os);
                                    block = os.str();
                                    key = block.substr(block.find('\t'));
                                } else {
                                    key.resize(config.top * 4);
                                    for (size_t t2 = 0; t2 < config.top; ++t2) memcpy(&key[t2 * 4], &line_class[ri[t2]], 4);
                                }
                                if (c == 0) done.first_key = key;
                                else if (key == last) continue;
                                last = key;
                                if (dev_cons) {
                                    block.resize(cons_.line_cap);
                                    block.resize((size_t)(put_consensus_line(block.data(), job.first_read + r, rc) - block.data()));
                                } else if (!config.consensus) {
                                    for (size_t t2 = 0; t2 < config.top; ++t2) {
                                        const uint32_t g = ri[t2];
                                        char num[48];
                                        block.append(num, (size_t)(put_u64(num, job.first_read + r) - num));
                                        block += mid[g];
                                        block.append(num, (size_t)(put_u64(num, rs[t2]) - num));
                                        block += tail[g];
                                    }
                                }
                                text += block;
                                if (c == 0) done.first_len = text.size();
                            }
                            done.last_key = last;
                        } else if (dev_cons) {
                            const uint32_t* codes = job.sl ? job.sl->cons : job.cons.data();
                            text.resize(job.n * cons_.line_cap);
                            char* p = text.data();
                            for (size_t r = 0; r < job.n; ++r) p = put_consensus_line(p, job.first_read + r, codes + r * cons_.nfeat);
                            text.resize((size_t)(p - text.data()));
                        } else if (config.consensus) {
                            std::ostringstream os;
                            for (size_t r = 0; r < job.n; ++r) print_results(sketches, geno, idx + r * config.top, sum + r * config.top, job.first_read + r, config, os);
                            text = os.str();
                        } else {
                            size_t need = 0;
                            for (size_t i = 0; i < job.n * config.top; ++i) need += 42 + mid[idx[i]].size() + tail[idx[i]].size();
                            text.resize(need);
                            char* p = text.data();
                            for (size_t r = 0; r < job.n; ++r)
                                for (size_t t2 = 0; t2 < config.top; ++t2) {
                                    const uint32_t g = idx[r * config.top + t2];
                                    p = put_u64(p, job.first_read + r);
                                    memcpy(p, mid[g].data(), mid[g].size()); p += mid[g].size();
                                    p = put_u64(p, sum[r * config.top + t2]);
                                    memcpy(p, tail[g].data(), tail[g].size()); p += tail[g].size();
                                }
                            text.resize((size_t)(p - text.data()));
                        }
                        if (job.sl) release_slot(job.sl);  // the rows are text now: the slot goes back to the parsers
                        std::lock_guard<std::mutex> w(write_mu);
                        done.text = std::move(text);
                        done_text.emplace(job.seq, std::move(done));
                        for (auto it = done_text.find(next_write); it != done_text.end(); it = done_text.find(next_write)) {
                            const Done& d = it->second;
                            const size_t skip = (config.changes && have_prev && d.first_key == prev_key) ? d.first_len : 0;
                            out.write(d.text.data() + skip, (std::streamsize)(d.text.size() - skip));
                            if (config.changes) { prev_key = d.last_key; have_prev = true; }
                            done_text.erase(it); ++next_write;
                        }
                    }
                } catch (...) { fail_with(std::current_exception()); }
            });

        // ---- stage 2: the device, in file order (this thread)
        size_t fed = 0, n_batches = 0, seq_no = 0;
        const auto t_first = clock::now();  // (the parsers have just been started: everything before was set-up)
        double s_wait_parse = 0, s_submit = 0, s_retire = 0;  // where this thread's time goes (--timing)
        auto since = [](clock::time_point t) { return std::chrono::duration<double>(clock::now() - t).count(); };
        try {
            std::deque<std::pair<Slot*, Job>> in_flight;  // submitted, rows not yet known to be on the host
            auto hand_to_format = [&](Job&& j) { { std::lock_guard<std::mutex> l(mu); format_q.push_back(std::move(j)); } cv_format.notify_one(); };
            // the library holds up to kInFlight batches between submit and rows (a submit first finishes the batch that last used
            // its staging slot): everything older is through, and skx_stream_wait on it returns at once -- waiting on a YOUNGER
            // ticket would cut its group short
            auto retire = [&](size_t keep) {
                while (in_flight.size() > keep) {
                    hip_check(skx_stream_wait(st, in_flight.front().second.ticket), "wait");
                    hand_to_format(std::move(in_flight.front().second)); in_flight.pop_front();
                }
            };
            bool limit_hit = false;
            for (size_t c = 0; !limit_hit; ++c) {
                Slot* sl = &slots[c % n_slots];
                {
                    const auto tw = clock::now();
                    std::unique_lock<std::mutex> l(mu);
                    cv_parsed.wait(l, [&] { return stop || (sl->state == 1 && slot_gen[c % n_slots] == c / n_slots); });
                    s_wait_parse += since(tw);
                    if (stop) break;
                }
                const bool last = sl->last;
                auto submit = [&](const uint8_t* packed, const uint64_t* offsets, size_t n, uint32_t* idx, uint64_t* sum, uint32_t* cons, Slot* owner) {
                    if (config.limit && fed + n >= config.limit) { n = config.limit - fed; limit_hit = true; }  // src/sketchy.rs:350-353
                    if (n == 0) { if (owner) release_slot(owner); return; }
                    uint64_t ticket = 0;
                    const auto ts = clock::now();
                    if (dev_cons) hip_check(skx_stream_bind_consensus(st, cons), "bind consensus");
                    const bool events = dev_chg && owner && owner->ev_n;
                    if (events) hip_check(skx_stream_bind_changes(st, (uint32_t)chg_cap, owner->ev_n, owner->ev_read, owner->ev_idx, owner->ev_sum, owner->ev_codes), "bind changes");
                    hip_check(skx_stream_submit(st, packed, offsets, (uint32_t)n, dev_cons ? nullptr : idx, dev_cons ? nullptr : sum, &ticket), "submit");
                    s_submit += since(ts);
                    Job j; j.sl = owner; j.seq = seq_no++; j.n = n; j.first_read = fed + 1; j.ticket = ticket; j.events = events;
                    fed += n; ++n_batches;
                    in_flight.emplace_back(owner, std::move(j));
                    const auto tr = clock::now();
                    retire(kInFlight);
                    s_retire += since(tr);
                };
                std::vector<Slot::Extra> extra;
                extra.swap(sl->extra);
                submit(sl->packed, sl->offsets, sl->n, sl->idx, sl->sum, sl->cons, sl);
                for (auto& e : extra) {  // the chunk's overflow, through the spill slot: drained each time (rare path)
                    if (limit_hit) break;
                    const size_t n = e.offsets.size() - 1;
                    memcpy(spill.packed, e.packed.data(), std::min(e.packed.size(), cap_bases / 2 + 64));
                    memcpy(spill.offsets, e.offsets.data(), e.offsets.size() * 8);
                    submit(spill.packed, spill.offsets, n, spill.idx, spill.sum, spill.cons, nullptr);
                    hip_check(skx_stream_drain(st), "drain");
                    Job& j = in_flight.back().second;  // its rows leave the spill slot before the next overflow batch uses it
                    if (dev_cons) j.cons.assign(spill.cons, spill.cons + j.n * cons_.nfeat);
                    else { j.idx.assign(spill.idx, spill.idx + j.n * config.top); j.sum.assign(spill.sum, spill.sum + j.n * config.top); }
                    retire(0);
                }
                if (last) break;
            }
            const auto td = clock::now();
            hip_check(skx_stream_drain(st), "drain");
            retire(0);
            s_retire += since(td);
        } catch (...) { fail_with(std::current_exception()); }
        { std::lock_guard<std::mutex> l(mu); format_closed = true; if (!error) stop = true; }
        cv_format.notify_all(); cv_free.notify_all(); cv_parsed.notify_all();
        for (auto& t : formatters) t.join();
        for (auto& t : parsers) t.join();
        out.flush();
        if (error) std::rethrow_exception(error);
        if (config.timing) {
            const double all_s = std::chrono::duration<double>(clock::now() - t_begin).count();
            const double run_s = std::chrono::duration<double>(clock::now() - t_first).count();
            // seconds_parse_start_to_last_row: from the moment the parser threads start (stream and page-locked slots exist) until
            // the last row is written; seconds_stream adds that set-up.  device thread: waiting for parsed chunks / inside
            // skx_stream_submit (it blocks when the library's staging slots are all in flight) / final drain + hand-over
            std::fprintf(stderr, "{\"sketchy_hip_timing\": {\"reads\": %zu, \"batches\": %zu, \"seconds_stream\": %.6f, \"seconds_open_input\": %.6f, \"seconds_parse_start_to_last_row\": %.6f, "
                                 "\"reads_per_s\": %.1f, \"parse_threads\": %u, \"format_threads\": %u, \"cpus_pinned_near_device\": %u, \"input\": \"%s\", \"batch_reads\": %zu, "
                                 "\"device_thread_s\": {\"wait_for_parsers\": %.6f, \"submit\": %.6f, \"drain_and_hand_over\": %.6f}}}\n",
                         fed, n_batches, all_s, open_s, run_s, fed / std::max(run_s, 1e-9), n_parse, n_format, pinned, mapped ? (map.inflated() ? (fastq ? "bgzf fastq" : "bgzf fasta") : (fastq ? "mapped fastq" : "mapped fasta")) : "streamed", want_reads,
                         s_wait_parse, s_submit, s_retire);
        }
    }

    // offline mode: one sketcher over all reads of a sample == bottom-s of the union of the per-read bottom-s sketches.  Every batch is
    // one group: the device pools its reads (skx_sketch_groups) and ONE row of s hashes comes back per batch, merged here.  All samples'
    // pooled rows are then counted and ranked in ONE call (skx_rank_sketches: `top` rows per sample come back).
    void shared_hashes(const std::vector<std::string>& paths, const std::vector<Sketch>& sketches, Ref& ref, const Genotypes& geno,
                       const PredictConfig& config, std::ostream& out) {
        const size_t n = paths.size(), n_ref = sketches.size();
        std::vector<std::vector<uint64_t>> pooled(n);
        std::vector<size_t> reads(n, 0);
        pool_samples(paths, ref, config, pooled, reads);
        rank_pooled(pooled, reads, sketches, n_ref, ref, geno, config, out);
    }
    // one pooled bottom-s sketch per sample, and the reads it was pooled from
    void pool_samples(const std::vector<std::string>& paths, Ref& ref, const PredictConfig& config, std::vector<std::vector<uint64_t>>& pooled,
                      std::vector<size_t>& reads) {
        const size_t n = paths.size();
        Batch b; std::string seq;
        std::vector<uint64_t> sk, merged, valid; std::vector<uint32_t> len, first;
        for (size_t f = 0; f < n; ++f) {
            FastxReader reader(paths[f]);
            auto flush = [&]() {
                if (b.n() == 0) return;
                first.assign({0u, (uint32_t)b.n()});
                pool_groups(b, first, ref.k, ref.seed, ref.s, false, sk, len, valid);
                merged.clear();
                std::set_union(pooled[f].begin(), pooled[f].end(), sk.begin(), sk.begin() + len[0], std::back_inserter(merged));
                if (merged.size() > ref.s) merged.resize(ref.s);
                pooled[f].swap(merged);
                b.clear();
            };
            while (reader.next(seq)) {
                b.add(seq); ++reads[f];
                if (b.n() == batch_ || b.bases.size() > (1ull << 29)) flush();
                if (reads[f] == config.limit) break;  // :296-299
            }
            flush();
        }
    }
    void rank_pooled(const std::vector<std::vector<uint64_t>>& pooled, const std::vector<size_t>& reads, const std::vector<Sketch>& sketches,
                     size_t n_ref, Ref& ref, const Genotypes& geno, const PredictConfig& config, std::ostream& out) {
        const size_t n = pooled.size();
        size_t stride = 1;
        for (const auto& p : pooled) stride = std::max(stride, p.size());
        std::vector<uint64_t> flat(n * stride, 0);
        std::vector<uint32_t> plen(n);
        for (size_t f = 0; f < n; ++f) { std::copy(pooled[f].begin(), pooled[f].end(), flat.begin() + f * stride); plen[f] = (uint32_t)pooled[f].size(); }
        std::vector<uint32_t> idx(n * config.top), shared(n * config.top);
        if (skx_rank_sketches && config.top >= 1 && config.top <= SKX_MAX_TOP) {
            hip_check(skx_rank_sketches(ref.h, flat.data(), plen.data(), (uint32_t)n, (uint32_t)stride, (uint32_t)config.top, idx.data(), shared.data(),
                                        nullptr), "rank");
        } else {  // a library without the ranking (or more rows than it ranks): every count comes back, sorted here
            std::vector<uint32_t> common(n * n_ref), order(n_ref);
            hip_check(skx_common_hashes(ref.h, flat.data(), plen.data(), (uint32_t)n, (uint32_t)stride, common.data()), "common");
            for (size_t f = 0; f < n; ++f) {
                const uint32_t* c = common.data() + f * n_ref;
                for (size_t i = 0; i < n_ref; ++i) order[i] = (uint32_t)i;
                std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b2) { return c[a] > c[b2]; });  // :310
                for (size_t j = 0; j < config.top; ++j) { idx[f * config.top + j] = order[j]; shared[f * config.top + j] = c[order[j]]; }
            }
        }
        if (config.consensus && cons_.on) {  // the vote of all samples in one call, a line each from its codes
            std::vector<uint32_t> codes(n * cons_.nfeat);
            hip_check(skx_consensus_rows(ref.h, idx.data(), n, (uint32_t)config.top, codes.data()), "consensus");
            std::string text(n * cons_.line_cap, '\0');
            char* p = text.data();
            for (size_t f = 0; f < n; ++f) p = put_consensus_line(p, reads[f], codes.data() + f * cons_.nfeat);
            out.write(text.data(), p - text.data());
            return;
        }
        std::vector<uint64_t> sum(config.top);
        for (size_t f = 0; f < n; ++f) {
            for (size_t j = 0; j < config.top; ++j) sum[j] = shared[f * config.top + j];
            print_results(sketches, geno, idx.data() + f * config.top, sum.data(), reads[f], config, out);
        }
    }

    // the consensus branch's vote (src/sketchy.rs:365-388) over one row of `top` genomes: per genotype column the string most of them carry
    static std::vector<std::string> vote(const std::vector<Sketch>& sketches, const Genotypes& geno, const uint32_t* idx, size_t top) {
        const size_t nfeat = geno.map.at(sketches[idx[0]].name).size();
        std::vector<std::string> call;
        for (size_t j = 0; j < nfeat; ++j) {
            std::map<std::string, size_t> counts;  // ties: the reference's HashMap order is unspecified; here: smallest value
            for (size_t t = 0; t < top; ++t) counts[geno.map.at(sketches[idx[t]].name)[j]]++;
            auto best = std::max_element(counts.begin(), counts.end(), [](const auto& a, const auto& b) { return a.second < b.second; });
            call.push_back(best->first);
        }
        return call;
    }

    // src/sketchy.rs:358-402
    void print_results(const std::vector<Sketch>& sketches, const Genotypes& geno, const uint32_t* idx, const uint64_t* sum,
                       size_t read, const PredictConfig& config, std::ostream& out) {
        if (config.consensus) {
            out << read << "\t-\t-\t" << join_tab(vote(sketches, geno, idx, config.top)) << "\n";
        } else {
            for (size_t t = 0; t < config.top; ++t) {
                const auto& name = sketches[idx[t]].name;
                out << read << "\t" << name << "\t" << sum[t] << "\t" << join_tab(geno.map.at(name)) << "\n";
            }
        }
    }

    int device_; size_t batch_;
};

}  // namespace sketchy

// ------------------------------------------------------------------ command line (src/cli.rs flag names)
static void usage() {
    std::fprintf(stderr,
                 "sketchy-hip sketch  -o OUT.msh [-i GENOME.fa[.gz] ...] [-s SIZE=1000] [-k K=16] [-e SEED=0] [--counts]   (paths on stdin without -i;\n"
                 "                    --counts: also write every hash's abundance, Mash's counts32)\n"
                 "sketchy-hip predict -r REF.msh [...] -g GENO.tsv [...] [-i READS.fx[.gz] ...] [-t TOP] [-l LIMIT] [-s] [-c] [-H] [-x] [-b BATCH_READS] [-j THREADS] [--timing] [--pin]\n"
                 "                    (without -s: several inputs, one sample each -- the rows of every sample in input order; -l per input; -s: one input;\n"
                 "                    -x / --changes, with -s: only read 1 and the reads whose lines, the shared_hashes column aside, differ from the read before)\n"
                 "                    several -r with as many -g (reference i goes with table i): all references resident together, and after every read the\n"
                 "                    rows or consensus of ONE species -- the lowest whose best sketch has the largest sum -- with the species (the file's name\n"
                 "                    without .msh) as second field; -H: one header line per reference\n"
                 "sketchy-hip neighbours -r REF.msh [-g GENO.tsv] [-t TOP=1] [-c] [-S] [-H]\n"
                 "                    (leave-one-out: per sketch of REF, in file order, the TOP other sketches that share the most hashes with it --\n"
                 "                    sketch_id neighbour_id shared_hashes [the neighbour's genotype columns]; -c, with -g and an odd TOP: one line per\n"
                 "                    sketch, the consensus of its neighbours; -S / --summary, with -g: one line per genotype column -- column, the\n"
                 "                    sketches whose own value is that consensus, all sketches)\n"
                 "sketchy-hip screen  -r REF.msh -i READS.fx[.gz] [-g GENO.tsv] [-t TOP=10] [-l LIMIT] [-H] [-d] [-I] [-w]\n"
                 "                    (containment of every sketch of REF in the read set: the TOP sketches by covered / sketch_size --\n"
                 "                    sketch_id covered sketch_size containment shared_hashes [median_multiplicity] [identity] [genotype columns];\n"
                 "                    covered = hashes of the sketch that at least one read shared; -d / --depth: median_multiplicity = the lower\n"
                 "                    median of the number of reads that shared each covered hash; -I / --identity: containment^(1/k); here -d\n"
                 "                    is --depth, the device is chosen with --device; one reference: several -r are not built;\n"
                 "                    -w / --winner-take-all: every seen hash is credited to ONE sketch, the best of those that hold it (by\n"
                 "                    containment, then covered, then file order): the TOP sketches by won / sketch_size, the columns won and\n"
                 "                    winner_containment behind shared_hashes, the identity from the winner containment)\n"
                 "sketchy-hip composition -r A.msh [B.msh ...] -i READS.fx[.gz] [-m MIN_HITS=1] [-l LIMIT] [-H] [--device N]\n"
                 "                    (what the read set is made of: every reference is one species, named by its file without .msh; a read is the\n"
                 "                    species' whose sketches share the most hashes with the read's own sketch, at least MIN_HITS -- species reads\n"
                 "                    fraction pairs, one line per reference; then ambiguous (several species tie) and unclassified)\n"
                 "sketchy-hip shared  -r REF.msh -q QUERY.msh\n"
                 "sketchy-hip info    -i SKETCH.msh [-p]\n"
                 "sketchy-hip check   -r REF.msh -g GENO.tsv\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { usage(); return 2; }
    const std::string cmd = argv[1];
    std::map<std::string, std::string> opt; std::map<std::string, bool> flag;
    std::vector<std::string> references, tables;  // `predict -r` / `-g` take several files: reference i goes with table i
    std::vector<std::string> inputs;  // `sketch -i` takes several paths (src/cli.rs:27-28: multiple = true); so does offline `predict -i`
    const std::map<std::string, std::string> longnames = {{"--input", "-i"}, {"--reference", "-r"}, {"--genotypes", "-g"}, {"--top", "-t"}, {"--limit", "-l"},
                                                          {"--stream", "-s"}, {"--consensus", "-c"}, {"--header", "-H"}, {"--query", "-q"}, {"--params", "-p"},
                                                          {"--device", "-d"}, {"--batch", "-b"}, {"--output", "-o"}, {"--sketch-size", "-s"},
                                                          {"--kmer-size", "-k"}, {"--seed", "-e"}, {"--threads", "-j"}, {"--timing", "-T"}, {"--pin", "-P"}, {"--counts", "-C"}, {"--changes", "-x"}, {"--summary", "-S"}};
    const bool is_sketch = cmd == "sketch";  // there -s takes a value (sketch size), elsewhere it is --stream
    const bool many_inputs = is_sketch || cmd == "predict";
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        if (is_sketch && a == "--stream") { usage(); return 2; }
        if (cmd == "screen" && (a == "-d" || a == "--depth")) { flag["--depth"] = true; continue; }  // (`screen`: -d is --depth; the device: --device)
        if (cmd == "screen" && (a == "-I" || a == "--identity")) { flag["--identity"] = true; continue; }
        if (cmd == "screen" && (a == "-w" || a == "--winner-take-all")) { flag["--winner-take-all"] = true; continue; }
        if (longnames.count(a)) a = longnames.at(a);
        // (predict: a lone "-" is a path -- stdin)
        if (many_inputs && a == "-i") { while (i + 1 < argc && (argv[i + 1][0] != '-' || (!is_sketch && !argv[i + 1][1]))) inputs.push_back(argv[++i]); continue; }
        if ((cmd == "predict" && (a == "-r" || a == "-g")) || (cmd == "composition" && a == "-r")) {
            auto& list = a == "-r" ? references : tables;
            if (i + 1 >= argc) { usage(); return 2; }
            while (i + 1 < argc && argv[i + 1][0] != '-') list.push_back(argv[++i]);
            if (!list.empty()) opt[a] = list[0];
            continue;
        }
        if ((!is_sketch && a == "-s") || a == "-c" || a == "-H" || a == "-p" || a == "-T" || a == "-P" || a == "-C" || a == "-x" || a == "-S") flag[a] = true;
        else if (i + 1 < argc) opt[a] = argv[++i];
        else { usage(); return 2; }
    }
    try {
        // (-b: reads per device batch.  Streaming: 65 536 by default -- up to four batches share one scan of the reference, and the
        // copy + kernels of a host-fed batch cost ~0.7 ms whatever its size below that (measured at C2 on an MI355X box, 1.57 M reads of
        // 1.5 kb from /dev/shm: 21 M reads/s with 32 768-read batches, 26-27 M with 65 536); it costs ~100 MB of page-locked memory per
        // slot, 27 slots with 16 threads)
        const bool streaming = cmd == "predict" && flag["-s"];
        sketchy::Sketchy app(opt.count("-d") ? std::atoi(opt["-d"].c_str()) : 0,
                             opt.count("-b") ? (size_t)std::max(1L, std::atol(opt["-b"].c_str())) : (streaming ? 65536 : 16384));
        if (cmd == "sketch") {
            if (!opt.count("-o")) { usage(); return 2; }
            if (inputs.empty()) { std::string line; while (std::getline(std::cin, line)) if (!line.empty()) inputs.push_back(line); }  // src/sketchy.rs:137-146
            app.sketch(inputs, opt["-o"], opt.count("-s") ? (size_t)std::atol(opt["-s"].c_str()) : 1000,
                       opt.count("-k") ? (uint32_t)std::atoi(opt["-k"].c_str()) : 16u, opt.count("-e") ? std::strtoull(opt["-e"].c_str(), nullptr, 10) : 0ull,
                       flag["-C"]);
        } else if (cmd == "predict") {
            if (!opt.count("-r") || !opt.count("-g")) { usage(); return 2; }
            if (references.size() != tables.size()) {
                std::fprintf(stderr, "Error: predict takes as many genotype tables (-g: %zu) as references (-r: %zu): reference i goes with table i\n",
                             tables.size(), references.size());
                return 2;
            }
            if (flag["-x"] && !flag["-s"]) {
                std::fprintf(stderr, "Error: predict --changes prints the change points of a stream: it needs -s\n");
                return 2;
            }
            if (flag["-s"] && inputs.size() > 1) {
                std::fprintf(stderr, "Error: predict -s (streaming) takes one input, %zu were given: several inputs are ranked offline (without -s)\n", inputs.size());
                return 2;
            }
            sketchy::PredictConfig cfg;
            cfg.top = opt.count("-t") ? (size_t)std::atol(opt["-t"].c_str()) : 1;
            cfg.limit = opt.count("-l") ? (size_t)std::atol(opt["-l"].c_str()) : 0;
            cfg.stream = flag["-s"]; cfg.consensus = flag["-c"]; cfg.header = flag["-H"]; cfg.changes = flag["-x"];
            cfg.threads = opt.count("-j") ? (size_t)std::max(1L, std::atol(opt["-j"].c_str())) : 0; cfg.timing = flag["-T"]; cfg.pin = flag["-P"];
            if (references.size() > 1) app.predict_multi(inputs, references, tables, cfg, std::cout);
            else app.predict(inputs, opt["-r"], opt["-g"], cfg, std::cout);
        } else if (cmd == "neighbours") {
            if (!opt.count("-r")) { usage(); return 2; }
            sketchy::NeighboursConfig cfg;
            const long top = opt.count("-t") ? std::atol(opt["-t"].c_str()) : 1;
            cfg.consensus = flag["-c"]; cfg.summary = flag["-S"]; cfg.header = flag["-H"];
            if (top < 1) { std::fprintf(stderr, "Error: --top must be at least 1\n"); return 2; }
            if ((cfg.consensus || cfg.summary) && !opt.count("-g")) {
                std::fprintf(stderr, "Error: neighbours --consensus / --summary call genotypes: they need -g\n");
                return 2;
            }
            if (cfg.consensus && top % 2 != 1) {  // (the rule of predict -c, src/sketchy.rs:74-79)
                std::fprintf(stderr, "Error: --top must be an odd number when using --consensus\n");
                return 2;
            }
            cfg.top = (size_t)top;
            app.neighbours(opt["-r"], opt.count("-g") ? opt["-g"] : std::string(), cfg, std::cout);
        } else if (cmd == "screen") {
            if (!opt.count("-r") || !opt.count("-i")) { usage(); return 2; }
            const long top = opt.count("-t") ? std::atol(opt["-t"].c_str()) : 10, limit = opt.count("-l") ? std::atol(opt["-l"].c_str()) : 0;
            if (top < 1) { std::fprintf(stderr, "Error: --top must be at least 1\n"); return 2; }
            app.screen(opt["-i"], opt["-r"], opt.count("-g") ? opt["-g"] : std::string(), (size_t)top, (size_t)std::max(0L, limit), flag["-H"], std::cout,
                       flag["--depth"], flag["--identity"], flag["--winner-take-all"]);
        } else if (cmd == "composition") {
            if (references.empty() || !opt.count("-i")) { usage(); return 2; }
            const long min_hits = opt.count("-m") ? std::atol(opt["-m"].c_str()) : 1, limit = opt.count("-l") ? std::atol(opt["-l"].c_str()) : 0;
            if (min_hits < 1 || min_hits > 0xFFFFFFFFL) { std::fprintf(stderr, "Error: -m (the hits that make a read a species') must be at least 1\n"); return 2; }
            app.composition(opt["-i"], references, (uint32_t)min_hits, (size_t)std::max(0L, limit), flag["-H"], std::cout);
        } else if (cmd == "shared") {
            if (!opt.count("-r") || !opt.count("-q")) { usage(); return 2; }
            app.shared(opt["-r"], opt["-q"], std::cout);
        } else if (cmd == "check") {
            if (!opt.count("-r") || !opt.count("-g")) { usage(); return 2; }
            app.check(opt["-r"], opt["-g"], std::cout);
        } else if (cmd == "info") {
            if (!opt.count("-i")) { usage(); return 2; }
            app.info(opt["-i"], flag["-p"], std::cout);
        } else { usage(); return 2; }
    } catch (const sketchy::UsageError& e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 2;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
    return 0;
}
