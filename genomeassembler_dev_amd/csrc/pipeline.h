// pipeline.h — host-side state of the device pipeline (reads -> distinct k-mers -> graph -> contigs -> scores).
#pragma once
#include "gasm_internal.h"
#include "kernels.h"

// ---- one launch site for both key widths: f(KeyTag<u64>) for one key word, f(KeyTag<K128>) for two.  GLAUNCH_K wraps a
// GLAUNCH whose kernel and arguments name the key type as K
template <class K> struct KeyTag { using type = K; };
template <class F> static inline int with_key(int words, F&& f) { return words == 1 ? f(KeyTag<u64>{}) : f(KeyTag<K128>{}); }
#define GLAUNCH_K(ctx, words, name, kern, grid, block, shmem, ...)          \
    GCHK(with_key(words, [&](auto _tag) -> int {                            \
        using K = typename decltype(_tag)::type;                            \
        GLAUNCH(ctx, name, kern, grid, block, shmem, __VA_ARGS__);          \
        return GASM_OK;                                                     \
    }))

// Reads of one or more segments, resident in HBM as one packed base stream.
struct DevReads {
    u32 n_segments = 0;
    u64 n_reads = 0, total_bases = 0;
    u32 fixed_len = 0;
    u32 min_len = 0, max_len = 0;          // over non-empty reads (0 if none)
    u64 n_empty = 0;
    std::vector<u64> h_read_off;            // ragged only
    std::vector<u64> h_seg_read_off;        // n_segments+1
    std::vector<u64> h_seg_empty;           // empty reads per segment
    bool positioned = false;                // fixed-length reads at the base positions in d_read_off (pooled builds)
    int sim_shift = 52;                     // fixed-point shift of the last weighted simulate()
    u64 upload_id = 0;                      // changes with every upload: "the same reads again?" (BuildState)
    DBuf d_words, d_read_off, d_seg_read_off;
    // tile directory cache (depends on reads per tile)
    u32 tiles_ipt = 0, tiles_orr = 0, n_tiles = 0;
    std::vector<u32> h_seg_tile_start, h_tile_info;
    DBuf d_seg_tile_start, d_tile_info;

    int upload(gasm_ctx* ctx, const char* reads, const u64* read_off, u64 n_reads, u32 fixed_len, const u64* seg_read_off,
               u32 n_segments);
    int upload_packed(gasm_ctx* ctx, const u64* words, const u64* read_off, u64 n_reads, u32 fixed_len, const u64* seg_read_off,
                      u32 n_segments);
    int adopt_packed(gasm_ctx* ctx, DBuf& words_dev, const u64* read_off, u64 n_reads, u32 fixed_len, const u64* seg_read_off, u32 n_segments);
    // reads simulated on the device from the genomes (lib/GenerateReads.R:235-313); d_kept_start receives every read's start
    int simulate(gasm_ctx* ctx, const char* genomes, const u64* genome_off, u32 n_segments, u32 read_len, double coverage, u64 seed, int kmer,
                 const double* table, DBuf& d_kept_start);
    int set_layout(const u64* read_off, u64 n_reads, u32 fixed_len, const u64* seg_read_off, u32 n_segments);
    int finish_upload(gasm_ctx* ctx);
    int set_tiles(gasm_ctx* ctx, u32 ipt, u32 orr);
    // this = the both-strand form of `src` (gasm_batch_build_strands, strands = 2): every segment's reads followed by their reverse
    // complements, same layout kind (k_reads_both_strands).  Build-only: scorers keep `src`.  Complete before it returns.
    int make_both_strands(gasm_ctx* ctx, const DevReads& src);
    u64 strands_of = 0;                     // upload_id of the reads this stream was made from by make_both_strands (0: none)
    ReadSet view() const;
    u64 read_len(u64 r) const { return fixed_len ? fixed_len : h_read_off[r + 1] - h_read_off[r]; }
    void release();
};

// Paths to score (contigs produced by a build, or caller-supplied sequences).
struct DevPaths {
    u32 n_segments = 0, n_paths = 0;
    u64 total_bases = 0;
    std::vector<u64> h_p_off;               // n_paths+1
    std::vector<u32> h_seg_path_off;        // n_segments+1
    std::vector<u64> h_seg_base_off;        // n_segments+1: first base of each segment's paths
    DBuf d_words, d_p_off, d_seg_path_off, d_seg_base_off;
    // borrowed device directories (the contigs of a build): used instead of the owned buffers when set
    const u64* b_p_off = nullptr;
    const u32* b_seg_path_off = nullptr;
    const u64* b_seg_base_off = nullptr;
    const u64* seg_base_off_dev() const { return b_seg_base_off ? b_seg_base_off : d_seg_base_off.as<u64>(); }
    int pack_from_device_ascii(gasm_ctx* ctx, const u8* d_ascii);
    int upload_ascii(gasm_ctx* ctx, const char* data, const u64* off, u32 n_paths);
    int upload_dirs(gasm_ctx* ctx);
    PathSet view() const;
    void release();
};

// Every option of a build, the one form in which they travel from the public entries (capi.hip) to the launches; the defaults are
// gasm_batch_build's.
// min_count > 1: only the distinct k-mers seen at least min_count times in their segment enter the graph (k_bucket_solid behind the
// de-duplication; 1: all of them, and not a launch more)
// strands = 2: built from the reads and their reverse complements (the caller hands pipeline_build the both-strand DevReads); the twin
// map exists for such a build only
// tip_len > 0: tip_rounds (1 .. GASM_MAX_TIP_ROUNDS) rounds of tip clipping behind the cutoff, contigs of at most tip_len bases
// bubble_len > 0 (<= GASM_MAX_BUBBLE_LEN): bubble_rounds (1 .. GASM_MAX_BUBBLE_ROUNDS) rounds of bubble popping behind the tip rounds
// cov_cutoff > 0 and cov_len > 0 (<= GASM_MAX_BUBBLE_LEN): cov_rounds (1 .. GASM_MAX_COV_ROUNDS) rounds of low-coverage removal behind the
// bubble rounds, contigs of at most cov_len bases whose mean multiplicity is below cov_cutoff
// A feature that is off costs not a launch.  Normalised (build_opts_normalised): the rounds of a feature that is off are 0
enum RoundKind : u32 { ROUNDS_TIP = 0, ROUNDS_BUBBLE, ROUNDS_LOWCOV, ROUND_KINDS };     // in the order the rounds run
struct BuildOpts {
    int k = 0;
    u64 genome_len_hint = 0;
    u32 min_count = 1, strands = 1, tip_len = 0, tip_rounds = 0, bubble_len = 0, bubble_rounds = 0, cov_cutoff = 0, cov_len = 0, cov_rounds = 0;
    bool lowcov() const { return cov_cutoff != 0 && cov_len != 0; }
    // rounds of one kind; normalised, 0 exactly when the kind is off
    u32 rounds(u32 kind) const { return kind == ROUNDS_TIP ? tip_rounds : kind == ROUNDS_BUBBLE ? bubble_rounds : cov_rounds; }
    u32 total_rounds() const { return tip_rounds + bubble_rounds + cov_rounds; }
};
// the argument rules of every build entry (GASM_ERR_INVALID and the error text), and the rounds of the features that are off set to 0
int build_opts_check(const BuildOpts& o);
BuildOpts build_opts_normalised(BuildOpts o);

// What the rounds of one kind removed in the last build.  The three kinds run the same mechanism (mark, k_bucket_solid compaction) and
// count the same way
struct RoundStats {
    u32 max_rounds;                         // GASM_MAX_TIP_ROUNDS / GASM_MAX_BUBBLE_ROUNDS / GASM_MAX_COV_ROUNDS
    DBuf d_stats;                           // the kind is on: u32[2][max_rounds][S], contigs then k-mers removed per round and segment
    std::vector<u32> h_contigs, h_kmers;    // pipeline_fetch_round_stats: [s * max_rounds + r]
};

// The tables a pass over a finished build writes, back to back in one device array in the order given, each at a multiple of its
// alignment (records that are stored 16 bytes at a time on 16, 64-bit counters on 8).  The queue function clears the array from the
// first `zeroed` table to its end with one memset, so the zeroed tables come last
struct PassTable {
    size_t n, elem, align;                  // elements, bytes per element, alignment in bytes
    bool zeroed;
    size_t off = 0;                         // set by PassLayout
    size_t bytes() const { return n * elem; }
};
struct PassLayout {
    std::vector<PassTable> t;
    size_t bytes = 0, zero_from = 0;        // of the whole array; where the first zeroed table starts
    PassLayout(std::initializer_list<PassTable> tables) : t(tables) {
        bool z = false;
        for (PassTable& x : t) {
            x.off = (bytes + x.align - 1) / x.align * x.align;
            if (x.zeroed && !z) { z = true; zero_from = x.off; }
            bytes = x.off + x.bytes();
        }
        if (!z) zero_from = bytes;
    }
    template <class T> T* at(const DBuf& d, size_t i) const { return reinterpret_cast<T*>(static_cast<char*>(d.p) + t[i].off); }
};
// What such a pass leaves: its device array, after its fetch the host copy of every table (in 8-byte words, one entry more than the table
// holds, so there is a pointer to hand out for an empty one), and what the layout of the last call depended on
struct PassState {
    DBuf d;
    std::vector<std::vector<u64>> h;
    bool queued = false;                    // the pass ran on the arrays of this build (pipeline_build clears it)
    u32 param[2] = {0, 0};
    template <class T> const T* host(size_t i) const { return reinterpret_cast<const T*>(h[i].data()); }
};
// the tables of the four passes, in layout order: u32 succ[4P], pred[4P], link_support[4P], span_support[16P], u64 skipped[S];
// int32 rec[4 * orientations * pairs], u32 insert_hist[S * (max_insert + 1)], u64 counters[S * GASM_PAIR_FIELDS];
// int32 rec[4 * reads], u32 pile[4 * contig bases], mismatch_hist[S * (max_mismatch + 1)], u64 counters[S * GASM_MAP_FIELDS];
// int32 rec[4 * reads], rec_gap[4 * reads], u32 pile[4 * contig bases], gap_pile[2 * contig bases], edit_hist[S * (max_edits + 1)],
// u64 counters[S * GASM_MAPG_FIELDS]
enum { LINKS_SUCC, LINKS_PRED, LINKS_LSUP, LINKS_SSUP, LINKS_SKIPPED };
enum { PAIRS_REC, PAIRS_HIST, PAIRS_CNT };
enum { MAP_REC, MAP_PILE, MAP_HIST, MAP_CNT };
// (behind them, when the mapping tried end gaps: int32 rec_end[4 * reads], u64 end_counters[S * GASM_MAPEND_FIELDS])
// (behind those, when the mapping kept the alignments: int32 rec_piece[2 * GASM_MAP_MAX_PIECES * reads], u32 ins_pile[4 * ins_cols * contig bases])
enum { MAPG_REC, MAPG_GAP, MAPG_PILE, MAPG_GPILE, MAPG_HIST, MAPG_CNT, MAPG_END, MAPG_ENDCNT, MAPG_PIECE, MAPG_INS };
// param[1] of the gapped mapping's PassState, what its layout depends on beside max_edits (param[0]): the end tables are there, the
// alignment tables are there, and from MAPG_COLS_SHIFT up the columns of the insertion pileup
enum : u32 { MAPG_HAS_ENDS = 1u, MAPG_HAS_TRACE = 2u, MAPG_COLS_SHIFT = 8u };
// mapped scoring (T = param[0] tables over P contigs): double out[3 T P] (table t: bp, norm_by_break_freqs, norm_by_len, P each), int32 out[2 P]
// (kmer_breaks, sequence_len), u32 cnt[P], u64 fx[T P], u32 start_pile[contig bases], u64 counters[S * GASM_MAPSCORE_FIELDS]
enum { MAPSC_F64, MAPSC_I32, MAPSC_CNT, MAPSC_FX, MAPSC_PILE, MAPSC_COUNTERS };

struct BuildState {
    // ---- plan (host-side, from the reads): key width, tile shape, partition
    int k = 0, bbits = 0, fbits = 9, words = 1, bb_cap = 0;
    bool small_tbl = true;                  // 2048-slot de-duplication tables (else 4096)
    bool rank_global = false;               // list ranking by whole-GPU pointer doubling only (set after the LDS ranking gave up)
    bool single_pass = true;                // partition in one pass into regions of fixed capacity (k_bucket_partition); cleared when a region overflowed
    // the region layout in d_bstart belongs to ... (uploaded once per batch shape)
    struct PartLayout {
        u64 reads_id = 0;
        int k = 0, bbits = 0, slack = 0, forced = 0;
        u32 padm = 0, g = 0;
        bool operator==(const PartLayout& o) const {
            return reads_id == o.reads_id && k == o.k && bbits == o.bbits && slack == o.slack && forced == o.forced && padm == o.padm && g == o.g;
        }
    } part;
    bool part_valid = false;
    u64 part_alloc = 0;                     // keys of all regions of that layout
    bool multi_pass = false;                // de-duplication in passes over key sub-ranges (set after the bucket bits ran out: k_bucket_dedup_multi)
    bool ranked_in_lds = false;
    u32 tile_g = 1;                         // threads per read of the tile kernels
    u64 n_kmers = 0, hint = 0, reads_id = 0;
    BuildOpts opts;                         // what this build was asked for, normalised (pipeline_build).  Every attempt of the retry ladder filters,
                                            // clips, pops and removes with it again, each step slot keeps its own, and scores of a graph that any of
                                            // them changed compare bases.  (k and hint above are what plan_build planned with: the hint doubled for
                                            // strands = 2.)  Pooled builds never set it: every feature off
    std::vector<u64> h_seg_nk;              // k-mers per segment
    // upper bounds the arrays are allocated at, and estimates the grids are sized from (the kernels loop beyond them)
    u64 D_cap = 0, maxD_cap = 0, bases_cap = 0;
    u32 maxD_est = 1, paths_est = 0;
    bool have_actual = false;               // maxD_est / paths_est / the partition come from a finished build of the same reads
    // ---- what the last attempt ran, for gasm_batch_build_plan (host fields only, set where the launches are chosen)
    u32 tile_orr = 1;                       // offset rounds of the tile kernels (plan_build)
    bool part_single = false;               // the partition ran in one pass (k_bucket_partition), else count + scan + scatter
    bool scan_in_dedup = false;             // the buckets' offsets came from the de-duplication's last workgroup, else k_scan_excl
    u32 ruler_shift = 0;                    // LDS list ranking: rulers every 2^ruler_shift-th edge (0: not ranked in LDS)
    u32 attempts_distinct = 0;              // launch_distinct calls of the last build (1 + partition / table retries)
    u32 attempts_graph = 0;                 // graph-only repeats of the last build (the LDS ranking gave up)
    // ---- report: written by the last kernels of a build into pinned memory, read by pipeline_build_finish
    u32* h_report = nullptr;
    size_t h_report_words = 0;
    u32 ticket = 0;
    bool pending = false;                   // a build is queued and its report has not been read
    // ---- results on the host (valid after pipeline_build_finish)
    u32 d_total = 0, n_contigs = 0;
    u64 contig_bases = 0;
    std::vector<u32> h_dstart;              // n_segments+1: first distinct k-mer of every segment
    std::vector<u32> h_seg_cstart;          // n_segments+1
    std::vector<u64> h_seg_bstart;          // n_segments+1
    DBuf d_keys2;                           // output of the multi-pass de-duplication (its passes re-read d_keys)
    DBuf d_keys, d_mult, d_hist, d_toff, d_tcnt, d_fdir, d_bstart, d_bucket_d, d_dstart, d_flags, d_rtab;
    DBuf d_solid_removed;                   // min_count > 1: distinct k-mers the cutoff removed, per segment (u32, zeroed with every attempt)
    RoundStats round_stats[ROUND_KINDS] = {{GASM_MAX_TIP_ROUNDS}, {GASM_MAX_BUBBLE_ROUNDS}, {GASM_MAX_COV_ROUNDS}};
    DBuf d_ccov;                            // per-contig coverage of the last build (u64 sums[P], then u32 edges[P]: pipeline_contig_coverage)
    std::vector<u64> h_ccov_m;
    std::vector<u32> h_ccov_n;
    bool coverage_queued = false;           // k_contig_cov ran on the arrays of this build
    // the passes that lay reads over the last build, each with the tables listed at its enum below: contig links (pipeline_contig_links),
    // read-pair places (pipeline_place_pairs; param: orientations, max_insert), read mapping and gapped read mapping (pipeline_map_reads;
    // param: max_mismatch / max_edits, and for mapg the MAPG_HAS_* bits and the insertion columns) — the two mappings independent of each other
    PassState links, pairs, map, mapg;
    // mapped scoring (pipeline_score_mapped; param: tables, source) from the records of map or mapg, and its tables' fixed-point shifts
    PassState mapscore;
    int mapscore_shift[GASM_MAX_TABLES] = {};
    DBuf d_spectrum;                        // k-mer spectrum of the last build (u32[S * 256], pipeline_kmer_spectrum)
    DBuf d_twin;                            // strands = 2: twin map (u32 per contig, then k_contig_twin's flag word), made by the first fetch
    std::vector<u32> h_twin;
    bool fetched_twins = false;
    DBuf d_dk_key, d_dk_cnt, d_eflag, d_nxt, d_link, d_clen, d_ecid, d_ecoff;
    DBuf d_seg_cbases, d_seg_cstart, d_seg_bstart, d_c_off, d_contig_ascii;
    // host copies filled by fetch
    std::vector<u64> h_seg_doff, h_dk_key, h_c_off, h_seg_coff;
    std::vector<u32> h_dk_cnt, h_nxt;
    std::vector<u64> h_solid_before, h_solid_after, h_spectrum;      // pipeline_fetch_solid_stats / pipeline_fetch_kmer_spectrum
    bool spectrum_queued = false;           // k_kmer_spectrum ran on the arrays of this build
    std::vector<u8> h_eflag;
    std::vector<char> h_contigs;
    bool fetched_distinct = false, fetched_contigs = false;
    void release();
};

struct ScoreTable {
    // direct-address tables over ACGT strings of length 1..8 (87 380 rows)
    DBuf d_prob, d_row, d_fix;
    std::vector<double> h_prob;   // direct-address table as uploaded
    std::vector<double> h_row_prob;   // the caller's table, row by row (KS statistic: rows in ascending-probability order)
    double h_absmax = 0;          // max |prob| over the finite entries (set with the table)
    bool h_finite = false;        // no NaN or infinity in the table (set_standard)
    int fix_shift = -1;           // d_fix = round(prob * 2^fix_shift), -1 = not built
    u32 n_table = 0;
    // the fixed-point shift for at most max_terms reads per path, -1 = the table needs the FP64 scorer (gasm_host::fixed_point_shift)
    int fixed_shift(u64 max_terms) const;
    int set_fixed(gasm_ctx* ctx, int shift);
    int set(gasm_ctx* ctx, const char* bp_kmer, const u64* bp_off, u64 n_table, const double* bp_prob);
    int set_standard(gasm_ctx* ctx, const double* table69904);
    void release();
};

struct ScoreState {
    DBuf d_tbl_off, d_seed, d_gpos, d_poscnt, d_total, d_out_f64, d_out_i32, d_freq, d_pd_off, d_pd, d_seg_empty, d_fxsum, d_first, d_first_off;
    std::vector<u64> h_toff;
    u32 n_paths = 0, n_table = 0;
    // breakage tables of the last launch.  Table t's bp / nf / nl arrays lie at d_out_f64 +
    // 3 t stride, its fixed-point sums at t * stride behind table 0's, its prob_dist at t * h_pd_off[n_paths]; on the host
    // h_bp / h_nf / h_nl / h_pd hold table after table (table 0 first: what single-table readers see)
    u32 n_tables = 1;
    size_t stride = 1;                      // entries per output array on the device (paths + 1, or their upper bound + 1)
    const BuildState* graph = nullptr;      // batch scoring of a build's own contigs: the number of paths comes with its report
    bool want_freq = false, want_pd = false, launched = false;
    bool verify = false;                    // the graph scorer compared every read with its contig (GASM_SCORE_VERIFY)
    std::vector<double> h_bp, h_nf, h_nl, h_freq, h_pd;
    std::vector<int32_t> h_breaks, h_len;
    std::vector<u64> h_pd_off;
    bool valid = false;
    void release();
};

// queues a whole build on the ctx stream and returns; pipeline_build_finish (called by every fetch) waits for its report
// and repeats it with a larger configuration if it failed.  *rebuilt: the device arrays were produced anew (a score
// queued behind the first attempt must be queued again).
// `o` has passed build_opts_check and is stored normalised in bs.opts.  strands = 2: `rd` is the both-strand form of the batch's reads
// (DevReads::make_both_strands, else GASM_ERR_STATE) and must be handed to every later call that takes this build's reads (finish,
// fetches); genome_len_hint still means the genome: the estimate of the distinct k-mers is doubled here.  Every round of tip clipping,
// bubble popping and low-coverage removal is a graph pass up to the chain lengths, the kind's marking kernel and a compaction of the
// buckets' runs; the last graph pass alone writes the report
int pipeline_build(gasm_ctx* ctx, DevReads& rd, BuildState& bs, const BuildOpts& o);
int pipeline_build_finish(gasm_ctx* ctx, DevReads& rd, BuildState& bs, bool* rebuilt);
int pipeline_build_finish_n(gasm_ctx* ctx, DevReads* rd, u32 n_segments, BuildState& bs, bool* rebuilt);
// The overflow retry ladder of every build path: after an attempt raised the GASM_OVF_* bits `ovf`, advance the configuration by
// the first rung that applies among those the caller permits — a region overflowed: exact partition; small tables: large ones
// (64-bit keys only); two more bucket bits up to bb_cap; multi-pass de-duplication — or return false: none is left
enum : u32 { GASM_RUNG_EXACT = 1, GASM_RUNG_TABLE = 2, GASM_RUNG_BBITS = 4, GASM_RUNG_MULTI = 8, GASM_RUNG_ALL = 15 };
bool build_next_config(u32 ovf, u32 rungs, int words, int bb_cap, bool& single_pass, bool& small_tbl, int& bbits, bool& multi_pass);
// one row of gasm_batch_build_plan (GASM_PLAN_FIELDS words, include/gasm.h) from a finished build's host fields
void pipeline_build_plan(const DevReads& rd, const BuildState& bs, int32_t* row);
// building blocks shared with the pooled build (pool.hip)
int plan_build(gasm_ctx* ctx, DevReads& rd, int k, u64 hint, BuildState& bs);
void distinct_caps(BuildState& bs, u32 n_segments);
int launch_distinct(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
int launch_graph(gasm_ctx* ctx, u32 n_segments, BuildState& bs);
int pipeline_fetch_distinct(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
int pipeline_fetch_contigs(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
// distinct k-mers per segment before and after the cutoff of the finished build (equal at min_count = 1)
int pipeline_fetch_solid_stats(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
// contigs and k-mers removed per segment and round by the finished build's rounds of `kind`, into bs.round_stats[kind] (zero for rounds
// not run and with the kind off)
int pipeline_fetch_round_stats(gasm_ctx* ctx, DevReads& rd, BuildState& bs, u32 kind);
// per-contig sum of multiplicities and number of edges of the finished build: queue (k_contig_cov, reads the build's arrays only), then
// fetch h_ccov_m / h_ccov_n, one entry per contig in the order of the contig list
int pipeline_contig_coverage(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
int pipeline_fetch_contig_coverage(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
// Contig links (kernels_links.hip; the rule: include/gasm.h "Contig links") of the finished build: queue k_contig_links and k_read_thread on the
// build's stream behind it (they read the build's arrays, the contig text and the reads `rd` the build was made from — the both-strand stream
// of a strands = 2 build, so every read and its reverse complement are threaded), then fetch bs.links' tables: succ / pred / link support
// (4 per contig), span support (16 per contig) and skipped (per segment; reads, each once whatever the strands).  Positioned reads (pooled
// builds): GASM_ERR_STATE
int pipeline_contig_links(gasm_ctx* ctx, DevReads& rd, BuildState& bs, u32 span_len);
int pipeline_fetch_contig_links(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
// Read pairs (k_pair_place in kernels_links.hip; the rule: include/gasm.h "Read pairs") of the finished build: queue the kernel on the build's
// stream behind it (it reads the build's arrays and the batch's OWN reads `rd`, in which reads 2p and 2p + 1 are pair p — `rd_build` is what
// the build was made from: the both-strand stream of a strands = 2 build, which then makes two orientations per pair), then fetch bs.pairs'
// tables: records (4 per oriented pair), insert histogram (max_insert + 1 per segment) and counters (GASM_PAIR_FIELDS per segment).  A
// segment with an odd number of reads: GASM_ERR_INVALID.  Positioned reads (pooled builds): GASM_ERR_STATE
int pipeline_place_pairs(gasm_ctx* ctx, DevReads& rd_build, DevReads& rd, BuildState& bs, u32 max_insert);
int pipeline_fetch_pair_places(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
// Read mapping of the finished build (k_read_map in kernels_map.hip; the rules: include/gasm.h "Read mapping" and "Gapped read mapping"):
// queue the kernel on the build's stream behind it (it reads the build's arrays and the batch's OWN reads `rd`, as given, whatever the
// build's strands), then fetch the tables.  gapped = false: into bs.map, max_edits is max_mismatch, max_gap is not used; gapped = true: into
// bs.mapg, beside the other and independent of it
// end_gap > 0 (gapped only): k_read_map_ends, which tries one gap at each end of every chain ("End gaps") and leaves two more tables
// trace (gapped only, any end_gap): k_read_map_trace alone, which leaves those eight and the piece records and the insertion pileup ("Alignments")
int pipeline_map_reads(gasm_ctx* ctx, DevReads& rd_build, DevReads& rd, BuildState& bs, bool gapped, u32 max_edits, u32 max_gap, u32 end_gap = 0, bool trace = false);
int pipeline_fetch_read_map(gasm_ctx* ctx, DevReads& rd, BuildState& bs, bool gapped);
// Mapped scoring of the finished build (k_score_mapped in kernels_score.hip; the rule: include/gasm.h "Mapped scoring"): queue the kernel and a
// k_score_finish per table on the build's stream behind it, then fetch the tables.  It reads the records of bs.map (gapped = false) or bs.mapg,
// which must have been queued over this build (else GASM_ERR_STATE), the build's contig text and the batch's OWN reads' lengths.  tbs: T tables
// of the pass's own, each with a fixed-point shift for these reads (else GASM_ERR_INVALID, nothing queued)
int pipeline_score_mapped(gasm_ctx* ctx, DevReads& rd_build, DevReads& rd, BuildState& bs, bool gapped, int kmer, ScoreTable* const* tbs, u32 T, bool partial);
int pipeline_fetch_mapped_scores(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
// multiplicity histogram of the finished build's dense arrays: queue (k_kmer_spectrum, reads dstart / dk_cnt only), then fetch
// n_segments x 256 counts
int pipeline_kmer_spectrum(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
int pipeline_fetch_kmer_spectrum(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
// twin map of a finished strands = 2 build (k_contig_twin, once per build): h_twin[c] = index inside its segment of the contig that
// is contig c's reverse complement.  GASM_ERR_STATE after a strands = 1 build, GASM_ERR_INTERNAL if a contig has no twin
int pipeline_fetch_contig_twins(gasm_ctx* ctx, DevReads& rd, BuildState& bs);
// Read correction (k_read_correct; the rule: include/gasm.h) of the reads `rd` against the distinct k-mers of the FINISHED build `bs` (the
// caller has read its report: a retry cannot swap the arrays underneath; a pending build is GASM_ERR_STATE).  out_words: a copy of
// rd's packed stream, padding words included, with the fixes applied; d_stats: GASM_CORRECT_FIELDS u32 counters per segment.  Both are
// (re)allocated here; everything is queued on the ctx stream, behind the build, and the caller waits.  `rd` is always the batch's own
// reads, never the both-strand stream of a strands = 2 build (whose k-mer set holds both orientations already).  Positioned reads
// (pooled builds): GASM_ERR_STATE.  Reads only the build's arrays and the reads: no build or score result changes.
int pipeline_correct_reads(gasm_ctx* ctx, DevReads& rd, BuildState& bs, DBuf& out_words, DBuf& d_stats);
// the packed reads of `rd` as ASCII in h_ascii (k_unpack_ascii; GASM_ERR_STATE for positioned reads) and their n_reads + 1 offsets
int pipeline_fetch_reads(gasm_ctx* ctx, DevReads& rd, std::vector<char>& h_ascii, std::vector<u64>& h_read_off);
int pipeline_fetch_graph(gasm_ctx* ctx, DevReads& rd, BuildState& bs);    // h_eflag / h_nxt: per-edge flags and successors
// paths of the build as a DevPaths (packs the contig text on the device; works on a queued build); the host-side numbers
// of the same paths once the build's report has been read
int pipeline_contig_paths(gasm_ctx* ctx, const DevReads& rd, const BuildState& bs, DevPaths& dp);
void pipeline_contig_paths_host(const DevReads& rd, const BuildState& bs, DevPaths& dp);
// Scores the paths of `dp` against the reads under n_tables tables (1 .. GASM_MAX_TABLES) that share their keys (tbs[0]'s rows
// serve path_freq): position counters / graph match once, sums (and prob_dist) per table; table t bit for bit what a call
// with tbs[t] alone gives.  graph != nullptr: dp holds the contigs of that build (same order), so reads are matched through
// the edge list.
int pipeline_score_launch(gasm_ctx* ctx, DevReads& rd, DevPaths& dp, int kmer, ScoreTable* const* tbs, u32 n_tables, bool want_freq,
                          bool want_pd, ScoreState& ss, const BuildState* graph);
int pipeline_score_fetch(gasm_ctx* ctx, ScoreState& ss);
// batch scoring can go through the build's graph (queued without waiting for the build) when every read holds a k-mer
// and every table has a fixed-point shift for these reads (ScoreTable::fixed_shift); otherwise all tables take the FP64
// position path
bool pipeline_score_uses_graph(const DevReads& rd, const BuildState& graph, ScoreTable* const* tbs, u32 n_tables);
// Levenshtein distance of every path of `dp` against `target` (ASCII) on the GPU (k_levenshtein).  *done = false when
// the target holds a byte outside ACGT (the packed form cannot represent it): the caller then uses the host routine.
// Two-sample KS statistic of every path's path_freq against the genome's per-position window probabilities
// (lib/DeNovoAssembler.R:414-424); needs the position counters of a general (non-graph) pipeline_score_launch.
int pipeline_ks(gasm_ctx* ctx, DevPaths& dp, ScoreState& ss, const ScoreTable& tb, const char* genome, u64 genome_len, int kmer, std::vector<double>& ks);
// its two halves: the genome's windows counted per table row (does not depend on the probabilities), and the statistic of
// every path under one table's probabilities
int pipeline_ks_genome_hist(gasm_ctx* ctx, const ScoreTable& tb, const char* genome, u64 genome_len, int kmer, std::vector<u32>& hist);
int pipeline_ks_paths(gasm_ctx* ctx, DevPaths& dp, ScoreState& ss, const ScoreTable& tb, const std::vector<u32>& hist, int kmer, std::vector<double>& ks);
// contig_frac_len (lib/DeNovoAssembler.R:432-445)
int pipeline_coverage(gasm_ctx* ctx, const long long* start, const long long* len, u64 n, long long seq_len, double* percent);
int pipeline_levenshtein(gasm_ctx* ctx, DevPaths& dp, const char* target, u64 target_len, bool infix, std::vector<int32_t>& lev, bool* done);

// count_read_kmers (kernels_count.hip): every segment's GASM_TABLE_ROWS window counts into d_out, queued on the ctx stream.
// read_kmer_windows_check (host, once per set of reads): GASM_ERR_CAPACITY where a segment holds 2^32 or more windows of
// length 2, the only way a u32 counter could wrap.  read_kmer_split: workgroups per segment (GASM_RKC_SPLIT)
int read_kmer_windows_check(const DevReads& rd);
int launch_read_kmer_count(gasm_ctx* ctx, const DevReads& rd, u32* d_out);
int read_kmer_split();

// grow `b` to `bytes` and queue the copy of `src` into it on the ctx stream (the caller keeps `src` alive until the stream got there)
int h2d(gasm_ctx* ctx, DBuf& b, const void* src, size_t bytes);
// wait for `ticket` to appear at `word` (pinned memory written last by a kernel of the ctx stream); spin, then poll with a deadline
int gasm_wait_word32(gasm_ctx* ctx, const volatile u32* word, u32 ticket);
int gasm_wait_word64(gasm_ctx* ctx, const volatile u64* word, u64 ticket);

// sequence files parsed and packed on the device (ingest.hip); on_device[f] = 0 where the host reader took an irregular file
int ingest_files_device(gasm_ctx* ctx, const char* const* paths, u32 n_files, const gasm_host::IngestOpts& o, DBuf& d_words, std::vector<u64>& read_off,
                        std::vector<u64>& seg, u64* dropped, std::vector<u8>& on_device, std::vector<u64>& stats, std::vector<u64>& hist);
