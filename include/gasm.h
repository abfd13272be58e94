/* gasm.h — C ABI of libgasm, the MI355X (gfx950) implementation of the de Bruijn graph + k-meric breakage scoring
 * hot path of SahakyanLab/GenomeAssembler_dev.
 *
 * This header is the drop-in boundary.  The reference crosses exactly one FFI: R -> C++ through Rcpp::sourceCpp
 * (`// [[Rcpp::export]]` in lib/DeNovoAssembler.cpp:85,214,316 and lib/BreakageScorer.cpp:79,185).  Every entry
 * point below names the exported reference function it replaces; integration/DeNovoAssemblerHIP.cpp (shown in
 * INTEGRATION.md) is the Rcpp glue a maintainer would source instead of the reference file.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross this boundary;
 *   - every function returns GASM_OK (0) or a negative gasm_status; gasm_last_error() (thread-local) has the text;
 *     no exception ever leaves the library (the reference's C++ exceptions become R errors through Rcpp's
 *     BEGIN_RCPP/END_RCPP; the glue re-raises a non-zero status as Rcpp::stop);
 *   - string lists are one byte buffer + n+1 uint64 offsets (string i = data[off[i] .. off[i+1]));
 *   - results are library-allocated objects read through accessors and released with their *_free;
 *   - bases are upper-case ACGT.  2-bit packing cannot hold anything else: other bytes return GASM_ERR_NON_ACGT
 *     (documented divergence: the reference would silently create new hash keys);
 *   - a gasm_ctx owns one GPU (device ordinal given at creation), one HIP stream and its scratch memory; calls on one
 *     ctx must not overlap in time, different ctxs are independent.  There is no CPU fallback: without a usable
 *     gfx950 device gasm_ctx_create fails with GASM_ERR_NO_DEVICE.
 */
#ifndef GASM_H
#define GASM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gasm_status {
    GASM_OK = 0,
    GASM_ERR_INVALID = -1,    /* bad argument (null pointer, k out of range, inconsistent sizes) */
    GASM_ERR_NON_ACGT = -2,   /* a base outside upper-case ACGT */
    GASM_ERR_NO_DEVICE = -3,  /* no usable gfx950 GPU / HIP runtime error at start-up */
    GASM_ERR_HIP = -4,        /* HIP runtime error during a call */
    GASM_ERR_CAPACITY = -5,   /* input exceeds a documented limit */
    GASM_ERR_RANGE = -6,      /* the reference would throw std::out_of_range here (substr past the end) */
    GASM_ERR_STATE = -7,      /* call order violated (e.g. score before build) */
    GASM_ERR_INTERNAL = -8    /* a result contradicts an invariant of the library (a bug: please report it) */
} gasm_status;

#define GASM_MAX_K 63          /* k-mer keys are 64-bit for k <= 31 and 128-bit for 32 <= k <= 63 */
#define GASM_TABLE_ROWS 69904  /* 4^2 + 4^4 + 4^6 + 4^8 rows of the breakage table, in that order, each lexicographic */

typedef struct gasm_ctx gasm_ctx;
typedef struct gasm_contigs gasm_contigs;
typedef struct gasm_strlist gasm_strlist;
typedef struct gasm_scores gasm_scores;
typedef struct gasm_batch gasm_batch;

const char* gasm_last_error(void);
const char* gasm_version(void);

int gasm_ctx_create(int device, gasm_ctx** out);
void gasm_ctx_destroy(gasm_ctx* ctx);
/* waits for everything queued on the ctx stream */
int gasm_ctx_sync(gasm_ctx* ctx);
/* the ctx's hipStream_t as an opaque pointer (for callers that time with their own HIP events) */
void* gasm_ctx_stream(gasm_ctx* ctx);

/* ------------------------------------------------------------------------------------------------------------------
 * get_contigs(read_kmers, dbg_kmer, seed)                       replaces lib/DeNovoAssembler.cpp:86-206
 *   kmers/n_kmers : the exploded k-mers, each exactly dbg_kmer characters, concatenated (what
 *                   lib/DeNovoAssembler.R:109-130 builds); duplicates allowed, order irrelevant.
 *   matrix_rows   : the reference's baked-in 10 000 (lib/DeNovoAssembler.cpp:195); 0 skips the shuffle.
 * Result: the sorted unique contigs (the value of `contigs` after :192) and the shuffle matrix of :195-203 as
 * matrix_rows x count indices into them (row-major).  The shuffle is std::shuffle with std::mt19937(seed) on the
 * host, exactly as the reference draws it.
 * Graph by-products kept for parity checks: the distinct k-mers (sorted, = the distinct edge list) with their
 * multiplicities, 2-bit packed big-endian in `words` 64-bit words per k-mer (1 for k<=31, else 2; base 0 is the most
 * significant pair of the k-mer's 2k bits).
 * ---------------------------------------------------------------------------------------------------------------- */
int gasm_get_contigs(gasm_ctx* ctx, const char* kmers, uint64_t n_kmers, int dbg_kmer, int seed, int matrix_rows,
                     gasm_contigs** out);
/* The same from the reads themselves — get_kmers_from_reads (lib/DeNovoAssembler.R:109-130: substring() of every read at every
 * offset, 31 characters per k-mer handed across the R / C++ boundary) and get_contigs in one call: the k-mers are taken on the
 * GPU from the 2-bit packed reads.  reads: the reads' characters back to back, read_off[n_reads + 1] their offsets; a read
 * shorter than dbg_kmer has no k-mers.  Same result as gasm_get_contigs on the exploded k-mers (the k-mers' order never
 * mattered: lib/DeNovoAssembler.cpp:91-122 counts them). */
int gasm_get_contigs_from_reads(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                int matrix_rows, gasm_contigs** out);
/* The same with a multiplicity cutoff (gasm_batch_build_solid below): only k-mers seen at least min_count times become edges; the
 * distinct k-mers handed back are the survivors, with their true multiplicities.  min_count = 1 is gasm_get_contigs_from_reads,
 * min_count = 0 GASM_ERR_INVALID. */
int gasm_get_contigs_from_reads_solid(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                      int matrix_rows, uint32_t min_count, gasm_contigs** out);
/* The same from both strands (gasm_batch_build_strands below): strands = 2 adds the reverse complement of every read before the
 * k-mers are taken; strands = 1 is gasm_get_contigs_from_reads_solid, anything else GASM_ERR_INVALID. */
int gasm_get_contigs_from_reads_strands(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                        int matrix_rows, uint32_t min_count, uint32_t strands, gasm_contigs** out);
/* The same with tip clipping (gasm_batch_build_tips below): tip_len > 0 removes, for tip_rounds rounds, the short dead-end contigs
 * of the graph before the contigs are cut; tip_len = 0 is gasm_get_contigs_from_reads_strands and tip_rounds is not read. */
int gasm_get_contigs_from_reads_tips(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                     int matrix_rows, uint32_t min_count, uint32_t strands, uint32_t tip_len, uint32_t tip_rounds,
                                     gasm_contigs** out);
/* The same with bubble popping (gasm_batch_build_bubbles below): bubble_len > 0 removes, for bubble_rounds rounds behind the tip
 * rounds, the weaker of parallel short contigs; bubble_len = 0 is gasm_get_contigs_from_reads_tips and bubble_rounds is not read. */
int gasm_get_contigs_from_reads_bubbles(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                        int matrix_rows, uint32_t min_count, uint32_t strands, uint32_t tip_len, uint32_t tip_rounds,
                                        uint32_t bubble_len, uint32_t bubble_rounds, gasm_contigs** out);
/* The positional chain build -> _solid -> _strands -> _tips -> _bubbles ends here: every knob of a build in one struct, for this entry and
 * for gasm_batch_build_params below.  size must be sizeof(gasm_build_params), else GASM_ERR_INVALID (a caller compiled against another
 * header).  Zeroed optional fields mean the defaults of the positional entries: min_count 0 -> 1, strands 0 -> 1, tip_len = 0 no
 * clipping, bubble_len = 0 no popping, cov_cutoff = 0 or cov_len = 0 no low-coverage removal (the rounds of a feature that is off
 * are not read).  genome_len_hint is read by gasm_batch_build_params only. */
typedef struct gasm_build_params {
    uint32_t size;
    int32_t  k;
    uint64_t genome_len_hint;
    uint32_t min_count, strands;
    uint32_t tip_len, tip_rounds;
    uint32_t bubble_len, bubble_rounds;
    uint32_t cov_cutoff, cov_len, cov_rounds;
} gasm_build_params;
/* The same with everything gasm_build_params holds (gasm_batch_build_params below): with cov_cutoff = 0 or cov_len = 0 it is
 * gasm_get_contigs_from_reads_bubbles with the struct's other fields; params->k is the dbg_kmer of the other entries. */
int gasm_get_contigs_from_reads_params(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int seed, int matrix_rows,
                                       const gasm_build_params* params, gasm_contigs** out);
uint64_t gasm_contigs_count(const gasm_contigs* c);
const char* gasm_contigs_data(const gasm_contigs* c);
const uint64_t* gasm_contigs_offsets(const gasm_contigs* c);       /* count+1 */
uint64_t gasm_contigs_rows(const gasm_contigs* c);
const uint32_t* gasm_contigs_perm(const gasm_contigs* c);          /* rows*count */
uint64_t gasm_contigs_distinct_count(const gasm_contigs* c);
int gasm_contigs_key_words(const gasm_contigs* c);
const uint64_t* gasm_contigs_distinct_keys(const gasm_contigs* c); /* distinct_count*words */
const uint32_t* gasm_contigs_distinct_mult(const gasm_contigs* c); /* distinct_count */
void gasm_contigs_free(gasm_contigs* c);

/* ------------------------------------------------------------------------------------------------------------------
 * assemble_contigs(contig_matrix, dbg_kmer)                      replaces lib/DeNovoAssembler.cpp:215-305
 *   the matrix is `rows` rows of `row_len` entries (perm, row-major indices into the `n` distinct strings); for
 *   get_contigs' output every row is a permutation of all n contigs, so row_len == n.
 * assemble_contigs(velvet_contigs, dbg_kmer, seed)               replaces lib/BreakageScorer.cpp:80-174
 *   rows = the reference's baked-in 20 000 (lib/BreakageScorer.cpp:86).
 * Result: distinct scaffolds, longest first (same std::sort call as the reference).  GASM_ERR_RANGE where the
 * reference's substr would throw (a contig shorter than the overlap being tried).
 * ---------------------------------------------------------------------------------------------------------------- */
int gasm_assemble_contigs(gasm_ctx* ctx, const char* contigs, const uint64_t* off, uint64_t n, const uint32_t* perm,
                          uint64_t rows, uint64_t row_len, int dbg_kmer, gasm_strlist** out);
int gasm_assemble_contigs_velvet(gasm_ctx* ctx, const char* contigs, const uint64_t* off, uint64_t n, int dbg_kmer,
                                 int seed, int rows, gasm_strlist** out);
/* The same two functions with the scaffolds left on the GPU (2-bit, the reference's order: longest first) behind a handle
 * that gasm_calc_breakscore_dev takes as its `path` argument: the text of the scaffolds (3.8e8 characters for one 50 kb
 * experiment) is only made when gasm_scaffolds_fetch asks for it.  Same results as the string forms. */
typedef struct gasm_scaffolds gasm_scaffolds;
int gasm_assemble_contigs_dev(gasm_ctx* ctx, const char* contigs, const uint64_t* off, uint64_t n, const uint32_t* perm,
                              uint64_t rows, uint64_t row_len, int dbg_kmer, gasm_scaffolds** out);
int gasm_assemble_contigs_velvet_dev(gasm_ctx* ctx, const char* contigs, const uint64_t* off, uint64_t n, int dbg_kmer, int seed,
                                     int rows, gasm_scaffolds** out);
uint64_t gasm_scaffolds_count(const gasm_scaffolds* s);
/* who ran the greedy merge behind these scaffolds: 1 the GPU (k_asm_merge), 2 host threads, 3 both (*rows_on_host of the
 * permutations went back to the host routine: two chains of equal length need the reference's full-string test) */
int gasm_scaffolds_merge_device(const gasm_scaffolds* s, uint64_t* rows_on_host);
const uint64_t* gasm_scaffolds_offsets(const gasm_scaffolds* s);   /* count + 1 base offsets: lengths without a fetch */
int gasm_scaffolds_fetch(const gasm_scaffolds* s, gasm_strlist** out);
void gasm_scaffolds_free(gasm_scaffolds* s);
uint64_t gasm_strlist_count(const gasm_strlist* s);
const char* gasm_strlist_data(const gasm_strlist* s);
const uint64_t* gasm_strlist_offsets(const gasm_strlist* s);
void gasm_strlist_free(gasm_strlist* s);

/* ------------------------------------------------------------------------------------------------------------------
 * calc_breakscore(path, sequencing_reads, true_solution, kmer, bp_kmer, bp_prob)
 *   variant GASM_SCORE_OWN    replaces lib/DeNovoAssembler.cpp:317-477  (returns path_freq)
 *   variant GASM_SCORE_VELVET replaces lib/BreakageScorer.cpp:186-353   (returns path_prob_dist(+_startpos),
 *                                                                         Levenshtein in infix mode)
 * flags: GASM_WANT_LEV computes lev_dist_vs_true (else zeros) — global distance for the own variant, infix for the velvet
 *        one, as the reference's two calc_levenshtein do; on the GPU when that is the quicker place (many or long paths),
 *        on the host for a handful of short ones or a true_solution with bytes outside ACGT (same numbers either way;
 *        GASM_LEV_GPU / GASM_LEV_HOST in the environment force one or the other); GASM_WANT_FREQ materialises the dense path_freq
 * (n_paths x n_table doubles, in bp_kmer order — the reference emits them in hash-iteration order, so only the
 * multiset per path is defined there).
 * bp_kmer keys must be distinct ACGT strings of length 1..8 (the reference tables hold lengths 2,4,6,8).
 * Scores are FP64, summed in a fixed order (deterministic run to run); the reference sums in hash-iteration order.
 * Numeric contract (u = 2^-53, per path m = kmer_breaks and S = sum |p * c| over the hit rows): bp_score and
 * norm_by_break_freqs lie within (m+2) u S (S / kmer_breaks for the latter) of the exact sums, whatever the summation order;
 * norm_by_len == bp_score / len and every path_freq entry == the correctly rounded count / kmer_breaks, bit for bit; NaN and
 * infinite table rows that are hit follow IEEE double arithmetic.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_SCORE_OWN 0
#define GASM_SCORE_VELVET 1
#define GASM_WANT_LEV 1
#define GASM_WANT_FREQ 2
#define GASM_WANT_KS 4       /* stat_test_KS per path: lib/DeNovoAssembler.R:414-424 (own variant; true_solution must be ACGT) */
int gasm_calc_breakscore(gasm_ctx* ctx, const char* paths, const uint64_t* path_off, uint64_t n_paths,
                         const char* reads, const uint64_t* read_off, uint64_t n_reads, const char* true_solution,
                         uint64_t true_len, int kmer, const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table,
                         const double* bp_prob, int variant, int flags, gasm_scores** out);
/* calc_breakscore of device-resident scaffolds (gasm_assemble_contigs_dev); everything else as gasm_calc_breakscore */
int gasm_calc_breakscore_dev(gasm_ctx* ctx, const gasm_scaffolds* paths, const char* reads, const uint64_t* read_off, uint64_t n_reads,
                             const char* true_solution, uint64_t true_len, int kmer, const char* bp_kmer, const uint64_t* bp_off,
                             uint64_t n_table, const double* bp_prob, int variant, int flags, gasm_scores** out);
uint64_t gasm_scores_count(const gasm_scores* s);
const int32_t* gasm_scores_sequence_len(const gasm_scores* s);
const double* gasm_scores_bp_score(const gasm_scores* s);
const double* gasm_scores_norm_by_break_freqs(const gasm_scores* s);
const double* gasm_scores_norm_by_len(const gasm_scores* s);
const int32_t* gasm_scores_kmer_breaks(const gasm_scores* s);
const int32_t* gasm_scores_lev_dist(const gasm_scores* s);
const double* gasm_scores_path_freq(const gasm_scores* s);          /* count*n_table or NULL */
const int32_t* gasm_scores_startpos(const gasm_scores* s);          /* velvet variant, else NULL */
const double* gasm_scores_prob_dist(const gasm_scores* s);          /* velvet: concatenated, see offsets */
const uint64_t* gasm_scores_prob_dist_offsets(const gasm_scores* s);/* count+1 */
/* two-sample Kolmogorov-Smirnov statistic D of the path's path_freq (NaN entries dropped) against the probabilities of
 * the true solution's kmer-long windows (kmer_from_seq, lib/GenerateReads.R:243-259): what ks.test(...)$statistic gives in
 * lib/DeNovoAssembler.R:419-424; NaN where no read matched (R stops with an error there).  NULL without GASM_WANT_KS. */
const double* gasm_scores_ks(const gasm_scores* s);
/* who computed lev_dist_vs_true: 0 nobody (not asked for), 1 the GPU (k_levenshtein), 2 host threads (a cost model prefers them
 * for a handful of short paths; targets with bytes outside ACGT; GASM_LEV_HOST) — same numbers either way */
int gasm_scores_lev_device(const gasm_scores* s);
void gasm_scores_free(gasm_scores* s);

/* ------------------------------------------------------------------------------------------------------------------
 * calc_breakscore under several breakage tables at once: what score_solutions() needs (lib/DeNovoAssembler.R:325-355 runs
 * calc_breakscore twice per experiment, `for random_prob in (FALSE, TRUE)`: same paths, reads and true solution, only
 * bp_prob differs — the true table, then the uniform one).
 *   bp_probs: n_tables rows of n_table probabilities (row-major), all for the keys bp_kmer; n_tables in 1..GASM_MAX_TABLES,
 *   else GASM_ERR_INVALID.  out: n_tables entries; out[t] is an ordinary gasm_scores (every accessor above; free each with
 *   gasm_scores_free) holding bit for bit what gasm_calc_breakscore(..., bp_probs + t * n_table, ...) returns with the same
 *   variant and flags (gasm_calc_breakscore is the n_tables = 1 case of the same code).  On any error every out[t] is NULL.
 * Done once per call (none of it depends on the table): read upload and index, the first occurrence of every read in every
 * path, kmer_breaks, sequence_len, lev_dist_vs_true (GPU or host, as gasm_calc_breakscore chooses), the velvet variant's
 * startpos, the genome's row histogram for the KS statistic, and the path_freq counts — count / total, one dense buffer
 * shared by the n_tables result objects (gasm_scores_path_freq returns the same pointer for each; it lives until the last
 * of them is freed).  Done per table: bp_score, norm_by_break_freqs, norm_by_len (one kernel gathers the T probabilities of
 * a hit position; per table the summation order of the single-table call), the KS statistic (it ranks the table's
 * probabilities) and the velvet variant's path_prob_dist.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAX_TABLES 8
int gasm_calc_breakscore_tables(gasm_ctx* ctx, const char* paths, const uint64_t* path_off, uint64_t n_paths, const char* reads,
                                const uint64_t* read_off, uint64_t n_reads, const char* true_solution, uint64_t true_len, int kmer,
                                const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table, const double* bp_probs, uint32_t n_tables,
                                int variant, int flags, gasm_scores** out);
int gasm_calc_breakscore_tables_dev(gasm_ctx* ctx, const gasm_scaffolds* paths, const char* reads, const uint64_t* read_off,
                                    uint64_t n_reads, const char* true_solution, uint64_t true_len, int kmer, const char* bp_kmer,
                                    const uint64_t* bp_off, uint64_t n_table, const double* bp_probs, uint32_t n_tables, int variant,
                                    int flags, gasm_scores** out);

/* contig_frac_len of lib/DeNovoAssembler.R:432-445: percentage of [1, seq_len] covered by the union of the inclusive
 * ranges [start_i, start_i + len_i] (GRanges reduce + setdiff). */
int gasm_coverage_percent(gasm_ctx* ctx, const int64_t* start, const int64_t* len, uint64_t n, int64_t seq_len, double* percent);

/* Levenshtein distance as the reference takes it from edlib (lib/DeNovoAssembler.cpp:41-55 global,
 * lib/BreakageScorer.cpp:41-55 infix); 0 for an empty operand, like the reference's failure branch. */
int gasm_levenshtein(const char* query, uint64_t nq, const char* target, uint64_t nt, int infix, int32_t* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Segment batches: the reads-in / contigs+scores-out surface for many independent segments at once (the reference
 * loops `for(i in 1:total_iters)` over independent segments, scripts/02_Real_vs_rand_prob_own.R:33-53).  No
 * reference function takes reads directly: k-mer extraction is R code (lib/DeNovoAssembler.R:109-130); here it is
 * the first kernel.  All data stays in HBM between the three calls; only gasm_batch_fetch_* copies back.
 *
 *   reads        : all reads of all segments, concatenated ASCII, segment after segment
 *   read_off     : n_reads+1 offsets, or NULL when every read has fixed_len bases
 *   seg_read_off : n_segments+1 indices into the read list
 * gasm_batch_build(k)  : k-mers -> distinct k-mers + multiplicities -> (k-1)-mer graph -> contigs, per segment
 *                        (get_contigs without the shuffle; results identical to calling it per segment)
 * gasm_batch_score     : calc_breakscore (own variant, without Levenshtein/path_freq) of every segment's contigs
 *                        against that segment's reads; table = GASM_TABLE_ROWS normalised probabilities (any doubles).
 *                        Fixed point when every read holds a k-mer, the table is all finite and a shift with
 *                        max|p| * (most reads of a segment) * 2^shift in [2^60, 2^62) lies in [0, 1000]: per path
 *                        fx = sum round(p * 2^shift) exactly, bp_score == fx * 2^-shift, norm_by_break_freqs ==
 *                        bp_score / kmer_breaks (0 without hits), norm_by_len == bp_score / len, bit for bit, and
 *                        |bp_score - exact| <= m 2^-(shift+1) + u |exact|.  Otherwise the FP64 scorer of
 *                        gasm_calc_breakscore, with its contract; gasm_batch_fetch_score_fixed and gasm_batch_guided then
 *                        return GASM_ERR_STATE.
 * Both queue work on the ctx stream and return; gasm_ctx_sync (or any fetch) waits.
 * ---------------------------------------------------------------------------------------------------------------- */
int gasm_batch_create(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, uint32_t fixed_len,
                      const uint64_t* seg_read_off, uint32_t n_segments, gasm_batch** out);
/* the same from reads that are 2-bit packed already: A=0 C=1 G=2 T=3, first base in the two most significant bits of words[0],
 * 32 bases per word, reads back to back (read i = bases [read_off[i], read_off[i+1]), or i * fixed_len); a quarter of the
 * bytes over PCIe and no packing kernel */
int gasm_batch_create_packed(gasm_ctx* ctx, const uint64_t* words, const uint64_t* read_off, uint64_t n_reads, uint32_t fixed_len,
                             const uint64_t* seg_read_off, uint32_t n_segments, gasm_batch** out);
/* FASTQ / FASTA in: one file per segment (FASTQ with four-line records, FASTA with one- or multi-line sequences, plain or
 * gzip; lower case folded to upper case).  The reference has no reader of its own on this path (reads are simulated in R
 * and written as FASTA, lib/GenerateReads.R:405-433).  on_non_acgt: 0 = reads holding a byte outside ACGT are dropped and
 * counted in *dropped_reads, 1 = GASM_ERR_NON_ACGT.  The host packs 2-bit while it parses. */
int gasm_batch_from_files(gasm_ctx* ctx, const char* const* paths, uint32_t n_files, int on_non_acgt, gasm_batch** out,
                          uint64_t* dropped_reads);
/* Simulated reads, made on the device (lib/GenerateReads.R:235-313): per segment ceil(coverage * L / read_len) start
 * positions drawn with replacement, the weight of a position = table probability of the kmer-long window starting there
 * (table = the GASM_TABLE_ROWS normalised probabilities, kmer in {2,4,6,8}; table = NULL: every one of the L - kmer + 1
 * positions weighs the same), starts whose read would run past the end dropped, reads = substrings of the genome, forward
 * strand.  R's sample()/set.seed stream is not reproducible without R; the draws here are a documented counter-based
 * generator (kernels_sim.hip), identical for the same (seed, genomes) and restated by the oracle.
 * gasm_batch_fetch_read_starts: the 0-based start of every read in its genome (n_segments + 1 offsets, n_reads starts). */
int gasm_batch_simulate(gasm_ctx* ctx, const char* genomes, const uint64_t* genome_off, uint32_t n_segments, uint32_t read_len,
                        double coverage, uint64_t seed, int kmer, const double* table, gasm_batch** out);
int gasm_batch_fetch_read_starts(gasm_batch* b, const uint64_t** seg_read_off, const uint32_t** starts);
/* the reader alone (host only, no GPU needed): the reads of the files, packed as gasm_batch_create_packed takes them */
typedef struct gasm_packed gasm_packed;
int gasm_read_files(const char* const* paths, uint32_t n_files, int on_non_acgt, gasm_packed** out);
/* The same through the device path (csrc/ingest.hip): the host opens and inflates the file, the GPU finds the records (newline
 * scan), validates and 2-bit packs them; a text it does not recognise as plain four-line FASTQ or FASTA goes to the host reader,
 * whose grammar is the definition (gasm_packed_parsed_on_device(g, file) = 0 then).  Same results as gasm_read_files. */
int gasm_read_files_device(gasm_ctx* ctx, const char* const* paths, uint32_t n_files, int on_non_acgt, gasm_packed** out);
int gasm_packed_parsed_on_device(const gasm_packed* g, uint32_t file);
uint64_t gasm_packed_n_reads(const gasm_packed* g);
uint32_t gasm_packed_n_segments(const gasm_packed* g);
const uint64_t* gasm_packed_words(const gasm_packed* g);
const uint64_t* gasm_packed_read_off(const gasm_packed* g);        /* n_reads + 1 */
const uint64_t* gasm_packed_seg_read_off(const gasm_packed* g);    /* n_segments + 1 */
uint64_t gasm_packed_dropped(const gasm_packed* g);
void gasm_packed_free(gasm_packed* g);
/* ---- Quality trimming at ingest ------------------------------------------------------------------------------------------------
 * The file entries above with options: FASTQ records trimmed by base quality, filtered by length, mates kept together, and a report
 * of what was done.  size must be sizeof(gasm_ingest_params), else GASM_ERR_INVALID (as gasm_build_params).  With every field but
 * size and on_non_acgt zero an entry below is the plain entry of the same name: the same host code, the same kernel launches.  The
 * plain entries fill the struct with their on_non_acgt and take the same path.
 *
 * THE RULE, per FASTQ record.  L = length of the sequence line as the reader takes it (CR and trailing blanks removed); the quality
 * line is trimmed the same way.
 *   Quality mode: on iff trim_q3 > 0 or trim_q5 > 0 or quality_hist != 0; only then are quality lines read at all.  In quality mode
 *     a record whose quality line is not L bytes long, or holds a byte outside [phred_offset, phred_offset + 93], is
 *     GASM_ERR_INVALID; the message names the file and the lowest such record index (0-based).
 *   Base quality: q_i = byte_i - phred_offset; for trimming, a base outside ACGTacgt has q_i = 0 whatever its byte says.
 *   3' end (BWA / cutadapt's running sum): s = 0, best = 0, e = L; for i = L-1 down to 0: s += trim_q3 - q_i; if s < 0 stop;
 *     if s > best: best = s, e = i.  Strictly greater: of equal candidates the outermost stays and less is trimmed.
 *     trim_q3 = 0: e = L.
 *   5' end, over the WHOLE read (not over [0, e)): s = 0, best = 0, a = 0; for i = 0 .. L-1: s += trim_q5 - q_i; if s < 0 stop;
 *     if s > best: best = s, a = i + 1.  trim_q5 = 0: a = 0.
 *   Span: [a, e) is kept.  a >= e: the span is empty, trimmed3 = L - e, trimmed5 = min(a, e).
 *   Class, exactly one per record, the earlier wins:
 *     non_acgt  the span holds a base outside ACGT (a terminal N that was trimmed does not count); on_non_acgt = 1: GASM_ERR_NON_ACGT
 *     short     the span has fewer than min_len bases (min_len = 0 keeps empty reads)
 *     mate      pairs = 1 and the record's mate (record r ^ 1 of the file) is non_acgt or short.  pairs = 1 and an odd number of
 *               records in a file: GASM_ERR_INVALID.  pairs means interleaved files only.
 *     kept
 *   Errors are met in record order: the lowest record that is malformed or (on_non_acgt = 1) non_acgt decides.
 * FASTA has no qualities: the cutoffs and the histogram do not apply to it, min_len and pairs apply to whole records.
 * Not done: adapter removal, sliding windows, per-base masking; qualities are not kept past the ingest.
 *
 * Statistics, per file (= segment), GASM_INGEST_STATS uint64 in this order: records, kept, dropped_non_acgt, dropped_short,
 * dropped_mate, bases_in, bases_kept (span bases of kept records), bases_dropped (span bases of the others), trimmed5, trimmed3 (over
 * all records), reads_trimmed (kept records that lost a base).  records = kept + the three drops; bases_in = bases_kept + bases_dropped
 * + trimmed5 + trimmed3.  The dropped-reads count of the plain accessors is the sum of the three drops.  The histogram (quality_hist
 * = 1, FASTQ): GASM_QUAL_BINS uint64 per file, bin q = positions of all records, before trimming, whose byte says quality q (an N
 * under its own byte).  Both are collected when an option besides on_non_acgt is set; after a plain ingest the accessors return
 * NULL and the fetch GASM_ERR_STATE.
 * The device entries trim with one wave per record (csrc/ingest.hip, k_ing_qual_trim); an irregular FASTQ, and a FASTA file under
 * min_len or pairs (record lengths there are sums over lines), are read by the host reader (gasm_packed_parsed_on_device = 0). */
typedef struct gasm_ingest_params {
    uint32_t size;           /* sizeof(gasm_ingest_params) */
    uint32_t on_non_acgt;    /* 0 drop and count, 1 error */
    uint32_t phred_offset;   /* 0 -> 33; 33 or 64 */
    uint32_t trim_q3, trim_q5;   /* 0..93, 0 = that end is not trimmed */
    uint32_t min_len;
    uint32_t pairs;          /* 0 / 1 */
    uint32_t quality_hist;   /* 0 / 1 */
} gasm_ingest_params;
#define GASM_INGEST_STATS 11
#define GASM_QUAL_BINS 94
int gasm_read_files_params(const char* const* paths, uint32_t n_files, const gasm_ingest_params* params, gasm_packed** out);
int gasm_read_files_device_params(gasm_ctx* ctx, const char* const* paths, uint32_t n_files, const gasm_ingest_params* params,
                                  gasm_packed** out);
int gasm_batch_from_files_params(gasm_ctx* ctx, const char* const* paths, uint32_t n_files, const gasm_ingest_params* params,
                                 gasm_batch** out, uint64_t* dropped_reads);
const uint64_t* gasm_packed_ingest_stats(const gasm_packed* g);    /* n_segments * GASM_INGEST_STATS */
const uint64_t* gasm_packed_quality_hist(const gasm_packed* g);    /* n_segments * GASM_QUAL_BINS */
/* the same two arrays of a batch made by gasm_batch_from_files_params */
int gasm_batch_fetch_ingest_stats(gasm_batch* b, const uint64_t** stats, const uint64_t** quality_hist);
void gasm_batch_free(gasm_batch* b);
/* genome_len_hint: expected distinct k-mers per segment (0 = derive from the k-mer count); only sizes buckets.
 * build and score only QUEUE their work (no host wait); the fetches below wait for it.  A batch keeps up to four
 * "step slots" — everything a step writes, on a stream of its own — and consecutive builds take them in
 * turn, so `build; score; build; score; ...` without a fetch in between runs step n + 1's streaming kernels beside step n's
 * graph and scoring kernels.  Every step still does all of its work, and every fetch returns the results of the LAST build
 * and score, bit for bit what one step at a time gives (GASM_PINGPONG=0 in the environment: exactly that; GASM_STEP_SLOTS:
 * 2..4 slots, default 3). */
int gasm_batch_build(gasm_batch* b, int k, uint64_t genome_len_hint);
int gasm_batch_score(gasm_batch* b, int kmer, const double* table);
/* ------------------------------------------------------------------------------------------------------------------
 * Solid k-mers: a build with a multiplicity cutoff.  (No counterpart in the reference, whose simulated reads are error-free;
 * Velvet calls the knob -cov_cutoff.  min_count = 1 is the reference's graph.)
 * One substituted base in a read makes up to k k-mers that occur once, each a spurious edge.  gasm_batch_build_solid keeps, after
 * the de-duplication, the distinct k-mers of a segment whose multiplicity IN THAT SEGMENT is >= min_count; everything downstream
 * — graph, contigs, scores, guided traversal, gasm_batch_fetch_distinct / _graph — sees the survivors only, with their true
 * multiplicities.  A read scores on a contig iff it is a substring of it: a read that holds a dropped k-mer lies in no contig and
 * adds nothing.  A segment without survivors behaves like an empty one.
 *   gasm_batch_build(b, k, hint) is gasm_batch_build_solid(b, k, hint, 1): same results, same kernel launches.
 *   min_count == 0: GASM_ERR_INVALID.  Each step slot remembers the cutoff of the build it holds.
 * (after a build with tip clipping, below, distinct_after still counts the survivors of the CUTOFF: the k-mers of
 * gasm_batch_fetch_distinct are distinct_after minus the segment's clipped k-mers of gasm_batch_fetch_tip_stats)
 * (the same after a build with bubble popping, further below: distinct_after adds back the popped k-mers of
 * gasm_batch_fetch_bubble_stats as it adds back the clipped ones; and after a build with low-coverage removal, below that: the removed
 * k-mers of gasm_batch_fetch_lowcov_stats)
 * genome_len_hint for noisy reads: it sizes the buckets for the distinct k-mers BEFORE the cutoff, and reads with errors hold
 * 5-10x more of them than their genome: about genome length + bases in the segment's reads x error rate x k (every wrong base
 * makes up to k new k-mers).  A smaller hint (the genome length alone) is still correct: the tables overflow, the build repeats
 * itself with the next larger configuration (gasm_batch_build_plan: GASM_PLAN_DISTINCT_ATTEMPTS > 1) and filters again.  0 derives
 * the size from the k-mer count, which is usually large enough.
 * gasm_batch_fetch_solid_stats   per segment, the distinct k-mers of the last build before and after its cutoff (n_segments entries
 *                                each; equal when min_count was 1).  Host copies, valid until the next call or build.
 * gasm_batch_kmer_spectrum       queues the multiplicity histogram of the last build's distinct k-mers (as the build left them: after
 *                                its cutoff); GASM_ERR_STATE before a build.  It reads the build's arrays only and changes no build
 *                                or score result.
 * gasm_batch_fetch_kmer_spectrum hist[s * 256 + m] = distinct k-mers of segment s with multiplicity m; multiplicities >= 255 are
 *                                counted in bin 255, bin 0 is always 0.  GASM_ERR_STATE without a spectrum of the last build.
 *                                Intended use: build with min_count = 1, read the spectrum, put the cutoff into the valley between
 *                                the error peak at 1 and the coverage peak, build again.
 * ---------------------------------------------------------------------------------------------------------------- */
int gasm_batch_build_solid(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count);
int gasm_batch_fetch_solid_stats(gasm_batch* b, const uint64_t** distinct_before, const uint64_t** distinct_after);
int gasm_batch_kmer_spectrum(gasm_batch* b);
int gasm_batch_fetch_kmer_spectrum(gasm_batch* b, const uint64_t** hist /* n_segments x 256 */);
/* ------------------------------------------------------------------------------------------------------------------
 * Both strands: a build from the reads and their reverse complements.  (No counterpart in the reference's assembler, which takes
 * its k-mers forward-strand only; its simulator writes read_2 as reverse complements, lib/GenerateReads.R:438.  Velvet's "twin"
 * nodes.  strands = 1 is the reference's graph and the default everywhere.)
 * A sequencer reads both strands; forward-only k-mers make two unconnected half-coverage graphs of such reads.  With strands = 2
 * a build sees, for every read r of a segment, the k-mers of r and the k-mers of rc(r) (r reversed, A<->T and C<->G swapped), and
 * everything behind the de-duplication sees that multiset:
 *   - the multiplicity of a k-mer x is count(x) + count(rc(x)) over the segment's reads; a k-mer that is its own reverse
 *     complement (even k only) therefore counts TWICE per occurrence;
 *   - min_count applies to these sums; gasm_batch_fetch_solid_stats, the k-mer spectrum, gasm_batch_fetch_distinct and
 *     gasm_batch_fetch_graph report the both-strand set; gasm_batch_total_kmers is twice the forward count;
 *   - the contigs of a segment are closed under reverse complement: the twin of every contig is a contig of the same segment
 *     (the branching rule treats a node and its reverse complement alike); a contig may be its own twin (even k).
 * Scoring is over the ORIGINAL reads only, each once: a read scores on a contig iff it is a substring of it, so a reverse-strand
 * read scores on the twin of the contig its forward form lies in.  The fixed-point shift is unchanged (it depends on the most
 * reads of a segment).  The guided traversal works on such a build as on any other.
 * gasm_batch_build_strands        strands = 1 is gasm_batch_build_solid: same host path, same kernel launches; strands = 2 as above;
 *                                 anything else GASM_ERR_INVALID.  genome_len_hint keeps meaning the genome's length (for noisy
 *                                 reads: see above); the library doubles its own estimate of the distinct k-mers.  The
 *                                 reverse-complemented read stream is made once per batch, by the first strands = 2 build, and
 *                                 costs as much device memory again as the packed reads.  Each step slot remembers the strands
 *                                 of the build it holds, as it remembers the cutoff.
 * gasm_batch_strands              strands of the last build (0 before the first).
 * gasm_batch_fetch_contig_twins   twin[c] = the index, INSIDE ITS SEGMENT, of the contig whose text is rc(contig c); one entry per
 *                                 contig in the order of gasm_batch_fetch_contigs; an involution; twin[c] == c for a self-twin.
 *                                 Host copy, valid until the next build.  GASM_ERR_STATE before a build or after a strands = 1
 *                                 build; GASM_ERR_INTERNAL if a contig has no twin (the closure above would be broken).
 * Pooled builds (gasm_pool_*) are forward-strand only and clip no tips (below).  They pop no bubbles either (further below).
 * They remove no low-coverage contigs (below that).
 * ---------------------------------------------------------------------------------------------------------------- */
int gasm_batch_build_strands(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count, uint32_t strands);
uint32_t gasm_batch_strands(const gasm_batch* b);
int gasm_batch_fetch_contig_twins(gasm_batch* b, const uint32_t** twin);
/* ------------------------------------------------------------------------------------------------------------------
 * Tip clipping: short dead-end branches leave the k-mer set before the contigs are cut.  (No counterpart in the reference, which
 * never simplifies its graph; Velvet clips tips right behind its coverage cutoff.  tip_len = 0 is the reference's graph and the
 * default everywhere.)
 * A substitution near the end of a read makes fewer than k wrong k-mers: a short branch that leaves the true path and ends
 * nowhere.  A cutoff removes most of them, but a tip seen min_count times survives, and every surviving tip makes its junction a
 * branching node, which cuts the true contig in two.  gasm_batch_build_tips removes tips from the k-mer set that survived the
 * cutoff, for exactly tip_rounds rounds; graph, contigs, scores and every by-product are made from what is left.
 * The rule, on the graph of a segment as everywhere here (edges = distinct k-mers with their multiplicities, nodes = (k-1)-mers,
 * degrees count distinct edges, contigs = the paths from branching node to branching node).  One round, on the current set:
 *   for a contig c let u = its first k-1 bases, v = its last k-1 bases, e_first = its first k-mer, e_last = its last k-mer;
 *   c is a FORWARD tip  if out(v) == 0 and u has another out-edge f != e_first with mult(f) > mult(e_first);
 *   c is a BACKWARD tip if in(u) == 0  and v has another in-edge  f != e_last  with mult(f) > mult(e_last);
 *   c is clipped if len(c) <= tip_len (bases) and it is a forward or a backward tip.
 *   The comparison is strict: among siblings of equal multiplicity nobody is clipped, and there is no tie-break by key (a key
 *   order is not symmetric under reverse complement).  A contig with nothing attached at either end is not a tip and stays.
 *   All tips of a round are found on the same graph and leave together, with all their k-mers (a k-mer lies in at most one
 *   contig); the next round starts from the remaining set.
 * A build runs exactly tip_rounds rounds — a round that finds nothing changes nothing —, so it stays queued as a whole: the host
 * does not wait between rounds.  gasm_batch_fetch_tip_stats tells whether the last round still found something.
 * With strands = 2 the multiplicities are symmetric under reverse complement: a forward tip's twin is a backward tip and is
 * clipped in the same round, the contigs stay closed under reverse complement and gasm_batch_fetch_contig_twins keeps working.
 * The intended setting is tip_len = 2k - 1 (Velvet: "shorter than 2k"); tip_len < k can match no contig and is allowed.
 * tip_len has no upper limit, but its cost has: in every round one GPU thread per contig of at most tip_len bases walks that
 * contig edge by edge (tip_len - k + 1 dependent loads at most).  That is nothing at 2k - 1; with a tip_len of thousands a
 * long unbranched contig is one thread's walk in every round — still correct and bounded by the segment, only slow.
 * Everything behind the build — contigs, gasm_batch_fetch_distinct / _graph, the k-mer spectrum, twins, scores under one or
 * several tables, the guided traversal — sees the clipped set with its true multiplicities.  A read scores on a contig iff it is
 * a substring of it: a read that holds a clipped k-mer adds nothing.
 * gasm_batch_build_tips         tip_len == 0 is gasm_batch_build_strands: same host path, same kernel launches, tip_rounds is
 *                               not read.  tip_len > 0 needs tip_rounds in 1..GASM_MAX_TIP_ROUNDS, else GASM_ERR_INVALID.  Each
 *                               step slot remembers tip_len and tip_rounds of the build it holds, as it remembers the cutoff
 *                               and the strands.
 * gasm_batch_tip_len / _tip_rounds   of the last build (0: no clipping, or no build yet).
 * gasm_batch_fetch_tip_stats    tips[s * GASM_MAX_TIP_ROUNDS + r] = contigs clipped in segment s, round r; kmers[...] = k-mers
 *                               clipped, same index; rounds not run are 0.  Host copies, valid until the next call or build.
 *                               GASM_ERR_STATE before a build or after a build with tip_len == 0.
 * Pooled builds (gasm_pool_*) do not clip.  They do not remove low-coverage contigs either.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAX_TIP_ROUNDS 8
int gasm_batch_build_tips(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count, uint32_t strands,
                          uint32_t tip_len, uint32_t tip_rounds);
uint32_t gasm_batch_tip_len(const gasm_batch* b);      /* of the last build; 0: none */
uint32_t gasm_batch_tip_rounds(const gasm_batch* b);
int gasm_batch_fetch_tip_stats(gasm_batch* b, const uint32_t** tips, const uint32_t** kmers);
/* ------------------------------------------------------------------------------------------------------------------
 * Bubble popping: of two parallel short paths the weaker leaves the k-mer set before the contigs are cut.  (No counterpart in the
 * reference; Velvet (Tour Bus) and SPAdes pop bubbles after they clip tips.  bubble_len = 0 is the default everywhere.)
 * A substitution in the middle of a read makes k wrong k-mers: a second path of k edges that leaves the true path at one node and
 * rejoins it k edges later.  Both ends stay attached, so it is no tip; seen min_count times it survives the cutoff; and each such
 * bubble cuts the true contig in three and adds a fourth, false one.  gasm_batch_build_bubbles removes bubbles from the k-mer set
 * that the cutoff and the tip rounds left, for exactly bubble_rounds rounds; everything else is made from what is left.
 * The rule, on the same graph as the tip rule (edges = distinct k-mers with their multiplicities, nodes = (k-1)-mers, contigs =
 * what the build would cut).  For a contig c let u(c) = its first node, v(c) = its last node, n(c) = its edges, m(c) = the sum of
 * its edges' multiplicities, len(c) = n(c) + k - 1 bases.  One round, on the current set:
 *   c and d are PARALLEL if d != c, u(d) == u(c) and v(d) == v(c).  (d starts with a sibling out-edge of c's first edge: every
 *   out-edge of a node with two or more is the head of a contig.)
 *   c is POPPED if len(c) <= bubble_len and a parallel d exists with len(d) <= bubble_len and STRICTLY higher mean multiplicity:
 *   m(d) * n(c) > m(c) * n(d), compared exactly in 64-bit integers.
 *   The two paths need not be equally long (an indel makes them differ).  The comparison is strict, with no tie-break by key:
 *   among parallel paths of equal mean multiplicity nobody is popped, for the reason given for tips (a key order is not symmetric
 *   under reverse complement).  With strands = 2 the twin of a popped contig is popped in the same round, and two paths that are
 *   each other's twin tie and both stay.  Of three parallel paths the two weaker go in the same round.  u == v (two parallel
 *   loops) gets no special case.
 *   All bubbles of a round are found on the same graph and leave together, with all their k-mers (a k-mer lies in at most one
 *   contig); the next round starts from the remaining set.
 * A build runs exactly bubble_rounds rounds, queued as a whole, AFTER all tip rounds: a tip that hangs on a bubble's branch splits
 * that branch, so the bubble is only seen once the tip is gone.  A nested bubble — a bubble inside one branch of a larger one —
 * takes two rounds: the inner one goes first, then the re-joined branch.
 * STATED LIMIT: two bubbles that OVERLAP are not popped by this rule — two errors less than k apart in different reads, say, each
 * branching off inside the other's span: neither has a parallel contig, because the true path between their ends is itself cut.
 * Tour Bus handles that case; this rule does not try to.
 * bubble_len <= GASM_MAX_BUBBLE_LEN keeps m * n inside 64 bits for any 32-bit multiplicities and bounds a GPU thread's walk: in
 * every round one thread per short contig that has siblings walks its own chain and those of at most three siblings, edge by edge.
 * The intended setting is 2k - 1, the exact length of a single-substitution bubble; bubble_len < k can match no contig and is
 * allowed.  As for tip_len, a bubble_len of thousands is paid for in dependent loads: still correct, only slow.
 * Everything behind the build — contigs, gasm_batch_fetch_distinct / _graph, the k-mer spectrum, twins, scores under one or
 * several tables, the guided traversal — sees the popped set with its true multiplicities.  A read scores on a contig iff it is a
 * substring of it: a read that holds a popped k-mer adds nothing.
 * gasm_batch_build_bubbles      bubble_len == 0 is gasm_batch_build_tips: same host path, same kernel launches, bubble_rounds is
 *                               not read.  bubble_len > 0 needs bubble_len <= GASM_MAX_BUBBLE_LEN and bubble_rounds in
 *                               1..GASM_MAX_BUBBLE_ROUNDS, else GASM_ERR_INVALID.  Each step slot remembers both of the build it
 *                               holds, as it remembers tip_len and tip_rounds.
 * gasm_batch_bubble_len / _bubble_rounds   of the last build (0: no popping, or no build yet).
 * gasm_batch_fetch_bubble_stats bubbles[s * GASM_MAX_BUBBLE_ROUNDS + r] = contigs popped in segment s, round r; kmers[...] =
 *                               k-mers popped, same index; rounds not run are 0.  Host copies, valid until the next call or
 *                               build.  GASM_ERR_STATE before a build or after a build with bubble_len == 0.
 * Pooled builds (gasm_pool_*) pop no bubbles.  They remove no low-coverage contigs either.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAX_BUBBLE_ROUNDS 8
#define GASM_MAX_BUBBLE_LEN 65535
int gasm_batch_build_bubbles(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count, uint32_t strands,
                             uint32_t tip_len, uint32_t tip_rounds, uint32_t bubble_len, uint32_t bubble_rounds);
uint32_t gasm_batch_bubble_len(const gasm_batch* b);   /* of the last build; 0: none */
uint32_t gasm_batch_bubble_rounds(const gasm_batch* b);
int gasm_batch_fetch_bubble_stats(gasm_batch* b, const uint32_t** bubbles, const uint32_t** kmers);
/* ------------------------------------------------------------------------------------------------------------------
 * Low-coverage removal: short contigs of low mean multiplicity leave the k-mer set before the contigs are cut; and the per-contig
 * coverage such a cutoff is chosen from.  (No counterpart in the reference; Velvet removes nodes below its per-node -cov_cutoff behind
 * Tour Bus and prints every contig's coverage in its name, SPAdes removes low-coverage and isolated edges.  cov_cutoff = 0 is the
 * default everywhere.)
 * What the cutoff, the tip rounds and the bubble rounds leave of sequencing errors is short and sits at the cutoff: ISLANDS (short false
 * contigs seen exactly min_count times with nothing attached at either end: "not a tip and stays", above), the remains of OVERLAPPING
 * BUBBLES (the bubble rule's stated limit) and of tied tips, and chimeric links attached at both ends.  Each one that hangs on the true
 * path makes its junction a branching node and cuts the true contig there.  True contigs sit at the coverage of the reads, far above.
 * gasm_batch_build_params removes such contigs from the k-mer set that the cutoff, the tip rounds and the bubble rounds left, for exactly
 * cov_rounds rounds; everything else is made from what is left.
 * The rule, on the same graph as the tip and the bubble rule (edges = distinct k-mers with their multiplicities, nodes = (k-1)-mers,
 * contigs = what the build would cut).  For a contig c let n(c) = its edges, m(c) = the sum of its edges' multiplicities,
 * len(c) = n(c) + k - 1 bases.  One round, on the current set:
 *   c is REMOVED if len(c) <= cov_len and m(c) < cov_cutoff * n(c), compared exactly in 64-bit integers: a mean multiplicity STRICTLY
 *   below cov_cutoff.  A mean equal to cov_cutoff stays.
 *   There is NO attachment test: islands, links attached at both ends and the remains of overlapping bubbles all go.
 *   All contigs of a round are found on the same graph and leave together, with all their k-mers (a k-mer lies in at most one
 *   contig); the next round starts from the remaining set.
 * A build runs exactly cov_rounds rounds, queued as a whole with no host wait, AFTER all tip rounds and all bubble rounds.
 * With strands = 2 a contig and its twin have equal n and m: they go in the same round, the contigs stay closed under reverse
 * complement and gasm_batch_fetch_contig_twins keeps working.
 * cov_cutoff = 0 or cov_len = 0 switches the feature off.  cov_cutoff <= min_count can match nothing and is allowed (every multiplicity
 * is at least min_count).  cov_len <= GASM_MAX_BUBBLE_LEN for the two reasons given for bubble_len: it keeps cov_cutoff * n inside 64 bits
 * and bounds a GPU thread's walk (in every round one thread per short contig walks its own chain, edge by edge).  The intended setting
 * is cov_len = 2k - 1, cov_cutoff = min_count + 1, one round.
 * STATED LIMITS: a TRUE stretch that is short and thinly covered goes too — the rule cannot tell it from an error.  And once the junk is
 * gone new tips can appear (a tip that was tied with a junk contig, say); this build does not clip again: a second pass of tip and
 * bubble rounds behind the low-coverage rounds is not made.
 * Everything behind the build — contigs, gasm_batch_fetch_distinct / _graph, the k-mer spectrum, twins, scores under one or several
 * tables, the guided traversal — sees what is left with its true multiplicities.  A read scores on a contig iff it is a substring of
 * it: a read that holds a removed k-mer adds nothing.
 * gasm_batch_build_params       the struct form of gasm_batch_build_bubbles plus cov_cutoff, cov_len, cov_rounds (gasm_build_params, above).
 *                               With cov_cutoff == 0 or cov_len == 0 it is gasm_batch_build_bubbles with the struct's other fields: same
 *                               host path, same kernel launches, cov_rounds is not read.  Otherwise cov_len <= GASM_MAX_BUBBLE_LEN and
 *                               cov_rounds in 1..GASM_MAX_COV_ROUNDS, else GASM_ERR_INVALID.  Each step slot remembers the three values
 *                               of the build it holds.
 * gasm_batch_cov_cutoff / _cov_len / _cov_rounds   of the last build (cov_rounds 0: no removal, or no build yet).
 * gasm_batch_fetch_lowcov_stats contigs[s * GASM_MAX_COV_ROUNDS + r] = contigs removed in segment s, round r; kmers[...] = k-mers
 *                               removed, same index; rounds not run are 0.  Host copies, valid until the next call or build.
 *                               GASM_ERR_STATE before a build or after a build with the feature off.
 * gasm_batch_contig_coverage    queues the per-contig coverage of the last build's contigs (as the build left them, whatever it removed);
 *                               GASM_ERR_STATE before a build.  It reads the build's arrays only and changes no build or score result.
 * gasm_batch_fetch_contig_coverage   mult_sum[c] = m(c), n_edges[c] = n(c), one entry per contig in the order of
 *                               gasm_batch_fetch_contigs; m(c) / n(c) is the contig's mean multiplicity (Velvet's "cov").  Integer sums:
 *                               exact.  Host copies, valid until the next call or build.  GASM_ERR_STATE before a build or without a
 *                               coverage pass over the last build.
 * Pooled builds (gasm_pool_*) remove no low-coverage contigs.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAX_COV_ROUNDS 8
int gasm_batch_build_params(gasm_batch* b, const gasm_build_params* params);
uint32_t gasm_batch_cov_cutoff(const gasm_batch* b);   /* of the last build */
uint32_t gasm_batch_cov_len(const gasm_batch* b);
uint32_t gasm_batch_cov_rounds(const gasm_batch* b);   /* 0: none */
int gasm_batch_fetch_lowcov_stats(gasm_batch* b, const uint32_t** contigs, const uint32_t** kmers);
int gasm_batch_contig_coverage(gasm_batch* b);
int gasm_batch_fetch_contig_coverage(gasm_batch* b, const uint64_t** mult_sum, const uint32_t** n_edges);
/* ------------------------------------------------------------------------------------------------------------------
 * Read correction: substituted bases of the reads are repaired against the k-mer set of a build.  (No counterpart in the reference,
 * whose simulated reads are error-free; spectral correction is the first stage of Quake, BFC, Musket and the SPAdes hammer.)
 * The cutoff, both strands, the tip, bubble and low-coverage rounds all make the GRAPH tolerate sequencing errors by throwing k-mers
 * away; none of them repairs a READ.  Scoring is an exact match of a read against the contigs: a read with one wrong base scores
 * nothing, although its start — the breakpoint — is good.  And at low coverage a cutoff removes true k-mers with the wrong ones; a
 * corrected read gives its coverage back to the true path.
 * The rule.  The TRUSTED SET of a segment is the distinct k-mers of that segment in the batch's last finished build, whatever options
 * that build had (min_count, strands, tips, bubbles, low coverage): what gasm_batch_fetch_distinct returns.  A k-mer of a read is WEAK
 * if it is not in the trusted set of the read's segment.  For a read of len bases let n = len - k + 1; its k-mer starts are 0 .. n-1.
 *   n <= 0: the read is copied and counted as no_kmer.
 *   No weak k-mer: copied and counted as clean.
 *   Otherwise every maximal run [a, b] of weak k-mer starts is judged ON THE READ AS GIVEN.  Runs do not interact: no k-mer of one run
 *   contains another run's candidate position, so the order of evaluation cannot matter.
 *     a == 0 and b == n-1 (the whole read is weak): left.
 *     Interior (a > 0, b < n-1): only a run of exactly k k-mers is tried, at position p = b.  Any other length is left.
 *     Touching the start (a == 0, b < n-1): p = b.  (A single substitution makes such a run at most k long; a longer one holds k-mers
 *     without position b, which stay weak whatever stands there: no candidate fits.)
 *     Touching the end (a > 0, b == n-1): a run longer than k is left; otherwise p = a + k - 1.
 *     At p each of the three other bases is tried.  A candidate FITS if all k-mers a .. b of the read with that base at p are in the
 *     trusted set.  The run is FIXED, and the base is written, only if EXACTLY ONE candidate fits; zero, or two or more, leave the run.
 *   Read counters: corrected (it had weak runs, all fixed), partial (some fixed), left (none fixed); bases_changed counts written bases.
 * STATED LIMITS: two errors closer than k merge into one long run and stay; a read whose every k-mer contains the error stays (a read
 * of fewer than 2k - 1 bases with an error in its middle, or of exactly k bases); substitutions only, no insertions or deletions; a read
 * of more than GASM_CORRECT_MAX_KMERS k-mers is copied and counted as left.  Against the same trusted set the rule is idempotent:
 * correcting the corrected reads changes nothing.
 * gasm_batch_correct_reads        GASM_ERR_STATE before any build.  Finishes the pending build, corrects on the stream of the step slot
 *                                 that holds it and is complete before it returns.  *out is a new batch of the same context with the
 *                                 same layout (fixed_len / read_off / seg_read_off) whose reads are the corrected ones; the packed bases
 *                                 never leave the device.  It always corrects the batch's own reads, each once, also after a strands = 2
 *                                 build, whose trusted set holds both orientations.  The source batch, its reads, its build and its
 *                                 scores are untouched; the new batch has no build yet.  Free it with gasm_batch_free.
 * gasm_batch_fetch_correct_stats  of a batch gasm_batch_correct_reads made: n_segments x GASM_CORRECT_FIELDS counters, per segment in
 *                                 the order no_kmer, clean, corrected, partial, left, bases_changed (the first five sum to the
 *                                 segment's reads).  Host copy, valid until the next call or free.  GASM_ERR_STATE on any other batch.
 * gasm_batch_fetch_reads          the reads of a batch as ASCII, back to back, with n_reads + 1 offsets: of any batch, before or after
 *                                 a build (the corrected reads, for the FASTQ a user wants to keep).  Host copies, valid until the next
 *                                 call or free.
 * Pooled builds (gasm_pool_*) have no read correction.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_CORRECT_FIELDS 6
#define GASM_CORRECT_MAX_KMERS 4096
int gasm_batch_correct_reads(gasm_batch* b, gasm_batch** out);
int gasm_batch_fetch_correct_stats(gasm_batch* b, const uint32_t** stats);
int gasm_batch_fetch_reads(gasm_batch* b, const char** ascii, const uint64_t** read_off);
/* ------------------------------------------------------------------------------------------------------------------
 * Contig links: the graph between the contigs of a build, and what the reads say about it.  (The reference forgets which contig
 * continues into which and tries 10 000 random orders instead, lib/DeNovoAssembler.cpp:195-203; Velvet writes LastGraph, SPAdes a GFA.)
 * A build cuts contigs at branching nodes.  A repeat of k-1 < L < read length bases cuts the true sequence into flanks plus one shared
 * contig, and the reads that run from one flank through the repeat into the next say how to put them back together.
 * The rule.  The graph is the one of the batch's LAST FINISHED BUILD, whatever its options: edges = the distinct k-mers that build left,
 * nodes = (k-1)-mers, contigs = what gasm_batch_fetch_contigs returns.  Contig indices are the ones INSIDE THE SEGMENT, as in
 * gasm_batch_fetch_contig_twins.  For a contig c let u(c) / v(c) = its first / last k-1 bases, e_first(c) / e_last(c) = its first / last
 * k-mer, n(c) = its edges, len(c) = n(c) + k - 1.
 *   LINKS.  (a, b) is a LINK if v(a) == u(b).  b == a is allowed — a loop, or an unbranched cycle whose cut point is both its ends —
 *   and gets no special case.  A node has at most four out-edges and four in-edges, so the links need no lists:
 *     succ[4 a + x] = the contig whose first k-mer is v(a) followed by base x (A, C, G, T = 0..3), or 0xFFFFFFFF;
 *     pred[4 b + x] = the contig whose last k-mer is base x followed by u(b), or 0xFFFFFFFF.
 *   The two tables state the same set of links.
 *   LINK SUPPORT.  A read of n = len - k + 1 > 0 k-mers is THREADED as given.  Position i is a CROSSING of link (a, b) if k-mer i is
 *   e_last(a) and k-mer i + 1 is e_first(b), both in the build's set.  link_support[4 a + x] counts crossings (x as in succ): occurrences,
 *   not reads — a read that goes round a loop twice counts twice.  Two consecutive k-mers of a read that are both in the set either follow
 *   each other inside one contig or are a crossing.
 *   SPAN SUPPORT.  For a contig r with len(r) <= span_len, a SPAN (x, r, y) at position i is: k-mer i is the in-edge x u(r), k-mers
 *   i + 1 .. i + n(r) are the edges of r, and k-mer i + n(r) + 1 is the out-edge v(r) y, all of them in the set.
 *   span_support[16 r + 4 x + y] counts them.  (r is unbranched inside: after a crossing into r, a run of n(r) + 1 further k-mers in
 *   the set must be r followed by an out-edge.)  For len(r) > span_len the sixteen entries are 0; span_len = 0 leaves the whole table 0
 *   and no span work is done.
 *   STRANDS.  After a strands = 2 build every read AND its reverse complement are threaded, as the build saw them: then
 *   link_support(a, b) == link_support(twin(b), twin(a)), and likewise for spans.  After a strands = 1 build only the reads as given.
 *   LIMITS.  A read of more than GASM_THREAD_MAX_KMERS k-mers is not threaded: it is counted in skipped[s] (reads, each once whatever
 *   the strands).  span_len <= GASM_MAX_SPAN_LEN.  A k-mer of an isolated cycle lies in no contig (gasm_batch_fetch_contigs has none for
 *   it): for this rule it is not in the set.  Pooled builds (gasm_pool_*) get none of this.
 * All counts are integers accumulated with atomic adds: exact and independent of the order the reads are taken in.
 * gasm_batch_contig_links         queues both kernels (k_contig_links, k_read_thread) on the step slot of the last build, behind it;
 *                                 GASM_ERR_STATE before a build, GASM_ERR_INVALID for span_len > GASM_MAX_SPAN_LEN.  It reads the
 *                                 build's arrays and the reads only: build, contig, score, coverage and twin results fetched before and
 *                                 after it are identical, and a batch that never calls it launches exactly what it launched without.
 * gasm_batch_fetch_contig_links   succ, pred, link_support: 4 entries per contig, span_support: 16 per contig, in the order of
 *                                 gasm_batch_fetch_contigs (contig c of the batch at 4 c resp. 16 c; the VALUES of succ / pred are
 *                                 indices inside the contig's segment); skipped: n_segments entries.  Host copies, valid until the
 *                                 next call or build.  GASM_ERR_STATE before a build or without a links pass over the last build.
 * What to do with them (GFA output, resolving repeats shorter than a read) is host code: genomeassembler_dev_amd/links.py.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_THREAD_MAX_KMERS 4096
#define GASM_MAX_SPAN_LEN 65535
int gasm_batch_contig_links(gasm_batch* b, uint32_t span_len);
int gasm_batch_fetch_contig_links(gasm_batch* b, const uint32_t** succ, const uint32_t** pred, const uint32_t** link_support,
                                  const uint32_t** span_support, const uint64_t** skipped /* n_segments */);
/* ------------------------------------------------------------------------------------------------------------------
 * Read pairs: where the two reads of a sequenced fragment lie on the contigs.  (The reference writes read_2 as reverse complements,
 * lib/GenerateReads.R:437-458, and hands both files to Velvet as -shortPaired, lib/DeNovoAssembler.R:182-203.)  A repeat longer than the
 * reads stays cut whatever the reads that run through it say (Contig links, above); a fragment whose mates lie in the two flanks still
 * says which flank continues into which.
 * The rule.  PAIRS.  Inside every segment reads 2p and 2p + 1 are the two MATES of pair p: an interleaved layout, which
 * gasm_batch_from_files yields for an interleaved FASTQ.  The pairs are forward-reverse: mate 1 is the fragment's first bases, mate 2
 * the reverse complement of its last bases.  A segment with an odd number of reads makes the call fail with GASM_ERR_INVALID.  Dropping
 * non-ACGT reads at ingest breaks the pairing: that is the caller's business (gasm_batch_from_files_params with pairs = 1 drops mates
 * together and so keeps it).
 *   THE SET.  The graph is the one of the batch's LAST FINISHED BUILD, whatever its options, exactly as for contig links.  A k-mer is IN
 *   THE SET if the build holds it and it lies in a contig; a k-mer of an isolated cycle is not in the set.  Contig indices are the ones
 *   INSIDE THE SEGMENT; len(c) is counted in bases.
 *   PLACEMENT of an oriented pair (first, second).  i1 = the smallest k-mer start of `first` whose k-mer is in the set, at contig c1,
 *   offset o1: S = o1 - i1 is where the fragment starts on c1 (it may be negative).  i2 = the smallest k-mer start of `second` whose
 *   REVERSE-COMPLEMENTED k-mer is in the set, at contig c2, offset o2: E = o2 + k + i2 is one past where the fragment ends on c2 (it may
 *   exceed len(c2)).  A mate shorter than k, or with no such position, is UNPLACED.  A pair with a mate of more than
 *   GASM_THREAD_MAX_KMERS k-mers is SKIPPED: neither mate is looked at.
 *   ORIENTATIONS.  Orientation 0 is (mate 1, mate 2).  After a strands = 2 build orientation 1 = (mate 2, mate 1) is placed as well, as
 *   the build saw the reads; after a strands = 1 build only orientation 0.  After a both-strand build, orientation 1 of a pair is
 *   (twin(c2), len(c2) - E, twin(c1), len(c1) - S) of its orientation 0.
 *   OUTPUTS, all exact integers, accumulated with integer atomics: independent of the order the pairs are taken in.
 *     rec[(o * n_pairs + p) * 4 + 0..3] = c1, S, c2, E as int32; p = the pair's index in the batch (read index / 2), n_pairs = reads of
 *       the batch / 2, o = the orientation.  A contig of -1 with position 0: the mate is unplaced.  Both contigs -1: skipped (or neither
 *       placed: the counters tell).
 *     insert_hist[s * (max_insert + 1) + d] counts the oriented pairs of segment s with both mates placed on the SAME contig and
 *       d = E - S > 0; bin max_insert collects every d >= max_insert.  max_insert is in 1..GASM_MAX_INSERT, else GASM_ERR_INVALID.
 *     counters[s * GASM_PAIR_FIELDS + f] counts oriented pairs, f in this order: skipped, none_placed, one_placed, same_contig (d > 0),
 *       reversed (same contig, d <= 0), diff_contig.  The six sum to the segment's pairs x orientations.
 * gasm_batch_place_pairs          finishes the pending build and queues k_pair_place on the step slot of the last build, behind it;
 *                                 GASM_ERR_STATE before a build and for the positioned reads of pooled builds, GASM_ERR_INVALID for a
 *                                 null batch, a bad max_insert or an odd segment.  It reads the build's arrays and the reads only:
 *                                 build, contig, score, coverage, twin and link results fetched before and after it are identical,
 *                                 and a batch that never calls it launches exactly what it launched without.
 * gasm_batch_fetch_pair_places    host copies, valid until the next call or build; *orientations = 1 or 2.  GASM_ERR_STATE before a
 *                                 build or without a placement over the last build.
 * What to do with them (insert size, mate links, resolving repeats longer than a read) is host code: genomeassembler_dev_amd/pairs.py.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAX_INSERT 65535
#define GASM_PAIR_FIELDS 6
int gasm_batch_place_pairs(gasm_batch* b, uint32_t max_insert);
int gasm_batch_fetch_pair_places(gasm_batch* b, const int32_t** rec, const uint32_t** insert_hist, const uint64_t** counters,
                                 uint32_t* orientations);
/* ------------------------------------------------------------------------------------------------------------------
 * Read mapping: where every read lies on the contigs once it carries substitutions.  (Contig links and read pairs match k-mers exactly:
 * a read with one wrong base in every k-mer is invisible to them.)  A seed-and-verify pass: exact k-mers seed a place, the whole read is
 * then compared with the contig's text base by base.
 * The rule.  INPUTS.  The contigs of the batch's LAST FINISHED BUILD, whatever its options; the batch's reads AS GIVEN (never the
 * both-strand stream); max_mismatch in 0..GASM_MAP_MAX_MISMATCH.  A k-mer of an isolated cycle lies in no contig: for this rule it is
 * not in the set.  Contig indices are the ones INSIDE THE SEGMENT.  Pooled builds (gasm_pool_*) get none of this.
 *   PER READ of len bases and n = len - k + 1 k-mers:
 *   1. len < k: the read is SHORT.  n > GASM_THREAD_MAX_KMERS: it is SKIPPED.  Neither does anything more.
 *   2. Position j is a SEED if k-mer j lies in a contig c at offset off.  Its DIAGONAL is d = off - j, signed: read base i lies over
 *      base d + i of c.  A read with no seed is UNSEEDED.
 *   3. The seeds are walked in increasing j; positions without a seed are ignored.  A seed whose (c, d) differs from the previous
 *      seed's is a HEAD.  A head whose (c, d) equals an earlier head's of the same read is ignored (an error can produce A, B, A).  At
 *      most GASM_MAP_MAX_BLOCKS distinct heads are kept per read; each further distinct head adds 1 to blocks_dropped and is ignored.
 *      ("Earlier" means KEPT: a dropped head is not remembered, so if it comes again behind another head it adds 1 again.)
 *   4. Each kept head is VERIFIED.  The overlap is i in [max(0, -d), min(len, len(c) - d)); it always holds at least k bases.  m = the
 *      number of overlap bases that differ from the contig's text.  The head is ACCEPTED iff m <= max_mismatch.  Bases outside the
 *      overlap are clipped and never counted.
 *   5. Every accepted block adds 1 to pile[4 * (c_off[c] + d + i) + base(read[i])] for every i of its overlap, and 1 to
 *      mismatch_hist[m].  A read that runs from one contig into the next is accepted on both: the k - 1 bases the two contigs share
 *      are counted on each, which is what depth per contig base should mean.
 *   6. The read's record is that of its BEST accepted block: largest overlap, then fewest mismatches, then smallest head position.
 *      With no accepted block the read is REJECTED, with exactly one MAPPED_ONE, with several MAPPED_MULTI.
 *   OUTPUTS, all exact integers, accumulated with integer atomics where shared: independent of the order the reads are taken in.
 *     rec[4 r + 0..3] = c, d, m | accepted blocks << 16, overlap as int32, r = the read's index in the batch; -1, 0, 0, 0 for a read
 *       with no place.
 *       (readmap.ReadMap.records() splits the packed word: FIVE columns c, d, m, accepted blocks, overlap — the overlap is column 4.)
 *     pile: 4 uint32 (A, C, G, T) per base of the batch's contig text, in the order of gasm_batch_fetch_contigs.
 *     mismatch_hist[s * (max_mismatch + 1) + m] counts the accepted blocks of segment s.
 *     counters[s * GASM_MAP_FIELDS + f], f in this order: short, skipped, unseeded, rejected, mapped_one, mapped_multi, blocks_dropped.
 *       The first six sum to the segment's reads; mismatch_hist sums to the accepted blocks, pile to their overlaps.
 *   STRANDS.  After a strands = 2 build the reads are still mapped as given: a read lies on whichever contig of a twin pair has its
 *   orientation.  Folding the twin's pileup in is host arithmetic.
 *   LIMITS.  Insertions and deletions are not mapped (by this pass: see "Gapped read mapping" below).  Two placements of one read on
 *   the same contig at different diagonals are both counted.  The cap of GASM_MAP_MAX_BLOCKS heads.  A read whose every k-mer holds
 *   an error is unseeded.
 * gasm_batch_map_reads            finishes the pending build and queues k_read_map on the step slot of the last build, behind it;
 *                                 GASM_ERR_STATE before a build and for the positioned reads of pooled builds, GASM_ERR_INVALID for a
 *                                 null batch or max_mismatch > GASM_MAP_MAX_MISMATCH.  It reads the build's arrays and the reads only.
 * gasm_batch_fetch_read_map       host copies, valid until the next call or build.  GASM_ERR_STATE before a build or without a mapping
 *                                 over the last build.
 * What to do with them (depth, error rate, consensus, variants) is host code: genomeassembler_dev_amd/readmap.py.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAP_MAX_MISMATCH 255
#define GASM_MAP_MAX_BLOCKS 8
#define GASM_MAP_FIELDS 7
int gasm_batch_map_reads(gasm_batch* b, uint32_t max_mismatch);
int gasm_batch_fetch_read_map(gasm_batch* b, const int32_t** rec, const uint32_t** pile, const uint32_t** mismatch_hist,
                              const uint64_t** counters);
/* ------------------------------------------------------------------------------------------------------------------
 * Gapped read mapping: read mapping for reads that carry insertions and deletions as well.  (A one-base indel in the middle of a read
 * moves every later seed to the next diagonal: read mapping sees two heads on one contig, verifies each against the whole read, finds
 * about three quarters of the far side differing and rejects the read.)  The two heads say where the gap is: this pass joins them.
 * A second pass beside read mapping, with tables of its own; gasm_batch_map_reads is untouched and with max_gap = 0 this pass gives its
 * tables.
 * The rule.  INPUTS.  As for read mapping, plus max_edits in 0..GASM_MAP_MAX_MISMATCH and max_gap in 0..GASM_MAP_MAX_GAP.
 *   PER READ of len bases:
 *   1-3. UNCHANGED.  Short, skipped, seeds, diagonals and the kept heads of a read are exactly those of read mapping.  Head i is
 *      (J_i, c_i, d_i), J_i the seed position at which the head starts; at most GASM_MAP_MAX_BLOCKS heads are kept, in walk order; the
 *      A, B, A rule and blocks_dropped apply as before.
 *   4. CHAINS.  The kept heads are walked in order; the first opens a chain.  Head i + 1 JOINS the chain that head i closed when all
 *      three hold: c_{i+1} = c_i; g = d_{i+1} - d_i satisfies 0 < |g| <= max_gap; and, for g < 0 (an insertion of G = -g read bases),
 *      J_{i+1} - G >= J_i + 1.  Otherwise head i + 1 opens a new chain.  Only consecutive kept heads join.
 *   5. BREAKPOINTS.  Between joined heads i and i + 1 there is one breakpoint t_i.  G = -g for an insertion, G = 0 for a deletion.
 *      The window of t is [J_i + 1, J_{i+1} - G].  t_i is the smallest t in the window that minimises the sum of two counts: the
 *      positions x in [J_i + 1, t) where read[x] != c[d_i + x], and the positions x in [t + G, J_{i+1}) where read[x] != c[d_{i+1} + x].
 *      The windows of successive breakpoints are disjoint and increasing, and the bases a piece holds outside them do not depend on any
 *      t (read bases J_i .. J_i + k - 1 match): each t_i is chosen on its own and together they are the joint optimum.
 *   6. PIECES.  Piece 1 starts at s_1 = max(0, -d_1).  Piece i is read bases [s_i, t_i) on diagonal d_i; s_{i+1} = t_i + G; the last
 *      piece ends at min(len, len(c) - d_q), q = the chain's heads.  For an insertion read bases [t_i, t_i + G) lie on nothing; for a
 *      deletion contig bases [d_i + t_i, d_i + t_i + g) are skipped.  Every piece is non-empty and inside the contig: s_i <= J_i <
 *      t_i (s_1 <= J_1 because k-mer J_1 lies at d_1 + J_1 >= 0; s_{i+1} = t_i + G <= J_{i+1} by the window), the last piece holds k-mer
 *      J_q; and a base x of [J_i + 1, J_{i+1}) lies inside c on both diagonals: d_i + x > d_i + J_i >= 0, d_{i+1} + x < d_{i+1} + J_{i+1}
 *      < len(c), and on the other side d_i + x = d_{i+1} + x - g, where for a deletion (g > 0) the upper bound and for an insertion
 *      (x < J_{i+1} - G on the left, x >= J_i + 1 + G on the right) both bounds follow from the two just given.
 *   7. COST AND ACCEPTANCE.  COST = mismatches over all pieces + the sum of |g|; OVERLAP = the sum of the piece lengths.  A chain is
 *      ACCEPTED iff cost <= max_edits.  A chain of one head is exactly step 4 of read mapping.  A chain of two or more heads is
 *      verified only as a chain: its heads are not tried alone.
 *   8. Every accepted chain adds 1 to pile[4 * (c_off[c] + d_i + x) + base(read[x])] for every base x of every piece i, 1 to
 *      gap_pile[2 p + 0] for every skipped contig base p, 1 to gap_pile[2 p + 1] at p = c_off[c] + d_i + t_i, the contig base that
 *      the first read base behind an insertion sits on (this counts insertions, not inserted bases), and 1 to edit_hist[cost].
 *   9. The read's record is that of its BEST accepted chain: largest overlap, then lowest cost, then smallest J_1.  Classes as
 *      before, over chains: rejected, mapped_one, mapped_multi.
 *   OUTPUTS, all exact integers, accumulated with integer atomics where shared: independent of the order the reads are taken in.
 *     rec[4 r + 0..3] = c, d_1, cost | accepted chains << 16, overlap as int32; -1, 0, 0, 0 for a read with no place.
 *     rec_gap[4 r + 0..3] = pieces q, inserted bases, deleted bases, d_q of the best chain; all zero for a read with no place.
 *     pile: 4 uint32 per contig base; gap_pile: 2 uint32 (deletions, insertions) per contig base; both in the order of
 *       gasm_batch_fetch_contigs.
 *     edit_hist[s * (max_edits + 1) + cost] counts the accepted chains of segment s.
 *     counters[s * GASM_MAPG_FIELDS + f]: the seven of read mapping in their order, then gapped: the reads whose best chain has
 *       q >= 2.  The first six sum to the segment's reads.
 *   STRANDS.  As for read mapping: the reads are mapped as given.
 *   LIMITS.  An indel closer than k to an end of the read leaves no seed beyond it: that end is compared ungapped, and usually the
 *   read is rejected (of simulated 80-base reads with an indel about 45 % stay unplaced for this reason at k = 21, of 150-base reads
 *   about a third).  A spurious head between two heads of a chain cuts the chain.  A read that returns to an earlier diagonal is not
 *   chained through, because of A, B, A.  The sequence of inserted bases is not recorded (by this form and by end gaps; "Alignments"
 *   below records it, and every read's pieces).  A gap longer than max_gap is not joined.
 *   Gaps cost their length: no affine score.  Pooled builds (gasm_pool_*) get none of this.
 * gasm_batch_map_reads_gapped        finishes the pending build and queues k_read_map_gapped on the step slot of the last build, behind
 *                                    it; GASM_ERR_STATE before a build and for the positioned reads of pooled builds, GASM_ERR_INVALID
 *                                    for a null batch, max_edits > GASM_MAP_MAX_MISMATCH or max_gap > GASM_MAP_MAX_GAP.  It reads the
 *                                    build's arrays and the reads only; a gasm_batch_map_reads over the same build stays fetchable, and
 *                                    the other way round; a batch that never calls it launches exactly what it launched without.
 * gasm_batch_fetch_read_map_gapped   host copies, valid until the next call or build.  GASM_ERR_STATE before a build or without a
 *                                    gapped mapping over the last build.
 * What to do with them (depth, error rate, consensus, indels) is host code: genomeassembler_dev_amd/readmap.py, GappedReadMap.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAP_MAX_GAP 16
#define GASM_MAPG_FIELDS 8
int gasm_batch_map_reads_gapped(gasm_batch* b, uint32_t max_edits, uint32_t max_gap);
int gasm_batch_fetch_read_map_gapped(gasm_batch* b, const int32_t** rec, const int32_t** rec_gap, const uint32_t** pile,
                                     const uint32_t** gap_pile, const uint32_t** edit_hist, const uint64_t** counters);
/* ------------------------------------------------------------------------------------------------------------------
 * End gaps: gapped read mapping that also tries ONE GAP AT EACH END of every chain, between the read's end and the chain's outermost
 * seed.  Gapped read mapping joins heads, so it sees only an indel with a seed on both sides; an indel closer than k to an end of the
 * read leaves no seed beyond it (the first of its LIMITS above).  This form closes most of that limit with the breakpoint search of
 * step 5, run once more at each end of a chain.  A third form of the pass; the other two are untouched, and with end_gap = 0 this one
 * gives the gapped mapping's tables.  Since the first piece's diagonal is what rec holds, mapped scoring (below) needs no change: a
 * read with an indel near its start is placed, and its break lands on the right contig base.  What the LIMITS of gapped read mapping
 * and of mapped scoring say about an indel within k of a read's end or start holds for gasm_batch_map_reads_gapped and for end_gap = 0.
 * The rule.  INPUTS.  As for gapped read mapping, plus end_gap in 0..GASM_MAP_MAX_GAP.
 *   PER READ of len bases:
 *   1-5. UNCHANGED.  Short, skipped, seeds, heads, chains and the breakpoints of the joins are exactly those of gapped read mapping.
 *      A chain has the heads (J_i, c, d_i), i = 1..q; clen = len(c).  mism(lo, hi, d) is the number of x in [lo, hi) with
 *      read[x] != c[d + x].
 *   5a. BACK END.  The window starts at B = J_q + k.  The end is ELIGIBLE iff d_q + len <= clen: the read's last base lies on the
 *      contig on the ungapped diagonal.  m0 = mism(B, len, d_q).  A CANDIDATE is (g, t) with 0 < |g| <= end_gap, G = max(0, -g),
 *      d_q + g + len <= clen and t in [B, len - G - 1]: the piece behind the gap is non-empty, the part in front of it may be empty.
 *      Its cost is |g| + mism(B, t, d_q) + mism(t + G, len, d_q + g).  The BEST candidate is the smallest under the key (cost, |g|,
 *      deletion before insertion, t): lowest cost, then shortest gap, then a deletion (g > 0) before an insertion, then the smallest t.
 *      It is TAKEN iff its cost is strictly below m0.  Hence nothing is taken when m0 < 2, and no |g| >= m0 needs to be tried.
 *   5b. FRONT END.  The window is [0, J_1).  The end is eligible iff d_1 >= 0 and J_1 > 0.  m0 = mism(0, J_1, d_1).  A candidate is
 *      (g, t) with 0 < |g| <= end_gap, G = max(0, -g), d_0 = d_1 - g >= 0 and t in [1, J_1 - G]: the piece in front of the gap, read
 *      bases [0, t) on d_0, is non-empty.  Its cost is |g| + mism(0, t, d_0) + mism(t + G, J_1, d_1).  The same key; taken iff the cost
 *      is strictly below m0.
 *      The two end windows and all join windows are pairwise disjoint: [0, J_1) lies in front of J_1 + 1, where the first join window
 *      starts, and [J_q + k, len) lies behind J_q, where the last one ends; the bases a piece holds outside the windows do not depend
 *      on any choice.  Each choice is therefore made on its own, and together they are the joint optimum under "at most one gap per
 *      end".
 *   6'. PIECES.  A taken front gap (g_0, t_0) puts a piece [0, t_0) on d_0 in front of piece 1, which then starts at t_0 + G_0.  A
 *      taken back gap (g_b, t_b) ends piece q at t_b and adds a piece [t_b + G_b, len) on d_q + g_b.  Every piece lies inside the
 *      contig.  Front: d_0 >= 0 is asked, and a base x < t_0 <= J_1 - G_0 lies at d_0 + x = d_1 + x - g_0 < d_1 + J_1 < clen (for a
 *      deletion because g_0 > 0, for an insertion because x + G_0 < J_1).  Back: d_q + g_b + len <= clen is asked, and a base x >=
 *      t_b + G_b lies at d_q + g_b + x >= d_q + t_b >= d_q + J_q >= 0 (for a deletion because g_b > 0, for an insertion because
 *      x - G_b >= t_b).  Both pieces next to a gap are non-empty: t_0 >= 1, piece 1 holds k-mer J_1 >= t_0 + G_0; piece q holds
 *      k-mer J_q, which ends at B <= t_b; and t_b + G_b < len.
 *   7-9. UNCHANGED in wording.  COST is the mismatches over all pieces plus all gap lengths, end gaps included; OVERLAP the sum of the
 *      piece lengths; a chain is ACCEPTED iff cost <= max_edits.  Pileup and gap pileup take an end gap exactly as step 8 takes a
 *      join: a deletion adds its skipped contig bases, an insertion adds 1 in front of the contig base at (left diagonal) + t.  Best
 *      chain and classes as before.
 *   PROPERTIES.  For every chain the cost with end gaps is at most its cost without (a gap is taken only where it is cheaper), so
 *   every read placed without end gaps is placed with them.  On error-free reads m0 = 0 everywhere: the six tables are the gapped
 *   mapping's and the two new ones are zero.
 *   OUTPUTS.  The six arrays of the gapped mapping, with the same shapes.  rec[4 r + 1] is the diagonal of the FIRST piece: d_0
 *   where a front gap was taken.  rec_gap counts pieces, inserted bases and deleted bases with the end pieces in; its last word is
 *   the LAST piece's diagonal.  The eighth counter, gapped, stays "the best chain has 2 or more pieces".  And two more:
 *     rec_end[4 r + 0..3] = g_front, t_front, g_back, t_back of the read's best chain; the two values of an end without a gap are
 *       0; all four are zero for a read with no place.
 *     end_counters[s * GASM_MAPEND_FIELDS + f], f in this order: front, the accepted chains with a front gap; back, likewise;
 *       rescued, the accepted chains whose cost plus the savings m0 - cost of their taken end gaps exceeds max_edits (chains that
 *       would not have been accepted without); start_moved, the reads whose best chain has a front gap.
 *   LIMITS.  An end clipped by the contig's end is not extended (not eligible).  At most one gap per end.  A gap next to the read's
 *   very end can be explained away by substitutions, which is why the comparison is strict: such a gap is not taken.  A short
 *   matching stub behind a gap can be chance (about 1 read in 1000 at 3 % substitutions).  And the limits of the chains themselves.
 * gasm_batch_map_reads_gapped_ends   as gasm_batch_map_reads_gapped, and end_gap > GASM_MAP_MAX_GAP: GASM_ERR_INVALID.  It fills the
 *                                    gapped mapping's own state: gasm_batch_fetch_read_map_gapped and gasm_batch_score_mapped(source =
 *                                    GASM_MAPSCORE_GAPPED) work on it unchanged.  end_gap > 0 queues k_read_map_ends; end_gap = 0
 *                                    queues exactly the k_read_map_gapped of gasm_batch_map_reads_gapped and leaves no end tables.
 * gasm_batch_fetch_read_map_ends     host copies, valid until the next call or build.  GASM_ERR_STATE before a build, without a gapped
 *                                    mapping over the last build, and when the last one tried no end gaps (it was not made by
 *                                    gasm_batch_map_reads_gapped_ends, or with end_gap = 0).
 * What to do with them is host code: genomeassembler_dev_amd/readmap.py, GappedReadMap.end_records, end_counters.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAPEND_FIELDS 4
int gasm_batch_map_reads_gapped_ends(gasm_batch* b, uint32_t max_edits, uint32_t max_gap, uint32_t end_gap);
int gasm_batch_fetch_read_map_ends(gasm_batch* b, const int32_t** rec_end, const uint64_t** end_counters);
/* ------------------------------------------------------------------------------------------------------------------
 * Alignments: gapped read mapping with end gaps that KEEPS what it worked out: every read's pieces, from which its CIGAR and a SAM line
 * follow, and the bases of every insertion.  The two forms above verify a complete base-level alignment of every accepted chain and
 * keep its first and last diagonal, its piece count and its totals; the inner diagonals and the breakpoints are kept nowhere, and an
 * insertion is counted without its bases.  A fourth form of the pass; the other three, their tables and their launches are untouched.
 * The rule is that of "End gaps", steps 1 to 9, word for word; end_gap = 0 is legal and takes no end gap (the eight tables are then the
 * gapped mapping's six and zero end tables).  Nothing about places, costs, pileups or counters changes; two tables are added.
 *   OUTPUTS.  The eight arrays of "End gaps" with the same shapes and values, and:
 *     rec_piece[(r * GASM_MAP_MAX_PIECES + i) * 2 + 0..1] = s | e << 16, d: piece i of the read's best chain holds read bases [s, e) on
 *       diagonal d (read base x lies on contig base d + x), exactly the pieces that steps 6 / 6' verify, after the clamps to the read
 *       and to the contig, end-gap pieces included, in read order.  rec_gap[4 r + 0] pieces are valid; the others, and all pieces of
 *       a read with no place, are zero.  GASM_MAP_MAX_PIECES = GASM_MAP_MAX_BLOCKS + 2: a chain over every kept head and a piece
 *       beyond the gap at each end.  e <= GASM_THREAD_MAX_KMERS + 62, so the halves cannot overflow.  80 bytes per read.
 *     ins_pile[((p * W + l) * 4) + x], W = ins_cols = max(max_gap, end_gap) columns of 4 uint32 per contig base p, in the order of
 *       gasm_batch_fetch_contigs; l the column, x the base code (A, C, G, T).  Every ACCEPTED chain adds to it as it adds to gap_pile:
 *       an insertion of G read bases with breakpoint t in front of contig base p (the p that gets gap_pile[2 p + 1]) adds 1 at column
 *       l, base read[t + l], for l in [0, G); joins and both end gaps alike.  16 W bytes per contig base (48 at the defaults, 256 at
 *       W = 16); W = 0 gives an empty table.
 *   INVARIANTS, all integer and independent of the order of the adds.  Column 0's four counts sum to gap_pile[2 p + 1].  The column
 *   sums never increase with l.  The grand total is the inserted bases over all accepted chains.
 *   CIGAR of a placed read of len bases with the pieces (s_i, e_i, d_i), i = 1..q: s_1 S if s_1 > 0; e_i - s_i M per piece; between
 *   pieces i and i + 1, g = d_{i+1} - d_i: g D if g > 0, -g I if g < 0; len - e_q S if that is positive.  Read bases off either end of
 *   the contig are soft clips.  The leftmost contig base is d_1 + s_1 (SAM's POS less 1).  M + I + S sum to len, M to rec[4 r + 3],
 *   I and D to rec_gap[4 r + 1] and [4 r + 2]; the M runs number rec_gap[4 r + 0].  A read with no place has the CIGAR "*".
 *   LIMITS.  The pieces are the best chain's only; ins_pile counts every accepted chain, as the pileups do.  The columns are indexed
 *   from the insertion's first base, without its length: insertions of different lengths at one place share their leading columns,
 *   and a twin's insertion (after a both-strand build) cannot be reversed column by column, so the insertion pileup is not folded over
 *   twins.  An index by (length, column) would lift this and is not built.  No mapping quality, no pairing, no qualities.  And the
 *   limits of "End gaps".  Pooled builds get none of this.
 * gasm_batch_map_reads_aligned       as gasm_batch_map_reads_gapped_ends: the same checks and error codes.  It fills the gapped
 *                                    mapping's own state: gasm_batch_fetch_read_map_gapped, gasm_batch_fetch_read_map_ends (also for
 *                                    end_gap = 0: zero tables) and gasm_batch_score_mapped(source = GASM_MAPSCORE_GAPPED) work on it
 *                                    unchanged.  It queues k_read_map_trace alone.  A later gasm_batch_map_reads_gapped or
 *                                    gasm_batch_map_reads_gapped_ends forgets the two tables; a batch that never calls it launches
 *                                    exactly what it launched without.
 * gasm_batch_fetch_read_alignments   host copies, valid until the next call or build.  GASM_ERR_STATE before a build, without a gapped
 *                                    mapping over the last build, and when the last one was not made by gasm_batch_map_reads_aligned;
 *                                    GASM_ERR_INVALID for a null argument.
 * What to do with them (pieces, CIGAR, SAM, inserted strings, consensus with insertions) is host code:
 * genomeassembler_dev_amd/readmap.py, AlignedReadMap.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAP_MAX_PIECES 10
int gasm_batch_map_reads_aligned(gasm_batch* b, uint32_t max_edits, uint32_t max_gap, uint32_t end_gap);
int gasm_batch_fetch_read_alignments(gasm_batch* b, const int32_t** rec_piece, const uint32_t** ins_pile, uint32_t* ins_cols);
/* ------------------------------------------------------------------------------------------------------------------
 * Mapped scoring: breakage scores from mapped reads, so that reads with errors count too.  gasm_batch_score matches exactly: a read
 * scores iff it is a substring of a contig, so a read with one wrong base scores nothing although its start, the breakpoint, is
 * good.  The two read mappings leave, for every read, the contig and the diagonal d of its best alignment: the contig base under the
 * read's first base is d.  This pass turns those records into breaks.  A pass of its own, with arrays and tables of its own:
 * gasm_batch_score*, gasm_batch_map_reads* and their tables stay as they are, and a batch that never calls it launches exactly what it
 * launched without.
 * The rule.  INPUTS.  The contigs of the batch's LAST FINISHED BUILD, whatever its options; the records of gasm_batch_map_reads
 * (source = GASM_MAPSCORE_UNGAPPED) or of gasm_batch_map_reads_gapped (GASM_MAPSCORE_GAPPED) made OVER THAT BUILD; kmer, as
 * gasm_batch_score takes it; n_tables in 1..GASM_MAX_TABLES tables of GASM_TABLE_ROWS doubles; flags.
 *   PER READ of len bases take rec = (c, d_1, cost | n << 16, overlap); for the gapped source also ins = rec_gap[1], the inserted
 *   bases, for the ungapped source ins = 0.  Exactly one class applies, tested in this order:
 *   1. c < 0: UNPLACED.  This covers short, skipped, unseeded and rejected reads.
 *   2. d_1 < 0: START_CLIPPED.  The read's first base lies in front of the contig, so its break is not on this contig.  It is never
 *      scored.
 *   3. overlap + ins < len: END_CLIPPED.  The read starts on the contig and runs off its end.  It is scored only with the flag
 *      GASM_MAPSCORE_PARTIAL.
 *   4. Otherwise: WHOLE.  It is scored.
 *   A SCORED READ adds 1 to kmer_breaks[c], 1 to start_pile[c_off[c] + d_1], and for every table t fix_t[window] to the 64-bit sum
 *   fx[t][c].  window is the break window of a hit at position j = d_1 of contig c, exactly the scorer's (lib/DeNovoAssembler.cpp:
 *   366-386: the octamer around the break, 2 / 4 / 6 bases wide for j = 1 / 2 / 3, cut where the contig ends).  fix_t =
 *   llrint(p * 2^shift_t), shift_t by gasm_batch_score's rule with n = the most reads of one segment.
 *   THE BEST ALIGNMENT ONLY.  A read is one fragment with one break, so accepted alignments other than the record's do not score.
 *   This differs from the pileups, which count every accepted block or chain.
 *   OUTPUTS per contig and table, formed as gasm_batch_score forms them: bp_score = fx * 2^-shift, norm_by_break_freqs = bp_score /
 *   kmer_breaks (0 without hits), norm_by_len = bp_score / len, sequence_len.  start_pile: one uint32 per base of the batch's contig
 *   text, the reads scored with their start there.  counters[s * GASM_MAPSCORE_FIELDS + f], f in this order: unplaced,
 *   start_clipped, end_clipped, whole; they sum to the segment's reads.  All sums are integer atomics: the results do not depend on
 *   the order the reads are taken in.
 *   NO FP64 FALLBACK.  A table with a non-finite entry, or one without a shift in [0, 1000], makes the call return GASM_ERR_INVALID,
 *   and nothing is queued.  A read shorter than k is unplaced and scores nothing: a stated difference from gasm_batch_score, where an
 *   empty read hits every path at position 0.
 *   STRANDS.  Nothing is added: the records are of the reads as given, so a reverse-strand read scores on the twin, as it does in
 *   gasm_batch_score.
 *   THE PROPERTY that ties it to gasm_batch_score.  Take a batch that has no read shorter than k and no read of more than
 *   GASM_THREAD_MAX_KMERS k-mers.  After any build of it, mapped scoring from gasm_batch_map_reads(b, 0) without
 *   GASM_MAPSCORE_PARTIAL gives, for every table and bit for bit, the results of gasm_batch_score_tables with the same tables: fx,
 *   shift, kmer_breaks, sequence_len, bp_score, norm_by_break_freqs and norm_by_len.  (A read is a substring of a contig iff its
 *   first k-mer's head on that contig verifies with 0 mismatches and overlap = len; that block has the largest possible overlap; and
 *   no second contig can hold all of the read's k-mers.)  The same holds for the gapped source at max_edits = max_gap = 0.
 *   LIMITS.  An accepted alignment can still be the wrong place: a repeat copy within max_edits.  An indel within k of a read's start
 *   leaves the read unplaced: the mapping's own limit.  gasm_batch_guided keeps using gasm_batch_score's sums.  Pooled builds
 *   (gasm_pool_*) get none of this.
 * gasm_batch_score_mapped          finishes the pending build and queues k_score_mapped and the final sums on the step slot of the last
 *                                  build, behind it.  GASM_ERR_STATE before a build, without a mapping of that source over the last
 *                                  build, and for the positioned reads of pooled builds; GASM_ERR_INVALID for a null batch or table, a
 *                                  bad source, unknown flag bits, n_tables out of range, a kmer that gasm_batch_score refuses, or a table
 *                                  without a shift.
 * gasm_batch_fetch_mapped_scores   table t's results, one entry per contig in the order of gasm_batch_fetch_contigs; host copies, valid
 * gasm_batch_fetch_mapped_starts   until the next call or build.  t >= n_tables: GASM_ERR_INVALID; without a mapped score over the
 *                                  last build: GASM_ERR_STATE.
 * What to do with them is host code: genomeassembler_dev_amd/readmap.py, MappedScores.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_MAPSCORE_UNGAPPED 0
#define GASM_MAPSCORE_GAPPED 1
#define GASM_MAPSCORE_PARTIAL 1u /* flags */
#define GASM_MAPSCORE_FIELDS 4   /* unplaced, start_clipped, end_clipped, whole: they sum to the segment's reads */
int gasm_batch_score_mapped(gasm_batch* b, int source, int kmer, const double* tables, uint32_t n_tables, uint32_t flags);
int gasm_batch_fetch_mapped_scores(gasm_batch* b, uint32_t t, const double** bp_score, const double** norm_by_break_freqs,
                                   const double** norm_by_len, const int32_t** kmer_breaks, const int32_t** sequence_len,
                                   const int64_t** fx, int* shift);
int gasm_batch_fetch_mapped_starts(gasm_batch* b, const uint32_t** start_pile /* one per contig base */,
                                   const uint64_t** counters /* n_segments x GASM_MAPSCORE_FIELDS */);
uint64_t gasm_batch_total_kmers(const gasm_batch* b);   /* k-mers extracted by the last build */
uint64_t gasm_batch_total_reads(const gasm_batch* b);

/* results of the last build (host copies, valid until the next build/free) */
int gasm_batch_fetch_distinct(gasm_batch* b, const uint64_t** seg_off /*n_segments+1*/, const uint64_t** keys,
                              const uint32_t** mult, int* words);
/* The (k-1)-mer graph of the last build, one entry per distinct k-mer (= distinct edge) in the order of gasm_batch_fetch_distinct:
 * restates the degree table and the branching-node list of lib/DeNovoAssembler.cpp:125-169 and one step of its walk (:172-189).
 *   edge_flags bit 0: the edge's source node (its first k-1 bases) is a branching node (in-degree != 1 or out-degree != 1);
 *              bit 1: (on the first out-edge of a node, in sorted order) the node has two or more in-edges;
 *   edge_next: the edge the walk continues with (index into the batch's distinct list), 0xFFFFFFFF where a contig ends. */
int gasm_batch_fetch_graph(gasm_batch* b, const uint8_t** edge_flags, const uint32_t** edge_next);
int gasm_batch_fetch_contigs(gasm_batch* b, const uint64_t** seg_contig_off /*n_segments+1*/, const uint64_t** off,
                             const char** data);
/* results of the last score: one entry per contig, in the order of gasm_batch_fetch_contigs */
int gasm_batch_fetch_scores(gasm_batch* b, const double** bp_score, const double** norm_by_break_freqs,
                            const double** norm_by_len, const int32_t** kmer_breaks, const int32_t** sequence_len);

/* ------------------------------------------------------------------------------------------------------------------
 * count_read_kmers(sequencing_reads, kmer)                      replaces lib/DeNovoAssembler.R:135-168
 *   (the reference's only_kmers_from_reads mode: table() of every kmer-long window of the reads, match()ed onto the
 *   breakage table of that length, absent k-mers 0 — table_read_kmer_prob)
 * A window counts only if it lies inside one read; a read shorter than kmer has none.
 * gasm_batch_count_read_kmers   every segment's counts of all four lengths at once: GASM_TABLE_ROWS u32 per segment in
 *                               breakage-table order (rows 0 / 16 / 272 / 4368 start k = 2 / 4 / 6 / 8, each lexicographic).
 *                               Queued on the stream the batch's reads were made on; no host wait.  Reads only the packed
 *                               reads: it works before any build, between a build and its score and after both, and changes
 *                               no build or score result.  GASM_ERR_CAPACITY where a segment holds 2^32 or more windows of
 *                               length 2 (below that no counter can wrap).  GASM_RKC_SPLIT in the environment: workgroups per
 *                               segment (2, 4 or 8; the bins are split between them by the leading bits of the k-mer).
 * gasm_batch_fetch_read_kmer_counts   n_segments x GASM_TABLE_ROWS counts of the last count, segment after segment; the host
 *                               copy stays valid until the next count or free.  GASM_ERR_STATE before any count.
 * gasm_count_read_kmers         the string form (what the Rcpp glue calls), one segment through the same kernel: counts[i] =
 *                               occurrences of key i (duplicates allowed; each key kmer ACGT bytes, else GASM_ERR_INVALID /
 *                               GASM_ERR_NON_ACGT); keys == NULL: all 4^kmer k-mers in lexicographic order (the order of the
 *                               reference's df_prob[[kmer_k]]) and n_keys is not read.  kmer must be 2, 4, 6 or 8.
 * ---------------------------------------------------------------------------------------------------------------- */
int gasm_batch_count_read_kmers(gasm_batch* b);
int gasm_batch_fetch_read_kmer_counts(gasm_batch* b, const uint32_t** counts);
int gasm_count_read_kmers(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int kmer, const char* keys,
                          const uint64_t* key_off, uint64_t n_keys, uint32_t* counts);

/* ------------------------------------------------------------------------------------------------------------------
 * Pooled builds over several GPUs: the reads of every segment are spread over the ranks, k-mers are bucketed by
 * (segment, first bits of the k-mer) and every bucket's records are brought together on one rank by an all-to-all before
 * the global edge-list merge (SURVEY.md §8(e) mode 2; the reference has no counterpart: it loops over segments on one
 * thread, scripts/02_Real_vs_rand_prob_own.R:33-53).  One gasm_pool per rank; the library does the device work of every
 * stage and packs / consumes device buffers, the caller moves them between ranks (RCCL through its own runtime —
 * genomeassembler_dev_amd/pooled.py uses torch.distributed — or plain copies between virtual ranks of one process) and
 * decides which rank owns which bucket and which segment.  Records travel as two streams: keys (8 bytes for k <= 31, 16
 * bytes hi:lo for k <= 63, sorted inside a run) and 32-bit counts; the bucket a run belongs to follows from its place in
 * the bucket lists both sides derive from the ownership function.  Results do not depend on the number of ranks.
 *
 *   (pooled builds take their k-mers forward-strand only: there is no strands argument here; they do not clip tips either:
 *   there is no tip_len argument; and they pop no bubbles: there is no bubble_len argument; and they remove no low-coverage contigs:
 *   there is no cov_cutoff argument)
 *   gasm_pool_create       this rank's reads (fixed length) of ALL n_segments segments
 *   gasm_pool_local_runs   k-mers of those reads -> one sorted run of distinct (key, count) per bucket; bucket index =
 *                          segment << bbits | first bbits bits of the k-mer; run_len (host, n_segments << bbits entries)
 *   gasm_pool_pack_runs    the current runs of the listed buckets, back to back, into caller-owned device buffers
 *   gasm_pool_merge_runs   n_out output buckets, each the union (counts added) of up to n_src runs found at record offset
 *                          run_off[j * n_src + s], length run_len[j * n_src + s] (0 = none) of the input buffers; the
 *                          merged runs become the pool's current runs (bucket index = j); merged_len: host, n_out entries
 *   gasm_pool_graph        the current runs are the buckets of n_local segments (n_local << bbits, segment-major):
 *                          graph, traversal, contigs of those segments (as gasm_batch_build)
 *   gasm_pool_piece_words / gasm_pool_pack_reads   the 2-bit reads of segments [seg_lo, seg_hi) of this rank as
 *                          word-aligned pieces, one per segment, back to back
 *   gasm_pool_set_reads    the reads of the rank's own segments as received: piece i holds piece_reads[i] reads of local
 *                          segment piece_seg[i] (non-decreasing) from word piece_word_off[i] of d_words
 *   gasm_pool_score        as gasm_batch_score, for the rank's own segments
 *   gasm_pool_fetch_*      as gasm_batch_fetch_*, for the rank's own segments
 * GASM_ERR_CAPACITY from local_runs / merge_runs: a bucket holds too many distinct k-mers — use more bucket bits (all
 * ranks must use the same bbits).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct gasm_pool gasm_pool;
int gasm_pool_create(gasm_ctx* ctx, const char* reads, uint64_t n_reads, uint32_t fixed_len, const uint64_t* seg_read_off,
                     uint32_t n_segments, gasm_pool** out);
void gasm_pool_free(gasm_pool* p);
int gasm_pool_key_words(const gasm_pool* p);   /* 64-bit words per key: 1 (k <= 31) or 2; valid after gasm_pool_local_runs */
int gasm_pool_local_runs(gasm_pool* p, int k, int bbits, const uint32_t** run_len);
int gasm_pool_pack_runs(gasm_pool* p, const uint32_t* bucket_ix, uint64_t n, void* d_keys_out, void* d_counts_out);
int gasm_pool_merge_runs(gasm_pool* p, uint32_t n_out, uint32_t n_src, const uint64_t* run_off, const uint32_t* run_len,
                         const void* d_keys_in, const void* d_counts_in, const uint32_t** merged_len);
/* Debugging aid (tests): the fine directories gasm_pool_merge_runs wrote, one row of 2^fbits + 1 offsets per merged run
 * (offsets, relative to the run, of the key bins below the bucket prefix).  Host memory of the pool, valid until the next call. */
int gasm_pool_fetch_fine_directory(gasm_pool* p, const uint16_t** fdir, int* fbits);
int gasm_pool_graph(gasm_pool* p, uint32_t n_local_segments);
int gasm_pool_piece_words(gasm_pool* p, uint32_t seg_lo, uint32_t seg_hi, uint64_t* n_words /* seg_hi - seg_lo */);
int gasm_pool_pack_reads(gasm_pool* p, uint32_t seg_lo, uint32_t seg_hi, void* d_words_out);
int gasm_pool_set_reads(gasm_pool* p, const void* d_words, uint64_t n_words, uint32_t n_pieces, const uint32_t* piece_seg,
                        const uint64_t* piece_reads, const uint64_t* piece_word_off);
int gasm_pool_score(gasm_pool* p, int kmer, const double* table);
int gasm_pool_fetch_distinct(gasm_pool* p, const uint64_t** seg_off, const uint64_t** keys, const uint32_t** mult, int* words);
int gasm_pool_fetch_contigs(gasm_pool* p, const uint64_t** seg_contig_off, const uint64_t** off, const char** data);
int gasm_pool_fetch_scores(gasm_pool* p, const double** bp_score, const double** norm_by_break_freqs, const double** norm_by_len,
                           const int32_t** kmer_breaks, const int32_t** sequence_len);

/* ------------------------------------------------------------------------------------------------------------------
 * The pooled step with the exchanges inside the library (csrc/exchange.hip): what the north star calls "an RCCL all-to-all
 * over xGMI to bucket k-mers by hash before the global edge-list merge", as ONE call per step.  The reference analogue is
 * the sequential loop over segments, scripts/02_Real_vs_rand_prob_own.R:33-53.
 *
 *   gasm_comm_unique_id          128 bytes (ncclUniqueId) made by one rank and handed to all others by the caller's
 *                                bootstrap (a file, MPI, torch.distributed's store, ...): the only thing the host layer moves
 *   gasm_comm_create             ncclCommInitRank on the context's GPU: one rank per process, RCCL over xGMI
 *   gasm_comm_create_virtual     `world` ranks inside this process on one GPU; exchanges become device copies on the context's
 *                                stream — the same plans, kernels and directories, testable on a one-GPU box
 *   gasm_comm_stage              what the running gasm_pool_exchange_build is doing (10 local runs, 11/12/13 exchange 1: plan,
 *                                transfer, merge, 21/22/23 exchange 2, 31 reads, 32 scoring, 0 idle): for watchdogs
 *   gasm_pool_bucket_owner       owner rank of every bucket (index = segment << bbits | prefix)
 *   gasm_pool_segment_bounds     first[r] .. first[r + 1]: the segments rank r builds, scores and returns
 *   gasm_pool_exchange_build     local runs -> all-to-all #1 -> merge -> all-to-all #2 -> graph + contigs -> all-to-all #3
 *                                (reads) -> scoring (table != NULL).  pools: the caller's pool (RCCL) or one pool per
 *                                virtual rank, in rank order.  Run lengths, offsets and run directories stay on the device;
 *                                the host waits for two small reports per step (per-peer totals: ncclSend / ncclRecv take their
 *                                counts from the host).  Capacity failures are collective: every rank's overflow flag travels
 *                                with the length tables, all ranks take the same step of the retry ladder (exact partition,
 *                                larger tables, two more bucket bits) or return GASM_ERR_CAPACITY together.
 *                                stats (optional, 8 words): bytes the first local rank sent in exchange 1, 2, 3; of those to
 *                                other ranks; attempts; bucket bits used.  Results: gasm_pool_fetch_* of every pool.
 * ---------------------------------------------------------------------------------------------------------------- */
#define GASM_COMM_ID_BYTES 128
typedef struct gasm_comm gasm_comm;
int gasm_comm_unique_id(void* id /* GASM_COMM_ID_BYTES */);
int gasm_comm_create(gasm_ctx* ctx, const void* id, int rank, int world, gasm_comm** out);
int gasm_comm_create_virtual(gasm_ctx* ctx, int world, gasm_comm** out);
void gasm_comm_destroy(gasm_comm* c);
int gasm_comm_world(const gasm_comm* c);
int gasm_comm_rank(const gasm_comm* c);      /* -1: virtual */
int gasm_comm_stage(const gasm_comm* c);
/* Debugging aid (tests): read-only access to the exchange plans.  After gasm_comm_keep_plans(c, 1) every
 * gasm_pool_exchange_build sets the arrays its plan kernels wrote aside (device copies behind each plan; no kernel launch, and
 * nothing at all while keeping is off, the default).  gasm_comm_fetch_plan copies out plan `which` (1: every bucket's runs to
 * the bucket's owner, 2: the merged runs to the segment's owner) of the last attempt of the last exchange for one local rank
 * (virtual communicator: the rank; RCCL: 0).  sizes = {entries of send_off, of run_off / run_len (rows x world), of bstart,
 * world}; send_tot and recv_tot have `world` entries; info = {info[0], info[1], the OR-ed flag word} (plan 1: info[0] = the
 * merged runs' capacity, info[1] = 0; plan 2: the rank's distinct k-mers in all and of its largest segment).  The arrays are
 * host memory of the communicator, valid until the next fetch of the same plan and rank. */
int gasm_comm_keep_plans(gasm_comm* c, int on);
int gasm_comm_fetch_plan(gasm_comm* c, int which, uint32_t local_rank, uint64_t* sizes /* 4 */, const uint64_t** send_off,
                         const uint64_t** send_tot, const uint64_t** run_off, const uint32_t** run_len, const uint64_t** recv_tot,
                         const uint64_t** bstart, const uint64_t** info /* 3 */);
int gasm_pool_bucket_owner(uint32_t n_segments, int bbits, uint32_t world, uint32_t* owner /* n_segments << bbits */);
int gasm_pool_segment_bounds(uint32_t n_segments, uint32_t world, uint32_t* first /* world + 1 */);
int gasm_pool_exchange_build(gasm_comm* c, gasm_pool* const* pools, uint32_t n_pools, int k, int bbits, int kmer,
                             const double* table /* 69 904 rows or NULL */, uint64_t* stats /* 8 words or NULL */);

/* ------------------------------------------------------------------------------------------------------------------
 * Breakage-score-guided traversal (BASELINE configs[4]'s "combined" mode).  NOT in the reference
 * (README.md:83 "out of scope"): specified by this project, parity = agreement with the project's own CPU
 * restatement (oracle/guided_oracle.py).  Contigs end at branching nodes; guided scaffolds chain them through those nodes:
 * seeds by descending breakage score per base (exact rational of the fixed-point sums), each extended to the right, then to
 * the left, by the best-scoring unused contig that overlaps by k-1 bases; every contig is used once.  Call after
 * gasm_batch_build + gasm_batch_score.  fetch: scaffolds per segment (longest first), their text and scores.
 * ---------------------------------------------------------------------------------------------------------------- */
int gasm_batch_guided(gasm_batch* b);
int gasm_batch_fetch_guided(gasm_batch* b, const uint64_t** seg_off /*n_segments+1*/, const uint64_t** off, const char** data,
                            const double** bp_score, const double** norm_by_len, const int32_t** kmer_breaks);
/* the exact fixed-point sums behind the batch scores: bp_score[c] == fx[c] * 2^-shift.  GASM_ERR_STATE when the last
 * gasm_batch_score took the FP64 scorer (reads shorter than k, or a table the fixed point cannot hold: see gasm_batch_score);
 * gasm_batch_guided needs the same sums and fails the same way */
int gasm_batch_fetch_score_fixed(gasm_batch* b, const int64_t** fx, int* shift);

/* ------------------------------------------------------------------------------------------------------------------
 * gasm_batch_score under several tables at once (the batch form of gasm_calc_breakscore_tables: the true and the uniform
 * table of lib/DeNovoAssembler.R:325-355 over one match).  tables: n_tables x GASM_TABLE_ROWS, row-major; n_tables in
 * 1..GASM_MAX_TABLES (else GASM_ERR_INVALID); n_tables == 1 is gasm_batch_score.  Queued on the build's step slot like
 * gasm_batch_score (no host wait on the fixed-point path; `build; score_tables; build; score_tables` overlaps the same way).
 * Shared by the tables: each read's k-mer lookup, link, contig and break window, and the per-contig hit count.  Per table:
 * the gather of the window's weight and the 64-bit sum, each table with its own fixed-point shift by gasm_batch_score's
 * rule.  The graph-indexed fixed-point scorer runs when the reads allow it and EVERY table has a valid shift; otherwise all
 * tables go through the FP64 position scorer (gasm_batch_fetch_score_fixed_table then returns GASM_ERR_STATE for each).
 * Table t's results are bit for bit those of gasm_batch_score with table t whenever both take the same scorer (always,
 * except for a table that has a shift of its own while another table of the call sent them all to the FP64 scorer).
 * gasm_batch_fetch_scores_table / gasm_batch_fetch_score_fixed_table: table t of the last score; t must be below its table
 * count (1 after a plain gasm_batch_score), else GASM_ERR_INVALID.  gasm_batch_fetch_scores, gasm_batch_fetch_score_fixed
 * and gasm_batch_guided refer to table 0.  Each fetch's host copy stays valid until the next fetch of the batch.
 * ---------------------------------------------------------------------------------------------------------------- */
int gasm_batch_score_tables(gasm_batch* b, int kmer, const double* tables, uint32_t n_tables);
int gasm_batch_fetch_scores_table(gasm_batch* b, uint32_t t, const double** bp_score, const double** norm_by_break_freqs,
                                  const double** norm_by_len, const int32_t** kmer_breaks, const int32_t** sequence_len);
int gasm_batch_fetch_score_fixed_table(gasm_batch* b, uint32_t t, const int64_t** fx, int* shift);

/* Per-kernel device time of the stages of build/score, accumulated with HIP events on the ctx stream since the last
 * reset (profiling on costs one event pair per launch).  names/ms/launches point into library storage. */
int gasm_profile_enable(gasm_ctx* ctx, int on);
/* restrict profiling to the comma-separated kernel names (NULL or "" = every kernel) */
int gasm_profile_filter(gasm_ctx* ctx, const char* names);
int gasm_profile_reset(gasm_ctx* ctx);
int gasm_profile_read(gasm_ctx* ctx, int* n, const char* const** names, const double** ms, const uint64_t** launches);

/* The path the last finished gasm_batch_build took: one row of GASM_PLAN_FIELDS int32 words that describes the final
 * attempt of the build.  A pending build is finished first, as the fetches do.  Host bookkeeping only: no device reads,
 * no effect on the pipeline.  Returns the number of rows (always 1) and writes the row when it fits in n words (out may
 * be NULL when n == 0); a negative value is a GASM_ERR status (GASM_ERR_STATE before the first build). */
#define GASM_PLAN_FIELDS 15
#define GASM_PLAN_KEY_WORDS 0          /* 1: 64-bit keys (k <= 31), 2: 128-bit keys */
#define GASM_PLAN_BUCKET_BITS 1        /* buckets per segment = 2^bits */
#define GASM_PLAN_TABLE_SLOTS 2        /* LDS table of the one-pass de-duplication: 2048 or 4096 slots */
#define GASM_PLAN_SINGLE_PASS 3        /* 1: one-pass partition (k_bucket_partition); 0: count + scan + scatter */
#define GASM_PLAN_MULTI_PASS 4         /* 1: de-duplication in passes over key sub-ranges (k_bucket_dedup_multi) */
#define GASM_PLAN_SCAN_IN_DEDUP 5      /* 1: bucket offsets from the de-duplication's last workgroup; 0: k_scan_excl */
#define GASM_PLAN_RANKED_IN_LDS 6      /* 1: list ranking in LDS (k_rank_rulers, k_rank_lds, k_link_jump) */
#define GASM_PLAN_RULER_SHIFT 7        /* LDS ranking: rulers every 2^shift-th edge; 0 when not ranked in LDS */
#define GASM_PLAN_RANK_GLOBAL 8        /* 1: whole-GPU ranking forced (GASM_RANK_GLOBAL, or after the LDS ranking gave up) */
#define GASM_PLAN_TILE_G 9             /* threads per read of the tile kernels */
#define GASM_PLAN_OFFSET_ROUNDS 10     /* offset rounds (tiles) per group of reads */
#define GASM_PLAN_DISTINCT_ATTEMPTS 11 /* partition + de-duplication attempts (1 + overflow retries; 0: no k-mers) */
#define GASM_PLAN_GRAPH_ATTEMPTS 12    /* graph-only repeats (the LDS ranking gave up) */
#define GASM_PLAN_K 13
#define GASM_PLAN_SEGMENTS 14          /* segments of the batch */
int gasm_batch_build_plan(gasm_batch* b, int32_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* GASM_H */
