// capi.hip — the extern "C" surface declared in include/gasm.h.
#include <algorithm>
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>

#include "pipeline.h"
#include "scaffolds.h"

struct gasm_strlist {
    std::vector<char> data;
    std::vector<u64> off;
};

struct gasm_contigs {
    std::vector<char> data;
    std::vector<u64> off;
    u64 rows = 0;
    std::vector<u32> perm;
    int words = 1;
    std::vector<u64> dkeys;
    std::vector<u32> dmult;
};

struct gasm_packed {
    gasm_host::PackedReads pr;
    std::vector<u64> seg;
    u64 dropped = 0;
    std::vector<u8> on_device;       // per file: parsed and packed by the device path (gasm_read_files_device)
    std::vector<u64> stats, hist;    // an ingest under options: GASM_INGEST_STATS / GASM_QUAL_BINS per file (else empty)
};

struct gasm_scores {
    u64 n = 0;
    std::vector<int32_t> len, breaks, lev, startpos;
    std::vector<double> bp, nf, nl, pd, ks;
    // path_freq does not depend on the table: the results of one gasm_calc_breakscore_tables call share one buffer (at
    // 22 000 scaffolds a dense copy per table would be several GB)
    std::shared_ptr<const std::vector<double>> freq;
    std::vector<u64> pd_off;
    bool has_freq = false, velvet = false, has_ks = false;
    int lev_device = 0;      // who computed lev: 0 nobody (not asked), 1 the GPU (k_levenshtein), 2 host threads (gasm_host::levenshtein)
};

// What one step (build + scoring) of a batch owns: the graph, the contigs as paths, the scores — and the stream it runs on.
struct StepSlot {
    gasm_ctx* cx = nullptr;
    BuildState bs;
    DevPaths dp;
    ScoreState ss;
    bool paths_ready = false;
};

struct gasm_batch {
    gasm_ctx* ctx = nullptr;
    u32 n_segments = 0;
    u64 n_reads = 0;
    DevReads rd;
    // strands = 2 builds read this instead: the reads and their reverse complements (DevReads::make_both_strands), made by the first
    // such build and shared read-only by every step slot; scoring, read k-mer counts and the guided traversal keep `rd`
    DevReads rd2;
    // the reads the build a slot holds was made from (whoever finishes, repeats or fetches that build hands them on)
    DevReads& build_reads(const StepSlot& x) { return x.bs.opts.strands == 2 ? rd2 : rd; }
    // the breakage tables of gasm_batch_score(_tables) (table 0: what gasm_batch_score, gasm_batch_guided and the plain
    // fetches use) and what each was set from (empty: never); a table stays resident until another takes its place
    ScoreTable tb[GASM_MAX_TABLES];
    std::vector<double> table_copy[GASM_MAX_TABLES];
    void table_ptrs(ScoreTable** tbs) { for (u32 t = 0; t < GASM_MAX_TABLES; ++t) tbs[t] = &tb[t]; }
    // the tables of gasm_batch_score_mapped, its own: what gasm_batch_score(_tables) set stays what it was
    ScoreTable mtb[GASM_MAX_TABLES];
    std::vector<double> mtable_copy[GASM_MAX_TABLES];
    GuidedState guided;
    // Step slots, taken in turn (GASM_PINGPONG=0 switches it off): consecutive steps of a resident pipeline are independent
    // of each other — same reads, own graph, own scores — so step n + 1 is queued on the next slot's stream with that slot's
    // buffers, and its streaming kernels (partition, de-duplication: HBM and LDS) run beside the graph and scoring kernels
    // of the steps before it (latency-bound, a few waves per CU).  GASM_STEP_SLOTS of them (2..4, default 3).  Results are
    // always those of the slot the last gasm_batch_build took.
    StepSlot slot[4];
    int cur = 0, n_slots = 2;
    StepSlot& S() {
        StepSlot& x = slot[cur];
        if (!x.cx) x.cx = cur ? ctx->lane((size_t)cur) : ctx;      // (lane 0 stays idle: the streams the slots were measured on)
        if (!x.cx) x.cx = ctx;                // (no second stream to be had: every slot on the batch's own)
        return x;
    }
    const StepSlot& S() const { return slot[cur]; }
    bool built = false;
    // the last gasm_batch_score(_tables), kept to queue it again behind a build that had to be repeated
    bool scored = false;
    int score_kmer = 0;
    u32 score_tables = 1;
    int last_k = 0;                         // k of the last gasm_batch_build
    // simulated batches: the start of every read in its genome
    DBuf d_read_start;
    std::vector<u32> h_read_start;
    std::vector<int64_t> h_fx;
    std::vector<u64> h_sim_seg_off;
    // break-k-mer counts of the reads (gasm_batch_count_read_kmers): GASM_TABLE_ROWS per segment; reads only d_words / d_read_off
    DBuf d_rkc;
    bool rkc_checked = false;               // read_kmer_windows_check passed (the reads never change)
    bool rkc_counted = false;
    std::vector<u32> h_rkc;
    // a batch made by gasm_batch_correct_reads: the correction's counters, GASM_CORRECT_FIELDS per segment
    DBuf d_correct;
    bool corrected = false;
    std::vector<u32> h_correct;
    // gasm_batch_fetch_reads: the reads as ASCII and their offsets
    std::vector<char> h_reads_ascii;
    std::vector<u64> h_reads_off;
    // a batch made by gasm_batch_from_files_params under options: what the ingest did, per segment (else empty)
    std::vector<u64> h_ingest_stats, h_ingest_hist;
};

// the last gasm_batch_score or gasm_batch_score_tables on slot x
static int batch_queue_score(gasm_batch* b, StepSlot& x) {
    ScoreTable* tbs[GASM_MAX_TABLES];
    b->table_ptrs(tbs);
    return pipeline_score_launch(x.cx, b->rd, x.dp, b->score_kmer, tbs, b->score_tables, false, false, x.ss, &x.bs);
}

// Read the report of the batch's queued build (repeating the build if it failed, and then the scoring queued behind it).
static int batch_finish(gasm_batch* b) {
    StepSlot& x = b->S();
    bool rebuilt = false;
    GCHK(pipeline_build_finish(x.cx, b->build_reads(x), x.bs, &rebuilt));
    if (rebuilt) {
        x.paths_ready = false;
        if (b->scored) {
            GCHK(pipeline_contig_paths(x.cx, b->rd, x.bs, x.dp));
            x.paths_ready = true;
            pipeline_contig_paths_host(b->rd, x.bs, x.dp);
            GCHK(batch_queue_score(b, x));
        }
    }
    return GASM_OK;
}

static void strlist_from(const std::vector<std::string>& v, std::vector<char>& data, std::vector<u64>& off) {
    off.assign(v.size() + 1, 0);
    size_t tot = 0;
    for (size_t i = 0; i < v.size(); ++i) { tot += v[i].size(); off[i + 1] = tot; }
    data.resize(tot);
    for (size_t i = 0; i < v.size(); ++i) memcpy(data.data() + off[i], v[i].data(), v[i].size());
}

// a new batch of `ctx` whose reads `fill(batch)` puts in place; handed out only if that succeeded
template <class F>
static int new_batch(gasm_ctx* ctx, u32 n_segments, u64 n_reads, gasm_batch** out, F&& fill) {
    gasm_batch* b = new gasm_batch();
    b->ctx = ctx;
    b->n_segments = n_segments;
    b->n_reads = n_reads;
    const int st = fill(b);
    if (st != GASM_OK) { gasm_batch_free(b); return st; }
    *out = b;
    return GASM_OK;
}

extern "C" {

static int breakscore_impl(gasm_ctx* ctx, DevPaths& dp, const std::function<std::string(u64)>& path_text, uint64_t n_paths, const char* reads,
                           const uint64_t* read_off, uint64_t n_reads, const char* true_solution, uint64_t true_len, int kmer,
                           const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table, const double* bp_probs, uint32_t n_tables,
                           int variant, int flags, gasm_scores** out);

// ------------------------------------------------------------------------------------------------- get_contigs
// reads (ragged when read_off != nullptr, else n_reads reads of fixed_len) of ONE segment -> contigs + shuffle matrix; `o` has passed
// build_opts_check
static int contigs_of_reads(gasm_ctx* ctx, const char* bases, const u64* read_off, u64 n_reads, u32 fixed_len, int seed, int matrix_rows, gasm_contigs** out,
                            const BuildOpts& o) {
    DevReads rd, rd2;
    BuildState bs;
    const u64 seg_off[2] = {0, n_reads};
    int st = rd.upload(ctx, bases, read_off, n_reads, fixed_len, seg_off, 1);
    if (st == GASM_OK && o.strands == 2) st = rd2.make_both_strands(ctx, rd);
    DevReads& br = o.strands == 2 ? rd2 : rd;
    if (st == GASM_OK) st = pipeline_build(ctx, br, bs, o);
    if (st == GASM_OK) st = pipeline_fetch_distinct(ctx, br, bs);
    if (st == GASM_OK) st = pipeline_fetch_contigs(ctx, br, bs);
    gasm_contigs* c = nullptr;
    if (st == GASM_OK) {
        c = new gasm_contigs();
        c->data = bs.h_contigs;
        c->off = bs.h_c_off;
        c->words = bs.words;
        c->dkeys = bs.h_dk_key;
        c->dmult = bs.h_dk_cnt;
        c->rows = (u64)matrix_rows;
        // lib/DeNovoAssembler.cpp:195-203
        gasm_host::shuffle_perm(bs.n_contigs, seed, (u64)matrix_rows, c->perm);
    }
    rd.release(); rd2.release();
    bs.release();
    if (st != GASM_OK) return st;
    *out = c;
    return GASM_OK;
}

// what every gasm_get_contigs_from_reads* entry does with the options it filled `o` from; `entry`: the one that was called
static int contigs_from_reads(const char* entry, gasm_ctx* ctx, const char* reads, const u64* read_off, u64 n_reads, int seed, int matrix_rows, const BuildOpts& o,
                              gasm_contigs** out) {
    if (!ctx || !out || (n_reads && (!reads || !read_off))) { gasm_set_error("%s: null argument", entry); return GASM_ERR_INVALID; }
    if (matrix_rows < 0) { gasm_set_error("matrix_rows must be >= 0"); return GASM_ERR_INVALID; }
    // (min_count and strands in front of *out = nullptr, the other options behind it: the order the entries have always had)
    BuildOpts first;
    first.min_count = o.min_count; first.strands = o.strands;
    GCHK(build_opts_check(first));
    *out = nullptr;
    GCHK(build_opts_check(o));
    return contigs_of_reads(ctx, reads, read_off, n_reads, 0, seed, matrix_rows, out, o);
}

// the struct form: its own checks (null, size) and its "0 means default" mapping; the fields' rules are build_opts_check's
static int opts_from_params(const char* entry, const gasm_build_params* p, BuildOpts& o) {
    if (!p) { gasm_set_error("%s: params is null", entry); return GASM_ERR_INVALID; }
    if (p->size != sizeof(gasm_build_params)) {
        gasm_set_error("%s: params->size is %u, this library's gasm_build_params has %zu bytes", entry, p->size, sizeof(gasm_build_params));
        return GASM_ERR_INVALID;
    }
    o.k = p->k; o.genome_len_hint = p->genome_len_hint;
    o.min_count = p->min_count ? p->min_count : 1; o.strands = p->strands ? p->strands : 1;
    o.tip_len = p->tip_len; o.tip_rounds = p->tip_rounds;
    o.bubble_len = p->bubble_len; o.bubble_rounds = p->bubble_rounds;
    o.cov_cutoff = p->cov_cutoff; o.cov_len = p->cov_len; o.cov_rounds = p->cov_rounds;
    return GASM_OK;
}

int gasm_get_contigs(gasm_ctx* ctx, const char* kmers, uint64_t n_kmers, int dbg_kmer, int seed, int matrix_rows,
                     gasm_contigs** out) {
    API_GUARD_BEGIN
    if (!ctx || !out || (n_kmers && !kmers)) { gasm_set_error("gasm_get_contigs: null argument"); return GASM_ERR_INVALID; }
    if (matrix_rows < 0) { gasm_set_error("matrix_rows must be >= 0"); return GASM_ERR_INVALID; }
    *out = nullptr;
    // the exploded k-mers are reads of length k with one k-mer each
    BuildOpts o;
    o.k = dbg_kmer;
    return contigs_of_reads(ctx, kmers, nullptr, n_kmers, (u32)dbg_kmer, seed, matrix_rows, out, o);
    API_GUARD_END
}

int gasm_get_contigs_from_reads(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                int matrix_rows, gasm_contigs** out) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = dbg_kmer;
    return contigs_from_reads("gasm_get_contigs_from_reads", ctx, reads, read_off, n_reads, seed, matrix_rows, o, out);
    API_GUARD_END
}

int gasm_get_contigs_from_reads_solid(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                      int matrix_rows, uint32_t min_count, gasm_contigs** out) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = dbg_kmer; o.min_count = min_count;
    return contigs_from_reads("gasm_get_contigs_from_reads_solid", ctx, reads, read_off, n_reads, seed, matrix_rows, o, out);
    API_GUARD_END
}

int gasm_get_contigs_from_reads_strands(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                        int matrix_rows, uint32_t min_count, uint32_t strands, gasm_contigs** out) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = dbg_kmer; o.min_count = min_count; o.strands = strands;
    return contigs_from_reads("gasm_get_contigs_from_reads_strands", ctx, reads, read_off, n_reads, seed, matrix_rows, o, out);
    API_GUARD_END
}

int gasm_get_contigs_from_reads_tips(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                     int matrix_rows, uint32_t min_count, uint32_t strands, uint32_t tip_len, uint32_t tip_rounds,
                                     gasm_contigs** out) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = dbg_kmer; o.min_count = min_count; o.strands = strands; o.tip_len = tip_len; o.tip_rounds = tip_rounds;
    return contigs_from_reads("gasm_get_contigs_from_reads_tips", ctx, reads, read_off, n_reads, seed, matrix_rows, o, out);
    API_GUARD_END
}

int gasm_get_contigs_from_reads_bubbles(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed,
                                        int matrix_rows, uint32_t min_count, uint32_t strands, uint32_t tip_len, uint32_t tip_rounds,
                                        uint32_t bubble_len, uint32_t bubble_rounds, gasm_contigs** out) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = dbg_kmer; o.min_count = min_count; o.strands = strands; o.tip_len = tip_len; o.tip_rounds = tip_rounds;
    o.bubble_len = bubble_len; o.bubble_rounds = bubble_rounds;
    return contigs_from_reads("gasm_get_contigs_from_reads_bubbles", ctx, reads, read_off, n_reads, seed, matrix_rows, o, out);
    API_GUARD_END
}

int gasm_get_contigs_from_reads_params(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int seed, int matrix_rows,
                                       const gasm_build_params* params, gasm_contigs** out) {
    API_GUARD_BEGIN
    BuildOpts o;
    GCHK(opts_from_params("gasm_get_contigs_from_reads_params", params, o));
    return contigs_from_reads("gasm_get_contigs_from_reads_params", ctx, reads, read_off, n_reads, seed, matrix_rows, o, out);
    API_GUARD_END
}

uint64_t gasm_contigs_count(const gasm_contigs* c) { return c ? c->off.size() - 1 : 0; }
const char* gasm_contigs_data(const gasm_contigs* c) { return c ? c->data.data() : nullptr; }
const uint64_t* gasm_contigs_offsets(const gasm_contigs* c) { return c ? c->off.data() : nullptr; }
uint64_t gasm_contigs_rows(const gasm_contigs* c) { return c ? c->rows : 0; }
const uint32_t* gasm_contigs_perm(const gasm_contigs* c) { return c ? c->perm.data() : nullptr; }
uint64_t gasm_contigs_distinct_count(const gasm_contigs* c) { return c ? c->dmult.size() : 0; }
int gasm_contigs_key_words(const gasm_contigs* c) { return c ? c->words : 0; }
const uint64_t* gasm_contigs_distinct_keys(const gasm_contigs* c) { return c ? c->dkeys.data() : nullptr; }
const uint32_t* gasm_contigs_distinct_mult(const gasm_contigs* c) { return c ? c->dmult.data() : nullptr; }
void gasm_contigs_free(gasm_contigs* c) { delete c; }

// -------------------------------------------------------------------------------------------- assemble_contigs
// the device route: greedy merge on contig indices (host threads), scaffolds expanded, ordered and de-duplicated on the GPU
// *used = false when the index form does not apply (the caller takes the host's string form)
static int assemble_device(gasm_ctx* ctx, const char* contigs, const u64* off, u64 n, const u32* perm, u64 rows, u64 row_len, int k, gasm_scaffolds** out,
                           bool* used) {
    *used = false;
    std::vector<std::string> c(n);
    for (u64 i = 0; i < n; ++i) c[i].assign(contigs + off[i], contigs + off[i + 1]);
    for (u64 i = 0; i < rows * row_len; ++i)
        if (perm[i] >= n) { gasm_set_error("perm[%llu] = %u out of range", (unsigned long long)i, perm[i]); return GASM_ERR_INVALID; }
    if (row_len != n) return GASM_OK;                       // (rows that are not permutations of all contigs: the string form)
    std::vector<std::string> sigs;
    bool on_gpu = false;
    // the merge itself on the GPU (a wave per permutation); GASM_ASM_HOST_MERGE=1: on host threads (same signatures)
    u64 rows_on_host = 0;
    if (!getenv("GASM_ASM_HOST_MERGE")) GCHK(assemble_signatures_device(ctx, c, perm, rows, row_len, k, sigs, &on_gpu, &rows_on_host));
    if (!on_gpu && !gasm_host::assemble_signatures(c, perm, rows, row_len, k, sigs)) return GASM_OK;
    *used = true;
    GCHK(scaffolds_from_signatures(ctx, c, sigs, out));
    // who ran the greedy merge (the results are the same; a caller can ask): the GPU, host threads, or both
    (*out)->rows_total = rows;
    (*out)->rows_on_host = on_gpu ? rows_on_host : rows;
    return GASM_OK;
}

static int assemble_common(gasm_ctx* ctx, const char* contigs, const u64* off, u64 n, const u32* perm, u64 rows, u64 row_len, int k, gasm_strlist** out) {
    if (ctx && !getenv("GASM_ASM_HOST")) {
        gasm_scaffolds* sc = nullptr;
        bool used = false;
        GCHK(assemble_device(ctx, contigs, off, n, perm, rows, row_len, k, &sc, &used));
        if (used) {
            gasm_strlist* s = new gasm_strlist();
            const int st = scaffolds_fetch(sc, s->data, s->off);
            gasm_scaffolds_free(sc);
            if (st != GASM_OK) { delete s; return st; }
            *out = s;
            return GASM_OK;
        }
    }
    std::vector<std::string> c(n);
    for (u64 i = 0; i < n; ++i) c[i].assign(contigs + off[i], contigs + off[i + 1]);
    for (u64 i = 0; i < rows * row_len; ++i)
        if (perm[i] >= n) { gasm_set_error("perm[%llu] = %u out of range", (unsigned long long)i, perm[i]); return GASM_ERR_INVALID; }
    std::vector<std::string> res;
    GCHK(gasm_host::assemble(c, perm, rows, row_len, k, res));
    gasm_strlist* s = new gasm_strlist();
    strlist_from(res, s->data, s->off);
    *out = s;
    return GASM_OK;
}

int gasm_assemble_contigs(gasm_ctx* ctx, const char* contigs, const uint64_t* off, uint64_t n, const uint32_t* perm,
                          uint64_t rows, uint64_t row_len, int dbg_kmer, gasm_strlist** out) {
    API_GUARD_BEGIN
    if (!out || !off || (n && !contigs) || (rows && row_len && !perm)) { gasm_set_error("gasm_assemble_contigs: null argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    return assemble_common(ctx, contigs, off, n, perm, rows, row_len, dbg_kmer, out);
    API_GUARD_END
}

int gasm_assemble_contigs_velvet(gasm_ctx* ctx, const char* contigs, const uint64_t* off, uint64_t n, int dbg_kmer, int seed,
                                 int rows, gasm_strlist** out) {
    API_GUARD_BEGIN
    if (!out || !off || (n && !contigs) || rows < 0) { gasm_set_error("gasm_assemble_contigs_velvet: bad argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    std::vector<u32> perm;
    gasm_host::shuffle_perm(n, seed, (u64)rows, perm);  // lib/BreakageScorer.cpp:86-94
    return assemble_common(ctx, contigs, off, n, perm.data(), (u64)rows, n, dbg_kmer, out);
    API_GUARD_END
}

// ---- the same with the scaffolds left on the device
int gasm_assemble_contigs_dev(gasm_ctx* ctx, const char* contigs, const uint64_t* off, uint64_t n, const uint32_t* perm, uint64_t rows, uint64_t row_len,
                              int dbg_kmer, gasm_scaffolds** out) {
    API_GUARD_BEGIN
    if (!ctx || !out || !off || (n && !contigs) || (rows && row_len && !perm)) { gasm_set_error("gasm_assemble_contigs_dev: null argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    bool used = false;
    GCHK(assemble_device(ctx, contigs, off, n, perm, rows, row_len, dbg_kmer, out, &used));
    if (!used) {
        // contigs shorter than k-1 (the reference compares whole strings or throws there), or rows that are not full
        // permutations: the host's string form, then the text goes to the device as a one-contig-per-scaffold chain set
        gasm_strlist* sl = nullptr;
        GCHK(assemble_common(nullptr, contigs, off, n, perm, rows, row_len, dbg_kmer, &sl));
        std::vector<std::string> txt(sl->off.size() - 1), sigs;
        for (size_t i = 0; i + 1 < sl->off.size(); ++i) txt[i].assign(sl->data.data() + sl->off[i], sl->data.data() + sl->off[i + 1]);
        gasm_strlist_free(sl);
        // (already sorted, distinct and in final order: hand them over as they are)
        gasm_scaffolds* sc = new gasm_scaffolds();
        sc->ctx = ctx; sc->n = (u32)txt.size();
        sc->h_off.assign(1, 0);
        std::string cat;
        for (auto& t : txt) { cat += t; sc->h_off.push_back(cat.size()); }
        DevPaths tmp;
        std::vector<u64> o(sc->h_off);
        const int st = tmp.upload_ascii(ctx, cat.data(), o.data(), sc->n);
        if (st != GASM_OK) { tmp.release(); delete sc; return st; }
        sc->d_words = tmp.d_words; tmp.d_words = DBuf();
        tmp.release();
        *out = sc;
    }
    return GASM_OK;
    API_GUARD_END
}

int gasm_assemble_contigs_velvet_dev(gasm_ctx* ctx, const char* contigs, const uint64_t* off, uint64_t n, int dbg_kmer, int seed, int rows,
                                     gasm_scaffolds** out) {
    API_GUARD_BEGIN
    if (!ctx || !out || !off || (n && !contigs) || rows < 0) { gasm_set_error("gasm_assemble_contigs_velvet_dev: bad argument"); return GASM_ERR_INVALID; }
    std::vector<u32> perm;
    gasm_host::shuffle_perm(n, seed, (u64)rows, perm);  // lib/BreakageScorer.cpp:86-94
    return gasm_assemble_contigs_dev(ctx, contigs, off, n, perm.data(), (u64)rows, n, dbg_kmer, out);
    API_GUARD_END
}

uint64_t gasm_scaffolds_count(const gasm_scaffolds* s) { return s ? s->n : 0; }
int gasm_scaffolds_merge_device(const gasm_scaffolds* s, uint64_t* rows_on_host) {
    if (rows_on_host) *rows_on_host = s ? s->rows_on_host : 0;
    if (!s) return 0;
    return s->rows_on_host == 0 ? 1 : (s->rows_on_host >= s->rows_total ? 2 : 3);
}
const uint64_t* gasm_scaffolds_offsets(const gasm_scaffolds* s) { return s ? s->h_off.data() : nullptr; }
int gasm_scaffolds_fetch(const gasm_scaffolds* s, gasm_strlist** out) {
    API_GUARD_BEGIN
    if (!s || !out) { gasm_set_error("gasm_scaffolds_fetch: null argument"); return GASM_ERR_INVALID; }
    gasm_strlist* l = new gasm_strlist();
    const int st = scaffolds_fetch(s, l->data, l->off);
    if (st != GASM_OK) { delete l; return st; }
    *out = l;
    return GASM_OK;
    API_GUARD_END
}
void gasm_scaffolds_free(gasm_scaffolds* s) {
    if (!s) return;
    if (s->ctx) { (void)hipSetDevice(s->ctx->device); (void)hipStreamSynchronize(s->ctx->stream); }
    s->d_words.release();
    delete s;
}

// out[t] = NULL for the entries a tables call may hand back; false (and the error set) when n_tables is out of range
static bool tables_out_clear(const char* who, gasm_scores** out, uint32_t n_tables) {
    if (out) for (uint32_t t = 0; t < std::min<uint32_t>(n_tables, GASM_MAX_TABLES); ++t) out[t] = nullptr;
    if (n_tables >= 1 && n_tables <= GASM_MAX_TABLES) return true;
    gasm_set_error("%s: n_tables must be 1..%d (got %u)", who, GASM_MAX_TABLES, n_tables);
    return false;
}

// gasm_calc_breakscore_dev (one table) and gasm_calc_breakscore_tables_dev
static int breakscore_dev(const char* who, gasm_ctx* ctx, const gasm_scaffolds* paths, const char* reads, const uint64_t* read_off, uint64_t n_reads,
                          const char* true_solution, uint64_t true_len, int kmer, const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table,
                          const double* bp_probs, uint32_t n_tables, int variant, int flags, gasm_scores** out) {
    if (!tables_out_clear(who, out, n_tables)) return GASM_ERR_INVALID;
    if (!ctx || !out || !paths || !read_off || !bp_off || (n_table && (!bp_kmer || !bp_probs)) || (true_len && !true_solution)) {
        gasm_set_error("%s: null argument", who);
        return GASM_ERR_INVALID;
    }
    if (variant != GASM_SCORE_OWN && variant != GASM_SCORE_VELVET) { gasm_set_error("unknown variant %d", variant); return GASM_ERR_INVALID; }
    DevPaths dp;
    int st = scaffolds_as_paths(paths, dp);
    // text of single paths is rarely needed (velvet startpos, host Levenshtein): fetched once, on first use
    std::vector<char> txt;
    std::vector<u64> toff;
    std::mutex mu;
    bool have = false;
    auto path_text = [&](u64 p) {
        std::lock_guard<std::mutex> g(mu);
        if (!have) { (void)scaffolds_fetch(paths, txt, toff); have = true; }
        return toff.size() > p + 1 ? std::string(txt.data() + toff[p], txt.data() + toff[p + 1]) : std::string();
    };
    if (st == GASM_OK)
        st = breakscore_impl(ctx, dp, path_text, paths->n, reads, read_off, n_reads, true_solution, true_len, kmer, bp_kmer, bp_off, n_table, bp_probs,
                             n_tables, variant, flags, out);
    dp.release();
    return st;
}

int gasm_calc_breakscore_dev(gasm_ctx* ctx, const gasm_scaffolds* paths, const char* reads, const uint64_t* read_off, uint64_t n_reads,
                             const char* true_solution, uint64_t true_len, int kmer, const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table,
                             const double* bp_prob, int variant, int flags, gasm_scores** out) {
    API_GUARD_BEGIN
    return breakscore_dev("gasm_calc_breakscore_dev", ctx, paths, reads, read_off, n_reads, true_solution, true_len, kmer, bp_kmer, bp_off, n_table, bp_prob, 1,
                          variant, flags, out);
    API_GUARD_END
}

int gasm_calc_breakscore_tables_dev(gasm_ctx* ctx, const gasm_scaffolds* paths, const char* reads, const uint64_t* read_off, uint64_t n_reads,
                                    const char* true_solution, uint64_t true_len, int kmer, const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table,
                                    const double* bp_probs, uint32_t n_tables, int variant, int flags, gasm_scores** out) {
    API_GUARD_BEGIN
    return breakscore_dev("gasm_calc_breakscore_tables_dev", ctx, paths, reads, read_off, n_reads, true_solution, true_len, kmer, bp_kmer, bp_off, n_table,
                          bp_probs, n_tables, variant, flags, out);
    API_GUARD_END
}

uint64_t gasm_strlist_count(const gasm_strlist* s) { return s ? s->off.size() - 1 : 0; }
const char* gasm_strlist_data(const gasm_strlist* s) { return s ? s->data.data() : nullptr; }
const uint64_t* gasm_strlist_offsets(const gasm_strlist* s) { return s ? s->off.data() : nullptr; }
void gasm_strlist_free(gasm_strlist* s) { delete s; }

// -------------------------------------------------------------------------------------------- calc_breakscore
int gasm_levenshtein(const char* query, uint64_t nq, const char* target, uint64_t nt, int infix, int32_t* out) {
    API_GUARD_BEGIN
    if (!out || (nq && !query) || (nt && !target)) { gasm_set_error("gasm_levenshtein: null argument"); return GASM_ERR_INVALID; }
    *out = gasm_host::levenshtein(query, nq, target, nt, infix != 0);
    return GASM_OK;
    API_GUARD_END
}

// calc_breakscore proper.  `dp` holds the paths on the device (uploaded text or the scaffolds of a device-side
// assemble_contigs); path_text(p) hands out path p as text for the few host-side steps that want it (the velvet variant's
// startpos find, the host Levenshtein routine for a target outside ACGT).
// bp_probs holds n_tables rows of n_table probabilities: the match once and the sums per table (pipeline_score_launch),
// out[0 .. n_tables); gasm_calc_breakscore is n_tables = 1.
// Everything below that does not read a probability runs once and is copied (or, for path_freq, shared) between the results.
static int breakscore_impl(gasm_ctx* ctx, DevPaths& dp, const std::function<std::string(u64)>& path_text, uint64_t n_paths, const char* reads,
                           const uint64_t* read_off, uint64_t n_reads, const char* true_solution, uint64_t true_len, int kmer,
                           const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table, const double* bp_probs, uint32_t n_tables,
                           int variant, int flags, gasm_scores** out) {
    const bool velvet = variant == GASM_SCORE_VELVET;
    const u32 T = n_tables;
    DevReads rd;
    ScoreTable tb[GASM_MAX_TABLES];
    ScoreTable* tbs[GASM_MAX_TABLES];
    for (u32 t = 0; t < GASM_MAX_TABLES; ++t) tbs[t] = &tb[t];
    ScoreState ss;
    const u64 seg_off[2] = {0, n_reads};
    static const char empty = 0;
    int st = rd.upload(ctx, reads ? reads : &empty, read_off, n_reads, 0, seg_off, 1);
    for (u32 t = 0; t < T && st == GASM_OK; ++t) st = tb[t].set(ctx, bp_kmer, bp_off, n_table, bp_probs + (size_t)t * n_table);
    const bool want_freq = !velvet && (flags & GASM_WANT_FREQ);
    if (st == GASM_OK) st = pipeline_score_launch(ctx, rd, dp, kmer, tbs, T, want_freq, velvet, ss, nullptr);
    if (st == GASM_OK) st = pipeline_score_fetch(ctx, ss);
    std::vector<gasm_scores*> res(T, nullptr);
    gasm_scores* s = nullptr;               // table 0's result: what is computed once lands here first
    if (st == GASM_OK) {
        std::shared_ptr<const std::vector<double>> freq;
        if (want_freq) freq = std::make_shared<const std::vector<double>>(std::move(ss.h_freq));
        const size_t P = n_paths, pd_n = ss.h_pd_off.empty() ? 0 : (size_t)ss.h_pd_off.back();
        for (u32 t = 0; t < T; ++t) {
            gasm_scores* r = res[t] = new gasm_scores();
            r->n = n_paths;
            r->velvet = velvet;
            r->len = ss.h_len; r->breaks = ss.h_breaks;
            r->bp.assign(ss.h_bp.begin() + t * P, ss.h_bp.begin() + (t + 1) * P);
            r->nf.assign(ss.h_nf.begin() + t * P, ss.h_nf.begin() + (t + 1) * P);
            r->nl.assign(ss.h_nl.begin() + t * P, ss.h_nl.begin() + (t + 1) * P);
            r->lev.assign(n_paths, 0);
            if (want_freq) { r->freq = freq; r->has_freq = true; }
            if (velvet) {
                if (ss.h_pd.size() >= (t + 1) * pd_n) r->pd.assign(ss.h_pd.begin() + t * pd_n, ss.h_pd.begin() + (t + 1) * pd_n);
                r->pd_off = ss.h_pd_off;
            }
        }
        s = res[0];
        if (velvet) {
            // lib/BreakageScorer.cpp:273-274: start of the path inside the true solution, taken only when a read matched
            s->startpos.assign(n_paths, 0);
            const std::string truth(true_solution ? true_solution : "", true_len);
            for (u64 p = 0; p < n_paths; ++p) {
                if (ss.h_breaks[p] <= 0) continue;
                s->startpos[p] = (int32_t)(int)truth.find(path_text(p));
            }
        }
        if (flags & GASM_WANT_KS) {
            // lib/DeNovoAssembler.R:414-424: ks.test(path_freq, kmer_from_seq)$statistic per path.  The genome's windows are
            // counted per table row once; the ranking of the rows by probability and the paths' side are per table
            std::vector<u32> hist;
            if (n_paths) st = pipeline_ks_genome_hist(ctx, tb[0], true_solution ? true_solution : "", true_len, kmer, hist);
            for (u32 t = 0; t < T && st == GASM_OK; ++t) st = pipeline_ks_paths(ctx, dp, ss, tb[t], hist, kmer, res[t]->ks);
            for (u32 t = 0; t < T; ++t) res[t]->has_ks = st == GASM_OK;
        }
        bool lev_done = false;
        // GPU or host?  One wave walks a path's bands column by column (~0.25 us per column and band, whatever the number
        // of paths up to a few thousand), the host routine costs ~1.5 ns per 64 cells and runs 32 paths at a time: a
        // handful of contigs is quicker on the host, thousands of scaffolds 10-60x quicker on the GPU.
        bool lev_gpu = !getenv("GASM_LEV_HOST");
        if (lev_gpu && !getenv("GASM_LEV_GPU") && (flags & GASM_WANT_LEV)) {
            u64 max_bands = 0;
            double cells = 0;
            for (u64 p = 0; p < n_paths; ++p) {
                const u64 nq = dp.h_p_off[p + 1] - dp.h_p_off[p];
                max_bands = std::max<u64>(max_bands, (nq + 4095) / 4096);
                cells += (double)nq * (double)true_len;
            }
            // measured (k_levenshtein, round 2): 0.24 us per column and band for a wave alone on its SIMD, 0.58 us with four waves per
            // SIMD; k_levenshtein2 needs 0.6 of its instructions
            const double per_simd = (double)n_paths / 1024.0;
            const double share = std::max(1.0, 0.6 * std::min(per_simd, 4.0)), rounds = std::max(1.0, per_simd / 4.0);
            const double gpu_ms = 0.05 + (double)max_bands * (double)(true_len + 63) * 0.00015 * share * rounds;
            const double host_ms = cells / 64.0 * 1.5e-6 / (double)std::max<u64>(1, std::min<u64>(32, n_paths));
            lev_gpu = gpu_ms < host_ms;
        }
        if (st == GASM_OK && (flags & GASM_WANT_LEV) && lev_gpu) {
            // lib/DeNovoAssembler.cpp:463 (global) / lib/BreakageScorer.cpp:339 (infix): one wave per path on the GPU
            st = pipeline_levenshtein(ctx, dp, true_solution, true_len, velvet, s->lev, &lev_done);
            if (lev_done) s->lev_device = 1;
        }
        if (st == GASM_OK && (flags & GASM_WANT_LEV) && !lev_done) {
            // target with bytes outside ACGT (or GASM_LEV_HOST set): the host routine, threads over paths
            s->lev_device = 2;
            std::atomic<u64> next(0);
            unsigned nt = std::thread::hardware_concurrency();
            nt = std::max(1u, std::min(nt, 32u));
            if (n_paths < 2) nt = 1;
            auto work = [&]() {
                while (true) {
                    const u64 p = next.fetch_add(1);
                    if (p >= n_paths) break;
                    const std::string q = path_text(p);
                    s->lev[p] = gasm_host::levenshtein(q.data(), q.size(), true_solution, true_len, velvet);
                }
            };
            if (nt == 1) work();
            else {
                std::vector<std::thread> th;
                for (unsigned t = 0; t < nt; ++t) th.emplace_back(work);
                for (auto& t : th) t.join();
            }
        }
        for (u32 t = 1; t < T; ++t) { res[t]->lev = s->lev; res[t]->lev_device = s->lev_device; res[t]->startpos = s->startpos; }
    }
    rd.release(); ss.release();
    for (ScoreTable& x : tb) x.release();
    if (st != GASM_OK) { for (gasm_scores* r : res) delete r; return st; }
    for (u32 t = 0; t < T; ++t) out[t] = res[t];
    return GASM_OK;
}

// gasm_calc_breakscore (one table) and gasm_calc_breakscore_tables
static int breakscore_strings(const char* who, gasm_ctx* ctx, const char* paths, const uint64_t* path_off, uint64_t n_paths, const char* reads,
                              const uint64_t* read_off, uint64_t n_reads, const char* true_solution, uint64_t true_len, int kmer,
                              const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table, const double* bp_probs, uint32_t n_tables,
                              int variant, int flags, gasm_scores** out) {
    if (!tables_out_clear(who, out, n_tables)) return GASM_ERR_INVALID;
    if (!ctx || !out || !path_off || !read_off || !bp_off || (n_table && (!bp_kmer || !bp_probs)) || (true_len && !true_solution)) {
        gasm_set_error("%s: null argument", who);
        return GASM_ERR_INVALID;
    }
    if (variant != GASM_SCORE_OWN && variant != GASM_SCORE_VELVET) { gasm_set_error("unknown variant %d", variant); return GASM_ERR_INVALID; }
    if (n_paths > 0xFFFFFFF0ull) { gasm_set_error("too many paths"); return GASM_ERR_CAPACITY; }
    static const char empty = 0;
    DevPaths dp;
    int st = dp.upload_ascii(ctx, paths ? paths : &empty, path_off, (u32)n_paths);
    if (st == GASM_OK)
        st = breakscore_impl(ctx, dp, [&](u64 p) { return std::string(paths + path_off[p], paths + path_off[p + 1]); }, n_paths, reads, read_off, n_reads,
                             true_solution, true_len, kmer, bp_kmer, bp_off, n_table, bp_probs, n_tables, variant, flags, out);
    dp.release();
    return st;
}

int gasm_calc_breakscore(gasm_ctx* ctx, const char* paths, const uint64_t* path_off, uint64_t n_paths, const char* reads,
                         const uint64_t* read_off, uint64_t n_reads, const char* true_solution, uint64_t true_len, int kmer,
                         const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table, const double* bp_prob, int variant,
                         int flags, gasm_scores** out) {
    API_GUARD_BEGIN
    return breakscore_strings("gasm_calc_breakscore", ctx, paths, path_off, n_paths, reads, read_off, n_reads, true_solution, true_len, kmer, bp_kmer, bp_off,
                              n_table, bp_prob, 1, variant, flags, out);
    API_GUARD_END
}

int gasm_calc_breakscore_tables(gasm_ctx* ctx, const char* paths, const uint64_t* path_off, uint64_t n_paths, const char* reads,
                                const uint64_t* read_off, uint64_t n_reads, const char* true_solution, uint64_t true_len, int kmer,
                                const char* bp_kmer, const uint64_t* bp_off, uint64_t n_table, const double* bp_probs, uint32_t n_tables,
                                int variant, int flags, gasm_scores** out) {
    API_GUARD_BEGIN
    return breakscore_strings("gasm_calc_breakscore_tables", ctx, paths, path_off, n_paths, reads, read_off, n_reads, true_solution, true_len, kmer, bp_kmer,
                              bp_off, n_table, bp_probs, n_tables, variant, flags, out);
    API_GUARD_END
}

uint64_t gasm_scores_count(const gasm_scores* s) { return s ? s->n : 0; }
const int32_t* gasm_scores_sequence_len(const gasm_scores* s) { return s ? s->len.data() : nullptr; }
const double* gasm_scores_bp_score(const gasm_scores* s) { return s ? s->bp.data() : nullptr; }
const double* gasm_scores_norm_by_break_freqs(const gasm_scores* s) { return s ? s->nf.data() : nullptr; }
const double* gasm_scores_norm_by_len(const gasm_scores* s) { return s ? s->nl.data() : nullptr; }
const int32_t* gasm_scores_kmer_breaks(const gasm_scores* s) { return s ? s->breaks.data() : nullptr; }
const int32_t* gasm_scores_lev_dist(const gasm_scores* s) { return s ? s->lev.data() : nullptr; }
const double* gasm_scores_path_freq(const gasm_scores* s) { return s && s->has_freq && s->freq ? s->freq->data() : nullptr; }
const int32_t* gasm_scores_startpos(const gasm_scores* s) { return s && s->velvet ? s->startpos.data() : nullptr; }
const double* gasm_scores_prob_dist(const gasm_scores* s) { return s && s->velvet ? s->pd.data() : nullptr; }
const uint64_t* gasm_scores_prob_dist_offsets(const gasm_scores* s) { return s && s->velvet ? s->pd_off.data() : nullptr; }
const double* gasm_scores_ks(const gasm_scores* s) { return s && s->has_ks ? s->ks.data() : nullptr; }
int gasm_scores_lev_device(const gasm_scores* s) { return s ? s->lev_device : 0; }

int gasm_coverage_percent(gasm_ctx* ctx, const int64_t* start, const int64_t* len, uint64_t n, int64_t seq_len, double* percent) {
    API_GUARD_BEGIN
    if (!ctx || !percent || (n && (!start || !len))) { gasm_set_error("gasm_coverage_percent: null argument"); return GASM_ERR_INVALID; }
    return pipeline_coverage(ctx, reinterpret_cast<const long long*>(start), reinterpret_cast<const long long*>(len), n, (long long)seq_len, percent);
    API_GUARD_END
}
void gasm_scores_free(gasm_scores* s) { delete s; }

// ------------------------------------------------------------------------------------------------------ batches
int gasm_batch_create(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, uint32_t fixed_len,
                      const uint64_t* seg_read_off, uint32_t n_segments, gasm_batch** out) {
    API_GUARD_BEGIN
    if (!ctx || !out) { gasm_set_error("gasm_batch_create: null argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    if (n_segments == 0 || !seg_read_off) { gasm_set_error("need at least one segment and seg_read_off"); return GASM_ERR_INVALID; }
    if (seg_read_off[0] != 0 || seg_read_off[n_segments] != n_reads) { gasm_set_error("seg_read_off must run from 0 to n_reads"); return GASM_ERR_INVALID; }
    for (u32 s = 0; s < n_segments; ++s) if (seg_read_off[s] > seg_read_off[s + 1]) { gasm_set_error("seg_read_off not monotone"); return GASM_ERR_INVALID; }
    return new_batch(ctx, n_segments, n_reads, out, [&](gasm_batch* b) { return b->rd.upload(ctx, reads, read_off, n_reads, fixed_len, seg_read_off, n_segments); });
    API_GUARD_END
}

// a batch from reads that are packed already
static int batch_from_packed(gasm_ctx* ctx, const u64* words, const u64* read_off, u64 n_reads, u32 fixed_len, const u64* seg_read_off,
                             u32 n_segments, gasm_batch** out) {
    return new_batch(ctx, n_segments, n_reads, out, [&](gasm_batch* b) { return b->rd.upload_packed(ctx, words, read_off, n_reads, fixed_len, seg_read_off, n_segments); });
}

int gasm_batch_create_packed(gasm_ctx* ctx, const uint64_t* words, const uint64_t* read_off, uint64_t n_reads, uint32_t fixed_len,
                             const uint64_t* seg_read_off, uint32_t n_segments, gasm_batch** out) {
    API_GUARD_BEGIN
    if (!ctx || !out) { gasm_set_error("gasm_batch_create_packed: null argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    return batch_from_packed(ctx, words, read_off, n_reads, fixed_len, seg_read_off, n_segments, out);
    API_GUARD_END
}

// gasm_ingest_params, checked -> the options every reader takes (the plain entries come here with their on_non_acgt alone)
static int ingest_opts_from(const gasm_ingest_params* p, const char* who, gasm_host::IngestOpts& o) {
    if (!p) { gasm_set_error("%s: params is null", who); return GASM_ERR_INVALID; }
    if (p->size != sizeof(gasm_ingest_params)) { gasm_set_error("%s: params->size is %u, not sizeof(gasm_ingest_params) = %zu", who, p->size, sizeof(gasm_ingest_params)); return GASM_ERR_INVALID; }
    if (p->on_non_acgt > 1 || p->pairs > 1 || p->quality_hist > 1) { gasm_set_error("%s: on_non_acgt, pairs and quality_hist are 0 or 1", who); return GASM_ERR_INVALID; }
    if (p->phred_offset != 0 && p->phred_offset != 33 && p->phred_offset != 64) { gasm_set_error("%s: phred_offset %u is neither 33 nor 64", who, p->phred_offset); return GASM_ERR_INVALID; }
    if (p->trim_q3 > 93 || p->trim_q5 > 93) { gasm_set_error("%s: trim_q3 and trim_q5 are at most 93", who); return GASM_ERR_INVALID; }
    o.error_on_non_acgt = p->on_non_acgt != 0;
    o.phred_offset = p->phred_offset ? p->phred_offset : 33;
    o.trim_q3 = p->trim_q3; o.trim_q5 = p->trim_q5; o.min_len = p->min_len;
    o.pairs = p->pairs != 0; o.quality_hist = p->quality_hist != 0;
    return GASM_OK;
}
static gasm_ingest_params plain_ingest_params(int on_non_acgt) {
    gasm_ingest_params p = {};
    p.size = sizeof(p);
    p.on_non_acgt = on_non_acgt != 0;
    return p;
}

static int parse_files(const char* const* paths, uint32_t n_files, const gasm_host::IngestOpts& o, gasm_packed& g) {
    g.pr.read_off.assign(1, 0);
    g.seg.assign((size_t)n_files + 1, 0);
    g.dropped = 0;
    if (o.any()) { g.stats.assign((size_t)n_files * GASM_INGEST_STATS, 0); g.hist.assign((size_t)n_files * GASM_QUAL_BINS, 0); }
    for (u32 f = 0; f < n_files; ++f) {
        if (!paths[f]) { gasm_set_error("paths[%u] is null", f); return GASM_ERR_INVALID; }
        u64 kept = 0;
        GCHK(gasm_host::read_sequence_file(paths[f], o, g.pr, &kept, &g.dropped, o.any() ? &g.stats[(size_t)f * GASM_INGEST_STATS] : nullptr,
                                           o.any() ? &g.hist[(size_t)f * GASM_QUAL_BINS] : nullptr));
        g.seg[f + 1] = g.seg[f] + kept;
    }
    return GASM_OK;
}

int gasm_read_files_params(const char* const* paths, uint32_t n_files, const gasm_ingest_params* params, gasm_packed** out) {
    API_GUARD_BEGIN
    if (!out || !paths || n_files == 0) { gasm_set_error("gasm_read_files: bad argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    gasm_host::IngestOpts o;
    GCHK(ingest_opts_from(params, "gasm_read_files_params", o));
    gasm_packed* g = new gasm_packed();
    const int st = parse_files(paths, n_files, o, *g);
    if (st != GASM_OK) { delete g; return st; }
    *out = g;
    return GASM_OK;
    API_GUARD_END
}
int gasm_read_files(const char* const* paths, uint32_t n_files, int on_non_acgt, gasm_packed** out) {
    const gasm_ingest_params p = plain_ingest_params(on_non_acgt);
    return gasm_read_files_params(paths, n_files, &p, out);
}
uint64_t gasm_packed_n_reads(const gasm_packed* g) { return g ? g->pr.read_off.size() - 1 : 0; }
uint32_t gasm_packed_n_segments(const gasm_packed* g) { return g ? (uint32_t)(g->seg.size() - 1) : 0; }
const uint64_t* gasm_packed_words(const gasm_packed* g) { return g ? g->pr.words.data() : nullptr; }
const uint64_t* gasm_packed_read_off(const gasm_packed* g) { return g ? g->pr.read_off.data() : nullptr; }
const uint64_t* gasm_packed_seg_read_off(const gasm_packed* g) { return g ? g->seg.data() : nullptr; }
uint64_t gasm_packed_dropped(const gasm_packed* g) { return g ? g->dropped : 0; }
const uint64_t* gasm_packed_ingest_stats(const gasm_packed* g) { return g && !g->stats.empty() ? g->stats.data() : nullptr; }
const uint64_t* gasm_packed_quality_hist(const gasm_packed* g) { return g && !g->hist.empty() ? g->hist.data() : nullptr; }
void gasm_packed_free(gasm_packed* g) { delete g; }

// the same files through the device path (ingest.hip: record scan + 2-bit pack on the GPU, the host only inflates), results
// copied back: what gasm_batch_from_files builds its batch from without the copy
int gasm_read_files_device_params(gasm_ctx* ctx, const char* const* paths, uint32_t n_files, const gasm_ingest_params* params, gasm_packed** out) {
    API_GUARD_BEGIN
    if (!ctx || !out || !paths || n_files == 0) { gasm_set_error("gasm_read_files_device: bad argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    gasm_host::IngestOpts o;
    GCHK(ingest_opts_from(params, "gasm_read_files_device_params", o));
    gasm_packed* g = new gasm_packed();
    DBuf d_words;
    struct Rel { DBuf& b; ~Rel() { b.release(); } } rel{d_words};
    const int st = ingest_files_device(ctx, paths, n_files, o, d_words, g->pr.read_off, g->seg, &g->dropped, g->on_device, g->stats, g->hist);
    if (st != GASM_OK) { delete g; return st; }
    g->pr.total_bases = g->pr.read_off.back();
    const u64 nw = (g->pr.total_bases + 31) / 32;
    g->pr.words.resize(nw);
    if (nw && hipMemcpy(g->pr.words.data(), d_words.p, nw * 8, hipMemcpyDeviceToHost) != hipSuccess) { delete g; gasm_set_error("copy of the packed reads failed"); return GASM_ERR_HIP; }
    *out = g;
    return GASM_OK;
    API_GUARD_END
}
int gasm_read_files_device(gasm_ctx* ctx, const char* const* paths, uint32_t n_files, int on_non_acgt, gasm_packed** out) {
    const gasm_ingest_params p = plain_ingest_params(on_non_acgt);
    return gasm_read_files_device_params(ctx, paths, n_files, &p, out);
}
int gasm_packed_parsed_on_device(const gasm_packed* g, uint32_t file) { return g && file < g->on_device.size() ? g->on_device[file] : 0; }

int gasm_batch_from_files_params(gasm_ctx* ctx, const char* const* paths, uint32_t n_files, const gasm_ingest_params* params, gasm_batch** out,
                                 uint64_t* dropped_reads) {
    API_GUARD_BEGIN
    if (!ctx || !out || !paths || n_files == 0) { gasm_set_error("gasm_batch_from_files: bad argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    gasm_host::IngestOpts o;
    GCHK(ingest_opts_from(params, "gasm_batch_from_files_params", o));
    // record scan and 2-bit packing on the device (ingest.hip); the packed stream never leaves it
    DBuf d_words;
    struct Rel { DBuf& b; ~Rel() { b.release(); } } rel{d_words};
    std::vector<u64> read_off, seg, stats, hist;
    std::vector<u8> on_device;
    u64 dropped = 0;
    GCHK(ingest_files_device(ctx, paths, n_files, o, d_words, read_off, seg, &dropped, on_device, stats, hist));
    if (dropped_reads) *dropped_reads = dropped;
    const u64 n = read_off.size() - 1;
    // fixed-length reads (the usual case) need no offset array on the device
    u32 flen = n ? (u32)std::min<u64>(read_off[1], 0xFFFFFFFFull) : 0;
    bool fixed = n > 0 && flen > 0;
    for (u64 r = 0; fixed && r < n; ++r) fixed = read_off[r + 1] - read_off[r] == flen;
    return new_batch(ctx, n_files, n, out, [&](gasm_batch* b) {
        b->h_ingest_stats = std::move(stats);
        b->h_ingest_hist = std::move(hist);
        return b->rd.adopt_packed(ctx, d_words, fixed ? nullptr : read_off.data(), n, fixed ? flen : 0, seg.data(), n_files);
    });
    API_GUARD_END
}
int gasm_batch_from_files(gasm_ctx* ctx, const char* const* paths, uint32_t n_files, int on_non_acgt, gasm_batch** out, uint64_t* dropped_reads) {
    const gasm_ingest_params p = plain_ingest_params(on_non_acgt);
    return gasm_batch_from_files_params(ctx, paths, n_files, &p, out, dropped_reads);
}
int gasm_batch_fetch_ingest_stats(gasm_batch* b, const uint64_t** stats, const uint64_t** quality_hist) {
    API_GUARD_BEGIN
    if (!b || !stats || !quality_hist) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (b->h_ingest_stats.empty()) { gasm_set_error("not a batch made from files under ingest options: no statistics were collected"); return GASM_ERR_STATE; }
    *stats = b->h_ingest_stats.data();
    *quality_hist = b->h_ingest_hist.data();
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_simulate(gasm_ctx* ctx, const char* genomes, const uint64_t* genome_off, uint32_t n_segments, uint32_t read_len, double coverage,
                        uint64_t seed, int kmer, const double* table, gasm_batch** out) {
    API_GUARD_BEGIN
    if (!ctx || !out || !genomes || !genome_off) { gasm_set_error("gasm_batch_simulate: null argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    return new_batch(ctx, n_segments, 0, out, [&](gasm_batch* b) {
        GCHK(b->rd.simulate(ctx, genomes, genome_off, n_segments, read_len, coverage, seed, kmer, table, b->d_read_start));
        b->n_reads = b->rd.n_reads;
        b->h_sim_seg_off = b->rd.h_seg_read_off;
        return (int)GASM_OK;
    });
    API_GUARD_END
}

int gasm_batch_fetch_read_starts(gasm_batch* b, const uint64_t** seg_read_off, const uint32_t** starts) {
    API_GUARD_BEGIN
    if (!b || !seg_read_off || !starts) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (b->h_sim_seg_off.empty()) { gasm_set_error("not a simulated batch"); return GASM_ERR_STATE; }
    b->h_read_start.resize(b->n_reads);
    HIPCHK(hipSetDevice(b->ctx->device));
    if (b->n_reads) HIPCHK(hipMemcpyAsync(b->h_read_start.data(), b->d_read_start.p, b->n_reads * 4, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    *seg_read_off = b->h_sim_seg_off.data();
    *starts = b->h_read_start.data();
    return GASM_OK;
    API_GUARD_END
}

void gasm_batch_free(gasm_batch* b) {
    if (!b) return;
    b->d_read_start.release();
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    for (StepSlot& x : b->slot) { if (x.cx && x.cx != b->ctx) (void)hipStreamSynchronize(x.cx->stream); x.bs.release(); x.dp.release(); x.ss.release(); }
    b->rd.release(); b->rd2.release(); b->guided.release(); b->d_rkc.release(); b->d_correct.release();
    for (ScoreTable& t : b->tb) t.release();
    for (ScoreTable& t : b->mtb) t.release();
    delete b;
}

// every gasm_batch_build* entry, with the options it filled `o` from
static int batch_build(gasm_batch* b, const BuildOpts& o) {
    if (!b) { gasm_set_error("batch is null"); return GASM_ERR_INVALID; }
    GCHK(build_opts_check(o));                // (everything is refused here: nothing below is undone, and the build before stays fetchable)
    b->built = false; b->scored = false;
    // consecutive steps take the slots in turn: this build does not wait for the last steps' graph and scoring, it runs
    // beside them.  A change of k rewrites the tile tables every slot reads: everything drains first.  GASM_PINGPONG=0: the
    // build stays on the slot the last build took, behind whatever that slot still has queued.
    const bool pingpong = env_int("GASM_PINGPONG", 1) != 0;
    if (pingpong && b->slot[0].cx == nullptr && b->slot[1].cx == nullptr)       // (fixed with the first build)
        b->n_slots = std::max(2, std::min(4, env_int("GASM_STEP_SLOTS", 3)));
    if (pingpong) {
        if (b->last_k && b->last_k != o.k) for (StepSlot& x : b->slot) if (x.cx) HIPCHK(hipStreamSynchronize(x.cx->stream));
        b->cur = (b->cur + 1) % b->n_slots;
    }
    StepSlot& st = b->S();
    st.paths_ready = false; st.ss.valid = false; st.ss.launched = false;
    // both strands: the reverse-complemented stream is made once per upload (on this slot's stream, complete before the call
    // returns: the other slots read it without waiting for this one)
    if (o.strands == 2 && b->rd2.strands_of != b->rd.upload_id) GCHK(b->rd2.make_both_strands(st.cx, b->rd));
    // (the slot's BuildState keeps the options of the build it holds)
    GCHK(pipeline_build(st.cx, o.strands == 2 ? b->rd2 : b->rd, st.bs, o));
    b->last_k = o.k;
    b->built = true;
    return GASM_OK;
}

int gasm_batch_build(gasm_batch* b, int k, uint64_t genome_len_hint) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = k; o.genome_len_hint = genome_len_hint;
    return batch_build(b, o);
    API_GUARD_END
}

int gasm_batch_build_solid(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = k; o.genome_len_hint = genome_len_hint; o.min_count = min_count;
    return batch_build(b, o);
    API_GUARD_END
}

int gasm_batch_build_strands(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count, uint32_t strands) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = k; o.genome_len_hint = genome_len_hint; o.min_count = min_count; o.strands = strands;
    return batch_build(b, o);
    API_GUARD_END
}

int gasm_batch_build_tips(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count, uint32_t strands, uint32_t tip_len, uint32_t tip_rounds) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = k; o.genome_len_hint = genome_len_hint; o.min_count = min_count; o.strands = strands; o.tip_len = tip_len; o.tip_rounds = tip_rounds;
    return batch_build(b, o);
    API_GUARD_END
}

int gasm_batch_build_bubbles(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count, uint32_t strands, uint32_t tip_len, uint32_t tip_rounds,
                             uint32_t bubble_len, uint32_t bubble_rounds) {
    API_GUARD_BEGIN
    BuildOpts o;
    o.k = k; o.genome_len_hint = genome_len_hint; o.min_count = min_count; o.strands = strands; o.tip_len = tip_len; o.tip_rounds = tip_rounds;
    o.bubble_len = bubble_len; o.bubble_rounds = bubble_rounds;
    return batch_build(b, o);
    API_GUARD_END
}

int gasm_batch_build_params(gasm_batch* b, const gasm_build_params* params) {
    API_GUARD_BEGIN
    BuildOpts o;
    GCHK(opts_from_params("gasm_batch_build_params", params, o));
    return batch_build(b, o);
    API_GUARD_END
}

// the options of the last build as its slot keeps them (normalised); 0 before the first
uint32_t gasm_batch_strands(const gasm_batch* b) { return b && b->built ? b->S().bs.opts.strands : 0; }
uint32_t gasm_batch_tip_len(const gasm_batch* b) { return b && b->built ? b->S().bs.opts.tip_len : 0; }
uint32_t gasm_batch_tip_rounds(const gasm_batch* b) { return b && b->built ? b->S().bs.opts.tip_rounds : 0; }
uint32_t gasm_batch_bubble_len(const gasm_batch* b) { return b && b->built ? b->S().bs.opts.bubble_len : 0; }
uint32_t gasm_batch_bubble_rounds(const gasm_batch* b) { return b && b->built ? b->S().bs.opts.bubble_rounds : 0; }
uint32_t gasm_batch_cov_cutoff(const gasm_batch* b) { return b && b->built ? b->S().bs.opts.cov_cutoff : 0; }
uint32_t gasm_batch_cov_len(const gasm_batch* b) { return b && b->built ? b->S().bs.opts.cov_len : 0; }
uint32_t gasm_batch_cov_rounds(const gasm_batch* b) { return b && b->built ? b->S().bs.opts.cov_rounds : 0; }

// gasm_batch_fetch_tip_stats, _bubble_stats and _lowcov_stats: what the last build's rounds of `kind` removed
static int batch_fetch_round_stats(gasm_batch* b, u32 kind, const uint32_t** contigs, const uint32_t** kmers) {
    static const char* const entry[ROUND_KINDS] = {"gasm_batch_fetch_tip_stats", "gasm_batch_fetch_bubble_stats", "gasm_batch_fetch_lowcov_stats"};
    static const char* const off[ROUND_KINDS] = {"the last build clipped no tips (tip_len = 0)", "the last build popped no bubbles (bubble_len = 0)",
                                                 "the last build removed no low-coverage contigs (cov_cutoff = 0 or cov_len = 0)"};
    if (!b || !contigs || !kmers) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (!b->built) { gasm_set_error("%s before a build", entry[kind]); return GASM_ERR_STATE; }
    if (!b->S().bs.opts.rounds(kind)) { gasm_set_error("%s", off[kind]); return GASM_ERR_STATE; }
    GCHK(batch_finish(b));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_round_stats(b->S().cx, b->build_reads(b->S()), bs, kind));
    *contigs = bs.round_stats[kind].h_contigs.data(); *kmers = bs.round_stats[kind].h_kmers.data();
    return GASM_OK;
}

int gasm_batch_fetch_tip_stats(gasm_batch* b, const uint32_t** tips, const uint32_t** kmers) {
    API_GUARD_BEGIN
    return batch_fetch_round_stats(b, ROUNDS_TIP, tips, kmers);
    API_GUARD_END
}

int gasm_batch_fetch_bubble_stats(gasm_batch* b, const uint32_t** bubbles, const uint32_t** kmers) {
    API_GUARD_BEGIN
    return batch_fetch_round_stats(b, ROUNDS_BUBBLE, bubbles, kmers);
    API_GUARD_END
}

int gasm_batch_fetch_lowcov_stats(gasm_batch* b, const uint32_t** contigs, const uint32_t** kmers) {
    API_GUARD_BEGIN
    return batch_fetch_round_stats(b, ROUNDS_LOWCOV, contigs, kmers);
    API_GUARD_END
}

// ---- the passes over the last build.  A queueing entry: batch non-null, its own arguments in range (`args`: what its check gave, the
// error already set), built, the pending build finished.  A fetching entry: no null argument, built
static int batch_pass_ready(gasm_batch* b, const char* entry, int args = GASM_OK) {
    if (!b) { gasm_set_error("batch is null"); return GASM_ERR_INVALID; }
    if (args != GASM_OK) return args;
    if (!b->built) { gasm_set_error("%s before a build", entry); return GASM_ERR_STATE; }
    return batch_finish(b);
}
static int batch_fetch_ready(const gasm_batch* b, const char* entry, bool no_null) {
    if (!b || !no_null) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (!b->built) { gasm_set_error("%s before a build", entry); return GASM_ERR_STATE; }
    return GASM_OK;
}
static int at_most(const char* name, u32 v, u32 max) {
    if (v > max) { gasm_set_error("%s must be <= %u (got %u)", name, max, v); return GASM_ERR_INVALID; }
    return GASM_OK;
}

int gasm_batch_contig_coverage(gasm_batch* b) {
    API_GUARD_BEGIN
    GCHK(batch_pass_ready(b, "gasm_batch_contig_coverage"));
    return pipeline_contig_coverage(b->S().cx, b->build_reads(b->S()), b->S().bs);
    API_GUARD_END
}

int gasm_batch_fetch_contig_coverage(gasm_batch* b, const uint64_t** mult_sum, const uint32_t** n_edges) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_contig_coverage", mult_sum && n_edges));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_contig_coverage(b->S().cx, b->build_reads(b->S()), bs));
    *mult_sum = bs.h_ccov_m.data(); *n_edges = bs.h_ccov_n.data();
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_contig_links(gasm_batch* b, uint32_t span_len) {
    API_GUARD_BEGIN
    GCHK(batch_pass_ready(b, "gasm_batch_contig_links", at_most("span_len", span_len, GASM_MAX_SPAN_LEN)));
    return pipeline_contig_links(b->S().cx, b->build_reads(b->S()), b->S().bs, span_len);
    API_GUARD_END
}

int gasm_batch_fetch_contig_links(gasm_batch* b, const uint32_t** succ, const uint32_t** pred, const uint32_t** link_support, const uint32_t** span_support,
                                  const uint64_t** skipped) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_contig_links", succ && pred && link_support && span_support && skipped));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_contig_links(b->S().cx, b->build_reads(b->S()), bs));
    *succ = bs.links.host<uint32_t>(LINKS_SUCC); *pred = bs.links.host<uint32_t>(LINKS_PRED); *link_support = bs.links.host<uint32_t>(LINKS_LSUP);
    *span_support = bs.links.host<uint32_t>(LINKS_SSUP); *skipped = bs.links.host<uint64_t>(LINKS_SKIPPED);
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_place_pairs(gasm_batch* b, uint32_t max_insert) {
    API_GUARD_BEGIN
    int args = GASM_OK;
    if (max_insert < 1 || max_insert > GASM_MAX_INSERT) { gasm_set_error("max_insert must be 1..%d (got %u)", GASM_MAX_INSERT, max_insert); args = GASM_ERR_INVALID; }
    GCHK(batch_pass_ready(b, "gasm_batch_place_pairs", args));
    return pipeline_place_pairs(b->S().cx, b->build_reads(b->S()), b->rd, b->S().bs, max_insert);
    API_GUARD_END
}

int gasm_batch_fetch_pair_places(gasm_batch* b, const int32_t** rec, const uint32_t** insert_hist, const uint64_t** counters, uint32_t* orientations) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_pair_places", rec && insert_hist && counters && orientations));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_pair_places(b->S().cx, b->rd, bs));
    *rec = bs.pairs.host<int32_t>(PAIRS_REC); *insert_hist = bs.pairs.host<uint32_t>(PAIRS_HIST); *counters = bs.pairs.host<uint64_t>(PAIRS_CNT);
    *orientations = bs.pairs.param[0];
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_map_reads(gasm_batch* b, uint32_t max_mismatch) {
    API_GUARD_BEGIN
    GCHK(batch_pass_ready(b, "gasm_batch_map_reads", at_most("max_mismatch", max_mismatch, GASM_MAP_MAX_MISMATCH)));
    return pipeline_map_reads(b->S().cx, b->build_reads(b->S()), b->rd, b->S().bs, false, max_mismatch, 0);
    API_GUARD_END
}

int gasm_batch_fetch_read_map(gasm_batch* b, const int32_t** rec, const uint32_t** pile, const uint32_t** mismatch_hist, const uint64_t** counters) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_read_map", rec && pile && mismatch_hist && counters));
    const PassState& ps = b->S().bs.map;
    GCHK(pipeline_fetch_read_map(b->S().cx, b->rd, b->S().bs, false));
    *rec = ps.host<int32_t>(MAP_REC); *pile = ps.host<uint32_t>(MAP_PILE); *mismatch_hist = ps.host<uint32_t>(MAP_HIST); *counters = ps.host<uint64_t>(MAP_CNT);
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_map_reads_gapped(gasm_batch* b, uint32_t max_edits, uint32_t max_gap) {
    API_GUARD_BEGIN
    int args = at_most("max_edits", max_edits, GASM_MAP_MAX_MISMATCH);
    if (args == GASM_OK) args = at_most("max_gap", max_gap, GASM_MAP_MAX_GAP);
    GCHK(batch_pass_ready(b, "gasm_batch_map_reads_gapped", args));
    return pipeline_map_reads(b->S().cx, b->build_reads(b->S()), b->rd, b->S().bs, true, max_edits, max_gap);
    API_GUARD_END
}

int gasm_batch_fetch_read_map_gapped(gasm_batch* b, const int32_t** rec, const int32_t** rec_gap, const uint32_t** pile, const uint32_t** gap_pile,
                                     const uint32_t** edit_hist, const uint64_t** counters) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_read_map_gapped", rec && rec_gap && pile && gap_pile && edit_hist && counters));
    const PassState& ps = b->S().bs.mapg;
    GCHK(pipeline_fetch_read_map(b->S().cx, b->rd, b->S().bs, true));
    *rec = ps.host<int32_t>(MAPG_REC); *rec_gap = ps.host<int32_t>(MAPG_GAP); *pile = ps.host<uint32_t>(MAPG_PILE); *gap_pile = ps.host<uint32_t>(MAPG_GPILE);
    *edit_hist = ps.host<uint32_t>(MAPG_HIST); *counters = ps.host<uint64_t>(MAPG_CNT);
    return GASM_OK;
    API_GUARD_END
}

// ---- end gaps (kernels_map.hip, k_read_map_ends; the rule: include/gasm.h "End gaps"): the gapped mapping's own state, two more tables
int gasm_batch_map_reads_gapped_ends(gasm_batch* b, uint32_t max_edits, uint32_t max_gap, uint32_t end_gap) {
    API_GUARD_BEGIN
    int args = at_most("max_edits", max_edits, GASM_MAP_MAX_MISMATCH);
    if (args == GASM_OK) args = at_most("max_gap", max_gap, GASM_MAP_MAX_GAP);
    if (args == GASM_OK) args = at_most("end_gap", end_gap, GASM_MAP_MAX_GAP);
    GCHK(batch_pass_ready(b, "gasm_batch_map_reads_gapped_ends", args));
    return pipeline_map_reads(b->S().cx, b->build_reads(b->S()), b->rd, b->S().bs, true, max_edits, max_gap, end_gap);
    API_GUARD_END
}

int gasm_batch_fetch_read_map_ends(gasm_batch* b, const int32_t** rec_end, const uint64_t** end_counters) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_read_map_ends", rec_end && end_counters));
    const PassState& ps = b->S().bs.mapg;
    if (ps.queued && !(ps.param[1] & MAPG_HAS_ENDS)) {
        gasm_set_error("gasm_batch_fetch_read_map_ends: the last gapped mapping over the last build tried no end gaps (gasm_batch_map_reads_gapped_ends with end_gap > 0 does)");
        return GASM_ERR_STATE;
    }
    GCHK(pipeline_fetch_read_map(b->S().cx, b->rd, b->S().bs, true));
    *rec_end = ps.host<int32_t>(MAPG_END); *end_counters = ps.host<uint64_t>(MAPG_ENDCNT);
    return GASM_OK;
    API_GUARD_END
}

// ---- alignments (kernels_map.hip, k_read_map_trace; include/gasm.h "Alignments"): the gapped mapping's own state with the end tables (zero
// for end_gap = 0) and two more tables behind them
int gasm_batch_map_reads_aligned(gasm_batch* b, uint32_t max_edits, uint32_t max_gap, uint32_t end_gap) {
    API_GUARD_BEGIN
    int args = at_most("max_edits", max_edits, GASM_MAP_MAX_MISMATCH);
    if (args == GASM_OK) args = at_most("max_gap", max_gap, GASM_MAP_MAX_GAP);
    if (args == GASM_OK) args = at_most("end_gap", end_gap, GASM_MAP_MAX_GAP);
    GCHK(batch_pass_ready(b, "gasm_batch_map_reads_aligned", args));
    return pipeline_map_reads(b->S().cx, b->build_reads(b->S()), b->rd, b->S().bs, true, max_edits, max_gap, end_gap, true);
    API_GUARD_END
}

int gasm_batch_fetch_read_alignments(gasm_batch* b, const int32_t** rec_piece, const uint32_t** ins_pile, uint32_t* ins_cols) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_read_alignments", rec_piece && ins_pile && ins_cols));
    const PassState& ps = b->S().bs.mapg;
    if (ps.queued && !(ps.param[1] & MAPG_HAS_TRACE)) {
        gasm_set_error("gasm_batch_fetch_read_alignments: the last gapped mapping over the last build kept no alignments (gasm_batch_map_reads_aligned does)");
        return GASM_ERR_STATE;
    }
    GCHK(pipeline_fetch_read_map(b->S().cx, b->rd, b->S().bs, true));
    *rec_piece = ps.host<int32_t>(MAPG_PIECE); *ins_pile = ps.host<uint32_t>(MAPG_INS); *ins_cols = ps.param[1] >> MAPG_COLS_SHIFT;
    return GASM_OK;
    API_GUARD_END
}

// ---- mapped scoring (kernels_score.hip, k_score_mapped; the rule: include/gasm.h "Mapped scoring")
int gasm_batch_score_mapped(gasm_batch* b, int source, int kmer, const double* tables, uint32_t n_tables, uint32_t flags) {
    API_GUARD_BEGIN
    int args = GASM_OK;
    if (b && !tables) { gasm_set_error("gasm_batch_score_mapped: null argument"); args = GASM_ERR_INVALID; }
    else if (source != GASM_MAPSCORE_UNGAPPED && source != GASM_MAPSCORE_GAPPED) { gasm_set_error("source must be GASM_MAPSCORE_UNGAPPED or GASM_MAPSCORE_GAPPED (got %d)", source); args = GASM_ERR_INVALID; }
    else if (flags & ~(uint32_t)GASM_MAPSCORE_PARTIAL) { gasm_set_error("unknown flag bits 0x%x", flags & ~(uint32_t)GASM_MAPSCORE_PARTIAL); args = GASM_ERR_INVALID; }
    else if (n_tables < 1 || n_tables > GASM_MAX_TABLES) { gasm_set_error("n_tables must be 1..%d (got %u)", GASM_MAX_TABLES, n_tables); args = GASM_ERR_INVALID; }
    else if (kmer < 0) { gasm_set_error("kmer must be >= 0"); args = GASM_ERR_INVALID; }
    GCHK(batch_pass_ready(b, "gasm_batch_score_mapped", args));
    StepSlot& x = b->S();
    const bool gapped = source == GASM_MAPSCORE_GAPPED;
    if (b->rd.positioned) { gasm_set_error("mapped scoring needs the reads back to back (pooled builds place them by position)"); return GASM_ERR_STATE; }
    if (!(gapped ? x.bs.mapg : x.bs.map).queued) {
        gasm_set_error("gasm_batch_score_mapped before %s (of the last build)", gapped ? "gasm_batch_map_reads_gapped" : "gasm_batch_map_reads");
        return GASM_ERR_STATE;
    }
    // No FP64 fallback: every table must have a fixed-point shift for these reads, checked before anything is set or queued
    u64 max_reads = 0;
    for (u32 s = 0; s < b->rd.n_segments; ++s) max_reads = std::max(max_reads, b->rd.h_seg_read_off[s + 1] - b->rd.h_seg_read_off[s]);
    for (u32 t = 0; t < n_tables; ++t) {
        double absmax = 0;
        const bool finite = gasm_host::table_range(tables + (size_t)t * GASM_TABLE_ROWS, GASM_TABLE_ROWS, &absmax);
        const int shift = gasm_host::fixed_point_shift(absmax, finite, max_reads);
        if (shift < 0 || shift > 1000) { gasm_set_error("gasm_batch_score_mapped: table %u has no fixed-point shift (a NaN or infinite entry, or a range the 64-bit fixed point cannot hold)", t); return GASM_ERR_INVALID; }
    }
    ScoreTable* tbs[GASM_MAX_TABLES];
    bool same[GASM_MAX_TABLES], all_same = true;
    for (u32 t = 0; t < GASM_MAX_TABLES; ++t) tbs[t] = &b->mtb[t];
    for (u32 t = 0; t < n_tables; ++t) {
        const std::vector<double>& have = b->mtable_copy[t];
        same[t] = !have.empty() && memcmp(have.data(), tables + (size_t)t * GASM_TABLE_ROWS, GASM_TABLE_ROWS * sizeof(double)) == 0;
        all_same = all_same && same[t];
    }
    if (!all_same) {
        for (StepSlot& y : b->slot) if (y.cx) HIPCHK(hipStreamSynchronize(y.cx->stream));      // (whatever still scores with the old tables)
        for (u32 t = 0; t < n_tables; ++t) {
            if (same[t]) continue;
            const double* src = tables + (size_t)t * GASM_TABLE_ROWS;
            GCHK(tbs[t]->set_standard(b->ctx, src));
            b->mtable_copy[t].assign(src, src + GASM_TABLE_ROWS);
        }
    }
    return pipeline_score_mapped(x.cx, b->build_reads(x), b->rd, x.bs, gapped, kmer, tbs, n_tables, (flags & GASM_MAPSCORE_PARTIAL) != 0);
    API_GUARD_END
}

int gasm_batch_fetch_mapped_scores(gasm_batch* b, uint32_t t, const double** bp_score, const double** norm_by_break_freqs, const double** norm_by_len,
                                   const int32_t** kmer_breaks, const int32_t** sequence_len, const int64_t** fx, int* shift) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_mapped_scores", bp_score && norm_by_break_freqs && norm_by_len && kmer_breaks && sequence_len && fx && shift));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_mapped_scores(b->S().cx, b->rd, bs));
    const u32 T = bs.mapscore.param[0];
    if (t >= T) { gasm_set_error("table %u of a mapped score with %u table(s)", t, T); return GASM_ERR_INVALID; }
    const size_t P = bs.n_contigs;
    const double* f = bs.mapscore.host<double>(MAPSC_F64) + (size_t)t * 3 * P;
    *bp_score = f; *norm_by_break_freqs = f + P; *norm_by_len = f + 2 * P;
    *kmer_breaks = bs.mapscore.host<int32_t>(MAPSC_I32); *sequence_len = bs.mapscore.host<int32_t>(MAPSC_I32) + P;
    *fx = bs.mapscore.host<int64_t>(MAPSC_FX) + (size_t)t * P;
    *shift = bs.mapscore_shift[t];
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_fetch_mapped_starts(gasm_batch* b, const uint32_t** start_pile, const uint64_t** counters) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_mapped_starts", start_pile && counters));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_mapped_scores(b->S().cx, b->rd, bs));
    *start_pile = bs.mapscore.host<uint32_t>(MAPSC_PILE); *counters = bs.mapscore.host<uint64_t>(MAPSC_COUNTERS);
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_fetch_contig_twins(gasm_batch* b, const uint32_t** twin) {
    API_GUARD_BEGIN
    if (!b || !twin) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (!b->built) { gasm_set_error("gasm_batch_fetch_contig_twins before a build"); return GASM_ERR_STATE; }
    GCHK(batch_finish(b));
    StepSlot& x = b->S();
    GCHK(pipeline_fetch_contig_twins(x.cx, b->build_reads(x), x.bs));
    *twin = x.bs.h_twin.data();
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_fetch_solid_stats(gasm_batch* b, const uint64_t** distinct_before, const uint64_t** distinct_after) {
    API_GUARD_BEGIN
    if (!b || !distinct_before || !distinct_after) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (!b->built) { gasm_set_error("gasm_batch_fetch_solid_stats before a build"); return GASM_ERR_STATE; }
    GCHK(batch_finish(b));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_solid_stats(b->S().cx, b->build_reads(b->S()), bs));
    *distinct_before = bs.h_solid_before.data(); *distinct_after = bs.h_solid_after.data();
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_kmer_spectrum(gasm_batch* b) {
    API_GUARD_BEGIN
    GCHK(batch_pass_ready(b, "gasm_batch_kmer_spectrum"));
    return pipeline_kmer_spectrum(b->S().cx, b->build_reads(b->S()), b->S().bs);
    API_GUARD_END
}

int gasm_batch_fetch_kmer_spectrum(gasm_batch* b, const uint64_t** hist) {
    API_GUARD_BEGIN
    GCHK(batch_fetch_ready(b, "gasm_batch_fetch_kmer_spectrum", hist != nullptr));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_kmer_spectrum(b->S().cx, b->build_reads(b->S()), bs));
    *hist = bs.h_spectrum.data();
    return GASM_OK;
    API_GUARD_END
}

// gasm_batch_score (n_tables = 1) and gasm_batch_score_tables: the step's scoring under n_tables tables over one match
static int batch_score(gasm_batch* b, const char* who, int kmer, const double* tables, uint32_t n_tables) {
    if (!b || !tables) { gasm_set_error("%s: null argument", who); return GASM_ERR_INVALID; }
    if (n_tables < 1 || n_tables > GASM_MAX_TABLES) { gasm_set_error("%s: n_tables must be 1..%d (got %u)", who, GASM_MAX_TABLES, n_tables); return GASM_ERR_INVALID; }
    if (!b->built) { gasm_set_error("%s before gasm_batch_build", who); return GASM_ERR_STATE; }
    ScoreTable* tbs[GASM_MAX_TABLES];
    b->table_ptrs(tbs);
    bool same[GASM_MAX_TABLES], all_same = true;
    for (u32 t = 0; t < n_tables; ++t) {
        const std::vector<double>& have = b->table_copy[t];
        same[t] = !have.empty() && memcmp(have.data(), tables + (size_t)t * GASM_TABLE_ROWS, GASM_TABLE_ROWS * sizeof(double)) == 0;
        all_same = all_same && same[t];
    }
    if (!all_same) {
        for (StepSlot& x : b->slot) if (x.cx) HIPCHK(hipStreamSynchronize(x.cx->stream));      // (whatever still scores with the old tables)
        for (u32 t = 0; t < n_tables; ++t) {
            if (same[t]) continue;
            const double* src = tables + (size_t)t * GASM_TABLE_ROWS;
            GCHK(tbs[t]->set_standard(b->ctx, src));
            b->table_copy[t].assign(src, src + GASM_TABLE_ROWS);
        }
    }
    // reads shorter than k (or none), or a table without a fixed-point shift: every table through the general scorer, which
    // sizes its arrays on the host — after the build's report
    const bool through_graph = pipeline_score_uses_graph(b->rd, b->S().bs, tbs, n_tables);
    if (!through_graph) GCHK(batch_finish(b));
    // on the stream of the build's slot, behind the build (its queue, not its completion: stream order does the rest)
    StepSlot& x = b->S();
    if (!x.paths_ready) {
        GCHK(pipeline_contig_paths(x.cx, b->rd, x.bs, x.dp));
        x.paths_ready = true;
    }
    if (!through_graph) pipeline_contig_paths_host(b->rd, x.bs, x.dp);
    GCHK(pipeline_score_launch(x.cx, b->rd, x.dp, kmer, tbs, n_tables, false, false, x.ss, &x.bs));
    b->scored = true;
    b->score_kmer = kmer;
    b->score_tables = n_tables;
    return GASM_OK;
}

int gasm_batch_score(gasm_batch* b, int kmer, const double* table) {
    API_GUARD_BEGIN
    return batch_score(b, "gasm_batch_score", kmer, table, 1);
    API_GUARD_END
}

int gasm_batch_score_tables(gasm_batch* b, int kmer, const double* tables, uint32_t n_tables) {
    API_GUARD_BEGIN
    return batch_score(b, "gasm_batch_score_tables", kmer, tables, n_tables);
    API_GUARD_END
}

// ---- row A16: breakage-score-guided traversal of a built + scored batch
int gasm_batch_guided(gasm_batch* b) {
    API_GUARD_BEGIN
    if (!b) { gasm_set_error("batch is null"); return GASM_ERR_INVALID; }
    if (!b->built || !b->scored) { gasm_set_error("gasm_batch_guided needs gasm_batch_build and gasm_batch_score first"); return GASM_ERR_STATE; }
    GCHK(batch_finish(b));
    StepSlot& x = b->S();
    GCHK(pipeline_score_fetch(x.cx, x.ss));
    return guided_build(x.cx, b->rd, x.bs, x.dp, x.ss, b->tb[0], b->score_kmer, b->guided);
    API_GUARD_END
}

int gasm_batch_fetch_guided(gasm_batch* b, const uint64_t** seg_off, const uint64_t** off, const char** data, const double** bp_score,
                            const double** norm_by_len, const int32_t** kmer_breaks) {
    API_GUARD_BEGIN
    if (!b || !seg_off || !off || !data || !bp_score || !norm_by_len || !kmer_breaks) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (!b->guided.valid) { gasm_set_error("fetch before gasm_batch_guided"); return GASM_ERR_STATE; }
    GuidedState& g = b->guided;
    GCHK(guided_fetch_text(b->S().cx, g));
    *seg_off = g.h_seg_off.data(); *off = g.h_text_off.data(); *data = g.h_text.data();
    *bp_score = g.ss.h_bp.data(); *norm_by_len = g.ss.h_nl.data(); *kmer_breaks = g.ss.h_breaks.data();
    return GASM_OK;
    API_GUARD_END
}

// the fixed-point breakage sums behind the last gasm_batch_score: bp_score[c] = fx[c] * 2^-shift exactly (what the guided
// traversal compares, and what its CPU restatement recomputes)
static int batch_fetch_fixed(gasm_batch* b, uint32_t t, const int64_t** fx, int* shift) {
    if (!b || !fx || !shift) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (!b->scored) { gasm_set_error("gasm_batch_fetch_score_fixed needs a scored batch"); return GASM_ERR_STATE; }
    if (t >= b->score_tables) { gasm_set_error("table %u of a score with %u table(s)", t, b->score_tables); return GASM_ERR_INVALID; }
    GCHK(batch_finish(b));
    StepSlot& x = b->S();
    if (!x.ss.graph) {
        gasm_set_error("the batch was scored in FP64, not in fixed point (reads shorter than k, or a table with NaN / infinite entries or a "
                       "range the 64-bit fixed point cannot hold): there are no fixed-point sums");
        return GASM_ERR_STATE;
    }
    const u32 P = x.bs.n_contigs;
    b->h_fx.resize(P);
    const size_t fx_off = (x.ss.stride * 4 + 15) & ~(size_t)15;
    HIPCHK(hipSetDevice(b->ctx->device));
    if (P) HIPCHK(hipMemcpyAsync(b->h_fx.data(), static_cast<const char*>(x.ss.d_total.p) + fx_off + (size_t)t * x.ss.stride * 8, (size_t)P * 8, hipMemcpyDeviceToHost, x.cx->stream));
    HIPCHK(hipStreamSynchronize(x.cx->stream));
    *fx = b->h_fx.data();
    *shift = b->tb[t].fix_shift;
    return GASM_OK;
}

int gasm_batch_fetch_score_fixed(gasm_batch* b, const int64_t** fx, int* shift) {
    API_GUARD_BEGIN
    return batch_fetch_fixed(b, 0, fx, shift);
    API_GUARD_END
}

int gasm_batch_fetch_score_fixed_table(gasm_batch* b, uint32_t t, const int64_t** fx, int* shift) {
    API_GUARD_BEGIN
    return batch_fetch_fixed(b, t, fx, shift);
    API_GUARD_END
}

// ---- the path of the last build (host fields of its BuildState; pipeline_build_plan): one row
int gasm_batch_build_plan(gasm_batch* b, int32_t* out, int n) {
    API_GUARD_BEGIN
    if (!b || n < 0 || (n > 0 && !out)) { gasm_set_error("gasm_batch_build_plan: bad argument"); return GASM_ERR_INVALID; }
    if (!b->built) { gasm_set_error("gasm_batch_build_plan before gasm_batch_build"); return GASM_ERR_STATE; }
    GCHK(batch_finish(b));
    if (n >= GASM_PLAN_FIELDS) pipeline_build_plan(b->rd, b->S().bs, out);      // (reads: the number of segments only)
    return 1;
    API_GUARD_END
}

// ---- count_read_kmers (lib/DeNovoAssembler.R:135-168): break-k-mer counts of the reads, kernels_count.hip
int gasm_batch_count_read_kmers(gasm_batch* b) {
    API_GUARD_BEGIN
    if (!b) { gasm_set_error("batch is null"); return GASM_ERR_INVALID; }
    if (!b->rkc_checked) GCHK(read_kmer_windows_check(b->rd));
    b->rkc_checked = true;
    // on the stream the reads were made on: behind them in stream order, beside whatever the step slots run (the kernel only
    // reads the packed stream and its offsets, which no build or score writes)
    HIPCHK(hipSetDevice(b->ctx->device));
    GCHK(b->d_rkc.ensure((size_t)b->n_segments * GASM_TABLE_ROWS * 4));
    GCHK(launch_read_kmer_count(b->ctx, b->rd, b->d_rkc.as<u32>()));
    b->rkc_counted = true;
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_fetch_read_kmer_counts(gasm_batch* b, const uint32_t** counts) {
    API_GUARD_BEGIN
    if (!b || !counts) { gasm_set_error("gasm_batch_fetch_read_kmer_counts: null argument"); return GASM_ERR_INVALID; }
    if (!b->rkc_counted) { gasm_set_error("gasm_batch_fetch_read_kmer_counts before gasm_batch_count_read_kmers"); return GASM_ERR_STATE; }
    b->h_rkc.resize((size_t)b->n_segments * GASM_TABLE_ROWS);
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipMemcpyAsync(b->h_rkc.data(), b->d_rkc.p, b->h_rkc.size() * 4, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    *counts = b->h_rkc.data();
    return GASM_OK;
    API_GUARD_END
}

// ---- read correction (kernels_correct.hip; the rule: include/gasm.h "Read correction")
int gasm_batch_correct_reads(gasm_batch* b, gasm_batch** out) {
    API_GUARD_BEGIN
    if (!b || !out) { gasm_set_error("gasm_batch_correct_reads: null argument"); return GASM_ERR_INVALID; }
    *out = nullptr;
    if (!b->built) { gasm_set_error("gasm_batch_correct_reads before a build"); return GASM_ERR_STATE; }
    GCHK(batch_finish(b));
    StepSlot& x = b->S();
    // on the stream of the slot that holds the build, behind it; always the batch's own reads (a strands = 2 build's k-mer set holds
    // both orientations already)
    DBuf words, stats;
    struct Rel { DBuf &a, &b; ~Rel() { a.release(); b.release(); } } rel{words, stats};
    GCHK(pipeline_correct_reads(x.cx, b->rd, x.bs, words, stats));
    HIPCHK(hipStreamSynchronize(x.cx->stream));
    const DevReads& rd = b->rd;
    return new_batch(b->ctx, b->n_segments, rd.n_reads, out, [&](gasm_batch* nb) {
        GCHK(nb->rd.adopt_packed(b->ctx, words, rd.fixed_len ? nullptr : rd.h_read_off.data(), rd.n_reads, rd.fixed_len, rd.h_seg_read_off.data(), rd.n_segments));
        std::swap(nb->d_correct, stats);
        nb->corrected = true;
        return (int)GASM_OK;
    });
    API_GUARD_END
}

int gasm_batch_fetch_correct_stats(gasm_batch* b, const uint32_t** stats) {
    API_GUARD_BEGIN
    if (!b || !stats) { gasm_set_error("gasm_batch_fetch_correct_stats: null argument"); return GASM_ERR_INVALID; }
    if (!b->corrected) { gasm_set_error("gasm_batch_fetch_correct_stats: not a batch made by gasm_batch_correct_reads"); return GASM_ERR_STATE; }
    b->h_correct.resize((size_t)b->n_segments * GASM_CORRECT_FIELDS);
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipMemcpyAsync(b->h_correct.data(), b->d_correct.p, b->h_correct.size() * 4, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    *stats = b->h_correct.data();
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_fetch_reads(gasm_batch* b, const char** ascii, const uint64_t** read_off) {
    API_GUARD_BEGIN
    if (!b || !ascii || !read_off) { gasm_set_error("gasm_batch_fetch_reads: null argument"); return GASM_ERR_INVALID; }
    GCHK(pipeline_fetch_reads(b->ctx, b->rd, b->h_reads_ascii, b->h_reads_off));
    *ascii = b->h_reads_ascii.data();
    *read_off = b->h_reads_off.data();
    return GASM_OK;
    API_GUARD_END
}

static const u32 kRkcRow[9] = {0, 0, 0, 0, 16, 0, 272, 0, 4368};      // first breakage-table row of each length

int gasm_count_read_kmers(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int kmer, const char* keys,
                          const uint64_t* key_off, uint64_t n_keys, uint32_t* counts) {
    API_GUARD_BEGIN
    if (!ctx || (n_reads && (!reads || !read_off)) || (keys && n_keys && !key_off)) { gasm_set_error("gasm_count_read_kmers: null argument"); return GASM_ERR_INVALID; }
    if (kmer != 2 && kmer != 4 && kmer != 6 && kmer != 8) { gasm_set_error("kmer must be 2, 4, 6 or 8 (got %d)", kmer); return GASM_ERR_INVALID; }
    const u64 n_out = keys ? n_keys : (1ull << (2 * kmer));
    if (n_out && !counts) { gasm_set_error("gasm_count_read_kmers: counts is null"); return GASM_ERR_INVALID; }
    // the table row of every key (base-4 value = lexicographic rank)
    std::vector<u32> row;
    if (keys) {
        row.resize(n_keys);
        for (u64 i = 0; i < n_keys; ++i) {
            if (key_off[i + 1] < key_off[i] || key_off[i + 1] - key_off[i] != (u64)kmer) {
                gasm_set_error("key %llu is not %d bases long", (unsigned long long)i, kmer);
                return GASM_ERR_INVALID;
            }
            u32 v = 0;
            for (u64 j = key_off[i]; j < key_off[i + 1]; ++j) {
                const u8 c = (u8)keys[j];
                if (c != 'A' && c != 'C' && c != 'G' && c != 'T') { gasm_set_error("key %llu holds a byte outside upper-case ACGT", (unsigned long long)i); return GASM_ERR_NON_ACGT; }
                v = v << 2 | (((c >> 1) & 3u) ^ ((c >> 2) & 1u));
            }
            row[i] = v;
        }
    }
    std::vector<u32> tab(1ull << (2 * kmer), 0);
    if (n_reads && read_off[n_reads] > read_off[0]) {
        // one segment of ragged reads through the batch kernel
        DevReads rd;
        DBuf d;
        struct Rel { DevReads& r; DBuf& d; ~Rel() { r.release(); d.release(); } } rel{rd, d};
        const u64 seg_off[2] = {0, n_reads};
        GCHK(rd.upload(ctx, reads, read_off, n_reads, 0, seg_off, 1));
        GCHK(read_kmer_windows_check(rd));
        GCHK(d.ensure((size_t)GASM_TABLE_ROWS * 4));
        GCHK(launch_read_kmer_count(ctx, rd, d.as<u32>()));
        HIPCHK(hipMemcpyAsync(tab.data(), d.as<u32>() + kRkcRow[kmer], tab.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    } else if (n_reads) {
        for (u64 r = 0; r < n_reads; ++r)
            if (read_off[r + 1] < read_off[r]) { gasm_set_error("read_off not monotone"); return GASM_ERR_INVALID; }
    }
    if (keys) for (u64 i = 0; i < n_keys; ++i) counts[i] = tab[row[i]];
    else memcpy(counts, tab.data(), tab.size() * 4);
    return GASM_OK;
    API_GUARD_END
}

uint64_t gasm_batch_total_kmers(const gasm_batch* b) { return b ? b->S().bs.n_kmers : 0; }
uint64_t gasm_batch_total_reads(const gasm_batch* b) { return b ? b->n_reads : 0; }

int gasm_batch_fetch_distinct(gasm_batch* b, const uint64_t** seg_off, const uint64_t** keys, const uint32_t** mult, int* words) {
    API_GUARD_BEGIN
    if (!b || !seg_off || !keys || !mult || !words) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (!b->built) { gasm_set_error("fetch before build"); return GASM_ERR_STATE; }
    GCHK(batch_finish(b));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_distinct(b->S().cx, b->build_reads(b->S()), bs));
    *words = bs.words;
    *seg_off = bs.h_seg_doff.data(); *keys = bs.h_dk_key.data(); *mult = bs.h_dk_cnt.data();
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_fetch_graph(gasm_batch* b, const uint8_t** edge_flags, const uint32_t** edge_next) {
    API_GUARD_BEGIN
    if (!b || !edge_flags || !edge_next) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (!b->built) { gasm_set_error("fetch before build"); return GASM_ERR_STATE; }
    GCHK(batch_finish(b));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_graph(b->S().cx, b->build_reads(b->S()), bs));
    *edge_flags = bs.h_eflag.data(); *edge_next = bs.h_nxt.data();
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_fetch_contigs(gasm_batch* b, const uint64_t** seg_contig_off, const uint64_t** off, const char** data) {
    API_GUARD_BEGIN
    if (!b || !seg_contig_off || !off || !data) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (!b->built) { gasm_set_error("fetch before build"); return GASM_ERR_STATE; }
    GCHK(batch_finish(b));
    BuildState& bs = b->S().bs;
    GCHK(pipeline_fetch_contigs(b->S().cx, b->build_reads(b->S()), bs));
    *seg_contig_off = bs.h_seg_coff.data(); *off = bs.h_c_off.data(); *data = bs.h_contigs.data();
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_fetch_scores(gasm_batch* b, const double** bp_score, const double** norm_by_break_freqs, const double** norm_by_len,
                            const int32_t** kmer_breaks, const int32_t** sequence_len) {
    API_GUARD_BEGIN
    if (!b || !bp_score || !norm_by_break_freqs || !norm_by_len || !kmer_breaks || !sequence_len) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    GCHK(batch_finish(b));
    ScoreState& ss = b->S().ss;
    GCHK(pipeline_score_fetch(b->S().cx, ss));
    *bp_score = ss.h_bp.data(); *norm_by_break_freqs = ss.h_nf.data(); *norm_by_len = ss.h_nl.data();
    *kmer_breaks = ss.h_breaks.data(); *sequence_len = ss.h_len.data();
    return GASM_OK;
    API_GUARD_END
}

int gasm_batch_fetch_scores_table(gasm_batch* b, uint32_t t, const double** bp_score, const double** norm_by_break_freqs, const double** norm_by_len,
                                  const int32_t** kmer_breaks, const int32_t** sequence_len) {
    API_GUARD_BEGIN
    if (!b || !bp_score || !norm_by_break_freqs || !norm_by_len || !kmer_breaks || !sequence_len) { gasm_set_error("null argument"); return GASM_ERR_INVALID; }
    if (t >= b->score_tables) { gasm_set_error("table %u of a score with %u table(s)", t, b->score_tables); return GASM_ERR_INVALID; }
    GCHK(batch_finish(b));
    ScoreState& ss = b->S().ss;
    GCHK(pipeline_score_fetch(b->S().cx, ss));
    const size_t at = (size_t)t * ss.n_paths;           // (the host arrays hold table after table)
    *bp_score = ss.h_bp.data() + at; *norm_by_break_freqs = ss.h_nf.data() + at; *norm_by_len = ss.h_nl.data() + at;
    *kmer_breaks = ss.h_breaks.data(); *sequence_len = ss.h_len.data();
    return GASM_OK;
    API_GUARD_END
}

}  // extern "C"
