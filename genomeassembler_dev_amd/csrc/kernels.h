// kernels.h — kernel declarations and the small POD views passed to them by value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "device_utils.h"
#include "keyops.h"

// Reads of all segments of a batch, packed 2-bit in one base stream.
struct ReadSet {
    const u64* words;          // packed bases (+2 padding words)
    const u64* read_off;       // n_reads+1 base offsets; nullptr for fixed-length reads back to back; n_reads base positions
                               // of fixed-length reads that do not lie back to back (read_span)
    const u64* seg_read_off;   // n_segments+1 read indices
    const u32* seg_tile_start; // n_segments+1 tile indices (depends on the tile width of the launch)
    const uint4* tile_info;    // per tile {segment, reads in the tile, first read lo, first read hi (16 bits) | offset round << 16}
    u32 fixed_len;
    u32 n_segments;
};

// Where read r lies in the packed stream.  Three layouts: ragged (read_off[n+1], fixed_len = 0), fixed length back to back
// (read_off = nullptr), and fixed length at given base positions (read_off[n] with fixed_len > 0: the reads of a pooled
// build arrive as word-aligned pieces from every rank, pipeline.hip "pool").
__device__ __forceinline__ void read_span(const ReadSet& rs, u64 r, u64* p0, u32* len) {
    if (rs.fixed_len) { *p0 = rs.read_off ? rs.read_off[r] : r * rs.fixed_len; *len = rs.fixed_len; }
    else { const u64 a = rs.read_off[r]; *p0 = a; *len = (u32)(rs.read_off[r + 1] - a); }
}

// Sorted distinct k-mers (= distinct edges) of all segments, dense, with the per-(segment,bucket) directory.
struct GraphView {
    const void* dk_key;  // D_total keys (u64 or K128), sorted inside each segment
    const u32* dstart;   // n_segments * 2^bbits + 1
    const u16* fdir;     // fine directory: per bucket 2^fbits + 1 offsets (relative to the bucket) of the key bins the
                         // de-duplication kernel sorted by — the next fbits key bits below the bucket prefix
    int k;
    int bbits;
    int fbits;
};

// Lower bound of k-mer t among the distinct k-mers of segment `seg`: bucket by the first bbits bits, bin by the next
// fbits bits (about 1.5 keys per bin), then a search inside the bin.  *bucket_hi = end of the bucket: the result is a
// valid lower bound inside [bucket start, *bucket_hi].
template <class K>
__device__ __forceinline__ u32 graph_lower_bound(const GraphView& gv, u32 seg, const K& t, u32* bucket_hi) {
    const K* dk = reinterpret_cast<const K*>(gv.dk_key);
    const u32 nb = 1u << gv.bbits;
    const int low = 2 * gv.k - gv.bbits;
    const u32 gb = seg * nb + (gv.bbits ? kfield(t, low) : 0u);
    // (two neighbours of a directory = ONE load each, unaligned: the lookups of the graph kernels are bound by the number of
    // line requests they send to L2 — ~16 per clock and XCD —, and a pair of 2- or 4-byte loads are two requests)
    uint2 dd;
    __builtin_memcpy(&dd, gv.dstart + gb, 8);
    const u32 base = dd.x;
    *bucket_hi = dd.y;
    const int bshift = low > gv.fbits ? low - gv.fbits : 0;
    const u32 nbin = 1u << gv.fbits;
    const u16* f = gv.fdir + (u64)gb * (nbin + 1) + (kfield(t, bshift) & (nbin - 1));
    u32 ff;
    __builtin_memcpy(&ff, f, 4);
    u32 lo = base + (ff & 0xFFFFu);
    u32 hi = base + (ff >> 16);
    // (a directory that is not one — a bucket of a failed build attempt whose kernels were queued ahead of its report —
    // must still end the search: bounds inside the bucket, in order)
    if (hi > *bucket_hi) hi = *bucket_hi;
    if (lo > hi) lo = hi;
    while (hi - lo > 4) {                          // only skewed bins are this long
        const u32 m = (lo + hi) >> 1;
        if (kless(dk[m], t)) lo = m + 1;
        else hi = m;
    }
    while (lo < hi && kless(dk[lo], t)) ++lo;      // bins usually hold one or two keys
    return lo;
}

// Paths (contigs or caller-supplied sequences) of all segments, packed, for scoring.
struct PathSet {
    const u64* words;        // packed bases of all paths, concatenated without gaps (+2 padding words)
    const u64* p_off;        // n_paths+1 base offsets
    const u32* seg_path_off; // n_segments+1 path indices
    u32 n_segments;
};

#define GASM_KT 16          // k-mers per thread and round of the tile kernels for 64-bit keys (8 for 128-bit keys)
#define GASM_SCORE_PATH_CAP 6144   // paths of one segment whose score accumulators k_score_reads_graph keeps in LDS
#define GASM_TBL 4096       // slots of the large LDS de-duplication table (the small one has 2048)
#define GASM_TBL_LIMIT 2816 // distinct keys one bucket may hold (11/16 of the table) before the host re-partitions
// Bins of the counting sort that orders a table of `tbl` slots (k_bucket_dedup, k_bucket_dedup_multi, k_bucket_merge) = entries
// of a bucket's row of the fine directory, and their logarithm: GraphView::fbits of what such a kernel wrote
constexpr int dedup_bins(int tbl) { return tbl / 4; }
constexpr int dedup_fbits(int tbl) { return tbl <= 4 ? 0 : 1 + dedup_fbits(tbl / 2); }
static_assert(1 << dedup_fbits(2048) == dedup_bins(2048) && 1 << dedup_fbits(GASM_TBL) == dedup_bins(GASM_TBL), "the bins are a power of two");

// ---- the flag area of a build (BuildState::d_flags): GASM_FLAG_WORDS u32 words, behind them the one-pass partition's cursors.
// The one definition of who writes which word, shared by the kernels and the host.
enum : u32 {
    GASM_FLAG_OVERFLOW = 0,         // GASM_OVF_* bits, raised by the partition, the de-duplications and the merge
    GASM_FLAG_RANK_FAILED = 1,      // the LDS list ranking gave up (k_rank_rulers, k_rank_lds)
    GASM_FLAG_SCORE_MISMATCH = 2,   // the graph scorer met a read that differs from its contig (GASM_SCORE_VERIFY)
    GASM_FLAG_DEDUP_DONE = 8,       // finished workgroups of k_bucket_dedup (its last one scans the buckets' counts)
    GASM_FLAG_CONTIG_DONE = 9,      // finished workgroups of k_contig_scan (its last one writes the report)
    GASM_FLAG_SOLID_DONE = 10,      // finished workgroups of k_bucket_solid (its last one redoes the scan)
    GASM_FLAG_ACTIVE = 16,          // "still active" word of every k_link_jump launch of a build ...
    GASM_FLAG_ACTIVE_N = 40,        // ... and how many launches have one
    GASM_FLAG_WORDS = 64,           // words the kernels below zero
    GASM_FLAG_CURSORS = 64,         // first cursor of k_bucket_partition (one per (segment, bucket))
    GASM_FLAG_BYTES = 256,          // size of the area without cursors
    GASM_OVF_TABLE = 1,             // a bucket holds more distinct keys than its table (or, multi-pass, than GASM_BUCKET_MAX)
    GASM_OVF_REGION = 2,            // a bucket outgrew its region of the one-pass partition
    GASM_OVF_TIP_RANK = 4,          // the LDS list ranking gave up in a tip-clipping, bubble-popping or low-coverage round before the
                                    // last graph pass (k_tip_mark, k_bubble_mark, k_lowcov_mark)
};
static_assert(GASM_FLAG_ACTIVE + GASM_FLAG_ACTIVE_N <= GASM_FLAG_WORDS && GASM_FLAG_WORDS * 4 == GASM_FLAG_BYTES, "flag area layout");
// Zeroing contract.  Every attempt at the distinct k-mers starts with all GASM_FLAG_WORDS words zero: the one-pass partition
// clears words and cursors with one fill on the stream, the two-pass partition has k_tile_scan clear the words, and the pooled
// stages that produce runs without a partition (merges, a rank without k-mers) fill GASM_FLAG_BYTES.  So the done counters are
// zero when their kernel starts, and GASM_FLAG_OVERFLOW holds what this attempt raised.  Every graph launch — the first, and a
// repeat after a failed ranking — starts with k_bucket_gather clearing every word except GASM_FLAG_OVERFLOW, which stays for
// the report: the ranking's flag, the scorer's flag, k_contig_scan's counter and the active words are zero again.  A build
// with tip clipping runs a graph pass per round: the gather of each pass also clears the done counter of the compaction
// (GASM_FLAG_SOLID_DONE) that ran in front of it, and k_tip_mark saves a ranking failure of its pass into the overflow word.
// The rounds of bubble popping behind them are the same passes with k_bubble_mark in k_tip_mark's place, and the low-coverage
// rounds behind those with k_lowcov_mark.

// The pinned report of a build over S segments (BuildState::h_report, u32 words), written by k_contig_scan's last workgroup,
// the ticket last: first distinct k-mer, first contig and first contig base (lo, hi) of every segment, each with the total in
// entry S; then flag word GASM_FLAG_OVERFLOW, flag word GASM_FLAG_RANK_FAILED and the ticket.
template <class W>
struct BuildReport {
    W* w;
    u32 S;
    __host__ __device__ W& dstart(u32 s) const { return w[s]; }
    __host__ __device__ W& cstart(u32 s) const { return (w + S + 1)[s]; }
    __host__ __device__ W& bstart_lo(u32 s) const { return (w + 2 * S + 2)[2 * s]; }
    __host__ __device__ W& bstart_hi(u32 s) const { return (w + 2 * S + 2)[2 * s + 1]; }
    __host__ __device__ W& flags() const { return w[4 * S + 4]; }
    __host__ __device__ W& rank_failed() const { return w[4 * S + 5]; }
    __host__ __device__ W& ticket() const { return w[4 * S + 6]; }
    static size_t words(u32 S) { return 4 * (size_t)S + 8; }
};

// ---- kernels_build.hip
__global__ void k_pack_ascii(const u8* ascii, u64 nbases_host, const u64* nbases_dev, u64* words, u32* err);
#define GASM_TILE_WG 512     // threads of a tile workgroup (k_tile_hist, k_bucket_scatter)
// ---- what k_bucket_scatter / k_bucket_partition and their launches (pipeline.hip) share: the one definition of each
// The staging area of a tile: NFL flush passes of 16 bytes per thread (the tile's keys + room for the padding of the staged
// runs), then eight trash slots per wave for the starts past a read's end.
template <class K> struct TileStage {
    static constexpr u32 KPU = 16 / sizeof(K);                                                 // keys per 16-byte unit
    static constexpr u32 CAP = KeyTraits<K>::NFL * GASM_TILE_WG * KPU;                         // keys staged at most
    static constexpr u32 TRASH = GASM_TILE_WG / 8;                                             // trash slots
    static constexpr u32 BYTES = (CAP + TRASH) * (u32)sizeof(K);
    static constexpr u32 PAD_ROOM = (KeyTraits<K>::NFL * KPU - KeyTraits<K>::KT) * GASM_TILE_WG; // keys of padding one tile may stage beyond its own
};
// Dynamic LDS of the two kernels for nb buckets: the arrays behind the staging area in the order the kernel carves them from
// one block (element counts; each array starts where the one before it ends), and the launch's total in bytes.  The
// per-bucket words and the dummy bin behind them are two counts, added to the pointer one after the other as the kernels
// always did: the sum formed first, in 32 bits, costs the compiler what it knows about the alignment of what follows.
template <class K> struct ScatterLds {
    u32 nb;
    static constexpr u32 n_key = TileStage<K>::CAP + TileStage<K>::TRASH;    // K
    constexpr u32 n_comb() const { return (nb + 1) & ~1u; }                   // u64: nb, rounded so that the cursors are 16-byte aligned
    constexpr u32 n_sub() const { return 4 * nb; }                            // u32: 4 per bucket (sub-cursors) ...
    static constexpr u32 n_dummy = 4;                                         // ... + the dummy bin
    static constexpr u32 n_tmp = 12;                                          // u32
    constexpr size_t total() const { return TileStage<K>::BYTES + (size_t)nb * 8 + ((size_t)n_sub() + n_dummy + n_tmp) * 4 + 32; }   // + 32 bytes: the rounding above, the rest spare
};
template <class K> struct PartitionLds {
    u32 nb;
    static constexpr u32 n_key = TileStage<K>::CAP + TileStage<K>::TRASH;    // K
    constexpr u32 n_comb() const { return nb; }                               // uint4
    constexpr u32 n_sub() const { return 4 * nb; }                            // u32, twice (bases, then sub-counters): 4 per bucket ...
    static constexpr u32 n_dummy = 4;                                         // ... + the dummy bin
    static constexpr u32 n_tmp = 12;                                          // u32
    constexpr u32 n_cin() const { return nb; }                                // u32
    constexpr size_t total() const { return TileStage<K>::BYTES + (size_t)n_comb() * 16 + (2 * ((size_t)n_sub() + n_dummy) + n_tmp + n_cin()) * 4; }
};
// The scratch line of the flush: one 16-byte slot per wave of GASM_FLUSH_WGS workgroup slots, behind the key array; the lanes
// of a store that have nothing to flush write there, so that the number of stores per thread does not vary
#define GASM_FLUSH_WGS 1024
#define GASM_FLUSH_SLOTS (GASM_FLUSH_WGS * (GASM_TILE_WG / 64))
__device__ __forceinline__ u32 flush_slot(u32 wave) { return (blockIdx.x % GASM_FLUSH_WGS) * (GASM_TILE_WG / 64) + wave; }      // < GASM_FLUSH_SLOTS
template <class K> __global__ void k_tile_hist(ReadSet rs, const uint4* tinfo, int k, int bbits, u32 g, u32 n_tiles, ushort4* tcnt);
__global__ void k_tile_scan(ReadSet rs, int bbits, u32 padm, const ushort4* tcnt, u32* toff, u32* hist, u32* flags);
template <class TO> __global__ void k_scan_excl(const u32* in, TO* out, u32 n);
__global__ void k_copy_u64(const u64* a, u64* b, u32 n);
template <class K>
__global__ void k_bucket_scatter(ReadSet rs, const uint4* tinfo, int k, int bbits, u32 g, u32 padm, u32 n_tiles, const u64* bstart, const u32* toff,
                                 const ushort4* tcnt, K* keys, u64 scratch);
#define GASM_RT_MAX 16      // rounds (read groups x offset rounds) one scatter tile may hold
template <class K>
__global__ void k_bucket_partition(ReadSet rs, const uint4* tinfo, int k, int bbits, u32 g, u32 padm, u32 n_tiles, const u64* bstart, u32* cursor,
                                   K* keys, u64 scratch, u32* flags);
template <class K, int TBL>
__global__ void k_bucket_dedup(K* keys, u32* mult, const u64* bstart, const u32* blen, u32* bucket_d, u32* overflow, u16* fdir, int low_bits, u32* dstart);
#define GASM_BUCKET_MAX 65535   // distinct keys of one bucket (16-bit fine directory)
template <class K>
__global__ void k_bucket_dedup_multi(const K* keys, K* keys_out, u32* mult, const u64* bstart, u32* bucket_d, u32* overflow, u16* fdir, int low_bits);
// multiplicity cutoff (min_count > 1): compacts every bucket's sorted run in place, rewrites its fine-directory row
template <class K>
__global__ void k_bucket_solid(K* keys, u32* mult, const u64* bstart, u32* bucket_d, u16* fdir, int low_bits, int fbits, int bbits, u32 min_count,
                               u32* removed, u32* done, u32* dstart);
// tip clipping (tip_len > 0): zeroes, in the bucket runs, the multiplicities of the edges of every tip of the ranked graph
template <class K>
__global__ void k_tip_mark(GraphView gv, u32 n_segments, u32 chunks, const u8* eflag, const u32* clen, const u32* nxt, const u32* dk_cnt, const u64* bstart,
                           u32* mult, u32 tip_len, u32* flags, u32* tips);
// bubble popping (bubble_len > 0): the same for every short contig beside which a parallel one of strictly higher mean multiplicity runs
template <class K>
__global__ void k_bubble_mark(GraphView gv, u32 n_segments, u32 chunks, const u8* eflag, const u32* clen, const u32* nxt, const u32* dk_cnt, const u64* bstart,
                              u32* mult, u32 bubble_len, u32* flags, u32* bubbles);
__global__ void k_kmer_spectrum(const u32* dstart, u32 nb, const u32* dk_cnt, u32 n_segments, u32 chunks, u32* hist);
// low-coverage removal (cov_cutoff > 0, cov_len > 0): the same for every short contig whose mean multiplicity is strictly below cov_cutoff
template <class K>
__global__ void k_lowcov_mark(GraphView gv, u32 n_segments, u32 chunks, const u8* eflag, const u32* clen, const u32* nxt, const u32* dk_cnt, const u64* bstart,
                              u32* mult, u32 cov_len, u32 cov_cutoff, u32* flags, u32* removed);
// per-contig coverage of a finished build: msum[c] += multiplicities, nedges[c] += 1 for every edge of contig c (both zeroed by the caller)
__global__ void k_contig_cov(const u32* dstart, u32 nb, u32 n_segments, u32 chunks, const u64* link, const u32* e_cid, const u32* dk_cnt,
                             const u32* seg_cstart, unsigned long long* msum, u32* nedges);
template <class K>
__global__ void k_bucket_gather(const K* keys, const u32* mult, const u64* bstart, const u32* dstart, K* dk_key, u32* dk_cnt, u32* claim, u8* eflag,
                                u32* flags);
template <class K> __global__ void k_edge_target(GraphView gv, u32 n_segments, u32 chunks, u32* tgt, u32* claim);
__global__ void k_edge_multi(GraphView gv, u32 n_segments, u32 chunks, const u32* tgt, const u32* claim, u8* eflag);
template <class K>
__global__ void k_node_flags(GraphView gv, u32 n_segments, u32 chunks, const u32* claim, u8* eflag, u64* link, u32* clen);
__global__ void k_edge_next(GraphView gv, u32 n_segments, u32 chunks, const u32* tgt, const u8* eflag, u32* nxt, u64* link);
__global__ void k_link_jump(GraphView gv, u32 n_segments, u32 chunks, u64* link, const u32* prev_active, u32* active, int jumps, const u32* nxt,
                            u32* clen);
__global__ void k_rank_rulers(GraphView gv, u32 n_segments, u32 chunks, u64* link, u32* rtab, u32 rshift, u32* flags);
__global__ void k_rank_lds(GraphView gv, const u32* rtab, u64* link, int max_rounds, u32 rshift, u32 lds_entries, u32* flags);
__global__ void k_chain_len(const u32* nxt, const u64* link, u32* clen, const u32* n_edges_p);
__global__ void k_contig_scan(GraphView gv, const u8* eflag, const u32* clen, u32* e_cid, u64* e_coff, u32* seg_ncontig,
                              u64* seg_cbases, u32* done, u32* seg_cstart, u64* seg_bstart, const u32* flags, u32* report, u32 ticket);
__global__ void k_contig_place(GraphView gv, const u8* eflag, const u32* seg_cstart, const u64* seg_bstart, u32* e_cid, u64* e_coff,
                               u64* c_off, u32 n_segments, u32 chunks);
template <class K>
__global__ void k_contig_emit(GraphView gv, const u64* link, const u32* nxt, const u64* e_coff, u8* out, u32 n_segments, u32 chunks);
// both strands (strands = 2): every segment's reads followed by their reverse complements, into a zeroed stream; g threads per read
__global__ void k_reads_both_strands(const u64* words, const u64* read_off, const u64* seg_read_off, u32 fixed_len, u32 n_segments, u64 n_reads, u32 g,
                                     unsigned long long* out);
// twin[c] = index inside its segment of the contig that is contig c's reverse complement; *bad |= 1 where there is none
template <class K>
__global__ void k_contig_twin(GraphView gv, const u64* link, const u32* e_cid, const u64* c_off, const u32* seg_cstart, const u8* text, u32 n_segments,
                              u32* twin, u32* bad);

// ---- kernels_pool.hip
template <class K>
__global__ void k_pack_runs(const K* keys, const u32* mult, const u64* bstart, const u32* bucket_d, const u32* gb_list, const u64* dst_off, K* out_keys,
                            u32* out_cnt);
template <class K, int TBL>
__global__ void k_bucket_merge(const K* in_keys, const u32* in_cnt, const u64* run_off, const u32* run_len, u32 n_src, K* out_keys, u32* out_cnt,
                               const u64* bstart, u32* bucket_d, u32* overflow, u16* fdir, int low_bits, const u64* src_base);
__global__ void k_repack_reads(const u64* src, const u64* dir, u64* words_out);
__global__ void k_piece_positions(const u64* piece_first, const u64* piece_word_off, u32 n_pieces, u64 n_reads, u32 fixed_len, u64* pos);
__global__ void k_slice_last(const u32* a, const u64* off, u32 n, u32* out);

// ---- kernels_asm.hip
__global__ void k_chain_expand(const u64* cwords, const u64* c_off, const u64* sig_off, const u32* elem_contig, const u32* elem_skip, const u64* elem_pos,
                               const u64* out_off, u32 n_scaffolds, u64* out, u64 n_words);
struct ChainSigs {             // the scaffolds' signatures beside their text (k_str_bitonic skips what two chains share)
    const u64* sig_off;        // n + 1
    const u32* elem_contig;
    const u32* elem_skip;
    const u64* elem_pos;       // where the element's own bases start in its scaffold
};
__global__ void k_str_bitonic(const u64* words, const u64* off, u32* idx, u32 n_pow2, u32 kk, u32 j, ChainSigs cs);
__global__ void k_str_bitonic_block(const u64* words, const u64* off, u32* idx, u32 n_pow2, u32 kk, u32 j0, ChainSigs cs);
__global__ void k_str_adjacent_eq(const u64* words, const u64* off, const u32* idx, u32 n, u8* same_as_prev, ChainSigs cs);
__global__ void k_unpack_ascii(const u64* words, u64 nbases, u8* out);
__global__ void k_guided_chain(PathSet ps, const unsigned long long* fx, int k, u32* g_next, u32* g_prev, u32* dbg_order);
__global__ void k_asm_match(const u64* cwords, const u64* c_off, u32 n, int k, u8* match, u8* row_any, u8* level_any);
__global__ void k_asm_merge(const u32* perm, u32 rows, u32 n, int k, const u32* clen, const u8* match, const u8* row_any, const u8* level_any,
                            const u64* cwords, const u64* c_off, u32* out_next, u8* out_ov, u32* out_heads, u32* out_nchains, u8* need_host);

// ---- kernels_sim.hip
__global__ void k_sim_weights(const u64* gwords, const u64* gbase, const u64* woff, u32 n_segments, int kmer, const long long* fixw, u64* w);
template <class T> __global__ void k_seg_scan_incl(T* a, const u64* off);
__global__ void k_sim_draw(const u64* cum, const u64* woff, const u64* doff, const u64* glen, u64 seed, u32 read_len, u32* start, u32* keep);
__global__ void k_sim_compact(const u32* start, const u32* keep, const u32* rank, const u64* doff, const u64* seg_read_off, u32* kept_start);
__global__ void k_sim_extract(const u64* gwords, const u64* gbase, const u64* seg_read_off, const u32* kept_start, u32 read_len, unsigned long long* out);

// ---- kernels_count.hip: break-k-mer counts of the reads, GASM_TABLE_ROWS per segment; 2^LS workgroups per segment
template <int LS>
__global__ void k_read_kmer_count(const u64* words, const u64* read_off, const u64* seg_read_off, u32 fixed_len, u32 n_segments, u32* out);

// ---- the passes that lay reads over a finished build (their shared frame: contig_index.h)
// what they need of the build beside the k-mer directory, one kernel argument as GraphView is (host: contig_index(bs))
struct ContigIndex {
    const u64* link;       // per edge: head << 32 | done << 31 | distance
    const u32* e_cid;      // at a head: its contig
    const u64* c_off;      // per contig: its first base in the batch's contig text (+ the end of the last)
    const u32* seg_cstart; // n_segments + 1 contig indices
    const u8* text;        // the contigs' ASCII, as the build emitted it
    int have_graph;        // 0: the build holds no contig at all, and the arrays above may not exist
};

// ---- kernels_correct.hip: read correction against the distinct k-mers of a finished build (include/gasm.h, "Read correction")
#define GASM_CORRECT_STATS 6          // = GASM_CORRECT_FIELDS of include/gasm.h (checked in pipeline.hip)
#define GASM_CORRECT_KMER_CAP 4096    // = GASM_CORRECT_MAX_KMERS: k-mers of a read whose weak bits one wave keeps (64 lanes x 64 bits)
// out_words: a copy of rs.words that receives the fixes; stats: GASM_CORRECT_STATS zeroed counters per segment
template <class K>
__global__ void k_read_correct(ReadSet rs, GraphView gv, int have_graph, u32 reads_per_wg, u32 chunks, unsigned long long* out_words, u32* stats);

// ---- kernels_links.hip: the links between the contigs of a finished build and the reads' support for them (include/gasm.h, "Contig links")
#define GASM_THREAD_KMER_CAP 4096     // = GASM_THREAD_MAX_KMERS: k-mers of a read whose in-set bits one wave keeps (64 words of 64 bits in LDS)
// succ / pred: 4 entries per contig, filled with GASM_NONE32 by the caller
template <class K>
__global__ void k_contig_links(GraphView gv, ContigIndex ci, u32 n_segments, u32* succ, u32* pred);
// link_support: 4 per contig, span_support: 16 per contig, skipped: one per segment, all zeroed by the caller
template <class K>
__global__ void k_read_thread(ReadSet rs, GraphView gv, ContigIndex ci, u32 span_len, u32 reads_per_wg, u32 chunks, u32* link_support, u32* span_support,
                              unsigned long long* skipped);
// read pairs (include/gasm.h, "Read pairs"): orient = 1 or 2 orientations per pair; rec: 4 int32 per oriented pair (16-byte aligned), n_pairs
// pairs per orientation; hist: max_insert + 1 bins per segment, counters: GASM_PAIR_COUNTERS per segment, both zeroed by the caller
#define GASM_PAIR_COUNTERS 6          // = GASM_PAIR_FIELDS of include/gasm.h (checked in pipeline.hip)
template <class K>
__global__ void k_pair_place(ReadSet rs, GraphView gv, ContigIndex ci, u32 orient, u32 max_insert, u64 n_pairs, u32 chunks, int32_t* rec, u32* hist,
                             unsigned long long* counters);

// ---- kernels_map.hip: read mapping, ungapped (include/gasm.h, "Read mapping") and gapped ("Gapped read mapping"): one body, GAPPED = false
// is the launch "k_read_map", GAPPED = true the launch "k_read_map_gapped", GAPPED and ENDS the launch "k_read_map_ends", all three flags
// the launch "k_read_map_trace" (include/gasm.h, "Alignments")
#define GASM_MAP_COUNTERS 7           // = GASM_MAP_FIELDS of include/gasm.h (checked in pipeline.hip)
#define GASM_MAPG_COUNTERS 8          // = GASM_MAPG_FIELDS: the same seven and the gapped reads
#define GASM_MAP_BLOCKS 8             // = GASM_MAP_MAX_BLOCKS: distinct heads of a read that are kept (one per lane 0 .. 7 of its wave)
#define GASM_MAPG_GAP 16              // = GASM_MAP_MAX_GAP: the longest gap between two heads of a chain (its skipped bases take one lane each)
// rec: 4 int32 per read (16-byte aligned); pile: 4 u32 per base of the contig text; hist: max_edits + 1 bins per segment (ungapped: max_edits
// is max_mismatch); counters: GASM_MAP_COUNTERS or GASM_MAPG_COUNTERS per segment.  Gapped only (else not read): rec_gap, 4 int32 per
// read (16-byte aligned), and gap_pile, 2 u32 per base of the text (deletions, insertions).  All but the records zeroed by the caller
// ENDS = true (with GAPPED; include/gasm.h, "End gaps"; the launch "k_read_map_ends") only (else not read): end_gap, rec_end, 4 int32 per read
// (16-byte aligned), and end_counters, GASM_MAPEND_COUNTERS per segment, zeroed by the caller
#define GASM_MAPEND_COUNTERS 4        // = GASM_MAPEND_FIELDS: front, back, rescued, start_moved
// TRACE = true (with GAPPED and ENDS; the launch "k_read_map_trace") only (else not read): rec_piece, GASM_MAP_PIECES pieces of 2 int32 per read
// (s | e << 16, d; 16-byte aligned; every read's are written), and ins_pile, max(max_gap, end_gap) columns of 4 u32 per base of the text,
// zeroed by the caller.  They come in a struct of their own behind MapOut's, so that the three other forms keep their kernel arguments
#define GASM_MAP_PIECES (GASM_MAP_BLOCKS + 2)      // = GASM_MAP_MAX_PIECES: a chain over every kept head and a piece beyond the gap at each end
struct MapOut {
    int32_t *rec, *rec_gap;
    u32 *pile, *gap_pile, *hist;
    unsigned long long* counters;
    int32_t* rec_end;
    unsigned long long* end_counters;
};
struct MapOutTrace : MapOut {
    int32_t* rec_piece;
    u32* ins_pile;
};
template <bool TRACE>
using MapOutOf = std::conditional_t<TRACE, MapOutTrace, MapOut>;
template <class K, bool GAPPED, bool ENDS, bool TRACE>
__global__ void k_read_map(ReadSet rs, GraphView gv, ContigIndex ci, u32 max_edits, u32 max_gap, u32 end_gap, u32 reads_per_wg, u32 chunks, MapOutOf<TRACE> out);

// ---- kernels_score.hip
struct SeedTable {
    u64* seed;            // slot -> seed value
    u32* gpos;            // slot -> read index (GASM_NONE32 = empty)
    const u64* tbl_off;   // n_segments+1 slot offsets; every segment's table size is a power of two
};
__global__ void k_read_insert(ReadSet rs, SeedTable st, int w);
__global__ void k_path_scan(ReadSet rs, PathSet ps, SeedTable st, const u64* seg_base_off, int w, const u64* first_off, u32* first, u32 seg0,
                            u32 path_lo, u32 path_hi);
__global__ void k_first_to_poscnt(const u32* first, u64 n, u32* poscnt);
// the scorers take T = 1 .. GASM_SCORE_MAX_TABLES breakage tables over one match (one table: T = 1)
#define GASM_SCORE_MAX_TABLES 8    // = GASM_MAX_TABLES of include/gasm.h (checked in pipeline.hip)
struct FixTables { const long long* p[GASM_SCORE_MAX_TABLES]; };     // direct-address fixed-point tables (ScoreTable::d_fix)
struct ProbTables { const double* p[GASM_SCORE_MAX_TABLES]; };       // direct-address probability tables (ScoreTable::d_prob)
// sums of table t at sum + t * sum_stride; LDS: T * lds_paths u64 + lds_paths u32
template <class K, int T>
__global__ void k_score_reads_graph(ReadSet rs, GraphView gv, const u64* link, const u32* e_cid, PathSet ps, FixTables dfix, int kmer,
                                    u32 reads_per_wg, u32 chunks, u32 lds_paths, u32* cnt, unsigned long long* sum, u64 sum_stride, int verify,
                                    u32* verify_flag);
// mapped scoring (include/gasm.h, "Mapped scoring"): rec (GAPPED: and rec_gap) are a read mapping's records over the build of `ci`, 4 int32 per
// read; cnt, sum (table t at sum + t * sum_stride), start_pile (one per base of the contig text) and counters (GASM_MAPSCORE_CLASSES per segment)
// zeroed by the caller; LDS as k_score_reads_graph
#define GASM_MAPSCORE_CLASSES 4       // = GASM_MAPSCORE_FIELDS of include/gasm.h (checked in pipeline.hip)
template <int T, bool GAPPED>
__global__ void k_score_mapped(ReadSet rs, ContigIndex ci, const int32_t* rec, const int32_t* rec_gap, FixTables dfix, int kmer, u32 partial,
                               u32 reads_per_wg, u32 chunks, u32 lds_paths, u32* cnt, unsigned long long* sum, u64 sum_stride, u32* start_pile,
                               unsigned long long* counters);
__global__ void k_levenshtein(PathSet ps, u32 n_paths, const u64* twords, u32 nt, int infix, u8* carry_ws, u64 carry_stride, int32_t* out);
__global__ void k_levenshtein2(PathSet ps, u32 n_paths, const u64* twords, u32 nt, int infix, uint4* carry_ws, u64 carry_stride, int32_t* out);
__global__ void k_score_zero(u32* cnt, unsigned long long* sum, u64 sum_stride, u32 n_tables, const u32* n_paths_p);
__global__ void k_score_finish(PathSet ps, const u32* cnt, const unsigned long long* sum, const long long* dfix, const u64* seg_empty,
                               int kmer, double inv_scale, double* bp_score, double* norm_freq, double* norm_len, int32_t* kmer_breaks,
                               int32_t* seq_len, const u32* n_paths_p);
// outputs of table t at bp_score / norm_freq / norm_len + t * out_stride; kmer_breaks and seq_len once
template <int T>
__global__ void k_path_reduce(PathSet ps, const u32* poscnt, const u32* extra, ProbTables dprob, int kmer, double* bp_score, double* norm_freq,
                              double* norm_len, u64 out_stride, int32_t* kmer_breaks, int32_t* seq_len, u32 n_paths);
__global__ void k_path_freq(PathSet ps, const u32* poscnt, const u32* total, const int32_t* drow, int kmer, u32 n_table,
                            u32* freq_cnt, u32 n_paths);
__global__ void k_ks_genome_hist(const u64* gwords, u64 glen, int kmer, const int32_t* drow, u32* hist);
__global__ void k_path_ks(PathSet ps, const u32* poscnt, const int32_t* drow, int kmer, u32 n_table, const double* pv, const u32* cumy, u32* scratch,
                          double* out, u32 n_paths, const u32* list);
__global__ void k_path_ks2(PathSet ps, const u32* poscnt, const int32_t* drow, int kmer, u32 n_table, const double* pv, const u32* cumy, const u32* run_end,
                           u32* scratch, double* out, u32* flags, u32 n_paths, u32 bins);
__global__ void k_cover_mark(const long long* start, const long long* len, u64 n, long long seq_len, int* diff);
__global__ void k_cover_count(const int* diff, long long seq_len, unsigned long long* covered);
__global__ void k_prob_dist(PathSet ps, const double* dprob, int kmer, const u64* pd_off, double* out, u32 n_paths);

// ---- kernels_pool.hip: exchange plans (exchange.hip)
// the pinned report of an exchange plan among W ranks (u64 words; a rank keeps two of them back to back)
template <class T>
struct XReport {
    T* w;
    u32 W;
    __host__ __device__ T& send_tot(u32 d) const { return w[d]; }
    __host__ __device__ T& recv_tot(u32 d) const { return w[W + d]; }
    __host__ __device__ T& info(u32 j) const { return w[2 * W + j]; }      // 0: records the merge will hold in all; 1 (plan 2): the most of one segment
    __host__ __device__ T& flags() const { return w[2 * W + 4]; }          // OR of every rank's GASM_FLAG_OVERFLOW word
    __host__ __device__ T& ticket() const { return w[2 * W + 5]; }
    static size_t words(u32 W) { return 2 * (size_t)W + 6; }
};
__global__ void k_x_flag_word(const u32* flags, u32* row_tail);
__global__ void k_x1_plan(const u32* lens_all, u64 stride, u32 nbt, const u32* order, const u32* dst_first, const u32* mine, u32 n_mine, u32 W, u32 r, u32 limit,
                          u64* send_off, u64* send_tot, u64* run_off, u32* run_len, u64* recv_tot, u64* bstart, u32* flags_or);
__global__ void k_x2_fill(u32* G, u32 nbt, const u32* mine, u32 n_mine, const u32* bucket_d, const u32* flags);
__global__ void k_x2_plan(const u32* G, const u16* own1, u32 W, u32 r, u32 gb_lo, u32 n_out, int bbits, const u32* mine, u32 n_mine, const u32* seg_first,
                          u64* send_off, u64* send_tot, u64* run_off, u32* run_len, u64* recv_tot, u64* bstart, u64* info);
__global__ void k_x_report(const u64* send_tot, const u64* recv_tot, u32 W, const u64* info, u32 n_info, const u32* flags_or, u64* report, u64 ticket);
__global__ void k_x_add_u32(u32* acc, const u32* v, u64 n);
