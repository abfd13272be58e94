// pipeline.hip — host orchestration of the device pipeline.  All launches go to the ctx stream; the host only waits
// where a size is needed to allocate the next stage (distinct count, contig bytes) and at fetch time.
#include <atomic>
#include <chrono>
#include <thread>
#include "pipeline.h"

#include <algorithm>
#include <cmath>

// ---------------------------------------------------------------------------------------------------------------
// small local kernels
// ---------------------------------------------------------------------------------------------------------------
__global__ void k_set_u64(u64* p, u64 v) { *p = v; }

// empty reads match every path at position 0 (std::string::find("") == 0, lib/DeNovoAssembler.cpp:360)
__global__ void k_add_empty_reads(PathSet ps, const u64* __restrict__ seg_empty, u32* __restrict__ poscnt, u32* __restrict__ total) {
    const u32 seg = blockIdx.y;
    const u32 p = ps.seg_path_off[seg] + blockIdx.x * GASM_WG + threadIdx.x;
    if (p >= ps.seg_path_off[seg + 1]) return;
    const u32 e = (u32)seg_empty[seg];
    if (!e) return;
    if (ps.p_off[p + 1] > ps.p_off[p]) poscnt[ps.p_off[p]] += e;
    else total[p] += e;   // an empty path has no position counter: carried as an extra addend
}

// Tuning / diagnostic knobs, read from the environment once (none changes results):
//   GASM_DEDUP_TBL=2048|4096   force the de-duplication table size        GASM_SCATTER_WGS=n   scatter workgroups per CU (8)
//   GASM_HIST_WGS=n            histogram workgroups per CU (64)           GASM_DBG_BBITS_ADD=n extra bucket bits (tuning)
//   GASM_RULER_SHIFT=1..4      rulers of the LDS list ranking = every 2^n-th edge     GASM_RANK_GLOBAL=1   whole-GPU list ranking only
//   GASM_DBG_RANK_ROUNDS=n     cap the LDS ranking rounds (ablation)
//   GASM_SYNC_BUILD=1          every build waits for its own report (no queued-ahead builds)
struct Knobs {
    int dedup_tbl = 0, scatter_wgs = 8, hist_wgs = 64, rank_rounds = 18, bbits_add = 0, ruler_shift = 0;
    bool rank_global = false, sync_build = false;
    Knobs() {
        if (const char* v = getenv("GASM_DEDUP_TBL")) dedup_tbl = atoi(v);
        if (const char* v = getenv("GASM_SCATTER_WGS")) scatter_wgs = std::max(1, atoi(v));
        if (const char* v = getenv("GASM_HIST_WGS")) hist_wgs = std::max(1, atoi(v));
        if (const char* v = getenv("GASM_DBG_BBITS_ADD")) bbits_add = std::max(0, atoi(v));
        if (const char* v = getenv("GASM_RULER_SHIFT")) ruler_shift = std::min(4, std::max(0, atoi(v)));
        if (const char* v = getenv("GASM_DBG_RANK_ROUNDS")) rank_rounds = atoi(v);
        rank_global = getenv("GASM_RANK_GLOBAL") != nullptr;
        sync_build = getenv("GASM_SYNC_BUILD") != nullptr;       // wait for every build's report at once (diagnostic)
    }
};
static const Knobs& knobs() { static const Knobs k; return k; }
// knobs read at every build (tests switch them inside one process):
//   GASM_SINGLE_PASS=0     two-pass partition (count, scan, scatter) from the start       GASM_PART_SLACK=percent   room per bucket region (100)
//   GASM_DBG_PART_CAP=n    force the capacity of every bucket region to n keys (exercises the overflow path)
//   GASM_DBG_PART_GRID=n   at most n workgroups for k_bucket_partition (small batches: several tiles, and segments, per workgroup — the carry)
// and at every batch score through the graph (one table or several):
//   GASM_DBG_SCORE_LDS_PATHS=n   cap the paths per segment whose accumulators k_score_reads_graph keeps in LDS (segments
//                                with more go to global atomics: same numbers; exercises that branch)

// Wait for a report a kernel writes into pinned host memory: the kernel's last store is `ticket` at `word`.  Spinning on
// that word costs a few microseconds; waking up from hipStreamSynchronize costs 15-20 us (more on a busy host) — twice
// per build, with the GPU idle meanwhile.  After ~2 ms of spinning (a large batch) the thread polls the stream with short
// sleeps, up to a deadline (GASM_WAIT_TIMEOUT_S, default 300 s): a kernel that never finishes becomes an error, not a hang.
template <class T>
static int wait_word(gasm_ctx* ctx, const volatile T* word, T ticket) {
    const auto t0 = std::chrono::steady_clock::now();
    for (u32 spin = 0;; ++spin) {
        if (*word == ticket) { std::atomic_thread_fence(std::memory_order_acquire); return GASM_OK; }
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    static const double limit_s = [] { const char* v = getenv("GASM_WAIT_TIMEOUT_S"); const double x = v && *v ? atof(v) : 300.0; return x > 0 ? x : 300.0; }();
    for (;;) {
        if (*word == ticket) { std::atomic_thread_fence(std::memory_order_acquire); return GASM_OK; }
        const hipError_t q = hipStreamQuery(ctx->stream);
        if (q == hipSuccess) break;                       // the stream has drained: the report is there or never comes
        if (q != hipErrorNotReady) { gasm_set_error("the stream failed while a report was awaited: %s", hipGetErrorString(q)); return GASM_ERR_HIP; }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s) {
            gasm_set_error("no report from the device within %.0f s (GASM_WAIT_TIMEOUT_S): a kernel hangs or the GPU is lost", limit_s);
            return GASM_ERR_HIP;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    if (*word != ticket) { gasm_set_error("a kernel finished without writing its report"); return GASM_ERR_HIP; }
    std::atomic_thread_fence(std::memory_order_acquire);
    return GASM_OK;
}
int gasm_wait_word32(gasm_ctx* ctx, const volatile u32* word, u32 ticket) { return wait_word<u32>(ctx, word, ticket); }
int gasm_wait_word64(gasm_ctx* ctx, const volatile u64* word, u64 ticket) { return wait_word<u64>(ctx, word, ticket); }
static int wait_report(gasm_ctx* ctx, const volatile u32* word, u32 ticket) { return wait_word<u32>(ctx, word, ticket); }
static u32 next_ticket() { static std::atomic<u32> t{1}; u32 v = t.fetch_add(1); return v ? v : t.fetch_add(1); }

// grid of the segment-major kernels (seg_chunk, device_utils.h): 8 x chunks x ceil(S / 8) workgroups
static dim3 seg_grid(u32 chunks, u32 S) { return dim3(8u * chunks * ((S + 7u) / 8u)); }

int h2d(gasm_ctx* ctx, DBuf& b, const void* src, size_t bytes) {
    GCHK(b.ensure(bytes ? bytes : 8));
    if (bytes) HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return GASM_OK;
}

// Device -> host copy of a small array, then wait.  Goes through the ctx's pinned area (a pageable destination makes
// hipMemcpyAsync stage through the runtime and costs tens of microseconds more per call).
static int d2h_sync(gasm_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) { HIPCHK(hipStreamSynchronize(ctx->stream)); return GASM_OK; }
    if (bytes <= ctx->h_pin_words * sizeof(u64)) {
        HIPCHK(hipMemcpyAsync(ctx->h_pin, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        memcpy(dst, ctx->h_pin, bytes);
    } else {
        HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return GASM_OK;
}

static int pack_ascii(gasm_ctx* ctx, const u8* d_ascii, u64 nbases, DBuf& words, u32* d_err) {
    const u64 nw = (nbases + 31) / 32;
    GCHK(words.ensure((nw + 4) * 8));     // four zero padding words: a 128-bit rolling window reads up to three words ahead
    // (the kernel also writes the padding words: positions past the last base pack as zero)
    GLAUNCH(ctx, "k_pack_ascii", k_pack_ascii, dim3(std::min<u32>(ceil_div_u64(nw + 4, GASM_WG), (u32)ctx->n_cu * 32u)), dim3(GASM_WG), 0, d_ascii, nbases,
            (const u64*)nullptr, words.as<u64>(), d_err);
    return GASM_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// DevReads
// ---------------------------------------------------------------------------------------------------------------
// host-side layout of a batch's reads: per-segment directories, shortest / longest read, empty reads
int DevReads::set_layout(const u64* read_off, u64 n, u32 flen, const u64* seg_off, u32 S) {
    if (S == 0 || !seg_off) { gasm_set_error("need at least one segment and seg_read_off"); return GASM_ERR_INVALID; }
    if (S > 65535) { gasm_set_error("at most 65535 segments per batch (got %u)", S); return GASM_ERR_CAPACITY; }
    if (!read_off && flen == 0 && n) { gasm_set_error("give read_off or fixed_len"); return GASM_ERR_INVALID; }
    if (seg_off[0] != 0 || seg_off[S] != n) { gasm_set_error("seg_read_off must run from 0 to n_reads"); return GASM_ERR_INVALID; }
    for (u32 s = 0; s < S; ++s) if (seg_off[s] > seg_off[s + 1]) { gasm_set_error("seg_read_off not monotone"); return GASM_ERR_INVALID; }
    n_segments = S; n_reads = n; fixed_len = read_off ? 0 : flen;
    positioned = false;
    h_seg_read_off.assign(seg_off, seg_off + S + 1);
    h_seg_empty.assign(S, 0);
    n_empty = 0; min_len = 0; max_len = 0;
    if (read_off) {
        h_read_off.resize(n + 1);
        for (u64 r = 0; r <= n; ++r) {
            if (r && read_off[r] < read_off[r - 1]) { gasm_set_error("read_off not monotone"); return GASM_ERR_INVALID; }
            h_read_off[r] = read_off[r] - read_off[0];
        }
        total_bases = h_read_off[n];
        u32 s = 0;
        for (u64 r = 0; r < n; ++r) {
            while (r >= h_seg_read_off[s + 1]) ++s;
            const u64 L = h_read_off[r + 1] - h_read_off[r];
            if (L > 0xFFFFFFFFull) { gasm_set_error("read longer than 2^32"); return GASM_ERR_CAPACITY; }
            if (L == 0) { ++n_empty; ++h_seg_empty[s]; continue; }
            if (min_len == 0 || L < min_len) min_len = (u32)L;
            if (L > max_len) max_len = (u32)L;
        }
    } else {
        h_read_off.clear();
        total_bases = n * (u64)flen;
        if (n) { min_len = max_len = flen; }
    }
    return GASM_OK;
}

int DevReads::finish_upload(gasm_ctx* ctx) {
    if (!fixed_len) GCHK(h2d(ctx, d_read_off, h_read_off.data(), (n_reads + 1) * 8));
    GCHK(h2d(ctx, d_seg_read_off, h_seg_read_off.data(), ((size_t)n_segments + 1) * 8));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    tiles_ipt = 0;
    static std::atomic<u64> uploads{0};
    upload_id = ++uploads;
    return GASM_OK;
}

int DevReads::upload(gasm_ctx* ctx, const char* reads, const u64* read_off, u64 n, u32 flen, const u64* seg_off, u32 S) {
    if (!ctx) { gasm_set_error("ctx is null"); return GASM_ERR_INVALID; }
    GCHK(set_layout(read_off, n, flen, seg_off, S));
    HIPCHK(hipSetDevice(ctx->device));
    const char* base = read_off ? reads + read_off[0] : reads;
    if (n && !reads && total_bases) { gasm_set_error("reads is null"); return GASM_ERR_INVALID; }
    DBuf ascii, err;
    struct Rel { DBuf &a, &b; ~Rel() { a.release(); b.release(); } } rel{ascii, err};      // (also on the early returns below)
    GCHK(err.ensure(8));
    HIPCHK(hipMemsetAsync(err.p, 0, 8, ctx->stream));
    GCHK(h2d(ctx, ascii, base, total_bases));
    int st = pack_ascii(ctx, ascii.as<u8>(), total_bases, d_words, err.as<u32>());
    u32 herr = 0;
    if (st == GASM_OK && hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) st = GASM_ERR_HIP;
    if (st == GASM_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { gasm_set_error("sync failed after packing"); st = GASM_ERR_HIP; }
    ascii.release(); err.release();
    if (st != GASM_OK) return st;
    if (herr) { gasm_set_error("reads contain a base outside upper-case ACGT"); return GASM_ERR_NON_ACGT; }
    return finish_upload(ctx);
}

// Reads that are 2-bit packed already (first base most significant, 32 per word, back to back): a quarter of the bytes over
// PCIe, no packing kernel.  Bits past the last base are ignored.
int DevReads::upload_packed(gasm_ctx* ctx, const u64* words, const u64* read_off, u64 n, u32 flen, const u64* seg_off, u32 S) {
    if (!ctx) { gasm_set_error("ctx is null"); return GASM_ERR_INVALID; }
    GCHK(set_layout(read_off, n, flen, seg_off, S));
    if (read_off && read_off[0] != 0) { gasm_set_error("packed reads: read_off must start at 0"); return GASM_ERR_INVALID; }
    if (total_bases && !words) { gasm_set_error("words is null"); return GASM_ERR_INVALID; }
    HIPCHK(hipSetDevice(ctx->device));
    const u64 nw = (total_bases + 31) / 32;
    GCHK(d_words.ensure((nw + 4) * 8));
    if (nw) HIPCHK(hipMemcpyAsync(d_words.p, words, nw * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(static_cast<char*>(d_words.p) + nw * 8, 0, 32, ctx->stream));
    if (nw && (total_bases & 31)) {
        // the tail of the last word must be zero (windows read past the last base)
        const u64 last = words[nw - 1] & (~0ull << (64 - 2 * (total_bases & 31)));
        HIPCHK(hipMemcpyAsync(static_cast<char*>(d_words.p) + (nw - 1) * 8, &last, 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return finish_upload(ctx);
}

// Reads packed on the device already (ingest.hip): the stream is taken over as it is (zero beyond its last base, padding words
// included); only the directories come from the host.
int DevReads::adopt_packed(gasm_ctx* ctx, DBuf& words_dev, const u64* read_off, u64 n, u32 flen, const u64* seg_off, u32 S) {
    if (!ctx) { gasm_set_error("ctx is null"); return GASM_ERR_INVALID; }
    GCHK(set_layout(read_off, n, flen, seg_off, S));
    HIPCHK(hipSetDevice(ctx->device));
    const u64 nw = (total_bases + 31) / 32;
    if (words_dev.cap < (nw + 4) * 8) { gasm_set_error("adopt_packed: the stream is shorter than its directories say"); return GASM_ERR_INVALID; }
    d_words.release();
    std::swap(d_words, words_dev);
    return finish_upload(ctx);
}

// ---------------------------------------------------------------------------------------------------------------
// Simulated reads, made on the device (kernels_sim.hip; lib/GenerateReads.R:235-313)
// ---------------------------------------------------------------------------------------------------------------
int DevReads::simulate(gasm_ctx* ctx, const char* genomes, const u64* genome_off, u32 S, u32 read_len, double coverage, u64 seed, int kmer,
                       const double* table, DBuf& d_kept_start) {
    if (!ctx || !genome_off || S == 0) { gasm_set_error("simulate: bad argument"); return GASM_ERR_INVALID; }
    if (read_len == 0 || !(coverage >= 0.0) || kmer < 1 || kmer > 8) { gasm_set_error("simulate: read_len > 0, coverage >= 0, 1 <= kmer <= 8"); return GASM_ERR_INVALID; }
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<u64> gbase((size_t)S + 1), glen(S), woff((size_t)S + 1, 0), doff((size_t)S + 1, 0);
    u64 max_np = 0, max_nd = 0;
    for (u32 s = 0; s <= S; ++s) {
        if (s && genome_off[s] < genome_off[s - 1]) { gasm_set_error("genome_off not monotone"); return GASM_ERR_INVALID; }
        gbase[s] = genome_off[s] - genome_off[0];
    }
    for (u32 s = 0; s < S; ++s) {
        const u64 L = gbase[s + 1] - gbase[s];
        if (L > 0xFFFFFFF0ull) { gasm_set_error("genome longer than 2^32"); return GASM_ERR_CAPACITY; }
        glen[s] = L;
        const u64 np = L >= (u64)kmer ? L - kmer + 1 : 0;                                // lib/GenerateReads.R:243
        const u64 nd = np ? (u64)std::ceil(coverage * (double)L / (double)read_len) : 0;   // :302
        woff[s + 1] = woff[s] + np;
        doff[s + 1] = doff[s] + nd;
        max_np = std::max(max_np, np); max_nd = std::max(max_nd, nd);
    }
    DBuf ascii, err, gwords, d_gbase, d_glen, d_woff, d_doff, d_w, d_fix, d_start, d_keep, d_rank, d_sro;
    struct Rel { std::vector<DBuf*> v; ~Rel() { for (DBuf* b : v) b->release(); } } rel{{&ascii, &err, &gwords, &d_gbase, &d_glen, &d_woff, &d_doff, &d_w, &d_fix,
                                                                                         &d_start, &d_keep, &d_rank, &d_sro}};
    GCHK(err.ensure(8));
    HIPCHK(hipMemsetAsync(err.p, 0, 8, ctx->stream));
    GCHK(h2d(ctx, ascii, genomes + genome_off[0], gbase[S]));
    GCHK(pack_ascii(ctx, ascii.as<u8>(), gbase[S], gwords, err.as<u32>()));
    GCHK(h2d(ctx, d_gbase, gbase.data(), gbase.size() * 8));
    GCHK(h2d(ctx, d_glen, glen.data(), glen.size() * 8));
    GCHK(h2d(ctx, d_woff, woff.data(), woff.size() * 8));
    GCHK(h2d(ctx, d_doff, doff.data(), doff.size() * 8));
    const long long* fixw = nullptr;
    if (table) {
        // the kmer-long rows of the standard table (rows of lengths 2, 4, 6, 8 in that order), direct-addressed, in fixed point
        if (kmer != 2 && kmer != 4 && kmer != 6 && kmer != 8) { gasm_set_error("the weighted simulator needs kmer in {2,4,6,8} (the table's row lengths)"); return GASM_ERR_INVALID; }
        // fixed-point weights round(p * 2^shift), running sums in 64 bits: shift = 52 unless a segment's sum could then pass
        // 2^62 (kmer = 2 on a genome of more than ~65 kb: the sum used to wrap and k_sim_draw bisected a non-monotone CDF) —
        // then the largest shift that cannot.  The oracle takes the same shift (sim_weight_shift, oracle/orc.py)
        std::vector<long long> fx(87380, 0);
        double max_p = 0;
        {
            u32 src = 0;
            for (u32 Lk = 2; Lk <= 8; Lk += 2) {
                const u32 n = 1u << (2 * Lk);
                for (u32 v = 0; v < n; ++v, ++src) if ((int)Lk == kmer) max_p = std::max(max_p, table[src]);
            }
        }
        int shift = 52;
        while (shift > 0 && std::ldexp(max_p, shift) * (double)std::max<u64>(max_np, 1) >= 4611686018427387904.0) --shift;
        sim_shift = shift;
        u32 src = 0;
        for (u32 Lk = 2; Lk <= 8; Lk += 2) {
            const u32 n = 1u << (2 * Lk), b = ((1u << (2 * Lk)) - 4u) / 3u;
            for (u32 v = 0; v < n; ++v, ++src) if ((int)Lk == kmer) fx[b + v] = std::llrint(std::ldexp(table[src], shift));
        }
        GCHK(h2d(ctx, d_fix, fx.data(), fx.size() * 8));
        fixw = d_fix.as<long long>();
    }
    GCHK(d_w.ensure(std::max<u64>(woff[S], 1) * 8));
    GCHK(d_start.ensure(std::max<u64>(doff[S], 1) * 4));
    GCHK(d_keep.ensure(std::max<u64>(doff[S], 1) * 4));
    GCHK(d_rank.ensure(std::max<u64>(doff[S], 1) * 4));
    const u32 gx_p = std::max(1u, std::min<u32>(ceil_div_u64(std::max<u64>(max_np, 1), GASM_WG), 64u));
    const u32 gx_d = std::max(1u, std::min<u32>(ceil_div_u64(std::max<u64>(max_nd, 1), GASM_WG), 64u));
    GLAUNCH(ctx, "k_sim_weights", k_sim_weights, dim3(gx_p, S), dim3(GASM_WG), 0, gwords.as<u64>(), d_gbase.as<u64>(), d_woff.as<u64>(), S, kmer, fixw, d_w.as<u64>());
    GLAUNCH(ctx, "k_seg_scan_incl", k_seg_scan_incl<u64>, dim3(S), dim3(1024), 0, d_w.as<u64>(), d_woff.as<u64>());
    GLAUNCH(ctx, "k_sim_draw", k_sim_draw, dim3(gx_d, S), dim3(GASM_WG), 0, d_w.as<u64>(), d_woff.as<u64>(), d_doff.as<u64>(), d_glen.as<u64>(), seed, read_len,
            d_start.as<u32>(), d_keep.as<u32>());
    if (doff[S]) HIPCHK(hipMemcpyAsync(d_rank.p, d_keep.p, doff[S] * 4, hipMemcpyDeviceToDevice, ctx->stream));
    GLAUNCH(ctx, "k_seg_scan_incl", k_seg_scan_incl<u32>, dim3(S), dim3(1024), 0, d_rank.as<u32>(), d_doff.as<u64>());
    // kept reads per segment = the last rank of the segment (one small kernel + one copy, not a copy per segment)
    std::vector<u32> last(S, 0);
    u32 herr = 0;
    GCHK(d_sro.ensure((size_t)S * 4 + 8));
    GLAUNCH(ctx, "k_slice_last", k_slice_last, dim3(ceil_div_u64(S, GASM_WG)), dim3(GASM_WG), 0, d_rank.as<u32>(), d_doff.as<u64>(), S, d_sro.as<u32>());
    HIPCHK(hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(last.data(), d_sro.p, (size_t)S * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (herr) { gasm_set_error("a genome holds a base outside upper-case ACGT"); return GASM_ERR_NON_ACGT; }
    std::vector<u64> sro((size_t)S + 1, 0);
    for (u32 s = 0; s < S; ++s) sro[s + 1] = sro[s] + last[s];
    const u64 n = sro[S];
    GCHK(set_layout(nullptr, n, read_len, sro.data(), S));
    GCHK(h2d(ctx, d_sro, sro.data(), sro.size() * 8));
    GCHK(d_kept_start.ensure(std::max<u64>(n, 1) * 4));
    GLAUNCH(ctx, "k_sim_compact", k_sim_compact, dim3(gx_d, S), dim3(GASM_WG), 0, d_start.as<u32>(), d_keep.as<u32>(), d_rank.as<u32>(), d_doff.as<u64>(), d_sro.as<u64>(),
            d_kept_start.as<u32>());
    const u64 nw = (total_bases + 31) / 32;
    GCHK(d_words.ensure((nw + 4) * 8));
    HIPCHK(hipMemsetAsync(d_words.p, 0, (nw + 4) * 8, ctx->stream));
    if (n) GLAUNCH(ctx, "k_sim_extract", k_sim_extract, dim3(std::max(1u, std::min<u32>(ceil_div_u64(max_nd * ((read_len + 31) / 32), GASM_WG), 256u)), S), dim3(GASM_WG), 0,
                   gwords.as<u64>(), d_gbase.as<u64>(), d_sro.as<u64>(), d_kept_start.as<u32>(), read_len, d_words.as<unsigned long long>());
    return finish_upload(ctx);
}

// Tile table: a tile = up to ipt consecutive reads of one segment at one of orr offset rounds (kernels_build.hip, "Tiles").
// The table is shared by every step slot of the batch, and a slot whose build finds it cached waits for nothing on the
// uploading slot's stream: so an upload (first build, or a new tile geometry) is complete before this returns.
int DevReads::set_tiles(gasm_ctx* ctx, u32 ipt, u32 orr) {
    if (tiles_ipt == ipt && tiles_orr == orr) return GASM_OK;
    std::vector<u32>& t = h_seg_tile_start;
    t.assign(n_segments + 1, 0);
    for (u32 s = 0; s < n_segments; ++s) {
        const u64 rs = h_seg_read_off[s + 1] - h_seg_read_off[s];
        const u64 nt = (rs + ipt - 1) / ipt * orr;
        if ((u64)t[s] + nt > 0xFFFFFFF0ull) { gasm_set_error("too many tiles"); return GASM_ERR_CAPACITY; }
        t[s + 1] = t[s] + (u32)nt;
    }
    GCHK(h2d(ctx, d_seg_tile_start, t.data(), t.size() * 4));
    n_tiles = t[n_segments];
    std::vector<u32>& info = h_tile_info;
    info.assign((size_t)n_tiles * 4 + 4, 0);
    for (u32 s = 0; s < n_segments; ++s)
        for (u32 tile = t[s]; tile < t[s + 1]; ++tile) {
            const u32 grp = (tile - t[s]) / orr, o = (tile - t[s]) % orr;
            const u64 first = h_seg_read_off[s] + (u64)grp * ipt;
            const u64 left = h_seg_read_off[s + 1] - first;
            if ((first >> 48) != 0) { gasm_set_error("too many reads"); return GASM_ERR_CAPACITY; }
            u32* e = &info[(size_t)tile * 4];
            e[0] = s; e[1] = (u32)std::min<u64>(left, ipt); e[2] = (u32)first; e[3] = (u32)(first >> 32) | (o << 16);
        }
    GCHK(h2d(ctx, d_tile_info, info.data(), info.size() * 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    tiles_ipt = ipt;
    tiles_orr = orr;
    return GASM_OK;
}

// Both strands: the reads of `src` and their reverse complements as a read set of its own, segment by segment (forward reads,
// then their reverse complements in the same order).  Like the tile table it is shared read-only by every step slot of a
// batch, so it is complete — stream and directories — before this returns.
int DevReads::make_both_strands(gasm_ctx* ctx, const DevReads& src) {
    if (src.positioned) { gasm_set_error("both-strand builds of pooled reads are not supported"); return GASM_ERR_STATE; }
    HIPCHK(hipSetDevice(ctx->device));
    const u32 S = src.n_segments;
    const u64 n = src.n_reads;
    std::vector<u64> seg2((size_t)S + 1), off2;
    for (u32 s = 0; s <= S; ++s) seg2[s] = 2 * src.h_seg_read_off[s];
    if (!src.fixed_len) {
        off2.resize(2 * n + 1);
        u64 at = 0, w = 0;
        off2[0] = 0;
        for (u32 s = 0; s < S; ++s)
            for (int pass = 0; pass < 2; ++pass)
                for (u64 r = src.h_seg_read_off[s]; r < src.h_seg_read_off[s + 1]; ++r) { at += src.h_read_off[r + 1] - src.h_read_off[r]; off2[++w] = at; }
    }
    GCHK(set_layout(src.fixed_len ? nullptr : off2.data(), 2 * n, src.fixed_len, seg2.data(), S));
    const u64 nw = (total_bases + 31) / 32;
    GCHK(d_words.ensure((nw + 4) * 8));
    HIPCHK(hipMemsetAsync(d_words.p, 0, (nw + 4) * 8, ctx->stream));
    if (n && src.total_bases) {
        // threads per read: a power of two that covers the longest read's 32-base pieces, 64 at most (longer reads: rounds)
        const u32 g = std::min(64u, next_pow2_u32((src.max_len + 31) / 32));
        const u32 grid = (u32)std::min<u64>((n * g + GASM_WG - 1) / GASM_WG, (u64)ctx->n_cu * 64);
        GLAUNCH(ctx, "k_reads_both_strands", k_reads_both_strands, dim3(std::max(1u, grid)), dim3(GASM_WG), 0, src.d_words.as<u64>(),
                src.fixed_len ? (const u64*)nullptr : src.d_read_off.as<u64>(), src.d_seg_read_off.as<u64>(), src.fixed_len, S, n, g,
                d_words.as<unsigned long long>());
    }
    GCHK(finish_upload(ctx));           // (directories up, stream drained, an upload_id of its own)
    strands_of = src.upload_id;
    return GASM_OK;
}

ReadSet DevReads::view() const {
    ReadSet v;
    v.words = d_words.as<u64>();
    v.read_off = (fixed_len && !positioned) ? nullptr : d_read_off.as<u64>();
    v.seg_read_off = d_seg_read_off.as<u64>();
    v.seg_tile_start = d_seg_tile_start.as<u32>();
    v.tile_info = d_tile_info.as<uint4>();
    v.fixed_len = fixed_len;
    v.n_segments = n_segments;
    return v;
}

void DevReads::release() { d_words.release(); d_read_off.release(); d_seg_read_off.release(); d_seg_tile_start.release(); d_tile_info.release(); }

// ---------------------------------------------------------------------------------------------------------------
// DevPaths
// ---------------------------------------------------------------------------------------------------------------
int DevPaths::upload_dirs(gasm_ctx* ctx) {
    GCHK(h2d(ctx, d_p_off, h_p_off.data(), h_p_off.size() * 8));
    GCHK(h2d(ctx, d_seg_path_off, h_seg_path_off.data(), h_seg_path_off.size() * 4));
    std::vector<u64>& sb = h_seg_base_off;
    sb.resize(n_segments + 1);
    for (u32 s = 0; s <= n_segments; ++s) sb[s] = h_p_off[h_seg_path_off[s]];
    GCHK(h2d(ctx, d_seg_base_off, sb.data(), sb.size() * 8));
    return GASM_OK;
}

int DevPaths::pack_from_device_ascii(gasm_ctx* ctx, const u8* d_ascii) {
    DBuf err;
    GCHK(err.ensure(8));
    HIPCHK(hipMemsetAsync(err.p, 0, 8, ctx->stream));
    int st = pack_ascii(ctx, d_ascii, total_bases, d_words, err.as<u32>());
    u32 herr = 0;
    if (st == GASM_OK && hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) st = GASM_ERR_HIP;
    if (st == GASM_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = GASM_ERR_HIP;
    err.release();
    if (st != GASM_OK) return st;
    if (herr) { gasm_set_error("paths contain a base outside upper-case ACGT"); return GASM_ERR_NON_ACGT; }
    return GASM_OK;
}

int DevPaths::upload_ascii(gasm_ctx* ctx, const char* data, const u64* off, u32 np) {
    n_segments = 1; n_paths = np;
    b_p_off = nullptr; b_seg_path_off = nullptr; b_seg_base_off = nullptr;
    h_p_off.resize((size_t)np + 1);
    for (u32 i = 0; i <= np; ++i) {
        if (i && off[i] < off[i - 1]) { gasm_set_error("path offsets not monotone"); return GASM_ERR_INVALID; }
        h_p_off[i] = off[i] - off[0];
    }
    total_bases = h_p_off[np];
    if (total_bases >= 0xFFFFFFF0ull) { gasm_set_error("paths exceed 2^32 bases"); return GASM_ERR_CAPACITY; }
    h_seg_path_off = {0u, np};
    DBuf ascii;
    GCHK(h2d(ctx, ascii, data + off[0], total_bases));
    int st = pack_from_device_ascii(ctx, ascii.as<u8>());
    ascii.release();
    GCHK(st);
    return upload_dirs(ctx);
}

PathSet DevPaths::view() const {
    PathSet v;
    v.words = d_words.as<u64>();
    v.p_off = b_p_off ? b_p_off : d_p_off.as<u64>();
    v.seg_path_off = b_seg_path_off ? b_seg_path_off : d_seg_path_off.as<u32>();
    v.n_segments = n_segments;
    return v;
}

void DevPaths::release() { d_words.release(); d_p_off.release(); d_seg_path_off.release(); d_seg_base_off.release(); }

void BuildState::release() {
    for (DBuf* b : {&d_solid_removed, &d_ccov, &links.d, &pairs.d, &map.d, &mapg.d, &mapscore.d, &d_spectrum, &d_twin, &d_keys, &d_keys2, &d_mult, &d_hist, &d_toff, &d_tcnt, &d_fdir, &d_bstart, &d_bucket_d, &d_dstart, &d_flags, &d_dk_key, &d_dk_cnt,
                    &d_eflag, &d_nxt, &d_link, &d_clen, &d_ecid, &d_ecoff, &d_rtab, &d_seg_cbases, &d_seg_cstart,
                    &d_seg_bstart, &d_c_off, &d_contig_ascii})
        b->release();
    for (RoundStats& rs : round_stats) rs.d_stats.release();
    part_valid = false;         // (d_bstart no longer holds the partition's region layout)
    if (h_report) { (void)hipHostFree(h_report); h_report = nullptr; h_report_words = 0; }
}

void ScoreState::release() {
    for (DBuf* b : {&d_tbl_off, &d_seed, &d_gpos, &d_poscnt, &d_total, &d_out_f64, &d_out_i32, &d_freq, &d_pd_off, &d_pd, &d_seg_empty, &d_fxsum, &d_first, &d_first_off}) b->release();
}

// ---------------------------------------------------------------------------------------------------------------
// build.  The host queues a whole build — k-mers -> buckets -> distinct k-mers -> graph -> contigs — without waiting for
// any size: arrays are allocated at upper bounds known from the reads (288 GB of HBM are there for this), grids come from
// estimates with the kernels looping over what is really there, and the last kernel writes every size the host will
// need, plus the failure flags, into the batch's pinned report.  pipeline_build_finish reads it when results are asked
// for; a build that tripped a flag (a bucket's table overflowed, list ranking's LDS estimate was too small) is repeated
// with the next larger configuration there.  So a step of a resident pipeline (build + score, fetch much later) never
// stalls the stream.
// ---------------------------------------------------------------------------------------------------------------
static int ensure_lds_attrs(gasm_ctx* ctx) {
    if (ctx->lds_attrs_set) return GASM_OK;         // per context = per device: the attribute is a property of the device's code object
#define GASM_LDS_ATTR(kern, bytes) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
#define GASM_SCORE_LDS_ATTR(T) GASM_LDS_ATTR((k_score_reads_graph<K, T>), GASM_SCORE_PATH_CAP * 12)
    for (int words = 1; words <= 2; ++words)
        GCHK(with_key(words, [&](auto tag) -> int {
            using K = typename decltype(tag)::type;
            GASM_LDS_ATTR(k_bucket_scatter<K>, 160 * 1024) GASM_LDS_ATTR(k_bucket_partition<K>, 160 * 1024) GASM_LDS_ATTR(k_tile_hist<K>, 160 * 1024)
            GASM_SCORE_LDS_ATTR(1) GASM_SCORE_LDS_ATTR(2) GASM_SCORE_LDS_ATTR(3) GASM_SCORE_LDS_ATTR(4) GASM_SCORE_LDS_ATTR(5) GASM_SCORE_LDS_ATTR(6) GASM_SCORE_LDS_ATTR(7) GASM_SCORE_LDS_ATTR(8)
            return GASM_OK;
        }));
    GASM_LDS_ATTR(k_rank_lds, 160 * 1024 - 64)
#define GASM_MAPSCORE_LDS_ATTR(T) GASM_LDS_ATTR((k_score_mapped<T, false>), GASM_SCORE_PATH_CAP * 12) GASM_LDS_ATTR((k_score_mapped<T, true>), GASM_SCORE_PATH_CAP * 12)
    GASM_MAPSCORE_LDS_ATTR(1) GASM_MAPSCORE_LDS_ATTR(2) GASM_MAPSCORE_LDS_ATTR(3) GASM_MAPSCORE_LDS_ATTR(4) GASM_MAPSCORE_LDS_ATTR(5) GASM_MAPSCORE_LDS_ATTR(6)
    GASM_MAPSCORE_LDS_ATTR(7) GASM_MAPSCORE_LDS_ATTR(8)
#undef GASM_MAPSCORE_LDS_ATTR
#undef GASM_SCORE_LDS_ATTR
#undef GASM_LDS_ATTR
    ctx->lds_attrs_set = true;
    return GASM_OK;
}

// upper bound of the distinct k-mers of the segments, given the partition: a bucket holds at most `limit` (else it overflows)
void distinct_caps(BuildState& bs, u32 S) {
    const u64 limit = bs.multi_pass ? GASM_BUCKET_MAX : bs.small_tbl ? GASM_TBL_LIMIT / 2 : GASM_TBL_LIMIT;
    const u64 per_seg = ((u64)1 << bs.bbits) * limit;
    const u64 all = bs.k < 16 ? ((u64)1 << (2 * bs.k)) : ~(u64)0;     // 4^k different k-mers exist
    bs.D_cap = 0; bs.maxD_cap = 0;
    for (u32 s = 0; s < S; ++s) {
        const u64 c = std::min(std::min(bs.h_seg_nk[s], per_seg), all);
        bs.D_cap += c;
        bs.maxD_cap = std::max(bs.maxD_cap, c);
    }
}

static int launch_graph_dense(gasm_ctx* ctx, u32 S, BuildState& bs, bool last_pass);

static GraphView graph_view(const BuildState& bs) {
    GraphView gv;
    gv.dk_key = bs.d_dk_key.p;
    gv.dstart = bs.d_dstart.as<u32>();
    gv.fdir = bs.d_fdir.as<u16>();
    gv.k = bs.k;
    gv.bbits = bs.bbits;
    gv.fbits = bs.fbits;
    return gv;
}

// does the finished build hold a contig (and so the arrays of a ContigIndex)?
static bool have_contigs(const BuildState& bs) { return bs.n_contigs && bs.d_total && bs.n_kmers; }

static ContigIndex contig_index(const BuildState& bs) {
    return ContigIndex{bs.d_link.as<u64>(), bs.d_ecid.as<u32>(), bs.d_c_off.as<u64>(), bs.d_seg_cstart.as<u32>(), bs.d_contig_ascii.as<u8>(), have_contigs(bs) ? 1 : 0};
}

// k_bucket_dedup over the key width and the table size of `bs`: 64-bit keys have both tables, 128-bit keys the small one
template <class K, int TBL>
static int launch_bucket_dedup_as(gasm_ctx* ctx, BuildState& bs, u32 nbt, const u32* d_blen, u32* d_scan_out) {
    GLAUNCH(ctx, "k_bucket_dedup", (k_bucket_dedup<K, TBL>), dim3(nbt), dim3(GASM_WG), 0, bs.d_keys.as<K>(), bs.d_mult.as<u32>(), bs.d_bstart.as<u64>(), d_blen,
            bs.d_bucket_d.as<u32>(), bs.d_flags.as<u32>(), bs.d_fdir.as<u16>(), 2 * bs.k - bs.bbits, d_scan_out);
    return GASM_OK;
}
static int launch_bucket_dedup(gasm_ctx* ctx, BuildState& bs, u32 nbt, const u32* d_blen, u32* d_scan_out) {
    if (bs.words == 2) return launch_bucket_dedup_as<K128, 2048>(ctx, bs, nbt, d_blen, d_scan_out);
    if (bs.small_tbl) return launch_bucket_dedup_as<u64, 2048>(ctx, bs, nbt, d_blen, d_scan_out);
    return launch_bucket_dedup_as<u64, 4096>(ctx, bs, nbt, d_blen, d_scan_out);
}

// ---- reads -> per-(segment, bucket) distinct k-mers with multiplicities (in place in d_keys / d_mult) + dstart
int launch_distinct(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    GasmRange range("gasm:distinct (partition + de-duplication)");
    const int k = bs.k, W = bs.words, bbits = bs.bbits;
    const size_t KB = 8 * (size_t)W;
    const u32 S = rd.n_segments, nb = 1u << bbits, nbt = S * nb;
    const u64 N = bs.n_kmers;
    // every (tile, bucket) run is padded to a multiple of padm + 1 keys (a 128-byte line when the bucket count allows;
    // the padding of one tile must fit the flush passes k_bucket_scatter has beyond KT)
    const u32 line_keys = 128 / KB;
    const u32 pad_room = (u32)with_key(W, [](auto tag) -> int { return TileStage<typename decltype(tag)::type>::PAD_ROOM; });
    u32 padm = line_keys - 1;                 // a mask: 2^n - 1
    // (128-bit keys: + 1, so that k_bucket_partition has a thread for every key of a bucket's unfinished line — nb * (padm + 1)
    // <= GASM_TILE_WG; with 64-bit keys a thread takes two, and nb <= GASM_TILE_WG buckets keep that within the workgroup)
    while (padm && (u64)nb * (padm + (W == 2 ? 1u : 0u)) > pad_room) padm >>= 1;
    const ReadSet rs = rd.view();
    const u32 g = bs.tile_g;
    const u32 grid_tiles = std::min<u32>(rd.n_tiles, (u32)ctx->n_cu * (u32)knobs().hist_wgs);
    const u32 scratch_keys = GASM_FLUSH_SLOTS * (16 / KB);      // the flush's scratch line behind the keys: 16 bytes per slot (kernels.h)
    GCHK(bs.d_bstart.ensure(((size_t)nbt + 1) * 8));
    GCHK(bs.d_bucket_d.ensure((size_t)nbt * 4));
    GCHK(bs.d_dstart.ensure(((size_t)nbt + 2) * 4));
    u64 n_alloc;
    const u32* d_blen = nullptr;              // single pass: the buckets' padded lengths (the partition's cursors)
    const bool single = bs.single_pass && !bs.multi_pass && nb <= GASM_TILE_WG;
    bs.part_single = single;
    if (single) {
        // ---- one pass (k_bucket_partition): a region of fixed capacity per (segment, bucket) — the segment's k-mers per
        // bucket with `part_slack` percent to spare, room for Poisson noise and for the padding of its tiles' runs, in whole
        // lines — and a cursor per region behind the build's flag words
        const int slack = env_int("GASM_PART_SLACK", 100), forced = env_int("GASM_DBG_PART_CAP", 0);
        BuildState::PartLayout layout;
        layout.reads_id = rd.upload_id; layout.k = k; layout.bbits = bbits; layout.slack = slack; layout.forced = forced; layout.padm = padm; layout.g = g;
        if (!(bs.part_valid && bs.part == layout)) {
            std::vector<u64> h((size_t)nbt + 1);
            u64 at = 0;
            for (u32 s = 0; s < S; ++s) {
                const u64 mean = ceil_div_u64(bs.h_seg_nk[s], nb), tiles = rd.h_seg_tile_start[s + 1] - rd.h_seg_tile_start[s];
                u64 cap = mean + (u64)((double)mean * std::max(slack, 0) / 100.0) + (u64)(8.0 * std::sqrt((double)mean)) + 32 + tiles * padm;
                if (forced > 0) cap = (u64)forced;
                cap = (cap + line_keys - 1) / line_keys * line_keys;
                for (u32 b = 0; b < nb; ++b) { h[(size_t)s * nb + b] = at; at += cap; }
            }
            h[nbt] = at;
            bs.part_alloc = at;
            GCHK(h2d(ctx, bs.d_bstart, h.data(), h.size() * 8));
            HIPCHK(hipStreamSynchronize(ctx->stream));          // (`h` goes out of scope; only when the batch shape changes)
            bs.part_valid = true;
            bs.part = layout;
        }
        n_alloc = bs.part_alloc;
        GCHK(bs.d_keys.ensure((n_alloc + scratch_keys) * KB));
        GCHK(bs.d_mult.ensure(n_alloc * 4));
        GCHK(bs.d_flags.ensure(GASM_FLAG_BYTES + (size_t)nbt * 4));
        HIPCHK(hipMemsetAsync(bs.d_flags.p, 0, GASM_FLAG_BYTES + (size_t)nbt * 4, ctx->stream));
        u32* const d_cursor = bs.d_flags.as<u32>() + GASM_FLAG_CURSORS;
        d_blen = d_cursor;
        u32 grid_part = std::min<u32>(rd.n_tiles, (u32)ctx->n_cu * (u32)knobs().scatter_wgs);
        if (const int cap = env_int("GASM_DBG_PART_GRID", 0)) grid_part = std::min<u32>(grid_part, (u32)std::max(1, cap));
        GLAUNCH_K(ctx, W, "k_bucket_partition", k_bucket_partition<K>, dim3(grid_part), dim3(GASM_TILE_WG), PartitionLds<K>{nb}.total(), rs, rs.tile_info, k, bbits, g, padm, rd.n_tiles,
                  bs.d_bstart.as<u64>(), d_cursor, bs.d_keys.as<K>(), n_alloc, bs.d_flags.as<u32>());
    } else {
        // ---- two passes: count, scan, scatter (exact layout; the retry path of the single pass, > 512 buckets, multi-pass builds)
        bs.part_valid = false;                // (k_scan_excl overwrites d_bstart)
        GCHK(bs.d_hist.ensure((size_t)nbt * 4));
        GCHK(bs.d_toff.ensure((size_t)rd.n_tiles * nb * 4));
        n_alloc = N + (u64)padm * rd.n_tiles * nb;
        GCHK(bs.d_keys.ensure((n_alloc + scratch_keys) * KB));
        GCHK(bs.d_mult.ensure(n_alloc * 4));
        GCHK(bs.d_tcnt.ensure((size_t)rd.n_tiles * nb * 8 + 64));      // four 16-bit sub-counts per (tile, bucket)
        GLAUNCH_K(ctx, W, "k_tile_hist", k_tile_hist<K>, dim3(grid_tiles), dim3(GASM_TILE_WG), (size_t)nb * 16, rs, rs.tile_info, k, bbits, g, rd.n_tiles,
                  bs.d_tcnt.as<ushort4>());
        GLAUNCH(ctx, "k_tile_scan", k_tile_scan, dim3(S, std::max(1u, nb / 32u)), dim3(1024), 0, rs, bbits, padm, bs.d_tcnt.as<ushort4>(),
                bs.d_toff.as<u32>(), bs.d_hist.as<u32>(), bs.d_flags.as<u32>());
        GLAUNCH(ctx, "k_scan_excl", k_scan_excl<u64>, dim3(1), dim3(1024), 0, bs.d_hist.as<u32>(), bs.d_bstart.as<u64>(), nbt);
        // two workgroups per CU fit (LDS); a few tiles per workgroup so that the prefetch of the next tile pays
        const u32 grid_scatter = std::min<u32>(rd.n_tiles, (u32)ctx->n_cu * (u32)knobs().scatter_wgs);
        GLAUNCH_K(ctx, W, "k_bucket_scatter", k_bucket_scatter<K>, dim3(grid_scatter), dim3(GASM_TILE_WG), ScatterLds<K>{nb}.total(), rs, rs.tile_info, k, bbits, g, padm, rd.n_tiles,
                  bs.d_bstart.as<u64>(), bs.d_toff.as<u32>(), bs.d_tcnt.as<ushort4>(), bs.d_keys.as<K>(), n_alloc);
    }
    // the buckets' distinct counts -> dstart by the de-duplication's last workgroup; beyond 16 384 buckets one workgroup of 256 is too slow a scanner: k_scan_excl in a launch of its own
    const bool scan_in_dedup = !bs.multi_pass && nbt <= 16384 && env_int("GASM_SCAN_IN_DEDUP", 1) != 0;
    bs.scan_in_dedup = scan_in_dedup;
    u32* const d_scan_out = scan_in_dedup ? bs.d_dstart.as<u32>() : nullptr;
    bs.fbits = dedup_fbits(bs.small_tbl && !bs.multi_pass ? 2048 : GASM_TBL);   // bins of the de-duplication kernel's counting sort (the multi-pass kernel: 4096 slots)
    GCHK(bs.d_fdir.ensure((size_t)nbt * ((1u << bs.fbits) + 1) * 2));
    // (k_bucket_dedup writes every entry of its bucket's fine directory)
    if (bs.multi_pass) {
        // passes over key sub-ranges, for buckets no table can hold; they re-read the bucket, so the result goes to a second
        // array and is copied back
        GCHK(bs.d_keys2.ensure(n_alloc * KB));
        GLAUNCH_K(ctx, W, "k_bucket_dedup_multi", k_bucket_dedup_multi<K>, dim3(nbt), dim3(GASM_WG), 0, bs.d_keys.as<K>(), bs.d_keys2.as<K>(),
                  bs.d_mult.as<u32>(), bs.d_bstart.as<u64>(), bs.d_bucket_d.as<u32>(), bs.d_flags.as<u32>(), bs.d_fdir.as<u16>(), 2 * k - bbits);
        HIPCHK(hipMemcpyAsync(bs.d_keys.p, bs.d_keys2.p, n_alloc * KB, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        GCHK(launch_bucket_dedup(ctx, bs, nbt, d_blen, d_scan_out));
    }
    if (bs.opts.min_count > 1) {
        // the multiplicity cutoff, behind whichever de-duplication ran (every rung of pipeline_build_finish's ladder comes through
        // here): weak keys leave the buckets' runs before anything reads them.  Its last workgroup redoes the offsets, counting on
        // a flag word of its own
        GCHK(bs.d_solid_removed.ensure((size_t)S * 4));
        HIPCHK(hipMemsetAsync(bs.d_solid_removed.p, 0, (size_t)S * 4, ctx->stream));
        GLAUNCH_K(ctx, W, "k_bucket_solid", k_bucket_solid<K>, dim3(nbt), dim3(GASM_WG), 0, bs.d_keys.as<K>(), bs.d_mult.as<u32>(), bs.d_bstart.as<u64>(),
                  bs.d_bucket_d.as<u32>(), bs.d_fdir.as<u16>(), 2 * k - bbits, bs.fbits, bbits, bs.opts.min_count, bs.d_solid_removed.as<u32>(),
                  bs.d_flags.as<u32>() + GASM_FLAG_SOLID_DONE, d_scan_out);
    }
    if (!scan_in_dedup) GLAUNCH(ctx, "k_scan_excl", k_scan_excl<u32>, dim3(1), dim3(1024), 0, bs.d_bucket_d.as<u32>(), bs.d_dstart.as<u32>(), nbt);
    return GASM_OK;
}

// ---- the per-edge arrays at their upper bound (the number of distinct k-mers is not known on the host)
static int alloc_graph(BuildState& bs, u32 S) {
    const u64 D = std::max<u64>(bs.D_cap, 1);
    const size_t KB = 8 * (size_t)bs.words;
    if (D >= 0xFFFFFFF0ull) { gasm_set_error("more than 2^32 distinct k-mers possible in one batch: split it"); return GASM_ERR_CAPACITY; }
    GCHK(bs.d_dk_key.ensure(D * KB));
    GCHK(bs.d_dk_cnt.ensure(D * 4));
    GCHK(bs.d_eflag.ensure(D));
    GCHK(bs.d_nxt.ensure(D * 4));
    GCHK(bs.d_link.ensure(D * 8));
    GCHK(bs.d_clen.ensure(D * 4));
    GCHK(bs.d_ecid.ensure(D * 4));
    GCHK(bs.d_ecoff.ensure(D * 8));
    GCHK(bs.d_rtab.ensure((D / 2 + S + 2) * 4));
    GCHK(bs.d_seg_cbases.ensure((size_t)S * 8 + (size_t)S * 4));   // u64 bases[S] then u32 counts[S]
    GCHK(bs.d_seg_cstart.ensure(((size_t)S + 1) * 4));
    GCHK(bs.d_seg_bstart.ensure(((size_t)S + 1) * 8));
    // contigs: at most one per edge, k-1 bases of the first node + one base per edge
    bs.bases_cap = D * (u64)bs.k;
    if (bs.bases_cap >= 0xFFFFFFF0ull) { gasm_set_error("contigs could exceed 2^32 bases: split the batch"); return GASM_ERR_CAPACITY; }
    GCHK(bs.d_c_off.ensure((D + 1) * 8));
    GCHK(bs.d_contig_ascii.ensure(bs.bases_cap + 64));
    return GASM_OK;
}

// ---- dense arrays -> (k-1)-mer graph -> chains -> contigs + the report.  Inputs: d_keys/d_mult/d_bstart (the buckets'
// distinct runs) and d_dstart/d_fdir.
// With tip clipping (bs.opts.tip_len > 0) the graph is made tip_rounds + 1 times.  A round = a graph pass up to the chains' lengths
// (no contigs, no report), k_tip_mark, which zeroes the multiplicities of the tips' edges in the buckets' runs, and
// k_bucket_solid with a cutoff of 1, which compacts the runs in place, rewrites the directory rows and redoes the offsets as it
// does behind the de-duplication; then the next pass gathers what is left.  All of it is queued: the host waits for nothing
// between rounds, and only the last pass's k_contig_scan publishes the report.
// Bubble popping (bubble_len > 0) adds bubble_rounds such rounds behind the tip rounds, with k_bubble_mark as the marking
// kernel.  (Tips first: a tip that hangs on a bubble's branch splits it.)  Low-coverage removal (lowcov()) adds cov_rounds such rounds
// behind all of those, with k_lowcov_mark as the marking kernel: tip_rounds + bubble_rounds + cov_rounds + 1 passes in all.  The rounds
// of a kind that is off are 0 in bs.opts (normalised), and a round's statistics go to its kind's row of bs.round_stats.
int launch_graph(gasm_ctx* ctx, u32 S, BuildState& bs) {
    const int W = bs.words, bbits = bs.bbits;
    const u32 nb = 1u << bbits, nbt = S * nb;
    GCHK(alloc_graph(bs, S));
    u32* const d_claim = bs.d_nxt.as<u32>();      // claim words of the degree kernels live in nxt until k_edge_next overwrites them
    const BuildOpts& o = bs.opts;
    const u32 rounds = o.total_rounds();
    for (u32 kind = 0; kind < ROUND_KINDS; ++kind) {
        RoundStats& rs = bs.round_stats[kind];
        if (!o.rounds(kind)) continue;
        GCHK(rs.d_stats.ensure((size_t)2 * rs.max_rounds * S * 4));
        HIPCHK(hipMemsetAsync(rs.d_stats.p, 0, (size_t)2 * rs.max_rounds * S * 4, ctx->stream));
    }
    for (u32 r = 0; r <= rounds; ++r) {
        GLAUNCH_K(ctx, W, "k_bucket_gather", k_bucket_gather<K>, dim3(nbt), dim3(GASM_WG), 0, bs.d_keys.as<K>(), bs.d_mult.as<u32>(),
                  bs.d_bstart.as<u64>(), bs.d_dstart.as<u32>(), bs.d_dk_key.as<K>(), bs.d_dk_cnt.as<u32>(), d_claim, bs.d_eflag.as<u8>(), bs.d_flags.as<u32>());
        GCHK(launch_graph_dense(ctx, S, bs, r == rounds));
        if (r == rounds) break;
        // round r of the build = round kr of its kind
        u32 kind = ROUNDS_TIP, kr = r;
        while (kr >= o.rounds(kind)) kr -= o.rounds(kind++);
        static const char* const range_name[ROUND_KINDS] = {"gasm:tips (mark, compact)", "gasm:bubbles (mark, compact)", "gasm:lowcov (mark, compact)"};
        GasmRange range(range_name[kind]);
        const RoundStats& rs = bs.round_stats[kind];
        u32* const d_contigs = rs.d_stats.as<u32>() + (size_t)kr * S;
        u32* const d_kmers = rs.d_stats.as<u32>() + ((size_t)rs.max_rounds + kr) * S;
        const u32 est = std::max<u32>(1, (u32)std::min<u64>(bs.maxD_est, bs.maxD_cap));
        const u32 dchunks = (u32)ceil_div_u64(est, GASM_WG);
        if (kind == ROUNDS_TIP) {
            GLAUNCH_K(ctx, W, "k_tip_mark", k_tip_mark<K>, seg_grid(dchunks, S), dim3(GASM_WG), 0, graph_view(bs), S, dchunks, bs.d_eflag.as<u8>(), bs.d_clen.as<u32>(),
                      bs.d_nxt.as<u32>(), bs.d_dk_cnt.as<u32>(), bs.d_bstart.as<u64>(), bs.d_mult.as<u32>(), o.tip_len, bs.d_flags.as<u32>(), d_contigs);
        } else if (kind == ROUNDS_BUBBLE) {
            GLAUNCH_K(ctx, W, "k_bubble_mark", k_bubble_mark<K>, seg_grid(dchunks, S), dim3(GASM_WG), 0, graph_view(bs), S, dchunks, bs.d_eflag.as<u8>(),
                      bs.d_clen.as<u32>(), bs.d_nxt.as<u32>(), bs.d_dk_cnt.as<u32>(), bs.d_bstart.as<u64>(), bs.d_mult.as<u32>(), o.bubble_len,
                      bs.d_flags.as<u32>(), d_contigs);
        } else {
            GLAUNCH_K(ctx, W, "k_lowcov_mark", k_lowcov_mark<K>, seg_grid(dchunks, S), dim3(GASM_WG), 0, graph_view(bs), S, dchunks, bs.d_eflag.as<u8>(),
                      bs.d_clen.as<u32>(), bs.d_nxt.as<u32>(), bs.d_dk_cnt.as<u32>(), bs.d_bstart.as<u64>(), bs.d_mult.as<u32>(), o.cov_len, o.cov_cutoff,
                      bs.d_flags.as<u32>(), d_contigs);
        }
        // (the done word is zero: the gather of this pass cleared it behind the cutoff's or the last round's compaction)
        u32* const d_scan_out = bs.scan_in_dedup ? bs.d_dstart.as<u32>() : nullptr;
        GLAUNCH_K(ctx, W, "k_bucket_solid", k_bucket_solid<K>, dim3(nbt), dim3(GASM_WG), 0, bs.d_keys.as<K>(), bs.d_mult.as<u32>(), bs.d_bstart.as<u64>(),
                  bs.d_bucket_d.as<u32>(), bs.d_fdir.as<u16>(), 2 * bs.k - bbits, bs.fbits, bbits, 1u, d_kmers, bs.d_flags.as<u32>() + GASM_FLAG_SOLID_DONE, d_scan_out);
        if (!d_scan_out) GLAUNCH(ctx, "k_scan_excl", k_scan_excl<u32>, dim3(1), dim3(1024), 0, bs.d_bucket_d.as<u32>(), bs.d_dstart.as<u32>(), nbt);
    }
    return GASM_OK;
}

// last_pass = false (a tip-clipping, bubble-popping or low-coverage round): stops behind the chains' lengths — eflag, nxt and clen
// are what k_tip_mark, k_bubble_mark and k_lowcov_mark read
static int launch_graph_dense(gasm_ctx* ctx, u32 S, BuildState& bs, bool last_pass) {
    GasmRange range("gasm:graph (degrees, list ranking, contigs)");
    const int W = bs.words;
    u32* const d_claim = bs.d_nxt.as<u32>();
    u32* const d_seg_ncontig = reinterpret_cast<u32*>(bs.d_seg_cbases.as<u64>() + S);
    u32* const d_fl = bs.d_flags.as<u32>();
    const GraphView gv = graph_view(bs);
    const u32 nb = 1u << bs.bbits;
    const u32 est = std::max<u32>(1, (u32)std::min<u64>(bs.maxD_est, bs.maxD_cap));   // grids: the kernels loop when a segment is larger
    const u32 dchunks = (u32)ceil_div_u64(est, GASM_WG);     // workgroups per segment of the per-edge kernels
    const dim3 grid_seg = seg_grid(dchunks, S);
    const u32 gchunks = (u32)ceil_div_u64(est, GASM_WG * GASM_EDGE_ILP);     // the kernels that take GASM_EDGE_ILP edges per thread and round
    const dim3 grid_grp = seg_grid(gchunks, S);
    u32* const d_tgt = bs.d_ecid.as<u32>();        // first out-edge of every edge's target node; e_cid is written later (k_contig_scan)
    GLAUNCH_K(ctx, W, "k_edge_target", k_edge_target<K>, grid_seg, dim3(GASM_WG), 0, gv, S, dchunks, d_tgt, d_claim);
    GLAUNCH(ctx, "k_edge_multi", k_edge_multi, grid_grp, dim3(GASM_WG), 0, gv, S, gchunks, d_tgt, d_claim, bs.d_eflag.as<u8>());
    // (links: k_edge_next is their only writer — every edge's — before the ranking reads them; chain lengths: k_link_jump / k_chain_len)
    GLAUNCH_K(ctx, W, "k_node_flags", k_node_flags<K>, grid_seg, dim3(GASM_WG), 0, gv, S, dchunks, d_claim, bs.d_eflag.as<u8>(), bs.d_link.as<u64>(), bs.d_clen.as<u32>());
    GLAUNCH(ctx, "k_edge_next", k_edge_next, grid_grp, dim3(GASM_WG), 0, gv, S, gchunks, d_tgt, bs.d_eflag.as<u8>(), bs.d_nxt.as<u32>(), bs.d_link.as<u64>());
    u32* const act = d_fl + GASM_FLAG_ACTIVE;     // "still active" words of the k_link_jump launches
    const u32 jchunks = (u32)ceil_div_u64(est, GASM_WG * GASM_JUMP_ILP);
    bs.ranked_in_lds = est <= 65534 && !bs.rank_global && !knobs().rank_global;
    bs.ruler_shift = 0;
    if (bs.ranked_in_lds) {
        // every second edge (the rulers) is ranked inside LDS, the others then need a step or two (kernels_build.hip)
        // rulers: every 2nd edge when every CU has a segment of its own to rank, every 4th when segments are few
        const u32 rshift = knobs().ruler_shift ? (u32)knobs().ruler_shift : (S >= (u32)ctx->n_cu / 4 ? 1u : 2u);
        bs.ruler_shift = rshift;
        const u32 rchunks = (u32)ceil_div_u64((est + (1u << rshift) - 1) >> rshift, GASM_WG);
        // LDS list of a segment: everything a workgroup can have while a CU only ever holds one of them, else the
        // estimate with a quarter to spare (a segment that does not fit raises GASM_FLAG_RANK_FAILED: pipeline_build_finish)
        u32 lds_entries = 32767;
        if (S > (u32)ctx->n_cu) lds_entries = std::min<u32>(32767, (((est + est / 4) >> rshift) + 1024) & ~1023u);
        GLAUNCH(ctx, "k_rank_rulers", k_rank_rulers, seg_grid(rchunks, S), dim3(GASM_WG), 0, gv, S, rchunks, bs.d_link.as<u64>(), bs.d_rtab.as<u32>(), rshift, d_fl);
        GLAUNCH(ctx, "k_rank_lds", k_rank_lds, dim3(S), dim3(1024), (size_t)lds_entries * 4 + 4, gv, bs.d_rtab.as<u32>(), bs.d_link.as<u64>(), knobs().rank_rounds, rshift,
                lds_entries, d_fl);
        // the odd edges: the ruler behind an edge is usually one or two steps away (a longer gap is geometrically rare)
        // (a thread stops as soon as its link is final; spans grow by a factor of jumps + 1 per launch at the very
        // least, so two launches cover any segment of this size, and the second normally returns at once)
        const int jumps = 255, launches = 2;
        static_assert(launches <= GASM_FLAG_ACTIVE_N, "an active word per launch");
        for (int r = 0; r < launches; ++r)
            GLAUNCH(ctx, "k_link_jump", k_link_jump, seg_grid(jchunks, S), dim3(GASM_WG), 0, gv, S, jchunks, bs.d_link.as<u64>(), r ? act + r - 1 : nullptr, act + r, jumps,
                    bs.d_nxt.as<u32>(), bs.d_clen.as<u32>());         // (+ the chains' lengths: k_chain_len's work)
    } else {
        // whole-GPU launches of `jumps` doubling steps each; a launch returns at once when its predecessor found every chain done
        // (spans grow by at least jumps + 1 = 5 per launch: log2(5) > 2.3 rounds' worth)
        int rounds = 1;
        while ((1ull << rounds) < bs.maxD_cap) ++rounds;
        rounds += 1;
        const int jumps = 4, launches = (rounds * 10 + 22) / 23 + 1;
        if (launches > (int)GASM_FLAG_ACTIVE_N) { gasm_set_error("segment too large for the list-ranking flags"); return GASM_ERR_CAPACITY; }
        for (int r = 0; r < launches; ++r)
            GLAUNCH(ctx, "k_link_jump", k_link_jump, seg_grid(jchunks, S), dim3(GASM_WG), 0, gv, S, jchunks, bs.d_link.as<u64>(), r ? act + r - 1 : nullptr, act + r, jumps,
                    (const u32*)nullptr, (u32*)nullptr);
    }
    const u32 grid_all = (u32)std::min<u64>(ceil_div_u64((u64)est * S, GASM_WG), (u64)ctx->n_cu * 64);
    if (!bs.ranked_in_lds)      // (the LDS path's k_link_jump launches publish the chains' lengths themselves)
        GLAUNCH(ctx, "k_chain_len", k_chain_len, dim3(std::max(1u, grid_all)), dim3(GASM_WG), 0, bs.d_nxt.as<u32>(), bs.d_link.as<u64>(),
                bs.d_clen.as<u32>(), gv.dstart + (size_t)S * nb);
    if (!last_pass) return GASM_OK;
    // segment directories of the contigs + the report (ticket last): written by the last workgroup of k_contig_scan to finish
    const size_t words = BuildReport<u32>::words(S);
    if (bs.h_report_words < words) {
        if (bs.h_report) (void)hipHostFree(bs.h_report);
        bs.h_report = nullptr; bs.h_report_words = 0;
        HIPCHK(hipHostMalloc((void**)&bs.h_report, words * 4, hipHostMallocCoherent));
        bs.h_report_words = words;
    }
    bs.ticket = next_ticket();
    BuildReport<volatile u32>{bs.h_report, S}.ticket() = 0;     // (the report of the previous build has been read or is void)
    GLAUNCH(ctx, "k_contig_scan", k_contig_scan, dim3(S), dim3(1024), 0, gv, bs.d_eflag.as<u8>(), bs.d_clen.as<u32>(),
            bs.d_ecid.as<u32>(), bs.d_ecoff.as<u64>(), d_seg_ncontig, bs.d_seg_cbases.as<u64>(), d_fl + GASM_FLAG_CONTIG_DONE, bs.d_seg_cstart.as<u32>(),
            bs.d_seg_bstart.as<u64>(), d_fl, bs.h_report, bs.ticket);
    GLAUNCH(ctx, "k_contig_place", k_contig_place, grid_seg, dim3(GASM_WG), 0, gv, bs.d_eflag.as<u8>(),
            bs.d_seg_cstart.as<u32>(), bs.d_seg_bstart.as<u64>(), bs.d_ecid.as<u32>(), bs.d_ecoff.as<u64>(), bs.d_c_off.as<u64>(), S, dchunks);
    GLAUNCH_K(ctx, W, "k_contig_emit", k_contig_emit<K>, grid_grp, dim3(GASM_WG), 0, gv, bs.d_link.as<u64>(), bs.d_nxt.as<u32>(),
              bs.d_ecoff.as<u64>(), bs.d_contig_ascii.as<u8>(), S, gchunks);
    bs.pending = true;
    return GASM_OK;
}

// host-side sizes of a batch's reads for key width / tile shape / bucket bits
int plan_build(gasm_ctx* ctx, DevReads& rd, int k, u64 hint, BuildState& bs) {
    if (k < 2 || k > GASM_MAX_K) { gasm_set_error("k = %d not supported (2..%d)", k, GASM_MAX_K); return GASM_ERR_INVALID; }
    const int W = k <= 31 ? 1 : 2;            // 64-bit keys up to k = 31, 128-bit keys (K128) up to k = 63
    const u32 KT = (u32)with_key(W, [](auto tag) -> int { return KeyTraits<typename decltype(tag)::type>::KT; });   // k-mers per thread and round of the tile kernels
    HIPCHK(hipSetDevice(ctx->device));
    GCHK(ensure_lds_attrs(ctx));
    const u32 S = rd.n_segments;
    const bool same = bs.k == k && bs.words == W && bs.h_seg_nk.size() == S && bs.hint == hint && bs.reads_id == rd.upload_id;
    bs.words = W; bs.k = k; bs.hint = hint; bs.reads_id = rd.upload_id;
    bs.fetched_distinct = bs.fetched_contigs = false;
    bs.pending = false;
    // ---- sizes known on the host
    u64 N = 0, maxNs = 0;
    bs.h_seg_nk.assign(S, 0);
    if (rd.fixed_len) {
        const u64 nk = rd.fixed_len >= (u32)k ? rd.fixed_len - k + 1 : 0;
        for (u32 s = 0; s < S; ++s) bs.h_seg_nk[s] = (rd.h_seg_read_off[s + 1] - rd.h_seg_read_off[s]) * nk;
    } else {
        u32 s = 0;
        for (u64 r = 0; r < rd.n_reads; ++r) {
            while (r >= rd.h_seg_read_off[s + 1]) ++s;
            const u64 L = rd.h_read_off[r + 1] - rd.h_read_off[r];
            if (L >= (u64)k) bs.h_seg_nk[s] += L - k + 1;
        }
    }
    for (u64 v : bs.h_seg_nk) { N += v; maxNs = std::max(maxNs, v); }
    bs.n_kmers = N;
    const u32 nk_max = rd.max_len >= (u32)k ? rd.max_len - k + 1 : 0;
    u32 g = next_pow2_u32((nk_max + KT - 1) / KT);     // threads per read (a power of two: divides the workgroup)
    g = std::max(1u, std::min((u32)GASM_TILE_WG, g));
    bs.tile_g = g;
    const u32 ipt = GASM_TILE_WG / g;
    // offset rounds: more than one only for reads with more than g*KT k-mers; every (read group, round) is a tile
    const u32 orr = std::max(1u, (nk_max + g * KT - 1) / (g * KT));
    if (orr > 0xFFFFu) { gasm_set_error("reads longer than %u bases are not supported", GASM_TILE_WG * KT * 0xFFFFu); return GASM_ERR_CAPACITY; }
    bs.tile_orr = orr;
    GCHK(rd.set_tiles(ctx, ipt, orr));
    // bucket bits: aim at <= ~900 distinct k-mers per bucket (2048-slot LDS table in two-slot sets, limit 1408)
    bs.bb_cap = std::min(10, 2 * (k - 1));
    const u64 dest = hint ? hint : std::max<u64>(1, maxNs / 8);
    if (!same || !bs.have_actual) {
        int bbits = 0;
        while (bbits < bs.bb_cap && (dest >> bbits) > 900) ++bbits;
        // few segments: up to two more bits so that there are enough (segment, bucket) workgroups to fill the chip
        for (int extra = 0; extra < 2 && bbits < bs.bb_cap && ((u64)S << bbits) < 1024; ++extra) ++bbits;
        bbits = std::min(bs.bb_cap, bbits + knobs().bbits_add);
        bs.bbits = bbits;
        // small (2048-slot) LDS tables when the expected number of distinct k-mers per bucket is small: more workgroups per CU
        bs.small_tbl = (dest >> bbits) <= 900;   // else the 4096-slot table (fewer workgroups per CU)
        if (knobs().dedup_tbl) bs.small_tbl = knobs().dedup_tbl == 2048;
        if (W == 2) bs.small_tbl = true;         // 128-bit keys: 2048-slot tables only
        bs.maxD_est = (u32)std::min<u64>(dest, 0xFFFFFFF0ull);
        bs.have_actual = false;
        bs.rank_global = false;
        bs.multi_pass = false;
        bs.single_pass = env_int("GASM_SINGLE_PASS", 1) != 0;
    }   // else: the same reads again — the partition that worked and the sizes the last build reported
    GCHK(bs.d_flags.ensure(GASM_FLAG_BYTES));
    bs.d_total = 0; bs.n_contigs = 0; bs.contig_bases = 0;
    return GASM_OK;
}

static void zero_results(BuildState& bs, u32 S) {
    bs.h_dstart.assign((size_t)S + 1, 0);
    bs.h_seg_cstart.assign((size_t)S + 1, 0);
    bs.h_seg_bstart.assign((size_t)S + 1, 0);
    bs.d_total = 0; bs.n_contigs = 0; bs.contig_bases = 0;
}

int build_opts_check(const BuildOpts& o) {
    if (o.min_count < 1) { gasm_set_error("min_count must be >= 1 (1 keeps every k-mer)"); return GASM_ERR_INVALID; }
    if (o.strands != 1 && o.strands != 2) { gasm_set_error("strands must be 1 or 2 (got %u)", o.strands); return GASM_ERR_INVALID; }
    if (o.tip_len && (o.tip_rounds < 1 || o.tip_rounds > GASM_MAX_TIP_ROUNDS)) {
        gasm_set_error("tip_rounds must be 1..%d when tip_len > 0 (got %u)", GASM_MAX_TIP_ROUNDS, o.tip_rounds);
        return GASM_ERR_INVALID;
    }
    // (the bound of every walk of k_bubble_mark, and what keeps its products inside 64 bits)
    if (o.bubble_len > GASM_MAX_BUBBLE_LEN) { gasm_set_error("bubble_len must be <= %d (got %u)", GASM_MAX_BUBBLE_LEN, o.bubble_len); return GASM_ERR_INVALID; }
    if (o.bubble_len && (o.bubble_rounds < 1 || o.bubble_rounds > GASM_MAX_BUBBLE_ROUNDS)) {
        gasm_set_error("bubble_rounds must be 1..%d when bubble_len > 0 (got %u)", GASM_MAX_BUBBLE_ROUNDS, o.bubble_rounds);
        return GASM_ERR_INVALID;
    }
    // (the same bound and the same two reasons for k_lowcov_mark; refused whatever cov_cutoff is, as it always was)
    if (o.cov_len > GASM_MAX_BUBBLE_LEN) { gasm_set_error("cov_len must be <= %d (got %u)", GASM_MAX_BUBBLE_LEN, o.cov_len); return GASM_ERR_INVALID; }
    if (o.lowcov() && (o.cov_rounds < 1 || o.cov_rounds > GASM_MAX_COV_ROUNDS)) {
        gasm_set_error("cov_rounds must be 1..%d when cov_cutoff > 0 and cov_len > 0 (got %u)", GASM_MAX_COV_ROUNDS, o.cov_rounds);
        return GASM_ERR_INVALID;
    }
    return GASM_OK;
}

BuildOpts build_opts_normalised(BuildOpts o) {
    if (!o.tip_len) o.tip_rounds = 0;
    if (!o.bubble_len) o.bubble_rounds = 0;
    if (!o.lowcov()) o.cov_rounds = 0;
    return o;
}

int pipeline_build(gasm_ctx* ctx, DevReads& rd, BuildState& bs, const BuildOpts& o) {
    if (o.strands == 2 && !rd.strands_of) { gasm_set_error("a both-strand build needs the both-strand reads"); return GASM_ERR_STATE; }
    // (both strands: up to twice the distinct k-mers of the genome; without a hint the estimate follows the doubled k-mer count)
    GCHK(plan_build(ctx, rd, o.k, o.strands == 2 ? 2 * o.genome_len_hint : o.genome_len_hint, bs));
    bs.opts = build_opts_normalised(o);
    bs.fetched_twins = false;
    bs.spectrum_queued = false;
    bs.coverage_queued = false;
    for (PassState* ps : {&bs.links, &bs.pairs, &bs.map, &bs.mapg, &bs.mapscore}) ps->queued = false;
    const u32 S = rd.n_segments;
    zero_results(bs, S);
    bs.part_single = bs.scan_in_dedup = bs.ranked_in_lds = false;
    bs.ruler_shift = 0;
    bs.attempts_distinct = bs.n_kmers ? 1 : 0;
    bs.attempts_graph = 0;
    if (bs.n_kmers == 0) {
        // nothing to do on the device; the directories the scorer borrows exist and are zero
        bs.bbits = 0; bs.D_cap = 0; bs.maxD_cap = 0;
        GCHK(alloc_graph(bs, S));
        GCHK(bs.d_dstart.ensure(((size_t)S + 2) * 4));
        HIPCHK(hipMemsetAsync(bs.d_dstart.p, 0, ((size_t)S + 2) * 4, ctx->stream));
        HIPCHK(hipMemsetAsync(bs.d_seg_cstart.p, 0, ((size_t)S + 1) * 4, ctx->stream));
        HIPCHK(hipMemsetAsync(bs.d_seg_bstart.p, 0, ((size_t)S + 1) * 8, ctx->stream));
        HIPCHK(hipMemsetAsync(bs.d_c_off.p, 0, 8, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return GASM_OK;
    }
    distinct_caps(bs, S);
    GCHK(launch_distinct(ctx, rd, bs));
    GCHK(launch_graph(ctx, S, bs));
    if (knobs().sync_build) GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    return GASM_OK;
}

bool build_next_config(u32 ovf, u32 rungs, int words, int bb_cap, bool& single_pass, bool& small_tbl, int& bbits, bool& multi_pass) {
    if ((rungs & GASM_RUNG_EXACT) && (ovf & GASM_OVF_REGION) && single_pass) single_pass = false;   // same partition, exact layout (count, scan, scatter)
    else if ((rungs & GASM_RUNG_TABLE) && small_tbl && words == 1) small_tbl = false;               // same partition, larger tables
    else if ((rungs & GASM_RUNG_BBITS) && bbits < bb_cap) bbits = std::min(bb_cap, bbits + 2);      // more buckets
    else if ((rungs & GASM_RUNG_MULTI) && !multi_pass) multi_pass = true;                           // all bucket bits used: key sub-ranges, pass by pass
    else return false;
    return true;
}

// Read the report of a queued build; repeat the build with the next larger configuration while it reports a failure.
int pipeline_build_finish(gasm_ctx* ctx, DevReads& rd, BuildState& bs, bool* rebuilt) {
    return pipeline_build_finish_n(ctx, &rd, rd.n_segments, bs, rebuilt);
}

// rd == nullptr: the dense arrays did not come from reads of this rank (pooled build): only the graph can be repeated
int pipeline_build_finish_n(gasm_ctx* ctx, DevReads* rd, u32 S, BuildState& bs, bool* rebuilt) {
    if (rebuilt) *rebuilt = false;
    if (!bs.pending) return GASM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    for (;;) {
        const BuildReport<const u32> rep{bs.h_report, S};
        GCHK(wait_report(ctx, &rep.ticket(), bs.ticket));
        bs.pending = false;
        const u32 overflow = rep.flags() & (GASM_OVF_TABLE | GASM_OVF_REGION);
        if (!overflow && !rep.rank_failed() && !(rep.flags() & GASM_OVF_TIP_RANK)) break;
        if (rebuilt) *rebuilt = true;
        if (overflow) {
            if (!rd) { gasm_set_error("a merged k-mer bucket overflowed its table: the pooled build needs more bucket bits"); return GASM_ERR_CAPACITY; }
            if (!build_next_config(overflow, GASM_RUNG_ALL, bs.words, bs.bb_cap, bs.single_pass, bs.small_tbl, bs.bbits, bs.multi_pass)) {
                gasm_set_error("a k-mer bucket holds more than %d distinct k-mers even with %d bucket bits", GASM_BUCKET_MAX, bs.bbits);
                return GASM_ERR_CAPACITY;
            }
            distinct_caps(bs, S);
            ++bs.attempts_distinct;
            GCHK(launch_distinct(ctx, *rd, bs));
        } else {
            bs.rank_global = true;        // whole-GPU pointer doubling instead of the LDS ranking
            ++bs.attempts_graph;
            // a clipped, popped or low-coverage-filtered build has compacted its runs round by round: a repeat of the graph alone would start from what the rounds
            // so far left and count them twice.  It starts over from the reads (same configuration, so the same k-mer set)
            if (bs.opts.total_rounds() && rd) { ++bs.attempts_distinct; GCHK(launch_distinct(ctx, *rd, bs)); }
        }
        GCHK(launch_graph(ctx, S, bs));
    }
    const BuildReport<const u32> rep{bs.h_report, S};
    bs.h_dstart.assign(&rep.dstart(0), &rep.dstart(S) + 1);
    u32 maxD = 0;
    for (u32 s = 0; s <= S; ++s) {
        bs.h_seg_cstart[s] = rep.cstart(s);
        bs.h_seg_bstart[s] = (u64)rep.bstart_lo(s) | ((u64)rep.bstart_hi(s) << 32);
        if (s < S) maxD = std::max(maxD, rep.dstart(s + 1) - rep.dstart(s));
    }
    bs.d_total = bs.h_dstart[S];
    bs.n_contigs = bs.h_seg_cstart[S];
    bs.contig_bases = bs.h_seg_bstart[S];
    // what the next build of the same reads starts from: sizes instead of estimates
    bs.maxD_est = std::max(1u, maxD);
    bs.paths_est = 1;
    for (u32 s = 0; s < S; ++s) bs.paths_est = std::max(bs.paths_est, bs.h_seg_cstart[s + 1] - bs.h_seg_cstart[s]);
    bs.have_actual = true;
    return GASM_OK;
}

// the path the last build took, from host fields only (GASM_PLAN_* in include/gasm.h)
void pipeline_build_plan(const DevReads& rd, const BuildState& bs, int32_t* row) {
    row[GASM_PLAN_KEY_WORDS] = bs.words;
    row[GASM_PLAN_BUCKET_BITS] = bs.bbits;
    row[GASM_PLAN_TABLE_SLOTS] = bs.small_tbl ? 2048 : 4096;
    row[GASM_PLAN_SINGLE_PASS] = bs.part_single;
    row[GASM_PLAN_MULTI_PASS] = bs.multi_pass;
    row[GASM_PLAN_SCAN_IN_DEDUP] = bs.scan_in_dedup;
    row[GASM_PLAN_RANKED_IN_LDS] = bs.ranked_in_lds;
    row[GASM_PLAN_RULER_SHIFT] = (int32_t)bs.ruler_shift;
    row[GASM_PLAN_RANK_GLOBAL] = bs.rank_global || knobs().rank_global;
    row[GASM_PLAN_TILE_G] = (int32_t)bs.tile_g;
    row[GASM_PLAN_OFFSET_ROUNDS] = (int32_t)bs.tile_orr;
    row[GASM_PLAN_DISTINCT_ATTEMPTS] = (int32_t)bs.attempts_distinct;
    row[GASM_PLAN_GRAPH_ATTEMPTS] = (int32_t)bs.attempts_graph;
    row[GASM_PLAN_K] = bs.k;
    row[GASM_PLAN_SEGMENTS] = (int32_t)rd.n_segments;
}

int pipeline_fetch_distinct(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    if (bs.fetched_distinct) return GASM_OK;
    const u32 S = rd.n_segments;
    bs.h_seg_doff.resize((size_t)S + 1);
    for (u32 s = 0; s <= S; ++s) bs.h_seg_doff[s] = bs.h_dstart.empty() ? 0 : bs.h_dstart[s];
    bs.h_dk_key.resize((size_t)bs.d_total * bs.words);     // 128-bit keys come back as (hi, lo) pairs
    bs.h_dk_cnt.resize(bs.d_total);
    if (bs.d_total) {
        HIPCHK(hipMemcpyAsync(bs.h_dk_key.data(), bs.d_dk_key.p, (size_t)bs.d_total * 8 * bs.words, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(bs.h_dk_cnt.data(), bs.d_dk_cnt.p, (size_t)bs.d_total * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    bs.fetched_distinct = true;
    return GASM_OK;
}

int pipeline_fetch_round_stats(gasm_ctx* ctx, DevReads& rd, BuildState& bs, u32 kind) {
    GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    RoundStats& rs = bs.round_stats[kind];
    const u32 S = rd.n_segments, R = rs.max_rounds;
    rs.h_contigs.assign((size_t)S * R, 0); rs.h_kmers.assign((size_t)S * R, 0);
    if (!bs.opts.rounds(kind) || !bs.n_kmers) return GASM_OK;          // (a build without k-mers launched nothing)
    std::vector<u32> h((size_t)2 * R * S);
    GCHK(d2h_sync(ctx, h.data(), rs.d_stats.p, h.size() * 4));
    for (u32 s = 0; s < S; ++s)
        for (u32 r = 0; r < R; ++r) { rs.h_contigs[(size_t)s * R + r] = h[(size_t)r * S + s]; rs.h_kmers[(size_t)s * R + r] = h[((size_t)R + r) * S + s]; }
    return GASM_OK;
}

int pipeline_fetch_solid_stats(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    const u32 S = rd.n_segments;
    std::vector<u32> removed(S, 0);
    // (a build without k-mers launched nothing, and min_count = 1 removed nothing)
    if (bs.opts.min_count > 1 && bs.n_kmers) GCHK(d2h_sync(ctx, removed.data(), bs.d_solid_removed.p, (size_t)S * 4));
    bs.h_solid_before.resize(S); bs.h_solid_after.resize(S);
    // (the tips clipped, the bubbles popped and the low-coverage contigs removed behind the cutoff are not the cutoff's: they count as
    // survivors here)
    for (u32 kind = 0; kind < ROUND_KINDS; ++kind) if (bs.opts.rounds(kind)) GCHK(pipeline_fetch_round_stats(ctx, rd, bs, kind));
    for (u32 s = 0; s < S; ++s) {
        bs.h_solid_after[s] = bs.h_dstart.empty() ? 0 : bs.h_dstart[s + 1] - bs.h_dstart[s];
        for (u32 kind = 0; kind < ROUND_KINDS; ++kind) {
            const RoundStats& rs = bs.round_stats[kind];
            if (bs.opts.rounds(kind)) for (u32 r = 0; r < rs.max_rounds; ++r) bs.h_solid_after[s] += rs.h_kmers[(size_t)s * rs.max_rounds + r];
        }
        bs.h_solid_before[s] = bs.h_solid_after[s] + removed[s];
    }
    return GASM_OK;
}

// k-mer spectrum: on the stream of the build, behind it; reads dstart and dk_cnt, writes an array of its own
int pipeline_kmer_spectrum(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    HIPCHK(hipSetDevice(ctx->device));
    const u32 S = rd.n_segments;
    GCHK(bs.d_spectrum.ensure((size_t)S * 256 * 4));
    HIPCHK(hipMemsetAsync(bs.d_spectrum.p, 0, (size_t)S * 256 * 4, ctx->stream));
    if (bs.d_total) {
        const u32 chunks = std::max(1u, std::min<u32>(ceil_div_u64(bs.maxD_est, GASM_WG * 8), 64u));      // a few rounds per workgroup: fewer flushes
        GLAUNCH(ctx, "k_kmer_spectrum", k_kmer_spectrum, seg_grid(chunks, S), dim3(GASM_WG), 0, bs.d_dstart.as<u32>(), 1u << bs.bbits, bs.d_dk_cnt.as<u32>(), S, chunks,
                bs.d_spectrum.as<u32>());
    }
    bs.spectrum_queued = true;
    return GASM_OK;
}

// per-contig coverage: on the stream of the build, behind it; reads dstart, the ranking's links, the contig ids and dk_cnt, writes an
// array of its own (u64 sums[P], then u32 edges[P])
int pipeline_contig_coverage(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    HIPCHK(hipSetDevice(ctx->device));
    const u32 S = rd.n_segments, P = bs.n_contigs;
    if (P && bs.d_total) {
        GCHK(bs.d_ccov.ensure((size_t)P * 12));
        HIPCHK(hipMemsetAsync(bs.d_ccov.p, 0, (size_t)P * 12, ctx->stream));
        const u32 chunks = std::max(1u, (u32)ceil_div_u64(bs.maxD_est, GASM_WG));
        GLAUNCH(ctx, "k_contig_cov", k_contig_cov, seg_grid(chunks, S), dim3(GASM_WG), 0, bs.d_dstart.as<u32>(), 1u << bs.bbits, S, chunks, bs.d_link.as<u64>(),
                bs.d_ecid.as<u32>(), bs.d_dk_cnt.as<u32>(), bs.d_seg_cstart.as<u32>(), reinterpret_cast<unsigned long long*>(bs.d_ccov.as<u64>()),
                reinterpret_cast<u32*>(bs.d_ccov.as<u64>() + P));
    }
    bs.coverage_queued = true;
    return GASM_OK;
}

int pipeline_fetch_contig_coverage(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    if (!bs.coverage_queued) { gasm_set_error("gasm_batch_fetch_contig_coverage before gasm_batch_contig_coverage (of the last build)"); return GASM_ERR_STATE; }
    const u32 P = bs.n_contigs;
    bs.h_ccov_m.assign(P, 0); bs.h_ccov_n.assign(P, 0);
    if (P && bs.d_total) {
        HIPCHK(hipMemcpyAsync(bs.h_ccov_m.data(), bs.d_ccov.p, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(bs.h_ccov_n.data(), bs.d_ccov.as<u64>() + P, (size_t)P * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GASM_OK;
}

static_assert(GASM_THREAD_KMER_CAP == GASM_THREAD_MAX_KMERS, "kernels.h and gasm.h disagree on read threading");
static_assert(GASM_PAIR_COUNTERS == GASM_PAIR_FIELDS, "kernels.h and gasm.h disagree on read pairs");
static_assert(GASM_MAP_COUNTERS == GASM_MAP_FIELDS && GASM_MAP_BLOCKS == GASM_MAP_MAX_BLOCKS, "kernels.h and gasm.h disagree on read mapping");
static_assert(GASM_MAPG_COUNTERS == GASM_MAPG_FIELDS && GASM_MAPG_GAP == GASM_MAP_MAX_GAP, "kernels.h and gasm.h disagree on gapped read mapping");
static_assert(GASM_MAPEND_COUNTERS == GASM_MAPEND_FIELDS, "kernels.h and gasm.h disagree on end gaps");
static_assert(GASM_MAP_PIECES == GASM_MAP_MAX_PIECES && GASM_MAP_MAX_PIECES == GASM_MAP_MAX_BLOCKS + 2, "kernels.h and gasm.h disagree on alignments");
static_assert(GASM_MAPSCORE_CLASSES == GASM_MAPSCORE_FIELDS, "kernels.h and gasm.h disagree on mapped scoring");
static_assert(GASM_CORRECT_STATS == GASM_CORRECT_FIELDS && GASM_CORRECT_KMER_CAP == GASM_CORRECT_MAX_KMERS, "kernels.h and gasm.h disagree on read correction");

// ---- the passes that lay reads over a finished build: each on the stream of the build, behind it; each reads the build's arrays and the
// packed reads and writes an array of its own (PassState), laid out by a PassLayout that the fetch derives again

// workgroups per segment of a pass over the reads of `rd` that takes units_per_wg units (reads; pairs: reads_per_unit = 2) per workgroup
// and round: as many as the largest segment needs, at most 8 per CU over all segments — the kernels loop where a segment holds more than
// the grid covers at once
static u32 read_pass_chunks(const gasm_ctx* ctx, const DevReads& rd, u32 units_per_wg, u32 reads_per_unit = 1) {
    u64 most = 1;
    for (u32 s = 0; s < rd.n_segments; ++s) most = std::max(most, (rd.h_seg_read_off[s + 1] - rd.h_seg_read_off[s]) / reads_per_unit);
    const u32 groups = (rd.n_segments + 7u) / 8u;
    return std::max(1u, std::min<u32>(ceil_div_u64(most, units_per_wg), std::max(1u, (u32)ctx->n_cu * 8u / groups)));
}

// the pass's array at the size of the layout, its zeroed tables cleared
static int pass_begin(gasm_ctx* ctx, PassState& ps, const PassLayout& l) {
    GCHK(ps.d.ensure(l.bytes));
    HIPCHK(hipMemsetAsync(l.at<char>(ps.d, 0) + l.zero_from, 0, l.bytes - l.zero_from, ctx->stream));
    return GASM_OK;
}

// every table of the layout into the pass's host copies; `entry`, `queue`: the public names for the error
static int pass_fetch(gasm_ctx* ctx, PassState& ps, const PassLayout& l, const char* entry, const char* queue) {
    if (!ps.queued) { gasm_set_error("%s before %s (of the last build)", entry, queue); return GASM_ERR_STATE; }
    ps.h.resize(l.t.size());
    for (size_t i = 0; i < l.t.size(); ++i) {
        ps.h[i].assign(l.t[i].bytes() / 8 + 1, 0);
        if (l.t[i].bytes()) HIPCHK(hipMemcpyAsync(ps.h[i].data(), l.at<char>(ps.d, i), l.t[i].bytes(), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GASM_OK;
}

static PassLayout links_layout(u32 P, u32 S) {
    const size_t p = P;
    return {{4 * p, 4, 4, false}, {4 * p, 4, 4, false}, {4 * p, 4, 4, true}, {16 * p, 4, 4, true}, {S, 8, 8, true}};
}

// contig links: succ and pred (filled with "none"), link support, span support, skipped reads
int pipeline_contig_links(gasm_ctx* ctx, DevReads& rd, BuildState& bs, u32 span_len) {
    if (rd.positioned) { gasm_set_error("contig links need the reads back to back (pooled builds place them by position)"); return GASM_ERR_STATE; }
    GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    HIPCHK(hipSetDevice(ctx->device));
    const u32 S = rd.n_segments, P = bs.n_contigs;
    const PassLayout l = links_layout(P, S);
    GCHK(pass_begin(ctx, bs.links, l));
    if (P) HIPCHK(hipMemsetAsync(bs.links.d.p, 0xFF, l.zero_from, ctx->stream));
    const GraphView gv = graph_view(bs);
    const ContigIndex ci = contig_index(bs);
    if (ci.have_graph) {
        const u32 grid = (u32)std::min<u64>(ceil_div_u64(P, GASM_WG), (u64)ctx->n_cu * 8);
        GLAUNCH_K(ctx, bs.words, "k_contig_links", k_contig_links<K>, dim3(grid), dim3(GASM_WG), 0, gv, ci, S, l.at<u32>(bs.links.d, LINKS_SUCC),
                  l.at<u32>(bs.links.d, LINKS_PRED));
    }
    if (rd.n_reads && S) {
        const u32 reads_per_wg = 64, chunks = read_pass_chunks(ctx, rd, reads_per_wg);      // 16 reads per wave, as the correction kernel
        GLAUNCH_K(ctx, bs.words, "k_read_thread", k_read_thread<K>, seg_grid(chunks, S), dim3(GASM_WG), 0, rd.view(), gv, ci, span_len, reads_per_wg, chunks,
                  l.at<u32>(bs.links.d, LINKS_LSUP), l.at<u32>(bs.links.d, LINKS_SSUP), l.at<unsigned long long>(bs.links.d, LINKS_SKIPPED));
    }
    bs.links.queued = true;
    return GASM_OK;
}

int pipeline_fetch_contig_links(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    GCHK(pass_fetch(ctx, bs.links, links_layout(bs.n_contigs, rd.n_segments), "gasm_batch_fetch_contig_links", "gasm_batch_contig_links"));
    if (bs.opts.strands == 2) for (u32 s = 0; s < rd.n_segments; ++s) bs.links.h[LINKS_SKIPPED][s] /= 2;      // (a read and its reverse complement are equally long)
    return GASM_OK;
}

static PassLayout pairs_layout(u64 n_pairs, u32 orient, u32 S, u32 max_insert) {
    return {{(size_t)n_pairs * orient * 4, 4, 16, false}, {(size_t)S * ((size_t)max_insert + 1), 4, 4, true}, {(size_t)S * GASM_PAIR_FIELDS, 8, 8, true}};
}

// read pairs: records, insert histogram, counters
int pipeline_place_pairs(gasm_ctx* ctx, DevReads& rd_build, DevReads& rd, BuildState& bs, u32 max_insert) {
    if (rd.positioned) { gasm_set_error("read pairs need the reads back to back (pooled builds place them by position)"); return GASM_ERR_STATE; }
    const u32 S = rd.n_segments;
    for (u32 s = 0; s < S; ++s)
        if ((rd.h_seg_read_off[s + 1] - rd.h_seg_read_off[s]) & 1) {
            gasm_set_error("segment %u holds an odd number of reads (%llu): reads 2p and 2p + 1 are the mates of pair p", s,
                           (unsigned long long)(rd.h_seg_read_off[s + 1] - rd.h_seg_read_off[s]));
            return GASM_ERR_INVALID;
        }
    GCHK(pipeline_build_finish(ctx, rd_build, bs, nullptr));
    HIPCHK(hipSetDevice(ctx->device));
    const u32 orient = bs.opts.strands == 2 ? 2u : 1u;
    const u64 n_pairs = rd.n_reads / 2;
    const PassLayout l = pairs_layout(n_pairs, orient, S, max_insert);
    GCHK(pass_begin(ctx, bs.pairs, l));
    if (n_pairs && S) {
        // a wave holds 64 scans (a mate of an oriented pair each), a workgroup four waves of them
        const u32 chunks = read_pass_chunks(ctx, rd, (GASM_WG / 64) * (32u / orient), 2);
        GLAUNCH_K(ctx, bs.words, "k_pair_place", k_pair_place<K>, seg_grid(chunks, S), dim3(GASM_WG), 0, rd.view(), graph_view(bs), contig_index(bs), orient, max_insert,
                  n_pairs, chunks, l.at<int32_t>(bs.pairs.d, PAIRS_REC), l.at<u32>(bs.pairs.d, PAIRS_HIST), l.at<unsigned long long>(bs.pairs.d, PAIRS_CNT));
    }
    bs.pairs.param[0] = orient;
    bs.pairs.param[1] = max_insert;
    bs.pairs.queued = true;
    return GASM_OK;
}

int pipeline_fetch_pair_places(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    return pass_fetch(ctx, bs.pairs, pairs_layout(rd.n_reads / 2, bs.pairs.param[0], rd.n_segments, bs.pairs.param[1]), "gasm_batch_fetch_pair_places",
                      "gasm_batch_place_pairs");
}

// (ends: the end records and the end counters behind the six tables of the gapped form, which keep their places; the end records are zeroed
// with the rest, so they come behind the first zeroed table; trace: behind those the piece records and the insertion pileup of ins_cols
// columns ("Alignments"), zeroed likewise)
static PassLayout map_layout(bool gapped, u64 n_reads, u64 contig_bases, u32 S, u32 max_edits, bool ends = false, bool trace = false, u32 ins_cols = 0) {
    const PassTable rec{(size_t)n_reads * 4, 4, 16, false}, pile{(size_t)contig_bases * 4, 4, 4, true}, gpile{(size_t)contig_bases * 2, 4, 4, true},
        hist{(size_t)S * ((size_t)max_edits + 1), 4, 4, true};
    if (gapped && ends && trace)
        return {rec, rec, pile, gpile, hist, {(size_t)S * GASM_MAPG_FIELDS, 8, 8, true}, {(size_t)n_reads * 4, 4, 16, true}, {(size_t)S * GASM_MAPEND_FIELDS, 8, 8, true},
                {(size_t)n_reads * GASM_MAP_PIECES * 2, 4, 16, true}, {(size_t)contig_bases * ins_cols * 4, 4, 16, true}};
    if (gapped && ends)
        return {rec, rec, pile, gpile, hist, {(size_t)S * GASM_MAPG_FIELDS, 8, 8, true}, {(size_t)n_reads * 4, 4, 16, true}, {(size_t)S * GASM_MAPEND_FIELDS, 8, 8, true}};
    if (gapped) return {rec, rec, pile, gpile, hist, {(size_t)S * GASM_MAPG_FIELDS, 8, 8, true}};
    return {rec, pile, hist, {(size_t)S * GASM_MAP_FIELDS, 8, 8, true}};
}

// read mapping, all forms: records, pileup, histogram, counters; gapped: and gap records and the gap pileup; end_gap > 0 (gapped only): and
// end records and end counters, by k_read_map_ends.  end_gap = 0 launches exactly k_read_map_gapped.  trace (gapped only, any end_gap): all
// eight and the piece records and the insertion pileup, by k_read_map_trace alone
int pipeline_map_reads(gasm_ctx* ctx, DevReads& rd_build, DevReads& rd, BuildState& bs, bool gapped, u32 max_edits, u32 max_gap, u32 end_gap, bool trace) {
    if (rd.positioned) { gasm_set_error("read mapping needs the reads back to back (pooled builds place them by position)"); return GASM_ERR_STATE; }
    GCHK(pipeline_build_finish(ctx, rd_build, bs, nullptr));
    HIPCHK(hipSetDevice(ctx->device));
    const u32 S = rd.n_segments;
    PassState& ps = gapped ? bs.mapg : bs.map;
    trace = trace && gapped;
    const bool ends = gapped && (end_gap > 0 || trace);
    const u32 ins_cols = trace ? std::max(max_gap, end_gap) : 0u;
    const PassLayout l = map_layout(gapped, rd.n_reads, bs.n_contigs ? bs.contig_bases : 0, S, max_edits, ends, trace, ins_cols);
    GCHK(pass_begin(ctx, ps, l));
    if (rd.n_reads && S) {
        const u32 reads_per_wg = GASM_WG / 64, chunks = read_pass_chunks(ctx, rd, reads_per_wg);       // a wave per read
        if (trace) {
            const MapOutTrace out{{l.at<int32_t>(ps.d, MAPG_REC), l.at<int32_t>(ps.d, MAPG_GAP), l.at<u32>(ps.d, MAPG_PILE), l.at<u32>(ps.d, MAPG_GPILE),
                                   l.at<u32>(ps.d, MAPG_HIST), l.at<unsigned long long>(ps.d, MAPG_CNT), l.at<int32_t>(ps.d, MAPG_END), l.at<unsigned long long>(ps.d, MAPG_ENDCNT)},
                                  l.at<int32_t>(ps.d, MAPG_PIECE), l.at<u32>(ps.d, MAPG_INS)};
            GLAUNCH_K(ctx, bs.words, "k_read_map_trace", (k_read_map<K, true, true, true>), seg_grid(chunks, S), dim3(GASM_WG), 0, rd.view(), graph_view(bs), contig_index(bs),
                      max_edits, max_gap, end_gap, reads_per_wg, chunks, out);
        } else if (ends) {
            const MapOut out{l.at<int32_t>(ps.d, MAPG_REC), l.at<int32_t>(ps.d, MAPG_GAP), l.at<u32>(ps.d, MAPG_PILE), l.at<u32>(ps.d, MAPG_GPILE),
                             l.at<u32>(ps.d, MAPG_HIST), l.at<unsigned long long>(ps.d, MAPG_CNT), l.at<int32_t>(ps.d, MAPG_END), l.at<unsigned long long>(ps.d, MAPG_ENDCNT)};
            GLAUNCH_K(ctx, bs.words, "k_read_map_ends", (k_read_map<K, true, true, false>), seg_grid(chunks, S), dim3(GASM_WG), 0, rd.view(), graph_view(bs), contig_index(bs),
                      max_edits, max_gap, end_gap, reads_per_wg, chunks, out);
        } else if (gapped) {
            const MapOut out{l.at<int32_t>(ps.d, MAPG_REC), l.at<int32_t>(ps.d, MAPG_GAP), l.at<u32>(ps.d, MAPG_PILE), l.at<u32>(ps.d, MAPG_GPILE),
                             l.at<u32>(ps.d, MAPG_HIST), l.at<unsigned long long>(ps.d, MAPG_CNT), nullptr, nullptr};
            GLAUNCH_K(ctx, bs.words, "k_read_map_gapped", (k_read_map<K, true, false, false>), seg_grid(chunks, S), dim3(GASM_WG), 0, rd.view(), graph_view(bs), contig_index(bs),
                      max_edits, max_gap, 0u, reads_per_wg, chunks, out);
        } else {
            const MapOut out{l.at<int32_t>(ps.d, MAP_REC), nullptr, l.at<u32>(ps.d, MAP_PILE), nullptr, l.at<u32>(ps.d, MAP_HIST),
                             l.at<unsigned long long>(ps.d, MAP_CNT), nullptr, nullptr};
            GLAUNCH_K(ctx, bs.words, "k_read_map", (k_read_map<K, false, false, false>), seg_grid(chunks, S), dim3(GASM_WG), 0, rd.view(), graph_view(bs), contig_index(bs),
                      max_edits, 0u, 0u, reads_per_wg, chunks, out);
        }
    }
    ps.param[0] = max_edits;
    ps.param[1] = (ends ? MAPG_HAS_ENDS : 0u) | (trace ? MAPG_HAS_TRACE : 0u) | ins_cols << MAPG_COLS_SHIFT;
    ps.queued = true;
    return GASM_OK;
}

int pipeline_fetch_read_map(gasm_ctx* ctx, DevReads& rd, BuildState& bs, bool gapped) {
    PassState& ps = gapped ? bs.mapg : bs.map;
    const u32 form = gapped ? ps.param[1] : 0u;
    return pass_fetch(ctx, ps, map_layout(gapped, rd.n_reads, bs.n_contigs ? bs.contig_bases : 0, rd.n_segments, ps.param[0], (form & MAPG_HAS_ENDS) != 0,
                                          (form & MAPG_HAS_TRACE) != 0, form >> MAPG_COLS_SHIFT),
                      gapped ? "gasm_batch_fetch_read_map_gapped" : "gasm_batch_fetch_read_map", gapped ? "gasm_batch_map_reads_gapped" : "gasm_batch_map_reads");
}

// read correction: on the stream of the build, behind it; reads the packed reads, dstart, the fine directory and the dense keys, writes a
// copy of the reads and a stats array, both the caller's
int pipeline_correct_reads(gasm_ctx* ctx, DevReads& rd, BuildState& bs, DBuf& out_words, DBuf& d_stats) {
    if (rd.positioned) { gasm_set_error("read correction needs the reads back to back (pooled builds place them by position)"); return GASM_ERR_STATE; }
    if (bs.pending || bs.k == 0) { gasm_set_error("read correction needs a finished build"); return GASM_ERR_STATE; }
    HIPCHK(hipSetDevice(ctx->device));
    const u32 S = rd.n_segments;
    const size_t bytes = ((rd.total_bases + 31) / 32 + 4) * 8;              // the stream and its four padding words
    GCHK(out_words.ensure(bytes));
    const size_t have = rd.d_words.p ? std::min(bytes, rd.d_words.cap) : 0;
    if (have) HIPCHK(hipMemcpyAsync(out_words.p, rd.d_words.p, have, hipMemcpyDeviceToDevice, ctx->stream));
    if (have < bytes) HIPCHK(hipMemsetAsync(static_cast<char*>(out_words.p) + have, 0, bytes - have, ctx->stream));
    GCHK(d_stats.ensure((size_t)S * GASM_CORRECT_FIELDS * 4));
    HIPCHK(hipMemsetAsync(d_stats.p, 0, (size_t)S * GASM_CORRECT_FIELDS * 4, ctx->stream));
    if (!rd.n_reads) return GASM_OK;
    // 64 reads per workgroup and round, 16 per wave: enough to amortise the workgroup's six atomics
    const u32 reads_per_wg = 64, chunks = read_pass_chunks(ctx, rd, reads_per_wg);
    const int have_graph = bs.n_kmers && bs.d_total ? 1 : 0;                // (the k-mer set is all it needs: a build without a contig has one)
    GLAUNCH_K(ctx, bs.words, "k_read_correct", k_read_correct<K>, seg_grid(chunks, S), dim3(GASM_WG), 0, rd.view(), graph_view(bs), have_graph, reads_per_wg,
              chunks, reinterpret_cast<unsigned long long*>(out_words.p), d_stats.as<u32>());
    return GASM_OK;
}

int pipeline_fetch_reads(gasm_ctx* ctx, DevReads& rd, std::vector<char>& h_ascii, std::vector<u64>& h_read_off) {
    if (rd.positioned) { gasm_set_error("the reads of a pooled build lie at positions, not back to back: nothing to fetch"); return GASM_ERR_STATE; }
    HIPCHK(hipSetDevice(ctx->device));
    const u64 T = rd.total_bases;
    h_read_off.resize(rd.n_reads + 1);
    for (u64 r = 0; r <= rd.n_reads; ++r) h_read_off[r] = rd.fixed_len ? r * (u64)rd.fixed_len : rd.h_read_off[r];
    h_ascii.assign(T + 1, 0);                   // (one byte more: a pointer to hand out for no bases at all)
    if (T) {
        DBuf d;
        struct Rel { DBuf& b; ~Rel() { b.release(); } } rel{d};
        GCHK(d.ensure(T));
        GLAUNCH(ctx, "k_unpack_ascii", k_unpack_ascii, dim3(std::min<u32>(ceil_div_u64(T, GASM_WG), (u32)ctx->n_cu * 32u)), dim3(GASM_WG), 0, rd.d_words.as<u64>(), T,
                d.as<u8>());
        HIPCHK(hipMemcpyAsync(h_ascii.data(), d.p, T, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return GASM_OK;
}

int pipeline_fetch_kmer_spectrum(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    if (!bs.spectrum_queued) { gasm_set_error("gasm_batch_fetch_kmer_spectrum before gasm_batch_kmer_spectrum (of the last build)"); return GASM_ERR_STATE; }
    const size_t n = (size_t)rd.n_segments * 256;
    std::vector<u32> h(n);
    HIPCHK(hipMemcpyAsync(h.data(), bs.d_spectrum.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    bs.h_spectrum.assign(h.begin(), h.end());
    return GASM_OK;
}

// twin map of a both-strand build: k_contig_twin on the build's stream behind it, once per build; reads the directory, the
// ranking's links, the contig ids and the contig text, writes an array of its own
int pipeline_fetch_contig_twins(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    if (bs.opts.strands != 2) { gasm_set_error("the twin map exists after a strands = 2 build only"); return GASM_ERR_STATE; }
    if (bs.fetched_twins) return GASM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const u32 P = bs.n_contigs;
    bs.h_twin.assign(P, 0);
    if (P) {
        GCHK(bs.d_twin.ensure(((size_t)P + 1) * 4));
        u32* const d_bad = bs.d_twin.as<u32>() + P;
        HIPCHK(hipMemsetAsync(d_bad, 0, 4, ctx->stream));
        const GraphView gv = graph_view(bs);
        const u32 grid = (u32)std::min<u64>(ceil_div_u64(P, GASM_WG), (u64)ctx->n_cu * 8);
        GLAUNCH_K(ctx, bs.words, "k_contig_twin", k_contig_twin<K>, dim3(grid), dim3(GASM_WG), 0, gv, bs.d_link.as<u64>(), bs.d_ecid.as<u32>(), bs.d_c_off.as<u64>(),
                  bs.d_seg_cstart.as<u32>(), bs.d_contig_ascii.as<u8>(), rd.n_segments, bs.d_twin.as<u32>(), d_bad);
        std::vector<u32> h((size_t)P + 1);
        HIPCHK(hipMemcpyAsync(h.data(), bs.d_twin.p, h.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (h[P]) { gasm_set_error("a contig of a both-strand build has no reverse-complement twin in its segment"); return GASM_ERR_INTERNAL; }
        bs.h_twin.assign(h.begin(), h.begin() + P);
    }
    bs.fetched_twins = true;
    return GASM_OK;
}

// per-edge flags and successors of the finished build (rows A4-A6 of SURVEY §8 made visible: lib/DeNovoAssembler.cpp:125-189)
int pipeline_fetch_graph(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    bs.h_eflag.resize(bs.d_total);
    bs.h_nxt.resize(bs.d_total);
    if (bs.d_total) {
        HIPCHK(hipMemcpyAsync(bs.h_eflag.data(), bs.d_eflag.p, (size_t)bs.d_total, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(bs.h_nxt.data(), bs.d_nxt.p, (size_t)bs.d_total * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GASM_OK;
}

int pipeline_fetch_contigs(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    GCHK(pipeline_build_finish(ctx, rd, bs, nullptr));
    if (bs.fetched_contigs) return GASM_OK;
    const u32 S = rd.n_segments;
    bs.h_seg_coff.resize((size_t)S + 1);
    for (u32 s = 0; s <= S; ++s) bs.h_seg_coff[s] = bs.h_seg_cstart.empty() ? 0 : bs.h_seg_cstart[s];
    bs.h_c_off.assign((size_t)bs.n_contigs + 1, 0);
    bs.h_contigs.resize(bs.contig_bases);
    if (bs.n_contigs) {
        HIPCHK(hipMemcpyAsync(bs.h_c_off.data(), bs.d_c_off.p, ((size_t)bs.n_contigs + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(bs.h_contigs.data(), bs.d_contig_ascii.p, bs.contig_bases, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    bs.fetched_contigs = true;
    return GASM_OK;
}

// The contigs of a build as paths: offsets and directories are the build's own device arrays (borrowed, no copy, no
// host round trip); only the 2-bit packing of the contig text is new.  Works on a build the host has not waited for:
// the number of bases is read on the device.
int pipeline_contig_paths(gasm_ctx* ctx, const DevReads& rd, const BuildState& bs, DevPaths& dp) {
    const u32 S = rd.n_segments;
    dp.n_segments = S;
    dp.n_paths = 0; dp.total_bases = 0;            // host-side numbers: pipeline_contig_paths_host, after the report
    dp.h_p_off.clear(); dp.h_seg_path_off.clear(); dp.h_seg_base_off.clear();
    dp.b_p_off = bs.d_c_off.as<u64>();
    dp.b_seg_path_off = bs.d_seg_cstart.as<u32>();
    dp.b_seg_base_off = bs.d_seg_bstart.as<u64>();
    const u64 cap_words = (bs.bases_cap + 31) / 32 + 4;
    GCHK(dp.d_words.ensure(cap_words * 8));
    const u32 grid = (u32)std::min<u64>(ceil_div_u64(std::max<u64>(1, (u64)bs.maxD_est * S / 32 + 4), GASM_WG), (u64)ctx->n_cu * 16);
    GLAUNCH(ctx, "k_pack_ascii", k_pack_ascii, dim3(std::max(1u, grid)), dim3(GASM_WG), 0, bs.d_contig_ascii.as<u8>(), (u64)0,
            bs.d_seg_bstart.as<u64>() + S, dp.d_words.as<u64>(), (u32*)nullptr);
    return GASM_OK;
}

void pipeline_contig_paths_host(const DevReads& rd, const BuildState& bs, DevPaths& dp) {
    dp.n_paths = bs.n_contigs;
    dp.total_bases = bs.contig_bases;
    dp.h_seg_path_off.assign(bs.h_seg_cstart.begin(), bs.h_seg_cstart.end());
    dp.h_seg_base_off.assign(bs.h_seg_bstart.begin(), bs.h_seg_bstart.end());
    if (dp.h_seg_path_off.size() != (size_t)rd.n_segments + 1) { dp.h_seg_path_off.assign((size_t)rd.n_segments + 1, 0); dp.h_seg_base_off.assign((size_t)rd.n_segments + 1, 0); }
}

// ---------------------------------------------------------------------------------------------------------------
// score tables
// ---------------------------------------------------------------------------------------------------------------
#define DIRECT_ROWS 87380
static inline u32 direct_base_h(u32 L) { return ((1u << (2 * L)) - 4u) / 3u; }

int ScoreTable::set(gasm_ctx* ctx, const char* bp_kmer, const u64* bp_off, u64 nt, const double* bp_prob) {
    if (nt > 0x7FFFFFFFull) { gasm_set_error("table too large"); return GASM_ERR_CAPACITY; }
    std::vector<double> prob(DIRECT_ROWS, 0.0);
    std::vector<int32_t> row(DIRECT_ROWS, -1);
    for (u64 i = 0; i < nt; ++i) {
        const u64 L = bp_off[i + 1] - bp_off[i];
        if (L < 1 || L > 8) { gasm_set_error("bp_kmer[%llu] has length %llu; supported: 1..8", (unsigned long long)i, (unsigned long long)L); return GASM_ERR_INVALID; }
        u32 v = 0;
        for (u64 j = 0; j < L; ++j) {
            const char c = bp_kmer[bp_off[i] + j];
            u32 code;
            switch (c) { case 'A': code = 0; break; case 'C': code = 1; break; case 'G': code = 2; break; case 'T': code = 3; break;
                default: gasm_set_error("bp_kmer[%llu] holds a base outside ACGT", (unsigned long long)i); return GASM_ERR_NON_ACGT; }
            v = (v << 2) | code;
        }
        const u32 idx = direct_base_h((u32)L) + v;
        if (row[idx] >= 0) { gasm_set_error("bp_kmer[%llu] repeats an earlier key", (unsigned long long)i); return GASM_ERR_INVALID; }
        row[idx] = (int32_t)i;
        prob[idx] = bp_prob[i];
    }
    n_table = (u32)nt;
    h_row_prob.assign(bp_prob, bp_prob + nt);
    GCHK(h2d(ctx, d_prob, prob.data(), prob.size() * 8));
    GCHK(h2d(ctx, d_row, row.data(), row.size() * 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return GASM_OK;
}

int ScoreTable::set_standard(gasm_ctx* ctx, const double* t) {
    std::vector<double> prob(DIRECT_ROWS, 0.0);
    std::vector<int32_t> row(DIRECT_ROWS, -1);
    u32 src = 0;
    for (u32 L = 2; L <= 8; L += 2) {
        const u32 n = 1u << (2 * L), b = direct_base_h(L);
        for (u32 v = 0; v < n; ++v) { prob[b + v] = t[src]; row[b + v] = (int32_t)src; ++src; }
    }
    n_table = GASM_TABLE_ROWS;
    GCHK(h2d(ctx, d_prob, prob.data(), prob.size() * 8));
    GCHK(h2d(ctx, d_row, row.data(), row.size() * 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    h_prob = prob;
    h_finite = gasm_host::table_range(h_prob.data(), h_prob.size(), &h_absmax);
    fix_shift = -1;
    return GASM_OK;
}

int ScoreTable::fixed_shift(u64 max_terms) const { return gasm_host::fixed_point_shift(h_absmax, h_finite, max_terms); }

// 64-bit fixed-point copy of the table for the batch scorer: round(prob * 2^shift), shift from fixed_shift (the sum
// over a segment's reads cannot pass 2^62)
int ScoreTable::set_fixed(gasm_ctx* ctx, int shift) {
    if (shift < 0 || !h_finite) { gasm_set_error("the table has no fixed-point shift for these reads"); return GASM_ERR_STATE; }
    if (shift == fix_shift) return GASM_OK;
    std::vector<long long> fx(h_prob.size());
    for (size_t i = 0; i < fx.size(); ++i) fx[i] = std::llrint(std::ldexp(h_prob[i], shift));
    GCHK(h2d(ctx, d_fix, fx.data(), fx.size() * 8));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    fix_shift = shift;
    return GASM_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Levenshtein distances
// ---------------------------------------------------------------------------------------------------------------
int pipeline_levenshtein(gasm_ctx* ctx, DevPaths& dp, const char* target, u64 target_len, bool infix, std::vector<int32_t>& lev, bool* done) {
    GasmRange range("gasm:levenshtein");
    *done = false;
    const u32 P = dp.n_paths;
    lev.assign(P, 0);
    if (P == 0 || target_len == 0) { *done = true; return GASM_OK; }      // (empty target: the reference returns 0)
    if (target_len >= 0xFFFFFF00ull) return GASM_OK;                       // host routine
    HIPCHK(hipSetDevice(ctx->device));
    DBuf ascii, err, twords, carry, d_out;
    struct Rel { std::vector<DBuf*> v; ~Rel() { for (DBuf* b : v) b->release(); } } rel{{&ascii, &err, &twords, &carry, &d_out}};
    GCHK(err.ensure(8));
    HIPCHK(hipMemsetAsync(err.p, 0, 8, ctx->stream));
    GCHK(h2d(ctx, ascii, target, target_len));
    int st = pack_ascii(ctx, ascii.as<u8>(), target_len, twords, err.as<u32>());
    u32 herr = 0;
    if (st == GASM_OK && hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) st = GASM_ERR_HIP;
    if (st == GASM_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = GASM_ERR_HIP;
    if (st != GASM_OK || herr) { ascii.release(); err.release(); twords.release(); return st; }   // not ACGT: host routine
    // a wave per path, in the order of the paths (scaffolds come longest first): the dispatcher hands the next workgroup to
    // the CU that has room, which balances better than a fixed share of paths per resident wave (22 053 scaffolds of one
    // segment: 329 -> 318 ms); what a wave parks for its next band is 16 bytes per 64 target columns, capped at 2 GB in all
    // (global distances may run with the roles of path and target swapped: the columns are then the path's)
    u64 max_cols = target_len;
    if (!infix) for (u32 p = 0; p < P; ++p) max_cols = std::max<u64>(max_cols, dp.h_p_off[p + 1] - dp.h_p_off[p]);
    const u64 per_wave = ((max_cols - 1) / 64 + 2) * 16;
    const u32 cap = (u32)std::max<u64>((u64)ctx->n_cu * 4u, std::min<u64>(1u << 20, (2ull << 30) / per_wave));      // (at least a wave per SIMD)
    const u32 waves = std::min<u32>(P, getenv("GASM_LEV_WAVES") ? (u32)ctx->n_cu * (u32)atoi(getenv("GASM_LEV_WAVES")) : cap);
    const u32 wgs = (waves + GASM_WG / 64 - 1) / (GASM_WG / 64);
    const bool v2 = env_int("GASM_LEV_V", 2) != 1;
    // what a band leaves for the next one, per wave: 16 bytes per 64 target columns (v2) / a byte per column
    const u64 stride = v2 ? ((max_cols - 1) / 64 + 2) : ((target_len + 64 + 63) & ~(u64)63);
    st = carry.ensure((size_t)wgs * (GASM_WG / 64) * stride * (v2 ? 16 : 1));
    if (st == GASM_OK) st = d_out.ensure((size_t)P * 4);
    if (st == GASM_OK) {
        if (v2) hipLaunchKernelGGL(k_levenshtein2, dim3(wgs), dim3(GASM_WG), 0, ctx->stream, dp.view(), P, twords.as<u64>(), (u32)target_len, infix ? 1 : 0,
                                   carry.as<uint4>(), stride, d_out.as<int32_t>());
        else hipLaunchKernelGGL(k_levenshtein, dim3(wgs), dim3(GASM_WG), 0, ctx->stream, dp.view(), P, twords.as<u64>(), (u32)target_len, infix ? 1 : 0,
                                carry.as<u8>(), stride, d_out.as<int32_t>());
        if (hipGetLastError() != hipSuccess) st = GASM_ERR_HIP;
    }
    if (st == GASM_OK && hipMemcpyAsync(lev.data(), d_out.p, (size_t)P * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) st = GASM_ERR_HIP;
    if (st == GASM_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { gasm_set_error("k_levenshtein failed"); st = GASM_ERR_HIP; }
    ascii.release(); err.release(); twords.release(); carry.release(); d_out.release();
    if (st == GASM_OK) *done = true;
    return st;
}

void ScoreTable::release() { d_prob.release(); d_row.release(); d_fix.release(); }

// ---------------------------------------------------------------------------------------------------------------
// F4: KS statistic and coverage (kernels_score.hip)
// ---------------------------------------------------------------------------------------------------------------
int pipeline_ks(gasm_ctx* ctx, DevPaths& dp, ScoreState& ss, const ScoreTable& tb, const char* genome, u64 genome_len, int kmer, std::vector<double>& ks) {
    ks.assign(dp.n_paths, std::nan(""));
    if (dp.n_paths == 0) return GASM_OK;
    std::vector<u32> h_hist;
    GCHK(pipeline_ks_genome_hist(ctx, tb, genome, genome_len, kmer, h_hist));
    return pipeline_ks_paths(ctx, dp, ss, tb, h_hist, kmer, ks);
}

// ---- the genome's side: rows of its kmer-long windows, counted (the table's rows, not its probabilities)
int pipeline_ks_genome_hist(gasm_ctx* ctx, const ScoreTable& tb, const char* genome, u64 genome_len, int kmer, std::vector<u32>& h_hist) {
    const u32 NT = tb.n_table;
    HIPCHK(hipSetDevice(ctx->device));
    DBuf ascii, err, gwords, hist;
    struct Rel { std::vector<DBuf*> v; ~Rel() { for (DBuf* b : v) b->release(); } } rel{{&ascii, &err, &gwords, &hist}};
    GCHK(err.ensure(8));
    HIPCHK(hipMemsetAsync(err.p, 0, 8, ctx->stream));
    GCHK(h2d(ctx, ascii, genome, genome_len));
    GCHK(pack_ascii(ctx, ascii.as<u8>(), genome_len, gwords, err.as<u32>()));
    GCHK(hist.ensure((size_t)std::max<u32>(NT, 1) * 4));
    HIPCHK(hipMemsetAsync(hist.p, 0, (size_t)std::max<u32>(NT, 1) * 4, ctx->stream));
    GLAUNCH(ctx, "k_ks_genome_hist", k_ks_genome_hist, dim3(std::max(1u, std::min<u32>(ceil_div_u64(genome_len + 1, GASM_WG), (u32)ctx->n_cu * 8u))), dim3(GASM_WG), 0,
            gwords.as<u64>(), genome_len, kmer, tb.d_row.as<int32_t>(), hist.as<u32>());
    h_hist.assign(NT, 0);
    u32 herr = 0;
    HIPCHK(hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (NT) HIPCHK(hipMemcpyAsync(h_hist.data(), hist.p, (size_t)NT * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (herr) { gasm_set_error("true_solution holds a base outside upper-case ACGT: the KS statistic needs its window probabilities"); return GASM_ERR_NON_ACGT; }
    return GASM_OK;
}

// ---- one table's probabilities: the genome's rows in ascending-probability order, prefix-summed; then the paths' side
int pipeline_ks_paths(gasm_ctx* ctx, DevPaths& dp, ScoreState& ss, const ScoreTable& tb, const std::vector<u32>& h_hist, int kmer, std::vector<double>& ks) {
    const u32 P = dp.n_paths, NT = tb.n_table;
    ks.assign(P, std::nan(""));
    if (P == 0) return GASM_OK;
    if (tb.h_row_prob.size() != NT || h_hist.size() != NT) { gasm_set_error("the KS statistic needs the table rows (ScoreTable::set)"); return GASM_ERR_STATE; }
    HIPCHK(hipSetDevice(ctx->device));
    DBuf d_pv, d_cumy, scratch, d_out;
    struct Rel { std::vector<DBuf*> v; ~Rel() { for (DBuf* b : v) b->release(); } } rel{{&d_pv, &d_cumy, &scratch, &d_out}};
    std::vector<u32> order(NT);
    for (u32 i = 0; i < NT; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return tb.h_row_prob[a] < tb.h_row_prob[b]; });
    std::vector<double> pv(NT);
    std::vector<u32> cumy(NT);
    u64 run = 0;
    for (u32 r = 0; r < NT; ++r) { pv[r] = tb.h_row_prob[order[r]]; run += h_hist[order[r]]; cumy[r] = (u32)run; }
    GCHK(h2d(ctx, d_pv, pv.data(), (size_t)NT * 8));
    GCHK(h2d(ctx, d_cumy, cumy.data(), (size_t)NT * 4));
    // ---- the paths' side: k_path_ks2 (histogram over the counts' values); a path with a count beyond its bins goes to k_path_ks
    const u32 bins = (u32)std::max(2, std::min(1024, env_int("GASM_DBG_KS_BINS", 1024)));
    const bool v2 = env_int("GASM_KS_V", 2) != 1 && NT > 0;
    const u32 grid = std::min<u32>(P, (u32)ctx->n_cu * (v2 ? 4u : 2u));
    GCHK(scratch.ensure((size_t)grid * 2 * std::max<u32>(NT, 1) * 4));
    GCHK(d_out.ensure((size_t)P * 8));
    std::vector<u32> todo;
    if (v2) {
        DBuf d_run_end, d_flags;
        struct Rel2 { std::vector<DBuf*> v; ~Rel2() { for (DBuf* b : v) b->release(); } } rel2{{&d_run_end, &d_flags}};
        std::vector<u32> run_end(NT);
        for (u32 r = NT; r-- > 0;) run_end[r] = (r + 1 < NT && pv[r + 1] == pv[r]) ? run_end[r + 1] : r;
        GCHK(h2d(ctx, d_run_end, run_end.data(), (size_t)NT * 4));
        GCHK(d_flags.ensure((size_t)P * 4));
        HIPCHK(hipMemsetAsync(d_flags.p, 0, (size_t)P * 4, ctx->stream));
        HIPCHK(hipMemsetAsync(scratch.p, 0, (size_t)grid * 2 * NT * 4, ctx->stream));         // (the kernel keeps the counts zero between paths)
        GLAUNCH(ctx, "k_path_ks2", k_path_ks2, dim3(grid), dim3(GASM_WG), 0, dp.view(), ss.d_poscnt.as<u32>(), tb.d_row.as<int32_t>(), kmer, NT, d_pv.as<double>(),
                d_cumy.as<u32>(), d_run_end.as<u32>(), scratch.as<u32>(), d_out.as<double>(), d_flags.as<u32>(), P, bins);
        std::vector<u32> h_flags(P);
        HIPCHK(hipMemcpyAsync(h_flags.data(), d_flags.p, (size_t)P * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(ks.data(), d_out.p, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (u32 p = 0; p < P; ++p) if (h_flags[p]) todo.push_back(p);
        if (todo.empty()) return GASM_OK;
    }
    {
        DBuf d_list;
        struct Rel3 { DBuf* b; ~Rel3() { b->release(); } } rel3{&d_list};
        const u32 n = v2 ? (u32)todo.size() : P;
        if (v2) GCHK(h2d(ctx, d_list, todo.data(), (size_t)n * 4));
        const u32 g1 = std::min<u32>(n, (u32)ctx->n_cu * 2u);
        GLAUNCH(ctx, "k_path_ks", k_path_ks, dim3(g1), dim3(GASM_WG), 0, dp.view(), ss.d_poscnt.as<u32>(), tb.d_row.as<int32_t>(), kmer, NT, d_pv.as<double>(),
                d_cumy.as<u32>(), scratch.as<u32>(), d_out.as<double>(), n, v2 ? d_list.as<u32>() : (const u32*)nullptr);
        HIPCHK(hipMemcpyAsync(ks.data(), d_out.p, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return GASM_OK;
}

int pipeline_coverage(gasm_ctx* ctx, const long long* start, const long long* len, u64 n, long long seq_len, double* percent) {
    *percent = 0.0;
    if (seq_len <= 0) return GASM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    DBuf d_s, d_l, diff, cov;
    struct Rel { std::vector<DBuf*> v; ~Rel() { for (DBuf* b : v) b->release(); } } rel{{&d_s, &d_l, &diff, &cov}};
    GCHK(h2d(ctx, d_s, start, n * 8));
    GCHK(h2d(ctx, d_l, len, n * 8));
    GCHK(diff.ensure(((size_t)seq_len + 3) * 4));
    GCHK(cov.ensure(8));
    HIPCHK(hipMemsetAsync(diff.p, 0, ((size_t)seq_len + 3) * 4, ctx->stream));
    if (n) GLAUNCH(ctx, "k_cover_mark", k_cover_mark, dim3(ceil_div_u64(n, GASM_WG)), dim3(GASM_WG), 0, d_s.as<long long>(), d_l.as<long long>(), n, seq_len, diff.as<int>());
    GLAUNCH(ctx, "k_cover_count", k_cover_count, dim3(1), dim3(1024), 0, diff.as<int>(), seq_len, cov.as<unsigned long long>());
    unsigned long long c = 0;
    HIPCHK(hipMemcpyAsync(&c, cov.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // lib/DeNovoAssembler.R:445: (1 - uncovered / seq_len) * 100
    *percent = (1.0 - (double)(seq_len - (long long)c) / (double)seq_len) * 100.0;
    return GASM_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// score: pipeline_score_launch queues everything on the stream; pipeline_score_fetch copies the results back.
// ---------------------------------------------------------------------------------------------------------------
static u64 max_seg_reads(const DevReads& rd) {
    u64 m = 0;
    for (u32 s = 0; s < rd.n_segments; ++s) m = std::max(m, rd.h_seg_read_off[s + 1] - rd.h_seg_read_off[s]);
    return m;
}

static_assert(GASM_SCORE_MAX_TABLES == GASM_MAX_TABLES, "kernels.h and gasm.h disagree on the number of tables");

#define GASM_TABLES_SWITCH(T, CASE)                                                                                      \
    switch (T) {                                                                                                         \
        case 1: CASE(1); break; case 2: CASE(2); break; case 3: CASE(3); break; case 4: CASE(4); break; case 5: CASE(5); break;  \
        case 6: CASE(6); break; case 7: CASE(7); break; default: CASE(8); break;                                         \
    }

// Batch scoring of a build's own contigs (gasm_batch_score, gasm_batch_score_tables) under T tables: queued behind the build
// without waiting for it.  The number of paths is read on the device (graph.d_seg_cstart[S]); outputs are allocated at the
// build's upper bound.  One k_score_zero, one k_score_reads_graph, a k_score_finish per table (tiny; each with its table's
// own fixed-point shift).  One count array, the sums of table t at t * stride behind table 0's.
static int score_launch_graph(gasm_ctx* ctx, DevReads& rd, DevPaths& dp, int kmer, ScoreTable* const* tbs, u32 T, ScoreState& ss,
                              const BuildState& graph) {
    GasmRange range("gasm:score (graph-indexed)");
    GCHK(ensure_lds_attrs(ctx));
    const u32 S = rd.n_segments;
    const size_t PC = (size_t)graph.D_cap + 1;
    ss.stride = PC;
    ss.graph = &graph;
    ss.n_paths = 0;
    const size_t fx_off = (PC * 4 + 15) & ~(size_t)15;
    GCHK(ss.d_total.ensure(fx_off + PC * 8 * T));
    GCHK(ss.d_out_f64.ensure(PC * 8 * 3 * T));
    GCHK(ss.d_out_i32.ensure(PC * 4 * 2));
    unsigned long long* const d_fx = reinterpret_cast<unsigned long long*>(static_cast<char*>(ss.d_total.p) + fx_off);
    const u32* const n_paths_p = graph.d_seg_cstart.as<u32>() + S;
    const u64 p_est = graph.have_actual ? std::max<u64>(graph.n_contigs, 1) : (u64)S * 256;
    const u32 grid_p = (u32)std::max<u64>(1, std::min<u64>(ceil_div_u64(p_est, GASM_WG), (u64)ctx->n_cu * 8));
    GLAUNCH(ctx, "k_score_zero", k_score_zero, dim3(grid_p), dim3(GASM_WG), 0, ss.d_total.as<u32>(), d_fx, (u64)PC, T, n_paths_p);
    const PathSet ps = dp.view();
    // the paths are this build's contigs and every read holds a k-mer: the sorted edge list is the index, and the
    // per-path sums are accumulated per read in fixed point (no position counters)
    const GraphView gv = graph_view(graph);
    const u64 max_reads = max_seg_reads(rd);
    FixTables ft = {};
    for (u32 t = 0; t < T; ++t) {
        GCHK(tbs[t]->set_fixed(ctx, tbs[t]->fixed_shift(max_reads)));
        ft.p[t] = tbs[t]->d_fix.as<long long>();
    }
    // GASM_SCORE_VERIFY=1: compare every read with the contig text where the graph says it lies (kernels_score.hip, graph_match);
    // a mismatch raises GASM_FLAG_SCORE_MISMATCH of the build and pipeline_score_fetch refuses the scores
    // A graph built with a multiplicity cutoff does not hold every k-mer of every read: the comparison is then part of the match
    // (verify = 2: a mismatch is "no match" and raises nothing)
    const int verify = (graph.opts.min_count > 1 || graph.opts.total_rounds()) ? 2 : env_int("GASM_SCORE_VERIFY", 0) != 0 ? 1 : 0;
    ss.verify = verify == 1;
    const u32 reads_per_wg = 256;     // one read per thread: the match is a chain of dependent loads
    const u32 rchunks = (u32)ceil_div_u64(max_reads, reads_per_wg);
    // per-path accumulators kept in LDS: sized from the last build of these reads (a segment with more paths than that
    // goes to global atomics: slower, same numbers); 4 + 8 T bytes per path, GASM_SCORE_PATH_CAP * 12 bytes at most
    u32 lds_paths = std::min<u32>(std::max<u32>(graph.have_actual ? graph.paths_est : 1024u, 1u), (u32)(GASM_SCORE_PATH_CAP * 12 / (4 + 8 * T)));
    if (const int cap = env_int("GASM_DBG_SCORE_LDS_PATHS", 0)) lds_paths = std::min<u32>(lds_paths, (u32)std::max(1, cap));
    const size_t lds_bytes = (size_t)lds_paths * (4 + 8 * (size_t)T);
#define GASM_LAUNCH_SCORE(TT)                                                                                                                       \
    GLAUNCH_K(ctx, graph.words, "k_score_reads_graph", (k_score_reads_graph<K, TT>), seg_grid(rchunks, S), dim3(GASM_WG), lds_bytes, rd.view(), gv, \
              graph.d_link.as<u64>(), graph.d_ecid.as<u32>(), ps, ft, kmer, reads_per_wg, rchunks, lds_paths, ss.d_total.as<u32>(), d_fx, (u64)PC,  \
              verify, graph.d_flags.as<u32>() + GASM_FLAG_SCORE_MISMATCH)
    GASM_TABLES_SWITCH(T, GASM_LAUNCH_SCORE)
#undef GASM_LAUNCH_SCORE
    int32_t* o_br = ss.d_out_i32.as<int32_t>();
    int32_t* o_ln = o_br + PC;
    const u64* d_se = nullptr;
    if (rd.n_empty) { GCHK(h2d(ctx, ss.d_seg_empty, rd.h_seg_empty.data(), (size_t)S * 8)); d_se = ss.d_seg_empty.as<u64>(); }
    for (u32 t = 0; t < T; ++t) {
        double* o_bp = ss.d_out_f64.as<double>() + (size_t)t * 3 * PC;
        GLAUNCH(ctx, "k_score_finish", k_score_finish, dim3(grid_p), dim3(GASM_WG), 0, ps, ss.d_total.as<u32>(), d_fx + (size_t)t * PC, ft.p[t], d_se, kmer,
                std::ldexp(1.0, -tbs[t]->fix_shift), o_bp, o_bp + PC, o_bp + 2 * PC, o_br, o_ln, n_paths_p);
    }
    ss.h_pd_off.clear();
    ss.launched = true;
    return GASM_OK;
}

// Mapped scoring: the records of the build's read mapping (bs.map or bs.mapg) into breakage sums under T tables, read starts per contig base
// and class counters.  Behind the finished build on its stream: the sizes are the report's.  One memset of the accumulators, one
// k_score_mapped, a k_score_finish per table (as it is: seg_empty = nullptr, the contigs' extents from c_off — it reads no packed path then)
static PassLayout mapscore_layout(u32 T, u32 P, u64 contig_bases, u32 S) {
    const size_t p = P;
    return {{3 * (size_t)T * p, 8, 8, false}, {2 * p, 4, 4, false}, {p, 4, 4, true}, {(size_t)T * p, 8, 8, true}, {(size_t)contig_bases, 4, 4, true},
            {(size_t)S * GASM_MAPSCORE_FIELDS, 8, 8, true}};
}

int pipeline_score_mapped(gasm_ctx* ctx, DevReads& rd_build, DevReads& rd, BuildState& bs, bool gapped, int kmer, ScoreTable* const* tbs, u32 T, bool partial) {
    if (rd.positioned) { gasm_set_error("mapped scoring needs the reads back to back (pooled builds place them by position)"); return GASM_ERR_STATE; }
    if (T < 1 || T > GASM_MAX_TABLES) { gasm_set_error("n_tables must be 1..%d (got %u)", GASM_MAX_TABLES, T); return GASM_ERR_INVALID; }
    if (kmer < 0) { gasm_set_error("kmer must be >= 0"); return GASM_ERR_INVALID; }
    GCHK(pipeline_build_finish(ctx, rd_build, bs, nullptr));
    const PassState& src = gapped ? bs.mapg : bs.map;
    if (!src.queued) { gasm_set_error("mapped scoring needs a read mapping of that source over the last build"); return GASM_ERR_STATE; }
    const u64 max_reads = max_seg_reads(rd);
    for (u32 t = 0; t < T; ++t)
        if (tbs[t]->fixed_shift(max_reads) < 0) { gasm_set_error("table %u has no fixed-point shift for these reads: mapped scoring has no FP64 form", t); return GASM_ERR_INVALID; }
    HIPCHK(hipSetDevice(ctx->device));
    GCHK(ensure_lds_attrs(ctx));
    const u32 S = rd.n_segments, P = bs.n_contigs;
    const u64 bases = P ? bs.contig_bases : 0;
    FixTables ft = {};
    for (u32 t = 0; t < T; ++t) {
        GCHK(tbs[t]->set_fixed(ctx, tbs[t]->fixed_shift(max_reads)));
        ft.p[t] = tbs[t]->d_fix.as<long long>();
        bs.mapscore_shift[t] = tbs[t]->fix_shift;
    }
    PassState& ps = bs.mapscore;
    ps.queued = false;
    const PassLayout l = mapscore_layout(T, P, bases, S);
    GCHK(pass_begin(ctx, ps, l));
    const PassLayout ml = map_layout(gapped, rd.n_reads, bases, S, src.param[0]);
    const ContigIndex ci = contig_index(bs);
    u32* const d_cnt = l.at<u32>(ps.d, MAPSC_CNT);
    unsigned long long* const d_fx = l.at<unsigned long long>(ps.d, MAPSC_FX);
    if (rd.n_reads && S) {
        const u32 reads_per_wg = GASM_WG;     // one read per thread: a record load, the contig's extent, a window, T gathers
        const u32 rchunks = (u32)ceil_div_u64(max_reads, reads_per_wg);
        // the LDS accumulators as score_launch_graph sizes them (the build is finished: its contig count is there)
        u32 lds_paths = std::min<u32>(std::max<u32>(bs.have_actual ? bs.paths_est : 1024u, 1u), (u32)(GASM_SCORE_PATH_CAP * 12 / (4 + 8 * T)));
        if (const int cap = env_int("GASM_DBG_SCORE_LDS_PATHS", 0)) lds_paths = std::min<u32>(lds_paths, (u32)std::max(1, cap));
        const size_t lds_bytes = (size_t)lds_paths * (4 + 8 * (size_t)T);
        const int32_t* const rec = ml.at<int32_t>(src.d, gapped ? (size_t)MAPG_REC : (size_t)MAP_REC);
        const int32_t* const rec_gap = gapped ? ml.at<int32_t>(src.d, MAPG_GAP) : nullptr;
#define GASM_LAUNCH_MAPSCORE(TT)                                                                                                                      \
    if (gapped) GLAUNCH(ctx, "k_score_mapped_gapped", (k_score_mapped<TT, true>), seg_grid(rchunks, S), dim3(GASM_WG), lds_bytes, rd.view(), ci, rec, rec_gap, \
                        ft, kmer, partial ? 1u : 0u, reads_per_wg, rchunks, lds_paths, d_cnt, d_fx, (u64)P, l.at<u32>(ps.d, MAPSC_PILE),               \
                        l.at<unsigned long long>(ps.d, MAPSC_COUNTERS));                                                                               \
    else GLAUNCH(ctx, "k_score_mapped", (k_score_mapped<TT, false>), seg_grid(rchunks, S), dim3(GASM_WG), lds_bytes, rd.view(), ci, rec, rec_gap, ft, kmer, \
                 partial ? 1u : 0u, reads_per_wg, rchunks, lds_paths, d_cnt, d_fx, (u64)P, l.at<u32>(ps.d, MAPSC_PILE),                                 \
                 l.at<unsigned long long>(ps.d, MAPSC_COUNTERS))
        GASM_TABLES_SWITCH(T, GASM_LAUNCH_MAPSCORE)
#undef GASM_LAUNCH_MAPSCORE
    }
    if (ci.have_graph) {
        PathSet pth = {};
        pth.p_off = ci.c_off; pth.seg_path_off = ci.seg_cstart; pth.n_segments = S;      // (words: not read without seg_empty)
        const u32 grid_p = (u32)std::max<u64>(1, std::min<u64>(ceil_div_u64(P, GASM_WG), (u64)ctx->n_cu * 8));
        int32_t* const o_br = l.at<int32_t>(ps.d, MAPSC_I32);
        for (u32 t = 0; t < T; ++t) {
            double* const o_bp = l.at<double>(ps.d, MAPSC_F64) + (size_t)t * 3 * P;
            GLAUNCH(ctx, "k_score_finish", k_score_finish, dim3(grid_p), dim3(GASM_WG), 0, pth, d_cnt, d_fx + (size_t)t * P, ft.p[t], (const u64*)nullptr, kmer,
                    std::ldexp(1.0, -tbs[t]->fix_shift), o_bp, o_bp + P, o_bp + 2 * (size_t)P, o_br, o_br + P, bs.d_seg_cstart.as<u32>() + S);
        }
    }
    ps.param[0] = T;
    ps.param[1] = gapped ? 1u : 0u;
    ps.queued = true;
    return GASM_OK;
}

int pipeline_fetch_mapped_scores(gasm_ctx* ctx, DevReads& rd, BuildState& bs) {
    return pass_fetch(ctx, bs.mapscore, mapscore_layout(bs.mapscore.param[0], bs.n_contigs, bs.n_contigs ? bs.contig_bases : 0, rd.n_segments),
                      "gasm_batch_fetch_mapped_scores", "gasm_batch_score_mapped");
}

bool pipeline_score_uses_graph(const DevReads& rd, const BuildState& graph, ScoreTable* const* tbs, u32 T) {
    if (!(graph.n_kmers > 0 && rd.n_reads > rd.n_empty && rd.min_len >= (u32)graph.k)) return false;
    const u64 max_reads = max_seg_reads(rd);
    for (u32 t = 0; t < T; ++t) if (tbs[t]->fixed_shift(max_reads) < 0) return false;
    return true;
}

// The part of the general scorer no table enters: the first occurrence of every read in every path as position counters
// (ss.d_poscnt, ss.d_total), and the output arrays for n_tables tables.  Arbitrary paths (or reads that do not all hold a
// k-mer): host-side sizes are needed — the caller has uploaded the paths or, for a build's contigs, read the build's report
// (pipeline_contig_paths_host)
static int score_positions(gasm_ctx* ctx, DevReads& rd, DevPaths& dp, ScoreState& ss, u32 n_tables) {
    ss.n_paths = dp.n_paths;
    const u32 S = rd.n_segments, P = dp.n_paths;
    const u64 TB = dp.total_bases;
    ss.stride = (size_t)P + 1;
    GCHK(ss.d_poscnt.ensure((TB + 1) * 4));
    GCHK(ss.d_total.ensure(((size_t)P + 1) * 4));
    GCHK(ss.d_out_f64.ensure(((size_t)P + 1) * 8 * 3 * n_tables));
    GCHK(ss.d_out_i32.ensure(((size_t)P + 1) * 4 * 2));
    HIPCHK(hipMemsetAsync(ss.d_poscnt.p, 0, (TB + 1) * 4, ctx->stream));
    HIPCHK(hipMemsetAsync(ss.d_total.p, 0, ((size_t)P + 1) * 4, ctx->stream));
    const PathSet ps = dp.view();
    const int w = (int)std::min<u32>(32, rd.min_len);
    if (P && TB && rd.n_reads > rd.n_empty && w >= 1) {
        // per-segment read tables (power of two, at least twice the reads) and the dense first-occurrence table
        std::vector<u64>& toff = ss.h_toff;
        toff.assign((size_t)S + 1, 0);
        std::vector<u64> foff((size_t)S + 1, 0);
        u64 max_bases = 0, max_reads = 0;
        for (u32 s = 0; s < S; ++s) {
            const u64 nbases = dp.h_seg_base_off[s + 1] - dp.h_seg_base_off[s];
            const u64 nreads = rd.h_seg_read_off[s + 1] - rd.h_seg_read_off[s];
            const u64 npaths = dp.h_seg_path_off[s + 1] - dp.h_seg_path_off[s];
            u64 slots = 2;
            while (slots < 2 * nreads) slots <<= 1;
            toff[s + 1] = toff[s] + slots;
            foff[s + 1] = foff[s] + npaths * nreads;
            max_bases = std::max(max_bases, nbases);
            max_reads = std::max(max_reads, nreads);
        }
        // the dense first-occurrence table holds paths x reads words: at most `budget` of them at a time, else the paths of
        // a segment are scored slice by slice (the read table is built once)
        const u64 budget = getenv("GASM_DBG_FIRST_BUDGET") ? (u64)atoll(getenv("GASM_DBG_FIRST_BUDGET")) : (2ull << 30);
        const bool sliced = foff[S] > budget;
        if (sliced && dp.h_p_off.size() != (size_t)P + 1) { gasm_set_error("paths x reads too large for one pass and the path offsets are not on the host"); return GASM_ERR_CAPACITY; }
        if (rd.n_reads > 0xFFFFFFF0ull || TB > 0xFFFFFFF0ull) { gasm_set_error("too many reads or path bases for 32-bit indices"); return GASM_ERR_CAPACITY; }
        GCHK(h2d(ctx, ss.d_tbl_off, toff.data(), toff.size() * 8));
        GCHK(h2d(ctx, ss.d_first_off, foff.data(), foff.size() * 8));
        GCHK(ss.d_seed.ensure(toff[S] * 8));
        GCHK(ss.d_gpos.ensure(toff[S] * 4));
        HIPCHK(hipMemsetAsync(ss.d_gpos.p, 0xFF, toff[S] * 4, ctx->stream));
        SeedTable st;
        st.seed = ss.d_seed.as<u64>();
        st.gpos = ss.d_gpos.as<u32>();
        st.tbl_off = ss.d_tbl_off.as<u64>();
        if (max_bases && max_reads) {
            GLAUNCH(ctx, "k_read_insert", k_read_insert, dim3(ceil_div_u64(max_reads, GASM_WG), S), dim3(GASM_WG), 0, rd.view(), st, w);
            if (!sliced) {
                GCHK(ss.d_first.ensure(foff[S] * 4 + 16));
                HIPCHK(hipMemsetAsync(ss.d_first.p, 0xFF, foff[S] * 4 + 16, ctx->stream));
                GLAUNCH(ctx, "k_path_scan", k_path_scan, dim3(ceil_div_u64(max_bases, GASM_WG), S), dim3(GASM_WG), 0, rd.view(), ps, st,
                        dp.seg_base_off_dev(), w, ss.d_first_off.as<u64>(), ss.d_first.as<u32>(), 0u, 0u, 0u);
                GLAUNCH(ctx, "k_first_to_poscnt", k_first_to_poscnt, dim3(ceil_div_u64(foff[S], GASM_WG)), dim3(GASM_WG), 0, ss.d_first.as<u32>(),
                        foff[S], ss.d_poscnt.as<u32>());
            } else {
                for (u32 s = 0; s < S; ++s) {
                    const u64 nreads = rd.h_seg_read_off[s + 1] - rd.h_seg_read_off[s];
                    const u32 p0 = dp.h_seg_path_off[s], p1 = dp.h_seg_path_off[s + 1];
                    if (!nreads || p0 == p1) continue;
                    const u32 step = (u32)std::max<u64>(1, std::min<u64>(budget / nreads, 0x7FFFFFFFull));
                    for (u32 a = p0; a < p1; a += step) {
                        const u32 e = (u32)std::min<u64>((u64)a + step, p1);
                        const u64 entries = (u64)(e - a) * nreads, bases = dp.h_p_off[e] - dp.h_p_off[a];
                        GCHK(ss.d_first.ensure(entries * 4 + 16));
                        HIPCHK(hipMemsetAsync(ss.d_first.p, 0xFF, entries * 4 + 16, ctx->stream));
                        if (bases) {
                            GLAUNCH(ctx, "k_path_scan", k_path_scan, dim3(ceil_div_u64(bases, GASM_WG), 1), dim3(GASM_WG), 0, rd.view(), ps, st,
                                    dp.seg_base_off_dev(), w, ss.d_first_off.as<u64>(), ss.d_first.as<u32>(), s, a, e);
                            GLAUNCH(ctx, "k_first_to_poscnt", k_first_to_poscnt, dim3(ceil_div_u64(entries, GASM_WG)), dim3(GASM_WG), 0,
                                    ss.d_first.as<u32>(), entries, ss.d_poscnt.as<u32>());
                        }
                    }
                }
            }
        }
    }
    if (P && rd.n_empty) {
        GCHK(h2d(ctx, ss.d_seg_empty, rd.h_seg_empty.data(), (size_t)S * 8));
        u32 maxp = 0;
        for (u32 s = 0; s < S; ++s) maxp = std::max(maxp, dp.h_seg_path_off[s + 1] - dp.h_seg_path_off[s]);
        if (maxp) hipLaunchKernelGGL(k_add_empty_reads, dim3(ceil_div_u64(maxp, GASM_WG), S), dim3(GASM_WG), 0, ctx->stream, ps,
                                     ss.d_seg_empty.as<u64>(), ss.d_poscnt.as<u32>(), ss.d_total.as<u32>());
    }
    return GASM_OK;
}

// path_freq counts (table rows, not probabilities) and the prob_dist offsets: the same for every table of a call
static int score_freq_and_pd_offsets(gasm_ctx* ctx, DevPaths& dp, int kmer, const ScoreTable& tb, bool want_pd, ScoreState& ss) {
    const u32 P = dp.n_paths;
    const PathSet ps = dp.view();
    if (P && ss.want_freq) {
        const size_t cells = (size_t)P * tb.n_table;
        GCHK(ss.d_freq.ensure(cells * 4));
        HIPCHK(hipMemsetAsync(ss.d_freq.p, 0, cells * 4, ctx->stream));
        GLAUNCH(ctx, "k_path_freq", k_path_freq, dim3(ceil_div_u64(P, GASM_WG / 64)), dim3(GASM_WG), 0, ps, ss.d_poscnt.as<u32>(),
                ss.d_total.as<u32>(), tb.d_row.as<int32_t>(), kmer, tb.n_table, ss.d_freq.as<u32>(), P);
    }
    ss.h_pd_off.clear();
    if (want_pd) {
        ss.h_pd_off.assign((size_t)P + 1, 0);
        for (u32 p = 0; p < P; ++p) {
            const u64 len = dp.h_p_off[p + 1] - dp.h_p_off[p];
            ss.h_pd_off[p + 1] = ss.h_pd_off[p] + (len >= (u64)kmer ? len - kmer + 1 : 0);
        }
        if (P) GCHK(h2d(ctx, ss.d_pd_off, ss.h_pd_off.data(), ss.h_pd_off.size() * 8));
    }
    return GASM_OK;
}

int pipeline_score_launch(gasm_ctx* ctx, DevReads& rd, DevPaths& dp, int kmer, ScoreTable* const* tbs, u32 T, bool want_freq, bool want_pd,
                          ScoreState& ss, const BuildState* graph) {
    if (T < 1 || T > GASM_MAX_TABLES) { gasm_set_error("n_tables must be 1..%d (got %u)", GASM_MAX_TABLES, T); return GASM_ERR_INVALID; }
    if (kmer < 0) { gasm_set_error("kmer must be >= 0"); return GASM_ERR_INVALID; }
    if (rd.n_segments != dp.n_segments) { gasm_set_error("reads and paths disagree on the number of segments"); return GASM_ERR_INVALID; }
    for (u32 t = 1; t < T; ++t) if (tbs[t]->n_table != tbs[0]->n_table) { gasm_set_error("the tables differ in their number of rows"); return GASM_ERR_INVALID; }
    HIPCHK(hipSetDevice(ctx->device));
    GasmRange range("gasm:score");
    ss.valid = false;
    ss.n_table = tbs[0]->n_table;
    ss.n_tables = T;
    ss.want_freq = want_freq && tbs[0]->n_table;
    ss.want_pd = want_pd;
    ss.graph = nullptr;
    if (graph && !want_freq && !want_pd && pipeline_score_uses_graph(rd, *graph, tbs, T)) return score_launch_graph(ctx, rd, dp, kmer, tbs, T, ss, *graph);
    GCHK(score_positions(ctx, rd, dp, ss, T));
    const u32 P = dp.n_paths;
    const PathSet ps = dp.view();
    const size_t stride = ss.stride;
    double* o_bp = ss.d_out_f64.as<double>();
    int32_t* o_br = ss.d_out_i32.as<int32_t>();
    ProbTables pt = {};
    for (u32 t = 0; t < T; ++t) pt.p[t] = tbs[t]->d_prob.as<double>();
    if (P) {
#define GASM_LAUNCH_REDUCE(TT)                                                                                                                  \
    GLAUNCH(ctx, "k_path_reduce", k_path_reduce<TT>, dim3(P), dim3(GASM_WG), 0, ps, ss.d_poscnt.as<u32>(), ss.d_total.as<u32>(), pt, kmer, o_bp, \
            o_bp + stride, o_bp + 2 * stride, (u64)(3 * stride), o_br, o_br + stride, P)
        GASM_TABLES_SWITCH(T, GASM_LAUNCH_REDUCE)
#undef GASM_LAUNCH_REDUCE
    }
    GCHK(score_freq_and_pd_offsets(ctx, dp, kmer, *tbs[0], want_pd, ss));
    if (want_pd && P) {
        const u64 per_table = ss.h_pd_off[P];
        GCHK(ss.d_pd.ensure((per_table * T + 1) * 8));
        for (u32 t = 0; t < T; ++t)
            GLAUNCH(ctx, "k_prob_dist", k_prob_dist, dim3(ceil_div_u64(P, GASM_WG / 64)), dim3(GASM_WG), 0, ps, pt.p[t], kmer, ss.d_pd_off.as<u64>(),
                    ss.d_pd.as<double>() + per_table * t, P);
    }
    ss.launched = true;
    return GASM_OK;
}

int pipeline_score_fetch(gasm_ctx* ctx, ScoreState& ss) {
    if (!ss.launched) { gasm_set_error("no scoring has been queued"); return GASM_ERR_STATE; }
    if (ss.valid) return GASM_OK;
    if (ss.graph) {
        if (ss.graph->pending) { gasm_set_error("scores fetched before the build's report was read"); return GASM_ERR_STATE; }
        ss.n_paths = ss.graph->n_contigs;
        if (ss.verify) {
            u32 bad = 0;
            HIPCHK(hipMemcpyAsync(&bad, ss.graph->d_flags.as<u32>() + GASM_FLAG_SCORE_MISMATCH, 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            if (bad) { gasm_set_error("GASM_SCORE_VERIFY: a read that fits its contig by the graph differs from the contig's text"); return GASM_ERR_STATE; }
        }
    }
    const u32 P = ss.n_paths, T = ss.n_tables;
    int32_t* o_br = ss.d_out_i32.as<int32_t>();
    int32_t* o_ln = o_br + ss.stride;
    ss.h_bp.resize((size_t)P * T); ss.h_nf.resize((size_t)P * T); ss.h_nl.resize((size_t)P * T); ss.h_breaks.resize(P); ss.h_len.resize(P);
    ss.h_freq.clear(); ss.h_pd.clear();
    std::vector<u32> h_fc;
    if (P) {
        for (u32 t = 0; t < T; ++t) {           // (one table: the three arrays, as ever)
            double* o_bp = ss.d_out_f64.as<double>() + (size_t)t * 3 * ss.stride;
            double* o_nf = o_bp + ss.stride;
            double* o_nl = o_nf + ss.stride;
            HIPCHK(hipMemcpyAsync(ss.h_bp.data() + (size_t)t * P, o_bp, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(ss.h_nf.data() + (size_t)t * P, o_nf, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(ss.h_nl.data() + (size_t)t * P, o_nl, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIPCHK(hipMemcpyAsync(ss.h_breaks.data(), o_br, (size_t)P * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(ss.h_len.data(), o_ln, (size_t)P * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (ss.want_freq) {
            h_fc.resize((size_t)P * ss.n_table);
            HIPCHK(hipMemcpyAsync(h_fc.data(), ss.d_freq.p, h_fc.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (ss.want_pd && ss.h_pd_off[P]) {
            ss.h_pd.resize(ss.h_pd_off[P] * T);
            HIPCHK(hipMemcpyAsync(ss.h_pd.data(), ss.d_pd.p, ss.h_pd_off[P] * 8 * T, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!h_fc.empty()) {
        // observed_breaks = count / total (lib/DeNovoAssembler.cpp:402); 0/0 = NaN as in the reference
        ss.h_freq.resize(h_fc.size());
        for (u32 p = 0; p < P; ++p) {
            const double tot = (double)ss.h_breaks[p];
            for (u32 j = 0; j < ss.n_table; ++j) ss.h_freq[(size_t)p * ss.n_table + j] = (double)h_fc[(size_t)p * ss.n_table + j] / tot;
        }
    }
    ss.valid = true;
    return GASM_OK;
}
