// contig_index.h — what the kernels that lay reads over a finished build share (kernels_links.hip, kernels_map.hip, kernels_correct.hip):
// where a k-mer lies on the contigs (ContigIndex, kmer_contig), a base of a packed stream (base_at), and the frame of a pass over the
// reads: the workgroup's segment and wave (ReadPass), the loop over a wave's reads (for_wave_reads), the counter flush
// (flush_wave_counters).
// Where an edge lies: list ranking left (head, distance) on every edge (link), the head carries the contig's id (e_cid), the contig's
// bases start at c_off[id] — what k_score_reads_graph and k_contig_cov go by.  An edge of an isolated cycle has no head and lies in no
// contig: for these kernels it is not there.
#pragma once
#include "kernels.h"

// the contig (index in the batch) and the offset in it of the k-mer `key` of segment `seg`, whose edges are [elo, ehi) and whose contigs
// are [c_lo, c_hi): false if the k-mer is not in the build's set or lies in no contig.  Every index is checked before it is used.
template <class K>
__device__ __forceinline__ bool kmer_contig(const GraphView& gv, const ContigIndex& ci, u32 seg, u32 elo, u32 ehi, u32 c_lo, u32 c_hi, const K& key, u32* cid,
                                            u32* off) {
    u32 hi;
    const u32 e = graph_lower_bound<K>(gv, seg, key, &hi);
    if (e >= hi || e >= ehi || !keq(reinterpret_cast<const K*>(gv.dk_key)[e], key)) return false;
    const u64 l = ci.link[e];
    const u32 a = (u32)(l >> 32);
    if (a == GASM_NONE32 || !(l & GASM_LINK_DONE) || a < elo || a >= ehi) return false;
    const u32 c = ci.e_cid[a];
    if (c < c_lo || c >= c_hi) return false;
    *cid = c;
    *off = (u32)l & 0x7FFFFFFFu;
    return true;
}

// base p of a packed stream
__device__ __forceinline__ u32 base_at(const u64* __restrict__ w, u64 p) { return (u32)(w[p >> 5] >> (62 - 2 * (u32)(p & 31))) & 3u; }

// ================================================================================================================
// The frame of a pass over the reads.  The workgroups of a segment share an XCD (seg_chunk: the segment's k-mers and directories stay in
// one L2), workgroup `chunk` of `chunks` takes every chunks-th group of reads_per_wg reads of the segment, a wave every
// GASM_READ_WAVES-th read of a group.  What a wave counts it keeps in scalars (c_cnt, wave-uniform); the workgroup sums them in LDS
// (s_cnt) and adds each non-zero counter to the segment's once.
// ================================================================================================================
#define GASM_READ_WAVES (GASM_WG / 64)

struct ReadPass {
    u32 seg, chunk, lane, wv;  // the workgroup's segment and its share of it; the thread's lane and (as a scalar) wave
    int k;
    u32 elo, ehi, c_lo, c_hi;  // the segment's edges and contigs (all 0 without a ContigIndex, or one of have_graph = 0)
    bool graph;                // the segment holds an edge and a contig
    u64 rbeg, rend;            // the segment's reads
};

// false: a padding workgroup (seg_chunk), which returns at once.  Zeroes s_cnt; contains a barrier.  ci = nullptr: a pass that needs the
// k-mer set only
template <u32 N>
__device__ __forceinline__ bool read_pass_begin(ReadPass& f, const ReadSet& rs, const GraphView& gv, const ContigIndex* ci, u32 chunks, u32 (&s_cnt)[N]) {
    if (!seg_chunk(rs.n_segments, chunks, &f.seg, &f.chunk)) return false;
    if (threadIdx.x < N) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    f.lane = threadIdx.x & 63u;
    f.wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    f.k = gv.k;
    f.rbeg = rs.seg_read_off[f.seg]; f.rend = rs.seg_read_off[f.seg + 1];
    f.elo = f.ehi = f.c_lo = f.c_hi = 0;
    if (ci && ci->have_graph) {
        const u32 nb = 1u << gv.bbits;
        f.elo = gv.dstart[f.seg * nb]; f.ehi = gv.dstart[(f.seg + 1) * nb];
        f.c_lo = ci->seg_cstart[f.seg]; f.c_hi = ci->seg_cstart[f.seg + 1];
    }
    f.graph = f.elo < f.ehi && f.c_lo < f.c_hi;
    return true;
}

// kmer_contig inside the frame's segment
template <class K>
__device__ __forceinline__ bool kmer_contig(const GraphView& gv, const ContigIndex& ci, const ReadPass& f, const K& key, u32* cid, u32* off) {
    return kmer_contig<K>(gv, ci, f.seg, f.elo, f.ehi, f.c_lo, f.c_hi, key, cid, off);
}

// g(r) for every read r of this wave, the whole wave in step (the idiom of for_seg_edges): the grid loops where a segment holds more
// reads than it covers at once
template <class F>
__device__ __forceinline__ void for_wave_reads(const ReadPass& f, u32 reads_per_wg, u32 chunks, F&& g) {
    for (u64 base = f.rbeg + (u64)f.chunk * reads_per_wg; base < f.rend; base += (u64)chunks * reads_per_wg) {
        const u64 end = base + reads_per_wg < f.rend ? base + reads_per_wg : f.rend;
        for (u64 r = base + f.wv; r < end; r += GASM_READ_WAVES) g(r);
    }
}

// the end of a pass: one LDS atomic per non-zero counter and wave, a barrier, one global atomic per non-zero counter and workgroup onto
// dst[0 .. N) (the segment's counters, zeroed by the caller: 32-bit or 64-bit)
template <u32 N, class T>
__device__ __forceinline__ void flush_wave_counters(const u32 (&c_cnt)[N], u32 (&s_cnt)[N], T* __restrict__ dst) {
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (u32 i = 0; i < N; ++i)
            if (c_cnt[i]) atomicAdd(&s_cnt[i], c_cnt[i]);
    }
    __syncthreads();
    if (threadIdx.x < N && s_cnt[threadIdx.x]) atomicAdd(&dst[threadIdx.x], (T)s_cnt[threadIdx.x]);
}
