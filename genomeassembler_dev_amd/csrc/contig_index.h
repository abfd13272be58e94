// contig_index.h — where a k-mer of a finished build lies on the contigs, and a base of a packed stream: what the kernels that lay reads
// over contigs share (kernels_links.hip, kernels_mapgap.hip).
// Where an edge lies: list ranking left (head, distance) on every edge (link), the head carries the contig's id (e_cid), the contig's
// bases start at c_off[id] — what k_score_reads_graph and k_contig_cov go by.  An edge of an isolated cycle has no head and lies in no
// contig: for these kernels it is not there.
#pragma once
#include "kernels.h"

// what the kernels need of a finished build beside the k-mer directory
struct ContigIndex {
    const u64* link;       // per edge: head << 32 | done << 31 | distance
    const u32* e_cid;      // at a head: its contig
    const u64* c_off;      // per contig: its first base in the batch's contig text (+ the end of the last)
    const u32* seg_cstart; // n_segments + 1 contig indices
};

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
