// kernels_links.hip — the graph between the contigs of a finished build and the reads' evidence on it (include/gasm.h, "Contig links"):
//   k_contig_links    one thread per contig: the contigs its last node leads to (succ) and the ones that lead to its first node (pred)
//   k_read_thread     one wave per read: every k-mer's contig and offset, the crossings from contig to contig (link support) and the
//                     short contigs a read passes through from an in-edge to an out-edge (span support)
//   k_pair_place      one lane per mate: where the two mates of a read pair lie on the contigs (include/gasm.h, "Read pairs")
// All read the build's arrays only.  Where an edge lies (ContigIndex, kmer_contig), a base of a packed stream (base_at) and the frame of
// the two passes over the reads (ReadPass: segment, wave, the segment's edges and contigs, the counter flush): contig_index.h.
#include "contig_index.h"

// ================================================================================================================
// succ / pred.  Contig c ends at node v(c) = its last k-1 bases and starts at node u(c) = its first k-1 bases (from the contig text, as
// k_contig_twin takes its k-mer).  The four candidate out-edges of v are v followed by A, C, G, T, the four candidate in-edges of u are
// A, C, G, T followed by u: eight independent look-ups, each the bucket pair, the bin pair and a key of graph_lower_bound, then the
// edge's link and its head's contig.  A contig ends at a branching node or at a dead end, so an out-edge of v(c) that exists is the
// FIRST edge of its contig (distance 0) and an in-edge of u(c) the LAST of its (distance = edges - 1): anything else is left as "none".
//   succ[4 c + x] = index inside the segment of the contig whose first k-mer is v(c) + x, pred[4 c + x] the one whose last k-mer is
//   x + u(c); 0xFFFFFFFF (the caller filled both arrays with it) where there is none.
// ================================================================================================================
template <class K>
__global__ void __launch_bounds__(GASM_WG) k_contig_links(GraphView gv, ContigIndex ci, u32 n_segments, u32* __restrict__ succ, u32* __restrict__ pred) {
    const u64* __restrict__ const c_off = ci.c_off;
    const u32* __restrict__ const seg_cstart = ci.seg_cstart;
    const u8* __restrict__ const text = ci.text;
    const u32 n = seg_cstart[n_segments];
    const u32 nb = 1u << gv.bbits;
    const int k = gv.k;
    for (u32 c = blockIdx.x * GASM_WG + threadIdx.x; c < n; c += gridDim.x * GASM_WG) {
        const u32 seg = upper_seg<u32>(seg_cstart, n_segments, c);
        const u32 elo = gv.dstart[seg * nb], ehi = gv.dstart[(seg + 1) * nb];
        const u32 c_lo = seg_cstart[seg], c_hi = seg_cstart[seg + 1];
        const u64 beg = c_off[c], end = c_off[c + 1];
        if (end - beg < (u64)k) continue;                                     // (no contig is shorter than one k-mer)
        K u = key_from_u64<K>(0), v = key_from_u64<K>(0);
        for (int i = 0; i < k - 1; ++i) {
            u = kor(kshl(u, 2), key_from_u64<K>(base_code(text[beg + i])));
            v = kor(kshl(v, 2), key_from_u64<K>(base_code(text[end - (u64)(k - 1) + i])));
        }
        u32 cid[8], off[8];
        bool ok[8];
#pragma unroll
        for (u32 x = 0; x < 4; ++x) {
            ok[x] = kmer_contig<K>(gv, ci, seg, elo, ehi, c_lo, c_hi, kor(kshl(v, 2), key_from_u64<K>(x)), &cid[x], &off[x]);
            ok[4 + x] = kmer_contig<K>(gv, ci, seg, elo, ehi, c_lo, c_hi, kor(kshl(key_from_u64<K>(x), 2 * (k - 1)), u), &cid[4 + x], &off[4 + x]);
        }
#pragma unroll
        for (u32 x = 0; x < 4; ++x) {
            if (ok[x] && off[x] == 0) succ[4 * (size_t)c + x] = cid[x] - c_lo;
            if (ok[4 + x]) {
                const u64 edges = c_off[cid[4 + x] + 1] - c_off[cid[4 + x]] - (u64)(k - 1);
                if ((u64)off[4 + x] + 1 == edges) pred[4 * (size_t)c + x] = cid[4 + x] - c_lo;
            }
        }
    }
}
template __global__ void k_contig_links<u64>(GraphView, ContigIndex, u32, u32*, u32*);
template __global__ void k_contig_links<K128>(GraphView, ContigIndex, u32, u32*, u32*);

// are the bits lo .. hi (inclusive) of the in-set words all set?  Word `w_now` is `m_now` (this chunk's ballot), the words behind it are
// in LDS; lo >> 6 >= w_now
__device__ __forceinline__ bool run_in_set(const u64* in, u32 lo, u32 hi, u32 w_now, u64 m_now) {
    for (u32 q = lo >> 6; q <= (hi >> 6); ++q) {
        const u64 word = q == w_now ? m_now : in[q];
        u64 need = ~0ull;
        if (q == (lo >> 6)) need &= ~0ull << (lo & 63u);
        if (q == (hi >> 6)) need &= ~0ull >> (63u - (hi & 63u));
        if ((word & need) != need) return false;
    }
    return true;
}

// ================================================================================================================
// Threading.  One wave per read, GASM_READ_WAVES reads of one segment per workgroup and round (ReadPass), chunks of 64 k-mer
// positions, as k_read_correct.  A gather like it: a look-up costs the three
// dependent requests of graph_lower_bound + the key, then the edge's link and the head's contig id — but only the first position of a
// chunk and the positions behind a place where the read leaves its contig's text make one (below): the kernel is bound by the requests
// it sends to L2, and most positions of a read follow their predecessor inside one contig.
// The chunks are taken LAST FIRST.  Position j asks two things of the positions behind it: where position j + 1 lies (a crossing of link
// (a, b): both in the set, and another contig or an offset that does not advance by one), and, once it crossed into a contig r of at
// most span_len bases, whether the n(r) + 1 positions j + 1 .. j + 1 + n(r) are all in the set.  Going backwards both are known when j's
// turn comes: the neighbour inside the chunk is a cross-lane move, across the 63|64 seam it is lane 0 of the chunk before (v_readlane,
// carried in a scalar), and "in the set" is one ballot per chunk, kept in LDS (64 words per wave for GASM_THREAD_KMER_CAP positions — the
// only thing a later position needs of an earlier chunk, so contig and offset never leave the registers).
// r is unbranched inside: after a crossing into r, a run of n(r) + 1 further positions in the set is r followed by one of its
// out-edges (include/gasm.h), so the run of bits is the whole test.  x = first base of k-mer j, y = last base of k-mer j + 1 + n(r).
//   link_support[4 a + last base of k-mer j + 1] += 1 per crossing, span_support[16 r + 4 x + y] += 1 per span (a, r: indices in the
//   batch); skipped[seg] += 1 per read of more than GASM_THREAD_KMER_CAP k-mers (the pass's one counter: flush_wave_counters).  All
//   zeroed by the caller; integer atomics: exact.
// ci.have_graph = 0: only `skipped` is counted.
// ================================================================================================================
template <class K>
__global__ void __launch_bounds__(GASM_WG) k_read_thread(ReadSet rs, GraphView gv, ContigIndex ci, u32 span_len, u32 reads_per_wg, u32 chunks,
                                                         u32* __restrict__ link_support, u32* __restrict__ span_support,
                                                         unsigned long long* __restrict__ skipped) {
    __shared__ u64 s_in[GASM_READ_WAVES][GASM_THREAD_KMER_CAP / 64];
    __shared__ u32 s_cnt[1];
    ReadPass rp;
    if (!read_pass_begin(rp, rs, gv, &ci, chunks, s_cnt)) return;
    const u64* __restrict__ const c_off = ci.c_off;
    const u8* __restrict__ const text = ci.text;
    const u32 lane = rp.lane;
    u64* const in = s_in[rp.wv];
    const int k = rp.k;
    u32 c_cnt[1] = {0};                                                       // of this wave's reads (wave-uniform)
    for_wave_reads(rp, reads_per_wg, chunks, [&](u64 r) {
        u64 p0;
        u32 len;
        read_span(rs, r, &p0, &len);
        if (len < (u32)k) return;
        const u32 n = len - (u32)k + 1;
        if (n > GASM_THREAD_KMER_CAP) { ++c_cnt[0]; return; }
        if (!rp.graph) return;
        u32 nx_cid = GASM_NONE32, nx_off = 0;                             // position 64 (w + 1): lane 0 of the chunk before (none yet)
        // the first position of every chunk, looked up by lane w for chunk w: one round of dependent requests for the whole read
        const u32 nw = (n + 63u) >> 6;
        u32 f_cid = GASM_NONE32, f_off = 0;
        if (lane < nw && !kmer_contig<K>(gv, ci, rp, kmer_key_at<K>(rs.words, p0 + (lane << 6), k), &f_cid, &f_off)) f_cid = GASM_NONE32;
        for (u32 w = nw; w-- > 0;) {
            const u32 j = (w << 6) + lane;
            u32 cid = GASM_NONE32, off = 0;
            // ---- the chunk's first position was looked up ahead of the loop.  Where it lies in a contig, the positions behind it that
            // read on as the contig's text does lie in the same contig at the next offsets (k-mer j + 1 is k-mer j without its first
            // base plus one more): one compare of the read's bases with the contig's text tells how far, and only the lanes behind
            // the first difference, or behind the contig's end, look up for themselves
            const u32 s_cid = (u32)__builtin_amdgcn_readlane((int)f_cid, (int)w), s_off = (u32)__builtin_amdgcn_readlane((int)f_off, (int)w);
            bool known = lane == 0;
            if (known) { cid = s_cid; off = s_off; }
            if (s_cid != GASM_NONE32) {
                const u64 cb = c_off[s_cid], edges = c_off[s_cid + 1] - cb - (u64)(k - 1);
                const bool same = lane == 0 || (j < n && (u64)s_off + lane < edges &&
                                                base_at(rs.words, p0 + j + (u32)k - 1) == base_code(text[cb + s_off + lane + (u32)k - 1]));
                const u64 differ = ~__ballot(same);
                if (lane < (differ ? (u32)__builtin_ctzll(differ) : 64u)) { cid = s_cid; off = s_off + lane; known = true; }
            }
            if (!known && j < n && !kmer_contig<K>(gv, ci, rp, kmer_key_at<K>(rs.words, p0 + j, k), &cid, &off)) cid = GASM_NONE32;
            const u64 m = __ballot(cid != GASM_NONE32);
            if (lane == 0) in[w] = m;
            __builtin_amdgcn_wave_barrier();
            u32 ncid = (u32)__shfl_down((int)cid, 1, 64), noff = (u32)__shfl_down((int)off, 1, 64);
            if (lane == 63) { ncid = nx_cid; noff = nx_off; }
            nx_cid = (u32)__builtin_amdgcn_readfirstlane((int)cid);
            nx_off = (u32)__builtin_amdgcn_readfirstlane((int)off);
            if (cid == GASM_NONE32 || ncid == GASM_NONE32 || (ncid == cid && noff == off + 1)) continue;
            // ---- a crossing of (cid, ncid) between positions j and j + 1
            atomicAdd(&link_support[4 * (size_t)cid + base_at(rs.words, p0 + j + (u32)k)], 1u);
            if (!span_len) continue;
            const u64 rlen = c_off[ncid + 1] - c_off[ncid];
            if (rlen > (u64)span_len || rlen < (u64)k) continue;
            const u32 last = j + 1 + (u32)(rlen - (u64)(k - 1));          // the position of the out-edge behind ncid
            if (last >= n || !run_in_set(in, j + 1, last, w, m)) continue;
            atomicAdd(&span_support[16 * (size_t)ncid + 4 * base_at(rs.words, p0 + j) + base_at(rs.words, p0 + last + (u32)k - 1)], 1u);
        }
    });
    flush_wave_counters(c_cnt, s_cnt, skipped + rp.seg);
}
template __global__ void k_read_thread<u64>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32*, u32*, unsigned long long*);
template __global__ void k_read_thread<K128>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32*, u32*, unsigned long long*);

// ================================================================================================================
// Read pairs (include/gasm.h, "Read pairs").  Reads 2p and 2p + 1 of a segment are the mates of pair p; an ORIENTED pair (first, second)
// is placed by two SCANS: the first in-set k-mer of `first` as given, and the first k-mer of `second` whose reverse complement is in the
// set (key_revcomp: the reads are taken as the batch holds them, whatever the build's strands — the both-strand stream has another read
// numbering and would save one ALU op per look-up of a kernel that waits on L2).  orient = 2 (after a strands = 2 build) adds
// (mate 2, mate 1): four scans per pair, two otherwise.
// Layout: ONE LANE PER SCAN, lane = (pair in the wave) * 2 orient + orientation * 2 + role, role 0 = `first`, role 1 = `second`: 32 or 16
// pairs per wave, 4 waves of pairs per workgroup and round, in k_read_thread's frame (ReadPass) with a loop of its own: over pairs.
//   1. every lane looks up position 0 of its mate: after a good build nearly every mate hits there, so one round of dependent requests
//      (graph_lower_bound's three + the key, the edge's link, the head's contig id) places 64 scans at once;
//   2. the lanes that missed are taken one after the other by the whole wave: 64 positions per chunk from position 1 on, one look-up per
//      lane, ballot, first set bit, next chunk — a mate without any k-mer in the set costs one look-up per k-mer, as in k_read_correct;
//   3. the two roles of an oriented pair sit in neighbouring lanes: the even lane takes (c2, E) from the odd one, writes the record as
//      one 16-byte store, classifies, and adds to its histogram bin (a no-return atomic; the bins of a segment are few and hot, which
//      the memory side serialises — measured in profiles/pairs/README.md).  The six counters are ballots summed per wave in
//      scalars, then flush_wave_counters.
// A pair with a mate of more than GASM_THREAD_KMER_CAP k-mers is skipped before any look-up.  rec: 4 int32 per oriented pair at
// (o * n_pairs + p) * 4 (16-byte aligned), every pair of every segment written; hist: max_insert + 1 bins per segment, counters:
// GASM_PAIR_COUNTERS per segment, both zeroed by the caller.  Every segment holds an even number of reads (the host checked).
// ci.have_graph = 0: no mate is placed.
// ================================================================================================================
template <class K>
__global__ void __launch_bounds__(GASM_WG) k_pair_place(ReadSet rs, GraphView gv, ContigIndex ci, u32 orient, u32 max_insert, u64 n_pairs, u32 chunks,
                                                        int32_t* __restrict__ rec, u32* __restrict__ hist, unsigned long long* __restrict__ counters) {
    __shared__ u32 s_cnt[GASM_PAIR_COUNTERS];
    ReadPass rp;
    if (!read_pass_begin(rp, rs, gv, &ci, chunks, s_cnt)) return;
    const u32 seg = rp.seg, lane = rp.lane, wv = rp.wv, c_lo = rp.c_lo;
    const int k = rp.k;
    const u64 pbeg = rp.rbeg >> 1, pend = rp.rend >> 1;
    const u32 two = orient == 2 ? 1u : 0u;
    const u32 role = lane & 1u, o = two ? (lane >> 1) & 1u : 0u, lp = lane >> (1 + two);
    const u32 pairs_per_wave = 32u >> two, pairs_per_wg = GASM_READ_WAVES * pairs_per_wave;
    u32 c_cnt[GASM_PAIR_COUNTERS] = {0, 0, 0, 0, 0, 0};                       // of this wave's oriented pairs (wave-uniform)
    for (u64 base = pbeg + (u64)rp.chunk * pairs_per_wg; base < pend; base += (u64)chunks * pairs_per_wg) {
        const u64 p = base + (u64)wv * pairs_per_wave + lp;
        const bool valid = p < pend;
        u64 p0 = 0;
        u32 n = 0;                                                            // k-mers of this lane's mate
        bool skip = false;
        if (valid) {
            const u32 mate = role ^ o;                                        // `first` is mate 1 in orientation 0, mate 2 in orientation 1
            u64 q0;
            u32 len, olen;
            read_span(rs, 2 * p + mate, &p0, &len);
            read_span(rs, 2 * p + (mate ^ 1u), &q0, &olen);
            n = len >= (u32)k ? len - (u32)k + 1 : 0;
            const u32 on = olen >= (u32)k ? olen - (u32)k + 1 : 0;
            skip = n > GASM_THREAD_KMER_CAP || on > GASM_THREAD_KMER_CAP;
        }
        const bool active = valid && !skip && rp.graph && n > 0;
        // ---- 1. position 0 of every mate
        bool found = false;
        u32 r_cid = GASM_NONE32;
        int r_pos = 0;                                                        // S of a `first`, E of a `second`
        if (active) {
            K key = kmer_key_at<K>(rs.words, p0, k);
            if (role) key = key_revcomp<K>(key, k);
            u32 cid, off;
            if (kmer_contig<K>(gv, ci, rp, key, &cid, &off)) {
                found = true; r_cid = cid; r_pos = role ? (int)off + k : (int)off;
            }
        }
        // ---- 2. the mates that missed, one after the other, 64 positions at a time
        u64 need = __ballot(active && !found && n > 1);
        while (need) {
            const int L = __builtin_ctzll(need);
            need &= need - 1;
            const u64 b_p0 = lane_word(p0, (u32)L);
            const u32 b_n = (u32)__builtin_amdgcn_readlane((int)n, L);
            const bool b_rc = (L & 1) != 0;
            for (u32 j0 = 1; j0 < b_n; j0 += 64) {
                const u32 j = j0 + lane;
                u32 cid = GASM_NONE32, off = 0;
                bool hit = false;
                if (j < b_n) {
                    K key = kmer_key_at<K>(rs.words, b_p0 + j, k);
                    if (b_rc) key = key_revcomp<K>(key, k);
                    hit = kmer_contig<K>(gv, ci, rp, key, &cid, &off);
                }
                const u64 m = __ballot(hit);
                if (!m) continue;
                const int f = __builtin_ctzll(m);
                const u32 h_cid = (u32)__builtin_amdgcn_readlane((int)cid, f), h_off = (u32)__builtin_amdgcn_readlane((int)off, f);
                const int i = (int)j0 + f;
                if ((int)lane == L) { found = true; r_cid = h_cid; r_pos = b_rc ? (int)h_off + k + i : (int)h_off - i; }
                break;
            }
        }
        // ---- 3. the record of every oriented pair, from its even lane
        const u32 n_cid = (u32)__shfl_down((int)r_cid, 1, 64);
        const int n_pos = __shfl_down(r_pos, 1, 64);
        const bool mine = valid && role == 0;
        u32 cls = GASM_PAIR_COUNTERS;
        if (mine) {
            const bool a = r_cid != GASM_NONE32, b = n_cid != GASM_NONE32;
            const int d = n_pos - r_pos;
            cls = skip ? 0u : !a && !b ? 1u : a != b ? 2u : r_cid != n_cid ? 5u : d > 0 ? 3u : 4u;
            int4 v;
            v.x = a ? (int)(r_cid - c_lo) : -1; v.y = a ? r_pos : 0;
            v.z = b ? (int)(n_cid - c_lo) : -1; v.w = b ? n_pos : 0;
            *reinterpret_cast<int4*>(rec + ((u64)o * n_pairs + p) * 4) = v;
            if (cls == 3u) atomicAdd(&hist[(size_t)seg * (max_insert + 1) + ((u32)d < max_insert ? (u32)d : max_insert)], 1u);
        }
#pragma unroll
        for (u32 f = 0; f < GASM_PAIR_COUNTERS; ++f) c_cnt[f] += (u32)__popcll(__ballot(cls == f));
    }
    flush_wave_counters(c_cnt, s_cnt, counters + (size_t)seg * GASM_PAIR_COUNTERS);
}
template __global__ void k_pair_place<u64>(ReadSet, GraphView, ContigIndex, u32, u32, u64, u32, int32_t*, u32*, unsigned long long*);
template __global__ void k_pair_place<K128>(ReadSet, GraphView, ContigIndex, u32, u32, u64, u32, int32_t*, u32*, unsigned long long*);
