// kernels_mapgap.hip — gapped read mapping (include/gasm.h, "Gapped read mapping"): k_read_map's seeds and heads, then the heads of a read
// that lie on neighbouring diagonals of one contig are joined into a chain and verified as one alignment with gaps.
// One wave per read, GASM_MAPG_WAVES reads of one segment per workgroup and round, the workgroups of a segment on one XCD (seg_chunk),
// chunks of 64 k-mer positions taken first to last: grid and loops are k_read_map's (kernels_links.hip).  Two phases per read:
//   PHASE 1, HEADS.  k_read_map's walk (a second copy of it, on purpose: that kernel stays as it is): one look-up per lane and chunk
//   (kmer_contig), a seeded lane compares its (contig, diagonal) with the previous seeded lane's, one ballot per chunk, and a wave-uniform
//   loop over the heads that keeps head i of the read in lane i's registers (my_J, my_c, my_d).  Nothing is verified here: whether a head
//   stands alone is known only once the next head has been seen.
//   PHASE 2, CHAINS, a wave-uniform loop over the kept heads.  A chain is extended while the next head joins (same contig, 0 < |g| <=
//   max_gap, a non-empty window).  For every join the BREAKPOINT: the lanes stride the window 64 positions at a time, two compares per
//   lane (position t on the left diagonal, position t + G on the right one), two ballots; the cost of breaking at t is the left
//   diagonal's mismatches in front of t (running count + popcount of the ballot below the lane) plus the right diagonal's from t + G on
//   (its total less its running count: for a window of more than 64 positions a first pass takes the total, else the one ballot holds
//   it); a wave minimum over cost << 16 | t gives the smallest t among equals.  It goes into lane i's my_t.  Then the chain's pieces are
//   verified like k_read_map's block, the count starting at the sum of the gap lengths and stopping once it exceeds max_edits, and an
//   accepted chain walks its pieces once more for the pileup (one no-return atomic add per lane and base), adds its skipped contig bases
//   (a lane each) or its insertion (lane 0) to the gap pileup and 1 to the histogram.  Two 16-byte stores per read by lane 0.
//   COUNTERS as in k_read_map: per wave in scalars, one LDS atomic per non-zero counter and wave, one global atomic per non-zero counter
//   and workgroup.
// Every index is bounded before use: a head's contig is inside the segment (kmer_contig); every compare and every pileup add checks its
// read position against [0, len) and its contig position against [0, len(c)) although the rule's argument (include/gasm.h) says that the
// pieces lie inside both; a gap-pileup add checks its contig position likewise.
// have_graph = 0: the build holds no contig at all (its arrays may not exist): only short, skipped and unseeded are counted.
#include "contig_index.h"

#define GASM_MAPG_WAVES (GASM_WG / 64)

// lane i's value (i wave-uniform) as a scalar
__device__ __forceinline__ int lane_value(int v, u32 i) { return __builtin_amdgcn_readfirstlane(__shfl(v, (int)i, 64)); }

__device__ __forceinline__ u32 wave_min_u32(u32 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const u32 x = (u32)__shfl_xor((int)v, o, 64);
        v = x < v ? x : v;
    }
    return (u32)__builtin_amdgcn_readfirstlane((int)v);
}

template <class K>
__global__ void __launch_bounds__(GASM_WG) k_read_map_gapped(ReadSet rs, GraphView gv, const u64* __restrict__ link, const u32* __restrict__ e_cid,
                                                             const u64* __restrict__ c_off, const u32* __restrict__ seg_cstart, const u8* __restrict__ text,
                                                             int have_graph, u32 max_edits, u32 max_gap, u32 reads_per_wg, u32 chunks,
                                                             int32_t* __restrict__ rec, int32_t* __restrict__ rec_gap, u32* __restrict__ pile,
                                                             u32* __restrict__ gap_pile, u32* __restrict__ hist, unsigned long long* __restrict__ counters) {
    __shared__ u32 s_cnt[GASM_MAPG_COUNTERS];
    u32 seg, chunk;
    if (!seg_chunk(rs.n_segments, chunks, &seg, &chunk)) return;
    if (threadIdx.x < GASM_MAPG_COUNTERS) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const ContigIndex ci{link, e_cid, c_off, seg_cstart};
    const u32 lane = threadIdx.x & 63u;
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int k = gv.k;
    u32 elo = 0, ehi = 0, c_lo = 0, c_hi = 0;
    if (have_graph) {
        const u32 nb = 1u << gv.bbits;
        elo = gv.dstart[seg * nb]; ehi = gv.dstart[(seg + 1) * nb];
        c_lo = seg_cstart[seg]; c_hi = seg_cstart[seg + 1];
    }
    const bool graph = elo < ehi && c_lo < c_hi;
    const u64 rbeg = rs.seg_read_off[seg], rend = rs.seg_read_off[seg + 1];
    const u64 below_lane = (1ull << lane) - 1ull;
    u32 c_cnt[GASM_MAPG_COUNTERS] = {0, 0, 0, 0, 0, 0, 0, 0};                 // of this wave's reads (wave-uniform)
    for (u64 base = rbeg + (u64)chunk * reads_per_wg; base < rend; base += (u64)chunks * reads_per_wg) {
        const u64 end = base + reads_per_wg < rend ? base + reads_per_wg : rend;
        for (u64 r = base + wv; r < end; r += GASM_MAPG_WAVES) {
            u64 p0;
            u32 len;
            read_span(rs, r, &p0, &len);
            const u32 n = len >= (u32)k ? len - (u32)k + 1 : 0;
            u32 cls;                                                          // the read's counter
            u32 n_heads = 0, n_acc = 0, dropped = 0, b_ov = 0, b_cost = 0, b_c = 0, b_q = 0, b_ins = 0, b_del = 0;
            int b_d = 0, b_dq = 0;
            bool seeded_any = false;
            if (n == 0) cls = 0;
            else if (n > GASM_THREAD_KMER_CAP) cls = 1;
            else if (!graph) cls = 2;
            else {
                // ================= phase 1: the kept heads, head i in lane i
                u32 my_c = GASM_NONE32, prev_c = GASM_NONE32;                 // lane i: kept head i; the last seeded position before this chunk
                int my_d = 0, my_J = 0, my_t = 0, prev_d = 0;                 // my_t: the breakpoint behind head i (phase 2)
                const u32 nw = (n + 63u) >> 6;
                for (u32 w = 0; w < nw; ++w) {
                    const u32 j = (w << 6) + lane;
                    u32 cid = GASM_NONE32, off = 0;
                    if (j < n && !kmer_contig<K>(gv, ci, seg, elo, ehi, c_lo, c_hi, kmer_key_at<K>(rs.words, p0 + j, k), &cid, &off)) cid = GASM_NONE32;
                    const int d = (int)off - (int)j;
                    const u64 sm = __ballot(cid != GASM_NONE32);
                    if (!sm) continue;
                    seeded_any = true;
                    // ---- heads: compare with the previous seeded lane (inside the chunk), or with the carry
                    const u64 below = sm & below_lane;
                    const int src = below ? 63 - __builtin_clzll(below) : (int)lane;
                    u32 pc = (u32)__shfl((int)cid, src, 64);
                    int pd = __shfl(d, src, 64);
                    if (!below) { pc = prev_c; pd = prev_d; }
                    u64 hb = __ballot(cid != GASM_NONE32 && (pc != cid || pd != d));
                    const int last = 63 - __builtin_clzll(sm);
                    prev_c = (u32)__builtin_amdgcn_readfirstlane(__shfl((int)cid, last, 64));
                    prev_d = __builtin_amdgcn_readfirstlane(__shfl(d, last, 64));
                    // ---- the head loop (wave-uniform)
                    while (hb) {
                        const int L = __builtin_ctzll(hb);
                        hb &= hb - 1;
                        const u32 h_c = (u32)__builtin_amdgcn_readfirstlane(__shfl((int)cid, L, 64));
                        const int h_d = __builtin_amdgcn_readfirstlane(__shfl(d, L, 64));
                        if (__ballot(lane < n_heads && my_c == h_c && my_d == h_d)) continue;      // A, B, A
                        if (n_heads == GASM_MAP_BLOCKS) { ++dropped; continue; }
                        if (lane == n_heads) { my_c = h_c; my_d = h_d; my_J = (int)(w << 6) + L; }
                        ++n_heads;
                    }
                }
                // ================= phase 2: the chains (wave-uniform)
                u32 h = 0;
                while (h < n_heads) {
                    const u32 h0 = h;                                          // the chain's first head
                    const u32 c = (u32)lane_value((int)my_c, h0);
                    const int d1 = lane_value(my_d, h0), J1 = lane_value(my_J, h0);
                    const u64 cb = c_off[c];
                    const long long clen = (long long)(c_off[c + 1] - cb);
                    // does read base x differ from the contig base under it on diagonal dd?  (false outside the read or the contig)
                    auto differ = [&](long long x, int dd) -> bool {
                        const long long p = (long long)dd + x;
                        return x >= 0 && x < (long long)len && p >= 0 && p < clen && base_at(rs.words, p0 + (u64)x) != base_code(text[cb + (u64)p]);
                    };
                    // ---- how far the chain goes, and the breakpoint of every join
                    u32 e = h0, gaps = 0, ins = 0, del = 0;
                    int d = d1, J = J1;
                    while (e + 1 < n_heads) {
                        const u32 c2 = (u32)lane_value((int)my_c, e + 1);
                        const int d2 = lane_value(my_d, e + 1), J2 = lane_value(my_J, e + 1);
                        const int g = d2 - d, ag = g < 0 ? -g : g, G = g < 0 ? -g : 0;
                        if (c2 != c || g == 0 || (u32)ag > max_gap || J2 - G < J + 1) break;
                        const int wlo = J + 1, whi = J2 - G;                   // the window of t, both ends inside
                        const bool one_chunk = whi - wlo < 64;
                        u32 b_total = 0;                                       // the right diagonal's mismatches over [wlo + G, J2)
                        if (!one_chunk)
                            for (int t0 = wlo; t0 < whi; t0 += 64) {
                                const int t = t0 + (int)lane;
                                b_total += (u32)__popcll(__ballot(t < whi && differ((long long)t + G, d2)));
                            }
                        u32 a_run = 0, b_run = 0, best = 0xFFFFFFFFu;
                        for (int t0 = wlo; t0 <= whi; t0 += 64) {
                            const int t = t0 + (int)lane;
                            const u64 ma = __ballot(t <= whi && differ((long long)t, d));
                            const u64 mb = __ballot(t < whi && differ((long long)t + G, d2));
                            if (one_chunk) b_total = (u32)__popcll(mb);
                            const u32 cost_t = a_run + (u32)__popcll(ma & below_lane) + b_total - b_run - (u32)__popcll(mb & below_lane);
                            const u32 m = wave_min_u32(t <= whi ? (cost_t << 16) | (u32)t : 0xFFFFFFFFu);
                            best = m < best ? m : best;
                            a_run += (u32)__popcll(ma);
                            b_run += (u32)__popcll(mb);
                        }
                        if (lane == e) my_t = (int)(best & 0xFFFFu);
                        gaps += (u32)ag; ins += (u32)G; del += g > 0 ? (u32)g : 0u;
                        d = d2; J = J2; ++e;
                    }
                    h = e + 1;
                    const int dq = d;
                    // ---- verify the pieces: piece i is read bases [s, en) on head i's diagonal
                    u32 cost = gaps, ov = 0;
                    bool ok = true;
                    long long s = d1 < 0 ? -(long long)d1 : 0;
                    for (u32 i = h0; i <= e; ++i) {
                        const int di = lane_value(my_d, i);
                        long long hi = clen - (long long)di;
                        if (hi > (long long)len) hi = (long long)len;
                        const long long en = i == e ? hi : (long long)lane_value(my_t, i);
                        if (en < hi) hi = en;
                        const long long lo = s < -(long long)di ? -(long long)di : s;
                        if (hi <= lo) { ok = false; break; }                   // (no finished build gives this: include/gasm.h, step 6)
                        for (long long i0 = lo; i0 < hi && cost <= max_edits; i0 += 64) {
                            const long long x = i0 + lane;
                            cost += (u32)__popcll(__ballot(x < hi && differ(x, di)));
                        }
                        if (cost > max_edits) { ok = false; break; }
                        ov += (u32)(hi - lo);
                        if (i < e) {
                            const int g = lane_value(my_d, i + 1) - di;
                            s = en + (g < 0 ? -(long long)g : 0);
                        }
                    }
                    if (!ok) continue;
                    // ---- accepted: pileup, gap pileup, histogram, best chain
                    s = d1 < 0 ? -(long long)d1 : 0;
                    for (u32 i = h0; i <= e; ++i) {
                        const int di = lane_value(my_d, i);
                        long long hi = clen - (long long)di;
                        if (hi > (long long)len) hi = (long long)len;
                        const long long en = i == e ? hi : (long long)lane_value(my_t, i);
                        if (en < hi) hi = en;
                        const long long lo = s < -(long long)di ? -(long long)di : s;
                        for (long long i0 = lo; i0 < hi; i0 += 64) {
                            const long long x = i0 + lane;
                            if (x < hi) atomicAdd(&pile[4 * (cb + (u64)((long long)di + x)) + base_at(rs.words, p0 + (u64)x)], 1u);
                        }
                        if (i < e) {
                            const int g = lane_value(my_d, i + 1) - di;
                            const long long p = (long long)di + en;            // the contig base at the breakpoint
                            if (g > 0) {                                       // a deletion: contig bases p .. p + g - 1 are skipped
                                const long long pp = p + lane;
                                if ((int)lane < g && pp >= 0 && pp < clen) atomicAdd(&gap_pile[2 * (cb + (u64)pp)], 1u);
                                s = en;
                            } else {                                           // an insertion in front of contig base p
                                if (lane == 0 && p >= 0 && p < clen) atomicAdd(&gap_pile[2 * (cb + (u64)p) + 1], 1u);
                                s = en - (long long)g;
                            }
                        }
                    }
                    if (lane == 0) atomicAdd(&hist[(size_t)seg * (max_edits + 1) + cost], 1u);
                    if (n_acc == 0 || ov > b_ov || (ov == b_ov && cost < b_cost)) {
                        b_ov = ov; b_cost = cost; b_c = c; b_d = d1; b_q = e - h0 + 1; b_ins = ins; b_del = del; b_dq = dq;
                    }
                    ++n_acc;
                }
                cls = !seeded_any ? 2u : n_acc == 0 ? 3u : n_acc == 1 ? 4u : 5u;
            }
            if (lane == 0) {
                int4 v, w;
                v.x = n_acc ? (int)(b_c - c_lo) : -1; v.y = n_acc ? b_d : 0;
                v.z = n_acc ? (int)(b_cost | (n_acc << 16)) : 0; v.w = (int)b_ov;
                w.x = (int)b_q; w.y = (int)b_ins; w.z = (int)b_del; w.w = n_acc ? b_dq : 0;
                *reinterpret_cast<int4*>(rec + r * 4) = v;
                *reinterpret_cast<int4*>(rec_gap + r * 4) = w;
            }
#pragma unroll
            for (u32 f = 0; f < 6; ++f) c_cnt[f] += cls == f ? 1u : 0u;
            c_cnt[6] += dropped;
            c_cnt[7] += n_acc && b_q >= 2 ? 1u : 0u;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (u32 f = 0; f < GASM_MAPG_COUNTERS; ++f)
            if (c_cnt[f]) atomicAdd(&s_cnt[f], c_cnt[f]);
    }
    __syncthreads();
    if (threadIdx.x < GASM_MAPG_COUNTERS && s_cnt[threadIdx.x]) atomicAdd(&counters[(size_t)seg * GASM_MAPG_COUNTERS + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}
template __global__ void k_read_map_gapped<u64>(ReadSet, GraphView, const u64*, const u32*, const u64*, const u32*, const u8*, int, u32, u32, u32, u32, int32_t*, int32_t*, u32*,
                                                u32*, u32*, unsigned long long*);
template __global__ void k_read_map_gapped<K128>(ReadSet, GraphView, const u64*, const u32*, const u64*, const u32*, const u8*, int, u32, u32, u32, u32, int32_t*, int32_t*, u32*,
                                                 u32*, u32*, unsigned long long*);
