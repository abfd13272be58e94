// kernels_map.hip — read mapping onto the contigs of a finished build, without gaps (include/gasm.h, "Read mapping") and with them
// ("Gapped read mapping"): ONE body, k_read_map<K, GAPPED, ENDS, TRACE>.  The heads of a read are found once for both; GAPPED = true joins the heads
// that lie on neighbouring diagonals of one contig into a chain and verifies it as one alignment with gaps, GAPPED = false takes every
// head as a chain of its own and compiles the rest out (the join loop, the breakpoints, my_J, my_t, the gap record, the gap pileup, the
// eighth counter).
// One wave per read, GASM_READ_WAVES reads of one segment per workgroup and round, chunks of 64 k-mer positions taken first to last:
// the frame of the passes over the reads (ReadPass, for_wave_reads, flush_wave_counters: contig_index.h).  Two phases per read:
//   PHASE 1, HEADS.
//     SEEDS.  One look-up per lane and chunk (kmer_contig): lane's position j, its contig and its diagonal d = offset - j.
//     HEADS.  A seeded lane compares its (contig, d) with the PREVIOUS SEEDED lane's: the highest set bit of the seed ballot below the
//     lane inside the chunk (one cross-lane move), the scalar carry (prev_c, prev_d) across the chunk seam.  One ballot per chunk.
//     HEAD LOOP, wave-uniform: a head is taken by count-trailing-zeros, its (contig, d) fetched from its lane, compared with the kept
//     heads — head i of the read sits in lane i's registers (my_c, my_d, my_J), so the compare is one ballot and the list takes no LDS.
//     Nothing is verified here: whether a head stands alone is known only once the next head has been seen.
//   PHASE 2, CHAINS, a wave-uniform loop over the kept heads.  A chain is extended while the next head joins (same contig, 0 < |g| <=
//   max_gap, a non-empty window).  For every join the BREAKPOINT: the lanes stride the window 64 positions at a time, two compares per
//   lane (position t on the left diagonal, position t + G on the right one), two ballots; the cost of breaking at t is the left
//   diagonal's mismatches in front of t (running count + popcount of the ballot below the lane) plus the right diagonal's from t + G on
//   (its total less its running count: for a window of more than 64 positions a first pass takes the total, else the one ballot holds
//   it); a wave minimum over cost << 16 | t gives the smallest t among equals.  It goes into lane i's my_t.  Then the chain's pieces
//   (for_pieces) are verified with the 64 lanes striding over each: read base from the packed stream, contig base from the build's
//   ASCII text, ballot and popcount, the count starting at the sum of the gap lengths and stopping once it exceeds max_edits.  An
//   accepted chain walks its pieces once more for the pileup (one no-return atomic add per lane and base), adds its skipped contig bases
//   (a lane each) or its insertion (lane 0) to the gap pileup and 1 to the histogram.  One 16-byte store per read and record by lane 0.
// Every index is bounded before use: a head's contig is inside the segment (kmer_contig); every compare and every pileup add checks its
// read position against [0, len) and its contig position against [0, len(c)) although the rule's argument (include/gasm.h) says that the
// pieces lie inside both; a gap-pileup add checks its contig position likewise.
// ci.have_graph = 0: only short, skipped and unseeded are counted.
// ENDS = true (with GAPPED; the launch "k_read_map_ends"; include/gasm.h, "End gaps") tries one gap at each end of every chain, between the
// read's end and the chain's outermost seed, before the pieces are verified.  Per end: one strided pass takes m0, the end's mismatches on
// the ungapped diagonal, and the wave leaves when m0 < 2 (nearly every read).  Else for |g| = 1 .. min(end_gap, m0 - 1), the deletion
// before the insertion, the breakpoint search of the joins runs once over the end's window (two ballots per 64 positions, running counts,
// a wave minimum over cost << 16 | t: t stays below 2^13 and a cost below 2^13 as well, both far inside their halves) and a candidate is
// kept only if it costs strictly less than the best so far, which starts at m0: that is the rule's key.  A taken gap adds a piece in front
// of or behind the chain's (for_pieces), its gap to the gap pileup as a join's, and the chain's savings say whether the gaps rescued it.
// ENDS = false compiles all of it out.
// TRACE = true (with GAPPED and ENDS; the launch "k_read_map_trace"; include/gasm.h, "Alignments") keeps the alignment that the other forms
// discard.  for_pieces is wave-uniform, so while a chain is verified lane i takes piece i of it (its clamped [lo, hi) and its diagonal) into
// two registers (cand_pc); a chain that becomes the read's best copies them to best_pc, zero in the lanes behind its last piece,
// and at the end lanes 0 .. GASM_MAP_PIECES - 1 store 8 bytes each into rec_piece: no LDS, no second walk.  Every accepted chain adds
// its inserted bases to ins_pile, one lane per base (trace_insertion), beside its add to gap_pile[2p + 1] and under the same bounds check.
// TRACE = false compiles all of it out: TracePieces<false> and TraceChain<false> are empty, and the other forms keep their kernel arguments
// (MapOutOf).
#include "contig_index.h"

// TRACE, lane i: piece i of a chain, s | e << 16 and its diagonal; of the chain at hand also n, the pieces walked so far (wave-uniform)
template <bool TRACE>
struct TracePieces {
    int se = 0, d = 0;
};
template <>
struct TracePieces<false> {};
template <bool TRACE>
struct TraceChain : TracePieces<TRACE> {
    u32 n = 0;
};
template <>
struct TraceChain<false> {};

// TRACE: an insertion of G read bases [t, t + G) of the read at p0 in front of base p of the contig at cb: column l of the W gets read base
// t + l, a lane each
__device__ __forceinline__ void trace_insertion(u32* __restrict__ ins_pile, const u64* __restrict__ words, u64 p0, u32 len, u64 cb, long long clen, u32 W, u32 lane,
                                                long long p, long long t, int G) {
    const long long x = t + lane;
    if ((int)lane < G && lane < W && p >= 0 && p < clen && x >= 0 && x < (long long)len)
        atomicAdd(&ins_pile[((cb + (u64)p) * W + lane) * 4 + base_at(words, p0 + (u64)x)], 1u);
}

template <class K, bool GAPPED, bool ENDS, bool TRACE>
__global__ void __launch_bounds__(GASM_WG) k_read_map(ReadSet rs, GraphView gv, ContigIndex ci, u32 max_edits, u32 max_gap, u32 end_gap, u32 reads_per_wg,
                                                      u32 chunks, MapOutOf<TRACE> out) {
    static_assert(GAPPED || !ENDS, "end gaps belong to the gapped form");
    static_assert(ENDS || !TRACE, "the alignment tables belong to the form with end gaps");
    constexpr u32 N_CNT = GAPPED ? GASM_MAPG_COUNTERS : GASM_MAP_COUNTERS;
    __shared__ u32 s_cnt[N_CNT];
    ReadPass rp;
    if (!read_pass_begin(rp, rs, gv, &ci, chunks, s_cnt)) return;
    const u64* __restrict__ const c_off = ci.c_off;
    const u8* __restrict__ const text = ci.text;
    const u32 lane = rp.lane;
    const int k = rp.k;
    const u64 below_lane = (1ull << lane) - 1ull;
    u32 c_cnt[N_CNT] = {};                                                    // of this wave's reads (wave-uniform)
    u32 c_end[ENDS ? GASM_MAPEND_COUNTERS : 1] = {};                          // front, back, rescued, start_moved
    for_wave_reads(rp, reads_per_wg, chunks, [&](u64 r) {
        u64 p0;
        u32 len;
        read_span(rs, r, &p0, &len);
        const u32 n = len >= (u32)k ? len - (u32)k + 1 : 0;
        u32 cls;                                                              // the read's counter
        u32 n_heads = 0, n_acc = 0, dropped = 0, b_ov = 0, b_cost = 0, b_c = 0, b_q = 0, b_ins = 0, b_del = 0;
        int b_d = 0, b_dq = 0;
        int b_gf = 0, b_tf = 0, b_gb = 0, b_tb = 0;                           // ENDS: the best chain's end gaps
        [[maybe_unused]] TracePieces<TRACE> best_pc;                          // TRACE, lane i: piece i of the best chain
        [[maybe_unused]] TraceChain<TRACE> cand_pc;                           // TRACE, lane i: piece i of the chain at hand
        bool seeded_any = false;
        if (n == 0) cls = 0;
        else if (n > GASM_THREAD_KMER_CAP) cls = 1;
        else if (!rp.graph) cls = 2;
        else {
            // ================= phase 1: the kept heads, head i in lane i
            u32 my_c = GASM_NONE32, prev_c = GASM_NONE32;                     // lane i: kept head i; the last seeded position before this chunk
            int my_d = 0, my_J = 0, my_t = 0, prev_d = 0;                     // my_t: the breakpoint behind head i (phase 2)
            const u32 nw = (n + 63u) >> 6;
            for (u32 w = 0; w < nw; ++w) {
                const u32 j = (w << 6) + lane;
                u32 cid = GASM_NONE32, off = 0;
                if (j < n && !kmer_contig<K>(gv, ci, rp, kmer_key_at<K>(rs.words, p0 + j, k), &cid, &off)) cid = GASM_NONE32;
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
                const u32 last = 63u - (u32)__builtin_clzll(sm);
                prev_c = (u32)lane_value((int)cid, last);
                prev_d = lane_value(d, last);
                // ---- the head loop (wave-uniform)
                while (hb) {
                    const int L = __builtin_ctzll(hb);
                    hb &= hb - 1;
                    const u32 h_c = (u32)lane_value((int)cid, (u32)L);
                    const int h_d = lane_value(d, (u32)L);
                    if (__ballot(lane < n_heads && my_c == h_c && my_d == h_d)) continue;      // A, B, A
                    if (n_heads == GASM_MAP_BLOCKS) { ++dropped; continue; }
                    if (lane == n_heads) {
                        my_c = h_c; my_d = h_d;
                        if constexpr (GAPPED) my_J = (int)(w << 6) + L;
                    }
                    ++n_heads;
                }
            }
            // ================= phase 2: the chains (wave-uniform)
            u32 h = 0;
            while (h < n_heads) {
                const u32 h0 = h;                                              // the chain's first head
                const u32 c = (u32)lane_value((int)my_c, h0);
                const int d1 = lane_value(my_d, h0);
                const u64 cb = c_off[c];
                const long long clen = (long long)(c_off[c + 1] - cb);
                // does read base x differ from the contig base under it on diagonal dd?  (false outside the read or the contig)
                auto differ = [&](long long x, int dd) -> bool {
                    const long long p = (long long)dd + x;
                    return x >= 0 && x < (long long)len && p >= 0 && p < clen && base_at(rs.words, p0 + (u64)x) != base_code(text[cb + (u64)p]);
                };
                // ---- how far the chain goes, and the breakpoint of every join
                u32 e = h0, gaps = 0, ins = 0, del = 0;
                int d = d1;
                if constexpr (GAPPED) {
                    int J = lane_value(my_J, h0);
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
                }
                h = e + 1;
                // ---- ENDS: one gap or none at either end (include/gasm.h, "End gaps", 5a and 5b)
                int gf = 0, tf = 0, gb = 0, tb = 0;                            // the taken gaps and their breakpoints (g = 0: none)
                u32 saved = 0;                                                 // m0 - cost over the taken gaps
                if constexpr (ENDS) {
                    const int J1 = lane_value(my_J, h0), Jq = lane_value(my_J, e);
                    for (int side = 0; side < 2; ++side) {
                        // the window [w0, w1) of the end, its ungapped diagonal dn (the chain's nearest) and whether it is eligible
                        const int w0 = side ? Jq + k : 0, w1 = side ? (int)len : J1;
                        const int dn = side ? d : d1;
                        if (w1 <= w0 || (side ? (long long)dn + (long long)len > clen : dn < 0)) continue;
                        u32 m0 = 0;
                        for (int x0 = w0; x0 < w1; x0 += 64) {
                            const int x = x0 + (int)lane;
                            m0 += (u32)__popcll(__ballot(x < w1 && differ((long long)x, dn)));
                        }
                        if (m0 < 2) continue;
                        u32 best_cost = m0;
                        int best_g = 0, best_t = 0;
                        for (int ag = 1; (u32)ag <= end_gap && (u32)ag < best_cost; ++ag)
                            for (int sg = 0; sg < 2; ++sg) {                   // the deletion first
                                const int g = sg ? -ag : ag, G = sg ? ag : 0;
                                // front: the piece [0, t) on dl = d_1 - g, then [t + G, J_1) on d_1; back: [B, t) on d_q, then [t + G, len)
                                // on dr = d_q + g.  t in [tlo, thi]; the left count runs from w0, the right one to w1 = whi + G
                                const int dl = side ? dn : dn - g, dr = side ? dn + g : dn;
                                const int whi = w1 - G, tlo = side ? w0 : 1, thi = side ? whi - 1 : whi;
                                if (thi < tlo || (side ? (long long)dr + (long long)len > clen : dl < 0)) continue;
                                const bool one_chunk = whi - w0 < 64;
                                u32 b_total = 0;
                                if (!one_chunk)
                                    for (int t0 = w0; t0 < whi; t0 += 64) {
                                        const int t = t0 + (int)lane;
                                        b_total += (u32)__popcll(__ballot(t < whi && differ((long long)t + G, dr)));
                                    }
                                u32 a_run = 0, b_run = 0, best = 0xFFFFFFFFu;
                                for (int t0 = w0; t0 <= whi; t0 += 64) {
                                    const int t = t0 + (int)lane;
                                    const u64 ma = __ballot(t <= whi && differ((long long)t, dl));
                                    const u64 mb = __ballot(t < whi && differ((long long)t + G, dr));
                                    if (one_chunk) b_total = (u32)__popcll(mb);
                                    const u32 cost_t = (u32)ag + a_run + (u32)__popcll(ma & below_lane) + b_total - b_run - (u32)__popcll(mb & below_lane);
                                    const u32 m = wave_min_u32(t >= tlo && t <= thi ? (cost_t << 16) | (u32)t : 0xFFFFFFFFu);
                                    best = m < best ? m : best;
                                    a_run += (u32)__popcll(ma);
                                    b_run += (u32)__popcll(mb);
                                }
                                if ((best >> 16) < best_cost) { best_cost = best >> 16; best_g = g; best_t = (int)(best & 0xFFFFu); }
                            }
                        if (best_g == 0) continue;
                        saved += m0 - best_cost;
                        const int ag = best_g < 0 ? -best_g : best_g;
                        gaps += (u32)ag; ins += best_g < 0 ? (u32)ag : 0u; del += best_g > 0 ? (u32)ag : 0u;
                        if (side) { gb = best_g; tb = best_t; } else { gf = best_g; tf = best_t; }
                    }
                }
                // the chain's pieces in turn: piece i is read bases [lo, hi) on head i's diagonal di, and en its end before the clamps (the
                // breakpoint behind head i; of the last piece, its hi).  piece(i, di, lo, hi, en) = false ends the walk, which then gives false
                auto for_pieces = [&](auto&& piece) -> bool {
                    long long s = d1 < 0 ? -(long long)d1 : 0;
                    if constexpr (ENDS)
                        if (gf) {                                              // the piece in front of the front gap: [0, t_f) on d_1 - g_f
                            const int d0 = d1 - gf;
                            long long hi = clen - (long long)d0;
                            if (hi > (long long)tf) hi = (long long)tf;
                            if (!piece(e, d0, d0 < 0 ? -(long long)d0 : 0ll, hi, (long long)tf)) return false;
                            s = (long long)tf + (gf < 0 ? -(long long)gf : 0);
                        }
                    for (u32 i = h0; i <= e; ++i) {
                        const int di = lane_value(my_d, i);
                        long long hi = clen - (long long)di;
                        if (hi > (long long)len) hi = (long long)len;
                        long long en = i == e ? hi : (long long)lane_value(my_t, i);
                        if constexpr (ENDS)
                            if (i == e && gb) en = (long long)tb;
                        if (en < hi) hi = en;
                        const long long lo = s < -(long long)di ? -(long long)di : s;
                        if (!piece(i, di, lo, hi, en)) return false;
                        if (i < e) {                                           // behind an insertion the read goes on -g bases later
                            const int g = lane_value(my_d, i + 1) - di;
                            s = en + (g < 0 ? -(long long)g : 0);
                        }
                    }
                    if constexpr (ENDS)
                        if (gb) {                                              // the piece behind the back gap: [t_b + G, len) on d_q + g_b
                            const int dl = d + gb;
                            long long hi = clen - (long long)dl;
                            if (hi > (long long)len) hi = (long long)len;
                            const long long sb = (long long)tb + (gb < 0 ? -(long long)gb : 0);
                            if (!piece(e, dl, sb < -(long long)dl ? -(long long)dl : sb, hi, hi)) return false;
                        }
                    return true;
                };
                // ---- verify the pieces
                u32 cost = gaps, ov = 0;
                if constexpr (TRACE) cand_pc.n = 0;
                if (!for_pieces([&](u32, int di, long long lo, long long hi, long long) {
                        if (hi <= lo) return false;                            // (no finished build gives this: include/gasm.h, step 6)
                        if constexpr (TRACE) {
                            if (lane == cand_pc.n) { cand_pc.se = (int)((u32)lo | (u32)hi << 16); cand_pc.d = di; }
                            ++cand_pc.n;
                        }
                        for (long long i0 = lo; i0 < hi && cost <= max_edits; i0 += 64) {
                            const long long x = i0 + lane;
                            cost += (u32)__popcll(__ballot(x < hi && differ(x, di)));
                        }
                        ov += (u32)(hi - lo);
                        return cost <= max_edits;
                    }))
                    continue;
                // ---- accepted: pileup, gap pileup, histogram, best chain
                for_pieces([&](u32 i, int di, long long lo, long long hi, long long en) {
                    for (long long i0 = lo; i0 < hi; i0 += 64) {
                        const long long x = i0 + lane;
                        if (x < hi) atomicAdd(&out.pile[4 * (cb + (u64)((long long)di + x)) + base_at(rs.words, p0 + (u64)x)], 1u);
                    }
                    if (GAPPED && i < e) {
                        const int g = lane_value(my_d, i + 1) - di;
                        const long long p = (long long)di + en;                // the contig base at the breakpoint
                        if (g > 0) {                                           // a deletion: contig bases p .. p + g - 1 are skipped
                            const long long pp = p + lane;
                            if ((int)lane < g && pp >= 0 && pp < clen) atomicAdd(&out.gap_pile[2 * (cb + (u64)pp)], 1u);
                        } else if (lane == 0 && p >= 0 && p < clen)            // an insertion in front of contig base p
                            atomicAdd(&out.gap_pile[2 * (cb + (u64)p) + 1], 1u);
                        if constexpr (TRACE)
                            if (g < 0) trace_insertion(out.ins_pile, rs.words, p0, len, cb, clen, max_gap > end_gap ? max_gap : end_gap, lane, p, en, -g);
                    }
                    return true;
                });
                if constexpr (ENDS) {                                          // the end gaps' adds to the gap pileup, as a join's
                    for (int side = 0; side < 2; ++side) {
                        const int g = side ? gb : gf;
                        if (!g) continue;
                        const long long p = side ? (long long)d + tb : (long long)(d1 - gf) + tf;      // left diagonal + breakpoint
                        if (g > 0) {
                            const long long pp = p + lane;
                            if ((int)lane < g && pp >= 0 && pp < clen) atomicAdd(&out.gap_pile[2 * (cb + (u64)pp)], 1u);
                        } else if (lane == 0 && p >= 0 && p < clen)
                            atomicAdd(&out.gap_pile[2 * (cb + (u64)p) + 1], 1u);
                        if constexpr (TRACE)
                            if (g < 0) trace_insertion(out.ins_pile, rs.words, p0, len, cb, clen, max_gap > end_gap ? max_gap : end_gap, lane, p, side ? tb : tf, -g);
                    }
                    c_end[0] += gf ? 1u : 0u; c_end[1] += gb ? 1u : 0u; c_end[2] += cost + saved > max_edits ? 1u : 0u;
                }
                if (lane == 0) atomicAdd(&out.hist[(size_t)rp.seg * (max_edits + 1) + cost], 1u);
                if (n_acc == 0 || ov > b_ov || (ov == b_ov && cost < b_cost)) {
                    b_ov = ov; b_cost = cost; b_c = c; b_d = d1; b_q = e - h0 + 1; b_ins = ins; b_del = del; b_dq = d;
                    if constexpr (ENDS) {
                        b_d = d1 - gf; b_q += (gf ? 1u : 0u) + (gb ? 1u : 0u); b_dq = d + gb;
                        b_gf = gf; b_tf = tf; b_gb = gb; b_tb = tb;
                    }
                    if constexpr (TRACE) {                                     // (zero behind the last piece: an earlier best may have had more)
                        best_pc.se = lane < cand_pc.n ? cand_pc.se : 0; best_pc.d = lane < cand_pc.n ? cand_pc.d : 0;
                    }
                }
                ++n_acc;
            }
            cls = !seeded_any ? 2u : n_acc == 0 ? 3u : n_acc == 1 ? 4u : 5u;
        }
        if constexpr (TRACE)
            if (lane < GASM_MAP_PIECES) {
                int2 v;
                v.x = n_acc ? best_pc.se : 0; v.y = n_acc ? best_pc.d : 0;
                *reinterpret_cast<int2*>(out.rec_piece + (r * GASM_MAP_PIECES + lane) * 2) = v;
            }
        if (lane == 0) {
            int4 v;
            v.x = n_acc ? (int)(b_c - rp.c_lo) : -1; v.y = n_acc ? b_d : 0;
            v.z = n_acc ? (int)(b_cost | (n_acc << 16)) : 0; v.w = (int)b_ov;
            *reinterpret_cast<int4*>(out.rec + r * 4) = v;
            if constexpr (GAPPED) {
                int4 w;
                w.x = (int)b_q; w.y = (int)b_ins; w.z = (int)b_del; w.w = n_acc ? b_dq : 0;
                *reinterpret_cast<int4*>(out.rec_gap + r * 4) = w;
            }
            if constexpr (ENDS) {
                int4 w;
                w.x = n_acc ? b_gf : 0; w.y = n_acc ? b_tf : 0; w.z = n_acc ? b_gb : 0; w.w = n_acc ? b_tb : 0;
                *reinterpret_cast<int4*>(out.rec_end + r * 4) = w;
            }
        }
#pragma unroll
        for (u32 q = 0; q < 6; ++q) c_cnt[q] += cls == q ? 1u : 0u;
        c_cnt[6] += dropped;
        if constexpr (GAPPED) c_cnt[7] += n_acc && b_q >= 2 ? 1u : 0u;
        if constexpr (ENDS) c_end[3] += n_acc && b_gf ? 1u : 0u;
    });
    if constexpr (ENDS)                                                       // (rare: one global atomic per non-zero counter and wave)
        if (lane == 0)
            for (u32 q = 0; q < GASM_MAPEND_COUNTERS; ++q)
                if (c_end[q]) atomicAdd(&out.end_counters[(size_t)rp.seg * GASM_MAPEND_COUNTERS + q], (unsigned long long)c_end[q]);
    flush_wave_counters(c_cnt, s_cnt, out.counters + (size_t)rp.seg * N_CNT);
}
template __global__ void k_read_map<u64, false, false, false>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32, u32, MapOut);
template __global__ void k_read_map<K128, false, false, false>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32, u32, MapOut);
template __global__ void k_read_map<u64, true, false, false>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32, u32, MapOut);
template __global__ void k_read_map<K128, true, false, false>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32, u32, MapOut);
template __global__ void k_read_map<u64, true, true, false>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32, u32, MapOut);
template __global__ void k_read_map<K128, true, true, false>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32, u32, MapOut);
template __global__ void k_read_map<u64, true, true, true>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32, u32, MapOutTrace);
template __global__ void k_read_map<K128, true, true, true>(ReadSet, GraphView, ContigIndex, u32, u32, u32, u32, u32, MapOutTrace);
