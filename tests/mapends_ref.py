"""CPU restatement of the end-gap rule (include/gasm.h, "End gaps"), on strings and lists (TEST INFRASTRUCTURE: imported by the end-gap
tests only; it shares no code with genomeassembler_dev_amd or the library; heads, chains, breakpoints and pieces are map_ref's and
mapgap_ref's).
    end_gap_of(read, contig, k, head, end_gap, side) -> (m0, best): the brute-force definition of steps 5a (side = "back", head = the
        chain's last) and 5b ("front", the chain's first).  m0: the end's mismatches on the ungapped diagonal (None: not eligible);
        best: (cost, g, t) of the taken gap or None
    end_gap_linear(...): the same in one pass per candidate g (prefix and suffix counts), which ends_of takes for windows of more than
        LINEAR_FROM positions
    place_ends(contigs, reads, k, max_edits, max_gap, end_gap) -> the dict of mapgap_ref.place_gapped, plus end_records[r] = [g_front,
        t_front, g_back, t_back] and end_counters = [front, back, rescued, start_moved]
and the hand-built cases and the generators the host and the GPU tests share.
"""
import random

import mapgap_ref as gr
from map_ref import MAX_KMERS, MAX_MISMATCH, NO_PLACE, heads_of
from mapgap_ref import MAX_GAP, NO_GAPS, P, PQ, R5, chain_cost, chains_of
from pairs_ref import where_of

END_FIELDS = ("front", "back", "rescued", "start_moved")
NO_ENDS = [0, 0, 0, 0]
LINEAR_FROM = 256


def mism(read, contig, lo, hi, d):
    return sum(1 for x in range(lo, hi) if read[x] != contig[d + x])


def _window(read, contig, k, head, side):
    """(w0, w1, eligible) of an end: the window [w0, w1) between the read's end and the outermost seed"""
    J, _, d = head
    if side == "back":
        return J + k, len(read), d + len(read) <= len(contig)
    return 0, J, d >= 0 and J > 0


def _candidates(read, contig, w0, w1, d, end_gap, side):
    """every admissible (g, G, t range, left diagonal, right diagonal) of an eligible end, in the key's order of (|g|, deletion first)"""
    for ag in range(1, end_gap + 1):
        for g in (ag, -ag):
            G = max(0, -g)
            if side == "back":
                if d + g + len(read) <= len(contig):
                    yield g, G, range(w0, w1 - G), d, d + g
            elif d - g >= 0:
                yield g, G, range(1, w1 - G + 1), d - g, d


def end_gap_of(read, contig, k, head, end_gap, side):
    w0, w1, eligible = _window(read, contig, k, head, side)
    if not eligible:
        return None, None
    m0 = mism(read, contig, w0, w1, head[2])
    best = None
    for g, G, ts, dl, dr in _candidates(read, contig, w0, w1, head[2], end_gap, side):
        for t in ts:
            key = (abs(g) + mism(read, contig, w0, t, dl) + mism(read, contig, t + G, w1, dr), abs(g), g < 0, t)
            if best is None or key < best:
                best = key
    if best is None or best[0] >= m0:
        return m0, None
    return m0, (best[0], -best[1] if best[2] else best[1], best[3])


def end_gap_linear(read, contig, k, head, end_gap, side):
    """end_gap_of in one pass per candidate g: the left diagonal's mismatches as prefix counts from the window's start, the right
    diagonal's as suffix counts back from its end.  end_gap_of stays the definition; tests/test_mapends_host.py holds the two equal"""
    w0, w1, eligible = _window(read, contig, k, head, side)
    if not eligible:
        return None, None
    m0 = mism(read, contig, w0, w1, head[2])
    best = None
    for g, G, ts, dl, dr in _candidates(read, contig, w0, w1, head[2], end_gap, side):
        if not len(ts):
            continue
        left = [0] * (w1 - w0 + 1)                                   # left[t - w0]: mismatches on dl in [w0, t)
        for t in range(w0 + 1, w1 + 1):
            left[t - w0] = left[t - w0 - 1] + (read[t - 1] != contig[dl + t - 1] if 0 <= dl + t - 1 < len(contig) else 0)
        right = [0] * (w1 - w0 + 2)                                  # right[x - w0]: mismatches on dr in [x, w1)
        for x in range(w1 - 1, w0 - 1, -1):
            right[x - w0] = right[x - w0 + 1] + (read[x] != contig[dr + x] if 0 <= dr + x < len(contig) else 0)
        for t in ts:
            key = (abs(g) + left[t - w0] + right[t + G - w0], abs(g), g < 0, t)
            if best is None or key < best:
                best = key
    if best is None or best[0] >= m0:
        return m0, None
    return m0, (best[0], -best[1] if best[2] else best[1], best[3])


def ends_of(read, contig, k, chain, end_gap):
    """((m0, best) of the front, (m0, best) of the back) of a chain"""
    out = []
    for head, side in ((chain[0], "front"), (chain[-1], "back")):
        w0, w1, _ = _window(read, contig, k, head, side)
        out.append((end_gap_linear if w1 - w0 > LINEAR_FROM else end_gap_of)(read, contig, k, head, end_gap, side))
    return tuple(out)


def pieces_with_ends(read, contig, chain, front, back, cuts=None):
    """step 6': [(s, e, d)] of the chain with the taken end gaps front = (cost, g, t) or None, back likewise"""
    ps = gr.pieces_of(read, contig, chain, cuts)
    if front:
        _, g, t = front
        s, e, d = ps[0]
        assert s == 0 and 0 < t and t + max(0, -g) <= chain[0][0] < e
        ps[0:1] = [(0, t, d - g), (t + max(0, -g), e, d)]
    if back:
        _, g, t = back
        s, e, d = ps[-1]
        assert e == len(read) and s <= chain[-1][0] < t and t + max(0, -g) < e
        ps[-1:] = [(s, t, d), (t + max(0, -g), e, d + g)]
    for s, e, d in ps:
        assert s < e and 0 <= d + s and d + e <= len(contig), "every piece is non-empty and inside the contig"
    return ps


def cost_of(read, contig, ps):
    """step 7 over pieces: (cost, overlap): the mismatches plus the gap between every two neighbouring pieces"""
    return (sum(mism(read, contig, s, e, d) for s, e, d in ps) + sum(abs(b[2] - a[2]) for a, b in zip(ps, ps[1:])), sum(e - s for s, e, _ in ps))


def place_ends(contigs, reads, k, max_edits, max_gap, end_gap, max_kmers=MAX_KMERS):
    assert 0 <= max_edits <= MAX_MISMATCH and 0 <= max_gap <= MAX_GAP and 0 <= end_gap <= MAX_GAP
    where = where_of(contigs, k)
    pile = [[[0] * 4 for _ in s] for s in contigs]
    gap_pile = [[[0] * 2 for _ in s] for s in contigs]
    hist, counters, records, gaps, ends = [0] * (max_edits + 1), dict.fromkeys(gr.FIELDS, 0), [], [], []
    endc = dict.fromkeys(END_FIELDS, 0)
    for read in reads:
        n = len(read) - k + 1
        records.append(list(NO_PLACE))
        gaps.append(list(NO_GAPS))
        ends.append(list(NO_ENDS))
        if n <= 0 or n > max_kmers:
            counters["short" if n <= 0 else "skipped"] += 1
            continue
        heads, dropped = heads_of(where, read, k)
        counters["blocks_dropped"] += dropped
        if not heads:
            counters["unseeded"] += 1
            continue
        accepted = []
        for chain in chains_of(heads, max_gap):
            c = chain[0][1]
            (m0f, front), (m0b, back) = ends_of(read, contigs[c], k, chain, end_gap)
            ps = pieces_with_ends(read, contigs[c], chain, front, back)
            cost, ov = cost_of(read, contigs[c], ps)
            saved = (m0f - front[0] if front else 0) + (m0b - back[0] if back else 0)
            assert cost + saved == chain_cost(read, contigs[c], chain)[0], "the chain's cost without end gaps less what they save"
            if cost > max_edits:
                continue
            for (s, e, d), nxt in zip(ps, ps[1:] + [None]):
                for x in range(s, e):
                    pile[c][d + x]["ACGT".index(read[x])] += 1
                if nxt is not None and nxt[2] > d:                  # a deletion: the contig bases between the pieces
                    assert nxt[0] == e
                    for p in range(d + e, nxt[2] + e):
                        gap_pile[c][p][0] += 1
                elif nxt is not None:                               # an insertion in front of the next piece's first base
                    assert nxt[2] + nxt[0] == d + e
                    gap_pile[c][d + e][1] += 1
            hist[cost] += 1
            endc["front"] += front is not None
            endc["back"] += back is not None
            endc["rescued"] += cost + saved > max_edits
            steps = [b[2] - a[2] for a, b in zip(ps, ps[1:])]
            rec_end = [front[1] if front else 0, front[2] if front else 0, back[1] if back else 0, back[2] if back else 0]
            accepted.append((-ov, cost, chain[0][0], c, ps[0][2], len(ps), sum(-g for g in steps if g < 0), sum(g for g in steps if g > 0), ps[-1][2], rec_end))
        if not accepted:
            counters["rejected"] += 1
            continue
        counters["mapped_one" if len(accepted) == 1 else "mapped_multi"] += 1
        ov, cost, _, c, d0, q, ins, dele, dq, rec_end = min(accepted, key=lambda a: a[:3])
        records[-1] = [c, d0, cost, len(accepted), -ov]
        gaps[-1] = [q, ins, dele, dq]
        ends[-1] = rec_end
        counters["gapped"] += q >= 2
        endc["start_moved"] += rec_end[0] != 0
    assert sum(counters[f] for f in gr.FIELDS[:6]) == len(reads)
    return dict(records=records, gap_records=gaps, pile=pile, gap_pile=gap_pile, edit_hist=hist, counters=[counters[f] for f in gr.FIELDS],
                end_records=ends, end_counters=[endc[f] for f in END_FIELDS])


SIX = ("records", "gap_records", "pile", "gap_pile", "edit_hist", "counters")


def six(t):
    return [t[name] for name in SIX]


def placed(t):
    return gr.placed(t)


# ---- hand-built cases on mapgap_ref.P (k = 5) and R5 (k = 6), written out by hand as mapgap_ref.HAND is, with the end record and counters:
# (k, contigs, read, max_edits, max_gap, end_gap, [c, d_first, cost, chains, overlap], [pieces, inserted, deleted, d_last],
#  [g_front, t_front, g_back, t_back], counter field, the pieces laid on the pileup [(c, first contig base, read bases)], the gap adds,
#  [front, back, rescued, start_moved])
# No base of P equals its neighbour, so a read shifted by one base against a diagonal differs from it in every base.  The cases lie on
#   P[24:48] = GCGT CACGTACAGT GACATCGTGT  (P[28] = C, P[38] = G)
# and every read's heads are listed in HAND_HEADS (the test holds heads_of to them): no k-mer across a junction is one of P's.
_FDEL = P[26:29] + P[30:46]          # GTC + P[30:46]: P without its base 29, three bases behind the read's start
_FINS = P[26:29] + "T" + P[29:46]    # a T between P[28] = C and P[29] = A
_BDEL = P[28:43] + P[44:48]          # P without its base 43, four bases in front of the read's (and the contig's) end
_BINS = P[28:43] + "A" + P[43:47]    # an A between P[42] = T and P[43] = C
_BOTH = P[26:29] + P[30:43] + P[44:48]
_TB = P[30:35] + P[36:48]            # P without its base 35, directly behind the first k-mer
_EQ = P[28:41] + P[43:45]            # P without its bases 41, 42, two bases in front of the read's end
_OFF = P[30:43] + P[44:48] + "AC"    # the back deletion again, and two bases beyond the contig's end
_TIE = P[28:40] + "ATA"
_R5 = R5[2:18] + R5[19:24]           # R5 without its base 18 (k = 6)
HAND = [
    # front deletion.  One head (3, P, 27).  Front window [0, 3): m0 = GTC against P[27:30] = TCA = 3.  g = 1: d_0 = 26, t = 3 costs
    # 1 + 0 + 0 (t = 1, 2: the bases behind t lie on diagonal 27, shifted: 1 + 2, 1 + 1); g = -1: d_0 = 28, G against C: 2 at least.
    # Pieces [0, 3) on 26 and [3, 19) on 27; P[29] skipped.  Without the gap 3 edits > 2: rescued
    (5, PQ, _FDEL, 2, 1, 1, [0, 26, 1, 1, 19], [2, 0, 1, 27], [1, 3, 0, 0], "mapped_one", [(0, 26, P[26:29]), (0, 30, P[30:46])], [(0, 29, "D")], [1, 0, 1, 1]),
    # the same read with end_gap = 0: three mismatches
    (5, PQ, _FDEL, 2, 1, 0, list(NO_PLACE), list(NO_GAPS), list(NO_ENDS), "rejected", [], [], [0, 0, 0, 0]),
    # front insertion.  One head (4, P, 25).  m0 = GTCT against P[25:29] = CGTC = 4.  g = 1: d_0 = 24, t = 1: G = P[24] but TCT against
    # GTC behind it: 1 + 0 + 3.  g = -1: G = 1, d_0 = 26, t in [1, 3], t = 3: 1 + 0 + 0.  Pieces [0, 3) on 26, [4, 21) on 25; read base 3
    # lies on nothing, the insertion stands in front of contig base 26 + 3
    (5, PQ, _FINS, 1, 1, 1, [0, 26, 1, 1, 20], [2, 1, 0, 25], [-1, 3, 0, 0], "mapped_one", [(0, 26, P[26:29]), (0, 29, P[29:46])], [(0, 29, "I")], [1, 0, 1, 1]),
    # back deletion at the contig's end.  One head (0, P, 28), B = 5; 28 + 19 = 47 <= 48 eligible, and g = 1 fits exactly: 29 + 19 = 48.
    # m0 = GTGT against P[43:47] = CGTG = 4.  g = 1, t = 15: 1 + 0 + 0 (t = 14: read base 14 = T against P[43] = C on diagonal 29: 2)
    (5, PQ, _BDEL, 1, 1, 1, [0, 28, 1, 1, 19], [2, 0, 1, 29], [0, 0, 1, 15], "mapped_one", [(0, 28, P[28:43]), (0, 44, P[44:48])], [(0, 43, "D")], [0, 1, 1, 0]),
    # back insertion.  One head (0, P, 28); 28 + 20 = 48 eligible; g = 1 is not admissible (29 + 20 > 48).  m0 = ACGTG against
    # P[43:48] = CGTGT = 5.  g = -1, G = 1: t in [5, 18], t = 15: 1 + 0 + 0.  Pieces [0, 15) on 28, [16, 20) on 27
    (5, PQ, _BINS, 1, 1, 1, [0, 28, 1, 1, 19], [2, 1, 0, 27], [0, 0, -1, 15], "mapped_one", [(0, 28, P[28:43]), (0, 43, P[43:47])], [(0, 43, "I")], [0, 1, 1, 0]),
    # both ends of one read.  One head (3, P, 27).  Front as _FDEL.  Back: B = 8, 27 + 20 = 47 eligible, m0 = GTGT against CGTG = 4,
    # g = 1 (28 + 20 = 48), t = 16.  Three pieces; without the gaps 3 + 4 edits
    (5, PQ, _BOTH, 2, 1, 1, [0, 26, 2, 1, 20], [3, 0, 2, 28], [1, 3, 1, 16], "mapped_one",
     [(0, 26, P[26:29]), (0, 30, P[30:43]), (0, 44, P[44:48])], [(0, 29, "D"), (0, 43, "D")], [1, 1, 1, 1]),
    # a gap directly behind the seed k-mer, t = B.  Heads (0, P, 30) and (5, P, 31); max_gap = 0 joins nothing: two chains.  Chain 1:
    # B = 5, m0 = the twelve bases behind it, all shifted = 12; g = 1 (31 + 17 = 48), t = 5 = B: 1.  Chain 2: front window [0, 5), m0 = 5,
    # g = 1, d_0 = 30, t = 5: 1 (t = 4: read base 4 shifted: 2).  Both chains are the same alignment, laid on the pileups twice; the
    # best is the one that starts first, chain 1, which has no front gap.  The end gaps do here what a join does at max_gap = 1
    (5, PQ, _TB, 1, 0, 1, [0, 30, 1, 2, 17], [2, 0, 1, 31], [0, 0, 1, 5], "mapped_multi",
     [(0, 30, P[30:35]), (0, 36, P[36:48])] * 2, [(0, 35, "D")] * 2, [1, 1, 2, 0]),
    # cost == m0: not taken.  One head (0, P, 28), B = 5.  m0 = CG against P[41:43] = AT = 2.  g = 1 costs 1 + CG against P[42:44] = TC;
    # g = -1: t = 13: 1 + G against P[41] = A, t = 12: 1 + CG against P[40:42] = CA: 2 each, not below m0; g = 2 would cost 2 + 0 = m0:
    # no |g| >= m0 is tried.  One piece, two mismatches
    (5, PQ, _EQ, 2, 1, 2, [0, 28, 2, 1, 15], [1, 0, 0, 28], list(NO_ENDS), "mapped_one", [(0, 28, _EQ)], [], [0, 0, 0, 0]),
    # an end that runs off the contig: 30 + 19 = 49 > 48, not eligible.  The piece is clipped at the contig's end: [0, 18) on 30 with
    # GTGT against CGTG and A against T: 5 mismatches where a gap would cost 1 (the stated limit)
    (5, PQ, _OFF, 5, 1, 1, [0, 30, 5, 1, 18], [1, 0, 0, 30], list(NO_ENDS), "mapped_one", [(0, 30, _OFF[:18])], [], [0, 0, 0, 0]),
    # a tie between a deletion and an insertion.  One head (0, P, 28), B = 5, the tail ATA at read 12 .. 14.  m0 = ATA against P[40:43] =
    # CAT = 3.  g = 1: t = 12: ATA against P[41:44] = ATC: 1 + 1 (t = 13, 14: 3, 4).  g = -1: t = 12: TA against P[40:42] = CA: 1 + 1;
    # t = 13: A against C, then A = P[41]: 1 + 1.  Three candidates of cost 2 and |g| = 1: the deletion wins
    (5, PQ, _TIE, 2, 1, 1, [0, 28, 2, 1, 15], [2, 0, 1, 29], [0, 0, 1, 12], "mapped_one", [(0, 28, P[28:40]), (0, 41, "ATA")], [(0, 40, "D")], [0, 1, 1, 0]),
    # k = 6 on R5: one head (0, R5, 2), B = 6; 2 + 21 = 23, g = 1: 24 = len(R5).  m0 = CGCAT against R5[18:23] = ACGCA = 5; t = 16
    (6, [R5], _R5, 1, 1, 3, [0, 2, 1, 1, 21], [2, 0, 1, 3], [0, 0, 1, 16], "mapped_one", [(0, 2, R5[2:18]), (0, 19, R5[19:24])], [(0, 18, "D")], [0, 1, 1, 0]),
]
HAND_HEADS = {_FDEL: [(3, 0, 27)], _FINS: [(4, 0, 25)], _BDEL: [(0, 0, 28)], _BINS: [(0, 0, 28)], _BOTH: [(3, 0, 27)], _TB: [(0, 0, 30), (5, 0, 31)],
              _EQ: [(0, 0, 28)], _OFF: [(0, 0, 30)], _TIE: [(0, 0, 28)], _R5: [(0, 0, 2)]}


def hand_adds(case):
    return sorted((c, p0 + i, x) for c, p0, text in case[10] for i, x in enumerate(text)), sorted(case[11])


# ---- generators
def end_indel_reads(genome, k, n, read_len, seed, lo=3):
    """n planted reads [(read, start, side, g, at)]: one indel of g in +-1..3 whose breakpoint lies lo .. k - 1 bases from the front or
    from the back end of the read"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        g, side = rnd.choice((1, 2, 3, -1, -2, -3)), ("front", "back")[i % 2]
        off = rnd.randrange(lo, k)
        at = off if side == "front" else read_len - off - max(0, -g)
        start = rnd.randrange(50, len(genome) - read_len - 60)
        out.append((gr.planted_indel_read(genome, start, read_len, at, g, rnd), start, side, g, at))
    return out


def back_strides(read, k, chain):
    """how often the kernel's loops go round the back window of a chain: 64 positions a time"""
    return (len(read) - (chain[-1][0] + k) + 63) // 64


WINDOW_K = (21, 63)


def window_case(k, seed=131):
    """(g, genome, planted, clean): a 6 kb genome, planted reads {name: read} and error-free 150-base reads at 30x.
        back300 / back1200 / back_max: 300, 1200 and 4096 + k - 1 bases with an indel 5 .. k - 1 bases from the back end
        front2: a read with an indel at 20 and a substitution at 70 (k = 63: J_1 > 64, a front window of two strides)
        skipped: a read of 4097 k-mers with an indel near its back end"""
    from genomeassembler_dev_amd import synth
    g = synth.make_segment(seed, 6000, planted=False)
    genome = g.tobytes().decode()
    rnd = random.Random(seed)
    planted = {}
    for name, n, start, gap in (("back300", 300, 200, 2), ("back1200", 1200, 600, -2), ("back_max", MAX_KMERS + k - 1, 900, 3)):
        off = rnd.randrange(5, k)
        planted[name] = gr.planted_indel_read(genome, start, n, n - off - max(0, -gap), gap, rnd)
    r = gr.planted_indel_read(genome, 2500, 400, 20, 1, rnd)
    planted["front2"] = r[:70] + "ACGT"[("ACGT".index(r[70]) + 1) % 4] + r[71:]
    planted["skipped"] = gr.planted_indel_read(genome, 700, MAX_KMERS + k, MAX_KMERS + k - 10, 1, rnd)
    return g, genome, planted, gr.clean_reads(g, 150, 30, 9)


ENDS_K, ENDS_SEED, ENDS_MIN_COUNT = 21, 28, 2


def contig_ends_case(seed=ENDS_SEED):
    """(g, reads, n_planted), following mapgap_ref.contig_ends_case: a 3 kb genome with a 150-base repeat, 60 planted 80-base reads whose
    indel lies within k of a read end and whose start lies within 100 bases of a repeat boundary, then error-free 80-base reads at 20x"""
    from genomeassembler_dev_amd import synth
    g, p1, p2 = synth.plant_repeat(synth.make_segment(seed, 3000, planted=False), 150, seed)
    genome = g.tobytes().decode()
    rnd = random.Random(seed)
    planted = []
    for i in range(60):
        end = rnd.choice((p1, p1 + 150, p2, p2 + 150))
        start = max(0, min(len(genome) - 100, end + rnd.randrange(-100, 21)))
        gap = rnd.choice((1, 2, 3, -1, -2, -3))
        off = rnd.randrange(3, ENDS_K)
        planted.append(gr.planted_indel_read(genome, start, 80, off if i % 2 else 80 - off - max(0, -gap), gap, rnd))
    return g, planted + gr.clean_reads(g, 80, 20, seed), len(planted)


def contig_end_properties(contigs, reads, k, max_gap, end_gap):
    """what the contig-ends case asks of a draw, on the build's contigs: (ends that are not eligible although they have a window, ends
    whose ungapped diagonal is eligible and a candidate g within end_gap is not, taken gaps)"""
    where = where_of(contigs, k)
    ineligible = partly = taken = 0
    for read in reads:
        if not k <= len(read) <= MAX_KMERS + k - 1:
            continue
        for chain in chains_of(heads_of(where, read, k)[0], max_gap):
            contig = contigs[chain[0][1]]
            for head, side in ((chain[0], "front"), (chain[-1], "back")):
                w0, w1, eligible = _window(read, contig, k, head, side)
                if w1 <= w0:
                    continue
                ineligible += not eligible
                if eligible:
                    partly += len(list(_candidates(read, contig, w0, w1, head[2], end_gap, side))) < 2 * end_gap
                    taken += end_gap_of(read, contig, k, head, end_gap, side)[1] is not None
    return ineligible, partly, taken


def slot_case():
    """(segs, steps): the two segments of mapgap_ref.slot_case and four alternating builds (k, min_count, strands) with the parameters
    (max_edits, max_gap, end_gap) of the end-gapped mapping after each"""
    segs, _ = gr.slot_case()
    return segs, [((21, 2, 1), (6, 3, 3)), ((33, 2, 1), (6, 3, 3)), ((21, 2, 1), (4, 0, 2)), ((33, 2, 1), (255, 16, 16))]
