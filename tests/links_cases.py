"""The hand-built k = 5 cases of the contig links and the read pairs (TEST INFRASTRUCTURE: plain data, imported by the host tests, which
hold the restatements against them, and by the GPU tests, which hold the device against them).  Every table and record here was written
out by hand, entry by entry: none is derived from any code.  Nodes are 4-mers.  The pieces: X = GCAATAGGG, R = TAATTCGC, Y = CGACGAGTA,
Z = AGCGTAGAT; the genome X R Y R Z is cut into Xc = g[0:13], R = g[9:17] = g[26:34], Zc = g[30:43], Yc = g[13:30] (contigs 0, 1, 2, 3)."""
import links_ref as lr
import pairs_ref as pr

K = 5
N = lr.NONE
X, R, Y, Z, W = "GCAATAGGG", "TAATTCGC", "CGACGAGTA", "AGCGTAGAT", "GGCTTACAC"


# ---- the hand-built cases: contigs in index order, and the non-empty entries of the tables
def _tab(n, succ=(), pred=(), link=(), span=()):
    """tables of n contigs from their non-empty entries: succ {(a, 'x'): b}, pred {(b, 'x'): a}, link {(a, 'x'): count}, span {(r, 'xy'): count}"""
    t = dict(succ=[[N] * 4 for _ in range(n)], pred=[[N] * 4 for _ in range(n)], link_support=[[0] * 4 for _ in range(n)],
             span_support=[[[0] * 4 for _ in range(4)] for _ in range(n)], skipped=0)
    for (a, x), b in dict(succ).items():
        t["succ"][a]["ACGT".index(x)] = b
    for (b, x), a in dict(pred).items():
        t["pred"][b]["ACGT".index(x)] = a
    for (a, x), c in dict(link).items():
        t["link_support"][a]["ACGT".index(x)] = c
    for (r, xy), c in dict(span).items():
        t["span_support"][r]["ACGT".index(xy[0])]["ACGT".index(xy[1])] = c
    return t


# X R Y R Z: X + TAAT, R, TCGC + Z, TCGC + Y + TAAT (sorted).  X ends with G and Y with A (the in-edges GTAAT, ATAAT); Y starts with C
# and Z with A (the out-edges TCGCC, TCGCA).  Z's contig is a dead end, X's has nothing in front.
G = X + R + Y + R + Z
XRYRZ = [X + "TAAT", R, "TCGC" + Z, "TCGC" + Y + "TAAT"]
XRYRZ_SUCC = {(0, "T"): 1, (1, "A"): 2, (1, "C"): 3, (3, "T"): 1}
XRYRZ_PRED = {(1, "G"): 0, (1, "A"): 3, (2, "T"): 1, (3, "T"): 1}
# three copies: X R Y R Z R W (W starts with G; Z ends with T)
G3 = X + R + Y + R + Z + R + W
THREE = [X + "TAAT", R, "TCGC" + Z + "TAAT", "TCGC" + Y + "TAAT", "TCGC" + W]
# n(r) == 1: the repeat is one k-mer, TAATC (nodes TAAT and AATC)
G1 = X + "TAATC" + Y + "TAATC" + Z
ONE = ["AATC" + Z, "AATC" + Y + "TAAT", X + "TAAT", "TAATC"]
# a loop: node TAAT, once round is TAAT CC TAAT; X comes in over GTAAT, GTCGTAGAC leaves over TAATG
LOOP = [X + "TAAT", "TAATCCTAAT", "TAATGTCGTAGAC"]
LOOP_ONCE = X + "TAATCCTAAT" + "GTCGTAGAC"
LOOP_THRICE = X + "TAATCC" * 3 + "TAAT" + "GTCGTAGAC"
# an unbranched cycle of five k-mers cut at node ACGT (no build makes this contig: an isolated cycle has no branching node to cut it at)
CYCLE = ["ACGTTACGT"]
# chained repeats: A R B R2 C, D R E, F R2 H
R2, D, E, F, H, CC = "CTGATCTT", "ATATCCCGC", "GGTCGGGCT", "GAACTCACC", "CCGTGCGCA", "TATGTCTGG"
CHAIN_READS = [X + R + Y + R2 + CC, D + R + E, F + R2 + H]
# a closing chain: the circle A R B R, read twice round
CIRCLE = [R, "TCGC" + Z + "TAAT", "TCGC" + Y + "TAAT"]
CIRCLE_READ = R + Z + R + Y + R + Z + R + Y + R

CASES = {
    "XRYRZ": (XRYRZ, [G], 8, _tab(4, XRYRZ_SUCC, XRYRZ_PRED, {(0, "T"): 1, (1, "A"): 1, (1, "C"): 1, (3, "T"): 1}, {(1, "GC"): 1, (1, "AA"): 1})),
    # len(R) == span_len above, span_len + 1 here: no span is counted
    "XRYRZ, span_len 7": (XRYRZ, [G], 7, _tab(4, XRYRZ_SUCC, XRYRZ_PRED, {(0, "T"): 1, (1, "A"): 1, (1, "C"): 1, (3, "T"): 1})),
    "XRYRZ, span_len 0": (XRYRZ, [G, G], 0, _tab(4, XRYRZ_SUCC, XRYRZ_PRED, {(0, "T"): 2, (1, "A"): 2, (1, "C"): 2, (3, "T"): 2})),
    # a chimeric read GGG R AGC beside the genome twice: X -> R -> Z, the mixed matrix
    "mixed": (XRYRZ, [G, G, "GGG" + R + "AGC", "GGG" + R + "AGC"], 8,
              _tab(4, XRYRZ_SUCC, XRYRZ_PRED, {(0, "T"): 4, (1, "A"): 4, (1, "C"): 2, (3, "T"): 2}, {(1, "GC"): 2, (1, "AA"): 2, (1, "GA"): 2})),
    "three copies": (THREE, [G3, G3], 8,
                     _tab(5, {(0, "T"): 1, (1, "A"): 2, (1, "C"): 3, (1, "G"): 4, (2, "T"): 1, (3, "T"): 1},
                          {(1, "G"): 0, (1, "T"): 2, (1, "A"): 3, (2, "T"): 1, (3, "T"): 1, (4, "T"): 1},
                          {(0, "T"): 2, (1, "A"): 2, (1, "C"): 2, (1, "G"): 2, (2, "T"): 2, (3, "T"): 2}, {(1, "GC"): 2, (1, "AA"): 2, (1, "TG"): 2})),
    "n(r) == 1": (ONE, [G1, G1], 5,
                  _tab(4, {(1, "C"): 3, (2, "C"): 3, (3, "A"): 0, (3, "C"): 1}, {(0, "T"): 3, (1, "T"): 3, (3, "A"): 1, (3, "G"): 2},
                       {(1, "C"): 2, (2, "C"): 2, (3, "A"): 2, (3, "C"): 2}, {(3, "GC"): 2, (3, "AA"): 2})),
    # the read that goes round three times crosses the link (loop, loop) twice; every entry into the loop followed by a whole round is a span
    "loop": (LOOP, [LOOP_ONCE, LOOP_THRICE], 10,
             _tab(3, {(0, "C"): 1, (0, "G"): 2, (1, "C"): 1, (1, "G"): 2}, {(1, "G"): 0, (1, "C"): 1, (2, "G"): 0, (2, "C"): 1},
                  {(0, "C"): 2, (1, "C"): 2, (1, "G"): 2}, {(1, "GG"): 1, (1, "GC"): 1, (1, "CC"): 1, (1, "CG"): 1})),
    # 15 k-mers, offsets 0 1 2 3 4 three times: crossings behind positions 4 and 9; only the first is followed by a whole round and one more k-mer
    "unbranched cycle": (CYCLE, ["ACGTT" * 3 + "ACGT"], 9, _tab(1, {(0, "T"): 0}, {(0, "T"): 0}, {(0, "T"): 2}, {(0, "TT"): 1})),
    # nothing attached, and a read that runs off the contig: its last two k-mers are not in the set
    "dead end": ([X], [X + "TT", "GCAA"], 9, _tab(1)),
}


# ---- read pairs on the contigs of X R Y R Z
CONTIGS = XRYRZ

# ---- the hand-built pairs: (mate 1, mate 2, the record of orientation 0, its counter field)
HAND = [
    (G[0:7], pr.rc(G[23:30]), [0, 0, 3, 17], "diff_contig"),                 # the fragment g[0:30): starts Xc, ends with Yc's last base
    (G[14:21], pr.rc(G[22:29]), [3, 1, 3, 16], "same_contig"),               # g[14:29) inside Yc = g[13:30): d = 15
    (G[22:29], pr.rc(G[14:21]), [3, 9, 3, 8], "reversed"),                   # the same two reads as an outie: d = -1
    ("GCA", pr.rc(G[22:29]), [-1, 0, 3, 16], "one_placed"),                  # mate 1 shorter than k
    ("ACACACA", "CCCCCCC", [-1, 0, -1, 0], "none_placed"),
    (G[0:15], pr.rc(G[23:30]), [-1, 0, -1, 0], "skipped"),                   # 11 k-mers against max_kmers = 10
    ("TT" + G[0:7], "GG" + pr.rc(G[38:43]), [0, -2, 2, 15], "diff_contig"),  # first hits at i1 = 2 and i2 = 2: S < 0, E > len(Zc) = 13
    (G[9:16], pr.rc(G[27:34]), [1, 0, 1, 8], "same_contig"),                 # both inside the repeat's contig R: d = 8 = len(R)
]
