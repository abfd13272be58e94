"""Inputs, CPU expectations and the comparison helper of the last-workgroup hand-off tests (TEST INFRASTRUCTURE: imported by
tests/test_handoff_host.py, tests/test_handoff_gpu.py and tests/test_build_paths_gpu.py; nothing here touches a GPU).

Three kernels of the build finish inside their own last workgroup: k_bucket_dedup and k_bucket_solid turn the buckets' counts bucket_d
into dstart, k_contig_scan turns seg_ncontig / seg_cbases into seg_cstart / seg_bstart and the report.  Every word handed over lives
in a buffer the next build on the same step slot writes again, so a stale read shows only where the build before left something
else in that word.  The cases below are pairs of builds of the same reads whose words differ in every segment:

    grid     2051 small segments, k = 21 and 33; X = build(k), Y = build(k, min_count = 2)
    ladder   the B input of tests/test_build_paths_gpu.py, k = 33; P = build(33, 12000) (one attempt), Q = build(33, 10) (the first
             attempt overflows its tables and leaves its words behind; the results are P's)
    rounds   64 segments of noisy reads, k = 21; Z = build_simplified(k, **correct_ref.readme_options(k)) (one k_bucket_solid
             hand-off per round), X = build(k)

A snapshot is a tuple in the order of FIELDS, arrays as bytes: what test_build_paths_gpu._snapshot fetches (twelve fields), or its
first seven (no scores).  expected_snapshot() makes the first seven from the oracle's per-segment results."""
import collections
import functools

import numpy as np

import bubbles_ref as br
import correct_ref as cr
import lowcov_ref as lr
import tips_ref as tr
from genomeassembler_dev_amd import synth
from oracle import orc

# name, dtype the bytes are compared in (scores by their bit patterns: NaN == NaN, as in a comparison of the bytes)
FIELDS = (("distinct segment offsets", "<u8"), ("distinct keys", "<u8"), ("multiplicities", "<u4"), ("key words", None),
          ("contig segment offsets", "<u8"), ("contig base offsets", "<u8"), ("contig text", "u1"),
          ("bp_score", "<u8"), ("bp_score_norm_by_break_freqs", "<u8"), ("bp_score_norm_by_len", "<u8"), ("kmer_breaks", "<i4"), ("sequence_len", "<i4"))
SEG_OFF, KEYS, MULT, WORDS, CSEG_OFF, C_OFF, TEXT = range(7)
SCORE_NAMES = tuple(n for n, _ in FIELDS[7:])


# ---------------------------------------------------------------------------------------------------------------- snapshots
def snapshot(b, scores=False):
    """the fetches of a built batch in the order of FIELDS: distinct() and contigs_raw(), with scores=True also scores()"""
    seg, keys, mult, w = b.distinct()
    so, off, raw = b.contigs_raw()
    out = (seg.tobytes(), keys.tobytes(), mult.tobytes(), w, so.tobytes(), off.tobytes(), raw)
    if scores:
        sc = b.scores()
        out += tuple(sc[n].tobytes() for n in SCORE_NAMES)
    return out


def pack_keys(kmers, k):
    """list of k-mer strings -> (n, words) uint64 in the layout of distinct() (include/gasm.h: base 0 most significant, the high word
    first)"""
    words = 1 if k <= 31 else 2
    out = np.zeros((len(kmers), words), dtype=np.uint64)
    if not kmers:
        return out
    lut = np.zeros(256, dtype=np.uint64)
    lut[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint64)
    code = lut[np.frombuffer("".join(kmers).encode(), dtype=np.uint8).reshape(len(kmers), k)]
    for j in range(k):
        bit = 2 * (k - 1 - j)
        out[:, words - 1 - bit // 64] |= code[:, j] << np.uint64(bit % 64)
    return out


def expected_snapshot(refs, k):
    """the first seven FIELDS of a whole batch from the oracle's results per segment (refs[s]: contigs, distinct, counts)"""
    seg = np.zeros(len(refs) + 1, dtype=np.uint64)
    so = np.zeros(len(refs) + 1, dtype=np.uint64)
    seg[1:] = np.cumsum([len(r["distinct"]) for r in refs], dtype=np.uint64)
    so[1:] = np.cumsum([len(r["contigs"]) for r in refs], dtype=np.uint64)
    keys = pack_keys([x for r in refs for x in r["distinct"]], k)
    mult = np.concatenate([np.asarray(r["counts"], dtype=np.int64) for r in refs] + [np.zeros(0, np.int64)]).astype(np.uint32)
    contigs = [c for r in refs for c in r["contigs"]]
    off = np.zeros(len(contigs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in contigs], dtype=np.uint64)
    return (seg.tobytes(), keys.tobytes(), mult.tobytes(), keys.shape[1], so.tobytes(), off.tobytes(), "".join(contigs).encode())


def _arr(snap, i):
    return np.frombuffer(snap[i], dtype=FIELDS[i][1])


def _segment_of(offsets, item):
    """the segment (or contig) whose range of `offsets` holds `item`; the last one for an item past the end"""
    return int(min(max(np.searchsorted(offsets, item, side="right") - 1, 0), len(offsets) - 2)) if len(offsets) > 1 else 0


def segment_value(snap, i, s):
    """what field i of a snapshot says about segment s, by the snapshot's own offsets: the number of distinct k-mers / of contigs for the
    two segment offset arrays, the contigs' lengths for the base offsets, else the segment's slice of the field"""
    if FIELDS[i][1] is None:
        return snap[i]
    seg, so = _arr(snap, SEG_OFF), _arr(snap, CSEG_OFF)
    if i in (SEG_OFF, CSEG_OFF):
        a = seg if i == SEG_OFF else so
        return int(a[s + 1]) - int(a[s]) if s + 1 < len(a) else None
    if i in (KEYS, MULT):
        if s + 1 >= len(seg):
            return None
        w = snap[WORDS] if i == KEYS else 1
        return _arr(snap, i)[int(seg[s]) * w:int(seg[s + 1]) * w].tobytes()
    if s + 1 >= len(so):
        return None
    a, z = int(so[s]), int(so[s + 1])
    if i in (C_OFF, TEXT):
        off = _arr(snap, C_OFF)
        if z >= len(off) or a > z:
            return None
        return np.diff(off[a:z + 1]).tobytes() if i == C_OFF else bytes(snap[TEXT][int(off[a]):int(off[z])])
    return _arr(snap, i)[a:z].tobytes()


def segment_values(snap, s):
    """segment_value of every array field the snapshot has"""
    return tuple(segment_value(snap, i, s) for i in range(len(snap)) if FIELDS[i][1] is not None)


def first_difference(got, want):
    """None, or (field index, segment, element, found, expected) of the first field, in the order of FIELDS, in which two snapshots differ
    and of the first element that differs there; the segment is told by the offsets of `want`"""
    assert len(got) == len(want), (len(got), len(want))
    for i in range(len(want)):
        if got[i] == want[i]:
            continue
        if FIELDS[i][1] is None:
            return i, 0, 0, got[i], want[i]
        g, w = _arr(got, i), _arr(want, i)
        n = min(len(g), len(w))
        ne = np.flatnonzero(g[:n] != w[:n])
        j = int(ne[0]) if len(ne) else n
        seg, so, off = _arr(want, SEG_OFF), _arr(want, CSEG_OFF), _arr(want, C_OFF)
        if i in (SEG_OFF, CSEG_OFF):
            s = min(max(j - 1, 0), max(len(w) - 2, 0))        # (offset j is wrong: the count of segment j - 1 is)
        elif i in (KEYS, MULT):
            s = _segment_of(seg, j // (want[WORDS] if i == KEYS else 1))
        else:
            c = max(j - 1, 0) if i == C_OFF else _segment_of(off, j) if i == TEXT else j
            s = _segment_of(so, c)
        return i, s, j, (int(g[j]) if j < len(g) else None), (int(w[j]) if j < len(w) else None)
    return None


def difference(got, want, others=None):
    """None where two snapshots are equal.  Else a sentence: the first field and the first segment that differ, and whether what was found
    for that segment equals the expectation of another build for it (others: {name: snapshot}; a stale word that build left behind), the
    same build's expectation for another segment (a word of another segment), or neither (a wrong value)"""
    d = first_difference(got, want)
    if d is None:
        return None
    i, s, j, g, w = d
    msg = f"{FIELDS[i][0]} (field {i + 1} of {len(want)}) differ(s) first in segment {s}, at element {j}: found {g}, expected {w}"
    if FIELDS[i][1] is None:
        return msg
    found = segment_value(got, i, s)
    if found is None:
        return msg + "; what was found for the segment cannot be cut out by the offsets found"
    n_seg = len(_arr(want, SEG_OFF)) - 1
    stale = [name for name, o in (others or {}).items() if len(o) > i and s < len(_arr(o, SEG_OFF)) - 1 and segment_value(o, i, s) == found]
    moved = [t for t in range(n_seg) if t != s and segment_value(want, i, t) == found]
    what = []
    if stale:
        what.append(f"equals the expectation of {', '.join(stale)} for this segment (a stale word of that build)")
    if moved:
        near = [t for t in moved if abs(t - s) == 1]
        what.append(f"equals this build's expectation for {len(moved)} other segment(s), the first {moved[:4]}" + (f", neighbours {near}" if near else "")
                    + " (a word of another segment)")
    if not what:
        what.append("equals neither another build's expectation for this segment nor this build's for another segment (a wrong value)")
    msg += "; what was found for the segment " + " and ".join(what)
    if i in (SEG_OFF, CSEG_OFF):
        # an offset array left behind as a whole line: the element found is the other build's OFFSET there although no count of it fits
        # (seen once on the distinct offsets: element 1184, the first word of a 128-byte line; DESIGN.md, the hand-offs, "One failure since")
        kept = [name for name, o in (others or {}).items() if len(o) > i and j < len(_arr(o, i)) and int(_arr(o, i)[j]) == g]
        if kept:
            msg += f"; element {j} itself equals the offset of {', '.join(kept)} there (that build's offsets left in place from here: a stale line of a scan's output)"
    return msg


def assert_same(got, want, tag, others=None):
    msg = difference(got, want, others)
    assert msg is None, (tag, msg)


def assert_segment(got, s, ref, k, tag, others=None):
    """segment s of a whole-batch snapshot against the oracle's result for that segment alone (ref: contigs, distinct, counts); others:
    {name: the oracle's result of another build for the same segment}, to tell a stale word from a wrong one"""
    want = expected_snapshot([ref], k)
    for i in range(len(want)):
        found = segment_value(got, i, s)
        if found == segment_value(want, i, 0):
            continue
        stale = [n for n, r in (others or {}).items() if segment_value(expected_snapshot([r], k), i, 0) == found]
        raise AssertionError((tag, f"{FIELDS[i][0]} of segment {s} differ(s) from the oracle's; what was found "
                              + (f"equals the expectation of {', '.join(stale)} for this segment (a stale word of that build)" if stale else
                                 "does not equal another build's expectation for this segment")))


def words_handed_over(plan, solid_handoffs):
    """the words the last workgroups of one attempt read: bucket_d once per bucket in k_bucket_dedup and in every k_bucket_solid,
    seg_ncontig and seg_cbases once per segment in k_contig_scan"""
    return (plan["segments"] << plan["bucket_bits"]) * (1 + solid_handoffs) + 2 * plan["segments"]


# ---------------------------------------------------------------------------------------------------------------- oracle
def solid_refs(rs, k, cutoffs):
    """the oracle composition of tests/test_solid_kmers_gpu.expected for one segment and several cutoffs: {c: get_contigs of the k-mers
    seen at least c times}"""
    km = orc.kmers_from_reads(rs, k)
    cnt = collections.Counter(km)
    return {c: tr.contigs_of(km if c <= 1 else [x for x in km if cnt[x] >= c], k) for c in cutoffs}


def _sub(read, p):
    """the read with the base at p cycled A -> C -> G -> T -> A"""
    return read[:p] + "ACGTA"["ACGT".index(read[p]) + 1] + read[p + 1:]


# ---------------------------------------------------------------------------------------------------------------- grid case
GRID_SEGMENTS = 2051
GRID_KS = (21, 33)


def grid_segment(s, k):
    """the reads of segment s: a genome of 2k + 60 + (7s mod 41) bases, its head g[:cut + k] twice and its tail g[cut:] once
    (cut = k + 10 + (5s mod 23)), and 1 + s mod 3 reads g[a:a + k + 6], a = 2 + 3j, each with one substitution at k // 2 + j"""
    g = tr.strs(synth.make_segment(100000 + s, 2 * k + 60 + 7 * s % 41, planted=False)[None, :])[0]
    cut = k + 10 + 5 * s % 23
    return [g[:cut + k]] * 2 + [g[cut:]] + [_sub(g[2 + 3 * j:2 + 3 * j + k + 6], k // 2 + j) for j in range(1 + s % 3)]


@functools.lru_cache(maxsize=None)
def grid(k):
    """dict(segs, refs = {"X": per segment, "Y": per segment}, snap = {"X": expected snapshot, "Y": ...}); X = build(k), Y = build(k,
    min_count = 2).  Computed once per process; read-only"""
    segs = [grid_segment(s, k) for s in range(GRID_SEGMENTS)]
    both = [solid_refs(rs, k, (1, 2)) for rs in segs]
    refs = dict(X=[r[1] for r in both], Y=[r[2] for r in both])
    return dict(segs=segs, refs=refs, snap={n: expected_snapshot(r, k) for n, r in refs.items()})


GRID_BUILDS = dict(X=dict(), Y=dict(min_count=2))


# ---------------------------------------------------------------------------------------------------------------- ladder case
LADDER_K = 33
LADDER_HINTS = dict(P=12000, Q=10)


def fixed_mixed(parts, rl, seed0):
    """fixed-length reads of segments of different lengths: parts = [(genome length, coverage), ...]"""
    reads, off = [], [0]
    for i, (L, cov) in enumerate(parts):
        r = synth.simulate_reads(synth.make_segment(seed0 + i, L, planted=False), rl, cov, seed0 + 7919 * (i + 1))
        reads.append(r)
        off.append(off[-1] + r.shape[0])
    return dict(reads=np.concatenate(reads, axis=0), seg_off=np.array(off, dtype=np.uint64), rl=rl)


def ladder_input():
    """the B input of tests/test_build_paths_gpu.py: 70 segments, the 36th fifteen times as large as the others"""
    return fixed_mixed([(800, 12)] * 35 + [(12000, 8)] + [(800, 12)] * 34, 60, 210)


@functools.lru_cache(maxsize=None)
def ladder():
    """dict(inp, segs, refs (per segment), snap): the genome_len_hint changes the path, not the result, so P and Q share them"""
    inp = ladder_input()
    r, so = inp["reads"], inp["seg_off"]
    segs = [tr.strs(r[int(so[s]):int(so[s + 1])]) for s in range(len(so) - 1)]
    refs = [solid_refs(rs, LADDER_K, (1,))[1] for rs in segs]
    return dict(inp=inp, segs=segs, refs=refs, snap=expected_snapshot(refs, LADDER_K))


# ---------------------------------------------------------------------------------------------------------------- rounds case
ROUNDS_K = 21
ROUNDS_SEGMENTS = 64
ROUNDS_CHECKED = (0, 1, 2, 3, 17, 33, 48, 63)
_ROUNDS_SHAPE = (4000, 80, 20)                       # the README example: 4 kb, 80-base reads at 20x, 1 % substitutions


@functools.lru_cache(maxsize=None)
def rounds_input():
    """(reads array, seg_off, reads per segment as strings): segment 0 and segments 1, 2 are the three of tests/test_lowcov_gpu.py's first
    row (their restatements are shared), 61 more of the same shape follow"""
    parts = [br.noisy_segments(*_ROUNDS_SHAPE, 5, 1), br.noisy_segments(*_ROUNDS_SHAPE, 105, 1, n_seg=2),
             br.noisy_segments(*_ROUNDS_SHAPE, 205, 1, n_seg=ROUNDS_SEGMENTS - 3)]
    reads = np.concatenate([p[0] for p in parts], axis=0)
    counts = np.concatenate([np.diff(p[1].astype(np.int64)) for p in parts])
    seg_off = np.zeros(len(counts) + 1, dtype=np.uint64)
    seg_off[1:] = np.cumsum(counts)
    return reads, seg_off, [s for p in parts for s in p[2]]


def rounds_expected(s, build):
    """segment s of the rounds case: build "Z": lowcov_ref.expected_cached's dict under the README's options (ref, tips, kmers, bubbles,
    bubble_kmers, lowcov, lowcov_kmers, ...); build "X": dict(ref = the oracle's plain result)"""
    rs = rounds_input()[2][s]
    if build == "Z":
        return lr.expected_cached(rs, ROUNDS_K, **cr.readme_options(ROUNDS_K))
    return _plain_cached(s)


@functools.lru_cache(maxsize=None)
def _plain_cached(s):
    return dict(ref=solid_refs(rounds_input()[2][s], ROUNDS_K, (1,))[1])
