"""Contig links on the device (gasm_batch_contig_links: k_contig_links, k_read_thread; SegmentBatch.contig_links()) against the CPU
restatement of the rule in tests/links_ref.py: per segment succ, pred, link support, span support and the skipped reads, all with ==,
and succ / pred stating the same links.  The contigs the restatement starts from are the build's own (other tests hold them against the
oracle).  Shapes: a few hundred bases per segment, reads placed so that crossings fall on the seams of the kernel's 64-position chunks."""
import ctypes as C
import random

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import links_cases as lc
import links_ref as lr
from genomeassembler_dev_amd import synth
from genomeassembler_dev_amd._lib import lib

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -7
_REF = {}


def ref_tables(contigs, reads, k, strands, span_len):
    key = (tuple(contigs), tuple(reads), k, strands, span_len)
    if key not in _REF:
        _REF[key] = lr.tables(contigs, reads, k, strands, span_len)
    return _REF[key]


def check_links(b, segs, k, strands, span_len, sample=None):
    """every (sampled) segment's five tables against the restatement; returns (ContigLinks, {segment: the restatement's tables})"""
    cl = b.contig_links(span_len)
    assert (cl.k, cl.span_len, cl.strands, cl.n_segments) == (k, span_len, strands, len(segs))
    contigs = b.contigs()
    out = {}
    for s in (range(len(segs)) if sample is None else sample):
        rs = segs[s]
        assert cl.contigs(s) == contigs[s]
        t = ref_tables(contigs[s], rs, k, strands, span_len)
        n = len(contigs[s])
        crossings, spans = sum(map(sum, t["link_support"])), sum(v for m in t["span_support"] for row in m for v in row)
        print(f"segment {s}: k {k} strands {strands} span_len {span_len}: {n} contigs, {len(lr.links_of(t['succ']))} links, {crossings} crossings, "
              f"{spans} spans, {t['skipped']} skipped")
        assert cl.succ(s).tolist() == t["succ"], (s, "succ")
        assert cl.pred(s).tolist() == t["pred"], (s, "pred")
        assert cl.link_support(s).tolist() == t["link_support"], (s, "link_support")
        assert cl.span_support(s).tolist() == t["span_support"], (s, "span_support")
        assert int(cl.skipped[s]) == t["skipped"], (s, "skipped")
        got = dict(succ=cl.succ(s).tolist(), pred=cl.pred(s).tolist())
        assert lr.consistent(got, contigs[s], k), (s, "succ and pred state different links")
        assert cl.links(s) == sorted((a, row[x], t["link_support"][a][x]) for a, row in enumerate(t["succ"]) for x in range(4) if row[x] != lr.NONE)
        assert cl.resolve_repeats(s) == lr.resolve(contigs[s], k, span_len, t, 2), (s, "resolve_repeats")
        out[s] = t
    return cl, out


def seamed_segment(k, seed):
    """a 600-base genome with one 2k-base stretch planted at 150 and 380, and its reads: ragged error-free reads (among them reads shorter
    than k, of exactly k and of k + 1 bases, and an empty one), and reads of 64 + k - 1, 64 + k and 129 + k bases cut so that a crossing
    falls between k-mers 62|63, 63|64 and 127|128 and a span starts in one chunk and ends in the next.  Returns (genome, reads, checks)"""
    rnd = random.Random(seed)
    L, Lr, p1, p2 = 600, 2 * k, 150, 380
    g = [rnd.choice("ACGT") for _ in range(L)]
    g[p2:p2 + Lr] = g[p1:p1 + Lr]
    # the flanks of the two copies differ on both sides, so the contig of the repeat is exactly the planted stretch
    g[p1 - 1], g[p2 - 1], g[p1 + Lr], g[p2 + Lr] = "A", "C", "G", "T"
    g = "".join(g)
    n_r = Lr - k + 1                                                 # edges of the repeat's contig
    reads = []
    for _ in range(90):
        n = rnd.randint(k + 2, 140)
        s = rnd.randint(0, L - n)
        reads.append(g[s:s + n])
    reads += [g[s:s + 120] for s in range(0, L, 60)]                 # (every base is covered: the genome is what the contigs add up to)
    reads += [g[:k - 1], g[5:5 + k], g[9:9 + k + 1], "", g[L - k:], g[:1]]
    q_in, q_out = p2 - 1, p2 + Lr - k                               # k-mer starts q | q + 1: Y -> R and R -> Z
    special = [(g[q_in - 62:q_in - 62 + 64 + k - 1], 62), (g[q_in - 63:q_in - 63 + 64 + k], 63), (g[q_out - 127:q_out - 127 + 129 + k], 127),
               (g[q_in - (63 - n_r // 2):q_in - (63 - n_r // 2) + 129 + k], 63 - n_r // 2)]
    reads += [r for r, _ in special]
    return g, reads, special, (p1, Lr, n_r)


def long_segment(k):
    """one read of exactly 4096 k-mers and one of 4097 (skipped) over a genome whose repeat puts crossings into the first and the last chunk"""
    rnd = random.Random(99 + k)
    Lr = 2 * k
    g = [rnd.choice("ACGT") for _ in range(4097 + k - 1)]
    g[4000:4000 + Lr] = g[100:100 + Lr]
    g[99], g[3999], g[100 + Lr], g[4000 + Lr] = "A", "C", "G", "T"
    g = "".join(g)
    return [g[:4096 + k - 1], g, g[3900:4090], g[50:300]]


@pytest.mark.parametrize("k", [11, 21, 31, 32, 33, 63])
def test_three_segments_and_the_chunk_seams(k):
    """also at the key-width seams: the in-edge of a contig's first node is built with a shift of 2 (k - 1) = 60, 62 and 124 bits"""
    g, reads, special, (p1, Lr, n_r) = seamed_segment(k, 5 + k)
    segs = [reads, [], [g[100:100 + 4 * k]]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k)
    span_len = max(len(r) for rs in segs for r in rs)                # (segment 2's read of 4k bases is the batch's longest from k = 49 on)
    cl, ts = check_links(b, segs, k, 1, span_len)
    contigs = b.contigs(0)
    r = contigs.index(g[p1:p1 + Lr])                                 # the repeat is a contig of its own
    for read, at in special:                                         # the reads do what they were cut for
        assert at in lr.crossings(contigs, read, k), at
    assert len(special[0][0]) - k + 1 == 64 and len(special[1][0]) - k + 1 == 65 and len(special[2][0]) - k + 1 == 130
    at = special[3][1]
    assert at < 63 < at + 1 + n_r and lr.tables(contigs, [special[3][0]], k, 1, span_len)["span_support"][r] != [[0] * 4] * 4
    # two spans on either path through the repeat resolve it; at k = 63 the 126-base repeat leaves too few reads that span it
    resolved = lr.resolve(contigs, k, span_len, ts[0], 2) == [g]
    assert resolved or k == 63
    assert sum(map(sum, ts[0]["span_support"][r])) >= (4 if resolved else 1) and ts[0]["skipped"] == 0
    assert len(contigs) == 4 and cl.resolve_repeats(0) == ([g] if resolved else lr.resolve(contigs, k, span_len, ts[0], 2))
    assert b.contigs(1) == [] and len(b.contigs(2)) == 1 and cl.links(2) == [] and cl.resolve_repeats(1) == []
    # default span_len: the longest read of the batch
    assert b.contig_links().span_len == span_len
    b.close()


def test_hand_built_tables_on_the_device():
    """the k = 5 cases of tests/links_cases.py, one segment each and an empty one, against the tables written out by hand: no restatement
    is asked.  (The unbranched cycle and the dead end stay on the host: a build does not cut those contigs.)  One links pass per span_len"""
    names = [n for n in sorted(lc.CASES) if n not in ("unbranched cycle", "dead end")]
    assert len(names) == 7
    segs = [lc.CASES[n][1] for n in names] + [[]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(lc.K)
    for s, n in enumerate(names):
        assert b.contigs(s) == lc.CASES[n][0], n
    assert b.contigs(len(names)) == []
    seen = []
    for span_len in sorted({lc.CASES[n][2] for n in names}):
        cl = b.contig_links(span_len)
        for s, n in enumerate(names):
            contigs, _, sl, want = lc.CASES[n]
            if sl != span_len:
                continue
            seen.append(n)
            assert cl.contigs(s) == contigs, n
            assert cl.succ(s).tolist() == want["succ"], (n, "succ")
            assert cl.pred(s).tolist() == want["pred"], (n, "pred")
            assert cl.link_support(s).tolist() == want["link_support"], (n, "link_support")
            assert cl.span_support(s).tolist() == want["span_support"], (n, "span_support")
            assert int(cl.skipped[s]) == want["skipped"] == 0, (n, "skipped")
        assert cl.links(len(names)) == [] and int(cl.skipped[len(names)]) == 0
    assert sorted(seen) == names
    b.close()


def test_a_read_of_4096_kmers_is_threaded_and_one_of_4097_is_skipped():
    k = 21
    segs = [long_segment(k), seamed_segment(k, 3)[1][:20]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k)
    cl, ts = check_links(b, segs, k, 1, 100)
    assert cl.skipped.tolist() == [1, 0] and sum(map(sum, ts[0]["link_support"])) >= 8
    contigs = b.contigs(0)
    assert {99, 3999} <= set(lr.crossings(contigs, segs[0][0], k))    # chunks 1 and 62 of the 4096-k-mer read
    b.close()


@pytest.mark.parametrize("k", [21, 32, 63])
def test_both_strands_twin_symmetry(k):
    g, reads, _, _ = seamed_segment(k, 8)
    reads = [r if i % 2 else lr.rc(r) for i, r in enumerate(reads)]
    segs = [reads, [g[:90]]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, strands=2)
    span_len = 160
    cl, ts = check_links(b, segs, k, 2, span_len)
    for s in range(2):
        tw = b.contig_twins(s).tolist()
        su, ls, sp = cl.succ(s), cl.link_support(s), cl.span_support(s)
        contigs = b.contigs(s)
        for a, bb, n in cl.links(s):
            xt = "ACGT".index(contigs[tw[a]][k - 1])
            assert int(su[tw[bb], xt]) == tw[a] and int(ls[tw[bb], xt]) == n, (s, a, bb)
        for r in range(len(contigs)):
            assert sp[r].tolist() == [[int(sp[tw[r], 3 - y, 3 - x]) for y in range(4)] for x in range(4)], (s, r)
        res = cl.resolve_repeats(s)
        assert sorted(lr.rc(x) for x in res) == res
    want = lr.resolve(b.contigs(0), k, span_len, ts[0], 2)
    assert sorted(want) == sorted([g, lr.rc(g)]) or k == 63          # (at k = 63 too few reads span the 126-base repeat)
    assert cl.resolve_repeats(0) == want
    b.close()


def test_after_a_simplified_build_and_after_correction():
    k = 21
    rnd = random.Random(17)
    g, clean, _, _ = seamed_segment(k, 12)
    clean = [r for r in clean if len(r) >= 2 * k] * 3
    noisy = []
    for i, r in enumerate(clean):
        if i % 4 == 0:
            p = rnd.randrange(len(r))
            r = r[:p] + rnd.choice([c for c in "ACGT" if c != r[p]]) + r[p + 1:]
        noisy.append(r)
    segs = [noisy, noisy[:40]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build_simplified(k, min_count=2, tip_len=2 * k - 1, tip_rounds=2, bubble_len=2 * k - 1, bubble_rounds=1, cov_cutoff=3, cov_len=2 * k - 1)
    check_links(b, segs, k, 1, 140)
    c = b.correct_reads()
    c.build(k, min_count=2)
    fixed = c.read_strings()
    cseg = [fixed[:len(noisy)], fixed[len(noisy):]]
    assert cseg[0] != noisy
    check_links(c, cseg, k, 1, 140)
    c.close()
    b.close()


def test_the_pass_changes_no_other_result(qtable):
    k = 21
    segs = [seamed_segment(k, 21)[1], seamed_segment(k, 22)[1][:50]]
    segs = [[r for r in rs if len(r) >= k] for rs in segs]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k, strands=2).score(8, qtable[1])

    def snapshot():
        sc = b.scores()
        return (b.contigs_raw()[2], tuple(sc[key].tobytes() for key in sorted(sc)), tuple(t.tobytes() for t in b.contig_coverage()),
                tuple(t.tobytes() for t in b.contig_twins()), b.distinct()[1].tobytes(), b.score_fixed()[0].tobytes())
    before = snapshot()
    first = b.contig_links(100)
    assert snapshot() == before
    again = b.contig_links(100)
    for s in range(2):
        assert first.link_support(s).tolist() == again.link_support(s).tolist() and first.span_support(s).tolist() == again.span_support(s).tolist()
    assert snapshot() == before
    b.close()


def test_span_len_zero_leaves_the_span_table_zero():
    k = 11
    segs = [seamed_segment(k, 31)[1]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build(k)
    cl, ts = check_links(b, segs, k, 1, 0)
    assert not cl.span_support(0).any() and cl.link_support(0).any()
    assert cl.resolve_repeats(0) == sorted(b.contigs(0))
    b.close()


def test_state_and_argument_errors():
    k = 21
    b = ga.SegmentBatch.from_strings([seamed_segment(k, 41)[1][:30]])
    ps = [C.c_void_p() for _ in range(5)]
    fetch = lambda: lib().gasm_batch_fetch_contig_links(b.h, *[C.byref(p) for p in ps])
    assert lib().gasm_batch_contig_links(b.h, 100) == STATE and fetch() == STATE          # before a build
    b.build(k)
    assert fetch() == STATE                                                               # no links pass over this build
    assert lib().gasm_batch_contig_links(b.h, 65536) == INVALID and fetch() == STATE
    assert lib().gasm_batch_contig_links(None, 100) == INVALID
    assert lib().gasm_batch_fetch_contig_links(b.h, None, None, None, None, None) == INVALID
    assert lib().gasm_batch_contig_links(b.h, 65535) == 0 and fetch() == 0
    b.build(k, min_count=2)
    assert fetch() == STATE                                                               # ... nor over this one yet
    with pytest.raises(ValueError):
        b.contig_links(70000)
    assert b.contig_links(80).n_segments == 1
    b.close()


def test_two_batches_interleaved_on_one_context():
    k1, k2 = 21, 33
    s1, s2 = [seamed_segment(k1, 51)[1]], [seamed_segment(k2, 52)[1], []]
    b1, b2 = ga.SegmentBatch.from_strings(s1), ga.SegmentBatch.from_strings(s2)
    b1.build(k1)
    b2.build(k2, strands=2)
    assert lib().gasm_batch_contig_links(b1.h, 150) == 0 and lib().gasm_batch_contig_links(b2.h, 150) == 0
    b1.build(k1)                                                     # a second step slot of b1, beside the pass queued on b2
    check_links(b2, s2, k2, 2, 150)
    check_links(b1, s1, k1, 1, 150)
    check_links(b2, s2, k2, 2, 90)
    b1.close()
    b2.close()


def test_worked_example_end_to_end():
    """the README's example: api.resolve_repeats gives back the genome"""
    seed, k = 28, 21
    g, p1, p2 = synth.plant_repeat(synth.make_segment(seed, 4000, planted=False), 40, seed)
    genome = g.tobytes().decode()
    reads = [r.tobytes().decode() for r in synth.simulate_reads(g, 80, 30, seed)]
    contigs, cl = ga.contig_graph(reads, k)
    assert [len(c) for c in contigs] == [698, 2203, 1099, 40] and cl.span_len == 80
    assert cl.span_support(0)[3].tolist() == [[0, 0, 0, 0], [0, 0, 0, 15], [0, 0, 0, 0], [14, 0, 0, 0]]
    assert cl.links(0) == [(0, 3, 23), (2, 3, 26), (3, 0, 20), (3, 1, 23)]          # Y -> R, X -> R, R -> Y, R -> Z
    assert ga.resolve_repeats(reads, k) == [genome]
    gfa = cl.to_gfa(0).splitlines()
    assert len(gfa) == 1 + 4 + 4 and gfa[-1] == "L\t3\t+\t1\t+\t20M\tRC:i:23"
