"""Gapped read mapping on the device where tests/test_mapgap_gpu.py's reads of 60 to 150 bases do not reach: breakpoint windows of 3 to 63
strides, chains of eight heads, the cap of eight heads on a chained read, costs up to 255 and max_gap = 16, ragged and edge batches, two
chains that tie, chains at contig ends on both strands, and the mapping arrays of a step slot that held another build's.  Every
comparison is tests/test_mapgap_gpu.py's check_gapped: == on all six tables of every segment against tests/mapgap_ref.py, which starts
from the build's own contigs.  The cases are tests/mapgap_ref.py's; tests/test_mapgap_host.py holds their preconditions on the CPU."""
import pytest

import genomeassembler_dev_amd as ga
import map_ref as mr
import mapgap_ref as gr
from test_links_gpu import check_links
from test_map_gpu import check_map
from test_mapgap_gpu import check_gapped, tables
from test_pairs_gpu import check_places

pytestmark = pytest.mark.gpu


def one_long_contig(b, genome):
    """the build's only contig and how many bases of the genome's front it lacks"""
    contigs = b.contigs(0)
    assert len(contigs) == 1 and 0 <= len(genome) - len(contigs[0]) <= 100, [len(c) for c in contigs]
    lost = genome.index(contigs[0])
    return contigs, lost


@pytest.mark.parametrize("k", [21, 32, 63])
def test_long_reads_and_wide_windows(k):
    """reads of 300 to 1500 bases beside error-free 150-base reads of a 6 kb genome: one-indel reads whose windows take 4, 5 and 6 strides
    at max_gap = 16 and 3, a 16-base insertion, a chain of eight heads at its cost and one below, and the same chain with a dropped
    ninth head behind it, at its cost (a few dozen, and one between 200 and 255) and one below"""
    g, genome, planted, clean = gr.long_read_case(k)
    names = list(planted)
    reads = [planted[n][0] for n in names] + clean
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k, min_count=2)
    contigs, lost = one_long_contig(b, genome)
    where = mr.where_of(contigs, k)
    own = {n: gr.one_read(contigs, planted[n][0], k, 255, 16) for n in names}
    cost = {n: own[n][0][2] for n in names}
    heads = {n: mr.heads_of(where, planted[n][0], k) for n in names}
    print(f"k {k}: contig {len(contigs[0])} bases, {lost} of the genome's front lost; costs {cost}; "
          f"strides {[(n, [gr.strides(x, y) for x, y in zip(heads[n][0], heads[n][0][1:])]) for n in names]}")
    assert [gr.strides(*heads[n][0]) for n in names[:3]] == [4, 5, 6] and [len(heads[n][0]) for n in names[4:]] == [8, 8, 8]
    assert [heads[n][1] for n in names] == [0, 0, 0, 0, 0, 1, 1] and 200 <= cost["ninth_far"] <= 255 and cost["eight"] < cost["ninth"] < 200

    def run(max_edits, max_gap, accepted=(), rejected=()):
        rm, ts = check_gapped(b, [reads], k, max_edits, max_gap)
        rec, gap = rm.records(0).tolist(), rm.gap_records(0).tolist()
        for n in accepted:
            read, start, gaps = planted[n]
            i = names.index(n)
            ins, dele = sum(-x for x in gaps if x < 0), sum(x for x in gaps if x > 0)
            assert rec[i] == [0, start - lost, cost[n], 1, len(read) - ins], (n, rec[i])          # the planted place, not the restatement's
            assert gap[i] == [len(gaps) + 1, ins, dele, start - lost + sum(gaps)], (n, gap[i])
        for n in rejected:
            assert rec[names.index(n)] == mr.NO_PLACE and gap[names.index(n)] == gr.NO_GAPS, n
        return rm, ts

    ones = names[:4]
    me = max(cost[n] for n in ones)
    assert me == 16
    run(me, 16, accepted=ones + ["eight"])
    _, ts = run(me, 3, accepted=["one_del2", "one_ins2"], rejected=["ins16"])          # the 16-base gaps are not joined
    assert ts[0]["gap_records"][names.index("one_del16")][0] <= 1
    rm, _ = run(cost["eight"], 3, accepted=["eight"], rejected=["ninth", "ninth_far"])
    assert rm.gap_records(0).tolist()[names.index("eight")] == [8, 2, 10, gr.CHAIN_START - lost + 8] and int(rm.counters(0)[6]) == 2
    run(cost["eight"] - 1, 3, rejected=["eight", "ninth", "ninth_far"])
    run(cost["ninth"], 3, accepted=["eight", "ninth"], rejected=["ninth_far"])
    run(cost["ninth"] - 1, 3, accepted=["eight"], rejected=["ninth", "ninth_far"])
    rm, ts = run(255, 3, accepted=["eight", "ninth", "ninth_far"])
    assert rm.edit_hist(0).tolist()[cost["ninth_far"]] >= 1 and sum(ts[0]["edit_hist"][200:]) >= 1 and int(rm.counters(0)[6]) == 2
    run(cost["ninth_far"] - 1, 3, accepted=["eight", "ninth"], rejected=["ninth_far"])
    b.close()


def test_ragged_reads_and_edge_batches():
    """tests/test_map_gpu.py's ragged batch for the gapped kernel: a read shorter than k, an empty read, reads of exactly 4096 k-mers
    with a deletion at 4000 (a window of 63 strides) and an insertion at 4050, one of 4097 k-mers, an empty segment, a segment of
    reads shorter than k, a segment without a seed; then a build that leaves no contig, and the first build again"""
    k = gr.RAGGED_K
    g, genome, segs, at = gr.ragged_case()
    reads = segs[1]
    b = ga.SegmentBatch.from_strings(segs)

    def first_build():
        b.build(k, min_count=2)
        lost = genome.index(b.contigs(1)[0])
        assert [len(b.contigs(s)) for s in (0, 1, 2, 4, 5)] == [0, 1, 0, 0, 0] and 0 <= len(genome) - len(b.contigs(1)[0]) <= 100
        rm, ts = check_gapped(b, segs, k, 6, 3)
        rec, gap = rm.records(1).tolist(), rm.gap_records(1).tolist()
        for n in ("short", "empty", "skipped"):
            assert rec[at[n]] == mr.NO_PLACE and gap[at[n]] == gr.NO_GAPS
        assert rec[at["del3"]] == [0, 500 - lost, 3, 1, 4116] and gap[at["del3"]] == [2, 0, 3, 503 - lost]
        assert rec[at["ins2"]] == [0, 900 - lost, 2, 1, 4114] and gap[at["ins2"]] == [2, 2, 0, 898 - lost]
        assert rm.counters(1).tolist()[:2] == [2, 1] and rm.counters(2).tolist() == [len(segs[2])] + [0] * 7
        assert rm.counters(4).tolist() == [0, 0, 20, 0, 0, 0, 0, 0] and rm.records(0).shape == (0, 5) and rm.records(5).shape == (0, 5)
        (x, y), _ = mr.heads_of(mr.where_of(b.contigs(1), k), reads[at["del3"]], k)
        assert gr.strides(x, y) == 63
        return {s: tables(rm, s) for s in range(len(segs))}
    before = first_build()
    b.build(k, min_count=1000)
    assert b.contigs() == [[]] * 6
    rm, _ = check_gapped(b, segs, k, 6, 3)
    assert rm.counters(1).tolist() == [2, 1, len(reads) - 3, 0, 0, 0, 0, 0] and rm.counters(3).tolist() == [0, 0, 10, 0, 0, 0, 0, 0]
    assert rm.counters(4).tolist() == [0, 0, 20, 0, 0, 0, 0, 0] and rm.counters(2).tolist() == [len(segs[2])] + [0] * 7
    assert all(rm.pileup(s) == [] and rm.gap_pileup(s) == [] for s in range(6)) and rm.records(0).shape == (0, 5)
    assert not rm.records(1)[:, 1:].any() and not rm.gap_records(1).any() and not rm.edit_hist(1).any()
    assert first_build() == before
    b.close()


def test_ties_between_chains():
    """two accepted chains of two heads with equal overlap and cost: the chain whose first head comes first wins, once on the contig with
    the lower index and once on the other; with one substitution in the first half the second chain wins on cost"""
    k = 21
    A, B, reads, at = gr.tie_case()
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k, min_count=3)
    contigs = b.contigs(0)
    assert contigs in ([A, B], [B, A])
    ia, ib = contigs.index(A), contigs.index(B)
    for me in (1, 2):
        rm, ts = check_gapped(b, [reads], k, me, 3)
        rec, gap = rm.records(0).tolist(), rm.gap_records(0).tolist()
        assert rec[at["AB"]] == [ia, 319, 1, 2, 80] and rec[at["BA"]] == [ib, 319, 1, 2, 80], rec[:2]
        assert gap[at["AB"]] == gap[at["BA"]] == [2, 0, 1, 320]
        assert rec[at["AB_sub"]] == [ib, -80, 1, me, 80] and rec[at["BA_sub"]] == [ia, -80, 1, me, 80], rec[2:4]
        assert rm.edit_hist(0).tolist() == ts[0]["edit_hist"] == ([6, 6] if me == 1 else [6, 6, 2])
    b.close()


@pytest.mark.parametrize("strands", [1, 2])
def test_chains_at_contig_ends(strands):
    """a repeat and thin coverage cut a 3 kb genome into several contigs; reads with one indel start within 100 bases of the repeat's
    ends: chains clipped at a contig end, neighbouring heads on different contigs, reads accepted on two contigs"""
    k, me, mg = gr.CONTIG_ENDS_K, gr.CONTIG_ENDS_EDITS, gr.CONTIG_ENDS_GAP
    _, reads, _ = gr.contig_ends_case()
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k, min_count=gr.CONTIG_ENDS_MIN_COUNT, strands=strands)
    contigs = b.contigs(0)
    assert len(contigs) > 2
    clipped, crossing, multi = gr.contig_end_properties(contigs, reads, k, me, mg)
    print(f"strands {strands}: {len(contigs)} contigs, clipped chains {clipped}, crossing heads {crossing}, mapped_multi {multi}")
    assert clipped >= 1 and crossing >= 1 and multi > 0
    rm, ts = check_gapped(b, [reads], k, me, mg)
    assert int(rm.counters(0)[5]) == multi
    if strands == 2:
        assert [f.tolist() for f in rm.pileup(0, fold_twins=True)] == mr.fold(contigs, ts[0]["pile"])
        assert [f.tolist() for f in rm.gap_pileup(0, fold_twins=True)] == gr.fold_gaps(contigs, ts[0]["gap_pile"])
    b.close()


def _after_a_build(b, segs, k, strands, params):
    """the four passes that keep arrays in the slot's build state, each against its restatement in full; returns all their tables"""
    m, e, g = params
    rm, _ = check_map(b, segs, k, m)
    gm, _ = check_gapped(b, segs, k, e, g)
    cl, _ = check_links(b, segs, k, strands, 100)
    pp, _ = check_places(b, segs, k, strands, 600)
    out = []
    for s in range(len(segs)):
        out.append((tables(gm, s), rm.records(s).tolist(), [p.tolist() for p in rm.pileup(s)], rm.mismatch_hist(s).tolist(), rm.counters(s).tolist(),
                    cl.succ(s).tolist(), cl.pred(s).tolist(), cl.link_support(s).tolist(), cl.span_support(s).tolist(),
                    pp.records(s).tolist(), pp.insert_hist(s).tolist(), pp.counters(s).tolist()))
    return out


@pytest.mark.parametrize("env", ["GASM_STEP_SLOTS=2", "GASM_PINGPONG=0"])
def test_a_slots_mapping_arrays_under_another_build(monkeypatch, env):
    """five builds on one batch, with two step slots (slot 1 holds builds 1, 3, 5, slot 0 builds 2 and 4) and with one: the contig bases
    shrink to nothing and grow to twice, the reads stay, the mapping parameters move with every step; after each build both mappings,
    the links and the pair places against their restatements, and the last step equal to the same step on a fresh batch"""
    monkeypatch.setenv(*env.split("="))
    segs, steps = gr.slot_case()
    b = ga.SegmentBatch.from_strings(segs)
    bases = []
    for (k, min_count, strands), params in steps:
        b.build(k, min_count=min_count, strands=strands)
        bases.append(sum(len(c) for cs in b.contigs() for c in cs))
        last = _after_a_build(b, segs, k, strands, params)
    b.close()
    print(f"{env}: contig bases per step {bases}")
    assert bases[2] == 0 and bases[3] > bases[1] > 0 and bases[4] == bases[0] > 0
    fresh = ga.SegmentBatch.from_strings(segs)
    (k, min_count, strands), params = steps[-1]
    fresh.build(k, min_count=min_count, strands=strands)
    assert _after_a_build(fresh, segs, k, strands, params) == last
    fresh.close()
