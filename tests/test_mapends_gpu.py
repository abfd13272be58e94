"""End gaps on the device (gasm_batch_map_reads_gapped_ends: k_read_map_ends; SegmentBatch.map_reads_gapped(end_gap=...)) against the
CPU restatement of the rule in tests/mapends_ref.py: per segment the records, gap records and end records of every read, the pileup and
the gap pileup of every contig base, the edit histogram, the eight counters and the four end counters, all with ==.  The contigs the
restatement starts from are the build's own.  The preconditions of the cases are asserted on the CPU in tests/test_mapends_host.py.
Shapes: segments of at most 6 kb."""
import ctypes as C

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import correct_ref as cr
import map_ref as mr
import mapends_ref as er
import mapgap_ref as gr
import mapscore_ref as ms
from genomeassembler_dev_amd import qtable as qt
from genomeassembler_dev_amd import synth
from genomeassembler_dev_amd._lib import lib

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -7
ALL = er.SIX + ("end_records", "end_counters")
_REF = {}


def ref_place(contigs, reads, k, max_edits, max_gap, end_gap):
    key = (tuple(contigs), len(reads), hash(tuple(reads)), k, max_edits, max_gap, end_gap)
    if key not in _REF:
        _REF[key] = er.place_ends(contigs, reads, k, max_edits, max_gap, end_gap)
    return _REF[key]


def tables(rm, s):
    t = dict(records=rm.records(s).tolist(), gap_records=rm.gap_records(s).tolist(), pile=[p.tolist() for p in rm.pileup(s)],
             gap_pile=[p.tolist() for p in rm.gap_pileup(s)], edit_hist=rm.edit_hist(s).tolist(), counters=rm.counters(s).tolist())
    if rm.end_gap:
        t.update(end_records=rm.end_records(s).tolist(), end_counters=rm.end_counters(s).tolist())
    return t


def check_ends(b, segs, k, max_edits, max_gap, end_gap):
    """every segment's eight tables against the restatement; returns (GappedReadMap, {segment: the restatement's tables})"""
    rm = b.map_reads_gapped(max_edits, max_gap, end_gap)
    assert (rm.k, rm.max_edits, rm.max_gap, rm.end_gap, rm.n_segments) == (k, max_edits, max_gap, end_gap, len(segs))
    contigs = b.contigs()
    out = {}
    for s in range(len(segs)):
        t = ref_place(contigs[s], segs[s], k, max_edits, max_gap, end_gap)
        got = tables(rm, s)
        print(f"segment {s}: k {k} ({max_edits}, {max_gap}, {end_gap}): {len(contigs[s])} contigs, {len(segs[s])} reads, "
              f"counters {dict(zip(gr.FIELDS, t['counters']))}, ends {dict(zip(er.END_FIELDS, t['end_counters']))}, hist {t['edit_hist'][:32]}")
        for name in ("counters", "end_counters", "edit_hist", "records", "gap_records", "end_records", "pile", "gap_pile"):
            assert got[name] == t[name], (s, name)
        out[s] = t
    return rm, out


def test_hand_built_cases_on_the_device():
    """the cases of tests/mapends_ref.py: the table is built from three copies of every contig with min_count = 3; records, gap records
    and end records as written out by hand, per (max_edits, max_gap, end_gap)"""
    for k, table in ((5, gr.PQ), (6, [gr.R5])):
        for params in sorted({h[3:6] for h in er.HAND if h[0] == k and h[5]}):
            hand = [h for h in er.HAND if h[0] == k and h[3:6] == params]
            reads = [h[2] for h in hand] + table * 3
            b = ga.SegmentBatch.from_strings([reads])
            b.build(k, min_count=3)
            assert b.contigs(0) == table
            rm, _ = check_ends(b, [reads], k, *params)
            n = len(hand)
            assert rm.records(0).tolist()[:n] == [h[6] for h in hand] and rm.gap_records(0).tolist()[:n] == [h[7] for h in hand]
            assert rm.end_records(0).tolist()[:n] == [h[8] for h in hand]
            assert rm.end_counters(0).tolist() == [sum(h[12][f] for h in hand) for f in range(4)]
            b.close()


@pytest.mark.parametrize("k", [21, 33])
def test_the_worked_example(k):
    """mapgap_ref.indel_reads(4000, 80, 20, 5) under the simplified build, at (6, 3, 3) and (6, 0, 3); k = 33 is the 128-bit key form"""
    _, reads = gr.indel_reads(4000, 80, 20, 5)
    b = ga.SegmentBatch.from_strings([reads])
    b.build_simplified(k, **cr.readme_options(k))
    rm, ts = check_ends(b, [reads], k, 6, 3, 3)
    _, t0 = check_ends(b, [reads], k, 6, 0, 3)
    plain = gr.place_gapped(b.contigs(0), reads, k, 6, 3)
    assert gr.placed(ts[0]) > gr.placed(plain) and sum(ts[0]["end_counters"][:2]) > 0 and ts[0]["end_counters"][2] > 0
    assert sum(t0[0]["end_counters"][:2]) > 0 and t0[0]["counters"][7] == sum(1 for e in t0[0]["end_records"] if e != er.NO_ENDS)
    # the host arithmetic takes the end gaps as it takes a join
    assert [d.tolist() for d in rm.depth(0)] == gr.depth(ts[0]["pile"], ts[0]["gap_pile"])
    assert rm.indels(0) == gr.indels(ts[0]["pile"], ts[0]["gap_pile"]) and rm.error_rate(0) == gr.error_rate(ts[0]["records"], ts[0]["gap_records"])
    assert rm.consensus(0) == gr.consensus(b.contigs(0), ts[0]["pile"], ts[0]["gap_pile"])
    b.close()


def test_after_a_both_strand_build():
    k = 21
    _, reads = gr.indel_reads(4000, 80, 20, 5)
    b = ga.SegmentBatch.from_strings([reads])
    b.build_simplified(k, strands=2, **cr.readme_options(k))
    rm, ts = check_ends(b, [reads], k, 6, 3, 3)
    assert sum(ts[0]["end_counters"][:2]) > 0
    assert [f.tolist() for f in rm.pileup(0, fold_twins=True)] == mr.fold(b.contigs(0), ts[0]["pile"])
    assert [f.tolist() for f in rm.gap_pileup(0, fold_twins=True)] == gr.fold_gaps(b.contigs(0), ts[0]["gap_pile"])
    b.close()


def test_end_gap_zero_is_the_gapped_mapping_and_launches_it(monkeypatch):
    """end_gap = 0 through the new entry and the old entry give the same six arrays with the launch k_read_map_gapped and no launch
    k_read_map_ends; the end tables are refused with the state error; end_gap > 0 launches k_read_map_ends alone"""
    k = 21
    monkeypatch.setenv("GASM_PINGPONG", "0")        # every launch on the batch's own context, where the profiler counts
    _, reads = gr.indel_reads(2000, 80, 20, 28)
    ctx = ga.Context(0)
    try:
        ctx.profile(True)
        b = ga.SegmentBatch.from_strings([reads], ctx=ctx)
        pe = [C.c_void_p() for _ in range(2)]
        fetch_ends = lambda: lib().gasm_batch_fetch_read_map_ends(b.h, *[C.byref(p) for p in pe])
        assert lib().gasm_batch_map_reads_gapped_ends(b.h, 6, 3, 3) == STATE and fetch_ends() == STATE      # before a build
        b.build(k, min_count=2)
        assert fetch_ends() == STATE                                                                      # no gapped mapping over this build
        for bad in ((6, 3, 17), (6, 17, 3), (256, 3, 3)):
            assert lib().gasm_batch_map_reads_gapped_ends(b.h, *bad) == INVALID
        assert lib().gasm_batch_map_reads_gapped_ends(None, 6, 3, 3) == INVALID and lib().gasm_batch_fetch_read_map_ends(b.h, None, None) == INVALID

        def launches(f):
            ctx.profile_reset()
            out = f()
            return out, {n: v[1] for n, v in ctx.profile_read().items() if v[1] and n.startswith("k_read_map")}
        old, names = launches(lambda: b.map_reads_gapped(6, 3))
        assert names == {"k_read_map_gapped": 1} and fetch_ends() == STATE
        with pytest.raises(ValueError):
            old.end_records(0)
        with pytest.raises(ValueError):
            old.end_counters(0)
        ps = [C.c_void_p() for _ in range(6)]
        (rc, rc2), names = launches(lambda: (lib().gasm_batch_map_reads_gapped_ends(b.h, 6, 3, 0),
                                             lib().gasm_batch_fetch_read_map_gapped(b.h, *[C.byref(p) for p in ps])))
        assert (rc, rc2) == (0, 0) and names == {"k_read_map_gapped": 1} and fetch_ends() == STATE
        n, bases = len(reads), sum(len(c) for c in b.contigs(0))
        raw = [np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(m,)).copy() if m else np.zeros(0, t)
               for p, t, m in zip(ps, (C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64), (4 * n, 4 * n, 4 * bases, 2 * bases, 7, 8))]
        rec = raw[0].reshape(-1, 4)
        assert np.c_[rec[:, :2], rec[:, 2] & 0xFFFF, rec[:, 2] >> 16, rec[:, 3]].tolist() == old.records(0).tolist()
        assert raw[1].reshape(-1, 4).tolist() == old.gap_records(0).tolist() and raw[4].tolist() == old.edit_hist(0).tolist()
        assert raw[2].tolist() == np.concatenate(old.pileup(0)).reshape(-1).tolist() and raw[3].tolist() == np.concatenate(old.gap_pileup(0)).reshape(-1).tolist()
        assert raw[5].tolist() == old.counters(0).tolist()
        assert tables(old, 0) == {name: x for name, x in zip(er.SIX, er.six(ref_place(b.contigs(0), reads, k, 6, 3, 0)))}
        with_, names = launches(lambda: b.map_reads_gapped(6, 3, 3))
        assert names == {"k_read_map_ends": 1} and fetch_ends() == 0 and with_.end_gap == 3
        b.map_reads_gapped(6, 3)                                                                          # and the old entry forgets the end tables
        assert fetch_ends() == STATE
        b.close()
    finally:
        ctx.profile(False)


def test_error_free_reads_take_no_end_gap():
    k = 21
    g = synth.make_segment(81, 4000, planted=False)
    reads = gr.clean_reads(g, 80, 20, 81)
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k, min_count=2)
    rm, ts = check_ends(b, [reads], k, 6, 3, 3)
    plain = b.map_reads_gapped(6, 3)
    assert {n: x for n, x in tables(rm, 0).items() if n in er.SIX} == tables(plain, 0)
    assert not rm.end_records(0).any() and not rm.end_counters(0).any() and ts[0]["counters"][4] + ts[0]["counters"][5] == len(reads)
    b.close()


@pytest.mark.parametrize("k", er.WINDOW_K)
def test_windows_of_several_strides(k):
    """planted reads of 300, 1200 and 4096 + k - 1 bases with an indel near the back end (back windows of 4, 18 and 64 strides), a read
    with a front window of two strides (k = 63), a skipped read, beside error-free reads"""
    g, genome, planted, clean = er.window_case(k)
    names = list(planted)
    reads = clean[:10] + [planted[n] for n in names] + clean[10:]
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k, min_count=2)
    contigs = b.contigs(0)
    assert [len(c) > 5900 for c in contigs] == [True]
    rm, ts = check_ends(b, [reads], k, 6, 3, 3)
    at = {n: 10 + i for i, n in enumerate(names)}
    ends, rec = rm.end_records(0).tolist(), rm.records(0).tolist()
    for n in ("back300", "back1200", "back_max"):
        assert ends[at[n]][2] != 0 and rec[at[n]][2] == abs(ends[at[n]][2]) and ends[at[n]][3] > len(planted[n]) - k - 3, (n, rec[at[n]], ends[at[n]])
    assert rec[at["skipped"]] == mr.NO_PLACE and ts[0]["counters"][1] == 1
    if k == 63:
        assert ends[at["front2"]][:2] == [1, 20] and rec[at["front2"]][2] == 2
    assert ts[0]["end_counters"][1] >= 3
    b.close()


@pytest.mark.parametrize("strands", [1, 2])
def test_end_gaps_at_contig_ends(strands):
    """a repeat and thin coverage cut a 3 kb genome into several contigs; reads with an indel near a read end start within 100 bases of
    the repeat's ends: ends that are not eligible, ends where a candidate g is not admissible, and taken gaps"""
    k = er.ENDS_K
    _, reads, _ = er.contig_ends_case()
    b = ga.SegmentBatch.from_strings([reads])
    b.build(k, min_count=er.ENDS_MIN_COUNT, strands=strands)
    contigs = b.contigs(0)
    ineligible, partly, taken = er.contig_end_properties(contigs, reads, k, 3, 3)
    print(f"strands {strands}: {len(contigs)} contigs, ends not eligible {ineligible}, a candidate not admissible {partly}, taken gaps {taken}")
    assert len(contigs) > 2 and ineligible >= 1 and partly >= 1 and taken >= 1
    check_ends(b, [reads], k, 6, 3, 3)
    b.close()


def test_mapped_scoring_over_an_end_gapped_mapping():
    """score_mapped(source="gapped") reads rec and rec_gap as it did: the four counters and the starts are mapscore_ref's from the
    restated records, and more reads score whole than without end gaps"""
    k = 21
    _, reads = gr.indel_reads(4000, 80, 20, 5)
    b = ga.SegmentBatch.from_strings([reads])
    b.build_simplified(k, **cr.readme_options(k))
    contigs = b.contigs(0)
    q = [qt.load_normalised()]
    whole = []
    for eg in (0, 3):
        b.map_reads_gapped(6, 3, eg)
        m = b.score_mapped(8, q[0], "gapped")
        t = ref_place(contigs, reads, k, 6, 3, eg)
        r = ms.score(contigs, reads, t["records"], t["gap_records"], q, 8, False, len(reads))
        assert m.counters(0).tolist() == r["counters"] and [x.tolist() for x in m.starts(0)] == r["start_pile"]
        fx, sh = m.score_fixed(0)
        assert fx.tolist() == r["fx"][0] and sh == r["shift"][0] and m.scores(0)["kmer_breaks"].tolist() == r["kmer_breaks"]
        whole.append(r["counters"][3])
    assert whole[1] > whole[0]
    b.close()
    m = ga.calc_breakscore_mapped(reads, k, end_gap=3, **cr.readme_options(k))
    assert m.counters(0).tolist()[3] == whole[1]


@pytest.mark.parametrize("env", ["GASM_STEP_SLOTS=2", "GASM_PINGPONG=0"])
def test_step_slots(monkeypatch, env):
    """alternating builds (k = 21 and k = 33) on one batch with an end-gapped mapping after each: every mapping equals its restatement,
    whichever slot's arrays it lies in"""
    monkeypatch.setenv(*env.split("="))
    segs, steps = er.slot_case()
    b = ga.SegmentBatch.from_strings(segs)
    for (k, min_count, strands), params in steps:
        b.build(k, min_count=min_count, strands=strands)
        check_ends(b, segs, k, *params)
    b.close()
