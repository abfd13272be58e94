"""Mapped scoring on the device (gasm_batch_score_mapped: k_score_mapped; SegmentBatch.score_mapped()): at zero edits it is the exact
scorer bit for bit (gasm_batch_score_tables), with errors it is the CPU restatement of the rule in tests/mapscore_ref.py over the records
of tests/map_ref.py and tests/mapgap_ref.py — kmer_breaks, fx, starts and counters with ==, the three doubles as fx * 2^-shift and its
quotients; one ragged batch; LDS and global accumulators; error returns and what the pass leaves alone.  The contigs the restatement
starts from are the build's own.  Shapes: segments of at most 4 kb and about 1000 reads."""
import ctypes as C

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import correct_ref as cr
import mapscore_ref as ms
from genomeassembler_dev_amd import qtable, synth
from genomeassembler_dev_amd._lib import GasmError, lib

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -7
ARRAYS = ("bp_score", "bp_score_norm_by_break_freqs", "bp_score_norm_by_len", "kmer_breaks", "sequence_len")


def eight_tables():
    """the query table, the uniform one and scaled copies: five different fixed-point shifts among them"""
    q = qtable.load_normalised()
    u = np.full(len(q), 1.0 / len(q))
    return np.stack([q, u, q * 3.5, q * 2.0 ** -7, u * 0.3, q * 1e3, q * 0.11, u * 17.0])


def fixed_batch(reads):
    """a batch of one segment from equally long reads, laid out by fixed_len (from_strings lays every batch out by read_off)"""
    n = len(reads[0])
    assert all(len(r) == n for r in reads)
    return ga.SegmentBatch(np.frombuffer("".join(reads).encode(), dtype=np.uint8), np.array([0, len(reads)], np.uint64), fixed_len=n)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------- 1. equals the exact scorer
def _exact_case(name):
    if name in ("clean-k21", "clean-k33"):
        reads, _, _ = synth.make_batch(1, 3000, 70, 14, seed0=23)
        return [r.tobytes().decode() for r in reads], (lambda b: b.build(21 if name == "clean-k21" else 33))
    if name == "readme-simplified":
        k, _, reads = ms.readme_example()
        return reads, (lambda b: b.build_simplified(k, **cr.readme_options(k)))
    _, clean = cr.noisy_and_clean(3000, 80, 12, 6, 2)
    return clean, (lambda b: b.build(21, strands=2))


@pytest.mark.parametrize("name", ["clean-k21", "clean-k33", "readme-simplified", "both-strands"])
def test_zero_edits_equal_the_exact_scorer(name):
    reads, build = _exact_case(name)
    assert min(len(r) for r in reads) >= 33
    b = fixed_batch(reads)
    build(b)
    tabs = eight_tables()
    assert sum(len(c) for c in b.contigs(0)) > 0
    b.map_reads(0)
    b.map_reads_gapped(0, 0)
    sources = ("ungapped", "gapped")
    shifts, scored = set(), 0
    for T in (1, 2, 8):
        for kmer in (2, 4, 6, 8):
            b.score_tables(kmer, tabs[:T])
            want = [(b.scores(t), b.score_fixed(t)) for t in range(T)]
            for source in sources:
                m = b.score_mapped(kmer, tabs[:T] if T > 1 else tabs[0], source=source)
                assert m.n_tables == T
                for t in range(T):
                    sc, (fx, sh) = m.scores(t), m.score_fixed(t)
                    for a in ARRAYS:
                        assert same_bits(sc[a], want[t][0][a]), (name, source, T, kmer, t, a)
                    assert same_bits(fx, want[t][1][0]) and sh == want[t][1][1], (name, source, T, kmer, t)
                    shifts.add(sh)
                c = m.counters(0)
                assert int(c.sum()) == len(reads) and int(c[3]) == int(want[0][0]["kmer_breaks"].sum())
                scored = int(c[3])
    print(f"{name}: {len(b.contigs(0))} contigs, {len(reads)} reads, {scored} scored, shifts {sorted(shifts)}")
    assert len(shifts) >= 4 and scored > 0
    b.close()


# ------------------------------------------------------------------------------------------- 2. against the restatement, with errors
def check_segment(m, s, contigs, reads, rec, gap, tabs, kmer, partial, max_reads):
    """segment s of a MappedScores against the restatement: integers with ==, the doubles as the library forms them from fx"""
    r = ms.score(contigs, reads, rec, gap, list(tabs), kmer, partial, max_reads)
    assert m.counters(s).tolist() == r["counters"], (s, m.counters(s).tolist(), r["counters"])
    assert [x.tolist() for x in m.starts(s)] == r["start_pile"], s
    for t in range(len(tabs)):
        sc, (fx, sh) = m.scores(t), m.score_fixed(t)
        a, e = int(sc["seg_contig_off"][s]), int(sc["seg_contig_off"][s + 1])
        assert e - a == len(contigs) and sh == r["shift"][t]
        assert sc["kmer_breaks"][a:e].tolist() == r["kmer_breaks"] and fx[a:e].tolist() == r["fx"][t], (s, t)
        assert sc["sequence_len"][a:e].tolist() == [len(c) for c in contigs]
        d = [ms.doubles(r["fx"][t][c], sh, r["kmer_breaks"][c], len(contigs[c])) for c in range(len(contigs))]
        for i, a_name in enumerate(ARRAYS[:3]):
            assert sc[a_name][a:e].tobytes() == np.array([x[i] for x in d], np.float64).tobytes(), (s, t, a_name)
    return r


@pytest.mark.parametrize("example,params", [("readme", (2,)), ("readme", (4,)), ("indel", (6, 0)), ("indel", (6, 3))])
def test_with_errors_against_the_restatement(example, params):
    k, want_contigs, reads = ms.readme_example() if example == "readme" else ms.indel_example()
    source = "ungapped" if example == "readme" else "gapped"
    b = fixed_batch(reads)
    b.build_simplified(k, **cr.readme_options(k))
    contigs = b.contigs(0)
    assert contigs == want_contigs
    b.map_reads(*params) if source == "ungapped" else b.map_reads_gapped(*params)
    rec, gap, _ = ms.placed(contigs, reads, k, source, *params)
    tabs = eight_tables()[:2]
    for partial in (False, True):
        m = b.score_mapped(8, tabs, source=source, partial=partial)
        r = check_segment(m, 0, contigs, reads, rec, gap, tabs, 8, partial, len(reads))
        print(f"{example} {params} partial {partial}: counters {dict(zip(ms.FIELDS, r['counters']))}, scored {sum(r['kmer_breaks'])}")
        assert m.scored_fraction(0) == sum(r["kmer_breaks"]) / len(reads)
        assert m.window_counts(0, 0) == ms.window_counts(contigs[0], r["start_pile"][0], 8)
    b.close()


# -------------------------------------------------------------------------------------------------- 3. a ragged batch in one call
def test_ragged_batch_in_one_call():
    k = 21
    _, segs = ms.ragged_segments()
    most = max(len(s) for s in segs)
    b = ga.SegmentBatch.from_strings(segs)
    tabs = eight_tables()[:2]
    b.build(k, min_count=2)
    contigs = b.contigs()
    assert contigs[0] == [] and contigs[1] == [] and len(contigs[2]) >= 1 and len(contigs[3]) >= 1
    b.map_reads_gapped(6, 3)
    b.map_reads(4)
    for source, params in (("gapped", (6, 3)), ("ungapped", (4,))):
        for partial in (False, True):
            m = b.score_mapped(8, tabs, source=source, partial=partial)
            for s, reads in enumerate(segs):
                assert int(m.counters(s).sum()) == len(reads)
                rec, gap, _ = ms.placed(contigs[s], reads, k, source, *params)
                r = check_segment(m, s, contigs[s], reads, rec, gap, tabs, 8, partial, most)
                print(f"{source} partial {partial} segment {s}: {len(contigs[s])} contigs, {len(reads)} reads, counters {r['counters']}")
            assert m.counters(1).tolist() == [len(segs[1]), 0, 0, 0] and all(m.counters(2).tolist())
    # a build in which no segment has a contig: every read is unplaced, nothing is scored
    b.build(k, min_count=1000)
    assert b.contigs() == [[], [], [], []]
    b.map_reads_gapped(6, 3)
    m = b.score_mapped(8, tabs, partial=True)
    assert [m.counters(s).tolist() for s in range(4)] == [[len(s), 0, 0, 0] for s in segs]
    assert len(m.scores(1)["bp_score"]) == 0 and m.starts(3) == []
    b.close()


# -------------------------------------------------------------------------------------------- 4. LDS and global accumulators
def test_lds_and_global_accumulators(monkeypatch):
    k, _, reads = ms.readme_example()
    b = fixed_batch(reads)
    b.build(k, min_count=2)
    contigs = b.contigs(0)
    assert len(contigs) == 34
    b.map_reads(4)
    rec, gap, _ = ms.placed(contigs, reads, k, "ungapped", 4)
    tabs = eight_tables()
    for T in (8, 1):
        monkeypatch.delenv("GASM_DBG_SCORE_LDS_PATHS", raising=False)
        in_lds = b.score_mapped(8, tabs[:T], source="ungapped", partial=True)
        check_segment(in_lds, 0, contigs, reads, rec, gap, tabs[:T], 8, True, len(reads))
        monkeypatch.setenv("GASM_DBG_SCORE_LDS_PATHS", "2")           # 34 contigs do not fit two: global atomics
        in_global = b.score_mapped(8, tabs[:T], source="ungapped", partial=True)
        for t in range(T):
            for a in ARRAYS:
                assert same_bits(in_lds.scores(t)[a], in_global.scores(t)[a]), (T, t, a)
            assert same_bits(in_lds.score_fixed(t)[0], in_global.score_fixed(t)[0]) and in_lds.score_fixed(t)[1] == in_global.score_fixed(t)[1]
        assert [x.tolist() for x in in_lds.starts(0)] == [x.tolist() for x in in_global.starts(0)]
        assert in_lds.counters(0).tolist() == in_global.counters(0).tolist()
    b.close()


# ------------------------------------------------------------------------------------------------------ 5. state and isolation
def _call(b, source, kmer, tabs, n, flags):
    t = np.ascontiguousarray(tabs, dtype=np.float64)
    return lib().gasm_batch_score_mapped(b.h, source, kmer, t.ctypes.data_as(C.c_void_p), n, flags)


def _fetch(b, t):
    ps, sh = [C.c_void_p() for _ in range(6)], C.c_int()
    return lib().gasm_batch_fetch_mapped_scores(b.h, t, *[C.byref(p) for p in ps], C.byref(sh))


def test_error_returns():
    k, _, reads = ms.readme_example()
    b = fixed_batch(reads[:300])
    q = eight_tables()
    assert _call(b, 0, 8, q, 1, 0) == STATE and _fetch(b, 0) == STATE                     # before a build
    b.build(k, min_count=2)
    assert _call(b, 0, 8, q, 1, 0) == STATE and _call(b, 1, 8, q, 1, 0) == STATE          # no mapping over this build
    assert _fetch(b, 0) == STATE
    b.map_reads(2)
    assert _call(b, 1, 8, q, 1, 0) == STATE                                               # ... of that source
    assert _call(b, 0, 8, q, 2, 0) == 0
    assert _fetch(b, 0) == 0 and _fetch(b, 1) == 0 and _fetch(b, 2) == INVALID
    before = b.score_mapped(8, q[:2], source="ungapped")
    bad = q[:2].copy()
    bad[1, 5] = np.nan
    huge = q[:1] * 2.0 ** 90
    for args in ((0, 8, bad, 2, 0), (0, 8, huge, 1, 0), (0, 8, q, 0, 0), (0, 8, q, 9, 0), (0, 8, q, 1, 2), (0, 8, q, 1, 0x80000000), (2, 8, q, 1, 0),
                 (-1, 8, q, 1, 0), (0, -1, q, 1, 0)):
        assert _call(b, *args) == INVALID, args[:2] + args[3:]
    assert lib().gasm_batch_score_mapped(b.h, 0, 8, None, 1, 0) == INVALID and lib().gasm_batch_score_mapped(None, 0, 8, None, 1, 0) == INVALID
    with pytest.raises(GasmError):
        b.score_mapped(8, bad, source="ungapped")
    # nothing was queued by the refused calls: the last mapped score is still there, with both its tables
    assert _fetch(b, 1) == 0
    sp, cp = C.c_void_p(), C.c_void_p()
    assert lib().gasm_batch_fetch_mapped_starts(b.h, C.byref(sp), C.byref(cp)) == 0
    assert np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_uint64)), shape=(4,)).tolist() == before.counters(0).tolist()
    b.build(33, min_count=2)
    assert _call(b, 0, 8, q, 1, 0) == STATE and _fetch(b, 0) == STATE                     # a new build: until it is mapped again
    assert lib().gasm_batch_fetch_mapped_starts(b.h, C.byref(sp), C.byref(cp)) == STATE
    b.map_reads_gapped(2, 1)
    assert _call(b, 0, 8, q, 1, 0) == STATE and _call(b, 1, 8, q, 1, 1) == 0 and _fetch(b, 0) == 0 and _fetch(b, 1) == INVALID
    b.close()


def _map_tables(rm, gapped):
    out = [rm.records(0), *rm.pileup(0), rm.mismatch_hist(0), rm.counters(0)]
    if gapped:
        out += [rm.gap_records(0), *rm.gap_pileup(0)]
    return [np.asarray(x).tobytes() for x in out]


def test_the_pass_leaves_the_others_alone():
    k, _, reads = ms.indel_example()
    b = fixed_batch(reads)
    b.build(k, min_count=2)
    q = eight_tables()

    def snapshot():
        sc, (fx, sh) = b.scores(), b.score_fixed()
        raw = [lib().gasm_batch_fetch_read_map, lib().gasm_batch_fetch_read_map_gapped]
        ps4, ps6 = [C.c_void_p() for _ in range(4)], [C.c_void_p() for _ in range(6)]
        assert raw[0](b.h, *[C.byref(p) for p in ps4]) == 0 and raw[1](b.h, *[C.byref(p) for p in ps6]) == 0
        total = sum(len(c) for c in b.contigs(0))
        sizes4 = [4 * 4 * len(reads), 4 * 4 * total, 4 * 5, 8 * 7]
        sizes6 = [4 * 4 * len(reads), 4 * 4 * len(reads), 4 * 4 * total, 4 * 2 * total, 4 * 7, 8 * 8]
        six = [C.string_at(p, n) for p, n in zip(ps4, sizes4)] + [C.string_at(p, n) for p, n in zip(ps6, sizes6)]
        return [sc[a].tobytes() for a in ARRAYS] + [fx.tobytes(), sh] + six + [repr(b.guided())]

    b.score(8, q[0])
    b.map_reads(4)
    b.map_reads_gapped(6, 3)
    before = snapshot()
    m = b.score_mapped(8, q[1:4], source="gapped", partial=True)       # (other tables than the scorer's)
    m2 = b.score_mapped(4, q[2:3], source="ungapped")
    assert m.n_tables == 3 and m2.n_tables == 1 and int(m.counters(0)[3]) > int(m2.counters(0)[3]) > 0
    assert snapshot() == before
    b.close()


def test_interleaved_builds_over_the_step_slots():
    k, _, reads = ms.indel_example()
    tabs = eight_tables()[:2]

    def result(b):
        b.map_reads_gapped(6, 3)
        m = b.score_mapped(8, tabs, partial=True)
        return [m.scores(t)[a].tobytes() for t in range(2) for a in ARRAYS] + [m.score_fixed(t)[0].tobytes() for t in range(2)] + \
               [[x.tolist() for x in m.starts(0)], m.counters(0).tolist()]

    b = fixed_batch(reads)
    b.build(21, min_count=2)
    first = result(b)
    b.build(33, min_count=2)
    second = result(b)
    b.build(21, min_count=2)
    third = result(b)
    fresh = fixed_batch(reads)
    fresh.build(33, min_count=2)
    assert result(fresh) == second and second != first and third == first
    b.close()
    fresh.close()


def test_calc_breakscore_mapped():
    k, contigs, reads = ms.indel_example()
    m = ga.calc_breakscore_mapped(reads, k, **cr.readme_options(k))
    assert isinstance(m, ga.MappedScores) and m.contigs(0) == contigs and m.source == "gapped" and not m.partial
    assert m.counters(0).tolist() == [97, 2, 0, 873] and int(m.scores()["kmer_breaks"].sum()) == 873
    rec, gap, _ = ms.placed(contigs, reads, k, "gapped", 6, 3)
    check_segment(m, 0, contigs, reads, rec, gap, [qtable.load_normalised()], 8, False, len(reads))
