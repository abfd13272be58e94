"""Mapped scoring without a GPU: include/gasm.h declares the entries and states the rule, libgasm.so exports them, the ctypes mirror and
the Python surface know them and check their arguments before the library is reached; the CPU restatement of the rule
(tests/mapscore_ref.py) reproduces the issue's two worked examples, agrees at zero edits with oracle/exact_scores over str.find, and gives
on hand-built records what is written out here by hand; readmap.MappedScores' host arithmetic agrees with its restatement; the
preconditions of the GPU cases (tests/test_mapscore_gpu.py) hold on the restatement."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import mapscore_ref as ms
from oracle import exact_scores as ex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeassembler_dev_amd", "libgasm.so")
HEADER = os.path.join(ROOT, "include", "gasm.h")
SIGNATURES = {
    "gasm_batch_score_mapped": "int gasm_batch_score_mapped(gasm_batch* b, int source, int kmer, const double* tables, uint32_t n_tables, uint32_t flags);",
    "gasm_batch_fetch_mapped_scores": "int gasm_batch_fetch_mapped_scores(gasm_batch* b, uint32_t t, const double** bp_score, const double** "
                                      "norm_by_break_freqs, const double** norm_by_len, const int32_t** kmer_breaks, const int32_t** sequence_len, "
                                      "const int64_t** fx, int* shift);",
    "gasm_batch_fetch_mapped_starts": "int gasm_batch_fetch_mapped_starts(gasm_batch* b, const uint32_t** start_pile, const uint64_t** counters);",
}


def _flat(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text).replace("( ", "(").replace(" )", ")").replace(" ,", ",")


def test_header_declares_the_entries_and_the_rule():
    with open(HEADER) as f:
        raw = f.read()
    flat = _flat(raw)
    for name, sig in SIGNATURES.items():
        assert _flat(sig) in flat, name
    for d in (r"#define GASM_MAPSCORE_UNGAPPED\s+0\b", r"#define GASM_MAPSCORE_GAPPED\s+1\b", r"#define GASM_MAPSCORE_PARTIAL\s+1u", r"#define GASM_MAPSCORE_FIELDS\s+4\b"):
        assert re.search(d, raw), d
    words = " ".join(re.sub(r"(?m)^ \* ?", " ", raw).split())
    for phrase in ("Mapped scoring", "c < 0: UNPLACED", "d_1 < 0: START_CLIPPED", "overlap + ins < len: END_CLIPPED", "Otherwise: WHOLE",
                   "adds 1 to kmer_breaks[c], 1 to start_pile[c_off[c] + d_1]", "THE BEST ALIGNMENT ONLY", "NO FP64 FALLBACK",
                   "unplaced, start_clipped, end_clipped, whole", "bit for bit, the results of gasm_batch_score_tables",
                   "a repeat copy within max_edits", "gasm_batch_guided keeps using gasm_batch_score's sums"):
        assert phrase in words, phrase


def test_library_exports_the_entries():
    lib = C.CDLL(LIB)                                                # (symbol table only: nothing here calls into the library)
    for name in SIGNATURES:
        assert hasattr(lib, name), name


def test_ctypes_mirror_and_python_surface():
    from genomeassembler_dev_amd import _lib, api, batch, readmap
    import genomeassembler_dev_amd as ga
    i, vp, pp, u32 = C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32
    want = {"gasm_batch_score_mapped": (i, [vp, i, i, vp, u32, u32]),
            "gasm_batch_fetch_mapped_scores": (i, [vp, u32, pp, pp, pp, pp, pp, pp, C.POINTER(i)]),
            "gasm_batch_fetch_mapped_starts": (i, [vp, pp, pp])}
    for name, (res, args) in want.items():
        assert _lib.SYMBOLS[name][0] is res and list(_lib.SYMBOLS[name][1]) == args, name
    assert tuple(_lib.MAPSCORE_FIELDS) == ms.FIELDS and len(_lib.MAPSCORE_FIELDS) == 4
    q = inspect.signature(batch.SegmentBatch.score_mapped).parameters
    assert [(n, q[n].default) for n in list(q)[1:]] == [("kmer", 8), ("tables", None), ("source", "gapped"), ("partial", False)]
    for name in ("scores", "score_fixed", "starts", "counters", "scored_fraction", "window_counts"):
        assert callable(getattr(readmap.MappedScores, name)), name
    assert ga.MappedScores is readmap.MappedScores and ga.calc_breakscore_mapped is api.calc_breakscore_mapped
    q = inspect.signature(api.calc_breakscore_mapped).parameters
    assert list(q)[:7] == ["reads", "k", "kmer", "tables", "max_edits", "max_gap", "partial"]
    assert (q["kmer"].default, q["tables"].default, q["max_edits"].default, q["max_gap"].default, q["partial"].default) == (8, None, 6, 3, False)


def test_argument_errors_come_before_the_library():
    from genomeassembler_dev_amd import batch, qtable
    b = batch.SegmentBatch.__new__(batch.SegmentBatch)               # (no library call is reached: the checks come first)
    b.h = None
    row = np.zeros(qtable.ROWS)
    for kw in (dict(tables=np.zeros(qtable.ROWS - 1)), dict(tables=np.zeros((2, 5))), dict(tables=np.zeros((0, qtable.ROWS))),
               dict(tables=np.zeros((9, qtable.ROWS))), dict(tables=np.zeros((1, 1, qtable.ROWS))), dict(tables=row, source="both"),
               dict(tables=row, source=1), dict(tables=row, kmer=-1)):
        with pytest.raises(ValueError):
            b.score_mapped(**kw)


# ---- the worked examples of the issue: counters in the order unplaced / start_clipped / end_clipped / whole
README_ROWS = [(0, [556, 1, 1, 422]), (2, [49, 2, 2, 927]), (4, [1, 2, 2, 975])]
INDEL_ROWS = [((0, 0), [643, 1, 0, 328], 0), ((6, 0), [176, 2, 0, 794], 0), ((6, 3), [97, 2, 0, 873], 79)]


def _query():
    from genomeassembler_dev_amd import qtable
    return qtable.load_normalised()


@pytest.mark.parametrize("mm,counters", README_ROWS)
def test_the_restatement_reproduces_the_readme_example(mm, counters):
    k, contigs, reads = ms.readme_example()
    assert [len(c) for c in contigs] == [3978] and len(reads) == 980 and sum(1 for r in reads if r in contigs[0]) == 422
    rec, gap, cnt = ms.placed(contigs, reads, k, "ungapped", mm)
    assert cnt[1] == 0 and cnt[6] == 0                                # no read skipped, no block dropped
    r = ms.score(contigs, reads, rec, gap, [_query()], 8, False, len(reads))
    assert r["counters"] == counters and sum(r["kmer_breaks"]) == counters[3] == sum(map(sum, r["start_pile"]))
    rp = ms.score(contigs, reads, rec, gap, [_query()], 8, True, len(reads))
    assert rp["counters"] == counters and sum(rp["kmer_breaks"]) == counters[2] + counters[3]


@pytest.mark.parametrize("params,counters,chained", INDEL_ROWS)
def test_the_restatement_reproduces_the_indel_example(params, counters, chained):
    k, contigs, reads = ms.indel_example()
    assert [len(c) for c in contigs] == [3951] and len(reads) == 972 and sum(1 for r in reads if r in contigs[0]) == 328
    rec, gap, cnt = ms.placed(contigs, reads, k, "gapped", *params)
    assert cnt[1] == 0 and cnt[6] == 0
    r = ms.score(contigs, reads, rec, gap, [_query()], 8, False, len(reads))
    assert r["counters"] == counters and sum(r["kmer_breaks"]) == counters[3]
    assert sum(1 for rc, g, rd in zip(rec, gap, reads) if g[0] >= 2 and ms.classify(rc, g[1], len(rd)) == 3) == chained


@pytest.mark.parametrize("example,source", [("readme", "ungapped"), ("readme", "gapped"), ("indel", "ungapped"), ("indel", "gapped")])
@pytest.mark.parametrize("kmer", [2, 8])
def test_zero_edits_equal_the_exact_scorer(example, source, kmer):
    """kmer_breaks, the window counts and the fixed-point sums equal oracle/exact_scores over str.find"""
    k, contigs, reads = ms.readme_example() if example == "readme" else ms.indel_example()
    rec, gap, _ = ms.placed(contigs, reads, k, source, 0, 0)
    q = _query()
    tables = [q, np.full(len(q), 1.0 / len(q)), q * 3.5]
    r = ms.score(contigs, reads, rec, gap, tables, kmer, False, len(reads))
    assert len(set(r["shift"])) > 1                                   # (the scaled copy has another shift)
    for t, row in enumerate(tables):
        assert r["shift"][t] == ex.fixed_shift(row, len(reads))
        paths = ex.score_paths(contigs, reads, ms.table_dict(row), kmer)
        for c, p in enumerate(paths):
            assert r["kmer_breaks"][c] == p.kmer_breaks and r["fx"][t][c] == p.fixed_sum(r["shift"][t])
            assert ms.window_counts(contigs[c], r["start_pile"][c], kmer) == {w: n for w, n in p.counts.items() if n}


def test_break_window_equals_the_oracles():
    from genomeassembler_dev_amd import readmap
    s = "ACGTTGCAAGCTTAGC"
    for kmer in (0, 1, 2, 3, 4, 6, 8):
        for j in range(len(s)):
            assert ms.window(s, j, kmer) == ex.window(s, j, kmer) == readmap.break_window(s, j, kmer), (kmer, j)


# ---- hand-built records on a short contig
HC = "ACGTTGCAAGCTTAGCCA"          # 18 bases
HREAD = 12                          # every read of the hand cases is this long


def _hand(records, gaps=None, kmer=8, partial=False, table=None):
    reads = ["A" * HREAD] * len(records)
    q = table if table is not None else _query()
    return ms.score([HC], reads, records, gaps, [q], kmer, partial, len(reads))


def test_hand_built_windows():
    td = ms.table_dict(_query())
    # d_1 = 0 .. 4 at kmer = 8: windows of 8, 2, 4, 6 and 8 bases from the contig's first base; d_1 = 5: bases 1 .. 8
    want = {0: HC[0:8], 1: HC[0:2], 2: HC[0:4], 3: HC[0:6], 4: HC[0:8], 5: HC[1:9]}
    for d1, w in want.items():
        assert ms.window(HC, d1, 8) == w
        r = _hand([[0, d1, 0, 1, HREAD]])
        assert r["counters"] == [0, 0, 0, 1] and r["kmer_breaks"] == [1] and r["start_pile"][0][d1] == 1 and sum(r["start_pile"][0]) == 1
        assert r["fx"][0][0] == ms.fix(td[w], r["shift"][0])
    # kmer = 2, 4, 6: the window starts kmer / 2 in front of the break; the narrow windows only where that is the contig's first base
    assert [ms.window(HC, 3, km) for km in (2, 4, 6, 8)] == [HC[2:10], HC[1:9], HC[0:6], HC[0:6]]
    assert [ms.window(HC, 1, km) for km in (2, 4, 6, 8)] == [HC[0:2]] * 4 and ms.window(HC, 2, 2) == HC[1:9] and ms.window(HC, 2, 4) == HC[0:4]
    for km in (2, 4, 6, 8):
        r = _hand([[0, 3, 0, 1, HREAD]], kmer=km)
        assert r["fx"][0][0] == ms.fix(td[ms.window(HC, 3, km)], r["shift"][0])
    # a start fewer than 8 bases before the contig's end: the window is cut; 6 bases are a table row, 5 and 3 are not (probability 0,
    # the read still counts)
    assert ms.window(HC, 16, 8) == HC[12:18] and ms.window(HC, 17, 8) == HC[13:18] and ms.window(HC, 17, 4) == HC[15:18]
    r = _hand([[0, 16, 0, 1, 2]], partial=True)
    assert r["counters"] == [0, 0, 1, 0] and r["kmer_breaks"] == [1] and r["fx"][0][0] == ms.fix(td[HC[12:18]], r["shift"][0])
    r = _hand([[0, 17, 0, 1, 1]], partial=True)
    assert r["kmer_breaks"] == [1] and r["fx"][0][0] == 0 and r["start_pile"][0][17] == 1


def test_hand_built_classes():
    # unplaced; d_1 = -1 (never scored, with or without partial); end-clipped with and without partial; whole
    recs = [[-1, 0, 0, 0, 0], [0, -1, 0, 1, HREAD - 1], [0, 10, 0, 1, 8], [0, 2, 1, 1, HREAD]]
    r = _hand(recs)
    assert r["counters"] == [1, 1, 1, 1] and r["kmer_breaks"] == [1] and [i for i, n in enumerate(r["start_pile"][0]) if n] == [2]
    r = _hand(recs, partial=True)
    assert r["counters"] == [1, 1, 1, 1] and r["kmer_breaks"] == [2] and [i for i, n in enumerate(r["start_pile"][0]) if n] == [2, 10]
    # gapped records: an insertion of two bases (overlap + ins == len: whole), the same record read as ungapped would be end-clipped;
    # a deletion of two bases (overlap == len: whole)
    ins, dele = [0, 1, 2, 1, HREAD - 2], [0, 1, 2, 1, HREAD]
    assert _hand([ins], gaps=[[2, 2, 0, -1]])["counters"] == [0, 0, 0, 1] and _hand([ins])["counters"] == [0, 0, 1, 0]
    assert _hand([dele], gaps=[[2, 0, 2, 3]])["counters"] == [0, 0, 0, 1]
    # a gapped record that is end-clipped although it holds an insertion
    assert _hand([[0, 9, 1, 1, 8]], gaps=[[2, 1, 0, 8]])["counters"] == [0, 0, 1, 0]


def test_fixed_point_restated():
    q = _query()
    for row, n in ((q, 980), (q, 1), (q * 3.5, 972), (np.full(len(q), 1.0 / len(q)), 4096), (np.zeros(len(q)), 10), (q * 2.0 ** -40, 7)):
        assert ms.fixed_shift(row, n) == ex.fixed_shift(row, n)
    bad = q.copy()
    bad[17] = np.nan
    assert ms.fixed_shift(bad, 10) is None and ms.fixed_shift(q * 2.0 ** 90, 10) is None and ex.fixed_shift(q * 2.0 ** 90, 10) is None
    assert [ms.fix(p, 1) for p in (0.25, 0.75, 1.25, -0.25, -0.75)] == [0, 2, 2, 0, -2]      # halves to even
    assert ms.doubles(3, 1, 2, 4) == (1.5, 0.75, 0.375) and ms.doubles(0, 5, 0, 7) == (0.0, 0.0, 0.0)


def _mapped_scores(contigs, r, kmer, partial):
    from genomeassembler_dev_amd import readmap
    n = len(contigs)
    per_table = []
    for t in range(len(r["fx"])):
        d = [ms.doubles(r["fx"][t][c], r["shift"][t], r["kmer_breaks"][c], len(contigs[c])) for c in range(n)]
        per_table.append((dict(bp_score=np.array([x[0] for x in d]), bp_score_norm_by_break_freqs=np.array([x[1] for x in d]),
                               bp_score_norm_by_len=np.array([x[2] for x in d]), kmer_breaks=np.array(r["kmer_breaks"], np.int32),
                               sequence_len=np.array([len(c) for c in contigs], np.int32), seg_contig_off=np.array([0, n], np.uint64)),
                          np.array(r["fx"][t], np.int64), r["shift"][t]))
    pile = np.array([x for p in r["start_pile"] for x in p], np.uint32)
    return readmap.MappedScores(kmer, "gapped", partial, [contigs], per_table, pile, np.array(r["counters"], np.uint64))


@pytest.mark.parametrize("partial", [False, True])
def test_mapped_scores_host_arithmetic(partial):
    k, contigs, reads = ms.indel_example()
    rec, gap, _ = ms.placed(contigs, reads, k, "gapped", 6, 3)
    r = ms.score(contigs, reads, rec, gap, [_query()], 8, partial, len(reads))
    m = _mapped_scores(contigs, r, 8, partial)
    assert m.n_segments == 1 and m.n_tables == 1 and m.contigs(0) == contigs
    assert m.counters(0).tolist() == r["counters"] and m.counters(0, as_dict=True) == dict(zip(ms.FIELDS, r["counters"]))
    scored = r["counters"][3] + (r["counters"][2] if partial else 0)
    assert m.scored_fraction(0) == scored / len(reads) and sum(r["kmer_breaks"]) == scored
    assert [s.tolist() for s in m.starts(0)] == r["start_pile"]
    assert m.window_counts(0, 0) == ms.window_counts(contigs[0], r["start_pile"][0], 8) and sum(m.window_counts(0, 0).values()) == scored
    fx, sh = m.score_fixed(0)
    assert fx.tolist() == r["fx"][0] and sh == r["shift"][0] and m.scores(0)["kmer_breaks"].tolist() == r["kmer_breaks"]
    with pytest.raises(IndexError):
        m.scores(1)
    with pytest.raises(IndexError):
        m.starts(1)
    from genomeassembler_dev_amd import readmap
    empty = readmap.MappedScores(8, "ungapped", False, [[]], [], np.zeros(0, np.uint32), np.zeros(4, np.uint64))
    assert empty.scored_fraction(0) == 0.0 and empty.starts(0) == []


# ---- the preconditions of the GPU cases, on the restatement (the contigs from the oracle composition, as the GPU tests' builds give them)
def test_gpu_case_preconditions():
    import correct_ref as cr
    import lowcov_ref as lr
    k, contigs, reads = ms.readme_example()
    # with errors: every class the cases claim to cover is there (start_clipped, end_clipped and whole in every row; unplaced too)
    for mm in (2, 4):
        rec, gap, cnt = ms.placed(contigs, reads, k, "ungapped", mm)
        assert cnt[0] == cnt[1] == cnt[6] == 0
        assert all(ms.score(contigs, reads, rec, gap, [_query()], 8, False, len(reads))["counters"])
    k, icontigs, ireads = ms.indel_example()
    for me, mg in ((6, 0), (6, 3)):
        rec, gap, cnt = ms.placed(icontigs, ireads, k, "gapped", me, mg)
        assert cnt[0] == cnt[1] == cnt[6] == 0
        c = ms.score(icontigs, ireads, rec, gap, [_query()], 8, False, len(ireads))["counters"]
        assert c[0] and c[1] and c[3] and not c[2]                    # (no read of this example runs off the contig's end)
    # the many-contig build: 34 contigs, more than the LDS cap of 2 the test sets
    many = lr.expected_cached(reads, 21, min_count=2)["ref"]["contigs"]
    assert len(many) == 34
    rec, gap, cnt = ms.placed(many, reads, 21, "ungapped", 4)
    r = ms.score(many, reads, rec, gap, [_query()], 8, True, len(reads))
    assert cnt[1] == 0 and sum(1 for n in r["kmer_breaks"] if n) > 2 and all(r["counters"][1:])
    # the ragged segment: reads shorter than k, reads over both contig ends
    g, segs = ms.ragged_segments()
    rs = segs[2]
    assert any(len(x) < 21 for x in rs) and "" not in rs
    contigs2 = lr.expected_cached(rs, 21, min_count=2)["ref"]["contigs"]
    rec, gap, cnt = ms.placed(contigs2, rs, 21, "gapped", 6, 3)
    r = ms.score(contigs2, rs, rec, gap, [_query()], 8, False, max(len(s) for s in segs))
    assert cnt[0] == 3 and cnt[1] == 0 and all(r["counters"]) and r["counters"][1] >= 3 and r["counters"][2] >= 3, r["counters"]
    assert max(len(c) for c in contigs2) >= 200 and lr.expected_cached(segs[1], 21, min_count=2)["ref"]["contigs"] == []
    assert lr.expected_cached(segs[3], 21, min_count=1000)["ref"]["contigs"] == []
