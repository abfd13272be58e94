"""Read mapping without a GPU: include/gasm.h declares the entries and states the rule, libgasm.so exports them, the ctypes mirror and the
Python surface know them; the CPU restatement of the rule (tests/map_ref.py) reproduces the worked example's table and gives on the
hand-built k = 5 cases the records, counters and pileups written out by hand; readmap.ReadMap's host arithmetic agrees with its
restatement."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import bubbles_ref as br
import correct_ref as cr
import lowcov_ref as lr
import map_ref as mr
from links_cases import CONTIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeassembler_dev_amd", "libgasm.so")
HEADER = os.path.join(ROOT, "include", "gasm.h")
SIGNATURES = {
    "gasm_batch_map_reads": "int gasm_batch_map_reads(gasm_batch* b, uint32_t max_mismatch);",
    "gasm_batch_fetch_read_map": "int gasm_batch_fetch_read_map(gasm_batch* b, const int32_t** rec, const uint32_t** pile, const uint32_t** mismatch_hist, "
                                 "const uint64_t** counters);",
}


def _flat(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text).replace("( ", "(").replace(" )", ")")


def test_header_declares_the_entries_and_the_rule():
    with open(HEADER) as f:
        raw = f.read()
    flat = _flat(raw)
    for name, sig in SIGNATURES.items():
        assert _flat(sig) in flat, name
    for d in ("#define GASM_MAP_MAX_MISMATCH 255", "#define GASM_MAP_MAX_BLOCKS 8", "#define GASM_MAP_FIELDS 7"):
        assert d in raw, d
    words = " ".join(re.sub(r"(?m)^ \* ?", " ", raw).split())
    for phrase in ("Read mapping", "Its DIAGONAL is d = off - j, signed", "A head whose (c, d) equals an earlier head's of the same read is ignored",
                   "The head is ACCEPTED iff m <= max_mismatch", "largest overlap, then fewest mismatches, then smallest head position",
                   "short, skipped, unseeded, rejected, mapped_one, mapped_multi, blocks_dropped", "Insertions and deletions are not mapped"):
        assert phrase in words, phrase


def test_library_exports_the_entries():
    lib = C.CDLL(LIB)                                                # (symbol table only: nothing here calls into the library)
    for name in SIGNATURES:
        assert hasattr(lib, name), name


def test_ctypes_mirror_and_python_surface():
    from genomeassembler_dev_amd import _lib, api, batch, readmap
    import genomeassembler_dev_amd as ga
    i, vp, pp, u32 = C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32
    want = {"gasm_batch_map_reads": (i, [vp, u32]), "gasm_batch_fetch_read_map": (i, [vp, pp, pp, pp, pp])}
    for name, (res, args) in want.items():
        assert _lib.SYMBOLS[name][0] is res and list(_lib.SYMBOLS[name][1]) == args, name
    assert tuple(_lib.MAP_FIELDS) == mr.FIELDS and len(_lib.MAP_FIELDS) == 7 and _lib.MAP_MAX_MISMATCH == mr.MAX_MISMATCH == 255
    assert _lib.MAP_MAX_BLOCKS == mr.MAX_BLOCKS == 8
    assert inspect.signature(batch.SegmentBatch.map_reads).parameters["max_mismatch"].default == 4
    for name in ("records", "pileup", "mismatch_hist", "counters", "contigs", "depth", "mapped_fraction", "error_rate", "consensus", "variants"):
        assert callable(getattr(readmap.ReadMap, name)), name
    q = inspect.signature(readmap.ReadMap.variants).parameters
    assert (q["min_depth"].default, q["min_frac"].default) == (8, 0.2) and inspect.signature(readmap.ReadMap.consensus).parameters["min_depth"].default == 3
    assert inspect.signature(readmap.ReadMap.pileup).parameters["fold_twins"].default is False
    assert ga.ReadMap is readmap.ReadMap and ga.map_reads is api.map_reads
    q = inspect.signature(api.map_reads).parameters
    assert list(q)[:3] == ["reads", "k", "max_mismatch"] and q["max_mismatch"].default == 4
    b = batch.SegmentBatch.__new__(batch.SegmentBatch)               # (no library call is reached: the check comes first)
    b.h = None
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            b.map_reads(bad)


def _readmap(contigs, t, k, max_mismatch, strands=1, twins=None):
    from genomeassembler_dev_amd import readmap
    rec = [[c, d, m | (nb << 16), ov] for c, d, m, nb, ov in t["records"]]
    pile = [x for p in t["pile"] for x in p]
    return readmap.ReadMap(k, strands, max_mismatch, [contigs], np.array(rec, np.int32).reshape(-1), np.array(pile, np.uint32).reshape(-1),
                           np.array(t["mismatch_hist"], np.uint32), np.array(t["counters"], np.uint64), twins)


TABLE = [  # strands, build, max_mismatch, [rejected, unseeded, one, multi], mismatch_hist, (overlap, mismatches) of the best blocks
    (1, None, 0, [555, 1, 424, 0], [424], (33907, 0)),
    (1, None, 2, [48, 1, 931, 0], [424, 370, 137], (74464, 644)),
    (1, None, 4, [0, 1, 979, 0], [424, 370, 137, 35, 13], (78304, 801)),
    (1, None, 8, [0, 1, 979, 0], [424, 370, 137, 35, 13, 0, 0, 0, 0], (78304, 801)),
    (2, None, 4, [0, 1, 979, 0], [424, 370, 137, 35, 13], (78304, 801)),
    (1, dict(min_count=2), 4, [0, 1, 779, 200], [679, 396, 129, 33, 10], (74677, 749)),
]


@pytest.mark.parametrize("strands,build,mm,classes,hist,best", TABLE)
def test_the_restatement_reproduces_the_worked_example(strands, build, mm, classes, hist, best):
    k = 21
    noisy, _ = cr.noisy_and_clean(4000, 80, 20, 5, strands)
    simplified = build is None
    contigs = lr.expected_cached(noisy, k, strands=strands, **(cr.readme_options(k) if simplified else build))["ref"]["contigs"]
    assert len(contigs) == (strands if simplified else 34) and len(noisy) == 980
    t = mr.place(contigs, noisy, k, mm)
    c = dict(zip(mr.FIELDS, t["counters"]))
    assert [c["rejected"], c["unseeded"], c["mapped_one"], c["mapped_multi"]] == classes and c["short"] == c["skipped"] == c["blocks_dropped"] == 0
    assert t["mismatch_hist"] == hist and mr.best_totals(t["records"]) == best
    assert sum(hist) == sum(r[3] for r in t["records"]) and sum(map(sum, (x for p in t["pile"] for x in p))) >= best[0]
    rm = _readmap(contigs, t, k, mm)
    assert rm.error_rate(0) == best[1] / best[0] and rm.mapped_fraction(0) == (classes[2] + classes[3]) / 980
    assert rm.consensus(0) == mr.consensus(contigs, t["pile"]) and rm.variants(0) == mr.variants(contigs, t["pile"])
    assert [d.tolist() for d in rm.depth(0)] == mr.depth(t["pile"]) and rm.records(0).tolist() == t["records"]
    if simplified and strands == 1:
        assert rm.consensus(0) == contigs
        if mm >= 2:
            assert min(min(d) for d in mr.depth(t["pile"])) >= 2


def test_the_small_example():
    noisy = br.noisy_segments(400, 40, 15, 9, 1)[2][0]
    contigs = lr.expected_cached(noisy, 11, min_count=2)["ref"]["contigs"]
    t = mr.place(contigs, noisy, 11, 3)
    assert len(contigs) == 6 and t["counters"][4:6] == [117, 14] and t["mismatch_hist"][:3] == [98, 41, 10]


def test_the_variant_case():
    k = 21
    g, h, reads = mr.variant_case()
    assert len(reads) == 1166
    plain = lr.expected_cached(reads, k)["ref"]["contigs"]
    assert len(plain) == 10 and sorted(map(len, plain))[:7] == [41] * 6 + [697]
    assert mr.variants(plain, mr.place(plain, reads, k, 2)["pile"]) == []
    popped = lr.expected_cached(reads, k, bubble_len=41)["ref"]["contigs"]
    assert popped == [g[3:]] and len(popped[0]) == 2997
    t = mr.place(popped, reads, k, 2)
    assert t["counters"] == [0, 0, 0, 0, 1166, 0, 0]
    want = [(0, 697, "G", "T", 9, 28), (0, 1497, "A", "C", 7, 20), (0, 2297, "C", "G", 8, 36)]
    assert mr.variants(popped, t["pile"]) == want == _readmap(popped, t, k, 2).variants(0)
    assert [(p + 3, b) for _, p, _, b, _, _ in want] == [(p, h[p]) for p in (700, 1500, 2300)]


def test_hand_built_cases():
    for read, mm, rec, field, adds in mr.HAND:
        t = mr.place(CONTIGS, [read], mr.HAND_K, mm)
        assert t["records"] == [rec], read
        assert t["counters"] == [1 if f == field else 0 for f in mr.FIELDS], read
        got = sorted((c, p, "ACGT"[x]) for c, pl in enumerate(t["pile"]) for p, v in enumerate(pl) for x in range(4) for _ in range(v[x]))
        assert got == sorted(adds), read
        assert sum(t["mismatch_hist"]) == rec[3] and (rec[0] < 0 or t["mismatch_hist"][rec[2]] >= 1)
    where = mr.where_of(CONTIGS, mr.HAND_K)
    assert mr.heads_of(where, mr.HAND_ABA["read"], mr.HAND_K) == (mr.HAND_ABA["heads"], 0)          # A, B, C, A: the fourth head is ignored
    for mm, rec in mr.HAND_ABA["records"].items():
        assert mr.place(CONTIGS, [mr.HAND_ABA["read"]], mr.HAND_K, mm)["records"] == [rec]
    heads, dropped = mr.heads_of(mr.where_of(mr.NINE, 5), mr.NINE_READ, 5)
    assert [h[1:] for h in heads] == [(i, 1 - 5 * i) for i in range(8)] and dropped == 1 and mr.NINE_READ == "".join(c[1:6] for c in mr.NINE)
    for mm, rec, counters, hist in mr.NINE_CASES:
        t = mr.place(mr.NINE, [mr.NINE_READ], 5, mm)
        assert (t["records"], t["counters"], t["mismatch_hist"]) == ([rec], counters, hist), mm
    for cs in (mr.NINE, mr.TIE):                                      # what a build from three copies of each gives: the table itself
        assert lr.expected_cached(cs * 3, 5, min_count=3)["ref"]["contigs"] == cs
    for read, mm, rec in mr.TIE_CASES:
        assert mr.place(mr.TIE, [read], 5, mm)["records"] == [rec], (read, mm)


def test_fold_consensus_and_variants_on_a_hand_written_pileup():
    contigs = ["AACGT", "ACGTT"]                                      # twins of each other
    pile = [[[9, 0, 0, 0], [2, 0, 0, 7], [0, 8, 2, 0], [0, 0, 1, 0], [0, 0, 0, 0]],
            [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 3, 0], [0, 0, 0, 2], [0, 0, 0, 1]]]
    t = dict(records=[], pile=pile, mismatch_hist=[0], counters=[0] * 7)
    rm = _readmap(contigs, t, 5, 0, strands=2, twins=[[1, 0]])
    # contig 0 position p gets contig 1 position 4 - p with the bases complemented: [1,0,0,0]@4 <- T count of c1[0]... written out:
    folded0 = [[10, 0, 0, 0], [4, 0, 0, 7], [0, 11, 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    assert rm.pileup(0, fold_twins=True)[0].tolist() == folded0 == mr.fold(contigs, pile)[0]
    assert rm.consensus(0) == ["ATCGT", "ACGTT"] == mr.consensus(contigs, pile)           # position 1: T holds 7 of 9
    assert rm.consensus(0, min_depth=10) == contigs
    assert rm.variants(0, min_depth=8) == [(0, 1, "A", "T", 7, 9), (0, 2, "C", "G", 2, 10)] == mr.variants(contigs, pile, 8, 0.2)
    with pytest.raises(ValueError):
        _readmap(contigs, t, 5, 0).pileup(0, fold_twins=True)
    with pytest.raises(IndexError):
        rm.records(1)
