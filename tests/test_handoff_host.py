"""The preconditions of the last-workgroup hand-off tests (tests/test_handoff_gpu.py), by the oracle alone: a stale word shows only
where the build before left something else in it, and a word of another segment only where the segments differ.  So in the grid case
all three values that change hands per segment (distinct k-mers -> dstart, contigs -> seg_cstart, contig bases -> seg_bstart) differ
between the two builds in every segment and between neighbouring segments; and the comparison helper names the field and the segment
of a planted difference and tells a stale word from a wrong one."""
import numpy as np
import pytest

import handoff_cases as hc
from genomeassembler_dev_amd.api import unpack_kmers


def _three(ref):
    """what the three hand-offs carry for a segment: distinct k-mers, contigs, contig bases"""
    return len(ref["distinct"]), len(ref["contigs"]), sum(len(c) for c in ref["contigs"])


@pytest.mark.parametrize("k", hc.GRID_KS)
def test_grid_builds_differ_in_every_segment(k):
    g = hc.grid(k)
    assert len(g["segs"]) == hc.GRID_SEGMENTS == 2051
    assert all(4 <= len(rs) <= 6 for rs in g["segs"])
    x, y = [_three(r) for r in g["refs"]["X"]], [_three(r) for r in g["refs"]["Y"]]
    for s in range(hc.GRID_SEGMENTS):
        assert all(a != b for a, b in zip(x[s], y[s])), (s, x[s], y[s])                  # every value, every segment: X against Y
        assert y[s][0] >= 1 and y[s][1] == 1 and 2 <= x[s][1] <= 4, (s, x[s], y[s])      # Y leaves k-mers everywhere
        if s:
            # neighbours differ: in the distinct k-mers and the contig bases under both builds, in the contigs under X (Y has one everywhere)
            assert x[s][0] != x[s - 1][0] and x[s][2] != x[s - 1][2] and x[s][1] != x[s - 1][1], (s, x[s - 1], x[s])
            assert y[s][0] != y[s - 1][0] and y[s][2] != y[s - 1][2], (s, y[s - 1], y[s])
            assert g["refs"]["X"][s]["distinct"] != g["refs"]["X"][s - 1]["distinct"] and g["refs"]["Y"][s]["contigs"] != g["refs"]["Y"][s - 1]["contigs"]
    assert g["snap"]["X"] != g["snap"]["Y"]


def test_ladder_hint_does_not_change_the_result():
    """P and Q are builds of the same reads with the same options: one expectation serves both, for all 70 segments"""
    lad = hc.ladder()
    assert len(lad["segs"]) == len(lad["refs"]) == 70 and all(r["contigs"] for r in lad["refs"])
    assert set(hc.LADDER_HINTS) == {"P", "Q"} and hc.LADDER_HINTS["P"] != hc.LADDER_HINTS["Q"]
    sizes = [len(r["distinct"]) for r in lad["refs"]]
    assert sizes[35] > 10 * max(sizes[:35] + sizes[36:])             # the large segment is what overflows Q's first tables


def test_rounds_case_loses_kmers_in_some_round():
    reads, seg_off, segs = hc.rounds_input()
    assert len(segs) == hc.ROUNDS_SEGMENTS == 64 and int(seg_off[-1]) == reads.shape[0] and len(hc.ROUNDS_CHECKED) == 8
    lost = 0
    for s in hc.ROUNDS_CHECKED:
        z, x = hc.rounds_expected(s, "Z"), hc.rounds_expected(s, "X")
        lost += sum(z["kmers"]) + sum(z["bubble_kmers"]) + sum(z["lowcov_kmers"])
        assert _three(z["ref"]) != _three(x["ref"]), s                                   # the two builds leave different words
    assert lost >= 1


@pytest.mark.parametrize("k", [5, 31, 32, 33, 63])
def test_pack_keys_is_the_layout_of_distinct(k):
    rng = np.random.default_rng(k)
    kmers = sorted({"".join("ACGT"[c] for c in rng.integers(0, 4, k)) for _ in range(50)}) + ["A" * k, "T" * k]
    keys = hc.pack_keys(kmers, k)
    assert keys.shape == (len(kmers), 1 if k <= 31 else 2)
    assert unpack_kmers(keys.reshape(-1), k, keys.shape[1]) == kmers
    order = sorted(range(len(kmers)), key=lambda i: tuple(int(x) for x in keys[i]))       # key order is the order of the strings
    assert [kmers[i] for i in order] == sorted(kmers)


def _refs():
    mk = lambda contigs, distinct, counts: dict(contigs=contigs, distinct=distinct, counts=np.array(counts))
    x = [mk(["ACGTA", "CCGT"], ["ACG", "CCG", "CGT", "GTA"], [1, 1, 2, 1]), mk(["TTGCA"], ["GCA", "TGC", "TTG"], [3, 1, 1]), mk(["GGGAC"], ["GAC", "GGA", "GGG"], [1, 2, 2])]
    y = [mk(["CGT"], ["CGT"], [2]), mk(["TTG"], ["TTG"], [3]), mk(["GGGA"], ["GGA", "GGG"], [2, 2])]
    return x, y


def test_the_helper_names_field_and_segment_and_tells_stale_from_wrong():
    x, y = _refs()
    X, Y = hc.expected_snapshot(x, 3), hc.expected_snapshot(y, 3)
    assert hc.difference(X, X) is None and hc.first_difference(Y, Y) is None
    hc.assert_same(X, X, "equal")
    assert hc.segment_values(X, 1) == hc.segment_values(hc.expected_snapshot([x[1]], 3), 0)
    # segment 1's count of distinct k-mers left behind by Y (a stale bucket_d word): dstart is wrong from offset 2 on
    stale = hc.expected_snapshot([x[0], dict(x[1], distinct=y[1]["distinct"], counts=y[1]["counts"]), x[2]], 3)
    assert hc.first_difference(stale, X)[:3] == (hc.SEG_OFF, 1, 2)
    msg = hc.difference(stale, X, dict(Y=Y))
    assert "distinct segment offsets" in msg and "segment 1," in msg and "stale word" in msg and "expectation of Y" in msg
    # segment 2's contigs replaced by segment 1's: the offsets agree (one contig of five bases each), the text does not
    moved = hc.expected_snapshot([x[0], x[1], dict(x[2], contigs=x[1]["contigs"])], 3)
    assert hc.first_difference(moved, X)[:2] == (hc.TEXT, 2)
    msg = hc.difference(moved, X, dict(Y=Y))
    assert "contig text" in msg and "segment 2," in msg and "another segment" in msg and "[1]" in msg and "stale" not in msg
    # a multiplicity nobody expects
    wrong = hc.expected_snapshot([x[0], dict(x[1], counts=np.array([3, 1, 7])), x[2]], 3)
    assert hc.first_difference(wrong, X) == (hc.MULT, 1, 6, 7, 1)
    assert "a wrong value" in hc.difference(wrong, X, dict(Y=Y))
    # Y's distinct offsets with X's left in place from element 2 on (a stale line of the scan's output): no build's count of segment 1
    # fits what was found, but the element itself is X's offset there, and the message says so
    offs = np.frombuffer(Y[hc.SEG_OFF], dtype="<u8").copy()
    offs[2:] = np.frombuffer(X[hc.SEG_OFF], dtype="<u8")[2:]
    line = (offs.tobytes(),) + Y[1:]
    assert hc.first_difference(line, Y)[:3] == (hc.SEG_OFF, 1, 2)
    msg = hc.difference(line, Y, dict(X=X))
    assert "a wrong value" in msg and "element 2 itself equals the offset of X there" in msg and "stale line" in msg
    assert "stale line" not in hc.difference(stale, X, dict(Y=Y))
    # a contig too many in segment 0: the contig segment offsets come first, then nothing else is looked at
    more = hc.expected_snapshot([dict(x[0], contigs=["ACGTA", "CCGT", "GTA"]), x[1], x[2]], 3)
    assert hc.first_difference(more, X)[:3] == (hc.CSEG_OFF, 0, 1)
    with pytest.raises(AssertionError, match="contig segment offsets"):
        hc.assert_same(more, X, "planted")
    # the twelve-field form: a score of the third contig belongs to segment 1
    score = lambda v: tuple(np.array(v, dtype=t).tobytes() for t in ("<f8", "<f8", "<f8", "<i4", "<i4"))
    a, b = X + score([1, 2, 3, 4]), X + score([1, 2, 3, 4])
    assert hc.difference(a, b) is None
    b = b[:10] + (np.array([1, 2, 9, 4], dtype="<i4").tobytes(),) + b[11:]
    assert hc.first_difference(a, b)[:3] == (10, 1, 2) and "kmer_breaks (field 11 of 12)" in hc.difference(a, b)
