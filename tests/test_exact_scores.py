"""The exact score reference (oracle/exact_scores.py) against the CPU oracle (liborc) on randomised small cases: first hits
at positions 0..5, windows cut short by the end of the path, empty reads and paths, duplicate reads, reads occurring twice
in a path, reads longer than the path, break k-mer sizes other than 8, both variants, non-finite and mixed-sign tables.
kmer_breaks and path_freq are compared exactly, the oracle's hash-order doubles against the FP64 bound of DESIGN.md §3."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

from oracle import exact_scores, guided_oracle, orc


def _rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _case(rng):
    alphabet = rng.choice(["ACGT", "AC", "ACGT"])
    paths = [_rnd(rng, rng.choice([0, 1, 2, 3, 5, 9, 17, 40, 120]), alphabet) for _ in range(rng.randint(1, 7))]
    reads = []
    for p in paths:
        for _ in range(rng.randint(0, 10)):
            if not p:
                break
            a = rng.choice([0, 1, 2, 3, 4, 5, rng.randrange(len(p))])
            a = min(a, len(p) - 1)
            e = min(len(p), a + rng.randint(1, 12)) if rng.random() < 0.8 else len(p)   # some reach the path's end
            reads.append(p[a:e])
    reads += [_rnd(rng, rng.randint(1, 6), alphabet) for _ in range(rng.randint(0, 6))]      # short: often occur twice in a path
    reads += [_rnd(rng, rng.randint(130, 140), alphabet) for _ in range(rng.randint(0, 2))]  # longer than any path
    reads += [""] * rng.choice([0, 0, 1, 2])
    reads += [rng.choice(reads) for _ in range(rng.randint(0, 4))] if reads else []        # duplicates
    rng.shuffle(reads)
    return paths, reads


def _check_against_oracle(paths, reads, keys, prob, kmer, velvet, full=True):
    if not full:
        # the rows these paths can hit plus every 37th row: the oracle's map build dominates a call over all 69 904 rows
        near = {p[a:a + w] for p in paths for a in range(len(p)) for w in (2, 4, 6, 8)}
        pick = [j for j, key in enumerate(keys) if key in near or j % 37 == 0]
        keys, prob = [keys[j] for j in pick], prob[pick]
    table = dict(zip(keys, prob.tolist()))
    o = orc.calc_breakscore(paths, reads, "", kmer, keys, prob, velvet=velvet, with_lev=False, with_freq=not velvet)
    ex = exact_scores.score_paths(paths, reads, table, kmer)
    for i, e in enumerate(ex):
        tag = (kmer, velvet, i, paths[i][:20])
        assert int(o["kmer_breaks"][i]) == e.kmer_breaks, tag
        assert int(o["sequence_len"][i]) == e.length, tag
        exact_scores.check_fp64(e, float(o["bp_score"][i]), float(o["bp_score_norm_by_break_freqs"][i]), float(o["bp_score_norm_by_len"][i]),
                                tag=tag)
        if not velvet:
            assert exact_scores.same_array(o["path_freq_by_input"][i], e.row_freq(keys)), tag
    return ex


@pytest.mark.parametrize("kmer", [0, 1, 2, 5, 8, 9, 16])
@pytest.mark.parametrize("velvet", [False, True])
def test_exact_reference_against_the_oracle(qtable, kmer, velvet):
    keys, prob = qtable
    rng = random.Random(1000 * kmer + velvet)
    hits0to5 = set()
    for _ in range(40):
        paths, reads = _case(rng)
        ex = _check_against_oracle(paths, reads, keys, prob, kmer, velvet, full=False)
        for p in paths:
            for r in set(reads):
                if p.find(r) >= 0:
                    hits0to5.add(min(p.find(r), 6))
        assert len(ex) == len(paths)
    assert hits0to5 >= {0, 1, 2, 3, 4, 5}


def test_exact_reference_fixed_length_index(qtable):
    """many reads of one length take the substring index instead of find(): same hits as find() read by read"""
    keys, prob = qtable
    rng = random.Random(7)
    g = _rnd(rng, 3000)
    reads = [g[a:a + 40] for a in (rng.randrange(len(g) - 40) for _ in range(400))] + [_rnd(rng, 40) for _ in range(20)]
    paths = sorted(set(g[a:a + rng.randint(30, 900)] for a in (rng.randrange(len(g) - 30) for _ in range(25)))) + [g[:39], ""]
    _check_against_oracle(paths, reads, keys, prob, 8, False)
    table = dict(zip(keys, prob.tolist()))
    ex = exact_scores.score_paths(paths, reads, table, 8)
    uniq = sorted(set(reads))
    for p, e in zip(paths, ex):
        slow = {}
        for r in uniq:
            j = p.find(r)
            if j >= 0:
                w = exact_scores.window(p, j, 8)
                slow[w] = slow.get(w, 0) + reads.count(r)
        assert slow == e.counts


def test_exact_reference_mixed_sign_and_non_finite_tables(qtable):
    """log-probabilities (all negative) and a table with NaN / +-inf rows: S = sum |p c| bounds the oracle; a hit NaN row
    or a hit pair of opposite infinities gives NaN, one infinity gives that infinity, an unhit NaN row changes nothing"""
    keys, prob = qtable
    rng = random.Random(11)
    logp = np.log(prob)
    mixed = prob * np.where(np.arange(prob.size) % 3 == 0, -1.0, 1.0)
    for table in (logp, mixed):
        for _ in range(20):
            paths, reads = _case(rng)
            _check_against_oracle(paths, reads, keys, table, 8, False, full=False)
    paths = ["ACGTACGTACGTAAAC", "TTTTGGGGCCCC", "ACGTTTTT"]
    reads = ["ACGTA", "TTTTG", "GGCC", "TTTT", ""]
    ix = {k: i for i, k in enumerate(keys)}
    cases = {"nan": ("ACGTACGT", math.nan), "pinf": ("TTTTGGGG", math.inf), "unhit nan": ("GAGAGAGA", math.nan)}
    for name, (key, v) in cases.items():
        t = prob.copy()
        t[ix[key]] = v
        ex = _check_against_oracle(paths, reads, keys, t, 8, False)
        hit = [key in e.counts for e in ex]
        for e, h in zip(ex, hit):
            if not h:
                assert e.finite
            elif math.isnan(v):
                assert math.isnan(e.bp) and math.isnan(e.nf) and math.isnan(e.nl)
            else:
                assert e.bp == math.inf and e.nf == math.inf and e.nl == math.inf
        assert any(hit) == (name != "unhit nan")
    t = prob.copy()
    t[ix["TTTTGGGG"]], t[ix["ACGTTTTT"]] = math.inf, -math.inf
    ex = _check_against_oracle(["TTTTGGGGACGTTTTT"], ["TTTTG", "ACGTT", "ACGTTTTT"], keys, t, 0, False)
    assert math.isnan(ex[0].bp)


def test_exact_reference_edges():
    table = {"AC": 0.5, "ACGT": 0.25, "ACGTAC": 0.125, "ACGTACGT": 2.0 ** -40}
    (e,) = exact_scores.score_paths(["ACGTACGTAC"], ["ACGTAC", "CGT", "GTA", "TACG", "", "", "X"], table, 8)
    # hits: "" x2 at 0 -> ACGTACGT; CGT at 1 -> AC; GTA at 2 -> ACGT; TACG at 3 -> ACGTAC; ACGTAC at 0 -> ACGTACGT
    assert e.counts == {"ACGTACGT": 3, "AC": 1, "ACGT": 1, "ACGTAC": 1}
    assert e.kmer_breaks == 6 and e.m == 6
    assert e.bp == Fraction(1, 2) + Fraction(1, 4) + Fraction(1, 8) + 3 * Fraction(1, 2 ** 40)
    assert e.nf == e.bp / 6 and e.nl == e.bp / 10
    assert e.fixed_sum(3) == 4 + 2 + 1 and e.fixed_sum(40) == 2 ** 39 + 2 ** 38 + 2 ** 37 + 3
    assert e.fixed_sum(2) == 2 + 1 + 0            # 0.5 rounds half to even
    (e,) = exact_scores.score_paths([""], ["", "A"], table, 8)
    assert e.kmer_breaks == 1 and e.bp == 0 and e.nl is None and e.row_freq(["AC"]).tolist() == [0.0]
    (e,) = exact_scores.score_paths(["ACGT"], ["T" * 9], table, 8)
    assert e.kmer_breaks == 0 and e.nf == 0 and math.isnan(e.row_freq(["AC"])[0])
    # the guided traversal's sums are these sums
    assert guided_oracle.fixed_sums(["ACGTACGTAC"], ["CGT", "GTA"], table, 8, 5) == [round(Fraction(3, 4) * 32)]


def test_fixed_shift_restatement():
    assert exact_scores.fixed_shift(np.full(10, 2.0 ** -4), 1) == 65           # x = 2^-4 exactly: x 2^65 = 2^61
    assert exact_scores.fixed_shift(np.full(10, 0.75 * 2.0 ** -4), 1) == 65    # x 2^65 = 1.5 2^60
    assert exact_scores.fixed_shift(np.zeros(4), 10) == 62
    assert exact_scores.fixed_shift(np.array([1.0, math.nan]), 10) is None
    assert exact_scores.fixed_shift(np.array([2.0 ** 62]), 1) is None
    assert exact_scores.fixed_shift(np.array([2.0 ** -950]), 1) is None
    assert exact_scores.fixed_shift(np.array([2.0 ** -939]), 1) == 1000
