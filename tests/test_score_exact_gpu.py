"""The breakage scores of every GPU entry point against exact sums (oracle/exact_scores.py), under the numeric contract of
DESIGN.md §3:
  * fixed-point path (batch and pool scorers): fx equals the exact integer sum; bp_score == fx 2^-shift, norm_by_break_freqs
    == bp_score / kmer_breaks and norm_by_len == bp_score / len bit for bit; |bp_score - exact| <= m 2^-(shift+1) + u |exact|;
    max|p| * max_reads * 2^shift in [2^60, 2^62);
  * FP64 position path (string API, scaffolds on the device, ragged-read batches, tables the fixed point cannot hold):
    |got - exact| <= (m+2) u S; norm_by_len and path_freq bit for bit; repeated runs and different splits bit-identical.
The table edge set runs on both paths with the same reads and contigs."""
from fractions import Fraction

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
from genomeassembler_dev_amd import qtable as qt
from genomeassembler_dev_amd import synth
from oracle import exact_scores as xs

pytestmark = pytest.mark.gpu


def _strs(a):
    return [r.tobytes().decode() for r in a]


def _table(keys, prob):
    return dict(zip(keys, np.asarray(prob, dtype=np.float64).tolist()))


def _seg_reads(reads, seg_off):
    return [_strs(reads[int(seg_off[s]):int(seg_off[s + 1])]) for s in range(len(seg_off) - 1)]


def _check_batch(b, segs, keys, prob, fixed, kmer=8, ragged=False, tag=""):
    """every contig of a built + scored batch against the exact sums; fixed: the batch must be on the fixed-point path (else
    on the FP64 path, which reads of fewer than k bases always take).  Returns the scores."""
    max_reads = max(len(r) for r in segs)
    want_shift = xs.fixed_shift(prob, max_reads)
    if not ragged:
        assert (want_shift is not None) == fixed, (tag, want_shift)
    contigs, sc = b.contigs(), b.scores()
    if fixed:
        fx, shift = b.score_fixed()
        assert shift == want_shift, (tag, shift, want_shift)
        mx = Fraction(float(np.abs(prob).max()))
        if mx:
            assert 2 ** 60 <= mx * max_reads * Fraction(2) ** shift < 2 ** 62, (tag, shift)
    else:
        with pytest.raises(ga.GasmError, match="GASM_ERR_STATE"):
            b.score_fixed()
    table = _table(keys, prob)
    for s, rs in enumerate(segs):
        a, e = int(sc["seg_contig_off"][s]), int(sc["seg_contig_off"][s + 1])
        assert e - a == len(contigs[s])
        ex = xs.score_paths(contigs[s], rs, table, kmer)
        for i, x in enumerate(ex):
            c = a + i
            assert int(sc["sequence_len"][c]) == x.length
            args = (x, float(sc["bp_score"][c]), float(sc["bp_score_norm_by_break_freqs"][c]), float(sc["bp_score_norm_by_len"][c]))
            if fixed:
                xs.check_fixed(*args, fx[c], shift, breaks=sc["kmer_breaks"][c], tag=(tag, s, i))
            else:
                xs.check_fp64(*args, breaks=sc["kmer_breaks"][c], tag=(tag, s, i))
    return sc


# ------------------------------------------------------------------------------------------------ headline shapes
@pytest.mark.parametrize("n_seg,L,rl,cov,k,seed0", [(100, 50000, 150, 50, 31, 1234), (10, 50000, 250, 100, 51, 5150)],
                         ids=["configs2", "configs4_per_gpu"])
def test_headline_shapes_every_contig_exact(qtable, n_seg, L, rl, cov, k, seed0):
    """configs[2] as bench.py runs it and configs[4]'s share of one GPU: the standard table stays on the fixed-point path
    (score_fixed succeeds) and every contig of every segment meets the contract"""
    keys, prob = qtable
    reads, seg_off, _ = synth.make_batch(n_seg, L, rl, cov, seed0=seed0, planted=True)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)
    b.build(k, genome_len_hint=L).score(8, prob)
    _check_batch(b, _seg_reads(reads, seg_off), keys, prob, fixed=True, tag="headline")
    b.close()


# ------------------------------------------------------------------------------------------------ FP64 position path
def _case(seed, L=1500, rl=24, cov=40, k=15, rows=300):
    g = synth.make_segment(seed, L, n_short=4, short_len=50, n_long=2, long_len=120, tandem_len=40, planted=True)
    reads = _strs(synth.simulate_reads(g, rl, cov, seed + 1))
    m = ga.get_contigs(ga.get_kmers_from_reads(reads, k), k, 1234, matrix_rows=rows)
    return g.tobytes().decode(), reads, m, k


def _check_api(out, paths, reads, keys, prob, kmer=8, with_freq=False, tag=""):
    ex = xs.score_paths(paths, reads, _table(keys, prob), kmer)
    assert len(out["bp_score"]) == len(ex)
    for i, x in enumerate(ex):
        assert int(out["sequence_len"][i]) == x.length
        xs.check_fp64(x, float(out["bp_score"][i]), float(out["bp_score_norm_by_break_freqs"][i]), float(out["bp_score_norm_by_len"][i]),
                      breaks=out["kmer_breaks"][i], tag=(tag, i))
        if with_freq:
            assert xs.same_array(out["path_freq"][i], x.row_freq(keys)), (tag, i)


def _bits(out):
    return [np.asarray(out[k]).tobytes() for k in ("bp_score", "bp_score_norm_by_break_freqs", "bp_score_norm_by_len", "kmer_breaks")]


def test_fp64_path_string_api_and_device_scaffolds(qtable, monkeypatch):
    keys, prob = qtable
    for seed in (61, 62):
        truth, reads, m, k = _case(seed)
        paths = ga.assemble_contigs(m, k, ctx=ga.default_context())
        reads_x = reads + ["", reads[3], paths[0][:3], paths[0][-5:], "T" * 300]     # empty, duplicate, at 0, at the end, too long
        for variant in ("own", "velvet"):
            freq = variant == "own"
            o1 = ga.calc_breakscore(paths, reads_x, truth, 8, keys, prob, variant=variant, with_lev=False, with_freq=freq)
            _check_api(o1, paths, reads_x, keys, prob, with_freq=freq, tag=(seed, variant))
            o2 = ga.calc_breakscore(paths, reads_x, truth, 8, keys, prob, variant=variant, with_lev=False, with_freq=freq)
            assert _bits(o1) == _bits(o2), (seed, variant, "two runs")
            if freq:
                assert xs.same_array(o1["path_freq"], o2["path_freq"])
            # the sliced first-occurrence table: same counters, same reduction, same bits
            monkeypatch.setenv("GASM_DBG_FIRST_BUDGET", str(7 * len(reads_x)))
            o3 = ga.calc_breakscore(paths, reads_x, truth, 8, keys, prob, variant=variant, with_lev=False, with_freq=freq)
            monkeypatch.delenv("GASM_DBG_FIRST_BUDGET")
            assert _bits(o3) == _bits(o1), (seed, variant, "sliced")
        # scaffolds left on the device (gasm_calc_breakscore_dev)
        sc = ga.assemble_contigs(m, k, on_device=True)
        assert sc.strings() == paths
        od = ga.calc_breakscore(sc, reads_x, truth, 8, keys, prob, variant="own", with_lev=False, with_freq=True)
        _check_api(od, paths, reads_x, keys, prob, with_freq=True, tag=(seed, "device"))
        sc.close()


def _ragged_segments(seed0, n=5, L=1500):
    rng = np.random.default_rng(seed0)
    segs = []
    for s in range(n):
        g = _strs(synth.make_segment(seed0 + s, L, planted=False)[None, :])[0]
        rs = [g[a:a + int(rng.integers(6, 60))] for a in rng.integers(0, L - 60, 300)]
        segs.append(rs + (["", rs[0]] if s % 2 else []))
    return segs


def test_fp64_path_ragged_batch_and_second_batch(qtable):
    """ragged reads (some shorter than k, some empty) send the batch scorer down the FP64 position path: every contig meets
    the FP64 bound, fixed-point sums are refused, and two runs and a second batch give the same bits"""
    keys, prob = qtable
    segs = _ragged_segments(8200)
    b = ga.SegmentBatch.from_strings(segs)
    b.build(13).score(8, prob)
    sc1 = _check_batch(b, segs, keys, prob, fixed=False, ragged=True, tag="ragged")
    with pytest.raises(ga.GasmError):
        b.score_fixed()
    b.build(13).score(8, prob)
    assert _bits(b.scores()) == _bits(sc1)
    b.close()
    b = ga.SegmentBatch.from_strings(segs)
    b.build(13).score(8, prob)
    assert _bits(b.scores()) == _bits(sc1)
    b.close()


# ------------------------------------------------------------------------------------------------ table edge set
def _edge_tables(prob, hit_key_ix, unhit_key_ix):
    rng = np.random.default_rng(77)
    wide = np.exp2(-rng.uniform(0, 60, prob.size))
    wide[rng.random(prob.size) < 0.3] = 0.0
    onehot = np.zeros_like(prob)
    onehot[hit_key_ix] = 1.0
    t_nan, t_inf, t_unhit = prob.copy(), prob.copy(), prob.copy()
    t_nan[hit_key_ix], t_inf[hit_key_ix], t_unhit[unhit_key_ix] = np.nan, np.inf, np.nan
    return {"standard": prob, "uniform": qt.uniform(), "wide": wide, "log": np.log(prob), "onehot": onehot,
            "x1e300": prob * 1e300, "x1e-300": prob * 1e-300, "nan_hit": t_nan, "inf_hit": t_inf, "nan_unhit": t_unhit}


EDGE = ["standard", "uniform", "wide", "log", "onehot", "x1e300", "x1e-300", "nan_hit", "inf_hit", "nan_unhit"]


@pytest.fixture(scope="module")
def edge_case(qtable):
    keys, prob = qtable
    n_seg, L, rl, cov, k = 3, 9000, 60, 15, 21          # (planted repeats: a few dozen contigs per segment)
    reads, seg_off, _ = synth.make_batch(n_seg, L, rl, cov, seed0=4400, planted=True)
    segs = _seg_reads(reads, seg_off)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)
    b.build(k).score(8, prob)
    contigs = b.contigs()
    b.close()
    assert sum(len(c) for c in contigs) >= 30
    # a row the reads hit often (most common 8-base window of segment 0) and an 8-base row no contig's window is
    hits = {}
    for s in range(n_seg):
        for x in xs.score_paths(contigs[s], segs[s], _table(keys, prob), 8):
            for w, c in x.counts.items():
                hits[w] = hits.get(w, 0) + c
    hit = max((w for w in hits if len(w) == 8), key=lambda w: hits[w])
    unhit = next(key for key in keys[::-1] if len(key) == 8 and key not in hits)
    ix = {key: i for i, key in enumerate(keys)}
    return reads, seg_off, segs, rl, k, contigs, _edge_tables(prob, ix[hit], ix[unhit])


@pytest.mark.parametrize("name", EDGE)
def test_edge_tables_on_both_paths(qtable, edge_case, name):
    """the same reads and contigs scored by the batch scorer (fixed point where the table allows it, else FP64) and by the
    string API (FP64): both meet the contract and follow the exact sums' IEEE semantics for NaN / inf rows"""
    keys, _ = qtable
    reads, seg_off, segs, rl, k, contigs, tables = edge_case
    t = tables[name]
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)
    b.build(k).score(8, t)
    fixed = name in ("standard", "uniform", "wide", "log", "onehot")
    _check_batch(b, segs, keys, t, fixed=fixed, tag=name)
    assert b.contigs() == contigs
    if not fixed:
        with pytest.raises(ga.GasmError, match="GASM_ERR_STATE"):
            b.guided()
    # the same batch scored again with the standard table is back on the fixed-point path
    b.score(8, tables["standard"])
    _check_batch(b, segs, keys, tables["standard"], fixed=True, tag=(name, "standard again"))
    b.close()
    for s in range(len(segs)):
        out = ga.calc_breakscore(contigs[s], segs[s], "", 8, keys, t, with_lev=False, with_freq=(s == 0))
        _check_api(out, contigs[s], segs[s], keys, t, with_freq=(s == 0), tag=(name, s))
    if name in ("nan_hit", "inf_hit"):
        x = xs.score_paths(sum(contigs, []), sum(segs, []), _table(keys, t), 8)
        assert any(not e.finite for e in x)


# ------------------------------------------------------------------------------------------------ break k-mer != 8
@pytest.mark.parametrize("kmer", [2, 5, 16])
def test_break_kmer_sizes_on_both_paths(qtable, edge_case, kmer):
    keys, prob = qtable
    reads, seg_off, segs, rl, k, contigs, _ = edge_case
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)
    b.build(k).score(kmer, prob)
    _check_batch(b, segs, keys, prob, True, kmer=kmer, tag=kmer)
    b.close()
    out = ga.calc_breakscore(contigs[0], segs[0], "", kmer, keys, prob, with_lev=False, with_freq=True)
    _check_api(out, contigs[0], segs[0], keys, prob, kmer=kmer, with_freq=True, tag=kmer)
