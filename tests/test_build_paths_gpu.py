"""Which path a build took, and that every path gives the oracle's results.

The build picks its kernels per build: the partition (one pass into fixed regions / count + scan + scatter), the
de-duplication table (2048 / 4096 slots / more bucket bits / passes over key sub-ranges), where the bucket offsets are
scanned (in the de-duplication / k_scan_excl) and the list ranking (LDS with rulers every 2nd or 4th edge / whole-GPU
doubling), from the shape and from the retry ladder of pipeline_build_finish_n.  Each case below is an input recipe,
a genome_len_hint and the plan (SegmentBatch.build_plan) it must produce; the launch counts of the profiler are an
independent witness of the same decisions.  Results are checked bit-exact against the oracle and the scores against
the exact sums, and a second build of the same batch must give the same bits on the plan that worked.

Then: the process-wide knobs (read once per process) in fresh child processes (tests/build_paths_child.py), and distinct
batches built alternately on one context with their steps queued between fetches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import handoff_cases as hc
from genomeassembler_dev_amd import synth
from oracle import exact_scores as xs
from oracle import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strs(a):
    return [r.tobytes().decode() for r in a]


def _fixed(n_seg, L, rl, cov, seed0, planted=True):
    reads, seg_off, _g = synth.make_batch(n_seg, L, rl, cov, seed0=seed0, planted=planted)
    return dict(reads=reads, seg_off=seg_off, rl=rl)


_fixed_mixed = hc.fixed_mixed          # (fixed-length reads of segments of different lengths: parts = [(genome length, coverage), ...])


def _skewed(alphabet, L, rl, cov, seed):
    g = np.frombuffer(alphabet, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(alphabet), L)]
    reads = synth.simulate_reads(g, rl, cov, seed + 1)
    return dict(reads=reads, seg_off=np.array([0, reads.shape[0]], dtype=np.uint64), rl=rl)


def _ragged_with_empty():
    rng = np.random.default_rng(3)
    g = _strs(synth.make_segment(5, 3000, planted=False)[None, :])[0]
    seg0 = [g[a:a + int(rng.integers(10, 90))] for a in rng.integers(0, 2900, 400)]
    return dict(strings=[seg0, [], ["ACGTACGTTGCA", "ACG"], seg0[:50]])


def _long_reads():
    g2 = _strs(synth.make_segment(93, 30000, planted=False)[None, :])[0]
    circ = _strs(synth.make_segment(94, 400, planted=False)[None, :])[0]
    long_reads = [g2[100:100 + 9000], g2[4000:4000 + 17001], (circ * 3)[:1000]]
    short = [g2[i:i + 80] for i in range(0, 29900, 37)]
    return dict(strings=[long_reads + short, [(circ * 4)[i:i + 150] for i in range(0, 800, 7)]])


def _segments(inp):
    if "strings" in inp:
        return inp["strings"]
    r, so = inp["reads"], inp["seg_off"]
    return [_strs(r[int(so[s]):int(so[s + 1])]) for s in range(len(so) - 1)]


def _batch(inp, ctx):
    if "strings" in inp:
        return ga.SegmentBatch.from_strings(inp["strings"], ctx=ctx)
    return ga.SegmentBatch(inp["reads"].reshape(-1), inp["seg_off"], fixed_len=inp["rl"], ctx=ctx)


_L64, _L128 = dict(key_words=1), dict(key_words=2)
_ONE = dict(distinct_attempts=1, graph_attempts=0)
_DEFAULT = dict(single_pass=1, multi_pass=0, scan_in_dedup=1, ranked_in_lds=1, rank_global=0)


def _p(*parts, **fields):
    out = {}
    for x in parts:
        out.update(x)
    out.update(fields)
    return out


# id -> (input recipe, k, genome_len_hint, env, plan the first build must report, segments checked against the oracle)
CASES = {
    # the default: one pass, 2048-slot tables, bucket offsets scanned in the de-duplication, LDS ranking with rulers every
    # 4th edge (fewer segments than n_cu / 4)
    "default_64": (lambda: _fixed(4, 3000, 60, 15, 100), 21, 3000, {},
                   _p(_L64, _DEFAULT, _ONE, bucket_bits=4, table_slots=2048, ruler_shift=2, tile_g=4, offset_rounds=1), None),
    "default_128": (lambda: _fixed(4, 3000, 60, 15, 100), 33, 3000, {},
                    _p(_L128, _DEFAULT, _ONE, bucket_bits=4, table_slots=2048, ruler_shift=2, tile_g=4, offset_rounds=1), None),
    # a hint of 10^6 bases: ten bucket bits still leave ~977 keys per bucket -> 4096-slot tables from the start (64-bit keys;
    # 128-bit keys have 2048-slot tables only).  1024 buckets do not fit the one-pass partition's 512 cursors: two passes
    "tbl4096_upfront_64": (lambda: _fixed(2, 3000, 60, 15, 110), 21, 1_000_000, {},
                           _p(_L64, _ONE, bucket_bits=10, table_slots=4096, single_pass=0, multi_pass=0, scan_in_dedup=1,
                                ranked_in_lds=1, ruler_shift=2, rank_global=0), None),
    "tbl4096_upfront_128": (lambda: _fixed(2, 3000, 60, 15, 110), 33, 1_000_000, {},
                            _p(_L128, _ONE, bucket_bits=10, table_slots=2048, single_pass=0, multi_pass=0, scan_in_dedup=1,
                                 ranked_in_lds=1, ruler_shift=2, rank_global=0), None),
    # a far too small hint: 4 buckets of ~2000 distinct k-mers overflow the 2048-slot table -> 4096 slots (64-bit keys); the
    # 128-bit keys have no larger table -> two more bucket bits
    "tbl_2048_to_4096_64": (lambda: _fixed_mixed([(8000, 10)], 60, 120), 21, 50, {},
                            _p(_L64, _DEFAULT, bucket_bits=2, table_slots=4096, ruler_shift=2, distinct_attempts=2, graph_attempts=0), None),
    "bbits_plus2_128": (lambda: _fixed_mixed([(8000, 10)], 60, 120), 33, 50, {},
                        _p(_L128, _DEFAULT, bucket_bits=4, table_slots=2048, ruler_shift=2, distinct_attempts=2, graph_attempts=0), None),
    # ~4000 distinct k-mers per bucket overflow both tables -> two more bucket bits after the 4096-slot attempt
    "bbits_plus2_64": (lambda: _fixed_mixed([(16000, 10)], 60, 130), 21, 50, {},
                       _p(_L64, _DEFAULT, bucket_bits=4, table_slots=4096, ruler_shift=2, distinct_attempts=3, graph_attempts=0), None),
    # 3 C : 1 A: the bucket of CCCCC holds more distinct k-mers than any table even at ten bucket bits -> passes over key
    # sub-ranges (k_bucket_dedup_multi), whose bucket offsets always come from k_scan_excl.  Five attempts: the first also
    # overflows its one-pass region (two passes), then the table (64-bit: 4096 slots; 128-bit: two more bits), then two
    # more bucket bits, then the multi-pass de-duplication
    "multi_pass_64": (lambda: _skewed(b"CCCA", 30000, 100, 8, 2024), 31, 30000, {},
                      _p(_L64, bucket_bits=10, table_slots=4096, single_pass=0, multi_pass=1, scan_in_dedup=0, ranked_in_lds=1,
                           rank_global=0, distinct_attempts=5, graph_attempts=0), None),
    "multi_pass_128": (lambda: _skewed(b"CCCA", 12000, 120, 10, 2025), 45, 12000, {},
                       _p(_L128, bucket_bits=10, table_slots=2048, single_pass=0, multi_pass=1, scan_in_dedup=0, ranked_in_lds=1,
                            rank_global=0, distinct_attempts=5, graph_attempts=0), None),
    # regions of 16 keys: every bucket outgrows its region -> the build comes back through count + scan + scatter
    "region_overflow_64": (lambda: _fixed(5, 2500, 70, 20, 140), 25, 2500, {"GASM_DBG_PART_CAP": "16"},
                           _p(_L64, bucket_bits=4, table_slots=2048, single_pass=0, multi_pass=0, scan_in_dedup=1, ranked_in_lds=1,
                                ruler_shift=2, rank_global=0, distinct_attempts=2, graph_attempts=0), None),
    "region_overflow_128": (lambda: _fixed(5, 2500, 70, 20, 140), 45, 2500, {"GASM_DBG_PART_CAP": "16"},
                            _p(_L128, bucket_bits=4, table_slots=2048, single_pass=0, multi_pass=0, scan_in_dedup=1, ranked_in_lds=1,
                                 ruler_shift=2, rank_global=0, distinct_attempts=2, graph_attempts=0), None),
    # 40 segments x 512 buckets = 20 480 > 16 384: one workgroup is too slow a scanner -> k_scan_excl (one pass still)
    "scan_excl_64": (lambda: _fixed(40, 1200, 50, 10, 150), 21, 400_000, {},
                     _p(_L64, _ONE, bucket_bits=9, table_slots=2048, single_pass=1, multi_pass=0, scan_in_dedup=0, ranked_in_lds=1,
                          ruler_shift=2, rank_global=0), [0, 1, 19, 38, 39]),
    "scan_excl_128": (lambda: _fixed(40, 1200, 50, 10, 150), 33, 400_000, {},
                      _p(_L128, _ONE, bucket_bits=9, table_slots=2048, single_pass=1, multi_pass=0, scan_in_dedup=0, ranked_in_lds=1,
                           ruler_shift=2, rank_global=0), [0, 1, 19, 38, 39]),
    # 80 segments >= n_cu / 4: rulers at every second edge
    "rulers_every_2nd_64": (lambda: _fixed(80, 1500, 40, 30, 160), 15, 1500, {},
                            _p(_L64, _DEFAULT, _ONE, ruler_shift=1), [0, 1, 63, 64, 79]),
    "rulers_every_2nd_128": (lambda: _fixed(80, 1500, 60, 20, 160), 33, 1500, {},
                             _p(_L128, _DEFAULT, _ONE, ruler_shift=1), [0, 1, 63, 64, 79]),
    # a segment of ~90 000 distinct k-mers with a hint that says so: whole-GPU doubling from the start
    "rank_global_est_64": (lambda: _fixed_mixed([(90000, 12)], 120, 170), 27, 90000, {},
                           _p(_L64, _DEFAULT, _ONE, ranked_in_lds=0, ruler_shift=0), None),
    "rank_global_est_128": (lambda: _fixed_mixed([(90000, 12)], 120, 170), 41, 90000, {},
                            _p(_L128, _DEFAULT, _ONE, ranked_in_lds=0, ruler_shift=0), None),
    # the LDS ranking gives up -> the graph alone again with whole-GPU ranking.  (a) 320 small segments (more than the
    # chip's CUs: the LDS list is sized from the hint) and two segments ~13 times larger than the hint: their rulers do not
    # fit.  (b) one segment whose hint is below 65 534 but which holds ~90 000 distinct k-mers
    "lds_rank_failed_64": (lambda: _fixed_mixed([(300, 10)] * 160 + [(4000, 10)] + [(300, 10)] * 160 + [(4000, 10)], 40, 180), 21, 300, {},
                           _p(_L64, _DEFAULT, ranked_in_lds=0, ruler_shift=0, rank_global=1, bucket_bits=2, table_slots=2048,
                                distinct_attempts=1, graph_attempts=1), [0, 1, 159, 160, 161, 320, 321]),
    "lds_rank_failed_128": (lambda: _fixed_mixed([(300, 10)] * 160 + [(4000, 10)] + [(300, 10)] * 160 + [(4000, 10)], 40, 180), 33, 300, {},
                            _p(_L128, _DEFAULT, ranked_in_lds=0, ruler_shift=0, rank_global=1, bucket_bits=2, table_slots=2048,
                                 distinct_attempts=1, graph_attempts=1), [0, 1, 159, 160, 161, 320, 321]),
    "lds_rank_failed_oversized_64": (lambda: _fixed_mixed([(90000, 12)], 120, 170), 27, 65000, {},
                                     _p(_L64, _DEFAULT, ranked_in_lds=0, ruler_shift=0, rank_global=1, bucket_bits=9,
                                          distinct_attempts=1, graph_attempts=1), None),
    # ragged reads, an empty segment and reads shorter than k: the general (FP64 position) scorer
    "ragged_empty_64": (_ragged_with_empty, 11, 0, {},
                        _p(_L64, _DEFAULT, _ONE, bucket_bits=4, table_slots=2048, ruler_shift=2, tile_g=8, offset_rounds=1), None),
    "ragged_empty_128": (_ragged_with_empty, 35, 0, {},
                         _p(_L128, _DEFAULT, _ONE, bucket_bits=3, table_slots=2048, ruler_shift=2, tile_g=8, offset_rounds=1), None),
    # reads of up to 17 001 bases: 512 threads per read and several offset rounds
    "long_reads_64": (_long_reads, 21, 0, {}, _p(_L64, _DEFAULT, _ONE, tile_g=512, offset_rounds=3), None),
    "long_reads_128": (_long_reads, 33, 0, {}, _p(_L128, _DEFAULT, _ONE, tile_g=512, offset_rounds=5), None),
}

_WITNESSES = ("k_tile_hist", "k_bucket_dedup_multi", "k_scan_excl", "k_chain_len", "k_rank_lds")


def _launches(ctx):
    got = ctx.profile_read()
    return {n: got.get(n, (0.0, 0))[1] for n in _WITNESSES}


def _launches_of_one_attempt(p):
    """what a build that needs no retry launches, from its plan"""
    return dict(k_tile_hist=1 - p["single_pass"], k_bucket_dedup_multi=p["multi_pass"], k_scan_excl=(1 - p["single_pass"]) + (1 - p["scan_in_dedup"]),
                k_chain_len=1 - p["ranked_in_lds"], k_rank_lds=p["ranked_in_lds"])


def _snapshot(b):
    """the twelve fields of handoff_cases.FIELDS, arrays as bytes"""
    return hc.snapshot(b, scores=True)


def _check_oracle_and_exact(b, segs, k, sample, keys, prob, tag):
    """contigs, distinct k-mers and multiplicities bit-exact against the oracle; scores against the exact sums (fixed-point
    path when every read holds a k-mer, else the FP64 position path)"""
    contigs, sc = b.contigs(), b.scores()
    fixed = all(len(r) >= k for rs in segs for r in rs)
    want_shift = xs.fixed_shift(prob, max(len(rs) for rs in segs))
    if fixed:
        fx, shift = b.score_fixed()
        assert shift == want_shift, (tag, shift, want_shift)
    else:
        with pytest.raises(ga.GasmError, match="GASM_ERR_STATE"):
            b.score_fixed()
    table = dict(zip(keys, np.asarray(prob, dtype=np.float64).tolist()))
    for s in sample:
        rs = segs[s]
        ref = orc.get_contigs(orc.kmers_from_reads(rs, k), k, 1, rows=1)
        assert contigs[s] == ref["contigs"], (tag, s, "contigs")
        dk, dm = b.distinct_kmers(s)
        assert dk == ref["distinct"] and dm.tolist() == ref["counts"].tolist(), (tag, s, "k-mer counts")
        a, e = int(sc["seg_contig_off"][s]), int(sc["seg_contig_off"][s + 1])
        assert e - a == len(contigs[s]), (tag, s)
        for i, x in enumerate(xs.score_paths(contigs[s], rs, table, 8)):
            c = a + i
            assert int(sc["sequence_len"][c]) == x.length, (tag, s, i)
            args = (x, float(sc["bp_score"][c]), float(sc["bp_score_norm_by_break_freqs"][c]), float(sc["bp_score_norm_by_len"][c]))
            if fixed:
                xs.check_fixed(*args, fx[c], shift, breaks=sc["kmer_breaks"][c], tag=(tag, s, i))
            else:
                xs.check_fp64(*args, breaks=sc["kmer_breaks"][c], tag=(tag, s, i))


@pytest.mark.parametrize("case", list(CASES))
def test_build_path_matrix(qtable, monkeypatch, case):
    make, k, hint, env, want, sample = CASES[case]
    keys, prob = qtable
    # every launch on the batch's own context: the profiler counts them there
    monkeypatch.setenv("GASM_PINGPONG", "0")
    for n, v in env.items():
        monkeypatch.setenv(n, v)
    inp = make()
    segs = _segments(inp)
    sample = range(len(segs)) if sample is None else sample
    assert len(segs) <= 20 or len(sample) < len(segs)
    ctx = ga.Context(0)
    b = None
    try:
        ctx.profile(True, only=_WITNESSES)
        b = _batch(inp, ctx)
        ctx.profile_reset()
        b.build(k, genome_len_hint=hint).score(8, prob)
        plan = b.build_plan()
        seen = _launches(ctx)
        assert plan["k"] == k and plan["segments"] == len(segs) and len(plan["blocks"]) == 1
        assert {n: plan[n] for n in want} == want, (case, plan)
        # the launches witness the plan: one graph per attempt, ranked in LDS or by whole-GPU doubling; the multi-pass
        # de-duplication only in the last attempt; count + scan + scatter at least where the final attempt used it
        assert seen["k_rank_lds"] + seen["k_chain_len"] == plan["distinct_attempts"] + plan["graph_attempts"], (case, seen)
        assert seen["k_bucket_dedup_multi"] == plan["multi_pass"], (case, seen)
        assert seen["k_chain_len"] >= 1 - plan["ranked_in_lds"] and seen["k_rank_lds"] >= plan["ranked_in_lds"], (case, seen)
        assert seen["k_tile_hist"] >= 1 - plan["single_pass"], (case, seen)
        assert seen["k_scan_excl"] >= (1 - plan["single_pass"]) + (1 - plan["scan_in_dedup"]), (case, seen)
        if plan["distinct_attempts"] == 1 and plan["graph_attempts"] == 0:
            assert seen == _launches_of_one_attempt(plan), (case, seen)
        _check_oracle_and_exact(b, segs, k, sample, keys, prob, case)
        first = _snapshot(b)
        # the same batch again: the plan that worked is kept (no retry) and the bits are the same
        ctx.profile_reset()
        b.build(k, genome_len_hint=hint).score(8, prob)
        again = b.build_plan()
        assert again == dict(plan, distinct_attempts=1, graph_attempts=0, blocks=again["blocks"]), (case, plan, again)
        assert _launches(ctx) == _launches_of_one_attempt(again), case
        assert _snapshot(b) == first, case
    finally:
        if b is not None:
            b.close()           # (a batch must go before its context)
        ctx.profile(False)
        ctx.close()


def test_build_plan_rows_per_block_and_state():
    """one plan row that covers every segment of the batch; asking before the first build is a state error"""
    inp = _fixed(11, 1500, 50, 15, 190)
    b = _batch(inp, None)
    with pytest.raises(ga.GasmError, match="GASM_ERR_STATE"):
        b.build_plan()
    b.build(21, genome_len_hint=1500)
    plan = b.build_plan()
    rows = plan["blocks"]
    assert len(rows) == 1 and rows[0]["segments"] == 11
    assert all(r["k"] == 21 and r["key_words"] == 1 and r["distinct_attempts"] == 1 for r in rows)
    segs = _segments(inp)
    for s in (0, 4, 10):
        ref = orc.get_contigs(orc.kmers_from_reads(segs[s], 21), 21, 1, rows=1)
        assert b.contigs(s) == ref["contigs"], s
    b.close()


# ------------------------------------------------------------------------------------------------ process-wide knobs
KNOB_SETS = [{"GASM_RANK_GLOBAL": "1"}, {"GASM_RULER_SHIFT": "1"}, {"GASM_RULER_SHIFT": "2"}, {"GASM_RULER_SHIFT": "3"},
             {"GASM_RULER_SHIFT": "4"}, {"GASM_DEDUP_TBL": "2048"}, {"GASM_DEDUP_TBL": "4096"},
             {"GASM_SCAN_IN_DEDUP": "0"}, {"GASM_SCATTER_WGS": "1", "GASM_HIST_WGS": "1"}]


@pytest.mark.timeout(1200)
def test_process_wide_knobs_in_child_processes():
    """The Knobs of pipeline.hip are read once per process: each set runs in a fresh child (one at a time), which builds a
    fixed set of small batches, checks them against the oracle and that the knob shows in the plan where it can.  The
    first child that fails, dies or times out ends the test."""
    child = os.path.join(ROOT, "tests", "build_paths_child.py")
    base = {n: v for n, v in os.environ.items() if not n.startswith("GASM_")}
    base["PYTHONPATH"] = ROOT + (os.pathsep + base["PYTHONPATH"] if base.get("PYTHONPATH") else "")
    for knobs in KNOB_SETS:
        try:
            r = subprocess.run([sys.executable, child], env=dict(base, **knobs), cwd=ROOT, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{knobs}: the child did not finish within 240 s")
        lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
        assert r.returncode == 0, f"{knobs}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
        verdict = json.loads(lines[-1])
        assert verdict["ok"] and verdict["knobs"] == knobs, verdict


# ------------------------------------------------------------------------------------------------ interleaved batches
def _interleaved(prob, A, B, C, ctx):
    """A, B, A, C, B (far too small hint), A (another k: another tile shape), fetch; A, C, B, fetch.  Steps queued without a
    fetch in between.  Returns the fetched snapshots and A's plans at both fetches."""
    ba, bb, bc = _batch(A, ctx), _batch(B, ctx), _batch(C, ctx)
    try:
        return _interleaved_steps(prob, ba, bb, bc)
    finally:
        for x in (ba, bb, bc):
            x.close()


def _interleaved_steps(prob, ba, bb, bc):
    ba.build(21, 2000).score(8, prob)
    bb.build(33, 12000).score(8, prob)
    ba.build(21, 2000).score(8, prob)
    bc.build(13, 0).score(8, prob)
    bb.build(33, 10).score(8, prob)
    ba.build(15, 2000).score(8, prob)
    mid = dict(A15=_snapshot(ba), B10=_snapshot(bb), C=_snapshot(bc))
    plans = dict(A15=ba.build_plan(), B10=bb.build_plan())
    ba.build(21, 2000).score(8, prob)
    bc.build(13, 0).score(8, prob)
    bb.build(33, 12000).score(8, prob)
    end = dict(A21=_snapshot(ba), C=_snapshot(bc), B=_snapshot(bb))
    plans.update(A21=ba.build_plan(), B=bb.build_plan())
    return mid, end, plans


def _alone(prob, inp, k, hint, ctx):
    b = _batch(inp, ctx)
    try:
        b.build(k, hint).score(8, prob)
        return _snapshot(b), b.build_plan()
    finally:
        b.close()


@pytest.mark.timeout(600)
def test_distinct_batches_interleaved_on_one_context(qtable, monkeypatch):
    """Three batches of different shapes on one Context, their steps queued alternately with no fetch in between: their step
    slots share the context's lane streams.  A: fixed length, k = 21 and then 15 (another tile shape); B: 70 segments, one
    of them large, k = 33 (128-bit keys), once with a far too small hint (the retry ladder runs while the others' steps are
    queued); C: ragged reads from strings.  Every fetch equals the same batch built alone without step slots, under the
    default slots and two slots, and the oracle on a sample.  (The tile tables of a batch are uploaded once per tile shape
    and shared by its slots: this exercises that pattern; it cannot force the race the upload once had.)"""
    keys, prob = qtable
    A = _fixed(6, 2000, 50, 15, 200)
    B = hc.ladder_input()                 # (_fixed_mixed([(800, 12)] * 35 + [(12000, 8)] + [(800, 12)] * 34, 60, 210))
    rng = np.random.default_rng(11)
    g = _strs(synth.make_segment(220, 2500, planted=False)[None, :])[0]
    C = dict(strings=[[g[a:a + int(rng.integers(20, 70))] for a in rng.integers(0, 2430, 300)], [], [g[:40], g[10:35]]])
    monkeypatch.setenv("GASM_PINGPONG", "0")
    ctx = ga.Context(0)
    try:
        _interleaved_against_alone(prob, keys, A, B, C, ctx, monkeypatch)
    finally:
        ctx.close()


def _interleaved_against_alone(prob, keys, A, B, C, ctx, monkeypatch):
    ref, ref_plan = {}, {}
    for name, inp, k, hint in (("A21", A, 21, 2000), ("A15", A, 15, 2000), ("B", B, 33, 12000), ("B10", B, 33, 10), ("C", C, 13, 0)):
        ref[name], ref_plan[name] = _alone(prob, inp, k, hint, ctx)
    # the k change on A changes the tile shape, the small hint on B runs the ladder
    assert (ref_plan["A21"]["tile_g"], ref_plan["A15"]["tile_g"]) == (2, 4)
    assert ref_plan["B10"]["distinct_attempts"] == 2 and ref_plan["B"]["distinct_attempts"] == 1
    for inp, k, hint, sample in ((A, 21, 2000, [0, 5]), (A, 15, 2000, [3]), (B, 33, 10, [0, 35, 69]), (C, 13, 0, [0, 1, 2])):
        b = _batch(inp, ctx)
        try:
            b.build(k, hint).score(8, prob)
            _check_oracle_and_exact(b, _segments(inp), k, sample, keys, prob, (k, hint))
        finally:
            b.close()
    for env in ({}, {"GASM_PINGPONG": "1", "GASM_STEP_SLOTS": "2"}):
        monkeypatch.delenv("GASM_PINGPONG", raising=False)
        monkeypatch.delenv("GASM_STEP_SLOTS", raising=False)
        for n, v in env.items():
            monkeypatch.setenv(n, v)
        mid, end, plans = _interleaved(prob, A, B, C, ctx)
        for name, snap in list(mid.items()) + list(end.items()):
            hc.assert_same(snap, ref[name], (env, name))            # (equal, or: which of the twelve fields differs first, in which segment)
        assert (plans["A15"]["tile_g"], plans["A21"]["tile_g"]) == (4, 2), env
        assert plans["B10"]["distinct_attempts"] == 2 and plans["B10"]["bucket_bits"] == ref_plan["B10"]["bucket_bits"], env
