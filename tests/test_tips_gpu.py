"""Tip clipping on the device (gasm_batch_build_tips, SegmentBatch.build_tips(tip_len=, tip_rounds=)) against the CPU restatement of
the rule in tests/tips_ref.py, per segment:
    distinct k-mers, multiplicities, contigs, kmer_breaks, sequence_len, the twin map and tip_stats bit for bit,
    scores within 1e-9, fixed-point sums exactly where the batch was scored in fixed point.
Noisy inputs: synth.make_batch(1, L, rl, cov, seed0=seed), noisy(reads, 0.01, seed + 1) and, for strands = 2,
flip_half(reads, seed)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import build_entries as be
import genomeassembler_dev_amd as ga
import tips_ref as tr
from genomeassembler_dev_amd import synth
from genomeassembler_dev_amd._lib import check, lib
from oracle import exact_scores as xs
from oracle import orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
R = tr.MAX_TIP_ROUNDS


def noisy_batch(L, rl, cov, seed, strands, n_seg=1, rate=0.01):
    reads, seg_off, _ = synth.make_batch(n_seg, L, rl, cov, seed0=seed)
    if rate:
        reads = tr.noisy(reads, rate, seed + 1)
    if strands == 2:
        reads = tr.flip_half(reads, seed)
    return reads, seg_off, [tr.strs(reads[int(seg_off[s]):int(seg_off[s + 1])]) for s in range(n_seg)]


def check_segments(b, segs, k, c, strands, tip_len, tip_rounds, keys, prob, sample=None, tables=None, scored=True):
    """every sampled segment of a built (and scored) batch against the restatement; returns its results per segment"""
    contigs = b.contigs()
    tables = [prob] if tables is None else tables
    fixed = scored and all(len(r) >= k for rs in segs for r in rs) and any(len(rs) for rs in segs)
    assert b.strands() == strands
    assert (int(lib().gasm_batch_tip_len(b.h)), int(lib().gasm_batch_tip_rounds(b.h))) == (tip_len, tip_rounds if tip_len else 0)
    twins = b.contig_twins() if strands == 2 else None            # (GASM_ERR_INTERNAL here: the clipping broke the twin closure)
    tips, kmers = b.tip_stats() if tip_len else (np.zeros((len(segs), R), np.uint32),) * 2
    before, after = b.solid_stats()
    out = {}
    for s in (range(len(segs)) if sample is None else sample):
        rs = segs[s]
        e = tr.expected(rs, k, c, strands, tip_len, tip_rounds)
        ref = out[s] = e["ref"]
        print(f"segment {s}: k {k} min_count {c} strands {strands} tip_len {tip_len} x {tip_rounds}: restatement clips {e['tips']} tips, "
              f"{e['kmers']} k-mers; device {tips[s].tolist()}, {kmers[s].tolist()}; contigs {len(ref['contigs'])} / {len(contigs[s])}")
        assert tips[s].tolist() == e["tips"] and kmers[s].tolist() == e["kmers"], (s, "tip_stats")
        assert contigs[s] == ref["contigs"], (s, "contigs")
        dk, dm = b.distinct_kmers(s)
        assert dk == ref["distinct"] and dm.tolist() == ref["counts"].tolist(), (s, "k-mer counts")
        assert (int(before[s]), int(after[s])) == (len(e["cnt"]), e["solid"]), (s, "solid_stats keep meaning the cutoff")
        assert len(dk) == e["solid"] - sum(e["kmers"]), s
        if strands == 2:
            at = {x: i for i, x in enumerate(ref["contigs"])}
            assert twins[s].tolist() == [at[tr.rc(x)] for x in ref["contigs"]], (s, "twin map")
        if not scored:
            continue
        for t, pr in enumerate(tables):
            sc = b.scores(table=t)
            a, z = int(sc["seg_contig_off"][s]), int(sc["seg_contig_off"][s + 1])
            assert z - a == len(ref["contigs"]), (s, t)
            o = orc.calc_breakscore(ref["contigs"], rs, "", 8, keys, pr, with_lev=False, with_freq=False)
            assert sc["kmer_breaks"][a:z].tolist() == o["kmer_breaks"].tolist(), (s, t, "kmer_breaks")
            assert sc["sequence_len"][a:z].tolist() == o["sequence_len"].tolist(), (s, t, "sequence_len")
            for name in ("bp_score", "bp_score_norm_by_break_freqs", "bp_score_norm_by_len"):
                x, y = sc[name][a:z], o[name]
                assert np.array_equal(np.isnan(x), np.isnan(y)), (s, t, name)
                ok = ~np.isnan(x)
                assert np.abs(x[ok] - y[ok]).max(initial=0.0) < TOL, (s, t, name)
            if fixed:
                fx, shift = b.score_fixed(table=t)
                table = dict(zip(keys, np.asarray(pr, dtype=np.float64).tolist()))
                for i, ex in enumerate(xs.score_paths(ref["contigs"], rs, table, 8)):
                    assert int(fx[a + i]) == ex.fixed_sum(shift), (s, t, i, "fixed-point sum")
    return out


def _uniform(prob):
    u = np.zeros_like(prob)
    at = 0
    for n in (16, 256, 4096, 65536):
        u[at:at + n] = 1.0 / n
        at += n
    return u


# L, read length, coverage, k, seed, min_count, strands, contigs before, after, tips and k-mers of round 0 (tip_len = 2k - 1)
TABLE = [(4000, 80, 20, 21, 5, 1, 1, 1548, 1031, 286, 2945), (4000, 80, 20, 21, 5, 2, 1, 34, 16, 9, 78),
         (4000, 80, 20, 21, 5, 1, 2, 3096, 2062, 572, 5890), (4000, 80, 20, 21, 5, 2, 2, 68, 32, 18, 156),
         (6000, 100, 20, 41, 9, 2, 1, 45, 9, 18, 269), (6000, 100, 20, 41, 9, 2, 2, 90, 18, 36, 538),
         (3000, 60, 30, 8, 7, 2, 1, 822, 662, 91, 141), (4000, 80, 20, 20, 5, 2, 2, 72, 44, 14, 76),
         # the key-width seams: all 62 bits of a 64-bit key, the first 128-bit key (its high word is 0) and 126 bits (both-strand rows on
         # half the genome: the oracle's scoring of twice as many contigs took 15 s)
         (3000, 100, 20, 31, 5, 1, 1, 1022, 559, 246, 3570), (1500, 100, 20, 32, 5, 1, 2, 1022, 546, 260, 3942),
         (3000, 150, 24, 63, 5, 1, 1, 858, 253, 318, 10160), (1500, 150, 24, 63, 5, 1, 2, 878, 260, 324, 10032)]


@pytest.mark.parametrize("L,rl,cov,k,seed,c,strands,n_before,n_after,n_tips,n_kmers", TABLE)
def test_noisy_reads(qtable, L, rl, cov, k, seed, c, strands, n_before, n_after, n_tips, n_kmers):
    """the rows of the issue's table: the restatement reproduces them (which pins the rule), the device reproduces the restatement"""
    keys, prob = qtable
    reads, seg_off, segs = noisy_batch(L, rl, cov, seed, strands)
    e = tr.expected(segs[0], k, c, strands, 2 * k - 1, 2)
    plain = tr.expected(segs[0], k, c, strands)["ref"]["contigs"]
    assert e["tips"][0] >= 1 and e["ref"]["contigs"] != plain                  # not vacuous
    assert (len(plain), len(e["ref"]["contigs"]), e["tips"][:2], e["kmers"][:2]) == (n_before, n_after, [n_tips, 0], [n_kmers, 0])
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)
    for rounds in (1, 2):
        b.build_tips(k, min_count=c, strands=strands, tip_len=2 * k - 1, tip_rounds=rounds).score(8, prob)
        check_segments(b, segs, k, c, strands, 2 * k - 1, rounds, keys, prob)
    h = b.kmer_spectrum()                                            # of the clipped set
    counts = np.asarray(e["ref"]["counts"], dtype=np.int64)
    assert h[0].tolist() == np.bincount(np.minimum(counts, 255), minlength=256).tolist()
    b.close()


@pytest.mark.parametrize("strands", [1, 2])
def test_two_round_case(qtable, strands):
    """the hand-built case: S goes in round 0, the re-joined T in round 1; a third round finds nothing and changes nothing"""
    keys, prob = qtable
    reads, G = tr.two_round_case(strands)
    b = ga.SegmentBatch.from_strings([reads])
    got = {}
    for rounds in (1, 2, 3):
        b.build_tips(21, strands=strands, tip_len=41, tip_rounds=rounds).score(8, prob)
        check_segments(b, [reads], 21, 1, strands, 41, rounds, keys, prob)
        got[rounds] = (b.contigs(), b.distinct()[1].tobytes(), b.scores()["bp_score"].tobytes())
        tips, kmers = b.tip_stats()
        assert tips[0].tolist() == [strands, strands if rounds > 1 else 0] + [0] * 6
    assert got[3] == got[2] != got[1]
    assert got[2][0] == [sorted([G, tr.rc(G)] if strands == 2 else [G])]
    # equal multiplicities clip nobody
    reads, G = tr.two_round_case(strands, equal=True)
    b2 = ga.SegmentBatch.from_strings([reads])
    b2.build_tips(21, strands=strands, tip_len=41, tip_rounds=3).score(8, prob)
    check_segments(b2, [reads], 21, 1, strands, 41, 3, keys, prob)
    assert b2.tip_stats()[0][0].tolist() == [strands] + [0] * 7
    b.close(); b2.close()


@pytest.mark.parametrize("strands", [1, 2])
def test_batch_of_several_segments(qtable, strands):
    """noisy segments, a clean one (no tips: the unclipped build), an empty one and one whose reads are all shorter than k"""
    keys, prob = qtable
    _, _, nz = noisy_batch(4000, 80, 20, 31, strands, n_seg=2)
    _, _, clean = noisy_batch(3000, 80, 12, 77, strands, rate=0)
    segs = [nz[0], clean[0], [], nz[1], ["ACGTACGTAC", "ACGTTGCA"]]
    b = ga.SegmentBatch.from_strings(segs)
    b.build_tips(21, min_count=2, strands=strands, tip_len=41, tip_rounds=2).score(8, prob)
    refs = check_segments(b, segs, 21, 2, strands, 41, 2, keys, prob)
    tips, _ = b.tip_stats()
    assert tips[0, 0] > 0 and tips[3, 0] > 0 and tips[1].sum() == tips[2].sum() == tips[4].sum() == 0
    assert refs[1]["contigs"] == tr.expected(clean[0], 21, 2, strands)["ref"]["contigs"] and refs[2]["contigs"] == refs[4]["contigs"] == []
    b.close()
    b = ga.SegmentBatch.from_strings([[], []])                       # nothing at all
    b.build_tips(21, strands=strands, tip_len=41, tip_rounds=2)
    assert b.contigs() == [[], []] and b.tip_stats()[0].tolist() == [[0] * R] * 2
    b.close()


def test_variable_length_reads(qtable):
    """ragged reads, some shorter than k: the FP64 scorer"""
    keys, prob = qtable
    reads, seg_off, segs = noisy_batch(4000, 80, 20, 5, 1)
    rng = np.random.default_rng(8)
    rs = [r[:int(n)] for r, n in zip(segs[0], rng.integers(10, 81, len(segs[0])))] + ["", "ACG"]
    e = tr.expected(rs, 21, 2, 1, 41, 2)
    assert e["tips"][0] >= 1
    b = ga.SegmentBatch.from_strings([rs])
    b.build_tips(21, min_count=2, tip_len=41, tip_rounds=2).score(8, prob)
    with pytest.raises(ga.GasmError, match="GASM_ERR_STATE"):
        b.score_fixed()
    check_segments(b, [rs], 21, 2, 1, 41, 2, keys, prob)
    b.close()


@pytest.mark.parametrize("strands", [1, 2])
def test_score_tables(qtable, strands):
    keys, prob = qtable
    reads, seg_off, segs = noisy_batch(4000, 80, 20, 5, strands, n_seg=2)
    tabs = np.stack([prob, _uniform(prob)])
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
    b.build_tips(21, min_count=2, strands=strands, tip_len=41, tip_rounds=1).score_tables(8, tabs)
    check_segments(b, segs, 21, 2, strands, 41, 1, keys, prob, tables=list(tabs))
    b.close()


def test_guided_on_the_clipped_contigs(qtable):
    from oracle import guided_oracle
    keys, prob = qtable
    table = dict(zip(keys, prob.tolist()))
    reads, seg_off, segs = noisy_batch(6000, 100, 20, 9, 2, n_seg=2)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=100)
    b.build_tips(21, min_count=2, strands=2, tip_len=41, tip_rounds=2).score(8, prob)
    refs = check_segments(b, segs, 21, 2, 2, 41, 2, keys, prob)
    fx, shift = b.score_fixed()
    sc = b.scores()
    g = b.guided()
    for s, rs in enumerate(segs):
        a, e = int(sc["seg_contig_off"][s]), int(sc["seg_contig_off"][s + 1])
        ofx = guided_oracle.fixed_sums(refs[s]["contigs"], rs, table, 8, shift)
        assert ofx == fx[a:e].tolist(), s
        assert [d["sequence"] for d in g[s]] == guided_oracle.guided_paths(refs[s]["contigs"], ofx, 21), s
    b.close()


@pytest.mark.parametrize("k", [21, 33])
def test_hint_far_too_small(qtable, k):
    """the tables overflow, the build repeats itself with a larger configuration and clips again"""
    keys, prob = qtable
    reads, seg_off, segs = noisy_batch(8000, 60, 12, 120, 2, n_seg=2)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=60)
    b.build_tips(k, genome_len_hint=50, min_count=2, strands=2, tip_len=2 * k - 1, tip_rounds=2).score(8, prob)
    assert b.build_plan()["distinct_attempts"] > 1
    check_segments(b, segs, k, 2, 2, 2 * k - 1, 2, keys, prob)
    assert b.tip_stats()[0][:, 0].min() > 0
    b.close()


def test_a_segment_beyond_the_lds_ranking(qtable):
    """more than 65 534 edges in a segment: whole-GPU list ranking in every round; and a hint that promises a small segment,
    so that the LDS ranking gives up in a ROUND and the build starts over from the reads (graph_attempts > 0)"""
    keys, prob = qtable
    reads, seg_off, segs = noisy_batch(50000, 100, 20, 4242, 2)
    e = tr.expected(segs[0], 31, 2, 2, 61, 1)
    assert e["solid"] > 65534 and e["tips"][0] >= 1
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=100)
    b.build_tips(31, min_count=2, strands=2, tip_len=61, tip_rounds=2).score(8, prob)
    assert b.build_plan()["ranked_in_lds"] == 0
    check_segments(b, segs, 31, 2, 2, 61, 2, keys, prob)
    b.close()
    # The only cover of GASM_OVF_TIP_RANK and its restart from the reads.  It leans on the planner: a hint of 25 000 (doubled for
    # both strands) must size the buckets so that no table overflows, yet put the LDS ranking's room (the estimate and a quarter)
    # below this segment's ~100 000 edges, so that the ranking gives up in round 0.  A planner that sizes differently fails the
    # assertion on the plan below rather than passing without the path: pick another hint then
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=100)
    b.build_tips(31, genome_len_hint=25000, min_count=2, strands=2, tip_len=61, tip_rounds=2).score(8, prob)
    plan = b.build_plan()
    print("plan after a hint of 25000:", {n: v for n, v in plan.items() if n != "blocks"})
    assert plan["graph_attempts"] >= 1 and plan["rank_global"] == 1 and plan["ranked_in_lds"] == 0, plan
    check_segments(b, segs, 31, 2, 2, 61, 2, keys, prob)
    b.close()


def _profile_of(ctx, b, prob, build):
    ctx.profile_reset()
    build()
    b.score(8, prob)
    b.scores()
    return {n: v[1] for n, v in ctx.profile_read().items() if v[1]}


def _all_fetches(b):
    seg, keys, mult, w = b.distinct()
    so, off, raw = b.contigs_raw()
    fl, nx = b.graph()
    sc = b.scores()
    fx, shift = b.score_fixed()
    before, after = b.solid_stats()
    tw = tuple(t.tobytes() for t in b.contig_twins()) if b.strands() == 2 else ()
    ts = tuple(t.tobytes() for t in b.tip_stats()) if lib().gasm_batch_tip_len(b.h) else ()
    return (seg.tobytes(), keys.tobytes(), mult.tobytes(), w, so.tobytes(), off.tobytes(), raw, fl.tobytes(), nx.tobytes(), fx.tobytes(), shift,
            before.tobytes(), after.tobytes(), b.total_kmers(), tw, ts,
            *(sc[n].tobytes() for n in ("bp_score", "bp_score_norm_by_break_freqs", "bp_score_norm_by_len", "kmer_breaks", "sequence_len")))


@pytest.mark.parametrize("c,strands", [(1, 1), (2, 1), (2, 2)])
def test_tip_len_0_is_todays_build(qtable, monkeypatch, c, strands):
    """gasm_batch_build_tips(.., tip_len = 0, ..) == gasm_batch_build_strands in every fetch, in the plan and in every launch"""
    keys, prob = qtable
    monkeypatch.setenv("GASM_PINGPONG", "0")        # every launch on the batch's own context, where the profiler counts
    reads, seg_off, segs = noisy_batch(4000, 80, 20, 77, strands, n_seg=2)
    ctx = ga.Context(0)
    try:
        ctx.profile(True)
        b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80, ctx=ctx)
        b.build(21, min_count=c, strands=strands).score(8, prob)
        b.scores()                                     # (the batch's shape is known from here on: every build below plans alike)
        old = _profile_of(ctx, b, prob, lambda: check(lib().gasm_batch_build_strands(b.h, 21, 0, c, strands)))
        snap, plan = _all_fetches(b), b.build_plan()
        new = _profile_of(ctx, b, prob, lambda: check(lib().gasm_batch_build_tips(b.h, 21, 0, c, strands, 0, 77)))      # tip_rounds is not read
        assert _all_fetches(b) == snap and b.build_plan() == plan
        assert new == old and "k_tip_mark" not in new, (new, old)
        p = C.c_void_p()
        assert lib().gasm_batch_fetch_tip_stats(b.h, C.byref(p), C.byref(p)) == -7            # GASM_ERR_STATE after tip_len = 0
        tipped = _profile_of(ctx, b, prob, lambda: b.build_tips(21, min_count=c, strands=strands, tip_len=41, tip_rounds=2))
        assert tipped["k_tip_mark"] == 2 and tipped["k_bucket_gather"] == 3 and tipped["k_contig_scan"] == 1, tipped
        check_segments(b, segs, 21, c, strands, 41, 2, keys, prob)
        b.close()
    finally:
        ctx.profile(False)


def test_bad_arguments_at_the_c_abi():
    b = ga.SegmentBatch.from_strings([["ACGTACGTAC"]])
    p = C.c_void_p()
    assert lib().gasm_batch_fetch_tip_stats(b.h, C.byref(p), C.byref(p)) == -7                # GASM_ERR_STATE before a build
    assert lib().gasm_batch_tip_len(b.h) == 0 and lib().gasm_batch_tip_rounds(b.h) == 0
    for rounds in (0, 9):
        assert lib().gasm_batch_build_tips(b.h, 5, 0, 1, 1, 9, rounds) == -1                  # GASM_ERR_INVALID
    assert lib().gasm_batch_build_tips(b.h, 5, 0, 0, 1, 9, 1) == -1 and lib().gasm_batch_build_tips(b.h, 5, 0, 1, 3, 9, 1) == -1
    assert lib().gasm_batch_build_tips(b.h, 5, 0, 1, 1, 3, 8) == 0                            # tip_len < k: allowed, matches no contig
    assert b.tip_stats()[0].sum() == 0
    b.close()
    be.refused_builds_change_nothing(("_solid", "_strands", "_tips"))        # a refused build leaves the build before it as it was


@pytest.mark.parametrize("slots", [2, 3])
def test_step_slots(qtable, monkeypatch, slots):
    """build(tips); score; build(no tips); score; build(tips, other tip_len); score without a fetch in between: every fetch
    matches the last build, as if it had run alone"""
    keys, prob = qtable
    monkeypatch.setenv("GASM_STEP_SLOTS", str(slots))
    reads, seg_off, segs = noisy_batch(4000, 80, 20, 5, 2, n_seg=2)
    order = [(2, 2, 41, 2), (2, 2, 0, 1), (2, 1, 30, 1), (1, 2, 41, 1), (2, 2, 41, 2)]
    alone = {}
    for step in set(order):
        c, st, tl, tr_ = step
        b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
        b.build_tips(21, min_count=c, strands=st, tip_len=tl, tip_rounds=tr_).score(8, prob)
        alone[step] = _all_fetches(b)
        b.close()
    assert alone[order[0]] != alone[order[1]]
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
    for upto in range(1, len(order) + 1):
        for c, st, tl, tr_ in order[:upto]:
            b.build_tips(21, min_count=c, strands=st, tip_len=tl, tip_rounds=tr_).score(8, prob)
        assert _all_fetches(b) == alone[order[upto - 1]], (slots, upto)
    check_segments(b, segs, 21, 2, 2, 41, 2, keys, prob)
    b.close()


@pytest.mark.parametrize("env", ["GASM_RANK_GLOBAL=1", "GASM_PINGPONG=0", "GASM_SINGLE_PASS=0"])
def test_in_a_child_process(env):
    """whole-GPU ranking only, no step slots, the two-pass partition: knobs a process reads once (tests/tips_child.py).  The child
    also queues the steps of test_step_slots (and two whose first attempt fails) back to back without a fetch: with
    GASM_PINGPONG=0 that is one slot and one stream, every build abandoning the queued one before it"""
    name, value = env.split("=")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tips_child.py")], env=dict(os.environ, **{name: value}), capture_output=True, text=True,
                       timeout=600)
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert lines, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    v = json.loads(lines[-1])
    assert r.returncode == 0 and v["ok"], v
    if name == "GASM_RANK_GLOBAL":
        assert all(p["rank_global"] == 1 and p["ranked_in_lds"] == 0 for p in v["plans"].values()), v["plans"]
    if name == "GASM_SINGLE_PASS":
        assert all(p["single_pass"] == 0 for p in v["plans"].values()), v["plans"]


@pytest.mark.parametrize("k,strands", [(21, 1), (21, 2), (41, 2), (8, 1)])
def test_string_entry(k, strands):
    """api.get_contigs_from_reads(..., tip_len, tip_rounds) against the restatement; the shuffle matrix permutes the clipped contigs"""
    _, _, segs = noisy_batch(4000, 80, 20, 5, strands)
    rs = segs[0] + ["ACG", ""]
    for c in (1, 2):
        e = tr.expected(rs, k, c, strands, 2 * k - 1, 2)
        assert e["tips"][0] >= 1
        m = ga.get_contigs_from_reads(rs, k, 3, matrix_rows=5, min_count=c, strands=strands, tip_len=2 * k - 1, tip_rounds=2)
        assert m.contigs == e["ref"]["contigs"], (k, c)
        assert m.distinct_kmers() == e["ref"]["distinct"] and np.asarray(m.distinct_mult).tolist() == e["ref"]["counts"].tolist(), (k, c)
        perm = np.asarray(m.perm)
        assert perm.shape == (5, len(m.contigs)) and all(sorted(row.tolist()) == list(range(len(m.contigs))) for row in perm), (k, c)
        m0 = ga.get_contigs_from_reads(rs, k, 3, matrix_rows=1, min_count=c, strands=strands, tip_len=0, tip_rounds=99)
        assert m0.contigs == tr.expected(rs, k, c, strands)["ref"]["contigs"], (k, c)
