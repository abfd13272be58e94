"""Low-coverage removal and per-contig coverage on the device (gasm_batch_build_params, SegmentBatch.build_simplified(),
contig_coverage()) against the CPU restatement of the rule in tests/lowcov_ref.py, per segment:
    distinct k-mers, multiplicities, contigs, kmer_breaks, sequence_len, the twin map, tip_stats, bubble_stats, lowcov_stats,
    solid_stats and the per-contig (m, n) bit for bit, scores within 1e-9, fixed-point sums exactly.
Noisy inputs: bubbles_ref.noisy_segments (several segments per batch, so that segment boundaries are crossed).  References are
computed once per process (lowcov_ref.expected_cached)."""
import ctypes as C

import numpy as np
import pytest

import bubbles_ref as br
import build_entries as be
import genomeassembler_dev_amd as ga
import lowcov_ref as lr
import tips_ref as tr
from genomeassembler_dev_amd._lib import BuildParams, check, default_context, lib
from oracle import exact_scores as xs
from oracle import orc

pytestmark = pytest.mark.gpu
TOL = 1e-9
R = lr.MAX_COV_ROUNDS
INVALID, STATE = -1, -7


def check_segments(b, segs, k, c, strands, tip, bub, cov, keys, prob, scored=True):
    """every segment of a built (and scored) batch against the restatement; tip = (tip_len, tip_rounds), bub = (bubble_len,
    bubble_rounds), cov = (cov_cutoff, cov_len, cov_rounds).  Returns the restatement's results per segment"""
    (tip_len, tip_rounds), (bubble_len, bubble_rounds), (cc, cl, cr) = tip, bub, cov
    on = cc > 0 and cl > 0
    contigs = b.contigs()
    assert b.strands() == strands
    assert (int(lib().gasm_batch_tip_len(b.h)), int(lib().gasm_batch_bubble_len(b.h))) == (tip_len, bubble_len)
    assert (int(lib().gasm_batch_cov_cutoff(b.h)), int(lib().gasm_batch_cov_len(b.h)), int(lib().gasm_batch_cov_rounds(b.h))) == (cc, cl, cr if on else 0)
    twins = b.contig_twins() if strands == 2 else None            # (GASM_ERR_INTERNAL here: the removal broke the twin closure)
    zeros = (np.zeros((len(segs), R), np.uint32),) * 2
    tips, tkmers = b.tip_stats() if tip_len else zeros
    bubbles, bkmers = b.bubble_stats() if bubble_len else zeros
    low, lkmers = b.lowcov_stats() if on else zeros
    before, after = b.solid_stats()
    cm, cn = b.contig_coverage()
    sc = b.scores() if scored else None
    so = b.contigs_raw()[0]
    fixed = scored and all(len(r) >= k for rs in segs for r in rs) and any(len(rs) for rs in segs)
    out = {}
    for s, rs in enumerate(segs):
        e = out[s] = lr.expected_cached(rs, k, c, strands, tip_len, tip_rounds, bubble_len, bubble_rounds, cc, cl, cr)
        ref = e["ref"]
        print(f"segment {s}: k {k} min_count {c} strands {strands} tips {tip} bubbles {bub} lowcov {cov}: restatement removes {e['lowcov']} / "
              f"{e['lowcov_kmers']}; device {low[s].tolist()} / {lkmers[s].tolist()}; contigs {len(ref['contigs'])} / {len(contigs[s])}")
        assert tips[s].tolist() == e["tips"] and tkmers[s].tolist() == e["kmers"], (s, "tip_stats")
        assert bubbles[s].tolist() == e["bubbles"] and bkmers[s].tolist() == e["bubble_kmers"], (s, "bubble_stats")
        assert low[s].tolist() == e["lowcov"] and lkmers[s].tolist() == e["lowcov_kmers"], (s, "lowcov_stats")
        assert contigs[s] == ref["contigs"], (s, "contigs")
        dk, dm = b.distinct_kmers(s)
        assert dk == ref["distinct"] and dm.tolist() == ref["counts"].tolist(), (s, "k-mer counts")
        assert (int(before[s]), int(after[s])) == (len(e["cnt"]), e["solid"]), (s, "solid_stats keep meaning the cutoff")
        assert len(dk) == e["solid"] - sum(e["kmers"]) - sum(e["bubble_kmers"]) - sum(e["lowcov_kmers"]), s
        a, z = int(so[s]), int(so[s + 1])
        assert list(zip(cm[a:z].tolist(), cn[a:z].tolist())) == e["coverage"], (s, "contig_coverage")
        sm, sn = b.contig_coverage(s)
        assert sm.tolist() == cm[a:z].tolist() and sn.tolist() == cn[a:z].tolist(), s
        if strands == 2:
            at = {x: i for i, x in enumerate(ref["contigs"])}
            assert twins[s].tolist() == [at[tr.rc(x)] for x in ref["contigs"]], (s, "twin map")
        if not scored:
            continue
        assert z - a == len(ref["contigs"]), s
        o = orc.calc_breakscore(ref["contigs"], rs, "", 8, keys, prob, with_lev=False, with_freq=False)
        assert sc["kmer_breaks"][a:z].tolist() == o["kmer_breaks"].tolist(), (s, "kmer_breaks")
        assert sc["sequence_len"][a:z].tolist() == o["sequence_len"].tolist(), (s, "sequence_len")
        for name in ("bp_score", "bp_score_norm_by_break_freqs", "bp_score_norm_by_len"):
            x, y = sc[name][a:z], o[name]
            assert np.array_equal(np.isnan(x), np.isnan(y)), (s, name)
            ok = ~np.isnan(x)
            assert np.abs(x[ok] - y[ok]).max(initial=0.0) < TOL, (s, name)
        if fixed:
            fx, shift = b.score_fixed()
            table = dict(zip(keys, np.asarray(prob, dtype=np.float64).tolist()))
            for i, ex in enumerate(xs.score_paths(ref["contigs"], rs, table, 8)):
                assert int(fx[a + i]) == ex.fixed_sum(shift), (s, i, "fixed-point sum")
    return out


# L, read length, coverage, k, seed, min_count, strands, cov_len, cov_cutoff: contigs and k-mers removed in round 0 of segment 0,
# contigs before -> after (the small rows of tests/test_lowcov_host.py's table; the k = 41 row is the 128-bit-key case)
ROWS = [(4000, 80, 20, 21, 5, 2, 1, 41, 3, 3, 21, 4, 1), (4000, 80, 20, 21, 5, 2, 2, 41, 3, 6, 42, 8, 2), (4000, 80, 40, 21, 5, 2, 1, 41, 3, 14, 147, 23, 1),
        (600, 50, 12, 15, 3, 1, 1, 29, 2, 16, 230, 55, 11), (400, 40, 15, 11, 9, 1, 1, 21, 2, 21, 228, 63, 5),
        (2000, 100, 30, 41, 5, 2, 2, 81, 3, 6, 60, 8, 2),
        # the key-width seams: all 62 bits of a 64-bit key, the first 128-bit key (its high word is 0) and 126 bits (both-strand rows on
        # half the genome: three segments of 3 kb took 15 s of the oracle's scoring)
        (3000, 100, 20, 31, 5, 1, 1, 61, 2, 142, 4245, 547, 160), (1500, 100, 20, 32, 5, 1, 2, 63, 2, 142, 4350, 546, 146),
        (3000, 150, 24, 63, 5, 1, 1, 125, 2, 49, 2567, 250, 128), (1500, 150, 24, 63, 5, 1, 2, 125, 2, 54, 2484, 256, 144)]


@pytest.mark.parametrize("L,rl,cov,k,seed,c,strands,cl,cc,n_rm,n_kmers,n_before,n_after", ROWS)
def test_noisy_reads(qtable, L, rl, cov, k, seed, c, strands, cl, cc, n_rm, n_kmers, n_before, n_after):
    """three segments per batch, the first the table's row: the restatement reproduces the row, the device the restatement"""
    keys, prob = qtable
    segs = br.noisy_segments(L, rl, cov, seed, strands)[2] + br.noisy_segments(L, rl, cov, seed + 100, strands, n_seg=2)[2]
    tl = 2 * k - 1
    e = lr.expected_cached(segs[0], k, c, strands, tl, 2, tl, 2, cc, cl, 2)
    assert (e["lowcov"][:2], e["lowcov_kmers"][:2], len(e["after_bubbles"]), len(e["ref"]["contigs"])) == ([n_rm, 0], [n_kmers, 0], n_before, n_after)
    b = ga.SegmentBatch.from_strings(segs)
    b.build_simplified(k, min_count=c, strands=strands, tip_len=tl, tip_rounds=2, bubble_len=tl, bubble_rounds=2, cov_cutoff=cc, cov_len=cl,
                       cov_rounds=2).score(8, prob)
    refs = check_segments(b, segs, k, c, strands, (tl, 2), (tl, 2), (cc, cl, 2), keys, prob)
    assert b.lowcov_stats()[0][0, 0] == n_rm >= 1 and b.contigs()[0] != e["after_bubbles"]
    h = b.kmer_spectrum()                                            # of what is left
    for s in range(3):
        counts = np.asarray(refs[s]["ref"]["counts"], dtype=np.int64)
        assert h[s].tolist() == np.bincount(np.minimum(counts, 255), minlength=256).tolist()
    # Velvet's automatic cutoff from the device's own coverage: host arithmetic, at least min_count + 1
    assert b.suggest_cov_cutoff(0) == max(c + 1, lr.weighted_median_half(refs[0]["coverage"]))
    # the low-coverage rounds alone, one round, no tips or bubbles in front
    b.build_simplified(k, min_count=c, strands=strands, cov_cutoff=cc, cov_len=cl).score(8, prob)
    check_segments(b, segs, k, c, strands, (0, 0), (0, 0), (cc, cl, 1), keys, prob)
    b.close()


def test_hand_built_cases(qtable):
    """island (goes below the cutoff, stays at it), link (goes, both backbones heal), the link one base longer than cov_len (stays);
    all in one batch with an empty segment between them"""
    keys, prob = qtable
    island, G, isl = lr.island_case()
    link, G1, G2, X = lr.link_case()
    longer, H1, H2, Y = lr.link_case(extra=1)
    segs = [island, link, [], longer]
    b = ga.SegmentBatch.from_strings(segs)
    b.build_simplified(21, cov_cutoff=3, cov_len=41, cov_rounds=2).score(8, prob)
    check_segments(b, segs, 21, 1, 1, (0, 0), (0, 0), (3, 41, 2), keys, prob)
    low, kmers = b.lowcov_stats()
    assert low.tolist() == [[1, 0] + [0] * 6, [1, 0] + [0] * 6, [0] * 8, [0] * 8] and kmers[:, 0].tolist() == [21, 21, 0, 0]
    assert b.contigs() == [[G], sorted([G1, G2]), [], sorted(lr.expected_cached(longer, 21)["ref"]["contigs"])] and Y in b.contigs()[3]
    b.build_simplified(21, cov_cutoff=2, cov_len=41).score(8, prob)                  # the island's mean is exactly 2: it stays
    check_segments(b, segs, 21, 1, 1, (0, 0), (0, 0), (2, 41, 1), keys, prob)
    assert b.lowcov_stats()[0][:, 0].tolist() == [0, 1, 0, 0] and b.contigs()[0] == sorted([G, isl])
    b.close()


def test_contig_coverage(qtable):
    """a plain build, a fully simplified one, a segment with no k-mers, and GASM_ERR_STATE before a build or a coverage pass"""
    keys, prob = qtable
    _, _, nz = br.noisy_segments(4000, 80, 20, 5, 2, n_seg=2)
    _, _, clean = br.noisy_segments(3000, 80, 30, 77, 2, rate=0)    # (at 12x a thin true stretch sits at the cutoff and goes: the stated limit)
    segs = [nz[0], [], clean[0], ["ACGTACGTAC", "ACGTTGCA"], nz[1]]
    b = ga.SegmentBatch.from_strings(segs)
    m, n = C.c_void_p(), C.c_void_p()
    assert lib().gasm_batch_contig_coverage(b.h) == STATE
    assert lib().gasm_batch_fetch_contig_coverage(b.h, C.byref(m), C.byref(n)) == STATE
    b.build(21)
    assert lib().gasm_batch_fetch_contig_coverage(b.h, C.byref(m), C.byref(n)) == STATE           # no coverage pass over this build
    check_segments(b, segs, 21, 1, 1, (0, 0), (0, 0), (0, 0, 0), keys, prob, scored=False)
    snap = (b.contigs(), b.distinct()[1].tobytes())
    b.build_simplified(21, min_count=2, strands=2, tip_len=41, tip_rounds=2, bubble_len=41, bubble_rounds=2, cov_cutoff=3, cov_len=41).score(8, prob)
    assert lib().gasm_batch_fetch_contig_coverage(b.h, C.byref(m), C.byref(n)) == STATE           # ... nor over this one yet
    refs = check_segments(b, segs, 21, 2, 2, (41, 2), (41, 2), (3, 41, 1), keys, prob)
    assert refs[0]["lowcov"][0] >= 1 and refs[4]["lowcov"][0] >= 1 and refs[2]["lowcov"] == [0] * 8
    assert len(b.contig_coverage(1)[0]) == len(b.contig_coverage(3)[0]) == 0
    ms, ns = b.contig_coverage()
    assert ms.dtype == np.uint64 and ns.dtype == np.uint32 and int(ns.sum()) == len(b.distinct()[1])   # (no isolated cycles in these inputs)
    b.build(21)                                                                                   # the coverage pass changed nothing
    assert (b.contigs(), b.distinct()[1].tobytes()) == snap
    b.close()
    b = ga.SegmentBatch.from_strings([[], []])                                                    # nothing at all
    b.build_simplified(21, cov_cutoff=3, cov_len=41)
    assert b.contigs() == [[], []] and b.lowcov_stats()[0].tolist() == [[0] * R] * 2 and len(b.contig_coverage()[0]) == 0
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
    bs = tuple(t.tobytes() for t in b.bubble_stats()) if lib().gasm_batch_bubble_len(b.h) else ()
    ls = tuple(t.tobytes() for t in b.lowcov_stats()) if lib().gasm_batch_cov_rounds(b.h) else ()
    cv = tuple(t.tobytes() for t in b.contig_coverage())
    return (seg.tobytes(), keys.tobytes(), mult.tobytes(), w, so.tobytes(), off.tobytes(), raw, fl.tobytes(), nx.tobytes(), fx.tobytes(), shift,
            before.tobytes(), after.tobytes(), b.total_kmers(), tw, ts, bs, ls, cv,
            *(sc[n].tobytes() for n in ("bp_score", "bp_score_norm_by_break_freqs", "bp_score_norm_by_len", "kmer_breaks", "sequence_len")))


@pytest.mark.parametrize("c,strands,tl,bl", [(1, 1, 0, 0), (2, 2, 41, 41)])
def test_cov_cutoff_0_is_todays_build(qtable, monkeypatch, c, strands, tl, bl):
    """gasm_batch_build_params with cov_cutoff = 0 (or cov_len = 0) == gasm_batch_build_bubbles in every fetch, in the plan and in every
    launch; build_simplified() with the feature off likewise"""
    keys, prob = qtable
    monkeypatch.setenv("GASM_PINGPONG", "0")        # every launch on the batch's own context, where the profiler counts
    reads, seg_off, segs = br.noisy_segments(4000, 80, 20, 77, strands, n_seg=2)
    ctx = ga.Context(0)
    try:
        ctx.profile(True)
        b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80, ctx=ctx)
        b.build_bubbles(21, min_count=c, strands=strands, tip_len=tl, tip_rounds=2, bubble_len=bl, bubble_rounds=2).score(8, prob)
        b.scores()                                     # (the batch's shape is known from here on: every build below plans alike)
        old = _profile_of(ctx, b, prob, lambda: check(lib().gasm_batch_build_bubbles(b.h, 21, 0, c, strands, tl, 2, bl, 2)))
        snap, plan = _all_fetches(b), b.build_plan()
        for cutoff, length in ((0, 41), (3, 0)):                      # cov_rounds is not read
            p = BuildParams.make(21, min_count=c, strands=strands, tip_len=tl, tip_rounds=2, bubble_len=bl, bubble_rounds=2, cov_cutoff=cutoff,
                                 cov_len=length, cov_rounds=77)
            new = _profile_of(ctx, b, prob, lambda: check(lib().gasm_batch_build_params(b.h, C.byref(p))))
            assert _all_fetches(b) == snap and b.build_plan() == plan
            assert new == old and "k_lowcov_mark" not in new, (new, old)
            assert lib().gasm_batch_cov_rounds(b.h) == 0
            q = C.c_void_p()
            assert lib().gasm_batch_fetch_lowcov_stats(b.h, C.byref(q), C.byref(q)) == STATE
        new = _profile_of(ctx, b, prob, lambda: b.build_simplified(21, min_count=c, strands=strands, tip_len=tl, tip_rounds=2, bubble_len=bl, bubble_rounds=2))
        assert _all_fetches(b) == snap and new == old
        on = _profile_of(ctx, b, prob, lambda: b.build_simplified(21, min_count=c, strands=strands, tip_len=41, tip_rounds=2, bubble_len=41,
                                                                  bubble_rounds=2, cov_cutoff=3, cov_len=41, cov_rounds=2))
        assert (on["k_tip_mark"], on["k_bubble_mark"], on["k_lowcov_mark"], on["k_bucket_gather"], on["k_contig_scan"]) == (2, 2, 2, 7, 1), on
        check_segments(b, segs, 21, c, strands, (41, 2), (41, 2), (3, 41, 2), keys, prob)
        assert ctx.profile_read()["k_contig_cov"][1] >= 1
        b.close()
    finally:
        ctx.profile(False)


def test_struct_form_at_the_c_abi(qtable):
    keys, prob = qtable
    rs = ["ACGTTGCATGCC"]                          # (one unbranched path: its only contig is the read)
    b = ga.SegmentBatch.from_strings([rs])
    q = C.c_void_p()
    assert lib().gasm_batch_fetch_lowcov_stats(b.h, C.byref(q), C.byref(q)) == STATE              # before a build
    assert lib().gasm_batch_cov_cutoff(b.h) == lib().gasm_batch_cov_len(b.h) == lib().gasm_batch_cov_rounds(b.h) == 0
    assert lib().gasm_batch_build_params(b.h, None) == INVALID
    p = BuildParams.make(5)
    p.size -= 4
    assert lib().gasm_batch_build_params(b.h, C.byref(p)) == INVALID                              # a wrong size
    assert lib().gasm_batch_build_params(b.h, C.byref(BuildParams.make(5, cov_cutoff=2, cov_len=65536, cov_rounds=1))) == INVALID
    for rounds in (0, 9):
        assert lib().gasm_batch_build_params(b.h, C.byref(BuildParams.make(5, cov_cutoff=2, cov_len=9, cov_rounds=rounds))) == INVALID
    assert lib().gasm_batch_build_params(b.h, C.byref(BuildParams.make(5, strands=3))) == INVALID  # the other fields are still checked
    assert lib().gasm_batch_build_params(b.h, C.byref(BuildParams.make(5, tip_len=9, tip_rounds=9))) == INVALID
    assert lib().gasm_batch_build_params(b.h, C.byref(BuildParams.make(5, bubble_len=65536, bubble_rounds=1))) == INVALID
    assert lib().gasm_batch_build_params(b.h, C.byref(BuildParams.make(5, cov_cutoff=1, cov_len=65535, cov_rounds=8))) == 0
    assert b.lowcov_stats()[0].sum() == 0 and b.contigs() == [rs]                                 # cov_cutoff <= min_count: allowed, matches nothing
    assert (lib().gasm_batch_cov_cutoff(b.h), lib().gasm_batch_cov_len(b.h), lib().gasm_batch_cov_rounds(b.h)) == (1, 65535, 8)
    assert lib().gasm_batch_build_params(b.h, C.byref(BuildParams.make(5, cov_cutoff=2, cov_len=3, cov_rounds=1))) == 0
    assert b.lowcov_stats()[0].sum() == 0 and b.contigs() == [rs]                                 # cov_len < k: allowed, matches no contig
    assert lib().gasm_batch_build_params(b.h, C.byref(BuildParams.make(5, cov_cutoff=2, cov_len=12, cov_rounds=2))) == 0
    low, kmers = b.lowcov_stats()                                                                 # the only contig has mean 1 < 2: nothing is left
    assert (low[0].tolist(), kmers[0].tolist()) == ([1, 0] + [0] * 6, [8, 0] + [0] * 6) == (lr.expected(rs, 5, 1, 1, 0, 1, 0, 1, 2, 12, 2)["lowcov"],
                                                                                            lr.expected(rs, 5, 1, 1, 0, 1, 0, 1, 2, 12, 2)["lowcov_kmers"])
    assert b.contigs() == [[]] and len(b.contig_coverage()[0]) == 0 and b.solid_stats()[1].tolist() == [8]
    b.close()
    # zeroed optional fields are gasm_batch_build
    reads, seg_off, segs = br.noisy_segments(4000, 80, 20, 5, 1, n_seg=2)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
    b.build(21).score(8, prob)
    snap = _all_fetches(b)
    check(lib().gasm_batch_build_params(b.h, C.byref(BuildParams.make(21))))
    b.score(8, prob)
    assert _all_fetches(b) == snap and b.strands() == 1
    b.close()
    # a refused build leaves the build before it as it was, through every entry; the one-shot entries refuse the same values with the
    # same words
    texts = be.refused_builds_change_nothing()
    assert set(texts) == {what for what, *_ in be.REFUSED}
    ctx = default_context()
    assert be.refused_calls(lambda sfx, opts, size_off: be.contigs_from_reads(ctx, rs, sfx, 5, 1, 3, opts, size_off)[0], tuple(be.TAKES)) == texts


# the settings of test_every_entry_*: everything off; cutoff, both strands and tips; the same plus bubbles
SETTINGS = [dict(), dict(min_count=2, strands=2, tip_len=21, tip_rounds=2),
            dict(min_count=2, strands=2, tip_len=21, tip_rounds=2, bubble_len=21, bubble_rounds=2)]


@pytest.mark.parametrize("opts", SETTINGS, ids=["off", "tips", "tips+bubbles"])
def test_every_entry_builds_what_the_struct_entry_builds(qtable, monkeypatch, opts):
    """each positional gasm_batch_build* entry that can express the setting against gasm_batch_build_params: every fetch, the plan and
    the getters.  (The Python wrappers call the struct entry only: these raw calls are what covers the positional ones.)  Two segments
    of the smallest row of tests/test_lowcov_host.py's table, where tips, bubbles and low-coverage contigs all occur"""
    keys, prob = qtable
    monkeypatch.setenv("GASM_PINGPONG", "0")        # one slot: every build starts from the same BuildState, so the plans compare
    reads, seg_off, segs = br.noisy_segments(400, 40, 15, 9, 1, n_seg=2)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=40)
    b.k = 11

    def built(sfx):
        assert be.batch_build(b, sfx, 11, opts) == 0, sfx
        b.score(8, prob)
        return _all_fetches(b), b.build_plan(), be.getters(b)
    built("_params")                                 # (the batch's shape is known from here on: every build below plans alike)
    want = built("_params")
    assert want[2] == tuple(opts.get(name, 0 if name != "strands" else 1) for name in be.GETTERS)
    took = be.entries_for(opts)
    assert took[-1] == "_params" and len(took) == {0: 6, 4: 3, 6: 2}[len(opts)]
    for sfx in took[:-1]:
        assert built(sfx) == want, sfx
    if opts:                                         # the setting does something: what is compared is not trivially equal
        assert sum(int(t.sum()) for t in b.tip_stats()) > 0
    b.close()


@pytest.mark.parametrize("opts", SETTINGS, ids=["off", "tips", "tips+bubbles"])
def test_every_one_shot_entry_gives_what_the_struct_entry_gives(opts):
    """the same for gasm_get_contigs_from_reads* on one segment with matrix_rows = 3: contigs (and with them their offsets), perm, the
    distinct keys and their multiplicities"""
    rs = br.noisy_segments(400, 40, 15, 9, 1)[2][0]
    ctx = default_context()

    def got(sfx):
        st, m = be.contigs_from_reads(ctx, rs, sfx, 11, 7, 3, opts)
        assert st == 0, sfx
        return m.contigs, m.perm.shape, m.perm.tobytes(), m.words, m.distinct_keys.tobytes(), m.distinct_mult.tobytes()
    want = got("_params")
    assert want[1] == (3, len(want[0])) and len(want[0]) > 1
    for sfx in be.entries_for(opts)[:-1]:
        assert got(sfx) == want, sfx


@pytest.mark.parametrize("slots", [2, 3])
def test_step_slots(qtable, monkeypatch, slots):
    """build_simplified; score twice and more without a fetch, alternating settings: every fetch shows the last setting"""
    keys, prob = qtable
    monkeypatch.setenv("GASM_STEP_SLOTS", str(slots))
    reads, seg_off, segs = br.noisy_segments(4000, 80, 20, 5, 2, n_seg=2)
    # strands, tips, bubbles, (cov_cutoff, cov_len, cov_rounds)
    A, B, OFF = (2, 41, 41, (3, 41, 1)), (1, 0, 41, (4, 60, 2)), (2, 41, 41, (0, 0, 1))

    def step(b, st, tl, bl, cov):
        b.build_simplified(21, min_count=2, strands=st, tip_len=tl, tip_rounds=2, bubble_len=bl, bubble_rounds=2, cov_cutoff=cov[0], cov_len=cov[1],
                           cov_rounds=cov[2]).score(8, prob)

    alone = {}
    for s in (A, B, OFF):
        b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
        step(b, *s)
        alone[s] = _all_fetches(b)
        b.close()
    assert alone[A] != alone[B] != alone[OFF] != alone[A]
    order = [A, B, A, OFF, B, A]
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
    for upto in range(2, len(order) + 1):
        for s in order[:upto]:
            step(b, *s)
        assert _all_fetches(b) == alone[order[upto - 1]], (slots, upto)
    check_segments(b, segs, 21, 2, 2, (41, 2), (41, 2), (3, 41, 1), keys, prob)
    b.close()


@pytest.mark.parametrize("L,rl,cov,seed,k,c,strands,cc", [(4000, 80, 20, 5, 21, 2, 1, 3), (2000, 100, 30, 5, 41, 2, 2, 3), (400, 40, 15, 9, 11, 1, 1, 2)])
def test_string_entry(L, rl, cov, seed, k, c, strands, cc):
    """api.get_contigs_from_reads_simplified equals the batch result on one segment, and the restatement"""
    _, _, segs = br.noisy_segments(L, rl, cov, seed, strands)            # (rows of test_noisy_reads: their references are shared)
    rs = segs[0] + ["ACG", ""]
    tl = 2 * k - 1
    e = lr.expected_cached(segs[0], k, c, strands, tl, 2, tl, 2, cc, tl, 2)
    assert e["lowcov"][0] >= 1
    m = ga.get_contigs_from_reads_simplified(rs, k, 3, matrix_rows=5, min_count=c, strands=strands, tip_len=tl, tip_rounds=2, bubble_len=tl,
                                             bubble_rounds=2, cov_cutoff=cc, cov_len=tl, cov_rounds=2)
    b = ga.SegmentBatch.from_strings([rs])
    b.build_simplified(k, min_count=c, strands=strands, tip_len=tl, tip_rounds=2, bubble_len=tl, bubble_rounds=2, cov_cutoff=cc, cov_len=tl, cov_rounds=2)
    assert m.contigs == b.contigs()[0] == e["ref"]["contigs"], k
    assert m.distinct_kmers() == e["ref"]["distinct"] and np.asarray(m.distinct_mult).tolist() == e["ref"]["counts"].tolist(), k
    b.close()
    perm = np.asarray(m.perm)
    assert perm.shape == (5, len(m.contigs)) and all(sorted(row.tolist()) == list(range(len(m.contigs))) for row in perm), k
    m0 = ga.get_contigs_from_reads_simplified(rs, k, 3, matrix_rows=1, min_count=c, strands=strands, tip_len=tl, tip_rounds=2, bubble_len=tl,
                                              bubble_rounds=2, cov_cutoff=0, cov_len=tl, cov_rounds=99)
    assert m0.contigs == e["after_bubbles"], k
