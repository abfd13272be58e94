"""The last-workgroup hand-offs of the build where a stale read would show.

k_bucket_dedup, k_bucket_solid and k_contig_scan finish inside the workgroup whose relaxed agent-scope add came last: it reads one
word per workgroup (bucket_d; seg_ncontig and seg_cbases) with relaxed agent-scope loads, with no release fence and no acquire
(kernels_build.hip, above publish_u32 / count_in_last; DESIGN.md "The last-workgroup hand-offs").  Every such word lives in a buffer
the next build on the same step slot writes again, so a stale read is invisible wherever two builds leave the same words.  Here two
builds that leave different words in every segment alternate on the same buffers (tests/handoff_cases.py, preconditions:
tests/test_handoff_host.py), and every fetch is compared whole — distinct() segment offsets, keys and multiplicities, contigs_raw()
segment offsets, contig offsets and text — against the CPU oracle, never against another GPU run.  (The rounds case alone checks 8
of its 64 segments against the restatement and the others against the first fetch of the same build.)  A failure names the first field
and segment that differ and says whether what was found is the other build's word for that segment (stale), another segment's, or
neither.

The numbers of builds are fixed: nothing here loops until something fails.  Every test prints how many handed-over words its checked
builds read."""
import pytest

import genomeassembler_dev_amd as ga
import handoff_cases as hc
from correct_ref import readme_options

pytestmark = pytest.mark.gpu


def _env(monkeypatch, **env):
    for n in ("GASM_PINGPONG", "GASM_STEP_SLOTS"):
        monkeypatch.delenv(n, raising=False)
    for n, v in env.items():
        monkeypatch.setenv(n, v)


def _grid_batch(k, ctx):
    return ga.SegmentBatch.from_strings(hc.grid(k)["segs"], ctx=ctx)


def _ladder_batch(ctx):
    inp = hc.ladder()["inp"]
    return ga.SegmentBatch(inp["reads"].reshape(-1), inp["seg_off"], fixed_len=inp["rl"], ctx=ctx)


def _checked_grid_fetch(b, k, name, tag):
    """fetch the grid batch's last build (name: "X" or "Y") and compare all of it with the oracle; returns the words its last workgroups
    read.  The plan must say that the bucket offsets were scanned in the de-duplication: else the first hand-off is not under test"""
    snap = hc.grid(k)["snap"]
    other = "Y" if name == "X" else "X"
    hc.assert_same(hc.snapshot(b), snap[name], tag, {other: snap[other]})
    plan = b.build_plan()
    assert plan["scan_in_dedup"] == 1 and plan["segments"] == hc.GRID_SEGMENTS, (tag, plan)
    return hc.words_handed_over(plan, 1 if name == "Y" else 0)


@pytest.mark.parametrize("k", hc.GRID_KS)
def test_one_slot_alternating(monkeypatch, k):
    """one step slot, X, Y, X, Y, ... 32 builds, every one fetched and checked: every build reads its hand-off words from the buffers
    the other build filled"""
    _env(monkeypatch, GASM_PINGPONG="0")
    ctx = ga.Context(0)
    b = None
    try:
        b = _grid_batch(k, ctx)
        words = 0
        for i in range(32):
            name = "XY"[i % 2]
            b.build(k, **hc.GRID_BUILDS[name])
            words += _checked_grid_fetch(b, k, name, (k, i, name))
        assert b.build_plan()["bucket_bits"] == 0                    # (one bucket per segment: 2051 words per hand-off)
        print(f"test_one_slot_alternating[{k}]: 32 builds checked, {words} handed-over words read")
    finally:
        if b is not None:
            b.close()
        ctx.close()


@pytest.mark.parametrize("k", hc.GRID_KS)
def test_slots_under_load(monkeypatch, k):
    """the default three step slots, 16 rounds of three builds queued without a fetch (X, Y, X, then Y, X, Y, ...), the last one
    fetched and checked: its de-duplication runs beside the tails of the two before it, and a second batch on the same context (the
    ladder case's P, queued in front of every round) shares the context's lane streams.  Three slots taken in turn by two alternating
    builds: every slot holds the other build's words each time it is taken again — asserted from the order of the builds"""
    _env(monkeypatch)
    lad = hc.ladder()
    ctx = ga.Context(0)
    b = bp = None
    try:
        b, bp = _grid_batch(k, ctx), _ladder_batch(ctx)
        order, words = [], 0
        for r in range(16):
            bp.build(hc.LADDER_K, hc.LADDER_HINTS["P"])
            for _ in range(3):
                name = "XY"[len(order) % 2]
                order.append(name)
                b.build(k, **hc.GRID_BUILDS[name])
            words += _checked_grid_fetch(b, k, name, (k, r, name))
        # build i takes slot (i + 1) mod 3 (gasm_batch_build: the slots in turn): no slot sees the same build twice in a row
        assert len(order) == 48
        for slot in range(3):
            mine = [order[i] for i in range(48) if (i + 1) % 3 == slot]
            assert len(mine) == 16 and all(x != y for x, y in zip(mine, mine[1:])), (slot, mine)
        hc.assert_same(hc.snapshot(bp), lad["snap"], (k, "P beside the rounds"))
        print(f"test_slots_under_load[{k}]: 16 of 48 builds checked, {words} handed-over words read")
    finally:
        for x in (b, bp):
            if x is not None:
                x.close()
        ctx.close()


def test_rebuild_after_a_failed_attempt(monkeypatch):
    """the ladder case on two step slots, 12 builds, each fetched and compared with the oracle on all 70 segments.  Q's first attempt
    overflows its tables and leaves its words behind; the second attempt's last workgroups read theirs from the same buffers.

    The order is P, Q, Q, P, P, Q, Q, P, ...: a slot's BuildState keeps the plan that worked for as long as the same reads come with the
    same k and hint (plan_build), so under a strict P, Q, P, Q on two slots every Q after the first would land on the slot of the Q
    before it and build in one attempt.  In this order every slot alternates between P and Q, every Q starts from its too small hint
    and must report two attempts.  Q also runs as the very first build of a fresh batch, whose buffers never held a finished build"""
    _env(monkeypatch, GASM_PINGPONG="1", GASM_STEP_SLOTS="2")
    lad = hc.ladder()
    ctx = ga.Context(0)
    b = fresh = None
    try:
        b = _ladder_batch(ctx)
        order = [("P", "Q", "Q", "P")[i % 4] for i in range(12)]
        for slot in range(2):                                        # (build i takes slot (i + 1) mod 2)
            mine = [order[i] for i in range(12) if (i + 1) % 2 == slot]
            assert all(x != y for x, y in zip(mine, mine[1:])), (slot, mine)
        words = 0
        for i, name in enumerate(order):
            b.build(hc.LADDER_K, hc.LADDER_HINTS[name])
            hc.assert_same(hc.snapshot(b), lad["snap"], (i, name))
            plan = b.build_plan()
            assert plan["distinct_attempts"] == (2 if name == "Q" else 1) and plan["scan_in_dedup"] == 1, (i, name, plan)
            words += hc.words_handed_over(plan, 0)
        fresh = _ladder_batch(ctx)
        fresh.build(hc.LADDER_K, hc.LADDER_HINTS["Q"])
        hc.assert_same(hc.snapshot(fresh), lad["snap"], "Q first on a fresh batch")
        plan = fresh.build_plan()
        assert plan["distinct_attempts"] == 2 and plan["scan_in_dedup"] == 1, plan
        words += hc.words_handed_over(plan, 0)
        print(f"test_rebuild_after_a_failed_attempt: 13 builds checked, {words} handed-over words read by their final attempts")
    finally:
        for x in (b, fresh):
            if x is not None:
                x.close()
        ctx.close()


def test_rounds_alternating(monkeypatch):
    """one step slot, Z (cutoff, two tip, two bubble and two low-coverage rounds: seven k_bucket_solid hand-offs, each over the words
    the round before wrote), X, Z, X, ... 8 builds, each fetched.  8 segments against the restatements the low-coverage tests share
    (Z) and the oracle (X); all 64 against the first fetch of the same build; every Z's round statistics against the first Z's"""
    _env(monkeypatch, GASM_PINGPONG="0")
    k = hc.ROUNDS_K
    reads, seg_off, segs = hc.rounds_input()
    opts = readme_options(k)
    ctx = ga.Context(0)
    b = None
    try:
        b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=reads.shape[1], ctx=ctx)
        first, first_stats, words = {}, None, 0
        for i in range(8):
            name, other = ("Z", "X") if i % 2 == 0 else ("X", "Z")
            if name == "Z":
                b.build_simplified(k, **opts)
            else:
                b.build(k)
            snap = hc.snapshot(b)
            for s in hc.ROUNDS_CHECKED:
                hc.assert_segment(snap, s, hc.rounds_expected(s, name)["ref"], k, (i, name), {other: hc.rounds_expected(s, other)["ref"]})
            if name in first:
                hc.assert_same(snap, first[name], (i, name, "against the first fetch of the same build"), {other: first.get(other, ())})
            first.setdefault(name, snap)
            if name == "Z":
                tips, bubbles, low = b.tip_stats(), b.bubble_stats(), b.lowcov_stats()
                for s in hc.ROUNDS_CHECKED:
                    e = hc.rounds_expected(s, "Z")
                    assert (tips[0][s].tolist(), tips[1][s].tolist()) == (e["tips"], e["kmers"]), (i, s, "tip_stats")
                    assert (bubbles[0][s].tolist(), bubbles[1][s].tolist()) == (e["bubbles"], e["bubble_kmers"]), (i, s, "bubble_stats")
                    assert (low[0][s].tolist(), low[1][s].tolist()) == (e["lowcov"], e["lowcov_kmers"]), (i, s, "lowcov_stats")
                stats = tuple(t.tobytes() for pair in (tips, bubbles, low) for t in pair)
                first_stats = stats if first_stats is None else first_stats
                assert stats == first_stats, (i, "round statistics differ from the first Z's")
            plan = b.build_plan()
            assert plan["scan_in_dedup"] == 1 and plan["segments"] == hc.ROUNDS_SEGMENTS, (i, plan)
            words += hc.words_handed_over(plan, 7 if name == "Z" else 0)
        assert first["Z"] != first["X"]
        print(f"test_rounds_alternating: 8 builds checked, {words} handed-over words read")
    finally:
        if b is not None:
            b.close()
        ctx.close()
