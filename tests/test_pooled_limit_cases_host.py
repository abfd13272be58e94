"""The cases of tests/pooled_limit_cases.py reach the limits they are built for, and tests/pooled_plan_ref.py restates the
exchange plans correctly: proved on the CPU alone (oracle + loops), no GPU.

tests/test_pooled_limits_gpu.py runs the plan kernels, the merge and the read repacking on these inputs and compares the plan
arrays with the restatement.  What makes an input take a second pass of the plan scan, fill the merge table exactly or cut a
read piece inside a word is a property of the input, so it is asserted here; the thresholds are the kernels' own constants
(8 192 entries per scan pass, the merge's LIMIT read off the sources, 32 bases per word), not measurements."""
import numpy as np
import pytest

import pooled_limit_cases as plc
import pooled_plan_ref as ref
from oracle import orc


def _distinct(reads, k):
    return orc.get_contigs(orc.kmers_from_reads(plc.strs(reads), k), k, 1, rows=1)["distinct"]


@pytest.mark.parametrize("case", plc.SCAN_CASES, ids=lambda c: c.name)
def test_scan_cases_take_the_carry(case):
    b = case.build()
    k, bbits, seg_off = b["k"], b["bbits"], b["seg_off"]
    n_seg = len(seg_off) - 1
    nbt = n_seg << bbits
    assert nbt > plc.SCAN_ENTRIES_ABOVE[case.name] and bbits <= 2 * (k - 1) and bbits <= 10
    n_reads = np.diff(seg_off.astype(np.int64))
    assert n_reads[1] == 0 and n_reads[2] == 1                       # a segment without reads, one with a single read
    # the merged table in bucket order (what a world of one scans in every block of both plans) ...
    G = plc.run_lengths(b["reads"], seg_off, k, bbits)
    s = 0
    want = _distinct(b["reads"][int(seg_off[s]):int(seg_off[s + 1])], k)
    assert int(G[:1 << bbits].sum()) == len(want)                    # (the string-set count is the oracle's)
    uneven_segments = False
    for world in b["worlds"]:
        own1 = ref.bucket_owner(n_seg, bbits, world)
        first = ref.segment_bounds(n_seg, world)
        if world > 1:
            cnt = np.bincount(own1, minlength=world)
            assert cnt.min() > 0 and cnt.min() != cnt.max(), (world, cnt)        # owners are uneven
            uneven_segments |= len(set(np.diff(first).tolist())) > 1
        order = np.argsort(own1, kind="stable")
        for r, (rr, so) in enumerate(b["deal"](world)):
            # ... and every rank's own table in the order its runs leave (sorted by owner): run lengths on both sides of every
            # pass boundary, so a lost carry moves records
            row = plc.run_lengths(rr, so, k, bbits)[order]
            for edge in range(plc.PASS_ENTRIES, nbt, plc.PASS_ENTRIES):
                assert row[:edge].sum() > 0 and row[edge:].sum() > 0, (world, r, edge)
                assert row[edge - 1024:edge].sum() > 0 and row[edge:edge + 1024].sum() > 0, (world, r, edge)
    for edge in range(plc.PASS_ENTRIES, nbt, plc.PASS_ENTRIES):
        assert G[:edge].sum() > 0 and G[edge:].sum() > 0
    assert uneven_segments or b["worlds"] == (1,)
    assert any(n_seg % w and nbt % w for w in b["worlds"])           # a world that divides neither count


@pytest.mark.parametrize("case", plc.LIMIT_CASES, ids=lambda c: c.name)
def test_limit_cases_fill_the_merge_table_exactly(case):
    b = case.build()
    k, limit = b["k"], b["limit"]
    assert limit == plc.merge_limit(1 if k <= 31 else 2) and limit in (2816, 1408)      # (today's values; the cases follow the sources)
    assert len(_distinct(b["reads"], k)) == b["union"] and b["union"] - limit == (1 if case.name.endswith("+1") else 0)
    local = [set(_distinct(rr, k)) for rr, _ in b["deal"](3)]
    assert all(0 < len(s) < limit // 2 for s in local), [len(s) for s in local]         # every local run far below the limit
    assert all(local[a] & local[c] and local[a] - local[c] for a in range(3) for c in range(3) if a != c)     # partial overlap
    assert len(set.union(*local)) == b["union"]


@pytest.mark.parametrize("case", plc.PIECE_CASES, ids=lambda c: c.name)
def test_piece_cases_cut_inside_words(case):
    b = case.build()
    rl = b["rl"]
    n_reads = np.diff(b["seg_off"].astype(np.int64))
    assert len(n_reads) == 5 and all((n * rl) % 32 for n in n_reads)
    for world in b["worlds"]:
        dealt = b["deal"](world)
        cnt = np.stack([np.diff(so.astype(np.int64)) for _, so in dealt])          # [rank, segment]
        assert cnt.sum(axis=0).tolist() == n_reads.tolist()
        starts = np.stack([so[:-1].astype(np.int64) * rl for _, so in dealt])
        assert ((cnt == 0).sum(axis=0) >= 1).all() and ((cnt == 1).sum(axis=0) >= 1).all()     # ranks with 0 / 1 read of every segment
        assert ((cnt > 0).sum(axis=0) >= 3).all()                                  # several pieces per owner and segment
        if rl < 32:
            assert ((cnt > 0) & (cnt * rl < 32)).any()                             # a piece shorter than one word
        assert ((cnt > 0) & (cnt * rl % 32 != 0) & (cnt * rl < 64)).any()          # a piece of one read: its last word is partial
        assert ((cnt > 0) & (starts % 32 != 0)).any()                              # pieces that start inside a word


# ------------------------------------------------------------------------------------------------ the plan restatement
def _brute_x1(lens_all, flags, own1, limit, W, r):
    nbt = lens_all.shape[1]
    mine = [gb for gb in range(nbt) if own1[gb] == r]
    run_off, run_len, recv_tot = np.zeros((len(mine), W), np.uint64), np.zeros((len(mine), W), np.uint32), np.zeros(W, np.uint64)
    bstart, cap = np.zeros(len(mine) + 1, np.uint64), 0
    for j, gb in enumerate(mine):
        tot = 0
        for s in range(W):
            run_off[j, s] = recv_tot[s]
            run_len[j, s] = lens_all[s, gb]
            recv_tot[s] += lens_all[s, gb]
            tot += int(lens_all[s, gb])
        bstart[j] = cap
        cap += min(tot, limit)
    bstart[len(mine)] = cap
    send_off, send_tot, run = np.zeros(nbt + 1, np.uint64), np.zeros(W, np.uint64), 0
    i = 0
    for d in range(W):
        for gb in range(nbt):
            if own1[gb] == d:
                send_off[i] = run
                run += int(lens_all[r, gb])
                send_tot[d] += lens_all[r, gb]
                i += 1
    send_off[nbt] = run
    f = 0
    for v in flags:
        f |= int(v)
    return dict(send_off=send_off, send_tot=send_tot, run_off=run_off, run_len=run_len, recv_tot=recv_tot, bstart=bstart,
                info=np.array([cap, 0], np.uint64), flags=f)


def _brute_x2(G, own1, first, bbits, W, r):
    nb = 1 << bbits
    lo, hi = int(first[r]) * nb, int(first[r + 1]) * nb
    run_off, run_len, recv_tot = np.zeros((hi - lo, W), np.uint64), np.zeros((hi - lo, W), np.uint32), np.zeros(W, np.uint64)
    bstart, tot, seg_max, seg_sum = np.zeros(hi - lo + 1, np.uint64), 0, 0, 0
    for i in range(hi - lo):
        for s in range(W):
            run_off[i, s] = recv_tot[s]
            if own1[lo + i] == s:
                run_len[i, s] = G[lo + i]
                recv_tot[s] += G[lo + i]
        bstart[i] = tot
        tot += int(G[lo + i])
        seg_sum = int(G[lo + i]) + (seg_sum if i % nb else 0)
        seg_max = max(seg_max, seg_sum)
    bstart[hi - lo] = tot
    mine = [gb for gb in range(len(G)) if own1[gb] == r]
    send_off, send_tot, run = np.zeros(len(mine) + 1, np.uint64), np.zeros(W, np.uint64), 0
    for j, gb in enumerate(mine):
        send_off[j] = run
        run += int(G[gb])
        seg = gb >> bbits
        d = [d for d in range(W) if first[d] <= seg < first[d + 1]][0]
        send_tot[d] += G[gb]
    send_off[len(mine)] = run
    return dict(send_off=send_off, send_tot=send_tot, run_off=run_off, run_len=run_len, recv_tot=recv_tot, bstart=bstart,
                info=np.array([tot, seg_max], np.uint64), flags=0)


@pytest.mark.parametrize("n_entries", [1, 8191, 8192, 8193, 20000])
def test_plan_restatement_against_a_loop_per_bucket(n_entries):
    rng = np.random.default_rng(4000 + n_entries)
    for W, bbits in ((1, 0), (3, 0), (4, 2 if n_entries % 4 == 0 else 0)):
        n_seg = n_entries >> bbits
        own1 = ref.bucket_owner(n_seg, bbits, W)
        first = ref.segment_bounds(n_seg, W)
        assert first[0] == 0 and first[-1] == n_seg and (np.diff(first) >= 0).all() and np.diff(first).max() - np.diff(first).min() <= 1
        lens_all = rng.integers(0, 40, (W, n_entries)) * (rng.random((W, n_entries)) < 0.7)
        limit = 60                                                          # some unions above it, some below
        flags = [0] * (W - 1) + [2 if W > 1 else 0]
        G = np.minimum(lens_all.sum(axis=0), limit).astype(np.uint64)       # any table will do for plan 2
        for r in range(W):
            ref.assert_plans_equal(ref.x1_plan(lens_all, flags, own1, limit, W, r), _brute_x1(lens_all, flags, own1, limit, W, r), ("x1", W, r))
            ref.assert_plans_equal(ref.x2_plan(G, own1, first, bbits, W, r), _brute_x2(G, own1, first, bbits, W, r), ("x2", W, r))
        parts = [ref.x2_fill(G[own1 == r], own1, r) for r in range(W)]
        assert np.array_equal(np.sum(parts, axis=0), G)
        for r in range(W):
            assert (parts[r][own1 != r] == 0).all()
