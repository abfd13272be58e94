"""The exchange plans of the pooled build, restated in numpy (plain module: no test functions, no GPU, no libgasm).

What `k_x1_plan`, `k_x2_fill` and `k_x2_plan` (csrc/kernels_pool.hip) must compute, written from the comments above those
kernels and from DESIGN.md §7: every array is a gather of a run-length table followed by an exclusive prefix sum.
tests/test_pooled_limits_gpu.py compares the arrays the kernels wrote (gasm_comm_fetch_plan) with these, entry by entry;
tests/test_pooled_limit_cases_host.py checks these against a loop per bucket.

Names: W ranks, r this rank; nbt = n_segments << bbits buckets, bucket gb = segment << bbits | prefix; own1[gb] = the rank
that merges bucket gb; seg_first[d] .. seg_first[d + 1] = the segments rank d builds; lens_all[s, gb] = rank s's local run
length of bucket gb; G[gb] = length of the merged run of bucket gb."""
import numpy as np

PASS_ENTRIES = 8192      # entries one pass of the plan kernels' workgroup scan covers (1024 threads x 8)


def bucket_owner(n_segments, bbits, world):
    """a multiplicative hash of (segment, prefix) mod the world size"""
    gb = np.arange(n_segments << bbits, dtype=np.uint64)
    seg, pre = gb >> np.uint64(bbits), gb & np.uint64((1 << bbits) - 1)
    h = seg * np.uint64(0x9E3779B97F4A7C15) + pre * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(0x165667B19E3779F9)
    h ^= h >> np.uint64(29)
    h = h * np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    return (h % np.uint64(world)).astype(np.int64)


def segment_bounds(n_segments, world):
    """contiguous blocks, the first n_segments % world ranks hold one more"""
    n = np.full(world, n_segments // world, dtype=np.int64)
    n[:n_segments % world] += 1
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def _excl(v):
    """exclusive prefix sums of v with the total appended"""
    return np.concatenate([[0], np.cumsum(np.asarray(v, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)


def x1_plan(lens_all, flags, own1, limit, W, r):
    """exchange 1: every bucket's runs to the bucket's owner"""
    lens_all = np.asarray(lens_all, dtype=np.uint64).reshape(W, -1)
    own1 = np.asarray(own1, dtype=np.int64)
    mine = np.nonzero(own1 == r)[0]                                     # the buckets this rank merges, increasing
    order = np.argsort(own1, kind="stable")                             # all buckets by owner, increasing inside an owner
    got = lens_all[:, mine].T                                           # [j, source]: what arrives for this rank's j-th bucket
    run_off = np.cumsum(got, axis=0, dtype=np.uint64) - got             # records from the source's first
    send_off = _excl(lens_all[r, order])
    send_tot = np.array([lens_all[r, own1 == d].sum() for d in range(W)], dtype=np.uint64)
    cap = np.minimum(got.sum(axis=1, dtype=np.uint64), np.uint64(limit))       # a merged run holds at most what the table holds
    bstart = _excl(cap)
    f = 0
    for v in flags:
        f |= int(v)
    return dict(send_off=send_off, send_tot=send_tot, run_off=run_off.astype(np.uint64), run_len=got.astype(np.uint32),
                recv_tot=got.sum(axis=0, dtype=np.uint64), bstart=bstart, info=np.array([bstart[-1], 0], dtype=np.uint64), flags=f)


def x2_fill(merged_len, own1, r):
    """the table rank r contributes to the all-reduce: the merged lengths of its buckets (in increasing bucket order), zero elsewhere"""
    own1 = np.asarray(own1, dtype=np.int64)
    G = np.zeros(own1.size, dtype=np.uint64)
    G[own1 == r] = np.asarray(merged_len, dtype=np.uint64)
    return G


def x2_plan(G, own1, seg_first, bbits, W, r):
    """exchange 2: the merged runs to their segment's owner"""
    G = np.asarray(G, dtype=np.uint64)
    own1 = np.asarray(own1, dtype=np.int64)
    seg_first = np.asarray(seg_first, dtype=np.int64)
    lo, hi = int(seg_first[r]) << bbits, int(seg_first[r + 1]) << bbits
    got = np.zeros((hi - lo, W), dtype=np.uint64)                       # [bucket of this rank's segments, rank that merged it]
    got[np.arange(hi - lo), own1[lo:hi]] = G[lo:hi]
    run_off = np.cumsum(got, axis=0, dtype=np.uint64) - got
    mine = np.nonzero(own1 == r)[0]
    send_off = _excl(G[mine])
    dst = np.searchsorted(seg_first, mine >> bbits, side="right") - 1   # owner of the segment of every merged run
    send_tot = np.array([G[mine[dst == d]].sum() for d in range(W)], dtype=np.uint64)
    bstart = _excl(G[lo:hi])
    per_seg = G[lo:hi].reshape(-1, 1 << bbits).sum(axis=1, dtype=np.uint64)
    return dict(send_off=send_off, send_tot=send_tot, run_off=run_off.astype(np.uint64), run_len=got.astype(np.uint32),
                recv_tot=got.sum(axis=0, dtype=np.uint64), bstart=bstart,
                info=np.array([bstart[-1], per_seg.max(initial=0)], dtype=np.uint64), flags=0)


PLAN_ARRAYS = ("send_off", "send_tot", "run_off", "run_len", "recv_tot", "bstart", "info")


def assert_plans_equal(got, want, tag):
    for name in PLAN_ARRAYS:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        if not np.array_equal(g.astype(np.uint64), w.astype(np.uint64)):
            bad = np.nonzero(g.astype(np.uint64).reshape(-1) != w.astype(np.uint64).reshape(-1))[0]
            raise AssertionError((tag, name, "first difference at flat index", int(bad[0]), int(g.reshape(-1)[bad[0]]), int(w.reshape(-1)[bad[0]]),
                                  "differences", bad.size))
    assert int(got["flags"]) == int(want["flags"]), (tag, "flags", got["flags"], want["flags"])
