"""The pooled exchange past its plan-scan and merge-table limits (inputs: tests/pooled_limit_cases.py, proved on the CPU by
tests/test_pooled_limit_cases_host.py).

Three kinds of check: the differential of tests/test_pooled_gpu.py (virtual ranks = single-GPU build = oracle) on inputs whose
plan tables take more than one 8 192-entry scan pass, whose merged bucket holds exactly LIMIT / LIMIT + 1 keys, and whose read
pieces are cut inside words; every array the plan kernels wrote (gasm_comm_fetch_plan) against the numpy restatement of
tests/pooled_plan_ref.py, which localises a failure of the differential; `k_pack_runs` / `k_bucket_merge` alone through the
staged entry points against a numpy merge."""
import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import pooled_limit_cases as plc
import pooled_plan_ref as ref
from genomeassembler_dev_amd import pooled
from oracle import exact_scores, orc
from test_pooled_gpu import _check_against_single

pytestmark = pytest.mark.gpu

_built = {}


def _case(case):
    if case.name not in _built:
        _built[case.name] = case.build()
    return _built[case.name]


def _single(b, prob):
    single = ga.SegmentBatch(b["reads"].reshape(-1), b["seg_off"], fixed_len=b["rl"])
    single.build(b["k"]).score(8, prob)
    return single


def _same_bits(b, single, prob):
    """the condition test_exchange_build_headline_shape states: one fixed-point shift for every read count of the batch"""
    n = np.diff(b["seg_off"].astype(np.int64))
    return bool(n.min() > 0 and exact_scores.fixed_shift(prob, n.min()) == exact_scores.fixed_shift(prob, n.max()) == single.score_fixed()[1])


def _exchange(b, world, prob, keep=False):
    ctx = ga.default_context()
    comm = pooled.Comm.virtual(ctx, world)
    if keep:
        comm.keep_plans()
    be = [pooled.GasmBackend(rr, so, b["rl"]) for rr, so in b["deal"](world)]
    stats, own = pooled.exchange_build(comm, be, b["k"], b["bbits"], kmer=8, table=prob)
    return comm, be, stats, own


def _close(comm, be):
    for x in be:
        x.close()
    comm.close()


def _check_plans(b, comm, world, bbits, single, tag):
    """plan 1 and plan 2 of every virtual rank, entry by entry, against the restatement"""
    k, n_seg = b["k"], len(b["seg_off"]) - 1
    limit = plc.merge_limit(1 if k <= 31 else 2)
    own1, first = ref.bucket_owner(n_seg, bbits, world), ref.segment_bounds(n_seg, world)
    lib_own, lib_first = pooled.owners(n_seg, bbits, world)
    assert lib_own.tolist() == own1.tolist() and lib_first.tolist() == first.tolist(), tag
    lens = []
    for rr, so in b["deal"](world):                       # the run-length tables, from pools of their own
        x = pooled.GasmBackend(rr, so, b["rl"])
        lens.append(x.local_runs(k, bbits).astype(np.int64))
        x.close()
        assert lens[-1].tolist() == plc.run_lengths(rr, so, k, bbits).tolist(), tag
    lens_all = np.stack(lens)
    G = np.zeros(n_seg << bbits, dtype=np.uint64)         # merged lengths: the single build's distinct k-mers per bucket
    for s in range(n_seg):
        G[s << bbits:(s + 1) << bbits] = np.bincount(plc.bucket_of(single.distinct_kmers(s)[0], k, bbits), minlength=1 << bbits)
    assert np.array_equal(np.sum([ref.x2_fill(G[own1 == r], own1, r) for r in range(world)], axis=0), G)
    for r in range(world):
        ref.assert_plans_equal(comm.fetch_plan(1, r), ref.x1_plan(lens_all, [0] * world, own1, limit, world, r), (tag, "plan 1", r))
        ref.assert_plans_equal(comm.fetch_plan(2, r), ref.x2_plan(G, own1, first, bbits, world, r), (tag, "plan 2", r))


# ------------------------------------------------------------------------------------------------ A: more than one scan pass
@pytest.mark.parametrize("case", plc.SCAN_CASES, ids=lambda c: c.name)
def test_exchange_build_past_one_scan_pass(qtable, case):
    keys, prob = qtable
    b = _case(case)
    k, bbits, seg_off = b["k"], b["bbits"], b["seg_off"]
    n_seg = len(seg_off) - 1
    assert n_seg << bbits > ref.PASS_ENTRIES
    single = _single(b, prob)
    same = _same_bits(b, single, prob)
    for world in b["worlds"]:
        comm, be, stats, own = _exchange(b, world, prob, keep=True)
        assert stats["bbits"] == bbits, stats                  # (no bucket overflows: the table sizes are the ones asked for)
        _check_plans(b, comm, world, bbits, single, (case.name, world))
        _check_against_single(dict(enumerate(be)), own, single, n_seg, (case.name, world), same_bits=same)
        _close(comm, be)
    # the single build against the oracle: the first segment, the one with a single read, the one whose buckets straddle entry 8 192
    s_contigs = single.contigs()
    assert s_contigs[1] == []
    for s in (0, 2, ref.PASS_ENTRIES >> bbits):
        rs = plc.strs(b["reads"][int(seg_off[s]):int(seg_off[s + 1])])
        o = orc.get_contigs(orc.kmers_from_reads(rs, k), k, 1, rows=1)
        dk, dm = single.distinct_kmers(s)
        assert s_contigs[s] == o["contigs"] and dk == o["distinct"] and dm.tolist() == o["counts"].tolist(), (case.name, s)
    single.close()


# ------------------------------------------------------------------------------------------------ B: the merge table at its limit
@pytest.mark.parametrize("case", plc.LIMIT_CASES, ids=lambda c: c.name)
def test_exchange_build_at_the_merge_limit(qtable, case):
    """A union of exactly LIMIT keys fits the merge table at the bucket bits asked for; one key more and every rank moves to more
    bucket bits in the same call.  Either way the result is the single build's, and the plans are the restatement's."""
    keys, prob = qtable
    b = _case(case)
    k, limit = b["k"], b["limit"]
    single = _single(b, prob)
    assert len(single.distinct_kmers(0)[0]) == b["union"]
    comm, be, stats, own = _exchange(b, 3, prob, keep=True)
    print(f"{case.name}: union {b['union']} of limit {limit}: bucket bits {stats['bbits']} after {stats['attempts']} attempt(s)")
    if b["union"] == limit:
        assert stats["bbits"] == 0, stats                      # the first bucket configuration: one bucket holds the whole union
        p2 = comm.fetch_plan(2, 0)
        assert p2["flags"] == 0 and int(p2["info"][0]) == limit and int(p2["info"][1]) == limit, p2
    else:
        assert stats["bbits"] >= 2 and stats["attempts"] >= 2, stats
    _check_plans(b, comm, 3, stats["bbits"], single, case.name)
    _check_against_single(dict(enumerate(be)), own, single, 1, case.name, same_bits=_same_bits(b, single, prob))
    _close(comm, be)
    single.close()


# ------------------------------------------------------------------------------------------------ C: read pieces
@pytest.mark.parametrize("case", plc.PIECE_CASES, ids=lambda c: c.name)
def test_exchange_build_with_pieces_inside_words(qtable, case):
    keys, prob = qtable
    b = _case(case)
    k, seg_off = b["k"], b["seg_off"]
    single = _single(b, prob)
    same = _same_bits(b, single, prob)
    for world in b["worlds"]:
        comm, be, stats, own = _exchange(b, world, prob)
        for step in range(2):                                  # the second step sends the pieces straight into place
            if step:
                stats, own = pooled.exchange_build(comm, be, k, b["bbits"], kmer=8, table=prob)
            assert stats["bbits"] == b["bbits"], stats
            _check_against_single(dict(enumerate(be)), own, single, 5, (case.name, world, step), same_bits=same)
        _close(comm, be)
    s_contigs, s_sc = single.contigs(), single.scores()
    for s in (0, 2, 4):
        o = orc.build_score(plc.strs(b["reads"][int(seg_off[s]):int(seg_off[s + 1])]), k, 8, keys, prob)
        ca, ce = int(s_sc["seg_contig_off"][s]), int(s_sc["seg_contig_off"][s + 1])
        assert s_contigs[s] == o["contigs"] and s_sc["kmer_breaks"][ca:ce].tolist() == o["kmer_breaks"].tolist(), (case.name, s)
        assert np.abs(s_sc["bp_score"][ca:ce] - o["bp_score"]).max(initial=0.0) < 1e-9, (case.name, s)
        assert exact_scores.rel_close(s_sc["bp_score"][ca:ce], o["bp_score"]).all(), (case.name, s)
    single.close()


# ------------------------------------------------------------------------------------------------ the merge and the packing alone
@pytest.fixture(scope="module")
def real_runs():
    """k -> sorted distinct (key, count) runs of a small real build, one per bucket: (backend, [keys [n, words] uint64], [counts],
    bbits); built once per key width, the pools closed when the module is done"""
    import torch
    cache = {}

    def get(k):
        if k not in cache:
            rng = np.random.default_rng(500 + k)
            g = plc._genome(rng, 1500)
            reads = plc._reads_at(g, rng.integers(0, 1500 - 60 + 1, 200), 60)
            be = pooled.GasmBackend(reads, np.array([0, reads.shape[0]], dtype=np.uint64), 60)
            bbits = 2
            lens = be.local_runs(k, bbits).astype(np.int64)
            keys, cnt = be.pack_runs(np.arange(4), int(lens.sum()))
            torch.cuda.synchronize()
            kk = keys.cpu().numpy().view(np.uint64).reshape(-1, be.words)
            cc = cnt.cpu().numpy().astype(np.int64)
            assert lens.tolist() == plc.run_lengths(reads, np.array([0, reads.shape[0]]), k, bbits).tolist() and lens.min() > 100
            off = np.concatenate([[0], np.cumsum(lens)])
            cache[k] = (be, [kk[off[j]:off[j + 1]] for j in range(4)], [cc[off[j]:off[j + 1]] for j in range(4)], bbits)
        return cache[k]
    yield get
    for be, *_ in cache.values():
        be.close()


def _key_ints(keys):
    return [int(r[0]) if keys.shape[1] == 1 else (int(r[0]) << 64) | int(r[1]) for r in keys]


@pytest.mark.parametrize("shape", ["one_source", "identical", "interleaved"])
@pytest.mark.parametrize("n_src", [1, 2, 8])
@pytest.mark.parametrize("k", [21, 35])
def test_merge_and_pack_runs_alone(real_runs, k, n_src, shape):
    import torch
    be, rkeys, rcnt, bbits = real_runs(k)
    words, n_out = be.words, 4
    for j in range(n_out):                                     # (the inputs are sorted, distinct runs of valid k-mers)
        ints = _key_ints(rkeys[j])
        assert ints == sorted(set(ints))
    in_keys, in_cnt = [], []
    run_off, run_len = np.zeros((n_out, n_src), np.uint64), np.zeros((n_out, n_src), np.uint32)
    pos = 0
    for j in range(n_out):
        for s in range(n_src):
            if shape == "one_source":
                sel = slice(None) if s == (j + n_src - 1) % n_src else slice(0, 0)
            elif shape == "identical":
                sel = slice(None)
            else:
                sel = slice(s, None, n_src)
            kk, cc = rkeys[j][sel], rcnt[j][sel]
            run_off[j, s], run_len[j, s] = pos, kk.shape[0]
            pos += kk.shape[0]
            in_keys.append(kk)
            in_cnt.append(cc)
    want = [{} for _ in range(n_out)]                            # the merge of the records: a count per distinct key, keys sorted
    i = 0
    for j in range(n_out):
        for s in range(n_src):
            for v, c in zip(_key_ints(in_keys[i]), in_cnt[i].tolist()):
                want[j][v] = want[j].get(v, 0) + c
            i += 1
    d_keys = torch.as_tensor(np.concatenate(in_keys).reshape(-1).view(np.int64), device=be.device)
    d_cnt = torch.as_tensor(np.concatenate(in_cnt).astype(np.int32), device=be.device)
    merged = be.merge_runs(n_out, n_src, run_off, run_len, d_keys, d_cnt).astype(np.int64)
    assert merged.tolist() == [len(w) for w in want], (k, n_src, shape)                     # bucket_d
    fdir, fbits = be.fine_directory(n_out)
    assert fbits == (10 if words == 1 else 9)
    out_keys, out_cnt = be.pack_runs(np.arange(n_out), int(merged.sum()))                     # the merged runs, through k_pack_runs
    torch.cuda.synchronize()
    ok = out_keys.cpu().numpy().view(np.uint64).reshape(-1, words)
    oc = out_cnt.cpu().numpy().astype(np.int64)
    off = np.concatenate([[0], np.cumsum(merged)])
    low_bits = 2 * k - bbits
    bshift = max(low_bits - fbits, 0)
    for j in range(n_out):
        got = _key_ints(ok[off[j]:off[j + 1]])
        assert got == sorted(want[j]), (k, n_src, shape, j)                                   # keys sorted, each once
        assert oc[off[j]:off[j + 1]].tolist() == [want[j][v] for v in got], (k, n_src, shape, j)      # counts summed
        if shape == "identical":
            assert oc[off[j]:off[j + 1]].tolist() == (rcnt[j] * n_src).tolist()
        bins = np.array([(v >> bshift) & ((1 << fbits) - 1) for v in got], dtype=np.int64)
        assert (np.diff(bins) >= 0).all()
        row = np.searchsorted(bins, np.arange((1 << fbits) + 1), side="left")                 # offset of every bin inside the bucket
        row[-1] = bins.size
        assert fdir[j].astype(np.int64).tolist() == row.tolist(), (k, n_src, shape, j)
