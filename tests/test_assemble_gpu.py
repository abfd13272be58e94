"""assemble_contigs on the device at the sizes the product runs, against the CPU oracle (strings compared exactly).

The inputs are those of tests/assemble_cases.py; tests/test_assemble_cases_host.py proves, with the oracle alone, that each
reaches the path it is built for: a second and third ballot chunk of k_asm_merge's backwards scan and compaction (more than
64 / 128 contigs), chains_equal returning true (a chain that spells another contig, a duplicated string), k_asm_match's second
32-base window (k = 41), the global bitonic step k_str_bitonic and the stage bookkeeping across LDS blocks (more than 512, and
once more than 32 768, distinct chains), chain_common against the plain comparison, k_chain_expand over elements that
contribute no base (contigs exactly k-1 long), and the n <= 2 048 gate on both sides.

Launch counts.  The sort runs on the m distinct chains, padded to p2 = the next power of two: one k_str_bitonic_block launch
per stage (log2 p2 of them) and, in a stage of width 2^s > 512, s - 9 launches of k_str_bitonic, (b - 9)(b - 8) / 2 in all
for b = log2 p2 >= 10.  The oracle gives the distinct scaffolds, not the distinct chains; m lies between their number (two
chains may spell one string, never the other way round) and what `rows` permutations of n contigs can give at all
(rows * n chains, and no more than the ordered arrangements of n contigs), so b is held to that range and the two counts to
each other; with more than 512 distinct scaffolds k_str_bitonic must have run, with at most 512 possible chains it must not."""
import functools
import time

import pytest

import assemble_cases as ac
import genomeassembler_dev_amd as ga
from oracle import orc
from test_gpu_parity import _check_scores

pytestmark = pytest.mark.gpu

ALL = [c.name for c in ac.CASES]
DIFFERENTIAL = [c.name for c in ac.CASES if c.claims.get("differential")]
SCORED = [c.name for c in ac.CASES if c.claims.get("score")]
GATE = 2048                                                      # assemble_signatures_device: more contigs go to the host merge


@functools.lru_cache(maxsize=2)
def _built(name):
    b = ac.BY_NAME[name].build()
    return b, ac.reference(b)


def _matrix(b):
    return ga.ContigMatrix(b["contigs"], b["perm"], b["k"], None, None, 1)


def _handle(b):
    if b["form"] == "graph":
        return ga.assemble_contigs(_matrix(b), b["k"], on_device=True)
    return ga.assemble_contigs_velvet(b["contigs"], b["k"], b["seed"], rows=b["rows"], on_device=True)


def _strings(b):
    ctx = ga.default_context()
    if b["form"] == "graph":
        return ga.assemble_contigs(_matrix(b), b["k"], ctx=ctx)
    return ga.assemble_contigs_velvet(b["contigs"], b["k"], b["seed"], rows=b["rows"], ctx=ctx)


def _first_difference(mine, ref):
    for i, (a, r) in enumerate(zip(mine, ref)):
        if a != r:
            return f"scaffold {i} differs: lengths {len(a)} / {len(r)}, first differing base {next((p for p in range(min(len(a), len(r))) if a[p] != r[p]), min(len(a), len(r)))}"
    return f"{len(mine)} scaffolds, the oracle has {len(ref)}"


def _assert_same(mine, ref):
    assert mine == ref, _first_difference(mine, ref)


def _arrangements(n, cap):
    """ordered arrangements of 1..n out of n contigs, or `cap` if there are more"""
    total, term = 0, 1
    for j in range(n):
        term *= n - j
        total += term
        if total >= cap:
            return cap
    return total


def _log2_ceil(x):
    return 0 if x <= 1 else (x - 1).bit_length()


@pytest.mark.parametrize("name", ALL)
def test_scaffolds_equal_the_oracle(name):
    b, ref = _built(name)
    n, rows, k = len(b["contigs"]), b["rows"], b["k"]
    ctx = ga.default_context()
    ctx.profile(True)
    try:
        ctx.profile_reset()
        t0 = time.perf_counter()
        sc = _handle(b)
        wall = time.perf_counter() - t0
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
    launches = {kn: prof.get(kn, (0.0, 0))[1] for kn in ("k_asm_match", "k_asm_merge", "k_chain_expand", "k_str_bitonic_block", "k_str_bitonic",
                                                          "k_str_adjacent_eq")}
    ms = {kn: round(prof.get(kn, (0.0, 0))[0], 3) for kn in launches}
    print(f"\n[assemble] {name}: n={n} rows={rows} k={k} distinct scaffolds={len(ref)} merge={sc.merge_device} rows_on_host={sc.rows_on_host} "
          f"launches={launches} kernel_ms={ms} call_s={wall:.3f}")
    try:
        assert len(sc) == len(ref)
        assert sc.lengths.tolist() == [len(s) for s in ref]
        _assert_same(sc.strings(), ref)
        if n <= GATE:
            assert sc.merge_device == "gpu" and sc.rows_on_host == 0
            assert launches["k_asm_match"] == 1 and launches["k_asm_merge"] == 1
        else:
            assert sc.merge_device == "host" and sc.rows_on_host == rows
            assert launches["k_asm_match"] == 0 and launches["k_asm_merge"] == 0
        assert launches["k_chain_expand"] == 2
        assert launches["k_str_adjacent_eq"] == 1
        blocks, steps = launches["k_str_bitonic_block"], launches["k_str_bitonic"]
        lo, hi = _log2_ceil(len(ref)), _log2_ceil(_arrangements(n, rows * n))
        assert lo <= blocks <= hi
        assert steps == ((blocks - 9) * (blocks - 8) // 2 if blocks >= 10 else 0)
        if len(ref) > 512:
            assert steps > 0
        if hi <= 9:
            assert steps == 0
    finally:
        sc.close()
    _assert_same(_strings(b), ref)                               # the string form through a context: the same device route


@pytest.mark.parametrize("name", DIFFERENTIAL)
def test_plain_sort_and_host_merge_give_the_same_list(name, monkeypatch):
    """GASM_ASM_PLAIN_SORT=1: the sort compares whole strings instead of skipping the elements two chains share
    (chain_common); GASM_ASM_HOST_MERGE=1: the greedy merge on host threads, expansion and sort on the GPU.  Both are read per
    call.  A difference with one of them set says which part to look at: merge, or expansion and sort."""
    b, ref = _built(name)
    monkeypatch.setenv("GASM_ASM_PLAIN_SORT", "1")
    sc = _handle(b)
    try:
        assert sc.merge_device == "gpu"
        _assert_same(sc.strings(), ref)
    finally:
        sc.close()
    monkeypatch.delenv("GASM_ASM_PLAIN_SORT")
    monkeypatch.setenv("GASM_ASM_HOST_MERGE", "1")
    sc = _handle(b)
    try:
        assert sc.merge_device == "host" and sc.rows_on_host == b["rows"]
        assert sc.lengths.tolist() == [len(s) for s in ref]
        _assert_same(sc.strings(), ref)
    finally:
        sc.close()
    monkeypatch.setenv("GASM_ASM_PLAIN_SORT", "1")               # neither the device merge nor the signature shortcut
    _assert_same(_strings(b), ref)


@pytest.mark.parametrize("name", SCORED)
def test_scores_from_the_handle(name, qtable):
    """the second expansion handed to calc_breakscore on the device, at a size where one 32-base word of the stream holds the
    end of one scaffold and the start of the next thousands of times: same scores as the oracle's on its own strings"""
    keys, prob = qtable
    b, ref = _built(name)
    sc = _handle(b)
    try:
        mine = ga.calc_breakscore(sc, b["reads"], b["truth"], 8, keys, prob, with_lev=False, with_freq=False)
    finally:
        sc.close()
    o = orc.calc_breakscore(ref, b["reads"], b["truth"], 8, keys, prob, with_lev=False, with_freq=False)
    _check_scores(mine, o, with_lev=False)
