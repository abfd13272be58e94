"""The cases of tests/assemble_cases.py reach the paths they are built for: proved with the CPU oracle alone (no GPU).

tests/test_assemble_gpu.py runs k_asm_match / k_asm_merge / k_chain_expand / k_str_bitonic* on these inputs.  What makes an
input reach a second ballot chunk, the global bitonic step, the second 32-base window or the full-string test is a property
of the input, so it is asserted here: a later edit of a builder cannot quietly shrink a case back to what the older tests
covered.  The thresholds are the kernels' own constants (64 lanes, 512 positions per LDS block, 32 bases per window, 32 768 =
the last power of two the 54 004-scaffold case passes), not measurements."""
import pytest

import genomeassembler_dev_amd as ga
import assemble_cases as ac


def _suffix_index(contigs, ov):
    ix = {}
    for i, c in enumerate(contigs):
        ix.setdefault(c[len(c) - ov:], []).append(i)
    return ix


def check_claims(case, b, ref):
    """every property `case.claims` names holds for the built case `b` and the oracle's scaffolds `ref`"""
    cl, contigs, k = case.claims, b["contigs"], b["k"]
    n = len(contigs)
    assert all(len(c) >= k - 1 for c in contigs)               # (the index form of the merge applies)
    if "n_exact" in cl:
        assert n == cl["n_exact"]
    if "n_above" in cl:
        assert n > cl["n_above"]
    if "scaffolds_above" in cl:
        assert len(set(ref)) == len(ref) > cl["scaffolds_above"]
    if cl.get("large"):
        assert len(ref) > 32768
    suf = _suffix_index(contigs, k - 1)
    if cl.get("spelled"):
        have = set(contigs)
        assert any(a != bb and contigs[a] + contigs[bb][k - 1:] in have - {contigs[a], contigs[bb]}
                   for bb in range(n) for a in suf.get(contigs[bb][:k - 1], ()))
    if cl.get("has_k1"):
        short = [i for i, c in enumerate(contigs) if len(c) == k - 1]
        assert short and any(a != i for i in short for a in suf.get(contigs[i], ()))
    if cl.get("merged_above_32"):
        assert k - 1 > 32
        assert any(a != bb and contigs[a] != contigs[bb] for bb in range(n) for a in suf.get(contigs[bb][:k - 1], ()))
        assert max(len(s) for s in ref) > max(len(c) for c in contigs)
    if cl.get("decoy_above_32"):
        assert k - 1 > 32
        first = {}
        for i, c in enumerate(contigs):
            first.setdefault(c[len(c) - (k - 1):][:32], []).append(i)
        assert any(a != bb and contigs[a][len(contigs[a]) - (k - 1):] != contigs[bb][:k - 1]
                   for bb in range(n) if len(contigs[bb]) > 32 for a in first.get(contigs[bb][:32], ()))
    if cl.get("duplicate"):
        assert len(set(contigs)) < n


@pytest.mark.parametrize("case", ac.CASES, ids=[c.name for c in ac.CASES])
def test_case_reaches_its_path(case):
    b = case.build()
    ref = ac.reference(b)
    check_claims(case, b, ref)
    assert [len(s) for s in ref] == sorted((len(s) for s in ref), reverse=True)
    if not case.claims.get("large"):
        # the host's index merge (what GASM_ASM_HOST_MERGE=1 and the n > 2 048 gate fall back to) at these sizes
        if b["form"] == "graph":
            mine = ga.assemble_contigs(ga.ContigMatrix(b["contigs"], b["perm"], b["k"], None, None, 1), b["k"])
        else:
            mine = ga.assemble_contigs_velvet(b["contigs"], b["k"], b["seed"], rows=b["rows"])
        assert mine == ref


def test_the_case_set_covers_both_sides_of_every_threshold():
    cl = {c.name: c.claims for c in ac.CASES}
    ns = sorted(c["n_exact"] for c in cl.values() if "n_exact" in c)
    assert {63, 64, 65, 128, 129, 2048, 2049} <= set(ns)
    assert sum(1 for c in cl.values() if c.get("has_k1")) >= 2
    assert sum(1 for c in cl.values() if c.get("large")) == 1
    assert any(c.get("merged_above_32") for c in cl.values()) and any(c.get("decoy_above_32") for c in cl.values())
    assert any(c.get("duplicate") for c in cl.values())
    assert sum(1 for c in cl.values() if c.get("differential") and c.get("scaffolds_above", 0) >= 512) >= 2
