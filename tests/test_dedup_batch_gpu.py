"""The batch paths of the 64-bit de-duplication (k_bucket_dedup / dedup_step, kernels_build.hip) at the inputs where a change to
its probe or claim protocol would show first: every lane after one slot, tables filled to their limit and past it, key
counts around the iteration size, both table sizes, and the multi-pass rung.  Every case builds through SegmentBatch.build and compares distinct k-mers, multiplicities and contigs with the
oracle, as tests/test_gpu_parity.py does.

Run as a script (`--child`) this file is the child process of test_random_batches_both_tables: the table size
(GASM_DEDUP_TBL) is read once per process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import genomeassembler_dev_amd as ga  # noqa: E402
from genomeassembler_dev_amd import synth  # noqa: E402
from oracle import orc  # noqa: E402

pytestmark = pytest.mark.gpu


def _strs(a):
    return [r.tobytes().decode() for r in a]


def _check(b, segs, k, tag):
    """contigs, distinct k-mers and multiplicities of every segment against the oracle"""
    contigs = b.contigs()
    for s, rs in enumerate(segs):
        ref = orc.get_contigs(orc.kmers_from_reads(rs, k), k, 1, rows=1)
        assert contigs[s] == ref["contigs"], (tag, s)
        dk, dm = b.distinct_kmers(s)
        assert dk == ref["distinct"] and dm.tolist() == ref["counts"].tolist(), (tag, s)


def _one_segment(reads, rl):
    return ga.SegmentBatch(reads.reshape(-1), np.array([0, reads.shape[0]], dtype=np.uint64), fixed_len=rl)


@pytest.mark.parametrize("k", [15, 31])
def test_every_lane_claims_the_same_slot(k):
    """One segment of identical poly-A reads (40 x 50 bases = 2 kb): every key of every lane is the same k-mer, so in the
    first iteration all lanes see the same empty home set and go for the same slot — one CAS returns EMPTY, all the
    others return the key — and all counts go to one word."""
    rl, n = 50, 40
    reads = np.full((n, rl), ord("A"), dtype=np.uint8)
    b = _one_segment(reads, rl)
    b.build(k)
    _check(b, [_strs(reads)], k, k)
    dk, dm = b.distinct_kmers(0)
    assert dk == ["A" * k] and dm.tolist() == [n * (rl - k + 1)]
    b.close()


@pytest.mark.parametrize("k", [15, 31])
def test_same_homes_and_the_overflow_ladder(k):
    """A two-letter (A, C) random genome at 30x with a hint that gives two bucket bits (one segment: 900 >> 0 <= 900 -> no
    bit from the estimate, + 2 bits to fill the chip): the k-mers fall into the buckets of the prefixes A and C only.
    L = 3000 bases -> about 2830 (k = 15) and 2960 (k = 31) distinct k-mers, 1390 to 1510 per bucket against the 2048-slot
    table's limit of 11/16 * 2048 = 1408: the tables run up to the limit (long walks past full home sets) and at least one
    bucket exceeds it -> GASM_OVF_TABLE -> the next rung, the same partition with 4096-slot tables, which holds them.  The
    plan says which rung ran."""
    rng = np.random.default_rng(4100 + k)
    L, rl = 3000, 60
    g = np.frombuffer(b"AC", dtype=np.uint8)[rng.integers(0, 2, L)]
    reads = synth.simulate_reads(g, rl, 30, 7)
    rs = _strs(reads)
    ref = orc.get_contigs(orc.kmers_from_reads(rs, k), k, 1, rows=1)
    per_bucket = np.unique([x[0] for x in ref["distinct"]], return_counts=True)[1]
    assert per_bucket.max() > 1408 and per_bucket.min() > 1100, per_bucket          # the case is what it says
    b = _one_segment(reads, rl)
    b.build(k, genome_len_hint=900)
    assert b.contigs(0) == ref["contigs"]
    dk, dm = b.distinct_kmers(0)
    assert dk == ref["distinct"] and dm.tolist() == ref["counts"].tolist()
    p = b.build_plan()
    assert (p["bucket_bits"], p["table_slots"], p["multi_pass"]) == (2, 4096, 0), p
    # one attempt failed on the tables; a second one only if the skewed buckets also outgrew their regions (exact layout)
    assert p["distinct_attempts"] == (2 if p["single_pass"] else 3), p
    b.close()


@pytest.mark.parametrize("n_keys", [1535, 1536, 1537, 3071, 3073])
def test_iteration_boundary_key_counts(n_keys):
    """One bucket with n_keys keys around the iteration size of the 2048-slot kernel: 256 threads x 3 loads x 2 keys = 1536
    keys per iteration.  Reads of exactly k bases are one k-mer each, and all start with A: with genome_len_hint = 700
    (700 >> 0 <= 900: no bit from the estimate, + 2 bits for a one-segment batch) the two bucket bits are the first base,
    so the bucket of A holds every key, n_keys of them (plus whatever filler the partition pads its runs with, which the
    kernel skips: the counts bracket the boundary from both sides for that reason).  1535: tail lanes in a workgroup that
    has only a first iteration; 1536: exactly one; 1537, 3071, 3073: a last iteration of one key or of all but one.
    700 distinct k-mers (under the 1408 limit), so the table is never the reason for a rung of the ladder."""
    k = 31
    rng = np.random.default_rng(1000 + n_keys)
    pool = rng.integers(0, 4, (700, k))
    pool[:, 0] = 0
    reads = np.frombuffer(b"ACGT", dtype=np.uint8)[pool[rng.integers(0, 700, n_keys)]]
    b = _one_segment(reads, k)
    b.build(k, genome_len_hint=700)
    _check(b, [_strs(reads)], k, n_keys)
    p = b.build_plan()
    # (all keys in one of four bucket regions: the one-pass partition's region overflows and the exact layout is the one
    # rung taken; the table is the first attempt's)
    assert (p["bucket_bits"], p["table_slots"], p["multi_pass"]) == (2, 2048, 0), p
    assert p["distinct_attempts"] == (1 if p["single_pass"] else 2), p
    assert b.total_kmers() == n_keys
    b.close()


def _random_batches():
    out = []
    for k in (15, 31):
        reads, seg_off, _g = synth.make_batch(4, 5000, 100, 40, seed0=8800 + k, planted=True)
        out.append((k, reads, seg_off))
    return out


def _child():
    """four segments of 5 kb at 40x, k = 15 and k = 31, under the knobs of this process; one JSON verdict line"""
    verdict = dict(ok=False, plans={}, failures=[])
    try:
        for k, reads, seg_off in _random_batches():
            b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=100)
            b.build(k, genome_len_hint=5000)
            p = b.build_plan()
            verdict["plans"][str(k)] = {n: v for n, v in p.items() if n != "blocks"}
            _check(b, [_strs(reads[int(seg_off[s]):int(seg_off[s + 1])]) for s in range(4)], k, k)
            if p["distinct_attempts"] == 1 and p["table_slots"] != int(os.environ["GASM_DEDUP_TBL"]):
                verdict["failures"].append(f"k = {k}: {p['table_slots']} slots")
            b.close()
        verdict["ok"] = not verdict["failures"]
    except BaseException as e:      # (an AssertionError of _check included)
        verdict["failures"].append(repr(e)[-1500:])
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["ok"] else 1


@pytest.mark.parametrize("tbl", ["2048", "4096"])
def test_random_batches_both_tables(tbl):
    """Random batches through both table sizes.  The knob is read once per process: one child per table size."""
    env = {n: v for n, v in os.environ.items() if not n.startswith("GASM_DEDUP_")}
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env["GASM_DEDUP_TBL"] = tbl
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert r.returncode == 0 and lines, f"exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    verdict = json.loads(lines[-1])
    assert verdict["ok"], verdict
    assert all(p["table_slots"] == int(tbl) and p["key_words"] == 1 for p in verdict["plans"].values()), verdict


def test_multi_pass_rung_small():
    """A small case that reaches k_bucket_dedup_multi (which probes through the same dedup_step).  The rung needs a bucket
    of more than 2816 distinct 64-bit keys with all ten bucket bits used.  test_buckets_no_table_can_hold gets there with
    3 C : 1 A at 30 kb (the prefix CCCCC: (3/4)^5 = 24 % of 30 000 k-mers); at a tenth of that size the same composition
    leaves ~700 keys in that bucket and never reaches the rung, so the composition is skewed further instead — 7 C : 1 A,
    (7/8)^5 = 51 % of the ~6 900 distinct k-mers of 9 kb at 8x, about 3100 > 2816 — which keeps the case at under a third
    of the size (715 reads)."""
    rng = np.random.default_rng(2025)
    k, rl, L, cov = 31, 100, 9000, 8
    g = np.frombuffer(b"CCCCCCCA", dtype=np.uint8)[rng.integers(0, 8, L)]
    reads = synth.simulate_reads(g, rl, cov, 13)
    rs = _strs(reads)
    ref = orc.get_contigs(orc.kmers_from_reads(rs, k), k, 1, rows=1)
    top = max(np.unique([x[:5] for x in ref["distinct"]], return_counts=True)[1])
    assert top > 2816, top                                        # the case really needs the rung
    b = _one_segment(reads, rl)
    b.build(k, genome_len_hint=L)
    assert b.contigs(0) == ref["contigs"]
    dk, dm = b.distinct_kmers(0)
    assert dk == ref["distinct"] and dm.tolist() == ref["counts"].tolist()
    p = b.build_plan()
    assert (p["multi_pass"], p["bucket_bits"]) == (1, 10), p
    b.close()


if __name__ == "__main__":
    sys.exit(_child() if "--child" in sys.argv else 2)
