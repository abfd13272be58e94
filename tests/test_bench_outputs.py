"""bench.py --dump-outputs on the host: the k-mers of the pooled results packed again as gasm.h packs them, and the .npy
files written from a batch's fetches — float32 / float64 only, every value exact, the same sample every time, the size cap
enforced.  The GPU side (a real run, twice) is test_gpu_parity.py::test_bench_plain_run_and_dumped_outputs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from genomeassembler_dev_amd.api import unpack_kmers  # noqa: E402


def _fake_batch(rng, n_seg, k):
    words = 1 if k <= 31 else 2
    per_seg = rng.integers(0, 60, n_seg)
    seg = np.concatenate([[0], np.cumsum(per_seg)]).astype(np.uint64)
    n = int(seg[-1])
    keys = rng.integers(0, 2**64, (n, words), dtype=np.uint64)
    keys[:, 0] &= np.uint64((1 << (2 * k - 64 * (words - 1))) - 1)          # only the bits k bases use
    keys = keys.reshape(-1)
    kmers = unpack_kmers(keys, k, words)
    mult = rng.integers(1, 1000, n).astype(np.uint32)
    contigs = [["".join(rng.choice(list("ACGT"), int(rng.integers(k, 3 * k)))) for _ in range(int(rng.integers(0, 4)))] for _ in range(n_seg)]
    flat = [c.encode() for cs in contigs for c in cs]
    cseg = np.concatenate([[0], np.cumsum([len(cs) for cs in contigs])]).astype(np.uint64)
    coff = np.concatenate([[0], np.cumsum([len(c) for c in flat])]).astype(np.uint64)
    nc = len(flat)
    scores = dict(bp_score=rng.random(nc), bp_score_norm_by_break_freqs=rng.random(nc), bp_score_norm_by_len=rng.random(nc),
                  kmer_breaks=rng.integers(0, 500, nc).astype(np.int32), sequence_len=np.array([len(c) for c in flat], dtype=np.int32))
    batch = dict(seg=seg, keys=keys, words=words, mult=mult, cseg=cseg, coff=coff, raw=b"".join(flat), scores=scores)
    res = []
    for s in range(n_seg):
        a, b, ca, cb = int(seg[s]), int(seg[s + 1]), int(cseg[s]), int(cseg[s + 1])
        res.append(dict(distinct=kmers[a:b], counts=mult[a:b].astype(np.int64), contigs=contigs[s], **{n: v[ca:cb] for n, v in scores.items()}))
    return batch, res


@pytest.mark.parametrize("k", [21, 31, 51])
def test_pooled_results_take_the_batch_form(k):
    batch, res = _fake_batch(np.random.default_rng(k), 7, k)
    got = bench._pooled_outputs(res, k)
    assert got["words"] == batch["words"] and got["raw"] == batch["raw"]
    for n in ("seg", "keys", "mult", "cseg", "coff"):
        assert np.array_equal(got[n], batch[n]), n
    for n, v in batch["scores"].items():
        assert np.array_equal(got["scores"][n], v), n


def test_written_outputs_are_exact_floats_and_a_fixed_sample(tmp_path):
    batch, _ = _fake_batch(np.random.default_rng(3), 40, 51)
    bench._write_outputs(str(tmp_path / "a"), batch, "", 5, 64_000_000)
    bench._write_outputs(str(tmp_path / "b"), batch, "", 5, 64_000_000)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 12
    d = {}
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        d[n[:-4]] = a
    seg = batch["seg"].astype(np.int64)
    sample = d["sample_segments"].astype(np.int64)
    assert len(sample) == 5 and (np.diff(sample) > 0).all()
    assert np.array_equal(d["distinct_kmers_per_segment"], np.diff(seg))
    assert np.array_equal(d["bp_score"], batch["scores"]["bp_score"])
    ix = np.concatenate([np.arange(seg[s], seg[s + 1]) for s in sample])
    words = batch["keys"].reshape(-1, 2)[ix]
    back = (d["sample_kmer_key_hi32"].astype(np.uint64) << np.uint64(32)) | d["sample_kmer_key_lo32"].astype(np.uint64)
    assert np.array_equal(back, words)
    assert np.array_equal(d["sample_kmer_multiplicity"], batch["mult"][ix])
    raw, cseg, coff = np.frombuffer(batch["raw"], np.uint8), batch["cseg"].astype(np.int64), batch["coff"].astype(np.int64)
    bases = np.concatenate([raw[coff[cseg[s]]:coff[cseg[s + 1]]] for s in sample])
    assert np.array_equal(d["sample_contig_bases"], bases.astype(np.float32))
    with pytest.raises(SystemExit):
        bench._write_outputs(str(tmp_path / "c"), batch, "", 40, 1000)
