"""Device time of gasm_batch_count_read_kmers (kernels_count.hip, count_read_kmers of lib/DeNovoAssembler.R:135-168) on
  - the configs[2] shape: 100 x 50 kb segments, 150 bp reads at 50x (synth.make_batch, the reads bench.py builds from);
  - worst cases: one segment of as many bases, all poly-A reads (every lane adds to one LDS word), and one of 6-bp tandem reads.
For each split (workgroups per segment, GASM_RKC_SPLIT) the kernel is timed with the library's HIP-event pair per launch
(gasm_profile_*), after warm-up; one JSON line per (case, split).  Bytes read: the packed reads, once per workgroup of a
segment (plus the read offsets of ragged batches); bytes written: 69 904 u32 per segment."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import genomeassembler_dev_amd as ga  # noqa: E402
from genomeassembler_dev_amd import _lib, qtable, readkmers, synth  # noqa: E402


def _time(b, ctx, split, reps, warmup):
    os.environ["GASM_RKC_SPLIT"] = str(split)
    L = _lib.lib()
    for _ in range(warmup):
        _lib.check(L.gasm_batch_count_read_kmers(b.h))
    ctx.sync()
    ctx.profile(True, only=["k_read_kmer_count"])
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        _lib.check(L.gasm_batch_count_read_kmers(b.h))
    ctx.sync()
    wall = (time.perf_counter() - t0) / reps
    ms, n = ctx.profile_read()["k_read_kmer_count"]
    ctx.profile(False)
    return ms / n, wall * 1e3


def _case(name, b, ctx, n_segments, read_lens_per_seg, splits, reps, warmup):
    bases = sum(int(np.sum(x)) for x in read_lens_per_seg)
    windows = sum(int(np.sum(np.maximum(0, x - k + 1))) for x in read_lens_per_seg for k in readkmers.KMERS)
    packed = sum((int(np.sum(x)) + 31) // 32 * 8 for x in read_lens_per_seg)
    c = b.count_read_kmers()
    for k in readkmers.KMERS:      # every window counted once (a cheap whole-batch check; the tests compare with the oracle)
        want = [int(np.sum(np.maximum(0, x - k + 1))) for x in read_lens_per_seg]
        assert c[:, readkmers.table_slice(k)].sum(axis=1, dtype=np.int64).tolist() == want, (name, k)
    for split in splits:
        ms, wall_ms = _time(b, ctx, split, reps, warmup)
        rd = split * packed
        wr = n_segments * qtable.ROWS * 4
        print(json.dumps(dict(case=name, split=split, kernel_ms=round(ms, 4), call_ms_host=round(wall_ms, 4), segments=n_segments,
                              bases=bases, windows_all_k=windows, windows_per_s=round(windows / (ms * 1e-3), 1),
                              bytes_read=rd, bytes_written=wr, gb_per_s=round((rd + wr) / (ms * 1e-3) / 1e9, 2))), flush=True)
    if os.environ.get("GASM_RKC_SPLIT"):
        del os.environ["GASM_RKC_SPLIT"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--splits", default="2,4,8")
    args = ap.parse_args()
    splits = [int(s) for s in args.splits.split(",")]
    ctx = ga.default_context()

    n, L, rl, cov = 100, 50000, 150, 50
    reads, seg_off, _ = synth.make_batch(n, L, rl, cov, seed0=1234, planted=True)
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)
    lens = [np.full(int(seg_off[s + 1] - seg_off[s]), rl, dtype=np.int64) for s in range(n)]
    _case("configs2", b, ctx, n, lens, splits, args.reps, args.warmup)
    b.close()
    del reads

    nr = int(np.ceil(cov * L / rl))            # one segment of the same size, every read the same skewed string
    for name, unit in (("poly_a", "A"), ("tandem6", "ACGGTC")):
        read = (unit * (rl // len(unit) + 1))[:rl].encode()
        flat = np.frombuffer(read * nr, dtype=np.uint8)
        b = ga.SegmentBatch(flat, np.array([0, nr], dtype=np.uint64), fixed_len=rl)
        _case(name, b, ctx, 1, [np.full(nr, rl, dtype=np.int64)], splits, args.reps, args.warmup)
        b.close()


if __name__ == "__main__":
    main()
