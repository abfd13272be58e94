"""What read correction (SegmentBatch.correct_reads(), k_read_correct) costs on a configs[2]-shaped batch, beside one build step of the
same batch.

Workload: 100 x 50 kb segments, 150-base reads at 50x with 1 % substitutions, k = 31, min_count = 2 (the shape of
tools/bench_lowcov.py).  One process, one step in flight (GASM_PINGPONG=0: every launch on the batch's own context, where the
profiler counts).  Lines of JSON:
  build       `build(k, min_count = 2)` alone and `build; score`, host clock between two synchronisations, --steps steps per repetition
  correct     k_read_correct's own duration (HIP events around the kernel, gasm_profile_read) over --launches calls of correct_reads(),
              the call's host time (copy of the packed reads, kernel, new batch), the six counters summed over the segments, and
              first-pass look-ups per second: the k-mers of the reads (every one is looked up once) over the kernel's duration.  The
              candidate look-ups of the weak runs (up to 3k per run) come on top and are not counted.
There is no time target: the kernel's time is recorded against the build step of the same commit, for later work to beat.

  python tools/bench_correct.py [--segments 100] [--reps 5] [--steps 10] [--launches 10]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--segments", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--label", default="")
args = ap.parse_args()

L, RL, COV, K, MIN_COUNT, RATE = 50000, 150, 50, 31, 2, 0.01


def main():
    os.environ["GASM_PINGPONG"] = "0"
    sys.path.insert(0, ROOT)
    import numpy as np

    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import qtable, synth
    from genomeassembler_dev_amd._lib import CORRECT_FIELDS
    reads, seg_off, _ = synth.make_batch(args.segments, L, RL, COV, seed0=1234, planted=True)
    # 1 % substitutions: a mask, then a shift of 1..3 mod 4 in ACGT
    rng = np.random.default_rng(1235)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = np.zeros(256, dtype=np.uint8)
    code[lut] = np.arange(4, dtype=np.uint8)
    mask = rng.random(reads.shape) < RATE
    shift = rng.integers(1, 4, reads.shape).astype(np.uint8)
    reads = np.where(mask, lut[(code[reads] + shift) & 3], reads).astype(np.uint8)
    del mask, shift
    table = qtable.load_normalised()
    ctx = ga.default_context()
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=RL, ctx=ctx)
    shape = dict(segments=args.segments, seg_len=L, read_len=RL, coverage=COV, k=K, min_count=MIN_COUNT, rate=RATE, reads=int(seg_off[-1]))

    def timed(f):
        out = []
        for _ in range(args.reps):
            f()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f()
            ctx.sync()
            out.append((time.perf_counter() - t0) * 1e3 / args.steps)
        return dict(ms=[round(x, 4) for x in out], min_ms=round(min(out), 4), median_ms=round(statistics.median(out), 4), max_ms=round(max(out), 4))

    build = lambda: b.build(K, genome_len_hint=L, min_count=MIN_COUNT)
    print(json.dumps(dict(line="build", label=args.label, unit="ms per step", steps_per_rep=args.steps, build=timed(build),
                          build_score=timed(lambda: build().score(8, table)), **shape)), flush=True)
    build()
    kmers = b.total_kmers()
    b.correct_reads().close()                                    # (first call: allocations)
    ctx.profile(True, only=["k_read_correct"])
    ctx.profile_reset()
    host, stats = [], None
    for _ in range(args.launches):
        ctx.sync()
        t0 = time.perf_counter()
        c = b.correct_reads()
        host.append((time.perf_counter() - t0) * 1e3)
        stats = c.correction_stats().sum(axis=0).tolist()
        c.close()
    ms, n = ctx.profile_read()["k_read_correct"]
    ctx.profile(False)
    print(json.dumps(dict(line="correct", label=args.label, k_read_correct_ms=round(ms / n, 5), launches=n, correct_reads_host_ms_median=round(statistics.median(host), 4),
                          first_pass_lookups=kmers, first_pass_lookups_per_s=round(kmers / (ms / n * 1e-3)), stats=dict(zip(CORRECT_FIELDS, stats)), **shape)), flush=True)
    b.close()


if __name__ == "__main__":
    main()
