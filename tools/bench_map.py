"""What the read-mapping pass (SegmentBatch.map_reads(): k_read_map) costs on a configs[2]-shaped batch kept on the device, next to
k_read_thread of the same build — the kernel that makes the same look-up per k-mer and neither verifies nor piles up.

Workload: 100 x 50 kb segments with planted repeats (synth.make_batch), 150-base reads at 50x, k = 31, max_mismatch = 4.  Lines:
  clean   the error-free reads, build(k)
  noisy   the same reads with 1 % substitutions (every base changed with probability 0.01 to one of the three others), build(k, min_count = 2):
          the two lines differ in their build as well as in their reads; inside a line k_read_map and k_read_thread see the same build
Per line: the kernels' own durations by HIP events (gasm_profile_read; one step in flight, GASM_PINGPONG=0), mean over --reps launches
after --warmup, every launch behind a synchronise; and what the pass counted (the seven counters, accepted blocks, pileup adds issued),
so the durations can be set against read bases and adds.  One JSON line per line of the table.

  python tools/bench_map.py [--segments 100] [--reps 10]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--segments", type=int, default=100)
ap.add_argument("--seg-len", type=int, default=50000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-mismatch", type=int, default=4)
args = ap.parse_args()

RL, COV, K = 150, 50, 31
KERNELS = ["k_read_thread", "k_read_map"]


def substitute(reads, rate, seed):
    rng = np.random.default_rng(seed)
    flat = reads.reshape(-1).copy()
    hit = np.nonzero(rng.random(flat.size) < rate)[0]
    code = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), flat[hit])
    flat[hit] = np.frombuffer(b"ACGT", np.uint8)[(code + rng.integers(1, 4, hit.size)) % 4]
    return flat.reshape(reads.shape), int(hit.size)


def main():
    os.environ["GASM_PINGPONG"] = "0"
    sys.path.insert(0, ROOT)
    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import synth
    from genomeassembler_dev_amd._lib import MAP_FIELDS, GasmError, check, lib
    clean, seg_off, _ = synth.make_batch(args.segments, args.seg_len, RL, COV, seed0=1234, planted=True)
    noisy, n_subs = substitute(clean, 0.01, 99)
    ctx = ga.default_context()
    n_reads = int(seg_off[-1])
    for name, reads, min_count, subs in (("clean", clean, 1, 0), ("noisy", noisy, 2, n_subs)):
        b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=RL)

        def step():
            b.build(K, genome_len_hint=args.seg_len, min_count=min_count)
            ctx.sync()
            check(lib().gasm_batch_contig_links(b.h, 0))
            check(lib().gasm_batch_map_reads(b.h, args.max_mismatch))
            ctx.sync()
        try:
            for _ in range(args.warmup):
                step()
        except GasmError as e:                                        # (a batch of noisy reads can exceed the build's capacity bound: say so, go on)
            print(json.dumps(dict(line=name, segments=args.segments, min_count=min_count, error=str(e))), flush=True)
            b.close()
            continue
        ctx.profile(True, only=KERNELS)
        ctx.profile_reset()
        for _ in range(args.reps):
            step()
        got = ctx.profile_read()
        ctx.profile(False)
        rm = b.map_reads(args.max_mismatch)
        cnt = np.sum([rm.counters(s) for s in range(rm.n_segments)], axis=0)
        hist = np.sum([rm.mismatch_hist(s) for s in range(rm.n_segments)], axis=0)
        adds = sum(int(p.sum()) for s in range(rm.n_segments) for p in rm.pileup(s))
        ms = {k: round(got[k][0] / got[k][1], 5) for k in KERNELS if k in got and got[k][1]}
        bases = n_reads * RL
        print(json.dumps(dict(line=name, segments=args.segments, seg_len=args.seg_len, read_len=RL, coverage=COV, k=K, min_count=min_count,
                              max_mismatch=args.max_mismatch, reads=n_reads, read_bases=bases, substitutions=subs,
                              contigs=sum(len(rm.contigs(s)) for s in range(rm.n_segments)), counters=dict(zip(MAP_FIELDS, map(int, cnt))),
                              mismatch_hist=[int(x) for x in hist], accepted_blocks=int(hist.sum()), pileup_adds=adds,
                              launches={k: got[k][1] for k in KERNELS if k in got}, mean_ms=ms,
                              map_over_thread=round(ms["k_read_map"] / ms["k_read_thread"], 2),
                              ns_per_read_base=round(ms["k_read_map"] * 1e6 / bases, 5),
                              ns_per_pileup_add=round(ms["k_read_map"] * 1e6 / adds, 5) if adds else None)), flush=True)
        b.close()


if __name__ == "__main__":
    main()
