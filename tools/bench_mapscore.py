"""What mapped scoring (SegmentBatch.score_mapped(): k_score_mapped) costs on a configs[2]-shaped batch kept on the device, next to the
exact scorer (k_score_reads_graph) and to the mapping passes that feed it (k_read_map_gapped, k_read_map), all on the same build in the
same run.

Workload: 100 x 50 kb segments with planted repeats, 150-base reads at 50x, k = 31.  Lines:
  clean   the error-free reads (synth.make_batch), build(k), map_reads_gapped(0, 0) and map_reads(0)
  indel   synth.simulate_reads_indel reads of the same genomes (1 % substitutions, 0.3 % indels), build(k, min_count = 2),
          map_reads_gapped(6, 3) and map_reads(6)
Per line and T = 1, 2 tables: the kernels' own durations by HIP events (gasm_profile_read; one step in flight, GASM_PINGPONG=0), mean over
--reps launches after --warmup, every launch behind a synchronise; and the four class counters.  In every step the exact scorer runs
first, then the gapped mapping and mapped scoring from it (k_score_mapped_gapped: two 16-byte records per read), then the ungapped mapping
and mapped scoring from it (k_score_mapped: one record per read).  One JSON line per (line, T).

  python tools/bench_mapscore.py [--segments 100] [--reps 10]"""
import argparse
import ctypes as C
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
args = ap.parse_args()

RL, COV, K, KMER = 150, 50, 31, 8
KERNELS = ["k_score_mapped_gapped", "k_score_mapped", "k_score_reads_graph", "k_read_map_gapped", "k_read_map", "k_score_finish"]


def main():
    os.environ["GASM_PINGPONG"] = "0"
    sys.path.insert(0, ROOT)
    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import qtable, synth
    from genomeassembler_dev_amd._lib import MAPSCORE_FIELDS, GasmError, check, lib
    clean, seg_off, genomes = synth.make_batch(args.segments, args.seg_len, RL, COV, seed0=1234, planted=True)
    noisy = [synth.simulate_reads_indel(g, RL, COV, 4321 + s, 0.01, 0.003) for s, g in enumerate(genomes)]
    noisy_off = np.concatenate([[0], np.cumsum([len(r) for r in noisy])]).astype(np.uint64)
    q = qtable.load_normalised()
    tabs = np.stack([q, np.full(len(q), 1.0 / len(q))])
    ctx = ga.default_context()
    for name, reads, off, min_count, edits, gap in (("clean", clean, seg_off, 1, 0, 0), ("indel", np.concatenate(noisy, axis=0), noisy_off, 2, 6, 3)):
        n_reads = int(off[-1])
        b = ga.SegmentBatch(reads.reshape(-1), off, fixed_len=RL)
        for T in (1, 2):
            t = np.ascontiguousarray(tabs[:T])

            def step():
                b.build(K, genome_len_hint=args.seg_len, min_count=min_count)
                ctx.sync()
                check(lib().gasm_batch_score_tables(b.h, KMER, t.ctypes.data_as(C.c_void_p), T))
                ctx.sync()
                check(lib().gasm_batch_map_reads_gapped(b.h, edits, gap))
                ctx.sync()
                check(lib().gasm_batch_score_mapped(b.h, 1, KMER, t.ctypes.data_as(C.c_void_p), T, 0))
                ctx.sync()
                check(lib().gasm_batch_map_reads(b.h, edits))
                ctx.sync()
                check(lib().gasm_batch_score_mapped(b.h, 0, KMER, t.ctypes.data_as(C.c_void_p), T, 0))
                ctx.sync()
            try:
                for _ in range(args.warmup):
                    step()
            except GasmError as e:                                    # (a batch of noisy reads can exceed the build's capacity bound: say so, go on)
                print(json.dumps(dict(line=name, tables=T, segments=args.segments, min_count=min_count, error=str(e))), flush=True)
                break
            ctx.profile(True, only=KERNELS)
            ctx.profile_reset()
            for _ in range(args.reps):
                step()
            got = ctx.profile_read()
            ctx.profile(False)
            sp, cp = C.c_void_p(), C.c_void_p()
            check(lib().gasm_batch_fetch_mapped_starts(b.h, C.byref(sp), C.byref(cp)))
            S = b.n_segments
            cnt = np.ctypeslib.as_array(C.cast(cp, C.POINTER(C.c_uint64)), shape=(S * len(MAPSCORE_FIELDS),)).reshape(S, -1).sum(axis=0)
            seg = b.contigs_raw()[0]
            ms = {k: round(got[k][0] / got[k][1], 5) for k in KERNELS if k in got and got[k][1]}
            print(json.dumps(dict(line=name, tables=T, segments=args.segments, seg_len=args.seg_len, read_len=RL, coverage=COV, k=K, min_count=min_count,
                                  max_edits=edits, max_gap=gap, reads=n_reads, contigs=int(seg[-1]), counters=dict(zip(MAPSCORE_FIELDS, map(int, cnt))),
                                  launches={k: got[k][1] for k in KERNELS if k in got}, mean_ms=ms,
                                  mapped_over_exact=round(ms["k_score_mapped_gapped"] / ms["k_score_reads_graph"], 2),
                                  mapped_over_mapping=round(ms["k_score_mapped_gapped"] / ms["k_read_map_gapped"], 4),
                                  ns_per_read=round(ms["k_score_mapped_gapped"] * 1e6 / n_reads, 4))), flush=True)
        b.close()


if __name__ == "__main__":
    main()
