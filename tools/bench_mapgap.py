"""What the gapped read-mapping pass (SegmentBatch.map_reads_gapped(): k_read_map_gapped) costs on a configs[2]-shaped batch kept on the
device, next to k_read_map of the same build in the same run.

Workload: 100 x 50 kb segments with planted repeats, 150-base reads at 50x, k = 31, max_edits = 6.  Lines:
  clean   the error-free reads (synth.make_batch), build(k), max_gap = 0: what the two-phase form costs where it finds what k_read_map finds
  indel   synth.simulate_reads_indel reads of the same genomes (1 % substitutions, 0.3 % indels), build(k, min_count = 2), max_gap = 3
Per line: the kernels' own durations by HIP events (gasm_profile_read; one step in flight, GASM_PINGPONG=0), mean over --reps launches
after --warmup, every launch behind a synchronise; and what the pass counted: the eight counters, the edit histogram, pileup and
gap-pileup adds.  accepted_chains is the histogram's sum: the chains that were verified AND kept.  A chain verified and rejected is
counted nowhere; rejected_reads are the reads none of whose chains was kept.  In every step k_read_map runs first, k_read_map_gapped
behind it.  One JSON line per line of the table.

  python tools/bench_mapgap.py [--segments 100] [--reps 10]"""
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
ap.add_argument("--max-edits", type=int, default=6)
args = ap.parse_args()

RL, COV, K = 150, 50, 31
KERNELS = ["k_read_map", "k_read_map_gapped"]


def main():
    os.environ["GASM_PINGPONG"] = "0"
    sys.path.insert(0, ROOT)
    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import synth
    from genomeassembler_dev_amd._lib import MAPG_FIELDS, GasmError, check, lib
    clean, seg_off, genomes = synth.make_batch(args.segments, args.seg_len, RL, COV, seed0=1234, planted=True)
    noisy = [synth.simulate_reads_indel(g, RL, COV, 4321 + s, 0.01, 0.003) for s, g in enumerate(genomes)]
    noisy_off = np.concatenate([[0], np.cumsum([len(r) for r in noisy])]).astype(np.uint64)
    ctx = ga.default_context()
    for name, reads, off, min_count, max_gap in (("clean", clean, seg_off, 1, 0), ("indel", np.concatenate(noisy, axis=0), noisy_off, 2, 3)):
        n_reads = int(off[-1])
        b = ga.SegmentBatch(reads.reshape(-1), off, fixed_len=RL)

        def step():
            b.build(K, genome_len_hint=args.seg_len, min_count=min_count)
            ctx.sync()
            check(lib().gasm_batch_map_reads(b.h, args.max_edits))
            check(lib().gasm_batch_map_reads_gapped(b.h, args.max_edits, max_gap))
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
        # what the last pass counted, summed straight from the library's host copies (no per-contig Python objects: the noisy build has
        # very many contigs)
        ps = [C.c_void_p() for _ in range(6)]
        check(lib().gasm_batch_fetch_read_map_gapped(b.h, *[C.byref(p) for p in ps]))
        seg, o, _ = b.contigs_raw()
        S, contigs = b.n_segments, int(seg[-1])
        cbases = int(o[-1]) if contigs else 0

        def arr(p, ct, n):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,)) if n else np.zeros(0, ct)
        cnt = arr(ps[5], C.c_uint64, S * len(MAPG_FIELDS)).reshape(S, -1).sum(axis=0)
        hist = arr(ps[4], C.c_uint32, S * (args.max_edits + 1)).reshape(S, -1).sum(axis=0, dtype=np.int64)
        adds = int(arr(ps[2], C.c_uint32, 4 * cbases).sum(dtype=np.int64))
        gap_adds = int(arr(ps[3], C.c_uint32, 2 * cbases).sum(dtype=np.int64))
        ms = {k: round(got[k][0] / got[k][1], 5) for k in KERNELS if k in got and got[k][1]}
        bases = n_reads * RL
        print(json.dumps(dict(line=name, segments=args.segments, seg_len=args.seg_len, read_len=RL, coverage=COV, k=K, min_count=min_count,
                              max_edits=args.max_edits, max_gap=max_gap, reads=n_reads, read_bases=bases, contigs=contigs,
                              counters=dict(zip(MAPG_FIELDS, map(int, cnt))), edit_hist=[int(x) for x in hist],
                              accepted_chains=int(hist.sum()), rejected_reads=int(cnt[3]), gapped_reads=int(cnt[7]), pileup_adds=adds,
                              gap_pileup_adds=gap_adds, launches={k: got[k][1] for k in KERNELS if k in got}, mean_ms=ms,
                              gapped_over_map=round(ms["k_read_map_gapped"] / ms["k_read_map"], 2),
                              ns_per_read_base=round(ms["k_read_map_gapped"] * 1e6 / bases, 5))), flush=True)
        b.close()


if __name__ == "__main__":
    main()
