"""What placing read pairs (SegmentBatch.place_pairs(): k_pair_place) costs on a configs[2]-shaped batch kept on the device, next to
k_read_thread of the same build on the same batch — the kernel of the same family (k-mer -> edge -> contig, offset), which looks up
once per chunk of a read and behind every crossing where the placement looks up a mate's first k-mer and scans on only after a miss.

Workload: 100 x 50 kb segments, 150-base reads at 50x, k = 31.  Lines:
  cfg2_fwd     synth.make_batch (planted repeats, error-free single reads) taken as interleaved pairs, build(k): one orientation.  The
               "mates" are unrelated reads: every mate 2 is looked up reverse-complemented in a forward-strand build, misses at
               position 0 and is scanned to its end — the kernel's worst case
  cfg2_both    the same reads, build(k, strands = 2): two orientations, every mate hits at position 0
  paired_both  synth.simulate_pairs of the same genomes (insert 500 +- --insert-sd, both strands), build(k, strands = 2)
Per line: the kernels' own durations by HIP events (gasm_profile_read; one step in flight, GASM_PINGPONG=0), mean over --reps launches
after --warmup, every launch behind a synchronise; and the placement's counters.  One JSON line per line of the table.

  python tools/bench_pairs.py [--segments 100] [--reps 10] [--insert-sd 50]"""
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
ap.add_argument("--insert-sd", type=float, default=50.0)
ap.add_argument("--max-insert", type=int, default=1024)
args = ap.parse_args()

RL, COV, K = 150, 50, 31
KERNELS = ["k_read_thread", "k_pair_place"]


def main():
    os.environ["GASM_PINGPONG"] = "0"
    sys.path.insert(0, ROOT)
    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import synth
    from genomeassembler_dev_amd._lib import PAIR_FIELDS, check, lib
    reads, seg_off, genomes = synth.make_batch(args.segments, args.seg_len, RL, COV, seed0=1234, planted=True)
    # an even number of reads per segment: the last read of an odd segment is left out
    keep = np.ones(len(reads), dtype=bool)
    for s in range(args.segments):
        if (int(seg_off[s + 1]) - int(seg_off[s])) & 1:
            keep[int(seg_off[s + 1]) - 1] = False
    even_off = np.concatenate([[0], np.cumsum([int(keep[int(seg_off[s]):int(seg_off[s + 1])].sum()) for s in range(args.segments)])])
    singles = (reads[keep], even_off)
    per_seg = [synth.simulate_pairs(genomes[s], RL, COV, 500, args.insert_sd, 1234 + s, both_strands=True)
               for s in range(args.segments)]
    paired = (np.concatenate(per_seg), np.concatenate([[0], np.cumsum([len(p) for p in per_seg])]))
    ctx = ga.default_context()
    for name, (data, off), strands in (("cfg2_fwd", singles, 1), ("cfg2_both", singles, 2), ("paired_both", paired, 2)):
        b = ga.SegmentBatch(data.reshape(-1), off, fixed_len=RL)

        def step():
            b.build(K, genome_len_hint=args.seg_len, strands=strands)
            ctx.sync()
            check(lib().gasm_batch_contig_links(b.h, RL))
            ctx.sync()
            check(lib().gasm_batch_place_pairs(b.h, args.max_insert))
            ctx.sync()
        for _ in range(args.warmup):
            step()
        ctx.profile(True, only=KERNELS)
        ctx.profile_reset()
        for _ in range(args.reps):
            step()
        got = ctx.profile_read()
        ctx.profile(False)
        pp = b.place_pairs(args.max_insert)
        counters = {f: int(sum(int(pp.counters(s)[i]) for s in range(pp.n_segments))) for i, f in enumerate(PAIR_FIELDS)}
        ms = {k: round(got[k][0] / got[k][1], 5) for k in KERNELS if k in got and got[k][1]}
        n_reads, oriented = int(off[-1]), pp.n_pairs * pp.orientations
        try:
            insert = pp.insert_size(0)
        except ValueError:
            insert = None
        print(json.dumps(dict(line=name, segments=args.segments, seg_len=args.seg_len, read_len=RL, coverage=COV, k=K, strands=strands,
                              max_insert=args.max_insert, insert_sd=args.insert_sd if name == "paired_both" else None, reads=n_reads, pairs=pp.n_pairs,
                              oriented_pairs=oriented, contigs=sum(len(pp.contigs(s)) for s in range(pp.n_segments)), counters=counters,
                              insert_size_segment0=insert, launches={k: got[k][1] for k in KERNELS if k in got}, mean_ms=ms,
                              place_over_thread=round(ms["k_pair_place"] / ms["k_read_thread"], 3),
                              ns_per_oriented_pair=round(ms["k_pair_place"] * 1e6 / oriented, 4),
                              ns_per_kmer_threaded=round(ms["k_read_thread"] * 1e6 / (n_reads * strands * (RL - K + 1)), 4))), flush=True)
        b.close()


if __name__ == "__main__":
    main()
