"""What the aligned form of the gapped read mapping (SegmentBatch.align_reads: k_read_map_trace) costs on a configs[2]-shaped batch kept on
the device, next to k_read_map_gapped and k_read_map_ends of the same build in the same run, and what it writes.

Workload: 50 x 50 kb segments with planted repeats, 150-base reads at 50x, k = 31, max_edits = 6, max_gap = 3, end_gap = 3.  Lines:
  clean   the error-free reads (synth.make_batch), build(k): one piece per read, nothing inserted
  indel   synth.simulate_reads_indel reads of the same genomes (1 % substitutions, 0.3 % indels), build(k, min_count = 2)
Per line: the kernels' own durations by HIP events (gasm_profile_read; one step in flight, GASM_PINGPONG=0), mean over --reps launches
after --warmup, every launch behind a synchronise; in every step k_read_map_gapped runs first, k_read_map_ends behind it, k_read_map_trace
last.  And what the aligned pass wrote: the piece records (80 bytes per read), the insertion pileup's size (16 W bytes per contig base,
cleared before the launch) and the adds to it (the inserted bases over all accepted chains), the reads by pieces of their best chain.
The eight tables of the aligned pass are held against the end-gapped pass's (counters, end counters, accepted chains).  One JSON line per
line of the table.

--old-only times k_read_map_gapped and k_read_map_ends alone and needs no aligned entry: with --root pointing at a checkout of the parent
commit (built), those are the parent's figures, to hold against this tree's TRACE = false instantiations.

  python tools/bench_maptrace.py [--segments 50] [--reps 10] [--old-only] [--root DIR]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--segments", type=int, default=50)
ap.add_argument("--seg-len", type=int, default=50000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-edits", type=int, default=6)
ap.add_argument("--max-gap", type=int, default=3)
ap.add_argument("--end-gap", type=int, default=3)
ap.add_argument("--old-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()

RL, COV, K = 150, 50, 31
PIECES = 10
KERNELS = ["k_read_map_gapped", "k_read_map_ends"] + ([] if args.old_only else ["k_read_map_trace"])


def main():
    os.environ["GASM_PINGPONG"] = "0"
    sys.path.insert(0, os.path.abspath(args.root))
    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import synth
    from genomeassembler_dev_amd._lib import MAPG_FIELDS, GasmError, check, lib
    clean, seg_off, genomes = synth.make_batch(args.segments, args.seg_len, RL, COV, seed0=1234, planted=True)
    noisy = [synth.simulate_reads_indel(g, RL, COV, 4321 + s, 0.01, 0.003) for s, g in enumerate(genomes)]
    noisy_off = np.concatenate([[0], np.cumsum([len(r) for r in noisy])]).astype(np.uint64)
    ctx = ga.default_context()
    for name, reads, off, min_count in (("clean", clean, seg_off, 1), ("indel", np.concatenate(noisy, axis=0), noisy_off, 2)):
        n_reads = int(off[-1])
        b = ga.SegmentBatch(reads.reshape(-1), off, fixed_len=RL)
        S = b.n_segments

        def arr(p, ct, n):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,)) if n else np.zeros(0, ct)

        def counted():
            """(the eight counters, accepted chains, the four end counters) of the gapped mapping that ran last, summed over the segments"""
            ps, pe = [C.c_void_p() for _ in range(6)], [C.c_void_p() for _ in range(2)]
            check(lib().gasm_batch_fetch_read_map_gapped(b.h, *[C.byref(p) for p in ps]))
            check(lib().gasm_batch_fetch_read_map_ends(b.h, *[C.byref(p) for p in pe]))
            cnt = arr(ps[5], C.c_uint64, S * len(MAPG_FIELDS)).reshape(S, -1).sum(axis=0)
            return ([int(x) for x in cnt], int(arr(ps[4], C.c_uint32, S * (args.max_edits + 1)).sum(dtype=np.int64)),
                    [int(x) for x in arr(pe[1], C.c_uint64, S * 4).reshape(S, 4).sum(axis=0)])
        seen = {}

        def step(fetch=False):
            b.build(K, genome_len_hint=args.seg_len, min_count=min_count)
            ctx.sync()
            check(lib().gasm_batch_map_reads_gapped(b.h, args.max_edits, args.max_gap))
            ctx.sync()
            check(lib().gasm_batch_map_reads_gapped_ends(b.h, args.max_edits, args.max_gap, args.end_gap))
            ctx.sync()
            if fetch:
                seen["ends"] = counted()
            if not args.old_only:
                check(lib().gasm_batch_map_reads_aligned(b.h, args.max_edits, args.max_gap, args.end_gap))
                ctx.sync()
                if fetch:
                    seen["trace"] = counted()
                    pa, cols = [C.c_void_p() for _ in range(2)], C.c_uint32()
                    check(lib().gasm_batch_fetch_read_alignments(b.h, *[C.byref(p) for p in pa], C.byref(cols)))
                    bases = sum(len(c) for cs in b.contigs() for c in cs)
                    W = int(cols.value)
                    ps = [C.c_void_p() for _ in range(6)]
                    check(lib().gasm_batch_fetch_read_map_gapped(b.h, *[C.byref(p) for p in ps]))
                    q = arr(ps[1], C.c_int32, 4 * n_reads).reshape(-1, 4)[:, 0]
                    ins = arr(pa[1], C.c_uint32, 4 * W * bases)
                    seen.update(ins_cols=W, contig_bases=bases, ins_adds=int(ins.sum(dtype=np.int64)), ins_cells=int(np.count_nonzero(ins)),
                                reads_by_pieces=[int(x) for x in np.bincount(q, minlength=PIECES + 1)],
                                valid_pieces=int(np.count_nonzero(arr(pa[0], C.c_int32, 2 * PIECES * n_reads).reshape(-1, 2)[:, 0])))
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
        step(fetch=True)
        ms = {k: round(got[k][0] / got[k][1], 5) for k in KERNELS if k in got and got[k][1]}
        out = dict(line=name, segments=args.segments, seg_len=args.seg_len, read_len=RL, coverage=COV, k=K, min_count=min_count, max_edits=args.max_edits,
                   max_gap=args.max_gap, end_gap=args.end_gap, reads=n_reads, read_bases=n_reads * RL, launches={k: got[k][1] for k in KERNELS if k in got},
                   mean_ms=ms, ends_over_gapped=round(ms["k_read_map_ends"] / ms["k_read_map_gapped"], 3), placed_ends=seen["ends"][0][4] + seen["ends"][0][5],
                   accepted_chains_ends=seen["ends"][1])
        if not args.old_only:
            assert seen["trace"] == seen["ends"], "the aligned pass counts what the end-gapped pass counts"
            assert seen["valid_pieces"] == sum(i * n for i, n in enumerate(seen["reads_by_pieces"]))
            out.update(trace_over_ends=round(ms["k_read_map_trace"] / ms["k_read_map_ends"], 3), piece_record_bytes=2 * 4 * PIECES * n_reads, ins_cols=seen["ins_cols"],
                       contig_bases=seen["contig_bases"], ins_pile_bytes=16 * seen["ins_cols"] * seen["contig_bases"], ins_pile_adds=seen["ins_adds"],
                       ins_pile_cells=seen["ins_cells"], reads_by_pieces=seen["reads_by_pieces"])
        print(json.dumps(out), flush=True)
        b.close()


if __name__ == "__main__":
    main()
