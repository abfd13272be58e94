"""What the contig-links pass (SegmentBatch.contig_links(): k_contig_links + k_read_thread) costs on a configs[2]-shaped batch kept on
the device, next to k_score_reads_graph of the same build — the kernel that makes the same first look-up (k-mer -> edge -> contig,
offset), once per READ where threading makes it once per K-MER.

Workload: 100 x 50 kb segments with planted repeats (synth.make_batch), error-free 150-base reads at 50x, k = 31.  Lines:
  fwd          build(k), strands = 1, span_len = 150
  fwd_nospan   the same pass with span_len = 0
  both         build(k, strands = 2): every read and its reverse complement are threaded
Per line: the kernels' own durations by HIP events (gasm_profile_read; one step in flight, GASM_PINGPONG=0), mean over --reps launches
after --warmup, every launch behind a synchronise; and what the pass counted (contigs, links, crossings, spans), so the durations can be
set against k-mers threaded.  One JSON line per line of the table.

  python tools/bench_links.py [--segments 100] [--reps 10]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--segments", type=int, default=100)
ap.add_argument("--seg-len", type=int, default=50000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

RL, COV, K = 150, 50, 31
KERNELS = ["k_score_reads_graph", "k_contig_links", "k_read_thread"]
LINES = {"fwd": (1, RL), "fwd_nospan": (1, 0), "both": (2, RL)}          # (strands, span_len)


def main():
    os.environ["GASM_PINGPONG"] = "0"
    sys.path.insert(0, ROOT)
    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import qtable, synth
    from genomeassembler_dev_amd._lib import check, lib
    table = qtable.load_normalised()
    reads, seg_off, _ = synth.make_batch(args.segments, args.seg_len, RL, COV, seed0=1234, planted=True)
    ctx = ga.default_context()
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=RL)
    n_reads = int(seg_off[-1])
    for name, (strands, span_len) in LINES.items():
        def step():
            b.build(K, genome_len_hint=args.seg_len, strands=strands).score(8, table)
            ctx.sync()
            check(lib().gasm_batch_contig_links(b.h, span_len))
            ctx.sync()
        for _ in range(args.warmup):
            step()
        ctx.profile(True, only=KERNELS)
        ctx.profile_reset()
        for _ in range(args.reps):
            step()
        got = ctx.profile_read()
        ctx.profile(False)
        cl = b.contig_links(span_len)
        crossings = sum(int(cl.link_support(s).sum()) for s in range(cl.n_segments))
        spans = sum(int(cl.span_support(s).sum()) for s in range(cl.n_segments))
        links = sum(len(cl.links(s)) for s in range(cl.n_segments))
        ms = {k: round(got[k][0] / got[k][1], 5) for k in KERNELS if k in got and got[k][1]}
        threaded = n_reads * strands * (RL - K + 1)
        print(json.dumps(dict(line=name, segments=args.segments, seg_len=args.seg_len, read_len=RL, coverage=COV, k=K, strands=strands, span_len=span_len,
                              reads=n_reads, kmers_threaded=threaded, contigs=int(cl.seg_contig_off[-1]), links=links, crossings=crossings, spans=spans,
                              skipped=int(cl.skipped.sum()), launches={k: got[k][1] for k in KERNELS if k in got}, mean_ms=ms,
                              thread_over_score=round(ms["k_read_thread"] / ms["k_score_reads_graph"], 2) if "k_score_reads_graph" in ms else None,
                              ns_per_kmer_threaded=round(ms["k_read_thread"] * 1e6 / threaded, 4),
                              ns_per_read_scored=round(ms["k_score_reads_graph"] * 1e6 / n_reads, 4) if "k_score_reads_graph" in ms else None)), flush=True)
    b.close()


if __name__ == "__main__":
    main()
