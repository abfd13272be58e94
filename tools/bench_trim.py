"""What quality trimming at ingest costs (gasm_read_files_device_params: k_ing_qual_trim, one wave per FASTQ record) on configs[2]-shaped
files, next to k_ing_lines of the same ingest, which reads the same bytes with one thread per line.

Workload: one FASTQ file per segment, 20 segments of 50 kb, 150-base reads at 50x with synth.simulate_qualities qualities and errors where
they say (synth.apply_quality_errors), written to a temporary directory.  Measured:
  kernels   k_ing_lines and k_ing_qual_trim (and k_ing_trim_fold) by HIP events (gasm_profile_read), mean per launch (= per file) over --reps
            ingests at trim_q3 = 20 after --warmup, and the bytes per second each makes of a file's text; the same with quality_hist
  whole     wall time of seqio.read_files_device(paths) without options, with trim_q3 = 20, min_len = 31, quality_hist, and with parts of
            these (no histogram; the histogram alone; min_len alone, which reads no text): min and mean over --reps
  host      host_probe: the host reader over the same files and a 100 MB numpy copy in the same process, min of 3 / 5: what the process's
            host side does apart from the device path (the whole-call figures are mostly host work)
One JSON line.

--plain-only measures the option-free ingest alone and needs none of the new entries: with --root pointing at a checkout of the parent
commit (built), that is the parent's figure, to hold against this tree's all-zero-options ingest.

  python tools/bench_trim.py [--segments 20] [--reps 10] [--plain-only] [--root DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--segments", type=int, default=20)
ap.add_argument("--seg-len", type=int, default=50000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()

RL, COV = 150, 50
KERNELS = ["k_ing_lines", "k_ing_qual_trim", "k_ing_trim_fold"]
TRIM = dict(trim_q3=20, min_len=31, quality_hist=True)


def write_fastq(path, reads, quals):
    """(tools/ runs against the parent's package too, which has no synth.write_fastq)"""
    import numpy as np
    n, rl = reads.shape
    name = np.frombuffer(b"@r\n", np.uint8)
    rec = np.concatenate([np.broadcast_to(name, (n, 3)), reads, np.broadcast_to(np.frombuffer(b"\n+\n", np.uint8), (n, 3)),
                          (quals + 33).astype(np.uint8), np.full((n, 1), 10, np.uint8)], axis=1)
    rec.tofile(path)


def qualities(np, n, rl, seed):
    """synth.simulate_qualities with its defaults, restated so that --root may point at a tree without it"""
    rng = np.random.Generator(np.random.MT19937(seed))
    tail = max(1, int(round(rl * 0.3)))
    prof = np.full(rl, 38.0)
    prof[rl - tail:] = np.linspace(38, 12, tail + 1)[1:]
    q = np.rint(prof)[None, :].astype(np.int64) + rng.integers(-3, 4, size=(n, 1)) + rng.integers(-2, 3, size=(n, rl))
    return np.clip(q, 2, 41)


def main():
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np

    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import seqio, synth
    ctx = ga.default_context()
    with tempfile.TemporaryDirectory() as d:
        paths, n_reads, n_bytes = [], 0, 0
        for s in range(args.segments):
            g = synth.make_segment(1234 + s, args.seg_len, planted=True)
            reads = synth.simulate_reads(g, RL, COV, 10_000_019 + 1234 + s)
            q = qualities(np, reads.shape[0], RL, 99 + s)
            rng = np.random.Generator(np.random.MT19937(7 + s))
            err = rng.random(reads.shape) < 10.0 ** (-q / 10.0)
            code = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), reads)
            reads = np.where(err, np.frombuffer(b"ACGT", np.uint8)[(code + rng.integers(1, 4, size=reads.shape)) % 4], reads).astype(np.uint8)
            p = os.path.join(d, f"seg{s:02d}.fastq")
            write_fastq(p, reads, q)
            paths.append(p)
            n_reads += reads.shape[0]
            n_bytes += os.path.getsize(p)

        def wall(**opts):
            ts = []
            for i in range(args.warmup + args.reps):
                ctx.sync()
                t0 = time.perf_counter()
                seqio.read_files_device(paths, **opts)
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = ts[args.warmup:]
            return dict(min_ms=round(min(ts), 3), mean_ms=round(sum(ts) / len(ts), 3))
        def host_probe():
            """how fast this process's host side is, apart from the ingest: the host reader over the same files (no GPU), and a 100 MB copy"""
            big = np.ones(100_000_000 // 8)
            ts, th = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                big.copy()
                ts.append((time.perf_counter() - t0) * 1e3)
            for _ in range(3):
                t0 = time.perf_counter()
                seqio.read_files(paths)
                th.append((time.perf_counter() - t0) * 1e3)
            return dict(copy_100mb_min_ms=round(min(ts), 3), host_reader_min_ms=round(min(th), 3), cpus=len(os.sched_getaffinity(0)))
        out = dict(segments=args.segments, seg_len=args.seg_len, read_len=RL, coverage=COV, reads=n_reads, text_bytes=n_bytes, reps=args.reps,
                   whole_plain=wall(), host_probe=host_probe())
        if not args.plain_only:
            out["whole_trim"] = wall(**TRIM)
            out["whole_trim_no_hist"] = wall(trim_q3=20, min_len=31)
            out["whole_hist_only"] = wall(quality_hist=True)
            out["whole_min_len_only"] = wall(min_len=31)
            out["trim_options"] = TRIM
            per_file = n_bytes / args.segments
            for key, opts in (("", dict(trim_q3=20)), ("_hist", dict(trim_q3=20, quality_hist=True))):
                for _ in range(args.warmup):
                    seqio.read_files_device(paths, **opts)
                ctx.profile(True, only=KERNELS)
                ctx.profile_reset()
                for _ in range(args.reps):
                    r = seqio.read_files_device(paths, **opts)
                got = ctx.profile_read()
                ctx.profile(False)
                out["mean_ms_per_file" + key] = {k: round(got[k][0] / got[k][1], 5) for k in KERNELS if k in got and got[k][1]}
                if not key:
                    res = r
                    out["launches"] = {k: got[k][1] for k in KERNELS if k in got}
                    out["text_gb_per_s"] = {k: round(per_file / (v * 1e-3) / 1e9, 2) for k, v in out["mean_ms_per_file"].items() if k != "k_ing_trim_fold"}
            st = res[-1]
            out["trim_q3_20"] = dict(kept=int(st.kept.sum()), bases_in=int(st.bases_in.sum()), trimmed3=int(st.trimmed3.sum()), reads_trimmed=int(st.reads_trimmed.sum()))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
