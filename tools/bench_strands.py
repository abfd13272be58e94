"""What a both-strand build (build(k, strands=2)) costs on configs[2]'s batch, parent commit and this one in one call.

Workload: 100 x 50 kb segments, 150-base reads at 50x, k = 31 (what bench.py builds from), and the same reads with a random
half reverse-complemented.  Lines, each `build; score` per step:
  plain_s1, flipped_s1    strands = 1                                             both checkouts
  plain_s2, flipped_s2    strands = 2                                             this checkout

The driver writes the reads to a scratch directory once and starts one worker process per checkout (--package-root of the
parent, and this one); the workers keep their batches on the device and the driver asks them for one repetition of one line
at a time, parent and new taking turns inside every repetition, so drift hits both alike.  A repetition is `--steps` steps
between two synchronisations, host clock, the first step outside it.  One JSON line per (checkout, line): every
repetition, min / median / max.  Then, one JSON line each:
  the kernels' own durations (gasm_profile_read, one step in flight: GASM_PINGPONG=0) of every line; the strands = 2 lines
  fetch the twin map in every step, so k_contig_twin is among them (hold it against k_score_zero + k_score_finish);
  k_reads_both_strands on a fresh batch (it runs once per upload) beside device-to-device copies of the packed stream (its
  input) and of twice that (its output), timed with events in the same process.

  python tools/bench_strands.py --parent-root /path/to/parent/checkout        (built: its libgasm.so must exist)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit (left out: this checkout alone)")
ap.add_argument("--package-root", default=ROOT)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--segments", type=int, default=100)
ap.add_argument("--worker", default="", help="(internal) directory with the reads: serve repetitions on stdin / stdout")
ap.add_argument("--label", default="")
args = ap.parse_args()

L, RL, COV, K = 50000, 150, 50, 31
LINES = {"plain_s1": ("plain", 1), "plain_s2": ("plain", 2), "flipped_s1": ("flipped", 1), "flipped_s2": ("flipped", 2)}


def worker():
    sys.path.insert(0, os.path.abspath(args.package_root))
    import inspect

    import numpy as np

    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import qtable
    both = "strands" in inspect.signature(ga.SegmentBatch.build).parameters
    table = qtable.load_normalised()
    seg_off = np.load(os.path.join(args.worker, "seg_off.npy"))
    ctx = ga.default_context()
    batches = {n: ga.SegmentBatch(np.load(os.path.join(args.worker, n + ".npy")).reshape(-1), seg_off, fixed_len=RL) for n in ("plain", "flipped")}

    def step(b, s, twins=False):
        if not both:
            return lambda: b.build(K, genome_len_hint=L).score(8, table)
        if twins and s == 2:
            return lambda: (b.build(K, genome_len_hint=L, strands=s).score(8, table), b.contig_twins())
        return lambda: b.build(K, genome_len_hint=L, strands=s).score(8, table)

    print(json.dumps(dict(ready=True, both=both)), flush=True)
    for cmd in sys.stdin:
        what, line = cmd.split()
        if what == "quit":
            break
        if what == "rc":
            # the reverse-complement kernel on a fresh batch (once per upload), and copies of its input and output sizes
            import torch
            os.environ["GASM_PINGPONG"] = "0"
            b = ga.SegmentBatch(np.load(os.path.join(args.worker, "flipped.npy")).reshape(-1), seg_off, fixed_len=RL)
            ctx.profile(True)
            ctx.profile_reset()
            b.build(K, genome_len_hint=L, strands=2)
            ctx.sync()
            got = ctx.profile_read()
            ctx.profile(False)
            del os.environ["GASM_PINGPONG"]
            n_bytes = (int(seg_off[-1]) * RL + 31) // 32 * 8
            out = dict(k_reads_both_strands_ms=round(got["k_reads_both_strands"][0], 5), stream_bytes=n_bytes)
            for name, n in (("copy_input_size_ms", n_bytes), ("copy_output_size_ms", 2 * n_bytes)):
                src, dst = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
                best = []
                for _ in range(12):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    dst.copy_(src)
                    e1.record()
                    e1.synchronize()
                    best.append(e0.elapsed_time(e1))
                out[name] = round(min(best[2:]), 5)
            b.close()
            print(json.dumps(dict(rc=out)), flush=True)
            continue
        if LINES[line][1] > 1 and not both:
            print(json.dumps(dict(skip=True)), flush=True)
            continue
        b = batches[LINES[line][0]]
        if what == "rep":
            f = step(b, LINES[line][1])
            f()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f()
            ctx.sync()
            print(json.dumps(dict(ms=(time.perf_counter() - t0) * 1e3 / args.steps)), flush=True)
        else:                       # "kernels": one step in flight, every launch on the batch's own context
            os.environ["GASM_PINGPONG"] = "0"
            f = step(b, LINES[line][1], twins=True)
            f()
            ctx.sync()
            ctx.profile(True)
            ctx.profile_reset()
            n = 10
            for _ in range(n):
                f()
                ctx.sync()
            got = ctx.profile_read()
            ctx.profile(False)
            del os.environ["GASM_PINGPONG"]
            extra = dict(plan={k: v for k, v in b.build_plan().items() if k != "blocks"}, total_kmers=b.total_kmers(), distinct=int(b.distinct()[0][-1]),
                         contigs=int(b.contigs_raw()[0][-1]))
            print(json.dumps(dict(kernels={k: [round(v[0] / n, 5), v[1] / n] for k, v in sorted(got.items()) if v[1]}, **extra)), flush=True)
    for b in batches.values():
        b.close()


class Worker:
    def __init__(self, root, data):
        self.root = os.path.abspath(root)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", data, "--package-root", self.root, "--steps", str(args.steps)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self.both = self.ask(None)["both"]

    def ask(self, cmd):
        if cmd:
            self.p.stdin.write(cmd + "\n")
            self.p.stdin.flush()
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError(f"the worker of {self.root} ended (exit status {self.p.poll()})")
            if line.startswith("{"):
                return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write("quit -\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=120)


def driver():
    sys.path.insert(0, os.path.abspath(args.package_root))
    import numpy as np

    from genomeassembler_dev_amd import synth
    with tempfile.TemporaryDirectory() as data:
        reads, seg_off, _ = synth.make_batch(args.segments, L, RL, COV, seed0=1234, planted=True)
        np.save(os.path.join(data, "plain.npy"), reads)
        comp = np.zeros(256, dtype=np.uint8)
        comp[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)
        m = np.random.default_rng(1234).random(reads.shape[0]) < 0.5
        reads[m] = comp[reads[m][:, ::-1]]
        np.save(os.path.join(data, "flipped.npy"), reads)
        np.save(os.path.join(data, "seg_off.npy"), seg_off)
        del reads, m
        workers = {}
        if args.parent_root:
            workers["parent"] = Worker(args.parent_root, data)
        workers["new"] = Worker(args.package_root, data)
        try:
            ms = {(w, n): [] for w in workers for n in LINES}
            for r in range(args.warmup + args.reps):
                for n in LINES:
                    for w, wk in workers.items():
                        got = wk.ask(f"rep {n}")
                        if "ms" in got and r >= args.warmup:
                            ms[(w, n)].append(got["ms"])
            for (w, n), v in ms.items():
                if v:
                    print(json.dumps(dict(checkout=w, line=n, label=args.label, unit="ms per step (build; score)", steps_per_rep=args.steps, reps=len(v),
                                          ms=[round(x, 4) for x in v], min_ms=round(min(v), 4), median_ms=round(statistics.median(v), 4),
                                          max_ms=round(max(v), 4))), flush=True)
            for n in LINES:
                for w, wk in workers.items():
                    got = wk.ask(f"kernels {n}")
                    if "kernels" in got:
                        print(json.dumps(dict(checkout=w, line=n, label=args.label, one_step_in_flight=True, **got)), flush=True)
            print(json.dumps(dict(checkout="new", label=args.label, **workers["new"].ask("rc -"))), flush=True)
        finally:
            for wk in workers.values():
                wk.close()


if __name__ == "__main__":
    worker() if args.worker else driver()
