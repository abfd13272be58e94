"""What low-coverage removal (build_simplified(k, ..., cov_cutoff=, cov_len=, cov_rounds=)) and the per-contig coverage pass
(contig_coverage()) cost on configs[2]-shaped batches, parent commit and this one in one call.

Workload: 100 x 50 kb segments, 150-base reads at 50x with 1 % substitutions, k = 31, min_count = 2.  Lines, each
`build; score` per step (tips: tip_len = 2k - 1, two rounds; bubbles: bubble_len = 2k - 1, two rounds; low coverage: cov_len =
2k - 1, cov_cutoff = min_count + 1):
  plain        no tips, no bubbles                          both checkouts
  tips         tips only                                    both checkouts
  bubbles      tips, then bubbles                           both checkouts (the parent's build_bubbles; here build_simplified(cov_cutoff=0))
  bubbles_c1   tips, bubbles, one low-coverage round        this checkout
  bubbles_c2   tips, bubbles, two low-coverage rounds       this checkout
  c1           one low-coverage round alone                 this checkout
So a round's cost is bubbles_c1 - bubbles (or bubbles_c2 - bubbles_c1, or c1 - plain), and `plain` / `tips` / `bubbles` on both
checkouts say whether cov_cutoff = 0 still costs what the parent's build costs.

The driver writes the reads to a scratch directory once and starts one worker process per checkout (--parent-root, and this
one); the workers keep their batches on the device and the driver asks them for one repetition of one line at a time, parent
and new taking turns inside every repetition, so drift hits both alike.  A repetition is `--steps` steps between two
synchronisations, host clock, the first step outside it.  One JSON line per (checkout, line): every repetition, min /
median / max.  Then one JSON line per (checkout, line) with the kernels' own durations (gasm_profile_read, one step in
flight: GASM_PINGPONG=0), the build plan, the round statistics and the sizes of the result.  Last, this checkout alone:
k_contig_cov's own duration (HIP events around the kernel, 10 launches each) over a plain build of the CLEAN reads of the same
shape (few long contigs: every lane of a wave adds to the same contig) and over a plain min_count = 2 build of the noisy reads
(many short contigs).

  python tools/bench_lowcov.py --parent-root /path/to/parent/checkout        (built: its libgasm.so must exist)"""
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

L, RL, COV, K, MIN_COUNT, RATE = 50000, 150, 50, 31, 2, 0.01
LINES = {"plain": (0, 0, 0), "tips": (2, 0, 0), "bubbles": (2, 2, 0), "bubbles_c1": (2, 2, 1), "bubbles_c2": (2, 2, 2), "c1": (0, 0, 1)}   # (tip, bubble, low-coverage rounds)


def worker():
    sys.path.insert(0, os.path.abspath(args.package_root))
    import numpy as np

    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import qtable
    lowcov = hasattr(ga.SegmentBatch, "build_simplified")
    table = qtable.load_normalised()
    seg_off = np.load(os.path.join(args.worker, "seg_off.npy"))
    ctx = ga.default_context()
    b = ga.SegmentBatch(np.load(os.path.join(args.worker, "noisy.npy")).reshape(-1), seg_off, fixed_len=RL)

    def step(rounds):
        tr_, br_, cr_ = rounds
        tl, bl = (2 * K - 1 if tr_ else 0), (2 * K - 1 if br_ else 0)
        if not lowcov:
            return lambda: b.build_bubbles(K, genome_len_hint=L, min_count=MIN_COUNT, tip_len=tl, tip_rounds=tr_ or 1, bubble_len=bl,
                                           bubble_rounds=br_ or 1).score(8, table)
        return lambda: b.build_simplified(K, genome_len_hint=L, min_count=MIN_COUNT, tip_len=tl, tip_rounds=tr_ or 1, bubble_len=bl, bubble_rounds=br_ or 1,
                                          cov_cutoff=MIN_COUNT + 1 if cr_ else 0, cov_len=2 * K - 1, cov_rounds=cr_ or 1).score(8, table)

    print(json.dumps(dict(ready=True, lowcov=lowcov)), flush=True)
    for cmd in sys.stdin:
        what, line = cmd.split()
        if what == "quit":
            break
        if what == "coverage":
            print(json.dumps(coverage_times(ga, ctx, b, seg_off)), flush=True)
            continue
        if LINES[line][2] and not lowcov:
            print(json.dumps(dict(skip=True)), flush=True)
            continue
        f = step(LINES[line])
        if what == "rep":
            f()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f()
            ctx.sync()
            print(json.dumps(dict(ms=(time.perf_counter() - t0) * 1e3 / args.steps)), flush=True)
        else:                       # "kernels": one step in flight, every launch on the batch's own context
            os.environ["GASM_PINGPONG"] = "0"
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
            if LINES[line][0]:
                t, km = b.tip_stats()
                extra.update(tips_per_round=t.sum(axis=0).tolist(), tip_kmers_per_round=km.sum(axis=0).tolist())
            if LINES[line][1]:
                t, km = b.bubble_stats()
                extra.update(bubbles_per_round=t.sum(axis=0).tolist(), bubble_kmers_per_round=km.sum(axis=0).tolist())
            if LINES[line][2]:
                t, km = b.lowcov_stats()
                extra.update(lowcov_per_round=t.sum(axis=0).tolist(), lowcov_kmers_per_round=km.sum(axis=0).tolist())
            print(json.dumps(dict(kernels={k: [round(v[0] / n, 5), v[1] / n] for k, v in sorted(got.items()) if v[1]}, **extra)), flush=True)
    b.close()


def coverage_times(ga, ctx, noisy, seg_off):
    """k_contig_cov alone over a plain build of the clean reads and a min_count = 2 build of the noisy ones: mean ms of 10 launches"""
    import numpy as np
    out = {}
    clean = ga.SegmentBatch(np.load(os.path.join(args.worker, "clean.npy")).reshape(-1), seg_off, fixed_len=RL)
    for name, b, c in (("clean", clean, 1), ("noisy", noisy, MIN_COUNT)):
        os.environ["GASM_PINGPONG"] = "0"
        b.build(K, genome_len_hint=L, min_count=c)
        b.contig_coverage()
        ctx.sync()
        ctx.profile(True, only=["k_contig_cov"])
        ctx.profile_reset()
        for _ in range(10):
            ms, ns = b.contig_coverage()
        got = ctx.profile_read()
        ctx.profile(False)
        del os.environ["GASM_PINGPONG"]
        out[name] = dict(k_contig_cov_ms=round(got["k_contig_cov"][0] / got["k_contig_cov"][1], 5), launches=got["k_contig_cov"][1], contigs=len(ns),
                         edges=int(ns.sum()), longest_contig_edges=int(ns.max()) if len(ns) else 0)
    clean.close()
    return dict(coverage=out)


class Worker:
    def __init__(self, root, data):
        self.root = os.path.abspath(root)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", data, "--package-root", self.root, "--steps", str(args.steps)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self.lowcov = self.ask(None)["lowcov"]

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
        # 1 % substitutions: a mask, then a shift of 1..3 mod 4 in ACGT
        rng = np.random.default_rng(1235)
        lut = np.frombuffer(b"ACGT", dtype=np.uint8)
        code = np.zeros(256, dtype=np.uint8)
        code[lut] = np.arange(4, dtype=np.uint8)
        mask = rng.random(reads.shape) < RATE
        shift = rng.integers(1, 4, reads.shape).astype(np.uint8)
        np.save(os.path.join(data, "clean.npy"), reads)
        reads = np.where(mask, lut[(code[reads] + shift) & 3], reads).astype(np.uint8)
        np.save(os.path.join(data, "noisy.npy"), reads)
        np.save(os.path.join(data, "seg_off.npy"), seg_off)
        del reads, mask, shift
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
            print(json.dumps(dict(checkout="new", label=args.label, **workers["new"].ask("coverage -"))), flush=True)
        finally:
            for wk in workers.values():
                wk.close()


if __name__ == "__main__":
    worker() if args.worker else driver()
