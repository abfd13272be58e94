"""What scoring under two breakage tables costs: two single-table calls (A) against one multi-table call (B).

  experiment   the reference's one-segment experiment (tools/bench_workflow.py: 50 kb, 150 bp reads at 50x, k = 31, the
               scaffolds of `--rows` shuffles left on the device), calc_breakscore with Levenshtein + KS:
                 A  calc_breakscore(true) then calc_breakscore(uniform)        B  calc_breakscore_tables([true, uniform])
  batch        configs[2] (100 x 50 kb segments, the reads bench.py builds from), per step:
                 A  build; score(true); score(uniform)      B  build; score_tables([true, uniform])      single  build; score(true)

Host clock around calls that end in a device synchronise (the string API returns host arrays; the batch loop ends in
Context.sync()).  Every line is warmed up, then measured `--reps` times, the lines taking turns inside each repetition so
that drift hits them alike; one JSON line per (case, line) with every repetition and min / median / max.  B's results are
compared bit for bit with A's before anything is timed.

--package-root DIR imports the package from another checkout (the parent commit's, for the baseline): lines that checkout
does not have are left out.  --label goes into every JSON line (the commit the package was built from)."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rows", type=int, default=10000, help="shuffles of the one-segment experiment")
ap.add_argument("--steps", type=int, default=50, help="batch steps per repetition")
ap.add_argument("--cases", default="experiment,batch")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

import numpy as np  # noqa: E402

import genomeassembler_dev_amd as ga  # noqa: E402
from genomeassembler_dev_amd import qtable, synth  # noqa: E402

HAVE_TABLES = hasattr(ga, "calc_breakscore_tables")


def _report(case, line, ms, **extra):
    print(json.dumps(dict(case=case, line=line, label=args.label, package_root=os.path.abspath(args.package_root), reps=len(ms),
                          ms=[round(x, 3) for x in ms], min_ms=round(min(ms), 3), median_ms=round(statistics.median(ms), 3),
                          max_ms=round(max(ms), 3), **extra)), flush=True)


def _take_turns(lines):
    """lines: {name: callable}; every callable args.warmup times, then args.reps rounds of all of them in turn -> {name: [ms]}"""
    for f in lines.values():
        for _ in range(args.warmup):
            f()
    out = {n: [] for n in lines}
    for _ in range(args.reps):
        for n, f in lines.items():
            t0 = time.perf_counter()
            own = f()                   # (a line may time itself: the batch loops leave their first step out)
            out[n].append(own if isinstance(own, float) else (time.perf_counter() - t0) * 1e3)
    return out


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def experiment():
    L, cov, k = 50000, 50, 31
    g = synth.make_segment(1234, L, planted=True)
    reads = [r.tobytes().decode() for r in synth.simulate_reads(g, 150, cov, 1234 + 10000019)]
    truth = g.tobytes().decode()
    keys, true_t, uni_t = qtable.keys(), qtable.load_normalised(), qtable.uniform()
    m = ga.get_contigs_from_reads(reads, k, 1234, matrix_rows=args.rows)
    dv = ga.assemble_contigs(m, k, on_device=True)
    kw = dict(with_lev=True, with_freq=False, with_ks=True)
    lines = {"A": lambda: [ga.calc_breakscore(dv, reads, truth, 8, keys, t, **kw) for t in (true_t, uni_t)]}
    if HAVE_TABLES:
        lines["B"] = lambda: ga.calc_breakscore_tables(dv, reads, truth, 8, keys, [true_t, uni_t], **kw)
        for x, y in zip(lines["A"](), lines["B"]()):
            for name in ("bp_score", "bp_score_norm_by_break_freqs", "bp_score_norm_by_len", "kmer_breaks", "sequence_len", "lev_dist_vs_true", "stat_test_KS"):
                assert _same(x[name], y[name]), name
    res = _take_turns(lines)
    for n, ms in res.items():
        _report("experiment", n, ms, scaffolds=len(dv), scaffold_bases=int(dv.lengths.sum()), reads=len(reads), flags="lev+ks")
    dv.close()


def batch():
    n, L, rl, cov, k = 100, 50000, 150, 50, 31
    reads, seg_off, _ = synth.make_batch(n, L, rl, cov, seed0=1234, planted=True)
    true_t, uni_t = qtable.load_normalised(), qtable.uniform()
    both = np.stack([true_t, uni_t])
    ctx = ga.default_context()
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)

    def loop(step):
        def run():
            # one step outside the clock: the line before left other tables on the device, and a change of tables drains the
            # step slots and uploads — once per repetition for `single` and B, twice per step for A (where it belongs to the step)
            step()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3
        return run
    lines = {"A": loop(lambda: b.build(k, genome_len_hint=L).score(8, true_t).score(8, uni_t)),
             "single": loop(lambda: b.build(k, genome_len_hint=L).score(8, true_t))}
    if HAVE_TABLES:
        lines["B"] = loop(lambda: b.build(k, genome_len_hint=L).score_tables(8, both))
        b.build(k, genome_len_hint=L).score_tables(8, both)
        got = [b.scores(table=t) for t in (0, 1)]
        for t, table in enumerate((true_t, uni_t)):
            b.build(k, genome_len_hint=L).score(8, table)
            want = b.scores()
            for name in want:
                assert _same(got[t][name], want[name]), (t, name)
    res = _take_turns(lines)
    for name, ms in res.items():
        _report("batch_cfg2", name, [x / args.steps for x in ms], unit="ms per step", steps_per_rep=args.steps, segments=n, reads=int(seg_off[-1]),
                kmers=b.total_kmers())
    b.close()


if __name__ == "__main__":
    for c in args.cases.split(","):
        {"experiment": experiment, "batch": batch}[c]()
