"""Child process of tests/test_bubbles_gpu.py::test_in_a_child_process (not a test module).

Started with GASM_RANK_GLOBAL=1 (whole-GPU list ranking in every graph pass), GASM_PINGPONG=0 (no step slots) or
GASM_SINGLE_PASS=0 (the two-pass partition) in the environment.  Noisy reads with 64- and 128-bit keys are built with tips and
bubbles, with bubbles alone, with tips alone and with neither in turn, scored, and checked against the restatement through the
parent module's check_segments.  Then steps are queued back to back with no fetch in between (unfetched_steps): without step
slots that is one BuildState and one stream, where every build abandons the queued one before it — its rounds of either kind,
its compactions and the repeat it may still have needed (one of the steps carries a hint that makes its first attempt fail).
Prints one JSON verdict line; exits non-zero on any failure."""
import itertools
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import genomeassembler_dev_amd as ga  # noqa: E402
from oracle import orc  # noqa: E402
import test_bubbles_gpu as T  # noqa: E402


# min_count, strands, tip_len, tip_rounds, bubble_len, bubble_rounds, genome_len_hint.  The hint of 50 is far too small: the first
# attempt of that step fails (its tables overflow), and where the step is abandoned nobody reads that.  The plans of the steps
# built alone are in the verdict
STEPS = [(2, 2, 41, 2, 41, 2, 0), (2, 2, 41, 2, 0, 1, 0), (2, 1, 0, 1, 41, 1, 0), (2, 2, 41, 1, 41, 3, 50), (2, 2, 0, 1, 0, 1, 0),
         (2, 2, 41, 2, 41, 2, 0)]


def unfetched_steps(verdict, keys, prob):
    """builds with mixed (tip_len, bubble_len), each scored, and only then a fetch: every fetch matches the last build as if it had
    run alone, whatever the builds before it left queued"""
    reads, seg_off, segs = T.noisy_batch(4000, 80, 20, 5, 2, n_seg=2)

    def step(b, c, st, tl, tr_, bl, br_, hint):
        b.build_bubbles(21, genome_len_hint=hint, min_count=c, strands=st, tip_len=tl, tip_rounds=tr_, bubble_len=bl, bubble_rounds=br_).score(8, prob)

    alone = {}
    for s in set(STEPS):
        b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
        step(b, *s)
        alone[s] = T._all_fetches(b)
        verdict["plans"]["alone/" + "/".join(map(str, s))] = {n: v for n, v in b.build_plan().items() if n != "blocks"}
        b.close()
    assert alone[STEPS[0]] != alone[STEPS[1]] != alone[STEPS[2]]
    b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80)
    for upto in range(1, len(STEPS) + 1):
        for s in STEPS[:upto]:
            step(b, *s)
        if T._all_fetches(b) != alone[STEPS[upto - 1]]:
            verdict["failures"].append(f"unfetched steps: after {STEPS[:upto]} the fetches are not those of the last step built alone")
    c, st, tl, tr_, bl, br_, _ = STEPS[-1]
    try:
        T.check_segments(b, segs, 21, c, st, (tl, tr_), (bl, br_), keys, prob)
    except AssertionError as e:
        verdict["failures"].append(f"unfetched steps, the last against the restatement: {e}")
    b.close()


def main():
    names = ("GASM_RANK_GLOBAL", "GASM_PINGPONG", "GASM_SINGLE_PASS")
    verdict = dict(ok=False, env={n: os.environ.get(n) for n in names}, plans={}, failures=[])
    try:
        raw = np.fromfile(os.path.join(ROOT, "genomeassembler_dev_amd", "data", "querytable_raw_f64.bin"), dtype="<f8")
        prob = orc.normalise_tables(raw, [16, 256, 4096, 65536])
        keys = ["".join(t) for k in (2, 4, 6, 8) for t in itertools.product("ACGT", repeat=k)]
        for k, rl in ((21, 80), (41, 100)):
            reads, seg_off, segs = T.noisy_batch(5000, rl, 20, 600 + k, 2, n_seg=2)
            b = ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=rl)
            for c, strands, tip, bub in ((2, 2, (2 * k - 1, 2), (2 * k - 1, 2)), (2, 1, (0, 0), (2 * k - 1, 1)), (2, 2, (2 * k - 1, 1), (0, 0)),
                                         (1, 1, (0, 0), (0, 0)), (2, 2, (2 * k - 1, 1), (2 * k - 1, 3))):
                b.build_bubbles(k, min_count=c, strands=strands, tip_len=tip[0], tip_rounds=tip[1] or 1, bubble_len=bub[0],
                                bubble_rounds=bub[1] or 1).score(8, prob)
                plan = b.build_plan()
                verdict["plans"][f"k{k}/c{c}/s{strands}/t{tip[0]}x{tip[1]}/b{bub[0]}x{bub[1]}"] = {n: v for n, v in plan.items() if n != "blocks"}
                try:
                    T.check_segments(b, segs, k, c, strands, tip, bub, keys, prob)
                except AssertionError as e:
                    verdict["failures"].append(f"k {k} min_count {c} strands {strands} tips {tip} bubbles {bub}: {e}")
            b.close()
        unfetched_steps(verdict, keys, prob)
        verdict["ok"] = not verdict["failures"]
    except Exception:
        verdict["failures"].append(traceback.format_exc()[-2000:])
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
