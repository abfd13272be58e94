"""Child process of tests/test_strands_gpu.py::test_in_a_child_process (not a test module).

Started with GASM_SINGLE_PASS=0 (every build of the process partitions by count + scan + scatter) or with GASM_PINGPONG=0 (no
step slots: every build on the batch's own stream) in the environment.  Half-flipped fixed-length reads with 64- and 128-bit
keys and a ragged batch are built from both strands, alternating with forward-only builds, scored and checked against the
oracle composition of the parent module.  Prints one JSON verdict line; exits non-zero on any failure."""
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
import test_strands_gpu as T  # noqa: E402


def main():
    verdict = dict(ok=False, env={n: os.environ.get(n) for n in ("GASM_SINGLE_PASS", "GASM_PINGPONG")}, plans={}, failures=[])
    try:
        raw = np.fromfile(os.path.join(ROOT, "genomeassembler_dev_amd", "data", "querytable_raw_f64.bin"), dtype="<f8")
        prob = orc.normalise_tables(raw, [16, 256, 4096, 65536])
        keys = ["".join(t) for k in (2, 4, 6, 8) for t in itertools.product("ACGT", repeat=k)]
        reads, seg_off, segs = T.half_flipped(4000, 80, 20, 610, n_seg=3)
        ragged = T._ragged_segments()
        cases = [("flipped_64", segs, lambda: ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80), 21),
                 ("flipped_128", segs, lambda: ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80), 33),
                 ("ragged_64", ragged, lambda: ga.SegmentBatch.from_strings(ragged), 13)]
        for name, sg, make, k in cases:
            b = make()
            for c, strands in ((2, 2), (1, 1), (1, 2)):
                b.build(k, min_count=c, strands=strands).score(8, prob)
                plan = b.build_plan()
                verdict["plans"][f"{name}/c{c}/s{strands}"] = {n: v for n, v in plan.items() if n != "blocks"}
                try:
                    T.check_segments(b, sg, k, c, strands, keys, prob)
                except AssertionError as e:
                    verdict["failures"].append(f"{name} min_count {c} strands {strands}: {e}")
            b.close()
        verdict["ok"] = not verdict["failures"]
    except Exception:
        verdict["failures"].append(traceback.format_exc()[-2000:])
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
