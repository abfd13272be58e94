"""Child process of tests/test_solid_kmers_gpu.py::test_two_pass_partition_in_child_process (not a test module).

Started with GASM_SINGLE_PASS=0 in the environment: every build of the process partitions by count + scan + scatter, and the
multiplicity cutoff (min_count = 2) runs behind the de-duplication of that path.  Noisy fixed-length reads with 64- and
128-bit keys and a ragged batch are built, scored and checked against the oracle composition of the parent module.  Prints
one JSON verdict line; exits non-zero on any failure."""
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
from genomeassembler_dev_amd import synth  # noqa: E402
from oracle import orc  # noqa: E402
import test_solid_kmers_gpu as T  # noqa: E402


def main():
    verdict = dict(ok=False, single_pass_env=os.environ.get("GASM_SINGLE_PASS"), plans={}, failures=[])
    try:
        raw = np.fromfile(os.path.join(ROOT, "genomeassembler_dev_amd", "data", "querytable_raw_f64.bin"), dtype="<f8")
        prob = orc.normalise_tables(raw, [16, 256, 4096, 65536])
        keys = ["".join(t) for k in (2, 4, 6, 8) for t in itertools.product("ACGT", repeat=k)]
        reads, seg_off, _ = synth.make_batch(3, 4000, 80, 20, seed0=610)
        reads = T.noisy(reads, 0.01, 610)
        segs = [T._strs(reads[int(seg_off[s]):int(seg_off[s + 1])]) for s in range(3)]
        rng = np.random.default_rng(611)
        g = T._strs(synth.make_segment(612, 2000, planted=False)[None, :])[0]
        ragged = [[g[a:a + int(rng.integers(8, 70))] for a in rng.integers(0, 1930, 900)], [], ["ACGTTGCA", "AC"]]
        cases = [("noisy_64", segs, lambda: ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80), 21),
                 ("noisy_128", segs, lambda: ga.SegmentBatch(reads.reshape(-1), seg_off, fixed_len=80), 33),
                 ("ragged_64", ragged, lambda: ga.SegmentBatch.from_strings(ragged), 13)]
        for name, sg, make, k in cases:
            b = make()
            b.build(k, min_count=2).score(8, prob)
            plan = b.build_plan()
            verdict["plans"][name] = {n: v for n, v in plan.items() if n != "blocks"}
            try:
                T.check_segments(b, sg, k, 2, keys, prob)
            except AssertionError as e:
                verdict["failures"].append(f"{name}: {e}")
            b.close()
        verdict["ok"] = not verdict["failures"]
    except Exception:
        verdict["failures"].append(traceback.format_exc()[-2000:])
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
