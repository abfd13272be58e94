"""Child process of tests/test_build_paths_gpu.py::test_process_wide_knobs_in_child_processes (not a test module).

The Knobs of pipeline.hip (GASM_RANK_GLOBAL, GASM_RULER_SHIFT, GASM_DEDUP_TBL, GASM_SCATTER_WGS,
GASM_HIST_WGS) are read once per process, so each set runs here in a fresh process, from the environment it was started
with.  A fixed set of small batches — 64- and 128-bit keys, more than 64 segments, ragged reads with an empty segment, a
4096-slot-table build and a two-pass partition — is built and checked against the oracle (contigs, distinct k-mers and
multiplicities of every segment), and each plan against what the knobs must show.  Prints one JSON verdict line; exits
non-zero on any failure."""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import genomeassembler_dev_amd as ga  # noqa: E402
from genomeassembler_dev_amd import synth  # noqa: E402
from oracle import orc  # noqa: E402

KNOBS = ("GASM_RANK_GLOBAL", "GASM_RULER_SHIFT", "GASM_DEDUP_TBL", "GASM_SCAN_IN_DEDUP", "GASM_SCATTER_WGS",
         "GASM_HIST_WGS")


def _strs(a):
    return [r.tobytes().decode() for r in a]


def _cases():
    """(name, segments as read strings, batch factory, k, hint, per-build environment)"""
    out = []
    for name, (n, L, rl, cov, k, hint, seed) in {"many_64": (70, 1000, 50, 12, 21, 1000, 500),
                                                 "wide_128": (5, 2500, 80, 12, 33, 2500, 510),
                                                 "tbl4096_64": (2, 2500, 60, 12, 21, 1_000_000, 520)}.items():
        reads, seg_off, _g = synth.make_batch(n, L, rl, cov, seed0=seed, planted=True)
        segs = [_strs(reads[int(seg_off[s]):int(seg_off[s + 1])]) for s in range(n)]
        make = (lambda r=reads, so=seg_off, rl=rl: ga.SegmentBatch(r.reshape(-1), so, fixed_len=rl))
        out.append((name, segs, make, k, hint, {}))
        if name == "many_64":        # the count + scan + scatter partition (k_tile_hist: GASM_HIST_WGS)
            out.append(("two_pass_64", segs, make, k, hint, {"GASM_SINGLE_PASS": "0"}))
    rng = np.random.default_rng(530)
    g = _strs(synth.make_segment(531, 2000, planted=False)[None, :])[0]
    ragged = [[g[a:a + int(rng.integers(8, 70))] for a in rng.integers(0, 1930, 250)], [], ["ACGTTGCA", "AC"]]
    out.append(("ragged_64", ragged, lambda: ga.SegmentBatch.from_strings(ragged), 13, 0, {}))
    return out


def _expect(plan, name, env, local):
    """what the knobs must show in a plan; returns a list of failures"""
    bad = []

    def want(field, value):
        if plan[field] != value:
            bad.append(f"{name}: {field} = {plan[field]}, the knobs say {value}")
    if env.get("GASM_RANK_GLOBAL"):
        want("ranked_in_lds", 0), want("rank_global", 1), want("ruler_shift", 0)
    else:
        want("ranked_in_lds", 1), want("rank_global", 0)
        if env.get("GASM_RULER_SHIFT"):
            want("ruler_shift", min(4, int(env["GASM_RULER_SHIFT"])))
    if plan["distinct_attempts"] == 1:
        if plan["key_words"] == 2:
            want("table_slots", 2048)
        elif env.get("GASM_DEDUP_TBL"):
            want("table_slots", int(env["GASM_DEDUP_TBL"]))
        else:
            want("table_slots", 4096 if name == "tbl4096_64" else 2048)
    if env.get("GASM_SCAN_IN_DEDUP") == "0":
        want("scan_in_dedup", 0)
    if local.get("GASM_SINGLE_PASS") == "0":
        want("single_pass", 0)
    return bad


def main():
    env = {n: os.environ[n] for n in KNOBS if n in os.environ}
    verdict = dict(ok=False, knobs=env, plans={}, failures=[])
    try:
        for name, segs, make, k, hint, local in _cases():
            os.environ.update(local)
            try:
                b = make()
                b.build(k, genome_len_hint=hint)
                plan = b.build_plan()
                contigs = b.contigs()
                verdict["plans"][name] = {n: v for n, v in plan.items() if n != "blocks"}
                verdict["failures"] += _expect(plan, name, env, local)
                for s, rs in enumerate(segs):
                    ref = orc.get_contigs(orc.kmers_from_reads(rs, k), k, 1, rows=1)
                    dk, dm = b.distinct_kmers(s)
                    if contigs[s] != ref["contigs"]:
                        verdict["failures"].append(f"{name}: segment {s}: contigs differ from the oracle")
                    if dk != ref["distinct"] or dm.tolist() != ref["counts"].tolist():
                        verdict["failures"].append(f"{name}: segment {s}: k-mer counts differ from the oracle")
                b.close()
            finally:
                for n in local:
                    del os.environ[n]
        verdict["ok"] = not verdict["failures"]
    except Exception:
        verdict["failures"].append(traceback.format_exc()[-2000:])
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
