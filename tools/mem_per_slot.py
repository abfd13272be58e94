"""Device memory a cfg2 batch takes with 1, 2, 3 step slots (hipMemGetInfo around the first steps).
usage: python tools/mem_per_slot.py [--strands 2] [--tips R]
    --strands 2: both-strand builds, build(k, strands=2)
    --tips R:    R rounds of tip clipping, build_tips(k, tip_len=2k-1, tip_rounds=R) (a slot grows by its counters, 64 bytes a segment)"""
import os
import subprocess
import sys


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


STRANDS = 2 if opt("--strands", 1) == 2 else 1
TIPS = opt("--tips", 0)
if len(sys.argv) > 1 and sys.argv[1].isdigit():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import genomeassembler_dev_amd as ga
    from genomeassembler_dev_amd import qtable, synth
    reads, seg_off, _g = synth.make_batch(100, 50000, 150, 50, seed0=1234, planted=True)
    ctx = ga.default_context()
    free0 = torch.cuda.mem_get_info()[0]
    b = ga.SegmentBatch.from_packed(synth.pack_2bit(reads), seg_off, fixed_len=150, ctx=ctx)
    table = qtable.load_normalised()
    for _ in range(6):
        if TIPS:
            b.build_tips(31, genome_len_hint=50000, strands=STRANDS, tip_len=61, tip_rounds=TIPS).score(8, table)
        else:
            b.build(31, genome_len_hint=50000, strands=STRANDS).score(8, table)
    b.distinct()
    ctx.sync()
    used = free0 - torch.cuda.mem_get_info()[0]
    print(f"strands={STRANDS} tips={TIPS} slots={sys.argv[1]} pingpong={os.environ.get('GASM_PINGPONG', '1')}: {used / 2**30:.2f} GiB ({used} bytes)")
else:
    for pp, n in (("0", "1"), ("1", "2"), ("1", "3")):
        env = dict(os.environ, GASM_PINGPONG=pp, GASM_STEP_SLOTS=n)
        subprocess.run([sys.executable, __file__, n, "--strands", str(STRANDS), "--tips", str(TIPS)], env=env, check=True)
