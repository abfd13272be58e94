"""CPU-side checks: the C-ABI library loads and exports every symbol include/gasm.h declares; host-side algorithms of
the boundary (shuffle, greedy merge, Levenshtein, table normalisation) agree with the oracle.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
from genomeassembler_dev_amd import _lib, qtable
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "gasm.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(gasm_[a-z_0-9]+)\s*\(", hdr))
    assert len(declared) > 40
    L = _lib.lib()
    for name in sorted(declared):
        assert hasattr(L, name), f"libgasm.so does not export {name}"
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    assert b"gfx950" in L.gasm_version()


def test_build_plan_fields_match_the_header():
    """SegmentBatch.build_plan names the words of a gasm_batch_build_plan row in the order of the GASM_PLAN_* indices"""
    hdr = open(os.path.join(ROOT, "include", "gasm.h")).read()
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define GASM_PLAN_([A-Z_]+)\s+(\d+)", hdr)}
    n = idx.pop("fields")
    assert n == len(_lib.PLAN_FIELDS) and sorted(idx.values()) == list(range(n)), idx
    assert [_lib.PLAN_FIELDS[i] for i in sorted(idx.values())] == [f for f, _ in sorted(idx.items(), key=lambda t: t[1])]


def test_tile_kernel_layouts_match_the_launch_figures():
    """The LDS layouts, staging area, pad room, scratch slots and directory bits that the tile kernels and their launches take
    from one definition (csrc/kernels.h) equal the figures the launches used to restate, for every bucket count 1 .. 1024:
    tests/lds_layout_check.cpp, built for the host only."""
    import subprocess
    csrc = os.path.join(ROOT, "genomeassembler_dev_amd", "csrc")
    exe = os.path.join(ROOT, "oracle", "_build", "lds_layout_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-x", "hip", "--offload-host-only", "-Wall", "-Wno-unused-function", "-I" + csrc,
                    os.path.join(ROOT, "tests", "lds_layout_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 mismatches over nb = 1 .. 1024" in r.stdout, r.stdout + r.stderr


def test_no_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(ga.GasmError) as e:
        ga.Context(0)
    assert "GASM_ERR_NO_DEVICE" in str(e.value)


def test_table_normalisation_matches_oracle(qtable):
    _, prob = qtable
    mine = ga.qtable.load_normalised()
    assert np.array_equal(mine, prob)
    raw = ga.qtable.load_raw().copy()
    raw[[3, 20, 5000]] = np.nan
    assert np.array_equal(ga.qtable.normalise(raw), orc.normalise_tables(raw, [16, 256, 4096, 65536]))


@pytest.mark.parametrize("infix", [False, True])
def test_levenshtein_matches_oracle(infix):
    rng = np.random.default_rng(5)
    for n, m in [(1, 1), (5, 9), (63, 64), (64, 64), (65, 130), (200, 777), (700, 150), (1000, 1000)]:
        q = "".join(rng.choice(list("ACGT"), n))
        t = "".join(rng.choice(list("ACGT"), m))
        if n > 20:  # make it a noisy copy so distances are not trivially large
            t = (q[: n // 2] + t[: m // 3] + q[n // 2:])[:m] if m >= n else t
        assert ga.levenshtein(q, t, infix) == orc.levenshtein(q, t, infix), (n, m)
    assert ga.levenshtein("", "ACGT", infix) == 0 and ga.levenshtein("ACGT", "", infix) == 0


def _random_contig_set(rng, n, k):
    g = "".join(rng.choice(list("ACGT"), 400))
    cs = set()
    for _ in range(n):
        a = int(rng.integers(0, 300))
        cs.add(g[a:a + int(rng.integers(k, 80))])
    return sorted(cs)


def test_shuffle_and_assemble_match_oracle():
    rng = np.random.default_rng(11)
    for k in (5, 9, 15):
        contigs = _random_contig_set(rng, 9, k)
        rows = 300
        # velvet form: the oracle shuffles strings, the library shuffles indices — same std::shuffle draws
        assert ga.assemble_contigs_velvet(contigs, k, 1234, rows=rows) == orc.assemble_contigs_velvet(contigs, k, 1234, rows=rows)
        # matrix form
        m = np.stack([np.random.default_rng(i).permutation(len(contigs)) for i in range(50)]).astype(np.uint32)
        assert ga.assemble_contigs(ga.ContigMatrix(contigs, m, k, None, None, 1), k) == orc.assemble_contigs(contigs, m, k)
        # list-of-lists form (the reference's R shape)
        assert ga.assemble_contigs([[contigs[j] for j in row] for row in m], k) == orc.assemble_contigs(contigs, m, k)


def test_assemble_index_merge_randomised_against_oracle():
    """the index form of the merge (suffix/prefix matches precomputed per contig pair, chains of contig ids, strings built
    once per distinct chain) against the oracle's string form: windows of a genome overlapping by k-1, random extras,
    contigs only k-1 long, and a chain that spells another contig exactly (the `c[i] != c[j]` test of the reference)."""
    rng = np.random.default_rng(5)

    def rnd(n):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, n))

    done = 0
    for trial in range(40):
        k = int(rng.integers(3, 12))
        g = rnd(int(rng.integers(60, 400)))
        cuts = sorted(set(rng.integers(0, len(g) - k, int(rng.integers(3, 14))).tolist() + [0]))
        contigs = [g[a:min(len(g), b + k - 1)] for a, b in zip(cuts, cuts[1:] + [len(g)])]
        contigs += [rnd(int(rng.integers(k - 1, 30))) for _ in range(int(rng.integers(0, 4)))]
        contigs = sorted(set(c for c in contigs if len(c) >= k - 1))
        if len(contigs) < 2:
            continue
        rows = int(rng.integers(1, 80))
        assert ga.assemble_contigs_velvet(contigs, k, 7 + trial, rows=rows) == orc.assemble_contigs_velvet(contigs, k, 7 + trial, rows=rows)
        done += 1
    assert done > 30
    # "ACGT" + "GTAC"[2:] == "ACGTAC", which is also a contig: equal strings must not be merged into each other
    for seed in range(6):
        contigs = ["ACGT", "ACGTAC", "GTAC", "TTGA"]
        assert ga.assemble_contigs_velvet(contigs, 3, seed, rows=20) == orc.assemble_contigs_velvet(contigs, 3, seed, rows=20)


def test_fastq_fasta_reader(tmp_path):
    """libgasm's C++ reader (csrc/seqio.cpp, host only: runs without a GPU) against the Python restatement in
    oracle/seq_oracle.py, record by record: FASTQ with header extras and '@' in the qualities, lower case, a read with an N,
    CRLF line ends, gzipped multi-line FASTA, blank lines, an empty file, a file without a final newline"""
    import gzip

    import numpy as np

    from genomeassembler_dev_amd import seqio
    from oracle import seq_oracle
    fq = tmp_path / "a.fastq"
    fq.write_text("@r1\nACGTAC\n+\nIIIIII\n@r2 extra\nacgtn\n+r2\nIIIII\n@r3\nTTTT\n+\n@@@@\n\n")
    fa = tmp_path / "b.fa.gz"
    with gzip.open(fa, "wb") as f:
        f.write(b">c1\nACG\nTAC\n>c2\nGGGG\n\n>c3 multi\nAC\n\nGT\n")
    crlf = tmp_path / "c.fq"
    crlf.write_bytes(b"@x\r\nACGT\r\n+\r\nIIII\r\n@y\r\nGGCC\r\n+\r\nIIII")
    empty = tmp_path / "d.fa"
    empty.write_text("")
    rng = np.random.default_rng(4)
    big = tmp_path / "e.fastq.gz"
    recs = ["".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(1, 200)))) for _ in range(3000)]
    with gzip.open(big, "wb") as f:
        f.write("".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(recs)).encode())
    files = [fq, fa, crlf, empty, big]
    words, off, seg, dropped = seqio.read_files(files)
    reads, ooff, oseg, odropped = seq_oracle.segments_from_files(files)
    assert dropped == odropped == 1
    assert seg.tolist() == oseg.tolist() == [0, 2, 5, 7, 7, 3007]
    assert off.tolist() == ooff.tolist()
    mine = seqio.unpack_reads(words, off)
    assert mine == [reads[int(ooff[i]):int(ooff[i + 1])].tobytes() for i in range(len(ooff) - 1)]
    assert mine[:7] == [b"ACGTAC", b"TTTT", b"ACGTAC", b"GGGG", b"ACGT", b"ACGT", b"GGCC"] and mine[7:] == [r.encode() for r in recs]
    with pytest.raises(ga.GasmError) as e:
        seqio.read_files([fq], non_acgt="error")
    assert "GASM_ERR_NON_ACGT" in str(e.value)
    with pytest.raises(ValueError):
        seq_oracle.segments_from_files([fq], non_acgt="error")
    bad = tmp_path / "f.txt"
    bad.write_text("hello\n")
    with pytest.raises(ga.GasmError):
        seqio.read_files([bad])
    with pytest.raises(ValueError):
        seq_oracle.read_sequences(bad)
    with pytest.raises(ga.GasmError):
        seqio.read_files([tmp_path / "does_not_exist.fq"])


def test_assemble_short_contig_raises_like_reference():
    with pytest.raises(IndexError):
        ga.assemble_contigs_velvet(["ACG", "TTTTTTTT"], 6, 1, rows=3)
    with pytest.raises(IndexError):
        orc.assemble_contigs_velvet(["ACG", "TTTTTTTT"], 6, 1, rows=3)


def test_get_kmers_from_reads_matches_oracle():
    reads = ["ACGTACGTAC", "TTTT", "ACG", "GATTACAGATTACA"]
    for k in (3, 4, 5):
        assert ga.get_kmers_from_reads(reads, k) == orc.kmers_from_reads(reads, k)


def test_one_hip_runtime_whatever_the_import_order():
    """libgasm and PyTorch must share ONE copy of the HIP runtime, whichever is loaded first (round 2 lost a GPU test run to
    "No HIP GPUs are available": libgasm had mapped ROCm's copy, torch then brought its own)."""
    import subprocess
    import sys
    code_a = ("from genomeassembler_dev_amd import _lib; _lib.lib(); import torch; torch.cuda.is_available(); "
              "print(len(_lib.hip_runtimes_mapped()))")
    code_b = ("import torch; from genomeassembler_dev_amd import _lib; _lib.lib(); torch.cuda.is_available(); "
              "print(len(_lib.hip_runtimes_mapped()))")
    for code in (code_a, code_b):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1] == "1", out.stdout


def test_ownership_functions_c_and_python_agree():
    """gasm_pool_bucket_owner / gasm_pool_segment_bounds (what the library's exchange plans with) against pooled.py's numpy
    forms (what the gloo tests run)."""
    import numpy as np

    from genomeassembler_dev_amd import pooled
    from genomeassembler_dev_amd.parallel import shard_bounds
    for n_seg, bbits, world in ((1, 0, 1), (7, 3, 2), (100, 6, 8), (1000, 6, 8), (13, 10, 5), (3, 2, 7)):
        own, first = pooled.owners(n_seg, bbits, world)
        assert own.tolist() == pooled.bucket_owner(n_seg, bbits, world).tolist(), (n_seg, bbits, world)
        assert first.tolist() == [a for a, _ in shard_bounds(n_seg, world)] + [n_seg], (n_seg, bbits, world)


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` without a launcher must start two ranks under torch.distributed.run before anything touches
    a GPU; without GPUs the ranks then fail at "no GPU" — and the parent reports the failure with a non-zero status."""
    import subprocess
    import sys

    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the driver's own runs cover this")
    env = dict(os.environ)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None); env.pop("LOCAL_RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode != 0
    assert "starting 2 ranks" in p.stderr
    assert p.stderr.count("No HIP GPUs are available") + p.stderr.count("GASM_ERR_NO_DEVICE") >= 1, p.stderr[-3000:]
    assert "rank      : 1" in p.stderr or "local_rank: 1" in p.stderr       # the second rank existed
