"""The preconditions of the device-ingest tests (tests/test_ingest_seams_gpu.py), without a GPU: csrc/ingest.hip still states the
constants the cases of tests/ingest_cases.py are sized by; each case reaches, by its own numbers, the path it is there for; and the two
other readers of the grammar — the host reader (csrc/seqio.cpp, the definition) and oracle/seq_oracle.py — yield what each case says
it yields by construction."""
import os
import re

import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import ingest_cases as ic
from genomeassembler_dev_amd import seqio
from oracle import seq_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CU = 256                                       # an MI355X; the GPU test takes the device's own count
_CASES = {}


def case(name, *args):
    if (name, args) not in _CASES:
        _CASES[(name, args)] = getattr(ic, name)(*args)
    return _CASES[(name, args)]


def _host_reader_agrees(c, tmp_path):
    words, off, seg, dropped = seqio.read_files(c.write(tmp_path))
    assert dropped == c.dropped and np.array_equal(seg, c.seg_read_off) and np.array_equal(off, c.read_off)
    assert np.array_equal(words, c.words)


def _oracle_agrees(c, tmp_path):
    """file by file, the regular ones: every record in file order (the oracle reads strict four-line FASTQ only), then the whole call
    where every file is regular"""
    paths = c.write(tmp_path)
    for f, p in zip(c.files, paths):
        if f.regular:
            assert seq_oracle.read_sequences(p) == f.recs, f.name
    if all(c.on_device):
        reads, off, seg, dropped = seq_oracle.segments_from_files(paths)
        assert dropped == c.dropped and np.array_equal(seg, c.seg_read_off) and np.array_equal(off, c.read_off) and np.array_equal(reads, c.bases)


def test_ingest_hip_states_the_constants_the_cases_are_sized_by():
    src = open(os.path.join(ROOT, "genomeassembler_dev_amd", "csrc", "ingest.hip")).read()
    assert re.search(r"constexpr u32 CH = (\d+);", src).group(1) == str(ic.CH)
    assert re.search(r"constexpr u32 SB = (\d+);", src).group(1) == str(ic.SB)
    # 16 bytes per thread of 256 in the newline count, 8 elements per thread of 1024 in the block scans: CH and SB again
    assert src.count("(u64)blockIdx.x * CH + threadIdx.x * 16") == 2 and 256 * 16 == ic.CH
    assert src.count("(u64)blockIdx.x * SB + threadIdx.x * 8") == 2 and 1024 * 8 == ic.SB
    # the carry loop: one workgroup of SCAN_TRIP threads, SCAN_TRIP block sums per trip
    assert f"__launch_bounds__({ic.SCAN_TRIP}) k_ing_scan_sums(" in src
    assert f"for (u32 base = 0; base < nb; base += {ic.SCAN_TRIP})" in src
    assert f"hipLaunchKernelGGL(k_ing_scan_sums, dim3(1), dim3({ic.SCAN_TRIP})" in src
    assert "const u32 nb = std::max<u32>(1, (u32)((n + SB - 1) / SB));" in src
    # the pack and the append launches, and the fallback's
    grid = f"dim3((u32)std::min<u64>((nw + 255) / 256, (u64)ctx->n_cu * {ic.WG_PER_CU})), dim3(256)"
    assert f"hipLaunchKernelGGL(k_ing_pack, {grid}" in src and f"hipLaunchKernelGGL(k_ing_append, {grid}" in src
    assert f"const u64 nw = (bases + 31) / 32 + {ic.PAD_WORDS};" in src
    assert f"hipLaunchKernelGGL(k_ing_append, dim3((u32)std::min<u64>((nwh + 255) / 256 + 1, (u64)ctx->n_cu * {ic.WG_PER_CU})), dim3(256)" in src
    assert src.count("+= (u64)gridDim.x * 256)") == 2                  # the two grid-stride loops


def test_scan_carry_fastq_reaches_the_second_trip(tmp_path):
    c = case("scan_carry_fastq")
    data = c.files[0].data
    n_rec = c.note["n_rec"]
    assert n_rec == 2_200_000 and len(data) == 12 * n_rec and data.count(b"\n") + 1 == c.note["n_lines"] == 8_800_001
    assert c.note["n_lines"] > ic.SB * ic.SCAN_TRIP and ic.scan_trips(c.note["n_lines"]) == 2          # plen -> pbase
    assert ic.scan_trips(n_rec) == 1                 # keep -> keep_ex stays in one trip here: scan_carry_fasta carries it
    # bases and dropped records on both sides of the trip: line SB * SCAN_TRIP belongs to record 2 097 152
    seam = ic.SB * ic.SCAN_TRIP // 4
    assert c.dropped == 2200 and c.note["first_dropped"] < seam < n_rec - 1000
    assert len(c.read_off) == n_rec - 2200 + 1 and int(c.read_off[-1]) == 3 * (n_rec - 2200)
    assert data[:12 * 2].count(b"N") == 0 and data[12 * 999:12 * 1000].count(b"N") == 1
    _host_reader_agrees(c, tmp_path)


def test_scan_carry_fasta_carries_every_scan(tmp_path):
    c = case("scan_carry_fasta")
    data = c.files[0].data
    n_rec = c.note["n_rec"]
    assert data.count(b">") == n_rec and data.count(b"\n") + 1 == c.note["n_lines"] == 2 * n_rec + 1
    assert n_rec > ic.SB * ic.SCAN_TRIP and ic.scan_trips(n_rec) == 2                                   # keep -> keep_ex; rec_line[hdr_ex[i]] past 2^23
    assert ic.scan_trips(c.note["n_lines"]) == 3                                                       # hdr -> hdr_ex, plen -> pbase
    lens = np.diff(c.read_off.astype(np.int64))
    assert sorted(set(lens.tolist())) == [1, 2, 3] and c.dropped == n_rec // 1000 and len(lens) == n_rec - c.dropped
    _host_reader_agrees(c, tmp_path)


def test_pack_stride_fasta_has_more_words_than_threads(tmp_path):
    c = case("pack_stride_fasta", N_CU)
    big = c.note["big_bases"]
    nw, wgs = ic.pack_grid(big, N_CU)
    assert 34_000_000 < big < 35_000_000 and big % 100_000 == 0
    assert wgs == N_CU * ic.WG_PER_CU and nw > wgs * 256 and (big + 31) // 32 > wgs * 256              # a second trip over words that hold bases
    assert nw < 2 * wgs * 256                                                                            # (for 3 % of the threads)
    assert c.note["dst_off"] == int(c.read_off[1]) == 13 and len(c.files) == 2
    assert int(c.read_off[-1]) == 13 + big and c.files[1].data.count(b"\n") == big // 1000 + big // 100_000
    _host_reader_agrees(c, tmp_path)
    small = ic.pack_stride_fasta(2)                                # the rule scales with the device
    nw, wgs = ic.pack_grid(small.note["big_bases"], 2)
    assert wgs == 2 * ic.WG_PER_CU and nw > wgs * 256


def test_append_sweep_covers_every_residue_and_class(tmp_path):
    c = case("append_sweep")
    assert len(c.files) <= 400 and all(1 <= len(f.recs) <= 3 or f.note["klass"] == "zero" for f in c.files)
    want = ic.append_pairs()
    assert len(want) == 32 * 6 - 4 and {r for r, _ in want} == set(range(32))
    assert {k for r, k in want if r == 0} == {"zero", "inside", "big_aligned", "big_unaligned"}
    # the table against the files themselves: residue and class of every file from the offsets of the construction
    met, at = {}, 0
    for i, f in enumerate(c.files):
        n = int(f.kept_lens.sum())
        assert (f.note["residue"], f.note["klass"], f.note["n_bases"]) == (at % 32, ic.append_class(at % 32, n), n), f.name
        met.setdefault((at % 32, f.note["klass"]), []).append(i)
        at += n
    assert met == c.note["coverage"] and set(met) == want
    irregular = {(f.note["residue"], f.note["klass"]) for f in c.files if not f.regular}
    assert irregular == c.note["irregular"] and len({r for r, _ in irregular if r}) >= 8 and any(k == "spills" for _, k in irregular)
    assert all(f.name.endswith((".fastq", ".fastq.gz")) and b"\n\n@" in f.data.replace(b"\r", b"") for f in c.files if not f.regular)
    assert sum(f.name.endswith(".gz") for f in c.files) >= 5 and any(not f.regular and f.name.endswith(".gz") for f in c.files)
    assert {len(f.data) == 0 for f in c.files if f.note["klass"] == "zero"} == {True, False}
    _host_reader_agrees(c, tmp_path)
    _oracle_agrees(c, tmp_path)


def test_zero_and_exact_files_are_what_they_say(tmp_path):
    c = case("zero_and_exact")
    by = {f.name: f for f in c.files}
    for name in ("alldrop.fastq", "alldrop.fa"):
        assert len(by[name].kept_lens) == 0 and by[name].dropped == 3
    assert c.files[c.note["all_dropped"]].name == "alldrop.fastq"
    for name in ("empties.fastq", "empties.fa"):
        assert by[name].kept_lens.tolist() == [0, 0, 0] and by[name].dropped == 0
    assert by["nothing.fastq"].data == b""
    assert by["fits64.fa"].kept_lens.sum() == 64 and by["fits96.fastq"].kept_lens.sum() == 96 and not by["fits96.fastq"].data.endswith(b"\n")
    for name in ("boundary.fa", "boundary.fastq"):
        f = by[name]
        assert f.kept_lens.tolist()[:4] == [32, 0, 0, 5] and f.dropped == 3 and len(f.recs[1]) == 51
    assert by["onebase.fa"].data.startswith(b">r0\n" + b"\n".join(bytes([b]) for b in by["onebase.fa"].recs[0]) + b"\n>r1\n")
    assert by["onebase.fastq"].kept_lens.tolist() == [1] * 40
    # a kept file on either side of every special one, and residues that are not all zero
    special = [i for i, f in enumerate(c.files) if not f.name.startswith("k")]
    assert all(c.files[i - 1].name.startswith("k") and c.files[i + 1].name.startswith("k") for i in special)
    assert all(c.on_device)
    _host_reader_agrees(c, tmp_path)
    _oracle_agrees(c, tmp_path)
    paths = c.write(tmp_path)
    with pytest.raises(ga.GasmError, match="outside ACGT"):
        seqio.read_files([paths[0], paths[2], paths[c.note["all_dropped"]]], non_acgt="error")


def test_chunk_seams_hold_the_bytes_they_name(tmp_path):
    c = case("chunk_seams")
    seen, sizes = set(), set()
    for f in c.files:
        d = f.data
        if "pos" in f.note:
            p = f.note["pos"]
            assert d[p:p + 1] == b"\n" and (d[p - 1:p] == b"\r") == f.note["crlf"] and d[:p].count(b"\n") == (f.name[0] == "l"), f.name
            seen.add((f.name[0], f.name.rsplit(".", 1)[1], p, f.note["crlf"]))
        else:
            assert len(d) == f.note["size"] and d.endswith(b"\n") == f.note["final_nl"], f.name
            sizes.add((f.name.rsplit(".", 1)[1], f.note["size"], f.note["final_nl"]))
    assert ic.SEAM_POSITIONS == (15, 16, 4094, 4095, 4096, 4097, 4098, 8191, 8192, 8193) and ic.CH == 4096
    assert {s for s in seen if s[0] == "h"} == {("h", k, p, x) for k in ("fa", "fastq") for p in ic.SEAM_POSITIONS for x in (False, True)}
    assert {s for s in seen if s[0] == "l"} == {("l", "fa", p, x) for p in ic.SEAM_POSITIONS if p > 16 for x in (False, True)}
    assert sizes == {(k, s, n) for k in ("fa", "fastq") for s in (4096, 4097, 8192) for n in (False, True)}
    split = next(f for f in c.files if f.name == "h4096c.fastq")               # CR the last byte of chunk 0, LF the first of chunk 1
    assert split.data[ic.CH - 1:ic.CH + 1] == b"\r\n"
    assert all(f.regular and f.dropped == (1 if "pos" in f.note and f.name[0] == "h" else 0) for f in c.files)
    _host_reader_agrees(c, tmp_path)
    _oracle_agrees(c, tmp_path)


def test_scan_seams_have_the_lines_they_name(tmp_path):
    c = case("scan_seams")
    fasta = [f for f in c.files if f.name.endswith(".fa")]
    assert {f.note["n_lines"] for f in fasta} == {8191, 8192, 8193, 16384, 16385} and ic.SB == 8192
    for f in c.files:
        assert f.data.count(b"\n") + 1 == f.note["n_lines"], f.name
    for f in fasta:
        lines = f.data.split(b"\n")
        assert all(lines[h].startswith(b">") for h in f.note["headers"]) and sum(l.startswith(b">") for l in lines[8000:]) <= len(f.note["headers"]) + 9, f.name
        assert f.dropped >= 3 and len(f.kept_lens) >= 6
    for n in (8192, 8193, 16384, 16385):
        assert any(f.note["n_lines"] == n and 8191 in f.note["headers"] for f in fasta)
    for n in (8193, 16384, 16385):
        assert any(f.note["n_lines"] == n and 8192 in f.note["headers"] for f in fasta)
    assert any(f.note["headers"] == [f.note["n_lines"] - 1] for f in fasta)                  # a header as the last line: an empty last record
    assert sorted(f.note["n_lines"] for f in c.files if f.name.endswith(".fastq")) == [8192, 8193, 8196]
    _host_reader_agrees(c, tmp_path)
    _oracle_agrees(c, tmp_path)
