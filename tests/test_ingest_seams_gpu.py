"""Device ingest (csrc/ingest.hip) at the sizes the product runs and at its seams, against what each file yields BY CONSTRUCTION
(tests/ingest_cases.py; the host reader and the Python oracle are held against the same constructions in tests/test_ingest_cases_host.py):
the carry loop of the device-wide scan, the grid-stride trips of the pack and the append, the append over every residue of dst_off and
every class of n_bases (the host-fallback launch included), totals of zero and exact fits, and newlines, headers and file ends at fixed
positions of the newline count's chunks and the scans' blocks.  Words, read_off, seg_read_off and dropped are compared exactly."""
import numpy as np
import pytest
import torch

import genomeassembler_dev_amd as ga
import ingest_cases as ic
from genomeassembler_dev_amd import seqio

pytestmark = pytest.mark.gpu


def _device_equals_construction(c, tmp_path):
    paths = c.write(tmp_path)
    words, off, seg, dropped, on = seqio.read_files_device(paths)
    assert on == c.on_device, [f.name for f, a, b in zip(c.files, on, c.on_device) if a != b]
    assert dropped == c.dropped and np.array_equal(seg, c.seg_read_off), (dropped, c.dropped)
    assert off.shape == c.read_off.shape, (off.shape, c.read_off.shape)
    if not np.array_equal(off, c.read_off):
        i = int(np.flatnonzero(off != c.read_off)[0])
        raise AssertionError(f"read_off differs first at read {i} of {len(off) - 1}: {int(off[i])}, expected {int(c.read_off[i])}")
    assert words.shape == c.words.shape
    if not np.array_equal(words, c.words):
        w = int(np.flatnonzero(words != c.words)[0])
        r = int(np.searchsorted(c.read_off, np.uint64(32 * w), side="right")) - 1
        f = int(np.searchsorted(c.seg_read_off, np.uint64(r), side="right")) - 1
        raise AssertionError(f"word {w} of {len(words)} differs ({int(words[w]):016x}, expected {int(c.words[w]):016x}): base {32 * w}, read {r}, "
                             f"file {c.files[f].name} {c.files[f].note}; {int((words != c.words).sum())} words differ")
    return paths


def _batch_equals_construction(c, paths):
    """the path without a copy-back: the batch adopts the device stream"""
    b = ga.SegmentBatch.from_fastq(paths)
    try:
        assert b.n_reads == len(c.read_off) - 1 and b.dropped_reads == c.dropped
        data, off = b.reads()
        assert np.array_equal(off, c.read_off) and np.array_equal(data, c.bases)
        assert b.read_strings() == [r.decode() for r in c.reads()]
    finally:
        b.close()


def test_scan_carry_fastq(tmp_path):
    c = ic.scan_carry_fastq()
    assert ic.scan_trips(c.note["n_lines"]) == 2                   # precondition (not a reference): the launch rule of scan_u32, restated
    _device_equals_construction(c, tmp_path)


def test_scan_carry_fasta(tmp_path):
    c = ic.scan_carry_fasta()
    assert ic.scan_trips(c.note["n_rec"]) == 2 and ic.scan_trips(c.note["n_lines"]) == 3
    _device_equals_construction(c, tmp_path)


def test_pack_stride_fasta(tmp_path):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c = ic.pack_stride_fasta(n_cu)
    # precondition (not a reference): min(ceil(nw / 256), n_cu * 16) workgroups of 256 threads, fewer threads than words that hold bases
    nw, wgs = ic.pack_grid(c.note["big_bases"], n_cu)
    assert wgs == n_cu * ic.WG_PER_CU and (c.note["big_bases"] + 31) // 32 > wgs * 256 and c.note["dst_off"] % 32 != 0, (n_cu, nw, wgs)
    _device_equals_construction(c, tmp_path)


def test_append_sweep(tmp_path):
    c = ic.append_sweep()
    assert set(c.note["coverage"]) == ic.append_pairs() and not all(c.on_device)
    paths = _device_equals_construction(c, tmp_path)
    _batch_equals_construction(c, paths)


def test_zero_and_exact(tmp_path):
    c = ic.zero_and_exact()
    paths = _device_equals_construction(c, tmp_path)
    _batch_equals_construction(c, paths)
    # the file whose every read is dropped, behind two clean ones, when a base outside ACGT is an error
    clean = [p for p, f in zip(paths, c.files) if f.dropped == 0 and len(f.kept_lens)][:2]
    refused = clean + [paths[c.note["all_dropped"]]]
    assert seqio.read_files_device(clean, non_acgt="error")[3] == 0
    with pytest.raises(ga.GasmError, match="outside ACGT"):
        seqio.read_files_device(refused, non_acgt="error")
    with pytest.raises(ga.GasmError, match="outside ACGT"):
        ga.SegmentBatch.from_fastq(refused, non_acgt="error")
    # each of the special files alone: dst_off = 0, and nothing before it in the scratch buffers of the call
    for f in c.files:
        if not f.name.startswith("k"):
            _device_equals_construction(ic.assemble([f]), tmp_path)


def test_chunk_seams(tmp_path):
    c = ic.chunk_seams()
    _device_equals_construction(c, tmp_path)
    for f in c.files:                                              # and each alone, so that a text is the first thing in the buffers
        if f.note.get("pos", 0) in (4095, 4096, 8192) or "size" in f.note:
            _device_equals_construction(ic.assemble([f]), tmp_path)


def test_scan_seams(tmp_path):
    c = ic.scan_seams()
    _device_equals_construction(c, tmp_path)
