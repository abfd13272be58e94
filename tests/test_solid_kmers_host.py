"""The multiplicity cutoff's C ABI without a GPU: libgasm.so exports the new entries, include/gasm.h declares them with the
agreed signatures, and the Python mirror refuses min_count < 1 before anything reaches the device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeassembler_dev_amd", "libgasm.so")
HEADER = os.path.join(ROOT, "include", "gasm.h")

SIGNATURES = {
    "gasm_batch_build_solid": "int gasm_batch_build_solid(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count);",
    "gasm_get_contigs_from_reads_solid": "int gasm_get_contigs_from_reads_solid(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, "
                                         "int dbg_kmer, int seed, int matrix_rows, uint32_t min_count, gasm_contigs** out);",
    "gasm_batch_fetch_solid_stats": "int gasm_batch_fetch_solid_stats(gasm_batch* b, const uint64_t** distinct_before, const uint64_t** distinct_after);",
    "gasm_batch_kmer_spectrum": "int gasm_batch_kmer_spectrum(gasm_batch* b);",
    "gasm_batch_fetch_kmer_spectrum": "int gasm_batch_fetch_kmer_spectrum(gasm_batch* b, const uint64_t** hist);",
}


def _flat(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text).replace("( ", "(").replace(" )", ")")


def test_header_declares_the_new_entries():
    with open(HEADER) as f:
        flat = _flat(f.read())
    for name, sig in SIGNATURES.items():
        assert _flat(sig) in flat, name
    # the existing entries keep their signatures
    assert "int gasm_batch_build(gasm_batch* b, int k, uint64_t genome_len_hint);" in flat
    assert ("int gasm_get_contigs_from_reads(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, int dbg_kmer, int seed, "
            "int matrix_rows, gasm_contigs** out);") in flat


def test_library_exports_the_new_entries():
    # (symbol table only: the library's own dependencies need no GPU to be mapped, but nothing here calls into it)
    lib = C.CDLL(LIB)
    for name in SIGNATURES:
        assert hasattr(lib, name), name


def test_python_mirror_knows_them_and_refuses_min_count_below_one():
    from genomeassembler_dev_amd import _lib, api, batch
    for name in SIGNATURES:
        assert name in _lib.SYMBOLS, name
    b = batch.SegmentBatch.__new__(batch.SegmentBatch)
    b.h = None
    with pytest.raises(ValueError):
        b.build(21, min_count=0)
    with pytest.raises(ValueError):
        api.get_contigs_from_reads(["ACGT"], 3, 1, min_count=0)
