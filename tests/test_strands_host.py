"""The both-strand build's C ABI without a GPU: libgasm.so exports the new entries, include/gasm.h declares them with the agreed
signatures, the ctypes mirror knows them, and the Python surface refuses strands outside {1, 2} before anything reaches the
library."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "genomeassembler_dev_amd", "libgasm.so")
HEADER = os.path.join(ROOT, "include", "gasm.h")

SIGNATURES = {
    "gasm_batch_build_strands": "int gasm_batch_build_strands(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count, uint32_t strands);",
    "gasm_get_contigs_from_reads_strands": "int gasm_get_contigs_from_reads_strands(gasm_ctx* ctx, const char* reads, const uint64_t* read_off, uint64_t n_reads, "
                                           "int dbg_kmer, int seed, int matrix_rows, uint32_t min_count, uint32_t strands, gasm_contigs** out);",
    "gasm_batch_fetch_contig_twins": "int gasm_batch_fetch_contig_twins(gasm_batch* b, const uint32_t** twin);",
    "gasm_batch_strands": "uint32_t gasm_batch_strands(const gasm_batch* b);",
}


def _flat(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text).replace("( ", "(").replace(" )", ")")


def test_header_declares_the_new_entries():
    with open(HEADER) as f:
        raw = f.read()
    flat = _flat(raw)
    for name, sig in SIGNATURES.items():
        assert _flat(sig) in flat, name
    # the existing entries keep their signatures, the plan row its width
    assert "int gasm_batch_build(gasm_batch* b, int k, uint64_t genome_len_hint);" in flat
    assert "int gasm_batch_build_solid(gasm_batch* b, int k, uint64_t genome_len_hint, uint32_t min_count);" in flat
    assert "#define GASM_PLAN_FIELDS 15" in raw
    assert "GASM_ERR_INTERNAL = -8" in flat
    assert re.search(r"[Pp]ooled builds[^.]*forward-strand only", raw)


def test_library_exports_the_new_entries():
    # (symbol table only: the library's own dependencies need no GPU to be mapped, but nothing here calls into it)
    lib = C.CDLL(LIB)
    for name in SIGNATURES:
        assert hasattr(lib, name), name


def test_ctypes_mirror_knows_their_signatures():
    from genomeassembler_dev_amd import _lib
    u32, u64, i, vp, pp = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)
    want = {
        "gasm_batch_build_strands": (i, [vp, i, u64, u32, u32]),
        "gasm_get_contigs_from_reads_strands": (i, [vp, vp, vp, u64, i, i, i, u32, u32, pp]),
        "gasm_batch_fetch_contig_twins": (i, [vp, pp]),
        "gasm_batch_strands": (u32, [vp]),
    }
    for name, (res, args) in want.items():
        assert name in _lib.SYMBOLS, name
        assert _lib.SYMBOLS[name][0] is res and list(_lib.SYMBOLS[name][1]) == args, name
    assert _lib.STATUS[-8] == "GASM_ERR_INTERNAL"


def test_python_surface_refuses_strands_outside_1_and_2():
    from genomeassembler_dev_amd import api, batch
    b = batch.SegmentBatch.__new__(batch.SegmentBatch)
    b.h = None                                       # (nothing behind it: a call that reached the library would fail otherwise)
    for bad in (0, 3, -1):
        with pytest.raises(ValueError):
            b.build(21, strands=bad)
        with pytest.raises(ValueError):
            api.get_contigs_from_reads(["ACGT"], 3, 1, strands=bad)
    with pytest.raises(ValueError):
        b.build(21, 0, 0, 2)                         # min_count is still checked


def test_build_keeps_its_positional_form():
    from genomeassembler_dev_amd import api, batch
    p = list(inspect.signature(batch.SegmentBatch.build).parameters.values())
    assert [x.name for x in p] == ["self", "k", "genome_len_hint", "min_count", "strands"]
    assert [x.default for x in p[2:]] == [0, 1, 1]
    q = inspect.signature(api.get_contigs_from_reads).parameters
    assert list(q)[:7] == ["reads", "dbg_kmer", "seed", "matrix_rows", "ctx", "as_lists", "min_count"] and q["strands"].default == 1
    c = inspect.signature(batch.SegmentBatch.contigs).parameters
    assert list(c) == ["self", "segment", "one_per_pair"] and c["one_per_pair"].default is False
    assert callable(batch.SegmentBatch.contig_twins)
