"""Several breakage tables in one pass (gasm_calc_breakscore_tables, gasm_batch_score_tables): what can be checked without a
GPU — the new symbols resolve through _lib, every new entry refuses a NULL context / batch with GASM_ERR_INVALID before it
touches a device, and GASM_MAX_TABLES of the header is the Python constant."""
import ctypes as C
import os
import re

import numpy as np

from genomeassembler_dev_amd import _lib, qtable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gasm_calc_breakscore_tables", "gasm_calc_breakscore_tables_dev", "gasm_batch_score_tables", "gasm_batch_fetch_scores_table",
       "gasm_batch_fetch_score_fixed_table")
INVALID = -1


def test_new_symbols_resolve():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        f = getattr(L, name)
        assert f.restype is C.c_int and list(f.argtypes) == _lib.SYMBOLS[name][1], name


def test_max_tables_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "gasm.h")).read()
    m = re.search(r"#define GASM_MAX_TABLES\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.MAX_TABLES == 8


def _last_error():
    return (_lib.lib().gasm_last_error() or b"").decode()


def test_null_context_or_batch_is_invalid_without_a_device():
    L = _lib.lib()
    off = np.zeros(1, dtype=np.uint64)
    off2 = np.array([0, 2], dtype=np.uint64)
    probs = np.full(2, 0.5)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    junk = 0x1000                                   # never dereferenced: the entries must come back NULL
    for n_tables in (1, 2, _lib.MAX_TABLES):
        hs = (C.c_void_p * _lib.MAX_TABLES)(*([junk] * _lib.MAX_TABLES))
        st = L.gasm_calc_breakscore_tables(None, b"", p(off), 0, b"", p(off), 0, b"", 0, 8, b"AC", p(off2), 1, p(probs), n_tables, _lib.SCORE_OWN, 0, hs)
        assert st == INVALID and "null argument" in _last_error()
        assert [h for h in hs] == [None] * n_tables + [junk] * (_lib.MAX_TABLES - n_tables)
        hs = (C.c_void_p * _lib.MAX_TABLES)(*([junk] * _lib.MAX_TABLES))
        st = L.gasm_calc_breakscore_tables_dev(None, None, b"", p(off), 0, b"", 0, 8, b"AC", p(off2), 1, p(probs), n_tables, _lib.SCORE_OWN, 0, hs)
        assert st == INVALID and "null argument" in _last_error()
        assert [h for h in hs] == [None] * n_tables + [junk] * (_lib.MAX_TABLES - n_tables)
    # the number of tables is checked before anything else
    for n_tables in (0, _lib.MAX_TABLES + 1):
        hs = (C.c_void_p * (_lib.MAX_TABLES + 1))()
        assert L.gasm_calc_breakscore_tables(None, b"", p(off), 0, b"", p(off), 0, b"", 0, 8, b"AC", p(off2), 1, p(probs), n_tables, _lib.SCORE_OWN, 0,
                                             hs) == INVALID
        assert "n_tables" in _last_error()
    tables = np.ascontiguousarray(np.stack([qtable.uniform(), qtable.uniform()]))
    assert L.gasm_batch_score_tables(None, 8, p(tables), 2) == INVALID
    ps = [C.c_void_p() for _ in range(5)]
    assert L.gasm_batch_fetch_scores_table(None, 0, *[C.byref(x) for x in ps]) == INVALID
    fx, sh = C.c_void_p(), C.c_int()
    assert L.gasm_batch_fetch_score_fixed_table(None, 0, C.byref(fx), C.byref(sh)) == INVALID
