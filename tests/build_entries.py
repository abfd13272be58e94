"""The build entries of the C ABI called raw: the five positional gasm_batch_build* / gasm_get_contigs_from_reads* entries and the struct
entry of each family.  The Python wrappers go through the struct entries only, so these calls are what covers the positional ones:
test_lowcov_gpu.py compares every entry that can express a setting, and the C-ABI refusal tests of test_tips_gpu.py, test_bubbles_gpu.py
and test_lowcov_gpu.py check with refused_builds_change_nothing() that a build refused for its arguments leaves the batch as it was."""
import ctypes as C
import re

from genomeassembler_dev_amd import api
from genomeassembler_dev_amd._lib import BuildParams, lib

KNOBS = ("min_count", "strands", "tip_len", "tip_rounds", "bubble_len", "bubble_rounds", "cov_cutoff", "cov_len", "cov_rounds")
OFF = dict(min_count=1, strands=1, tip_len=0, tip_rounds=0, bubble_len=0, bubble_rounds=0)
# entry suffix -> how many of KNOBS, from the left, the entry takes
TAKES = {"": 0, "_solid": 1, "_strands": 2, "_tips": 4, "_bubbles": 6, "_params": 9}
GETTERS = ("strands", "tip_len", "tip_rounds", "bubble_len", "bubble_rounds", "cov_cutoff", "cov_len", "cov_rounds")
INVALID = -1


def entries_for(opts, positional_only=False):
    """the suffixes of the entries that can express `opts` (a dict of knobs): those that take every knob it names"""
    need = max((KNOBS.index(name) + 1 for name in opts), default=0)
    return [sfx for sfx, n in TAKES.items() if n >= need and not (positional_only and sfx == "_params")]


def _params(k, opts, size_off=0):
    p = BuildParams.make(k, **opts)
    p.size += size_off
    return p


def batch_build(b, sfx, k, opts, size_off=0):
    """status of gasm_batch_build<sfx> for the knobs in `opts`, the others off"""
    if sfx == "_params":
        return lib().gasm_batch_build_params(b.h, C.byref(_params(k, opts, size_off)))
    return getattr(lib(), "gasm_batch_build" + sfx)(b.h, k, 0, *(opts.get(name, OFF[name]) for name in KNOBS[:TAKES[sfx]]))


def contigs_from_reads(ctx, reads, sfx, k, seed, rows, opts, size_off=0):
    """(status, ContigMatrix or None) of gasm_get_contigs_from_reads<sfx> for the knobs in `opts`, the others off"""
    buf, off = api._pack(reads)
    h = C.c_void_p()
    if sfx == "_params":
        st = lib().gasm_get_contigs_from_reads_params(ctx.h, buf, api._ptr(off), len(reads), seed, rows, C.byref(_params(k, opts, size_off)), C.byref(h))
    else:
        st = getattr(lib(), "gasm_get_contigs_from_reads" + sfx)(ctx.h, buf, api._ptr(off), len(reads), k, seed, rows,
                                                                 *(opts.get(name, OFF[name]) for name in KNOBS[:TAKES[sfx]]), C.byref(h))
    return st, (api._contig_matrix(h, k, False) if st == 0 else None)


def getters(b):
    return tuple(int(getattr(lib(), "gasm_batch_" + name)(b.h)) for name in GETTERS)


def last_error():
    """gasm_last_error() without a leading entry name"""
    return re.sub(r"^gasm_\w+: ", "", lib().gasm_last_error().decode())


# every kind of refused build: (what, the knobs, only the positional entries?, bytes added to the struct's size)
REFUSED = [("tip_rounds 0", dict(tip_len=9, tip_rounds=0), False, 0), ("tip_rounds 9", dict(tip_len=9, tip_rounds=9), False, 0),
           ("bubble_rounds 0", dict(bubble_len=9, bubble_rounds=0), False, 0), ("bubble_rounds 9", dict(bubble_len=9, bubble_rounds=9), False, 0),
           ("cov_rounds 0", dict(cov_cutoff=2, cov_len=9, cov_rounds=0), False, 0), ("cov_rounds 9", dict(cov_cutoff=2, cov_len=9, cov_rounds=9), False, 0),
           ("strands 3", dict(strands=3), False, 0),
           ("min_count 0", dict(min_count=0), True, 0),                      # (in the struct 0 means the default)
           ("wrong size", dict(cov_cutoff=0, cov_len=0, cov_rounds=0), False, -4),   # (the struct entry only)
           ("bubble_len 65536", dict(bubble_len=65536, bubble_rounds=1), False, 0),
           ("cov_len 65536", dict(cov_cutoff=2, cov_len=65536, cov_rounds=1), False, 0)]


def refused_calls(call, suffixes):
    """every kind of refused call, through each entry among `suffixes` that accepts the bad value: all GASM_ERR_INVALID, and per bad
    value one error text whatever the entry.  call(sfx, opts, size_off) -> status.  Returns {what: text}"""
    texts = {}
    for what, opts, positional_only, size_off in REFUSED:
        seen = set()
        for sfx in entries_for(opts, positional_only):
            if sfx not in suffixes:
                continue
            assert call(sfx, opts, size_off) == INVALID, (what, sfx)
            seen.add(last_error())
        assert len(seen) <= 1, (what, seen)
        if seen:
            texts[what] = seen.pop()
    return texts


def refused_builds_change_nothing(suffixes=tuple(TAKES)):
    """a good build with tips on, every kind of refused build through the entries `suffixes`, and contigs(), tip_stats(), the getters
    and build_plan() are what they were; a good build then succeeds.  Returns the refused calls' texts"""
    import genomeassembler_dev_amd as ga
    rs = ["ACGTTGCATGCC"]                          # (one unbranched path: its only contig is the read)
    b = ga.SegmentBatch.from_strings([rs])
    b.k = 5
    assert batch_build(b, "_tips", 5, dict(tip_len=9, tip_rounds=2)) == 0

    def state():
        return b.contigs(), tuple(t.tobytes() for t in b.tip_stats()), getters(b), b.build_plan()
    before = state()
    assert before[0] == [rs] and before[2] == (1, 9, 2, 0, 0, 0, 0, 0)
    texts = refused_calls(lambda sfx, opts, size_off: batch_build(b, sfx, 5, opts, size_off), suffixes)
    assert texts and state() == before
    assert batch_build(b, "_bubbles", 5, dict(tip_len=9, tip_rounds=1, bubble_len=9, bubble_rounds=1)) == 0
    assert b.contigs() == [rs] and getters(b) == (1, 9, 1, 9, 1, 0, 0, 0)
    b.close()
    return texts
