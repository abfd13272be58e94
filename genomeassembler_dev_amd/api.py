"""Host-side mirror of the reference's R-callable entry points (same names, argument meaning and error behaviour),
over the C ABI of libgasm (include/gasm.h):

    get_contigs(read_kmers, dbg_kmer, seed)                  lib/DeNovoAssembler.cpp:86-206
    assemble_contigs(contig_matrix, dbg_kmer)                lib/DeNovoAssembler.cpp:215-305
    assemble_contigs_velvet(velvet_contigs, dbg_kmer, seed)  lib/BreakageScorer.cpp:80-174
    calc_breakscore(path, sequencing_reads, true_solution, kmer, bp_kmer, bp_prob)
                                                              lib/DeNovoAssembler.cpp:317-477 (variant="own")
                                                              lib/BreakageScorer.cpp:186-353  (variant="velvet")
    get_kmers_from_reads(reads, dbg_kmer)                    lib/DeNovoAssembler.R:109-130

Where the reference raises an R error (a C++ exception through Rcpp), these raise GasmError / IndexError.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GasmError, check, default_context, lib


def _pack(strs):
    """sequence of str/bytes -> (bytes, uint64 offsets[n+1])"""
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in strs]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return b"".join(bs), off


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _strings(data_ptr, off_ptr, n):
    if n == 0:
        return []
    off = np.ctypeslib.as_array(C.cast(off_ptr, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
    raw = C.string_at(data_ptr, int(off[-1])) if off[-1] else b""
    return [raw[int(off[i]):int(off[i + 1])].decode() for i in range(n)]


def _arr(ptr, ctype, n):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=ctype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).copy()


def unpack_kmers(keys, k, words=1):
    """2-bit packed k-mers (gasm.h layout: base 0 most significant) -> list of str"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, words)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = np.empty((keys.shape[0], k), dtype=np.uint8)
    for j in range(k):
        bit = 2 * (k - 1 - j)
        w = words - 1 - bit // 64
        out[:, j] = lut[((keys[:, w] >> np.uint64(bit % 64)) & np.uint64(3)).astype(np.int64)]
    return [r.tobytes().decode() for r in out]


def get_kmers_from_reads(reads, dbg_kmer):
    """Every k-mer of every read, read-major, duplicates kept (lib/DeNovoAssembler.R:109-130).  Host convenience for
    callers of get_contigs; the batch path (SegmentBatch) extracts k-mers on the GPU instead."""
    out = []
    for r in reads:
        out.extend(r[i:i + dbg_kmer] for i in range(len(r) - dbg_kmer + 1))
    return out


class ContigMatrix:
    """get_contigs' return value without materialising rows x contigs strings: the sorted unique contigs plus the
    shuffle matrix as indices.  `rows()` / `as_lists()` give the reference's list-of-character-vectors shape."""

    def __init__(self, contigs, perm, dbg_kmer, distinct_keys, distinct_mult, words):
        self.contigs, self.perm, self.dbg_kmer = contigs, perm, dbg_kmer
        self.distinct_keys, self.distinct_mult, self.words = distinct_keys, distinct_mult, words

    def distinct_kmers(self):
        return unpack_kmers(self.distinct_keys, self.dbg_kmer, self.words)

    def row(self, i):
        return [self.contigs[j] for j in self.perm[i]]

    def as_lists(self):
        return [self.row(i) for i in range(self.perm.shape[0])]


def get_contigs(read_kmers, dbg_kmer, seed, matrix_rows=10000, ctx=None, as_lists=False):
    """read_kmers: list of str (each exactly dbg_kmer long), or a uint8 array of shape (n, dbg_kmer)."""
    ctx = ctx or default_context()
    if isinstance(read_kmers, np.ndarray):
        a = np.ascontiguousarray(read_kmers, dtype=np.uint8)
        if a.ndim != 2 or a.shape[1] != dbg_kmer:
            raise ValueError("read_kmers array must have shape (n, dbg_kmer)")
        n, buf = a.shape[0], a
        p = _ptr(a)
    else:
        n = len(read_kmers)
        for s in read_kmers:
            if len(s) != dbg_kmer:
                raise ValueError(f"every k-mer must be exactly dbg_kmer={dbg_kmer} long (got {len(s)})")
        buf = "".join(read_kmers).encode() if n and isinstance(read_kmers[0], str) else b"".join(read_kmers)
        p = C.cast(C.c_char_p(buf), C.c_void_p)
    h = C.c_void_p()
    check(lib().gasm_get_contigs(ctx.h, p, n, int(dbg_kmer), int(seed), int(matrix_rows), C.byref(h)))
    return _contig_matrix(h, dbg_kmer, as_lists)


def _check_tips(tip_len, tip_rounds):
    """the argument rule of every tip-clipping entry: tip_len >= 0, and 1.._lib.MAX_TIP_ROUNDS rounds when it is on"""
    if int(tip_len) < 0 or int(tip_len) > 0xFFFFFFFF:
        raise ValueError("tip_len must be >= 0 (0: no tip clipping)")
    if int(tip_len) > 0 and not 1 <= int(tip_rounds) <= _lib.MAX_TIP_ROUNDS:
        raise ValueError(f"tip_rounds must be 1..{_lib.MAX_TIP_ROUNDS} when tip_len > 0")


def _check_bubbles(bubble_len, bubble_rounds):
    """the argument rule of every bubble-popping entry: 0 <= bubble_len <= _lib.MAX_BUBBLE_LEN, and 1.._lib.MAX_BUBBLE_ROUNDS rounds
    when it is on"""
    if not 0 <= int(bubble_len) <= _lib.MAX_BUBBLE_LEN:
        raise ValueError(f"bubble_len must be 0..{_lib.MAX_BUBBLE_LEN} (0: no bubble popping)")
    if int(bubble_len) > 0 and not 1 <= int(bubble_rounds) <= _lib.MAX_BUBBLE_ROUNDS:
        raise ValueError(f"bubble_rounds must be 1..{_lib.MAX_BUBBLE_ROUNDS} when bubble_len > 0")


def _check_lowcov(cov_cutoff, cov_len, cov_rounds):
    """the argument rule of every low-coverage entry: cov_cutoff >= 0, 0 <= cov_len <= _lib.MAX_BUBBLE_LEN, and 1.._lib.MAX_COV_ROUNDS
    rounds when both are positive (either 0: the feature is off and cov_rounds is not read)"""
    if not 0 <= int(cov_cutoff) <= 0xFFFFFFFF:
        raise ValueError("cov_cutoff must be >= 0 (0: no low-coverage removal)")
    if not 0 <= int(cov_len) <= _lib.MAX_BUBBLE_LEN:
        raise ValueError(f"cov_len must be 0..{_lib.MAX_BUBBLE_LEN} (0: no low-coverage removal)")
    if int(cov_cutoff) > 0 and int(cov_len) > 0 and not 1 <= int(cov_rounds) <= _lib.MAX_COV_ROUNDS:
        raise ValueError(f"cov_rounds must be 1..{_lib.MAX_COV_ROUNDS} when cov_cutoff > 0 and cov_len > 0")


def _check_build_opts(min_count=1, strands=1, tip_len=0, tip_rounds=1, bubble_len=0, bubble_rounds=1, cov_cutoff=0, cov_len=0, cov_rounds=1):
    """the argument rules of every build entry, of SegmentBatch and of this module: ValueError before anything reaches the library"""
    if int(min_count) < 1:
        raise ValueError("min_count must be >= 1 (1 keeps every k-mer)")
    if int(strands) not in (1, 2):
        raise ValueError("strands must be 1 (forward k-mers only) or 2 (both strands)")
    _check_tips(tip_len, tip_rounds)
    _check_bubbles(bubble_len, bubble_rounds)
    _check_lowcov(cov_cutoff, cov_len, cov_rounds)


def _contigs_from_reads(reads, dbg_kmer, seed, matrix_rows, ctx, as_lists, **opts):
    """every get_contigs_from_reads*() below: check the options, hand them to the library as one gasm_build_params
    (gasm_get_contigs_from_reads_params)"""
    _check_build_opts(**opts)
    ctx = ctx or default_context()
    buf, off = _pack(reads)
    h = C.c_void_p()
    p = _lib.BuildParams.make(dbg_kmer, **opts)
    check(lib().gasm_get_contigs_from_reads_params(ctx.h, buf, _ptr(off), len(reads), int(seed), int(matrix_rows), C.byref(p), C.byref(h)))
    return _contig_matrix(h, dbg_kmer, as_lists)


def get_contigs_from_reads(reads, dbg_kmer, seed, matrix_rows=10000, ctx=None, as_lists=False, min_count=1, strands=1, tip_len=0,
                           tip_rounds=1):
    """get_kmers_from_reads + get_contigs in one call: the k-mers are taken on the GPU from the packed reads instead of being
    exploded into len(reads) * (read_len - k + 1) strings first (lib/DeNovoAssembler.R:109-130).
    reads: list of str / bytes.  Same ContigMatrix as get_contigs(get_kmers_from_reads(reads, k), k, seed).
    min_count > 1: only k-mers seen at least min_count times become edges.
    strands = 2: the k-mers of every read and of its reverse complement.
    tip_len > 0: tip_rounds rounds of tip clipping before the contigs are cut (include/gasm.h).
    Bubble popping behind the tips: get_contigs_from_reads_bubbles()."""
    return _contigs_from_reads(reads, dbg_kmer, seed, matrix_rows, ctx, as_lists, min_count=min_count, strands=strands, tip_len=tip_len,
                               tip_rounds=tip_rounds)


def get_contigs_from_reads_bubbles(reads, dbg_kmer, seed, matrix_rows=10000, ctx=None, as_lists=False, min_count=1, strands=1, tip_len=0,
                                   tip_rounds=1, bubble_len=0, bubble_rounds=1):
    """get_contigs_from_reads with bubble popping: after the tip rounds, bubble_rounds rounds (1.._lib.MAX_BUBBLE_ROUNDS) in which
    every contig of at most bubble_len bases (<= _lib.MAX_BUBBLE_LEN) beside which a parallel one of strictly higher mean
    multiplicity runs leaves the k-mer set (the rule: include/gasm.h).  bubble_len = 0 is get_contigs_from_reads(..., tip_len,
    tip_rounds), and bubble_rounds is not read.  (An entry of its own, as build_bubbles() is beside build_tips():
    get_contigs_from_reads keeps its parameter list.)"""
    return _contigs_from_reads(reads, dbg_kmer, seed, matrix_rows, ctx, as_lists, min_count=min_count, strands=strands, tip_len=tip_len,
                               tip_rounds=tip_rounds, bubble_len=bubble_len, bubble_rounds=bubble_rounds)


def get_contigs_from_reads_simplified(reads, dbg_kmer, seed, matrix_rows=10000, ctx=None, as_lists=False, *, min_count=1, strands=1, tip_len=0,
                                      tip_rounds=1, bubble_len=0, bubble_rounds=1, cov_cutoff=0, cov_len=0, cov_rounds=1):
    """get_contigs_from_reads_bubbles with low-coverage removal: after the tip and the bubble rounds, cov_rounds rounds
    (1.._lib.MAX_COV_ROUNDS) in which every contig of at most cov_len bases (<= _lib.MAX_BUBBLE_LEN) whose mean multiplicity is
    strictly below cov_cutoff leaves the k-mer set, attached or not (the rule: include/gasm.h).  cov_cutoff = 0 or cov_len = 0 is
    get_contigs_from_reads_bubbles with the other arguments, and cov_rounds is not read.  The knobs are keyword-only: the
    positional chain ends with get_contigs_from_reads_bubbles."""
    return _contigs_from_reads(reads, dbg_kmer, seed, matrix_rows, ctx, as_lists, min_count=min_count, strands=strands, tip_len=tip_len,
                               tip_rounds=tip_rounds, bubble_len=bubble_len, bubble_rounds=bubble_rounds, cov_cutoff=cov_cutoff, cov_len=cov_len,
                               cov_rounds=cov_rounds)


def _contig_matrix(h, dbg_kmer, as_lists):
    try:
        L = lib()
        nc = L.gasm_contigs_count(h)
        contigs = _strings(L.gasm_contigs_data(h), L.gasm_contigs_offsets(h), nc)
        rows = L.gasm_contigs_rows(h)
        perm = _arr(L.gasm_contigs_perm(h), C.c_uint32, rows * nc).reshape(rows, nc)
        nd, words = L.gasm_contigs_distinct_count(h), L.gasm_contigs_key_words(h)
        dk = _arr(L.gasm_contigs_distinct_keys(h), C.c_uint64, nd * words)
        dm = _arr(L.gasm_contigs_distinct_mult(h), C.c_uint32, nd)
    finally:
        lib().gasm_contigs_free(h)
    m = ContigMatrix(contigs, perm, dbg_kmer, dk, dm, words)
    return m.as_lists() if as_lists else m


def _strlist(h):
    L = lib()
    try:
        return _strings(L.gasm_strlist_data(h), L.gasm_strlist_offsets(h), L.gasm_strlist_count(h))
    finally:
        L.gasm_strlist_free(h)


def _raise(e):
    if e.status == -6:
        raise IndexError(str(e)) from None
    raise e


class Scaffolds:
    """Distinct scaffolds of assemble_contigs left on the GPU (2-bit, the reference's order: longest first).  Pass it to
    calc_breakscore as `path`; `.strings()` makes the text."""

    def __init__(self, h, ctx):
        self.h, self.ctx = h, ctx
        n = lib().gasm_scaffolds_count(h)
        off = _arr(lib().gasm_scaffolds_offsets(h), C.c_uint64, n + 1)
        self.lengths = np.diff(off).astype(np.int64) if n else np.zeros(0, np.int64)
        r = C.c_uint64()
        self.merge_device = {0: None, 1: "gpu", 2: "host", 3: "gpu+host"}[lib().gasm_scaffolds_merge_device(h, C.byref(r))]
        self.rows_on_host = int(r.value)

    def __len__(self):
        return len(self.lengths)

    def strings(self):
        h = C.c_void_p()
        check(lib().gasm_scaffolds_fetch(self.h, C.byref(h)))
        return _strlist(h)

    def close(self):
        if self.h:
            lib().gasm_scaffolds_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def assemble_contigs(contig_matrix, dbg_kmer, ctx=None, on_device=False):
    """contig_matrix: a ContigMatrix, or the reference's list of equally long lists of strings.
    on_device=True: returns a `Scaffolds` handle (nothing is copied back) instead of the list of strings."""
    if isinstance(contig_matrix, ContigMatrix):
        contigs, perm = contig_matrix.contigs, contig_matrix.perm
    else:
        rows = [list(r) for r in contig_matrix]
        width = len(rows[0]) if rows else 0
        if any(len(r) != width for r in rows):
            raise ValueError("all rows of contig_matrix must have the same length")
        contigs = sorted(set(s for r in rows for s in r))
        ix = {s: i for i, s in enumerate(contigs)}
        perm = np.array([[ix[s] for s in r] for r in rows], dtype=np.uint32).reshape(len(rows), width)
    buf, off = _pack(contigs)
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    h = C.c_void_p()
    try:
        if on_device:
            ctx = ctx or default_context()
            check(lib().gasm_assemble_contigs_dev(ctx.h, buf, _ptr(off), len(contigs), _ptr(perm), perm.shape[0], perm.shape[1], int(dbg_kmer),
                                                  C.byref(h)))
            return Scaffolds(h, ctx)
        check(lib().gasm_assemble_contigs(ctx.h if ctx else None, buf, _ptr(off), len(contigs), _ptr(perm), perm.shape[0],
                                          perm.shape[1], int(dbg_kmer), C.byref(h)))
    except GasmError as e:
        _raise(e)
    return _strlist(h)


def assemble_contigs_velvet(velvet_contigs, dbg_kmer, seed, rows=20000, ctx=None, on_device=False):
    buf, off = _pack(velvet_contigs)
    h = C.c_void_p()
    try:
        if on_device:
            ctx = ctx or default_context()
            check(lib().gasm_assemble_contigs_velvet_dev(ctx.h, buf, _ptr(off), len(velvet_contigs), int(dbg_kmer), int(seed), int(rows), C.byref(h)))
            return Scaffolds(h, ctx)
        check(lib().gasm_assemble_contigs_velvet(ctx.h if ctx else None, buf, _ptr(off), len(velvet_contigs), int(dbg_kmer),
                                                 int(seed), int(rows), C.byref(h)))
    except GasmError as e:
        _raise(e)
    return _strlist(h)


def levenshtein(query, target, infix=False):
    q = query.encode() if isinstance(query, str) else bytes(query)
    t = target.encode() if isinstance(target, str) else bytes(target)
    out = C.c_int32()
    check(lib().gasm_levenshtein(q, len(q), t, len(t), int(infix), C.byref(out)))
    return out.value


def _breakscore_args(sequencing_reads, true_solution, bp_kmer, variant, with_lev, with_freq, with_ks):
    """the argument packing calc_breakscore and calc_breakscore_tables share: (velvet, reads, their offsets, the keys, their
    offsets, the true solution as bytes, the C variant, the flags); the arrays must outlive the C call"""
    velvet = variant == "velvet"
    if variant not in ("own", "velvet"):
        raise ValueError("variant must be 'own' or 'velvet'")
    rb, ro = _pack(sequencing_reads)
    kb, ko = _pack(bp_kmer)
    t = true_solution.encode() if isinstance(true_solution, str) else bytes(true_solution)
    flags = (_lib.WANT_LEV if with_lev else 0) | (_lib.WANT_FREQ if with_freq and not velvet else 0) | (_lib.WANT_KS if with_ks else 0)
    return velvet, rb, ro, kb, ko, t, _lib.SCORE_VELVET if velvet else _lib.SCORE_OWN, flags


def calc_breakscore(path, sequencing_reads, true_solution, kmer, bp_kmer, bp_prob, variant="own", with_lev=True,
                    with_freq=True, with_ks=False, ctx=None):
    """Returns a dict with the names of the reference's Rcpp::List (lib/DeNovoAssembler.cpp:467-476 /
    lib/BreakageScorer.cpp:343-353).  path_freq rows follow bp_kmer order (the reference: hash order).
    with_ks adds stat_test_KS: what lib/DeNovoAssembler.R:419-424 computes from path_freq afterwards."""
    ctx = ctx or default_context()
    velvet, rb, ro, kb, ko, t, v, flags = _breakscore_args(sequencing_reads, true_solution, bp_kmer, variant, with_lev, with_freq, with_ks)
    prob = np.ascontiguousarray(bp_prob, dtype=np.float64)
    h = C.c_void_p()
    if isinstance(path, Scaffolds):
        # the scaffolds are on the device already (assemble_contigs(..., on_device=True)): no text, no upload
        check(lib().gasm_calc_breakscore_dev(ctx.h, path.h, rb, _ptr(ro), len(sequencing_reads), t, len(t), int(kmer), kb, _ptr(ko), len(bp_kmer),
                                             _ptr(prob), v, flags, C.byref(h)))
    else:
        pb, po = _pack(path)
        check(lib().gasm_calc_breakscore(ctx.h, pb, _ptr(po), len(path), rb, _ptr(ro), len(sequencing_reads), t, len(t), int(kmer),
                                         kb, _ptr(ko), len(bp_kmer), _ptr(prob), v, flags, C.byref(h)))
    try:
        return _scores_dict(h, path, len(bp_kmer), velvet, with_freq, with_ks)
    finally:
        lib().gasm_scores_free(h)


def _scores_dict(h, path, n_table, velvet, with_freq, with_ks, path_freq=None):
    """a gasm_scores object as calc_breakscore's dict; path_freq: an array to use instead of copying the object's (the
    results of one calc_breakscore_tables call share it)"""
    L = lib()
    n = L.gasm_scores_count(h)
    out = dict(sequence=(path if isinstance(path, Scaffolds) else list(path)),
               sequence_len=_arr(L.gasm_scores_sequence_len(h), C.c_int32, n),
               bp_score=_arr(L.gasm_scores_bp_score(h), C.c_double, n),
               bp_score_norm_by_break_freqs=_arr(L.gasm_scores_norm_by_break_freqs(h), C.c_double, n),
               bp_score_norm_by_len=_arr(L.gasm_scores_norm_by_len(h), C.c_double, n),
               kmer_breaks=_arr(L.gasm_scores_kmer_breaks(h), C.c_int32, n),
               lev_dist_vs_true=_arr(L.gasm_scores_lev_dist(h), C.c_int32, n))
    if velvet:
        out["path_prob_dist_startpos"] = _arr(L.gasm_scores_startpos(h), C.c_int32, n)
        off = _arr(L.gasm_scores_prob_dist_offsets(h), C.c_uint64, n + 1)
        pd = _arr(L.gasm_scores_prob_dist(h), C.c_double, int(off[-1]) if n else 0)
        out["path_prob_dist"] = [pd[int(off[i]):int(off[i + 1])] for i in range(n)]
    elif with_freq:
        if path_freq is None:
            path_freq = _arr(L.gasm_scores_path_freq(h), C.c_double, n * n_table).reshape(n, n_table)
        out["path_freq"] = path_freq
    if with_ks:
        out["stat_test_KS"] = _arr(L.gasm_scores_ks(h), C.c_double, n)
    out["lev_device"] = {0: None, 1: "gpu", 2: "host"}[L.gasm_scores_lev_device(h)]      # (not a reference column: who did the work)
    return out


def calc_breakscore_tables(path, sequencing_reads, true_solution, kmer, bp_kmer, bp_probs, variant="own", with_lev=True,
                           with_freq=True, with_ks=False, ctx=None):
    """calc_breakscore under several breakage tables at once (gasm_calc_breakscore_tables): bp_probs is a sequence of 1 to
    _lib.MAX_TABLES probability vectors over the same bp_kmer — what score_solutions() passes one after the other
    (lib/DeNovoAssembler.R:325-355: the true table, then the uniform one).  Returns a list with, per table, the dict
    calc_breakscore returns for it, bit for bit; the reads are matched once (and Levenshtein, the KS test's genome side and
    path_freq computed once: the dicts share one path_freq array).  `path` may be a Scaffolds handle."""
    ctx = ctx or default_context()
    velvet, rb, ro, kb, ko, t, v, flags = _breakscore_args(sequencing_reads, true_solution, bp_kmer, variant, with_lev, with_freq, with_ks)
    probs = np.ascontiguousarray(bp_probs, dtype=np.float64)
    if probs.ndim != 2 or probs.shape[1] != len(bp_kmer):
        raise ValueError("bp_probs must hold one row of len(bp_kmer) probabilities per table")
    T = probs.shape[0]
    hs = (C.c_void_p * max(T, 1))()
    if isinstance(path, Scaffolds):
        check(lib().gasm_calc_breakscore_tables_dev(ctx.h, path.h, rb, _ptr(ro), len(sequencing_reads), t, len(t), int(kmer), kb, _ptr(ko), len(bp_kmer),
                                                    _ptr(probs), T, v, flags, hs))
    else:
        pb, po = _pack(path)
        check(lib().gasm_calc_breakscore_tables(ctx.h, pb, _ptr(po), len(path), rb, _ptr(ro), len(sequencing_reads), t, len(t), int(kmer),
                                                kb, _ptr(ko), len(bp_kmer), _ptr(probs), T, v, flags, hs))
    try:
        out = []
        for h in hs:
            out.append(_scores_dict(h, path, len(bp_kmer), velvet, with_freq, with_ks, path_freq=out[0].get("path_freq") if out else None))
        return out
    finally:
        for h in hs:
            lib().gasm_scores_free(h)


def count_read_kmers(sequencing_reads, kmer, bp_kmer=None, ctx=None):
    """count_read_kmers (lib/DeNovoAssembler.R:135-168, the reference's only_kmers_from_reads mode): occurrences of every
    kmer-long window (kmer in 2, 4, 6, 8) lying inside one read, as np.uint32 aligned to bp_kmer (duplicates allowed, absent
    k-mers 0).  bp_kmer=None: all 4**kmer k-mers in lexicographic ACGT order, the row order of the breakage table of that
    length.  Counted on the GPU (gasm_count_read_kmers)."""
    ctx = ctx or default_context()
    rb, ro = _pack(sequencing_reads)
    if bp_kmer is None:
        out = np.zeros(4 ** int(kmer) if kmer in (2, 4, 6, 8) else 0, dtype=np.uint32)
        check(lib().gasm_count_read_kmers(ctx.h, rb, _ptr(ro), len(sequencing_reads), int(kmer), None, None, 0, _ptr(out)))
    else:
        kb, ko = _pack(bp_kmer)
        out = np.zeros(len(bp_kmer), dtype=np.uint32)
        check(lib().gasm_count_read_kmers(ctx.h, rb, _ptr(ro), len(sequencing_reads), int(kmer), kb, _ptr(ko), len(bp_kmer), _ptr(out)))
    return out


def coverage_percent(starts, lens, seq_len, ctx=None):
    """contig_frac_len (lib/DeNovoAssembler.R:432-445): percentage of [1, seq_len] covered by the union of the inclusive
    ranges [start, start + len]"""
    ctx = ctx or default_context()
    a = np.ascontiguousarray(starts, dtype=np.int64)
    b = np.ascontiguousarray(lens, dtype=np.int64)
    out = C.c_double()
    check(lib().gasm_coverage_percent(ctx.h, _ptr(a), _ptr(b), len(a), int(seq_len), C.byref(out)))
    return out.value


def correct_reads(reads, k, min_count=2, strands=1, ctx=None):
    """the reads (a list of str: one segment) with their substitution errors repaired against their own solid k-mers: build(k,
    min_count, strands), SegmentBatch.correct_reads(), fetch.  Returns a list of str of the same lengths in the same order; a read the
    rule cannot repair comes back as it was (the rule and its limits: include/gasm.h "Read correction")."""
    from .batch import SegmentBatch
    b = SegmentBatch.from_strings([list(reads)], ctx=ctx)
    try:
        c = b.build(int(k), min_count=min_count, strands=strands).correct_reads()
        try:
            return c.read_strings()
        finally:
            c.close()
    finally:
        b.close()


def get_contigs_from_fastq(paths, k, non_acgt="drop", trim_q3=0, trim_q5=0, min_len=0, pairs=False, phred_offset=33, quality_hist=False, ctx=None, **build):
    """FASTQ in, contigs out, in one call: the files (one per segment, FASTQ or FASTA, plain or .gz) read, trimmed and packed on the
    device (SegmentBatch.from_fastq with its options: the rule is include/gasm.h's "Quality trimming at ingest"), then one
    build_simplified(k, **build) over what is left.  Returns (contigs: one list of str per segment, seqio.IngestStats or None when no
    ingest option is set).  build: as for contig_graph."""
    from .batch import SegmentBatch
    b = SegmentBatch.from_fastq(paths, non_acgt=non_acgt, ctx=ctx, trim_q3=trim_q3, trim_q5=trim_q5, min_len=min_len, pairs=pairs, phred_offset=phred_offset,
                                quality_hist=quality_hist)
    try:
        stats = b.ingest_stats() if b.ingest_options else None
        b.build_simplified(int(k), **build)
        return [b.contigs(s) for s in range(b.n_segments)], stats
    finally:
        b.close()


def contig_graph(reads, k, span_len=None, ctx=None, **build):
    """the contigs of one segment's reads (a list of str) and the graph between them: (contigs, links.ContigLinks).  build: the keyword
    set of SegmentBatch.build_simplified (min_count, strands, tip_len, tip_rounds, bubble_len, bubble_rounds, cov_cutoff, cov_len,
    cov_rounds, genome_len_hint).  The ContigLinks speaks of segment 0: links(0), to_gfa(0), resolve_repeats(0).  span_len = None: the
    longest read."""
    from .batch import SegmentBatch
    b = SegmentBatch.from_strings([list(reads)], ctx=ctx)
    try:
        cl = b.build_simplified(int(k), **build).contig_links(span_len)
        return cl.contigs(0), cl
    finally:
        b.close()


def map_reads(reads, k, max_mismatch=4, ctx=None, **build):
    """one segment's reads (a list of str) mapped onto the contigs of their own build within max_mismatch substitutions: a
    readmap.ReadMap that speaks of segment 0 (records(0), pileup(0), depth(0), mapped_fraction(0), error_rate(0), consensus(0),
    variants(0); the rule and its limits: include/gasm.h "Read mapping").  build: as for contig_graph."""
    from .batch import SegmentBatch
    b = SegmentBatch.from_strings([list(reads)], ctx=ctx)
    try:
        return b.build_simplified(int(k), **build).map_reads(max_mismatch)
    finally:
        b.close()


def map_reads_gapped(reads, k, max_edits=6, max_gap=3, end_gap=0, ctx=None, **build):
    """map_reads for reads with insertions and deletions: heads on neighbouring diagonals, at most max_gap apart, are joined and the
    read is verified as one alignment of at most max_edits edits: a readmap.GappedReadMap that speaks of segment 0 (ReadMap's methods,
    and gap_records(0), gap_pileup(0), indels(0); the rule and its limits: include/gasm.h "Gapped read mapping").  end_gap > 0: one gap
    of at most end_gap bases is also tried at each end of every chain, which places most reads with an indel within k of an end
    ("End gaps"; end_records(0), end_counters(0)).  build: as for contig_graph."""
    from .batch import SegmentBatch
    b = SegmentBatch.from_strings([list(reads)], ctx=ctx)
    try:
        return b.build_simplified(int(k), **build).map_reads_gapped(max_edits, max_gap, end_gap)
    finally:
        b.close()


def align_reads(reads, k, max_edits=6, max_gap=3, end_gap=3, ctx=None, **build):
    """map_reads_gapped that keeps every read's alignment: a readmap.AlignedReadMap that speaks of segment 0 (GappedReadMap's methods, and
    pieces(0), cigars(0), to_sam(0, reads), insert_pileup(0), insertions(0), consensus(0) with the insertions applied; include/gasm.h
    "Alignments").  build: as for contig_graph."""
    from .batch import SegmentBatch
    b = SegmentBatch.from_strings([list(reads)], ctx=ctx)
    try:
        return b.build_simplified(int(k), **build).align_reads(max_edits, max_gap, end_gap)
    finally:
        b.close()


def calc_breakscore_mapped(reads, k, kmer=8, tables=None, max_edits=6, max_gap=3, partial=False, ctx=None, end_gap=0, **build):
    """breakage scores of the contigs of one segment's reads (a list of str) from the reads' mapped starts: build, gapped mapping
    within max_edits edits and gaps of at most max_gap, mapped scoring — a readmap.MappedScores that speaks of segment 0 (scores(),
    score_fixed(), starts(0), counters(0), scored_fraction(0), window_counts(0, c); the rule and its limits: include/gasm.h "Mapped
    scoring").  A read with errors scores where its first base lies; calc_breakscore scores it only as an exact substring.  tables,
    partial: as SegmentBatch.score_mapped; end_gap: as SegmentBatch.map_reads_gapped (above 0 a read with an indel near its start is
    placed, with its break on the right base); build: as for contig_graph."""
    from .batch import SegmentBatch
    b = SegmentBatch.from_strings([list(reads)], ctx=ctx)
    try:
        b.build_simplified(int(k), **build).map_reads_gapped(max_edits, max_gap, end_gap)
        return b.score_mapped(kmer, tables, "gapped", partial)
    finally:
        b.close()


def resolve_repeats(reads, k, min_support=2, ctx=None, **build):
    """the contigs of one segment's reads with the repeats shorter than a read put back into their flanks, where the reads that run
    through a repeat say so unambiguously (links.ContigLinks.resolve_repeats: the rule and its limits); a sorted list of str.
    build: as for contig_graph."""
    return contig_graph(reads, k, None, ctx, **build)[1].resolve_repeats(0, min_support)


def resolve_repeats_paired(reads, k, min_support=2, max_insert=None, ctx=None, **build):
    """the contigs of one segment's PAIRED reads (a list of str: reads 2p and 2p + 1 are the mates of pair p, forward-reverse) with the
    repeats put back into their flanks where the read pairs say so unambiguously — repeats longer than a read among them
    (pairs.PairPlaces.resolve_repeats: the rule and its limits); a sorted list of str.  max_insert: as SegmentBatch.place_pairs;
    build: as for contig_graph."""
    from .batch import SegmentBatch
    b = SegmentBatch.from_strings([list(reads)], ctx=ctx)
    try:
        cl = b.build_simplified(int(k), **build).contig_links()
        return b.place_pairs(max_insert).resolve_repeats(0, cl, min_support)
    finally:
        b.close()
