"""The quality-trimming rule of the ingest as plain Python loops, written from the rule's text (include/gasm.h, "Quality trimming at
ingest"), not from csrc/seqio.cpp: what tests/test_trim_host.py holds the host reader to and tests/test_trim_gpu.py the device path.

A file is a list of records (seq: bytes, qual: bytes or None for FASTA), as the reader takes them: CR and trailing blanks gone."""

STATS = ("records", "kept", "dropped_non_acgt", "dropped_short", "dropped_mate", "bases_in", "bases_kept", "bases_dropped", "trimmed5", "trimmed3",
         "reads_trimmed")
QUAL_BINS = 94
KEPT, NON_ACGT, SHORT, MATE = "kept", "non_acgt", "short", "mate"
ERR_INVALID, ERR_NON_ACGT = -1, -2


class TrimError(Exception):
    """what the reader refuses: status (ERR_INVALID / ERR_NON_ACGT) and, for a malformed record, its index"""

    def __init__(self, status, record=None):
        super().__init__(f"status {status}, record {record}")
        self.status, self.record = status, record


def quality_mode(trim_q3=0, trim_q5=0, quality_hist=False, **_):
    return trim_q3 > 0 or trim_q5 > 0 or bool(quality_hist)


def base_quality(seq, qual, i, phred_offset):
    if seq[i] not in b"ACGTacgt":
        return 0
    return qual[i] - phred_offset


def trim_span(seq, qual, trim_q3=0, trim_q5=0, phred_offset=33):
    """(a, e): the raw cuts of one record"""
    L = len(seq)
    e = L
    if trim_q3 > 0:
        s, best = 0, 0
        i = L - 1
        while i >= 0:
            s += trim_q3 - base_quality(seq, qual, i, phred_offset)
            if s < 0:
                break
            if s > best:
                best, e = s, i
            i -= 1
    a = 0
    if trim_q5 > 0:
        s, best = 0, 0
        for i in range(L):
            s += trim_q5 - base_quality(seq, qual, i, phred_offset)
            if s < 0:
                break
            if s > best:
                best, a = s, i + 1
    return a, e


def classify_file(records, trim_q3=0, trim_q5=0, min_len=0, pairs=False, phred_offset=33, quality_hist=False, non_acgt="drop"):
    """per record (class, L, trimmed5, span length, trimmed3) and the file's quality histogram; TrimError for what the rule refuses,
    met in record order"""
    qm = quality_mode(trim_q3, trim_q5, quality_hist)
    rows, hist = [], [0] * QUAL_BINS
    for r, (seq, qual) in enumerate(records):
        L = len(seq)
        a, e = 0, L
        if qm and qual is not None:
            if len(qual) != L:
                raise TrimError(ERR_INVALID, r)
            for b in qual:
                if b < phred_offset or b > phred_offset + 93:
                    raise TrimError(ERR_INVALID, r)
            if quality_hist:
                for b in qual:
                    hist[b - phred_offset] += 1
            a, e = trim_span(seq, qual, trim_q3, trim_q5, phred_offset)
        if a >= e:
            t3, t5, n = L - e, min(a, e), 0
        else:
            t3, t5, n = L - e, a, e - a
        cls = KEPT
        if any(c not in b"ACGTacgt" for c in seq[t5:t5 + n]):
            if non_acgt == "error":
                raise TrimError(ERR_NON_ACGT, r)
            cls = NON_ACGT
        elif n < min_len:
            cls = SHORT
        rows.append([cls, L, t5, n, t3])
    if pairs:
        if len(records) % 2:
            raise TrimError(ERR_INVALID, None)
        first = [row[0] for row in rows]
        for r, row in enumerate(rows):
            if first[r] == KEPT and first[r ^ 1] in (NON_ACGT, SHORT):
                row[0] = MATE
    return [tuple(row) for row in rows], hist


def reads(records, rows):
    """the kept spans, upper case, in file order"""
    return [seq[t5:t5 + n].upper() for (seq, _), (cls, _, t5, n, _) in zip(records, rows) if cls == KEPT]


def stats(rows):
    """the eleven counters, in STATS' order"""
    c = dict.fromkeys(STATS, 0)
    for cls, L, t5, n, t3 in rows:
        c["records"] += 1
        c["bases_in"] += L
        c["trimmed5"] += t5
        c["trimmed3"] += t3
        if cls == KEPT:
            c["kept"] += 1
            c["bases_kept"] += n
            if t5 > 0 or t3 > 0:
                c["reads_trimmed"] += 1
        else:
            c["dropped_" + cls] += 1
            c["bases_dropped"] += n
    return [c[name] for name in STATS]


def suggest_trim_q(hist):
    """the largest q with at most 5 % of the bases below it, clamped to 2..30"""
    total = sum(hist)
    best = 0
    for q in range(QUAL_BINS + 1):
        if 20 * sum(hist[:q]) <= total:
            best = q
    return max(2, min(30, best))
