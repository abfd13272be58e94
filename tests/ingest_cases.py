"""Inputs and expectations of the device-ingest tests (tests/test_ingest_seams_gpu.py, preconditions and witnesses in
tests/test_ingest_cases_host.py): sequence files sized by the constants of csrc/ingest.hip, each with what it must yield BY CONSTRUCTION —
the kept reads, read_off, seg_read_off, dropped and the packed words (synth.pack_2bit of the kept bases).  No libgasm here and no test
functions.  The constants are restated below; test_ingest_cases_host.py holds them against the text of ingest.hip.

A case is a list of files read in ONE call (one file per segment).  The three big cases are made with numpy (a tiled byte matrix, the
sequence columns overwritten); the small ones record by record."""
import gzip
import os
from dataclasses import dataclass, field

import numpy as np

from genomeassembler_dev_amd import synth

CH = 4096                      # bytes per workgroup of the newline count (16 per thread)
SB = 8192                      # elements per block of the device-wide scans
SCAN_TRIP = 1024               # block sums per trip of k_ing_scan_sums (its workgroup size)
WG_PER_CU = 16                 # k_ing_pack and k_ing_append launch min(ceil(nw / 256), n_cu * WG_PER_CU) workgroups of 256 threads
PAD_WORDS = 4                  # padding words the pack launch counts in (nw = ceil(bases / 32) + 4)
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_IS_ACGT = np.zeros(256, dtype=bool)
_IS_ACGT[_ACGT] = True


def scan_trips(n):
    """trips of the carry loop of k_ing_scan_sums over an array of n elements (scan_u32: nb = max(1, ceil(n / SB)) block sums)"""
    nb = max(1, -(-n // SB))
    return -(-nb // SCAN_TRIP)


def pack_grid(bases, n_cu):
    """(words the pack launch covers, workgroups it launches) for a file of `bases` kept bases"""
    nw = (bases + 31) // 32 + PAD_WORDS
    return nw, min(-(-nw // 256), n_cu * WG_PER_CU)


@dataclass
class File:
    name: str
    data: bytes                      # the text (before gzip, if the name ends in .gz)
    kept_bases: np.ndarray           # ASCII upper case, kept reads back to back
    kept_lens: np.ndarray            # their lengths
    dropped: int
    regular: bool = True             # False: blank lines between FASTQ records, the host reader's file
    recs: list = None                # small files: every record in file order, upper case, the dropped ones included
    note: dict = field(default_factory=dict)


@dataclass
class Case:
    files: list
    bases: np.ndarray
    read_off: np.ndarray
    seg_read_off: np.ndarray
    dropped: int
    words: np.ndarray
    on_device: list
    note: dict = field(default_factory=dict)

    def write(self, directory):
        """the files under `directory` -> their paths, in the order of the call"""
        paths = []
        for f in self.files:
            p = os.path.join(str(directory), f.name)
            if f.name.endswith(".gz"):
                with gzip.open(p, "wb", compresslevel=1) as g:
                    g.write(f.data)
            else:
                with open(p, "wb") as g:
                    g.write(f.data)
            paths.append(p)
        return paths

    def reads(self):
        """the kept reads as a list of bytes (small cases)"""
        raw = self.bases.tobytes()
        return [raw[int(self.read_off[i]):int(self.read_off[i + 1])] for i in range(len(self.read_off) - 1)]


def assemble(files, **note):
    lens = np.concatenate([np.asarray(f.kept_lens, dtype=np.uint64) for f in files]) if files else np.zeros(0, np.uint64)
    read_off = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=read_off[1:])
    seg = np.zeros(len(files) + 1, dtype=np.uint64)
    np.cumsum(np.array([len(f.kept_lens) for f in files], dtype=np.uint64), out=seg[1:])
    bases = np.concatenate([np.asarray(f.kept_bases, dtype=np.uint8).reshape(-1) for f in files])
    assert bases.size == int(read_off[-1])
    words = synth.pack_2bit(bases) if bases.size else np.zeros(0, np.uint64)
    return Case(files, bases, read_off, seg, int(sum(f.dropped for f in files)), words, [f.regular for f in files], dict(note))


# ---- small files, record by record

def _kept(rec):
    return bool(_IS_ACGT[np.frombuffer(rec, dtype=np.uint8)].all())


def _small(name, data, recs, regular=True, **note):
    """a small file and what its records yield: a record with a byte outside ACGT is dropped, every other one kept (empty ones too)"""
    recs = [bytes(r) for r in recs]
    kept = [r for r in recs if _kept(r)]
    return File(name, bytes(data), np.frombuffer(b"".join(kept), dtype=np.uint8), np.array([len(r) for r in kept], dtype=np.uint64),
                len(recs) - len(kept), regular, recs, dict(note))


def fastq_text(recs, eol=b"\n", final_eol=True, gap=False, names=None, lower=False):
    """four-line records; gap: a blank line between records (what only the host reader takes)"""
    lines = []
    for i, s in enumerate(recs):
        if gap and i:
            lines.append(b"")
        lines += [names[i] if names else b"@r%d" % i, s.lower() if lower else s, b"+", b"I" * len(s)]
    return eol.join(lines) + (eol if final_eol else b"")


def fasta_text(recs, width=60, eol=b"\n", final_eol=True, names=None, lower=False):
    lines = []
    for i, s in enumerate(recs):
        lines.append(names[i] if names else b">r%d" % i)
        s = s.lower() if lower else s
        lines += [s[j:j + width] for j in range(0, len(s), width)]
    return eol.join(lines) + (eol if final_eol and lines else b"")


def _seq(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


# ---- the three big files

def scan_carry_fastq(n_rec=2_200_000):
    """n_rec four-line records of three bases, every 1000th with an N (dropped): 4 n_rec + 1 lines, so the scan of the per-line base counts
    (plen -> pbase) goes through the carry loop twice, with bases and dropped records on both sides of the trip"""
    rng = np.random.default_rng(20)
    m = np.tile(np.frombuffer(b"@\nACG\n+\nIII\n", dtype=np.uint8), (n_rec, 1))
    m[:, 2:5] = _ACGT[rng.integers(0, 4, (n_rec, 3))]
    bad = np.arange(n_rec) % 1000 == 999
    m[bad, 3] = ord("N")
    kept = m[~bad, 2:5]
    f = File("carry.fastq", m.tobytes(), kept.reshape(-1), np.full(kept.shape[0], 3, dtype=np.uint64), int(bad.sum()))
    return assemble([f], n_lines=4 * n_rec + 1, n_rec=n_rec, first_dropped=999)


def scan_carry_fasta(n_rec=8_400_000):
    """n_rec two-line records, '>' then one to three bases, every 1000th with an N.  More than SB * SCAN_TRIP RECORDS, not only lines: the
    scans of hdr (2 n_rec + 1 lines), of plen and of keep (n_rec records) all carry, and rec_line[hdr_ex[i]] is indexed past the first trip"""
    rng = np.random.default_rng(21)
    m = np.tile(np.frombuffer(b">\nACG\n", dtype=np.uint8), (n_rec, 1))
    m[:, 2:5] = _ACGT[rng.integers(0, 4, (n_rec, 3))]
    lens = rng.integers(1, 4, n_rec)
    bad = np.arange(n_rec) % 1000 == 500
    m[bad, 2] = ord("N")
    there = np.ones(m.shape, dtype=bool)
    there[:, 3] = lens >= 2
    there[:, 4] = lens >= 3
    seq = there[:, 2:5] & ~bad[:, None]
    f = File("carry.fa", m[there].tobytes(), m[:, 2:5][seq], lens[~bad].astype(np.uint64), int(bad.sum()))
    return assemble([f], n_lines=2 * n_rec + 1, n_rec=n_rec)


def pack_stride_fasta(n_cu):
    """a 13-base file, then records of 100 000 bases on 1000-base lines, about 1.03 * n_cu * 16 * 256 * 32 bases: more words than the pack
    and the append launches have threads, appended at base 13 (the append's s < 0 word, then its strided trips)"""
    rng = np.random.default_rng(22)
    target = int(1.03 * n_cu * WG_PER_CU * 256 * 32)
    n_rec = -(-target // 100_000)
    body = np.empty((n_rec * 100, 1001), dtype=np.uint8)
    body[:, :1000] = _ACGT[rng.integers(0, 4, (n_rec * 100, 1000), dtype=np.uint8)]
    body[:, 1000] = 10
    m = np.empty((n_rec, 2 + 100 * 1001), dtype=np.uint8)
    m[:, 0], m[:, 1] = ord(">"), 10
    m[:, 2:] = body.reshape(n_rec, -1)
    big = File("stride.fa", m.tobytes(), body[:, :1000].reshape(-1), np.full(n_rec, 100_000, dtype=np.uint64), 0)
    front = _small("front.fa", b">s\nACGTACGTACGTA\n", [b"ACGTACGTACGTA"])
    return assemble([front, big], n_cu=n_cu, big_bases=n_rec * 100_000, dst_off=13)


# ---- the append over its cases

CLASSES = ("zero", "inside", "fills", "spills", "big_aligned", "big_unaligned")


def append_class(r, n):
    """class of a file of n kept bases appended at residue r = dst_off % 32"""
    if n == 0:
        return "zero"
    if n < 32:
        return "inside" if r + n < 32 else "fills" if r + n == 32 else "spills"
    return "big_aligned" if (r + n) % 32 == 0 else "big_unaligned"


def append_pairs():
    """every (residue, class) that exists: residue 0 has no 'fills' or 'spills', residue 1 no 'spills', residue 31 no 'inside'"""
    return {(r, append_class(r, n)) for r in range(32) for n in range(0, 97)}


def append_sweep():
    """at most 400 files of 1 to 3 reads in one call, so that every (dst_off % 32, class) of append_pairs() is met.  Files at residues
    3, 7, .. 31 (all but the 'zero' and 'big_aligned' ones) are FASTQ with a blank line between the records — the host reader's, appended
    by the fallback launch; every 23rd file is gzip.  note['coverage']: (residue, class) -> file indices; note['irregular']: the pairs the
    fallback met"""
    rng = np.random.default_rng(23)
    need = append_pairs()
    files, coverage, irregular = [], {}, set()
    cur = 0
    while need:
        cands = [n for n in range(0, 97) if (cur % 32, append_class(cur % 32, n)) in need]
        if cands:
            left = lambda n: sum(1 for p in need if p[0] == (cur + n) % 32 and p != (cur % 32, append_class(cur % 32, n)))
            n = max(cands, key=lambda n: (left(n), -n))
        else:
            n = min(d for d in range(1, 32) if any(p[0] == (cur + d) % 32 for p in need))
        r, i = cur % 32, len(files)
        c = append_class(r, n)
        need.discard((r, c))
        coverage.setdefault((r, c), []).append(i)
        irr = r % 4 == 3 and c not in ("zero", "big_aligned")
        ext = ".gz" if i % 23 == 5 else ""
        if n == 0:
            v = len(coverage[(r, c)]) + r
            if v % 4 == 0:
                f = _small(f"z{i}.fastq{ext}", fastq_text([b""]), [b""])
            elif v % 4 == 1:
                recs = [_seq(rng, 3) + b"N", b"N" + _seq(rng, 5)]
                f = _small(f"z{i}.fastq{ext}", fastq_text(recs), recs)
            elif v % 4 == 2:
                f = _small(f"z{i}.fa{ext}", fasta_text([b"", b"", b""]), [b"", b"", b""])
            else:
                f = _small(f"z{i}.fa{ext}", b"", [])
        else:
            k = max(2, 1 + i % 3) if irr else 1 + i % 3
            cuts = sorted(int(x) for x in rng.integers(0, n + 1, k - 1))
            s = _seq(rng, n)
            recs = [s[a:b] for a, b in zip([0] + cuts, cuts + [n])]
            eol = b"\r\n" if i % 4 >= 2 else b"\n"
            if irr:
                irregular.add((r, c))
                f = _small(f"g{i}.fastq{ext}", fastq_text(recs, eol=eol, gap=True, lower=i % 5 == 0), recs, regular=False)
            elif i % 2 == 0:
                f = _small(f"s{i}.fastq{ext}", fastq_text(recs, eol=eol, final_eol=i % 3 != 0, lower=i % 5 == 0), recs)
            else:
                f = _small(f"s{i}.fa{ext}", fasta_text(recs, width=(7, 1000)[i % 4 == 1], eol=eol, final_eol=i % 3 != 0, lower=i % 5 == 0), recs)
        f.note.update(residue=r, klass=c, n_bases=n)
        files.append(f)
        cur += n
    return assemble(files, coverage=coverage, irregular=irregular)


# ---- totals of zero and exact fits

def zero_and_exact():
    """the totals of zero (every read dropped; empty records only; an empty file) and the exact fits (bases that fill the file's last word;
    a kept record that ends on a word boundary, followed by dropped and empty records; a word gathered from 32 one-base lines), each its
    own file, kept files between them.  note['all_dropped']: index of the FASTQ file whose every read is dropped"""
    rng = np.random.default_rng(24)
    files = []

    def kept_file():
        i = len(files)
        recs = [_seq(rng, 10 + i % 7), _seq(rng, 9)]
        files.append(_small(f"k{i}.fastq", fastq_text(recs), recs) if i % 2 == 0 else _small(f"k{i}.fa", fasta_text(recs, width=8), recs))

    def add(name, data, recs, **note):
        files.append(_small(name, data, recs, what=name.split(".")[0], **note))
        kept_file()

    kept_file()
    recs = [_seq(rng, 4) + b"N" + _seq(rng, 3), b"N", _seq(rng, 40) + b"RY"]
    add("alldrop.fastq", fastq_text(recs), recs)
    add("alldrop.fa", fasta_text(recs, width=16), recs)
    add("empties.fastq", fastq_text([b"", b"", b""]), [b"", b"", b""])
    add("empties.fa", fasta_text([b"", b"", b""]), [b"", b"", b""])
    add("nothing.fastq", b"", [])
    recs = [_seq(rng, 20), _seq(rng, 12), _seq(rng, 32)]
    add("fits64.fa", fasta_text(recs, width=9), recs)
    recs = [_seq(rng, 31), _seq(rng, 1), _seq(rng, 64)]
    add("fits96.fastq", fastq_text(recs, final_eol=False), recs)
    # a kept record ends on base 32 of the file; then dropped and empty records (zero-length pieces on many lines), then a kept one
    recs = [_seq(rng, 32), _seq(rng, 25) + b"N" + _seq(rng, 25), b"", b"", b"NNNN", _seq(rng, 5), b"", _seq(rng, 27), b"N", b"", _seq(rng, 3)]
    add("boundary.fa", fasta_text(recs, width=10), recs)
    add("boundary.fastq", fastq_text(recs), recs)
    # a word from 32 one-base lines: a FASTA record on 40 lines of one base, and 40 FASTQ reads of one base
    recs = [_seq(rng, 40), _seq(rng, 33)]
    add("onebase.fa", fasta_text(recs, width=1), recs)
    recs = [_seq(rng, 1) for _ in range(40)]
    add("onebase.fastq", fastq_text(recs), recs)
    return assemble(files, all_dropped=[f.name for f in files].index("alldrop.fastq"))


# ---- fixed positions of the newline count

SEAM_POSITIONS = (15, 16, 4094, 4095, 4096, 4097, 4098, 8191, 8192, 8193)
EXACT_SIZES = (4096, 4097, 8192)


def _exact_fasta(rng, size, final_nl):
    """a FASTA text of exactly `size` bytes: '>s', lines of 60 bases, a last line that ends the text with or without its newline"""
    room = size - 3 - (1 if final_nl else 0)
    full, rest = divmod(room, 61)
    if rest == 0:
        full, rest = full - 1, 61
    s = _seq(rng, full * 60 + rest)
    lines = [b">s"] + [s[j:j + 60] for j in range(0, full * 60, 60)] + [s[full * 60:]]
    return b"\n".join(lines) + (b"\n" if final_nl else b""), [s]


def _exact_fastq(rng, size, final_nl):
    """a FASTQ text of exactly `size` bytes: records of 50 bases, then one sized to end the text there"""
    recs, names = [_seq(rng, 50) for _ in range(20)], [b"@r"] * 20
    room = size - 20 * (3 + 51 + 2 + 51) - (1 if final_nl else 0)            # '@..\n' seq '\n+\n' qual
    name = b"@q" if (room - 6) % 2 == 0 else b"@qq"
    m = (room - len(name) - 4) // 2
    recs.append(_seq(rng, m))
    names.append(name)
    return fastq_text(recs, final_eol=final_nl, names=names), recs


def chunk_seams():
    """texts whose chosen newline sits at a fixed byte: the newline of a padded first header (FASTA and FASTQ, LF and CRLF — at 4096 the
    CR is the last byte of a chunk and the LF the first of the next) and of a first sequence line (FASTA) at every SEAM_POSITIONS; texts of
    exactly EXACT_SIZES bytes with and without a final newline.  Each file's note says what sits where"""
    rng = np.random.default_rng(25)
    files = []
    for pos in SEAM_POSITIONS:
        for crlf in (False, True):
            eol = b"\r\n" if crlf else b"\n"
            pad = b"h" * (pos - 1 - (1 if crlf else 0))
            recs = [_seq(rng, 37), _seq(rng, 3), _seq(rng, 2) + b"N", _seq(rng, 33)]
            tag = f"{pos}{'c' if crlf else ''}"
            files.append(_small(f"h{tag}.fa", fasta_text(recs, width=10, eol=eol, names=[b">" + pad, b">b", b">c", b">d"]), recs, pos=pos, crlf=crlf))
            files.append(_small(f"h{tag}.fastq", fastq_text(recs, eol=eol, names=[b"@" + pad, b"@b", b"@c", b"@d"]), recs, pos=pos, crlf=crlf))
            if pos > 16:
                first = pos - 1 - 2 * len(eol)                  # '>s' eol, `first` bases, eol: its LF is byte `pos`
                recs = [_seq(rng, first + 45), _seq(rng, 7)]
                text = b">s" + eol + recs[0][:first] + eol + recs[0][first:] + eol + b">t" + eol + recs[1] + eol
                files.append(_small(f"l{tag}.fa", text, recs, pos=pos, crlf=crlf))
    for size in EXACT_SIZES:
        for final_nl in (True, False):
            for kind, make in (("fa", _exact_fasta), ("fastq", _exact_fastq)):
                text, recs = make(rng, size, final_nl)
                files.append(_small(f"x{size}{'n' if final_nl else ''}.{kind}", text, recs, size=size, final_nl=final_nl))
    return assemble(files)


SCAN_LINES = (8191, 8192, 8193, 16384, 16385)


def _fasta_lines(n_lines, headers, final_nl):
    """a FASTA text the device counts n_lines lines in (newlines + 1; with final_nl the last one is the empty line behind the last newline):
    headers on the lines of `headers`, on line 0 and on every line i with i % 997 == 500; sequence lines of one to four bases, an empty
    one where i % 1111 == 7, an N where i % 2500 == 1234"""
    text_lines = n_lines - 1 if final_nl else n_lines
    lines, recs, cur = [], [], None
    for i in range(text_lines):
        if i == 0 or i % 997 == 500 or i in headers:
            if cur is not None:
                recs.append(b"".join(cur))
            cur = []
            lines.append(b">%d" % i)
        else:
            s = b"" if i % 1111 == 7 else b"N" if i % 2500 == 1234 else b"ACGTTGCAGTCA"[i % 9:i % 9 + 1 + (i * 7) % 4]
            lines.append(s)
            cur.append(s)
    recs.append(b"".join(cur))
    return b"\n".join(lines) + (b"\n" if final_nl else b""), recs


def scan_seams():
    """FASTA files of exactly SCAN_LINES lines (as the device counts them) with a header on line 8191 (the last element of the scans' first
    block) or 8192 (the first of the second), or on the last line where the file is shorter; FASTQ files of 8192, 8193 and 8196 lines"""
    files = []
    for n in SCAN_LINES:
        for final_nl in (False, True):
            last_text = n - 2 if final_nl else n - 1
            sets = [{h} for h in (8191, 8192) if h <= last_text] or [{last_text}]
            if n == 16385:
                sets.append({8191, 8192, 16383, last_text})
            for hs in sets:
                text, recs = _fasta_lines(n, hs, final_nl)
                files.append(_small(f"n{n}{'n' if final_nl else ''}_{'_'.join(map(str, sorted(hs)))}.fa", text, recs, n_lines=n, headers=sorted(hs)))
    rng = np.random.default_rng(26)
    for n_rec, final_nl in ((2048, False), (2048, True), (2049, False)):
        recs = [_seq(rng, 1 + i % 5) if i % 300 != 7 else b"AN" for i in range(n_rec)]
        files.append(_small(f"q{n_rec}{'n' if final_nl else ''}.fastq", fastq_text(recs, final_eol=final_nl), recs, n_lines=4 * n_rec + (1 if final_nl else 0)))
    return assemble(files)
