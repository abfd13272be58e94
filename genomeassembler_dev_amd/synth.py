"""Seeded synthetic inputs: a 50 kb ACGT segment with planted repeat structure so the graph branches the
way a T2T segment does, and fixed-length error-free forward-strand reads.  The reference's own simulator
(lib/GenerateReads.R:235-313) needs R, Biostrings and the BSgenome T2T package, none of which exist here; what is kept
of it: n = ceil(coverage * L / read_len) start positions (:302), starts whose read would run past the end are dropped
(:310-313), optional start weights = normalised 8-mer probability of the window beginning at the start (:243-259)."""
import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_segment(seed, length=50000, n_short=20, short_len=300, n_long=5, long_len=2000, tandem_unit=6, tandem_len=1000,
                 planted=True):
    """uint8 ASCII array.  planted=True copies one 300-bp block to 20 places, one 2-kb block to 5 places and lays one
    1-kb tandem repeat of a 6-bp unit, at seeded random offsets (recipe printed by bench.py)."""
    rng = np.random.Generator(np.random.MT19937(seed))
    g = _ACGT[rng.integers(0, 4, size=length)]
    if planted and length >= 4 * long_len:
        blk = _ACGT[rng.integers(0, 4, size=short_len)]
        for p in rng.integers(0, length - short_len, size=n_short):
            g[p:p + short_len] = blk
        blk = _ACGT[rng.integers(0, 4, size=long_len)]
        for p in rng.integers(0, length - long_len, size=n_long):
            g[p:p + long_len] = blk
        unit = _ACGT[rng.integers(0, 4, size=tandem_unit)]
        p = int(rng.integers(0, length - tandem_len))
        g[p:p + tandem_len] = np.resize(unit, tandem_len)
    return g


def plant_repeat(genome, rep_len, seed, min_gap=200):
    """a copy of `genome` in which one rep_len-base stretch occurs twice, more than min_gap bases apart (the second copy overwrites
    what was there); returns (genome, position of the first copy, position of the second) — the README's repeat-resolution example"""
    rng = np.random.Generator(np.random.MT19937(seed))
    g = genome.copy()
    L = g.size
    p1 = int(rng.integers(min_gap, L // 2 - rep_len))
    p2 = int(rng.integers(p1 + rep_len + min_gap + 1, L - rep_len - min_gap))
    g[p2:p2 + rep_len] = g[p1:p1 + rep_len]
    return g, p1, p2


def simulate_pairs(genome, read_len, coverage, insert_mean, insert_sd, seed, both_strands=False):
    """(2 * pairs, read_len) uint8 array of forward-reverse read pairs, interleaved (rows 2p and 2p + 1 are the mates of pair p): fragments
    with uniform starts and normal lengths (rounded, at least read_len; a fragment that runs past the genome's end is dropped), with
    both_strands each from either strand; mate 1 = the fragment's first read_len bases, mate 2 = the reverse complement of its last —
    the README's paired example"""
    rng = np.random.Generator(np.random.MT19937(seed))
    L = genome.size
    n = int(np.ceil(coverage * L / (2 * read_len)))
    starts = rng.integers(0, L, size=n)
    ins = np.maximum(read_len, np.rint(rng.normal(insert_mean, insert_sd, size=n))).astype(np.int64)
    flip = rng.integers(0, 2, size=n) if both_strands else np.zeros(n, dtype=np.int64)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    keep = starts + ins <= L
    s, d, f = starts[keep], ins[keep], flip[keep].astype(bool)
    j = np.arange(read_len)
    head = genome[s[:, None] + j]                                   # the fragment's first bases on the genome's strand ...
    tail = comp[genome[(s + d - 1)[:, None] - j]]                   # ... and the reverse complement of its last
    out = np.empty((2 * s.size, read_len), dtype=np.uint8)
    out[0::2] = np.where(f[:, None], tail, head)                    # (a flipped fragment starts where the other ends)
    out[1::2] = np.where(f[:, None], head, tail)
    return out


def simulate_reads(genome, read_len, coverage, seed, weights=None):
    """(n_reads, read_len) uint8 array of reads; starts uniform, or drawn with `weights` (one per start position)."""
    L = genome.size
    rng = np.random.Generator(np.random.MT19937(seed))
    n = int(np.ceil(coverage * L / read_len))
    if weights is None:
        starts = rng.integers(0, L, size=n)
    else:
        w = np.asarray(weights, dtype=np.float64)
        starts = rng.choice(L, size=n, p=w / w.sum())
    starts = starts[starts + read_len <= L]
    idx = starts[:, None] + np.arange(read_len)[None, :]
    return genome[idx]


def simulate_reads_indel(genome, read_len, coverage, seed, sub_rate, indel_rate):
    """(n_reads, read_len) uint8 array of reads with substitutions, insertions and deletions; starts uniform.  Every read is written
    by read_len + 32 steps along the genome, each of which is, with probability indel_rate, an insertion (a random base, the genome
    does not advance) or a deletion (the genome base is skipped) with equal chances, and else copies the genome base, changed with
    probability sub_rate to one of the three others; the first read_len bases written are the read.  A start too close to the
    genome's end for all steps, or (next to never) a read with fewer than read_len bases written, is left out."""
    L, M = genome.size, read_len + 32
    rng = np.random.Generator(np.random.MT19937(seed))
    n = int(np.ceil(coverage * L / read_len))
    starts = rng.integers(0, L, size=n)
    starts = starts[starts + M <= L]
    u = rng.random((starts.size, M))
    ins, dele = u < indel_rate / 2, (u >= indel_rate / 2) & (u < indel_rate)
    sub = ~ins & ~dele & (rng.random((starts.size, M)) < sub_rate)
    shift = rng.integers(1, 4, size=(starts.size, M))
    rand = rng.integers(0, 4, size=(starts.size, M))
    gpos = starts[:, None] + np.cumsum(~ins, axis=1) - (~ins)                # the genome base of every step
    code = np.searchsorted(_ACGT, genome[np.minimum(gpos, L - 1)])
    code = np.where(ins, rand, np.where(sub, (code + shift) % 4, code))
    opos = np.cumsum(~dele, axis=1) - (~dele)                                # where a step that writes a base writes it
    keep = (~dele).sum(axis=1) >= read_len
    out = np.zeros((starts.size, read_len), dtype=np.uint8)
    rows, cols = np.nonzero(~dele & (opos < read_len))
    out[rows, opos[rows, cols]] = _ACGT[code[rows, cols]]
    return out[keep]


def simulate_qualities(n_reads, read_len, seed, q_start=38, q_end=12, tail_frac=0.3):
    """(n_reads, read_len) int64 base qualities in the shape of a short-read run: q_start over the read's head, then a straight decline
    to q_end over its last tail_frac, each read shifted as a whole by a jitter of -3..3 and each base by -2..2; clipped to 2..41."""
    rng = np.random.Generator(np.random.MT19937(seed))
    tail = max(1, int(round(read_len * tail_frac)))
    prof = np.full(read_len, float(q_start))
    prof[read_len - tail:] = np.linspace(q_start, q_end, tail + 1)[1:]
    q = np.rint(prof)[None, :].astype(np.int64) + rng.integers(-3, 4, size=(n_reads, 1)) + rng.integers(-2, 3, size=(n_reads, read_len))
    return np.clip(q, 2, 41)


def apply_quality_errors(reads, quals, seed):
    """the reads (uint8 ASCII, (n, read_len)) with base i of a read substituted, with probability 10^(-q_i / 10), by one of the three
    other bases: errors where the qualities say they are.  Returns (reads with errors, bool array of the substituted bases)."""
    rng = np.random.Generator(np.random.MT19937(seed))
    reads = np.asarray(reads, dtype=np.uint8)
    err = rng.random(reads.shape) < 10.0 ** (-np.asarray(quals, dtype=np.float64) / 10.0)
    shift = rng.integers(1, 4, size=reads.shape)
    code = np.searchsorted(_ACGT, reads)
    return np.where(err, _ACGT[(code + shift) % 4], reads).astype(np.uint8), err


def write_fastq(path, reads, quals, names=None, phred_offset=33):
    """four-line FASTQ: reads and quals are sequences of equal length (rows of arrays, or bytes / lists of int of any lengths)"""
    with open(path, "wb") as f:
        for i, (r, q) in enumerate(zip(reads, quals)):
            name = names[i] if names is not None else f"r{i}"
            seq = bytes(r) if isinstance(r, (bytes, bytearray)) else np.asarray(r, dtype=np.uint8).tobytes()
            qs = (np.asarray(q, dtype=np.int64) + phred_offset).astype(np.uint8).tobytes()
            f.write(b"@" + str(name).encode() + b"\n" + seq + b"\n+\n" + qs + b"\n")
    return path


def make_batch(n_segments, seg_len, read_len, coverage, seed0=1234, planted=True):
    """reads of n_segments segments as one (total_reads, read_len) uint8 array + seg_read_off + the genomes"""
    reads, off, genomes = [], [0], []
    for s in range(n_segments):
        g = make_segment(seed0 + s, seg_len, planted=planted)
        r = simulate_reads(g, read_len, coverage, 10_000_019 + seed0 + s)
        genomes.append(g)
        reads.append(r)
        off.append(off[-1] + r.shape[0])
    return np.concatenate(reads, axis=0), np.array(off, dtype=np.uint64), genomes


def pack_2bit(ascii_bases):
    """ASCII ACGT (uint8, any shape, read after read) -> uint64 words, 32 bases per word, first base most significant
    (A=0 C=1 G=2 T=3): the layout gasm_batch_create_packed takes — a quarter of the bytes over PCIe"""
    a = np.ascontiguousarray(ascii_bases, dtype=np.uint8).reshape(-1)
    code = ((a >> 1) & 3) ^ ((a >> 2) & 1)
    n = code.size
    pad = (-n) % 32
    if pad:
        code = np.concatenate([code, np.zeros(pad, dtype=np.uint8)])
    c = code.reshape(-1, 32).astype(np.uint64)
    shifts = (62 - 2 * np.arange(32, dtype=np.uint64)).astype(np.uint64)
    return np.bitwise_or.reduce(c << shifts[None, :], axis=1)
