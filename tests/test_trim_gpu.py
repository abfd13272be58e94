"""Quality trimming at ingest on the device (csrc/ingest.hip: k_ing_qual_trim, a wave per record, and k_ing_trim_fold) against the host
reader under the same options, word for word, and against the rule restated in tests/trim_ref.py."""
import numpy as np
import pytest

import genomeassembler_dev_amd as ga
import trim_cases as tc
import trim_ref
from genomeassembler_dev_amd import seqio, synth

pytestmark = pytest.mark.gpu

OPTS = (dict(trim_q3=20, trim_q5=20), dict(trim_q3=20, trim_q5=20, min_len=31, pairs=True, quality_hist=True), dict(trim_q3=10, trim_q5=30, min_len=1),
        dict(trim_q3=25), dict(trim_q5=2, quality_hist=True), dict(quality_hist=True), dict(min_len=64, pairs=True))


def _same(paths, files=None, on_device=None, **opts):
    """the device path equals the host reader; both equal the rule where the records are given"""
    host = seqio.read_files(paths, **opts)
    dev = seqio.read_files_device(paths, **opts)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(dev[:3], host[:3])) and dev[3] == host[3]
    assert dev[-1] == host[-1], (dev[-1], host[-1])
    assert dev[4] == (on_device if on_device is not None else [True] * len(paths))
    if files is not None:
        tc.agrees(dev, files, **opts)
    return dev


def test_shaped_records(tmp_path):
    shaped = tc.shaped_records()
    records = [(s, q) for _, s, q in shaped]
    assert len(records) % 2 == 0
    nonl = tc.write(tmp_path, "shaped_nonl.fastq", tc.fastq_bytes(records, final_newline=False))
    crlf = tc.write(tmp_path, "shaped_crlf.fastq", tc.fastq_bytes(records, eol=b"\r\n"))
    for opts in OPTS:
        _same([nonl, crlf], [records, records], **opts)


def test_lengths_at_the_trip_seams(tmp_path):
    files = [tc.random_records(300 + i, 3000, lengths=(0, 1, 63, 64, 65, 128, 129, 200)) for i in range(2)]
    paths = [tc.write(tmp_path, "a.fastq", tc.fastq_bytes(files[0])), tc.write(tmp_path, "b.fastq.gz", tc.fastq_bytes(files[1], final_newline=False))]
    for opts in OPTS[:3]:
        _same(paths, files, **opts)


def test_every_append_residue_behind_a_trimmed_file(tmp_path):
    files = tc.residue_files()
    paths = [tc.write(tmp_path, f"res{i:02d}.fastq", tc.fastq_bytes(r)) for i, r in enumerate(files)]
    dev = _same(paths, files, trim_q3=20)
    assert [int(dev[1][2 * f]) % 32 for f in range(34)] == [f % 32 for f in range(34)]


def test_more_records_than_one_grid_trip(tmp_path):
    """9000 records: several trips of the kernel's grid-stride loop on any device it is sized for, and every workgroup flushing its
    histogram bins"""
    records = tc.random_records(9, 9000, lengths=(1, 31, 36, 65))
    path = tc.write(tmp_path, "many.fastq", tc.fastq_bytes(records))
    _same([path], [records], trim_q3=20, trim_q5=20, min_len=20, pairs=True, quality_hist=True)


def test_errors_are_the_host_readers(tmp_path):
    records = tc.random_records(10, 9000, lengths=(1, 31, 36, 65), n_rate=0)
    records = [(s.replace(b"N", b"A"), q) for s, q in records]

    def both(data, name="err.fastq", **opts):
        p = tc.write(tmp_path, name, data)
        with pytest.raises(ga.GasmError) as eh:
            seqio.read_files([p], **opts)
        with pytest.raises(ga.GasmError) as ed:
            seqio.read_files_device([p], **opts)
        assert ed.value.status == eh.value.status and str(ed.value) == str(eh.value)
        return str(ed.value)

    bad = list(records)
    for r in (8300, 5000, 777):                                            # three workgroups, in different trips of the grid
        s, q = bad[r]
        bad[r] = (s, q[:-1]) if r != 5000 else (s, b"\x7f" + q[1:])
    assert "record 777 " in both(tc.fastq_bytes(bad), trim_q3=20)
    assert "record 777 " in both(tc.fastq_bytes(bad), quality_hist=True)
    bad[777] = records[777]
    bad[4000] = (b"ACGTNACGT", tc.quals(*[40] * 9))
    assert "record 5000 " in both(tc.fastq_bytes(bad), trim_q5=20)
    assert "outside ACGT" in both(tc.fastq_bytes(bad), trim_q5=20, non_acgt="error")        # record 4000 comes first
    bad[4000] = records[4000]
    bad[6000] = (b"ACGTNACGT", tc.quals(*[40] * 9))
    assert "record 5000 " in both(tc.fastq_bytes(bad), trim_q5=20, non_acgt="error")
    assert "odd" in both(tc.fastq_bytes(records[:4001]), min_len=5, pairs=True)
    assert "record 0 " in both(tc.fastq_bytes([(b"ACGT", b"III")], final_newline=False), trim_q3=2)
    assert "record 1 " in both(b"@a\nAC\n+\nII\n@b\nACGT\n+", trim_q3=2)                    # the last record has no quality line at all
    seqio.read_files_device([tc.write(tmp_path, "fine.fastq", tc.fastq_bytes(bad))])          # without quality mode the quality lines are not read


def test_all_zero_options_are_the_plain_device_ingest(tmp_path):
    files = [tc.random_records(400 + i, 1500) for i in range(2)]
    paths = [tc.write(tmp_path, "z0.fastq", tc.fastq_bytes(files[0])), tc.write(tmp_path, "z1.fastq", tc.fastq_bytes(files[1], blank_between=True)),
             tc.write(tmp_path, "z2.fa", tc.fasta_bytes(files[0], width=70))]
    plain = seqio.read_files_device(paths)
    host = seqio.read_files(paths)
    assert len(plain) == 5 and plain[4] == [True, False, True]
    assert all(np.array_equal(a, b) for a, b in zip(plain[:3], host[:3])) and plain[3] == host[3]
    for opts in (dict(trim_q3=0, trim_q5=0, min_len=0, pairs=False, quality_hist=False), dict(phred_offset=64)):
        got = seqio.read_files_device(paths, **opts)
        assert len(got) == 5 and got[3:] == plain[3:] and all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got[:3], plain[:3]))
    b = ga.SegmentBatch.from_fastq(paths)
    try:
        with pytest.raises(ga.GasmError) as ei:
            b.ingest_stats()
        assert ei.value.status == -7
    finally:
        b.close()


def test_what_goes_to_the_host_reader(tmp_path):
    records = tc.random_records(500, 1200, lengths=(0, 1, 31, 64, 150))
    fasta = [(s, None) for s, _ in records]
    paths = [tc.write(tmp_path, "reg.fastq", tc.fastq_bytes(records)), tc.write(tmp_path, "blank.fastq", tc.fastq_bytes(records, blank_between=True)),
             tc.write(tmp_path, "x.fa", tc.fasta_bytes(fasta, width=60)), tc.write(tmp_path, "reg2.fastq", tc.fastq_bytes(records))]
    files = [records, records, fasta, records]
    _same(paths, files, on_device=[True, False, True, True], trim_q3=20, quality_hist=True)          # FASTA: nothing applies, read on the device
    _same(paths, files, on_device=[True, False, False, True], trim_q3=20, min_len=31)
    _same(paths, files, on_device=[True, False, False, True], pairs=True)


def test_batch_from_fastq_trims_and_builds(tmp_path):
    k = 21
    g, clean, reads, q, err = tc.worked_example()
    records = [(r.tobytes(), (row + 33).astype(np.uint8).tobytes()) for r, row in zip(reads, q)]
    path = synth.write_fastq(str(tmp_path / "example.fastq"), reads, q)
    other = tc.random_records(600, 400, lengths=(31, 64, 150))
    path2 = tc.write(tmp_path, "other.fastq", tc.fastq_bytes(other))
    cut = seqio.read_files([path], quality_hist=True)[-1].suggest_trim_q(0)
    report = {}
    for name, opts in (("untrimmed", dict(quality_hist=True)), ("trimmed", dict(trim_q3=cut, min_len=k, quality_hist=True))):
        want, _, _, dropped, st, hist = tc.expected([records, other], **opts)
        b = ga.SegmentBatch.from_fastq([path, path2], **opts)
        try:
            assert b.read_strings() == [r.decode() for r in want] and b.dropped_reads == dropped
            got = b.ingest_stats()
            assert np.array_equal(got.counters, st) and np.array_equal(got.quality_hist, hist)
            assert got == seqio.read_files([path, path2], **opts)[-1]
            n0 = int(st[0][1])
            ref = ga.SegmentBatch.from_strings([[r.decode() for r in want[:n0]], [r.decode() for r in want[n0:]]])
            try:
                for s in (0, 1):
                    assert b.build(k, min_count=2).contigs(s) == ref.build(k, min_count=2).contigs(s)
                report[name] = (len(b.contigs(0)), max(len(c) for c in b.contigs(0)))
            finally:
                ref.close()
        finally:
            b.close()
        contigs, stats = ga.get_contigs_from_fastq([path, path2], k, min_count=2, **opts)
        assert stats == got and len(contigs[0]) == report[name][0]
    print("worked example, min_count = 2 build at k = 21: (contigs, longest) ", report)
    contigs, stats = ga.get_contigs_from_fastq([path], k)
    assert stats is None and contigs[0]
