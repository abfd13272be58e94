// seqio.cpp — FASTQ / FASTA in (the north star's "FASTQ-in" surface).  The reference has no file
// reader on this path — it simulates reads in R and writes FASTA (lib/GenerateReads.R:405-433: one record per read,
// header "<chr>_<start>_<end>:0_<i>/1", sequence on one line); README.md:29-31 names kseq.h but nothing includes it.
// Accepted here: FASTQ with four-line records (what sequencers and the usual simulators write), FASTA with sequences on
// one or several lines, plain or gzip (zlib's gzread reads both), lower case folded to upper case.  A read holding a
// byte outside ACGT (N, IUPAC codes) cannot be packed in 2 bits: it is dropped and counted, or refused.
// The sequences are packed 2-bit on the fly (first base most significant, 32 bases per word, reads back to back): what
// goes over PCIe is a quarter of the text.
#include <zlib.h>

#include <algorithm>

#include "gasm_internal.h"

namespace gasm_host {

struct LineReader {
    gzFile f = nullptr;
    std::vector<char> buf;
    size_t pos = 0, end = 0;
    bool failed = false;          // a read error or a truncated / corrupt gzip stream: the reads so far are NOT the file's reads
    std::string fail_text;
    bool open(const char* path) {
        f = gzopen(path, "rb");
        if (!f) return false;
        gzbuffer(f, 1 << 20);
        buf.resize(1 << 20);
        return true;
    }
    ~LineReader() { if (f) gzclose(f); }
    // next line without its terminator ("\n" or "\r\n"); false at the end of the file
    bool line(std::string& out) {
        out.clear();
        bool any = false;
        for (;;) {
            if (pos == end) {
                const int n = gzread(f, buf.data(), (unsigned)buf.size());
                if (n < 0 || (n == 0 && !gzeof(f))) {       // (n == 0 at a clean end of file; anything else is an error)
                    int code = 0;
                    const char* msg = gzerror(f, &code);
                    failed = true;
                    fail_text = msg && *msg ? msg : "read error";
                    break;
                }
                if (n == 0) {
                    // zlib reports a gzip stream that stops short of its trailer through gzerror (Z_BUF_ERROR), not through gzread
                    int code = 0;
                    const char* msg = gzerror(f, &code);
                    if (code != Z_OK && code != Z_STREAM_END) { failed = true; fail_text = msg && *msg ? msg : "truncated stream"; }
                    break;
                }
                pos = 0; end = (size_t)n;
            }
            any = true;
            const char* b = buf.data() + pos;
            const char* nl = static_cast<const char*>(memchr(b, '\n', end - pos));
            if (nl) {
                out.append(b, (size_t)(nl - b));
                pos = (size_t)(nl - buf.data()) + 1;
                if (!out.empty() && out.back() == '\r') out.pop_back();
                return true;
            }
            out.append(b, end - pos);
            pos = end;
        }
        if (any && !out.empty() && out.back() == '\r') out.pop_back();
        return any;
    }
};

static inline int base_code_host(unsigned char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return -1;
    }
}

void PackedReads::append_span(const char* seq, size_t n) {
    for (size_t q = 0; q < n; ++q) {
        const u64 p = total_bases++;
        if ((p & 31) == 0) words.push_back(0);
        words.back() |= (u64)base_code_host((unsigned char)seq[q]) << (62 - 2 * (p & 31));
    }
    read_off.push_back(total_bases);
}

// The rule of include/gasm.h ("Quality trimming at ingest"), stated once: everything else on the host calls this, the device kernel
// (k_ing_qual_trim) and tests/trim_ref.py restate it.
void trim_span(const char* seq, const char* qual, u32 L, const IngestOpts& o, u32* a_out, u32* e_out) {
    auto q_of = [&](u32 i) -> long long { return base_code_host((unsigned char)seq[i]) < 0 ? 0 : (long long)(unsigned char)qual[i] - (long long)o.phred_offset; };
    u32 a = 0, e = L;
    if (o.trim_q3 > 0) {
        long long s = 0, best = 0;
        for (u32 i = L; i-- > 0;) {
            s += (long long)o.trim_q3 - q_of(i);
            if (s < 0) break;
            if (s > best) { best = s; e = i; }
        }
    }
    if (o.trim_q5 > 0) {
        long long s = 0, best = 0;
        for (u32 i = 0; i < L; ++i) {
            s += (long long)o.trim_q5 - q_of(i);
            if (s < 0) break;
            if (s > best) { best = s; a = i + 1; }
        }
    }
    *a_out = a;
    *e_out = e;
}

// one file -> its reads appended to `out`.  Returns GASM_OK / GASM_ERR_INVALID (unreadable, malformed) / GASM_ERR_NON_ACGT.
// With every option of `o` zero this is the reader as it always was: quality lines are skipped, every record is whole.
int read_sequence_file(const char* path, const IngestOpts& o, PackedReads& out, u64* n_kept, u64* n_dropped, u64* stats, u64* hist) {
    LineReader lr;
    if (!lr.open(path)) { gasm_set_error("cannot open %s", path); return GASM_ERR_INVALID; }
    *n_kept = 0;
    if (out.read_off.empty()) out.read_off.push_back(0);
    std::string ln, seq;
    u64 st[GASM_INGEST_STATS] = {0};
    // a record whose class (before the mate rule) is known: its span [t5, t5 + len) of `text`, L bases in all
    struct Rec { std::string text; u32 L = 0, t5 = 0, len = 0; u8 cls = ING_KEPT; };
    Rec held;                     // pairs: the first mate waits for the second
    bool holding = false;
    auto settle = [&](const Rec& r, const std::string& text, u8 cls) {
        ++st[0];
        st[1 + cls] += 1;
        st[5] += r.L;
        st[cls == ING_KEPT ? 6 : 7] += r.len;
        st[8] += r.t5;
        st[9] += r.L - r.t5 - r.len;
        if (cls == ING_KEPT) {
            if (r.len < r.L) ++st[10];
            out.append_span(text.data() + r.t5, r.len);
            ++*n_kept;
        } else {
            ++*n_dropped;
        }
    };
    // seq (and qual in quality mode, null for FASTA) of record `rec` -> classified, settled at once or with its mate
    auto take = [&](const std::string& s, const std::string* qual, u64 rec) -> int {
        Rec r;
        r.L = (u32)s.size();
        u32 a = 0, e = r.L;
        if (qual) {
            bool ok = qual->size() == s.size();
            for (size_t i = 0; ok && i < qual->size(); ++i) {
                const u32 b = (unsigned char)(*qual)[i];
                ok = b >= o.phred_offset && b <= o.phred_offset + 93;
            }
            if (!ok) {
                gasm_set_error("%s: record %llu has a malformed quality line (not as long as its sequence, or a byte outside [%u, %u])", path,
                               (unsigned long long)rec, o.phred_offset, o.phred_offset + 93);
                return GASM_ERR_INVALID;
            }
            if (hist && o.quality_hist) for (unsigned char c : *qual) ++hist[c - o.phred_offset];
            trim_span(s.data(), qual->data(), r.L, o, &a, &e);
        }
        r.t5 = std::min(a, e);
        r.len = e - r.t5;
        bool bad = false;
        for (u32 i = r.t5; i < e && !bad; ++i) bad = base_code_host((unsigned char)s[i]) < 0;
        if (bad) {
            if (o.error_on_non_acgt) { gasm_set_error("%s: a read holds a base outside ACGT", path); return GASM_ERR_NON_ACGT; }
            r.cls = ING_NON_ACGT;
        } else if (r.len < o.min_len) {
            r.cls = ING_SHORT;
        }
        if (!o.pairs) { settle(r, s, r.cls); return GASM_OK; }
        if (!holding) { held = std::move(r); held.text = s; holding = true; return GASM_OK; }
        holding = false;
        const bool drop = held.cls != ING_KEPT || r.cls != ING_KEPT;
        settle(held, held.text, held.cls == ING_KEPT && drop ? (u8)ING_MATE : held.cls);
        settle(r, s, r.cls == ING_KEPT && drop ? (u8)ING_MATE : r.cls);
        return GASM_OK;
    };
    auto finish = [&]() -> int {
        if (lr.failed) { gasm_set_error("%s: %s (truncated or corrupt file: its reads are not used)", path, lr.fail_text.c_str()); return GASM_ERR_INVALID; }
        if (holding) { gasm_set_error("%s: an odd number of records (%llu) with pairs = 1", path, (unsigned long long)(st[0] + 1)); return GASM_ERR_INVALID; }
        if (stats) for (u32 q = 0; q < GASM_INGEST_STATS; ++q) stats[q] += st[q];
        return GASM_OK;
    };
    auto eof_status = [&]() -> int {
        if (lr.failed) { gasm_set_error("%s: %s (truncated or corrupt file)", path, lr.fail_text.c_str()); return GASM_ERR_INVALID; }
        return GASM_OK;
    };
    if (!lr.line(ln)) return eof_status();                  // empty file: no reads
    while (ln.empty()) if (!lr.line(ln)) return eof_status();
    if (ln[0] == '@') {
        u64 rec = 0;
        for (;;) {
            if (ln.empty()) { if (!lr.line(ln)) break; continue; }           // blank lines between records
            if (ln[0] != '@') { gasm_set_error("%s: record %llu does not start with '@'", path, (unsigned long long)rec); return GASM_ERR_INVALID; }
            std::string plus, qual;
            if (!lr.line(seq) || !lr.line(plus) || plus.empty() || plus[0] != '+') {
                gasm_set_error("%s: record %llu has no '+' line (multi-line FASTQ is not supported)", path, (unsigned long long)rec);
                return GASM_ERR_INVALID;
            }
            lr.line(qual);
            while (!seq.empty() && (seq.back() == ' ' || seq.back() == '\t')) seq.pop_back();
            if (o.quality()) while (!qual.empty() && (qual.back() == ' ' || qual.back() == '\t')) qual.pop_back();
            GCHK(take(seq, o.quality() ? &qual : nullptr, rec));
            ++rec;
            if (!lr.line(ln)) break;
        }
    } else if (ln[0] == '>') {
        bool have = false;
        u64 rec = 0;
        seq.clear();
        for (;;) {
            if (!ln.empty() && ln[0] == '>') {
                if (have) GCHK(take(seq, nullptr, rec++));
                have = true;
                seq.clear();
            } else if (have) {
                size_t a = 0, b = ln.size();
                while (a < b && (ln[a] == ' ' || ln[a] == '\t')) ++a;
                while (b > a && (ln[b - 1] == ' ' || ln[b - 1] == '\t')) --b;
                seq.append(ln, a, b - a);
            }
            if (!lr.line(ln)) break;
        }
        if (have) GCHK(take(seq, nullptr, rec++));
    } else {
        gasm_set_error("%s: neither FASTQ ('@') nor FASTA ('>')", path);
        return GASM_ERR_INVALID;
    }
    return finish();
}

int read_sequence_file(const char* path, bool error_on_non_acgt, PackedReads& out, u64* n_kept, u64* n_dropped) {
    IngestOpts o;
    o.error_on_non_acgt = error_on_non_acgt;
    return read_sequence_file(path, o, out, n_kept, n_dropped, nullptr, nullptr);
}

}  // namespace gasm_host
