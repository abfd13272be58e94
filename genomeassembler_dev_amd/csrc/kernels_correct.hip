// kernels_correct.hip — spectral read correction (include/gasm.h, "Read correction"): substitutions in the reads are repaired
// against the distinct k-mers of a finished build.
//   k_read_correct    one wave per read: membership of every k-mer, the weak runs, the candidates of every run, the fix
// The pass's frame (segment, wave, the loop over a wave's reads, the counter flush): contig_index.h; of a finished build it needs the
// k-mer set only.
#include "contig_index.h"

// is `key` one of the distinct k-mers of segment `seg`?  (bucket, bin, a one-or-two-key search, one key load)
template <class K>
__device__ __forceinline__ bool kmer_trusted(const GraphView& gv, u32 seg, const K& key) {
    u32 hi;
    const u32 e = graph_lower_bound<K>(gv, seg, key, &hi);
    return e < hi && keq(reinterpret_cast<const K*>(gv.dk_key)[e], key);
}

// the key with the 2-bit code x XOR-ed onto the base whose pair of bits starts at bit s (0 <= s <= 2k - 2)
__device__ __forceinline__ u64 kflip(u64 a, u32 x, int s) { return a ^ ((u64)x << s); }
__device__ __forceinline__ K128 kflip(const K128& a, u32 x, int s) {
    const K128 m = kshl(K128{0, (u64)x}, s);
    return K128{a.hi ^ m.hi, a.lo ^ m.lo};
}

// One wave per read, GASM_READ_WAVES reads of one segment per workgroup and round (ReadPass).  The kernel is a gather: every k-mer
// costs the three dependent requests of graph_lower_bound + the key (bucket pair, bin pair, key), and 64 lanes of a wave have 64 such chains in flight — there is nothing to stage in LDS and the
// registers are few, so the occupancy is the launch bound's.
//   pass 1   lane j takes k-mer starts j, j + 64, ...; the weak bits of 64 starts are one __ballot, kept by lane w for word w (a read of
//            GASM_CORRECT_KMER_CAP = 64 x 64 k-mers fills the wave's 64 lanes; no LDS).  No weak bit: the read is clean and the wave
//            goes on to its next read without having touched the output.
//   runs     the maximal runs of weak starts, word by word with count-trailing-zero steps, in wave-uniform code (the words come back
//            through v_readlane, so the branches are scalar).
//   a run    the rule of include/gasm.h picks the one position p a single substitution could sit at.  The three other bases are the
//            codes old ^ 1, old ^ 2, old ^ 3: candidate x replaces the base by XOR-ing x onto its two bits, in the k-mer's key for the
//            test and in the output word for the fix, so the base itself is never read.  The 3 x (run length) <= 3k look-ups are spread
//            over the lanes (candidate-major), each round joined by one ballot per candidate; a round after which no candidate is left
//            ends the run.  Exactly one fitting candidate: lane 0 XORs it onto the output word, atomically — reads of different waves
//            share words.
// Every test reads the INPUT stream, every fix goes to the OUTPUT stream (a copy of the input made by the caller): runs are judged on
// the read as given.
// have_graph = 0: the build holds no k-mer at all (its arrays may not exist): every k-mer is weak.
// stats: GASM_CORRECT_STATS counters per segment (in the order of include/gasm.h: no k-mer, clean, corrected, partial, left, bases),
// zeroed by the caller (flush_wave_counters).
template <class K>
__global__ void __launch_bounds__(GASM_WG) k_read_correct(ReadSet rs, GraphView gv, int have_graph, u32 reads_per_wg, u32 chunks,
                                                          unsigned long long* __restrict__ out_words, u32* __restrict__ stats) {
    __shared__ u32 s_cnt[GASM_CORRECT_STATS];
    ReadPass rp;
    if (!read_pass_begin(rp, rs, gv, nullptr, chunks, s_cnt)) return;
    const u32 seg = rp.seg, lane = rp.lane;
    const int k = rp.k;
    enum { NOKMER, CLEAN, CORRECTED, PARTIAL, LEFT, BASES };
    u32 c_cnt[GASM_CORRECT_STATS] = {0, 0, 0, 0, 0, 0};                           // of this wave's reads (wave-uniform)
    for_wave_reads(rp, reads_per_wg, chunks, [&](u64 r) {
        u64 p0;
        u32 len;
        read_span(rs, r, &p0, &len);
        if (len < (u32)k) { ++c_cnt[NOKMER]; return; }
        const u32 n = len - (u32)k + 1;
        if (n > GASM_CORRECT_KMER_CAP || !have_graph) { ++c_cnt[LEFT]; return; }
        // ---- pass 1: the weak bits
        const u32 nw = (n + 63u) >> 6;
        u64 mymask = 0, any = 0;
        for (u32 w = 0; w < nw; ++w) {
            const u32 j = (w << 6) + lane;
            bool weak = false;
            if (j < n) weak = !kmer_trusted<K>(gv, seg, kmer_key_at<K>(rs.words, p0 + j, k));
            const u64 m = __ballot(weak);
            if (lane == w) mymask = m;
            any |= m;
        }
        if (!any) { ++c_cnt[CLEAN]; return; }
        // ---- the runs (one more, empty, word closes a run that fills the last word to its end)
        u32 n_runs = 0, n_fixed = 0, a = 0;
        bool in_run = false;
        for (u32 w = 0; w <= nw; ++w) {
            const u64 m = w < nw ? lane_word(mymask, w) : 0ull;
            u32 pos = 0;
            while (pos < 64) {
                if (!in_run) {
                    const u64 mm = m >> pos;
                    if (!mm) break;
                    pos += (u32)__builtin_ctzll(mm);
                    a = (w << 6) + pos;
                    in_run = true;
                    continue;
                }
                const u64 z = ~m >> pos;                 // the zero bits of m from pos on
                if (!z) break;                           // the run goes on in the next word
                pos += (u32)__builtin_ctzll(z);
                const u32 b = (w << 6) + pos - 1;
                in_run = false;
                ++n_runs;
                // ---- run [a, b]: where a single substitution would sit, if the rule tries this run at all
                const u32 L = b - a + 1;
                u32 p;
                bool tried;
                if (a == 0 && b == n - 1) { tried = false; p = 0; }                      // the whole read is weak
                else if (a > 0 && b < n - 1) { tried = L == (u32)k; p = b; }             // interior: exactly k k-mers
                else if (a == 0) { tried = L <= (u32)k; p = b; }                         // (a longer one holds k-mers without position b:
                                                                                         // weak whatever stands there, no candidate fits)
                else { tried = L <= (u32)k; p = a + (u32)k - 1; }                        // touches the end
                if (!tried) continue;
                const u32 total = 3 * L;
                u32 fail = 0;                                                            // bit x - 1: candidate x does not fit
                for (u32 it = 0; it < total && fail != 7u; it += 64) {
                    const u32 idx = it + lane;
                    const u32 c = (idx >= L ? 1u : 0u) + (idx >= 2 * L ? 1u : 0u);
                    bool bad = false;
                    if (idx < total) {
                        const u32 j = a + idx - c * L;                                   // j <= p <= j + k - 1 for every j of the run
                        const K key = kflip(kmer_key_at<K>(rs.words, p0 + j, k), c + 1, 2 * (k - 1 - (int)(p - j)));
                        bad = !kmer_trusted<K>(gv, seg, key);
                    }
                    if (__ballot(bad && c == 0)) fail |= 1u;
                    if (__ballot(bad && c == 1)) fail |= 2u;
                    if (__ballot(bad && c == 2)) fail |= 4u;
                }
                if (fail == 6u || fail == 5u || fail == 3u) {                            // exactly one candidate fits
                    const u32 x = fail == 6u ? 1u : fail == 5u ? 2u : 3u;
                    const u64 P = p0 + p;
                    if (lane == 0) atomicXor(&out_words[P >> 5], (unsigned long long)x << (62 - 2 * (u32)(P & 31)));
                    ++n_fixed;
                    ++c_cnt[BASES];
                }
            }
        }
        if (n_fixed == n_runs) ++c_cnt[CORRECTED];
        else if (n_fixed) ++c_cnt[PARTIAL];
        else ++c_cnt[LEFT];
    });
    flush_wave_counters(c_cnt, s_cnt, stats + (size_t)seg * GASM_CORRECT_STATS);
}

template __global__ void k_read_correct<u64>(ReadSet, GraphView, int, u32, u32, unsigned long long*, u32*);
template __global__ void k_read_correct<K128>(ReadSet, GraphView, int, u32, u32, unsigned long long*, u32*);
