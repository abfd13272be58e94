// kernels_count.hip — break-k-mer counts of the reads (count_read_kmers, lib/DeNovoAssembler.R:135-168): for every segment,
// how often each ACGT string of length 2, 4, 6 and 8 occurs as a window inside one read, in breakage-table order
// (GASM_TABLE_ROWS rows: 16 / 256 / 4096 / 65536, each lexicographic = the base-4 value of the window).
//
// One LDS counter per position: only the 8-mer bin of a position p with p + 8 <= read end is incremented; the last 7 positions
// of a read, where no 8-mer starts, go to small "tail" tables of the shorter lengths.  count_k[x] = the sum of count_8 over
// the 4^(8-k) extensions of x, plus tail_k[x] — exact, and about one LDS atomic per base instead of four.
// 65 536 u32 bins do not fit in LDS, so the S = 2^LS workgroups of a segment split them by the leading LS bits of the key:
// the bin of x of every length, and the bins of all of x's 8-mer extensions, belong to the same workgroup, which sums its own
// share to final values in LDS and stores them with plain coalesced stores (no global atomics, no memset, deterministic).
// Every workgroup of a segment reads all of the segment's packed reads; the S of them lie on one XCD (seg_chunk) and share
// its L2.
#include <algorithm>

#include "pipeline.h"

#define GASM_RKC_WG 512
#define GASM_RKC_SPLIT_DEFAULT 2      // measured at configs[2]: 1.28 ms (2), 1.71 (4), 2.82 (8); the skewed single segments tie

// the 16 u32 at a (LDS, 16-byte aligned)
__device__ __forceinline__ u32 sum16(const u32* a) {
    u32 t = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint4 v = reinterpret_cast<const uint4*>(a)[j];
        t += v.x + v.y + v.z + v.w;
    }
    return t;
}

template <int LS>
__global__ void __launch_bounds__(GASM_RKC_WG) k_read_kmer_count(const u64* __restrict__ words, const u64* __restrict__ read_off,
                                                                 const u64* __restrict__ seg_read_off, u32 fixed_len, u32 n_segments,
                                                                 u32* __restrict__ out) {
    constexpr u32 N8 = 65536u >> LS, N6 = 4096u >> LS, N4 = 256u >> LS, N2 = 16u >> LS;
    __shared__ __align__(16) u32 s8[N8];
    __shared__ __align__(16) u32 t6[N6];
    __shared__ u32 t4[N4], t2[N2];
    __shared__ __align__(16) u32 a6[N6];
    __shared__ __align__(16) u32 a4[N4];       // sums over the 8-mer extensions (the tails not included)
    u32 seg, part;
    if (!seg_chunk(n_segments, 1u << LS, &seg, &part)) return;
    const u32 tid = threadIdx.x;
    for (u32 i = tid; i < N8 / 4; i += GASM_RKC_WG) reinterpret_cast<uint4*>(s8)[i] = make_uint4(0, 0, 0, 0);
    for (u32 i = tid; i < N6; i += GASM_RKC_WG) t6[i] = 0;
    if (tid < N4) t4[tid] = 0;
    if (tid < N2) t2[tid] = 0;
    __syncthreads();

    const u64 r0 = seg_read_off[seg], r1 = seg_read_off[seg + 1];
    const u64 b0 = fixed_len ? r0 * fixed_len : (r0 < r1 ? read_off[r0] : 0);
    const u64 b1 = fixed_len ? r1 * fixed_len : (r0 < r1 ? read_off[r1] : 0);
    if (b1 > b0) {
        // one thread per packed word: the word's (up to) 32 positions, with the next word for the windows that run past it
        for (u64 i = (b0 >> 5) + tid; i < (b1 + 31) >> 5; i += GASM_RKC_WG) {
            u64 p = i << 5 > b0 ? i << 5 : b0;
            const u64 pe = (i << 5) + 32 < b1 ? (i << 5) + 32 : b1;
            u64 hi = words[i], lo = words[i + 1];
            const u32 s = (u32)(p - (i << 5)) << 1;
            if (s) { hi = (hi << s) | (lo >> (64 - s)); lo <<= s; }
            // the read holding p and its end
            u64 r, e;
            if (fixed_len) { r = p / fixed_len; e = (r + 1) * fixed_len; }
            else { r = r0 + upper_seg(read_off + r0, (u32)(r1 - r0), p); e = read_off[r + 1]; }
            for (; p < pe; ++p) {
                while (p >= e) {                      // (empty reads are skipped here)
                    if (fixed_len) e += fixed_len;
                    else { ++r; e = read_off[r + 1]; }
                }
                const u64 rem = e - p;
                const u32 x8 = (u32)(hi >> 48);      // the 8 bases from p on (past the read end: the next read's or padding)
                if (rem >= 8) {
                    if ((x8 >> (16 - LS)) == part) atomicAdd(&s8[x8 & (N8 - 1)], 1u);
                } else {
                    if (rem >= 6 && (x8 >> (16 - LS)) == part) atomicAdd(&t6[(x8 >> 4) & (N6 - 1)], 1u);
                    if (rem >= 4 && (x8 >> (16 - LS)) == part) atomicAdd(&t4[(x8 >> 8) & (N4 - 1)], 1u);
                    if (rem >= 2 && (x8 >> (16 - LS)) == part) atomicAdd(&t2[(x8 >> 12) & (N2 - 1)], 1u);
                }
                hi = (hi << 2) | (lo >> 62);
                lo <<= 2;
            }
        }
    }
    __syncthreads();

    // the workgroup's share of every length: rows [part * N_k, (part + 1) * N_k) of that length's table
    u32* o = out + (u64)seg * GASM_TABLE_ROWS;
    uint4* o8 = reinterpret_cast<uint4*>(o + 4368 + part * N8);      // (16-byte aligned: 69 904, 4368 and N8 are multiples of 4)
    for (u32 i = tid; i < N8 / 4; i += GASM_RKC_WG) o8[i] = reinterpret_cast<const uint4*>(s8)[i];
    // a shorter k-mer x has 16 extensions by two bases, adjacent in the longer table: rows 16x .. 16x + 15
    for (u32 x = tid; x < N6; x += GASM_RKC_WG) {
        const u32 a = sum16(s8 + 16 * x);
        a6[x] = a;
        o[272 + part * N6 + x] = a + t6[x];
    }
    __syncthreads();
    if (tid < N4) {
        const u32 a = sum16(a6 + 16 * tid);
        a4[tid] = a;
        o[16 + part * N4 + tid] = a + t4[tid];
    }
    __syncthreads();
    if (tid < N2) o[part * N2 + tid] = sum16(a4 + 16 * tid) + t2[tid];
}

template __global__ void k_read_kmer_count<1>(const u64*, const u64*, const u64*, u32, u32, u32*);
template __global__ void k_read_kmer_count<2>(const u64*, const u64*, const u64*, u32, u32, u32*);
template __global__ void k_read_kmer_count<3>(const u64*, const u64*, const u64*, u32, u32, u32*);

// workgroups per segment: GASM_RKC_SPLIT (2, 4 or 8; other values are rounded down to a power of two and clamped)
int read_kmer_split() {
    const int v = std::max(2, std::min(8, env_int("GASM_RKC_SPLIT", GASM_RKC_SPLIT_DEFAULT)));
    return v >= 8 ? 8 : v >= 4 ? 4 : 2;
}

int read_kmer_windows_check(const DevReads& rd) {
    for (u32 s = 0; s < rd.n_segments; ++s) {
        u64 w = 0;
        if (rd.fixed_len) w = (rd.h_seg_read_off[s + 1] - rd.h_seg_read_off[s]) * (u64)(rd.fixed_len - 1);
        else
            for (u64 r = rd.h_seg_read_off[s]; r < rd.h_seg_read_off[s + 1]; ++r) {
                const u64 L = rd.h_read_off[r + 1] - rd.h_read_off[r];
                if (L > 1) w += L - 1;
            }
        if (w > 0xFFFFFFFFull) {
            gasm_set_error("segment %u has %llu windows of length 2: the 32-bit counters hold at most 2^32 - 1", s, (unsigned long long)w);
            return GASM_ERR_CAPACITY;
        }
    }
    return GASM_OK;
}

int launch_read_kmer_count(gasm_ctx* ctx, const DevReads& rd, u32* d_out) {
    if (rd.positioned) { gasm_set_error("read k-mer counts of pooled reads are not supported"); return GASM_ERR_STATE; }
    HIPCHK(hipSetDevice(ctx->device));
    const u32 S = (u32)read_kmer_split();
    const dim3 grid(8u * S * ((rd.n_segments + 7u) / 8u)), block(GASM_RKC_WG);
    const u64* ro = rd.fixed_len ? nullptr : rd.d_read_off.as<u64>();
    const u64* so = rd.d_seg_read_off.as<u64>();
    const u64* w = rd.d_words.as<u64>();
    if (S == 2) GLAUNCH(ctx, "k_read_kmer_count", k_read_kmer_count<1>, grid, block, 0, w, ro, so, rd.fixed_len, rd.n_segments, d_out);
    else if (S == 4) GLAUNCH(ctx, "k_read_kmer_count", k_read_kmer_count<2>, grid, block, 0, w, ro, so, rd.fixed_len, rd.n_segments, d_out);
    else GLAUNCH(ctx, "k_read_kmer_count", k_read_kmer_count<3>, grid, block, 0, w, ro, so, rd.fixed_len, rd.n_segments, d_out);
    return GASM_OK;
}
