// Host check of the numbers that the tile kernels and their launches share (csrc/kernels.h: TileStage, ScatterLds, PartitionLds,
// the flush's scratch slots, the fine directory's bits) against the figures the launches used to write out by hand, for every
// bucket count nb = 1 .. 1024.  Built for the host only and run by tests/test_cabi_and_host.py; needs no GPU.
#include <cstdio>

#include "kernels.h"

template <class K>
static int check(const char* name) {
    const size_t KB = sizeof(K), W = KB / 8;
    const size_t stage = (W == 1 ? 18 : 9) * (size_t)GASM_TILE_WG * KB + (GASM_TILE_WG / 8) * KB;      // NFL passes of 16 bytes per thread + trash slots
    int bad = 0;
    if (TileStage<K>::BYTES != stage) { printf("%s: staging area %u bytes, expected %zu\n", name, TileStage<K>::BYTES, stage); ++bad; }
    if (TileStage<K>::PAD_ROOM != (W == 1 ? 2u * GASM_TILE_WG : (unsigned)GASM_TILE_WG)) { printf("%s: pad room %u\n", name, TileStage<K>::PAD_ROOM); ++bad; }
    for (u32 nb = 1; nb <= 1024; ++nb) {
        const PartitionLds<K> p{nb};
        if (p.total() != stage + (size_t)nb * 52 + 80) { printf("%s: partition, nb = %u: %zu bytes\n", name, nb, p.total()); ++bad; }
        const ScatterLds<K> s{nb};
        if (s.total() != stage + (size_t)nb * 24 + 96) { printf("%s: scatter, nb = %u: %zu bytes\n", name, nb, s.total()); ++bad; }
        // what the scatter's carve-up really covers (its u64 array is rounded up to 16 bytes) lies inside the total
        const size_t end = stage + (size_t)s.n_comb() * 8 + ((size_t)s.n_sub() + s.n_dummy + s.n_tmp) * 4;
        if (end > s.total()) { printf("%s: scatter, nb = %u: arrays end at %zu of %zu bytes\n", name, nb, end, s.total()); ++bad; }
    }
    return bad;
}

int main() {
    static_assert(KeyTraits<u64>::KT == 16 && KeyTraits<K128>::KT == 8, "k-mers per thread and round");
    static_assert(GASM_FLUSH_SLOTS == 1024 * (GASM_TILE_WG / 64), "1024 workgroup slots x waves per workgroup");
    static_assert(dedup_fbits(2048) == 9 && dedup_fbits(4096) == 10, "bits of the fine directory");
    const int bad = check<u64>("u64") + check<K128>("K128");
    printf("lds layout check: %d mismatches over nb = 1 .. 1024, two key widths\n", bad);
    return bad ? 1 : 0;
}
