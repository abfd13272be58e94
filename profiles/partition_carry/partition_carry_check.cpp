// partition_carry_check.cpp — host restatement of k_bucket_partition's per-tile bookkeeping with the carry
// (csrc/kernels_build.hip): counts, carried keys, staging ranges, reservation, flush by staging index, the remainder's
// units and the last tile's filler line, as plain arrays.  Workgroups are sequential actors that take turns tile by tile
// over one shared cursor array.  Not part of the library; not loaded into Python.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined partition_carry_check.cpp -o partition_carry_check && ./partition_carry_check
//
// Checked for every case: every key lands in its (segment, bucket) region exactly once; cursors are whole lines; a region
// holds at most padm fillers per (workgroup, segment) visit; nothing is written outside a region except to the scratch
// line; a region that overflowed raised the flag (the build is then repeated by the two-pass kernels).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

typedef uint32_t u32;
typedef uint64_t u64;

static const u32 WG = 512, NFL = 9;
static const int BSHIFT = 40;                       // key = bucket << 40 | serial; filler: top bit set
static const u64 FILLER = 1ull << 63;

struct Tile { u32 seg; std::vector<u64> keys; };     // at most WG * KT keys

struct Case {
    const char* name;
    u32 kpu;                                         // keys per 16-byte unit: 2 (64-bit keys) or 1 (128-bit keys)
    u32 nb, n_seg, grid;
    u64 cap;                                         // capacity of every region (keys, whole lines); 0 = roomy
    std::vector<Tile> tiles;
};

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { printf("  FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Comb { u64 cb; u32 fend; u32 w; };
struct Unit { u64 x, y; };

static void run_case(const Case& c, std::mt19937_64& rng) {
    const u32 kpu = c.kpu, nb = c.nb, kt = kpu == 2 ? 16 : 8, line = kpu == 2 ? 16 : 8;
    const u32 CAP = NFL * WG * kpu, pad_room = kpu == 2 ? 2 * WG : WG;
    u32 padm = line - 1;
    while (padm && (u64)nb * (padm + (kpu == 1 ? 1u : 0u)) > pad_room) padm >>= 1;      // the host's rule (launch_distinct)
    const bool carry = padm != 0;
    const u32 ush = carry ? (u32)__builtin_ctz(padm + 1) - (kpu == 2 ? 1u : 0u) : 0u;
    const u32 n_carry = carry ? nb << ush : 0u, unit_m = carry ? kpu - 1 : 0u;
    CHECK(n_carry <= WG, "%s: %u carrying threads", c.name, n_carry);

    const u32 n_tiles = (u32)c.tiles.size(), nbt = c.n_seg * nb;
    // regions as the host lays them out: roomy = all keys of the bucket + padm per tile, in whole lines
    std::vector<u64> bstart(nbt + 1), expect_n(nbt, 0);
    std::vector<std::vector<u64>> expect(nbt);
    for (const Tile& t : c.tiles) {
        CHECK(t.keys.size() <= WG * kt, "%s: tile of %zu keys", c.name, t.keys.size());
        for (u64 key : t.keys) expect[t.seg * nb + (u32)(key >> BSHIFT)].push_back(key);
    }
    u64 at = 0;
    for (u32 gb = 0; gb < nbt; ++gb) {
        u64 cap = c.cap ? c.cap : expect[gb].size() + (u64)n_tiles * padm + line;
        cap = (cap + line - 1) / line * line;
        bstart[gb] = at; at += cap;
    }
    bstart[nbt] = at;
    const u64 scratch = at;                          // one unit: the scratch line
    std::vector<u64> keys(at + 2, 0);
    std::vector<unsigned char> written(at + 2, 0);
    std::vector<u32> cursor(nbt, 0), visits(nbt, 0);
    bool flag_overflow = false;
    u32 n_unaligned = 0;

    const u32 grid = std::min(c.grid, n_tiles), per_wg = (n_tiles + grid - 1) / grid;
    struct Wg {
        u32 tile, tile_end;
        bool fresh = true;
        std::vector<u64> s_key;
        std::vector<Comb> s_comb;
        std::vector<Unit> cu;
    };
    std::vector<Wg> wgs(grid);
    for (u32 b = 0; b < grid; ++b) {
        Wg& w = wgs[b];
        w.tile = b * per_wg; w.tile_end = std::min(n_tiles, (b + 1) * per_wg);
        w.s_key.resize(CAP + WG / 8);
        for (u64& k : w.s_key) k = rng();      // uninitialised LDS: any bucket, fillers too
        w.s_comb.assign(nb, Comb{0, 0, 0});
        w.cu.assign(WG, Unit{0, 0});
    }
    auto store_unit = [&](u64 dst, const u64* v, u64 beg, u64 end, bool to_scratch) {
        if (to_scratch) return;
        for (u32 j = 0; j < kpu; ++j) {
            CHECK(dst + j >= beg && dst + j < end, "%s: store at %llu outside [%llu, %llu)", c.name, (unsigned long long)(dst + j), (unsigned long long)beg, (unsigned long long)end);
            if (dst + j >= scratch) continue;
            CHECK(!written[dst + j], "%s: key slot %llu written twice", c.name, (unsigned long long)(dst + j));
            written[dst + j] = 1; keys[dst + j] = v[j];
        }
    };
    auto one_tile = [&](Wg& w) {
        const Tile& tl = c.tiles[w.tile];
        const u32 seg = tl.seg;
        const bool last = !carry || w.tile + 1 >= w.tile_end || c.tiles[w.tile + 1].seg != seg;
        // count = rank (the order of the ranks within a bucket is arbitrary: shuffle)
        std::vector<std::vector<u64>> by(nb);
        for (u64 key : tl.keys) by[(u32)(key >> BSHIFT)].push_back(key);
        std::vector<u32> cin(nb), cnt(nb), flush(nb), res(nb), soff(nb), run(nb, 0);
        u32 total = 0, total_lines = 0;
        for (u32 b = 0; b < nb; ++b) total_lines += (((w.fresh ? 0u : (w.s_comb[b].w & 31u)) + (u32)by[b].size()) + padm) & ~padm;
        const bool lines = total_lines <= CAP;           // staging ranges on whole lines where they fit, else on 16-byte units
        CHECK(total_lines < 65536, "%s: the packed scan overflows", c.name);
        n_unaligned += !lines;
        for (u32 b = 0; b < nb; ++b) {
            std::shuffle(by[b].begin(), by[b].end(), rng);
            cin[b] = w.fresh ? 0u : (w.s_comb[b].w & 31u);
            cnt[b] = cin[b] + (u32)by[b].size();
            flush[b] = cnt[b] & ~padm;
            res[b] = last ? (cnt[b] + padm) & ~padm : flush[b];
            soff[b] = total;
            total += lines ? (cnt[b] + padm) & ~padm : (cnt[b] + unit_m) & ~unit_m;
        }
        CHECK(total <= CAP, "%s: %u keys staged, capacity %u", c.name, total, CAP);
        for (u32 b = 0; b < nb; ++b) {
            const u32 gb = seg * nb + b;
            if (w.fresh) ++visits[gb];
            if (res[b]) { run[b] = cursor[gb]; cursor[gb] += res[b]; }
        }
        // carried keys at the head of the range
        if (!w.fresh)
            for (u32 t = 0; t < n_carry; ++t) {
                const u32 b = t >> ush, f = (t & ((1u << ush) - 1u)) * kpu, n = cin[b];
                if (f < n) w.s_key[soff[b] + f] = w.cu[t].x;
                if (kpu == 2 && f + 1 < n) w.s_key[soff[b] + f + 1] = w.cu[t].y;
            }
        // the rest of an unfinished line (staged on whole lines only): of this bucket, so that the flush does not take it for another's
        for (u32 t = 0; t < n_carry; ++t) {
            const u32 b = t >> ush, f = (t & ((1u << ush) - 1u)) * kpu, n = lines && cnt[b] != flush[b] ? cnt[b] - flush[b] : 31u;
            for (u32 j = 0; j < kpu; ++j)
                if (f + j >= n) w.s_key[soff[b] + flush[b] + f + j] = FILLER | ((u64)b << BSHIFT);
        }
        for (u32 b = 0; b < nb; ++b)
            for (u32 r = 0; r < by[b].size(); ++r) w.s_key[soff[b] + cin[b] + r] = by[b][r];
        for (u32 b = 0; b < nb; ++b) {
            const u32 gb = seg * nb + b;
            const bool fits = (u64)run[b] + res[b] <= bstart[gb + 1] - bstart[gb];
            w.s_comb[b] = Comb{bstart[gb] + run[b] - soff[b], fits ? soff[b] + flush[b] : 1u << 31, (lines ? 1u << 31 : 0u) | ((soff[b] + flush[b]) << 5) | (cnt[b] - flush[b])};
            if (!fits) flag_overflow = true;
        }
        // what stays behind
        for (u32 t = 0; t < n_carry; ++t) {
            const u32 b = t >> ush, f = (t & ((1u << ush) - 1u)) * kpu;
            const Comb cm = w.s_comb[b];
            const u32 rbeg = (cm.w << 1) >> 6, n = cm.w & 31u;
            CHECK(rbeg + f + kpu <= w.s_key.size(), "%s: remainder read at %u past the staging area", c.name, rbeg + f);
            w.cu[t].x = w.s_key[rbeg + f];
            w.cu[t].y = kpu == 2 ? w.s_key[rbeg + f + 1] : 0;
            if (last && n && !(cm.fend >> 31)) {
                u64 o[2] = {w.cu[t].x, w.cu[t].y};
                const u64 fl = FILLER | ((u64)b << BSHIFT);
                if (f >= n) o[0] = fl;
                if (kpu == 2 && f + 1 >= n) o[1] = fl;
                const u32 gb = seg * nb + b;
                store_unit(cm.cb + rbeg + f, o, bstart[gb], bstart[gb + 1], false);
            }
        }
        // flush: NFL passes of one unit per thread; the bucket comes from the unit's first key
        for (u32 i = 0; i < NFL * WG * kpu; i += kpu) {
            const u32 bkt = (u32)(w.s_key[i] >> BSHIFT) & (nb - 1);
            const Comb cm = w.s_comb[bkt];
            const u32 gb = seg * nb + bkt;
            store_unit(cm.cb + i, &w.s_key[i], bstart[gb], bstart[gb + 1], !((int)i < (int)cm.fend));
        }
        w.fresh = last;
        ++w.tile;
    };
    for (bool any = true; any;) {                      // the workgroups take turns, one tile each, in a random order per round
        any = false;
        std::vector<u32> order(grid);
        for (u32 b = 0; b < grid; ++b) order[b] = b;
        std::shuffle(order.begin(), order.end(), rng);
        for (u32 b : order)
            if (wgs[b].tile < wgs[b].tile_end) { one_tile(wgs[b]); any = true; }
    }
    // ---- the four properties
    u64 n_fill = 0, n_over = 0;
    for (u32 gb = 0; gb < nbt; ++gb) {
        const u64 beg = bstart[gb], cap = bstart[gb + 1] - beg;
        CHECK(cursor[gb] % (padm + 1) == 0, "%s: cursor %u of bucket %u is no whole line", c.name, cursor[gb], gb);
        if (cursor[gb] > cap) { ++n_over; continue; }
        std::vector<u64> got;
        u32 fill = 0;
        for (u64 i = 0; i < cursor[gb]; ++i) {
            CHECK(written[beg + i], "%s: slot %llu of bucket %u below its cursor was never written", c.name, (unsigned long long)i, gb);
            if (keys[beg + i] >> 63) { ++fill; CHECK(keys[beg + i] == (FILLER | ((u64)(gb % nb) << BSHIFT)), "%s: foreign filler in bucket %u", c.name, gb); }
            else got.push_back(keys[beg + i]);
        }
        for (u64 i = cursor[gb]; i < cap; ++i) CHECK(!written[beg + i], "%s: bucket %u written past its cursor", c.name, gb);
        CHECK(fill <= visits[gb] * padm, "%s: bucket %u holds %u fillers after %u visits", c.name, gb, fill, visits[gb]);
        n_fill += fill;
        std::vector<u64> want = expect[gb];
        std::sort(got.begin(), got.end()); std::sort(want.begin(), want.end());
        CHECK(got == want, "%s: bucket %u holds %zu keys, %zu expected (or other keys)", c.name, gb, got.size(), want.size());
    }
    CHECK((n_over != 0) == flag_overflow, "%s: %llu regions overflowed, flag %d", c.name, (unsigned long long)n_over, (int)flag_overflow);
    u64 n_keys = 0;
    for (const Tile& t : c.tiles) n_keys += t.keys.size();
    printf("%-44s kpu %u nb %3u padm %2u grid %3u tiles %4u: %9llu keys, %7llu fillers (per-tile padding: <= %llu), %llu regions overflowed, %u tiles staged on units\n", c.name, kpu, nb, padm,
           grid, n_tiles, (unsigned long long)n_keys, (unsigned long long)n_fill, (unsigned long long)n_tiles * nb * padm, (unsigned long long)n_over, n_unaligned);
}

static u64 serial = 0;
static Tile make_tile(u32 seg, u32 nb, u32 n, std::mt19937_64& rng, u32 hot = 0) {
    Tile t; t.seg = seg;
    for (u32 i = 0; i < n; ++i) {
        const u32 b = hot ? (u32)(rng() % hot) : (u32)(rng() % nb);     // hot: only the first `hot` buckets are hit
        t.keys.push_back(((u64)b << BSHIFT) | (serial++ & ((1ull << BSHIFT) - 1)));
    }
    return t;
}

int main() {
    std::mt19937_64 rng(20240611);
    std::vector<Case> cases;
    for (u32 kpu : {2u, 1u}) {
        const u32 full = 512 * (kpu == 2 ? 16 : 8);
        for (u32 nb : {1u, 2u, 64u, 128u, 512u}) {
            {   // random tiles, segments of random length, several grids
                for (u32 grid : {1u, 3u, 16u}) {
                    Case c{"random tiles", kpu, nb, 5, grid, 0, {}};
                    for (u32 s = 0; s < 5; ++s) for (u32 i = 0, n = 1 + (u32)(rng() % 12); i < n; ++i) c.tiles.push_back(make_tile(s, nb, (u32)(rng() % (full + 1)), rng));
                    cases.push_back(c);
                }
            }
            {   // full tiles: the staging area's worst case
                Case c{"full tiles", kpu, nb, 2, 2, 0, {}};
                for (u32 i = 0; i < 40; ++i) c.tiles.push_back(make_tile(i / 23, nb, full - (u32)(rng() % 3), rng));
                cases.push_back(c);
            }
            {   // fewer than a line per bucket, many tiles in a row: the carry persists over several tiles
                Case c{"thin tiles", kpu, nb, 2, 2, 0, {}};
                for (u32 i = 0; i < 60; ++i) c.tiles.push_back(make_tile(i / 45, nb, std::max(1u, nb / 2) * (1 + (u32)(rng() % 3)), rng));
                for (u32 i = 0; i < 6; ++i) c.tiles.push_back(make_tile(1, nb, 0, rng));          // and tiles without a k-mer
                cases.push_back(c);
            }
            {   // a segment change at every tile
                Case c{"segment change at every tile", kpu, nb, 24, 3, 0, {}};
                for (u32 i = 0; i < 24; ++i) c.tiles.push_back(make_tile(i, nb, (u32)(rng() % (full / 4)), rng));
                cases.push_back(c);
            }
            {   // nearly all keys in two buckets
                Case c{"two hot buckets", kpu, nb, 2, 1, 0, {}};
                for (u32 i = 0; i < 16; ++i) c.tiles.push_back(make_tile(i / 8, nb, full - (u32)(rng() % 100), rng, std::min(nb, 2u)));
                cases.push_back(c);
            }
            {   // regions too small: the overflow path while a carry is pending
                Case c{"small regions (overflow)", kpu, nb, 3, 2, 64, {}};
                for (u32 i = 0; i < 18; ++i) c.tiles.push_back(make_tile(i / 6, nb, (u32)(rng() % (full / 2)), rng));
                cases.push_back(c);
            }
        }
    }
    for (const Case& c : cases) run_case(c, rng);
    printf("%zu cases, %d failed checks\n", cases.size(), fails);
    return fails ? 1 : 0;
}
