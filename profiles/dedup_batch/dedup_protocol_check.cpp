// Host-side check of the probe and claim protocol of the 64-bit de-duplication table (k_bucket_dedup, kernels_build.hip),
// restated in plain C++ over an array table.  Stand-alone: build with -fsanitize=address,undefined and run; exit status 0
// means every assertion held.
//
// The protocol, as in the kernel:
//   * the table is NSETS sets of two slots; a key's probe sequence is home A (top bits of khash), home B (A xor the next
//     field of khash, never zero), then A+1, A+2, ... (mod NSETS): a pure function of the key;
//   * a lane takes a batch of keys: it reads the snapshots of A and B of every key of a sub-batch, counts hits, and
//     claims new keys — one CAS per key on the FIRST empty slot of the first snapshot with room, all issued before any
//     outcome is looked at — then adds the counts; CAS returns EMPTY (inserted), the key (a hit) or another key (missed);
//   * missed keys (lost claims restart at the set they lost in; keys whose A and B were full of others start at A+1) go
//     through the one-key probe loop, which re-reads before every claim and is bounded by 8 * NSETS probes;
//   * slots never change once written.
// Lanes are threads.  Two schedules: free-running threads, and a seeded baton that lets exactly one lane run between any
// two table operations (a fixed interleaving per seed: stale snapshots and lost races happen on every machine alike).
// Checked afterwards: no key in two slots, every count equals the key's multiplicity, the distinct counter equals the
// number of filled slots, and every key is found by walking its probe sequence before a set with room (searchable).
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

using u32 = uint32_t;
using u64 = uint64_t;
static const u64 EMPTY = ~0ull;
static const int KPL = 6, SUB = 3;      // keys per lane and batch, keys per sub-batch (the 2048-slot kernel's)

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

static u32 khash(u64 a) {               // keyops.h
    const u32 lo = (u32)a, hi = (u32)(a >> 32);
    u32 x = lo ^ ((hi << 13) | (hi >> 19));
    x ^= x >> 17;
    return ((x & 0xFFFFFFu) * 0xB5297Au) ^ (((x >> 8) & 0xFFFFFFu) * 0x68E31Du);
}

struct Baton {                          // one lane runs at a time; pass() hands over to a seeded-random live lane
    bool on = false;
    std::mutex m;
    std::condition_variable cv;
    std::mt19937 rng;
    std::vector<int> live;
    int turn = -1;
    void start(int n, u32 seed) { rng.seed(seed); live.clear(); for (int i = 0; i < n; ++i) live.push_back(i); turn = live[rng() % live.size()]; }
    void enter(int me) { if (!on) return; std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return turn == me; }); }
    void pass(int me) {
        if (!on) return;
        std::unique_lock<std::mutex> l(m);
        turn = live[rng() % live.size()];
        cv.notify_all();
        cv.wait(l, [&] { return turn == me; });
    }
    void leave(int me) {
        if (!on) return;
        std::unique_lock<std::mutex> l(m);
        for (size_t i = 0; i < live.size(); ++i) if (live[i] == me) { live.erase(live.begin() + i); break; }
        turn = live.empty() ? -1 : live[rng() % live.size()];
        cv.notify_all();
    }
};

struct Table {
    int log_sets;
    u32 nsets;
    std::vector<std::atomic<u64>> key;
    std::vector<std::atomic<u32>> cnt;
    std::atomic<u32> distinct{0}, overflow{0};
    explicit Table(int ls) : log_sets(ls), nsets(1u << ls), key(2u << ls), cnt(2u << ls) {
        for (auto& k : key) k.store(EMPTY);
        for (auto& c : cnt) c.store(0);
    }
    u32 home_a(u32 h) const { return h >> (32 - log_sets); }
    u32 home_b(u32 h) const { const u32 d = (h >> (32 - 2 * log_sets)) & (nsets - 1); return home_a(h) ^ (d ? d : 1u); }
    u32 probe_set(u64 k, u32 step) const {
        const u32 h = khash(k);
        return step == 0 ? home_a(h) : step == 1 ? home_b(h) : (home_a(h) + step - 1) & (nsets - 1);
    }
};

struct Snap { u64 x, y; };
static u32 look(const Snap& c, u64 key) { return c.x == key ? 0u : c.y == key ? 1u : c.x == EMPTY ? 2u : c.y == EMPTY ? 3u : 4u; }

struct Lane {
    Table& t;
    Baton& b;
    int id;
    Snap read(u32 set) {                // (the two halves of the 16-byte read may even be seen at different times here)
        Snap s;
        s.x = t.key[2 * set].load(std::memory_order_relaxed);
        b.pass(id);
        s.y = t.key[2 * set + 1].load(std::memory_order_relaxed);
        b.pass(id);
        return s;
    }
    u64 cas(u32 slot, u64 key) {
        u64 old = EMPTY;
        t.key[slot].compare_exchange_strong(old, key, std::memory_order_relaxed);
        b.pass(id);
        return old;                     // EMPTY: inserted; otherwise what the slot holds
    }
    // dedup_step: one probe at probe state st
    bool step(u64 key, u32& st) {
        const u32 set = t.probe_set(key, st);
        const Snap c = read(set);
        const u32 r = look(c, key);
        if (r == 4u) { ++st; return false; }
        if (r >= 2u) {
            const u64 old = cas(2 * set + (r & 1u), key);
            if (old == EMPTY) t.distinct.fetch_add(1, std::memory_order_relaxed);
            else if (old != key) return false;
        }
        t.cnt[2 * set + (r & 1u)].fetch_add(1, std::memory_order_relaxed);
        b.pass(id);
        return true;
    }
    void batch(const u64* kx, int n) {  // n <= KPL keys (a tail batch has fewer)
        u32 missed = 0, mstep = 0, nins = 0;
        for (int q0 = 0; q0 < n; q0 += SUB) {
            const int m = n - q0 < SUB ? n - q0 : SUB;
            Snap ca[SUB], cb[SUB];
            u32 sa[SUB], sb[SUB], at[SUB], claim = 0;
            for (int j = 0; j < m; ++j) {
                const u32 h = khash(kx[q0 + j]);
                sa[j] = t.home_a(h); sb[j] = t.home_b(h);
                CHECK(sa[j] != sb[j], "homes of %llx", (unsigned long long)kx[q0 + j]);
                ca[j] = read(sa[j]);
                cb[j] = read(sb[j]);
            }
            for (int j = 0; j < m; ++j) {
                const u64 key = kx[q0 + j];
                at[j] = ~0u;
                u32 r = look(ca[j], key), base = 2 * sa[j];
                const u32 rb = look(cb[j], key);
                const bool to_b = r == 4u;
                r = to_b ? rb : r;
                base = to_b ? 2 * sb[j] : base;
                mstep |= (to_b ? (r == 4u ? 2u : 1u) : 0u) << (2 * (q0 + j));
                if (r == 4u) { missed |= 1u << (q0 + j); continue; }
                at[j] = base + (r & 1u);
                claim |= (r >> 1) << j;
            }
            u64 old[SUB] = {};
            for (int j = 0; j < m; ++j) if (claim >> j & 1u) old[j] = cas(at[j], kx[q0 + j]);
            for (int j = 0; j < m; ++j)
                if (claim >> j & 1u) {
                    if (old[j] == EMPTY) ++nins;
                    else if (old[j] != kx[q0 + j]) { missed |= 1u << (q0 + j); at[j] = ~0u; }
                }
            for (int j = 0; j < m; ++j) if (at[j] != ~0u) { t.cnt[at[j]].fetch_add(1, std::memory_order_relaxed); b.pass(id); }
        }
        if (nins) t.distinct.fetch_add(nins, std::memory_order_relaxed);
        while (missed) {
            const u32 q = (u32)__builtin_ctz(missed);
            missed &= missed - 1;
            u32 st = (mstep >> (2 * q)) & 3u;
            bool ok = false;
            for (u32 probe = 0; probe < 8 * t.nsets && !ok; ++probe) ok = step(kx[q], st);
            if (!ok) t.overflow.store(1);
        }
    }
};

// all lanes put `keys` through a table of 2^log_sets sets; lane l takes keys l*KPL .. of every stride of lanes*KPL keys
static void run(const char* name, const std::vector<u64>& keys, int log_sets, int lanes, bool baton, u32 seed, bool may_overflow) {
    Table t(log_sets);
    Baton b;
    b.on = baton;
    if (baton) b.start(lanes, seed);
    std::vector<std::thread> th;
    for (int l = 0; l < lanes; ++l)
        th.emplace_back([&, l] {
            Lane lane{t, b, l};
            b.enter(l);
            for (size_t c = (size_t)l * KPL; c < keys.size(); c += (size_t)lanes * KPL) {
                const int n = keys.size() - c < (size_t)KPL ? (int)(keys.size() - c) : KPL;
                lane.batch(&keys[c], n);
            }
            b.leave(l);
        });
    for (auto& x : th) x.join();
    std::map<u64, u32> want;
    for (u64 k : keys) ++want[k];
    // no key in two slots; counts; the distinct counter; sets fill left to right
    std::map<u64, u32> where;
    u32 filled = 0;
    for (u32 s = 0; s < 2 * t.nsets; ++s) {
        const u64 k = t.key[s].load();
        if (k == EMPTY) { CHECK(t.cnt[s].load() == 0, "%s: count in an empty slot %u", name, s); continue; }
        ++filled;
        CHECK(want.count(k), "%s: slot %u holds a key nobody inserted", name, s);
        CHECK(!where.count(k), "%s: key %llx in slots %u and %u", name, (unsigned long long)k, where[k], s);
        where[k] = s;
        if (s & 1u) CHECK(t.key[s - 1].load() != EMPTY, "%s: set %u filled right to left", name, s / 2);
    }
    CHECK(t.distinct.load() == filled, "%s: distinct counter %u, filled slots %u", name, t.distinct.load(), filled);
    if (t.overflow.load()) {
        CHECK(may_overflow, "%s: overflow with %zu distinct keys in %u slots", name, want.size(), 2 * t.nsets);
        CHECK(filled == 2 * t.nsets, "%s: overflow raised with %u of %u slots filled", name, filled, 2 * t.nsets);
        for (auto& kv : where) CHECK(t.cnt[kv.second].load() <= want[kv.first], "%s: a count above the multiplicity", name);
        std::printf("ok  %-34s %7zu keys, overflow raised on a full table\n", name, keys.size());
        return;
    }
    CHECK(where.size() == want.size(), "%s: %zu distinct keys in the table, %zu in the input", name, where.size(), want.size());
    for (auto& kv : want) {
        CHECK(t.cnt[where[kv.first]].load() == kv.second, "%s: key %llx counted %u times, occurs %u times", name,
              (unsigned long long)kv.first, t.cnt[where[kv.first]].load(), kv.second);
        // searchable: walking the probe sequence meets the key before any set with room
        bool found = false;
        for (u32 st = 0; st <= t.nsets + 1 && !found; ++st) {
            const u32 set = t.probe_set(kv.first, st);
            const u64 x = t.key[2 * set].load(), y = t.key[2 * set + 1].load();
            if (x == kv.first || y == kv.first) found = true;
            else CHECK(x != EMPTY && y != EMPTY, "%s: key %llx lives behind set %u, which has room", name, (unsigned long long)kv.first, set);
        }
        CHECK(found, "%s: key not found on its probe sequence", name);
    }
    std::printf("ok  %-34s %7zu keys, %6zu distinct, %s\n", name, keys.size(), want.size(), baton ? "baton" : "threads");
}

int main() {
    std::mt19937_64 rng(12345);
    auto rnd_keys = [&](size_t n, size_t distinct) {
        std::vector<u64> pool(distinct), out(n);
        for (auto& k : pool) k = rng() >> 2;                   // (2k <= 62 bits: never the EMPTY pattern)
        for (auto& k : out) k = pool[rng() % distinct];
        return out;
    };
    // keys that share home A (and, for `both`, home B too) in a table of 2^ls sets
    auto same_home = [&](size_t distinct, int ls, bool both) {
        Table t(ls);
        std::vector<u64> pool;
        while (pool.size() < distinct) {
            const u64 k = rng() >> 2;
            const u32 h = khash(k);
            if (t.home_a(h) == 3 && (!both || t.home_b(h) == 5)) pool.push_back(k);
        }
        return pool;
    };
    for (int baton = 1; baton >= 0; --baton) {
        const u32 seeds = baton ? 3 : 3;
        const size_t f = baton ? 4 : 1;          // (a baton hand-over per table operation: fewer keys)
        for (u32 seed = 0; seed < seeds; ++seed) {
            const int lanes = baton ? 5 + (int)seed : 8;
            run("every lane claims the same slot", std::vector<u64>(600 / f, 0x0123456789ull), 10, lanes, baton, seed, false);
            run("random, 600 distinct in 2048 slots", rnd_keys(6000 / f, 600), 10, lanes, baton, seed, false);
            run("random, up to the 11/16 limit", rnd_keys(8000 / f, 1408), 10, lanes, baton, seed, false);
            run("random, tail batches", rnd_keys(6 * lanes * 7 + 5, 90), 6, lanes, baton, seed, false);
            {   // one home A: the keys spill into their homes B, then A+1, A+2, ...
                auto pool = same_home(40, 6, false);
                std::vector<u64> ks;
                for (int r = 0; r < (baton ? 6 : 20); ++r) for (u64 k : pool) ks.push_back(k);
                run("40 keys with one home A", ks, 6, lanes, baton, seed, false);
            }
            {   // one home A and one home B: everything beyond four keys walks A+1, A+2, ...
                auto pool = same_home(24, 4, true);
                std::vector<u64> ks;
                for (int r = 0; r < (baton ? 6 : 15); ++r) for (u64 k : pool) ks.push_back(k);
                run("24 keys with the same two homes", ks, 4, lanes, baton, seed, false);
            }
            run("a table filled to the last slot", rnd_keys(1500 / f, 32), 4, lanes, baton, seed, true);
            run("more distinct keys than slots", rnd_keys(1200 / f, 48), 4, lanes, baton, seed, true);
        }
    }
    std::printf("dedup protocol check: all passed\n");
    return 0;
}
