// blocktab_check.cpp -- the block address table of kf_split_whole<true> (csrc/taf_blocktab.h) checked on the CPU, without HIP: for
// random columns -- runs of 0, 1, a few, a few dozen and 65 535 records in every mix, gaps between the runs' addresses from none to
// beyond 2^28 -- the table is built the way the kernel builds it (one bt_build_run per chunk, in any order) and EVERY list position's
// address through the table (or, for a block marked as fallback, through the walk from the chunk the entry names) must be the one the
// plain L / D definition gives.  Built with -fsanitize=address,undefined by tests/test_blocktab_cpu.py; exit status 0 = all held.
#include "taf_blocktab.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <vector>

using namespace frlw_bt;

static long long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                                   \
    do {                                                                                                   \
        ++g_checks;                                                                                        \
        if (!(cond) && ++g_failed <= 20) { fprintf(stderr, "FAILED %s  [", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "]\n"); } \
    } while (0)

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s * 0x2545F4914F6CDD1Dull; }
    uint32_t below(uint32_t n) { return (uint32_t)((next() >> 32) * (uint64_t)n >> 32); }
};

static long long g_columns = 0, g_positions = 0, g_blocks = 0, g_fallback = 0, g_two_part = 0;

// one column: cnt[c] records in chunk c, whose run starts gap[c] addresses behind the end of the run in front of it
static void check_column(const std::vector<uint32_t> &cnt, const std::vector<uint32_t> &gap, uint32_t addr0, Rng &rng, int id)
{
    const int C = (int)cnt.size();
    std::vector<uint32_t> L(C + 1), D(C), first(C);
    uint32_t at = addr0;
    L[0] = 0;
    for (int c = 0; c < C; ++c) {
        at += gap[c];
        first[c] = at;
        D[c] = at - L[c];
        L[c + 1] = L[c] + cnt[c];
        at += cnt[c];
    }
    const uint32_t n = L[C];
    ++g_columns;
    if (n == 0) return; // (the kernel leaves before the table is made)
    const size_t nb = ((size_t)n + 15) / 16;
    // built twice over different fillers: an entry that is the same in both was written, and the order of the chunks does not matter
    std::vector<BtEntry> tab(nb, BtEntry{0xdeadbeefu, 0x12345670u}), tab2(nb, BtEntry{0x0badf00du, 0x76543210u});
    std::vector<int> order(C);
    std::iota(order.begin(), order.end(), 0);
    for (int c = 0; c < C; ++c) bt_build_run(L.data(), D.data(), C, c, n, tab.data());
    for (int c = C - 1; c > 0; --c) std::swap(order[c], order[rng.below((uint32_t)c + 1)]);
    for (int c : order) bt_build_run(L.data(), D.data(), C, c, n, tab2.data());
    for (size_t k = 0; k < nb; ++k) {
        CHECK(tab[k].a == tab2[k].a && tab[k].w == tab2[k].w, "column %d block %zu of %zu: not written", id, k, nb);
        ++g_blocks;
        if (tab[k].w == kBtFallback) { ++g_fallback; CHECK(tab[k].a < (uint32_t)C && L[tab[k].a] <= 16 * k, "column %d block %zu: fallback chunk %u", id, k, tab[k].a); }
        else if (tab[k].w != 0u) { ++g_two_part; CHECK((tab[k].w & 15u) != 0u, "column %d block %zu: boundary at 0", id, k); }
    }
    uint32_t i = 0;
    for (int c = 0; c < C; ++c)
        for (uint32_t j = 0; j < cnt[c]; ++j, ++i) {
            const BtEntry e = tab[i >> 4];
            const uint32_t got = e.w == kBtFallback ? bt_walk(L.data(), D.data(), e.a, i) : bt_addr(e, i);
            CHECK(got == first[c] + j, "column %d position %u (chunk %d + %u): %u, want %u; entry %08x %08x", id, i, c, j, got, first[c] + j, e.a, e.w);
            ++g_positions;
        }
}

static uint32_t draw_count(Rng &rng, int kind)
{
    switch (kind) {
    case 0: return 0u;
    case 1: return 1u;
    case 2: return 1u + rng.below(15u);  // shorter than a block
    case 3: return 16u * (1u + rng.below(4u)); // whole blocks: boundaries on multiples of 16 while the runs in front are too
    case 4: return 20u + rng.below(50u); // the headline's ~43
    case 5: return 200u + rng.below(100u); // 64 GEN1 streams
    default: return 65535u;               // the directory's largest count
    }
}

int main(int argc, char **argv)
{
    const int n_cols = argc > 1 ? atoi(argv[1]) : 1500;
    Rng rng(20240607);
    for (int id = 0; id < n_cols; ++id) {
        const int C = id % 7 == 0 ? 1 + (int)rng.below(3) : 1 + (int)rng.below(id % 5 == 0 ? kBtCols : 96);
        // the mix of run lengths of this column: every pure kind, then random weights
        int weight[7];
        for (int k = 0; k < 7; ++k) weight[k] = id < 7 ? (k == id ? 1 : 0) : (int)rng.below(4);
        if (id >= 7 && id % 10 != 3) weight[6] = 0; // (most columns without the 65 535-record runs: they take the time)
        int wsum = 0;
        for (int k = 0; k < 7; ++k) wsum += weight[k];
        if (wsum == 0) { weight[4] = 1; wsum = 1; }
        // gaps: none (runs back to back), a chunk's stretch, or -- every 11th column -- up to 2^24: over a few dozen chunks the difference
        // between neighbouring runs' D then passes 2^28 somewhere
        const uint32_t gap_max = id % 11 == 10 ? (1u << 24) : (id % 2 ? 0u : 20480u);
        std::vector<uint32_t> cnt(C), gap(C);
        uint64_t total = 0;
        for (int c = 0; c < C; ++c) {
            int r = (int)rng.below((uint32_t)wsum), kind = 0;
            while (r >= weight[kind]) r -= weight[kind++];
            cnt[c] = draw_count(rng, kind);
            if (kind == 6 && total > (2u << 20)) cnt[c] = draw_count(rng, 4); // (a few dozen of them per column at the most)
            gap[c] = gap_max ? rng.below(gap_max + 1u) : 0u;
            if (id % 11 == 10 && c % 20 == 7) gap[c] = (1u << 28) + rng.below(1u << 20); // one difference that does not fit 28 bits
            if (id % 11 == 10 && c >= 60) gap[c] = rng.below(4096u);                      // (the addresses stay below 2^32)
            total += cnt[c];
        }
        check_column(cnt, gap, rng.below(1u << 20), rng, id);
    }
    // the edges by hand: a boundary exactly on a multiple of 16, a list of exactly 16 k records, 8192 and 8193 records, a lone record
    // behind a 65 535-record run, empty runs at both ends and between two boundaries of one block
    const std::vector<std::vector<uint32_t>> edges = {
        {16, 16, 32, 1}, {32}, {8192}, {8193}, {8191, 1, 1}, {65535, 1}, {1, 65535, 0, 0, 1}, {0, 0, 5, 0, 0, 3, 0, 9, 0}, {15, 1, 15, 1}, {0},
        {0, 0, 0}, {17, 0, 0, 0, 15, 0, 1}, {3, 3, 3, 3, 3, 3, 3}, {16, 0, 16}, {1}, {15}, {16}, {17}};
    int id = n_cols;
    for (const auto &cnt : edges)
        for (uint32_t g : {0u, 7u, 20480u}) check_column(cnt, std::vector<uint32_t>(cnt.size(), g), 5u, rng, id++);
    printf("blocktab_check: %lld columns, %lld positions, %lld blocks (%lld with a boundary, %lld fallback), %lld checks, %lld failed\n", g_columns, g_positions,
           g_blocks, g_two_part, g_fallback, g_checks, g_failed);
    return g_failed ? 1 : 0;
}
