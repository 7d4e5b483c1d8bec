// taf_blocktab.h -- the block address table of kf_split_whole<true>: one 8-byte entry per 16 positions of a bin's list, made from the
// bin's column (taf_column.h: L[c] = records in front of chunk c, D[c] = address of the run's first record MINUS L[c]), so that a lane
// finds rec[]'s index of its list position with ONE LDS read and no walk.
// Pure integer arithmetic: NO HIP header and no HIP type, so tests/host/blocktab_check.cpp runs it without a GPU.
// Expects nothing before it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FRLW_BT_HD __host__ __device__ __forceinline__
#else
#define FRLW_BT_HD inline
#endif

namespace frlw_bt {
// Block k = positions 16 k .. 16 k + 15.  With a = the run that holds position 16 k and b = the next run that is not empty:
//   a = D[a]
//   w = (D[b] - D[a]) << 4 | (L[b] - 16 k)   when b starts inside the block (L[b] - 16 k is 1 .. 15)
//   w = 0                                    when the whole block lies in run a (or the list ends inside it)
// -> address of position i = a + i + ((i & 15) >= (w & 15) ? w >> 4 : 0).  D[b] - D[a] >= 0: the runs lie at ascending addresses and
// run b starts behind run a's last record; it is below 2^28 while rec[] holds fewer than 2^28 records.
// A block that holds a SECOND run boundary (runs shorter than 16 records, a skewed neighbour) or whose difference does not fit is
// marked w = kBtFallback, a = the chunk of run a: whoever reads it walks the column from there (bt_walk; col_addr on the GPU).
constexpr uint32_t kBtFallback = 0xffffffffu;
constexpr int kBtCols = 1024; // chunks per sequence up to which column + table fit the staging area (8 KB + 16 KB of 32 KB)

struct alignas(8) BtEntry {
    uint32_t a, w;
};

// The entries of the blocks that START inside run c (none for an empty run or one that covers no multiple of 16), n = L[C].
FRLW_BT_HD void bt_build_run(const uint32_t *L, const uint32_t *D, int C, int c, uint32_t n, BtEntry *tab)
{
    const uint32_t hi = L[c + 1];
    uint32_t i = (L[c] + 15u) & ~15u;
    if (i >= hi) return;
    const uint32_t da = D[c];
    for (; hi - i >= 16u; i += 16u) tab[i >> 4] = BtEntry{da, 0u}; // whole blocks of the run
    if (i >= hi) return;
    // the block the run ends in: 16 k = i < hi < i + 16
    BtEntry e{da, 0u};
    if (hi < n) { // (else: the list ends here too)
        int b = c + 1;
        while (b < C - 1 && L[b + 1] == hi) ++b; // empty runs in between (hi < n: a run with records follows)
        const uint32_t end = n - i < 16u ? n : i + 16u, delta = D[b] - da;
        const uint32_t w = delta << 4 | (hi - i);
        if (L[b + 1] < end || delta >= (1u << 28) || w == kBtFallback) e = BtEntry{(uint32_t)c, kBtFallback};
        else e.w = w;
    }
    tab[i >> 4] = e;
}

FRLW_BT_HD uint32_t bt_addr(BtEntry e, uint32_t i) { return e.a + i + ((i & 15u) >= (e.w & 15u) ? e.w >> 4 : 0u); } // e.w != kBtFallback

// The plain definition: position i (< L[C]) lies in the chunk c with L[c] <= i < L[c + 1], at D[c] + i; from a chunk at or in front of it.
FRLW_BT_HD uint32_t bt_walk(const uint32_t *L, const uint32_t *D, uint32_t c, uint32_t i)
{
    while (L[c + 1] <= i) ++c;
    return D[c] + i;
}
} // namespace frlw_bt
