// taf_column.h -- the consumer side of the chunk-major partition: a bin's column of the directory (col_*: loaders, run gather, addresses) and the LDS fences.
// Expects frlw_common.h (wave_incl_scan) and taf_plan.h (SeqTab, kColMax).
#pragma once
#include "frlw_common.h"
#include "taf_plan.h"

namespace {
using namespace frlw;
#define LDS_FENCE() asm volatile("" ::: "memory")
#define LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory") // workgroup barrier that publishes LDS only: loads / stores in flight stay in flight

// ---- the consumer side of the chunk-major partition: a bin's column of the directory ----------------------------------

struct CmP { // kernel argument of the chunk-major consumers
    const uint32_t *dir; // [TB][n_chunks]: count << 16 | offset of the bin's run inside the chunk's records
    int n_chunks;        // chunks of the call (all sequences)
    const uint32_t *rec; // chunk-major records (kf_scatter_cm)
    int TB;              // bins per sequence
    int chunk_ev;        // events per chunk = records a chunk's stretch of rec[] can hold
    uint32_t *hot_start; // [pairs] skewed tiles: where the tile's 16 lists start in rec2[]
    uint32_t *hot_seg0;  // [pairs] ... and the id of the tile's first split segment
    uint32_t *segdesc;   // [max_segs] pair of every split segment
    int max_segs;
};

// Column of bin `b` of sequence `s`: L[c] = records of the bin in the sequence's chunks before c (L[C] = all of them, the
// return value), D[c] = index in rec[] of the bin's first record of chunk c MINUS L[c] -- list position i (stream order) is
// rec[D[c] + i] for the chunk c with L[c] <= i < L[c + 1].  NT threads, workgroup barriers inside; wsum: NT / 64 + 1 words.
template <int NT>
__device__ __forceinline__ uint32_t col_load(const CmP &m, const SeqTab &S, int s, int b, uint32_t *L, uint32_t *D, uint32_t *wsum)
{
    constexpr int NWV = NT / kWave;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wvs = __builtin_amdgcn_readfirstlane(wv);
    const int c0 = S.chunk0[s], C = S.chunk0[s + 1] - c0; // >= 1: an empty sequence keeps one (empty) chunk
    const uint32_t out0 = (uint32_t)(S.ev0[s] - S.ev0[0]);
    uint32_t carry = 0;
    for (int cb = 0; cb < C; cb += NT) { // passes of NT chunks, one per thread (workgroup-uniform trip count: usually one)
        const int c = cb + tid;
        // (clamped index, masked value: no load sits under a lane condition)
        const uint32_t v = m.dir[(long long)b * m.n_chunks + (c0 + (c < C ? c : C - 1))];
        const uint32_t e = c < C ? v : 0u, cnt = e >> 16;
        const uint32_t inc = wave_incl_scan(cnt);
        if (lane == kWave - 1) wsum[wv] = inc;
        __syncthreads();
        // the wavefronts' sums, scanned by every wavefront for itself with lane k = wavefront k: the sum of the wavefronts in front
        // of this one and the pass's total come out of two lanes as SCALARS.  (As "for k: if (k < wv) run += wsum[k]" the compiler
        // kept the NWV - 1 lane masks of `k < wv` in scalar register pairs across the pass: 30 of them in a 1024-thread kernel,
        // which pushed kf_split_whole<true>'s list pointers out into a vector register -- the one its gather then spilled a record for.)
        const uint32_t ws = lane < NWV ? wsum[lane] : 0u, wsi = wave_incl_scan(ws);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)wsi, NWV - 1);
        const uint32_t run = carry + inc - cnt + (uint32_t)__builtin_amdgcn_readlane((int)(wsi - ws), wvs);
        if (c < C) {
            L[c] = run;
            D[c] = out0 + (uint32_t)c * (uint32_t)m.chunk_ev + (e & 0xffffu) - run;
        }
        carry += total;
        __syncthreads(); // wsum is reused by the next pass
    }
    if (tid == 0) L[C] = carry;
    __syncthreads();
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)carry); // (uniform for the compiler too: scalar branches downstream)
}

// The same column (same L, D and return value) made by ONE wavefront, 64 chunks per step, for workgroups whose wavefronts work on
// different bins and share no barrier (kf_ev_sub<., true>).  No barrier inside: the wavefront reads L / D back behind an LDS_FENCE().
__device__ __forceinline__ uint32_t col_load_wave(const CmP &m, const SeqTab &S, int s, int b, uint32_t *L, uint32_t *D)
{
    const int lane = threadIdx.x & 63;
    const int c0 = S.chunk0[s], C = S.chunk0[s + 1] - c0;
    const uint32_t out0 = (uint32_t)(S.ev0[s] - S.ev0[0]);
    uint32_t n = 0;
    for (int cb = 0; cb < C; cb += kWave) { // (wave-uniform trip count)
        const int c = cb + lane;
        const uint32_t v = m.dir[(long long)b * m.n_chunks + (c0 + (c < C ? c : C - 1))];
        const uint32_t e = c < C ? v : 0u, cnt = e >> 16;
        const uint32_t inc = wave_incl_scan(cnt), run = n + inc - cnt;
        if (c < C) { L[c] = run; D[c] = out0 + (uint32_t)c * (uint32_t)m.chunk_ev + (e & 0xffffu) - run; }
        n += (uint32_t)__builtin_amdgcn_readlane((int)inc, kWave - 1);
    }
    if (lane == 0) L[C] = n;
    return n;
}

// The runs of a column, in chunk order: sink(list position, record word) for every record of the list.  NG groups of 16 lanes (this
// thread: lane l16 of group g16) take runs g16, g16 + NG, ...; a step issues the loads of RU runs' first 16 records, then their
// sinks, then the tails of the runs above 16 records.  (Clamped index: a lane behind a run's end re-reads an address that exists.)
template <int NG, int RU, class Sink>
__device__ __forceinline__ void col_gather(const uint32_t *L, const uint32_t *D, int C, int g16, int l16, const uint32_t *rec, Sink sink)
{
    for (int cc0 = g16; cc0 < C; cc0 += NG * RU) {
        uint32_t v[RU], at[RU], cnt[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int c = cc0 + NG * u, cc = c < C ? c : C - 1;
            const uint32_t lo = L[cc];
            cnt[u] = c < C ? L[cc + 1] - lo : 0u;
            at[u] = lo;
            v[u] = rec[D[cc] + lo + ((uint32_t)l16 < cnt[u] ? (uint32_t)l16 : 0u)];
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            if ((uint32_t)l16 < cnt[u]) sink(at[u] + l16, v[u]);
            if (cnt[u] > 16u) { // (wave-divergent, rare for the short runs of a direct-mode call)
                const int c = cc0 + NG * u; // (L[c] again, not at[u]: a sink that ignores the position then keeps no at[] alive)
                const uint32_t d = D[c], lo = L[c];
                for (uint32_t j = 16u + l16; j < cnt[u]; j += 16u) sink(lo + j, rec[d + lo + j]);
            }
        }
    }
}

// idx[(i - lo) >> 4] = the chunk that holds list position i, for every i = lo (mod 16) ... in [lo, hi) -- lo a multiple of 16:
// a lane then finds its own position's chunk with the short walk of col_addr instead of a bisection.  Call after col_load.
template <int NT>
__device__ __forceinline__ void col_index(const uint32_t *L, int C, uint32_t lo, uint32_t hi, uint16_t *idx)
{
    for (int c = threadIdx.x; c < C; c += NT) {
        const uint32_t a = L[c] > lo ? L[c] : lo, z = L[c + 1] < hi ? L[c + 1] : hi;
        for (uint32_t i = (a + 15u) & ~15u; i < z; i += 16u) idx[(i - lo) >> 4] = (uint16_t)c;
    }
}

__device__ __forceinline__ uint32_t col_addr(const uint32_t *L, const uint32_t *D, uint32_t c, uint32_t i); // below

// The same for one wavefront's 64 consecutive positions lo + r0 .. lo + r0 + 63 of a range [lo, lo + nr) indexed by idx (this
// lane: lo + ric): when they all lie inside ONE run -- the rule for the long runs of a skewed tile -- the run is found once,
// with scalar compares, and a lane only adds.
__device__ __forceinline__ uint32_t col_addr_wave(const uint32_t *L, const uint32_t *D, const uint16_t *idx, uint32_t lo, uint32_t r0,
                                                  uint32_t ric, uint32_t nr)
{
    if (r0 >= nr) return D[0] + L[0]; // (wave-uniform: nothing of this wavefront's batch is inside the range; any address that exists)
    const uint32_t i0 = lo + r0, last = lo + (r0 + 63u < nr ? r0 + 63u : nr - 1u);
    uint32_t cs = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx[r0 >> 4]);
    uint32_t lnext = (uint32_t)__builtin_amdgcn_readfirstlane((int)L[cs + 1]);
    while (lnext <= i0) { ++cs; lnext = (uint32_t)__builtin_amdgcn_readfirstlane((int)L[cs + 1]); }
    if (lnext > last) return (uint32_t)__builtin_amdgcn_readfirstlane((int)D[cs]) + lo + ric;
    return col_addr(L, D, idx[ric >> 4], lo + ric);
}

__device__ __forceinline__ uint32_t col_addr(const uint32_t *L, const uint32_t *D, uint32_t c, uint32_t i) // c: a chunk at or in front of i's
{
    // (i < L[C]: ends inside the column; empty runs are stepped over).  Two steps without a branch -- 16 positions rarely span
    // more runs -- then the loop for whoever is still short
    c += L[c + 1] <= i ? 1u : 0u;
    c += L[c + 1] <= i ? 1u : 0u;
    if (__builtin_expect(__ballot(L[c + 1] <= i) != 0ull, 0))
        while (L[c + 1] <= i) ++c;
    return D[c] + i;
}
} // namespace
