// taf_split.h -- the second level: a tile's records sub-tile-major, stably (kf_split_whole, the segment kernels kf_split_place and
// kf_segcount_cm); TileP, the kernel argument it shares with the walk.
// Expects taf_decode.h (FastHeader), taf_partition.h (whole_max_of, split_segments), taf_column.h and taf_blocktab.h.
#pragma once
#include "taf_blocktab.h"
#include "taf_column.h"
#include "taf_partition.h"
#include <type_traits>

namespace {
// ---- 4. per-tile split by sub-tile (5., one workgroup per sub-tile: taf_walk.h) ------------------------------
struct TileP {
    int H, W, twl, thl, tiles_x, T, K, n_windows, wb, flip;
    uint32_t win;
    const uint32_t *rec;   // tile-major records (scatter output)
    uint32_t *rec2;        // the same records, inside every tile sub-tile-major (split output)
    const uint32_t *base;  // [pairs + 1]
    uint32_t *sub;         // [pairs * 16 + 1] first record of every sub-tile in rec2
    uint32_t *sub_end;     // chunk-major partition: [pairs * 16] end of every sub-tile's list (lists are placed through a cursor,
                           // not back to back in pair order); NULL otherwise: a list ends where the next one starts
    const uint32_t *seg0;  // [pairs + 1] first split segment of every (sequence, tile) pair
    uint32_t *segcnt;      // [segments][16] records of every sub-tile in a segment, then their offsets inside the sub-tile
    int pairs;
    int direct;            // 1: rec2 / sub are the scatter's own output (sub-tile bins): no split kernel has run
    int seg_grid;          // segment workgroups launched (they stride over the segments: most calls have none)
    uint32_t tile_max;     // tiles with more records than this go through the segment split
    const float *tlut;
    const uint32_t *leaky_thr;
    FastHeader *hdr;
    double rcp;      // FastGeom::rcp
    float *state;    // (B, H, W, 2, K)
    float *view_f32; // (B, 2K, H, W) or NULL
    uint8_t *out_u8; // (B, K, 2, H, W) or NULL
    // window starts, written by kf_split_whole<true> for the tiles it splits (TAF only; NULL otherwise): wst[sg * (n_windows + 1)
    // + w] = list position of the first record of window w in sub-tile list sg, 0xffffffff: the window has none -- what the walk's
    // own scan finds; wst_flag[pair] = 0: no table (the walk scans its list), 1: table valid, 2: a list of the tile is not
    // window-sorted (the walk filters the whole list per window)
    uint32_t *wst, *wst_flag;
};

__device__ __forceinline__ int pair_of_segment(const uint32_t *seg0, int pairs, uint32_t seg)
{
    int lo = 0, hi = pairs; // largest g with seg0[g] <= seg
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg0[mid] <= seg) lo = mid; else hi = mid;
    }
    return lo;
}

// Count the records of rec[beg, end) per (wavefront, sub-tile) into wtot: eight loads in flight per thread (indices
// clamped, values masked -- a load under a lane condition, or one load per loop iteration, is one exposed round trip each:
// a 22 000-record tile took 22 of them).
__device__ __forceinline__ void count_subtiles(const uint32_t *rec, uint32_t beg, uint32_t end, uint32_t (*wtot)[kFW])
{
    const int tid = threadIdx.x, wv = tid >> 6;
    for (uint32_t c0 = beg; c0 < end; c0 += 8 * kFT) {
        uint32_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t i = c0 + (uint32_t)(u * kFT + tid);
            v[u] = rec[i < end ? i : end - 1u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (c0 + (uint32_t)(u * kFT + tid) < end) atomicAdd(&wtot[wv][(v[u] & (kCells - 1)) >> 8], 1u);
    }
}

__device__ __forceinline__ void split_count_segment(const TileP &q, uint32_t seg, uint32_t (*wtot)[kFW])
{
    const int tid = threadIdx.x, wv = tid >> 6;
    if (seg >= q.seg0[q.pairs]) return;
    const int g = pair_of_segment(q.seg0, q.pairs, seg);
    const uint32_t beg = q.base[g] + (seg - q.seg0[g]) * (uint32_t)kSplitSeg;
    const uint32_t end = q.base[g + 1] - beg < (uint32_t)kSplitSeg ? q.base[g + 1] : beg + kSplitSeg;
    if (tid < kFW * kFW) (&wtot[0][0])[tid] = 0u;
    __syncthreads();
    count_subtiles(q.rec, beg, end, wtot);
    __syncthreads();
    if (tid < kFW) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kFW; ++w) t += wtot[w][tid];
        q.segcnt[(long long)seg * kFW + tid] = t;
    }
}

// Inclusive prefix sums inside every row of 16 lanes (lane & 15 = sub-tile), in registers: the first four steps of wave_incl_scan.
// (As four __shfl_up + compare steps the compiler kept the four shuffle addresses in vector registers from the first scan to the
// last chunk's, and every step was a trip through LDS.)  All lanes must be active.
__device__ __forceinline__ uint32_t row16_incl_scan(uint32_t v)
{
    static_assert(kFW == 16, "one DPP row per set of sub-tile counters");
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); // row_shr:8
    return v;
}

// 4a. Tiles of ordinary size (at most kSplitWhole records): ONE workgroup per (sequence, tile) reorders the tile's
// records sub-tile-major, STABLY, in ONE pass over the list: every thread loads its (up to) 32 records at once -- all
// loads of the tile in flight together, the list is read once and stays in registers -- and takes one returning LDS
// atomic per record on a (sub-tile, batch) counter, batch = the 64 records of one wave-instruction: lanes of one
// instruction are served in lane order and the batches are numbered in stream order, so the ticket plus the prefix of the
// sub-tile's earlier batches is the record's stable slot.  (Until round 3 this kernel counted the sub-tiles in a first
// pass and then re-read the list in chunks of 8192: six dependent trips to memory per workgroup where this has one.)
constexpr int kWholeChunks = FRLW_WHOLE_SEGS;
constexpr int kWholeBatches = kWholeChunks * kSplitSeg / kWave; // 512 batches of 64 records
constexpr int kWholeRow = kWholeBatches + 1;                    // row stride of scnt: the 16 counters of one batch in 16 banks

// CM (chunk-major partition): the tile's list is not contiguous -- it is gathered from the tile's column of the directory
// (col_*), the 16 sub-tile lists go wherever the header's cursor says, and a skewed tile only books its space and its split
// segments here (kf_segcount_cm / kf_split_place<true> do the work: the segments are not known before this kernel runs).
template <bool CM>
__global__ __launch_bounds__(kFT) __attribute__((amdgpu_waves_per_eu(8, 8))) void kf_split_whole(TileP q, CmP cm, SeqTab S) // (64 VGPRs: two workgroups per CU)
{
    constexpr int RPT = kSplitSeg / kFT; // 8 records per thread and chunk of 8192
    constexpr int kBtGroup = 4;          // table entries (and record loads) a thread has in flight at a time in step 1
    // scnt [sub-tile][batch] tickets, then exclusive prefixes | stage: one chunk of records, sub-tile-major.  CM, while the
    // list is gathered (before either is used): the column L | D | the block address table (or the position index)
    // CM: the column lies over the STAGING area (+ a tail of its own), not over the counters: the counters are zeroed in front of
    // the gather and the tickets are taken as the gathered records arrive -- no barrier, no drained load queue in between
    constexpr int kColWords = 2 * kColMax + 1 + kSplitWhole / 32 + 1;
    constexpr int kPoolTail = CM && kColWords > kSplitSeg ? kColWords - kSplitSeg : 0;
    __shared__ __attribute__((aligned(16))) uint32_t pool[kFW * kWholeRow + kSplitSeg + kPoolTail];
    uint32_t *scnt = pool, *stage = pool + kFW * kWholeRow;
    __shared__ uint32_t wtot[kFW][kFW];        // segment counting (4b): [wavefront][sub-tile]
    __shared__ uint32_t vtot[kFW];             // records of every sub-tile
    __shared__ uint32_t vbeg[kFW][kFW];        // [wavefront]: every wavefront's own copy of the sub-tile starts
    __shared__ uint32_t cE[kFW][kFW], cD[kFW][kFW]; // [wavefront]: per chunk, see step 4
    __shared__ uint32_t s_start, s_first;
    __shared__ int s_unsorted;
    __shared__ int s_fw[kWholeChunks][kFW], s_lw[kWholeChunks][kFW]; // (CM, TAF) first / last window of every sub-tile list inside every chunk, -1: no record
    __shared__ uint32_t s_wst[CM ? kFW * (FRLW_MAX_WINDOWS + 1) : 1];  // (CM, TAF) the tile's rows of TileP::wst while they are made
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // (CM: the status is REQUESTED here and tested behind the directory column -- a test in front of it made the column's load
    // wait for the header's round trip; the directory lies at addresses the plan fixes, reading it is safe whatever the status)
    const int32_t status0 = q.hdr->status;
    if (!CM && status0 != 0) return;
    const int blk = (int)blockIdx.x;
    if (!CM && blk >= q.pairs) { // the blocks behind the tiles: one segment of a skewed tile each (4b, counting)
        const uint32_t nseg = q.seg0[q.pairs];
        for (uint32_t seg = (uint32_t)(blk - q.pairs); seg < nseg; seg += (uint32_t)q.seg_grid) {
            split_count_segment(q, seg, wtot);
            __syncthreads(); // wtot is reused
        }
        return;
    }
    // CM: the tile comes from the XCD mapping -- tiles g and g + 1 share the cache lines at the ends of their runs in every
    // chunk's stretch of rec[] (a run is ~43 records at an arbitrary offset on the headline: 2.3 lines for 1.3 lines' worth of
    // records), and neighbouring BLOCKS sit on different L2s.  Everything below is keyed by g, never by the block.
    const int g = CM ? (int)xcd_owned_index(blockIdx.x, gridDim.x) : blk;
    PPROF_INIT(); // (developer timeline, -DFRLW_SPLIT_PROF: the stamps are listed in taf_partition.h)
    uint32_t beg = 0u, n;
    uint32_t m[kWholeChunks][RPT];
    if (CM) {
        const int s = g / q.T, C = S.chunk0[s + 1] - S.chunk0[s];
        // The usual call (a sequence of at most kBtCols chunks, fewer than 2^28 records): L | D | the block address table
        // (taf_blocktab.h) in 24 KB of the staging area; otherwise the column at its full length and the position index behind it
        const bool tabled = C <= frlw_bt::kBtCols && S.ev0[S.n_seq] - S.ev0[0] < (1ll << 28); // (kernel argument: uniform)
        static_assert(2 * frlw_bt::kBtCols + 2 + kSplitWhole / 16 * 2 <= kSplitSeg, "column + table inside the staging area");
        uint32_t *colL = stage, *colD = stage + (tabled ? frlw_bt::kBtCols : kColMax) + 1;
        uint16_t *idx = (uint16_t *)(stage + 2 * kColMax + 1);
        frlw_bt::BtEntry *tab = (frlw_bt::BtEntry *)(stage + 2 * frlw_bt::kBtCols + 2); // (8-byte aligned: stage is, at 16)
        for (int i = tid; i < kFW * kWholeRow; i += kFT) scnt[i] = 0u; // (published by the barriers of col_load)
        // (readfirstlane: the workgroup-uniform values that come out of LDS are uniform for the COMPILER too -- as vector values
        // they turned every "is this chunk of the list there at all" test below into divergent control flow, and 19 of the 32
        // records were spilled)
        n = col_load<kFT>(cm, S, s, g - s * q.T, colL, colD, &wtot[0][0]);
        PPROF(0);
        if (status0 != 0) return;
        if (n == 0u) {
            if (tid < kFW) { q.sub[(long long)g * kFW + tid] = 0u; q.sub_end[(long long)g * kFW + tid] = 0u; }
            if (q.wst && tid == 0) q.wst_flag[g] = 0u; // (empty lists: the walk's scan finds nothing to read)
            return;
        }
        const bool hot = n > q.tile_max;
        // The tile's 16 lists: n records of rec2[] from `start` on.  The add is ISSUED here, so that its trip to the header overlaps
        // the table build and the gather, but an ordinary tile does not wait for it here: every workgroup of the launch books on this
        // one word at about the same moment (they queue there), and a wait in front of the barrier below kept the other fifteen
        // wavefronts -- and the tile's gather -- behind thread 0's place in that queue.  The value stays in thread 0's register
        // until the last gather address is out and is published by the barrier behind the tickets.
        uint32_t start = 0u;
        if (tid == 0) {
            // (an offset of zero through a vector register: with a uniform address the compiler folds the add over the wavefront's
            // active lanes and reads the sum back with a readfirstlane right here -- which is a wait for the returning add, right here)
            uint32_t zero = 0u;
            asm volatile("" : "+v"(zero));
            start = atomicAdd(&q.hdr->rec_cursor + zero, n);
            if (hot) { // (needs both values at once: the wait stays here)
                s_start = start;
                s_first = atomicAdd(&q.hdr->seg_cursor, (n + kSplitSeg - 1) / kSplitSeg);
                if (q.wst) q.wst_flag[g] = 0u; // (the segment kernels place this tile: no table)
            }
            s_unsorted = 0;
        }
        if (q.wst && !hot) { // the tile's rows of the window table start at "no record" (published by the barriers below)
            if (tid < kWholeChunks * kFW) { (&s_fw[0][0])[tid] = -1; (&s_lw[0][0])[tid] = -1; }
            for (int i = tid; i < kFW * (q.n_windows + 1); i += kFT) s_wst[i] = 0xffffffffu;
        }
        if (hot) { // a skewed tile (or a call with few tiles): cut into segments of 8192 list positions, one workgroup each
            __syncthreads();
            const uint32_t nseg = (n + kSplitSeg - 1) / kSplitSeg, first = s_first;
            if (tid == 0) { cm.hot_start[g] = s_start; cm.hot_seg0[g] = first; }
            for (uint32_t k = tid; k < nseg; k += kFT)
                if (first + k < (uint32_t)cm.max_segs) cm.segdesc[first + k] = (uint32_t)g;
            return;
        }
        if (tabled) {
            for (int c = tid; c < C; c += kFT) frlw_bt::bt_build_run(colL, colD, C, c, n, tab);
        } else {
            col_index<kFT>(colL, C, 0u, n, idx);
        }
        __syncthreads();
        PPROF(2);
        const uint32_t wvs = (uint32_t)__builtin_amdgcn_readfirstlane(wv); // (the wavefront index as a scalar: uniform branches below)
        // 1. the whole list into registers: list position -> address through the block table (without one: chunk through the index + a
        // walk over at most a few run boundaries); the loads go through one buffer descriptor with 32-bit offsets: with 64-bit
        // addresses next to the 32 records the compiler spilled 19 of them, each spill waiting for its load
        {
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)cm.rec, 0, 0xffffffffu, 0x00020000);
            // (a staging chunk the list does not reach issues no load at all -- a 22 000-record tile has three of the four; its m[c][.]
            // stay unset and unread: every later step tests the same bound)
            if (tabled) {
#pragma unroll
                for (int c = 0; c < kWholeChunks; ++c) {
                    if ((uint32_t)(c * kSplitSeg) >= n) break; // workgroup-uniform
                    // one 8-byte entry per 16 positions: no index, no walk (and no scalar search for a single run either: that is two
                    // dependent LDS trips per wave-instruction where this is one read).  Four entries are read together, then their
                    // four loads go out; lanes behind the list's end take its last record's entry (clamped: it exists)
#pragma unroll
                    for (int u0 = 0; u0 < RPT; u0 += kBtGroup) {
                        frlw_bt::BtEntry e[kBtGroup];
                        uint32_t ic[kBtGroup], wmax = 0u;
#pragma unroll
                        for (int k = 0; k < kBtGroup; ++k) {
                            const uint32_t i = (uint32_t)(c * kSplitSeg + (u0 + k) * kFT + tid);
                            ic[k] = i < n ? i : n - 1u;
                            e[k] = tab[ic[k] >> 4];
                        }
#pragma unroll
                        for (int k = 0; k < kBtGroup; ++k) wmax = e[k].w > wmax ? e[k].w : wmax;
                        if (__builtin_expect(__ballot(wmax == frlw_bt::kBtFallback) == 0ull, 1)) {
#pragma unroll
                            for (int k = 0; k < kBtGroup; ++k)
                                m[c][u0 + k] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)(frlw_bt::bt_addr(e[k], ic[k]) << 2), 0, 0);
                        } else { // a block with two run boundaries (runs shorter than 16 records, a skewed neighbour): those lanes walk the column
#pragma unroll
                            for (int k = 0; k < kBtGroup; ++k) {
                                const uint32_t off = e[k].w == frlw_bt::kBtFallback ? frlw_bt::bt_walk(colL, colD, e[k].a, ic[k]) : frlw_bt::bt_addr(e[k], ic[k]);
                                m[c][u0 + k] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)(off << 2), 0, 0);
                            }
                        }
                    }
                }
            } else {
#pragma unroll
            for (int c = 0; c < kWholeChunks; ++c) {
                if ((uint32_t)(c * kSplitSeg) >= n) break; // workgroup-uniform
#pragma unroll
                for (int u = 0; u < RPT; ++u) {
                    const uint32_t i = (uint32_t)(c * kSplitSeg + u * kFT + tid), ic = i < n ? i : n - 1u;
                    // the wavefront's 64 positions i0 .. i0 + 63: mostly inside ONE run when the runs are long (64 sequences of
                    // 1 M events: 226 records per run) -- then the run is found once, with scalar compares, and a lane only adds
                    const uint32_t i0 = (uint32_t)(c * kSplitSeg + u * kFT) + wvs * kWave;
                    uint32_t off = 0u;
                    if (i0 < n) { // wave-uniform
                        const uint32_t last = i0 + 63u < n ? i0 + 63u : n - 1u;
                        uint32_t cs = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx[i0 >> 4]);
                        uint32_t lnext = (uint32_t)__builtin_amdgcn_readfirstlane((int)colL[cs + 1]);
                        while (lnext <= i0) { ++cs; lnext = (uint32_t)__builtin_amdgcn_readfirstlane((int)colL[cs + 1]); }
                        if (lnext > last) off = (uint32_t)__builtin_amdgcn_readfirstlane((int)colD[cs]) + ic;
                        else off = col_addr(colL, colD, idx[ic >> 4], ic);
                    }
                    m[c][u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)(off << 2), 0, 0);
                }
            }
            // This form's records are waited for HERE (s_waitcnt vmcnt(0)), not by its tickets.  Both forms hold divergent loops, so
            // the compiler chains them -- this one, then the table form, each skipped by a flag -- and places its waits for a register
            // as if a workgroup could run both: the table form's first loads waited for loads only THIS form issues into the same
            // registers -- in effect for everything their wavefront had in flight: three of its first four records (one memory round
            // trip in every gather) and thread 0's returning add.  Drained here, this form leaves nothing to wait for.  Its own
            // tickets lose next to nothing: the first of them waited for all but seven of the records anyway.
            __builtin_amdgcn_s_waitcnt(0x0F70); // (vmcnt(0), expcnt and lgkmcnt left alone)
            }
        }
        // The last gather address is out: thread 0's wavefront waits for the add here, the other fifteen do not -- and they all wait
        // for their records next, which were requested behind the add and come back behind it.  (The empty asm: the compiler waits
        // for a value where it is first used, and would move this store up to the add.)
        PPROF(3);
        PPROF_CURSOR(n);
        PPROF(1);
        if (tid == 0) { asm volatile("" : "+v"(start)); s_start = start; }
        // (the column is dead once the last address is out; its space is written again in step 4, three barriers from here)
    } else {
        beg = q.base[g];
        const uint32_t end = q.base[g + 1];
        if (g == q.pairs - 1 && tid == 0) q.sub[(long long)q.pairs * kFW] = end; // end of the last sub-tile's list
        if (end - beg > whole_max_of(q.pairs)) return; // a skewed tile (or a call with few tiles): left to the segment kernels below
        n = end - beg;
        if (n == 0u) {
            if (tid < kFW) q.sub[(long long)g * kFW + tid] = beg;
            return;
        }
        // 1. the whole list into registers (indices clamped: no load sits under a lane condition)
#pragma unroll
        for (int c = 0; c < kWholeChunks; ++c)
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const uint32_t i = (uint32_t)(c * kSplitSeg + u * kFT + tid);
                m[c][u] = q.rec[beg + (i < n ? i : n - 1u)];
            }
    }
    if (!CM) {
        for (int i = tid; i < kFW * kWholeRow; i += kFT) scnt[i] = 0u;
        __syncthreads();
    }
    // 2. tickets: batch (c, u, wv) of the stream, counter [sub-tile][batch]; packed four to a register (a ticket is < 64)
    uint32_t rk[kWholeChunks][RPT / 4];
#pragma unroll
    for (int c = 0; c < kWholeChunks; ++c) {
#pragma unroll
        for (int u4 = 0; u4 < RPT / 4; ++u4) rk[c][u4] = 0u;
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const uint32_t i0 = (uint32_t)(c * kSplitSeg + u * kFT + wv * kWave); // first record of the batch: wave-uniform
            if (i0 < n) {
                const bool valid = i0 + (uint32_t)lane < n;
                const uint32_t b = valid ? (m[c][u] & (kCells - 1)) >> 8 : (uint32_t)(lane & 15); // (lanes behind the end add 0, spread over the counters)
                const uint32_t t = atomicAdd(&scnt[b * kWholeRow + (c * RPT + u) * kFW + wv], valid ? 1u : 0u);
                rk[c][u >> 2] |= t << (8 * (u & 3));
            }
        }
    }
    if (CM) PPROF(4);
    __syncthreads();
    // 3. wavefront b: exclusive prefix of sub-tile b's batch counts in stream order (eight scans of 64 batches)
    {
        uint32_t carry = 0;
#pragma unroll
        for (int k = 0; k < kWholeBatches / kWave; ++k) {
            if ((uint32_t)(k * kWave * kWave) < n) { // (batches behind the end of the list hold zeros)
                const uint32_t v = scnt[wv * kWholeRow + k * kWave + lane];
                const uint32_t inc = wave_incl_scan(v);
                scnt[wv * kWholeRow + k * kWave + lane] = carry + inc - v;
                carry += __shfl(inc, kWave - 1);
            }
        }
        if (lane == 0) vtot[wv] = carry;
    }
    __syncthreads();
    if (CM) PPROF(5);
    if (CM) beg = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_start); // (published two barriers ago, behind the tickets)
    {
        // every wavefront: where the 16 lists start (its own copy: no further barrier)
        const uint32_t t = vtot[lane & 15];
        const uint32_t inc = row16_incl_scan(t);
        if (lane < kFW) {
            vbeg[wv][lane] = beg + inc - t;
            if (wv == 0) {
                q.sub[(long long)g * kFW + lane] = beg + inc - t;
                if (CM) q.sub_end[(long long)g * kFW + lane] = beg + inc;
            }
        }
        LDS_FENCE();
    }
    // 4. records to their slots, chunk by chunk THROUGH LDS: the 8192 records of a chunk are laid out sub-tile-major in the
    // staging area (slot = the chunk's records of lower sub-tiles + the record's rank inside the chunk), then leave in one
    // linear sweep -- consecutive threads write consecutive records of a sub-tile's run (whole lines; the direct form wrote
    // 64 records of one instruction to 16 lists, ~16 bytes per line touched: 61 MB of write traffic for 40 MB of records).
    // Per chunk and sub-tile b (every wavefront keeps its own copy, no barrier for the tables):
    //   cE[b] = (records of sub-tiles < b in the chunk) - (prefix of b at the chunk's first batch)   -> slot = cE[b] + prefix + ticket
    //   cD[b] = (start of b's list) + (prefix of b at the chunk's first batch) - (records of sub-tiles < b)  -> address = cD[b] + slot
    const bool wtab = CM && q.wst != nullptr; // (kernel-uniform)
#pragma unroll
    for (int c = 0; c < kWholeChunks; ++c) {
        if ((uint32_t)(c * kSplitSeg) >= n) break; // workgroup-uniform
        const uint32_t nch = n - (uint32_t)(c * kSplitSeg) < (uint32_t)kSplitSeg ? n - (uint32_t)(c * kSplitSeg) : (uint32_t)kSplitSeg;
        {
            const int b = lane & 15;
            const uint32_t p0 = scnt[b * kWholeRow + c * (kSplitSeg / kWave)];
            const uint32_t p1 = (uint32_t)((c + 1) * kSplitSeg) < n ? scnt[b * kWholeRow + (c + 1) * (kSplitSeg / kWave)] : vtot[b];
            const uint32_t cnt = p1 - p0;
            const uint32_t inc = row16_incl_scan(cnt);
            if (lane < kFW) {
                cE[wv][lane] = (inc - cnt) - p0;
                cD[wv][lane] = vbeg[wv][lane] + p0 - (inc - cnt);
            }
            LDS_FENCE();
        }
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const uint32_t i = (uint32_t)(u * kFT + tid);
            if (i < nch) {
                const uint32_t b = (m[c][u] & (kCells - 1)) >> 8;
                const uint32_t t = (rk[c][u >> 2] >> (8 * (u & 3))) & 255u;
                stage[cE[wv][b] + scnt[b * kWholeRow + (c * RPT + u) * kFW + wv] + t] = m[c][u];
            }
        }
        __syncthreads();
        if (CM) PPROF(6);
        // (CM, TAF) the window starts kf_taf_walk needs, so that it does not have to scan its list for them.  The staged chunk is
        // sub-tile-major and stable: neighbours of one sub-tile are neighbours of that sub-tile's LIST.  A record whose sub-tile or
        // window differs from its staged predecessor's (and the chunk's first record) is a candidate for "first record of its
        // window in its list": the minimum list position over the candidates IS that record (a candidate that is no true start --
        // the first record of a sub-tile in a later chunk -- has an earlier record of its window in front of it, a candidate
        // too), taken with one LDS atomicMin -- a handful per chunk; two LDS reads + four instructions per record otherwise.
#pragma unroll
        for (int u = 0; u < RPT; ++u) {
            const uint32_t i = (uint32_t)(u * kFT + tid);
            if (i < nch) {
                const uint32_t r = stage[i];
                q.rec2[cD[wv][(r & (kCells - 1)) >> 8] + i] = r;
            }
        }
        if (wtab) { // (a pass of its own: a branch per record inside the sweep above kept its LDS reads from being issued together)
            const uint32_t dmask = (((1u << q.wb) - 1u) << kCellBits) | (uint32_t)(kCells - 1) >> 8 << 8;
            uint32_t cand = 0u; // bit u: record u * 1024 + tid of the chunk is a candidate
#pragma unroll
            for (int u0 = 0; u0 < RPT; u0 += 2) { // two records' reads issued together (clamped indices; the empty asm keeps the
                uint32_t r[2], rp[2];               // compiler from putting each read under its own `i < nch` branch, one LDS round trip each;
#pragma unroll                                      // four at a time spilled five of the later chunks' records)
                for (int k = 0; k < 2; ++k) {
                    const uint32_t i = (uint32_t)((u0 + k) * kFT + tid);
                    r[k] = stage[i];                            // (i < 8192: inside the staging area whatever nch is; what lies
                    rp[k] = stage[(i - 1u) & (kSplitSeg - 1)];  // behind the chunk's end, or in front of record 0, is masked below)
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) asm volatile("" : "+v"(r[k]), "+v"(rp[k]));
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const uint32_t i = (uint32_t)((u0 + k) * kFT + tid);
                    cand |= (i < nch && (((r[k] ^ rp[k]) & dmask) != 0u || i == 0u || i == nch - 1u) ? 1u : 0u) << (u0 + k);
                }
            }
            while (cand) { // rare: a handful of records per chunk
                const int u = __builtin_ctz(cand);
                cand &= cand - 1u;
                const uint32_t i = (uint32_t)(u * kFT + tid);
                const uint32_t r = stage[i], rp = stage[i > 0u ? i - 1u : 0u];
                const int bsub = (int)((r & (kCells - 1)) >> 8), bp = (int)((rp & (kCells - 1)) >> 8);
                const int wc = (int)__builtin_amdgcn_ubfe(r, kCellBits, q.wb), wpn = (int)__builtin_amdgcn_ubfe(rp, kCellBits, q.wb);
                const bool same = i > 0u && bp == bsub; // the staged predecessor is the list predecessor
                // (an LDS atomic: global ones sat in front of every chunk's barrier, which waits for the memory queue to drain)
                if (!same || wc != wpn) atomicMin(&s_wst[bsub * (q.n_windows + 1) + wc], cD[wv][bsub] + i - vbeg[wv][bsub]);
                if (same && wc < wpn) s_unsorted = 1;
                if (!same) { s_fw[c][bsub] = wc; if (i > 0u) s_lw[c][bp] = wpn; } // first window of list bsub / last of list bp in this chunk
                if (i == nch - 1u) s_lw[c][bsub] = wc;
            }
        }
        // the staging area is reused by the next chunk; behind the LAST chunk only step 5 follows, which touches LDS alone: a raw
        // barrier there (a __syncthreads() would make the workgroup wait for the drain of its last 32 KB of stores)
        if (wtab && (uint32_t)((c + 1) * kSplitSeg) >= n) LDS_BARRIER();
        else __syncthreads();
        if (CM) PPROF(7);
    }
    // 5. (CM, TAF) a window index that DEcreases between list neighbours marks the tile unsorted (the walk then filters the whole
    // list per window, as it does after its own scan): inside a chunk the sweep saw it at the neighbour; across chunks it is the
    // list's last window in one chunk against its first in the next one that has any.
    if (wtab) {
        if (tid < kFW) {
            int prev = -1;
            for (int c = 0; c < kWholeChunks; ++c)
                if (s_fw[c][tid] >= 0) { if (s_fw[c][tid] < prev) s_unsorted = 1; prev = s_lw[c][tid]; }
        }
        uint32_t *const wr = q.wst + (long long)g * kFW * (q.n_windows + 1);
        for (int i = tid; i < kFW * (q.n_windows + 1); i += kFT) wr[i] = s_wst[i];
        LDS_BARRIER();
        if (tid == 0) q.wst_flag[g] = s_unsorted ? 2u : 1u;
    }
    if (CM) { PPROF(8); PPROF_END(); }
}

// 4b. Skewed tiles (more than kSplitWhole records).  Reorders every tile's records sub-tile-major (sub-tile = the 256 cells [256 v, 256 v + 256) one workgroup of
// kf_taf_walk owns), STABLY, so that every sub-tile's list is still in stream order.  A tile's list is cut into segments
// of 8192 records, one workgroup each -- a tile that holds a large share of the stream (skew) is split by hundreds of
// workgroups instead of one:
//   kf_split_count    records of every sub-tile in the segment
//   kf_split_offsets  one 16-lane group per tile: running sums over its segments -> where each segment's records of
//                     sub-tile v go inside v's list, and where v's list starts (sub[])
//   kf_split_place    ranks inside the segment with one returning LDS atomic per record on (round, wavefront, sub-tile)
//                     counters: lanes of one instruction are served in lane order, (round, wavefront) is the stream
//                     order of the 64-record batches.
constexpr int kSplitRpt = kSplitSeg / kFT;
struct PlaceLds {
    uint32_t scnt[kSplitRpt][kFW][kFW]; // [round][wavefront][sub-tile] tickets, then prefixes inside the segment
    uint32_t vtot[kFW];                 // records of every sub-tile in the whole tile
    uint32_t stot[kFW], sdst[kFW];      // this segment: records of sub-tile b / where they go in b's list
    uint32_t cE[kFW][kFW], cD[kFW][kFW]; // [wavefront]: slot = cE[b] + prefix + ticket, address = cD[b] + slot (as in kf_split_whole)
    uint32_t stage[kSplitSeg];          // the segment's records, sub-tile-major
};

// CM: the chunk-major partition's form -- the segment is 8192 positions of the tile's list, gathered through the tile's column
// of the directory (cl: L | D | position index, loaded per segment); the tile's space and segment ids were booked by
// kf_split_whole<true>.
struct ColLds {
    uint32_t L[kColMax + 1], D[kColMax];
    uint16_t idx[kSplitSeg / 16];
    uint32_t wsum[kFW + 1];
};

template <bool CM>
__device__ __forceinline__ void split_place_segment(const TileP &q, uint32_t seg, PlaceLds &L, const CmP &cm, const SeqTab &S, ColLds *cl)
{
    constexpr int RPT = kSplitRpt, NE = RPT * kFW;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int g;
    uint32_t beg, nrec, seg_first, seg_last, tile_start;
    if (CM) {
        g = __builtin_amdgcn_readfirstlane((int)cm.segdesc[seg]);
        const int s = g / q.T;
        const uint32_t n = col_load<kFT>(cm, S, s, g - s * q.T, cl->L, cl->D, cl->wsum);
        seg_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)cm.hot_seg0[g]);
        seg_last = seg_first + (n + kSplitSeg - 1) / kSplitSeg;
        beg = (seg - seg_first) * (uint32_t)kSplitSeg; // a list position
        nrec = n - beg < (uint32_t)kSplitSeg ? n - beg : (uint32_t)kSplitSeg;
        tile_start = (uint32_t)__builtin_amdgcn_readfirstlane((int)cm.hot_start[g]);
        col_index<kFT>(cl->L, S.chunk0[s + 1] - S.chunk0[s], beg, beg + nrec, cl->idx);
    } else {
        g = pair_of_segment(q.seg0, q.pairs, seg);
        beg = q.base[g] + (seg - q.seg0[g]) * (uint32_t)kSplitSeg;
        const uint32_t end = q.base[g + 1] - beg < (uint32_t)kSplitSeg ? q.base[g + 1] : beg + kSplitSeg;
        nrec = end - beg;
        seg_first = q.seg0[g];
        seg_last = q.seg0[g + 1];
        tile_start = q.base[g];
    }
    for (int i = tid; i < RPT * kFW * kFW; i += kFT) (&L.scnt[0][0][0])[i] = 0u;
    // where this segment's records of sub-tile v (= this wavefront) go: v's list starts behind the lists of the
    // sub-tiles before it, and the earlier segments of the tile come first inside it.  Every workgroup adds up the
    // tile's segment counts for itself (<= a few hundred segments x 16 values, L2-resident).
    uint32_t before = 0, total = 0;
    for (uint32_t sg = seg_first + lane; sg < seg_last; sg += kWave) {
        const uint32_t c = q.segcnt[(long long)sg * kFW + wv];
        total += c;
        if (sg < seg) before += c;
    }
#pragma unroll
    for (int o2 = 32; o2 >= 1; o2 >>= 1) { before += __shfl_xor(before, o2); total += __shfl_xor(total, o2); }
    if (lane == 0) L.vtot[wv] = total;
    __syncthreads(); // (CM: also orders col_index's writes before the reads below)
    uint32_t vstart = tile_start;
    for (int k = 0; k < wv; ++k) vstart += L.vtot[k];
    if (seg == seg_first && lane == 0) { // the tile's first segment publishes sub[]
        q.sub[(long long)g * kFW + wv] = vstart;
        if (CM) q.sub_end[(long long)g * kFW + wv] = vstart + total;
    }
    uint32_t m[RPT], rk[RPT];
    const uint32_t wvs = (uint32_t)__builtin_amdgcn_readfirstlane(wv);
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        const uint32_t i = (uint32_t)(u * kFT + tid);
        if (CM) {
            const uint32_t ic = i < nrec ? i : nrec - 1u; // (nrec >= 1: a segment is never empty)
            const uint32_t v = cm.rec[col_addr_wave(cl->L, cl->D, cl->idx, beg, (uint32_t)(u * kFT) + wvs * kWave, ic, nrec)];
            m[u] = i < nrec ? v : 0u;
        } else {
            m[u] = i < nrec ? q.rec[beg + i] : 0u;
        }
    }
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        const uint32_t i = (uint32_t)(u * kFT + tid);
        rk[u] = 0u;
        if (i < nrec) rk[u] = atomicAdd(&L.scnt[u][wv][(m[u] & (kCells - 1)) >> 8], 1u);
    }
    __syncthreads();
    {
        // wavefront b: exclusive prefix of sub-tile b's counts over (round, wavefront) = stream order inside the segment
        uint32_t v0 = 0, v1 = 0;
        const int e0 = 2 * lane, e1 = 2 * lane + 1;
        if (e0 < NE) v0 = L.scnt[e0 / kFW][e0 % kFW][wv];
        if (e1 < NE) v1 = L.scnt[e1 / kFW][e1 % kFW][wv];
        const uint32_t inc = wave_incl_scan(v0 + v1);
        const uint32_t ex = inc - (v0 + v1);
        if (e0 < NE) L.scnt[e0 / kFW][e0 % kFW][wv] = ex;
        if (e1 < NE) L.scnt[e1 / kFW][e1 % kFW][wv] = ex + v0;
        if (lane == kWave - 1) { L.stot[wv] = inc; L.sdst[wv] = vstart + before; }
    }
    __syncthreads();
    {
        // every wavefront for itself: the segment's records sub-tile-major in the staging area (see kf_split_whole, step 4)
        const int b = lane & 15;
        const uint32_t cnt = L.stot[b];
        uint32_t inc = cnt;
#pragma unroll
        for (int o2 = 1; o2 < kFW; o2 <<= 1) {
            const uint32_t u = __shfl_up(inc, o2);
            if (b >= o2) inc += u;
        }
        if (lane < kFW) { L.cE[wv][lane] = inc - cnt; L.cD[wv][lane] = L.sdst[lane] - (inc - cnt); }
        LDS_FENCE();
    }
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
        const uint32_t i = (uint32_t)(u * kFT + tid);
        if (i < nrec) {
            const uint32_t b = (m[u] & (kCells - 1)) >> 8;
            L.stage[L.cE[wv][b] + L.scnt[u][wv][b] + rk[u]] = m[u];
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < RPT; ++u) { // linear sweep: consecutive threads write consecutive records of a sub-tile's run
        const uint32_t i = (uint32_t)(u * kFT + tid);
        if (i < nrec) {
            const uint32_t r = L.stage[i];
            q.rec2[L.cD[wv][(r & (kCells - 1)) >> 8] + i] = r;
        }
    }
}

template <bool CM>
__global__ __launch_bounds__(kFT) __attribute__((amdgpu_waves_per_eu(8, 8))) void kf_split_place(TileP q, CmP cm, SeqTab S)
{
    __shared__ PlaceLds L;
    __shared__ typename std::conditional<CM, ColLds, uint32_t>::type clmem; // the column: only the chunk-major form has one
    ColLds *cl = reinterpret_cast<ColLds *>(&clmem);
    if (q.hdr->status != 0) return;
    uint32_t nseg = CM ? q.hdr->seg_cursor : q.seg0[q.pairs];
    if (CM && nseg > (uint32_t)cm.max_segs) nseg = (uint32_t)cm.max_segs;
    // (the segment from the block index, NOT through xcd_owned_index: a skewed call has fewer segments than workgroups (a few hundred of 512 with a
    // quarter of 10 M events in one blob), and the mapping would hand them all to the first XCDs and leave the others idle)
    for (uint32_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) { // (workgroup-uniform: most calls have no segment at all)
        split_place_segment<CM>(q, seg, L, cm, S, cl);
        __syncthreads(); // the LDS image is reused
    }
}

// chunk-major partition: records of every sub-tile in every split segment (kf_split_whole<false> does this in its spare
// workgroups; here the segments only exist once kf_split_whole<true> has run).  Most calls have none: the workgroups leave
// after one load.
__global__ __launch_bounds__(kFT) __attribute__((amdgpu_waves_per_eu(8, 8))) void kf_segcount_cm(TileP q, CmP cm, SeqTab S) // (64 VGPRs: two workgroups per CU)
{
    __shared__ ColLds cl;
    __shared__ uint32_t wtot[kFW][kFW];
    const int tid = threadIdx.x, wv = tid >> 6;
    if (q.hdr->status != 0) return;
    uint32_t nseg = q.hdr->seg_cursor;
    if (nseg > (uint32_t)cm.max_segs) nseg = (uint32_t)cm.max_segs;
    for (uint32_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) { // (not through xcd_owned_index: see kf_split_place)
        const int g = __builtin_amdgcn_readfirstlane((int)cm.segdesc[seg]), s = g / q.T;
        const uint32_t n = col_load<kFT>(cm, S, s, g - s * q.T, cl.L, cl.D, cl.wsum);
        const uint32_t beg = (seg - (uint32_t)__builtin_amdgcn_readfirstlane((int)cm.hot_seg0[g])) * (uint32_t)kSplitSeg;
        const uint32_t nrec = n - beg < (uint32_t)kSplitSeg ? n - beg : (uint32_t)kSplitSeg;
        col_index<kFT>(cl.L, S.chunk0[s + 1] - S.chunk0[s], beg, beg + nrec, cl.idx);
        if (tid < kFW * kFW) (&wtot[0][0])[tid] = 0u;
        __syncthreads();
        uint32_t v[kSplitRpt];
        const uint32_t wvs = (uint32_t)__builtin_amdgcn_readfirstlane(wv);
#pragma unroll
        for (int u = 0; u < kSplitRpt; ++u) {
            const uint32_t i = (uint32_t)(u * kFT + tid), ic = i < nrec ? i : nrec - 1u;
            v[u] = cm.rec[col_addr_wave(cl.L, cl.D, cl.idx, beg, (uint32_t)(u * kFT) + wvs * kWave, ic, nrec)];
        }
#pragma unroll
        for (int u = 0; u < kSplitRpt; ++u)
            if ((uint32_t)(u * kFT + tid) < nrec) atomicAdd(&wtot[wv][(v[u] & (kCells - 1)) >> 8], 1u);
        __syncthreads();
        if (tid < kFW) {
            uint32_t t = 0;
#pragma unroll
            for (int w = 0; w < kFW; ++w) t += wtot[w][tid];
            q.segcnt[(long long)seg * kFW + tid] = t;
        }
        __syncthreads(); // the column and wtot are reused
    }
}
} // namespace
