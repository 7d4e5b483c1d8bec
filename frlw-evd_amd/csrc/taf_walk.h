// taf_walk.h -- kf_taf_walk: one workgroup per sub-tile list, a window per wavefront, then the FIFO steps.
// Expects taf_split.h (TileP), taf_fifo.h (fifo_step, fifo_mean, kMaxK), taf_mean.h (mean_by_recip, kMeanTab) and taf_column.h; the leaky table
// (kLeakyTableWords, leaky.h).
#pragma once
#include "taf_fifo.h"
#include "taf_mean.h"
#include "taf_split.h"

namespace {
// The same step for K = 8 with TWO lanes per cell: the even lane holds slots 0..3, the odd lane slots 4..7 of the row
// (the whole workgroup works in phase 2, and a lane moves 16 bytes of the row).  Slot 3 takes over slot 4 from the
// partner lane through a DPP row shift; the float operations per slot are those of fifo_step.
__device__ __forceinline__ void fifo_step_half(float (&st)[4], bool upper, bool has, uint32_t n, float mean)
{
    const bool hit = n != 0u;
    const float up = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, st[0]), 0x101, 0xf, 0xf, false)); // row_shl:1: lane l reads lane l + 1
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float nxt = k < 3 ? st[k + 1] : (upper ? 0.0f : up);
        const float v = (hit ? nxt : st[k]) - 1.0f;
        const float nv = (hit && upper && k == 3) ? mean : v;
        st[k] = has ? nv : st[k];
    }
}

// 5. One workgroup of eight wavefronts per (sequence, tile, sub-tile of 256 cells).  The per-window sums of a cell do
// not depend on each other -- only the FIFO steps that consume them are sequential -- so the eight wavefronts take ONE
// WINDOW EACH (rounds of eight windows) and the FIFO steps follow with one cell per lane:
//   phase 0  the list is scanned once for the first record of every window (the split is stable: a time-sorted stream
//            gives a window-sorted list; a window that runs backwards switches the whole sub-tile to the general mode,
//            where every wavefront sweeps the whole list for its window's records);
//   phase 1  wavefront w, passes of up to 256 records of its window:
//              1. every record takes a ticket from its cell's LDS counter with one returning atomic (two 16-bit
//                 counters per word): lanes of one instruction are served in lane order and the four instructions of a
//                 pass are in stream order, so the ticket is the record's stream rank inside its cell -- a STABLE
//                 counting sort without any ordering pass;
//              2. the lanes read the counts of their four cells, a wavefront scan turns them into segment offsets;
//              3. every record's f32 value goes to sorted[offset of its cell + ticket];
//              4. every lane adds its cells' segments front to back into registers: the reference's sequential
//                 `sum += t - 1` (generate_taf.py:25-26);
//            then (sum, count) of the 256 cells go to LDS;
//   phase 2  lane c of the first four wavefronts owns cell c: K-deep FIFO row in registers (consecutive lanes hold
//            consecutive 32-byte rows of the (H, W, 2, K) state: whole lines), the round's means sum / (n + 1e-8) by a table
//            reciprocal and two FMAs (taf_mean.h; by division where the wavefront holds a count of 64 or more), one FIFO step
//            per window in order (generate_taf.py:27-49), skipped for windows that are empty in the whole sequence (:40-41).
// (ds_add_f32 would do the ordered sum in one instruction -- it applies same-address lanes in lane order with v_add_f32
// rounding, checked by the self-test in taf_fast.hip -- but runs at 192 cycles per wave-instruction per CU: measured, not used.)
constexpr int kWalkWaves = 8;
constexpr int kWalkThreads = kWalkWaves * kWave;
constexpr int kWalkRpt = 4;                 // records per lane and pass
constexpr int kWalkChunk = kWalkRpt * kWave;
constexpr int kWalkSlots = 4;               // ranks of a cell inside one pass that have a plane of their own
constexpr int kWalkWaveWords = kWalkSlots * kSubCells + kSubCells / 2; // LDS words per wavefront: the planes + the ticket counters
// (two 16-bit counters per word: 36 KB of planes and counters for the eight wavefronts -- FOUR workgroups per CU; with 32-bit
// counters the workgroup needs 41.3 KB, three fit, and the walk ran 8 % slower although it issued fewer instructions, measured)

// CMD (chunk-major partition, direct mode: the partition's bins ARE the sub-tiles): the sub-tile's list does not exist yet --
// its runs sit in the chunks' stretches of rec[].  The workgroup reads its column of the directory, books the list's space
// through the header's cursor, copies the runs there in chunk order (a pure copy: groups of 16 lanes take a run each) and then
// walks the contiguous list like any other; no gather kernel, no second launch.
constexpr int kWalkListCap = 3584; // records of a sub-tile's list kept in LDS by the CMD walk (14 KB: three workgroups per CU): no trip to memory between
                                   // the gather and the two sweeps over the list; longer lists are copied to rec2[]
template <bool K8, bool CMD = false>
__global__ __launch_bounds__(kWalkThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void kf_taf_walk(TileP q, CmP cm, SeqTab S)
{
    // per wavefront: kWalkSlots planes of 256 floats (plane r, cell c = the value of the cell's r-th record of the pass; +0 when
    // there is none) + 256 ticket counters.  The (sum, count) rows phase 2 reads lie over planes 0 and 1 of their wavefront;
    // the CMD column and the uint8 staging at the end lie over the whole area.
    __shared__ __attribute__((aligned(16))) uint32_t s_area[kWalkWaves][kWalkWaveWords];
    __shared__ uint32_t wstart[FRLW_MAX_WINDOWS + 1];
    __shared__ uint32_t thr[kLeakyTableWords]; // thresholds + bucket table of the leaky transform (leaky_u8_bucket_n)
    __shared__ float s_recip[kMeanTab]; // RN(1 / n) for the counts below kMeanTab ([0] = +0): the means of phase 2 (taf_mean.h)
    __shared__ int s_unsorted;
    __shared__ __attribute__((aligned(16))) uint32_t s_list[CMD ? kWalkListCap : 4]; // CMD: the gathered list, when it fits (else it goes to rec2[])
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // CMD: the sub-tile comes from the XCD mapping -- the short runs of neighbouring bins (a dozen records, several to a cache line,
    // in every chunk's stretch of rec[]) go through one L2.  The other forms read whole lists, which share next to nothing with
    // their neighbours (measured: same time), and keep the block index: the heavy sub-tiles of a hot spot stay spread over the XCDs.
    const int sg = CMD ? (int)xcd_owned_index(blockIdx.x, gridDim.x) : (int)blockIdx.x, g = sg / kFW, sub = sg - g * kFW;
    const int s = g / q.T, tile = g - s * q.T;
    // Everything the workgroup needs from the header and the list tables is requested in ONE go, in front of the status test:
    // each of these is a scalar load of its own round trip, and one behind a branch waits for the one in front of it.  (The
    // tables lie at addresses the plan fixes: reading them is safe whatever the status says; the LIST is only read behind it.)
    const int32_t status0 = q.hdr->status;
    const unsigned long long wmask = q.hdr->wmask[s];
    const uint32_t mul_bad0 = q.hdr->mul_bad;
    uint32_t beg = 0u, end = 0u;
    uint32_t wtab = 0u; // 1 / 2: kf_split_whole<true> has left this tile's window starts / found its list unsorted (TileP::wst_flag)
    uint32_t fw_row = 0xffffffffu; // this lane's entry of the list's row of TileP::wst (meaningless while wtab == 0)
    if (!CMD) {
        // (sub[] of the NEXT pair is only written if that pair went through a split kernel: take the tile's own end)
        beg = q.sub[sg];
        end = q.sub_end ? q.sub_end[sg] : ((sub == kFW - 1 && !q.direct) ? q.base[g + 1] : q.sub[sg + 1]);
        if (q.wst) {
            wtab = q.wst_flag[g];
            // the list's row of the window table rides with the header words (lane = window; the lanes behind the last one repeat entry n_windows): its address
            // is the plan's, whatever the flag says -- loaded behind the flag it was a second dependent trip in front of the list
            fw_row = q.wst[(long long)sg * (q.n_windows + 1) + (lane < q.n_windows ? lane : q.n_windows)];
        }
    }
    if (status0 != 0) return; // data-dependent error: nothing is written (the caller re-runs the general path)
    WPROF_INIT();
    const int K = K8 ? 8 : q.K;
    const int NW = q.n_windows;
    const uint32_t *list = q.rec2; // where the sweeps below read the list (CMD: LDS when the list fits)
    if (CMD) {
        uint32_t *colL = &s_area[0][0], *colD = colL + (kColDirect + 1); // (free until phase 1 starts: zeroed below)
        static_assert(2 * (kColDirect + 1) <= kWalkWaves * kWalkWaveWords, "the column fits");
        const int C = S.chunk0[s + 1] - S.chunk0[s];
        const uint32_t n = col_load<kWalkThreads>(cm, S, s, sg - s * cm.TB, colL, colD, wstart);
        const bool in_lds = n <= (uint32_t)kWalkListCap; // workgroup-uniform
        uint32_t *dstl;
        if (in_lds) {
            beg = 0u;
            dstl = s_list;
            list = s_list;
        } else {
            if (tid == 0) wstart[0] = atomicAdd(&q.hdr->rec_cursor, n);
            __syncthreads();
            beg = (uint32_t)__builtin_amdgcn_readfirstlane((int)wstart[0]);
            dstl = q.rec2 + beg;
        }
        end = beg + n;
        // runs -> list: every group of 16 lanes takes runs g16, g16 + 32, ...; four runs' loads in flight before their stores
        const int g16 = tid >> 4, l16 = tid & 15;
        for (int c0 = g16; c0 < C; c0 += 4 * (kWalkThreads / 16)) {
            uint32_t v[4], at[4], cnt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u * (kWalkThreads / 16), cc = c < C ? c : C - 1;
                const uint32_t lo = colL[cc];
                cnt[u] = c < C ? colL[cc + 1] - lo : 0u;
                at[u] = lo;
                // (clamped index: a lane behind the run's end re-reads an address that exists; runs longer than 16 loop below)
                v[u] = cm.rec[colD[cc] + lo + ((uint32_t)l16 < cnt[u] ? (uint32_t)l16 : 0u)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if ((uint32_t)l16 < cnt[u]) dstl[at[u] + l16] = v[u];
                if (cnt[u] > 16u) { // (wave-divergent, rare for the short runs of a direct-mode call)
                    const int c = c0 + u * (kWalkThreads / 16);
                    const uint32_t d = colD[c];
                    for (uint32_t j = 16u + l16; j < cnt[u]; j += 16u) dstl[at[u] + j] = cm.rec[d + at[u] + j];
                }
            }
        }
        __syncthreads(); // the list is complete (and visible to the workgroup); the column's space is free again
    }
    // phase-2 ownership: cell = tid (< 256), the whole K-slot row in one lane (the first four wavefronts; K = 8 used to split
    // the row over two lanes so that all 512 threads work -- but the kernel is bound by VALU issue, and a step costs a
    // half row's lane the same 13 instructions as a whole row's).  Cell c: pixel 128 sub + c / 2 of the tile, polarity c & 1.
    const int ty = tile / q.tiles_x, tx = tile - ty * q.tiles_x;
    const int x0 = tx << q.twl, y0 = ty << q.thl, tw1 = (1 << q.twl) - 1;
    const long long plane = (long long)q.H * q.W;
    const bool owner = tid < kSubCells;
    // (the row's address is worked out again wherever it is needed, from a thread id the compiler cannot recognise: kept alive
    // across phase 1 its pieces were spilled -- 32 bytes of scratch per lane, which the write counter showed as 73 MB per encode)
    auto row_of = [&](int t, bool &in_frame) -> float * {
        asm volatile("" : "+v"(t));
        const int c = t & (kSubCells - 1), p2 = sub * (kSubCells / 2) + (c >> 1);
        const int yy = y0 + (p2 >> q.twl), xx = x0 + (p2 & tw1);
        in_frame = t < kSubCells && yy < q.H && xx < q.W;
        return q.state + (((long long)s * plane + (long long)yy * q.W + xx) * 2 + (c & 1)) * K;
    };
    float st[kMaxK];
    // The state rows are needed behind phase 1 (and their registers should not be alive during it) -- but their trip to HBM should
    // overlap the window scan: one word of every row is requested HERE (a wavefront's rows are 2 KB in a row: all its lines come
    // in) and dropped behind phase 0; the real load then finds the lines in the caches.
    float row_touch = 0.0f;
    {
        bool in_frame;
        const float *r = row_of(tid, in_frame);
        if (in_frame) row_touch = r[0];
    }

    // The window starts: read from the table kf_split_whole<true> left (wtab != 0: no scan, no barrier -- the planes and counters
    // a wavefront zeroes are its own), or found by a scan of the list (phase 0: every other partition form).
    uint32_t first_w = 0u;
    unsigned long long nonempty = 0ull;
    bool general;
    const bool use_mul = mul_bad0 == 0u; // checked for every r of the domain by the partition kernel
    const double rcp = q.rcp;
    const uint32_t wfield = (1u << q.wb) - 1u;
    const int rshift = kCellBits + q.wb;
    {   // planes and counters start at zero (CMD: the column is dead since the barrier behind the gather)
        uint2 *z = (uint2 *)&s_area[wv][0];
        static_assert(kWalkWaveWords % (2 * kWave) == 0, "whole 8-byte sweeps");
#pragma unroll
        for (int i = 0; i < kWalkWaveWords / 2 / kWave; ++i) z[i * kWave + lane] = make_uint2(0u, 0u);
    }
    // The reciprocal table, one correctly rounded division per lane of the LAST wavefront (it has no cells in phase 2); the barrier
    // in front of the first phase 2 publishes it.
    static_assert(kMeanTab == kWave, "lane = count");
    if (wv == kWalkWaves - 1) s_recip[lane] = mean_recip_entry(lane);
    if (!CMD && wtab != 0u) { // workgroup-uniform
        // lane = window: records of the list in front of window `lane` (window-sorted list); entry NW = all of them
        const uint32_t fw0 = fw_row;
        // (until the row came with the header words, a loop here requested one word of every line of the list while the row was
        // on its way; with nothing in front of phase 1's loads any more it only cost its instructions: 52.2 -> 51.5 us without)
        first_w = fw0 != 0xffffffffu ? beg + fw0 : end; // what the scan leaves in wstart[]
        nonempty = __ballot(lane < NW && fw0 != 0xffffffffu);
        general = wtab == 2u;
        asm volatile("" ::"v"(row_touch));
        WPROF(0);
        WPROF(1);
    } else {
    for (int i = tid; i <= NW; i += kWalkThreads) wstart[i] = end;
    if (tid == 0) s_unsorted = 0;
    __syncthreads();
    WPROF(0);
    // ---- phase 0: first record of every window; a window index that decreases = not window-sorted.  A thread looks at four
    // consecutive records -- ONE 16-byte load from the 16-byte block they share (the list's neighbours in front of `beg` and
    // behind `end` are read and masked: the blocks lie inside rec2[] / the LDS list) -- and at the record in front of them.
    {
        const uint32_t n_list = end - beg;
        for (uint32_t c0 = beg & ~3u; c0 < end; c0 += 4 * kWalkThreads) {
            const uint32_t i0 = c0 + 4u * (uint32_t)tid, il = i0 < end ? i0 : (end - 1u) & ~3u; // (lanes behind the end repeat the last block: harmless)
            const uint4 v4 = *(const uint4 *)(list + il);
            const uint32_t pv = list[il > beg ? il - 1u : beg];
            const uint32_t w0 = __builtin_amdgcn_ubfe(v4.x, kCellBits, q.wb), w1 = __builtin_amdgcn_ubfe(v4.y, kCellBits, q.wb);
            const uint32_t w2 = __builtin_amdgcn_ubfe(v4.z, kCellBits, q.wb), w3 = __builtin_amdgcn_ubfe(v4.w, kCellBits, q.wb);
            const uint32_t wp = il > beg ? __builtin_amdgcn_ubfe(pv, kCellBits, q.wb) : 0xffffffffu; // the record in front (none: 0xffffffff)
            const bool full = n_list >= 4u && il - beg <= n_list - 4u; // all four records belong to the list (unsigned: false in front of beg)
            if (full) {
                if (w0 != wp || w1 != w0 || w2 != w1 || w3 != w2) { // a window starts here: a handful of lanes per list
                    if (w0 != wp) { atomicMin(&wstart[w0], il); if (wp != 0xffffffffu && w0 < wp) s_unsorted = 1; }
                    if (w1 != w0) { atomicMin(&wstart[w1], il + 1u); if (w1 < w0) s_unsorted = 1; }
                    if (w2 != w1) { atomicMin(&wstart[w2], il + 2u); if (w2 < w1) s_unsorted = 1; }
                    if (w3 != w2) { atomicMin(&wstart[w3], il + 3u); if (w3 < w2) s_unsorted = 1; }
                }
            } else { // the blocks the list's ends lie in: record by record
                const uint32_t ws[5] = {wp, w0, w1, w2, w3};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t k = il + (uint32_t)e;
                    if (k - beg < n_list) {
                        const bool first = k == beg;
                        if (first || ws[e + 1] != ws[e]) {
                            atomicMin(&wstart[ws[e + 1]], k);
                            if (!first && ws[e + 1] < ws[e]) s_unsorted = 1;
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    asm volatile("" ::"v"(row_touch)); // (the touch has landed; nothing else wants the value)
    WPROF(1);
    general = s_unsorted != 0;
    // wstart[w'] = first record of window w', or `end` for a window without records: window w's stretch starts at the minimum over
    // w' >= w (a window without records starts where the next one does) -- every wavefront finds that window for itself in a
    // ballot over the lanes (lane = window), instead of one thread walking the table between two barriers (12 % of the
    // workgroup's life)
    first_w = wstart[lane < NW ? lane : NW];
    nonempty = __ballot(lane < NW && first_w != end); // (lane = window; window-sorted list: their starts ascend)
    }
    if (general && tid == 0) atomicAdd(&q.hdr->filtered_tiles, 1u);
    WPROF(2);

    float *rplane = (float *)&s_area[wv][0];                      // [kWalkSlots][256]
    uint32_t *cnt = &s_area[wv][kWalkSlots * kSubCells];          // [128] two 16-bit tickets per word, all zero between passes
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma nounroll
    for (int g0 = 0; g0 < NW; g0 += kWalkWaves) {
        // ---- phase 1: wavefront wv sums window g0 + wv; lane l owns cells 4 l .. 4 l + 3
        const int w = g0 + wv;
        float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t num[4] = {0u, 0u, 0u, 0u};
        if (g0 > 0) { // the (sum, count) rows of the previous round lay over planes 0 and 1
            ((float4 *)rplane)[lane] = zero4;
            ((float4 *)rplane)[kWave + lane] = zero4;
        }
        if (w < NW) {
            uint32_t lo = beg, hi = end;
            if (!general) { // the first window with records at or behind w (behind w) starts the stretch (ends it); none: the list's end
                const unsigned long long at = nonempty >> w, behind = w + 1 < 64 ? nonempty >> (w + 1) : 0ull;
                lo = at ? (uint32_t)__builtin_amdgcn_readlane((int)first_w, w + __builtin_ctzll(at)) : end;
                hi = behind ? (uint32_t)__builtin_amdgcn_readlane((int)first_w, w + 1 + __builtin_ctzll(behind)) : end;
            }
#pragma nounroll
            for (uint32_t ptr = lo; ptr < hi; ptr += kWalkChunk) {
                uint32_t m[kWalkRpt], rk[kWalkRpt];
                float val[kWalkRpt];
                // (no load under a lane condition -- each would wait for its own data: lanes behind the end re-read the last record)
#pragma unroll
                for (int u = 0; u < kWalkRpt; ++u) {
                    const uint32_t i = ptr + (uint32_t)(u * kWave + lane);
                    m[u] = list[i < hi ? i : hi - 1u];
                }
                // the ticket = the record's stream rank inside its cell: lanes of one returning LDS atomic are served in lane
                // order, the four instructions of a pass are in stream order
#pragma unroll
                for (int u = 0; u < kWalkRpt; ++u) {
                    const bool take = ptr + (uint32_t)(u * kWave + lane) < hi && (int)((m[u] >> kCellBits) & wfield) == w;
                    rk[u] = 0xffffffffu; // not taken
                    if (take) {
                        const uint32_t lc = m[u] & 255u, sh = (lc & 1u) << 4;
                        rk[u] = (atomicAdd(&cnt[lc >> 1], 1u << sh) >> sh) & 0xffffu;
                    }
                }
                // the value t - 1 with t = (t - t_min) / (w + 1e-8) in f64 (generate_taf.py:215, :26), for every lane (those
                // without a record never store theirs)
                if (use_mul) {
#pragma unroll
                    for (int u = 0; u < kWalkRpt; ++u) val[u] = (float)((double)(m[u] >> rshift) * rcp) - 1.0f;
                } else {
#pragma unroll
                    for (int u = 0; u < kWalkRpt; ++u) {
                        const uint32_t r = m[u] >> rshift;
                        val[u] = q.tlut[r < q.win ? r : q.win];
                    }
                }
                LDS_FENCE();
                const uint2 np = ((const uint2 *)cnt)[lane]; // the counts of cells 4 l .. 4 l + 3
                LDS_FENCE();
                ((uint2 *)cnt)[lane] = make_uint2(0u, 0u);
                const uint4 nn = make_uint4(np.x & 0xffffu, np.x >> 16, np.y & 0xffffu, np.y >> 16);
                const uint32_t n01 = nn.x > nn.y ? nn.x : nn.y, n23 = nn.z > nn.w ? nn.z : nn.w, nmax = n01 > n23 ? n01 : n23;
                // Ranks 0 .. 3 of every cell go straight to plane[rank][cell] (no offsets, no scan, no sorted list); the owner
                // adds its four cells' planes front to back -- a cell without a rank-r record reads +0, and x + 0 == x for every
                // sum that can occur (sums start at +0 and never become -0) -- and clears them.  Cells with more than four
                // records in the pass (0.06 % at 0.7 records per cell and window) cost the wavefront further rounds of four.
#pragma nounroll
                for (uint32_t base = 0u;;) {
#pragma unroll
                    for (int u = 0; u < kWalkRpt; ++u) {
                        const uint32_t rr = rk[u] - base; // (not taken: 0xffffffff - base stays out of range)
                        if (rr < (uint32_t)kWalkSlots) rplane[rr * kSubCells + (m[u] & 255u)] = val[u];
                    }
                    LDS_FENCE();
#pragma unroll
                    for (int r = 0; r < kWalkSlots; ++r) { // sum += t - 1 in stream order, generate_taf.py:26
                        const float4 pr = ((const float4 *)(rplane + r * kSubCells))[lane];
                        LDS_FENCE();
                        ((float4 *)(rplane + r * kSubCells))[lane] = zero4;
                        sum[0] = sum[0] + pr.x;
                        sum[1] = sum[1] + pr.y;
                        sum[2] = sum[2] + pr.z;
                        sum[3] = sum[3] + pr.w;
                    }
                    base += (uint32_t)kWalkSlots;
                    if (__ballot(nmax > base) == 0ull) break;
                }
                num[0] += nn.x; num[1] += nn.y; num[2] += nn.z; num[3] += nn.w;
                LDS_FENCE();
            }
        }
        // (sum, count) of the four cells: rows over planes 0 (sums) and 1 (counts).  The mean is taken in phase 2, behind the barrier
        // that publishes the reciprocal table: a product and two FMAs per (cell, window) there against a full division expansion
        // (2 x v_div_scale, v_rcp, 4 FMAs, a product, v_div_fmas, v_div_fixup) here
        ((float4 *)rplane)[lane] = make_float4(sum[0], sum[1], sum[2], sum[3]);
        ((uint4 *)(rplane + kSubCells))[lane] = make_uint4(num[0], num[1], num[2], num[3]);
        // the 256 thresholds of the leaky transform come to LDS behind phase 2 (requested here, stored in front of its barrier):
        // at the top of the kernel the load's trip was on the path of every wavefront's first barrier
        static_assert(kLeakyTableWords <= kWalkThreads, "one word per thread");
        uint32_t thr_v = 0u;
        if (g0 == 0 && tid < kLeakyTableWords) thr_v = q.leaky_thr[tid];
        if (g0 == 0) { // the state rows: requested behind phase 1 (their registers are not alive during it), used behind the barrier
#pragma unroll
            for (int kk = 0; kk < kMaxK; ++kk) st[kk] = 0.0f;
            bool ok;
            const float *srow = row_of(tid, ok);
            if (ok) {
                if (K8) {
                    const float4 a = ((const float4 *)srow)[0], b = ((const float4 *)srow)[1];
                    st[0] = a.x; st[1] = a.y; st[2] = a.z; st[3] = a.w; st[4] = b.x; st[5] = b.y; st[6] = b.z; st[7] = b.w;
                } else {
#pragma unroll
                    for (int kk = 0; kk < kMaxK; ++kk)
                        if (kk < K) st[kk] = srow[kk];
                }
            }
        }
        WPROF(3);
        __syncthreads();
        WPROF(4);
        // ---- phase 2: one cell per lane, the FIFO steps of this round's windows in order
        if (owner) {
            // (the eight (count, sum) pairs are requested together, in front of the steps: a step that waits for its own pair
            // is an LDS round trip on the workgroup's critical path, eight times)
            uint32_t rn[kWalkWaves];
            float rm[kWalkWaves];
#pragma unroll
            for (int ws = 0; ws < kWalkWaves; ++ws) {
                rn[ws] = s_area[ws][kSubCells + tid];
                rm[ws] = __uint_as_float(s_area[ws][tid]);
            }
            // sum -> mean = sum / ((float)n + 1e-8f) (generate_taf.py:27).  No count of the wavefront at or above kMeanTab (all but
            // the cells of a hot spot): the reciprocals come from the table, their eight loads in flight together, and
            // mean_by_recip gives the division's bits (taf_mean.h; every reachable sum checked on the CPU).  Otherwise the whole
            // wavefront divides.
            uint32_t nmax = rn[0];
#pragma unroll
            for (int ws = 1; ws < kWalkWaves; ++ws) nmax = rn[ws] > nmax ? rn[ws] : nmax;
            if (__ballot(nmax >= (uint32_t)kMeanTab) == 0ull) { // wave-uniform
                float rr[kWalkWaves];
#pragma unroll
                for (int ws = 0; ws < kWalkWaves; ++ws) rr[ws] = s_recip[rn[ws]];
#pragma unroll
                for (int ws = 0; ws < kWalkWaves; ++ws) rm[ws] = mean_by_recip(rm[ws], (float)rn[ws], rr[ws]);
            } else {
#pragma unroll
                for (int ws = 0; ws < kWalkWaves; ++ws) rm[ws] = fifo_mean(rn[ws], rm[ws]);
            }
#pragma unroll
            for (int ws = 0; ws < kWalkWaves; ++ws)
                if (g0 + ws < NW && ((wmask >> (g0 + ws)) & 1ull)) fifo_step(st, K, true, rn[ws], rm[ws]);
        }
        if (g0 == 0 && tid < kLeakyTableWords) thr[tid] = thr_v;
        __syncthreads();
        WPROF(5);
    }

    // ---- write-out: state, optional f32 view (2K, H, W), optional uint8 leaky transform (K, 2, H, W)
    uint8_t *ob = (uint8_t *)&s_area[0][0]; // [2K planes][128 pixels of the sub-tile] (the last phase 2 ended with a barrier)
    // K = 8: a lane holds a whole 32-byte row; stored from here it would leave as two instructions of 16 bytes at a 32-byte stride
    // -- half a sector each, twice the write requests (WRITE_SIZE showed 147 MB for 74).  The rows go through LDS instead and
    // leave below from all 512 threads, 16 bytes each, consecutive threads writing consecutive pieces: whole lines.
    float4 *rowst = (float4 *)&s_area[1][0]; // [256 rows][2] (behind the 2 KB of uint8 staging; the plane areas are dead)
    static_assert(kWalkWaveWords * 4 >= 2 * kMaxK * (kSubCells / 2) && (kWalkWaves - 1) * kWalkWaveWords * 4 >= kSubCells * 32, "staging fits");
    if (K8 && owner) {
        rowst[2 * tid] = make_float4(st[0], st[1], st[2], st[3]);
        rowst[2 * tid + 1] = make_float4(st[4], st[5], st[6], st[7]);
    }
    const int pol = tid & 1;
    {
        bool ok;
        float *srow = row_of(tid, ok);
        if (ok) {
            if (!K8) {
#pragma unroll
                for (int k = 0; k < kMaxK; ++k)
                    if (k < K) srow[k] = st[k];
            }
            if (q.view_f32) { // (the row's element index / (2 K) is the pixel, generate_taf.py:55)
                float *vw = q.view_f32 + (long long)s * 2 * K * plane + ((srow - q.state) / (2 * K) - (long long)s * plane);
#pragma unroll
                for (int k = 0; k < kMaxK; ++k)
                    if (k < K) vw[(long long)(2 * k + pol) * plane] = st[k];
            }
        }
    }
    if (q.out_u8) {
        if (owner) {
            uint8_t lv[kMaxK];
            leaky_u8_bucket_n<kMaxK>(st, thr, lv); // the eight table look-ups in flight together
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) {
                if (k < K) {
                    const int ko = q.flip ? (K - 1 - k) : k;
                    ob[(2 * ko + pol) * (kSubCells / 2) + (tid >> 1)] = lv[k];
                }
            }
        }
    }
    WPROF(6);
    if (K8 || q.out_u8) __syncthreads(); // (workgroup-uniform)
    WPROF(7);
    if (K8) { // thread t: half t & 1 of the row of cell t / 2
        const int c2 = tid >> 1, pt2 = sub * (kSubCells / 2) + (c2 >> 1);
        const int py2 = y0 + (pt2 >> q.twl), px2 = x0 + (pt2 & tw1);
        if (py2 < q.H && px2 < q.W)
            ((float4 *)(q.state + (((long long)s * plane + (long long)py2 * q.W + px2) * 2 + (c2 & 1)) * 8))[tid & 1] = rowst[tid];
    }
    if (q.out_u8) {
        // the (K, 2, H, W) volume leaves plane by plane in 16-pixel pieces: one 16-byte store where the row allows
        for (int c = tid; c < 2 * K * 8; c += kWalkThreads) {
            const int pl = c >> 3, part = c & 7;
            const int p16 = sub * (kSubCells / 2) + 16 * part;
            const int y = y0 + (p16 >> q.twl), x = x0 + (p16 & tw1);
            if (y >= q.H || x >= q.W) continue;
            const uint8_t *src = ob + pl * (kSubCells / 2) + 16 * part;
            uint8_t *dst = q.out_u8 + ((long long)s * 2 * K + pl) * plane + (long long)y * q.W + x;
            if (x + 16 <= q.W && (((uintptr_t)dst) & 15u) == 0) {
                *(uint4 *)dst = *(const uint4 *)src;
            } else {
                const int nv = q.W - x < 16 ? q.W - x : 16;
                for (int e = 0; e < nv; ++e) dst[e] = src[e];
            }
        }
    }
    WPROF(8);
    WPROF_END();
}
} // namespace
