// ev_fast.h -- the Event Volume consumers: the ticket sort of one wavefront (WavePass), kf_ev_sub and kf_ev_fadd.
// Expects taf_decode.h (FastHeader), frlw_consts.h (kMaxK) and taf_column.h.
#pragma once
#include "taf_column.h"
#include "taf_decode.h"

namespace {
// ---- the ticket sort of one wavefront (kf_ev_sub) ------------------------------------------------------------------------
// Wave-private pass (the core of kf_taf_walk's phase 1, factored out): up to 256 records of ONE sub-tile, in stream order,
// become per-cell ordered segments -- a ticket per record from two-per-word 16-bit LDS counters (lane-ordered, so the
// ticket is the stream rank inside the cell), a wave scan of the cell counts, values to sorted[offset(cell) + ticket] --
// and every lane then walks the segments of its four cells (64 j + lane) front to back.
struct WavePass {
    uint32_t *cnt;  // [128]: two 16-bit tickets per word, all zero between passes
    uint16_t *off;  // [256]
    float *sorted;  // [256] (Event Volume: [2 * 256 + 2], pairs of weights + one all-zero pair)
};

// m[u], u < 4: the lane's records of this pass (0xffffffff = none), record u * 64 + lane of the pass in stream order;
// val(m) -> the f32 to sort.  Returns the lane's four cell counts n[] and segment starts o[] in sorted[]; the caller
// walks the segments (wave_segments below) and ends the pass with LDS_FENCE().  wave_rank: the part both sorts share --
// rk[u] = the ticket of record u (0xffffffff = none), n[] and o[].
__device__ __forceinline__ void wave_rank(const WavePass &P, const uint32_t (&m)[4], int lane, uint32_t (&rk)[4], uint32_t (&n)[4], uint32_t (&o)[4])
{
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        rk[u] = 0xffffffffu;
        if (m[u] != 0xffffffffu) {
            const uint32_t lc = m[u] & 255u, sh = 16u * (lc & 1u);
            rk[u] = (atomicAdd(&P.cnt[lc >> 1], 1u << sh) >> sh) & 0xffffu;
        }
    }
    LDS_FENCE();
#pragma unroll
    for (int j = 0; j < 4; ++j) n[j] = (P.cnt[32 * j + (lane >> 1)] >> (16 * (lane & 1))) & 0xffffu;
    LDS_FENCE();
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (!(lane & 1)) P.cnt[32 * j + (lane >> 1)] = 0u; // after both lanes of the word have read it
    {
        const uint32_t tl = n[0] + n[1] + n[2] + n[3];
        const uint32_t inc = wave_incl_scan(tl);
        o[0] = inc - tl; o[1] = o[0] + n[0]; o[2] = o[1] + n[1]; o[3] = o[2] + n[2];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) P.off[64 * j + lane] = (uint16_t)o[j];
    LDS_FENCE();
}
template <class Val>
__device__ __forceinline__ void wave_sort(const WavePass &P, const uint32_t (&m)[4], int lane, Val val, uint32_t (&n)[4], uint32_t (&o)[4])
{
    uint32_t rk[4];
    wave_rank(P, m, lane, rk, n, o);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (rk[u] != 0xffffffffu) P.sorted[(uint32_t)P.off[m[u] & 255u] + rk[u]] = val(m[u]);
    LDS_FENCE();
}

// The same with a PAIR of f32 per record (val2(m, a, b)): sorted[2 * slot], sorted[2 * slot + 1]; slot 256 is kept all zero.
template <class Val2>
__device__ __forceinline__ void wave_sort2(const WavePass &P, const uint32_t (&m)[4], int lane, Val2 val2, uint32_t (&n)[4], uint32_t (&o)[4])
{
    uint32_t rk[4];
    wave_rank(P, m, lane, rk, n, o);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (rk[u] != 0xffffffffu) {
            float a, b;
            val2(m[u], u, a, b);
            *(float2 *)&P.sorted[2u * ((uint32_t)P.off[m[u] & 255u] + rk[u])] = make_float2(a, b);
        }
    LDS_FENCE();
}

// add2(j, a, b): cell j of this lane receives the pair next; slots behind a segment's end read the all-zero pair, and
// adding +0 to these non-negative sums changes nothing -- no select around the accumulators at all.
template <class Add2>
__device__ __forceinline__ void wave_segments2(const WavePass &P, const uint32_t (&n)[4], const uint32_t (&o)[4], Add2 add2)
{
    uint32_t nmax = n[0] > n[1] ? n[0] : n[1];
    nmax = n[2] > nmax ? n[2] : nmax;
    nmax = n[3] > nmax ? n[3] : nmax;
    const uint32_t nm = wave_max_u32(nmax);
#pragma nounroll
    for (uint32_t a = 0; a < nm; ++a) {
        float2 e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = *(const float2 *)&P.sorted[2u * (a < n[j] ? o[j] + a : 256u)];
#pragma unroll
        for (int j = 0; j < 4; ++j) add2(j, e[j].x, e[j].y);
    }
}

// add(j, v, live): "cell j of this lane receives v next" when live -- a select, not a branch (divergent control flow
// around the accumulators makes the compiler keep copies of all of them).
template <class Add>
__device__ __forceinline__ void wave_segments(const WavePass &P, const uint32_t (&n)[4], const uint32_t (&o)[4], Add add)
{
    uint32_t nmax = n[0] > n[1] ? n[0] : n[1];
    nmax = n[2] > nmax ? n[2] : nmax;
    nmax = n[3] > nmax ? n[3] : nmax;
    const uint32_t nm = wave_max_u32(nmax); // the longest segment of the wavefront: a uniform trip count
#pragma nounroll
    for (uint32_t a = 0; a < nm; ++a) {
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t at = o[j] + a;
            e[j] = P.sorted[at < 255u ? at : 255u];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) add(j, e[j], a < n[j]);
    }
}

// ---- Event Volume ------------------------------------------------------------------------------------------------------
struct EvTileP {
    int H, W, twl, thl, tiles_x, T, bins;
    uint32_t win;
    double rcp;           // FastGeom::rcp
    const uint32_t *rec2; // sub-tile-major records: the lists kf_ev_sub walks (chunk-major + direct: where a consumer books space for a long list)
    const uint32_t *base; // [pairs + 1]
    const uint32_t *sub;  // [pairs * 16 + 1]
    const uint32_t *sub_end; // TileP::sub_end
    int pairs;
    int direct;           // TileP::direct
    const float *tlut;    // tlut[r] = float(r / window)
    FastHeader *hdr;
    float *out_f32;       // (B, 2 * bins, H, W) or NULL
    uint8_t *out_u8;      // (B, 2 * bins, H, W) or NULL
};

// generate_eventvolume.py:23-32 for one event of normalised time tn on one cell: t* = bins * float(t); bin k (1-based)
// receives 1 - |k - t*| when that is not negative.  Only the two bins around t*, k0 = floor(t*) and k0 + 1, can: for the
// others |k - t*| >= 1 already before rounding, so their weight is zero or dropped and changes no sum.
template <int BINS>
__device__ __forceinline__ void ev_add(float (&acc)[BINS], float binsf, float tn, bool live)
{
    const float ts = binsf * tn;
#pragma unroll
    for (int k = 0; k < BINS; ++k) {
        const float d = (float)(k + 1) - ts;
        const float w = 1.0f - fabsf(d); // :28
        const float na = acc[k] + w;
        acc[k] = (live && w > 0.0f) ? na : acc[k]; // :29 (w == 0 adds nothing either)
    }
}

// One pass of up to 256 records of one sub-tile through the wave's accumulators.  Usual case (a pass is 256 consecutive
// records of one sub-tile of a time-sorted stream): floor(t*) = K0 is the same for every record -- then each record works
// out its own two weights (bins K0 and K0 + 1) once, and the owner lanes only ADD them in stream order.
template <int BINS>
__device__ __forceinline__ void ev_pass(const WavePass &P, const uint32_t (&pm)[4], int lane, const EvTileP &q, bool use_mul, double rcp,
                                        float binsf, float (&acc)[4][BINS])
{
    uint32_t n[4], o[4];
    float tn[4];
    bool differs = false;
    // (lane 0, u = 0 holds the pass's first record: a pass is never empty)
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)pm[0]) >> kCellBits;
    const int kfirst = (int)(binsf * (use_mul ? (float)((double)r0 * rcp) : q.tlut[r0]));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        tn[u] = 0.0f;
        if (pm[u] != 0xffffffffu) {
            const uint32_t r = pm[u] >> kCellBits;
            tn[u] = use_mul ? (float)((double)r * rcp) : q.tlut[r]; // float((t - t0) / window), generate_eventvolume.py:141, :23
            differs |= (int)(binsf * tn[u]) != kfirst;
        }
    }
    const int k0 = __ballot(differs) ? -1 : kfirst;
    if (k0 >= 0 && k0 <= BINS) {
        // weights of the 1-based bins k0 (if >= 1) and k0 + 1 (if <= BINS), exactly as ev_add computes them; they are >= 0
        const bool lo_ok = k0 >= 1, hi_ok = k0 + 1 <= BINS;
        const float klo = (float)k0, khi = (float)(k0 + 1);
        wave_sort2(P, pm, lane,
                   [&](uint32_t, int u, float &a, float &b) {
                       const float ts = binsf * tn[u]; // t* = bins * float(t), :23
                       const float wl = 1.0f - fabsf(klo - ts), wh = 1.0f - fabsf(khi - ts); // :28
                       a = (lo_ok && wl > 0.0f) ? wl : 0.0f; // :29
                       b = (hi_ok && wh > 0.0f) ? wh : 0.0f;
                   }, n, o);
        switch (k0) {
#define EV_CASE(K) case K: wave_segments2(P, n, o, [&](int j, float a, float b) { \
            if (K >= 1 && K - 1 < BINS) acc[j][K >= 1 ? K - 1 : 0] += a; \
            if (K < BINS) acc[j][K < BINS ? K : 0] += b; }); break;
            EV_CASE(0) EV_CASE(1) EV_CASE(2) EV_CASE(3) EV_CASE(4) EV_CASE(5) EV_CASE(6) EV_CASE(7) EV_CASE(8)
#undef EV_CASE
        default: break;
        }
    } else {
        wave_sort(P, pm, lane, [&](uint32_t w) { const uint32_t r = w >> kCellBits; return use_mul ? (float)((double)r * rcp) : q.tlut[r]; }, n, o);
        wave_segments(P, n, o, [&](int j, float t, bool live) { ev_add<BINS>(acc[j], binsf, t, live); });
    }
    LDS_FENCE();
}

// the cells 64 j + lane of a sub-tile: scale (generate_eventvolume.py:37) and write both outputs
template <int BINS>
__device__ __forceinline__ void ev_store_cells(const EvTileP &q, int s, int tile, int sub, int lane, int j, const float (&acc)[BINS])
{
    const int ty = tile / q.tiles_x, tx = tile - ty * q.tiles_x;
    const int x0 = tx << q.twl, y0 = ty << q.thl, tw1 = (1 << q.twl) - 1;
    const long long plane = (long long)q.H * q.W;
    const int pol = lane & 1, ch = pol ? 0 : 1; // weights [p, 1 - p]: channel 0 = p == 1
    const int pt = sub * (kSubCells / 2) + 32 * j + (lane >> 1); // cell 64 j + lane = pixel 32 j + lane / 2, polarity lane & 1
    const int py = y0 + (pt >> q.twl), px = x0 + (pt & tw1);
    if (py >= q.H || px >= q.W) return;
#pragma unroll
    for (int k = 0; k < BINS; ++k) {
        if (k < q.bins) {
            const float v = acc[k] / 5.0f * 255.0f; // generate_eventvolume.py:37
            const long long idx = ((long long)s * 2 * q.bins + (2 * k + ch)) * plane + (long long)py * q.W + px;
            if (q.out_f32) q.out_f32[idx] = v;
            if (q.out_u8) q.out_u8[idx] = f32_to_u8(v > 255.0f ? 255.0f : v);
        }
    }
}

template <int BINS>
__device__ __forceinline__ void ev_store(const EvTileP &q, int s, int tile, int sub, int lane, const float (&acc)[4][BINS])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) ev_store_cells<BINS>(q, s, tile, sub, lane, j, acc[j]);
}

// After the segment split (kf_split_whole's counting blocks + kf_split_place): one wavefront per sub-tile walks its own
// contiguous list -- the skewed tiles of any call, and every tile of a call with few (sequence, tile) pairs.
// CMD (chunk-major partition, direct mode): the wavefront first gathers its sub-tile's runs from the chunks' stretches of rec[]
// -- its column of the directory, scanned 64 chunks at a time, then groups of 16 lanes copy a run each -- into LDS when the list
// fits (kEvListCap records), else into rec2[] at the header's cursor; everything after that is the walk over one contiguous list.
constexpr int kEvListCap = 2048;  // records of a sub-tile's list kept in LDS per wavefront
template <int BINS, bool CMD = false>
// (five wavefronts per SIMD where the registers allow it without spills -- the five-bin list walk, 102 -> 92 VGPRs: every
// wavefront is a latency chain of its own, one more of them per SIMD hides more of it)
__global__ __launch_bounds__(4 * kWave) __attribute__((amdgpu_waves_per_eu((BINS <= 5 && !CMD) ? 5 : 1, 8))) void kf_ev_sub(EvTileP q, CmP cm, SeqTab S)
{
    __shared__ uint32_t s_cnt[4][kSubCells / 2];
    __shared__ uint16_t s_off[4][kSubCells];
    __shared__ __attribute__((aligned(8))) float s_sorted[4][2 * kSubCells + 2];
    __shared__ uint32_t s_colL[CMD ? 4 : 1][CMD ? kColEv + 1 : 1], s_colD[CMD ? 4 : 1][CMD ? kColEv : 1];
    __shared__ uint32_t s_list[CMD ? 4 : 1][CMD ? kEvListCap : 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (lane < 2) s_sorted[wv][2 * kSubCells + lane] = 0.0f; // the all-zero pair behind the segments
    // (CMD: the workgroup's four bins through the XCD mapping -- the runs of neighbouring bins share cache lines of rec[])
    const int sg = (CMD ? (int)xcd_owned_index(blockIdx.x, gridDim.x) : (int)blockIdx.x) * 4 + wv;
    if (sg >= q.pairs * kFW || q.hdr->status != 0) return;
    const int g = sg / kFW, sub = sg - g * kFW;
    const int s = g / q.T, tile = g - s * q.T;
    for (int i = lane; i < kSubCells / 2; i += kWave) s_cnt[wv][i] = 0u;
    const WavePass P = {s_cnt[wv], s_off[wv], s_sorted[wv]};
    const bool use_mul = q.hdr->mul_bad == 0u;
    const double rcp = q.rcp;
    const float binsf = (float)q.bins;
    float acc[4][BINS];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < BINS; ++k) acc[j][k] = 0.0f;
    uint32_t beg, end;
    const uint32_t *list = q.rec2;
    if (CMD) {
        uint32_t *colL = s_colL[wv], *colD = s_colD[wv];
        const int C = S.chunk0[s + 1] - S.chunk0[s];
        const uint32_t n = col_load_wave(cm, S, s, sg - s * cm.TB, colL, colD);
        LDS_FENCE();
        uint32_t *dstl;
        if (n <= (uint32_t)kEvListCap) { // wave-uniform
            beg = 0u;
            dstl = s_list[wv];
            list = s_list[wv];
        } else {
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(&q.hdr->rec_cursor, n);
            beg = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
            dstl = const_cast<uint32_t *>(q.rec2) + beg;
        }
        end = beg + n;
        // four groups of 16 lanes, eight runs each per step
        col_gather<4, 8>(colL, colD, C, lane >> 4, lane & 15, cm.rec, [&](uint32_t i, uint32_t w) { dstl[i] = w; });
        __threadfence_block(); // (the wavefront reads back what its own lanes wrote: LDS in order; rec2[] through the fence)
        LDS_FENCE();
    } else {
        // (sub[] of the NEXT pair is only written if that pair went through a split kernel: take the tile's own end)
        beg = q.sub[sg];
        end = q.sub_end ? q.sub_end[sg] : ((sub == kFW - 1 && !q.direct) ? q.base[g + 1] : q.sub[sg + 1]);
    }
    uint32_t nx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint32_t i = beg + (uint32_t)(u * kWave + lane);
        nx[u] = 0xffffffffu;
        if (end > beg) { const uint32_t v = list[i < end ? i : end - 1u]; nx[u] = i < end ? v : 0xffffffffu; }
    }
    LDS_FENCE();
    // A pass whose records all lie in ONE slice of the window (same floor(t*)) takes ev_pass's cheap form -- two weights per
    // record, pairs added in stream order -- a pass that straddles a slice boundary the general one (every bin tried for every
    // record).  A time-sorted list of ~1 700 records crosses the five boundaries in five of its seven 256-record passes; so a
    // pass is CUT at the first record of the next slice (the rest of its 256 records is fetched again by the next pass): twelve
    // cheap passes instead of two cheap and five general ones.  The cut uses an approximate slice index (float(r * bins) / window:
    // monotone in r); ev_pass still classifies exactly, so a record the approximation puts on the wrong side of a boundary only
    // costs that pass the general form.  Cuts in front of record 64 are not made (an unsorted list would otherwise crawl).
    const float inv_win = 1.0f / (float)q.win;
    const uint32_t ubins = (uint32_t)q.bins;
    for (uint32_t p0 = beg; p0 < end;) {
        uint32_t pm[4];
        uint32_t take = 256u;
        {
            const uint32_t k0 = (uint32_t)((float)(((uint32_t)__builtin_amdgcn_readfirstlane((int)nx[0]) >> kCellBits) * ubins) * inv_win);
#pragma unroll
            for (int u = 3; u >= 0; --u) { // (descending: the lowest u with a differing record wins)
                pm[u] = nx[u];
                const unsigned long long d = __ballot(pm[u] != 0xffffffffu && (uint32_t)((float)((pm[u] >> kCellBits) * ubins) * inv_win) != k0);
                if (d) take = (uint32_t)(u * kWave) + (uint32_t)__builtin_ctzll(d);
            }
            if (take < (uint32_t)kWave) take = 256u;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((uint32_t)(u * kWave + lane) >= take) pm[u] = 0xffffffffu;
            const uint32_t i = p0 + take + (uint32_t)(u * kWave + lane);
            const uint32_t v = list[i < end ? i : end - 1u];
            nx[u] = i < end ? v : 0xffffffffu;
        }
        ev_pass<BINS>(P, pm, lane, q, use_mul, rcp, binsf, acc);
        p0 += take;
    }
    ev_store<BINS>(q, s, tile, sub, lane, acc);
}

// Small direct-mode calls (ONE label window of a GEN1-shaped stream: 576 sub-tile lists of ~1 700 records): kf_ev_sub's ticket
// sort is built for throughput and leaves such a call on a latency chain of seven dependent passes per wavefront (30 us).  Here
// the sums are made by the LDS itself: ds_add_f32 applies the lanes of one instruction that hit one address in ascending lane
// order with the rounding of v_add_f32 (fact 2 of DESIGN.md 3.2; the library's self-test checks it on the first call and this
// kernel is only used where it held), a wavefront's instructions are served in program order -- so one wavefront that feeds its
// list through `acc[bin][cell] += weight` 64 records at a time makes exactly the reference's sequential sums
// (generate_eventvolume.py:28-32), without tickets, scans or segment walks.  It costs 192 cycles per instruction and CU (3 x the
// ticket scheme per record), which is why only small calls come here.  Four wavefronts share a sub-tile: they gather its list
// together, and then EACH walks the whole list but adds only into the bins k with k % 4 == its index -- every (cell, bin) sum
// stays one wavefront's chain in stream order, and the four chains of atomics run side by side.
// An event adds to the two bins around t* = bins * float(t): records of one instruction whose floor(t*) differ are issued run by
// run (equal floors, lane order), because the upper weight of an earlier record and the lower weight of a later one can meet in
// one bin -- a time-sorted stream has one run per instruction except at the five slice boundaries.
constexpr int kFaddWaves = 4; // wavefronts per sub-tile: they gather the list together, then wavefront w owns the bins k with k % 4 == w
template <int BINS>
__global__ __launch_bounds__(kFaddWaves *kWave) void kf_ev_fadd(EvTileP q, CmP cm, SeqTab S)
{
    constexpr int NT = kFaddWaves * kWave;
    __shared__ float s_acc[BINS][kSubCells];
    __shared__ uint32_t s_colL[kColEv + 1], s_colD[kColEv], s_wsum[kFaddWaves + 1];
    __shared__ uint32_t s_list[kEvListCap];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int sg = (int)xcd_owned_index(blockIdx.x, gridDim.x); // (neighbouring bins, whose runs share cache lines of rec[], through one L2)
    if (sg >= q.pairs * kFW || q.hdr->status != 0) return;
    const int g = sg / kFW, sub = sg - g * kFW;
    const int s = g / q.T, tile = g - s * q.T;
    const bool use_mul = q.hdr->mul_bad == 0u;
    const double rcp = q.rcp;
    const float binsf = (float)q.bins;
    for (int i = tid; i < BINS * kSubCells; i += NT) (&s_acc[0][0])[i] = 0.0f;
    // the list: this sub-tile's runs in the chunks' stretches of rec[] (the column of the directory, then groups of 16 lanes
    // copy a run each: what kf_ev_sub<BINS, true> does with one wavefront, here with four)
    const int C = S.chunk0[s + 1] - S.chunk0[s]; // (<= kColEv)
    const uint32_t n = col_load<NT>(cm, S, s, sg - s * cm.TB, s_colL, s_colD, s_wsum);
    uint32_t beg = 0u;
    uint32_t *dstl = s_list;
    const uint32_t *list = s_list;
    if (n > (uint32_t)kEvListCap) { // (workgroup-uniform) a list too long for LDS goes through rec2[]
        if (tid == 0) s_wsum[kFaddWaves] = atomicAdd(&q.hdr->rec_cursor, n);
        __syncthreads();
        beg = s_wsum[kFaddWaves];
        dstl = const_cast<uint32_t *>(q.rec2) + beg;
        list = q.rec2;
    }
    const uint32_t end = beg + n;
    // groups of 16 lanes, ten runs each per step (one step for the 144 chunks of a GEN1 stream)
    col_gather<NT / 16, 10>(s_colL, s_colD, C, tid >> 4, tid & 15, cm.rec, [&](uint32_t i, uint32_t w) { dstl[i] = w; });
    __syncthreads(); // the list is complete (LDS, or rec2[] written and read on this CU)
    // every wavefront walks the whole list in stream order and adds into ITS bins only: a (cell, bin) sum is one wavefront's chain
    float *accl = &s_acc[0][0];
    for (uint32_t p0 = beg; p0 < end; p0 += 4 * kWave) {
        uint32_t pm[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { // (four instructions' records in flight; clamped index, masked below)
            const uint32_t i = p0 + (uint32_t)(u * kWave + lane);
            pm[u] = list[i < end ? i : end - 1u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool valid = p0 + (uint32_t)(u * kWave + lane) < end;
            const uint32_t r = pm[u] >> kCellBits, cell = pm[u] & 255u;
            const float tn = use_mul ? (float)((double)r * rcp) : q.tlut[r < q.win ? r : q.win]; // float((t - t0) / window), :141, :23
            const float ts = binsf * tn;                       // t* = bins * float(t), :23
            const int k0 = (int)ts;                            // floor (t* >= 0): the 1-based bins k0 and k0 + 1 can receive
            const float wl = 1.0f - fabsf((float)k0 - ts), wh = 1.0f - fabsf((float)(k0 + 1) - ts); // :28
            // :29 (a weight of zero adds nothing either); 0-based bin k0 - 1 takes wl, bin k0 takes wh
            const bool lo_ok = valid && k0 >= 1 && k0 <= q.bins && wl > 0.0f && ((k0 - 1) & (kFaddWaves - 1)) == wv;
            const bool hi_ok = valid && k0 + 1 <= q.bins && wh > 0.0f && (k0 & (kFaddWaves - 1)) == wv;
            if (__ballot(lo_ok || hi_ok) == 0ull) continue; // (none of this instruction's records touches my bins)
            const int kv = valid ? k0 : -1;
            const int kprev = __shfl_up(kv, 1);
            unsigned long long starts = __ballot(lane == 0 || kv != kprev); // runs of equal floor(t*), in lane order
            while (starts) {
                const int rb = __builtin_ctzll(starts);
                starts &= starts - 1ull;
                const int re = starts ? __builtin_ctzll(starts) : kWave;
                const bool in = lane >= rb && lane < re;
                if (in && lo_ok) atomicAdd(&accl[(k0 - 1) * kSubCells + (int)cell], wl);
                if (in && hi_ok) atomicAdd(&accl[k0 * kSubCells + (int)cell], wh);
            }
        }
    }
    __syncthreads();
    float acc[BINS];
#pragma unroll
    for (int k = 0; k < BINS; ++k) acc[k] = s_acc[k][64 * wv + lane];
    ev_store_cells<BINS>(q, s, tile, sub, lane, wv, acc);
}
} // namespace
