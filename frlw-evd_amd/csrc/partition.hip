// partition.hip -- stable tile partition of an event stream (steps 1-3 of every encoder).
//
// The reference's accumulators (torch index_add_, generate_eventvolume.py:32, generate_taf.py:24-26)
// are defined by the single-thread result: f32 adds in STREAM ORDER.  To reproduce that on a GPU the
// events are first partitioned by tile ((1 << twl) x 8 pixels) with a STABLE counting sort, so that
// every tile's records are still in stream order and one workgroup can own the tile's accumulators.
//
//   k_hist      one workgroup (16 wavefronts) per contiguous chunk of 1024*bpw events; LDS histogram
//               over tiles -> counts[wg][tile]          (events read once, bpw loads in flight / lane)
//   k_slabscan  exclusive prefix over the 32 workgroups of a slab, in place + slabtot[slab][tile]
//   k_tilescan  exclusive prefix over slabs (in place) and over tiles      -> base[tile]
//   k_scatter   same chunks again.  Wavefront w of the workgroup owns the w-th run of 64*bpw events and
//               walks it 64 events at a time in stream order; the rank of an event among the events
//               of its batch that fall in the same tile comes from an LDS tag round (write the lane
//               id, read it back: a mismatch marks a collision) plus one ballot per colliding tile.
//               Per-wave running counts live in LDS; after a workgroup barrier they are prefix-summed
//               over the 16 waves, and the whole workgroup writes its 8-byte records in ONE burst, so
//               each tile's run (~chunk / n_tiles records) is completed in the L2 while it is hot.

#include "frlw_common.h"
#include <type_traits>

namespace frlw {

int hip_fail(hipError_t e, const char *what, int line)
{
#ifdef FRLW_DEV_BUILD // developer build only: the product library prints nothing and reads no environment
    fprintf(stderr, "frlw_evd: %s failed at line %d: %s\n", what, line, hipGetErrorString(e));
#else
    (void)e; (void)what; (void)line;
#endif
    return FRLW_ERR_HIP;
}

namespace {
template <int LAYOUT, int KIND, bool HAS_MAP>
__global__ __launch_bounds__(kPartThreads) void k_hist(Decode P, int bpw, uint32_t *counts,
                                                        int32_t *errs, float *tlut_w)
{
    extern __shared__ uint32_t lds[];
    uint32_t *hist = lds; // [n_tiles]
    __shared__ int serr;
    const int tid = threadIdx.x;
    const long long wg = chunk_of_block(blockIdx.x, gridDim.x);
    for (int b = tid; b < P.n_tiles; b += kPartThreads) hist[b] = 0;
    if (tid == 0) serr = 0;
    __syncthreads();
    const long long begin = wg * (long long)kPartThreads * bpw;
    int err = 0;
    if (KIND == KIND_TAF && tlut_w) {
        // value table for k_scatter: tlut[r] = float(r / (win + 1e-8)) - 1 (generate_taf.py:215, :26);
        // one correctly rounded f64 division per distinct in-window time instead of one per event
        const double den = (double)P.win + 1e-8;
        for (long long r = wg * kPartThreads + tid; r <= P.win; r += (long long)gridDim.x * kPartThreads)
            tlut_w[r] = (float)((double)r / den) - 1.0f;
    }
    if (LAYOUT == FRLW_LAYOUT_DAT8) {
        const uint2 *src = (const uint2 *)P.data + begin;
        const long long left = P.n - begin;
        const uint32_t nloc = left < (long long)kPartThreads * bpw ? (uint32_t)(left < 0 ? 0 : left) : (uint32_t)(kPartThreads * bpw);
        uint2 q[kMaxBpw];
#pragma unroll
        for (int j = 0; j < kMaxBpw; ++j) {
            const uint32_t i = (uint32_t)(j * kPartThreads + tid);
            q[j] = i < nloc ? src[i] : make_uint2(0u, 0xffffffffu);
        }
#pragma unroll
        for (int j = 0; j < kMaxBpw; ++j) {
            const uint32_t i = (uint32_t)(j * kPartThreads + tid);
            if (i < nloc) {
                const Pos o = dat_pos<KIND, HAS_MAP>(P, q[j]);
                err |= o.err;
                if (o.tile >= 0) atomicAdd(&hist[o.tile], 1u);
            }
        }
    } else {
        for (int j = 0; j < bpw; ++j) {
            const long long i = begin + (long long)j * kPartThreads + tid;
            if (i < P.n) {
                double t;
                const Pos o = f64_pos<KIND>(P, i, t);
                err |= o.err;
                if (o.tile >= 0) atomicAdd(&hist[o.tile], 1u);
            }
        }
    }
    if (err) atomicOr(&serr, err);
    __syncthreads();
    uint32_t *row = counts + wg * (long long)P.n_tiles;
    for (int b = tid; b < P.n_tiles; b += kPartThreads) row[b] = hist[b];
    // data-dependent errors of this chunk: a plain store per workgroup, OR-ed into the header by k_tilescan (which
    // also resets the header -- no memset launch, no pre-zeroed workspace needed)
    if (tid == 0) errs[wg] = serr;
}

// counts[u][b], u in one slab of 32 workgroups -> exclusive prefix over u (in place), slabtot[slab][b]
__global__ __launch_bounds__(kWave) void k_slabscan(uint32_t *counts, int units, int n_tiles,
                                                     uint32_t *slabtot)
{
    const int b = blockIdx.x * kWave + threadIdx.x;
    const int slab = blockIdx.y;
    const int u0 = slab * kSlabUnits;
    if (b >= n_tiles) return;
    uint32_t v[kSlabUnits];
#pragma unroll
    for (int k = 0; k < kSlabUnits; ++k)
        v[k] = (u0 + k < units) ? counts[(long long)(u0 + k) * n_tiles + b] : 0u;
    uint32_t run = 0;
#pragma unroll
    for (int k = 0; k < kSlabUnits; ++k) {
        const uint32_t t = v[k];
        v[k] = run;
        run += t;
    }
#pragma unroll
    for (int k = 0; k < kSlabUnits; ++k)
        if (u0 + k < units) counts[(long long)(u0 + k) * n_tiles + b] = v[k];
    slabtot[(long long)slab * n_tiles + b] = run;
}

// slabtot[s][b] -> exclusive prefix over s (in place); then exclusive scan over tiles -> base[0..n]
__global__ __launch_bounds__(1024) void k_tilescan(uint32_t *slabtot, int slabs, int n, uint32_t *base,
                                                   WsHeader *hdr, uint32_t hot_thr, const int32_t *errs, int units)
{
    __shared__ uint32_t tot[kMaxTiles];
    __shared__ uint32_t wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) { hdr->status = 0; hdr->pad = 0; hdr->wmask = 0ull; hdr->n_hot = 0u; hdr->hot_thr = hot_thr; }
    __syncthreads();
    {
        int e = 0;
        for (int u = tid; u < units; u += 1024) e |= errs[u];
        if (e) atomicOr(&hdr->status, e);
    }
    for (int b = tid; b < n; b += 1024) {
        uint32_t run = 0;
        for (int s0 = 0; s0 < slabs; s0 += 8) { // 8 independent loads in flight, then the 8 prefix stores
            uint32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = s0 + k < slabs ? slabtot[(long long)(s0 + k) * n + b] : 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (s0 + k < slabs) slabtot[(long long)(s0 + k) * n + b] = run;
                run += v[k];
            }
        }
        tot[b] = run;
        if (run > hot_thr) { // skewed stream: list the tile, its cells will be shared by several workgroups
            const uint32_t slot = atomicAdd(&hdr->n_hot, 1u);
            if (slot < (uint32_t)kMaxHot) hdr->hot[slot] = (uint32_t)b;
        }
    }
    __syncthreads();
    const int per = (n + 1023) / 1024;
    const int b0 = tid * per;
    int b1 = b0 + per;
    if (b1 > n) b1 = n;
    uint32_t s = 0;
    for (int b = b0; b < b1; ++b) s += tot[b];
    const uint32_t inc = wave_incl_scan(s); // inclusive scan inside the wave
    if (lane == kWave - 1) wsum[wv] = inc;
    __syncthreads();
    uint32_t pre = 0;
    for (int k = 0; k < wv; ++k) pre += wsum[k];
    uint32_t run = pre + inc - s;
    for (int b = b0; b < b1; ++b) {
        base[b] = run;
        run += tot[b];
    }
    if (tid == 1023) base[n] = pre + inc;
    if (tid == 0) fold_sticky_status(hdr, hdr->status); // every error flag was OR-ed in before the first barrier above
}

// (kStageCap, stage_off and the LDS sizes: enc_plan.h)
template <int LAYOUT, int KIND, bool HAS_MAP, bool STAGED>
__global__ __launch_bounds__(kPartThreads, 8) void k_scatter(Decode P, int bpw, const uint32_t *counts,
                                                           const uint32_t *slabtot,
                                                           const uint32_t *base, uint2 *records,
                                                           WsHeader *hdr)
{
    extern __shared__ uint32_t lds[];
    // gs[n_tiles] u32 | wcnt[16][n_tiles] u16 | tag[16][n_tiles] u8
    uint32_t *gs = lds;
    uint16_t *wcnt_all = (uint16_t *)(lds + P.n_tiles);
    const int nt2 = (P.n_tiles + 1) & ~1;
    uint8_t *tag_all = (uint8_t *)(wcnt_all + (size_t)kPartWaves * nt2);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long wg = chunk_of_block(blockIdx.x, gridDim.x);
    // volatile: the tag write-then-read-back must reach LDS (another lane may have overwritten it)
    volatile uint16_t *wcnt = wcnt_all + (size_t)wv * nt2;
    volatile uint8_t *tag = tag_all + (size_t)wv * P.n_tiles;
    for (int b = tid; b < kPartWaves * nt2; b += kPartThreads) wcnt_all[b] = 0;
    __syncthreads();

    const long long wave_begin = (wg * kPartWaves + wv) * (long long)kWave * bpw;
    const uint64_t lt = lanemask_lt();
    // this workgroup's first record slot of tile `tid` (needed only in phase B: issue the loads now)
    uint32_t gs_pre = 0;
    if (tid < P.n_tiles)
        gs_pre = base[tid] + slabtot[(wg / kSlabUnits) * (long long)P.n_tiles + tid] + counts[wg * (long long)P.n_tiles + tid];
    uint32_t where[kMaxBpw]; // tile << 16 | rank in (wave, tile); 0xffffffff = not encoded
    static_assert(kWave * kMaxBpw <= 65535 && kMaxTiles <= 65536, "wcnt is uint16_t, the rank the low and the tile the high half of `where`");
    uint32_t cells[kMaxBpw / 2]; // strip-free cell of every event, two 16-bit values per register
    static_assert((kTileH << 8) * 2 <= 65536, "a cell of the widest tile fits 16 bits");
    uint2 q[kMaxBpw];
    const long long left = P.n - wave_begin;
    const uint32_t nloc = left < (long long)kWave * bpw ? (uint32_t)(left < 0 ? 0 : left) : (uint32_t)(kWave * bpw);
    if (LAYOUT == FRLW_LAYOUT_DAT8) {
        const uint2 *src = (const uint2 *)P.data + wave_begin;
#pragma unroll
        for (int j = 0; j < kMaxBpw; ++j) {
            const uint32_t i = (uint32_t)(j * kWave + lane);
            q[j] = i < nloc ? src[i] : make_uint2(0u, 0xffffffffu);
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxBpw / 2; ++j) cells[j] = 0u;
    // ---- phase A: ranks inside the wave's run, batch by batch in stream order (positions only;
    //      windows and f32 values are computed in phase C so that few registers stay live)
#pragma unroll
    for (int j = 0; j < kMaxBpw; ++j) {
        where[j] = 0xffffffffu;
        if (j < bpw) { // wave-uniform
            const uint32_t i = (uint32_t)(j * kWave + lane);
            Pos o = {-1, 0u, 0};
            if (i < nloc) {
                if (LAYOUT == FRLW_LAYOUT_DAT8) {
                    o = dat_pos<KIND, HAS_MAP>(P, q[j]);
                } else {
                    double t;
                    o = f64_pos<KIND>(P, wave_begin + i, t);
                }
            }
            const bool act = o.tile >= 0;
            cells[j >> 1] |= (o.cell & 0xffffu) << (16 * (j & 1));
            const uint64_t am = __ballot(act);
            if (am != 0ull) {
                if (act) tag[o.tile] = (uint8_t)lane;
                const int seen = act ? (int)tag[o.tile] : lane; // LDS ops of a wave execute in order
                uint64_t cm = __ballot(act && seen != lane);
                uint32_t rank = 0, size = 1;
                while (cm) {
                    const int l0 = __ffsll((long long)cm) - 1;
                    const int g = __builtin_amdgcn_readlane(o.tile, l0);
                    const uint64_t mg = __ballot(act && o.tile == g);
                    if (act && o.tile == g) {
                        rank = (uint32_t)__popcll(mg & lt);
                        size = (uint32_t)__popcll(mg);
                    }
                    cm &= ~mg;
                }
                if (act) {
                    const uint32_t r = (uint32_t)wcnt[o.tile] + rank;
                    where[j] = ((uint32_t)o.tile << 16) | r;
                    if (rank + 1 == size) wcnt[o.tile] = (uint16_t)(r + 1); // after every member's read
                }
            }
        }
    }
    __syncthreads();
    // ---- phase B: per tile, exclusive prefix of the 16 wave counts; global start of this workgroup's run
    {
        const uint32_t *row = counts + wg * (long long)P.n_tiles;
        const uint32_t *srow = slabtot + (wg / kSlabUnits) * (long long)P.n_tiles;
        for (int b = tid; b < P.n_tiles; b += kPartThreads) {
            uint32_t run = 0;
#pragma unroll
            for (int w = 0; w < kPartWaves; ++w) {
                const uint32_t v = wcnt_all[w * nt2 + b];
                wcnt_all[w * nt2 + b] = (uint16_t)run;
                run += v;
            }
            gs[b] = b == tid ? gs_pre : base[b] + srow[b] + row[b];
            if (STAGED) ((uint32_t *)((uint8_t *)lds + stage_off(P.n_tiles)))[b] = run; // loff[b] <- tile total
        }
    }
    __syncthreads();
    // ---- phase C: window + value of every encoded event (all table loads first: vmcnt also counts
    //      stores, so a load issued after a store would wait for that store), then the burst write
    const int cb = P.twl + 4;
    const uint16_t *woff = wcnt_all + (size_t)wv * nt2;
    unsigned long long wseen = 0ull; // TAF: windows this lane has encoded an event for
    uint32_t meta[kMaxBpw], valb[kMaxBpw];
#pragma unroll
    for (int j = 0; j < kMaxBpw; ++j) {
        meta[j] = 0; valb[j] = 0;
        if (j < bpw && where[j] != 0xffffffffu) {
            int window = 0;
            float val = 0.0f;
            const uint32_t cell = (cells[j >> 1] >> (16 * (j & 1))) & 0xffffu;
            if (LAYOUT == FRLW_LAYOUT_DAT8) {
                dat_value<KIND>(P, q[j], window, val);
            } else {
                const double t = ((const double *)P.data + (wave_begin + j * kWave + lane) * (long long)P.row_stride)[2];
                val = f64_value<KIND>(t);
            }
            meta[j] = ((uint32_t)window << cb) | cell;
            valb[j] = __float_as_uint(val);
            if (KIND == KIND_TAF) wseen |= 1ull << window;
        }
    }
    if (STAGED) {
        // Large streams: records go through LDS in workgroup-sorted order (tile-major) and leave in windows of
        // kStageCap consecutive slots: consecutive threads write consecutive records of a tile's run, so the stores
        // of a wave cover whole lines instead of 64 separate 8-byte pieces (HBM write traffic of the scatter: 2.6x
        // its payload with direct stores).  Small streams keep the direct stores: fewer barriers.
        uint32_t *loff = (uint32_t *)((uint8_t *)lds + stage_off(P.n_tiles)); // [n_tiles + 2]
        uint2 *stage = (uint2 *)(loff + ((P.n_tiles + 2 + 1) & ~1));
        uint16_t *stile = (uint16_t *)(stage + kStageCap);
        __shared__ uint32_t wtot[kPartWaves];
        // per-tile totals of this workgroup = prefix end of the last wave + its count: recompute from the wave
        // prefixes (woff of wave 15 + that wave's count is not kept) -> phase B left the totals in loff[]
        __syncthreads();
        uint32_t a0 = 0, a1 = 0;
        if (2 * tid < P.n_tiles) a0 = loff[2 * tid];
        if (2 * tid + 1 < P.n_tiles) a1 = loff[2 * tid + 1];
        const uint32_t inc = wave_incl_scan(a0 + a1);
        if (lane == kWave - 1) wtot[wv] = inc;
        __syncthreads();
        uint32_t pre = 0, total = 0;
        for (int k = 0; k < kPartWaves; ++k) { if (k < wv) pre += wtot[k]; total += wtot[k]; }
        const uint32_t excl = pre + inc - (a0 + a1);
        if (2 * tid < P.n_tiles) loff[2 * tid] = excl;
        if (2 * tid + 1 < P.n_tiles) loff[2 * tid + 1] = excl + a0;
        __syncthreads();
        for (uint32_t w0 = 0; w0 < total; w0 += kStageCap) {
#pragma unroll
            for (int j = 0; j < kMaxBpw; ++j) {
                if (j < bpw && where[j] != 0xffffffffu) {
                    const uint32_t b = where[j] >> 16;
                    const uint32_t slot = loff[b] + (uint32_t)woff[b] + (where[j] & 0xffffu) - w0;
                    if (slot < (uint32_t)kStageCap) { stage[slot] = make_uint2(meta[j], valb[j]); stile[slot] = (uint16_t)b; }
                }
            }
            __syncthreads();
            const uint32_t nwin = total - w0 < (uint32_t)kStageCap ? total - w0 : (uint32_t)kStageCap;
            for (uint32_t qi = tid; qi < nwin; qi += kPartThreads) {
                const uint32_t b = stile[qi];
                records[gs[b] + (w0 + qi - loff[b])] = stage[qi];
            }
            __syncthreads();
        }
    } else {
#pragma unroll
        for (int j = 0; j < kMaxBpw; ++j) {
            if (j < bpw && where[j] != 0xffffffffu) {
                const uint32_t b = where[j] >> 16;
                const uint32_t pos = gs[b] + (uint32_t)woff[b] + (where[j] & 0xffffu);
                records[pos] = make_uint2(meta[j], valb[j]);
            }
        }
    }
    if (KIND == KIND_TAF) { // which windows hold events at all: decides "all(forward)", generate_taf.py:40
        // one same-address global atomic costs ~10 ns at the L2: OR inside the wave, then inside the
        // workgroup, and touch the global word only for bits it does not show yet
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)wseen, off), hi = __shfl_xor((unsigned)(wseen >> 32), off);
            wseen |= ((unsigned long long)hi << 32) | lo;
        }
        __syncthreads(); // gs[] is dead now: reuse its first words
        unsigned long long *wg_seen = (unsigned long long *)gs;
        if (tid == 0) *wg_seen = 0ull;
        __syncthreads();
        if (lane == 0 && wseen) atomicOr(wg_seen, wseen);
        __syncthreads();
        if (tid == 0) {
            const unsigned long long mine = *wg_seen;
            const unsigned long long have = __hip_atomic_load(&hdr->wmask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (mine & ~have) atomicOr(&hdr->wmask, mine);
        }
    }
}

struct PartBufs { // the regions of the caller's workspace (Plan's offsets applied) that the four launches share
    uint32_t *counts, *slabtot, *base; uint2 *records; WsHeader *hdr; int32_t *errs; float *tlut_w;
};

template <int LAYOUT, int KIND, bool HAS_MAP>
void launch_partition(const Decode &d, const Plan &p, const PartBufs &b, hipStream_t s)
{
    const ScatterLds l = scatter_lds(p, d.n);
    hipLaunchKernelGGL((k_hist<LAYOUT, KIND, HAS_MAP>), dim3(p.units), dim3(kPartThreads), l.hist, s, d, p.bpw, b.counts, b.errs, b.tlut_w);
    hipLaunchKernelGGL(k_slabscan, dim3((p.n_tiles + kWave - 1) / kWave, p.slabs), dim3(kWave), 0, s, b.counts, p.units, p.n_tiles, b.slabtot);
    hipLaunchKernelGGL(k_tilescan, dim3(1), dim3(1024), 0, s, b.slabtot, p.slabs, p.n_tiles, b.base, b.hdr, p.hot_thr, b.errs, p.units);
    if (l.staged) {
        if (l.staged_bytes > 64 * 1024)
            (void)hipFuncSetAttribute((const void *)k_scatter<LAYOUT, KIND, HAS_MAP, true>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.staged_bytes);
        hipLaunchKernelGGL((k_scatter<LAYOUT, KIND, HAS_MAP, true>), dim3(p.units), dim3(kPartThreads), l.staged_bytes, s, d, p.bpw,
                           b.counts, b.slabtot, b.base, b.records, b.hdr);
    } else {
        hipLaunchKernelGGL((k_scatter<LAYOUT, KIND, HAS_MAP, false>), dim3(p.units), dim3(kPartThreads), l.direct, s, d, p.bpw,
                           b.counts, b.slabtot, b.base, b.records, b.hdr);
    }
}

// event layout x encoder kind x coordinate maps -> the kernels' instances (the f64 layout has no maps: no such instance)
template <int LAYOUT>
void dispatch_partition(int kind, const Decode &d, const Plan &p, const PartBufs &b, hipStream_t s)
{
    const auto go = [&](auto k) {
        constexpr int KIND = decltype(k)::value;
        if constexpr (LAYOUT == FRLW_LAYOUT_DAT8) {
            if (d.xmap) return launch_partition<LAYOUT, KIND, true>(d, p, b, s);
        }
        launch_partition<LAYOUT, KIND, false>(d, p, b, s);
    };
    switch (kind) {
    case KIND_ECI: go(std::integral_constant<int, KIND_ECI>{}); break;
    case KIND_EV: go(std::integral_constant<int, KIND_EV>{}); break;
    case KIND_SAE: go(std::integral_constant<int, KIND_SAE>{}); break;
    default: go(std::integral_constant<int, KIND_TAF>{}); break;
    }
}
} // namespace

int partition_events(const frlw_events_t *ev, int H, int W, int kind, long long t0, long long win, int n_windows, int time_filter,
                     void *ws, size_t ws_bytes, hipStream_t s, Partitioned &out)
{
    if (!ev || !ws || (ev->n > 0 && !ev->data)) return FRLW_ERR_ARG;
    if (ev->layout != FRLW_LAYOUT_XYTP_F64 && ev->layout != FRLW_LAYOUT_DAT8) return FRLW_ERR_ARG;
    if (ev->layout == FRLW_LAYOUT_XYTP_F64 && ev->row_stride < 4) return FRLW_ERR_ARG;
    if ((ev->xmap == nullptr) != (ev->ymap == nullptr)) return FRLW_ERR_ARG;
    if (!tuning_valid(ev->tuning)) return FRLW_ERR_ARG;
    if (ev->n >= (1ll << 32)) return FRLW_ERR_UNSUPPORTED;
    if (win < 1) win = 1;
    if (kind == KIND_TAF && ev->layout == FRLW_LAYOUT_DAT8 &&
        ((long long)n_windows * win >= (1ll << 32) || win >= (1ll << 31)))
        return FRLW_ERR_UNSUPPORTED;
    Plan p;
    if (!make_plan(ev->n, H, W, ev->tuning, p)) return FRLW_ERR_UNSUPPORTED;
    if (ws_bytes < p.bytes) return FRLW_ERR_WORKSPACE;
    char *w8 = (char *)ws;
    PartBufs b = {(uint32_t *)(w8 + p.off_counts), (uint32_t *)(w8 + p.off_slabtot), (uint32_t *)(w8 + p.off_base),
                  (uint2 *)(w8 + p.off_records), (WsHeader *)w8, (int32_t *)(w8 + p.off_errs), nullptr};
    Decode d;
    d.data = ev->data; d.n = ev->n; d.row_stride = ev->row_stride;
    d.xmap = ev->layout == FRLW_LAYOUT_DAT8 ? ev->xmap : nullptr;
    d.ymap = ev->layout == FRLW_LAYOUT_DAT8 ? ev->ymap : nullptr;
    d.map_w = ev->map_w; d.map_h = ev->map_h;
    d.H = H; d.W = W; d.twl = p.twl; d.tiles_x = p.tiles_x; d.n_tiles = p.n_tiles;
    d.t0 = t0; d.win = win; d.n_windows = n_windows; d.time_filter = time_filter;
    const unsigned long long magic = (1ull << 32) / (unsigned long long)win;
    d.win_magic = magic > 0xffffffffull ? 0xffffffffu : (uint32_t)magic;
    if (kind == KIND_TAF && ev->layout == FRLW_LAYOUT_DAT8 && win <= kMaxTlut && !p.no_lut) b.tlut_w = (float *)(w8 + p.off_tlut);
    d.tlut = b.tlut_w;
    const uint32_t *leaky = nullptr; // level thresholds of uint8(leaky_transform(.)) for the tile kernel's epilogue (generate_taf.py:69-76)
    if (kind == KIND_TAF && !(leaky = leaky_table(s))) return FRLW_ERR_HIP;

    (void)hipGetLastError(); // stale errors of other libraries in the process
    if (ev->layout == FRLW_LAYOUT_DAT8) dispatch_partition<FRLW_LAYOUT_DAT8>(kind, d, p, b, s);
    else dispatch_partition<FRLW_LAYOUT_XYTP_F64>(kind, d, p, b, s);
    HIP_TRY(hipGetLastError());
    out.records = b.records; out.base = b.base; out.hdr = b.hdr; out.plan = p; out.leaky_thr = leaky;
    return FRLW_OK;
}

} // namespace frlw
