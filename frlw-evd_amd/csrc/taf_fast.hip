// taf_fast.hip -- the fast Temporal Active Focus path: a batch of independent, in-span DAT streams.
//
// Replaces, for B sequences at once, the harness loop generate_taf.py:193-235 around taf_cuda (:19-58): window
// selection, f64 time normalisation, per-window count / mean-time accumulation, K-deep FIFO ageing, leaky transform,
// uint8 truncation.  Same contract as the general path (encoders.hip): f32 sums in STREAM ORDER, bit for bit.
//
// What makes it fast (measured reasons in DESIGN.md section 3):
//   * 4-byte records {r | window | cell}: r = t - window start (the f32 value is tlut[r], one table of win + 1
//     floats), 12-bit cell inside a 4096-cell tile.  Half the record traffic of the general path.
//   * the stable partition ranks a batch of 64 consecutive events with ONE returning LDS atomic per event: gfx950
//     serves the lanes of a wave-instruction that hit one LDS address in ascending lane order (tools/lds_order_test.hip,
//     tests/test_taf_fast_gpu.py::test_lds_atomic_lane_order), so the returned value IS the stream rank.
//   * the records of a tile (4096 cells) are split once more, stably, by sub-tile of 256 cells (kf_split_whole; tiles
//     that hold a large share of the stream are cut into segments of 8192 records with one workgroup each,
//     kf_split_place), so skew costs more workgroups, not a longer critical path.
//   * the sums of different windows do not depend on each other -- only the FIFO steps that consume them are
//     sequential.  kf_taf_walk gives a sub-tile to eight wavefronts that take ONE WINDOW EACH: tickets from per-cell
//     LDS counters (the same lane-ordered atomic) turn the window's records into per-cell segments without any
//     ordering pass, owner lanes add each segment front to back (the reference's sequential index_add_), and the FIFO
//     steps follow with one cell per lane.
//   * sequences of a batch are independent problems in one launch sequence: own tiles, own window mask
//     (generate_taf.py:40-41 is a per-sequence rule), own t_start.
//
// Requirements, checked on device (violations -> status, NOTHING is written, the caller falls back to frlw_taf_encode):
// every event inside [t_start, t_start + n_windows * window_us] of its sequence and inside the frame.
//
// The files (each says in its first lines what it holds and expects): taf_plan.h the host planner (no HIP: tested on the CPU),
// taf_decode.h records, taf_partition.h both partitions, taf_column.h a bin's column of the chunk-major directory, taf_split.h the
// second level, taf_walk.h kf_taf_walk, ev_fast.h / sae_fast.h the Event Volume and SAE / Event Count Image consumers, ev_ranges.h the
// gather in front of the Event Volume batch for windows given as record ranges (frlw_ev_encode_ranges).  Here: the
// lane-order self-test, the launch helpers and the C entry points.

#include "ev_fast.h"
#include "ev_ranges.h"
#include "sae_fast.h"
#include "taf_walk.h"

#include <atomic>

using namespace frlw;

namespace {

// Self-test of the two hardware properties this file rests on, for lanes of ONE wave-instruction that hit the same LDS
// address: (1) a returning integer atomic serves them in ascending lane order (the returned count is the stream rank);
// (2) ds_add_f32 applies them in ascending lane order with the rounding of v_add_f32, i.e. it IS the sequential
// `sum = sum + v` of the lanes.  Random addresses and values in (-1, 0]; reference by counting / adding over lower lanes.
__global__ __launch_bounds__(kFT) void kf_selftest_lane_order(int n_addr, int iters, unsigned long long *out)
{
    extern __shared__ uint32_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t *mine = lds + (size_t)wv * 3 * n_addr;
    float *facc = (float *)(mine + n_addr);  // accumulated by the atomic
    float *fref = facc + n_addr;             // accumulated sequentially, lane by lane
    unsigned long long bad = 0, conf = 0, fbad = 0;
    for (int a = lane; a < n_addr; a += kWave) { facc[a] = 0.0f; fref[a] = 0.0f; }
    for (int it = 0; it < iters; ++it) {
        for (int a = lane; a < n_addr; a += kWave) mine[a] = 0;
        LDS_FENCE();
        uint32_t h = (blockIdx.x * (uint32_t)kFT + tid) * 2654435761u + it * 40503u;
        h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
        const uint32_t addr = h % (uint32_t)n_addr;
        const float v = (float)((double)(h >> 8 & 16383u) / 10000.00000001) - 1.0f; // the shape of the TAF values
        const uint32_t got = atomicAdd(&mine[addr], 1u);
        atomicAdd(&facc[addr], v);
        uint32_t want = 0;
        for (int l = 0; l < kWave; ++l) {
            const uint32_t other = __shfl(addr, l);
            const float ov = __shfl(v, l);
            if (l < lane && other == addr) ++want;
            LDS_FENCE();
            if (l == lane) ((volatile float *)fref)[addr] = ((volatile float *)fref)[addr] + ov;
            LDS_FENCE();
        }
        if (got != want) ++bad;
        if (want) ++conf;
        LDS_FENCE();
        if (__float_as_uint(((volatile float *)facc)[addr]) != __float_as_uint(((volatile float *)fref)[addr])) ++fbad;
        LDS_FENCE();
        if ((it & 7) == 7) // let the sums grow over 8 batches, then start again
            for (int a = lane; a < n_addr; a += kWave) { facc[a] = 0.0f; fref[a] = 0.0f; }
    }
    if (bad) atomicAdd(&out[0], bad);
    if (conf) atomicAdd(&out[1], conf);
    if (fbad) atomicAdd(&out[2], fbad);
}

// one instance of the bin-major scatter: the dynamic-LDS attribute where the chunk needs more than the default 64 KB, then the launch
template <bool HAS_MAP, bool EV, bool SIMPLE>
void launch_scatter(const FastGeom &G, const SeqTab &S, const FastPlan &p, char *w8, hipStream_t st)
{
    const size_t lds_sc = scatter_lds_bytes(p.TB, p.chunk);
    if (lds_sc > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)kf_scatter<HAS_MAP, EV, SIMPLE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sc);
    hipLaunchKernelGGL((kf_scatter<HAS_MAP, EV, SIMPLE>), dim3(p.chunks), dim3(kFT), lds_sc, st, G, S, (const uint32_t *)(w8 + p.off_counts),
                       (const uint32_t *)(w8 + p.off_slabtot), (const uint32_t *)(w8 + p.off_base), (uint32_t *)(w8 + p.off_records), (FastHeader *)w8);
}

// the histogram partition: kf_hist, the scans, kf_scatter
template <bool HAS_MAP, bool EV = false>
void launch_fast(const FastGeom &G, const SeqTab &S, const FastPlan &p, char *w8, hipStream_t st)
{
    FastHeader *hdr = (FastHeader *)w8;
    uint32_t *counts = (uint32_t *)(w8 + p.off_counts);
    uint32_t *slabtot = (uint32_t *)(w8 + p.off_slabtot);
    int32_t *errs = (int32_t *)(w8 + p.off_errs);
    float *tlut = (float *)(w8 + p.off_tlut);
    const int hist_grid = p.chunks < 512 ? p.chunks : 512; // persistent: two workgroups per CU
    const bool simple = !HAS_MAP && G.simple != 0;
    if (simple)
        hipLaunchKernelGGL((kf_hist<false, EV, true>), dim3(hist_grid), dim3(kFT), (size_t)p.TB * 4, st, G, S, counts, errs, tlut, p.chunks);
    else
        hipLaunchKernelGGL((kf_hist<HAS_MAP, EV>), dim3(hist_grid), dim3(kFT), (size_t)p.TB * 4, st, G, S, counts, errs, tlut, p.chunks);
    const bool inline_slabs = (long long)p.slabs * p.TB <= kInlineSlabScan;
    if (!inline_slabs)
        hipLaunchKernelGGL(kf_slabscan, dim3((p.TB + kWave - 1) / kWave, p.slabs), dim3(kWave), 0, st, S, counts, p.TB, slabtot);
    hipLaunchKernelGGL(kf_tilescan, dim3(1), dim3(kFT), 0, st, S, slabtot, p.TB, (uint32_t *)(w8 + p.off_base), (uint32_t *)(w8 + p.off_seg0), hdr, errs,
                       p.chunks, inline_slabs ? counts : (uint32_t *)nullptr, p.slabs, p.direct);
    if (simple) launch_scatter<false, EV, true>(G, S, p, w8, st);
    else launch_scatter<HAS_MAP, EV, false>(G, S, p, w8, st);
}

// the captured form's header reset (status, window masks, cursors): see cm_epoch
__global__ __launch_bounds__(256) void kf_header_reset(FastHeader *hdr)
{
    uint32_t *h32 = (uint32_t *)hdr;
    for (int i = threadIdx.x; i < (int)(offsetof(FastHeader, epoch) / 4); i += 256) h32[i] = 0u;
    if (threadIdx.x == 0) *(uint32_t *)((char *)hdr + kStallOffset) = 0u; // (the captured form has no wait and no stall of its own)
}

// The epoch kf_scatter_cm's first workgroup publishes behind its header reset: the next value of `counter`, with `range` OR-ed in
// (the SAE path keeps a range of its own: never equal to a TAF / Event Volume call's epoch of the same process ... within 2^30
// calls), never 0.
// Inside a stream capture the kernel arguments are frozen into the graph node: a host-made epoch would already be the
// published one on every replay after the first (workgroups could then OR their flags into the header BEFORE workgroup 0
// zeroes it).  A captured call resets the header with a kernel node of its own and passes epoch 0 = "nobody resets, nobody waits".
// (a kernel node, not hipMemsetAsync: a captured memset node of this runtime wrote a stale pattern into the header from its
// second replay on -- measured; tests/test_taf_fast_gpu.py replays a captured encode three times)
uint32_t cm_epoch(std::atomic<uint32_t> &counter, uint32_t range, FastHeader *hdr, hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    if (cap != hipStreamCaptureStatusNone) {
        hipLaunchKernelGGL(kf_header_reset, dim3(1), dim3(256), 0, st, hdr);
        return 0u;
    }
    uint32_t epoch = (counter.fetch_add(1u, std::memory_order_relaxed) + 1u) | range;
    if (epoch == 0u) epoch = (counter.fetch_add(1u, std::memory_order_relaxed) + 1u) | range; // (0 = the captured form)
    return epoch;
}

// one instance of the chunk-major scatter: the dynamic-LDS attribute where it is needed (always for the one-workgroup-per-CU
// form), then the launch.  tlut: the per-call value table the kernel fills on the side, or NULL (SAE / Event Count Image)
template <bool HAS_MAP, bool EV, bool SIMPLE, int MAXB = kMaxBpw, int SAE = 0>
void launch_scatter_cm(const FastGeom &G, const SeqTab &S, const FastPlan &p, char *w8, float *tlut, uint32_t epoch, hipStream_t st)
{
    const size_t lds_sc = scatter_cm_lds_bytes(p.TB, p.chunk);
    if (MAXB > kMaxBpw || lds_sc > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)kf_scatter_cm<HAS_MAP, EV, SIMPLE, MAXB, SAE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sc);
    hipLaunchKernelGGL((kf_scatter_cm<HAS_MAP, EV, SIMPLE, MAXB, SAE>), dim3(p.chunks), dim3(kFT), lds_sc, st, G, S, (uint32_t *)(w8 + p.off_counts),
                       (uint32_t *)(w8 + p.off_records), (FastHeader *)w8, tlut, epoch);
}

// the chunk-major partition: ONE kernel (its first workgroup resets the header; a reset kernel in front of it inside a capture)
template <bool HAS_MAP, bool EV = false>
void launch_fast_cm(const FastGeom &G, const SeqTab &S, const FastPlan &p, char *w8, hipStream_t st)
{
    static std::atomic<uint32_t> g_epoch{0};
    const uint32_t epoch = cm_epoch(g_epoch, 0u, (FastHeader *)w8, st);
    float *tlut = (float *)(w8 + p.off_tlut);
    const bool simple = !HAS_MAP && G.simple != 0;
    if (p.big && simple) launch_scatter_cm<false, EV, true, kBigBpw>(G, S, p, w8, tlut, epoch, st);
    else if (p.big) launch_scatter_cm<HAS_MAP, EV, false, kBigBpw>(G, S, p, w8, tlut, epoch, st);
    else if (simple) launch_scatter_cm<false, EV, true>(G, S, p, w8, tlut, epoch, st);
    else launch_scatter_cm<HAS_MAP, EV, false>(G, S, p, w8, tlut, epoch, st);
}

// the first level of a batch call: either partition, with or without coordinate maps
template <bool EV>
void launch_partition(const FastGeom &G, const SeqTab &S, const FastPlan &p, bool cm, char *w8, hipStream_t st)
{
    if (cm) { if (G.xmap) launch_fast_cm<true, EV>(G, S, p, w8, st); else launch_fast_cm<false, EV>(G, S, p, w8, st); }
    else if (G.xmap) launch_fast<true, EV>(G, S, p, w8, st);
    else launch_fast<false, EV>(G, S, p, w8, st);
}

// The argument checks the two batch entry points share (their own -- outputs, K / bins, window counts: all FRLW_ERR_ARG -- come
// in front of this).  t0: the per-sequence t_start / t_end array.
int batch_args_check(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t0, int n_seq, const void *workspace)
{
    if (!ev || !seq_offsets || !t0 || !workspace) return FRLW_ERR_ARG;
    if (n_seq < 1 || n_seq > kMaxSeq) return FRLW_ERR_ARG;
    if (ev->layout != FRLW_LAYOUT_DAT8) return FRLW_ERR_UNSUPPORTED;
    if ((ev->xmap == nullptr) != (ev->ymap == nullptr)) return FRLW_ERR_ARG;
    if (!tuning_valid(ev->tuning)) return FRLW_ERR_ARG;
    if (seq_offsets[0] < 0 || seq_offsets[n_seq] > ev->n) return FRLW_ERR_ARG;
    if (seq_offsets[n_seq] > seq_offsets[0] && !ev->data) return FRLW_ERR_ARG;
    return FRLW_OK;
}

// plan + layout of one batch call (tries the chunk-major plan first where the knob allows it), then what both entry points
// ask of the result: the workspace holds it, the scatter workgroup's LDS exists
inline int plan_call(const frlw_tuning_t *tu, bool ev, int n_seq, int H, int W, const int64_t *seq_offsets,
                     const int64_t *t0, int64_t window_us, size_t workspace_bytes, FastPlan &p, SeqTab &S, bool &cm)
{
    const int rc = plan_select(tuning_knob(tu, &frlw_tuning_t::chunk_major, CM_AUTO), tuning_knob(tu, &frlw_tuning_t::batches_per_wave, 0),
                               tuning_knob(tu, &frlw_tuning_t::direct_bins, -1), ev, n_seq, H, W, seq_offsets, t0, window_us, p, S, cm);
    if (rc != FRLW_OK) return rc;
    if (workspace_bytes < p.bytes) return FRLW_ERR_WORKSPACE;
    if (scatter_lds_bytes(p.TB, p.chunk) > 160 * 1024) return FRLW_ERR_UNSUPPORTED;
    return FRLW_OK;
}

// The FastGeom fields that come from the plan and the event descriptor, as a whole-frame call of ONE window; an entry point
// adds what is its own: windows (n_windows, wb, win, win_magic), rcp, simple / span, the stripe rows.
inline FastGeom plan_geom(const frlw_events_t *ev, const FastPlan &p, int H, int W)
{
    FastGeom G = {};
    G.data = (const uint2 *)ev->data;
    G.xmap = ev->xmap; G.ymap = ev->ymap; G.map_w = ev->map_w; G.map_h = ev->map_h;
    G.H = H; G.W = W; G.twl = p.twl; G.thl = p.thl; G.tiles_x = p.tiles_x; G.T = p.TB; G.bin_shift = p.bin_shift; G.bin_mask = p.direct ? 15 : 0; G.bpw = p.bpw;
    G.chunk_ev = p.chunk; G.run = p.chunk / kFW; G.n_total = ev->n;
    G.n_windows = 1; G.y_lo = 0; G.H_full = H;
    return G;
}

// every sequence's t0 inside the 32-bit range of the SIMPLE decode
inline bool t0_fits_simple(const SeqTab &S)
{
    for (int s = 0; s < S.n_seq; ++s)
        if (S.t0[s] < 0 || S.t0[s] > 0xffffffffll) return false;
    return true;
}

inline CmP cm_params(const FastPlan &p, char *w8)
{
    CmP cm;
    cm.dir = (const uint32_t *)(w8 + p.off_counts);
    cm.rec = (const uint32_t *)(w8 + p.off_records);
    cm.TB = p.TB;
    cm.n_chunks = p.chunks;
    cm.chunk_ev = p.chunk;
    cm.hot_start = (uint32_t *)(w8 + p.off_base);
    cm.hot_seg0 = (uint32_t *)(w8 + p.off_seg0);
    cm.segdesc = (uint32_t *)(w8 + p.off_segdesc);
    cm.max_segs = p.max_segs;
    return cm;
}

// The second level, for TAF and Event Volume: fills the partition-table fields of q and brings the records sub-tile-major --
// afterwards q.rec2 / q.sub / q.sub_end describe one contiguous list per sub-tile.  The four forms:
//   chunk-major + direct  nothing runs here: the consumers gather their own lists (and book space in rec2[] for the long ones)
//   chunk-major           kf_split_whole<true>, then the segment kernels for the skewed tiles it booked
//   direct                kf_scatter's bins were the sub-tiles: its output IS the sub-tile-major list, base[] its sub[]
//   histogram             kf_split_whole<false> (tiles, then segment counts in its spare workgroups) + kf_split_place<false>
// The caller has set what is its own (geometry, outputs, TAF: wst / wst_flag for the chunk-major form).
void launch_second_level(TileP &q, const FastPlan &p, const SeqTab &S, bool cm, char *w8, hipStream_t st)
{
    q.T = p.T; q.pairs = p.pairs; q.direct = p.direct;
    q.hdr = (FastHeader *)w8;
    q.rec = (const uint32_t *)(w8 + p.off_records);
    q.rec2 = (uint32_t *)(w8 + p.off_records2);
    q.base = (const uint32_t *)(w8 + p.off_base);
    q.sub = (uint32_t *)(w8 + p.off_sub);
    q.sub_end = nullptr;
    q.seg0 = (const uint32_t *)(w8 + p.off_seg0);
    q.segcnt = (uint32_t *)(w8 + p.off_segcnt);
    q.seg_grid = p.max_segs < 2048 ? p.max_segs : 2048;
    q.tile_max = whole_max_of(p.pairs);
    if (cm && p.direct) return;
    if (cm) {
        const CmP cmq = cm_params(p, w8);
        q.sub_end = (uint32_t *)(w8 + p.off_sub_end);
        const int seg_grid = p.max_segs < 512 ? p.max_segs : 512; // (they stride over the segments; most calls have none; two workgroups per CU)
        hipLaunchKernelGGL(kf_split_whole<true>, dim3(p.pairs), dim3(kFT), 0, st, q, cmq, S);
        hipLaunchKernelGGL(kf_segcount_cm, dim3(seg_grid), dim3(kFT), 0, st, q, cmq, S);
        hipLaunchKernelGGL(kf_split_place<true>, dim3(seg_grid), dim3(kFT), 0, st, q, cmq, S);
    } else if (p.direct) {
        q.rec2 = (uint32_t *)(w8 + p.off_records);
        q.sub = (uint32_t *)(w8 + p.off_base);
    } else {
        const CmP none = {};
        hipLaunchKernelGGL(kf_split_whole<false>, dim3(p.pairs + q.seg_grid), dim3(kFT), 0, st, q, none, S);
        hipLaunchKernelGGL(kf_split_place<false>, dim3(q.seg_grid), dim3(kFT), 0, st, q, none, S);
    }
}

// ---- one-time check of the hardware property this file rests on ------------------------------------------------------
// 0 = not yet tested on this device, 1 = lanes of one returning LDS atomic are served in lane order, 2 = they are not
// (a new stepping / compiler): the fast path then refuses (FRLW_ERR_UNSUPPORTED) and callers take the general path.
constexpr int kMaxDevices = 64;
std::atomic<int> g_lds_order[kMaxDevices];
std::atomic<int> g_lds_fadd[kMaxDevices]; // 1: ds_add_f32 made the sequential f32 sums in the same self-test run (kf_ev_fadd may be used)

int lds_order_ok(char *w8, hipStream_t st)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return FRLW_ERR_HIP;
    int have = g_lds_order[dev].load(std::memory_order_acquire);
    if (have == 0) {
        // first fast-path call on this device: 256 workgroups x 64 rounds of conflicting lanes (~3e5 conflicting lane
        // pairs), result into the spare bytes of the workspace header, ONE host synchronisation for the process lifetime
        unsigned long long *out = (unsigned long long *)(w8 + kSelftestOffset);
        unsigned long long host[3] = {1ull, 0ull, 0ull};
        (void)hipFuncSetAttribute((const void *)kf_selftest_lane_order, hipFuncAttributeMaxDynamicSharedMemorySize, kFW * 512 * 12);
        HIP_TRY(hipMemsetAsync(out, 0, 24, st));
        hipLaunchKernelGGL(kf_selftest_lane_order, dim3(256), dim3(kFT), (size_t)kFW * 40 * 12, st, 40, 64, out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, out, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        have = (host[0] == 0ull && host[1] > 0ull) ? 1 : 2; // no rank violation among > 0 conflicting pairs
        g_lds_fadd[dev].store((host[2] == 0ull && host[1] > 0ull) ? 1 : 0, std::memory_order_release);
        g_lds_order[dev].store(have, std::memory_order_release);
    }
    return have == 1 ? FRLW_OK : FRLW_ERR_UNSUPPORTED;
}

} // namespace

extern "C" {

#if defined(FRLW_WALK_PROF) || defined(FRLW_SCAT_PROF)
int frlw_debug_walk_prof(unsigned long long *out16)
{
    static unsigned long long host[kProfWgs * 9];
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_walk_prof), sizeof(host)) != hipSuccess) return FRLW_ERR_HIP;
    for (int i = 0; i < 16; ++i) out16[i] = 0;
    for (int w = 0; w < kProfWgs; ++w) {
        if (host[w * 9 + 8] == 0 && host[w * 9] == 0) continue;
        ++out16[15];
        for (int i = 0; i < 9; ++i) out16[i] += host[w * 9 + i];
    }
    void *dev = nullptr;
    if (hipGetSymbolAddress(&dev, HIP_SYMBOL(g_walk_prof)) != hipSuccess || hipMemset(dev, 0, sizeof(host)) != hipSuccess) return FRLW_ERR_HIP;
    return FRLW_OK;
}
#endif

#ifdef FRLW_DEV_BUILD // not in the product library: a process-wide switch has no place in its ABI
int frlw_debug_force_lds_order(int value)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return FRLW_ERR_HIP;
    if (value < -1 || value > 1) return FRLW_ERR_ARG;
    g_lds_order[dev].store(value < 0 ? 0 : (value == 1 ? 1 : 2), std::memory_order_release);
    return FRLW_OK;
}
#endif

int frlw_fast_path_verdict(void *workspace, size_t workspace_bytes, frlw_stream_t stream, int *ok_out)
{
    if (!workspace || workspace_bytes < kHeaderBytes || !ok_out) return FRLW_ERR_ARG;
    (void)hipGetLastError();
    const int rc = lds_order_ok((char *)workspace, (hipStream_t)stream); // runs the self-test on the first call per device, cached afterwards
    if (rc != FRLW_OK && rc != FRLW_ERR_UNSUPPORTED) return rc;
    *ok_out = rc == FRLW_OK ? 1 : 0;
    return FRLW_OK;
}

int frlw_selftest_lds_atomic_order(int n_addr, int iters, unsigned long long *out_dev, frlw_stream_t stream)
{
    if (!out_dev || n_addr < 1 || n_addr > 512 || iters < 1) return FRLW_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    (void)hipFuncSetAttribute((const void *)kf_selftest_lane_order, hipFuncAttributeMaxDynamicSharedMemorySize,
                              kFW * 512 * 12);
    HIP_TRY(hipMemsetAsync(out_dev, 0, 24, st));
    hipLaunchKernelGGL(kf_selftest_lane_order, dim3(256), dim3(kFT), (size_t)kFW * n_addr * 12, st, n_addr, iters, out_dev);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

size_t frlw_taf_batch_workspace_bytes(int64_t n_events, int n_seq, int H, int W, int64_t window_us)
{
    return batch_workspace_bytes(n_events, n_seq, H, W, window_us);
}

} // extern "C"

namespace {
enum : int { PHASE_PARTITION = 1, PHASE_FINISH = 2 };

// The batch encode in two halves: PARTITION = kf_hist, scans, kf_scatter (leaves the per-sequence window masks in the
// workspace header), FINISH = split + walk (reads them).  A row stripe [y_lo, y_lo + H) of an H_full-row frame runs the two
// halves as separate calls with an OR-reduce of the masks over the stripes in between (frlw_taf_stripe_*).
int taf_batch_run(int phases, const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_start, int n_seq, int H, int W,
                  int y_lo, int H_full, int K, int64_t window_us, int n_windows, float *state, float *view_f32, uint8_t *out_u8,
                  int flags, void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    if (!state && (phases & PHASE_FINISH)) return FRLW_ERR_ARG;
    if (y_lo < 0 || H < 1 || y_lo + H > H_full) return FRLW_ERR_ARG;
    if (K < 1 || K > FRLW_MAX_BINS || n_windows < 1 || n_windows > FRLW_MAX_WINDOWS || window_us < 1) return FRLW_ERR_ARG;
    {
        const int rc = batch_args_check(ev, seq_offsets, t_start, n_seq, workspace);
        if (rc != FRLW_OK) return rc;
    }
    // record = r | window | cell in 32 bits
    int wb = 0, rb = 0;
    while ((1 << wb) < n_windows) ++wb;
    while ((1ll << rb) <= window_us) ++rb;
    if (kCellBits + wb + rb > 32 || (long long)n_windows * window_us >= (1ll << 32)) return FRLW_ERR_UNSUPPORTED;
    FastPlan p;
    SeqTab S;
    bool cm = false;
    {
        const int rc = plan_call(ev->tuning, false, n_seq, H, W, seq_offsets, t_start, window_us, workspace_bytes, p, S, cm);
        if (rc != FRLW_OK) return rc;
    }

    FastGeom G = plan_geom(ev, p, H, W);
    G.n_windows = n_windows; G.wb = wb; G.win = (uint32_t)window_us;
    G.rcp = 1.0 / ((double)(uint32_t)window_us + 1e-8); // generate_taf.py:215: t / (w + 1e-8)
    G.y_lo = y_lo; G.H_full = H_full;
    const unsigned long long magic = (1ull << 32) / (unsigned long long)window_us;
    G.win_magic = magic > 0xffffffffull ? 0xffffffffu : (uint32_t)magic;
    G.simple = (y_lo == 0 && H_full == H && window_us >= 2 &&
                (unsigned long long)n_windows * (unsigned long long)window_us <= 0xffffffffull && t0_fits_simple(S)) ? 1 : 0;
    G.span = G.simple ? (uint32_t)((unsigned long long)n_windows * (unsigned long long)window_us) : 0u;
    G.m24 = (G.simple && G.span < (1u << 24) && G.win_magic < (1u << 24)) ? 1 : 0;

    hipStream_t st = (hipStream_t)stream;
    char *w8 = (char *)workspace;
    (void)hipGetLastError();
    {
        const int ok = lds_order_ok(w8, st); // cached per device after the first call
        if (ok != FRLW_OK) return ok;
    }
    if (phases & PHASE_PARTITION) launch_partition<false>(G, S, p, cm, w8, st);
    if (!(phases & PHASE_FINISH)) { HIP_TRY(hipGetLastError()); return FRLW_OK; }
    TileP q = {};
    q.H = H; q.W = W; q.twl = p.twl; q.thl = p.thl; q.tiles_x = p.tiles_x; q.K = K; q.n_windows = n_windows;
    q.wb = wb; q.flip = (flags & FRLW_TAF_U8_FLIP_K) ? 1 : 0; q.win = (uint32_t)window_us; q.rcp = G.rcp;
    q.tlut = (const float *)(w8 + p.off_tlut);
    if (!(q.leaky_thr = leaky_table(st))) return FRLW_ERR_HIP; // device-resident constant, built once per device (leaky.hip)
    q.state = state; q.view_f32 = view_f32; q.out_u8 = out_u8;
    if (cm && !p.direct && tuning_knob(ev->tuning, &frlw_tuning_t::walk_window_table, 1) != 0) { // kf_split_whole<true> leaves the walk its window starts
        q.wst = (uint32_t *)(w8 + p.off_wst);
        q.wst_flag = (uint32_t *)(w8 + p.off_wst_flag);
    }
    launch_second_level(q, p, S, cm, w8, st);
    const CmP cmq = cm ? cm_params(p, w8) : CmP{};
    if (cm && p.direct) { // the walk gathers its own list (no gather kernel)
        if (K == 8) hipLaunchKernelGGL((kf_taf_walk<true, true>), dim3(p.pairs * kFW), dim3(kWalkThreads), 0, st, q, cmq, S);
        else hipLaunchKernelGGL((kf_taf_walk<false, true>), dim3(p.pairs * kFW), dim3(kWalkThreads), 0, st, q, cmq, S);
    } else if (K == 8) hipLaunchKernelGGL((kf_taf_walk<true, false>), dim3(p.pairs * kFW), dim3(kWalkThreads), 0, st, q, cmq, S);
    else hipLaunchKernelGGL((kf_taf_walk<false, false>), dim3(p.pairs * kFW), dim3(kWalkThreads), 0, st, q, cmq, S);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}
} // namespace

extern "C" {

int frlw_taf_encode_batch(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_start, int n_seq, int H,
                          int W, int K, int64_t window_us, int n_windows, float *state, float *view_f32, uint8_t *out_u8,
                          int flags, void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    return taf_batch_run(PHASE_PARTITION | PHASE_FINISH, ev, seq_offsets, t_start, n_seq, H, W, 0, H, K, window_us, n_windows, state,
                         view_f32, out_u8, flags, workspace, workspace_bytes, stream);
}

int frlw_taf_stripe_partition(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_start, int n_seq, int H_full,
                              int W, int y_lo, int rows, int K, int64_t window_us, int n_windows, void *workspace,
                              size_t workspace_bytes, frlw_stream_t stream)
{
    return taf_batch_run(PHASE_PARTITION, ev, seq_offsets, t_start, n_seq, rows, W, y_lo, H_full, K, window_us, n_windows, nullptr,
                         nullptr, nullptr, 0, workspace, workspace_bytes, stream);
}

unsigned long long *frlw_taf_stripe_window_masks(void *workspace)
{
    return workspace ? ((FastHeader *)workspace)->wmask : nullptr;
}

int frlw_taf_stripe_finish(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_start, int n_seq, int H_full, int W,
                           int y_lo, int rows, int K, int64_t window_us, int n_windows, float *state, float *view_f32,
                           uint8_t *out_u8, int flags, void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    return taf_batch_run(PHASE_FINISH, ev, seq_offsets, t_start, n_seq, rows, W, y_lo, H_full, K, window_us, n_windows, state, view_f32,
                         out_u8, flags, workspace, workspace_bytes, stream);
}

size_t frlw_ev_batch_workspace_bytes(int64_t n_events, int n_seq, int H, int W, int64_t window_us)
{
    return frlw_taf_batch_workspace_bytes(n_events, n_seq, H, W, window_us); // same partition, same tables
}

} // extern "C"

namespace {
// The body of frlw_ev_encode_batch; frlw_ev_encode_ranges runs it on its copy of the windows' records.
int ev_batch_run(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_end, int n_seq, int H, int W,
                 int bins, int64_t window_us, float *out_f32, uint8_t *out_u8, void *workspace,
                 size_t workspace_bytes, frlw_stream_t stream, const RangeTab *gather = nullptr, const uint2 *gather_src = nullptr)
{
    if (!out_f32 && !out_u8) return FRLW_ERR_ARG;
    if (bins < 1 || bins > FRLW_MAX_BINS || window_us < 1) return FRLW_ERR_ARG;
    {
        const int rc = batch_args_check(ev, seq_offsets, t_end, n_seq, workspace);
        if (rc != FRLW_OK) return rc;
    }
    int rb = 0; // record = (t - t_begin) | cell in 32 bits
    while ((1ll << rb) <= window_us) ++rb;
    if (kCellBits + rb > 32) return FRLW_ERR_UNSUPPORTED;
    const long long n = seq_offsets[n_seq] - seq_offsets[0];
    FastPlan p;
    SeqTab S;
    int64_t t_begin[kMaxSeq];
    for (int s = 0; s < n_seq; ++s) t_begin[s] = t_end[s] - window_us; // generate_eventvolume.py:139-141
    bool cm = false;
    {
        const int rc = plan_call(ev->tuning, true, n_seq, H, W, seq_offsets, t_begin, window_us, workspace_bytes, p, S, cm);
        if (rc != FRLW_OK) return rc;
    }

    FastGeom G = plan_geom(ev, p, H, W);
    G.win = (uint32_t)window_us;
    G.rcp = 1.0 / (double)(uint32_t)window_us; // generate_eventvolume.py:141
    G.simple = t0_fits_simple(S) ? 1 : 0; // (t0 = t_end - window is negative for a label in the first `window` microseconds of a file)

    hipStream_t st = (hipStream_t)stream;
    char *w8 = (char *)workspace;
    (void)hipGetLastError();
    {
        const int ok = lds_order_ok(w8, st); // cached per device after the first call
        if (ok != FRLW_OK) return ok;
    }
    if (gather && gather->blk[gather->n] > 0u) // every check has passed: the copy the partition is about to read
        hipLaunchKernelGGL(kf_gather_ranges, dim3(gather->blk[gather->n]), dim3(kGT), 0, st, gather_src, *gather, (uint2 *)ev->data);
    launch_partition<true>(G, S, p, cm, w8, st);
    TileP q = {}; // second level: kf_split_whole + kf_ev_sub (one wavefront per sub-tile list)
    launch_second_level(q, p, S, cm, w8, st);
    EvTileP e;
    e.H = H; e.W = W; e.twl = p.twl; e.thl = p.thl; e.tiles_x = p.tiles_x; e.T = p.T; e.bins = bins; e.win = (uint32_t)window_us; e.rcp = G.rcp;
    e.rec2 = q.rec2; e.base = q.base; e.sub = q.sub; e.sub_end = q.sub_end; e.pairs = p.pairs; e.direct = p.direct;
    e.tlut = (const float *)(w8 + p.off_tlut); e.hdr = (FastHeader *)w8; e.out_f32 = out_f32; e.out_u8 = out_u8;
    const int sub_grid = (p.pairs * kFW + 3) / 4;
    const CmP cmq = cm ? cm_params(p, w8) : CmP{};
    bool fadd = false;
    {
        // kf_ev_fadd: calls whose lists are few and short enough that the LDS float atomics' 192 cycles per instruction and CU
        // stay below the ticket kernel's latency chain (measured: 1 M events in 576 lists 25 against 35 us, the whole call 40 against 50; with plain stores instead of the atomics the kernel takes 19 us: gather and decode are most of it; the ticket kernel
        // wins from about 3 M events on), on devices where the self-test saw ds_add_f32 make the sequential sums
        int dev = 0;
        const bool hw_ok = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDevices && g_lds_fadd[dev].load(std::memory_order_acquire) == 1;
        const int knob = tuning_knob(ev->tuning, &frlw_tuning_t::ev_lds_float_atomics, -1);
        fadd = cm && p.direct && hw_ok && (knob >= 0 ? knob != 0 : n <= 3000000ll);
    }
    if (fadd) {
        if (bins <= 5) hipLaunchKernelGGL((kf_ev_fadd<5>), dim3(p.pairs * kFW), dim3(kFaddWaves * kWave), 0, st, e, cmq, S);
        else hipLaunchKernelGGL((kf_ev_fadd<kMaxK>), dim3(p.pairs * kFW), dim3(kFaddWaves * kWave), 0, st, e, cmq, S);
    } else if (cm && p.direct) { // the sub-tile wavefronts gather their own lists
        if (bins <= 5) hipLaunchKernelGGL((kf_ev_sub<5, true>), dim3(sub_grid), dim3(4 * kWave), 0, st, e, cmq, S);
        else hipLaunchKernelGGL((kf_ev_sub<kMaxK, true>), dim3(sub_grid), dim3(4 * kWave), 0, st, e, cmq, S);
    } else if (bins <= 5) hipLaunchKernelGGL((kf_ev_sub<5, false>), dim3(sub_grid), dim3(4 * kWave), 0, st, e, cmq, S);
    else hipLaunchKernelGGL((kf_ev_sub<kMaxK, false>), dim3(sub_grid), dim3(4 * kWave), 0, st, e, cmq, S);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}
} // namespace

extern "C" {

int frlw_ev_encode_batch(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_end, int n_seq, int H, int W,
                         int bins, int64_t window_us, float *out_f32, uint8_t *out_u8, void *workspace,
                         size_t workspace_bytes, frlw_stream_t stream)
{
    return ev_batch_run(ev, seq_offsets, t_end, n_seq, H, W, bins, window_us, out_f32, out_u8, workspace, workspace_bytes, stream);
}

// The batch call's workspace comes FIRST (its header is the workspace header: status, sticky status and the self-test result
// stay where frlw_workspace_init / frlw_encoder_deferred_status expect them), the copy of the windows' records behind it.
static size_t ranges_copy_offset(int64_t n_gathered, int n_win, int H, int W, int64_t window_us)
{
    const size_t inner = frlw_ev_batch_workspace_bytes(n_gathered, n_win, H, W, window_us);
    return inner ? frlw::align_up(inner, 256) : 0;
}

size_t frlw_ev_ranges_workspace_bytes(int64_t n_gathered, int n_win, int H, int W, int64_t window_us)
{
    if (n_gathered < 0 || n_win < 1 || n_win > kMaxSeq) return 0;
    const size_t off = ranges_copy_offset(n_gathered, n_win, H, W, window_us);
    return off ? off + frlw::align_up((size_t)n_gathered * 8, 16) : 0;
}

int frlw_ev_encode_ranges(const frlw_events_t *ev, const int64_t *win_lo, const int64_t *win_hi, const int64_t *t_end, int n_win,
                          int H, int W, int bins, int64_t window_us, float *out_f32, uint8_t *out_u8, void *workspace,
                          size_t workspace_bytes, frlw_stream_t stream)
{
    if (!out_f32 && !out_u8) return FRLW_ERR_ARG;
    if (bins < 1 || bins > FRLW_MAX_BINS || window_us < 1) return FRLW_ERR_ARG;
    if (!ev || !win_lo || !win_hi || !t_end || !workspace || n_win < 1 || n_win > kMaxSeq) return FRLW_ERR_ARG;
    if (ev->layout != FRLW_LAYOUT_DAT8) return FRLW_ERR_UNSUPPORTED;
    RangeTab T = {};
    int64_t offs[kMaxSeq + 1];
    unsigned long long blocks = 0;
    offs[0] = 0;
    for (int w = 0; w < n_win; ++w) {
        if (win_lo[w] < 0 || win_hi[w] < win_lo[w] || win_hi[w] > ev->n) return FRLW_ERR_ARG;
        T.lo[w] = win_lo[w];
        T.dst[w] = offs[w];
        T.blk[w] = (uint32_t)blocks;
        offs[w + 1] = offs[w] + (win_hi[w] - win_lo[w]);
        if (offs[w + 1] >= (1ll << 31)) return FRLW_ERR_UNSUPPORTED; // (the partition's own limit on a call's records)
        blocks += (unsigned long long)((win_hi[w] - win_lo[w] + kGSlice - 1) / kGSlice); // (< 2^31 / kGSlice + 64: fits 32 bits)
    }
    for (int w = n_win; w <= kMaxSeq; ++w) { T.dst[w] = offs[n_win]; T.blk[w] = (uint32_t)blocks; }
    T.n = n_win;
    const int64_t n_gathered = offs[n_win];
    if (n_gathered > 0 && !ev->data) return FRLW_ERR_ARG;
    const size_t copy_off = ranges_copy_offset(n_gathered, n_win, H, W, window_us);
    if (copy_off == 0) return (H <= 0 || W <= 0) ? FRLW_ERR_ARG : FRLW_ERR_UNSUPPORTED;
    if (workspace_bytes < copy_off + frlw::align_up((size_t)n_gathered * 8, 16)) return FRLW_ERR_WORKSPACE;
    uint2 *copy = (uint2 *)((char *)workspace + copy_off);
    frlw_events_t local = *ev; // maps and tuning are the caller's, the records are the copy
    local.data = copy;
    local.n = n_gathered;
    const int rc = ev_batch_run(&local, offs, t_end, n_win, H, W, bins, window_us, out_f32, out_u8, workspace, copy_off, stream, &T,
                                (const uint2 *)ev->data);
    if (rc != FRLW_OK) return rc;
    g_chain_counts[1].fetch_add(1ull, std::memory_order_relaxed);
    return FRLW_OK;
}

} // extern "C"

namespace frlw {
size_t sae_fast_workspace_bytes(long long n, int H, int W)
{
    FastPlan p;
    SeqTab S;
    return sae_fast_plan(n, H, W, 0, p, S) ? p.bytes : 0;
}

std::atomic<unsigned long long> g_path_counts[4]; // [0] SAE two-launch, [1] SAE general, [2] ECI two-launch, [3] ECI general / scan

// frlw_sae_encode's two-launch form (see kf_sae_sub).  Returns FRLW_OK when it has launched the encode, 1 when the call is not
// eligible (nothing launched: the caller takes the general path), a negative FRLW_ERR_* on a HIP failure.
int sae_fast_try(const frlw_events_t *ev, int H, int W, const float *lam, int n_lamda, const float *mem_in, float *mem_out,
                 long long now, long long window_us, float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes,
                 hipStream_t st)
{
    // (mem_out == nullptr: the Event Count Image -- lam[0 .. 20] is its count -> value table, no time filter)
    const bool eci = mem_out == nullptr;
    if (eci) { now = -1; window_us = 0; }
    if (!ev || ev->layout != FRLW_LAYOUT_DAT8 || !ev->data || !workspace || (!eci && window_us <= 0)) return 1;
    if ((ev->xmap == nullptr) != (ev->ymap == nullptr) || !tuning_valid(ev->tuning)) return 1;
    const long long n = ev->n;
    if (tuning_knob(ev->tuning, &frlw_tuning_t::staged_scatter, -1) == 0) return 1; // staged_scatter = 0 keeps the general path (tests)
    FastPlan p;
    SeqTab S;
    if (!sae_fast_plan(n, H, W, now - window_us, p, S)) return 1;
    if (workspace_bytes < p.bytes) return 1; // (frlw_encoder_workspace_bytes covers p.bytes: only a caller that sized the workspace itself gets here)
    FastGeom G = plan_geom(ev, p, H, W); // (the plan is a direct-mode one: sub-tile bins)
    G.win = 0xffffffffu;
    G.simple = t0_fits_simple(S) ? 1 : 0;
    char *w8 = (char *)workspace;
    FastHeader *hdr = (FastHeader *)w8;
    (void)hipGetLastError();
    static std::atomic<uint32_t> g_epoch_sae{0};
    const uint32_t epoch = cm_epoch(g_epoch_sae, 0x40000000u, hdr, st);
    float *const no_table = nullptr;
    if (eci) { // (t0 = -1 is outside the SIMPLE decode's range: the general form keeps every event)
        if (ev->xmap) launch_scatter_cm<true, true, false, kMaxBpw, 2>(G, S, p, w8, no_table, epoch, st);
        else launch_scatter_cm<false, true, false, kMaxBpw, 2>(G, S, p, w8, no_table, epoch, st);
    } else if (ev->xmap) launch_scatter_cm<true, true, false, kMaxBpw, 1>(G, S, p, w8, no_table, epoch, st);
    else if (G.simple) launch_scatter_cm<false, true, true, kMaxBpw, 1>(G, S, p, w8, no_table, epoch, st);
    else launch_scatter_cm<false, true, false, kMaxBpw, 1>(G, S, p, w8, no_table, epoch, st);
    SaeFastP q;
    q.H = H; q.W = W; q.twl = p.twl; q.thl = p.thl; q.tiles_x = p.tiles_x; q.T = p.T; q.n_lamda = n_lamda;
    for (int l = 0; l < (eci ? 21 : n_lamda); ++l) q.lam[l] = lam[l];
    q.nowf = (float)now;
    q.data = (const uint2 *)ev->data;
    q.mem_in = mem_in; q.mem_out = mem_out; q.out_f32 = out_f32; q.out_u8 = out_u8; q.hdr = hdr;
    const CmP cmq = cm_params(p, w8);
    if (eci) hipLaunchKernelGGL(kf_sae_sub<true>, dim3(p.pairs * kFW), dim3(kSubCells), 0, st, q, cmq, S);
    else hipLaunchKernelGGL(kf_sae_sub<false>, dim3(p.pairs * kFW), dim3(kSubCells), 0, st, q, cmq, S);
    HIP_TRY(hipGetLastError());
    g_path_counts[eci ? 2 : 0].fetch_add(1ull, std::memory_order_relaxed);
    return FRLW_OK;
}
} // namespace frlw
