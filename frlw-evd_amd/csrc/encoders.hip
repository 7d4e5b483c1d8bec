// encoders.hip -- the tile-kernel launcher (step 4) and the C-ABI of the event-stream -> tensor encoders.
//
// Replaces the bodies of the reference's four encoder functions (file:line in the reference):
//   generate_eventframe               generate_eventcountimage.py:19-41      (ECI)
//   generate_agile_event_volume_cuda  generate_eventvolume.py:15-42          (Event Volume)
//   generate_leaky_cuda / taf_cuda    generate_surfaceofactiveevents.py:44-80 (SAE)
//   generate_taf_cuda / taf_cuda      generate_taf.py:19-67, leaky_transform :69-76 (TAF)
// and, for raw DAT streams, the harness glue around them (generate_taf.py:197-227).
//
// partition.hip has already grouped the events by tile ((1 << twl) x 8 pixels), keeping stream order inside a tile (records
// {window << (twl + 4) | cell, f32 value}).  One workgroup of NT = 4 << twl threads owns one tile; thread t owns the four cells
// t, t + NT, t + 2NT, t + 3NT and keeps their accumulators (and, for TAF, their K-deep FIFO) in registers: enc_eci.h, enc_sae.h,
// enc_ev.h and enc_taf.h say how, enc_tile.h holds what they share.  EV and TAF bodies are templated on the cells per thread: 4
// for a whole tile; 1 for a "quarter" -- four workgroups per tile -- used for tiles the partition lists as hot (skew) and for
// every tile of a frame too small to give each SIMD a wavefront.
//
// Everything is exact-f32 arithmetic in the reference's operation order (-ffp-contract=off).

#include "enc_eci.h"
#include "enc_ev.h"
#include "enc_sae.h"
#include "enc_taf.h"
#include <type_traits>

using namespace frlw;

namespace {
// One launch of a tile kernel on `blocks` workgroups of NT = 4 << twl threads.  `pick` maps the compile-time NT to the kernel's
// instance: [](auto nt) { return k_x_tile<decltype(nt)::value>; }.
template <typename Pick, typename... Args>
void launch_tile(Pick pick, const Plan &p, int blocks, hipStream_t s, Args... args)
{
    const auto go = [&](auto nt) { hipLaunchKernelGGL(pick(nt), dim3(blocks), dim3(decltype(nt)::value), 0, s, args...); };
    if (p.twl == 8) go(std::integral_constant<int, 1024>{});
    else if (p.twl == 7) go(std::integral_constant<int, 512>{});
    else go(std::integral_constant<int, 256>{});
}

int status_code(int st)
{
    return (st & ST_INDEX) ? FRLW_ERR_INDEX : (st & ST_POLARITY) ? FRLW_ERR_POLARITY : (st & ST_SPAN) ? FRLW_ERR_SPAN : (st & ST_STALL) ? FRLW_ERR_HIP : FRLW_OK;
}
} // namespace

extern "C" { // ---- C-ABI

#ifdef FRLW_TILE_PROF
int frlw_debug_prof(unsigned long long *out, int reset)
{
    if (out) hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * 16);
    if (reset) { unsigned long long z[16] = {}; hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z); }
    return 0;
}
#endif

const char *frlw_version(void) { return "frlw_evd 0.5.0 gfx950"; }

size_t frlw_encoder_workspace_bytes(int64_t n_events, int H, int W)
{
    Plan p;
    if (!make_plan(n_events, H, W, nullptr, p)) return 0;
    // frlw_sae_encode / frlw_eci_encode take the two-launch form of taf_fast.hip when the call is eligible: its chunk-major tables
    // are a little larger than the general plan's (1 M events at 304x240: 372 against 347 KB on top of the same 8 n bytes of
    // records), and a caller that allocates exactly what this query returns must get that path too
    const size_t fast = sae_fast_workspace_bytes(n_events, H, W);
    return fast > p.bytes ? fast : p.bytes;
}

int frlw_encoder_path_counts(uint64_t counts[4])
{
    if (!counts) return FRLW_ERR_ARG;
    for (int i = 0; i < 4; ++i) counts[i] = (uint64_t)g_path_counts[i].load(std::memory_order_relaxed);
    return FRLW_OK;
}

int frlw_encoder_status(const void *workspace, frlw_stream_t stream, int *status_out)
{
    if (!workspace || !status_out) return FRLW_ERR_ARG;
    int32_t st = 0;
    uint32_t stall = 0u;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&st, workspace, sizeof(st), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&stall, (const char *)workspace + kStallOffset, sizeof(stall), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (stall) st |= ST_STALL; // (kept outside the range a late workgroup 0 resets: frlw_common.h kStallOffset)
    *status_out = status_code(st);
    return FRLW_OK;
}

int frlw_workspace_init(void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    if (!workspace || workspace_bytes < kHeaderBytes) return FRLW_ERR_ARG;
    HIP_TRY(hipMemsetAsync(workspace, 0, kHeaderBytes, (hipStream_t)stream));
    return FRLW_OK;
}

int frlw_encoder_deferred_status(void *workspace, frlw_stream_t stream, int *status_out)
{
    if (!workspace || !status_out) return FRLW_ERR_ARG;
    int32_t st = 0;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&st, (char *)workspace + kStickyOffset, sizeof(st), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync((char *)workspace + kStickyOffset, 0, sizeof(st), s));
    HIP_TRY(hipStreamSynchronize(s));
    *status_out = status_code(st);
    return FRLW_OK;
}

int frlw_eci_encode(const frlw_events_t *ev, int H, int W, float *out_f32, uint8_t *out_u8,
                    void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    if (!out_f32 && !out_u8) return FRLW_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    EciParams q;
    q.H = H; q.W = W; q.twl = 0; q.tiles_x = 0; q.out_f32 = out_f32; q.out_u8 = out_u8;
    eci_lut(q.lut);
    // calls of the GEN1 class with at least 16 384 events: two launches through the chunk-major partition (taf_fast.hip:
    // kf_scatter_cm<.., 2> + kf_sae_sub<true>: 100 000 events 21 -> 12 us)
    if (tuning_knob(ev ? ev->tuning : nullptr, &frlw_tuning_t::staged_scatter, -1) != 0) {
        const int rc2 = sae_fast_try(ev, H, W, q.lut, 21, nullptr, nullptr, 0, 0, out_f32, out_u8, workspace, workspace_bytes, s);
        if (rc2 <= 0) return rc2;
    }
    // one launch for smaller calls: every workgroup of 2048 pixels reads all events (k_eci_scan); at most 8 M event reads in all
    // (36 workgroups x 100 000 events at 304x240: 29 -> ~8 us); frlw_tuning_t::staged_scatter = 0 keeps the general path (tests)
    if (ev && workspace && workspace_bytes >= kHeaderBytes && ev->layout == FRLW_LAYOUT_DAT8 && H > 0 && W > 0 && ev->n > 0 && ev->data &&
        tuning_valid(ev->tuning) && (ev->xmap == nullptr) == (ev->ymap == nullptr) &&
        tuning_knob(ev->tuning, &frlw_tuning_t::staged_scatter, -1) != 0) {
        const long long wgs = ((long long)H * W + kEciScanPix - 1) / kEciScanPix;
        // W <= 65536: k_eci_scan forms the flat pixel x + W * y in 32 bits, and x, y reach 65535 through the coordinate maps -- a
        // wider frame (which the general path places with 64-bit arithmetic) could wrap an out-of-frame event back into the frame
        if (wgs * ev->n <= (8ll << 20) && (long long)H * W < (1ll << 31) && W <= 65536) {
            (void)hipGetLastError();
            // (without maps the kernel does not read its four map arguments)
            hipLaunchKernelGGL(ev->xmap ? k_eci_scan<true> : k_eci_scan<false>, dim3((unsigned)wgs), dim3(kEciScanThreads), 0, s,
                               (const uint2 *)ev->data, (long long)ev->n, ev->xmap, ev->ymap, ev->map_w, ev->map_h, q, (WsHeader *)workspace);
            HIP_TRY(hipGetLastError());
            g_path_counts[3].fetch_add(1ull, std::memory_order_relaxed);
            return FRLW_OK;
        }
    }
    g_path_counts[3].fetch_add(1ull, std::memory_order_relaxed);
    Partitioned pt;
    int rc = partition_events(ev, H, W, KIND_ECI, 0, 1, 1, 0, workspace, workspace_bytes, s, pt);
    if (rc != FRLW_OK) return rc;
    q.twl = pt.plan.twl; q.tiles_x = pt.plan.tiles_x;
    launch_tile([](auto nt) { return k_eci_tile<decltype(nt)::value>; }, pt.plan, pt.plan.n_tiles, s, pt.records, pt.base, q);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

int frlw_ev_encode(const frlw_events_t *ev, int H, int W, int bins, int64_t t_end,
                   int64_t window_us, float *out_f32, uint8_t *out_u8, void *workspace,
                   size_t workspace_bytes, frlw_stream_t stream)
{
    if ((!out_f32 && !out_u8) || bins < 1 || bins > FRLW_MAX_BINS) return FRLW_ERR_ARG;
    if (ev && ev->layout == FRLW_LAYOUT_DAT8 && window_us <= 0) return FRLW_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Partitioned pt;
    int rc = partition_events(ev, H, W, KIND_EV, t_end - window_us, window_us, 1, 1, workspace, workspace_bytes, s, pt);
    if (rc != FRLW_OK) return rc;
    EvParams q;
    q.H = H; q.W = W; q.twl = pt.plan.twl; q.tiles_x = pt.plan.tiles_x; q.bins = bins;
    q.hdr = pt.hdr; q.out_f32 = out_f32; q.out_u8 = out_u8;
    const TileGrid g = tile_grid(pt.plan);
    if (bins <= 5) launch_tile([](auto nt) { return k_ev_tile5<decltype(nt)::value>; }, pt.plan, g.blocks, s, pt.records, pt.base, q, g.n_tiles_arg);
    else launch_tile([](auto nt) { return k_ev_tile<decltype(nt)::value>; }, pt.plan, g.blocks, s, pt.records, pt.base, q, g.n_tiles_arg);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

int frlw_sae_encode(const frlw_events_t *ev, int H, int W, const double *lamdas, int n_lamda,
                    const float *mem_in, float *mem_out, int64_t now, int64_t window_us,
                    float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes,
                    frlw_stream_t stream)
{
    if (!mem_out || !lamdas || n_lamda < 0 || n_lamda > FRLW_MAX_LAMDAS) return FRLW_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    SaeParams q;
    for (int l = 0; l < n_lamda; ++l) q.lam[l] = (float)lamdas[l];
    // single calls of the GEN1 class: two launches instead of five (taf_fast.hip: kf_scatter_cm<.., SAE> + kf_sae_sub)
    const int rc2 = sae_fast_try(ev, H, W, q.lam, n_lamda, mem_in, mem_out, now, window_us, out_f32, out_u8, workspace, workspace_bytes, s);
    if (rc2 <= 0) return rc2;
    g_path_counts[1].fetch_add(1ull, std::memory_order_relaxed);
    Partitioned pt;
    const int filt = window_us > 0;
    int rc = partition_events(ev, H, W, KIND_SAE, now - window_us, 1, 1, filt, workspace, workspace_bytes, s, pt);
    if (rc != FRLW_OK) return rc;
    q.H = H; q.W = W; q.twl = pt.plan.twl; q.tiles_x = pt.plan.tiles_x; q.n_lamda = n_lamda; q.nowf = (float)now;
    q.mem_in = mem_in; q.mem_out = mem_out; q.out_f32 = out_f32; q.out_u8 = out_u8;
    launch_tile([](auto nt) { return k_sae_tile<decltype(nt)::value>; }, pt.plan, pt.plan.n_tiles, s, pt.records, pt.base, q);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

int frlw_taf_encode(const frlw_events_t *ev, int H, int W, int K, int64_t t_start,
                    int64_t window_us, int n_windows, float *state, float *view_f32,
                    uint8_t *out_u8, int flags, void *workspace, size_t workspace_bytes,
                    frlw_stream_t stream)
{
    if (!state || K < 1 || K > FRLW_MAX_BINS || n_windows < 1 || n_windows > FRLW_MAX_WINDOWS) return FRLW_ERR_ARG;
    if (ev && ev->layout == FRLW_LAYOUT_XYTP_F64 && n_windows != 1) return FRLW_ERR_ARG;
    if (ev && ev->layout == FRLW_LAYOUT_DAT8 && window_us <= 0) return FRLW_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Partitioned pt;
    int rc = partition_events(ev, H, W, KIND_TAF, t_start, window_us, n_windows, 0, workspace, workspace_bytes, s, pt);
    if (rc != FRLW_OK) return rc;
    TafParams q;
    q.H = H; q.W = W; q.twl = pt.plan.twl; q.tiles_x = pt.plan.tiles_x; q.K = K;
    q.n_windows = n_windows; q.flip = (flags & FRLW_TAF_U8_FLIP_K) ? 1 : 0;
    q.hdr = pt.hdr; q.state = state; q.view_f32 = view_f32; q.out_u8 = out_u8; q.leaky_thr = pt.leaky_thr;
    q.emit_mask = 0; q.snap_u8 = nullptr;
    const TileGrid g = tile_grid(pt.plan);
    launch_tile([](auto nt) { return k_taf_tile<decltype(nt)::value>; }, pt.plan, g.blocks, s, pt.records, pt.base, q, g.n_tiles_arg);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

int frlw_taf_encode_chain(const frlw_events_t *ev, int H, int W, int K, int64_t t_start, int64_t window_us,
                          int n_windows, uint64_t emit_mask, float *state, uint8_t *snap_u8, int flags,
                          void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    if (!state || !snap_u8 || K < 1 || K > FRLW_MAX_BINS || n_windows < 1 || n_windows > FRLW_MAX_WINDOWS) return FRLW_ERR_ARG;
    if (emit_mask == 0 || (n_windows < 64 && (emit_mask >> n_windows) != 0)) return FRLW_ERR_ARG;
    if (!ev || ev->layout != FRLW_LAYOUT_DAT8 || window_us <= 0) return FRLW_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Partitioned pt;
    int rc = partition_events(ev, H, W, KIND_TAF, t_start, window_us, n_windows, 0, workspace, workspace_bytes, s, pt);
    if (rc != FRLW_OK) return rc;
    TafParams q;
    q.H = H; q.W = W; q.twl = pt.plan.twl; q.tiles_x = pt.plan.tiles_x; q.K = K;
    q.n_windows = n_windows; q.flip = (flags & FRLW_TAF_U8_FLIP_K) ? 1 : 0;
    q.hdr = pt.hdr; q.state = state; q.view_f32 = nullptr; q.out_u8 = nullptr; q.leaky_thr = pt.leaky_thr;
    q.emit_mask = emit_mask; q.snap_u8 = snap_u8;
    const TileGrid g = tile_grid(pt.plan);
    launch_tile([](auto nt) { return k_taf_tile_snap<decltype(nt)::value>; }, pt.plan, g.blocks, s, pt.records, pt.base, q, g.n_tiles_arg);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

} // extern "C"
