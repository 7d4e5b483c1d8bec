// motion.hip -- the device half of the motion-level evaluation (frlw_time_surface_batch, frlw_box_flow_sums).
//
// Time-surface pairs (generate_opticalflow.py:72-92, :176-187): per label window two (H, W) images of "when was this pixel last
// hit", volume1 from the events older than end_stamp - 50 ms and volume2 from all of them, both scaled to 0..255 between the first
// and the last timestamp OF THE EVENTS.  The reference walks the events one by one; a cell keeps its last writer in stream order,
// which is the order-free integer key of kb_sae_last (encoders_batch.hip), so a window is a record range of the raw DAT tensor:
//
//   kb_zero       key planes and stamp words <- 0, the call's status word <- 0                                     (enc_batch.h)
//   kt_range      (window, slice of 4096 records): min / max timestamp over the in-bounds events, 64-bit atomicMin / atomicMax
//   kt_last       (window, slice): planeB[y][x] = max(planeB, (position + 1) << 32 | t) for every in-bounds event, planeA the same
//                 for the events with t < end_stamp - 50000; polarity is ignored.  t is the record's 32-bit field itself, so the key
//                 carries it exactly (float(t), the payload of the Surface of Active Events key, would not do: the value is used in
//                 float64)
//   kt_out        per cell, in float64 and in the reference's operation order: (last - start) / den * 255 and
//                 (last - start - 50000) / den * 255 with den = end - 50000 - start, untouched cells = 0 before the subtraction,
//                 negative -> 0, truncated to uint8.  A window without an in-bounds event gives zeros; a window with den <= 0 is
//                 left to the caller (numpy's own division and cast decide there): zeros are stored, the stamps tell which.
//
// Four launches, no host synchronisation, nothing but the caller's workspace: capturable.
//
// Box flow sums (motion_level_statistics_gt.py:130): sum over a box of sqrt(fx^2 + fy^2) of a (T, H, W, 2) float32 flow batch.  One
// workgroup per box; the magnitude in float32 with every operation rounded on its own (no FMA), the sum in float64, reduced in a
// fixed order: deterministic.

#include "frlw_common.h"
#include "enc_batch.h"

using namespace frlw;

namespace {

constexpr long long kCut = 50000;            // generate_opticalflow.py:79,83: the 50 ms between the two surfaces
constexpr long long kMinBias = 1ll << 32;    // the min word holds t - 2^32 (< 0 for every 32-bit t), so the zeroed word is "none yet"

// per window two 64-bit words behind the key planes: [0] min (biased, signed), [1] max + 1 (0 = no in-bounds event)
struct Stamps { long long lo; unsigned long long hi; };

__device__ __forceinline__ long long shfl_xor_ll(long long v, int m)
{
    const int a = __shfl_xor((int)(uint32_t)((unsigned long long)v & 0xffffffffull), m, 64);
    const int b = __shfl_xor((int)(uint32_t)((unsigned long long)v >> 32), m, 64);
    return (long long)(((unsigned long long)(uint32_t)b << 32) | (uint32_t)a);
}

// ---- stamp range --------------------------------------------------------------------------------
__global__ __launch_bounds__(kBT) void kt_range(BatchDecode D, BatchTab T, Stamps *stamps)
{
    const int t = threadIdx.x;
    const int w = window_of_block(T, blockIdx.x);
    const long long s0 = T.lo[w] + (long long)(blockIdx.x - T.blk[w]) * kBSlice;
    const long long s1 = s0 + kBSlice < T.hi[w] ? s0 + kBSlice : T.hi[w];
    long long mn = 0, mx = -1; // biased min (0 = none), max
    for (long long i0 = s0; i0 < s1; i0 += kBU * kBT) {
        uint2 r[kBU];
#pragma unroll
        for (int u = 0; u < kBU; ++u) {
            const long long i = i0 + u * kBT + t;
            r[u] = D.data[i < s1 ? i : s1 - 1];
        }
#pragma unroll
        for (int u = 0; u < kBU; ++u) {
            const int x = (int)(r[u].y & 16383u), y = (int)((r[u].y >> 14) & 16383u);
            if (i0 + u * kBT + t < s1 && x < D.W && y < D.H) { // generate_opticalflow.py:178: dropped, no error
                const long long ts = (long long)r[u].x;
                if (ts - kMinBias < mn) mn = ts - kMinBias;
                if (ts > mx) mx = ts;
            }
        }
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const long long on = shfl_xor_ll(mn, m), ox = shfl_xor_ll(mx, m);
        if (on < mn) mn = on;
        if (ox > mx) mx = ox;
    }
    if ((t & (kWave - 1)) == 0 && mx >= 0) {
        __hip_atomic_fetch_min(&stamps[w].lo, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&stamps[w].hi, (unsigned long long)mx + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- last writer per cell, both surfaces ---------------------------------------------------------
__global__ __launch_bounds__(kBT) void kt_last(BatchDecode D, BatchTab T, const Stamps *stamps, unsigned long long *last)
{
    const int t = threadIdx.x;
    const int s = window_of_block(T, blockIdx.x);
    // back to front, as kb_sae_last: the late slices start first and most earlier events find their cell already beaten
    const long long slice = (long long)(T.blk[s + 1] - 1u - blockIdx.x);
    const long long s0 = T.lo[s] + slice * kBSlice;
    const long long s1 = s0 + kBSlice < T.hi[s] ? s0 + kBSlice : T.hi[s];
    const long long total = (long long)D.H * D.W;
    const long long first = T.lo[s];
    const unsigned long long hi = stamps[s].hi;
    if (hi == 0ull) return; // no in-bounds event in the whole window (uniform)
    const long long cut = (long long)(hi - 1ull) - kCut; // volume1 takes t < end_stamp - 50000 (:79)
    unsigned long long *planeA = last + (long long)s * 2 * total, *planeB = planeA + total;
    for (long long i0 = s0; i0 < s1; i0 += kBU * kBT) {
        uint2 r[kBU];
#pragma unroll
        for (int u = 0; u < kBU; ++u) {
            const long long i = i0 + u * kBT + t;
            r[u] = D.data[i < s1 ? i : s1 - 1];
        }
        long long cell[kBU];
        unsigned long long key[kBU], seenA[kBU], seenB[kBU];
        bool early[kBU];
#pragma unroll
        for (int u = 0; u < kBU; ++u) {
            const long long i = i0 + u * kBT + t;
            const int x = (int)(r[u].y & 16383u), y = (int)((r[u].y >> 14) & 16383u);
            const bool ok = i < s1 && x < D.W && y < D.H;
            cell[u] = ok ? (long long)y * D.W + x : -1;
            early[u] = ok && (long long)r[u].x < cut;
            // last writer in stream order = max over (position in the window + 1, t): the key of kb_sae_last with the exact stamp
            key[u] = ((unsigned long long)(i - first + 1) << 32) | r[u].x;
            seenB[u] = ok ? __hip_atomic_load(&planeB[cell[u]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
            seenA[u] = early[u] ? __hip_atomic_load(&planeA[cell[u]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
        }
#pragma unroll
        for (int u = 0; u < kBU; ++u) {
            if (cell[u] >= 0 && seenB[u] < key[u]) atomicMax(&planeB[cell[u]], key[u]); // (a stale read is a smaller one)
            if (early[u] && seenA[u] < key[u]) atomicMax(&planeA[cell[u]], key[u]);
        }
    }
}

// grid (cells, windows)
__global__ __launch_bounds__(256) void kt_out(const unsigned long long *last, long long cells, const Stamps *stamps, uint8_t *out,
                                              long long *stamp_out)
{
    const int s = blockIdx.y;
    const Stamps st = stamps[s];
    const bool any = st.hi != 0ull;
    const long long start = any ? st.lo + kMinBias : -1, end = any ? (long long)(st.hi - 1ull) : -1;
    if (blockIdx.x == 0 && threadIdx.x == 0 && stamp_out) { stamp_out[2 * s] = start; stamp_out[2 * s + 1] = end; }
    const long long den_i = end - kCut - start;
    const bool live = any && den_i > 0; // den <= 0: the caller's numpy decides (zeros here)
    const double startd = (double)start, den = (double)den_i;
    const unsigned long long *planeA = last + (long long)s * 2 * cells, *planeB = planeA + cells;
    uint8_t *outA = out + (long long)s * 2 * cells, *outB = outA + cells;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += stride) {
        uint8_t a = 0, b = 0;
        if (live) {
            const unsigned long long ka = planeA[c], kb = planeB[c];
            // untouched cells carry 0.0, as the reference's zero-initialised arrays do; subtract, divide, multiply (:82-85)
            double v1 = (ka ? (double)(uint32_t)ka : 0.0) - startd;
            double v2 = (kb ? (double)(uint32_t)kb : 0.0) - startd - 50000.0;
            v1 = v1 / den * 255.0;
            v2 = v2 / den * 255.0;
            if (v1 < 0.0) v1 = 0.0; // np.where(volume < 0, 0, volume) :90-91
            if (v2 < 0.0) v2 = 0.0;
            a = (uint8_t)(int)v1;   // 0 <= v <= 255 here (last < end - 50000 resp. last <= end): .astype(np.uint8) truncates
            b = (uint8_t)(int)v2;
        }
        outA[c] = a;
        outB[c] = b;
    }
}

// ---- box flow sums ------------------------------------------------------------------------------
// One workgroup per box.  The 256 threads form rows of `lanes` threads (a power of two >= the box width, 256 at most): a row of
// threads strides along x with 8-byte reads, 256 / lanes image rows are in flight, the rest are looped.
__global__ __launch_bounds__(256) void k_box_flow_sums(const float2 *flows, int n_flows, int H, int W, const int *boxes, double *out)
{
#pragma clang fp contract(off)
    __shared__ double part[256 / kWave];
    const int *bx = boxes + 5ll * blockIdx.x;
    const int f = bx[0], x0 = bx[1], x1 = bx[2], y0 = bx[3], y1 = bx[4];
    if (x0 >= x1 || y0 >= y1) { // empty slice: np.sum of nothing
        if (threadIdx.x == 0) out[blockIdx.x] = 0.0;
        return;
    }
    if (f < 0 || f >= n_flows || x0 < 0 || y0 < 0 || x1 > W || y1 > H) { // never read outside the batch: the host refuses such a box first
        if (threadIdx.x == 0) out[blockIdx.x] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    int lanes = 1;
    while (lanes < x1 - x0 && lanes < 256) lanes <<= 1;
    const int rows = 256 / lanes;
    const int tx = threadIdx.x & (lanes - 1), ty = threadIdx.x / lanes;
    const float2 *img = flows + (long long)f * H * W;
    double acc = 0.0;
    for (int y = y0 + ty; y < y1; y += rows) {
        const float2 *row = img + (long long)y * W;
        for (int x = x0 + tx; x < x1; x += lanes) {
            const float2 v = row[x];
            const float xx = v.x * v.x, yy = v.y * v.y; // each rounded to float32 on its own, as numpy's flow**2 + flow**2
            const float ss = xx + yy;
            acc += (double)sqrtf(ss);
        }
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) acc += __longlong_as_double(shfl_xor_ll(__double_as_longlong(acc), m));
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = part[0];
        for (int i = 1; i < 256 / kWave; ++i) sum += part[i];
        out[blockIdx.x] = sum;
    }
}

std::atomic<unsigned long long> g_motion_counts[2]; // calls served: [0] frlw_time_surface_batch, [1] frlw_box_flow_sums

size_t surface_bytes(int n, int H, int W)
{
    const size_t planes = batch_bytes(n, H, W, sizeof(unsigned long long)); // two key planes per window: volume1, volume2
    return planes == 0 ? 0 : planes + (size_t)kMaxSeq * sizeof(Stamps);
}

} // namespace

extern "C" {

int frlw_motion_counts(uint64_t counts[2])
{
    if (!counts) return FRLW_ERR_ARG;
    for (int i = 0; i < 2; ++i) counts[i] = (uint64_t)g_motion_counts[i].load(std::memory_order_relaxed);
    return FRLW_OK;
}

size_t frlw_time_surface_workspace_bytes(int64_t n_records, int n_win, int H, int W)
{
    return n_records < 0 ? 0 : surface_bytes(n_win, H, W);
}

int frlw_time_surface_batch(const frlw_events_t *ev, const int64_t *win_lo, const int64_t *win_hi, int n_win, int H, int W,
                            uint8_t *out_u8, int64_t *stamps_out, void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    if (!out_u8 || !win_lo || !win_hi || !workspace || n_win < 1 || n_win > kMaxSeq) return FRLW_ERR_ARG;
    {
        const int rc = events_check(ev);
        if (rc != FRLW_OK) return rc;
    }
    if (ev->xmap) return FRLW_ERR_UNSUPPORTED; // the flow runs at the sensor's resolution: no coordinate maps
    if (H > 16384 || W > 16384) return FRLW_ERR_ARG;
    const size_t need = surface_bytes(n_win, H, W);
    if (need == 0) return FRLW_ERR_ARG;
    if (workspace_bytes < need) return FRLW_ERR_WORKSPACE;
    BatchTab T = {};
    for (int w = 0; w < n_win; ++w) { T.lo[w] = win_lo[w]; T.hi[w] = win_hi[w]; }
    if (!tab_ranges(T, ev, n_win)) return FRLW_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    WsHeader *hdr = (WsHeader *)workspace;
    unsigned long long *last = (unsigned long long *)((char *)workspace + kHeaderBytes);
    const long long cells = (long long)H * W;
    Stamps *stamps = (Stamps *)(last + (long long)n_win * 2 * cells); // (16-byte words: the planes hold an even number of keys)
    (void)hipGetLastError();
    const long long n16 = (long long)n_win * cells + kMaxSeq; // planes (2 keys = one 16-byte word per cell) + the stamp words
    hipLaunchKernelGGL(kb_zero, dim3(grid_for(n16, 256)), dim3(256), 0, s, (uint4 *)last, n16, hdr);
    const BatchDecode D = decode_of(ev, H, W);
    if (T.blk[n_win] > 0u) {
        hipLaunchKernelGGL(kt_range, dim3(T.blk[n_win]), dim3(kBT), 0, s, D, T, stamps);
        hipLaunchKernelGGL(kt_last, dim3(T.blk[n_win]), dim3(kBT), 0, s, D, T, (const Stamps *)stamps, last);
    }
    int gx = grid_for(cells, 256);
    if (gx > 2048 / n_win + 1) gx = 2048 / n_win + 1;
    hipLaunchKernelGGL(kt_out, dim3(gx, n_win), dim3(256), 0, s, (const unsigned long long *)last, cells, (const Stamps *)stamps, out_u8,
                       (long long *)stamps_out);
    HIP_TRY(hipGetLastError());
    g_motion_counts[0].fetch_add(1ull, std::memory_order_relaxed);
    return FRLW_OK;
}

int frlw_box_flow_sums(const float *flows, int n_flows, int H, int W, const int32_t *boxes, int64_t n_boxes, double *out,
                       frlw_stream_t stream)
{
    if (n_boxes < 0 || n_flows < 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31) || n_boxes >= (1ll << 31)) return FRLW_ERR_ARG;
    if (n_boxes == 0) return FRLW_OK;
    if (!flows || !boxes || !out || n_flows < 1 || ((uintptr_t)flows & 7u)) return FRLW_ERR_ARG;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_box_flow_sums, dim3((unsigned)n_boxes), dim3(256), 0, (hipStream_t)stream, (const float2 *)flows, n_flows, H, W,
                       (const int *)boxes, out);
    HIP_TRY(hipGetLastError());
    g_motion_counts[1].fetch_add(1ull, std::memory_order_relaxed);
    return FRLW_OK;
}

} // extern "C"
