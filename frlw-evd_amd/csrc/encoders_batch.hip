// encoders_batch.hip -- Event Count Image and Surface of Active Events for a BATCH of windows / streams in one launch sequence
// (frlw_eci_encode_batch, frlw_sae_encode_batch).
//
// Both encodings are order-free per cell: the count image depends on the number of events of a cell, saturating at
// 20 (generate_eventcountimage.py:32-34), the surface on the LAST event of a cell in stream order
// (generate_surfaceofactiveevents.py:49).  So neither needs the partition of partition.hip / taf_fast.hip nor the LDS lane-order
// property the batched TAF / Event Volume paths rest on: every record goes straight from the raw DAT array to an integer atomic on
// a per-window plane in the workspace -- exact in any arrival order -- and an element-wise kernel turns the planes into the outputs:
//
//   kb_zero        planes <- 0, the call's status word <- 0
//   kb_eci_count   (window, slice of 4096 records): cnt[w][p][y][x] += 1     (skipped once the cell reads >= 20: it is saturated)
//   kb_eci_out     cnt -> the 21-entry table of frlw_eci_encode (eci_lut, enc_plan.h) -> f32 / u8 (the plane already has the (2, H, W) layout)
//   kb_sae_last    (sequence, slice): last[s][p][y][x] = max(last, (position + 1) << 32 | bits(float(t)))  -- the key of k_sae_tile (enc_sae.h),
//                  so an unsorted stream gives the same last writer as frlw_sae_encode; the slices of a sequence are handed out
//                  back to front and a lane whose key is already beaten skips its atomic (only ~one atomic per touched cell is left)
//   kb_sae_out     key -> float(t) or the floor, torch.where against the carried memory, the n_lamda decays
//
// Three launches per call, no host synchronisation, nothing but the caller's workspace: capturable.  Windows of the count image may
// overlap or nest (the three nested windows per label of the offline command): each is a record range of its own.
//
// frlw_sae_encode_chain: the labels of ONE file are a chain (the memory label l leaves is the input of label l + 1), but only the
// last step of the surface is sequential -- the last writer of a cell within a step does not depend on the memory.  So the steps'
// key planes are filled by the same kb_sae_last launch (a step is a record range with its own now and window), and
//   kb_sae_chain_out   runs the scan over the steps per cell, the memory in a register, and stores the volumes of the emitting steps
// replaces kb_sae_out: kb_zero, kb_sae_last, kb_sae_chain_out for up to 64 labels.

#include "frlw_common.h"
#include "enc_batch.h" // BatchTab, BatchDecode, window_of_block, kb_zero, the host-side range checks (shared with motion.hip)

using namespace frlw;

namespace {

// ---- Event Count Image -------------------------------------------------------------------------
template <bool HAS_MAP>
__global__ __launch_bounds__(kBT) void kb_eci_count(BatchDecode D, BatchTab T, uint32_t *cnt, WsHeader *hdr)
{
    const int t = threadIdx.x;
    const int w = window_of_block(T, blockIdx.x);
    const long long s0 = T.lo[w] + (long long)(blockIdx.x - T.blk[w]) * kBSlice;
    const long long s1 = s0 + kBSlice < T.hi[w] ? s0 + kBSlice : T.hi[w];
    const long long total = (long long)D.H * D.W; // (< 2^31: the host checks)
    uint32_t *plane = cnt + (long long)w * 2 * total;
    int err = 0;
    for (long long i0 = s0; i0 < s1; i0 += kBU * kBT) {
        uint2 r[kBU];
#pragma unroll
        for (int u = 0; u < kBU; ++u) {
            const long long i = i0 + u * kBT + t;
            r[u] = D.data[i < s1 ? i : s1 - 1];
        }
        long long cell[kBU];
        uint32_t seen[kBU];
#pragma unroll
        for (int u = 0; u < kBU; ++u) {
            const bool live = i0 + u * kBT + t < s1;
            int x = (int)(r[u].y & 16383u), y = (int)((r[u].y >> 14) & 16383u);
            const long long p = (r[u].y >> 28) & 1u;
            bool ok = live;
            if (HAS_MAP) {
                ok = ok && x < D.map_w && y < D.map_h;
                x = D.xmap[x < D.map_w ? x : 0];
                y = D.ymap[y < D.map_h ? y : 0];
            }
            // the reference indexes the flat cell 2 x + 2 W y + p (generate_eventcountimage.py:32): x >= W aliases into the next
            // row, only a flat pixel outside the frame raises
            const long long flat = (long long)x + (long long)D.W * y;
            if (live && (!ok || flat >= total)) err |= ST_INDEX;
            cell[u] = (ok && flat < total) ? p * total + flat : -1;
            // counts only grow and the value saturates at 20 adds: a cell that already reads 20 needs no further add (a stale
            // read is a smaller one: never skipped too early), so a hot pixel costs loads, not a queue of atomics on one address
            seen[u] = cell[u] >= 0 ? __hip_atomic_load(&plane[cell[u]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        }
#pragma unroll
        for (int u = 0; u < kBU; ++u)
            if (cell[u] >= 0 && seen[u] < 20u) atomicAdd(&plane[cell[u]], 1u);
    }
    if (err) {
        atomicOr(&hdr->status, err);
        fold_sticky_status(hdr, err);
    }
}

struct EciLut {
    float v[21]; // value * 255 after n sequential +0.05f adds, clamped (n >= 20 -> 255)
};

__global__ __launch_bounds__(256) void kb_eci_out(const uint32_t *cnt, long long n, EciLut L, float *out_f32, uint8_t *out_u8)
{
    __shared__ float lut[21];
    if (threadIdx.x < 21) lut[threadIdx.x] = L.v[threadIdx.x];
    __syncthreads();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t c = cnt[i];
        const float v = lut[c > 20u ? 20u : c];
        if (out_f32) out_f32[i] = v; // plane layout = output layout: (window, polarity, y, x), generate_eventcountimage.py:36
        if (out_u8) out_u8[i] = f32_to_u8(v);
    }
}

// ---- Surface of Active Events ------------------------------------------------------------------
template <bool HAS_MAP>
__global__ __launch_bounds__(kBT) void kb_sae_last(BatchDecode D, BatchTab T, int time_filter, unsigned long long *last, WsHeader *hdr)
{
    const int t = threadIdx.x;
    const int s = window_of_block(T, blockIdx.x);
    // back to front: the late slices of a sequence start first, and most earlier events then find their cell already beaten
    const long long slice = (long long)(T.blk[s + 1] - 1u - blockIdx.x);
    const long long s0 = T.lo[s] + slice * kBSlice;
    const long long s1 = s0 + kBSlice < T.hi[s] ? s0 + kBSlice : T.hi[s];
    const long long total = (long long)D.H * D.W;
    const long long t0 = T.t0[s], first = T.lo[s];
    unsigned long long *plane = last + (long long)s * 2 * total;
    int err = 0;
    for (long long i0 = s0; i0 < s1; i0 += kBU * kBT) {
        uint2 r[kBU];
#pragma unroll
        for (int u = 0; u < kBU; ++u) {
            const long long i = i0 + u * kBT + t;
            r[u] = D.data[i < s1 ? i : s1 - 1];
        }
        long long cell[kBU];
        unsigned long long key[kBU], seen[kBU];
#pragma unroll
        for (int u = 0; u < kBU; ++u) {
            const long long i = i0 + u * kBT + t;
            const bool live = i < s1;
            int x = (int)(r[u].y & 16383u), y = (int)((r[u].y >> 14) & 16383u);
            const long long p = (r[u].y >> 28) & 1u;
            bool ok = live;
            if (HAS_MAP) {
                if (live && (x >= D.map_w || y >= D.map_h)) err |= ST_INDEX;
                ok = ok && x < D.map_w && y < D.map_h;
                x = D.xmap[x < D.map_w ? x : 0];
                y = D.ymap[y < D.map_h ? y : 0];
            }
            ok = ok && x < D.W && y < D.H;                         // generate_surfaceofactiveevents.py:72: dropped, no error
            if (time_filter) ok = ok && (long long)r[u].x > t0;    // :183
            cell[u] = ok ? p * total + (long long)y * D.W + x : -1;
            // last writer in stream order = max over (position in the sequence + 1, bits of float(t)): the key of k_sae_tile (enc_sae.h)
            key[u] = ((unsigned long long)(i - first + 1) << 32) | __float_as_uint((float)r[u].x);
            seen[u] = cell[u] >= 0 ? __hip_atomic_load(&plane[cell[u]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
        }
#pragma unroll
        for (int u = 0; u < kBU; ++u)
            if (cell[u] >= 0 && seen[u] < key[u]) atomicMax(&plane[cell[u]], key[u]); // (a stale read is a smaller one)
    }
    if (err) {
        atomicOr(&hdr->status, err);
        fold_sticky_status(hdr, err);
    }
}

struct SaeOutP {
    int n_lamda;
    float lam[FRLW_MAX_LAMDAS];
    const float *mem_in;
    float *mem_out;
    float *out_f32;
    uint8_t *out_u8;
};

// grid (cells, sequences)
__global__ __launch_bounds__(256) void kb_sae_out(const unsigned long long *last, long long cells, BatchTab T, SaeOutP q)
{
    const int s = blockIdx.y;
    const float nowf = T.nowf[s];
    const float init = (0.0f + nowf) - 5000000.0f; // generate_surfaceofactiveevents.py:48
    const long long base = (long long)s * cells, stride = (long long)gridDim.x * blockDim.x;
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += stride) {
        const unsigned long long key = last[base + c];
        float tv = key ? __uint_as_float((uint32_t)key) : init;
        if (q.mem_in) {
            const float m = q.mem_in[base + c];
            if (!(tv > m)) tv = m; // torch.where(t_img > memory, t_img, memory) :52
        }
        q.mem_out[base + c] = tv;
        const float dt = tv - nowf;
        for (int l = 0; l < q.n_lamda; ++l) {
            const float v = expf(q.lam[l] * dt) * 255.0f;
            const long long oi = ((long long)s * q.n_lamda + l) * cells + c;
            if (q.out_f32) q.out_f32[oi] = v;
            if (q.out_u8) q.out_u8[oi] = f32_to_u8(v);
        }
    }
}

// ---- Surface of Active Events, chained steps -----------------------------------------------------
// The steps of one chain, by value like BatchTab: float(now) of step s and where its volume goes (-1: the step only advances the memory)
struct ChainTab {
    float nowf[kMaxSeq];
    int slot[kMaxSeq];
    int n;
};

constexpr int kChainU = 8; // steps whose keys are in flight before the first is used

// One thread per cell of the ONE (2, H, W) memory plane, the running memory in a register: the scan over the steps that
// n calls of kb_sae_out would make through mem_in / mem_out.  The keys do not depend on the memory, so kChainU steps' loads are
// issued together (planes are step-major: every load and store is coalesced across the workgroup).
__global__ __launch_bounds__(256) void kb_sae_chain_out(const unsigned long long *last, long long cells, ChainTab T, SaeOutP q)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += stride) {
        bool has = q.mem_in != nullptr;
        float m = has ? q.mem_in[c] : 0.0f;
        for (int s0 = 0; s0 < T.n; s0 += kChainU) {
            unsigned long long key[kChainU];
#pragma unroll
            for (int u = 0; u < kChainU; ++u) key[u] = s0 + u < T.n ? last[(long long)(s0 + u) * cells + c] : 0ull;
#pragma unroll
            for (int u = 0; u < kChainU; ++u) {
                const int s = s0 + u;
                if (s < T.n) {
                    const float nowf = T.nowf[s];
                    float tv = key[u] ? __uint_as_float((uint32_t)key[u]) : (0.0f + nowf) - 5000000.0f; // kb_sae_out's value
                    if (has && !(tv > m)) tv = m; // torch.where(t_img > memory, t_img, memory)
                    m = tv;
                    has = true;
                    const int slot = T.slot[s];
                    if (slot >= 0) {
                        const float dt = m - nowf;
                        for (int l = 0; l < q.n_lamda; ++l) {
                            const float v = expf(q.lam[l] * dt) * 255.0f;
                            const long long oi = ((long long)slot * q.n_lamda + l) * cells + c;
                            if (q.out_f32) q.out_f32[oi] = v;
                            if (q.out_u8) q.out_u8[oi] = f32_to_u8(v);
                        }
                    }
                }
            }
        }
        q.mem_out[c] = m;
    }
}

// ---- host --------------------------------------------------------------------------------------
std::atomic<unsigned long long> g_batch_counts[2]; // calls served: [0] Event Count Image, [1] Surface of Active Events

} // namespace

namespace frlw {
std::atomic<unsigned long long> g_chain_counts[2]; // calls served: [0] frlw_sae_encode_chain, [1] frlw_ev_encode_ranges (taf_fast.hip)
}

extern "C" {

int frlw_encoder_batch_counts(uint64_t counts[2])
{
    if (!counts) return FRLW_ERR_ARG;
    for (int i = 0; i < 2; ++i) counts[i] = (uint64_t)g_batch_counts[i].load(std::memory_order_relaxed);
    return FRLW_OK;
}

int frlw_encoder_chain_counts(uint64_t counts[2])
{
    if (!counts) return FRLW_ERR_ARG;
    for (int i = 0; i < 2; ++i) counts[i] = (uint64_t)g_chain_counts[i].load(std::memory_order_relaxed);
    return FRLW_OK;
}

size_t frlw_eci_batch_workspace_bytes(int64_t n_records, int n_win, int H, int W)
{
    return n_records < 0 ? 0 : batch_bytes(n_win, H, W, sizeof(uint32_t));
}

size_t frlw_sae_batch_workspace_bytes(int64_t n_records, int n_seq, int H, int W)
{
    return n_records < 0 ? 0 : batch_bytes(n_seq, H, W, sizeof(unsigned long long));
}

int frlw_eci_encode_batch(const frlw_events_t *ev, const int64_t *win_lo, const int64_t *win_hi, int n_win, int H, int W,
                          float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    if ((!out_f32 && !out_u8) || !win_lo || !win_hi || !workspace || n_win < 1 || n_win > kMaxSeq) return FRLW_ERR_ARG;
    {
        const int rc = events_check(ev);
        if (rc != FRLW_OK) return rc;
    }
    const size_t need = batch_bytes(n_win, H, W, sizeof(uint32_t));
    if (need == 0) return FRLW_ERR_ARG;
    if (workspace_bytes < need) return FRLW_ERR_WORKSPACE;
    BatchTab T = {};
    for (int w = 0; w < n_win; ++w) { T.lo[w] = win_lo[w]; T.hi[w] = win_hi[w]; }
    if (!tab_ranges(T, ev, n_win)) return FRLW_ERR_ARG;
    EciLut L;
    eci_lut(L.v); // the table of frlw_eci_encode
    hipStream_t s = (hipStream_t)stream;
    WsHeader *hdr = (WsHeader *)workspace;
    uint32_t *cnt = (uint32_t *)((char *)workspace + kHeaderBytes);
    const long long cells = (long long)n_win * 2 * H * W;
    (void)hipGetLastError();
    const long long n16 = (cells + 3) / 4; // (the planes are rounded up to whole 16-byte words: batch_bytes)
    hipLaunchKernelGGL(kb_zero, dim3(grid_for(n16, 256)), dim3(256), 0, s, (uint4 *)cnt, n16, hdr);
    const BatchDecode D = decode_of(ev, H, W);
    if (T.blk[n_win] > 0u) {
        if (ev->xmap) hipLaunchKernelGGL(kb_eci_count<true>, dim3(T.blk[n_win]), dim3(kBT), 0, s, D, T, cnt, hdr);
        else hipLaunchKernelGGL(kb_eci_count<false>, dim3(T.blk[n_win]), dim3(kBT), 0, s, D, T, cnt, hdr);
    }
    hipLaunchKernelGGL(kb_eci_out, dim3(grid_for(cells, 256)), dim3(256), 0, s, (const uint32_t *)cnt, cells, L, out_f32, out_u8);
    HIP_TRY(hipGetLastError());
    g_batch_counts[0].fetch_add(1ull, std::memory_order_relaxed);
    return FRLW_OK;
}

int frlw_sae_encode_batch(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *now, int n_seq, int H, int W,
                          const double *lamdas, int n_lamda, const float *mem_in, float *mem_out, int64_t window_us,
                          float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    if (!seq_offsets || !now || !mem_out || !workspace || n_seq < 1 || n_seq > kMaxSeq) return FRLW_ERR_ARG;
    if (n_lamda < 0 || n_lamda > FRLW_MAX_LAMDAS || (n_lamda > 0 && !lamdas)) return FRLW_ERR_ARG;
    {
        const int rc = events_check(ev);
        if (rc != FRLW_OK) return rc;
    }
    const size_t need = batch_bytes(n_seq, H, W, sizeof(unsigned long long));
    if (need == 0) return FRLW_ERR_ARG;
    if (workspace_bytes < need) return FRLW_ERR_WORKSPACE;
    BatchTab T = {};
    for (int q = 0; q < n_seq; ++q) {
        T.lo[q] = seq_offsets[q]; T.hi[q] = seq_offsets[q + 1];
        T.t0[q] = now[q] - window_us;
        T.nowf[q] = (float)now[q];
    }
    if (!tab_ranges(T, ev, n_seq)) return FRLW_ERR_ARG;
    SaeOutP q;
    q.n_lamda = n_lamda;
    for (int l = 0; l < FRLW_MAX_LAMDAS; ++l) q.lam[l] = l < n_lamda ? (float)lamdas[l] : 0.0f;
    q.mem_in = mem_in; q.mem_out = mem_out; q.out_f32 = out_f32; q.out_u8 = out_u8;
    hipStream_t s = (hipStream_t)stream;
    WsHeader *hdr = (WsHeader *)workspace;
    unsigned long long *last = (unsigned long long *)((char *)workspace + kHeaderBytes);
    const long long cells = 2ll * H * W;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kb_zero, dim3(grid_for(n_seq * cells / 2, 256)), dim3(256), 0, s, (uint4 *)last, n_seq * cells / 2, hdr);
    const BatchDecode D = decode_of(ev, H, W);
    const int filt = window_us > 0 ? 1 : 0;
    if (T.blk[n_seq] > 0u) {
        if (ev->xmap) hipLaunchKernelGGL(kb_sae_last<true>, dim3(T.blk[n_seq]), dim3(kBT), 0, s, D, T, filt, last, hdr);
        else hipLaunchKernelGGL(kb_sae_last<false>, dim3(T.blk[n_seq]), dim3(kBT), 0, s, D, T, filt, last, hdr);
    }
    int gx = grid_for(cells, 256);
    if (gx > 2048 / n_seq + 1) gx = 2048 / n_seq + 1;
    hipLaunchKernelGGL(kb_sae_out, dim3(gx, n_seq), dim3(256), 0, s, (const unsigned long long *)last, cells, T, q);
    HIP_TRY(hipGetLastError());
    g_batch_counts[1].fetch_add(1ull, std::memory_order_relaxed);
    return FRLW_OK;
}

size_t frlw_sae_chain_workspace_bytes(int64_t n_records, int n_steps, int H, int W)
{
    return n_records < 0 ? 0 : batch_bytes(n_steps, H, W, sizeof(unsigned long long)); // one key plane per step
}

int frlw_sae_encode_chain(const frlw_events_t *ev, const int64_t *step_lo, const int64_t *step_hi, const int64_t *now,
                          const int64_t *window_us, const uint8_t *emit, int n_steps, int H, int W, const double *lamdas, int n_lamda,
                          const float *mem_in, float *mem_out, float *out_f32, uint8_t *out_u8, void *workspace,
                          size_t workspace_bytes, frlw_stream_t stream)
{
    if (!step_lo || !step_hi || !now || !window_us || !emit || !mem_out || !workspace || n_steps < 1 || n_steps > kMaxSeq) return FRLW_ERR_ARG;
    if (n_lamda < 0 || n_lamda > FRLW_MAX_LAMDAS || (n_lamda > 0 && !lamdas)) return FRLW_ERR_ARG;
    {
        const int rc = events_check(ev);
        if (rc != FRLW_OK) return rc;
    }
    const size_t need = batch_bytes(n_steps, H, W, sizeof(unsigned long long));
    if (need == 0) return FRLW_ERR_ARG;
    if (workspace_bytes < need) return FRLW_ERR_WORKSPACE;
    BatchTab T = {};
    ChainTab Ch = {};
    int n_emit = 0;
    for (int s = 0; s < n_steps; ++s) {
        T.lo[s] = step_lo[s]; T.hi[s] = step_hi[s];
        // kb_sae_last keeps an event with t > t0 (t is a 32-bit unsigned): the smallest t0 keeps every event, which is what
        // window_us <= 0 asks for -- the per-step filter without a second form of the kernel
        T.t0[s] = window_us[s] > 0 ? now[s] - window_us[s] : INT64_MIN;
        T.nowf[s] = Ch.nowf[s] = (float)now[s];
        Ch.slot[s] = emit[s] ? n_emit++ : -1;
    }
    Ch.n = n_steps;
    if (n_emit > 0 && !out_f32 && !out_u8) return FRLW_ERR_ARG;
    if (!tab_ranges(T, ev, n_steps)) return FRLW_ERR_ARG;
    SaeOutP q;
    q.n_lamda = n_lamda;
    for (int l = 0; l < FRLW_MAX_LAMDAS; ++l) q.lam[l] = l < n_lamda ? (float)lamdas[l] : 0.0f;
    q.mem_in = mem_in; q.mem_out = mem_out; q.out_f32 = out_f32; q.out_u8 = out_u8;
    hipStream_t st = (hipStream_t)stream;
    WsHeader *hdr = (WsHeader *)workspace;
    unsigned long long *last = (unsigned long long *)((char *)workspace + kHeaderBytes);
    const long long cells = 2ll * H * W;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kb_zero, dim3(grid_for(n_steps * cells / 2, 256)), dim3(256), 0, st, (uint4 *)last, n_steps * cells / 2, hdr);
    const BatchDecode D = decode_of(ev, H, W);
    if (T.blk[n_steps] > 0u) {
        if (ev->xmap) hipLaunchKernelGGL(kb_sae_last<true>, dim3(T.blk[n_steps]), dim3(kBT), 0, st, D, T, 1, last, hdr);
        else hipLaunchKernelGGL(kb_sae_last<false>, dim3(T.blk[n_steps]), dim3(kBT), 0, st, D, T, 1, last, hdr);
    }
    hipLaunchKernelGGL(kb_sae_chain_out, dim3(grid_for(cells, 256)), dim3(256), 0, st, (const unsigned long long *)last, cells, Ch, q);
    HIP_TRY(hipGetLastError());
    g_chain_counts[0].fetch_add(1ull, std::memory_order_relaxed);
    return FRLW_OK;
}

} // extern "C"
