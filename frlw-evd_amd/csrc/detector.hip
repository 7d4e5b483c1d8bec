// detector.hip -- YOLOX detector forward on gfx950: fp32-MFMA implicit-GEMM convolutions + glue.
//
// Replaces the eval forward of the reference's PyTorch modules (file:line in the reference):
//   BaseConv = Conv2d + BatchNorm2d + SiLU     core/yolox/models/network_blocks.py:33-65
//   Focus space-to-depth                       network_blocks.py:196-221
//   SPPBottleneck max-pools 5 / 9 / 13         network_blocks.py:131-153
//   nn.Upsample(scale_factor=2, nearest)       core/yolox/models/yolo_pafpn.py:29,92-103
//   YOLOXHead predictions + sigmoid + cat      core/yolox/models/yolo_head.py:186-213
//   decode_outputs + torchvision.ops.nms       yolo_head.py:258-303
//
// Design for MI355X
//   - activations are NHWC f32; a convolution is the GEMM  Y[M = B*Ho*Wo][N = Cout] = A[M][K] * W[K][N]
//     with K = (ky, kx, ci) and A gathered on the fly (implicit im2col, zero padding);
//   - the contraction runs on the matrix cores with v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate,
//     bit-for-bit an fmaf chain, so the result differs from PyTorch's fp32 only by summation order
//     (the 1e-3 tolerance of north_star rules out bf16 inputs; fp32 MFMA peak = 157 TFLOP/s);
//   - 256 threads = 4 wavefronts per 128x128 (or 64x64 / 128x32) output tile, BK = 16, A and B tiles
//     double-buffered in LDS k-major so a fragment read is 32 consecutive floats (conflict-free);
//   - BatchNorm is folded into the weights; bias, SiLU / sigmoid and the Bottleneck residual are
//     applied on the accumulators; every tensor can be a channel slice of a wider NHWC buffer, so
//     torch.cat never moves data (producers write straight into the consumer's concat buffer);
//   - the whole network is a plan of launches built once and replayed natively (frlw_det_run).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <type_traits>
#include <utility>
#include <vector>

#include "frlw_evd.h"

namespace {

#include "conv_mfma.h"

// ---- glue kernels ------------------------------------------------------------------------------
// Focus: (B, C, H, W) NCHW -> (B, H/2, W/2, 4C) NHWC, channel blocks TL, BL, TR, BR (network_blocks.py:205-217).
// One workgroup per `Wp` pixels of an output row (b, oy): the 2C input rows are read along x as float2 = the two column
// parities of one output pixel (coalesced; eight loads in flight per thread), transposed through LDS and the piece of the
// output row (Wp x 4C floats, contiguous) is written along its memory order.  (Until round 3: scalar loads, one exposed
// round trip each, and whole rows = three workgroups per CU -- 0.7 TB/s.)
__global__ __launch_bounds__(256) void k_focus(const float *x, int B, int C, int H, int W, float *y, int Wp)
{
    extern __shared__ float frow[]; // [Wp][4C + 1]
    const int Ho = H / 2, Wo = W / 2, C4 = 4 * C, LD = C4 + 1, parts = Wo / Wp;
    const int part = blockIdx.x % parts, row = blockIdx.x / parts;
    const int b = row / Ho, oy = row - b * Ho, j0 = part * Wp;
    // source rows: r = c * 2 + row parity -> x[b][c][2 oy + (r & 1)][:]; pair j of a row = output pixel j, parities 0 / 1
    const int n2 = 2 * C * Wp;
    for (int i0 = threadIdx.x; i0 < n2; i0 += 8 * 256) {
        float2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + 256 * u, ic = i < n2 ? i : n2 - 1;
            const int j = ic % Wp, r = ic / Wp;
            v[u] = *(const float2 *)(x + (((long long)b * C + (r >> 1)) * H + 2 * oy + (r & 1)) * W + 2 * (j0 + j));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + 256 * u;
            if (i < n2) {
                const int j = i % Wp, r = i / Wp, c = r >> 1, py = r & 1;
                frow[j * LD + py * C + c] = v[u].x;           // q = py: TL / BL
                frow[j * LD + (py + 2) * C + c] = v[u].y;     // q = py + 2: TR / BR
            }
        }
    }
    __syncthreads();
    float *dst = y + (((long long)b * Ho + oy) * Wo + j0) * C4;
    for (int i = threadIdx.x; i < Wp * C4; i += 256) dst[i] = frow[(i / C4) * LD + (i % C4)];
}

inline bool launch_focus(const float *x, int B, int C, int H, int W, float *y, hipStream_t s)
{
    int Wp = W / 2; // pixels per workgroup: pieces of at most 20 KB (eight workgroups per CU) where the row divides
    while (Wp % 2 == 0 && (size_t)Wp * (4 * C + 1) * sizeof(float) > 20 * 1024) Wp /= 2;
    const size_t lds = (size_t)Wp * (4 * C + 1) * sizeof(float);
    if (lds > 150 * 1024) return false;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)k_focus, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_focus, dim3(B * (H / 2) * ((W / 2) / Wp)), dim3(256), lds, s, x, B, C, H, W, y, Wp);
    return true;
}

// Focus + stem convolution in one kernel (network_blocks.py:205-217 followed by the 3x3 BaseConv of darknet.py:292):
// the space-to-depth image is never written.  A persistent workgroup keeps the whole weight operand (9 * 4 C0 rows of 32
// output channels) in LDS and walks 8 x 16 output tiles: the 10 x 18 halo patch of the Focus image is built in LDS straight
// from the NCHW input (zero outside the frame), and the nine taps are shifted views of that patch -- every input value is
// fetched once instead of nine times.  k pairing as in k_conv_mfma: lane half h supplies ci = 8 j + 4 h + e of a tap.
struct FocusStemArgs {
    const float *x; int H, W;            // (B, C0, H, W)
    const float *w, *bias;               // (9 * 4 C0, 32) rows (tap * 4 C0 + q * C0 + c), q = py + 2 px as in k_focus; bias (Cout)
    float *y; int Cout, y_cs, y_co;      // NHWC view of the output, Ho = H / 2, Wo = W / 2
    int tiles_x, tiles_y, n_tiles;
    int prec;                            // 1: w is the split bf16 image of the operand (conv_mfma.h), three bf16 MFMAs per product
    int npad;                            // columns of the operand: 32, or 64 (k_focus_stem_wide)
};

// floats of LDS in front of the patch: the weight operand (P = 1: its split image, ceil16(K) rows, + the quad offset table)
template <int C0, int P> constexpr int focus_stem_w_floats()
{
    return P == 1 ? (9 * 4 * C0 + 15) / 16 * 16 * 32 + (9 * C0 + 7) / 4 * 4 : 9 * 4 * C0 * 32;
}

template <int C0, int P = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_focus_stem(FocusStemArgs a)
{
    constexpr int CF = 4 * C0, PS = CF + 4, TH = 8, TW = 16, PH = TH + 2, PW = TW + 2, KT = 9 * CF;
    constexpr int QT = CF / 4, NQ = 9 * QT, NS = (NQ + 3) / 4; // P = 1: quads per tap, quads, bf16 k-steps of 16 k = 4 quads
    static_assert(C0 % 2 == 0, "quads are paired");
    extern __shared__ __attribute__((aligned(16))) float fs_lds[];
    float *Ws = fs_lds, *patch = fs_lds + focus_stem_w_floats<C0, P>();
    int *qoff = (int *)(fs_lds + NS * 16 * 32); // P = 1: float offset of quad g inside the patch, relative to the tap-(0, 0) pixel
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (P == 1) {
        for (int i = tid; i < NS * 4 * 32; i += 256) ((uint4 *)Ws)[i] = ((const uint4 *)a.w)[i];
        for (int g = tid; g < NQ; g += 256) { const int tap = g / QT; qoff[g] = ((tap / 3) * PW + tap % 3) * PS + 4 * (g - tap * QT); }
    } else {
        for (int i = tid; i < KT * 8; i += 256) ((float4 *)Ws)[i] = ((const float4 *)a.w)[i];
    }
    const int Ho = a.H / 2, Wo = a.W / 2;
    const int fh = lane >> 5, m = lane & 31, n = lane & 31;
    const int pp0 = (2 * wv + (m >> 4)) * PW + (m & 15);
    const float bias = n < a.Cout ? a.bias[n] : 0.0f;
    // This thread's share of a patch fill: items i = tid + 256 u -> (c, input row iy, column pair jx).  Everything but the
    // tile origin is fixed, so the decomposition is done once; the NEXT tile's values are fetched into registers while the
    // current tile is multiplied and written to LDS after it.
    constexpr int NI = (C0 * 2 * PH * PW + 255) / 256;
    int it_src[NI], it_dst[NI], it_yx[NI];
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        const int i = tid + 256 * u;
        const int jx = i % PW, r = i / PW, iy = r % (2 * PH), c = r / (2 * PH);
        it_src[u] = (c * a.H + iy) * a.W + 2 * jx;
        it_dst[u] = ((iy >> 1) * PW + jx) * PS + (iy & 1) * C0 + c;
        it_yx[u] = i < C0 * 2 * PH * PW ? (iy << 16) | (2 * jx) : -1;
    }
    float2 pv[NI];
    auto fetch = [&](int tile) {
        const int b = tile / (a.tiles_x * a.tiles_y), tr = tile - b * (a.tiles_x * a.tiles_y);
        const int y0 = 2 * ((tr / a.tiles_x) * TH - 1), x0 = 2 * ((tr % a.tiles_x) * TW - 1);
        const float *base = a.x + ((long long)b * C0 * a.H + y0) * a.W + x0;
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int y = y0 + (it_yx[u] >> 16), xc = x0 + (it_yx[u] & 0xFFFF);
            pv[u] = make_float2(0.f, 0.f);
            if (it_yx[u] >= 0 && (unsigned)y < (unsigned)a.H && (unsigned)xc < (unsigned)a.W) pv[u] = *(const float2 *)(base + it_src[u]);
        }
    };
    auto fill = [&](float *dst) {
#pragma unroll
        for (int u = 0; u < NI; ++u)
            if (it_yx[u] >= 0) { dst[it_dst[u]] = pv[u].x; dst[it_dst[u] + 2 * C0] = pv[u].y; } // px = 0: q = py; px = 1: q = py + 2
    };
    if ((int)blockIdx.x < a.n_tiles) fetch(blockIdx.x);
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int b = tile / (a.tiles_x * a.tiles_y), tr = tile - b * (a.tiles_x * a.tiles_y);
        const int fy0 = (tr / a.tiles_x) * TH, fx0 = (tr % a.tiles_x) * TW;
        __syncthreads(); // the previous tile's reads of the patch are done (first pass: the weights are in LDS)
        fill(patch);
        __syncthreads();
        if (tile + (int)gridDim.x < a.n_tiles) fetch(tile + gridDim.x);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        if constexpr (P == 1) {
            // k = tap * CF + channel is cut into quads g = k / 4; bf16 k-step st takes quads 4 st + h and 4 st + 2 + h of lane half h
            // (the pairing of conv_mfma.h: conv_split_kmem), the weights' split image has the matching records
            const float *pbase = patch + pp0 * PS;
            const uint4 *wrec = (const uint4 *)Ws + 2 * fh * 32 + n;
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                const f32x4 q0 = *(const f32x4 *)(pbase + qoff[4 * st + fh]);
                f32x4 q1 = {0.0f, 0.0f, 0.0f, 0.0f};
                if (4 * st + 2 < NQ) q1 = *(const f32x4 *)(pbase + qoff[4 * st + 2 + fh]); // (compile-time: the tail step of K = 360)
                const uint4 bh4 = wrec[st * 4 * 32], bl4 = wrec[st * 4 * 32 + 32];
                const u32x4 bh = {bh4.x, bh4.y, bh4.z, bh4.w}, bl = {bl4.x, bl4.y, bl4.z, bl4.w};
                u32x4 ah, al;
                conv_split8(q0, q1, ah, al);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bl), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
            }
        } else
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float *prow = patch + (pp0 + (t / 3) * PW + (t % 3)) * PS + fh * 4;
            const float *wrow = Ws + (t * CF + 4 * fh) * 32 + n;
#pragma unroll
            for (int j = 0; j < C0 / 2; ++j) {
                const float4 av = *(const float4 *)(prow + 8 * j);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wrow[(8 * j + 0) * 32], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wrow[(8 * j + 1) * 32], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wrow[(8 * j + 2) * 32], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wrow[(8 * j + 3) * 32], acc, 0, 0, 0);
            }
        }
        // C/D layout of the 32x32 MFMA: col = lane & 31 (channel), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (pixel of the wave)
        if (n < a.Cout) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int pm = (r & 3) + 8 * (r >> 2) + 4 * fh;
                const int oy = fy0 + 2 * wv + (pm >> 4), ox = fx0 + (pm & 15);
                if (oy < Ho && ox < Wo)
                    a.y[(((long long)b * Ho + oy) * Wo + ox) * a.y_cs + a.y_co + n] = act_apply(acc[r] + bias, ACT_SILU);
            }
        }
    }
}

// The same walk for the stems k_focus_stem does not take: up to 64 output channels (the Darknet-21 stem of the AED recipes) and
// C0 = 4, 8 (their 2- and 4-bin inputs).  NA = accumulator tiles of 32 channels per wavefront:
//   NA = 2: the whole (9 * 4 C0, 64) operand is resident and channels 0-31 / 32-63 are two f32x16 accumulators fed from ONE read of
//           the patch (one float4 per four k in float32, one split of the quad pair per bf16 k-step) -- the A side of the LDS
//           traffic and the bf16 split are paid once per 64 channels.  C0 <= 10: 90 KiB of weights + 31 KiB of patch at C0 = 10.
//   NA = 1: the workgroup keeps ONE 32-column half of the operand, half = blockIdx.x % (npad / 32).  With npad = 64 (C0 = 16, whose
//           144 KiB operand leaves no room for the 48 KiB patch in the CU's 160 KiB) two workgroups walk the same tiles, one per
//           half, and the input is read twice -- the second time out of L2.  With npad = 32 it is k_focus_stem for C0 = 4, 8.
template <int C0, int P, int NA> constexpr int focus_stem_wide_w_floats()
{
    return P == 1 ? (9 * 4 * C0 + 15) / 16 * 16 * 32 * NA + (9 * C0 + 7) / 4 * 4 : 9 * 4 * C0 * 32 * NA;
}

template <int C0, int P, int NA>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_focus_stem_wide(FocusStemArgs a)
{
    constexpr int CF = 4 * C0, PS = CF + 4, TH = 8, TW = 16, PH = TH + 2, PW = TW + 2, KT = 9 * CF, NL = 32 * NA;
    constexpr int QT = CF / 4, NQ = 9 * QT, NS = (NQ + 3) / 4; // P = 1: quads per tap, quads, bf16 k-steps of 16 k = 4 quads
    static_assert(C0 % 2 == 0, "quads are paired");
    extern __shared__ __attribute__((aligned(16))) float fsw_lds[];
    float *Ws = fsw_lds, *patch = fsw_lds + focus_stem_wide_w_floats<C0, P, NA>();
    int *qoff = (int *)(fsw_lds + NS * 16 * NL); // P = 1: float offset of quad g inside the patch, relative to the tap-(0, 0) pixel
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int halves = a.npad / NL, half = blockIdx.x % halves, wg = blockIdx.x / halves, n_wg = gridDim.x / halves;
    const int c0 = 32 * half; // first output channel (= operand column) of this workgroup
    if (P == 1) { // rows of NL records out of rows of npad
        for (int i = tid; i < NS * 4 * NL; i += 256) ((uint4 *)Ws)[i] = ((const uint4 *)a.w)[(i / NL) * a.npad + c0 + i % NL];
        for (int g = tid; g < NQ; g += 256) { const int tap = g / QT; qoff[g] = ((tap / 3) * PW + tap % 3) * PS + 4 * (g - tap * QT); }
    } else {
        for (int i = tid; i < KT * (NL / 4); i += 256)
            ((float4 *)Ws)[i] = ((const float4 *)a.w)[(i / (NL / 4)) * (a.npad / 4) + c0 / 4 + i % (NL / 4)];
    }
    const int Ho = a.H / 2, Wo = a.W / 2;
    const int fh = lane >> 5, m = lane & 31, n = lane & 31;
    const int pp0 = (2 * wv + (m >> 4)) * PW + (m & 15);
    float bias[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) bias[i] = c0 + 32 * i + n < a.Cout ? a.bias[c0 + 32 * i + n] : 0.0f;
    // the patch fill of k_focus_stem: this thread's items are fixed but for the tile origin; the NEXT tile's values are fetched
    // into registers while the current tile is multiplied
    constexpr int NI = (C0 * 2 * PH * PW + 255) / 256;
    int it_src[NI], it_dst[NI], it_yx[NI];
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        const int i = tid + 256 * u;
        const int jx = i % PW, r = i / PW, iy = r % (2 * PH), c = r / (2 * PH);
        it_src[u] = (c * a.H + iy) * a.W + 2 * jx;
        it_dst[u] = ((iy >> 1) * PW + jx) * PS + (iy & 1) * C0 + c;
        it_yx[u] = i < C0 * 2 * PH * PW ? (iy << 16) | (2 * jx) : -1;
    }
    float2 pv[NI];
    auto fetch = [&](int tile) {
        const int b = tile / (a.tiles_x * a.tiles_y), tr = tile - b * (a.tiles_x * a.tiles_y);
        const int y0 = 2 * ((tr / a.tiles_x) * TH - 1), x0 = 2 * ((tr % a.tiles_x) * TW - 1);
        const float *base = a.x + ((long long)b * C0 * a.H + y0) * a.W + x0;
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int y = y0 + (it_yx[u] >> 16), xc = x0 + (it_yx[u] & 0xFFFF);
            pv[u] = make_float2(0.f, 0.f);
            if (it_yx[u] >= 0 && (unsigned)y < (unsigned)a.H && (unsigned)xc < (unsigned)a.W) pv[u] = *(const float2 *)(base + it_src[u]);
        }
    };
    auto fill = [&](float *dst) {
#pragma unroll
        for (int u = 0; u < NI; ++u)
            if (it_yx[u] >= 0) { dst[it_dst[u]] = pv[u].x; dst[it_dst[u] + 2 * C0] = pv[u].y; } // px = 0: q = py; px = 1: q = py + 2
    };
    if (wg < a.n_tiles) fetch(wg);
    for (int tile = wg; tile < a.n_tiles; tile += n_wg) {
        const int b = tile / (a.tiles_x * a.tiles_y), tr = tile - b * (a.tiles_x * a.tiles_y);
        const int fy0 = (tr / a.tiles_x) * TH, fx0 = (tr % a.tiles_x) * TW;
        __syncthreads(); // the previous tile's reads of the patch are done (first pass: the weights are in LDS)
        fill(patch);
        __syncthreads();
        if (tile + n_wg < a.n_tiles) fetch(tile + n_wg);
        f32x16 acc[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
        if constexpr (P == 1) {
            // quads and records as in k_focus_stem; the split of the patch's quad pair serves both accumulators
            const float *pbase = patch + pp0 * PS;
            const uint4 *wrec = (const uint4 *)Ws + 2 * fh * NL + n;
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                const f32x4 q0 = *(const f32x4 *)(pbase + qoff[4 * st + fh]);
                f32x4 q1 = {0.0f, 0.0f, 0.0f, 0.0f};
                if (4 * st + 2 < NQ) q1 = *(const f32x4 *)(pbase + qoff[4 * st + 2 + fh]); // (compile-time: the tail step of K = 360)
                u32x4 ah, al;
                conv_split8(q0, q1, ah, al);
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const uint4 bh4 = wrec[st * 4 * NL + 32 * i], bl4 = wrec[st * 4 * NL + NL + 32 * i];
                    const u32x4 bh = {bh4.x, bh4.y, bh4.z, bh4.w}, bl = {bl4.x, bl4.y, bl4.z, bl4.w};
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, bh), acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bl), acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bh), acc[i], 0, 0, 0);
                }
            }
        } else
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float *prow = patch + (pp0 + (t / 3) * PW + (t % 3)) * PS + fh * 4;
            const float *wrow = Ws + (t * CF + 4 * fh) * NL + n;
#pragma unroll
            for (int j = 0; j < C0 / 2; ++j) {
                const float4 av = *(const float4 *)(prow + 8 * j);
                const float ae[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < NA; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae[e], wrow[(8 * j + e) * NL + 32 * i], acc[i], 0, 0, 0);
            }
        }
        // C/D layout of the 32x32 MFMA: col = lane & 31 (channel), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (pixel of the wave)
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int ch = c0 + 32 * i + n;
            if (ch < a.Cout) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pm = (r & 3) + 8 * (r >> 2) + 4 * fh;
                    const int oy = fy0 + 2 * wv + (pm >> 4), ox = fx0 + (pm & 15);
                    if (oy < Ho && ox < Wo)
                        a.y[(((long long)b * Ho + oy) * Wo + ox) * a.y_cs + a.y_co + ch] = act_apply(acc[i][r] + bias[i], ACT_SILU);
                }
            }
        }
    }
}

// which kernel a Focus + stem shape runs on: 0 = none (Focus and a convolution), 1 = k_focus_stem, 2 = k_focus_stem_wide; for 2,
// na = accumulator tiles per wavefront and lds = its dynamic LDS in bytes
inline int focus_stem_form(int C, int Cout, int prec, int *na, size_t *lds)
{
    if (Cout < 1 || Cout > 64 || (C != 4 && C != 8 && C != 10 && C != 16)) return 0;
    if (Cout <= 32 && (C == 10 || C == 16)) return 1;
    const int npad = Cout <= 32 ? 32 : 64;
    // measured slower than Focus + convolution (batch 32, 256 x 320: 0.356 against 0.349 ms): the half-per-workgroup
    // form in the bf16x3 arithmetic, whose shorter MFMA time no longer hides the second read of the input
    if (C == 16 && npad == 64 && prec == 1) return 0;
    *na = (npad == 64 && C != 16) ? 2 : 1; // C = 16: the 64-column operand does not fit beside the patch, one half per workgroup
    const int nl = 32 * *na, k16 = (36 * C + 15) / 16 * 16;
    const size_t wfl = prec == 1 ? (size_t)k16 * nl + (size_t)(9 * C + 7) / 4 * 4 : (size_t)36 * C * nl;
    *lds = (wfl + (size_t)180 * (4 * C + 4)) * sizeof(float);
    return *lds <= 160 * 1024 ? 2 : 0; // (the CU's LDS; hipFuncSetAttribute is asked at launch and its refusal is an error)
}

// the instantiation behind (C, prec, na) of focus_stem_form's form 2; NULL: none
using FocusStemWideFn = void (*)(FocusStemArgs);
template <int C0, int NA> inline FocusStemWideFn focus_stem_wide_prec(int prec)
{
    return prec == 1 ? (FocusStemWideFn)k_focus_stem_wide<C0, 1, NA> : (FocusStemWideFn)k_focus_stem_wide<C0, 0, NA>;
}
inline FocusStemWideFn focus_stem_wide_kernel(int C, int prec, int na)
{
    if (C == 16) return na == 1 ? focus_stem_wide_prec<16, 1>(prec) : nullptr;
    if (C == 10) return na == 2 ? focus_stem_wide_prec<10, 2>(prec) : nullptr;
    if (C == 8) return na == 2 ? focus_stem_wide_prec<8, 2>(prec) : focus_stem_wide_prec<8, 1>(prec);
    if (C == 4) return na == 2 ? focus_stem_wide_prec<4, 2>(prec) : focus_stem_wide_prec<4, 1>(prec);
    return nullptr;
}

// BFM stem, per-pixel part (core/Others/Temporal_Active_Focus.py:62-127, Temporal_Active_Focus_connect.forward
// up to `self.patch`): log2(TC) grouped 1x1 convolutions (weight norm already applied) + ReLU, the first 4
// channels of every stage concatenated (ER = 4 log2(TC) channels), residual MLP ER -> 4 ER -> ER with SiLU
// (Dropout2d = identity in eval), written straight in the Focus layout NHWC (B, H/2, W/2, 4 ER), channel blocks
// TL, BL, TR, BR.  One thread per input pixel, everything in registers, weights broadcast from LDS.
// Stage i: tc = TC >> i time groups; inputs per group 2 * (i == 0 ? 2 : 4), outputs per group 4, tc / 2 groups.
template <int TC> struct BfmDims {
    static constexpr int R = TC == 2 ? 1 : (TC == 4 ? 2 : 3);
    static constexpr int ER = 4 * R;
    static constexpr int stage_in(int i) { return (i == 0 ? 2 : 4) * (TC >> i); }
    static constexpr int stage_out(int i) { return 2 * (TC >> i); }
    static constexpr int stage_ing(int i) { return 2 * (i == 0 ? 2 : 4); }
    static constexpr int stage_off(int i) { return i == 0 ? 0 : stage_off(i - 1) + stage_out(i - 1) * stage_ing(i - 1) + stage_out(i - 1); }
    static constexpr int up_off = stage_off(R);
    static constexpr int down_off = up_off + 4 * ER * ER + 4 * ER;
    static constexpr int total = down_off + ER * 4 * ER + ER;
};

// stage I of the grouped 1x1 stack: v[0 .. n_in) -> ReLU(W v + b) in v[0 .. n_out), first four outputs to cat
template <int TC, int I>
__device__ __forceinline__ void bfm_stage(float (&v)[2 * TC], float (&cat)[4 * BfmDims<TC>::R], const float *w)
{
    using D = BfmDims<TC>;
    if constexpr (I < D::R) {
        constexpr int n_out = D::stage_out(I), in_g = D::stage_ing(I);
        const float *wi = w + D::stage_off(I), *bi = wi + n_out * in_g;
        float nxt[n_out];
#pragma unroll
        for (int oc = 0; oc < n_out; ++oc) {
            float acc = bi[oc];
#pragma unroll
            for (int k = 0; k < in_g; ++k) acc += wi[oc * in_g + k] * v[(oc >> 2) * in_g + k];
            nxt[oc] = acc > 0.0f ? acc : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) cat[4 * I + c] = nxt[c];
#pragma unroll
        for (int c = 0; c < n_out; ++c) v[c] = nxt[c];
        bfm_stage<TC, I + 1>(v, cat, w);
    }
}

template <int TC>
__global__ __launch_bounds__(256) void k_bfm_stem(const float *x, int B, int H, int W, const float *wts, float *y)
{
    using D = BfmDims<TC>;
    constexpr int C = 2 * TC, ER = D::ER;
    __shared__ float w[D::total];
    for (int i = threadIdx.x; i < D::total; i += 256) w[i] = wts[i];
    __syncthreads();
    const long long total = (long long)B * H * W;
    for (long long o = blockIdx.x * 256ll + threadIdx.x; o < total; o += (long long)gridDim.x * 256) {
        const int ix = (int)(o % W), iy = (int)((o / W) % H), b = (int)(o / ((long long)W * H));
        float v[C], cat[ER], out[ER];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = x[(((long long)b * C + c) * H + iy) * W + ix];
        bfm_stage<TC, 0>(v, cat, w);
        const float *wu = w + D::up_off, *bu = wu + 4 * ER * ER;
        const float *wd = w + D::down_off, *bd = wd + ER * 4 * ER;
#pragma unroll
        for (int c = 0; c < ER; ++c) out[c] = bd[c];
#pragma unroll 4
        for (int h = 0; h < 4 * ER; ++h) { // one hidden unit at a time: trans_up row, SiLU, trans_down column
            float acc = bu[h];
#pragma unroll
            for (int c = 0; c < ER; ++c) acc += wu[h * ER + c] * cat[c];
            const float hv = acc / (1.0f + expf(-acc));
#pragma unroll
            for (int c = 0; c < ER; ++c) out[c] += wd[c * 4 * ER + h] * hv;
        }
        const int q = (iy & 1) + 2 * (ix & 1); // 0 TL, 1 BL, 2 TR, 3 BR
        float *dst = y + ((((long long)b * (H / 2) + (iy >> 1)) * (W / 2) + (ix >> 1)) * 4 + q) * ER;
#pragma unroll
        for (int c = 0; c < ER; ++c) dst[c] = cat[c] + out[c];
    }
}

// nearest x2 upsample of an NHWC channel slice into another slice
__global__ void k_upsample2x(const float *x, int B, int H, int W, int C, int x_cs, int x_co, float *y, int y_cs, int y_co)
{
    const int Ho = 2 * H, Wo = 2 * W;
    const long long total = (long long)B * Ho * Wo * C;
    for (long long o = blockIdx.x * (long long)blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(o % C);
        const long long p = o / C;
        const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), b = (int)(p / ((long long)Wo * Ho));
        y[(((long long)b * Ho + oy) * Wo + ox) * y_cs + y_co + c] = x[(((long long)b * H + (oy >> 1)) * W + (ox >> 1)) * x_cs + x_co + c];
    }
}

// SPP: channels [0, C) of an NHWC buffer -> max-pools 5 / 9 / 13 (stride 1, -inf padding) into [C, 4C)
// (network_blocks.py:139-151).  max-pool 9 = 5 o 5 and 13 = 5 o 5 o 5 for stride-1 pools with -inf padding, and each
// 5 x 5 pool is a row pass followed by a column pass: 30 reads per output instead of 169.  One workgroup per
// (image, group of 32 channels) keeps the H x W x 32 tile in LDS through the six passes.
constexpr int kSppCh = 32;
constexpr int kSppMaxPix = 512; // 16 x 20 maps and smaller (the SPP sits on the stride-32 map): 2 x 66 KB of LDS at most
__global__ __launch_bounds__(256) void k_spp_pool(float *buf, int H, int W, int C, int cs)
{
    extern __shared__ float spp_lds[];
    const int b = blockIdx.y, c0 = blockIdx.x * kSppCh, tid = threadIdx.x, n = H * W;
    float (*ta)[kSppCh + 1] = (float (*)[kSppCh + 1])spp_lds;
    float (*tb)[kSppCh + 1] = (float (*)[kSppCh + 1])(spp_lds + (size_t)n * (kSppCh + 1));
    float *base = buf + (long long)b * n * cs;
    for (int e = tid; e < n * kSppCh; e += blockDim.x) {
        const int p = e / kSppCh, c = e - p * kSppCh;
        ta[p][c] = c0 + c < C ? base[(long long)p * cs + c0 + c] : -INFINITY;
    }
    __syncthreads();
    for (int round = 1; round <= 3; ++round) {
        for (int e = tid; e < n * kSppCh; e += blockDim.x) { // along x
            const int p = e / kSppCh, c = e - p * kSppCh, y = p / W, x = p - y * W;
            float m = ta[p][c];
            for (int d = 1; d <= 2; ++d) {
                if (x - d >= 0) m = fmaxf(m, ta[p - d][c]);
                if (x + d < W) m = fmaxf(m, ta[p + d][c]);
            }
            tb[p][c] = m;
        }
        __syncthreads();
        for (int e = tid; e < n * kSppCh; e += blockDim.x) { // along y, and out: round r = pool 4 r + 1
            const int p = e / kSppCh, c = e - p * kSppCh, y = p / W;
            float m = tb[p][c];
            for (int d = 1; d <= 2; ++d) {
                if (y - d >= 0) m = fmaxf(m, tb[p - d * W][c]);
                if (y + d < H) m = fmaxf(m, tb[p + d * W][c]);
            }
            ta[p][c] = m;
            if (c0 + c < C) base[(long long)p * cs + round * C + c0 + c] = m;
        }
        __syncthreads();
    }
}

// ---- decode + NMS (yolo_head.py:258-303) ----------------------------------------------------------
// Three launches so that the quadratic part runs on the whole GPU (round 6; one workgroup per image did everything before:
// 32 or 8 of 256 CUs, a third of the forward's time on top of it):
//   k_decode_sort  one workgroup per image: decode, candidates obj > thr compacted in anchor order, sorted by score
//                  (descending, ties by anchor index = a stable sort); the order and the sorted xyxy boxes go to the workspace
//   k_nms_matrix   (image, 64-row block, 64-column word) wavefronts over the upper triangle: bit j of mask[row i][word] =
//                  "box i suppresses box j" = j > i and IoU(i, j) > thr -- every CU computes IoUs
//   k_nms_sweep    one small workgroup per image walks the rows in score order on 64-bit masks (thread t owns word t of the
//                  `removed` set; a chunk of 64 rows is resolved by the owner of its diagonal word, its kept rows are OR-ed
//                  into the later words; the next chunk's masks are in flight meanwhile); the kept bits go to the workspace
//   k_nms_emit     (image, 256 candidates) workgroups write the kept boxes in score order.
// Same comparison everywhere: inter / (area_i + area_j - inter) > thr on xyxy corners without + 1, f32, this operation order.
struct DecodeArgs {
    const float *raw; // (B, A, 5 + nc): [reg 4, sigmoid(obj), sigmoid(cls)...]
    int A, nc, n_levels;
    int lvl_h[4], lvl_w[4], lvl_stride[4];
    float obj_thr, iou_thr;
    float *decoded;   // optional (B, A, 5 + nc): boxes decoded, rest copied
    float *dets;      // (B, A, 6): [cx, cy, w, h, argmax cls, obj * max cls] in descending-score order
    int *counts;      // (B, 1 + A): detections per image (0 = the reference's single all-zero row), then the score order
    float *ws;        // (B, nms_ws_floats(A)): per image [n, pad x3 | kept bits u64 x 128 | sorted boxes float4 x A64 | mask u64 [A64][A64 / 64]]
};

constexpr int NMS_MAX = 8192; // candidates per image the device NMS holds (1 Mpx detector shape: 6720 anchors)
constexpr int kNmsHdr = 4 + 2 * (NMS_MAX / 64); // floats in front of the boxes: n, pad x3, the kept bits of k_nms_sweep
__host__ __device__ inline int nms_a64(int A) { return A < NMS_MAX ? (A + 63) / 64 * 64 : NMS_MAX; } // candidates <= min(A, NMS_MAX)
__host__ __device__ inline long long nms_ws_floats(int A)
{
    const long long a64 = nms_a64(A);
    return kNmsHdr + 4 * a64 + 2 * (a64 / 64) * a64;
}
// LDS of k_decode_sort (dynamic): the sort keys, skey[n] f32 | sidx[n] i32, n = candidates rounded up to a power of two.
__host__ __device__ inline size_t nms_lds_bytes(int cap) { return (size_t)cap * 8 + 64; }

__device__ __forceinline__ void nms_anchor_box(const DecodeArgs &a, int b, int i, float &cx, float &cy, float &w, float &h)
{
    int lvl = 0, off = i;
    while (lvl + 1 < a.n_levels && off >= a.lvl_h[lvl] * a.lvl_w[lvl]) { off -= a.lvl_h[lvl] * a.lvl_w[lvl]; ++lvl; }
    const float gx = (float)(off % a.lvl_w[lvl]), gy = (float)(off / a.lvl_w[lvl]), s = (float)a.lvl_stride[lvl];
    const float *r = a.raw + ((long long)b * a.A + i) * (5 + a.nc);
    cx = (r[0] + gx) * s;      // (xy + grid) * stride, yolo_head.py:271
    cy = (r[1] + gy) * s;
    w = (r[2] * r[2]) * s;     // square(wh) * stride, :272
    h = (r[3] * r[3]) * s;
}

__global__ __launch_bounds__(1024) void k_decode_sort(DecodeArgs a, int cap)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
    float *skey = (float *)nms_lds;
    int *sidx = (int *)(skey + cap);
    __shared__ int scount;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int F = 5 + a.nc;
    int *count_out = a.counts + (long long)b * (1 + a.A);
    int *order = count_out + 1; // anchor index of every candidate in score order
    float *wsb = a.ws + (long long)b * nms_ws_floats(a.A);
    int *n_out = (int *)wsb;
    float4 *boxes = (float4 *)(wsb + kNmsHdr);
    if (tid == 0) scount = 0;
    __syncthreads();
    // ---- decode; candidates = obj > threshold, compacted in anchor order by a block-wide stable scan
    // (sort stability must not depend on thread timing): do it in chunks of nt anchors
    for (int base = 0; base < a.A; base += nt) {
        const int i = base + tid;
        bool cand = false;
        float obj = 0;
        if (i < a.A) {
            const float *r = a.raw + ((long long)b * a.A + i) * F;
            obj = r[4];
            cand = obj > a.obj_thr;    // :276
            if (a.decoded) {
                float cx, cy, w, h;
                nms_anchor_box(a, b, i, cx, cy, w, h);
                float *d = a.decoded + ((long long)b * a.A + i) * F;
                d[0] = cx; d[1] = cy; d[2] = w; d[3] = h;
                for (int c = 4; c < F; ++c) d[c] = r[c];
            }
        }
        // stable compaction inside the chunk: rank = number of candidates with a smaller thread id
        const unsigned long long bal = __ballot(cand);
        __shared__ int wcount[16];
        const int lane = tid & 63, wv = tid >> 6;
        if (lane == 0) wcount[wv] = __popcll(bal);
        __syncthreads();
        int pre = scount;
        for (int k = 0; k < wv; ++k) pre += wcount[k];
        const int slot = pre + __popcll(bal & ((1ull << lane) - 1ull));
        if (cand && slot < cap) { skey[slot] = obj; sidx[slot] = i; }
        __syncthreads();
        if (tid == 0) { int t = scount; for (int k = 0; k < (nt + 63) / 64; ++k) t += wcount[k]; scount = t; }
        __syncthreads();
    }
    if (scount > cap) { if (tid == 0) { *count_out = -1; *n_out = -1; } return; } // more candidates than the LDS holds (A > 8192 only)
    const int n = scount;
    if (tid == 0) *n_out = n;
    if (n == 0) { if (tid == 0) *count_out = 0; return; }
    // ---- sort candidates by score descending, ties by anchor index ascending (= a stable sort):
    // bitonic network over the next power of two, keys (score, -index); one compare-exchange per thread and step
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int i = n + tid; i < np2; i += nt) { skey[i] = -INFINITY; sidx[i] = 0x7fffffff; }
    __syncthreads();
    for (int size = 2; size <= np2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = tid; p < (np2 >> 1); p += nt) {
                const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1)), j = i | stride;
                const bool up = (i & size) == 0; // descending blocks first
                const float ki = skey[i], kj = skey[j];
                const int ii = sidx[i], ij = sidx[j];
                const bool i_first = ki > kj || (ki == kj && ii < ij); // i should precede j in the final order
                if (up ? !i_first : i_first) { skey[i] = kj; skey[j] = ki; sidx[i] = ij; sidx[j] = ii; }
            }
            __syncthreads();
        }
    }
    // ---- the order and the sorted corner boxes leave for the workspace (x1, y1, x2, y2 as :280 forms them)
    for (int i = tid; i < n; i += nt) {
        const int anchor = sidx[i];
        order[i] = anchor;
        float cx, cy, w, h;
        nms_anchor_box(a, b, anchor, cx, cy, w, h);
        boxes[i] = make_float4(cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2);
    }
}

// grid (words / 4, row blocks, B), 4 wavefronts per workgroup: wavefront = one 64 x 64 block of the suppression matrix.
__global__ __launch_bounds__(256) void k_nms_matrix(DecodeArgs a)
{
    const int b = blockIdx.z, rb = blockIdx.y, lane = threadIdx.x & 63, cw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long a64 = nms_a64(a.A);
    float *wsb = a.ws + (long long)b * nms_ws_floats(a.A);
    const int n = *(const int *)wsb;
    if (n <= 0 || cw < rb || rb * 64 >= n || cw * 64 >= n) return; // (wave-uniform; no barrier in this kernel)
    const float4 *boxes = (const float4 *)(wsb + kNmsHdr);
    unsigned long long *mask = (unsigned long long *)(wsb + kNmsHdr + 4 * a64);
    const int gi = rb * 64 + lane, gj = cw * 64 + lane;
    const float4 rbx = gi < n ? boxes[gi] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 cbx = gj < n ? boxes[gj] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float r_area = (rbx.z - rbx.x) * (rbx.w - rbx.y), c_area = (cbx.z - cbx.x) * (cbx.w - cbx.y);
    const bool thr_nonneg = a.iou_thr >= 0.0f;
    unsigned long long mine = 0ull;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
        const float x1 = __shfl(rbx.x, i), y1 = __shfl(rbx.y, i), x2 = __shfl(rbx.z, i), y2 = __shfl(rbx.w, i), ai = __shfl(r_area, i);
        const float xx1 = fmaxf(x1, cbx.x), yy1 = fmaxf(y1, cbx.y);
        const float xx2 = fminf(x2, cbx.z), yy2 = fminf(y2, cbx.w);
        const float iw = fmaxf(xx2 - xx1, 0.0f), ih = fmaxf(yy2 - yy1, 0.0f);
        const float inter = iw * ih;
        const bool pair = rb * 64 + i < gj && gj < n && rb * 64 + i < n;
        unsigned long long bal = 0ull;
        // no overlap anywhere in this row of the block: 0 / x is 0 or NaN, never > thr (thr >= 0) -- the division is skipped
        if (!thr_nonneg || __ballot(pair && inter > 0.0f) != 0ull)
            bal = __ballot(pair && inter / (ai + c_area - inter) > a.iou_thr);
        if (lane == i) mine = bal;
    }
    mask[(long long)gi * (a64 / 64) + cw] = mine; // rows at or behind n: zero (one scattered 8-byte store per 64 x 64 IoUs)
}

constexpr int kSweepThreads = 128; // = NMS_MAX / 64 words
__global__ __launch_bounds__(kSweepThreads) void k_nms_sweep(DecodeArgs a)
{
    __shared__ unsigned long long keptw[kSweepThreads];
    const int b = blockIdx.x, t = threadIdx.x;
    const long long a64 = nms_a64(a.A);
    const int nw = (int)(a64 / 64);
    float *wsb = a.ws + (long long)b * nms_ws_floats(a.A);
    const int n = *(const int *)wsb;
    if (n <= 0) return; // (k_decode_sort has written the count: 0 or -1)
    const int nwn = (n + 63) >> 6;
    // row-major mask: the 64 lanes of a wavefront read 64 consecutive words of one row (thread t = word t)
    const unsigned long long *col = (const unsigned long long *)(wsb + kNmsHdr + 4 * a64) + t;
    const bool active = t < nwn;
    unsigned long long rem = 0ull;
    unsigned long long bufA[64], bufB[64];
    auto load = [&](unsigned long long (&m)[64], int c) {
        if (active && t >= c) {
            const unsigned long long *src = col + (long long)c * 64 * nw;
#pragma unroll
            for (int i = 0; i < 64; ++i) m[i] = src[(long long)i * nw];
        }
    };
    auto step = [&](unsigned long long (&cur)[64], unsigned long long (&nxt)[64], int c) {
        if (c + 1 < nwn) load(nxt, c + 1); // the next chunk's masks fly while this one is resolved
        const int nb = n - c * 64 < 64 ? n - c * 64 : 64;
        if (t == c) { // the owner of the diagonal word: the chunk's 64 rows in score order
            unsigned long long sup = rem, kept = 0ull;
            unsigned long long any = 0ull;
#pragma unroll
            for (int i = 0; i < 64; ++i) any |= cur[i];
            const unsigned long long valid = nb == 64 ? ~0ull : (1ull << nb) - 1ull;
            if ((any & valid) == 0ull) kept = ~sup & valid; // nobody inside the chunk suppresses anybody
            else {
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    const bool keep = i < nb && !((sup >> i) & 1ull);
                    kept |= keep ? 1ull << i : 0ull;
                    sup |= keep ? cur[i] : 0ull;
                }
            }
            keptw[c] = kept;
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // (LDS only: the prefetch above stays in flight)
        const unsigned long long kept = keptw[c];
        if (active && t > c) {
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                if ((kept >> (8 * g)) & 0xffull) { // wave-uniform
#pragma unroll
                    for (int i = 8 * g; i < 8 * g + 8; ++i) rem |= ((kept >> i) & 1ull) ? cur[i] : 0ull;
                }
            }
        }
    };
    load(bufA, 0);
    for (int c = 0; c < nwn; c += 2) {
        step(bufA, bufB, c);
        if (c + 1 < nwn) step(bufB, bufA, c + 1);
    }
    __syncthreads();
    unsigned long long *kept_out = (unsigned long long *)(wsb + 4);
    if (t < nwn) kept_out[t] = keptw[t];
}

// kept boxes -> dets rows in score order: output row = kept boxes in front.  grid (ceil(A64 / 256), B)
__global__ __launch_bounds__(256) void k_nms_emit(DecodeArgs a)
{
    __shared__ int wpre[NMS_MAX / 64 + 1];
    const int b = blockIdx.y, t = threadIdx.x;
    const int F = 5 + a.nc;
    float *wsb = a.ws + (long long)b * nms_ws_floats(a.A);
    const int n = *(const int *)wsb;
    if (n <= 0 || (int)blockIdx.x * 256 >= n) return;
    const unsigned long long *keptw = (const unsigned long long *)(wsb + 4);
    int *count_out = a.counts + (long long)b * (1 + a.A);
    const int *order = count_out + 1;
    const int nwn = (n + 63) >> 6;
    // kept boxes in front of every word: wavefront 0 scans the <= 128 popcounts (two per lane)
    if (t < 64) {
        const int c0 = 2 * t < nwn ? __popcll(keptw[2 * t]) : 0, c1 = 2 * t + 1 < nwn ? __popcll(keptw[2 * t + 1]) : 0;
        int inc = c0 + c1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(inc, off);
            if (t >= off) inc += v;
        }
        const int ex = inc - c0 - c1;
        if (2 * t < nwn) wpre[2 * t] = ex;
        if (2 * t + 1 < nwn) wpre[2 * t + 1] = ex + c0;
        if (t == 63) wpre[nwn] = inc; // all kept boxes
    }
    __syncthreads();
    if (blockIdx.x == 0 && t == 0) *count_out = wpre[nwn];
    const int i = blockIdx.x * 256 + t;
    if (i >= n) return;
    const unsigned long long kw = keptw[i >> 6];
    if (!((kw >> (i & 63)) & 1ull)) return;
    const int row = wpre[i >> 6] + __popcll(kw & ((1ull << (i & 63)) - 1ull));
    const int anchor = order[i];
    const float *r = a.raw + ((long long)b * a.A + anchor) * F;
    int best = 0;
    float bv = r[5];
    for (int c = 1; c < a.nc; ++c) if (r[5 + c] > bv) { bv = r[5 + c]; best = c; } // first max, like argmax
    float *d = a.dets + ((long long)b * a.A + row) * 6;
    nms_anchor_box(a, b, anchor, d[0], d[1], d[2], d[3]);
    d[4] = (float)best;
    d[5] = r[4] * bv; // obj * max cls, yolo_head.py:301
}

// ---- plan ------------------------------------------------------------------------------------------
enum OpType : int { OP_CONV = 0, OP_FOCUS = 1, OP_UPSAMPLE = 2, OP_SPP = 3, OP_DECODE = 4, OP_FORK = 5, OP_JOIN = 6, OP_BFM = 7, OP_PRED = 8, OP_FOCUS_STEM = 9 };
constexpr int kSideLanes = 2; // independent sub-graphs (the head levels) run on side streams

struct PredInferArgs {
    const float *x; int cs, co, C; // feature buffer: pixel stride, channel offset of reg_feat (cls_feat follows at + C)
    const float *w, *bias;         // (F, C) rows as above, (F)
    float *out; int F, hw, off; long long out_bs; // F = 5 + nc; anchors of this level per image, first anchor, image stride
    long long M;
};

struct Op {
    int type;
    int lane;               // 0 = the caller's stream, 1..kSideLanes = side streams
    int src, dst, res;      // buffer indices
    ConvArgs conv;          // pointers x / y / res filled at run time; w / bias are baked
    int C, H, W, cs_src, co_src, cs_dst, co_dst;
    DecodeArgs dec; int decoded_buf, dets_buf, counts_buf, nms_buf;
    int ups_buf;            // OP_CONV: > 0 = the buffer that also receives the output upsampled x2 (ConvArgs::y2); 0 (the network input's index): none
    const float *bfm_w;     // OP_BFM: packed weights (device)
    PredInferArgs pred;     // OP_PRED
    FocusStemArgs fstem;    // OP_FOCUS_STEM
};

// ---- prediction convolutions of one head level (yolo_head.py:205-231, eval branch) ------------------------------------
// out[b][off + p][j] = f_j(feat[b][p] . w[j] + bias[j]): rows j < 5 (reg, obj) read the first C channels of the level's
// [reg_feat | cls_feat] buffer, rows j >= 5 (cls) the second C; f = sigmoid for j >= 4.  5 + nc outputs per 2 C inputs is no
// work for a matrix pipe: one wavefront owns whole rows (lane l holds float4 chunk l of a row and of every weight row), the
// partial dots are folded over the lanes with a halving butterfly, and the row leaves as 5 + nc consecutive floats of the
// (B, A, 5 + nc) head tensor.  HBM-bound: 2 C * 4 bytes per anchor.

template <int NG>
__device__ __forceinline__ void pred_infer_body(const PredInferArgs &a, int block, int n_blocks)
{
    const int lane = threadIdx.x & 63, wave = block * 4 + (threadIdx.x >> 6), n_waves = n_blocks * 4;
    const int c4n = a.C / 4;
    const bool has = lane < c4n;
    float4 w[NG * 8];
#pragma unroll
    for (int j = 0; j < NG * 8; ++j) w[j] = (j < a.F && has) ? *(const float4 *)(a.w + (long long)j * a.C + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int sel = ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1); // output index this lane ends up with
    float bias[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) bias[g] = g * 8 + sel < a.F ? a.bias[g * 8 + sel] : 0.0f;
    for (long long m = wave; m < a.M; m += n_waves) {
        const float *row = a.x + m * a.cs + a.co + 4 * lane;
        const float4 xr = has ? *(const float4 *)row : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 xc = has ? *(const float4 *)(row + a.C) : make_float4(0.f, 0.f, 0.f, 0.f);
        float res[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int j = g * 8 + t;
                const float4 x = j < 5 ? xr : xc;
                v[t] = x.x * w[j].x + x.y * w[j].y + x.z * w[j].z + x.w * w[j].w;
            }
            float q[4], r2[2];
            const bool h1 = lane & 32, h2 = lane & 16, h3 = lane & 8;
#pragma unroll
            for (int t = 0; t < 4; ++t) q[t] = (h1 ? v[4 + t] : v[t]) + __shfl_xor(h1 ? v[t] : v[4 + t], 32, 64);
#pragma unroll
            for (int t = 0; t < 2; ++t) r2[t] = (h2 ? q[2 + t] : q[t]) + __shfl_xor(h2 ? q[t] : q[2 + t], 16, 64);
            float c = (h3 ? r2[1] : r2[0]) + __shfl_xor(h3 ? r2[0] : r2[1], 8, 64);
            c += __shfl_xor(c, 4, 64);
            c += __shfl_xor(c, 2, 64);
            c += __shfl_xor(c, 1, 64);
            res[g] = c;
        }
        if ((lane & 7) == 0) {
            const long long b = m / a.hw, p = m - b * a.hw;
            float *o = a.out + b * a.out_bs + (a.off + p) * a.F;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int j = g * 8 + sel;
                if (j < a.F) {
                    const float t = res[g] + bias[g];
                    o[j] = j >= 4 ? act_apply(t, ACT_SIGMOID) : t;
                }
            }
        }
    }
}

// the head levels' prediction ops as ONE launch (consecutive OP_PRED ops of a plan: frlw_det_run merges them): workgroups
// [first[l], first[l + 1]) serve level l
struct PredInferMulti { PredInferArgs lv[4]; int first[5]; int n; };
template <int NG>
__global__ __launch_bounds__(256) void k_pred_infer(PredInferMulti a)
{
    int l = 0;
    while (l + 1 < a.n && (int)blockIdx.x >= a.first[l + 1]) ++l;
    pred_infer_body<NG>(a.lv[l], (int)blockIdx.x - a.first[l], a.first[l + 1] - a.first[l]);
}

int grid_1d(long long n) { long long g = (n + 255) / 256; if (g > 4096) g = 4096; if (g < 1) g = 1; return (int)g; }

} // namespace

struct frlw_detector {
    std::vector<Op> ops;
    int scratch_buf = -1;        // split-K partial sums: (1 + kSideLanes) regions of scratch_floats
    long long scratch_floats = 0;
    int cur_lane = 0;
    int prec = 0;                // convolution operands added from now on: 0 float32 [K][Npad], 1 the split bf16 image
    bool have_side = false;
    hipStream_t side[kSideLanes] = {};
    hipEvent_t ev_fork = nullptr, ev_join[kSideLanes] = {};
};

// Bare fp32 MFMA loop: every wavefront of every CU issues v_mfma_f32_32x32x2_f32 back to back on four accumulators,
// operands in registers (random, so that the chip sees the switching activity of real data).  What this sustains is the
// rate the convolutions can at best approach on this chip under load: the 157.3 TFLOP/s of the data sheet assume 2.4 GHz.
template <int NACC>
__global__ __launch_bounds__(256) void k_mfma_f32_rate(int iters, const float *seed, float *sink)
{
    const int lane = threadIdx.x & 63;
    float a0 = seed[lane], a1 = seed[64 + lane], b0 = seed[128 + lane], b1 = seed[192 + lane];
    f32x16 c00, c01, c10, c11;
#pragma unroll
    for (int r = 0; r < 16; ++r) { c00[r] = 0.f; c01[r] = 0.f; c10[r] = 0.f; c11[r] = 0.f; }
#pragma nounroll
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, c00, 0, 0, 0);
            c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, c01, 0, 0, 0);
            if (NACC == 4) {
                c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, c10, 0, 0, 0);
                c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c11, 0, 0, 0);
            } else if (NACC == 2) {
                c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, c00, 0, 0, 0);
                c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c01, 0, 0, 0);
            } else {
                c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, c00, 0, 0, 0);
                c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c00, 0, 0, 0);
            }
        }
        a0 = -a0; b1 = -b1; // keep the sums bounded
    }
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += c00[r] + c01[r] + c10[r] + c11[r];
    if (t == 123.456f) sink[0] = t; // never true: keeps the loop alive
}

extern "C" {

// iters x 32 MFMAs per wavefront on `blocks` workgroups of 4 wavefronts; `seed`: 256 random floats (device).
int frlw_selftest_mfma_f32_rate(int blocks, int iters, const float *seed, float *sink, frlw_stream_t stream)
{
    int blocks_sel = 4;
    if (blocks < 0) { blocks_sel = (-blocks) % 10; blocks = (-blocks) / 10; } // developer experiments: -(blocks * 10 + nacc)
    if (blocks < 1 || iters < 1 || !seed || !sink) return FRLW_ERR_ARG;
    const int nacc = iters < 0 ? 0 : 4; // (developer experiments: negative blocks select fewer accumulators)
    (void)nacc;
    if (blocks_sel == 2) hipLaunchKernelGGL(k_mfma_f32_rate<2>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, iters, seed, sink);
    else if (blocks_sel == 1) hipLaunchKernelGGL(k_mfma_f32_rate<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, iters, seed, sink);
    else hipLaunchKernelGGL(k_mfma_f32_rate<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, iters, seed, sink);
    return hipGetLastError() == hipSuccess ? FRLW_OK : FRLW_ERR_HIP;
}

frlw_detector_t *frlw_det_create(void) { return new frlw_detector(); }
void frlw_det_destroy(frlw_detector_t *d)
{
    if (d && d->have_side) {
        for (int i = 0; i < kSideLanes; ++i) { (void)hipStreamDestroy(d->side[i]); (void)hipEventDestroy(d->ev_join[i]); }
        (void)hipEventDestroy(d->ev_fork);
    }
    delete d;
}

int frlw_det_set_lane(frlw_detector_t *d, int lane)
{
    if (!d || lane < 0 || lane > kSideLanes) return FRLW_ERR_ARG;
    d->cur_lane = lane;
    return FRLW_OK;
}

int frlw_det_set_precision(frlw_detector_t *d, int precision)
{
    if (!d || precision < 0 || precision > 1) return FRLW_ERR_ARG;
    d->prec = precision;
    return FRLW_OK;
}

size_t frlw_conv_split_operand_bytes(int K, int Npad)
{
    if (K < 1 || Npad < 1) return 0;
    return (size_t)((K + 15) / 16) * 4 * (size_t)Npad * 16;
}

int frlw_conv_split_operand(const float *w, int K, int Npad, void *out, frlw_stream_t stream)
{
    (void)hipGetLastError();
    if (!w || !out || K < 1 || Npad < 1) return FRLW_ERR_ARG;
    const long long nrec = (long long)((K + 15) / 16) * 4 * Npad;
    hipLaunchKernelGGL(k_conv_split_operand, dim3(conv_grid_1d(nrec)), dim3(256), 0, (hipStream_t)stream, w, K, Npad, (uint4 *)out);
    if (hipGetLastError() != hipSuccess) return FRLW_ERR_HIP;
    return FRLW_OK;
}

int frlw_det_add_fork(frlw_detector_t *d)
{
    if (!d) return FRLW_ERR_ARG;
    Op op = {};
    op.type = OP_FORK;
    d->ops.push_back(op);
    return FRLW_OK;
}

int frlw_det_add_join(frlw_detector_t *d)
{
    if (!d) return FRLW_ERR_ARG;
    Op op = {};
    op.type = OP_JOIN;
    d->ops.push_back(op);
    return FRLW_OK;
}
int frlw_det_num_ops(const frlw_detector_t *d) { return d ? (int)d->ops.size() : 0; }

int frlw_det_set_scratch(frlw_detector_t *d, int buf, int64_t n_floats)
{
    if (!d) return FRLW_ERR_ARG;
    d->scratch_buf = buf;
    d->scratch_floats = n_floats;
    return FRLW_OK;
}

int frlw_det_add_focus(frlw_detector_t *d, int src_buf, int C, int H, int W, int dst_buf)
{
    if (!d || C < 1 || (H & 1) || (W & 1)) return FRLW_ERR_ARG;
    Op op = {};
    op.type = OP_FOCUS; op.src = src_buf; op.dst = dst_buf; op.C = C; op.H = H; op.W = W;
    op.lane = d->cur_lane;
    d->ops.push_back(op);
    return FRLW_OK;
}

int frlw_focus_nhwc(const float *x, int B, int C, int H, int W, float *y, frlw_stream_t stream)
{
    (void)hipGetLastError();
    if (!x || !y || B < 1 || C < 1 || (H & 1) || (W & 1)) return FRLW_ERR_ARG;
    if (!launch_focus(x, B, C, H, W, y, (hipStream_t)stream)) return FRLW_ERR_UNSUPPORTED;
    return hipGetLastError() == hipSuccess ? FRLW_OK : FRLW_ERR_HIP;
}

int frlw_det_add_focus_stem(frlw_detector_t *d, int src_buf, int C, int H, int W, const float *w_dev, const float *bias_dev,
                            int Cout, int dst_buf, int dst_cs, int dst_co)
{
    if (!d || !w_dev || !bias_dev || (H & 1) || (W & 1) || Cout < 1) return FRLW_ERR_ARG;
    int na = 1; size_t wide_lds = 0;
    const int form = focus_stem_form(C, Cout, d->prec, &na, &wide_lds);
    if (form == 0) return FRLW_ERR_UNSUPPORTED; // other stems: frlw_det_add_focus + frlw_det_add_conv
    if (form == 2) { // the dynamic LDS is asked for HERE, where the builder can still take the unfused pair
        const FocusStemWideFn kern = focus_stem_wide_kernel(C, d->prec, na);
        if (!kern) return FRLW_ERR_UNSUPPORTED;
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) { // (no device: a plan built for its op list, never run)
            if (hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wide_lds) != hipSuccess) {
                (void)hipGetLastError();
                return FRLW_ERR_UNSUPPORTED;
            }
        } else (void)hipGetLastError();
    }
    Op op = {};
    op.type = OP_FOCUS_STEM; op.src = src_buf; op.dst = dst_buf; op.C = C;
    FocusStemArgs &a = op.fstem;
    a.H = H; a.W = W; a.w = w_dev; a.bias = bias_dev; a.Cout = Cout; a.y_cs = dst_cs; a.y_co = dst_co;
    a.prec = d->prec; // 1: w_dev is the split image of the (9 * 4 C, npad) operand (frlw_conv_split_operand)
    a.npad = Cout <= 32 ? 32 : 64;
    a.tiles_x = (W / 2 + 15) / 16; a.tiles_y = (H / 2 + 7) / 8;
    op.lane = d->cur_lane;
    d->ops.push_back(op);
    return FRLW_OK;
}

int frlw_det_bfm_weight_count(int C)
{
    switch (C) {
    case 4: return BfmDims<2>::total;
    case 8: return BfmDims<4>::total;
    case 16: return BfmDims<8>::total;
    default: return 0;
    }
}

int frlw_det_add_bfm_stem(frlw_detector_t *d, int src_buf, int C, int H, int W, const float *weights, int n_weights,
                          int dst_buf)
{
    if (!d || !weights || (H & 1) || (W & 1)) return FRLW_ERR_ARG;
    const int want = frlw_det_bfm_weight_count(C);
    if (want == 0) return FRLW_ERR_UNSUPPORTED; // TAF with K = 2, 4 or 8 FIFO slots
    if (n_weights != want) return FRLW_ERR_ARG;
    Op op = {};
    op.type = OP_BFM; op.src = src_buf; op.dst = dst_buf; op.C = C; op.H = H; op.W = W; op.bfm_w = weights;
    op.lane = d->cur_lane;
    d->ops.push_back(op);
    return FRLW_OK;
}

int frlw_det_add_upsample(frlw_detector_t *d, int src_buf, int cs_src, int co_src, int C, int H, int W,
                          int dst_buf, int cs_dst, int co_dst)
{
    if (!d) return FRLW_ERR_ARG;
    if (!d->ops.empty()) {
        // the slice was written by the convolution added just before (the FPN's lateral / reduce 1x1, yolo_pafpn.py:92-100): its
        // epilogue stores the upsampled copy as well -- four more 16-byte stores per output row instead of a launch
        Op &pv = d->ops.back();
        const ConvArgs &pc = pv.conv;
        if (pv.type == OP_CONV && pv.lane == d->cur_lane && pv.dst == src_buf && pc.y_cs == cs_src && pc.y_co == co_src && pc.Cout == C &&
            pc.Ho == H && pc.Wo == W && pc.y_rp == 0 && pv.ups_buf == 0 && dst_buf > 0 && ((cs_dst | co_dst | C) & 3) == 0) {
            pv.ups_buf = dst_buf;
            pv.conv.y2_cs = cs_dst; pv.conv.y2_co = co_dst; pv.conv.y2_bs = (long long)4 * H * W * cs_dst;
            return FRLW_OK;
        }
    }
    Op op = {};
    op.type = OP_UPSAMPLE; op.src = src_buf; op.dst = dst_buf; op.C = C; op.H = H; op.W = W;
    op.cs_src = cs_src; op.co_src = co_src; op.cs_dst = cs_dst; op.co_dst = co_dst;
    op.lane = d->cur_lane;
    d->ops.push_back(op);
    return FRLW_OK;
}

int frlw_det_add_spp_pool(frlw_detector_t *d, int buf, int cs, int C, int H, int W)
{
    if (!d || cs < 4 * C) return FRLW_ERR_ARG;
    if (H * W > kSppMaxPix) return FRLW_ERR_UNSUPPORTED;
    Op op = {};
    op.type = OP_SPP; op.src = buf; op.dst = buf; op.C = C; op.H = H; op.W = W; op.cs_src = cs;
    op.lane = d->cur_lane;
    d->ops.push_back(op);
    return FRLW_OK;
}

int frlw_det_add_conv(frlw_detector_t *d, int src_buf, int src_cs, int src_co, int Cin, int H, int W,
                      const float *w_dev, const float *bias_dev, int Cout, int Npad, int k, int stride,
                      int dst_buf, int dst_cs, int dst_co, int64_t dst_bs, int res_buf, int res_cs, int res_co,
                      int act, int sig_from, int group_n)
{
    if (!d || !w_dev || (k != 1 && k != 3) || (stride != 1 && stride != 2) || (Cin & 3) || (Npad & 31) ||
        Npad < Cout || (src_cs & 3) || (src_co & 3) || group_n < 0 || (group_n & 127))
        return FRLW_ERR_ARG; // groups: whole 128-column tiles per group
    Op op = {};
    op.type = OP_CONV; op.src = src_buf; op.dst = dst_buf; op.res = res_buf;
    ConvArgs &c = op.conv;
    c.H = H; c.W = W; c.Cin = Cin; c.x_cs = src_cs; c.x_co = src_co; c.x_bs = (long long)H * W * src_cs;
    c.w = w_dev; c.bias = bias_dev; c.Cout = Cout; c.Npad = Npad; c.k = k; c.stride = stride; c.pad = (k - 1) / 2;
    c.Ho = (H + 2 * c.pad - k) / stride + 1; c.Wo = (W + 2 * c.pad - k) / stride + 1;
    c.y_cs = dst_cs; c.y_co = dst_co; c.y_bs = dst_bs > 0 ? dst_bs : (long long)c.Ho * c.Wo * dst_cs;
    c.r_cs = res_cs; c.r_co = res_co; c.r_bs = (long long)c.Ho * c.Wo * res_cs;
    c.act = act; c.sig_from = sig_from; c.K = k * k * Cin; c.group_n = group_n;
    c.prec = d->prec;
    op.lane = d->cur_lane;
    d->ops.push_back(op);
    return FRLW_OK;
}

int frlw_det_add_pred(frlw_detector_t *d, int src_buf, int src_cs, int src_co, int C, int hw, const float *w_dev,
                      const float *bias_dev, int F, int dst_buf, int first_anchor, int64_t dst_bs)
{
    if (!d || !w_dev || !bias_dev || hw < 1 || F < 6 || dst_bs < 1) return FRLW_ERR_ARG;
    if (C < 4 || (C & 3) || C > 256 || F > 16 || (src_cs & 3) || (src_co & 3)) return FRLW_ERR_UNSUPPORTED;
    Op op = {};
    op.type = OP_PRED; op.src = src_buf; op.dst = dst_buf;
    PredInferArgs &a = op.pred;
    a.cs = src_cs; a.co = src_co; a.C = C; a.w = w_dev; a.bias = bias_dev; a.F = F; a.hw = hw; a.off = first_anchor; a.out_bs = dst_bs;
    op.lane = d->cur_lane;
    d->ops.push_back(op);
    return FRLW_OK;
}

long long frlw_det_nms_workspace_floats(int A) { return A < 1 ? 0 : nms_ws_floats(A); }

int frlw_det_add_decode_nms(frlw_detector_t *d, int raw_buf, int A, int nc, int n_levels, const int *lvl_h,
                            const int *lvl_w, const int *lvl_stride, float obj_thr, float iou_thr, int decoded_buf,
                            int dets_buf, int counts_buf, int nms_buf)
{
    if (!d || n_levels < 1 || n_levels > 4 || nc < 1 || nc > 80 || A < 1 || nms_buf < 0) return FRLW_ERR_ARG;
    Op op = {};
    op.type = OP_DECODE; op.src = raw_buf; op.decoded_buf = decoded_buf; op.dets_buf = dets_buf; op.counts_buf = counts_buf;
    op.nms_buf = nms_buf;
    DecodeArgs &a = op.dec;
    a.A = A; a.nc = nc; a.n_levels = n_levels; a.obj_thr = obj_thr; a.iou_thr = iou_thr;
    for (int i = 0; i < n_levels; ++i) { a.lvl_h[i] = lvl_h[i]; a.lvl_w[i] = lvl_w[i]; a.lvl_stride[i] = lvl_stride[i]; }
    d->ops.push_back(op);
    return FRLW_OK;
}

// Runs ops [first, last) (last < 0: to the end) for a batch of B images.  bufs[i]: device pointers.
int frlw_det_run(const frlw_detector_t *d, int B, void *const *bufs, int n_bufs, int first, int last,
                 frlw_stream_t stream)
{
    (void)hipGetLastError(); // stale errors of other libraries in the process
    if (!d || B < 1 || !bufs) return FRLW_ERR_ARG;
    hipStream_t s0 = (hipStream_t)stream;
    const int n_ops = (int)d->ops.size();
    if (last < 0 || last > n_ops) last = n_ops;
    frlw_detector *dm = const_cast<frlw_detector *>(d);
    for (int oi = first; oi < last; ++oi) {
        const Op &op = d->ops[oi];
        if (op.type == OP_FORK || op.type == OP_JOIN) {
            if (!dm->have_side) { // created once, outside any graph capture
                for (int i = 0; i < kSideLanes; ++i) {
                    if (hipStreamCreateWithFlags(&dm->side[i], hipStreamNonBlocking) != hipSuccess) return FRLW_ERR_HIP;
                    if (hipEventCreateWithFlags(&dm->ev_join[i], hipEventDisableTiming) != hipSuccess) return FRLW_ERR_HIP;
                }
                if (hipEventCreateWithFlags(&dm->ev_fork, hipEventDisableTiming) != hipSuccess) return FRLW_ERR_HIP;
                dm->have_side = true;
            }
            if (op.type == OP_FORK) {
                if (hipEventRecord(dm->ev_fork, s0) != hipSuccess) return FRLW_ERR_HIP;
                for (int i = 0; i < kSideLanes; ++i)
                    if (hipStreamWaitEvent(dm->side[i], dm->ev_fork, 0) != hipSuccess) return FRLW_ERR_HIP;
            } else {
                for (int i = 0; i < kSideLanes; ++i) {
                    if (hipEventRecord(dm->ev_join[i], dm->side[i]) != hipSuccess) return FRLW_ERR_HIP;
                    if (hipStreamWaitEvent(s0, dm->ev_join[i], 0) != hipSuccess) return FRLW_ERR_HIP;
                }
            }
            continue;
        }
        hipStream_t s = (op.lane > 0 && dm->have_side) ? dm->side[op.lane - 1] : s0;
        auto buf = [&](int i) -> float * { return (i >= 0 && i < n_bufs) ? (float *)bufs[i] : nullptr; };
        switch (op.type) {
        case OP_FOCUS: {
            if (!launch_focus(buf(op.src), B, op.C, op.H, op.W, buf(op.dst), s)) return FRLW_ERR_UNSUPPORTED;
            break;
        }
        case OP_FOCUS_STEM: {
            FocusStemArgs a = op.fstem;
            a.x = buf(op.src); a.y = buf(op.dst);
            if (!a.x || !a.y) return FRLW_ERR_ARG;
            a.n_tiles = B * a.tiles_x * a.tiles_y;
            int na = 1; size_t wide_lds = 0;
            if (focus_stem_form(op.C, a.Cout, a.prec, &na, &wide_lds) == 2) {
                const int halves = a.npad / (32 * na), per_cu = wide_lds <= 80 * 1024 ? 2 : 1;
                const int wgs = a.n_tiles < 256 * per_cu / halves ? a.n_tiles : 256 * per_cu / halves;
                const FocusStemWideFn kern = focus_stem_wide_kernel(op.C, a.prec, na);
                if (!kern) return FRLW_ERR_UNSUPPORTED; // (frlw_det_add_focus_stem accepts only what has a kernel)
                // (asked and checked once in frlw_det_add_focus_stem; the attribute is per device, so it is set again here)
                (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wide_lds);
                hipLaunchKernelGGL(kern, dim3(wgs * halves), dim3(256), wide_lds, s, a);
                break;
            }
            const int cf = 4 * op.C;
            const int wfl = a.prec == 1 ? (op.C == 10 ? focus_stem_w_floats<10, 1>() : focus_stem_w_floats<16, 1>()) : 9 * cf * 32;
            const size_t lds = ((size_t)wfl + (size_t)180 * (cf + 4)) * sizeof(float);
            const int per_cu = lds <= 80 * 1024 ? 2 : 1;
            const int grid = a.n_tiles < 256 * per_cu ? a.n_tiles : 256 * per_cu;
            auto go = [&](auto kern) {
                (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, a);
            };
            if (op.C == 10) { if (a.prec == 1) go(k_focus_stem<10, 1>); else go(k_focus_stem<10, 0>); }
            else { if (a.prec == 1) go(k_focus_stem<16, 1>); else go(k_focus_stem<16, 0>); }
            break;
        }
        case OP_BFM: {
            const int grid = grid_1d((long long)B * op.H * op.W);
            if (op.C == 4) hipLaunchKernelGGL(k_bfm_stem<2>, dim3(grid), dim3(256), 0, s, buf(op.src), B, op.H, op.W, op.bfm_w, buf(op.dst));
            else if (op.C == 8) hipLaunchKernelGGL(k_bfm_stem<4>, dim3(grid), dim3(256), 0, s, buf(op.src), B, op.H, op.W, op.bfm_w, buf(op.dst));
            else hipLaunchKernelGGL(k_bfm_stem<8>, dim3(grid), dim3(256), 0, s, buf(op.src), B, op.H, op.W, op.bfm_w, buf(op.dst));
            break;
        }
        case OP_UPSAMPLE: {
            const long long total = (long long)B * 4 * op.H * op.W * op.C;
            hipLaunchKernelGGL(k_upsample2x, dim3(grid_1d(total)), dim3(256), 0, s, buf(op.src), B, op.H, op.W, op.C,
                               op.cs_src, op.co_src, buf(op.dst), op.cs_dst, op.co_dst);
            break;
        }
        case OP_SPP: {
            const size_t lds = (size_t)2 * op.H * op.W * (kSppCh + 1) * sizeof(float);
            if (lds > 64 * 1024)
                (void)hipFuncSetAttribute((const void *)k_spp_pool, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k_spp_pool, dim3((op.C + kSppCh - 1) / kSppCh, B), dim3(256), lds, s, buf(op.src), op.H, op.W, op.C, op.cs_src);
            break;
        }
        case OP_CONV: {
            ConvArgs c = op.conv;
            c.x = buf(op.src); c.y = buf(op.dst); c.res = buf(op.res);
            c.y2 = op.ups_buf > 0 ? buf(op.ups_buf) : nullptr;
            if (!c.x || !c.y || (op.ups_buf > 0 && !c.y2)) return FRLW_ERR_ARG;
            c.M = B * c.Ho * c.Wo;
            {
                // a lane's scratch region: split-K partial sums, and in its last 1024 words the tiles' arrival counters of the
                // in-kernel reduction (zero when the caller hands the buffer over, reset by the kernel: frlw_det_set_scratch)
                float *sc = d->scratch_buf >= 0 ? buf(d->scratch_buf) + (long long)op.lane * d->scratch_floats : nullptr;
                const long long cap = d->scratch_buf >= 0 ? d->scratch_floats - 1024 : 0;
                static const long long sk_knob = dev_knob("FRLW_CONV_SK_INKERNEL", 1ll);
                int *counters = (sc && cap > 0 && sk_knob) ? (int *)(sc + cap) : nullptr;
                if (!launch_conv(c, sc, cap > 0 ? cap : 0, s, counters)) return FRLW_ERR_UNSUPPORTED;
            }
            break;
        }
        case OP_PRED: { // this op and the OP_PRED ops that directly follow it on the same lane (the head levels): one launch
            PredInferMulti pm = {};
            const int i = oi;
            int j = i;
            for (; j < last && j - i < 4 && d->ops[j].type == OP_PRED && d->ops[j].lane == op.lane && d->ops[j].pred.F == op.pred.F; ++j) {
                PredInferArgs a = d->ops[j].pred;
                a.x = buf(d->ops[j].src); a.out = buf(d->ops[j].dst);
                if (!a.x || !a.out) return FRLW_ERR_ARG;
                a.M = (long long)B * a.hw;
                long long wg = (a.M + 31) / 32; // >= 8 rows per wavefront
                if (wg > 2048) wg = 2048;
                pm.lv[j - i] = a;
                pm.first[j - i + 1] = pm.first[j - i] + (int)wg;
            }
            pm.n = j - i;
            if (op.pred.F <= 8) hipLaunchKernelGGL(k_pred_infer<1>, dim3(pm.first[pm.n]), dim3(256), 0, s, pm);
            else hipLaunchKernelGGL(k_pred_infer<2>, dim3(pm.first[pm.n]), dim3(256), 0, s, pm);
            oi = j - 1; // (the loop's ++oi steps behind the last merged op)
            break;
        }
        case OP_DECODE: {
            DecodeArgs a = op.dec;
            a.raw = buf(op.src); a.decoded = buf(op.decoded_buf); a.dets = buf(op.dets_buf);
            a.counts = (int *)buf(op.counts_buf);
            a.ws = buf(op.nms_buf);
            if (!a.raw || !a.dets || !a.counts || !a.ws) return FRLW_ERR_ARG;
            int cap = 1024; // LDS sized for the anchors of this network, up to NMS_MAX candidates
            while (cap < a.A && cap < NMS_MAX) cap <<= 1;
            const size_t lds = nms_lds_bytes(cap);
            if (lds > 64 * 1024)
                (void)hipFuncSetAttribute((const void *)k_decode_sort, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k_decode_sort, dim3(B), dim3(1024), lds, s, a, cap);
            const int words = nms_a64(a.A) / 64; // candidates never exceed min(A, NMS_MAX)
            hipLaunchKernelGGL(k_nms_matrix, dim3((words + 3) / 4, words, B), dim3(256), 0, s, a);
            hipLaunchKernelGGL(k_nms_sweep, dim3(B), dim3(kSweepThreads), 0, s, a);
            hipLaunchKernelGGL(k_nms_emit, dim3(words * 64 / 256 + 1, B), dim3(256), 0, s, a);
            break;
        }
        default: return FRLW_ERR_ARG;
        }
    }
    if (hipGetLastError() != hipSuccess) return FRLW_ERR_HIP;
    return FRLW_OK;
}

} // extern "C"
