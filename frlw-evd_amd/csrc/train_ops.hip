// train_ops.hip -- training-mode operators of BaseConv = Conv2d(bias=False) + BatchNorm2d (batch statistics) + SiLU
// (core/yolox/models/network_blocks.py:33-65) for the train step of core/exp.py:283-315, on NHWC float32 tensors
// (torch channels_last storage, so the autograd wrapper in frlw-evd_amd/yolox/train_ops.py passes pointers as is):
//
//   frlw_conv_weight_layouts   torch (Cout, Cin, k, k) -> the two GEMM operands: forward (k*k*Cin, Npad(Cout)) and
//                              data-gradient (k*k*Cout, Npad(Cin)) with the taps flipped
//   frlw_conv2d_fwd            z = conv(x, w)                    k_conv_mfma (conv_mfma.h), fp32 MFMA
//   frlw_conv2d_dgrad          dx = conv^T(dz, w)                the same kernel on the flipped operand; stride 2 through
//                              the transposed gather (tstride = 2)
//   frlw_conv2d_wgrad          dw = x^T * dz                     k_wgrad_mfma: M = k*k*Cin, N = Cout, contraction over
//                              the B*Ho*Wo output pixels split over blockIdx.z, deterministic two-stage reduction
//                              straight into torch's (Cout, Cin, k, k) layout
//   frlw_bn_stats              per-channel mean / biased variance (float64 sums, two-stage, deterministic)
//   frlw_bn_silu_fwd           y = silu(gamma * (z - mean) * invstd + beta)
//   frlw_bn_silu_bwd           dz, dgamma, dbeta from dy and z (u recomputed, nothing but z saved)
//
// MI355X: every contraction runs on the matrix cores, like the inference forward, in the arithmetic the caller names
// (`precision`: 0 = v_mfma_f32_32x32x2_f32, 1 = float32 products from three bf16 MFMAs on split operands: conv_mfma.h);
// the elementwise passes are HBM-bound float4 streams over the (M, C) view of the tensor.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <type_traits>

#include "frlw_evd.h"

namespace {

#include "conv_mfma.h"

#define TRY_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
        FRLW_DEV_LOG("frlw_evd train_ops: %s -> %s\n", #expr, hipGetErrorString(e_)); \
        return FRLW_ERR_HIP; } } while (0)

#include "train_weights.h"
#include "train_wgrad.h"
#include "train_bn.h"

// ---- convolutions -------------------------------------------------------------------------------
inline int conv_out_dim(int H, int k, int stride) { return (H + 2 * ((k - 1) / 2) - k) / stride + 1; }

// dense NHWC x (B, H, W, Cin) times the operand w (k*k*Cin rows, npad32(Cout) columns) -> dense NHWC y (B, Ho, Wo, Cout),
// padding (k - 1) / 2; no bias, activation, residual, statistics or transposed gather: the callers add what they need
inline ConvArgs conv_args_dense(const float *x, int B, int H, int W, int Cin, const float *w, int Cout, int k, int stride, int Ho, int Wo,
                                float *y, int precision)
{
    ConvArgs c = {};
    c.x = x; c.H = H; c.W = W; c.Cin = Cin; c.x_cs = Cin; c.x_bs = (long long)H * W * Cin;
    c.w = w; c.Cout = Cout; c.Npad = npad32(Cout); c.k = k; c.stride = stride; c.pad = (k - 1) / 2;
    c.y = y; c.Ho = Ho; c.Wo = Wo; c.y_cs = Cout; c.y_bs = (long long)Ho * Wo * Cout;
    c.act = ACT_NONE;
    c.M = B * Ho * Wo; c.K = k * k * Cin;
    c.prec = precision;
    return c;
}

// One convolution of conv_args_dense plus `res` (rows of res_rs floats, 0: dense; may be NULL) added in the epilogue.  c.stats
// asks for the statistics of the output; afterwards c.stats_rows > 0 says the launch produced them, c.splits > 1 that the in-kernel
// split-K epilogue did (launch_conv).
int conv_common(ConvArgs &c, int B, const float *res, long long res_rs, float *scratch, int64_t scratch_floats, hipStream_t s, int *sk_counters)
{
    if (c.prec != 0 && c.prec != 1) return FRLW_ERR_ARG;
    (void)hipGetLastError(); // other libraries in the process (torch's BLAS look-ups) leave stale errors behind
    if (!c.x || !c.w || !c.y || B < 1 || c.H < 1 || c.W < 1 || c.Cin < 4 || (c.Cin & 3) || c.Cout < 1 || c.k < 1) return FRLW_ERR_ARG;
    c.res = res; c.r_cs = (int)(res_rs > 0 ? res_rs : c.Cout); c.r_bs = (long long)c.Ho * c.Wo * c.r_cs;
    if (!launch_conv(c, scratch, scratch ? scratch_floats : 0, s, sk_counters)) return FRLW_ERR_UNSUPPORTED;
    TRY_HIP(hipGetLastError());
    return FRLW_OK;
}

// dx_add (may be NULL): dx = data gradient + dx_add in the epilogue (the gradient a second consumer of x has produced already;
// rows of dx_add_rs floats).  Stride-1 layers only: the parity classes of a stride-2 layer write interleaved rows.
int conv2d_dgrad(const float *dz, int B, int Ho, int Wo, int Cout, const float *w_dgrad, int Cin, int k, int stride, int H, int W,
                 float *dx, float *scratch, int64_t scratch_floats, int precision, hipStream_t s, int *sk_counters, const float *dx_add,
                 int64_t dx_add_rs)
{
    if (precision != 0 && precision != 1) return FRLW_ERR_ARG;
    if (dx_add && (stride != 1 || (dx_add_rs > 0 && (dx_add_rs < Cin || (dx_add_rs & 3))) || ((uintptr_t)dx_add & 15))) return FRLW_ERR_UNSUPPORTED;
    // dx[iy][ix][ci] = sum dz[(iy + pad - ky) / s][(ix + pad - kx) / s][co] * w[co][ci][ky][kx]: a stride-1 convolution of
    // dz (transposed gather for s = 2) with the flipped operand and padding k - 1 - pad = pad (odd k)
    if (stride != 1 && stride != 2) return FRLW_ERR_UNSUPPORTED;
    if (!(k & 1)) return FRLW_ERR_UNSUPPORTED;
    if (!frlw_conv2d_dgrad_parity(k, stride, H, W)) {
        ConvArgs c = conv_args_dense(dz, B, Ho, Wo, Cout, w_dgrad, Cin, k, 1, H, W, dx, precision);
        c.tstride = stride == 2 ? 2 : 0;
        return conv_common(c, B, dx_add, dx_add_rs, scratch, scratch_floats, s, sk_counters);
    }
    // four stride-1 convolutions of dz, one per output parity class, with 1 / 2 / 2 / 4 of the nine taps (no
    // multiplications by the zeros of the up-sampled gradient); class (py, px) writes dx[2 o' + (py, px)]
    if (Ho * 2 != H || Wo * 2 != W) return FRLW_ERR_ARG;
    if (!dz || !w_dgrad || !dx || B < 1 || Cout < 4 || (Cout & 3) || Cin < 1) return FRLW_ERR_ARG;
    if (!precision_ok(precision, Cout, 1)) return FRLW_ERR_UNSUPPORTED;
    (void)hipGetLastError();
    static const int row0[4] = {0, 1, 3, 5};
    for (int cls = 0; cls < 4; ++cls) {
        const int py = cls >> 1, px = cls & 1, kh = py ? 2 : 1, kwc = px ? 2 : 1;
        ConvArgs c = conv_args_dense(dz, B, Ho, Wo, Cout, w_dgrad + (long long)row0[cls] * Cout * npad32(Cin), Cin, kh, 1, Ho, Wo, dx, precision);
        c.kw = kwc; c.pad = 0; c.K = kh * kwc * Cout;
        c.y_cs = 2 * Cin; c.y_rp = 2 * W * Cin; c.y_co = (py * W + px) * Cin; c.y_bs = (long long)H * W * Cin;
        if (!launch_conv(c, scratch, scratch ? scratch_floats : 0, s, sk_counters)) return FRLW_ERR_UNSUPPORTED;
    }
    TRY_HIP(hipGetLastError());
    return FRLW_OK;
}

// ---- scratch of the block entries -----------------------------------------------------------------
constexpr int64_t kSplitKFloats = 8ll * 1024 * 1024; // split-K partials of forward / data gradient

// The six pieces of frlw_baseconv_train_scratch_bytes behind `base`, each on a multiple of 256 bytes (base NULL: the pointers are
// the offsets).  Operands are sized for precision 1: either precision fits.
struct TrainScratch { float *w_fwd, *w_dg; double *red; float *sums, *wgrad, *splitk; int64_t wgrad_floats, splitk_floats, total; };
inline TrainScratch train_scratch(void *base, int B, int Ho, int Wo, int Cin, int Cout, int k)
{
    uintptr_t p = (uintptr_t)base;
    int64_t sum = 0;
    auto take = [&](int64_t bytes) { void *r = (void *)p; p += (bytes + 255) / 256 * 256; sum += bytes; return r; };
    TrainScratch t;
    t.w_fwd = (float *)take(sizeof(float) * frlw_conv_operand_floats(k * k * Cin, Cout, 1)); // forward operand
    t.w_dg = (float *)take(sizeof(float) * frlw_conv_operand_floats(k * k * Cout, Cin, 1));  // data-gradient operand
    t.red = (double *)take(sizeof(double) * frlw_bn_scratch_doubles((int64_t)B * Ho * Wo, Cout)); // reduction partials
    t.sums = (float *)take(sizeof(float) * 2 * Cout);
    t.wgrad_floats = wgrad_scratch_floats(B, Ho, Wo, Cin, Cout, k);
    t.wgrad = (float *)take(sizeof(float) * t.wgrad_floats);
    t.splitk_floats = kSplitKFloats;
    t.splitk = (float *)take(sizeof(float) * t.splitk_floats);
    // the unrounded sizes plus 256 bytes per piece, not the end of the last piece (which is never larger): callers cache their
    // scratch by this number and it has always been this one
    t.total = sum + 6 * 256;
    return t;
}

} // namespace

extern "C" {

int frlw_conv_path_counts(uint64_t *counts, int n)
{
    if (!counts || n < 1) return FRLW_ERR_ARG;
    for (int i = 0; i < n && i < FRLW_CONV_PATH_COUNT; ++i) counts[i] = (uint64_t)g_conv_path_counts[i].load(std::memory_order_relaxed);
    return FRLW_CONV_PATH_COUNT;
}

int frlw_bn_path_counts(uint64_t *counts, int n)
{
    if (!counts || n < 1) return FRLW_ERR_ARG;
    for (int i = 0; i < n && i < FRLW_BN_PATH_COUNT; ++i) counts[i] = (uint64_t)g_bn_path_counts[i].load(std::memory_order_relaxed);
    return FRLW_BN_PATH_COUNT;
}

int frlw_conv2d_dgrad_parity(int k, int stride, int H, int W)
{
    return (stride == 2 && k == 3 && !(H & 1) && !(W & 1)) ? 1 : 0;
}

int64_t frlw_conv_operand_floats(int K, int N, int precision)
{
    if (K < 1 || N < 1) return 0;
    return operand_rows(K, precision) * (int64_t)npad32(N);
}

int frlw_conv_weight_layouts(const float *w, int Cout, int Cin, int k, int dgrad_parity, float *w_fwd, float *w_dgrad,
                             int precision, frlw_stream_t stream)
{
    return launch_weight_layouts(w, Block2{}, Cout, Cin, k, dgrad_parity, w_fwd, w_dgrad, precision, stream);
}

int frlw_conv_weight_layouts_batch(const frlw_weight_layout_item_t *items, int n, int64_t total, frlw_stream_t stream)
{
    (void)hipGetLastError();
    if (!items || n < 1 || total < 1) return FRLW_ERR_ARG;
    const long long tiles = (total + 2047) / 2048;
    hipLaunchKernelGGL(k_weight_layouts_batch, dim3((unsigned)(tiles < 8192 ? tiles : 8192)), dim3(256), 0, (hipStream_t)stream, items, n, (long long)total);
    TRY_HIP(hipGetLastError());
    return FRLW_OK;
}

int frlw_conv2d_fwd(const float *x, int B, int H, int W, int Cin, const float *w_fwd, int Cout, int k, int stride, float *z,
                    float *scratch, int64_t scratch_floats, int precision, frlw_stream_t stream)
{
    if (stride != 1 && stride != 2) return FRLW_ERR_UNSUPPORTED;
    ConvArgs c = conv_args_dense(x, B, H, W, Cin, w_fwd, Cout, k, stride, conv_out_dim(H, k, stride), conv_out_dim(W, k, stride), z, precision);
    return conv_common(c, B, nullptr, 0, scratch, scratch_floats, (hipStream_t)stream, nullptr);
}

int frlw_conv2d_dgrad(const float *dz, int B, int Ho, int Wo, int Cout, const float *w_dgrad, int Cin, int k, int stride,
                      int H, int W, float *dx, float *scratch, int64_t scratch_floats, int precision, frlw_stream_t stream)
{
    return conv2d_dgrad(dz, B, Ho, Wo, Cout, w_dgrad, Cin, k, stride, H, W, dx, scratch, scratch_floats, precision, (hipStream_t)stream, nullptr, nullptr, 0);
}

int64_t frlw_conv2d_wgrad_scratch_floats(int B, int Ho, int Wo, int Cin, int Cout, int k)
{
    return wgrad_scratch_floats(B, Ho, Wo, Cin, Cout, k);
}

int frlw_conv2d_wgrad(const float *x, int B, int H, int W, int Cin, const float *dz, int Ho, int Wo, int Cout, int k,
                      int stride, float *dw, float *scratch, int64_t scratch_floats, int precision, frlw_stream_t stream)
{
    (void)hipGetLastError(); // other libraries in the process (torch's BLAS look-ups) leave stale errors behind
    if (!x || !dz || !dw || !scratch || B < 1 || (Cin & 3) || (Cout & 3) || Cin < 4 || Cout < 4) return FRLW_ERR_ARG;
    if (precision != 0 && precision != 1) return FRLW_ERR_ARG;
    WgradArgs a = {};
    a.prec = precision;
    a.x = x; a.H = H; a.W = W; a.Cin = Cin; a.x_bs = (long long)H * W * Cin; a.x_cs = Cin;
    a.dz = dz; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout; a.dz_bs = (long long)Ho * Wo * Cout; a.dz_cs = Cout;
    a.k = k; a.stride = stride; a.pad = (k - 1) / 2;
    a.R = k * k * Cin; a.M = B * Ho * Wo;
    const long long per = (long long)a.R * Cout;
    // the splits the query sized its answer for, and the most the given scratch holds
    const long long want = wgrad_splits_in(wgrad_scratch_floats(B, Ho, Wo, Cin, Cout, k) / per), fit = wgrad_splits_in(scratch_floats / per);
    if (fit < 1) return FRLW_ERR_WORKSPACE;
    if (fit < want) conv_count(FRLW_CONV_PATH_WGRAD_SCRATCH_LIMITED);
    a.splits = (int)(want < fit ? want : fit);
    a.partial = scratch;
    hipStream_t s = (hipStream_t)stream;
    if (!launch_wgrad_tiles(a, s)) return FRLW_ERR_UNSUPPORTED; // a tensor beyond 3.7 GB: split the batch
    const float *final_src = scratch;
    int final_n = a.splits;
    if (a.splits > 64) { // group sums go behind the partial tiles (the scratch query reserves the room)
        const int groups = (a.splits + kWgradGroup - 1) / kWgradGroup;
        conv_count(FRLW_CONV_PATH_WGRAD_GROUP_SUM);
        float *gs = scratch + (long long)a.splits * per;
        hipLaunchKernelGGL(k_wgrad_group_sum, dim3(conv_grid_1d(per), groups), dim3(256), 0, s, scratch, a.splits, per, gs);
        final_src = gs;
        final_n = groups;
    }
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((a.R + 31) / 32, (Cout + 31) / 32), dim3(256), 0, s, final_src, final_n, a.R, Cout, Cin, k, dw);
    TRY_HIP(hipGetLastError());
    return FRLW_OK;
}

int64_t frlw_bn_scratch_doubles(int64_t M, int C)
{
    const int rows = bn_rows_per_wg(M);
    const int64_t pass = ((M + rows - 1) / rows) * (int64_t)C * 2;
    const int64_t fused = ((M + 63) / 64) * (int64_t)C * 2; // the convolution epilogue's slabs of >= 64 rows (conv_mfma.h: ConvArgs::stats)
    return pass > fused ? pass : fused;
}

int frlw_bn_stats(const float *z, int64_t M, int C, float eps, float *mean, float *var, float *invstd, double *scratch,
                  frlw_stream_t stream)
{
    return launch_bn_stats(z, M, C, eps, mean, var, invstd, scratch, nullptr, nullptr, 0.0f, nullptr, 0, Block2{}, stream);
}

int frlw_bn_silu_fwd(const float *z, int64_t M, int C, const float *gamma, const float *beta, const float *mean,
                     const float *invstd, float *y, frlw_stream_t stream)
{
    return launch_bn_silu_fwd(z, M, C, gamma, beta, mean, invstd, y, 0, nullptr, 0, Block2{}, stream);
}

int frlw_bn_silu_bwd(const float *dy, int64_t dy_row_stride, const float *z, int64_t M, int C, const float *gamma, const float *beta,
                     const float *mean, const float *invstd, float *dz, float *dgamma, float *dbeta, double *scratch,
                     float *sums, frlw_stream_t stream)
{
    return launch_bn_silu_bwd(dy, dy_row_stride, z, M, C, gamma, beta, mean, invstd, dz, dgamma, dbeta, scratch, sums, Block2{}, stream);
}

/* ---- one call per BaseConv and direction (the per-operator entry points above stay for tests / other callers) ---- */
int64_t frlw_baseconv_weight_cache_floats(int Cin, int Cout, int k, int precision)
{
    return frlw_conv_operand_floats(k * k * Cin, Cout, precision) + frlw_conv_operand_floats(k * k * Cout, Cin, precision);
}

int64_t frlw_baseconv_train_scratch_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride)
{
    return train_scratch(nullptr, B, conv_out_dim(H, k, stride), conv_out_dim(W, k, stride), Cin, Cout, k).total;
}

/* y = silu(bn(conv(x, w))) with batch statistics; z (the convolution output), mean, var (biased), invstd are outputs
 * the backward needs.  scratch: frlw_baseconv_train_scratch_bytes bytes, contents not needed afterwards. */
int frlw_baseconv_train_fwd(const float *x, const float *w, const float *gamma, const float *beta, float eps, int B, int H,
                            int W, int Cin, int Cout, int k, int stride, float *z, float *y, float *mean, float *var,
                            float *invstd, float *running_mean, float *running_var, float momentum,
                            int64_t *num_batches_tracked, float *w_cache, void *scratch, int64_t scratch_bytes,
                            int *splitk_counters, const frlw_baseconv_fuse_t *fuse, int precision, frlw_stream_t stream)
{
    if (!x || (!w && !w_cache) || !gamma || !beta || !z || !y || !mean || !var || !invstd || !scratch) return FRLW_ERR_ARG;
    if (fuse && fuse->struct_size != (int32_t)sizeof(frlw_baseconv_fuse_t)) return FRLW_ERR_ARG;
    Block2 b2; // split > 0: two blocks stacked along the output channels (frlw_evd.h)
    int rc;
    if ((rc = block2_of(fuse, Cout, false, w != nullptr, running_mean != nullptr, b2)) != FRLW_OK) return rc;
    if (stride != 1 && stride != 2) return FRLW_ERR_UNSUPPORTED;
    const int Ho = conv_out_dim(H, k, stride), Wo = conv_out_dim(W, k, stride);
    const TrainScratch t = train_scratch(scratch, B, Ho, Wo, Cin, Cout, k);
    if (scratch_bytes < t.total) return FRLW_ERR_WORKSPACE;
    // w_cache: both operands in ONE launch, kept by the caller (the backward of this step finds its operand ready); without w the
    // caller has laid them out already (frlw_conv_weight_layouts_batch)
    if (w && w_cache) rc = launch_weight_layouts(w, b2, Cout, Cin, k, frlw_conv2d_dgrad_parity(k, stride, H, W), w_cache,
                                                 w_cache + frlw_conv_operand_floats(k * k * Cin, Cout, precision), precision, stream);
    else if (w) rc = launch_weight_layouts(w, b2, Cout, Cin, k, 0, t.w_fwd, nullptr, precision, stream);
    if (rc != FRLW_OK) return rc;
    ConvArgs c = conv_args_dense(x, B, H, W, Cin, w_cache ? w_cache : t.w_fwd, Cout, k, stride, Ho, Wo, z, precision);
    c.stats = t.red; // granted: the convolution's epilogue leaves the column sums of its output slabs there
    if ((rc = conv_common(c, B, nullptr, 0, t.splitk, t.splitk_floats, (hipStream_t)stream, splitk_counters)) != FRLW_OK) return rc;
    if (c.stats_rows > 0) bn_count(c.splits > 1 ? FRLW_BN_PATH_STATS_SPLIT_INKERNEL : FRLW_BN_PATH_STATS_EPILOGUE);
    if ((rc = launch_bn_stats(z, (int64_t)B * Ho * Wo, Cout, eps, mean, var, invstd, t.red, running_mean, running_mean ? running_var : nullptr,
                              momentum, (long long *)num_batches_tracked, c.stats_rows, b2, stream)) != FRLW_OK) return rc;
    return launch_bn_silu_fwd(z, (int64_t)B * Ho * Wo, Cout, gamma, beta, mean, invstd, y, fuse ? fuse->y_row_stride : 0,
                              fuse ? fuse->residual : nullptr, fuse ? fuse->residual_row_stride : 0, b2, stream);
}

/* Gradients of the block: dx (NULL: not needed), dw (Cout, Cin, k, k), dgamma, dbeta.  dz: (B, Ho, Wo, Cout) work buffer. */
int frlw_baseconv_train_bwd(const float *dy, int64_t dy_row_stride, const float *x, const float *z, const float *w, const float *gamma,
                            const float *beta, const float *mean, const float *invstd, int B, int H, int W, int Cin,
                            int Cout, int k, int stride, float *dz, float *dx, float *dw, float *dgamma, float *dbeta,
                            const float *w_cache, void *scratch, int64_t scratch_bytes, int *splitk_counters,
                            const frlw_baseconv_fuse_t *fuse, int precision, frlw_stream_t stream)
{
    if (!dy || !x || !z || !w || !gamma || !beta || !mean || !invstd || !dz || !dw || !dgamma || !dbeta || !scratch)
        return FRLW_ERR_ARG;
    if (fuse && fuse->struct_size != (int32_t)sizeof(frlw_baseconv_fuse_t)) return FRLW_ERR_ARG;
    if (fuse && fuse->dx_add && (!dx || stride != 1)) return FRLW_ERR_UNSUPPORTED;
    Block2 b2;
    int rc;
    if ((rc = block2_of(fuse, Cout, true, !w_cache, false, b2)) != FRLW_OK) return rc;
    const int Ho = conv_out_dim(H, k, stride), Wo = conv_out_dim(W, k, stride);
    const TrainScratch t = train_scratch(scratch, B, Ho, Wo, Cin, Cout, k);
    if (scratch_bytes < t.total) return FRLW_ERR_WORKSPACE;
    if ((rc = launch_bn_silu_bwd(dy, dy_row_stride, z, (int64_t)B * Ho * Wo, Cout, gamma, beta, mean, invstd, dz, dgamma, dbeta, t.red, t.sums, b2,
                                 stream)) != FRLW_OK) return rc;
    if (dx) { // w_cache: the data-gradient operand was laid out by the forward of this step
        if (!w_cache && (rc = launch_weight_layouts(w, b2, Cout, Cin, k, frlw_conv2d_dgrad_parity(k, stride, H, W), nullptr, t.w_dg, precision, stream)) != FRLW_OK) return rc;
        if ((rc = conv2d_dgrad(dz, B, Ho, Wo, Cout, w_cache ? w_cache + frlw_conv_operand_floats(k * k * Cin, Cout, precision) : t.w_dg, Cin, k, stride, H, W,
                               dx, t.splitk, t.splitk_floats, precision, (hipStream_t)stream, splitk_counters, fuse ? fuse->dx_add : nullptr,
                               fuse ? fuse->dx_add_row_stride : 0)) != FRLW_OK) return rc;
    }
    return frlw_conv2d_wgrad(x, B, H, W, Cin, dz, Ho, Wo, Cout, k, stride, dw, t.wgrad, t.wgrad_floats, precision, stream);
}

} // extern "C"

