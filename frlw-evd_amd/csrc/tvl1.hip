// tvl1.hip -- Dual TV-L1 optical flow (Zach, Pock, Bischof 2007) for a batch of uint8 image pairs (frlw_tvl1_flow_batch), float32
// throughout, the algorithm as DESIGN.md's motion section states it and tests/tvl1_restated.py restates it in numpy.
//
// Planes of one pair (its slot of every region of the workspace is sized for the full frame, a level uses the front of it):
//   pyr0, pyr1   every level of both images, float
//   gxy          float2 (I1x, I1y) of the current level
//   wd           float4 (I1wx, I1wy, grad, rho_c) of the current warp
//   u[2]         float2 (u1, u2), two buffers: every kernel that needs a neighbour's OLD value reads one and writes the other
//   p[2]         float4 (p11, p12, p21, p22), likewise
//
// Launches, pairs in lockstep (grid.y = pair):
//   kv_u8 / kv_resize   the pyramids
//   per level:  kv_grad;  kv_upsample (flow of the coarser level, times 1 / scale_step) except on the coarsest
//   per warp:   kv_warp   three bicubic samples, grad, rho_c; moves u and p of the pair into buffer 0
//   per outer:  kv_median 5 x 5, u[b] -> u[b ^ 1]
//   per inner:  kv_iter   ONE launch: u_new on the tile and on its right / lower ring into LDS (p read old), u_new and p_new
//                         written for the tile's own pixels into the other buffers, the tile's part of the error
//   kv_out      the finest level's (u1, u2) -> flows (n, H, W, 2)
//
// Convergence: launch j of a warp leaves one partial error per tile in partial[j & 1]; every workgroup of launch j + 1 (and of the
// median launch that follows an outer iteration) adds the pair's partials in the same fixed order, so all of them reach the same
// verdict without waiting on each other, and workgroup 0 records it in the pair's word of this warp: 1 | buffer of u << 1 | buffer
// of p << 2, the buffers that hold the pair's result.  Later launches of the warp return at its sight; the next warp (or the
// upsample, or kv_out) reads the result from there, pairs that ran to the end from the buffers the host counted to.  The host
// reads the words of a warp once per outer iteration and stops enqueuing when all are set.  No atomics, no float sums whose
// order depends on timing or on the pair's place in the batch: bit-identical from run to run and alone or batched.

#include "frlw_common.h"

#include <math.h>

using namespace frlw;

namespace {

constexpr int kVT = 256;                 // threads of every kernel here
constexpr int kTW = 32, kTH = 16;        // kv_iter: own pixels of a workgroup (two per thread)
constexpr int kRW = kTW + 1, kRH = kTH + 1;
constexpr int kMW = 32, kMH = 8;         // kv_median: one pixel per thread, halo of 2
constexpr int kMaxLevels = FRLW_TVL1_MAX_LEVELS;
constexpr int kMaxWarps = 64;
constexpr float kA = -0.75f;             // Keys' cubic kernel

struct Params { int nscales, warps, inner, outer, median; float tau, lambda, theta, epsilon, scale_step; };

struct Level { int h, w; long long off; }; // off: floats in front of this level in a pair's pyramid slot

struct Layout {
    int n_levels, tiles0;
    long long cells0, pyr_cells;
    size_t done, partial, pyr0, pyr1, gxy, wd, u[2], p[2], total;
    Level lv[kMaxLevels];
};

int plan_levels(int H, int W, int nscales, double scale_step, Level *lv)
{
    int n = 0, h = H, w = W;
    long long off = 0;
    for (int s = 0; s < nscales && s < kMaxLevels; ++s) {
        if (h < 16 || w < 16) break;
        lv[n].h = h; lv[n].w = w; lv[n].off = off;
        off += (long long)h * w;
        ++n;
        h = (int)nearbyint((double)h * scale_step); // ties to even, as Python's round()
        w = (int)nearbyint((double)w * scale_step);
    }
    return n;
}

inline int tiles_of(int h, int w) { return ((w + kTW - 1) / kTW) * ((h + kTH - 1) / kTH); }
inline size_t up256(size_t v) { return (v + 255u) & ~(size_t)255u; }

bool layout_of(int n, int H, int W, const Params &P, Layout &L)
{
    if (n < 1 || n > FRLW_MAX_SEQUENCES || H < 16 || W < 16 || H > 16384 || W > 16384) return false;
    L.n_levels = plan_levels(H, W, P.nscales, (double)P.scale_step, L.lv);
    if (L.n_levels < 1) return false;
    L.cells0 = (long long)H * W;
    L.pyr_cells = L.lv[L.n_levels - 1].off + (long long)L.lv[L.n_levels - 1].h * L.lv[L.n_levels - 1].w;
    L.tiles0 = tiles_of(H, W);
    size_t at = 0;
    const size_t N = (size_t)n, c0 = (size_t)L.cells0;
    L.done = at;    at = up256(at + (size_t)kMaxLevels * kMaxWarps * FRLW_MAX_SEQUENCES * sizeof(int));
    L.partial = at; at = up256(at + N * 2 * (size_t)L.tiles0 * sizeof(float));
    L.pyr0 = at;    at = up256(at + N * (size_t)L.pyr_cells * sizeof(float));
    L.pyr1 = at;    at = up256(at + N * (size_t)L.pyr_cells * sizeof(float));
    L.gxy = at;     at = up256(at + N * c0 * sizeof(float2));
    L.wd = at;      at = up256(at + N * c0 * sizeof(float4));
    for (int b = 0; b < 2; ++b) { L.u[b] = at; at = up256(at + N * c0 * sizeof(float2)); }
    for (int b = 0; b < 2; ++b) { L.p[b] = at; at = up256(at + N * c0 * sizeof(float4)); }
    L.total = at;
    return true;
}

// ---- pyramid -------------------------------------------------------------------------------------
// grid (cells, n): both images of pair blockIdx.y, uint8 -> float
__global__ __launch_bounds__(kVT) void kv_u8(const uint8_t *pairs, long long cells, float *pyr0, float *pyr1, long long pyr_cells)
{
    const long long pair = blockIdx.y;
    const uint8_t *a = pairs + pair * 2 * cells, *b = a + cells;
    float *o0 = pyr0 + pair * pyr_cells, *o1 = pyr1 + pair * pyr_cells;
    const long long stride = (long long)gridDim.x * kVT;
    for (long long c = (long long)blockIdx.x * kVT + threadIdx.x; c < cells; c += stride) {
        o0[c] = (float)a[c];
        o1[c] = (float)b[c];
    }
}

struct Lerp { int i0, i1; float f; };
__device__ __forceinline__ Lerp lerp_of(int d, float scale, int n_src)
{
    const float s = ((float)d + 0.5f) * scale - 0.5f;
    const float fl = floorf(s);
    int i = (int)fl;
    Lerp r;
    r.f = s - fl;
    r.i0 = i < 0 ? 0 : (i > n_src - 1 ? n_src - 1 : i);
    ++i;
    r.i1 = i < 0 ? 0 : (i > n_src - 1 ? n_src - 1 : i);
    return r;
}

// grid (cells of the destination, n * 2): image (blockIdx.y & 1) of pair (blockIdx.y >> 1), level s - 1 -> level s
__global__ __launch_bounds__(kVT) void kv_resize(float *pyr0, float *pyr1, long long pyr_cells, long long src_off, int sh, int sw,
                                                 long long dst_off, int dh, int dw)
{
    float *base = ((blockIdx.y & 1) ? pyr1 : pyr0) + (long long)(blockIdx.y >> 1) * pyr_cells;
    const float *src = base + src_off;
    float *dst = base + dst_off;
    const float sx = (float)sw / (float)dw, sy = (float)sh / (float)dh;
    const int cells = dh * dw;
    for (int c = blockIdx.x * kVT + threadIdx.x; c < cells; c += gridDim.x * kVT) {
        const int y = c / dw, x = c - y * dw;
        const Lerp lx = lerp_of(x, sx, sw), ly = lerp_of(y, sy, sh);
        const float *r0 = src + (long long)ly.i0 * sw, *r1 = src + (long long)ly.i1 * sw;
        const float top = r0[lx.i0] * (1.0f - lx.f) + r0[lx.i1] * lx.f;
        const float bot = r1[lx.i0] * (1.0f - lx.f) + r1[lx.i1] * lx.f;
        dst[c] = top * (1.0f - ly.f) + bot * ly.f;
    }
}

// grid (cells, n): centred gradient of I1 at this level
__global__ __launch_bounds__(kVT) void kv_grad(const float *pyr1, long long pyr_cells, long long off, int h, int w, float2 *gxy,
                                               long long cells0)
{
    const float *s = pyr1 + (long long)blockIdx.y * pyr_cells + off;
    float2 *g = gxy + (long long)blockIdx.y * cells0;
    const int cells = h * w;
    for (int c = blockIdx.x * kVT + threadIdx.x; c < cells; c += gridDim.x * kVT) {
        const int y = c / w, x = c - y * w;
        const int xl = x > 0 ? x - 1 : 0, xr = x < w - 1 ? x + 1 : w - 1;
        const int yu = y > 0 ? y - 1 : 0, yd = y < h - 1 ? y + 1 : h - 1;
        g[c] = make_float2(0.5f * (s[(long long)y * w + xr] - s[(long long)y * w + xl]), 0.5f * (s[(long long)yd * w + x] - s[(long long)yu * w + x]));
    }
}

// ---- where a pair's result of warp g lies ----------------------------------------------------------
// done[g * FRLW_MAX_SEQUENCES + pair]: 0 = the pair ran to the end of warp g (the host's buffers hold), else 1 | ub << 1 | pb << 2
struct Src { int ub, pb; };
__device__ __forceinline__ Src result_of(const int *done, int g, int pair, int host_ub, int host_pb)
{
    const int word = done[g * FRLW_MAX_SEQUENCES + pair];
    Src r;
    r.ub = word ? (word >> 1) & 1 : host_ub;
    r.pb = word ? (word >> 2) & 1 : host_pb;
    return r;
}

struct Bufs { float2 *u[2]; float4 *p[2]; };

// grid (cells of the finer level, n): u of the coarser level, bilinear, times inv_step -> the buffer the coarser result is NOT in
__global__ __launch_bounds__(kVT) void kv_upsample(Bufs B, long long cells0, const int *done, int g_prev, int host_ub, int sh, int sw,
                                                   int dh, int dw, float inv_step)
{
    const int pair = blockIdx.y;
    const Src r = result_of(done, g_prev, pair, host_ub, 0);
    const float2 *src = B.u[r.ub] + (long long)pair * cells0;
    float2 *dst = B.u[r.ub ^ 1] + (long long)pair * cells0;
    const float sx = (float)sw / (float)dw, sy = (float)sh / (float)dh;
    const int cells = dh * dw;
    for (int c = blockIdx.x * kVT + threadIdx.x; c < cells; c += gridDim.x * kVT) {
        const int y = c / dw, x = c - y * dw;
        const Lerp lx = lerp_of(x, sx, sw), ly = lerp_of(y, sy, sh);
        const float2 *r0 = src + (long long)ly.i0 * sw, *r1 = src + (long long)ly.i1 * sw;
        const float2 a = r0[lx.i0], b = r0[lx.i1], cc = r1[lx.i0], d = r1[lx.i1];
        const float t1 = a.x * (1.0f - lx.f) + b.x * lx.f, b1 = cc.x * (1.0f - lx.f) + d.x * lx.f;
        const float t2 = a.y * (1.0f - lx.f) + b.y * lx.f, b2 = cc.y * (1.0f - lx.f) + d.y * lx.f;
        dst[c] = make_float2((t1 * (1.0f - ly.f) + b1 * ly.f) * inv_step, (t2 * (1.0f - ly.f) + b2 * ly.f) * inv_step);
    }
}

// ---- warp ----------------------------------------------------------------------------------------
__device__ __forceinline__ void cubic_weights(float t, float w[4])
{
    const float t1 = t + 1.0f;
    w[0] = ((kA * t1 - 5.0f * kA) * t1 + 8.0f * kA) * t1 - 4.0f * kA;
    w[1] = ((kA + 2.0f) * t - (kA + 3.0f)) * (t * t) + 1.0f;
    const float s = 1.0f - t;
    w[2] = ((kA + 2.0f) * s - (kA + 3.0f)) * (s * s) + 1.0f;
    w[3] = 1.0f - w[0] - w[1] - w[2];
}

// mode 0: the first warp of the coarsest level (u = 0, p = 0); 1: the first warp of another level (u where kv_upsample put it,
// p = 0); 2: a later warp (u and p where warp g_prev left them).  Leaves u and p of the pair in buffer 0.   grid (cells, n)
__global__ __launch_bounds__(kVT) void kv_warp(const float *pyr0, const float *pyr1, long long pyr_cells, long long off, int h, int w,
                                               const float2 *gxy, float4 *wd, Bufs B, long long cells0, const int *done, int mode,
                                               int g_prev, int host_ub, int host_pb)
{
    const int pair = blockIdx.y;
    Src r = {0, 0};
    if (mode != 0) r = result_of(done, g_prev, pair, host_ub, host_pb);
    if (mode == 1) r.ub ^= 1;
    const long long slot = (long long)pair * cells0;
    const float *I0 = pyr0 + (long long)pair * pyr_cells + off, *I1 = pyr1 + (long long)pair * pyr_cells + off;
    const float2 *G = gxy + slot;
    const int cells = h * w;
    for (int c = blockIdx.x * kVT + threadIdx.x; c < cells; c += gridDim.x * kVT) {
        const int y = c / w, x = c - y * w;
        float2 u = make_float2(0.0f, 0.0f);
        if (mode != 0) u = B.u[r.ub][slot + c];
        if (mode != 2 || r.ub != 0) B.u[0][slot + c] = u;
        if (mode != 2) B.p[0][slot + c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        else if (r.pb != 0) B.p[0][slot + c] = B.p[1][slot + c];
        const float fx = (float)x + u.x, fy = (float)y + u.y;
        float sI = 0.0f, sX = 0.0f, sY = 0.0f;
        if (fx > -3.0f && fx < (float)(w + 3) && fy > -3.0f && fy < (float)(h + 3)) { // else every tap lies outside (NaN too)
            const float flx = floorf(fx), fly = floorf(fy);
            const int ix = (int)flx, iy = (int)fly;
            float wx[4], wy[4];
            cubic_weights(fx - flx, wx);
            cubic_weights(fy - fly, wy);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int yy = iy + j - 1;
                const bool oky = yy >= 0 && yy < h;
                float rI = 0.0f, rX = 0.0f, rY = 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int xx = ix + i - 1;
                    float tI = 0.0f;
                    float2 tG = make_float2(0.0f, 0.0f);
                    if (oky && xx >= 0 && xx < w) {
                        tI = I1[(long long)yy * w + xx];
                        tG = G[(long long)yy * w + xx];
                    }
                    if (i == 0) { rI = wx[0] * tI; rX = wx[0] * tG.x; rY = wx[0] * tG.y; }
                    else { rI = rI + wx[i] * tI; rX = rX + wx[i] * tG.x; rY = rY + wx[i] * tG.y; }
                }
                if (j == 0) { sI = wy[0] * rI; sX = wy[0] * rX; sY = wy[0] * rY; }
                else { sI = sI + wy[j] * rI; sX = sX + wy[j] * rX; sY = sY + wy[j] * rY; }
            }
        }
        const float grad = sX * sX + sY * sY;
        const float rho_c = sI - sX * u.x - sY * u.y - I0[c];
        wd[slot + c] = make_float4(sX, sY, grad, rho_c);
    }
}

// ---- the verdict on a pair, workgroup-uniform -----------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
        const long long b = __double_as_longlong(v);
        const int lo = __shfl_xor((int)(uint32_t)((unsigned long long)b & 0xffffffffull), m, 64);
        const int hi = __shfl_xor((int)(uint32_t)((unsigned long long)b >> 32), m, 64);
        v += __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
    }
    return v;
}

// The sum of 256 per-thread values in a fixed order, the same in every thread.  `red` holds kVT / kWave doubles.
__device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum(v);
    __syncthreads(); // (red may still be read from an earlier call)
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// True when the pair is through with warp g: its word is set, or (`check`) the error the previous launch left is at or below
// scaled_eps -- then workgroup 0 sets the word, with the buffers this launch was about to read.  All threads must call it.
__device__ __forceinline__ bool pair_done(int *word, bool check, const float *partial, int n_tiles, float scaled_eps, int ub, int pb,
                                          double *red, int *flag)
{
    if (threadIdx.x == 0) *flag = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != 0) return true;
    if (!check) return false;
    double a = 0.0;
    for (int i = threadIdx.x; i < n_tiles; i += kVT) a += (double)partial[i];
    const double error = block_sum(a, red);
    if (error > (double)scaled_eps) return false;
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(word, 1 | (ub << 1) | (pb << 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

struct Ctl {
    int *done;        // this warp's words: done + g * FRLW_MAX_SEQUENCES
    float *partial;   // (n, 2, tiles0)
    int tiles0;
    float scaled_eps;
};

// ---- 5 x 5 median --------------------------------------------------------------------------------
__device__ __forceinline__ void cx(float &a, float &b)
{
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}
// among a[0 .. K-1]: the smallest to a[0], the largest to a[K-1]
template <int K> __device__ __forceinline__ void min_max(float (&a)[14])
{
#pragma unroll
    for (int i = 0; i < K / 2; ++i) cx(a[i], a[K - 1 - i]);
#pragma unroll
    for (int i = 1; i < (K + 1) / 2; ++i) cx(a[0], a[i]);
#pragma unroll
    for (int i = K / 2; i < K - 1; ++i) cx(a[i], a[K - 1]);
}
// Forgetful selection: of 14 values neither the smallest nor the largest can be the median of 25, so both are dropped and the
// next value takes the place of the smallest; the largest is cut off by shrinking K.  Eleven rounds leave three values.
template <int K> struct Forget {
    static __device__ __forceinline__ float run(float (&a)[14], const float (&rest)[11])
    {
        min_max<K>(a);
        a[0] = rest[14 - K];
        return Forget<K - 1>::run(a, rest);
    }
};
template <> struct Forget<3> {
    static __device__ __forceinline__ float run(float (&a)[14], const float (&)[11])
    {
        min_max<3>(a);
        return a[1];
    }
};

// grid (tiles of kMW x kMH, n).  `check`: an outer iteration lies behind this launch, its last error in partial[prev_parity].
__global__ __launch_bounds__(kVT) void kv_median(Ctl C, int h, int w, Bufs B, long long cells0, int ub, int pb, int check, int prev_parity,
                                                 int n_tiles)
{
    __shared__ float2 tile[kMH + 4][kMW + 4];
    __shared__ double red[kVT / kWave];
    __shared__ int flag;
    const int pair = blockIdx.y;
    if (pair_done(C.done + pair, check != 0, C.partial + ((long long)pair * 2 + prev_parity) * C.tiles0, n_tiles, C.scaled_eps, ub, pb, red,
                  &flag))
        return;
    const int tiles_x = (w + kMW - 1) / kMW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kMW, y0 = ty * kMH;
    const float2 *src = B.u[ub] + (long long)pair * cells0;
    for (int i = threadIdx.x; i < (kMH + 4) * (kMW + 4); i += kVT) {
        const int ly = i / (kMW + 4), lx = i - ly * (kMW + 4);
        int x = x0 + lx - 2, y = y0 + ly - 2;
        x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x); // replicated border
        y = y < 0 ? 0 : (y > h - 1 ? h - 1 : y);
        tile[ly][lx] = src[(long long)y * w + x];
    }
    __syncthreads();
    const int ly = threadIdx.x / kMW, lx = threadIdx.x - ly * kMW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    float a[14], b[14], ra[11], rb[11];
#pragma unroll
    for (int k = 0; k < 25; ++k) {
        const float2 v = tile[ly + k / 5][lx + k % 5];
        if (k < 14) { a[k] = v.x; b[k] = v.y; }
        else { ra[k - 14] = v.x; rb[k - 14] = v.y; }
    }
    B.u[ub ^ 1][(long long)pair * cells0 + (long long)y * w + x] = make_float2(Forget<14>::run(a, ra), Forget<14>::run(b, rb));
}

// ---- one inner iteration -------------------------------------------------------------------------
// grid (tiles of kTW x kTH, n).  j: the launch's index within the warp (0 = no error yet); reads u[ub], p[pb], writes the others.
__global__ __launch_bounds__(kVT) void kv_iter(Ctl C, int h, int w, const float4 *wd, Bufs B, long long cells0, int ub, int pb, int j,
                                               int n_tiles, float l_t, float theta, float taut, int *iters, int iters_stride)
{
    __shared__ float2 un[kRH][kRW + 1];
    __shared__ double red[kVT / kWave];
    __shared__ int flag;
    const int pair = blockIdx.y;
    float *partial = C.partial + (long long)pair * 2 * C.tiles0;
    if (pair_done(C.done + pair, j > 0, partial + (long long)((j - 1) & 1) * C.tiles0, n_tiles, C.scaled_eps, ub, pb, red, &flag)) return;
    if (iters && blockIdx.x == 0 && threadIdx.x == 0) iters[(long long)pair * iters_stride] += 1; // launches of a stream run one after the other
    const int tiles_x = (w + kTW - 1) / kTW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kTW, y0 = ty * kTH;
    const long long slot = (long long)pair * cells0;
    const float4 *WD = wd + slot, *P = B.p[pb] + slot;
    const float2 *U = B.u[ub] + slot;
    float2 *Un = B.u[ub ^ 1] + slot;
    float4 *Pn = B.p[pb ^ 1] + slot;
    float err = 0.0f;
    for (int i = threadIdx.x; i < kRH * kRW; i += kVT) {
        const int ly = i / kRW, lx = i - ly * kRW;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h) continue;
        const long long c = (long long)y * w + x;
        const float4 d = WD[c], p = P[c];
        const float2 u = U[c];
        const float rho = d.w + d.x * u.x + d.y * u.y;
        const float thr = l_t * d.z;
        float fi = 0.0f;
        if (rho < -thr) fi = l_t;
        else if (rho > thr) fi = -l_t;
        else if (d.z > 1.1920929e-07f) fi = -rho / d.z;
        const float v1 = u.x + fi * d.x, v2 = u.y + fi * d.y;
        float dx1 = p.x, dx2 = p.z, dy1 = p.y, dy2 = p.w;
        if (x > 0) { const float4 l = P[c - 1]; dx1 = p.x - l.x; dx2 = p.z - l.z; }
        if (y > 0) { const float4 t = P[c - w]; dy1 = p.y - t.y; dy2 = p.w - t.w; }
        const float n1 = v1 + theta * (dx1 + dy1), n2 = v2 + theta * (dx2 + dy2);
        un[ly][lx] = make_float2(n1, n2);
        if (lx < kTW && ly < kTH) { // the tile's own pixel
            Un[c] = make_float2(n1, n2);
            const float e1 = n1 - u.x, e2 = n2 - u.y;
            err += e1 * e1 + e2 * e2;
        }
    }
    const double total = block_sum((double)err, red); // (its barriers also publish `un`)
    if (threadIdx.x == 0) partial[(long long)(j & 1) * C.tiles0 + blockIdx.x] = (float)total;
    for (int i = threadIdx.x; i < kTH * kTW; i += kVT) {
        const int ly = i / kTW, lx = i - ly * kTW;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h) continue;
        const long long c = (long long)y * w + x;
        const float2 me = un[ly][lx];
        float u1x = 0.0f, u2x = 0.0f, u1y = 0.0f, u2y = 0.0f;
        if (x < w - 1) { const float2 r = un[ly][lx + 1]; u1x = r.x - me.x; u2x = r.y - me.y; }
        if (y < h - 1) { const float2 b = un[ly + 1][lx]; u1y = b.x - me.x; u2y = b.y - me.y; }
        const float g1 = sqrtf(u1x * u1x + u1y * u1y), g2 = sqrtf(u2x * u2x + u2y * u2y);
        const float den1 = 1.0f + taut * g1, den2 = 1.0f + taut * g2;
        const float4 p = P[c];
        Pn[c] = make_float4((p.x + taut * u1x) / den1, (p.y + taut * u1y) / den1, (p.z + taut * u2x) / den2, (p.w + taut * u2y) / den2);
    }
}

// grid (cells, n)
__global__ __launch_bounds__(kVT) void kv_out(Bufs B, long long cells0, const int *done, int g_last, int host_ub, float2 *flows)
{
    const int pair = blockIdx.y;
    const Src r = result_of(done, g_last, pair, host_ub, 0);
    const float2 *src = B.u[r.ub] + (long long)pair * cells0;
    float2 *dst = flows + (long long)pair * cells0;
    const long long stride = (long long)gridDim.x * kVT;
    for (long long c = (long long)blockIdx.x * kVT + threadIdx.x; c < cells0; c += stride) dst[c] = src[c];
}

std::atomic<unsigned long long> g_tvl1_counts[2]; // [0] calls served, [1] kernel launches they enqueued

int params_of(const frlw_tvl1_params_t *in, Params &P)
{
    P = Params{5, 5, 30, 10, 5, 0.25f, 0.15f, 0.3f, 0.01f, 0.8f};
    if (in) {
        if (in->struct_size < 8 || in->struct_size > 4096) return FRLW_ERR_ARG;
        const size_t have = (size_t)in->struct_size;
#define TVL1_FIELD(name) if (have >= offsetof(frlw_tvl1_params_t, name) + sizeof(in->name)) P.name = in->name
        TVL1_FIELD(nscales); TVL1_FIELD(warps); TVL1_FIELD(inner); TVL1_FIELD(outer); TVL1_FIELD(median);
        TVL1_FIELD(tau); TVL1_FIELD(lambda); TVL1_FIELD(theta); TVL1_FIELD(epsilon); TVL1_FIELD(scale_step);
#undef TVL1_FIELD
    }
    if (P.nscales < 1 || P.nscales > kMaxLevels || P.warps < 1 || P.warps > kMaxWarps || P.inner < 1 || P.inner > 100000 || P.outer < 1 ||
        P.outer > 100000 || (P.median > 1 && P.median != 5))
        return FRLW_ERR_ARG;
    if (!(P.tau > 0.0f) || !(P.lambda > 0.0f) || !(P.theta > 0.0f) || !(P.epsilon >= 0.0f) || !(P.scale_step >= 0.25f) || !(P.scale_step <= 0.95f))
        return FRLW_ERR_ARG;
    return FRLW_OK;
}

} // namespace

extern "C" {

int frlw_tvl1_plan(int H, int W, int nscales, double scale_step, int *levels_hw)
{
    if (nscales < 1 || nscales > kMaxLevels || !(scale_step >= 0.25) || !(scale_step <= 0.95) || H < 1 || W < 1) return 0;
    Level lv[kMaxLevels];
    const int n = plan_levels(H, W, nscales, scale_step, lv);
    if (levels_hw)
        for (int s = 0; s < n; ++s) { levels_hw[2 * s] = lv[s].h; levels_hw[2 * s + 1] = lv[s].w; }
    return n;
}

size_t frlw_tvl1_workspace_bytes(int n_pairs, int H, int W, const frlw_tvl1_params_t *params)
{
    Params P;
    Layout L;
    if (params_of(params, P) != FRLW_OK || !layout_of(n_pairs, H, W, P, L)) return 0;
    return L.total;
}

int frlw_tvl1_counts(uint64_t counts[2])
{
    if (!counts) return FRLW_ERR_ARG;
    for (int i = 0; i < 2; ++i) counts[i] = (uint64_t)g_tvl1_counts[i].load(std::memory_order_relaxed);
    return FRLW_OK;
}

int frlw_tvl1_flow_batch(const uint8_t *pairs, int n_pairs, int H, int W, const frlw_tvl1_params_t *params, float *flows,
                         int32_t *iters_out, void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    Params P;
    Layout L;
    if (!pairs || !flows || !workspace || ((uintptr_t)flows & 7u) || ((uintptr_t)workspace & 15u)) return FRLW_ERR_ARG;
    if (params_of(params, P) != FRLW_OK || !layout_of(n_pairs, H, W, P, L)) return FRLW_ERR_ARG;
    if (workspace_bytes < L.total) return FRLW_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    int *done = (int *)(ws + L.done);
    float *pyr0 = (float *)(ws + L.pyr0), *pyr1 = (float *)(ws + L.pyr1);
    float2 *gxy = (float2 *)(ws + L.gxy);
    float4 *wd = (float4 *)(ws + L.wd);
    Bufs B;
    for (int b = 0; b < 2; ++b) { B.u[b] = (float2 *)(ws + L.u[b]); B.p[b] = (float4 *)(ws + L.p[b]); }
    const int n = n_pairs, nl = L.n_levels;
    unsigned long long launches = 0;
    auto cells_grid = [&](long long cells) { // grid.x of the cell-strided kernels: about 2048 workgroups over the batch
        int gx = grid_for(cells, kVT);
        if (gx > 2048 / n + 1) gx = 2048 / n + 1;
        return gx;
    };
    (void)hipGetLastError();
    HIP_TRY(hipMemsetAsync(done, 0, (size_t)nl * P.warps * FRLW_MAX_SEQUENCES * sizeof(int), st));
    if (iters_out) HIP_TRY(hipMemsetAsync(iters_out, 0, (size_t)n * nl * P.warps * sizeof(int32_t), st));
    hipLaunchKernelGGL(kv_u8, dim3(cells_grid(L.cells0), n), dim3(kVT), 0, st, pairs, L.cells0, pyr0, pyr1, L.pyr_cells);
    ++launches;
    for (int s = 1; s < nl; ++s) {
        hipLaunchKernelGGL(kv_resize, dim3(cells_grid((long long)L.lv[s].h * L.lv[s].w), 2 * n), dim3(kVT), 0, st, pyr0, pyr1, L.pyr_cells,
                           L.lv[s - 1].off, L.lv[s - 1].h, L.lv[s - 1].w, L.lv[s].off, L.lv[s].h, L.lv[s].w);
        ++launches;
    }
    const float l_t = P.lambda * P.theta, taut = P.tau / P.theta, inv_step = 1.0f / P.scale_step;
    int ub = 0, pb = 0, g = 0; // the buffers a pair that runs every launch has its u and p in; the warp's index in the call
    int host_done[FRLW_MAX_SEQUENCES];
    for (int s = nl - 1; s >= 0; --s) {
        const int h = L.lv[s].h, w = L.lv[s].w;
        const long long cells = (long long)h * w;
        const int n_tiles = tiles_of(h, w), m_tiles = ((w + kMW - 1) / kMW) * ((h + kMH - 1) / kMH);
        const float scaled_eps = P.epsilon * P.epsilon * (float)cells;
        hipLaunchKernelGGL(kv_grad, dim3(cells_grid(cells), n), dim3(kVT), 0, st, (const float *)pyr1, L.pyr_cells, L.lv[s].off, h, w, gxy,
                           L.cells0);
        ++launches;
        if (s != nl - 1) {
            hipLaunchKernelGGL(kv_upsample, dim3(cells_grid(cells), n), dim3(kVT), 0, st, B, L.cells0, (const int *)done, g - 1, ub,
                               L.lv[s + 1].h, L.lv[s + 1].w, h, w, inv_step);
            ++launches;
        }
        for (int wi = 0; wi < P.warps; ++wi, ++g) {
            const int mode = wi > 0 ? 2 : (s == nl - 1 ? 0 : 1);
            hipLaunchKernelGGL(kv_warp, dim3(cells_grid(cells), n), dim3(kVT), 0, st, (const float *)pyr0, (const float *)pyr1, L.pyr_cells,
                               L.lv[s].off, h, w, (const float2 *)gxy, wd, B, L.cells0, (const int *)done, mode, g - 1, ub, pb);
            ++launches;
            ub = 0;
            pb = 0;
            Ctl C = {done + (long long)g * FRLW_MAX_SEQUENCES, (float *)(ws + L.partial), L.tiles0, scaled_eps};
            int *iters = iters_out ? iters_out + (long long)s * P.warps + wi : nullptr; // (+ pair * levels * warps in the kernel)
            int j = 0;
            for (int o = 0; o < P.outer; ++o) {
                if (P.median > 1) {
                    hipLaunchKernelGGL(kv_median, dim3(m_tiles, n), dim3(kVT), 0, st, C, h, w, B, L.cells0, ub, pb, o > 0 ? 1 : 0, (j - 1) & 1,
                                       n_tiles);
                    ++launches;
                    ub ^= 1;
                }
                if (o > 0) { // the one synchronisation of the call: stop enqueuing once every pair is through with this warp
                    HIP_TRY(hipMemcpyAsync(host_done, C.done, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipStreamSynchronize(st));
                    bool all = true;
                    for (int i = 0; i < n; ++i) all = all && host_done[i] != 0;
                    if (all) break;
                }
                for (int i = 0; i < P.inner; ++i, ++j) {
                    hipLaunchKernelGGL(kv_iter, dim3(n_tiles, n), dim3(kVT), 0, st, C, h, w, (const float4 *)wd, B, L.cells0, ub, pb, j, n_tiles,
                                       l_t, P.theta, taut, iters, nl * P.warps);
                    ++launches;
                    ub ^= 1;
                    pb ^= 1;
                }
            }
        }
    }
    hipLaunchKernelGGL(kv_out, dim3(cells_grid(L.cells0), n), dim3(kVT), 0, st, B, L.cells0, (const int *)done, g - 1, ub, (float2 *)flows);
    ++launches;
    HIP_TRY(hipGetLastError());
    g_tvl1_counts[0].fetch_add(1ull, std::memory_order_relaxed);
    g_tvl1_counts[1].fetch_add(launches, std::memory_order_relaxed);
    return FRLW_OK;
}

} // extern "C"
