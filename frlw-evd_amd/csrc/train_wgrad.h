// train_wgrad.h -- the weight gradient around k_wgrad_mfma (wgrad_mfma.h): the two reductions of its partial tiles and the
// host arithmetic of the pixel splits.  Included inside train_ops.hip's anonymous namespace, after train_weights.h.
//
// dW[r = (ky, kx, ci)][co] = sum over pixels m of x[m shifted by the tap][ci] * dz[m][co].
// 64 x 64 tile of (r, co) per workgroup, 4 wavefronts 2 x 2, k-tiles of 16 pixels, blockIdx.z owns a slice of the
// pixels and writes a partial tile (always: the reduction kernel also converts to torch's layout).
#include "wgrad_mfma.h"

// Thin layers have few output tiles and therefore many pixel splits: first add groups of kWgradGroup partial tiles
// in parallel (same layout), then the final pass below runs over the group sums.  Fixed order -> deterministic.
constexpr int kWgradGroup = 16;
__global__ void k_wgrad_group_sum(const float *partial, int splits, long long per, float *out)
{
    const int g = blockIdx.y;
    const int z0 = g * kWgradGroup, z1 = z0 + kWgradGroup < splits ? z0 + kWgradGroup : splits;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < per; i += (long long)gridDim.x * blockDim.x) {
        float t[kWgradGroup];
#pragma unroll
        for (int u = 0; u < kWgradGroup; ++u) t[u] = z0 + u < z1 ? partial[(long long)(z0 + u) * per + i] : 0.0f;
        float v = 0.0f;
#pragma unroll
        for (int u = 0; u < kWgradGroup; ++u) v += t[u];
        out[(long long)g * per + i] = v;
    }
}

// dw[co][ci][ky][kx] = sum over splits of partial[z][(ky*k + kx)*Cin + ci][co].  32 x 32 tiles through LDS: the
// partials are read along co (coalesced), the gradient is written along ci (contiguous for 1x1, stride k*k else).
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float *partial, int splits, int R, int Cout, int Cin, int k,
                                                      float *dw)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const long long per = (long long)R * Cout;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = r0 + ty + 8 * j, co = c0 + tx;
        float v = 0.0f;
        if (r < R && co < Cout) {
            const float *src = partial + (long long)r * Cout + co;
            int z = 0;
            for (; z + 8 <= splits; z += 8) { // eight independent loads in flight, fixed summation order
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = src[(long long)(z + u) * per];
#pragma unroll
                for (int u = 0; u < 8; ++u) v += t[u];
            }
            for (; z < splits; ++z) v += src[(long long)z * per];
        }
        tile[ty + 8 * j][tx] = v;
    }
    __syncthreads();
    const int kk = k * k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = r0 + tx, co = c0 + ty + 8 * j;
        if (r < R && co < Cout) {
            const int tap = r / Cin, ci = r - tap * Cin;
            dw[((long long)co * Cin + ci) * kk + tap] = tile[tx][ty + 8 * j];
        }
    }
}

// Scratch in partial tiles ("slots"): one per split and, above 64 splits, one per group sum behind them ...
inline long long wgrad_slots(long long sp) { return sp + (sp > 64 ? (sp + kWgradGroup - 1) / kWgradGroup : 0); }
// ... and the inverse: the most splits that fit into `slots` (64 splits need no group sums, so they fit wherever more slots do)
inline long long wgrad_splits_in(long long slots)
{
    if (slots <= 64) return slots;
    long long s = slots * kWgradGroup / (kWgradGroup + 1); // undo the group allowance: s + ceil(s / 16) <= slots
    while (s + (s + kWgradGroup - 1) / kWgradGroup > slots) --s;
    return s > 64 ? s : 64;
}
inline long long wgrad_scratch_floats(int B, int Ho, int Wo, int Cin, int Cout, int k)
{
    const long long R = (long long)k * k * Cin;
    static const long long target = dev_knob("FRLW_WGRAD_TARGET", 1024ll); // four 128 x 128 workgroups per CU (wgrad_want_splits rounds DOWN to it)
    return wgrad_slots(wgrad_want_splits(R, Cout, (long long)B * Ho * Wo, target)) * R * Cout;
}
