// enc_sae.h -- Surface of Active Events: SaeParams and k_sae_tile.
// Expects enc_tile.h (Owner, CPT).  Last writer per cell = LDS atomicMax over (position, t bits) (order-free), exp epilogue.
#pragma once
#include "enc_tile.h"

namespace {
struct SaeParams {
    int H, W, twl, tiles_x, n_lamda;
    float lam[FRLW_MAX_LAMDAS];
    float nowf;
    const float *mem_in;
    float *mem_out;
    float *out_f32;
    uint8_t *out_u8;
};

template <int NT>
__global__ __launch_bounds__(NT) void k_sae_tile(const uint2 *rec, const uint32_t *base, SaeParams q)
{
    // last writer in stream order per cell = max over (position in the tile's record list, t bits)
    constexpr int NC = NT * CPT;
    __shared__ unsigned long long last[NC];
    const int t = threadIdx.x, tile = blockIdx.x;
#pragma unroll
    for (int j = 0; j < CPT; ++j) last[t + NT * j] = 0ull;
    __syncthreads();
    const uint32_t beg = base[tile], end = base[tile + 1];
    for (uint32_t i = beg + t; i < end; i += NT) {
        const uint2 r = rec[i];
        const unsigned long long key = ((unsigned long long)(i - beg + 1u) << 32) | r.y;
        atomicMax(&last[r.x & (NC - 1)], key);
    }
    __syncthreads();
    const TileGeom g = tile_geom(tile, q.tiles_x, q.twl, q.H, q.W);
    const Owner<CPT> ow = make_owner<NT, CPT>(g, q.W, 0);
    const long long plane = (long long)q.H * q.W;
    const float init = (0.0f + q.nowf) - 5000000.0f; // generate_surfaceofactiveevents.py:48
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        if (ow.ok[j]) {
            const unsigned long long key = last[t + NT * j];
            float tv = key ? __uint_as_float((uint32_t)key) : init;
            const long long idx = ow.p * plane + ow.pix[j];
            if (q.mem_in) {
                const float m = q.mem_in[idx];
                if (!(tv > m)) tv = m; // torch.where(t_img > memory, t_img, memory) :52
            }
            q.mem_out[idx] = tv;
            const float dt = tv - q.nowf;
            for (int l = 0; l < q.n_lamda; ++l) {
                const float v = expf(q.lam[l] * dt) * 255.0f;
                const long long oi = (long long)l * 2 * plane + idx;
                if (q.out_f32) q.out_f32[oi] = v;
                if (q.out_u8) q.out_u8[oi] = f32_to_u8(v);
            }
        }
    }
}
} // namespace
