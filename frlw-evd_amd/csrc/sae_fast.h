// sae_fast.h -- Surface of Active Events / Event Count Image through the chunk-major partition: SaeFastP, kf_sae_sub.
// Expects taf_decode.h (FastHeader) and taf_column.h.
#pragma once
#include "taf_column.h"
#include "taf_decode.h"

namespace {
// ---- Surface of Active Events through the chunk-major partition (small single calls) ------------------------------------
// generate_leaky_cuda (generate_surfaceofactiveevents.py:44-80): t_img[p, y, x] = float(t) of the cell's LAST event in stream
// order, max with the memory, exp(lambda (t_img - now)) * 255.  The general path takes five launches (41 us for 1 M events at
// 304x240).  Here: kf_scatter_cm<.., SAE> writes records {position in the sequence << 12 | cell} chunk-major, and one workgroup
// per sub-tile takes the maximum record per cell with LDS atomics -- straight from the runs, no list, no order needed -- reads
// the time of that one event from the DAT array and writes memory and outputs with the arithmetic of k_sae_tile (enc_sae.h).
struct SaeFastP {
    int H, W, twl, thl, tiles_x, T, n_lamda;
    float lam[FRLW_MAX_LAMDAS > 21 ? FRLW_MAX_LAMDAS : 21]; // (ECI: the count -> value table)
    float nowf;
    const uint2 *data;
    const float *mem_in;
    float *mem_out, *out_f32;
    uint8_t *out_u8;
    FastHeader *hdr;
};

// ECI (template flag): the same walk over the runs COUNTS the records per cell instead; the image is the 21-entry table of
// n sequential +0.05f adds, clamped and scaled (generate_eventcountimage.py:32-41; q.lam[] carries the table, n_lamda = 21).
template <bool ECI>
__global__ __launch_bounds__(kSubCells) void kf_sae_sub(SaeFastP q, CmP cm, SeqTab S)
{
    __shared__ uint32_t s_last[kSubCells];
    __shared__ uint32_t s_colL[kColEv + 1], s_colD[kColEv], s_wsum[kSubCells / kWave + 1];
    constexpr int NT = kSubCells;
    const int tid = threadIdx.x;
    // (the bin through the XCD mapping: the runs of neighbouring bins share cache lines of rec[])
    const int sg = (int)xcd_owned_index(blockIdx.x, gridDim.x), tile = sg / kFW, sub = sg - tile * kFW; // (one sequence)
    if (q.hdr->status != 0) return;
    s_last[tid] = 0u;
    const int C = S.chunk0[1] - S.chunk0[0]; // (<= kColEv)
    col_load<NT>(cm, S, 0, sg, s_colL, s_colD, s_wsum); // the sub-tile's column of the directory
    // the runs: groups of 16 lanes take a run each, ten runs' loads in flight; the later record of a cell wins (position in the high bits)
    col_gather<NT / 16, 10>(s_colL, s_colD, C, tid >> 4, tid & 15, cm.rec, [&](uint32_t, uint32_t w) {
        if (ECI) atomicAdd(&s_last[w & 255u], 1u); else atomicMax(&s_last[w & 255u], w);
    });
    __syncthreads();
    // cell tid: pixel 128 sub + tid / 2 of the tile, polarity tid & 1
    const int ty = tile / q.tiles_x, tx = tile - ty * q.tiles_x;
    const int x0 = tx << q.twl, y0 = ty << q.thl, tw1 = (1 << q.twl) - 1;
    const int pol = tid & 1, pt = sub * (kSubCells / 2) + (tid >> 1);
    const int py = y0 + (pt >> q.twl), px = x0 + (pt & tw1);
    if (py >= q.H || px >= q.W) return;
    const long long plane = (long long)q.H * q.W, idx = (long long)pol * plane + (long long)py * q.W + px;
    const uint32_t w = s_last[tid];
    if (ECI) {
        const float v = q.lam[w > 20u ? 20u : w];
        if (q.out_f32) q.out_f32[idx] = v;
        if (q.out_u8) q.out_u8[idx] = f32_to_u8(v);
        return;
    }
    const float init = (0.0f + q.nowf) - 5000000.0f; // generate_surfaceofactiveevents.py:48
    // (the scatter stores position + 1: a record is never 0, 0 = the cell has no event)
    float tv = w ? (float)q.data[S.ev0[0] + (long long)(w >> kCellBits) - 1].x : init; // float(t), :76
    if (q.mem_in) {
        const float m = q.mem_in[idx];
        if (!(tv > m)) tv = m; // torch.where(t_img > memory, t_img, memory), :52
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
} // namespace
