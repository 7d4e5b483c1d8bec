// taf_fifo.h -- one FIFO step of one TAF cell (generate_taf.py:27,35-49): the arithmetic both TAF paths must share bit for bit.
// Expects frlw_consts.h (kMaxK) and the HIP runtime.
#pragma once
#include "frlw_consts.h"

namespace {
using namespace frlw;
// Cell without events: every slot - 1; otherwise shift down (slot k + 1, - 1) and the mean enters at K - 1.  `has` false (window
// empty in the whole sequence, :40-41): unchanged.
__device__ __forceinline__ float fifo_mean(uint32_t n, float sum) { return sum / ((float)n + 1e-8f); } // generate_taf.py:27
__device__ __forceinline__ void fifo_step(float (&st)[kMaxK], int K, bool has, uint32_t n, float mean)
{
    const bool hit = n != 0u;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        const float nxt = k + 1 < kMaxK ? st[k + 1] : 0.0f;
        const float v = (hit ? nxt : st[k]) - 1.0f;
        const float nv = (hit && k == K - 1) ? mean : v;
        st[k] = has ? nv : st[k];
    }
}
} // namespace
