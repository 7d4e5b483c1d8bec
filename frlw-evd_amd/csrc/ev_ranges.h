// ev_ranges.h -- kf_gather_ranges: the record ranges of frlw_ev_encode_ranges, copied one behind the other, so that overlapping
// or nested label windows become the contiguous sequences frlw_ev_encode_batch's partition takes.
// Expects taf_plan.h (kMaxSeq) and hip_runtime.
#pragma once
#include "taf_plan.h"

namespace {
constexpr int kGT = 256;                  // threads of a gather workgroup
constexpr int kGU = 8;                    // 8-byte loads in flight per thread
constexpr int kGSlice = 2 * kGU * kGT;    // records per workgroup

// The windows of one call, by value (host arrays in, no device table to fill: the call stays capturable).
struct RangeTab {
    long long lo[kMaxSeq];       // first record of window w in the source
    long long dst[kMaxSeq + 1];  // first record of window w in the copy: the prefix sums of the lengths
    uint32_t blk[kMaxSeq + 1];   // first workgroup of w
    int n;
};

// window of this workgroup: the last w with blk[w] <= b (empty windows own no workgroup); uniform (the lookup of
// encoders_batch.hip's counting grid)
__device__ __forceinline__ int range_of_block(const RangeTab &T, uint32_t b)
{
    int a = 0, z = T.n; // blk[a] <= b < blk[z]
    while (z - a > 1) {
        const int m = (a + z) >> 1;
        if (T.blk[m] <= b) a = m; else z = m;
    }
    return a;
}

// grid: one workgroup per slice of kGSlice records of a window.  8-byte accesses: a window may start at an odd record.
__global__ __launch_bounds__(kGT) void kf_gather_ranges(const uint2 *src, RangeTab T, uint2 *dst)
{
    const int t = threadIdx.x;
    const int w = range_of_block(T, blockIdx.x);
    const long long len = T.dst[w + 1] - T.dst[w];
    const long long a0 = (long long)(blockIdx.x - T.blk[w]) * kGSlice;
    const long long a1 = a0 + kGSlice < len ? a0 + kGSlice : len;
    const uint2 *s = src + T.lo[w];
    uint2 *d = dst + T.dst[w];
    for (long long i0 = a0; i0 < a1; i0 += kGU * kGT) {
        uint2 r[kGU];
#pragma unroll
        for (int u = 0; u < kGU; ++u) {
            const long long i = i0 + u * kGT + t;
            r[u] = s[i < a1 ? i : a1 - 1];
        }
#pragma unroll
        for (int u = 0; u < kGU; ++u) {
            const long long i = i0 + u * kGT + t;
            if (i < a1) d[i] = r[u];
        }
    }
}
} // namespace
