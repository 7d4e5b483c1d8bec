// enc_batch.h -- what the batched record-range encoders share (encoders_batch.hip, motion.hip): the by-value window table and
// decode descriptor, the workgroup -> window search, the zeroing kernel and the host-side range checks.  Every unit that includes
// this gets its own copy (internal linkage): the kernels of a unit stay in that unit's code object.
#pragma once
#include "frlw_common.h"

namespace {
using namespace frlw;

constexpr int kMaxSeq = FRLW_MAX_SEQUENCES;
constexpr int kBT = 256;                   // threads of a counting workgroup
constexpr int kBU = 8;                     // records in flight per thread
constexpr int kBSlice = 2 * kBU * kBT;     // records per workgroup

// The windows of one call, passed by value (host arrays in, no device table to fill: the call stays capturable).
struct BatchTab {
    long long lo[kMaxSeq], hi[kMaxSeq]; // record range of window / sequence w
    long long t0[kMaxSeq];              // SAE: now - window_us
    float nowf[kMaxSeq];                // SAE: float(now)
    uint32_t blk[kMaxSeq + 1];          // first workgroup of w in the counting grid
    int n;
};

// window of this workgroup: the last w with blk[w] <= b (empty windows own no workgroup); uniform, seven scalar steps at most
__device__ __forceinline__ int window_of_block(const BatchTab &T, uint32_t b)
{
    int a = 0, z = T.n; // blk[a] <= b < blk[z]
    while (z - a > 1) {
        const int m = (a + z) >> 1;
        if (T.blk[m] <= b) a = m; else z = m;
    }
    return a;
}

__global__ __launch_bounds__(256) void kb_zero(uint4 *planes, long long n16, WsHeader *hdr)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) planes[i] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr->status = 0;
}

struct BatchDecode {
    const uint2 *data;
    const uint16_t *xmap, *ymap;
    int map_w, map_h, H, W;
};

size_t batch_bytes(int n, int H, int W, size_t cell_bytes)
{
    if (n < 1 || n > kMaxSeq || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31)) return 0;
    return kHeaderBytes + (((size_t)n * 2 * (size_t)H * (size_t)W * cell_bytes + 15) & ~(size_t)15); // kb_zero stores 16-byte words
}

int events_check(const frlw_events_t *ev)
{
    if (!ev || ev->n < 0 || (ev->n > 0 && !ev->data) || (ev->xmap == nullptr) != (ev->ymap == nullptr) || !tuning_valid(ev->tuning))
        return FRLW_ERR_ARG;
    if (ev->xmap && (ev->map_w <= 0 || ev->map_h <= 0)) return FRLW_ERR_ARG;
    return ev->layout == FRLW_LAYOUT_DAT8 ? FRLW_OK : FRLW_ERR_UNSUPPORTED;
}

// record ranges -> the counting grid; false: a range outside the array, running backwards or too long for the 32-bit position / count
bool tab_ranges(BatchTab &T, const frlw_events_t *ev, int n)
{
    T.n = n;
    unsigned long long blocks = 0;
    for (int w = 0; w < n; ++w) {
        if (T.lo[w] < 0 || T.hi[w] < T.lo[w] || T.hi[w] > ev->n || T.hi[w] - T.lo[w] >= 0xffffffffll) return false;
        T.blk[w] = (uint32_t)blocks;
        blocks += (unsigned long long)((T.hi[w] - T.lo[w] + kBSlice - 1) / kBSlice);
        if (blocks >= (1ull << 31)) return false;
    }
    T.blk[n] = (uint32_t)blocks;
    for (int w = n; w < kMaxSeq; ++w) { T.lo[w] = T.hi[w] = 0; T.blk[w + 1] = T.blk[n]; }
    return true;
}

BatchDecode decode_of(const frlw_events_t *ev, int H, int W)
{
    BatchDecode D;
    D.data = (const uint2 *)ev->data; D.xmap = ev->xmap; D.ymap = ev->ymap; D.map_w = ev->map_w; D.map_h = ev->map_h; D.H = H; D.W = W;
    return D;
}

} // namespace
