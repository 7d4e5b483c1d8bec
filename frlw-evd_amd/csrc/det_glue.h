// det_glue.h -- nearest x2 upsample and the SPP max-pools.  Included inside detector.hip's anonymous namespace, after det_focus.h.

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

struct UpsampleOp { int src, dst, C, H, W, cs_src, co_src, cs_dst, co_dst; }; // plan payload: buffer indices, the (B, H, W, C) source slice

inline void launch_upsample2x(const UpsampleOp &o, const float *x, float *y, int B, hipStream_t s)
{
    const long long total = (long long)B * 4 * o.H * o.W * o.C;
    hipLaunchKernelGGL(k_upsample2x, dim3(conv_grid_1d(total)), dim3(256), 0, s, x, B, o.H, o.W, o.C, o.cs_src, o.co_src, y, o.cs_dst, o.co_dst);
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

struct SppOp { int buf, C, H, W, cs; }; // plan payload: the buffer's index, channels pooled, pixel stride (>= 4 C)

inline void launch_spp_pool(const SppOp &o, float *buf, int B, hipStream_t s)
{
    const size_t lds = (size_t)2 * o.H * o.W * (kSppCh + 1) * sizeof(float);
    launch_lds(k_spp_pool, dim3((o.C + kSppCh - 1) / kSppCh, B), dim3(256), lds, s, buf, o.H, o.W, o.C, o.cs);
}
