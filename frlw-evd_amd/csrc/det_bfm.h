// det_bfm.h -- the BFM stem of the AED recipes as one kernel.  Included inside detector.hip's anonymous namespace.

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

struct BfmOp { int src, dst, C, H, W; const float *w; }; // plan payload: buffer indices, C = 2 TC input channels, packed weights (device)

// packed weights of k_bfm_stem<C / 2>; 0: no kernel (TAF with K = 2, 4 or 8 FIFO slots only)
inline int bfm_weight_count(int C) { return C == 4 ? BfmDims<2>::total : C == 8 ? BfmDims<4>::total : C == 16 ? BfmDims<8>::total : 0; }

inline void launch_bfm_stem(const BfmOp &o, const float *x, float *y, int B, hipStream_t s)
{
    const dim3 grid(conv_grid_1d((long long)B * o.H * o.W));
    if (o.C == 4) hipLaunchKernelGGL(k_bfm_stem<2>, grid, dim3(256), 0, s, x, B, o.H, o.W, o.w, y);
    else if (o.C == 8) hipLaunchKernelGGL(k_bfm_stem<4>, grid, dim3(256), 0, s, x, B, o.H, o.W, o.w, y);
    else hipLaunchKernelGGL(k_bfm_stem<8>, grid, dim3(256), 0, s, x, B, o.H, o.W, o.w, y);
}
