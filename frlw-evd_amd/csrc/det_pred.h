// det_pred.h -- prediction convolutions of one head level (yolo_head.py:205-231, eval branch).  Included inside detector.hip's
// anonymous namespace, after conv_mfma.h (act_apply).
//
// out[b][off + p][j] = f_j(feat[b][p] . w[j] + bias[j]): rows j < 5 (reg, obj) read the first C channels of the level's
// [reg_feat | cls_feat] buffer, rows j >= 5 (cls) the second C; f = sigmoid for j >= 4.  5 + nc outputs per 2 C inputs is no
// work for a matrix pipe: one wavefront owns whole rows (lane l holds float4 chunk l of a row and of every weight row), the
// partial dots are folded over the lanes with a halving butterfly, and the row leaves as 5 + nc consecutive floats of the
// (B, A, 5 + nc) head tensor.  HBM-bound: 2 C * 4 bytes per anchor.
struct PredInferArgs {
    const float *x; int cs, co, C; // feature buffer: pixel stride, channel offset of reg_feat (cls_feat follows at + C)
    const float *w, *bias;         // (F, C) rows as above, (F)
    float *out; int F, hw, off; long long out_bs; // F = 5 + nc; anchors of this level per image, first anchor, image stride
    long long M;
};

template <int NG>
__device__ __forceinline__ void pred_infer_body(const PredInferArgs &a, int block, int n_blocks)
{
    const int lane = threadIdx.x & 63, wave = block * 4 + (threadIdx.x >> 6), n_waves = n_blocks * 4;
    const int c4n = a.C / 4;
    const bool has = lane < c4n;
    float4 w[NG * 8];
#pragma unroll
    for (int j = 0; j < NG * 8; ++j) w[j] = (j < a.F && has) ? *(const float4 *)(a.w + (long long)j * a.C + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int sel = ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1); // output index this lane ends up with
    float bias[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) bias[g] = g * 8 + sel < a.F ? a.bias[g * 8 + sel] : 0.0f;
    for (long long m = wave; m < a.M; m += n_waves) {
        const float *row = a.x + m * a.cs + a.co + 4 * lane;
        const float4 xr = has ? *(const float4 *)row : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 xc = has ? *(const float4 *)(row + a.C) : make_float4(0.f, 0.f, 0.f, 0.f);
        float res[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int j = g * 8 + t;
                const float4 x = j < 5 ? xr : xc;
                v[t] = x.x * w[j].x + x.y * w[j].y + x.z * w[j].z + x.w * w[j].w;
            }
            float q[4], r2[2];
            const bool h1 = lane & 32, h2 = lane & 16, h3 = lane & 8;
#pragma unroll
            for (int t = 0; t < 4; ++t) q[t] = (h1 ? v[4 + t] : v[t]) + __shfl_xor(h1 ? v[t] : v[4 + t], 32, 64);
#pragma unroll
            for (int t = 0; t < 2; ++t) r2[t] = (h2 ? q[2 + t] : q[t]) + __shfl_xor(h2 ? q[t] : q[2 + t], 16, 64);
            float c = (h3 ? r2[1] : r2[0]) + __shfl_xor(h3 ? r2[0] : r2[1], 8, 64);
            c += __shfl_xor(c, 4, 64);
            c += __shfl_xor(c, 2, 64);
            c += __shfl_xor(c, 1, 64);
            res[g] = c;
        }
        if ((lane & 7) == 0) {
            const long long b = m / a.hw, p = m - b * a.hw;
            float *o = a.out + b * a.out_bs + (a.off + p) * a.F;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int j = g * 8 + sel;
                if (j < a.F) {
                    const float t = res[g] + bias[g];
                    o[j] = j >= 4 ? act_apply(t, ACT_SIGMOID) : t;
                }
            }
        }
    }
}

// the head levels' prediction ops as ONE launch (consecutive OP_PRED ops of a plan: collect_pred of detector.hip): workgroups
// [first[l], first[l + 1]) serve level l
struct PredInferMulti { PredInferArgs lv[4]; int first[5]; int n; };
template <int NG>
__global__ __launch_bounds__(256) void k_pred_infer(PredInferMulti a)
{
    int l = 0;
    while (l + 1 < a.n && (int)blockIdx.x >= a.first[l + 1]) ++l;
    pred_infer_body<NG>(a.lv[l], (int)blockIdx.x - a.first[l], a.first[l + 1] - a.first[l]);
}

// a.lv[0 .. a.n) with x and out bound (levels of one F): >= 8 rows per wavefront, 2048 workgroups per level at most
inline void launch_pred_infer(PredInferMulti a, int B, hipStream_t s)
{
    for (int l = 0; l < a.n; ++l) {
        a.lv[l].M = (long long)B * a.lv[l].hw;
        const long long wg = (a.lv[l].M + 31) / 32;
        a.first[l + 1] = a.first[l] + (int)(wg > 2048 ? 2048 : wg);
    }
    if (a.lv[0].F <= 8) hipLaunchKernelGGL(k_pred_infer<1>, dim3(a.first[a.n]), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_pred_infer<2>, dim3(a.first[a.n]), dim3(256), 0, s, a);
}
