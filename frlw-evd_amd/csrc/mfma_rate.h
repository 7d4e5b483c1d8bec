// mfma_rate.h -- frlw_selftest_mfma_f32_rate's kernel (included by detector.hip after conv_mfma.h: f32x16).  Bare fp32 MFMA loop:
// every wavefront of every CU issues v_mfma_f32_32x32x2_f32 back to back on four accumulators, operands in registers (random, so
// that the chip sees the switching activity of real data).  What this sustains is the rate the convolutions can at best approach
// on this chip under load: the 157.3 TFLOP/s of the data sheet assume 2.4 GHz.
template <int NACC>
__global__ __launch_bounds__(256) void k_mfma_f32_rate(int iters, const float *seed, float *sink)
{
    const int lane = threadIdx.x & 63;
    float a0 = seed[lane], a1 = seed[64 + lane], b0 = seed[128 + lane], b1 = seed[192 + lane];
    f32x16 c00, c01, c10, c11;
#pragma unroll
    for (int r = 0; r < 16; ++r) { c00[r] = 0.f; c01[r] = 0.f; c10[r] = 0.f; c11[r] = 0.f; }
#pragma nounroll
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, c00, 0, 0, 0);
            c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, c01, 0, 0, 0);
            if (NACC == 4) {
                c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, c10, 0, 0, 0);
                c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c11, 0, 0, 0);
            } else if (NACC == 2) {
                c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, c00, 0, 0, 0);
                c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c01, 0, 0, 0);
            } else {
                c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, c00, 0, 0, 0);
                c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c00, 0, 0, 0);
            }
        }
        a0 = -a0; b1 = -b1; // keep the sums bounded
    }
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += c00[r] + c01[r] + c10[r] + c11[r];
    if (t == 123.456f) sink[0] = t; // never true: keeps the loop alive
}
