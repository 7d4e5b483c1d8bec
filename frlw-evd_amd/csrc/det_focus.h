// det_focus.h -- Focus (space-to-depth) and the fused Focus + stem convolution of the detector plan: kernels, the one place that
// resolves a stem shape to its kernel (focus_stem_plan), launchers.  Included inside detector.hip's anonymous namespace, after conv_mfma.h.

// A launch with dynamic LDS (every launcher of the det_*.h headers): more than the 64 KB a kernel may use unasked is requested
// first -- at every launch, because the attribute is per device and a plan may run on another device than the last one.
template <class Kern, class... Args>
inline void launch_lds(Kern kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args)
{
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
}

// Focus: (B, C, H, W) NCHW -> (B, H/2, W/2, 4C) NHWC, channel blocks TL, BL, TR, BR (network_blocks.py:205-217).
// One workgroup per `Wp` pixels of an output row (b, oy): the 2C input rows are read along x as float2 = the two column
// parities of one output pixel (coalesced; eight loads in flight per thread), transposed through LDS and the piece of the
// output row (Wp x 4C floats, contiguous) is written along its memory order.  (Until round 3: scalar loads, one exposed
// round trip each, and whole rows = three workgroups per CU -- 0.7 TB/s.)
__global__ __launch_bounds__(256) void k_focus(const float *x, int B, int C, int H, int W, float *y, int Wp)
{
    extern __shared__ float frow[]; // [Wp][4C + 1]
    const int Ho = H / 2, Wo = W / 2, C4 = 4 * C, LD = C4 + 1, parts = Wo / Wp;
    const int part = blockIdx.x % parts, row = blockIdx.x / parts;
    const int b = row / Ho, oy = row - b * Ho, j0 = part * Wp;
    // source rows: r = c * 2 + row parity -> x[b][c][2 oy + (r & 1)][:]; pair j of a row = output pixel j, parities 0 / 1
    const int n2 = 2 * C * Wp;
    for (int i0 = threadIdx.x; i0 < n2; i0 += 8 * 256) {
        float2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + 256 * u, ic = i < n2 ? i : n2 - 1;
            const int j = ic % Wp, r = ic / Wp;
            v[u] = *(const float2 *)(x + (((long long)b * C + (r >> 1)) * H + 2 * oy + (r & 1)) * W + 2 * (j0 + j));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + 256 * u;
            if (i < n2) {
                const int j = i % Wp, r = i / Wp, c = r >> 1, py = r & 1;
                frow[j * LD + py * C + c] = v[u].x;           // q = py: TL / BL
                frow[j * LD + (py + 2) * C + c] = v[u].y;     // q = py + 2: TR / BR
            }
        }
    }
    __syncthreads();
    float *dst = y + (((long long)b * Ho + oy) * Wo + j0) * C4;
    for (int i = threadIdx.x; i < Wp * C4; i += 256) dst[i] = frow[(i / C4) * LD + (i % C4)];
}

struct FocusOp { int src, dst, C, H, W; }; // plan payload: buffer indices, the (B, C, H, W) input

inline bool launch_focus(const float *x, int B, int C, int H, int W, float *y, hipStream_t s)
{
    int Wp = W / 2; // pixels per workgroup: pieces of at most 20 KB (eight workgroups per CU) where the row divides
    while (Wp % 2 == 0 && (size_t)Wp * (4 * C + 1) * sizeof(float) > 20 * 1024) Wp /= 2;
    const size_t lds = (size_t)Wp * (4 * C + 1) * sizeof(float);
    if (lds > 150 * 1024) return false;
    launch_lds(k_focus, dim3(B * (H / 2) * ((W / 2) / Wp)), dim3(256), lds, s, x, B, C, H, W, y, Wp);
    return true;
}

// Focus + stem convolution in one kernel (network_blocks.py:205-217 followed by the 3x3 BaseConv of darknet.py:292):
// the space-to-depth image is never written.  A persistent workgroup keeps the whole weight operand (9 * 4 C0 rows of 32
// output channels) in LDS and walks 8 x 16 output tiles: the 10 x 18 halo patch of the Focus image is built in LDS straight
// from the NCHW input (zero outside the frame), and the nine taps are shifted views of that patch -- every input value is
// fetched once instead of nine times.  k pairing as in k_conv_mfma: lane half h supplies ci = 8 j + 4 h + e of a tap.
struct FocusStemArgs {
    const float *x; int H, W;            // (B, C0, H, W)
    const float *w, *bias;               // (9 * 4 C0, 32) rows (tap * 4 C0 + q * C0 + c), q = py + 2 px as in k_focus; bias (Cout)
    float *y; int Cout, y_cs, y_co;      // NHWC view of the output, Ho = H / 2, Wo = W / 2
    int tiles_x, tiles_y, n_tiles;
    int prec;                            // 1: w is the split bf16 image of the operand (conv_mfma.h), three bf16 MFMAs per product
    int npad;                            // columns of the operand: 32, or 64 (k_focus_stem_wide)
};

// floats of LDS in front of the patch: the weight operand (P = 1: its split image, ceil16(K) rows, + the quad offset table)
template <int C0, int P> constexpr int focus_stem_w_floats()
{
    return P == 1 ? (9 * 4 * C0 + 15) / 16 * 16 * 32 + (9 * C0 + 7) / 4 * 4 : 9 * 4 * C0 * 32;
}

template <int C0, int P = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_focus_stem(FocusStemArgs a)
{
    constexpr int CF = 4 * C0, PS = CF + 4, TH = 8, TW = 16, PH = TH + 2, PW = TW + 2, KT = 9 * CF;
    constexpr int QT = CF / 4, NQ = 9 * QT, NS = (NQ + 3) / 4; // P = 1: quads per tap, quads, bf16 k-steps of 16 k = 4 quads
    static_assert(C0 % 2 == 0, "quads are paired");
    extern __shared__ __attribute__((aligned(16))) float fs_lds[];
    float *Ws = fs_lds, *patch = fs_lds + focus_stem_w_floats<C0, P>();
    int *qoff = (int *)(fs_lds + NS * 16 * 32); // P = 1: float offset of quad g inside the patch, relative to the tap-(0, 0) pixel
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (P == 1) {
        for (int i = tid; i < NS * 4 * 32; i += 256) ((uint4 *)Ws)[i] = ((const uint4 *)a.w)[i];
        for (int g = tid; g < NQ; g += 256) { const int tap = g / QT; qoff[g] = ((tap / 3) * PW + tap % 3) * PS + 4 * (g - tap * QT); }
    } else {
        for (int i = tid; i < KT * 8; i += 256) ((float4 *)Ws)[i] = ((const float4 *)a.w)[i];
    }
    const int Ho = a.H / 2, Wo = a.W / 2;
    const int fh = lane >> 5, m = lane & 31, n = lane & 31;
    const int pp0 = (2 * wv + (m >> 4)) * PW + (m & 15);
    const float bias = n < a.Cout ? a.bias[n] : 0.0f;
    // This thread's share of a patch fill: items i = tid + 256 u -> (c, input row iy, column pair jx).  Everything but the
    // tile origin is fixed, so the decomposition is done once; the NEXT tile's values are fetched into registers while the
    // current tile is multiplied and written to LDS after it.
    constexpr int NI = (C0 * 2 * PH * PW + 255) / 256;
    int it_src[NI], it_dst[NI], it_yx[NI];
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        const int i = tid + 256 * u;
        const int jx = i % PW, r = i / PW, iy = r % (2 * PH), c = r / (2 * PH);
        it_src[u] = (c * a.H + iy) * a.W + 2 * jx;
        it_dst[u] = ((iy >> 1) * PW + jx) * PS + (iy & 1) * C0 + c;
        it_yx[u] = i < C0 * 2 * PH * PW ? (iy << 16) | (2 * jx) : -1;
    }
    float2 pv[NI];
    auto fetch = [&](int tile) {
        const int b = tile / (a.tiles_x * a.tiles_y), tr = tile - b * (a.tiles_x * a.tiles_y);
        const int y0 = 2 * ((tr / a.tiles_x) * TH - 1), x0 = 2 * ((tr % a.tiles_x) * TW - 1);
        const float *base = a.x + ((long long)b * C0 * a.H + y0) * a.W + x0;
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int y = y0 + (it_yx[u] >> 16), xc = x0 + (it_yx[u] & 0xFFFF);
            pv[u] = make_float2(0.f, 0.f);
            if (it_yx[u] >= 0 && (unsigned)y < (unsigned)a.H && (unsigned)xc < (unsigned)a.W) pv[u] = *(const float2 *)(base + it_src[u]);
        }
    };
    auto fill = [&](float *dst) {
#pragma unroll
        for (int u = 0; u < NI; ++u)
            if (it_yx[u] >= 0) { dst[it_dst[u]] = pv[u].x; dst[it_dst[u] + 2 * C0] = pv[u].y; } // px = 0: q = py; px = 1: q = py + 2
    };
    if ((int)blockIdx.x < a.n_tiles) fetch(blockIdx.x);
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int b = tile / (a.tiles_x * a.tiles_y), tr = tile - b * (a.tiles_x * a.tiles_y);
        const int fy0 = (tr / a.tiles_x) * TH, fx0 = (tr % a.tiles_x) * TW;
        __syncthreads(); // the previous tile's reads of the patch are done (first pass: the weights are in LDS)
        fill(patch);
        __syncthreads();
        if (tile + (int)gridDim.x < a.n_tiles) fetch(tile + gridDim.x);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        if constexpr (P == 1) {
            // k = tap * CF + channel is cut into quads g = k / 4; bf16 k-step st takes quads 4 st + h and 4 st + 2 + h of lane half h
            // (the pairing of conv_mfma.h: conv_split_kmem), the weights' split image has the matching records
            const float *pbase = patch + pp0 * PS;
            const uint4 *wrec = (const uint4 *)Ws + 2 * fh * 32 + n;
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                const f32x4 q0 = *(const f32x4 *)(pbase + qoff[4 * st + fh]);
                f32x4 q1 = {0.0f, 0.0f, 0.0f, 0.0f};
                if (4 * st + 2 < NQ) q1 = *(const f32x4 *)(pbase + qoff[4 * st + 2 + fh]); // (compile-time: the tail step of K = 360)
                const uint4 bh4 = wrec[st * 4 * 32], bl4 = wrec[st * 4 * 32 + 32];
                const u32x4 bh = {bh4.x, bh4.y, bh4.z, bh4.w}, bl = {bl4.x, bl4.y, bl4.z, bl4.w};
                u32x4 ah, al;
                conv_split8(q0, q1, ah, al);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bl), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
            }
        } else
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float *prow = patch + (pp0 + (t / 3) * PW + (t % 3)) * PS + fh * 4;
            const float *wrow = Ws + (t * CF + 4 * fh) * 32 + n;
#pragma unroll
            for (int j = 0; j < C0 / 2; ++j) {
                const float4 av = *(const float4 *)(prow + 8 * j);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wrow[(8 * j + 0) * 32], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wrow[(8 * j + 1) * 32], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wrow[(8 * j + 2) * 32], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wrow[(8 * j + 3) * 32], acc, 0, 0, 0);
            }
        }
        // C/D layout of the 32x32 MFMA: col = lane & 31 (channel), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (pixel of the wave)
        if (n < a.Cout) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int pm = (r & 3) + 8 * (r >> 2) + 4 * fh;
                const int oy = fy0 + 2 * wv + (pm >> 4), ox = fx0 + (pm & 15);
                if (oy < Ho && ox < Wo)
                    a.y[(((long long)b * Ho + oy) * Wo + ox) * a.y_cs + a.y_co + n] = act_apply(acc[r] + bias, ACT_SILU);
            }
        }
    }
}

// The same walk for the stems k_focus_stem does not take: up to 64 output channels (the Darknet-21 stem of the AED recipes) and
// C0 = 4, 8 (their 2- and 4-bin inputs).  NA = accumulator tiles of 32 channels per wavefront:
//   NA = 2: the whole (9 * 4 C0, 64) operand is resident and channels 0-31 / 32-63 are two f32x16 accumulators fed from ONE read of
//           the patch (one float4 per four k in float32, one split of the quad pair per bf16 k-step) -- the A side of the LDS
//           traffic and the bf16 split are paid once per 64 channels.  C0 <= 10: 90 KiB of weights + 31 KiB of patch at C0 = 10.
//   NA = 1: the workgroup keeps ONE 32-column half of the operand, half = blockIdx.x % (npad / 32).  With npad = 64 (C0 = 16, whose
//           144 KiB operand leaves no room for the 48 KiB patch in the CU's 160 KiB) two workgroups walk the same tiles, one per
//           half, and the input is read twice -- the second time out of L2.  With npad = 32 it is k_focus_stem for C0 = 4, 8.
template <int C0, int P, int NA> constexpr int focus_stem_wide_w_floats()
{
    return P == 1 ? (9 * 4 * C0 + 15) / 16 * 16 * 32 * NA + (9 * C0 + 7) / 4 * 4 : 9 * 4 * C0 * 32 * NA;
}

template <int C0, int P, int NA>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_focus_stem_wide(FocusStemArgs a)
{
    constexpr int CF = 4 * C0, PS = CF + 4, TH = 8, TW = 16, PH = TH + 2, PW = TW + 2, KT = 9 * CF, NL = 32 * NA;
    constexpr int QT = CF / 4, NQ = 9 * QT, NS = (NQ + 3) / 4; // P = 1: quads per tap, quads, bf16 k-steps of 16 k = 4 quads
    static_assert(C0 % 2 == 0, "quads are paired");
    extern __shared__ __attribute__((aligned(16))) float fsw_lds[];
    float *Ws = fsw_lds, *patch = fsw_lds + focus_stem_wide_w_floats<C0, P, NA>();
    int *qoff = (int *)(fsw_lds + NS * 16 * NL); // P = 1: float offset of quad g inside the patch, relative to the tap-(0, 0) pixel
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int halves = a.npad / NL, half = blockIdx.x % halves, wg = blockIdx.x / halves, n_wg = gridDim.x / halves;
    const int c0 = 32 * half; // first output channel (= operand column) of this workgroup
    if (P == 1) { // rows of NL records out of rows of npad
        for (int i = tid; i < NS * 4 * NL; i += 256) ((uint4 *)Ws)[i] = ((const uint4 *)a.w)[(i / NL) * a.npad + c0 + i % NL];
        for (int g = tid; g < NQ; g += 256) { const int tap = g / QT; qoff[g] = ((tap / 3) * PW + tap % 3) * PS + 4 * (g - tap * QT); }
    } else {
        for (int i = tid; i < KT * (NL / 4); i += 256)
            ((float4 *)Ws)[i] = ((const float4 *)a.w)[(i / (NL / 4)) * (a.npad / 4) + c0 / 4 + i % (NL / 4)];
    }
    const int Ho = a.H / 2, Wo = a.W / 2;
    const int fh = lane >> 5, m = lane & 31, n = lane & 31;
    const int pp0 = (2 * wv + (m >> 4)) * PW + (m & 15);
    float bias[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) bias[i] = c0 + 32 * i + n < a.Cout ? a.bias[c0 + 32 * i + n] : 0.0f;
    // the patch fill of k_focus_stem: this thread's items are fixed but for the tile origin; the NEXT tile's values are fetched
    // into registers while the current tile is multiplied
    constexpr int NI = (C0 * 2 * PH * PW + 255) / 256;
    int it_src[NI], it_dst[NI], it_yx[NI];
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        const int i = tid + 256 * u;
        const int jx = i % PW, r = i / PW, iy = r % (2 * PH), c = r / (2 * PH);
        it_src[u] = (c * a.H + iy) * a.W + 2 * jx;
        it_dst[u] = ((iy >> 1) * PW + jx) * PS + (iy & 1) * C0 + c;
        it_yx[u] = i < C0 * 2 * PH * PW ? (iy << 16) | (2 * jx) : -1;
    }
    float2 pv[NI];
    auto fetch = [&](int tile) {
        const int b = tile / (a.tiles_x * a.tiles_y), tr = tile - b * (a.tiles_x * a.tiles_y);
        const int y0 = 2 * ((tr / a.tiles_x) * TH - 1), x0 = 2 * ((tr % a.tiles_x) * TW - 1);
        const float *base = a.x + ((long long)b * C0 * a.H + y0) * a.W + x0;
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int y = y0 + (it_yx[u] >> 16), xc = x0 + (it_yx[u] & 0xFFFF);
            pv[u] = make_float2(0.f, 0.f);
            if (it_yx[u] >= 0 && (unsigned)y < (unsigned)a.H && (unsigned)xc < (unsigned)a.W) pv[u] = *(const float2 *)(base + it_src[u]);
        }
    };
    auto fill = [&](float *dst) {
#pragma unroll
        for (int u = 0; u < NI; ++u)
            if (it_yx[u] >= 0) { dst[it_dst[u]] = pv[u].x; dst[it_dst[u] + 2 * C0] = pv[u].y; } // px = 0: q = py; px = 1: q = py + 2
    };
    if (wg < a.n_tiles) fetch(wg);
    for (int tile = wg; tile < a.n_tiles; tile += n_wg) {
        const int b = tile / (a.tiles_x * a.tiles_y), tr = tile - b * (a.tiles_x * a.tiles_y);
        const int fy0 = (tr / a.tiles_x) * TH, fx0 = (tr % a.tiles_x) * TW;
        __syncthreads(); // the previous tile's reads of the patch are done (first pass: the weights are in LDS)
        fill(patch);
        __syncthreads();
        if (tile + n_wg < a.n_tiles) fetch(tile + n_wg);
        f32x16 acc[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
        if constexpr (P == 1) {
            // quads and records as in k_focus_stem; the split of the patch's quad pair serves both accumulators
            const float *pbase = patch + pp0 * PS;
            const uint4 *wrec = (const uint4 *)Ws + 2 * fh * NL + n;
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                const f32x4 q0 = *(const f32x4 *)(pbase + qoff[4 * st + fh]);
                f32x4 q1 = {0.0f, 0.0f, 0.0f, 0.0f};
                if (4 * st + 2 < NQ) q1 = *(const f32x4 *)(pbase + qoff[4 * st + 2 + fh]); // (compile-time: the tail step of K = 360)
                u32x4 ah, al;
                conv_split8(q0, q1, ah, al);
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const uint4 bh4 = wrec[st * 4 * NL + 32 * i], bl4 = wrec[st * 4 * NL + NL + 32 * i];
                    const u32x4 bh = {bh4.x, bh4.y, bh4.z, bh4.w}, bl = {bl4.x, bl4.y, bl4.z, bl4.w};
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, bh), acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bl), acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bh), acc[i], 0, 0, 0);
                }
            }
        } else
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float *prow = patch + (pp0 + (t / 3) * PW + (t % 3)) * PS + fh * 4;
            const float *wrow = Ws + (t * CF + 4 * fh) * NL + n;
#pragma unroll
            for (int j = 0; j < C0 / 2; ++j) {
                const float4 av = *(const float4 *)(prow + 8 * j);
                const float ae[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < NA; ++i)
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae[e], wrow[(8 * j + e) * NL + 32 * i], acc[i], 0, 0, 0);
            }
        }
        // C/D layout of the 32x32 MFMA: col = lane & 31 (channel), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (pixel of the wave)
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int ch = c0 + 32 * i + n;
            if (ch < a.Cout) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pm = (r & 3) + 8 * (r >> 2) + 4 * fh;
                    const int oy = fy0 + 2 * wv + (pm >> 4), ox = fx0 + (pm & 15);
                    if (oy < Ho && ox < Wo)
                        a.y[(((long long)b * Ho + oy) * Wo + ox) * a.y_cs + a.y_co + ch] = act_apply(acc[i][r] + bias[i], ACT_SILU);
                }
            }
        }
    }
}

// What a Focus + stem shape runs on, decided ONCE (frlw_det_add_focus_stem keeps the answer in the op): the kernel, its dynamic LDS
// from the kernels' own constexprs, the operand's columns, the accumulator tiles per wavefront and the workgroups a CU holds.
// kern == NULL: no fused kernel takes the shape (Focus and a convolution instead).
using FocusStemFn = void (*)(FocusStemArgs);
struct FocusStemPlan { FocusStemFn kern; size_t lds; int wide, npad, na, per_cu; }; // wide: 0 k_focus_stem, 1 k_focus_stem_wide
constexpr int kFocusStemPatchPix = (8 + 2) * (16 + 2); // PH * PW of the kernels: the halo patch of an 8 x 16 tile, PS = 4 C0 + 4 floats each

template <int C0, int NA, bool WIDE, int P> inline FocusStemPlan focus_stem_plan_p(int npad)
{
    constexpr int wfl = WIDE ? focus_stem_wide_w_floats<C0, P, NA>() : focus_stem_w_floats<C0, P>(); // what the kernel puts in front of its patch
    constexpr size_t lds = ((size_t)wfl + kFocusStemPatchPix * (4 * C0 + 4)) * sizeof(float);
    static_assert(focus_stem_wide_w_floats<C0, P, 1>() == focus_stem_w_floats<C0, P>(), "a 32-column half of the wide kernel = k_focus_stem's operand");
    static_assert(lds <= 160 * 1024, "weights + patch fit the CU's LDS");
    constexpr int per_cu = lds <= 80 * 1024 ? 2 : 1;
    if constexpr (WIDE) return {k_focus_stem_wide<C0, P, NA>, lds, 1, npad, NA, per_cu};
    else return {k_focus_stem<C0, P>, lds, 0, npad, NA, per_cu};
}
template <int C0, int NA, bool WIDE> inline FocusStemPlan focus_stem_plan_of(int prec, int npad)
{
    return prec == 1 ? focus_stem_plan_p<C0, NA, WIDE, 1>(npad) : focus_stem_plan_p<C0, NA, WIDE, 0>(npad);
}

inline FocusStemPlan focus_stem_plan(int C, int Cout, int prec)
{
    if (Cout < 1 || Cout > 64) return {};
    const bool n32 = Cout <= 32; // npad = 32; else 64, as two accumulator tiles (NA = 2) where the whole operand fits beside the patch
    switch (C) {
    case 4: return n32 ? focus_stem_plan_of<4, 1, true>(prec, 32) : focus_stem_plan_of<4, 2, true>(prec, 64);
    case 8: return n32 ? focus_stem_plan_of<8, 1, true>(prec, 32) : focus_stem_plan_of<8, 2, true>(prec, 64);
    case 10: return n32 ? focus_stem_plan_of<10, 1, false>(prec, 32) : focus_stem_plan_of<10, 2, true>(prec, 64);
    case 16:
        if (n32) return focus_stem_plan_of<16, 1, false>(prec, 32);
        // C = 16: the 64-column operand does not fit beside the patch, one half per workgroup.  In the bf16x3 arithmetic that form
        // measured slower than Focus + convolution (batch 32, 256 x 320: 0.356 against 0.349 ms): its shorter MFMA
        // time no longer hides the second read of the input
        if (prec == 1) return {};
        return focus_stem_plan_of<16, 1, true>(prec, 64);
    default: return {};
    }
}

// `a` with x and y bound; persistent workgroups, per_cu on each of the 256 CUs at most (one per 32-column half: `halves` walk a tile).
// The LDS request is unconditional (checked once, for the wide kernels, where the builder can still take the unfused pair: at add).
inline void launch_focus_stem(FocusStemArgs a, const FocusStemPlan &p, int B, hipStream_t s)
{
    a.n_tiles = B * a.tiles_x * a.tiles_y;
    const int halves = p.npad / (32 * p.na), cap = 256 * p.per_cu / halves;
    const int wgs = a.n_tiles < cap ? a.n_tiles : cap;
    (void)hipFuncSetAttribute((const void *)p.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    hipLaunchKernelGGL(p.kern, dim3(wgs * halves), dim3(256), p.lds, s, a);
}
