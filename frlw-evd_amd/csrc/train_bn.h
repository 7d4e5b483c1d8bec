// train_bn.h -- BatchNorm (batch statistics) + SiLU: the statistics, forward and backward kernels and one host launcher per
// op.  Included inside train_ops.hip's anonymous namespace, after train_wgrad.h.
//
// The tensor is an (M, C) row-major matrix (NHWC), C % 4 == 0.  Reductions over M are two-stage and deterministic:
// a workgroup of 256 threads = C4 = min(C / 4, 256) float4 columns x 256 / C4 row lanes takes bn_rows_per_wg(M) rows (column
// chunks of 1024 channels), every thread keeps float64 sums of its four channels with four rows in flight, the row
// lanes are combined through LDS and the workgroup writes partial[wg][c][2]; a second kernel adds the partials of a
// channel with 16 lanes in parallel.
// rows per workgroup: enough workgroups to fill the chip on the mid-size layers, at most 512 rows
__host__ __device__ inline int bn_rows_per_wg(long long M)
{
    long long r = M / 1024;
    r = (r + 31) / 32 * 32;
    if (r < 32) r = 32;
    if (r > 512) r = 512;
    return (int)r;
}
inline int bn_workgroups(long long M) { return (int)((M + bn_rows_per_wg(M) - 1) / bn_rows_per_wg(M)); }

// f writes the eight terms of a row and float4 column into T[8].  F32_GROUPS: the four rows in flight are added in float32
// before they enter the float64 sums (one conversion and one f64 add per four rows instead of four each; f64 runs at half
// rate on this part).  Used for the backward sums only: the statistics pass squares in float64 (T = double: the square of a
// float32 is exact there) and adds in float64, because its sum of squares minus squared mean cancels.
template <typename T = float, bool F32_GROUPS = false, typename F>
__device__ __forceinline__ void bn_reduce_rows(long long M, int C, double *partial, F f)
{
    __shared__ double red[256][8];
    const int tid = threadIdx.x;
    const int rows = bn_rows_per_wg(M);
    const long long row0 = (long long)blockIdx.x * rows;
    long long row1 = row0 + rows;
    if (row1 > M) row1 = M;
    for (int c0 = 0; c0 < C; c0 += 1024) {
        const int c4n = (C - c0) / 4 < 256 ? (C - c0) / 4 : 256; // float4 columns in this chunk
        const int lanes = 256 / c4n;                              // row lanes (>= 1)
        const int q = tid % c4n, rl = tid / c4n;
        const int c = c0 + 4 * q;
        double acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.0;
        if (rl < lanes) {
            long long r = row0 + rl;
            for (; r + 3ll * lanes < row1; r += 4ll * lanes) { // four independent rows in flight
                T a0[8], a1[8], a2[8], a3[8];
                f(r, c, a0); f(r + lanes, c, a1); f(r + 2ll * lanes, c, a2); f(r + 3ll * lanes, c, a3);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    acc[i] += F32_GROUPS ? (double)((a0[i] + a1[i]) + (a2[i] + a3[i])) : ((double)a0[i] + (double)a1[i]) + ((double)a2[i] + (double)a3[i]);
            }
            for (; r < row1; r += lanes) {
                T a0[8];
                f(r, c, a0);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] += (double)a0[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) red[tid][i] = acc[i];
        __syncthreads();
        if (tid < c4n) {
            for (int l = 1; l < lanes; ++l)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] += red[tid + l * c4n][i];
            double *dst = partial + ((long long)blockIdx.x * C + c) * 2;
#pragma unroll
            for (int j = 0; j < 4; ++j) { dst[2 * j] = acc[j]; dst[2 * j + 1] = acc[4 + j]; }
        }
        __syncthreads();
    }
}

// partial[wg][c] = {sum, sum of squares} in float64 (every term exact)
__global__ __launch_bounds__(256) void k_bn_stats_partial(const float *z, long long M, int C, double *partial)
{
    bn_reduce_rows<double>(M, C, partial, [=](long long r, int c, double (&o)[8]) {
        const float4 v = *(const float4 *)(z + r * C + c);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        o[4] = o[0] * o[0]; o[5] = o[1] * o[1]; o[6] = o[2] * o[2]; o[7] = o[3] * o[3];
    });
}

// adds the partials of kFinCh channels per workgroup, 256 / kFinCh lanes per channel, in a fixed order
// -> tot[c] = {sum a, sum b}.  (16 channels x 16 lanes left 16 workgroups on the chip for a 256-channel layer and took
// 14 us, twice the pass that produced the partials; 4 x 64: C / 4 workgroups, a quarter of the rows per lane.)
constexpr int kFinCh = 4;
__device__ __forceinline__ void bn_sum_partials(const double *partial, int n_wg, int C, double &s0, double &s1, int &c_out)
{
    constexpr int L = 256 / kFinCh;
    __shared__ double red2[256][2];
    const int tid = threadIdx.x, cl = tid % kFinCh, lane = tid / kFinCh;
    const int c = blockIdx.x * kFinCh + cl;
    double a = 0.0, b = 0.0;
    if (c < C) {
        int w = lane;
        for (; w + 3 * L < n_wg; w += 4 * L) { // four independent rows in flight
            const double2 p0 = *(const double2 *)(partial + ((long long)w * C + c) * 2);
            const double2 p1 = *(const double2 *)(partial + ((long long)(w + L) * C + c) * 2);
            const double2 p2 = *(const double2 *)(partial + ((long long)(w + 2 * L) * C + c) * 2);
            const double2 p3 = *(const double2 *)(partial + ((long long)(w + 3 * L) * C + c) * 2);
            a += (p0.x + p1.x) + (p2.x + p3.x);
            b += (p0.y + p1.y) + (p2.y + p3.y);
        }
        for (; w < n_wg; w += L) { a += partial[((long long)w * C + c) * 2]; b += partial[((long long)w * C + c) * 2 + 1]; }
    }
    red2[tid][0] = a;
    red2[tid][1] = b;
    __syncthreads();
    for (int half = L / 2; half >= 1; half >>= 1) { // fixed tree over the lanes of a channel
        if (lane < half) { red2[tid][0] += red2[tid + half * kFinCh][0]; red2[tid][1] += red2[tid + half * kFinCh][1]; }
        __syncthreads();
    }
    s0 = red2[cl][0]; s1 = red2[cl][1]; c_out = (lane == 0 && c < C) ? c : -1;
}

// mean, biased variance, invstd = 1 / sqrt(var + eps) in float32 (what BatchNorm2d normalises with)
// (+ the running statistics of nn.BatchNorm2d when given: momentum update with the unbiased variance)
// The partials are plain float64 {sum, sum of squares} from every producer (k_bn_stats_partial; the convolution epilogues form
// theirs from shifted float32 sums, conv_mfma.h conv_stats_unshift), so the variance E v^2 - mu^2 cancels in float64: a
// channel whose mean is 1000 standard deviations loses 2^-53 * 1e6 of its variance.  M = 1: the variance is 0, and the
// running variance takes it as the unbiased one too (nn.BatchNorm2d refuses such a batch in training).
// (pair: two BaseConvs stacked along the channels -- channels >= split update the second block's running statistics)
struct RunStats2 { float *run_mean2, *run_var2; long long *tracked2; int split; };
__global__ __launch_bounds__(256) void k_bn_stats_final(const double *partial, int n_wg, int C, long long M, float eps,
                                                        float *mean, float *var, float *invstd, float *run_mean,
                                                        float *run_var, float momentum, long long *batches_tracked, RunStats2 pr)
{
    double s, ss;
    int c;
    if (batches_tracked && blockIdx.x == 0 && threadIdx.x == 0) *batches_tracked += 1; // nn.BatchNorm2d.num_batches_tracked
    if (pr.tracked2 && blockIdx.x == 0 && threadIdx.x == 0) *pr.tracked2 += 1;
    bn_sum_partials(partial, n_wg, C, s, ss, c);
    if (c < 0) return;
    const double mu = s / (double)M;
    double v = ss / (double)M - mu * mu;
    if (v < 0.0) v = 0.0;
    mean[c] = (float)mu;
    var[c] = (float)v;
    invstd[c] = (float)(1.0 / sqrt(v + (double)eps));
    if (run_mean) {
        const float unbiased = (float)v * ((float)M / (float)(M > 1 ? M - 1 : 1));
        float *rm = run_mean + c, *rv = run_var + c;
        if (pr.split > 0 && c >= pr.split) { rm = pr.run_mean2 + (c - pr.split); rv = pr.run_var2 + (c - pr.split); }
        *rm = *rm * (1.0f - momentum) + momentum * (float)mu;
        *rv = *rv * (1.0f - momentum) + momentum * unbiased;
    }
}

// sigmoid by the hardware exp2 / reciprocal (~1 ulp each), like the inference epilogue (conv_mfma.h): the exact expf + IEEE
// division are 25 instructions per element and made the backward reduction pass VALU-bound (1.18 ms per step against 0.65 ms of
// traffic); tolerance of the train step against torch is 1e-3, these differ from it by ~1e-7 relative.
__device__ __forceinline__ float sigmoid_fast(float u) { return __frcp_rn(1.0f + __expf(-u)); }
__device__ __forceinline__ float silu_f(float u) { return u * sigmoid_fast(u); }

// Two BaseConvs stacked along the channels (frlw_baseconv_fuse_t::split): channels [0, split) use the first block's gamma / beta
// and rows, channels [split, C) the second block's.  split == 0: one block.  (split % 4 == 0: a float4 never straddles.)
struct Aff2 { const float *g, *b, *g2, *b2; int split; };
__device__ __forceinline__ void aff_of(const Aff2 &a, int c, const float *&g, const float *&b)
{
    const bool second = a.split > 0 && c >= a.split;
    g = second ? a.g2 - a.split : a.g;
    b = second ? a.b2 - a.split : a.b;
}
struct Rows2 { const float *p; long long rs; const float *p2; long long rs2; int split; };
__device__ __forceinline__ const float *row_of(const Rows2 &d, long long r, int c)
{
    return (d.split > 0 && c >= d.split) ? d.p2 + r * d.rs2 + (c - d.split) : d.p + r * d.rs + c;
}

// y = silu(gamma * (z - mean) * invstd + beta) [+ res]
// FUSE: the rows of y and res may be channel slices of wider NHWC tensors (y_rs / res_rs floats between two rows), res may be NULL
template <bool FUSE>
__global__ void k_bn_silu_fwd(const float *z, long long n4, int C, const Aff2 ab, const float *mean,
                              const float *invstd, float *y, long long y_rs, const float *res, long long res_rs, float *y2, long long y2_rs)
{
    const int C4 = C >> 2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        const float4 v = ((const float4 *)z)[i];
        const float *gamma = ab.g, *beta = ab.b;
        if (FUSE) aff_of(ab, c, gamma, beta);
        float4 o;
        o.x = silu_f(gamma[c + 0] * ((v.x - mean[c + 0]) * invstd[c + 0]) + beta[c + 0]);
        o.y = silu_f(gamma[c + 1] * ((v.y - mean[c + 1]) * invstd[c + 1]) + beta[c + 1]);
        o.z = silu_f(gamma[c + 2] * ((v.z - mean[c + 2]) * invstd[c + 2]) + beta[c + 2]);
        o.w = silu_f(gamma[c + 3] * ((v.w - mean[c + 3]) * invstd[c + 3]) + beta[c + 3]);
        if (FUSE) {
            const long long r = i / C4;
            if (res) {
                const float4 rr = *(const float4 *)(res + r * res_rs + c);
                o.x += rr.x; o.y += rr.y; o.z += rr.z; o.w += rr.w;
            }
            if (ab.split > 0 && c >= ab.split) *(float4 *)(y2 + r * y2_rs + (c - ab.split)) = o;
            else *(float4 *)(y + r * y_rs + c) = o;
        } else {
            ((float4 *)y)[i] = o;
        }
    }
}

// du = dy * d silu(u) / du with u = gamma * zhat + beta
__device__ __forceinline__ float dsilu_times(float dy, float u)
{
    const float s = sigmoid_fast(u);
    return dy * (s * (1.0f + u * (1.0f - s)));
}

// partial[wg][c] = {sum du, sum du * zhat} in float64
// (dy_rs: floats between two rows of dy -- C when dense, more when dy is a channel slice of a wider NHWC gradient)
template <bool PAIR>
__global__ __launch_bounds__(256) void k_bn_silu_bwd_partial(const Rows2 dyr, const float *z, long long M, int C,
                                                             const Aff2 ab, const float *mean,
                                                             const float *invstd, double *partial)
{
    bn_reduce_rows<float, true>(M, C, partial, [=](long long r, int c, float (&o)[8]) {
        const float *gamma = ab.g, *beta = ab.b;
        if (PAIR) aff_of(ab, c, gamma, beta);
        const float4 zv = *(const float4 *)(z + r * C + c), gv = *(const float4 *)(PAIR ? row_of(dyr, r, c) : dyr.p + r * dyr.rs + c);
        const float zz[4] = {zv.x, zv.y, zv.z, zv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float zh = (zz[j] - mean[c + j]) * invstd[c + j];
            const float du = dsilu_times(gg[j], gamma[c + j] * zh + beta[c + j]);
            o[j] = du;
            o[4 + j] = du * zh;
        }
    });
}

// dbeta = sum du, dgamma = sum du * zhat (float32 outputs); sums[c] = {dbeta / M, dgamma / M} for the apply pass
__global__ __launch_bounds__(256) void k_bn_silu_bwd_final(const double *partial, int n_wg, int C, long long M,
                                                           float *dgamma, float *dbeta, float *sums)
{
    double s, sz;
    int c;
    bn_sum_partials(partial, n_wg, C, s, sz, c);
    if (c < 0) return;
    dbeta[c] = (float)s;
    dgamma[c] = (float)sz;
    sums[2 * c + 0] = (float)(s / (double)M);
    sums[2 * c + 1] = (float)(sz / (double)M);
}

// dz = gamma * invstd * (du - mean(du) - zhat * mean(du * zhat))
template <bool PAIR>
__global__ void k_bn_silu_bwd_apply(const Rows2 dyr, const float *z, long long n4, int C, const Aff2 ab,
                                    const float *mean, const float *invstd, const float *sums, float *dz)
{
    const int C4 = C >> 2;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        const float4 zv = ((const float4 *)z)[i];
        const float *gamma = ab.g, *beta = ab.b;
        if (PAIR) aff_of(ab, c, gamma, beta);
        const float *dy = dyr.p;
        const long long dy_rs = dyr.rs;
        const float4 gv = PAIR ? *(const float4 *)row_of(dyr, i / C4, c)
                               : (dy_rs == C ? ((const float4 *)dy)[i] : *(const float4 *)(dy + (i / C4) * dy_rs + c));
        const float zz[4] = {zv.x, zv.y, zv.z, zv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g = gamma[c + j], is = invstd[c + j];
            const float zh = (zz[j] - mean[c + j]) * is;
            const float du = dsilu_times(gg[j], g * zh + beta[c + j]);
            o[j] = g * is * (du - sums[2 * (c + j)] - zh * sums[2 * (c + j) + 1]);
        }
        ((float4 *)dz)[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// Which BatchNorm + SiLU form was enqueued (frlw_bn_path_counts, FRLW_BN_PATH_* of frlw_evd.h): host-side relaxed adds, no launch
std::atomic<unsigned long long> g_bn_path_counts[FRLW_BN_PATH_COUNT];
inline void bn_count(int path) { g_bn_path_counts[path].fetch_add(1ull, std::memory_order_relaxed); }

// have_partials > 0: the convolution's epilogue has written that many slabs into scratch.  b2 (Block2 of train_weights.h) with
// split > 0: channels [split, C) update the second block's running statistics when the first block's are given.
inline int launch_bn_stats(const float *z, int64_t M, int C, float eps, float *mean, float *var, float *invstd, double *scratch,
                           float *run_mean, float *run_var, float momentum, long long *batches_tracked, int have_partials,
                           const Block2 &b2, frlw_stream_t stream)
{
    (void)hipGetLastError(); // other libraries in the process (torch's BLAS look-ups) leave stale errors behind
    if (!z || !mean || !var || !invstd || !scratch || M < 1 || C < 4 || (C & 3)) return FRLW_ERR_ARG;
    const int n_wg = have_partials > 0 ? have_partials : bn_workgroups(M);
    hipStream_t s = (hipStream_t)stream;
    if (have_partials <= 0) {
        bn_count(FRLW_BN_PATH_STATS_PASS);
        hipLaunchKernelGGL(k_bn_stats_partial, dim3(n_wg), dim3(256), 0, s, z, (long long)M, C, scratch);
    }
    const RunStats2 pr = run_mean && b2.split > 0 ? RunStats2{b2.run_mean2, b2.run_var2, b2.tracked2, b2.split} : RunStats2{nullptr, nullptr, nullptr, 0};
    hipLaunchKernelGGL(k_bn_stats_final, dim3((C + kFinCh - 1) / kFinCh), dim3(256), 0, s, scratch, n_wg, C, (long long)M, eps, mean,
                       var, invstd, run_mean, run_var, momentum, batches_tracked, pr);
    TRY_HIP(hipGetLastError());
    return FRLW_OK;
}

// b2.split > 0: channels [split, C) are a second block's -- gamma2 / beta2, rows of y2 = b2.rows (b2.rs floats apart; the first
// block's y rows are then `split` wide by default)
inline int launch_bn_silu_fwd(const float *z, int64_t M, int C, const float *gamma, const float *beta, const float *mean,
                              const float *invstd, float *y, int64_t y_rs, const float *res, int64_t res_rs, const Block2 &b2, frlw_stream_t stream)
{
    (void)hipGetLastError(); // other libraries in the process (torch's BLAS look-ups) leave stale errors behind
    if (!z || !y || !gamma || !beta || !mean || !invstd || M < 1 || C < 4 || (C & 3)) return FRLW_ERR_ARG;
    const int c1 = b2.split > 0 ? b2.split : C; // channels of the (first) block
    float *y2 = (float *)b2.rows;
    const long long y2_rs = b2.rs > 0 ? b2.rs : C - c1;
    if (y_rs <= 0) y_rs = c1;
    if (res_rs <= 0) res_rs = C;
    if (y_rs < c1 || (y_rs & 3) || ((uintptr_t)y & 15) || (res && (res_rs < C || (res_rs & 3) || ((uintptr_t)res & 15)))) return FRLW_ERR_ARG;
    if (b2.split > 0 && (y2_rs < C - c1 || (y2_rs & 3) || ((uintptr_t)y2 & 15))) return FRLW_ERR_ARG;
    const long long n4 = (long long)M * C / 4;
    const Aff2 ab = {gamma, beta, b2.gamma2, b2.beta2, b2.split};
    const bool fused = res || y_rs != C || b2.split > 0; // else y_rs == C, res == y2 == NULL, y2_rs == 0
    bn_count(fused ? FRLW_BN_PATH_FWD_FUSED : FRLW_BN_PATH_FWD);
    auto launch = [&](auto F) {
        hipLaunchKernelGGL(k_bn_silu_fwd<decltype(F)::value>, dim3(conv_grid_1d(n4)), dim3(256), 0, (hipStream_t)stream, z, n4, C, ab, mean,
                           invstd, y, (long long)y_rs, res, (long long)(fused ? res_rs : C), y2, y2_rs);
    };
    if (fused) launch(std::true_type{}); else launch(std::false_type{});
    TRY_HIP(hipGetLastError());
    return FRLW_OK;
}

// b2.split > 0: channels [split, C) are a second block's -- gamma2 / beta2, gradient rows dy2 = b2.rows (b2.rs floats apart; dy's
// rows are then `split` wide by default); z, dz, mean, invstd, dgamma, dbeta stay stacked (C wide)
inline int launch_bn_silu_bwd(const float *dy, int64_t dy_row_stride, const float *z, int64_t M, int C, const float *gamma, const float *beta,
                              const float *mean, const float *invstd, float *dz, float *dgamma, float *dbeta, double *scratch,
                              float *sums, const Block2 &b2, frlw_stream_t stream)
{
    (void)hipGetLastError(); // other libraries in the process (torch's BLAS look-ups) leave stale errors behind
    if (!dy || !z || !dz || !dgamma || !dbeta || !scratch || !sums || M < 1 || C < 4 || (C & 3)) return FRLW_ERR_ARG;
    const int c1 = b2.split > 0 ? b2.split : C;
    const long long dy_rs = dy_row_stride > 0 ? dy_row_stride : c1;
    const long long dy2_rs = b2.rs > 0 ? b2.rs : C - c1;
    if (dy_rs < c1 || (dy_rs & 3) || ((uintptr_t)dy & 15)) return FRLW_ERR_ARG;
    if (b2.split > 0 && (dy2_rs < C - c1 || (dy2_rs & 3) || ((uintptr_t)b2.rows & 15))) return FRLW_ERR_ARG;
    const int n_wg = bn_workgroups(M);
    hipStream_t s = (hipStream_t)stream;
    const Aff2 ab = {gamma, beta, b2.gamma2, b2.beta2, b2.split};
    const Rows2 dyr = {dy, dy_rs, b2.rows, dy2_rs, b2.split};
    const long long n4 = (long long)M * C / 4;
    bn_count(b2.split > 0 ? FRLW_BN_PATH_BWD_PAIR : FRLW_BN_PATH_BWD);
    auto launch = [&](auto P) {
        constexpr bool PAIR = decltype(P)::value;
        hipLaunchKernelGGL(k_bn_silu_bwd_partial<PAIR>, dim3(n_wg), dim3(256), 0, s, dyr, z, (long long)M, C, ab, mean, invstd, scratch);
        hipLaunchKernelGGL(k_bn_silu_bwd_final, dim3((C + kFinCh - 1) / kFinCh), dim3(256), 0, s, scratch, n_wg, C, (long long)M, dgamma, dbeta, sums);
        hipLaunchKernelGGL(k_bn_silu_bwd_apply<PAIR>, dim3(conv_grid_1d(n4)), dim3(256), 0, s, dyr, z, n4, C, ab, mean, invstd, sums, dz);
    };
    if (b2.split > 0) launch(std::true_type{}); else launch(std::false_type{});
    TRY_HIP(hipGetLastError());
    return FRLW_OK;
}
