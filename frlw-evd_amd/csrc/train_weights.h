// train_weights.h -- torch weight (Cout, Cin, k, k) -> the two GEMM operands of the training convolutions, the record of a
// stacked second block and the launcher of one weight's layouts.  Included inside train_ops.hip's anonymous namespace, after
// conv_mfma.h.
//
// fwd[(ky*k + kx)*Cin + ci][co] = w[co][ci][ky][kx];  dgr[((k-1-ky)*k + (k-1-kx))*Cout + co][ci] = w[co][ci][ky][kx]
// One thread per element of the padded forward operand (rows (ky, kx, ci), np_f columns) and of the padded
// data-gradient operand: every element, padding included, is written, so no memset is needed.
// `parity` != 0 (stride-2, k = 3): the data-gradient operand is grouped by output parity class (py, px) in the order
// (0,0) (0,1) (1,0) (1,1) with 1, 2, 2, 4 taps -- row blocks starting at 0, 1, 3, 5 times Cout; inside a class the rows
// are (t_ky, t_kx, co) where tap t reads dz[o' + t] and stands for kernel index 1 (parity 0) or 2, 0 (parity 1, t = 0, 1).
// element (row, col) of the forward (which = 0) or data-gradient (which = 1) operand; zero in the padding (rows past K too)
// (WPair: two BaseConvs stacked along the output channels -- channels >= split come from the second block's weight)
struct WPair { const float *w, *w2; int split; };
__device__ __forceinline__ const float *wpair_of(const WPair &p, int co, int Cin, int kk)
{
    return (p.split > 0 && co >= p.split) ? p.w2 - (long long)p.split * Cin * kk : p.w; // indexed with the stacked co below
}
__device__ __forceinline__ float weight_operand_value(const WPair wp, int Cout, int Cin, int k, int which, int parity, long long row, int col)
{
    const int kk = k * k;
    if (which == 0) {
        const int ci = (int)(row % Cin), tap = (int)(row / Cin);
        return (col < Cout && tap < kk) ? wpair_of(wp, col, Cin, kk)[((long long)col * Cin + ci) * kk + tap] : 0.0f;
    }
    const int co = (int)(row % Cout), tapf = (int)(row / Cout); // tapf = flipped tap index
    if (tapf >= kk || col >= Cin) return 0.0f;
    const float *w = wpair_of(wp, co, Cin, kk);
    int tap = kk - 1 - tapf;
    if (parity) {
        const int cls = tapf < 1 ? 0 : (tapf < 3 ? 1 : (tapf < 5 ? 2 : 3));
        const int tl = tapf - (cls == 0 ? 0 : (cls == 1 ? 1 : (cls == 2 ? 3 : 5)));
        const int py = cls >> 1, px = cls & 1, kwc = px ? 2 : 1;
        const int t_ky = tl / kwc, t_kx = tl - t_ky * kwc;
        const int ky = py ? (t_ky == 0 ? 2 : 0) : 1, kx = px ? (t_kx == 0 ? 2 : 0) : 1;
        tap = ky * 3 + kx;
    }
    return w[((long long)co * Cin + col) * kk + tap];
}

__host__ __device__ inline long long operand_rows(long long K, int prec) { return prec == 1 ? (K + 15) / 16 * 16 : K; }

// float32 operands: one thread per element i of [forward | data gradient]
__device__ __forceinline__ void weight_layout_elem(const WPair w, int Cout, int Cin, int k, float *fwd, int np_f, float *dgr, int np_d,
                                                   int parity, long long nf, long long i)
{
    if (i < nf) fwd[i] = weight_operand_value(w, Cout, Cin, k, 0, 0, i / np_f, (int)(i % np_f));
    else dgr[i - nf] = weight_operand_value(w, Cout, Cin, k, 1, parity, (i - nf) / np_d, (int)((i - nf) % np_d));
}

// split operands (conv_mfma.h, prec = 1): one thread per PAIR of 16-byte records (hi and lo of the same eight values) =
// float-equivalents i .. i + 7 of [forward | data gradient], each operand ceil16(K) rows; i % 8 == 0
__device__ __forceinline__ void weight_layout_record(const WPair w, int Cout, int Cin, int k, float *fwd, int np_f, float *dgr, int np_d,
                                                     int parity, long long nf, long long i)
{
    const int which = i < nf ? 0 : 1;
    const long long r2 = (which ? i - nf : i) >> 3;
    const int np = which ? np_d : np_f;
    const int n = (int)(r2 % np), h = (int)((r2 / np) & 1);
    const long long kt = r2 / (2ll * np);
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) x[q] = weight_operand_value(w, Cout, Cin, k, which, parity, kt * 16 + conv_split_kmem(h, 2 * e + q), n);
        hi[e] = conv_bf16_pair(x[0], x[1]);
        lo[e] = conv_bf16_pair(x[0] - __builtin_bit_cast(float, hi[e] << 16), x[1] - __builtin_bit_cast(float, hi[e] & 0xFFFF0000u));
    }
    uint4 *out = (uint4 *)(which ? dgr : fwd) + ((kt * 2 + h) * 2) * np + n;
    out[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    out[np] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

__global__ void k_weight_layouts(const WPair w, int Cout, int Cin, int k, float *fwd, int np_f, float *dgr, int np_d, int parity, int prec)
{
    const int kk = k * k;
    const long long nf = fwd ? operand_rows((long long)kk * Cin, prec) * np_f : 0, nd = dgr ? operand_rows((long long)kk * Cout, prec) * np_d : 0;
    if (prec == 1) {
        for (long long i = 8 * (blockIdx.x * (long long)blockDim.x + threadIdx.x); i < nf + nd; i += 8ll * gridDim.x * blockDim.x)
            weight_layout_record(w, Cout, Cin, k, fwd, np_f, dgr, np_d, parity, nf, i);
        return;
    }
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nf + nd; i += (long long)gridDim.x * blockDim.x)
        weight_layout_elem(w, Cout, Cin, k, fwd, np_f, dgr, np_d, parity, nf, i);
}

// every weight of a model in one launch: element i belongs to the entry with the largest `first` <= i.  A workgroup walks
// tiles of 2048 consecutive elements and looks the entry of a tile's first element up ONCE (wave-uniform: scalar loads);
// only the elements of a tile that straddles two entries search again.  (Entries with split operands: 512 records per tile.)
__global__ __launch_bounds__(256) void k_weight_layouts_batch(const frlw_weight_layout_item_t *items, int n, long long total)
{
    constexpr int kTile = 2048;
    for (long long base = (long long)blockIdx.x * kTile; base < total; base += (long long)gridDim.x * kTile) {
        int lo = 0, hi = n;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (items[mid].first <= base) lo = mid; else hi = mid;
        }
        const frlw_weight_layout_item_t cur = items[lo];
        const long long next = lo + 1 < n ? items[lo + 1].first : total;
        if (cur.precision == 1 && base + kTile <= next) { // a whole tile of one split entry: one record pair per thread
            const int np_f = (cur.Cout + 31) / 32 * 32, np_d = (cur.Cin + 31) / 32 * 32;
            const long long nf = cur.w_fwd ? operand_rows((long long)cur.k * cur.k * cur.Cin, 1) * np_f : 0;
            weight_layout_record(WPair{cur.w, cur.w2, cur.split}, cur.Cout, cur.Cin, cur.k, cur.w_fwd, np_f, cur.w_dgrad, np_d, (cur.dgrad_parity && cur.k == 3) ? 1 : 0, nf,
                                 base - cur.first + 8 * threadIdx.x);
            continue;
        }
#pragma unroll
        for (int u = 0; u < kTile / 256; ++u) {
            const long long i = base + u * 256 + threadIdx.x;
            if (i >= total) break;
            frlw_weight_layout_item_t it = cur;
            if (i >= next) {
                int j = lo + 1;
                while (j + 1 < n && items[j + 1].first <= i) ++j;
                it = items[j];
            }
            const int np_f = (it.Cout + 31) / 32 * 32, np_d = (it.Cin + 31) / 32 * 32;
            const long long nf = it.w_fwd ? operand_rows((long long)it.k * it.k * it.Cin, it.precision) * np_f : 0;
            const int parity = (it.dgrad_parity && it.k == 3) ? 1 : 0;
            if (it.precision == 1) { // every eighth thread-slot lays a record pair (entries start at multiples of 32 elements)
                if ((i & 7) == 0) weight_layout_record(WPair{it.w, it.w2, it.split}, it.Cout, it.Cin, it.k, it.w_fwd, np_f, it.w_dgrad, np_d, parity, nf, i - it.first);
            } else {
                weight_layout_elem(WPair{it.w, it.w2, it.split}, it.Cout, it.Cin, it.k, it.w_fwd, np_f, it.w_dgrad, np_d, parity, nf, i - it.first);
            }
        }
    }
}

inline int npad32(int n) { return (n + 31) / 32 * 32; }

// precision 1 (split operands) needs the parity classes of the data-gradient operand to start on k-tiles of 16 rows
inline bool precision_ok(int precision, int Cout, int dgrad_parity)
{
    return precision == 0 || (precision == 1 && (!dgrad_parity || Cout % 16 == 0));
}

// The second block of a stacked pair (frlw_baseconv_fuse_t::split > 0) as the host launchers take it; all zero: one block.
// rows / rs: y2 and its row stride in the forward, dy2 and its row stride in the backward.
struct Block2 { int split; const float *w2, *gamma2, *beta2, *rows; long long rs; float *run_mean2, *run_var2; long long *tracked2; };

// need_w2: the call lays the weights out itself; need_run: it updates running statistics
inline int block2_of(const frlw_baseconv_fuse_t *f, int Cout, bool backward, bool need_w2, bool need_run, Block2 &b)
{
    b = Block2{};
    if (!f || f->split == 0) return FRLW_OK;
    const float *rows = backward ? f->dy2 : f->y2;
    if (f->split < 0 || (f->split & 3) || f->split >= Cout || !f->gamma2 || !f->beta2 || !rows || (!backward && f->residual)) return FRLW_ERR_ARG;
    if ((need_w2 && !f->w2) || (need_run && (!f->running_mean2 || !f->running_var2))) return FRLW_ERR_ARG;
    b = Block2{f->split, f->w2, f->gamma2, f->beta2, rows, backward ? f->dy2_row_stride : f->y2_row_stride,
               f->running_mean2, f->running_var2, (long long *)f->num_batches_tracked2};
    return FRLW_OK;
}

inline int launch_weight_layouts(const float *w, const Block2 &b, int Cout, int Cin, int k, int dgrad_parity, float *w_fwd, float *w_dgrad,
                                 int precision, frlw_stream_t stream)
{
    (void)hipGetLastError(); // other libraries in the process (torch's BLAS look-ups) leave stale errors behind
    if (!w || Cout < 1 || Cin < 1 || k < 1 || (!w_fwd && !w_dgrad)) return FRLW_ERR_ARG;
    if (!precision_ok(precision, Cout, dgrad_parity && w_dgrad)) return FRLW_ERR_UNSUPPORTED;
    const long long total = (w_fwd ? frlw_conv_operand_floats(k * k * Cin, Cout, precision) : 0) + (w_dgrad ? frlw_conv_operand_floats(k * k * Cout, Cin, precision) : 0);
    hipLaunchKernelGGL(k_weight_layouts, dim3(conv_grid_1d(precision == 1 ? total / 8 : total)), dim3(256), 0, (hipStream_t)stream, WPair{w, b.w2, b.split}, Cout, Cin, k, w_fwd,
                       npad32(Cout), w_dgrad, npad32(Cin), (dgrad_parity && k == 3) ? 1 : 0, precision);
    TRY_HIP(hipGetLastError());
    return FRLW_OK;
}
