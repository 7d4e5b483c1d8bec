// det_nms.h -- decode + NMS of the head tensor (yolo_head.py:258-303).  Included inside detector.hip's anonymous namespace, after det_focus.h.

// Three launches so that the quadratic part runs on the whole GPU (round 6; one workgroup per image did everything before:
// 32 or 8 of 256 CUs, a third of the forward's time on top of it):
//   k_decode_sort  one workgroup per image: decode, candidates obj > thr compacted in anchor order, sorted by score
//                  (descending, ties by anchor index = a stable sort); the order and the sorted xyxy boxes go to the workspace
//   k_nms_matrix   (image, 64-row block, 64-column word) wavefronts over the upper triangle: bit j of mask[row i][word] =
//                  "box i suppresses box j" = j > i and IoU(i, j) > thr -- every CU computes IoUs
//   k_nms_sweep    one small workgroup per image walks the rows in score order on 64-bit masks (thread t owns word t of the
//                  `removed` set; a chunk of 64 rows is resolved by the owner of its diagonal word, its kept rows are OR-ed
//                  into the later words; the next chunk's masks are in flight meanwhile); the kept bits go to the workspace
//   k_nms_emit     (image, 256 candidates) workgroups write the kept boxes in score order.
// Same comparison everywhere: inter / (area_i + area_j - inter) > thr on xyxy corners without + 1, f32, this operation order.
struct DecodeArgs {
    const float *raw; // (B, A, 5 + nc): [reg 4, sigmoid(obj), sigmoid(cls)...]
    int A, nc, n_levels;
    int lvl_h[4], lvl_w[4], lvl_stride[4];
    float obj_thr, iou_thr;
    float *decoded;   // optional (B, A, 5 + nc): boxes decoded, rest copied
    float *dets;      // (B, A, 6): [cx, cy, w, h, argmax cls, obj * max cls] in descending-score order
    int *counts;      // (B, 1 + A): detections per image (0 = the reference's single all-zero row), then the score order
    float *ws;        // (B, nms_ws_floats(A)): per image [n, pad x3 | kept bits u64 x 128 | sorted boxes float4 x A64 | mask u64 [A64][A64 / 64]]
};

constexpr int NMS_MAX = 8192; // candidates per image the device NMS holds (1 Mpx detector shape: 6720 anchors)
constexpr int kNmsHdr = 4 + 2 * (NMS_MAX / 64); // floats in front of the boxes: n, pad x3, the kept bits of k_nms_sweep
__host__ __device__ inline int nms_a64(int A) { return A < NMS_MAX ? (A + 63) / 64 * 64 : NMS_MAX; } // candidates <= min(A, NMS_MAX)
__host__ __device__ inline long long nms_ws_floats(int A)
{
    const long long a64 = nms_a64(A);
    return kNmsHdr + 4 * a64 + 2 * (a64 / 64) * a64;
}
// LDS of k_decode_sort (dynamic): the sort keys, skey[n] f32 | sidx[n] i32, n = candidates rounded up to a power of two.
__host__ __device__ inline size_t nms_lds_bytes(int cap) { return (size_t)cap * 8 + 64; }

__device__ __forceinline__ void nms_anchor_box(const DecodeArgs &a, int b, int i, float &cx, float &cy, float &w, float &h)
{
    int lvl = 0, off = i;
    while (lvl + 1 < a.n_levels && off >= a.lvl_h[lvl] * a.lvl_w[lvl]) { off -= a.lvl_h[lvl] * a.lvl_w[lvl]; ++lvl; }
    const float gx = (float)(off % a.lvl_w[lvl]), gy = (float)(off / a.lvl_w[lvl]), s = (float)a.lvl_stride[lvl];
    const float *r = a.raw + ((long long)b * a.A + i) * (5 + a.nc);
    cx = (r[0] + gx) * s;      // (xy + grid) * stride, yolo_head.py:271
    cy = (r[1] + gy) * s;
    w = (r[2] * r[2]) * s;     // square(wh) * stride, :272
    h = (r[3] * r[3]) * s;
}

__global__ __launch_bounds__(1024) void k_decode_sort(DecodeArgs a, int cap)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
    float *skey = (float *)nms_lds;
    int *sidx = (int *)(skey + cap);
    __shared__ int scount;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int F = 5 + a.nc;
    int *count_out = a.counts + (long long)b * (1 + a.A);
    int *order = count_out + 1; // anchor index of every candidate in score order
    float *wsb = a.ws + (long long)b * nms_ws_floats(a.A);
    int *n_out = (int *)wsb;
    float4 *boxes = (float4 *)(wsb + kNmsHdr);
    if (tid == 0) scount = 0;
    __syncthreads();
    // ---- decode; candidates = obj > threshold, compacted in anchor order by a block-wide stable scan
    // (sort stability must not depend on thread timing): do it in chunks of nt anchors
    for (int base = 0; base < a.A; base += nt) {
        const int i = base + tid;
        bool cand = false;
        float obj = 0;
        if (i < a.A) {
            const float *r = a.raw + ((long long)b * a.A + i) * F;
            obj = r[4];
            cand = obj > a.obj_thr;    // :276
            if (a.decoded) {
                float cx, cy, w, h;
                nms_anchor_box(a, b, i, cx, cy, w, h);
                float *d = a.decoded + ((long long)b * a.A + i) * F;
                d[0] = cx; d[1] = cy; d[2] = w; d[3] = h;
                for (int c = 4; c < F; ++c) d[c] = r[c];
            }
        }
        // stable compaction inside the chunk: rank = number of candidates with a smaller thread id
        const unsigned long long bal = __ballot(cand);
        __shared__ int wcount[16];
        const int lane = tid & 63, wv = tid >> 6;
        if (lane == 0) wcount[wv] = __popcll(bal);
        __syncthreads();
        int pre = scount;
        for (int k = 0; k < wv; ++k) pre += wcount[k];
        const int slot = pre + __popcll(bal & ((1ull << lane) - 1ull));
        if (cand && slot < cap) { skey[slot] = obj; sidx[slot] = i; }
        __syncthreads();
        if (tid == 0) { int t = scount; for (int k = 0; k < (nt + 63) / 64; ++k) t += wcount[k]; scount = t; }
        __syncthreads();
    }
    if (scount > cap) { if (tid == 0) { *count_out = -1; *n_out = -1; } return; } // more candidates than the LDS holds (A > 8192 only)
    const int n = scount;
    if (tid == 0) *n_out = n;
    if (n == 0) { if (tid == 0) *count_out = 0; return; }
    // ---- sort candidates by score descending, ties by anchor index ascending (= a stable sort):
    // bitonic network over the next power of two, keys (score, -index); one compare-exchange per thread and step
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    for (int i = n + tid; i < np2; i += nt) { skey[i] = -INFINITY; sidx[i] = 0x7fffffff; }
    __syncthreads();
    for (int size = 2; size <= np2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = tid; p < (np2 >> 1); p += nt) {
                const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1)), j = i | stride;
                const bool up = (i & size) == 0; // descending blocks first
                const float ki = skey[i], kj = skey[j];
                const int ii = sidx[i], ij = sidx[j];
                const bool i_first = ki > kj || (ki == kj && ii < ij); // i should precede j in the final order
                if (up ? !i_first : i_first) { skey[i] = kj; skey[j] = ki; sidx[i] = ij; sidx[j] = ii; }
            }
            __syncthreads();
        }
    }
    // ---- the order and the sorted corner boxes leave for the workspace (x1, y1, x2, y2 as :280 forms them)
    for (int i = tid; i < n; i += nt) {
        const int anchor = sidx[i];
        order[i] = anchor;
        float cx, cy, w, h;
        nms_anchor_box(a, b, anchor, cx, cy, w, h);
        boxes[i] = make_float4(cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2);
    }
}

// grid (words / 4, row blocks, B), 4 wavefronts per workgroup: wavefront = one 64 x 64 block of the suppression matrix.
__global__ __launch_bounds__(256) void k_nms_matrix(DecodeArgs a)
{
    const int b = blockIdx.z, rb = blockIdx.y, lane = threadIdx.x & 63, cw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long a64 = nms_a64(a.A);
    float *wsb = a.ws + (long long)b * nms_ws_floats(a.A);
    const int n = *(const int *)wsb;
    if (n <= 0 || cw < rb || rb * 64 >= n || cw * 64 >= n) return; // (wave-uniform; no barrier in this kernel)
    const float4 *boxes = (const float4 *)(wsb + kNmsHdr);
    unsigned long long *mask = (unsigned long long *)(wsb + kNmsHdr + 4 * a64);
    const int gi = rb * 64 + lane, gj = cw * 64 + lane;
    const float4 rbx = gi < n ? boxes[gi] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 cbx = gj < n ? boxes[gj] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float r_area = (rbx.z - rbx.x) * (rbx.w - rbx.y), c_area = (cbx.z - cbx.x) * (cbx.w - cbx.y);
    const bool thr_nonneg = a.iou_thr >= 0.0f;
    unsigned long long mine = 0ull;
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
        const float x1 = __shfl(rbx.x, i), y1 = __shfl(rbx.y, i), x2 = __shfl(rbx.z, i), y2 = __shfl(rbx.w, i), ai = __shfl(r_area, i);
        const float xx1 = fmaxf(x1, cbx.x), yy1 = fmaxf(y1, cbx.y);
        const float xx2 = fminf(x2, cbx.z), yy2 = fminf(y2, cbx.w);
        const float iw = fmaxf(xx2 - xx1, 0.0f), ih = fmaxf(yy2 - yy1, 0.0f);
        const float inter = iw * ih;
        const bool pair = rb * 64 + i < gj && gj < n && rb * 64 + i < n;
        unsigned long long bal = 0ull;
        // no overlap anywhere in this row of the block: 0 / x is 0 or NaN, never > thr (thr >= 0) -- the division is skipped
        if (!thr_nonneg || __ballot(pair && inter > 0.0f) != 0ull)
            bal = __ballot(pair && inter / (ai + c_area - inter) > a.iou_thr);
        if (lane == i) mine = bal;
    }
    mask[(long long)gi * (a64 / 64) + cw] = mine; // rows at or behind n: zero (one scattered 8-byte store per 64 x 64 IoUs)
}

constexpr int kSweepThreads = 128; // = NMS_MAX / 64 words
__global__ __launch_bounds__(kSweepThreads) void k_nms_sweep(DecodeArgs a)
{
    __shared__ unsigned long long keptw[kSweepThreads];
    const int b = blockIdx.x, t = threadIdx.x;
    const long long a64 = nms_a64(a.A);
    const int nw = (int)(a64 / 64);
    float *wsb = a.ws + (long long)b * nms_ws_floats(a.A);
    const int n = *(const int *)wsb;
    if (n <= 0) return; // (k_decode_sort has written the count: 0 or -1)
    const int nwn = (n + 63) >> 6;
    // row-major mask: the 64 lanes of a wavefront read 64 consecutive words of one row (thread t = word t)
    const unsigned long long *col = (const unsigned long long *)(wsb + kNmsHdr + 4 * a64) + t;
    const bool active = t < nwn;
    unsigned long long rem = 0ull;
    unsigned long long bufA[64], bufB[64];
    auto load = [&](unsigned long long (&m)[64], int c) {
        if (active && t >= c) {
            const unsigned long long *src = col + (long long)c * 64 * nw;
#pragma unroll
            for (int i = 0; i < 64; ++i) m[i] = src[(long long)i * nw];
        }
    };
    auto step = [&](unsigned long long (&cur)[64], unsigned long long (&nxt)[64], int c) {
        if (c + 1 < nwn) load(nxt, c + 1); // the next chunk's masks fly while this one is resolved
        const int nb = n - c * 64 < 64 ? n - c * 64 : 64;
        if (t == c) { // the owner of the diagonal word: the chunk's 64 rows in score order
            unsigned long long sup = rem, kept = 0ull;
            unsigned long long any = 0ull;
#pragma unroll
            for (int i = 0; i < 64; ++i) any |= cur[i];
            const unsigned long long valid = nb == 64 ? ~0ull : (1ull << nb) - 1ull;
            if ((any & valid) == 0ull) kept = ~sup & valid; // nobody inside the chunk suppresses anybody
            else {
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    const bool keep = i < nb && !((sup >> i) & 1ull);
                    kept |= keep ? 1ull << i : 0ull;
                    sup |= keep ? cur[i] : 0ull;
                }
            }
            keptw[c] = kept;
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // (LDS only: the prefetch above stays in flight)
        const unsigned long long kept = keptw[c];
        if (active && t > c) {
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                if ((kept >> (8 * g)) & 0xffull) { // wave-uniform
#pragma unroll
                    for (int i = 8 * g; i < 8 * g + 8; ++i) rem |= ((kept >> i) & 1ull) ? cur[i] : 0ull;
                }
            }
        }
    };
    load(bufA, 0);
    for (int c = 0; c < nwn; c += 2) {
        step(bufA, bufB, c);
        if (c + 1 < nwn) step(bufB, bufA, c + 1);
    }
    __syncthreads();
    unsigned long long *kept_out = (unsigned long long *)(wsb + 4);
    if (t < nwn) kept_out[t] = keptw[t];
}

// kept boxes -> dets rows in score order: output row = kept boxes in front.  grid (ceil(A64 / 256), B)
__global__ __launch_bounds__(256) void k_nms_emit(DecodeArgs a)
{
    __shared__ int wpre[NMS_MAX / 64 + 1];
    const int b = blockIdx.y, t = threadIdx.x;
    const int F = 5 + a.nc;
    float *wsb = a.ws + (long long)b * nms_ws_floats(a.A);
    const int n = *(const int *)wsb;
    if (n <= 0 || (int)blockIdx.x * 256 >= n) return;
    const unsigned long long *keptw = (const unsigned long long *)(wsb + 4);
    int *count_out = a.counts + (long long)b * (1 + a.A);
    const int *order = count_out + 1;
    const int nwn = (n + 63) >> 6;
    // kept boxes in front of every word: wavefront 0 scans the <= 128 popcounts (two per lane)
    if (t < 64) {
        const int c0 = 2 * t < nwn ? __popcll(keptw[2 * t]) : 0, c1 = 2 * t + 1 < nwn ? __popcll(keptw[2 * t + 1]) : 0;
        int inc = c0 + c1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(inc, off);
            if (t >= off) inc += v;
        }
        const int ex = inc - c0 - c1;
        if (2 * t < nwn) wpre[2 * t] = ex;
        if (2 * t + 1 < nwn) wpre[2 * t + 1] = ex + c0;
        if (t == 63) wpre[nwn] = inc; // all kept boxes
    }
    __syncthreads();
    if (blockIdx.x == 0 && t == 0) *count_out = wpre[nwn];
    const int i = blockIdx.x * 256 + t;
    if (i >= n) return;
    const unsigned long long kw = keptw[i >> 6];
    if (!((kw >> (i & 63)) & 1ull)) return;
    const int row = wpre[i >> 6] + __popcll(kw & ((1ull << (i & 63)) - 1ull));
    const int anchor = order[i];
    const float *r = a.raw + ((long long)b * a.A + anchor) * F;
    int best = 0;
    float bv = r[5];
    for (int c = 1; c < a.nc; ++c) if (r[5 + c] > bv) { bv = r[5 + c]; best = c; } // first max, like argmax
    float *d = a.dets + ((long long)b * a.A + row) * 6;
    nms_anchor_box(a, b, anchor, d[0], d[1], d[2], d[3]);
    d[4] = (float)best;
    d[5] = r[4] * bv; // obj * max cls, yolo_head.py:301
}

// the four launches, `a` with its pointers bound
inline void launch_decode_nms(const DecodeArgs &a, int B, hipStream_t s)
{
    int cap = 1024; // LDS sized for the anchors of this network, up to NMS_MAX candidates
    while (cap < a.A && cap < NMS_MAX) cap <<= 1;
    launch_lds(k_decode_sort, dim3(B), dim3(1024), nms_lds_bytes(cap), s, a, cap);
    const int words = nms_a64(a.A) / 64; // candidates never exceed min(A, NMS_MAX)
    hipLaunchKernelGGL(k_nms_matrix, dim3((words + 3) / 4, words, B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_nms_sweep, dim3(B), dim3(kSweepThreads), 0, s, a);
    hipLaunchKernelGGL(k_nms_emit, dim3(words * 64 / 256 + 1, B), dim3(256), 0, s, a);
}
