// coco_eval.hip -- COCO bounding-box mAP (pycocotools COCOeval, iouType 'bbox', default params, no crowd) on the GPU.
//
// Replaces what evaluate/src/metrics/coco_eval.py:89-113 (_coco_eval) asks of pycocotools: COCOeval.evaluate() and
// .accumulate() -> eval['precision'] (T=10, R=101, K, A=4, M=3) and eval['recall'] (T, K, A, M).  The host
// (frlw-evd_amd/coco_eval.py) windows the boxes, drops rows whose category is outside the label map and packs the windows
// ("images") as CSR arrays; the 12 summary numbers are means of the two small arrays, taken on the host.
//
//   1. match     one wavefront per (image, category): rank the image's detections of the category by score (stable),
//                keep 100, IoU matrix in double in LDS (recomputed from global memory when it does not fit), then one
//                greedy walk per (IoU threshold, area range) = 40 lanes; the outcome of detection d is two 40-bit
//                ballots (tp, fp; neither = ignored), written to the detection's slot.  Per (category, area) the count
//                of non-ignored ground truths goes to an integer atomic.
//   2. sort      a stable LSD radix sort of the slots: 8 byte passes over an order-preserving key of the score
//                (descending), then one pass over the category.  Slots are laid out image by image and, inside an
//                image, by rank, so ties keep (image, rank) order -- np.argsort(-scores, kind='mergesort') over the
//                concatenation of the images.  maxDets 1 / 10 are the same order filtered by rank < maxDet.
//   3. accumulate  per (IoU threshold, category, area, maxDets): the running tp / fp counts of that order (tile counts,
//                a scan over tiles, then a walk of each tile).  The precision envelope at recall threshold r is the max
//                of tp / ((fp + tp) + eps) over the true positives whose recall tp / npig reaches rec_thrs[r]: every
//                true positive drops its precision into the bucket of the highest threshold it reaches (integer max on
//                the bits of a non-negative double) and a suffix max over the 101 buckets gives the envelope.
//
// Every count is an integer and every double is computed by one thread from integers and the inputs, in the reference's
// operation order (-ffp-contract=off): the result does not depend on scheduling, and equals pycocotools' bit for bit.

#include <utility>

#include "frlw_common.h"

using namespace frlw;

namespace {

constexpr int kT = 10, kR = 101, kA = 4, kM = 3;
constexpr int kWalks = kT * kA;          // lane = area * 10 + threshold
constexpr int kCombos = kWalks * kM;     // q = maxdet * 40 + area * 10 + threshold
constexpr int kMaxDet = 100;
constexpr int kIouLds = 4096;            // doubles of the LDS IoU matrix (32 KB): 100 detections x 40 ground truths
constexpr int kGLds = 128;               // ground truths of one (image, category) that the LDS path holds
constexpr int kSortTile = 2048;
constexpr int kAccTile = 1024;
constexpr uint8_t kNoCat = 0xFF;         // slot without a kept detection: sorts after every category

__constant__ double kAreaLo[kA] = {0.0, 0.0, 1024.0, 9216.0};
__constant__ double kAreaHi[kA] = {1e10, 1024.0, 9216.0, 1e10};
__constant__ int kMaxDets[kM] = {1, 10, 100};

struct CocoIn {
    const double *gt_box, *gt_area; const int32_t *gt_cls; const int64_t *gt_off;
    const double *dt_box, *dt_area, *dt_score; const int32_t *dt_cls; const int64_t *dt_off;
    int n_img, n_cls;
    const double *iou_thrs, *rec_thrs;
};

struct Ws {
    uint64_t *key, *key2, *tpm, *fpm, *bucket;
    uint32_t *idx, *idx2, *hist, *htot, *cnt, *ctot, *base;
    uint8_t *cat, *rank, *gtm;
    int32_t *npig, *kept;
    long long n_stiles, n_atiles;
};

// np.argsort(-score, kind='mergesort') order as an unsigned key: larger score first, -0 == +0, NaN last.
__device__ __forceinline__ uint64_t score_key(double s)
{
    if (s != s) return ~0ull;
    if (s == 0.0) s = 0.0;
    uint64_t u = (uint64_t)__double_as_longlong(s);
    u = (u >> 63) ? ~u : (u | (1ull << 63));
    return ~u;
}

// pycocotools maskApi.c bbIou, no crowd: boxes [x, y, w, h].
__device__ __forceinline__ double box_iou(const double *d, const double *g)
{
    const double w = fmin(d[2] + d[0], g[2] + g[0]) - fmax(d[0], g[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(d[3] + d[1], g[3] + g[1]) - fmax(d[1], g[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = d[2] * d[3] + g[2] * g[3] - i;
    return i / u;
}

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// Stage 1.  Block = one wavefront = one (image, category).
__global__ __launch_bounds__(64) void k_coco_match(CocoIn in, Ws ws)
{
    __shared__ double s_iou[kIouLds];
    __shared__ double s_g[kGLds][5];   // x, y, w, h, area
    __shared__ double s_d[kMaxDet][5];
    __shared__ int s_dsel[kMaxDet];
    __shared__ int s_gsel[kGLds];
    __shared__ uint32_t s_gm[kGLds / 32][64]; // matched ground truths of lane's walk (LDS path)

    const int i = blockIdx.x / in.n_cls, k = blockIdx.x % in.n_cls, lane = threadIdx.x;
    const long long d0 = in.dt_off[i], d1 = in.dt_off[i + 1], g0 = in.gt_off[i], g1 = in.gt_off[i + 1];

    int nd_k = 0, nd_before = 0;
    for (long long b = d0; b < d1; b += 64) {
        const long long j = b + lane;
        const int c = j < d1 ? in.dt_cls[j] : -1;
        nd_k += __popcll(__ballot(c == k));
        nd_before += __popcll(__ballot(c >= 0 && c < k));
    }
    int ng = 0;
    for (long long b = g0; b < g1; b += 64) {
        const long long j = b + lane;
        const bool mine = j < g1 && in.gt_cls[j] == k;
        const uint64_t bal = __ballot(mine);
        if (mine) {
            const int p = ng + __popcll(bal & lanes_below(lane));
            if (p < kGLds) s_gsel[p] = (int)(j - g0);
        }
        ng += __popcll(bal);
    }
    if (nd_k == 0 && ng == 0) return; // evaluateImg -> None

    // npig: ground truths of this category inside each area range
    for (int a = 0; a < kA; ++a) {
        int n_in = 0;
        for (long long b = g0; b < g1; b += 64) {
            const long long j = b + lane;
            bool inr = false;
            if (j < g1 && in.gt_cls[j] == k) {
                const double ar = in.gt_area[j];
                inr = !(ar < kAreaLo[a] || ar > kAreaHi[a]);
            }
            n_in += __popcll(__ballot(inr));
        }
        if (lane == 0 && n_in) atomicAdd(&ws.npig[k * kA + a], n_in);
    }

    // stable rank by score of the category's detections; the first 100 are kept
    for (long long j = d0 + lane; j < d1; j += 64) {
        if (in.dt_cls[j] != k) continue;
        const uint64_t kj = score_key(in.dt_score[j]);
        int r = 0;
        for (long long j2 = d0; j2 < d1 && r < kMaxDet; ++j2) {
            if (in.dt_cls[j2] != k) continue;
            const uint64_t k2 = score_key(in.dt_score[j2]);
            r += (k2 < kj) || (k2 == kj && j2 < j);
        }
        if (r < kMaxDet) s_dsel[r] = (int)(j - d0);
    }
    const int nd = nd_k < kMaxDet ? nd_k : kMaxDet;
    if (lane == 0 && nd) atomicAdd(&ws.kept[k], nd);
    __syncthreads();

    const long long slot0 = d0 + nd_before; // this (image, category)'s slots: d0 + #detections of lower categories + rank
    for (int r = lane; r < nd; r += 64) {
        const long long j = d0 + s_dsel[r];
        for (int c = 0; c < 4; ++c) s_d[r][c] = in.dt_box[j * 4 + c];
        s_d[r][4] = in.dt_area[j];
        ws.key[slot0 + r] = score_key(in.dt_score[j]);
        ws.cat[slot0 + r] = (uint8_t)k;
        ws.rank[slot0 + r] = (uint8_t)r;
    }
    const bool lds = ng <= kGLds && nd * ng <= kIouLds;
    if (lds) {
        for (int g = lane; g < ng; g += 64) {
            const long long j = g0 + s_gsel[g];
            for (int c = 0; c < 4; ++c) s_g[g][c] = in.gt_box[j * 4 + c];
            s_g[g][4] = in.gt_area[j];
        }
        for (int w = 0; w < kGLds / 32; ++w) s_gm[w][lane] = 0u;
    } else if (lane < kWalks) {
        for (long long j = g0; j < g1; ++j)
            if (in.gt_cls[j] == k) ws.gtm[j * kWalks + lane] = 0;
    }
    __syncthreads();
    if (lds) {
        for (int e = lane; e < nd * ng; e += 64) s_iou[e] = box_iou(s_d[e / ng], s_g[e % ng]);
        __syncthreads();
    }

    // COCOeval.evaluateImg: for each detection in score order, the best still-unmatched ground truth with IoU >= the
    // threshold (ties: the later one), non-ignored ground truths first; ignored ones only when no non-ignored matched.
    const bool walking = lane < kWalks;
    const int ta = lane % kT, ar = lane / kT;
    const double thr = walking ? fmin(in.iou_thrs[ta], 1.0 - 1e-10) : 0.0;
    const double lo = kAreaLo[walking ? ar : 0], hi = kAreaHi[walking ? ar : 0];
    for (int d = 0; d < nd; ++d) {
        int state = 0; // 0 ignored, 1 tp, 2 fp
        if (walking) {
            double best = thr;
            int m = -1;
            bool m_ig = false;
            long long mj = -1;
            if (lds) {
                for (int pass = 0; pass < 2 && m < 0; ++pass)
                    for (int g = 0; g < ng; ++g) {
                        const bool ig = s_g[g][4] < lo || s_g[g][4] > hi;
                        if (ig != (pass == 1) || ((s_gm[g >> 5][lane] >> (g & 31)) & 1u)) continue;
                        const double v = s_iou[d * ng + g];
                        if (v < best) continue;
                        best = v; m = g; m_ig = ig;
                    }
                if (m >= 0) s_gm[m >> 5][lane] |= 1u << (m & 31);
            } else {
                for (int pass = 0; pass < 2 && m < 0; ++pass)
                    for (long long j = g0; j < g1; ++j) {
                        if (in.gt_cls[j] != k) continue;
                        const double ga = in.gt_area[j];
                        const bool ig = ga < lo || ga > hi;
                        if (ig != (pass == 1) || ws.gtm[j * kWalks + lane]) continue;
                        const double v = box_iou(s_d[d], in.gt_box + j * 4);
                        if (v < best) continue;
                        best = v; m = 0; mj = j; m_ig = ig;
                    }
                if (m >= 0) ws.gtm[mj * kWalks + lane] = 1;
            }
            if (m >= 0) state = m_ig ? 0 : 1;
            else state = (s_d[d][4] < lo || s_d[d][4] > hi) ? 0 : 2;
        }
        const uint64_t tp = __ballot(state == 1), fp = __ballot(state == 2);
        if (lane == 0) {
            ws.tpm[slot0 + d] = tp;
            ws.fpm[slot0 + d] = fp;
        }
    }
}

__global__ void k_iota(uint32_t *idx, long long n)
{
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x)
        idx[j] = (uint32_t)j;
}

__device__ __forceinline__ int sort_digit(const uint64_t *key, const uint32_t *idx, const uint8_t *cat, long long j, int pass)
{
    return pass < 8 ? (int)((key[j] >> (8 * pass)) & 255u) : (int)cat[idx[j]];
}

// Stage 2, per pass: digit histogram of each tile -> hist[digit][tile].
__global__ __launch_bounds__(256) void k_sort_hist(const uint64_t *key, const uint32_t *idx, const uint8_t *cat, long long n,
                                                   int pass, uint32_t *hist, long long n_tiles)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long t0 = blockIdx.x * (long long)kSortTile;
    for (int e = threadIdx.x; e < kSortTile && t0 + e < n; e += 256) atomicAdd(&h[sort_digit(key, idx, cat, t0 + e, pass)], 1u);
    __syncthreads();
    hist[threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}


// Inclusive scan of one value per thread of a 256-thread block; *total = the sum of all 256.
__device__ __forceinline__ uint32_t block_scan_256(uint32_t *s, uint32_t v, uint32_t *total)
{
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const uint32_t add = t >= o ? s[t - o] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const uint32_t r = s[t];
    *total = s[255];
    __syncthreads();
    return r;
}

// Exclusive scan of each row rows[blockIdx.x][0:n_cols] in place; totals[row] = the row's sum.
__global__ __launch_bounds__(256) void k_scan_rows(uint32_t *rows, long long n_cols, uint32_t *totals)
{
    __shared__ uint32_t s[256];
    uint32_t *row = rows + blockIdx.x * n_cols;
    uint32_t run = 0;
    for (long long b = 0; b < n_cols; b += 256) {
        const long long c = b + threadIdx.x;
        const uint32_t v = c < n_cols ? row[c] : 0u;
        uint32_t tot;
        const uint32_t inc = block_scan_256(s, v, &tot);
        if (c < n_cols) row[c] = run + inc - v;
        run += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = run;
}

// Stage 2, per pass: stable scatter of a tile.  Thread d moves the tile's records of digit d, in tile order.
__global__ __launch_bounds__(256) void k_sort_scatter(const uint64_t *key, const uint32_t *idx, const uint8_t *cat, long long n,
                                                      int pass, const uint32_t *hist, const uint32_t *htot, long long n_tiles,
                                                      uint64_t *key_out, uint32_t *idx_out)
{
    __shared__ uint32_t s[256];
    __shared__ uint8_t s_dig[kSortTile];
    __shared__ uint64_t s_key[kSortTile];
    __shared__ uint32_t s_idx[kSortTile];
    const int d = threadIdx.x;
    uint32_t tot;
    const uint32_t digit_base = block_scan_256(s, htot[d], &tot) - htot[d];
    const long long t0 = blockIdx.x * (long long)kSortTile;
    const int cnt = (int)(n - t0 < kSortTile ? n - t0 : kSortTile);
    for (int e = threadIdx.x; e < cnt; e += 256) {
        s_dig[e] = (uint8_t)sort_digit(key, idx, cat, t0 + e, pass);
        s_key[e] = key[t0 + e];
        s_idx[e] = idx[t0 + e];
    }
    __syncthreads();
    long long pos = (long long)digit_base + hist[d * n_tiles + blockIdx.x];
    for (int e = 0; e < cnt; ++e) {
        if (s_dig[e] != d) continue;
        if (key_out) key_out[pos] = s_key[e];
        idx_out[pos] = s_idx[e];
        ++pos;
    }
}

// Stage 3 helpers: the sorted records of a tile into LDS.
struct AccTile {
    uint64_t tp[kAccTile], fp[kAccTile];
    uint8_t cat[kAccTile], rank[kAccTile];
};

__device__ __forceinline__ int load_acc_tile(AccTile &s, const Ws &ws, const uint32_t *order, long long n, long long t0)
{
    const int cnt = (int)(n - t0 < kAccTile ? n - t0 : kAccTile);
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
        const uint32_t j = order[t0 + e];
        s.cat[e] = ws.cat[j];
        s.rank[e] = ws.rank[j];
        s.tp[e] = ws.tpm[j];
        s.fp[e] = ws.fpm[j];
    }
    __syncthreads();
    return cnt;
}

// tp / fp counts of combination q over the tile -> cnt[2q (+1)][tile].  Holes (kNoCat) sort last and count as nothing.
__global__ __launch_bounds__(128) void k_acc_count(Ws ws, const uint32_t *order, long long n)
{
    __shared__ AccTile s;
    const int cnt = load_acc_tile(s, ws, order, n, blockIdx.x * (long long)kAccTile);
    const int q = threadIdx.x;
    if (q >= kCombos) return;
    const int bit = q % kWalks, maxdet = kMaxDets[q / kWalks];
    uint32_t tp = 0, fp = 0;
    for (int e = 0; e < cnt; ++e) {
        if (s.cat[e] == kNoCat || s.rank[e] >= maxdet) continue;
        tp += (uint32_t)(s.tp[e] >> bit) & 1u;
        fp += (uint32_t)(s.fp[e] >> bit) & 1u;
    }
    ws.cnt[(2 * q) * ws.n_atiles + blockIdx.x] = tp;
    ws.cnt[(2 * q + 1) * ws.n_atiles + blockIdx.x] = fp;
}

// base[b][2q (+1)] = tp / fp count of combination q before the first record of category b (b = n_cls: the end).
__global__ __launch_bounds__(128) void k_acc_base(Ws ws, const uint32_t *order, int n_cls)
{
    const int b = blockIdx.x, q = threadIdx.x;
    if (q >= kCombos) return;
    long long p = 0;
    for (int k = 0; k < b; ++k) p += ws.kept[k];
    const long long tile = p / kAccTile;
    uint32_t tp, fp;
    if (tile >= ws.n_atiles) {
        tp = ws.ctot[2 * q];
        fp = ws.ctot[2 * q + 1];
    } else {
        tp = ws.cnt[(2 * q) * ws.n_atiles + tile];
        fp = ws.cnt[(2 * q + 1) * ws.n_atiles + tile];
        const int bit = q % kWalks, maxdet = kMaxDets[q / kWalks];
        for (long long e = tile * kAccTile; e < p; ++e) {
            const uint32_t j = order[e];
            if (ws.rank[j] >= maxdet) continue;
            tp += (uint32_t)(ws.tpm[j] >> bit) & 1u;
            fp += (uint32_t)(ws.fpm[j] >> bit) & 1u;
        }
    }
    ws.base[b * 2 * kCombos + 2 * q] = tp;
    ws.base[b * 2 * kCombos + 2 * q + 1] = fp;
}

// Highest r with rec_thrs[r] <= rc (rc >= 0 = rec_thrs[0]).
__device__ __forceinline__ int recall_bucket(const double *rt, double rc)
{
    int lo = 0, hi = kR; // rt[lo] <= rc < rt[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rt[mid] <= rc) lo = mid; else hi = mid;
    }
    return lo;
}

// Walk of a tile per combination: each true positive's precision into its recall bucket.
__global__ __launch_bounds__(128) void k_acc_walk(Ws ws, const uint32_t *order, long long n, const double *rec_thrs)
{
    __shared__ AccTile s;
    __shared__ double s_rt[kR];
    for (int r = threadIdx.x; r < kR; r += blockDim.x) s_rt[r] = rec_thrs[r];
    const int cnt = load_acc_tile(s, ws, order, n, blockIdx.x * (long long)kAccTile);
    const int q = threadIdx.x;
    if (q >= kCombos) return;
    const int bit = q % kWalks, a = (q % kWalks) / kT, maxdet = kMaxDets[q / kWalks];
    uint32_t tp = ws.cnt[(2 * q) * ws.n_atiles + blockIdx.x], fp = ws.cnt[(2 * q + 1) * ws.n_atiles + blockIdx.x];
    int cur = -1;          // bucket index (k * kCombos + q) * kR + r being maximised
    uint64_t cur_max = 0;
    for (int e = 0; e < cnt; ++e) {
        const int k = s.cat[e];
        if (k == kNoCat) break;
        if (s.rank[e] >= maxdet) continue;
        const uint32_t is_tp = (uint32_t)(s.tp[e] >> bit) & 1u, is_fp = (uint32_t)(s.fp[e] >> bit) & 1u;
        if (is_tp) {
            const int npig = ws.npig[k * kA + a];
            if (npig > 0) {
                const double c = (double)(tp + 1 - ws.base[k * 2 * kCombos + 2 * q]);
                const double f = (double)(fp - ws.base[k * 2 * kCombos + 2 * q + 1]);
                const double pr = c / ((f + c) + 2.220446049250313e-16);
                const double rc = c / (double)npig;
                const int bkt = (k * kCombos + q) * kR + recall_bucket(s_rt, rc);
                const uint64_t bits = (uint64_t)__double_as_longlong(pr);
                if (bkt != cur) {
                    if (cur >= 0) atomicMax((unsigned long long *)&ws.bucket[cur], (unsigned long long)cur_max);
                    cur = bkt;
                    cur_max = bits;
                } else if (bits > cur_max) {
                    cur_max = bits;
                }
            }
        }
        tp += is_tp;
        fp += is_fp;
    }
    if (cur >= 0) atomicMax((unsigned long long *)&ws.bucket[cur], (unsigned long long)cur_max);
}

// precision[t][r][k][a][m], recall[t][k][a][m]: -1 without non-ignored ground truth, else the suffix max of the buckets.
__global__ void k_acc_final(Ws ws, int n_cls, double *precision, double *recall)
{
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= kT * n_cls * kA * kM) return;
    const int m = id % kM, a = (id / kM) % kA, k = (id / (kM * kA)) % n_cls, t = id / (kM * kA * n_cls);
    const int q = m * kWalks + a * kT + t;
    const int npig = ws.npig[k * kA + a];
    const long long col = ((long long)k * kA + a) * kM + m, rstride = (long long)n_cls * kA * kM;
    double *prec = precision + (long long)t * kR * rstride + col;
    if (npig == 0) {
        recall[(long long)t * rstride + col] = -1.0;
        for (int r = 0; r < kR; ++r) prec[r * rstride] = -1.0;
        return;
    }
    const uint32_t tp_total = ws.base[(k + 1) * 2 * kCombos + 2 * q] - ws.base[k * 2 * kCombos + 2 * q];
    recall[(long long)t * rstride + col] = ws.kept[k] > 0 ? (double)tp_total / (double)npig : 0.0;
    uint64_t env = 0;
    for (int r = kR - 1; r >= 0; --r) {
        const uint64_t b = ws.bucket[((long long)k * kCombos + q) * kR + r];
        if (b > env) env = b;
        prec[r * rstride] = __longlong_as_double((long long)env);
    }
}

struct Layout {
    size_t off[16];
    size_t total;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// key, key2, tpm, fpm, bucket, idx, idx2, hist, htot, cnt, ctot, base, cat, rank, gtm, npig+kept
bool coco_layout(long long n_img, long long n_gt, long long n_dt, int n_cls, Layout &L)
{
    if (n_img < 0 || n_gt < 0 || n_dt < 0 || n_cls < 1 || n_cls >= kNoCat || n_dt >= (1ll << 31) || n_img >= (1ll << 31) / n_cls)
        return false;
    const long long st = (n_dt + kSortTile - 1) / kSortTile, at = (n_dt + kAccTile - 1) / kAccTile;
    const size_t sz[16] = {(size_t)n_dt * 8, (size_t)n_dt * 8, (size_t)n_dt * 8, (size_t)n_dt * 8,
                           (size_t)n_cls * kCombos * kR * 8, (size_t)n_dt * 4, (size_t)n_dt * 4, (size_t)st * 256 * 4, 256 * 4,
                           (size_t)at * 2 * kCombos * 4, 2 * kCombos * 4, (size_t)(n_cls + 1) * 2 * kCombos * 4,
                           (size_t)n_dt, (size_t)n_dt, (size_t)n_gt * kWalks, (size_t)n_cls * (kA + 1) * 4};
    size_t o = 0;
    for (int s = 0; s < 16; ++s) {
        L.off[s] = o;
        o += align256(sz[s]);
    }
    L.total = o;
    return true;
}

} // namespace

extern "C" int64_t frlw_coco_workspace_bytes(int64_t n_img, int64_t n_gt, int64_t n_dt, int n_cls)
{
    Layout L;
    return coco_layout(n_img, n_gt, n_dt, n_cls, L) ? (int64_t)L.total : 0;
}

extern "C" int frlw_coco_eval(const double *gt_box, const double *gt_area, const int32_t *gt_cls, const int64_t *gt_off, int64_t n_gt,
                              const double *dt_box, const double *dt_area, const double *dt_score, const int32_t *dt_cls,
                              const int64_t *dt_off, int64_t n_dt, int n_img, int n_cls, const double *iou_thrs,
                              const double *rec_thrs, void *workspace, int64_t workspace_bytes, double *precision,
                              double *recall, frlw_stream_t stream)
{
    Layout L;
    if (!coco_layout(n_img, n_gt, n_dt, n_cls, L) || !gt_off || !dt_off || !iou_thrs || !rec_thrs || !precision || !recall ||
        (n_gt > 0 && (!gt_box || !gt_area || !gt_cls)) || (n_dt > 0 && (!dt_box || !dt_area || !dt_score || !dt_cls)))
        return FRLW_ERR_ARG;
    if (!workspace || workspace_bytes < (int64_t)L.total) return FRLW_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)workspace;
    Ws ws;
    ws.key = (uint64_t *)(w + L.off[0]); ws.key2 = (uint64_t *)(w + L.off[1]);
    ws.tpm = (uint64_t *)(w + L.off[2]); ws.fpm = (uint64_t *)(w + L.off[3]); ws.bucket = (uint64_t *)(w + L.off[4]);
    ws.idx = (uint32_t *)(w + L.off[5]); ws.idx2 = (uint32_t *)(w + L.off[6]); ws.hist = (uint32_t *)(w + L.off[7]);
    ws.htot = (uint32_t *)(w + L.off[8]); ws.cnt = (uint32_t *)(w + L.off[9]); ws.ctot = (uint32_t *)(w + L.off[10]);
    ws.base = (uint32_t *)(w + L.off[11]);
    ws.cat = (uint8_t *)(w + L.off[12]); ws.rank = (uint8_t *)(w + L.off[13]); ws.gtm = (uint8_t *)(w + L.off[14]);
    ws.npig = (int32_t *)(w + L.off[15]); ws.kept = ws.npig + n_cls * kA;
    ws.n_stiles = (n_dt + kSortTile - 1) / kSortTile;
    ws.n_atiles = (n_dt + kAccTile - 1) / kAccTile;
    CocoIn in{gt_box, gt_area, gt_cls, gt_off, dt_box, dt_area, dt_score, dt_cls, dt_off, n_img, n_cls, iou_thrs, rec_thrs};

    (void)hipGetLastError(); // stale errors of other libraries
    HIP_TRY(hipMemsetAsync(ws.npig, 0, (size_t)n_cls * (kA + 1) * 4, st));
    HIP_TRY(hipMemsetAsync(ws.bucket, 0, (size_t)n_cls * kCombos * kR * 8, st));
    HIP_TRY(hipMemsetAsync(ws.base, 0, (size_t)(n_cls + 1) * 2 * kCombos * 4, st));
    HIP_TRY(hipMemsetAsync(ws.ctot, 0, 2 * kCombos * 4, st));
    if (n_dt > 0) {
        HIP_TRY(hipMemsetAsync(ws.cat, kNoCat, (size_t)n_dt, st));
        HIP_TRY(hipMemsetAsync(ws.key, 0, (size_t)n_dt * 8, st));
    }
    if (n_img > 0) {
        hipLaunchKernelGGL(k_coco_match, dim3((unsigned)(n_img * n_cls)), dim3(64), 0, st, in, ws);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t *order = ws.idx;
    if (n_dt > 0) {
        hipLaunchKernelGGL(k_iota, dim3(grid_for(n_dt, 256)), dim3(256), 0, st, ws.idx, (long long)n_dt);
        HIP_TRY(hipGetLastError());
        uint64_t *ka = ws.key, *kb = ws.key2;
        uint32_t *ia = ws.idx, *ib = ws.idx2;
        for (int pass = 0; pass < 9; ++pass) {
            hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)ws.n_stiles), dim3(256), 0, st, ka, ia, ws.cat, (long long)n_dt, pass,
                               ws.hist, ws.n_stiles);
            hipLaunchKernelGGL(k_scan_rows, dim3(256), dim3(256), 0, st, ws.hist, ws.n_stiles, ws.htot);
            hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)ws.n_stiles), dim3(256), 0, st, ka, ia, ws.cat, (long long)n_dt, pass,
                               ws.hist, ws.htot, ws.n_stiles, pass < 8 ? kb : (uint64_t *)nullptr, ib);
            HIP_TRY(hipGetLastError());
            std::swap(ka, kb);
            std::swap(ia, ib);
        }
        order = ia;
        hipLaunchKernelGGL(k_acc_count, dim3((unsigned)ws.n_atiles), dim3(128), 0, st, ws, order, (long long)n_dt);
        hipLaunchKernelGGL(k_scan_rows, dim3(2 * kCombos), dim3(256), 0, st, ws.cnt, ws.n_atiles, ws.ctot);
        hipLaunchKernelGGL(k_acc_base, dim3((unsigned)(n_cls + 1)), dim3(128), 0, st, ws, order, n_cls);
        hipLaunchKernelGGL(k_acc_walk, dim3((unsigned)ws.n_atiles), dim3(128), 0, st, ws, order, (long long)n_dt, rec_thrs);
        HIP_TRY(hipGetLastError());
    }
    const int n_out = kT * n_cls * kA * kM;
    hipLaunchKernelGGL(k_acc_final, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, ws, n_cls, precision, recall);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}
