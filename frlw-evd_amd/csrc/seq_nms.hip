// seq_nms.hip -- Seq-NMS (Han et al. 2016) over the detections of whole recordings: link boxes of neighbouring frames, pick the
// best-scoring path again and again, rescore its boxes and cut what it suppresses out of the graph (DESIGN.md "Seq-NMS").
//
//   k_seqnms_link    one wavefront per frame: lane i = box i of frame f against every box of frame f + 1 -> one 64-bit out-edge
//                    mask and the float64 area per box; also seeds the outputs (scores copied, ids and flags 0).
//   k_seqnms_select  one wavefront per recording runs the whole selection loop.  The dynamic programme keeps per box the best
//                    path value (float64) and the chosen successor (uint8) in the workspace and per frame the best root in LDS;
//                    the values of the frame above are read across lanes, and every step's loads are issued a frame ahead.
//                    After a selection only the frames it touched are recomputed, downwards, until a frame below them comes out
//                    unchanged; the result equals a full recompute bit for bit (tests/seqnms_restated.py recomputes everything).
//
// All arithmetic is float64 in the reference's operation order (the unit is built with -ffp-contract=off: area_i + area_j - iw * ih
// stays unfused).  One wavefront per workgroup: no workgroup waits on another, the loop is bounded by max_sequences.
#include "frlw_common.h"

namespace frlw {
namespace {

constexpr int kSeqMaxVideos = FRLW_MAX_SEQUENCES;
constexpr int kSeqMaxFrames = FRLW_SEQ_NMS_MAX_FRAMES;
constexpr int kSeqMaxBoxes = FRLW_SEQ_NMS_MAX_BOXES;
static_assert(kSeqMaxBoxes == 64, "one lane and one mask bit per box of a frame");
static_assert(kSeqMaxVideos <= 64, "the link kernel finds the last frame of a recording with one ballot");

struct SeqWs {
    double *area;         // per box
    uint64_t *mask;       // per box: bit j = edge to box j of the next frame
    double *val;          // per box: best path value from this box onwards
    uint8_t *succ;        // per box: the successor that value goes through (valid where mask != 0)
    int32_t *frame_start; // n_frames_total + 1 box offsets
    int32_t *video_start; // n_videos + 1 frame offsets
};

struct SeqLayout { size_t off[6]; size_t total; };

bool seq_layout(int64_t total_boxes, int64_t n_frames, int n_videos, SeqLayout &L)
{
    if (n_videos < 1 || n_videos > kSeqMaxVideos || n_frames < 0 || n_frames > (int64_t)n_videos * kSeqMaxFrames || total_boxes < 0 ||
        total_boxes > n_frames * kSeqMaxBoxes)
        return false;
    const size_t sizes[6] = {(size_t)total_boxes * 8, (size_t)total_boxes * 8, (size_t)total_boxes * 8, (size_t)total_boxes,
                             (size_t)(n_frames + 1) * 4, (size_t)(n_videos + 1) * 4};
    size_t at = 0;
    for (int i = 0; i < 6; ++i) {
        L.off[i] = at;
        at += (sizes[i] + 255) & ~(size_t)255;
    }
    L.total = at;
    return true;
}

__device__ __forceinline__ int readlane_i32(int v, int lane) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane)); }
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane)
{
    const uint32_t lo = (uint32_t)readlane_i32((int)(uint32_t)v, lane), hi = (uint32_t)readlane_i32((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double readlane_f64(double v, int lane) { return __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(v), lane)); }
__device__ __forceinline__ uint64_t lanes_below(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }
__device__ __forceinline__ int clamp_boxes(int n) { return n < 0 ? 0 : (n > kSeqMaxBoxes ? kSeqMaxBoxes : n); }

// compute_overlap_areas_given for one pair: box a (its area taken from the box) against query box b with the given area.
__device__ __forceinline__ double iou_f64(double ax1, double ay1, double ax2, double ay2, double a_area, double bx1, double by1, double bx2,
                                          double by2, double b_area)
{
    const double iw = (bx2 < ax2 ? bx2 : ax2) - (bx1 > ax1 ? bx1 : ax1);
    if (!(iw > 0)) return 0.0;
    const double ih = (by2 < ay2 ? by2 : ay2) - (by1 > ay1 ? by1 : ay1);
    if (!(ih > 0)) return 0.0;
    const double ua = a_area + b_area - iw * ih;
    return iw * ih / ua;
}

__global__ __launch_bounds__(64) void k_seqnms_link(const float4 *__restrict__ boxes, const double *__restrict__ scores,
                                                    const int32_t *__restrict__ labels, SeqWs ws, int n_videos, double link_thr,
                                                    double *__restrict__ out_scores, int32_t *__restrict__ out_seq,
                                                    uint8_t *__restrict__ out_flags)
{
    __shared__ double nb[5][64];
    __shared__ int32_t nl[64];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int b0 = ws.frame_start[f], b1 = ws.frame_start[f + 1];
    const int n = clamp_boxes(b1 - b0);
    // the last frame of a recording has no out-edges: f + 1 is then the end of some recording
    const bool last = __ballot(lane < n_videos && ws.video_start[lane + 1] == f + 1) != 0;
    const int n2 = last ? 0 : clamp_boxes(ws.frame_start[f + 2] - b1);
    if (lane < n2) {
        const float4 q = boxes[b1 + lane];
        const double x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
        nb[0][lane] = x1; nb[1][lane] = y1; nb[2][lane] = x2; nb[3][lane] = y2;
        nb[4][lane] = (x2 - x1) * (y2 - y1);
        nl[lane] = labels[b1 + lane];
    }
    __syncthreads();
    if (lane < n) {
        const float4 p = boxes[b0 + lane];
        const double x1 = p.x, y1 = p.y, x2 = p.z, y2 = p.w;
        const double area = (x2 - x1) * (y2 - y1);
        const int32_t lab = labels[b0 + lane];
        uint64_t m = 0;
        for (int j = 0; j < n2; ++j) {
            const double o = iou_f64(x1, y1, x2, y2, area, nb[0][j], nb[1][j], nb[2][j], nb[3][j], nb[4][j]);
            if (lab == nl[j] && o >= link_thr) m |= 1ull << j;
        }
        ws.area[b0 + lane] = area;
        ws.mask[b0 + lane] = m;
        out_scores[b0 + lane] = scores[b0 + lane];
        out_seq[b0 + lane] = 0;
        out_flags[b0 + lane] = 0;
    }
}

struct SelArgs {
    const float4 *boxes;
    SeqWs ws;
    double *scores;  // the outputs double as the loop's state: the dynamic programme reads the rescored values
    int32_t *seq;
    uint8_t *flags;
    int32_t *status;
    double nms_thr;
    int metric, skip, max_sequences;
};

struct SelLds {
    double rootval[kSeqMaxFrames];  // per frame: the largest value among its roots (-1: none), first maximum
    uint8_t rootidx[kSeqMaxFrames];
    uint8_t path[kSeqMaxFrames];    // the selected path, frame by frame
    int32_t fs[kSeqMaxFrames + 1];  // the recording's box offsets: every step needs two of them before it can load anything
};

// The first maximum among the lanes of `cand` (ascending lane order, strict >), -1 / lane 0 when there is none.
__device__ __forceinline__ void first_max(uint64_t cand, double v, double &best, int &at)
{
    best = -1.0;
    at = 0;
    for (uint64_t w = cand; w; w &= w - 1) {
        const int j = __ffsll((long long)w) - 1;
        const double x = readlane_f64(v, j);
        if (x > best) { best = x; at = j; }
    }
}

// What a step of the dynamic programme reads of its frame.  Nothing of it depends on the frame above, so the loads of frame f - 1
// are issued before frame f is worked on: a step then costs its arithmetic, not a trip to memory.
struct SweepIn { int b, n; uint64_t m; double sc, oldv; int olds; };
__device__ __forceinline__ SweepIn sweep_load(const SelArgs &a, const int32_t *fs, int f, bool first)
{
    const int lane = threadIdx.x;
    SweepIn r;
    r.b = fs[f];
    r.n = clamp_boxes(fs[f + 1] - r.b);
    r.m = 0; r.sc = 0.0; r.oldv = 0.0; r.olds = 0;
    if (lane < r.n) {
        r.m = a.ws.mask[r.b + lane];
        r.sc = a.scores[r.b + lane];
        if (!first) { r.oldv = a.ws.val[r.b + lane]; r.olds = a.ws.succ[r.b + lane]; }
    }
    return r;
}

// Frames hi .. lo of the dynamic programme, downwards: every frame down to must_lo, then on while a frame still changes.  Refreshes
// the root cache of every frame whose values or in-edges may have changed (hi + 1 included: its in-edges are frame hi's masks).
// The values of the frame above stay in registers (lane j: box j) and are read across lanes.
__device__ __forceinline__ void seq_sweep(const SelArgs &a, const int32_t *fs, int F, int hi, int must_lo, bool first, SelLds &s)
{
    const int lane = threadIdx.x;
    int nnext = 0;
    double vnext = 0.0;
    uint64_t edge_next = 0;
    if (hi + 1 < F) {
        const int b = fs[hi + 1];
        nnext = clamp_boxes(fs[hi + 2] - b);
        uint64_t m = 0;
        if (lane < nnext) { vnext = a.ws.val[b + lane]; m = a.ws.mask[b + lane]; }
        edge_next = __ballot(m != 0);
    }
    // One step: frame f from its loaded inputs; true = the sweep ends here.
    auto step = [&](int f, const SweepIn &in) -> bool {
        const int b = in.b, n = in.n;
        const uint64_t m = in.m;
        double best = -1.0;
        int su = 0;
        uint64_t w = m;
        while (__ballot(w != 0)) {   // every lane takes part in the exchange; ascending j, strict >: np.argmax's first maximum
            const int j = w ? __ffsll((long long)w) - 1 : 0;
            const double x = __shfl(vnext, j);
            if (w && x > best) { best = x; su = j; }
            w &= w - 1;
        }
        const double v = m ? in.sc + best : in.sc;
        const bool changed = lane < n && (first || v != in.oldv || su != in.olds);
        if (changed) { a.ws.val[b + lane] = v; a.ws.succ[b + lane] = (uint8_t)su; }
        const uint64_t has = __ballot(m != 0);
        if (f + 1 < F) {   // the roots of frame f + 1: boxes no box of this frame has an edge to
            uint64_t in_edges = 0;
            for (uint64_t q = has; q; q &= q - 1) in_edges |= readlane_u64(m, __ffsll((long long)q) - 1);
            uint64_t cand = lanes_below(nnext) & ~in_edges;
            if (a.skip) cand &= edge_next;
            double rb; int ri;
            first_max(cand, vnext, rb, ri);
            if (lane == 0) { s.rootval[f + 1] = rb; s.rootidx[f + 1] = (uint8_t)ri; }
        }
        if (f == 0) {      // every box of the first frame is a root
            uint64_t cand = lanes_below(n);
            if (a.skip) cand &= has;
            double rb; int ri;
            first_max(cand, v, rb, ri);
            if (lane == 0) { s.rootval[0] = rb; s.rootidx[0] = (uint8_t)ri; }
        }
        const bool any = __ballot(changed) != 0;
        vnext = v; nnext = n; edge_next = has;
        return f == 0 || (f < must_lo && !any);
    };
    // Two frames per round, each with its own registers: the loads of one are in flight while the other is worked on, and no
    // value has to be copied (and so waited for) where the loop closes.
    SweepIn even = sweep_load(a, fs, hi, first), odd = even;
    for (int f = hi;; f -= 2) {
        if (f > 0) odd = sweep_load(a, fs, f - 1, first);
        if (step(f, even)) break;
        if (f > 1) even = sweep_load(a, fs, f - 2, first);
        if (step(f - 1, odd)) break;
    }
    __syncthreads();   // val / succ and the root cache are read by other lanes from here on
}

// What a step up the selected path reads of its frame (again independent of the step below it: loaded one frame ahead).
struct PathIn { int b, n; float4 p; double ar, sc; uint64_t m; int su; };
__device__ __forceinline__ PathIn path_load(const SelArgs &a, const int32_t *fs, int g)
{
    const int lane = threadIdx.x;
    PathIn r;
    r.b = fs[g];
    r.n = clamp_boxes(fs[g + 1] - r.b);
    r.p = make_float4(0.f, 0.f, 0.f, 0.f);
    r.ar = 0.0; r.sc = 0.0; r.m = 0; r.su = 0;
    if (lane < r.n) {
        r.p = a.boxes[r.b + lane];
        r.ar = a.ws.area[r.b + lane];
        r.m = a.ws.mask[r.b + lane];
        r.su = a.ws.succ[r.b + lane];
        r.sc = a.scores[r.b + lane];
    }
    return r;
}

__global__ __launch_bounds__(64) void k_seqnms_select(SelArgs a)
{
    __shared__ SelLds s;
    const int lane = threadIdx.x, video = blockIdx.x;
    const int fb = a.ws.video_start[video];
    int F = a.ws.video_start[video + 1] - fb;
    F = F > kSeqMaxFrames ? kSeqMaxFrames : F;
    for (int i = lane; i <= F && F > 0; i += 64) s.fs[i] = a.ws.frame_start[fb + i];
    __syncthreads();
    const int32_t *fs = s.fs;
    int status = 0, nsel = 0;
    if (F > 0) seq_sweep(a, fs, F, F - 1, 0, true, s);
    while (F > 0) {
        // ---- the best root: largest value, strict > against 0; ties to the lowest frame (the cache holds the lowest box)
        double bv = 0.0;
        int bf = -1;
        for (int f = lane; f < F; f += 64) {
            const double x = s.rootval[f];
            if (x > bv) { bv = x; bf = f; }
        }
        for (int off = 32; off; off >>= 1) {
            const double ov = __shfl_xor(bv, off);
            const int of = __shfl_xor(bf, off);
            if (of >= 0 && (ov > bv || (ov == bv && (bf < 0 || of < bf)))) { bv = ov; bf = of; }
        }
        bf = __builtin_amdgcn_readfirstlane(bf);
        if (bf < 0) break;
        const double total = readlane_f64(bv, 0);
        int idx = s.rootidx[bf] & 63;
        if (a.ws.mask[fs[bf] + idx] == 0) break;   // a single box is the best "sequence": the reference stops here
        // ---- follow the successors: suppress around every path box, cut the suppressed boxes out of the graph
        int g = bf, len = 0, pb = 0, pn = 0;
        double mx = 0.0;
        uint64_t prevm = 0;   // lane i: the out-edges of box i of frame g - 1
        if (g > 0) {
            pb = fs[g - 1];
            pn = clamp_boxes(fs[g] - pb);
            if (lane < pn) prevm = a.ws.mask[pb + lane];
        }
        PathIn nx = path_load(a, fs, g);
        for (;;) {
            const PathIn in = nx;
            if (g + 1 < F) nx = path_load(a, fs, g + 1);
            const int b = in.b, n = in.n;
            uint64_t m = in.m;
            const double x1 = in.p.x, y1 = in.p.y, x2 = in.p.z, y2 = in.p.w;
            const double qx1 = readlane_f64(x1, idx), qy1 = readlane_f64(y1, idx), qx2 = readlane_f64(x2, idx), qy2 = readlane_f64(y2, idx);
            const double qa = readlane_f64(in.ar, idx), qsc = readlane_f64(in.sc, idx);
            const uint64_t qm = readlane_u64(m, idx);
            const int qs = readlane_i32(in.su, idx) & 63;
            const bool del = lane < n && iou_f64(qx1, qy1, qx2, qy2, qa, x1, y1, x2, y2, in.ar) >= a.nms_thr;
            const uint64_t D = __ballot(del);
            if (del) {
                if (m) a.ws.mask[b + lane] = 0;
                if (lane != idx) a.flags[b + lane] = 1;
                m = 0;
            }
            if (lane < pn && (prevm & D)) {
                prevm &= ~D;
                a.ws.mask[pb + lane] = prevm;
            }
            if (lane == 0) s.path[g] = (uint8_t)idx;
            ++len;
            if (qsc > mx) mx = qsc;
            if (qm == 0 || g + 1 >= F) break;
            prevm = m; pb = b; pn = n;
            idx = qs;
            ++g;
        }
        __syncthreads();
        // ---- rescore the path's boxes
        const double ns = a.metric == 0 ? total / (double)len : mx;
        ++nsel;
        for (int q = bf + lane; q <= g; q += 64) {
            const int k = fs[q] + s.path[q];
            a.scores[k] = ns;
            a.seq[k] = nsel;
        }
        __syncthreads();
        if (nsel >= a.max_sequences) { status |= FRLW_SEQ_NMS_TRUNCATED; break; }
        seq_sweep(a, fs, F, g, bf > 0 ? bf - 1 : 0, false, s);
    }
    if (lane == 0) a.status[video] = status;
}

} // namespace
} // namespace frlw

using namespace frlw;

extern "C" size_t frlw_seq_nms_workspace_bytes(int64_t total_boxes, int64_t n_frames_total, int n_videos)
{
    SeqLayout L;
    return seq_layout(total_boxes, n_frames_total, n_videos, L) ? L.total : 0;
}

extern "C" int frlw_seq_nms(const float *boxes, const double *scores, const int32_t *labels, const int32_t *frame_start,
                            const int32_t *video_frame_start, int n_videos, double link_thr, double nms_thr, int metric, int isolated,
                            int max_sequences, double *out_scores, int32_t *out_seq, uint8_t *out_flags, int32_t *status, void *workspace,
                            size_t workspace_bytes, frlw_stream_t stream)
{
    if (!frame_start || !video_frame_start || !status || n_videos < 1 || n_videos > kSeqMaxVideos || (metric != 0 && metric != 1) ||
        (isolated != 0 && isolated != 1) || max_sequences < 1 || !(link_thr == link_thr) || !(nms_thr <= 1.0))
        return FRLW_ERR_ARG; // nms_thr <= 1: a path's box (IoU 1 with itself) always leaves the graph, so every round makes progress
    // the offsets are HOST arrays: every limit the kernels rely on is checked here, before anything is enqueued
    if (video_frame_start[0] != 0) return FRLW_ERR_ARG;
    for (int v = 0; v < n_videos; ++v) {
        const int64_t d = (int64_t)video_frame_start[v + 1] - video_frame_start[v];
        if (d < 0 || d > kSeqMaxFrames) return FRLW_ERR_ARG;
    }
    const int64_t n_frames = video_frame_start[n_videos];
    if (frame_start[0] != 0) return FRLW_ERR_ARG;
    for (int64_t f = 0; f < n_frames; ++f) {
        const int64_t d = (int64_t)frame_start[f + 1] - frame_start[f];
        if (d < 0 || d > kSeqMaxBoxes) return FRLW_ERR_ARG;
    }
    const int64_t total = frame_start[n_frames];
    if (total > 0 && (!boxes || !scores || !labels || !out_scores || !out_seq || !out_flags || ((uintptr_t)boxes & 15))) return FRLW_ERR_ARG;
    SeqLayout L;
    if (!seq_layout(total, n_frames, n_videos, L)) return FRLW_ERR_ARG;
    if (!workspace || workspace_bytes < L.total || ((uintptr_t)workspace & 7)) return FRLW_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)workspace;
    SeqWs ws;
    ws.area = (double *)(w + L.off[0]);
    ws.mask = (uint64_t *)(w + L.off[1]);
    ws.val = (double *)(w + L.off[2]);
    ws.succ = (uint8_t *)(w + L.off[3]);
    ws.frame_start = (int32_t *)(w + L.off[4]);
    ws.video_start = (int32_t *)(w + L.off[5]);
    (void)hipGetLastError(); // stale errors of other libraries
    HIP_TRY(hipMemcpyAsync(ws.frame_start, frame_start, (size_t)(n_frames + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ws.video_start, video_frame_start, (size_t)(n_videos + 1) * 4, hipMemcpyHostToDevice, st));
    if (n_frames > 0) {
        hipLaunchKernelGGL(k_seqnms_link, dim3((unsigned)n_frames), dim3(64), 0, st, (const float4 *)boxes, scores, labels, ws, n_videos,
                           link_thr, out_scores, out_seq, out_flags);
        HIP_TRY(hipGetLastError());
    }
    SelArgs a{(const float4 *)boxes, ws, out_scores, out_seq, out_flags, status, nms_thr, metric, isolated, max_sequences};
    hipLaunchKernelGGL(k_seqnms_select, dim3((unsigned)n_videos), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}
