// detector.hip -- the YOLOX / AED detector's eval forward on gfx950 as a plan of launches, built once through the frlw_det_add_*
// entry points and replayed natively by frlw_det_run.  This unit holds the plan (Op, frlw_detector) and the C entry points; the
// kernels and their launchers are the headers below, included inside the anonymous namespace:
//   conv_mfma.h  BaseConv (Conv2d + folded BatchNorm + SiLU) as an implicit GEMM on the matrix cores, both arithmetics -- see there
//   det_focus.h  Focus, fused Focus + stem        det_bfm.h   the BFM stem            det_glue.h  nearest x2 upsample, SPP max-pools
//   det_pred.h   the head's prediction rows       det_nms.h   decode + NMS            mfma_rate.h the MFMA rate self-test
// Activations are NHWC f32 and every tensor may be a channel slice of a wider buffer (pixel stride, channel offset), so torch.cat
// never moves data: producers write straight into the consumer's concat buffer.  Buffers are indices into the table of a run.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <vector>

#include "frlw_evd.h"

namespace {

#include "conv_mfma.h"
#include "det_focus.h"
#include "det_bfm.h"
#include "det_glue.h"
#include "det_nms.h"
#include "det_pred.h"

enum OpType : int { OP_CONV = 0, OP_FOCUS = 1, OP_UPSAMPLE = 2, OP_SPP = 3, OP_DECODE = 4, OP_FORK = 5, OP_JOIN = 6, OP_BFM = 7, OP_PRED = 8, OP_FOCUS_STEM = 9 };
constexpr int kSideLanes = 2; // independent sub-graphs (the head levels) run on side streams

// Payloads of the kinds whose kernels take an argument struct: that struct with its baked fields (the pointers into buffers are
// bound at run time) and the buffers' indices.  FocusOp, BfmOp, UpsampleOp, SppOp: next to their launchers.
struct ConvOp { ConvArgs a; int src, dst, res, ups; }; // ups > 0: the buffer that also receives the output upsampled x2 (ConvArgs::y2); 0 (the network input's index): none
struct FocusStemOp { FocusStemArgs a; FocusStemPlan plan; int src, dst; };
struct PredOp { PredInferArgs a; int src, dst; };
struct DecodeOp { DecodeArgs a; int raw, decoded, dets, counts, ws; };

struct Op {
    int type, lane; // lane: 0 = the caller's stream, 1..kSideLanes = side streams
    union { ConvOp conv; FocusOp focus; UpsampleOp ups; SppOp spp; DecodeOp dec; BfmOp bfm; PredOp pred; FocusStemOp fstem; }; // the one of `type`; fork / join: none
};

struct Bufs { // the buffer table of a run: index -> device pointer, NULL outside the table
    void *const *p; int n;
    float *operator()(int i) const { return (i >= 0 && i < n) ? (float *)p[i] : nullptr; }
};

// The head levels' prediction ops run as ONE launch: ops[i] and the OP_PRED ops that directly follow it inside [i, last) on the same
// lane with the same F, four at most (PredInferMulti).  Binds their buffers into pm; returns the ops taken (>= 1), 0: a NULL buffer.
inline int collect_pred(const std::vector<Op> &ops, int i, int last, const Bufs &buf, PredInferMulti &pm)
{
    int j = i;
    for (; j < last && j - i < 4 && ops[j].type == OP_PRED && ops[j].lane == ops[i].lane && ops[j].pred.a.F == ops[i].pred.a.F; ++j) {
        PredInferArgs &a = pm.lv[j - i] = ops[j].pred.a;
        a.x = buf(ops[j].pred.src); a.out = buf(ops[j].pred.dst);
        if (!a.x || !a.out) return 0;
    }
    return pm.n = j - i;
}

} // namespace

struct frlw_detector {
    std::vector<Op> ops;
    int scratch_buf = -1;        // split-K partial sums: (1 + kSideLanes) regions of scratch_floats
    long long scratch_floats = 0;
    int cur_lane = 0;
    int prec = 0;                // convolution operands added from now on: 0 float32 [K][Npad], 1 the split bf16 image
    // streams and events of the side lanes: made by the first fork or join that RUNS (plans are built on machines without a device),
    // outside any graph capture -- the one thing a run changes in a plan, hence mutable
    mutable bool have_side = false;
    mutable hipStream_t side[kSideLanes] = {};
    mutable hipEvent_t ev_fork = nullptr, ev_join[kSideLanes] = {};

    bool ensure_side() const // false: a HIP error
    {
        if (have_side) return true;
        for (int i = 0; i < kSideLanes; ++i) {
            if (hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking) != hipSuccess) return false;
            if (hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming) != hipSuccess) return false;
        }
        if (hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess) return false;
        return have_side = true;
    }

    // fork: the side streams wait for what the caller's stream holds so far; join: the caller's stream waits for the side streams
    bool fork_or_join(bool fork, hipStream_t s0) const
    {
        if (!ensure_side()) return false;
        if (fork && hipEventRecord(ev_fork, s0) != hipSuccess) return false;
        for (int i = 0; i < kSideLanes; ++i) {
            if (fork) { if (hipStreamWaitEvent(side[i], ev_fork, 0) != hipSuccess) return false; }
            else if (hipEventRecord(ev_join[i], side[i]) != hipSuccess || hipStreamWaitEvent(s0, ev_join[i], 0) != hipSuccess) return false;
        }
        return true;
    }

    // A lane's split-K scratch: region `lane` of the scratch buffer.  All but its last 1024 words hold partial sums; those 1024 are
    // the tiles' arrival counters of the in-kernel reduction (zero when the caller hands the buffer over, reset by the kernel:
    // frlw_det_set_scratch).  No scratch buffer: NULL and 0, no split-K.
    struct LaneScratch { float *partial; long long floats; int *counters; };
    LaneScratch lane_scratch(const Bufs &buf, int lane) const
    {
        float *sc = scratch_buf >= 0 ? buf(scratch_buf) + (long long)lane * scratch_floats : nullptr;
        const long long cap = scratch_buf >= 0 ? scratch_floats - 1024 : 0;
        static const long long sk_knob = dev_knob("FRLW_CONV_SK_INKERNEL", 1ll);
        return {sc, cap > 0 ? cap : 0, (sc && cap > 0 && sk_knob) ? (int *)(sc + cap) : nullptr};
    }

    int add(int type, int lane, const Op &payload = {})
    {
        ops.push_back(payload);
        ops.back().type = type; ops.back().lane = lane;
        return FRLW_OK;
    }
};

#include "mfma_rate.h"

extern "C" {

// iters x 32 MFMAs per wavefront on `blocks` workgroups of 4 wavefronts; `seed`: 256 random floats (device).
int frlw_selftest_mfma_f32_rate(int blocks, int iters, const float *seed, float *sink, frlw_stream_t stream)
{
    int nacc = 4;
    if (blocks < 0) { nacc = (-blocks) % 10; blocks = (-blocks) / 10; } // developer experiments (tools/mfma_rate.py): -(blocks * 10 + accumulators)
    if (blocks < 1 || iters < 1 || !seed || !sink) return FRLW_ERR_ARG;
    if (nacc == 2) hipLaunchKernelGGL(k_mfma_f32_rate<2>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, iters, seed, sink);
    else if (nacc == 1) hipLaunchKernelGGL(k_mfma_f32_rate<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, iters, seed, sink);
    else hipLaunchKernelGGL(k_mfma_f32_rate<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, iters, seed, sink);
    return hipGetLastError() == hipSuccess ? FRLW_OK : FRLW_ERR_HIP;
}

frlw_detector_t *frlw_det_create(void) { return new frlw_detector(); }
void frlw_det_destroy(frlw_detector_t *d)
{
    if (d && d->have_side) {
        for (int i = 0; i < kSideLanes; ++i) { (void)hipStreamDestroy(d->side[i]); (void)hipEventDestroy(d->ev_join[i]); }
        (void)hipEventDestroy(d->ev_fork);
    }
    delete d;
}

int frlw_det_set_lane(frlw_detector_t *d, int lane)
{
    if (!d || lane < 0 || lane > kSideLanes) return FRLW_ERR_ARG;
    d->cur_lane = lane;
    return FRLW_OK;
}

int frlw_det_set_precision(frlw_detector_t *d, int precision)
{
    if (!d || precision < 0 || precision > 1) return FRLW_ERR_ARG;
    d->prec = precision;
    return FRLW_OK;
}

size_t frlw_conv_split_operand_bytes(int K, int Npad)
{
    return K < 1 || Npad < 1 ? 0 : (size_t)((K + 15) / 16) * 4 * (size_t)Npad * 16;
}

int frlw_conv_split_operand(const float *w, int K, int Npad, void *out, frlw_stream_t stream)
{
    (void)hipGetLastError();
    if (!w || !out || K < 1 || Npad < 1) return FRLW_ERR_ARG;
    const long long nrec = (long long)((K + 15) / 16) * 4 * Npad;
    hipLaunchKernelGGL(k_conv_split_operand, dim3(conv_grid_1d(nrec)), dim3(256), 0, (hipStream_t)stream, w, K, Npad, (uint4 *)out);
    return hipGetLastError() == hipSuccess ? FRLW_OK : FRLW_ERR_HIP;
}

int frlw_det_add_fork(frlw_detector_t *d) { return d ? d->add(OP_FORK, 0) : FRLW_ERR_ARG; }
int frlw_det_add_join(frlw_detector_t *d) { return d ? d->add(OP_JOIN, 0) : FRLW_ERR_ARG; }
int frlw_det_num_ops(const frlw_detector_t *d) { return d ? (int)d->ops.size() : 0; }

int frlw_det_set_scratch(frlw_detector_t *d, int buf, int64_t n_floats)
{
    if (!d) return FRLW_ERR_ARG;
    d->scratch_buf = buf; d->scratch_floats = n_floats;
    return FRLW_OK;
}

int frlw_det_add_focus(frlw_detector_t *d, int src_buf, int C, int H, int W, int dst_buf)
{
    if (!d || C < 1 || H < 1 || W < 1 || (H & 1) || (W & 1)) return FRLW_ERR_ARG;
    Op op = {};
    op.focus = FocusOp{src_buf, dst_buf, C, H, W};
    return d->add(OP_FOCUS, d->cur_lane, op);
}

int frlw_focus_nhwc(const float *x, int B, int C, int H, int W, float *y, frlw_stream_t stream)
{
    (void)hipGetLastError();
    if (!x || !y || B < 1 || C < 1 || (H & 1) || (W & 1)) return FRLW_ERR_ARG;
    if (!launch_focus(x, B, C, H, W, y, (hipStream_t)stream)) return FRLW_ERR_UNSUPPORTED;
    return hipGetLastError() == hipSuccess ? FRLW_OK : FRLW_ERR_HIP;
}

int frlw_det_add_focus_stem(frlw_detector_t *d, int src_buf, int C, int H, int W, const float *w_dev, const float *bias_dev,
                            int Cout, int dst_buf, int dst_cs, int dst_co)
{
    if (!d || !w_dev || !bias_dev || (H & 1) || (W & 1) || Cout < 1) return FRLW_ERR_ARG;
    const FocusStemPlan plan = focus_stem_plan(C, Cout, d->prec);
    if (!plan.kern) return FRLW_ERR_UNSUPPORTED; // other stems: frlw_det_add_focus + frlw_det_add_conv
    if (plan.wide) { // the dynamic LDS is asked for HERE, where the builder can still take the unfused pair
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) { // (no device: a plan built for its op list, never run)
            if (hipFuncSetAttribute((const void *)plan.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds) != hipSuccess) {
                (void)hipGetLastError();
                return FRLW_ERR_UNSUPPORTED;
            }
        } else (void)hipGetLastError();
    }
    Op op = {};
    op.fstem = FocusStemOp{{}, plan, src_buf, dst_buf};
    FocusStemArgs &a = op.fstem.a;
    a.H = H; a.W = W; a.w = w_dev; a.bias = bias_dev; a.Cout = Cout; a.y_cs = dst_cs; a.y_co = dst_co;
    a.prec = d->prec; // 1: w_dev is the split image of the (9 * 4 C, npad) operand (frlw_conv_split_operand)
    a.npad = plan.npad;
    a.tiles_x = (W / 2 + 15) / 16; a.tiles_y = (H / 2 + 7) / 8;
    return d->add(OP_FOCUS_STEM, d->cur_lane, op);
}

int frlw_det_bfm_weight_count(int C) { return bfm_weight_count(C); }

int frlw_det_add_bfm_stem(frlw_detector_t *d, int src_buf, int C, int H, int W, const float *weights, int n_weights, int dst_buf)
{
    if (!d || !weights || C < 1 || H < 1 || W < 1 || (H & 1) || (W & 1)) return FRLW_ERR_ARG;
    const int want = bfm_weight_count(C);
    if (want == 0) return FRLW_ERR_UNSUPPORTED; // TAF with K = 2, 4 or 8 FIFO slots
    if (n_weights != want) return FRLW_ERR_ARG;
    Op op = {};
    op.bfm = BfmOp{src_buf, dst_buf, C, H, W, weights};
    return d->add(OP_BFM, d->cur_lane, op);
}

int frlw_det_add_upsample(frlw_detector_t *d, int src_buf, int cs_src, int co_src, int C, int H, int W,
                          int dst_buf, int cs_dst, int co_dst)
{
    if (!d || C < 1 || H < 1 || W < 1) return FRLW_ERR_ARG;
    if (!d->ops.empty() && d->ops.back().type == OP_CONV) {
        // the slice was written by the convolution added just before (the FPN's lateral / reduce 1x1, yolo_pafpn.py:92-100): its
        // epilogue stores the upsampled copy as well -- four more 16-byte stores per output row instead of a launch
        Op &pv = d->ops.back();
        ConvArgs &pc = pv.conv.a;
        if (pv.lane == d->cur_lane && pv.conv.dst == src_buf && pc.y_cs == cs_src && pc.y_co == co_src && pc.Cout == C &&
            pc.Ho == H && pc.Wo == W && pc.y_rp == 0 && pv.conv.ups == 0 && dst_buf > 0 && ((cs_dst | co_dst | C) & 3) == 0) {
            pv.conv.ups = dst_buf;
            pc.y2_cs = cs_dst; pc.y2_co = co_dst; pc.y2_bs = (long long)4 * H * W * cs_dst;
            return FRLW_OK;
        }
    }
    Op op = {};
    op.ups = UpsampleOp{src_buf, dst_buf, C, H, W, cs_src, co_src, cs_dst, co_dst};
    return d->add(OP_UPSAMPLE, d->cur_lane, op);
}

int frlw_det_add_spp_pool(frlw_detector_t *d, int buf, int cs, int C, int H, int W)
{
    if (!d || C < 1 || H < 1 || W < 1 || cs < 4 * C) return FRLW_ERR_ARG;
    if (H * W > kSppMaxPix) return FRLW_ERR_UNSUPPORTED;
    Op op = {};
    op.spp = SppOp{buf, C, H, W, cs};
    return d->add(OP_SPP, d->cur_lane, op);
}

int frlw_det_add_conv(frlw_detector_t *d, int src_buf, int src_cs, int src_co, int Cin, int H, int W,
                      const float *w_dev, const float *bias_dev, int Cout, int Npad, int k, int stride,
                      int dst_buf, int dst_cs, int dst_co, int64_t dst_bs, int res_buf, int res_cs, int res_co,
                      int act, int sig_from, int group_n)
{
    if (!d || !w_dev || (k != 1 && k != 3) || (stride != 1 && stride != 2) || (Cin & 3) || (Npad & 31) ||
        Npad < Cout || (src_cs & 3) || (src_co & 3) || group_n < 0 || (group_n & 127))
        return FRLW_ERR_ARG; // groups: whole 128-column tiles per group
    Op op = {};
    op.conv = ConvOp{{}, src_buf, dst_buf, res_buf, 0};
    ConvArgs &c = op.conv.a; // pointers x / y / res / y2 are bound at run time; w / bias are baked
    c.H = H; c.W = W; c.Cin = Cin; c.x_cs = src_cs; c.x_co = src_co; c.x_bs = (long long)H * W * src_cs;
    c.w = w_dev; c.bias = bias_dev; c.Cout = Cout; c.Npad = Npad; c.k = k; c.stride = stride; c.pad = (k - 1) / 2;
    c.Ho = (H + 2 * c.pad - k) / stride + 1; c.Wo = (W + 2 * c.pad - k) / stride + 1;
    c.y_cs = dst_cs; c.y_co = dst_co; c.y_bs = dst_bs > 0 ? dst_bs : (long long)c.Ho * c.Wo * dst_cs;
    c.r_cs = res_cs; c.r_co = res_co; c.r_bs = (long long)c.Ho * c.Wo * res_cs;
    c.act = act; c.sig_from = sig_from; c.K = k * k * Cin; c.group_n = group_n;
    c.prec = d->prec;
    return d->add(OP_CONV, d->cur_lane, op);
}

int frlw_det_add_pred(frlw_detector_t *d, int src_buf, int src_cs, int src_co, int C, int hw, const float *w_dev,
                      const float *bias_dev, int F, int dst_buf, int first_anchor, int64_t dst_bs)
{
    if (!d || !w_dev || !bias_dev || hw < 1 || F < 6 || dst_bs < 1) return FRLW_ERR_ARG;
    if (C < 4 || (C & 3) || C > 256 || F > 16 || (src_cs & 3) || (src_co & 3)) return FRLW_ERR_UNSUPPORTED;
    Op op = {};
    op.pred = PredOp{{}, src_buf, dst_buf};
    PredInferArgs &a = op.pred.a;
    a.cs = src_cs; a.co = src_co; a.C = C; a.w = w_dev; a.bias = bias_dev; a.F = F; a.hw = hw; a.off = first_anchor; a.out_bs = dst_bs;
    return d->add(OP_PRED, d->cur_lane, op);
}

long long frlw_det_nms_workspace_floats(int A) { return A < 1 ? 0 : nms_ws_floats(A); }

int frlw_det_add_decode_nms(frlw_detector_t *d, int raw_buf, int A, int nc, int n_levels, const int *lvl_h,
                            const int *lvl_w, const int *lvl_stride, float obj_thr, float iou_thr, int decoded_buf,
                            int dets_buf, int counts_buf, int nms_buf)
{
    if (!d || n_levels < 1 || n_levels > 4 || nc < 1 || nc > 80 || A < 1 || nms_buf < 0) return FRLW_ERR_ARG;
    Op op = {};
    op.dec = DecodeOp{{}, raw_buf, decoded_buf, dets_buf, counts_buf, nms_buf};
    DecodeArgs &a = op.dec.a;
    a.A = A; a.nc = nc; a.n_levels = n_levels; a.obj_thr = obj_thr; a.iou_thr = iou_thr;
    for (int i = 0; i < n_levels; ++i) { a.lvl_h[i] = lvl_h[i]; a.lvl_w[i] = lvl_w[i]; a.lvl_stride[i] = lvl_stride[i]; }
    return d->add(OP_DECODE, 0, op); // (always on the caller's stream)
}

// Runs ops [first, last) (last < 0: to the end) for a batch of B images.  bufs[i]: device pointers.  Bind, dispatch, check: the
// launch of every kind is its launcher's.  A plan runs ONE call at a time (the side streams and their events are the plan's).
int frlw_det_run(const frlw_detector_t *d, int B, void *const *bufs, int n_bufs, int first, int last, frlw_stream_t stream)
{
    (void)hipGetLastError(); // stale errors of other libraries in the process
    if (!d || B < 1 || !bufs) return FRLW_ERR_ARG;
    const hipStream_t s0 = (hipStream_t)stream;
    const Bufs buf = {bufs, n_bufs};
    const int n_ops = (int)d->ops.size();
    if (last < 0 || last > n_ops) last = n_ops;
    for (int oi = first, used; oi < last; oi += used) {
        const Op &op = d->ops[oi];
        used = 1; // ops this turn runs: more than one only where prediction levels merge
        if (op.type == OP_FORK || op.type == OP_JOIN) {
            if (!d->fork_or_join(op.type == OP_FORK, s0)) return FRLW_ERR_HIP;
            continue;
        }
        const hipStream_t s = (op.lane > 0 && d->have_side) ? d->side[op.lane - 1] : s0;
        switch (op.type) {
        case OP_FOCUS: {
            const float *x = buf(op.focus.src);
            float *y = buf(op.focus.dst);
            if (!x || !y) return FRLW_ERR_ARG;
            if (!launch_focus(x, B, op.focus.C, op.focus.H, op.focus.W, y, s)) return FRLW_ERR_UNSUPPORTED;
            break;
        }
        case OP_FOCUS_STEM: {
            FocusStemArgs a = op.fstem.a;
            a.x = buf(op.fstem.src); a.y = buf(op.fstem.dst);
            if (!a.x || !a.y) return FRLW_ERR_ARG;
            launch_focus_stem(a, op.fstem.plan, B, s);
            break;
        }
        case OP_BFM: {
            const float *x = buf(op.bfm.src);
            float *y = buf(op.bfm.dst);
            if (!x || !y) return FRLW_ERR_ARG;
            launch_bfm_stem(op.bfm, x, y, B, s);
            break;
        }
        case OP_UPSAMPLE: {
            const float *x = buf(op.ups.src);
            float *y = buf(op.ups.dst);
            if (!x || !y) return FRLW_ERR_ARG;
            launch_upsample2x(op.ups, x, y, B, s);
            break;
        }
        case OP_SPP: {
            float *io = buf(op.spp.buf);
            if (!io) return FRLW_ERR_ARG;
            launch_spp_pool(op.spp, io, B, s);
            break;
        }
        case OP_CONV: {
            ConvArgs c = op.conv.a;
            c.x = buf(op.conv.src); c.y = buf(op.conv.dst); c.res = buf(op.conv.res);
            c.y2 = op.conv.ups > 0 ? buf(op.conv.ups) : nullptr;
            if (!c.x || !c.y || (op.conv.ups > 0 && !c.y2)) return FRLW_ERR_ARG;
            c.M = B * c.Ho * c.Wo;
            const frlw_detector::LaneScratch sc = d->lane_scratch(buf, op.lane);
            if (!launch_conv(c, sc.partial, sc.floats, s, sc.counters)) return FRLW_ERR_UNSUPPORTED;
            break;
        }
        case OP_PRED: {
            PredInferMulti pm = {};
            used = collect_pred(d->ops, oi, last, buf, pm);
            if (used == 0) return FRLW_ERR_ARG;
            launch_pred_infer(pm, B, s);
            break;
        }
        case OP_DECODE: {
            DecodeArgs a = op.dec.a;
            a.raw = buf(op.dec.raw); a.decoded = buf(op.dec.decoded); a.dets = buf(op.dec.dets);
            a.counts = (int *)buf(op.dec.counts); a.ws = buf(op.dec.ws);
            if (!a.raw || !a.dets || !a.counts || !a.ws) return FRLW_ERR_ARG;
            launch_decode_nms(a, B, s);
            break;
        }
        default: return FRLW_ERR_ARG;
        }
    }
    return hipGetLastError() == hipSuccess ? FRLW_OK : FRLW_ERR_HIP;
}

} // extern "C"
