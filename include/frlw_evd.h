/*
 * frlw_evd.h -- C-ABI of the MI355X-native FRLW-EvD hot path (libfrlw_evd.so, gfx950 only).
 *
 * The reference (HarmoniaLeo/FRLW-EvD) has no FFI on this path: its boundary is a set of Python
 * functions that take a device tensor of events and return fresh device tensors.  Each entry point
 * below replaces the body of one of those functions; the Python shims in frlw-evd_amd/ keep the
 * reference's names and argument meaning and call these through ctypes (INTEGRATION.md shows
 * the binding).  Citations are file:line in the reference tree.
 *
 * Conventions
 *   - every pointer except frlw_events_t itself, `lamdas` and `status_out` is DEVICE memory
 *     owned by the caller; nothing is allocated, retained or freed by the library;
 *   - calls are asynchronous on `stream` (a hipStream_t; NULL = the default stream),
 *     re-entrant (no globals) and contain no host synchronisation, so they can be captured
 *     into a hipGraph;
 *   - scratch comes from an explicit workspace: query frlw_encoder_workspace_bytes(), pass
 *     a device buffer of at least that size; one workspace per in-flight call;
 *   - return value: FRLW_OK or a negative FRLW_ERR_* for errors detectable at launch time.
 *     Data-dependent errors (coordinate out of range = the IndexError torch raises in
 *     index_add_, generate_eventvolume.py:32) are recorded in the workspace and read back
 *     with frlw_encoder_status(), which synchronises the stream.  After such an error the
 *     outputs are unspecified but no out-of-bounds access has happened.
 */
#ifndef FRLW_EVD_H
#define FRLW_EVD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *frlw_stream_t; /* hipStream_t */

enum {
    FRLW_OK = 0,
    FRLW_ERR_ARG = -1,       /* bad argument (NULL pointer, non-positive shape, ...) */
    FRLW_ERR_INDEX = -2,     /* event coordinate outside the encode shape (torch: IndexError) */
    FRLW_ERR_WORKSPACE = -3, /* workspace too small */
    FRLW_ERR_HIP = -4,       /* a HIP runtime call failed */
    FRLW_ERR_POLARITY = -5,  /* polarity outside {0, 1} */
    FRLW_ERR_UNSUPPORTED = -6,
    FRLW_ERR_SPAN = -7       /* frlw_taf_encode_batch: an event outside [t_start, t_start + n_windows * window_us] */
};

/* Event array layouts. */
enum {
    /* (N, row_stride) float64 rows [x, y, t, p, ...]: the tensor the reference functions take
     * (generate_eventvolume.py:135, generate_taf.py:195,203).  x, y, p are truncated toward
     * zero like .long(); t is used as the harness left it (already normalised / absolute). */
    FRLW_LAYOUT_XYTP_F64 = 0,
    /* raw 8-byte Prophesee DAT Event2D records: t:u32, then x = w & 16383,
     * y = (w >> 14) & 16383, p = (w >> 28) & 1 (src/io/dat_events_tools.py:16,96-98).
     * The window selection / f64 time normalisation the reference harness does on the host
     * tensor (generate_taf.py:197-215, generate_eventvolume.py:139-141) then runs on device. */
    FRLW_LAYOUT_DAT8 = 1
};

/* Optional per-call overrides of the launch heuristics (experiments, and tests that force a rarely taken path).
 * Every field: < 0 = the library's choice.  There is no process-wide state: the knobs travel with the call.
 * `struct_size` = sizeof(frlw_tuning_t) as the CALLER compiled it: the struct has grown and will grow at its end, and the
 * library reads only the fields that lie inside `struct_size` (the others take their defaults), so a caller built against
 * an older header never has its stack read past the struct.  A struct_size below 8 or above 4096 is FRLW_ERR_ARG. */
typedef struct frlw_tuning {
    int32_t struct_size;     /* = sizeof(frlw_tuning_t) */
    int32_t tile_width_log2; /* 6..8 */
    int32_t batches_per_wave; /* 1..8: 64-event batches per wavefront of a partition workgroup */
    int32_t hot_tile_records; /* a tile with more records than this is shared by several workgroups (EV / TAF) */
    int32_t staged_scatter;   /* 0 / 1: records leave the partition through an LDS staging area */
    int32_t quarter_below;    /* frames with at most this many wavefronts run every tile as four quarter workgroups */
    int32_t no_value_table;   /* 1: TAF DAT8 computes the f64 division per event instead of the per-call table */
    int32_t taf_tile_walk;    /* RETIRED (the slot keeps the struct's layout): once selected an opt-in second-level split that was
                               * measured slower and has been removed.  0 / 1 / -1 are accepted and ignored. */
    int32_t direct_bins;      /* frlw_taf_encode_batch / frlw_ev_encode_batch: 1 = the partition's bins are the 256-cell sub-tiles
                               * wherever the frame allows it (at most 64 tiles: the 304x240 class) -- no second-level split pass
                               * at all; 0 = always tile bins + split pass; default: sub-tile bins for calls with fewer than 512
                               * (sequence, tile) pairs and more than 8192 events per pair on average */
    int32_t chunk_major;      /* frlw_taf_encode_batch / frlw_ev_encode_batch: 1 = the chunk-major partition (no histogram pass: the
                               * scatter writes every chunk sorted by bin where it stands plus a directory row, the consumers
                               * gather -- the default wherever a sequence has at most 4096 chunks), 0 = histogram + scans +
                               * bin-major scatter (the only form for longer sequences) */
    int32_t ev_lds_float_atomics; /* frlw_ev_encode_batch, direct mode of the chunk-major partition: 1 = one wavefront per sub-tile
                               * sums its list with LDS float atomics in stream order (kf_ev_fadd: short latency chain, 3 x the
                               * cycles per record -- the default up to 3 M events per call), 0 = the ticket-sort kernel */
    int32_t walk_window_table; /* frlw_taf_encode_batch, chunk-major partition with tile bins: 1 = the split kernel leaves every
                               * sub-tile list's window starts in a table and the walk reads them (the default), 0 = the walk
                               * finds them with a scan of its list, as it does for every other partition form */
} frlw_tuning_t;

typedef struct frlw_events {
    const void *data;  /* device pointer to the event array */
    int64_t n;         /* number of events */
    int32_t layout;    /* FRLW_LAYOUT_* */
    int32_t row_stride; /* XYTP_F64: doubles per row (>= 4); ignored for DAT8 */
    /* Optional coordinate maps for DAT8 (device, uint16): x <- xmap[x], y <- ymap[y].  They carry
     * the harness' down-scale `x * rw, y * rh` + truncation (generate_taf.py:216-219); NULL =
     * identity.  map_w / map_h = table lengths (the sensor width / height). */
    const uint16_t *xmap;
    const uint16_t *ymap;
    int32_t map_w;
    int32_t map_h;
    const frlw_tuning_t *tuning; /* HOST pointer or NULL */
} frlw_events_t;

#define FRLW_MAX_WINDOWS 64
#define FRLW_MAX_LAMDAS 8
#define FRLW_MAX_BINS 8 /* Event Volume bins and TAF K: register-resident per cell */

/* frlw_taf_encode flags */
#define FRLW_TAF_U8_FLIP_K 1 /* write out_u8 newest slot first (np.flip(axis=0), generate_taf.py:229) */

/* Bytes of device workspace any encoder needs for `n_events` events on an H x W encode shape: the larger of the general
 * plan and of the two-launch form frlw_sae_encode / frlw_eci_encode take for eligible calls (a workspace of exactly this
 * size gets the same path a larger one gets). */
size_t frlw_encoder_workspace_bytes(int64_t n_events, int H, int W);

/* Which form frlw_sae_encode / frlw_eci_encode launched, counted per process since it loaded the library (diagnostics and
 * tests; the results are the same bits either way): counts[0] = Surface of Active Events through the two-launch form,
 * [1] = through the general path, [2] = Event Count Image through the two-launch form, [3] = through the single-launch
 * scan or the general path. */
int frlw_encoder_path_counts(uint64_t counts[4]);

/* Synchronise `stream` and fetch the data-dependent status of the last encoder call that used
 * `workspace`: FRLW_OK, FRLW_ERR_INDEX, FRLW_ERR_POLARITY, FRLW_ERR_SPAN, or FRLW_ERR_HIP when a workgroup of a
 * fast-path launch gave up waiting for the launch's header reset (a bounded wait; the call's outputs are then incomplete). */
int frlw_encoder_status(const void *workspace, frlw_stream_t stream, int *status_out);

/* Callers that do not synchronise after every call (a training loop that encodes batch after batch) still must not
 * train on a stale state: every encoder call also ORs its data-dependent status into a word of the workspace header
 * that survives the next call.  frlw_workspace_init() zeroes the header once after the workspace is allocated;
 * frlw_encoder_deferred_status() synchronises `stream`, returns the accumulated status of all calls since (FRLW_OK or
 * the first of FRLW_ERR_INDEX / _POLARITY / _SPAN / _HIP) and clears it.  The reference raises at the offending call
 * (torch's IndexError in index_add_, generate_taf.py:24); this is the same information, one host sync per batch. */
int frlw_workspace_init(void *workspace, size_t workspace_bytes, frlw_stream_t stream);
int frlw_encoder_deferred_status(void *workspace, frlw_stream_t stream, int *status_out);

/*
 * Event Count Image -- replaces generate_eventframe(events, shape),
 * generate_eventcountimage.py:19-41.  out_f32: (2, H, W), channel = polarity, value * 255.
 * out_u8 (optional): the same after .astype(uint8) (generate_eventcountimage.py:178-180).
 * All n events are used (the harness has already cut events[-events_window:], :155).
 */
int frlw_eci_encode(const frlw_events_t *ev, int H, int W, float *out_f32, uint8_t *out_u8,
                    void *workspace, size_t workspace_bytes, frlw_stream_t stream);

/*
 * Event Volume -- replaces generate_agile_event_volume_cuda(events, shape, events_window,
 * volume_bins), generate_eventvolume.py:15-42.  out_f32: (2*bins, H, W), channel
 * 2*(k-1) + (0 if p == 1 else 1), scaled / 5 * 255.  out_u8 (optional): clipped at 255 then
 * truncated (generate_eventvolume.py:155-157).
 * XYTP_F64: column t is the normalised time, t_end / window_us are ignored.
 * DAT8: events with t <= t_end - window_us are dropped and t <- (t - (t_end - window_us)) /
 * window_us in f64 (generate_eventvolume.py:139-141).
 */
int frlw_ev_encode(const frlw_events_t *ev, int H, int W, int bins, int64_t t_end,
                   int64_t window_us, float *out_f32, uint8_t *out_u8, void *workspace,
                   size_t workspace_bytes, frlw_stream_t stream);

/*
 * Surface of Active Events -- replaces generate_leaky_cuda(events, shape, lamdas, memory, now),
 * generate_surfaceofactiveevents.py:44-80.  Events with x >= W or y >= H are dropped (:72).
 * mem_in: previous (2, H, W) memory or NULL; mem_out: new memory (2, H, W), required, may alias
 * mem_in.  out_f32: (2*n_lamda, H, W) lamda-major then polarity, * 255; out_u8 optional.
 * lamdas: HOST array of n_lamda doubles (cast to f32 like torch does for a Python scalar).
 * DAT8: events with t <= now - window_us are dropped (:183); window_us <= 0 keeps all.
 */
int frlw_sae_encode(const frlw_events_t *ev, int H, int W, const double *lamdas, int n_lamda,
                    const float *mem_in, float *mem_out, int64_t now, int64_t window_us,
                    float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes,
                    frlw_stream_t stream);

/*
 * Temporal Active Focus -- replaces generate_taf_cuda(events, shape, past_volume, volume_bins)
 * (generate_taf.py:19-67) and, for DAT8 streams, the harness loop around it (:197-227) plus
 * leaky_transform (:69-76) and the uint8 truncation (:228-235) in ONE pass over the events.
 *   state   : (H, W, 2, K) f32, read and updated in place (the reference returns a new tensor;
 *             the shim clones first).  Initialise to -6000 for a fresh sequence (:205-209).
 *   view_f32: optional (2K, H, W) f32 = ecd_viewed after the last window, channel 2k + p.
 *   out_u8  : optional (K, 2, H, W) = uint8(leaky_transform(view)); FRLW_TAF_U8_FLIP_K reverses k.
 * XYTP_F64: one window; column t is the window-relative time in [0, 1]; n_windows must be 1 and
 * t_start / window_us are ignored.
 * DAT8: window of an event z = last i in [0, n_windows) with t_start + i*window_us <= t <=
 * t_start + (i+1)*window_us, else 0 (:197-203); t <- (t - t_min) / (window_us + 1e-8) in f64 (:215).
 * A window without any event leaves the state untouched (:40-41).
 */
int frlw_taf_encode(const frlw_events_t *ev, int H, int W, int K, int64_t t_start,
                    int64_t window_us, int n_windows, float *state, float *view_f32,
                    uint8_t *out_u8, int flags, void *workspace, size_t workspace_bytes,
                    frlw_stream_t stream);

/*
 * Temporal Active Focus with SNAPSHOTS (csrc/enc_taf.h, k_taf_tile_snap) -- frlw_taf_encode on a DAT8 stream that also hands out
 * the uint8 volume after chosen windows of the same launch: the volumes at several times along one stream for one partition, one
 * tile launch and one read of the event list.  Bit w of emit_mask (w < n_windows) asks for the volume after window w; snap_u8
 * (DEVICE, popcount(emit_mask) x (K, 2, H, W)) receives them in window order, each what frlw_taf_encode's out_u8 holds when the
 * call ends after that window (FRLW_TAF_U8_FLIP_K applies).  A window without any event does not step the FIFO (:40-41) and
 * still emits: its snapshot equals the one before it.  state is updated in place.  Always the general path; same partition,
 * workspace (frlw_encoder_workspace_bytes), status word and deferred status as frlw_taf_encode; stream-ordered, no host
 * synchronisation.  FRLW_ERR_ARG: emit_mask == 0 or a bit at or above n_windows, n_windows outside 1..FRLW_MAX_WINDOWS, state or
 * snap_u8 NULL, a layout other than DAT8, window_us <= 0.
 */
int frlw_taf_encode_chain(const frlw_events_t *ev, int H, int W, int K, int64_t t_start, int64_t window_us,
                          int n_windows, uint64_t emit_mask, float *state, uint8_t *snap_u8, int flags,
                          void *workspace, size_t workspace_bytes, frlw_stream_t stream);

/*
 * Temporal Active Focus, fast path for a BATCH of independent sequences (csrc/taf_fast.hip) -- the same harness loop
 * (generate_taf.py:193-235) for n_seq <= FRLW_MAX_SEQUENCES streams in one launch sequence.  Sequence s owns the DAT8
 * records [seq_offsets[s], seq_offsets[s + 1]) of ev->data (HOST array of n_seq + 1 event indices), starts at
 * t_start[s] (HOST array) and has its own FIFO state, its own outputs and its own "window without any event leaves the
 * state untouched" rule (:40-41 is evaluated per file, :143-160):
 *   state (n_seq, H, W, 2, K) in place; view_f32 (n_seq, 2K, H, W) or NULL; out_u8 (n_seq, K, 2, H, W) or NULL.
 * Bit-identical to n_seq calls of frlw_taf_encode.  Differences in contract:
 *   - DAT8 only; 12 + ceil(log2 n_windows) + bits(window_us) <= 32 (else FRLW_ERR_UNSUPPORTED at launch);
 *   - every event must lie inside [t_start[s], t_start[s] + n_windows * window_us] (the harness cuts the stream with
 *     seek_time, :162-193).  Checked on device: frlw_encoder_status() then reports FRLW_ERR_SPAN (or FRLW_ERR_INDEX)
 *     and NOTHING has been written -- state and outputs are untouched, so the caller can fall back to
 *     frlw_taf_encode, which places such events like the reference does.
 * The stream may be in any order (sums follow stream order); a time-sorted stream is the fast case.
 * Workspace: frlw_taf_batch_workspace_bytes(total events, n_seq, H, W, window_us); 0 = unsupported shape.
 */
#define FRLW_MAX_SEQUENCES 64
size_t frlw_taf_batch_workspace_bytes(int64_t n_events, int n_seq, int H, int W, int64_t window_us);
int frlw_taf_encode_batch(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_start, int n_seq, int H,
                          int W, int K, int64_t window_us, int n_windows, float *state, float *view_f32,
                          uint8_t *out_u8, int flags, void *workspace, size_t workspace_bytes, frlw_stream_t stream);

/*
 * Row-stripe sharding of ONE frame over several GPUs ("route events by y; each GPU owns its stripe of state /
 * output -- no halo, no exchange"): every rank holds the stream, encodes rows [y_lo, y_lo + rows) of the H_full x W frame
 * (events of other rows are skipped) into ITS stripe of the state / outputs -- (n_seq, rows, W, 2, K) and so on.  One quantity
 * is global: "a window without any event in the whole frame leaves the state untouched" (generate_taf.py:40-41).  So the
 * encode runs in two halves around one 8-byte-per-sequence exchange:
 *   frlw_taf_stripe_partition(...)            hist, scans, scatter of this stripe; leaves the stripe's window masks in the workspace
 *   frlw_taf_stripe_window_masks(workspace)   device pointer to the n_seq 64-bit masks: OR-reduce them IN PLACE over the ranks
 *                                             (RCCL all-reduce with BOR through torch.distributed in the shim), same stream order
 *   frlw_taf_stripe_finish(...)               split + walk with the reduced masks; same arguments, same workspace
 * The stripes put together are bit-identical to frlw_taf_encode_batch on the whole frame.  Workspace:
 * frlw_taf_batch_workspace_bytes(total events, n_seq, rows, W, window_us).
 */
int frlw_taf_stripe_partition(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_start, int n_seq, int H_full,
                              int W, int y_lo, int rows, int K, int64_t window_us, int n_windows, void *workspace,
                              size_t workspace_bytes, frlw_stream_t stream);
unsigned long long *frlw_taf_stripe_window_masks(void *workspace);
int frlw_taf_stripe_finish(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_start, int n_seq, int H_full, int W,
                           int y_lo, int rows, int K, int64_t window_us, int n_windows, float *state, float *view_f32,
                           uint8_t *out_u8, int flags, void *workspace, size_t workspace_bytes, frlw_stream_t stream);

/*
 * Event Volume for a batch of independent streams -- the harness lines generate_eventvolume.py:139-157 (window cut,
 * f64 normalisation) around generate_agile_event_volume_cuda (:15-42) for n_seq <= FRLW_MAX_SEQUENCES label windows in one
 * launch sequence.  Sequence s owns the DAT8 records [seq_offsets[s], seq_offsets[s + 1]) and ends at t_end[s] (HOST
 * arrays): events with t <= t_end[s] - window_us are dropped (:139), t <- (t - (t_end[s] - window_us)) / window_us in f64
 * (:141).  out_f32 (n_seq, 2 * bins, H, W) and / or out_u8 (the same clipped at 255 and truncated, :155-157).
 * Bit-identical to n_seq calls of frlw_ev_encode.  Differences in contract: DAT8 only; window_us < 2^20; an event with
 * t > t_end[s] is reported by frlw_encoder_status() as FRLW_ERR_SPAN and NOTHING is written (frlw_ev_encode places it).
 * Workspace: frlw_ev_batch_workspace_bytes(total events, n_seq, H, W, window_us); 0 = unsupported shape.
 */
size_t frlw_ev_batch_workspace_bytes(int64_t n_events, int n_seq, int H, int W, int64_t window_us);
int frlw_ev_encode_batch(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *t_end, int n_seq, int H, int W,
                         int bins, int64_t window_us, float *out_f32, uint8_t *out_u8, void *workspace,
                         size_t workspace_bytes, frlw_stream_t stream);

/*
 * Event Count Image for a batch of record windows (csrc/encoders_batch.hip) -- generate_eventframe
 * (generate_eventcountimage.py:19-41) for n_win <= FRLW_MAX_SEQUENCES windows in one launch sequence.  Window w is the DAT8
 * records [win_lo[w], win_hi[w]) of ev->data (HOST arrays of record indices); windows may overlap, nest (the offline command's
 * three windows per label end at the same record) or be empty.  out_f32 and / or out_u8: (n_win, 2, H, W).
 * Bit-identical to n_win calls of frlw_eci_encode on the same record ranges, coordinate maps included.  DAT8 only; an event whose
 * flat pixel lies outside the frame is reported by frlw_encoder_status() as FRLW_ERR_INDEX (the outputs are then unspecified).
 * The counts are integer atomics on a (n_win, 2, H, W) plane of the workspace: exact in any order, no dependence on the LDS
 * lane-order self-test.  Workspace: frlw_eci_batch_workspace_bytes(total records, n_win, H, W); 0 = n_win outside
 * 1..FRLW_MAX_SEQUENCES or an unsupported shape.  More windows than that, or a range running backwards / outside the array:
 * FRLW_ERR_ARG.
 */
size_t frlw_eci_batch_workspace_bytes(int64_t n_records, int n_win, int H, int W);
int frlw_eci_encode_batch(const frlw_events_t *ev, const int64_t *win_lo, const int64_t *win_hi, int n_win, int H, int W,
                          float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes, frlw_stream_t stream);

/*
 * Surface of Active Events for a batch of independent streams (csrc/encoders_batch.hip) -- generate_leaky_cuda and its harness
 * lines (generate_surfaceofactiveevents.py:44-80, :183) for n_seq <= FRLW_MAX_SEQUENCES streams in one launch sequence.  Sequence
 * s owns the DAT8 records [seq_offsets[s], seq_offsets[s + 1]) (HOST array of n_seq + 1 record indices), has its own now[s] (HOST
 * array) and its own memory plane: mem_in (or NULL = no memory yet, as for frlw_sae_encode) and mem_out are (n_seq, 2, H, W) and
 * may alias; out_f32 / out_u8 (both optional): (n_seq, 2 * n_lamda, H, W).  Bit-identical to n_seq calls of frlw_sae_encode --
 * memory, f32 and u8: events outside the frame are dropped, events with t <= now[s] - window_us are dropped (window_us <= 0
 * keeps all), a cell keeps its LAST event in stream order, cells without one start from now[s] - 5e6.  DAT8 only.
 * Workspace: frlw_sae_batch_workspace_bytes(total records, n_seq, H, W); 0 = n_seq outside 1..FRLW_MAX_SEQUENCES or an
 * unsupported shape.
 */
size_t frlw_sae_batch_workspace_bytes(int64_t n_records, int n_seq, int H, int W);
int frlw_sae_encode_batch(const frlw_events_t *ev, const int64_t *seq_offsets, const int64_t *now, int n_seq, int H, int W,
                          const double *lamdas, int n_lamda, const float *mem_in, float *mem_out, int64_t window_us,
                          float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes, frlw_stream_t stream);

/* Calls served by the two entry points above, counted per process since it loaded the library: counts[0] =
 * frlw_eci_encode_batch, counts[1] = frlw_sae_encode_batch (host-side: ENQUEUES, the replays of a captured graph add nothing). */
int frlw_encoder_batch_counts(uint64_t counts[2]);

/*
 * Surface of Active Events for a CHAIN of steps on ONE memory plane (csrc/encoders_batch.hip) -- the labels of one file of the
 * offline command (generate_surfaceofactiveevents.py:147-200), whose per-pixel memory goes from label to label.  Step s encodes the
 * DAT8 records [step_lo[s], step_hi[s]) with its own now[s] and window_us[s] (window_us[s] <= 0 keeps every event); ranges may
 * overlap, nest, repeat or be empty.  All five arrays are HOST arrays of n_steps <= FRLW_MAX_SEQUENCES entries.  mem_in (2, H, W)
 * is what step 0 starts from (NULL = no memory yet, as for frlw_sae_encode), step s + 1 starts from what step s left, mem_out
 * receives what the last step left; the two may alias.  A step with emit[s] != 0 writes its volume, the others only advance the
 * memory: the emitting steps are packed in step order into out_f32 and / or out_u8, (n_emit, 2 * n_lamda, H, W); no emitting step
 * and both outputs NULL is legal.  Bit-identical -- memory, f32 and u8 -- to n_steps successive calls of frlw_sae_encode, each on
 * its range and fed the previous call's memory.  Three launches, no host synchronisation.  A coordinate outside the maps is
 * reported by frlw_encoder_status() as FRLW_ERR_INDEX.  Workspace: frlw_sae_chain_workspace_bytes (one 64-bit key plane per step,
 * what frlw_sae_batch_workspace_bytes asks for as many sequences); 0 = n_steps outside 1..FRLW_MAX_SEQUENCES or an unsupported shape.
 */
size_t frlw_sae_chain_workspace_bytes(int64_t n_records, int n_steps, int H, int W);
int frlw_sae_encode_chain(const frlw_events_t *ev, const int64_t *step_lo, const int64_t *step_hi, const int64_t *now,
                          const int64_t *window_us, const uint8_t *emit, int n_steps, int H, int W, const double *lamdas, int n_lamda,
                          const float *mem_in, float *mem_out, float *out_f32, uint8_t *out_u8, void *workspace,
                          size_t workspace_bytes, frlw_stream_t stream);

/*
 * Event Volume for label windows given as RECORD RANGES (csrc/taf_fast.hip): window w is the DAT8 records [win_lo[w], win_hi[w])
 * of ev->data and ends at t_end[w] (HOST arrays, n_win <= FRLW_MAX_SEQUENCES); windows may overlap, nest or be empty -- the label
 * slices of one file (generate_eventvolume.py:118-137).  One launch copies the ranges one behind the other into the workspace
 * (n_gathered = the sum of the range lengths), then the code of frlw_ev_encode_batch runs on the copy: its contract holds
 * (bit-identical to n_win calls of frlw_ev_encode; DAT8 only; window_us < 2^20; an event behind its t_end is FRLW_ERR_SPAN and
 * nothing is written; FRLW_ERR_UNSUPPORTED where the batch call answers it).  Workspace: frlw_ev_ranges_workspace_bytes =
 * frlw_ev_batch_workspace_bytes(n_gathered, ...) rounded up, which lies in FRONT (the workspace header stays the status header),
 * plus 8 bytes per gathered record behind it; 0 = unsupported.
 */
size_t frlw_ev_ranges_workspace_bytes(int64_t n_gathered, int n_win, int H, int W, int64_t window_us);
int frlw_ev_encode_ranges(const frlw_events_t *ev, const int64_t *win_lo, const int64_t *win_hi, const int64_t *t_end, int n_win,
                          int H, int W, int bins, int64_t window_us, float *out_f32, uint8_t *out_u8, void *workspace,
                          size_t workspace_bytes, frlw_stream_t stream);

/* Calls served by the two entry points above, like frlw_encoder_batch_counts: counts[0] = frlw_sae_encode_chain, counts[1] =
 * frlw_ev_encode_ranges (host-side: ENQUEUES). */
int frlw_encoder_chain_counts(uint64_t counts[2]);

/*
 * Time-surface pairs for a batch of record windows (csrc/motion.hip) -- generate_timesurface and its harness lines
 * (generate_opticalflow.py:72-92, :176-187) for n_win <= FRLW_MAX_SEQUENCES windows in one launch sequence.  Window w is the DAT8
 * records [win_lo[w], win_hi[w]) of ev->data (HOST arrays of record indices); windows may overlap, nest or be empty.  Events
 * outside the frame are dropped without error, polarity is ignored.  start / end = the smallest / largest timestamp of the window's
 * in-bounds events; volume1 keeps per cell the LAST event in stream order with t < end - 50000, volume2 the last of all;
 * out_u8 (n_win, 2, H, W) = uint8((v1 - start) / den * 255), uint8((v2 - start - 50000) / den * 255) with den = end - 50000 - start,
 * in float64 and in that operation order, untouched cells 0 before the subtraction, negative values 0: byte for byte the
 * reference's pair.  A window without an in-bounds event gives zeros.  A window with den <= 0 (its events span 50 ms or less) is
 * NOT computed -- the reference divides by zero or a negative number there and numpy's cast decides -- zeros are stored and the
 * caller recomputes it; stamps_out (DEVICE, n_win x 2 int64, or NULL) receives start and end of every window (-1, -1: none) to tell.
 * Four launches, no host synchronisation.  DAT8 only, no coordinate maps (FRLW_ERR_UNSUPPORTED).  Workspace:
 * frlw_time_surface_workspace_bytes (two 64-bit key planes per window); 0 = n_win outside 1..FRLW_MAX_SEQUENCES or an unsupported
 * shape.  A range running backwards / outside the array: FRLW_ERR_ARG.
 */
size_t frlw_time_surface_workspace_bytes(int64_t n_records, int n_win, int H, int W);
int frlw_time_surface_batch(const frlw_events_t *ev, const int64_t *win_lo, const int64_t *win_hi, int n_win, int H, int W,
                            uint8_t *out_u8, int64_t *stamps_out, void *workspace, size_t workspace_bytes, frlw_stream_t stream);

/*
 * Sum of the flow magnitude over boxes (csrc/motion.hip) -- np.sum(np.sqrt(flow[y0:y1, x0:x1, 0]**2 + flow[y0:y1, x0:x1, 1]**2))
 * of motion_level_statistics_gt.py:130 for n_boxes boxes in one launch.  flows: DEVICE (n_flows, H, W, 2) float32, 8-byte aligned;
 * boxes: DEVICE (n_boxes, 5) int32 rows [flow index, x0, x1, y0, y1]; out: DEVICE (n_boxes) float64.  The magnitude is float32
 * with every operation rounded on its own (numpy's values exactly), the sum float64 in a fixed order: deterministic, and within
 * n * 2^-53 (relative) of any other float64 summation order.  An empty box (x0 >= x1 or y0 >= y1) gives 0; a box that leaves the
 * frame or names a flow outside the batch gives NaN and reads nothing.
 */
int frlw_box_flow_sums(const float *flows, int n_flows, int H, int W, const int32_t *boxes, int64_t n_boxes, double *out,
                       frlw_stream_t stream);

/* Calls served by the two entry points above, like frlw_encoder_batch_counts: counts[0] = frlw_time_surface_batch, counts[1] =
 * frlw_box_flow_sums (host-side: ENQUEUES). */
int frlw_motion_counts(uint64_t counts[2]);

/*
 * Dual TV-L1 optical flow (Zach, Pock, Bischof 2007) between the two images of n_pairs <= FRLW_MAX_SEQUENCES uint8 pairs in one
 * launch sequence (csrc/tvl1.hip) -- the solver generate_opticalflow.py:189-190 calls, with its default parameters, as DESIGN.md's
 * motion section specifies it and tests/tvl1_restated.py restates it.  float32 throughout; no illumination term, no initial flow.
 *
 * frlw_tvl1_params_t: `struct_size` = sizeof(frlw_tvl1_params_t) as the CALLER compiled it, read like frlw_tuning_t's (fields
 * outside it take their defaults; below 8 or above 4096 is FRLW_ERR_ARG).  NULL = every default.  nscales 1..FRLW_TVL1_MAX_LEVELS,
 * warps 1..64, inner and outer >= 1, median 5 (the 5 x 5 median of the flow in front of every outer iteration) or <= 1 (none),
 * tau, lambda, theta > 0, epsilon >= 0 (0: every loop runs its full count), scale_step in [0.25, 0.95]; else FRLW_ERR_ARG.
 *
 * frlw_tvl1_plan (HOST only): the pyramid of an H x W frame -- level 0 the frame, level s the bilinear resize of level s - 1 to
 * (round(h * scale_step), round(w * scale_step)), the first level with a side below 16 dropped with all above it.  Returns the
 * number of levels (0: the frame itself has a side below 16, or a bad argument) and writes h, w of each to levels_hw (2 ints per
 * level, room for FRLW_TVL1_MAX_LEVELS; may be NULL).
 *
 * frlw_tvl1_workspace_bytes (HOST only, 64-bit arithmetic: 64 pairs of 1280 x 720 ask for more than 4 GB): about 94 bytes per
 * pixel and pair; 0 = n_pairs outside 1..FRLW_MAX_SEQUENCES, a frame with a side below 16 or above 16384, or bad parameters.
 *
 * frlw_tvl1_flow_batch: pairs DEVICE (n_pairs, 2, H, W) uint8 -- what frlw_time_surface_batch writes; flows DEVICE (n_pairs, H,
 * W, 2) float32, 8-byte aligned, [..., 0] the x and [..., 1] the y component -- what frlw_box_flow_sums reads; iters_out DEVICE
 * (n_pairs, levels, warps) int32 or NULL: the inner iterations each pair ran per level (0 = the full frame) and warp; workspace
 * 16-byte aligned.  Pairs run through levels and warps in lockstep, each with its own error, "done" word and counters on the
 * device; a pair that has converged costs its workgroups one read.  The flow of a pair is bit-identical from run to run and
 * whether it is encoded alone or at any place of a batch.  NOT capturable: once per outer iteration the host reads the pairs'
 * done words (n_pairs ints, one stream synchronisation) to stop enqueuing when every pair is through with the warp.  Plain
 * launches only: no workgroup waits on another.  Bad arguments: FRLW_ERR_ARG, nothing enqueued; FRLW_ERR_WORKSPACE likewise.
 */
#define FRLW_TVL1_MAX_LEVELS 8
typedef struct frlw_tvl1_params {
    int32_t struct_size; /* = sizeof(frlw_tvl1_params_t) */
    int32_t nscales;     /* 5 */
    int32_t warps;       /* 5 */
    int32_t inner;       /* 30 */
    int32_t outer;       /* 10 */
    int32_t median;      /* 5 */
    float tau;           /* 0.25 */
    float lambda;        /* 0.15 */
    float theta;         /* 0.3 */
    float epsilon;       /* 0.01 */
    float scale_step;    /* 0.8 */
} frlw_tvl1_params_t;
int frlw_tvl1_plan(int H, int W, int nscales, double scale_step, int *levels_hw);
size_t frlw_tvl1_workspace_bytes(int n_pairs, int H, int W, const frlw_tvl1_params_t *params);
int frlw_tvl1_flow_batch(const uint8_t *pairs, int n_pairs, int H, int W, const frlw_tvl1_params_t *params, float *flows,
                         int32_t *iters_out, void *workspace, size_t workspace_bytes, frlw_stream_t stream);

/* The solver's own counters (frlw_motion_counts keeps its two slots): counts[0] = calls of frlw_tvl1_flow_batch served, counts[1] =
 * kernel launches they enqueued (host-side: ENQUEUES). */
int frlw_tvl1_counts(uint64_t counts[2]);

/*
 * Seq-NMS over the detections of n_videos <= FRLW_MAX_SEQUENCES recordings in one call (csrc/seq_nms.hip) -- what the reference's
 * core/Others/seqnms/seq_nms.py computes, as DESIGN.md's Seq-NMS section specifies it and tests/seqnms_restated.py restates it.
 * Recording v is the frames [video_frame_start[v], video_frame_start[v + 1]), at most FRLW_SEQ_NMS_MAX_FRAMES of them; frame f is the
 * boxes [frame_start[f], frame_start[f + 1]), at most FRLW_SEQ_NMS_MAX_BOXES.  Both offset arrays are HOST arrays (n_videos + 1 and
 * n_frames_total + 1 entries, starting at 0, ascending): every limit is checked on them before anything is enqueued, and they
 * are copied into the workspace.  boxes DEVICE (total, 4) float32 x1, y1, x2, y2, 16-byte aligned; scores DEVICE float64, >= 0;
 * labels DEVICE int32.
 *
 * Box i of frame f links to box j of frame f + 1 when the labels are equal and IoU >= link_thr (float64, areas without + 1).
 * Then, again and again: the path with the largest sum of scores (ties: the lowest start frame, the lowest box; inside a path
 * the lowest successor) is selected, its boxes are rescored (metric 0: sum / length, 1: the largest member) and every box of
 * a path frame with IoU >= nms_thr against the path's box -- any label, the path's box included -- loses all its edges.
 * isolated 0: the loop ends when the best path is a single box (the reference's rule); 1: single boxes are no candidates, the
 * loop ends when no path of two or more boxes is left.  max_sequences >= 1 bounds the loop: reaching it ends it and sets
 * FRLW_SEQ_NMS_TRUNCATED in status[v]; the outputs then hold the sequences selected so far.  nms_thr <= 1 (else FRLW_ERR_ARG):
 * a path's own boxes then always leave the graph, so the loop ends after at most total / 2 rounds whatever max_sequences says.
 *
 * Outputs, DEVICE, per box: out_scores float64 (the rescored score, else the input), out_seq int32 (1-based order of selection
 * inside the recording, 0: on no sequence), out_flags uint8 (bit 0: suppressed by a sequence it is not on); status DEVICE int32
 * per recording.  Two launches, no host synchronisation, one wavefront per recording in the second: no workgroup waits on another.
 * frlw_seq_nms_workspace_bytes is HOST only (25 bytes per box and the offsets); 0 = arguments over the limits.  Null pointers
 * or offsets over the limits: FRLW_ERR_ARG; a short workspace: FRLW_ERR_WORKSPACE; nothing is enqueued in either case.
 */
#define FRLW_SEQ_NMS_MAX_FRAMES 4096
#define FRLW_SEQ_NMS_MAX_BOXES 64
#define FRLW_SEQ_NMS_TRUNCATED 1
size_t frlw_seq_nms_workspace_bytes(int64_t total_boxes, int64_t n_frames_total, int n_videos);
int frlw_seq_nms(const float *boxes, const double *scores, const int32_t *labels, const int32_t *frame_start,
                 const int32_t *video_frame_start, int n_videos, double link_thr, double nms_thr, int metric, int isolated,
                 int max_sequences, double *out_scores, int32_t *out_seq, uint8_t *out_flags, int32_t *status, void *workspace,
                 size_t workspace_bytes, frlw_stream_t stream);

/*
 * Prophesee EVT 3.0 words -> FRLW_LAYOUT_DAT8 records (csrc/evt3.hip on csrc/evt_plan.h), as DESIGN.md's "EVT 3.0 decode" section defines the format
 * and tests/evt3_restated.py restates it.  words: DEVICE, little-endian 16-bit words (any 2-byte alignment; 16-byte alignment is
 * the fast case), at most 2^31 per call; width / height in 1..2048.  A longer stream is decoded piece by piece with the state
 * carried; the cut may fall anywhere, also inside a vector run.
 *
 * frlw_evt3_count   enqueues four launches that leave in the workspace: the plan (per chunk of words its carried-in state and the
 *                   offset of its first record), the counters and the carried-out state.  state_in: HOST, NULL = start of stream.
 * frlw_evt3_result  synchronises `stream` and copies counters, carried-out state (may be NULL) and the data-dependent status to
 *                   the host.  Between the two calls the caller reads counters.events to size `out`; after frlw_evt3_emit it reads
 *                   the status: FRLW_ERR_SPAN a t does not fit 32 bits (or lies below the shift), FRLW_ERR_ARG capacity below
 *                   counters.events -- NOTHING is written in either case; FRLW_ERR_HIP the words are not the ones counted.
 * frlw_evt3_emit    one launch: the same words, n_words, width, height and workspace again; out: DEVICE, capacity records of 8
 *                   bytes, never written at or beyond capacity; time_shift != 0 subtracts (first EVT_TIME_HIGH of the stream) << 12
 *                   from every t.  Records come out in stream order, each written once.
 * Counters: t values are unshifted.  No kernel waits on another workgroup; no host synchronisation outside frlw_evt3_result.
 * frlw_evt3_workspace_bytes and frlw_evt3_geometry (words per workgroup chunk and per lane piece) are HOST only; 0 = n_words
 * negative or over the limit.  NULL pointers, a width or height outside 1..2048, a wrong struct_size: FRLW_ERR_ARG; a short
 * workspace: FRLW_ERR_WORKSPACE; nothing is enqueued in either case.
 */
typedef struct frlw_evt3_state {
    int32_t struct_size; /* sizeof(frlw_evt3_state_t) */
    int32_t reserved;
    uint32_t flags;      /* bit 0 TIME_HIGH seen, 1 TIME_LOW seen, 2 ADDR_Y seen, 3 VECT_BASE_X seen, 4 its polarity */
    uint32_t loops;      /* clock wraps so far */
    uint32_t first_high; /* first EVT_TIME_HIGH of the stream */
    uint32_t last_high;
    uint32_t low_y;      /* last EVT_TIME_LOW | last EVT_ADDR_Y << 16 */
    uint32_t base;       /* x of the next vector word's bit 0 */
    uint32_t has_last_t; /* an event was emitted so far ... */
    uint32_t reserved2;
    uint64_t last_t;     /* ... and its t */
} frlw_evt3_state_t;
typedef struct frlw_evt3_counters {
    int32_t struct_size; /* sizeof(frlw_evt3_counters_t) */
    int32_t reserved;
    uint64_t events, before_sync, out_of_frame, triggers, other_words, time_loops, unsorted, first_t, last_t, min_t, max_t;
} frlw_evt3_counters_t;
size_t frlw_evt3_workspace_bytes(int64_t n_words);
int frlw_evt3_geometry(int *chunk_words, int *lane_words);
int frlw_evt3_count(const uint16_t *words, int64_t n_words, int width, int height, const frlw_evt3_state_t *state_in, void *workspace,
                    size_t workspace_bytes, frlw_stream_t stream);
int frlw_evt3_emit(const uint16_t *words, int64_t n_words, int width, int height, void *workspace, size_t workspace_bytes, void *out,
                   int64_t capacity, int time_shift, frlw_stream_t stream);
int frlw_evt3_result(const void *workspace, frlw_stream_t stream, frlw_evt3_counters_t *counters, frlw_evt3_state_t *state_out,
                     int *status_out);

/*
 * Prophesee EVT 2.0 (32-bit words) and EVT 2.1 (64-bit words, 32 events a word) -> FRLW_LAYOUT_DAT8 records (csrc/evt2.hip on csrc/evt_plan.h), as
 * DESIGN.md's "EVT 2.0 and EVT 2.1 decode" section defines the formats and tests/evt2_restated.py restates them.  The five entry
 * points mirror the frlw_evt3_* five, with `encoding` in front: FRLW_EVT_20 or FRLW_EVT_21 (anything else: FRLW_ERR_ARG, 0 from the
 * size query).  words: DEVICE, little-endian words of the encoding's width, aligned to that width (16-byte alignment is the fast
 * case), at most 2^31 per call; width / height in 1..2048.  A longer stream is decoded piece by piece with the state carried; the
 * cut may fall anywhere.
 *
 * frlw_evt2_count   enqueues four launches that leave plan, counters and carried-out state in the workspace.  state_in: HOST,
 *                   NULL = start of stream.
 * frlw_evt2_result  synchronises `stream` and copies counters (the record of the EVT 3.0 decoder: the same nine counters, min_t
 *                   and max_t; t values unshifted), carried-out state (may be NULL) and the data-dependent status to the host:
 *                   behind frlw_evt2_emit FRLW_ERR_SPAN a t does not fit 32 bits (or lies below the shift), FRLW_ERR_ARG
 *                   capacity below counters.events -- NOTHING is written in either case; FRLW_ERR_HIP the words are not the ones
 *                   counted.
 * frlw_evt2_emit    one launch: the same encoding, words, n_words, width, height and workspace again; out: DEVICE, capacity
 *                   records of 8 bytes, never written at or beyond capacity; time_shift != 0 subtracts (first EVT_TIME_HIGH of
 *                   the stream) << 6 from every t.  Records come out in stream order (ascending bit inside an EVT 2.1 word), each
 *                   written once.
 * No kernel waits on another workgroup; no host synchronisation outside frlw_evt2_result.  frlw_evt2_workspace_bytes and
 * frlw_evt2_geometry (words per workgroup chunk and per lane piece, per encoding) are HOST only; 0 = n_words negative or over the
 * limit.  NULL pointers, a width or height outside 1..2048, a wrong struct_size: FRLW_ERR_ARG; a short workspace:
 * FRLW_ERR_WORKSPACE; nothing is enqueued in either case.
 */
enum { FRLW_EVT_20 = 20, FRLW_EVT_21 = 21 };
typedef struct frlw_evt2_state {
    int32_t struct_size; /* sizeof(frlw_evt2_state_t) */
    int32_t reserved;
    uint32_t flags;      /* bit 0 EVT_TIME_HIGH seen */
    uint32_t loops;      /* clock wraps so far */
    uint32_t first_high; /* first EVT_TIME_HIGH of the stream */
    uint32_t last_high;
    uint32_t has_last_t; /* an event was emitted so far ... */
    uint32_t reserved2;
    uint64_t last_t;     /* ... and its t */
} frlw_evt2_state_t;
size_t frlw_evt2_workspace_bytes(int encoding, int64_t n_words);
int frlw_evt2_geometry(int encoding, int *chunk_words, int *lane_words);
int frlw_evt2_count(int encoding, const void *words, int64_t n_words, int width, int height, const frlw_evt2_state_t *state_in,
                    void *workspace, size_t workspace_bytes, frlw_stream_t stream);
int frlw_evt2_emit(int encoding, const void *words, int64_t n_words, int width, int height, void *workspace, size_t workspace_bytes,
                   void *out, int64_t capacity, int time_shift, frlw_stream_t stream);
int frlw_evt2_result(const void *workspace, frlw_stream_t stream, frlw_evt3_counters_t *counters, frlw_evt2_state_t *state_out,
                     int *status_out);

/* The verdict of the one-time LDS lane-order self-test of the fast paths (frlw_taf_encode_batch, frlw_ev_encode_batch, the
 * two-launch forms of frlw_sae_encode / frlw_eci_encode) for the CURRENT device: *ok_out = 1 when the property held, 0 when
 * it did not (those entry points then answer FRLW_ERR_UNSUPPORTED and callers take the general path -- same bits, different
 * step time).  The test runs once per process and device (0.7 ms, one host synchronisation), on the first fast-path call or
 * here, whichever comes first: a job of N ranks runs it N times, once on each GPU.  Ranks that must keep the same step time
 * agree on the MINIMUM of their verdicts before the first encode (frlw_evd_amd.dist.agree_fast_path: one all-reduce).
 * `workspace`: any initialised encoder workspace (>= 1 KB). */
int frlw_fast_path_verdict(void *workspace, size_t workspace_bytes, frlw_stream_t stream, int *ok_out);

/* Self-test of the gfx950 properties frlw_taf_encode_batch relies on, for the lanes of one LDS atomic instruction that
 * hit the same address: a returning integer add serves them in ascending lane order, and ds_add_f32 applies them in that
 * order with v_add_f32 rounding (= the reference's sequential f32 sum).  256 workgroups x `iters` batches of random
 * addresses in [0, n_addr <= 512); out_dev (device, 3 x uint64): [0] = rank mismatches (must be 0), [1] = lanes that
 * shared their address with a lower lane (the sample size), [2] = f32 sums that differ from the sequential sum (must be 0). */
int frlw_selftest_lds_atomic_order(int n_addr, int iters, unsigned long long *out_dev, frlw_stream_t stream);
/* frlw_taf_encode_batch runs that self-test by itself on its first call per device (one host synchronisation for the
 * lifetime of the process, result cached) and returns FRLW_ERR_UNSUPPORTED from then on if the property does not hold, so
 * that callers take frlw_taf_encode. */
#ifdef FRLW_DEV_BUILD
/* Developer builds only (-DFRLW_DEV_BUILD -> libfrlw_evd_dev.so; NOT a symbol of the product library): tests force the
 * cached verdict of the self-test: value 0 = "does not hold", 1 = "holds", -1 = forget. */
int frlw_debug_force_lds_order(int value);
#endif

/* leaky_transform(ecd), generate_taf.py:69-76, on n floats; either output may be NULL. */
int frlw_leaky_transform(const float *in, int64_t n, float *out_f32, uint8_t *out_u8,
                         frlw_stream_t stream);

/* F.interpolate(mode='nearest') of a (C, H, W) volume to (C, Ho, Wo) as the harnesses use it
 * (generate_eventvolume.py:149): src = min(floor(dst * f32(in / out)), in - 1). */
int frlw_resize_nearest_f32(const float *in, int C, int H, int W, int Ho, int Wo, float *out,
                            frlw_stream_t stream);
int frlw_resize_nearest_u8(const uint8_t *in, int C, int H, int W, int Ho, int Wo, uint8_t *out,
                           frlw_stream_t stream);

/* np.where(v > 255, 255, v).astype(uint8) (clip255 != 0) or plain .astype(uint8) truncation. */
int frlw_quantize_u8(const float *in, int64_t n, int clip255, uint8_t *out, frlw_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * YOLOX detector forward (eval): replaces the forward of the reference's nn.Modules
 * CSPDarknet / YOLOPAFPN / YOLOXHead (core/yolox/models/, all files) called from core/model.py:40-58.
 *
 * The network is a plan of kernel launches built once from the module tree (frlw-evd_amd/detector.py
 * walks the reference-named modules, folds BatchNorm into the weights and uploads them) and replayed
 * natively by frlw_det_run.  Tensors are NHWC f32; a tensor argument is (buffer index, pixel stride
 * in floats, channel offset), so a concat is just several producers writing disjoint channel slices
 * of one buffer.  Buffer indices refer to the `bufs` array passed to frlw_det_run.
 * ------------------------------------------------------------------------------------------- */
typedef struct frlw_detector frlw_detector_t;

enum { FRLW_ACT_NONE = 0, FRLW_ACT_SILU = 1, FRLW_ACT_SIGMOID = 2 };

frlw_detector_t *frlw_det_create(void);
void frlw_det_destroy(frlw_detector_t *d);
int frlw_det_num_ops(const frlw_detector_t *d);

/* Independent sub-graphs (the three head levels) can run concurrently: ops added after frlw_det_set_lane(d, l)
 * with l in 1..2 are launched on library-owned side streams between a fork (side streams wait for everything
 * launched so far on the caller's stream) and a join (the caller's stream waits for the side streams). */
int frlw_det_set_lane(frlw_detector_t *d, int lane);

/* Arithmetic of the convolutions added from now on (default 0):
 *   0  v_mfma_f32_32x32x2_f32 on float32 operands: every product exact, the float32 MFMA rate (157 TFLOP/s peak);
 *   1  float32 products from THREE bf16 MFMAs: x = hi + lo with hi = bf16(x), lo = bf16(x - hi);
 *      a * b ~ a_hi b_hi + a_hi b_lo + a_lo b_hi, float32 accumulation -- <= 2^-16 relative error per product (observed
 *      3e-6 of max |y| per layer; the detector's stated tolerance is 1e-3), 5.3 x the matrix rate.  The activations stay
 *      float32 in memory (split in registers); `w_dev` of frlw_det_add_conv is then the SPLIT IMAGE of the [K][Npad]
 *      operand, made by frlw_conv_split_operand (frlw_conv_split_operand_bytes(K, Npad) bytes, caller-allocated). */
int frlw_det_set_precision(frlw_detector_t *d, int precision);
size_t frlw_conv_split_operand_bytes(int K, int Npad);
int frlw_conv_split_operand(const float *w, int K, int Npad, void *out, frlw_stream_t stream);
int frlw_det_add_fork(frlw_detector_t *d);
int frlw_det_add_join(frlw_detector_t *d);

/* Optional scratch buffer (index into bufs; n_floats floats PER LANE, 3 lanes) for split-K partial sums of the
 * convolutions whose output grid would leave most CUs idle (8x10 feature maps).  The buffer must be ZERO when it is first
 * handed to frlw_det_run and is left alone by the caller afterwards: the last 1024 words of every lane's region are the
 * arrival counters of the in-kernel reduction (k_conv_mfma_sk: the split that arrives last at a tile's counter sums all
 * splits and resets it). */
int frlw_det_set_scratch(frlw_detector_t *d, int buf, int64_t n_floats);

/* Focus space-to-depth (network_blocks.py:205-217): NCHW (B, C, H, W) -> NHWC (B, H/2, W/2, 4C). */
int frlw_det_add_focus(frlw_detector_t *d, int src_buf, int C, int H, int W, int dst_buf);

/* BFM stem of the yolox_taf_bfm recipes, per-pixel part + Focus layout in one kernel
 * (core/Others/Temporal_Active_Focus.py:62-127 Temporal_Active_Focus_connect.forward up to self.conv; eval mode):
 * NCHW (B, C, H, W) with C = 2 T in {4, 8, 16} -> NHWC (B, H/2, W/2, 4 * 4 log2(T)).
 * `weights` (device, kept by reference): for every stage i its effective grouped 1x1 weight g * v / |v| as
 * (out_channels_i, in_channels_per_group_i) row-major then its bias; then trans_up weight (4E, E) + bias and
 * trans_down weight (E, 4E) + bias, E = 4 log2(T).  frlw_det_bfm_weight_count(C) floats (0: unsupported C). */
/* Focus space-to-depth (network_blocks.py:205-217) as a stand-alone call: (B, C, H, W) NCHW -> (B, H/2, W/2, 4C) NHWC with
 * the channel blocks TL, BL, TR, BR -- what the train step feeds its first BaseConv (the torch.cat + layout copy it
 * replaces cost 0.55 ms per step at batch 64). */
int frlw_focus_nhwc(const float *x, int B, int C, int H, int W, float *y, frlw_stream_t stream);

/* Focus + the stem's 3x3 BaseConv (darknet.py:292) fused: the space-to-depth image stays in LDS.  w_dev / bias_dev as for
 * frlw_det_add_conv with Cin = 4 C, k = 3, Npad = Cout rounded up to 32.  C in {4, 8, 10, 16} (2, 4, 5, 8 bins of two
 * polarities), Cout <= 64 (the CSPDarknet stem is 32 wide, the Darknet-21 stem 64: two 32-channel accumulators per wavefront,
 * at C = 16 one 32-channel half per workgroup, float32 arithmetic only: in bf16x3 that form measured slower than the unfused
 * pair), else FRLW_ERR_UNSUPPORTED (use frlw_det_add_focus + frlw_det_add_conv).  The kernel's dynamic LDS is asked for here,
 * so a refusal of the runtime is FRLW_ERR_UNSUPPORTED of this call and not an error of frlw_det_run. */
int frlw_det_add_focus_stem(frlw_detector_t *d, int src_buf, int C, int H, int W, const float *w_dev, const float *bias_dev,
                            int Cout, int dst_buf, int dst_cs, int dst_co);
int frlw_det_bfm_weight_count(int C);
int frlw_det_add_bfm_stem(frlw_detector_t *d, int src_buf, int C, int H, int W, const float *weights, int n_weights,
                          int dst_buf);

/* nn.Upsample(scale_factor=2, mode="nearest") of a channel slice (yolo_pafpn.py:29).  When the slice is the output of the
 * convolution added just before (same lane; the FPN's lateral / reduce 1x1 convolutions), no launch is added: that
 * convolution's epilogue stores the upsampled copy too. */
int frlw_det_add_upsample(frlw_detector_t *d, int src_buf, int cs_src, int co_src, int C, int H, int W,
                          int dst_buf, int cs_dst, int co_dst);

/* SPPBottleneck pools (network_blocks.py:139-151): channels [0, C) -> max-pool 5 / 9 / 13 into [C, 4C). */
int frlw_det_add_spp_pool(frlw_detector_t *d, int buf, int cs, int C, int H, int W);

/*
 * BaseConv (network_blocks.py:33-65) with BatchNorm folded: y = act(conv(x, w) + bias) [+ res].
 *   w_dev   : device, (k*k*Cin, Npad) row-major, row (ky*k + kx)*Cin + ci, Npad = Cout rounded up to 32
 *   bias_dev: device, Cout floats (or NULL)
 *   k in {1, 3}, stride in {1, 2}, padding (k-1)/2; Cin, src_cs, src_co multiples of 4
 *   dst_bs  : floats between images in the destination (0 = dense Ho*Wo*dst_cs); lets the prediction
 *             convs write straight into the (B, A, 5 + nc) head tensor (yolo_head.py:229-231)
 *   res_buf : < 0 for none; Bottleneck shortcut added AFTER the activation (network_blocks.py:108-110)
 *   act     : FRLW_ACT_*; with FRLW_ACT_SIGMOID only channels >= sig_from are squashed (yolo_head.py:209-211)
 *   group_n : 0, or a multiple of 128: grouped convolution -- output channels [g * group_n, (g + 1) * group_n) read the Cin
 *             input channels starting at src_co + g * Cin (two towers of the head in one launch)
 */
int frlw_det_add_conv(frlw_detector_t *d, int src_buf, int src_cs, int src_co, int Cin, int H, int W,
                      const float *w_dev, const float *bias_dev, int Cout, int Npad, int k, int stride,
                      int dst_buf, int dst_cs, int dst_co, int64_t dst_bs, int res_buf, int res_cs,
                      int res_co, int act, int sig_from, int group_n);

/*
 * decode_outputs (yolo_head.py:258-303): xy = (xy + grid) * stride, wh = square(wh) * stride, keep
 * obj > obj_thr, class-agnostic NMS at iou_thr (the documented torchvision.ops.nms semantics: descending
 * score, suppress IoU > thr), emit [cx, cy, w, h, argmax cls, obj * max cls] in descending-score order.
 *   raw_buf    : (B, A, 5 + nc) f32     decoded_buf: optional (B, A, 5 + nc), < 0 for none
 *   dets_buf   : (B, A, 6) f32          counts_buf : (B, 1 + A) int32; [b][0] = detections of image b: 0 = nothing
 *                passed (the reference then returns one all-zero row), -1 = more than 8192 candidates (only reachable
 *                with A > 8192; not handled on device); [b][1..] = scratch (the candidates' anchors in score order)
 *   nms_buf    : (B, frlw_det_nms_workspace_floats(A)) f32 of scratch: per image the candidate count, the sorted corner
 *                boxes and the bit matrix "box i suppresses box j" (A = 6720: 5.8 MB per image).  Three launches: decode +
 *                sort per image, the bit matrix over the whole GPU, one small workgroup per image walking it in score order.
 */
long long frlw_det_nms_workspace_floats(int A);

/* The three biased 1x1 prediction convolutions of one head level in eval mode (yolo_head.py:205-231) as ONE streaming
 * pass: rows 0..4 of w_dev (F = 5 + nc rows of C floats: reg x4, obj, cls x nc) read channels [src_co, src_co + C) of the
 * level's feature buffer, rows 5.. read [src_co + C, src_co + 2 C); sigmoid on outputs >= 4; the result lands at anchors
 * [first_anchor, first_anchor + hw) of the (B, A, F) head tensor (dst_bs = A * F).  C <= 256, F <= 16, else
 * FRLW_ERR_UNSUPPORTED (use frlw_det_add_conv with the block weight matrix). */
int frlw_det_add_pred(frlw_detector_t *d, int src_buf, int src_cs, int src_co, int C, int hw, const float *w_dev,
                      const float *bias_dev, int F, int dst_buf, int first_anchor, int64_t dst_bs);

int frlw_det_add_decode_nms(frlw_detector_t *d, int raw_buf, int A, int nc, int n_levels, const int *lvl_h,
                            const int *lvl_w, const int *lvl_stride, float obj_thr, float iou_thr,
                            int decoded_buf, int dets_buf, int counts_buf, int nms_buf);

/* Launch ops [first, last) (last < 0: to the end) for B images on `stream`; bufs: n_bufs device pointers.  An op of any kind
 * whose buffer index lies outside the table or holds NULL ends the run with FRLW_ERR_ARG before that op launches anything
 * (the optional ones excepted: a convolution's residual, the decoded boxes). */
int frlw_det_run(const frlw_detector_t *d, int B, void *const *bufs, int n_bufs, int first, int last,
                 frlw_stream_t stream);

/* The three biased 1x1 prediction convolutions of ONE head level in training mode and their gradients (csrc/pred_ops.hip)
 * -- replaces torch.cat([reg_preds[k](reg_feat), obj_preds[k](reg_feat), cls_preds[k](cls_feat)], 1) of
 * core/yolox/models/yolo_head.py:160-186 (training branch, no sigmoid) and its autograd.
 *   reg_feat, cls_feat (M = B*H*W, C) NHWC rows; w_reg (4, C), w_obj (1, C), w_cls (nc, C) as torch stores the 1x1 weights;
 *   out / dout (M, 5 + nc) rows [reg 0:4 | obj | cls]; C % 4 == 0, C <= 512, 1 <= nc <= 11.
 * Deterministic (fixed summation order for the weight and bias gradients). */
int64_t frlw_pred_bwd_scratch_floats(int64_t M, int C, int nc);
int frlw_pred_fwd(const float *reg_feat, const float *cls_feat, int64_t M, int C, int nc, const float *w_reg,
                  const float *b_reg, const float *w_obj, const float *b_obj, const float *w_cls, const float *b_cls,
                  float *out, frlw_stream_t stream);
int frlw_pred_bwd(const float *reg_feat, const float *cls_feat, const float *dout, int64_t M, int C, int nc,
                  const float *w_reg, const float *w_obj, const float *w_cls, float *d_reg_feat, float *d_cls_feat,
                  float *dw_reg, float *db_reg, float *dw_obj, float *db_obj, float *dw_cls, float *db_cls, float *scratch,
                  int64_t scratch_floats, frlw_stream_t stream);
/* Which form a call of frlw_pred_fwd / frlw_pred_bwd with these sizes takes (host arithmetic only, nothing is launched):
 * out = {CPL, NG, n_wg}, the template arguments of k_pred_fwd / k_pred_bwd (float4 chunks per lane, groups of 8 outputs) and
 * the workgroups of the launch.  Returns what the compute entries return for these sizes (FRLW_OK, FRLW_ERR_ARG,
 * FRLW_ERR_UNSUPPORTED; out untouched unless FRLW_OK); the launchers take their form from the same function. */
int frlw_pred_plan(int64_t M, int C, int nc, int32_t out[3]);

/* The pools of SPPBottleneck in training mode (network_blocks.py:139-151): out (B, H, W, 4C) NHWC = cat[x, maxpool5, maxpool9,
 * maxpool13] (stride 1, "same" padding, ATen's tie rule: the first maximum in row-major window order), argmax (B, H, W, 3, C)
 * uint16 input pixel of every pooled value; the backward gathers dx (B, H, W, C) from dout (B, H, W, 4C) in a fixed order.
 * The maps of 64, 32 or 16 channels must fit the LDS (H * W <= 512), else FRLW_ERR_UNSUPPORTED. */
int frlw_spp_train_fwd(const float *x, int B, int H, int W, int C, float *out, uint16_t *argmax, frlw_stream_t stream);
int frlw_spp_train_bwd(const float *dout, const uint16_t *argmax, int B, int H, int W, int C, float *dx, frlw_stream_t stream);
/* The form of frlw_spp_train_fwd / frlw_spp_train_bwd for these sizes (host arithmetic only): out = {channels per workgroup
 * (64, 32 or 16), dynamic LDS bytes of the forward, of the backward}.  Returns what the compute entries return for these
 * sizes (out untouched unless FRLW_OK); the launchers take channel width, grid and LDS size from the same function. */
int frlw_spp_train_plan(int B, int H, int W, int C, int32_t out[3]);

/* ---------------------------------------------------------------------------------------------
 * SimOTA label assignment of the YOLOX training branch, whole batch, no host round trips.
 * Replaces the per-image Python of core/yolox/models/yolo_head.py:482-584 (get_assignments),
 * :586-669 (get_in_boxes_info), :671-707 (dynamic_k_matching) and core/yolox/utils/boxes.py:79-102.
 *
 *   preds     (B, A, 5 + num_classes) f32: decoded cx, cy, w, h (yolo_head.py:237-256), obj and class logits
 *   labels    (B, G, 5) f64 rows [class, cx, cy, w, h]; an image's boxes are its first n rows, n = number of
 *             rows with a positive field sum (yolo_head.py:330,349-350)
 *   x_shifts, y_shifts, strides  (A) f32: grid coordinates and stride of every anchor (yolo_head.py:254-256)
 *   radius    centre-sampling radius in strides (core/exp.py:377-384: 5 for GEN1, 2.5 for 1 Mpx)
 * outputs (caller-allocated):
 *   fg (B, A) u8, matched_gt (B, A) i32 (-1 = background), matched_iou (B, A) f64 (IoU of the prediction
 *   with its matched box, the class target), num_fg (B) i32, nlabel (B) i32 (may be NULL).
 * (frlw_yolox_loss_fwd below runs this assignment as a part of the whole loss.) */
size_t frlw_simota_workspace_bytes(int B, int A, int G);
int frlw_simota_assign(const float *preds, const double *labels, const float *x_shifts, const float *y_shifts,
                       const float *strides, int B, int A, int G, int num_classes, float radius, uint8_t *fg,
                       int32_t *matched_gt, double *matched_iou, int32_t *num_fg, int32_t *nlabel, void *workspace,
                       size_t workspace_bytes, frlw_stream_t stream);

/* The training loss of a batch on the raw level outputs (core/yolox/models/yolo_head.py:237-256 get_output_and_grid,
 * :305-473 get_losses; core/yolox/models/losses.py:16-36 IOUloss "iou"; nn.BCEWithLogitsLoss for objectness and class):
 * decode + concatenation, the SimOTA assignment above, the three loss sums and -- in _bwd -- the gradient of the raw
 * outputs, as six + one launches with no host synchronisation.
 *   raw, h, w, strides  HOST arrays of n_levels (<= 4) entries: device pointer to the level's (B, h, w, 5 + nc) f32 rows
 *                       cat[reg, obj, cls] (no sigmoid), its grid shape and stride
 *   labels (B, G, 5) f64 as for frlw_simota_assign
 * _fwd outputs (caller-allocated, kept for _bwd): preds (B, A, 5 + nc) f32 decoded, A = sum h*w; fg, matched_gt,
 *   matched_iou as above; result (6) f64 = {loss, 5 * loss_iou, loss_obj, loss_cls, num_fg / max(num_gt, 1),
 *   max(num_fg, 1)} -- the tuple get_losses returns (its loss_l1 is the constant 0.0) and the divisor.
 * _bwd: grad_result (4+) f64 on the device = upstream gradient of result[0..3]; grad_raw: HOST array of n_levels device
 *   pointers, each receives the (B, h, w, 5 + nc) f32 gradient of its level (every element written).
 * Dtypes as in the reference: IoU and class terms float64 (float64 labels), objectness float32; sums in float64 in a
 * fixed order (bit-reproducible). */
size_t frlw_yolox_loss_workspace_bytes(int B, int A, int G);
int frlw_yolox_loss_fwd(const float *const *raw, const int32_t *h, const int32_t *w, const float *strides, int n_levels,
                        int B, int num_classes, const double *labels, int G, float radius, float *preds, uint8_t *fg,
                        int32_t *matched_gt, double *matched_iou, double *result, void *workspace,
                        size_t workspace_bytes, frlw_stream_t stream);
int frlw_yolox_loss_bwd(const float *const *raw, const int32_t *h, const int32_t *w, const float *strides, int n_levels,
                        int B, int num_classes, const double *labels, int G, const uint8_t *fg,
                        const int32_t *matched_gt, const double *matched_iou, const double *result,
                        const double *grad_result, float *const *grad_raw, frlw_stream_t stream);

/* Sample transform of the training loader for a batch (data/dataset.py:217-231 in propheseeDataset.__getitem__):
 * (B, C, H, W) uint8 -> (B, C, H, W) f32 = flip(crop(nearest_resize(x, (Hr, Wr)) / 255)).
 * params (device): B rows of five int32 {Hr = int(H * sr), Wr = int(W * sr), y0 = -cy, x0 = -cx, flip}. */
int frlw_sample_transform_u8(const uint8_t *in, int B, int C, int H, int W, const int32_t *params, float *out,
                             frlw_stream_t stream);

/* Volume hand-off: a detector batch from uint8 volumes that lie in different encoder outputs, in one launch.
 * src: HOST array of B (1..64) device pointers; src[b] is the first of C consecutive (h, w) uint8 planes of sample b, at any
 * byte address.  The pointers travel to the kernel by value: no device table, no copy, capturable.
 * out (B, C, H, W) f32: out[b][c][y][x] = (float)src[b][c][ys][xs] / 255.0f with the nearest rule of frlw_resize_nearest_u8
 * (ys = min(floor(y * (float)h / (float)H), h - 1), xs likewise) -- byte-equal to frlw_resize_nearest_u8 followed by
 * frlw_sample_transform_u8 with {H, W, 0, 0, 0} rows.  B outside 1..64, a non-positive size or a NULL pointer:
 * FRLW_ERR_ARG, nothing is written. */
int frlw_volume_hand_off_u8(const uint8_t *const *src, int B, int C, int h, int w, int H, int W, float *out,
                            frlw_stream_t stream);

/* Evaluator hand-off for the detections of a batch (evaluate/evaluator.py:56-63 transform_dt, and the mask of
 * evaluate/src/io/box_filtering.py:17-39): n packed rows [cx, cy, w, h, class, score] (detector pixels) ->
 * out (n, 8) f32 [t, x, y, w, h, class, score, 0] (sensor pixels; t = timestamps[img_of_row[i]]) and
 * keep[i] = t > skip_ts && w^2 + h^2 >= min_diag_sq && w >= min_w && h >= min_h. */
int frlw_eval_transform_dt(const float *dets, const int32_t *img_of_row, const int64_t *timestamps, int64_t n, float rw,
                           float rh, float skip_ts, float min_diag_sq, float min_w, float min_h, float *out,
                           uint8_t *keep, frlw_stream_t stream);

/* COCO bounding-box mAP (evaluate/src/metrics/coco_eval.py:89-113: pycocotools COCOeval, iouType 'bbox', default
 * params, no crowd annotations) of n_img images ("windows") and n_cls categories (frlw-evd_amd/coco_eval.py packs them).
 * Ground truths of image i are rows gt_off[i] .. gt_off[i+1]-1 (gt_off[n_img] = n_gt), detections likewise with dt_off:
 * box (n, 4) double [x, y, w, h], area double (w * h in the row's own dtype, widened), class int32 in [0, n_cls) (rows of
 * other classes are dropped by the caller), score double.  iou_thrs[10] = np.linspace(.5, .95, 10) and
 * rec_thrs[101] = np.linspace(0, 1, 101) as pycocotools builds them.  Outputs (device, float64, C order):
 * precision (10, 101, n_cls, 4, 3) and recall (10, n_cls, 4, 3), = COCOeval.eval['precision'] / ['recall'] bit for bit.
 * 1 <= n_cls <= 254, n_dt < 2^31.  Bad sizes: FRLW_ERR_ARG; workspace below frlw_coco_workspace_bytes(): FRLW_ERR_WORKSPACE.
 * The workspace query is host arithmetic only (0 for sizes the evaluator refuses). */
int64_t frlw_coco_workspace_bytes(int64_t n_img, int64_t n_gt, int64_t n_dt, int n_cls);
int frlw_coco_eval(const double *gt_box, const double *gt_area, const int32_t *gt_cls, const int64_t *gt_off, int64_t n_gt,
                   const double *dt_box, const double *dt_area, const double *dt_score, const int32_t *dt_cls,
                   const int64_t *dt_off, int64_t n_dt, int n_img, int n_cls, const double *iou_thrs, const double *rec_thrs,
                   void *workspace, int64_t workspace_bytes, double *precision, double *recall, frlw_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training-mode BaseConv = Conv2d(bias=False) + BatchNorm2d(batch statistics) + SiLU
 * (core/yolox/models/network_blocks.py:33-65) for the train step of core/exp.py:283-315: forward, data gradient,
 * weight gradient, BatchNorm + SiLU forward / backward.  All tensors NHWC float32 (= torch channels_last storage),
 * dense (pixel stride = channels).  Cin % 4 == 0 and Cout % 4 == 0.  `scratch` buffers are caller-owned.
 * `precision` (every contraction below): 0 = float32 MFMA, 1 = float32 products from three bf16 MFMAs (see
 * frlw_det_set_precision; the weight operands are then split images of ceil16(K) rows -- frlw_conv_operand_floats --
 * and the data-gradient operand of a parity-grouped layer needs Cout % 16 == 0, else FRLW_ERR_UNSUPPORTED: use 0 there).
 * ------------------------------------------------------------------------------------------- */
/* floats (4-byte units) of a GEMM operand with K rows and N columns: rows(K, precision) * pad32(N). */
int64_t frlw_conv_operand_floats(int K, int N, int precision);
/* torch weight (Cout, Cin, k, k) -> forward operand (k*k*Cin, pad32(Cout)) and / or data-gradient operand
 * (k*k*Cout, pad32(Cin)) with flipped taps; with dgrad_parity = frlw_conv2d_dgrad_parity(k, stride, H, W) != 0 the
 * rows of the latter are grouped by output parity class (see frlw_conv2d_dgrad).  pad32(n) = n rounded up to 32.
 * Either output may be NULL. */
int frlw_conv2d_dgrad_parity(int k, int stride, int H, int W);
int frlw_conv_weight_layouts(const float *w, int Cout, int Cin, int k, int dgrad_parity, float *w_fwd, float *w_dgrad,
                             int precision, frlw_stream_t stream);
/* The same for MANY weights in one launch (the ~74 BaseConv weights of the detector after an optimizer step: 74 launches
 * of ~5 us each otherwise).  `items`: DEVICE array of n entries, `first` = running sum of the entries' element counts
 * (frlw_conv_operand_floats(k*k*Cin, Cout, precision) + frlw_conv_operand_floats(k*k*Cout, Cin, precision) each; either
 * operand pointer may be NULL and then counts 0), `total` = the sum. */
typedef struct frlw_weight_layout_item {
    const float *w;
    float *w_fwd, *w_dgrad;
    int32_t Cout, Cin, k, dgrad_parity;
    int32_t precision, reserved;
    int64_t first;
    const float *w2;   /* split > 0: output channels [split, Cout) come from this second weight (Cout - split, Cin, k, k): the */
    int32_t split, reserved2; /* operands of two BaseConvs stacked along the output channels (frlw_baseconv_fuse_t::split) */
} frlw_weight_layout_item_t;
int frlw_conv_weight_layouts_batch(const frlw_weight_layout_item_t *items, int n, int64_t total, frlw_stream_t stream);
/* Which form every convolution and weight gradient of this process took (frlw_conv2d_fwd / _dgrad / _wgrad, the train-mode
 * BaseConv calls and the convolutions of frlw_det_run alike), counted per process since it loaded the library -- diagnostics
 * and tests that must know which kernel a shape reaches.  The counts are host-side: they count ENQUEUES, so the replays of a
 * captured hipGraph add nothing.  Each convolution launch counts one of 128X32 .. SPLIT_SCALAR (its tile, or for the 64 x 64
 * tile how the contraction is reduced: whole, split + k_splitk_reduce<vector | scalar>, split reduced inside the kernel with
 * or without the BatchNorm statistics of the train forward) and may count GATHERED (Cin % 16 != 0: taps gathered per k-tile)
 * and PARITY (one parity class of a stride-2 data gradient); HALF_BATCH counts each split of a batch whose view exceeds the
 * 32-bit buffer offsets.  Each weight gradient counts one WGRAD tile, and GROUP_SUM / SCRATCH_LIMITED when it sums its
 * partial tiles in groups / takes fewer splits than frlw_conv2d_wgrad_scratch_floats asked for.
 * frlw_conv_path_counts copies the first min(n, FRLW_CONV_PATH_COUNT) counters to `counts` (HOST memory) and returns
 * FRLW_CONV_PATH_COUNT; NULL or n < 1: FRLW_ERR_ARG. */
enum {
    FRLW_CONV_PATH_128X32 = 0,
    FRLW_CONV_PATH_128X128_4X1,          /* bf16x3 only */
    FRLW_CONV_PATH_128X128_2X2,
    FRLW_CONV_PATH_64X128,
    FRLW_CONV_PATH_64X64,                /* whole contraction */
    FRLW_CONV_PATH_SPLIT_VEC,            /* 64 x 64, split-K + k_splitk_reduce<true> */
    FRLW_CONV_PATH_SPLIT_SCALAR,         /* 64 x 64, split-K + k_splitk_reduce<false> */
    FRLW_CONV_PATH_SPLIT_INKERNEL,       /* k_conv_mfma_sk */
    FRLW_CONV_PATH_SPLIT_INKERNEL_STATS, /* k_conv_mfma_sk leaving the BatchNorm statistics too */
    FRLW_CONV_PATH_GATHERED,
    FRLW_CONV_PATH_HALF_BATCH,
    FRLW_CONV_PATH_PARITY,
    FRLW_CONV_PATH_WGRAD_128X128,
    FRLW_CONV_PATH_WGRAD_128X32,
    FRLW_CONV_PATH_WGRAD_128X64,
    FRLW_CONV_PATH_WGRAD_64X64,
    FRLW_CONV_PATH_WGRAD_GROUP_SUM,
    FRLW_CONV_PATH_WGRAD_SCRATCH_LIMITED,
    FRLW_CONV_PATH_COUNT
};
int frlw_conv_path_counts(uint64_t *counts, int n);
/* z (B, Ho, Wo, Cout) = conv2d(x (B, H, W, Cin), w), padding (k - 1) / 2, stride 1 or 2.  scratch: optional split-K
 * partial sums (scratch_floats floats; NULL = never split). */
int frlw_conv2d_fwd(const float *x, int B, int H, int W, int Cin, const float *w_fwd, int Cout, int k, int stride, float *z,
                    float *scratch, int64_t scratch_floats, int precision, frlw_stream_t stream);
/* dx (B, H, W, Cin) = gradient of the convolution above with respect to x, from dz (B, Ho, Wo, Cout).  Stride 2 with
 * k = 3 and even H, W (frlw_conv2d_dgrad_parity) runs as four stride-1 convolutions, one per output parity class
 * (1 / 2 / 2 / 4 taps) and needs the parity-grouped operand; other stride-2 shapes use a transposed gather. */
int frlw_conv2d_dgrad(const float *dz, int B, int Ho, int Wo, int Cout, const float *w_dgrad, int Cin, int k, int stride,
                      int H, int W, float *dx, float *scratch, int64_t scratch_floats, int precision, frlw_stream_t stream);
/* dw in torch's (Cout, Cin, k, k) layout = gradient with respect to the weight; scratch is REQUIRED
 * (frlw_conv2d_wgrad_scratch_floats floats for full parallelism; fewer = fewer splits). */
int64_t frlw_conv2d_wgrad_scratch_floats(int B, int Ho, int Wo, int Cin, int Cout, int k);
int frlw_conv2d_wgrad(const float *x, int B, int H, int W, int Cin, const float *dz, int Ho, int Wo, int Cout, int k,
                      int stride, float *dw, float *scratch, int64_t scratch_floats, int precision, frlw_stream_t stream);
/* Which BatchNorm + SiLU form of the train step was enqueued, counted like frlw_conv_path_counts (host-side, ENQUEUES: a
 * captured hipGraph's replays add nothing).  One of STATS_* per statistics computation, by where the per-channel sums come
 * from: PASS = a pass over z of its own (frlw_bn_stats, or a train forward whose convolution left no sums), EPILOGUE = the
 * unsplit convolution's epilogue, SPLIT_INKERNEL = the last arriver of an in-kernel split-K convolution.  FWD / FWD_FUSED: one
 * normalise + SiLU pass, dense or with a residual, a row stride or a stacked pair.  BWD / BWD_PAIR: one backward (partial
 * sums, final, apply), one block or a stacked pair.  frlw_bn_path_counts copies the first min(n, FRLW_BN_PATH_COUNT) counters
 * to `counts` (HOST memory) and returns FRLW_BN_PATH_COUNT; NULL or n < 1: FRLW_ERR_ARG. */
enum {
    FRLW_BN_PATH_STATS_PASS = 0,
    FRLW_BN_PATH_STATS_EPILOGUE,
    FRLW_BN_PATH_STATS_SPLIT_INKERNEL,
    FRLW_BN_PATH_FWD,
    FRLW_BN_PATH_FWD_FUSED,
    FRLW_BN_PATH_BWD,
    FRLW_BN_PATH_BWD_PAIR,
    FRLW_BN_PATH_COUNT
};
int frlw_bn_path_counts(uint64_t *counts, int n);
/* Per-channel batch statistics of z viewed as (M, C): mean, biased variance, invstd = 1 / sqrt(var + eps), accumulated in
 * float64 (the variance keeps float32 accuracy for any ratio of mean to spread).  M = 1: var = 0 (and a train forward's
 * running variance is updated with 0 as the unbiased variance; nn.BatchNorm2d refuses M = 1 in training).
 * scratch: frlw_bn_scratch_doubles(M, C) doubles. */
int64_t frlw_bn_scratch_doubles(int64_t M, int C);
int frlw_bn_stats(const float *z, int64_t M, int C, float eps, float *mean, float *var, float *invstd, double *scratch,
                  frlw_stream_t stream);
/* y = silu(gamma * (z - mean) * invstd + beta) */
int frlw_bn_silu_fwd(const float *z, int64_t M, int C, const float *gamma, const float *beta, const float *mean,
                     const float *invstd, float *y, frlw_stream_t stream);
/* dz, dgamma (C), dbeta (C) from dy and the saved z; sums: 2 C floats of scratch.  dy_row_stride: floats between two rows
 * of dy (0 or C: dense; larger: dy is a channel slice of a wider NHWC gradient -- what the backward of a concatenation hands
 * out -- read in place; multiple of 4, dy 16-byte aligned). */
int frlw_bn_silu_bwd(const float *dy, int64_t dy_row_stride, const float *z, int64_t M, int C, const float *gamma, const float *beta,
                     const float *mean, const float *invstd, float *dz, float *dgamma, float *dbeta, double *scratch,
                     float *sums, frlw_stream_t stream);

/* The whole block in one call per direction (what frlw-evd_amd/yolox/train_ops.py uses): forward = weight layout +
 * convolution + batch statistics + BatchNorm/SiLU; backward = BatchNorm/SiLU backward + data gradient (dx may be NULL)
 * + weight gradient.  x (B, H, W, Cin), z / y / dy / dz (B, Ho, Wo, Cout) NHWC; w and dw in torch's (Cout, Cin, k, k).
 * mean / var (biased) / invstd: (Cout).  running_mean / running_var (may be NULL) are updated in place like
 * nn.BatchNorm2d: r = (1 - momentum) r + momentum * {mean, unbiased variance}; num_batches_tracked (device int64, may be
 * NULL) is incremented by one in the same launch sequence.
 * scratch: frlw_baseconv_train_scratch_bytes(...) bytes, reusable between calls.
 * w_cache (may be NULL): frlw_baseconv_weight_cache_floats(Cin, Cout, k, precision) floats owned by the caller, one per layer: the
 * forward then lays the weight out for itself AND for the data gradient in one launch, and the backward of the same
 * step (weights unchanged in between) reuses it instead of laying the weight out again.  w == NULL with a w_cache in
 * the forward: the cache holds both operands of the current weights already (frlw_conv_weight_layouts_batch: forward
 * operand first, the data-gradient operand frlw_conv_operand_floats(k*k*Cin, Cout, precision) floats behind it) and no layout kernel is launched.
 * splitk_counters (may be NULL): 1024 ints owned by the caller, ZERO when first handed over and left alone by the caller
 * afterwards -- one buffer for all layers and calls of a stream.  With it, a convolution that splits its contraction over
 * blockIdx.z (thin layers: few output tiles, long contractions) sums the splits INSIDE the kernel -- the split that arrives
 * last at its tile's counter adds all of them in split order, the same bits as the separate reduction launch, and sets the
 * counter back to zero -- instead of launching k_splitk_reduce behind it (NULL).  frlw_det_run does the same with the last
 * 1024 words of every lane's scratch region (frlw_det_set_scratch: the caller hands the buffer over zeroed).
 * fuse (may be NULL): what the blocks AROUND this BaseConv would otherwise do in launches of their own (round 6) --
 *   residual: y = silu(bn(conv(x))) + residual -- the Bottleneck shortcut (network_blocks.py:109-111) in the pass that writes y;
 *   y_row_stride: y is a channel slice of a wider NHWC tensor (the concatenation buffer of a CSPLayer, network_blocks.py:191-193):
 *     the block writes its output where the concatenation would have copied it;
 *   dx_add: dx = data gradient + dx_add in the convolution's epilogue -- the gradient another consumer of the same x has
 *     produced already (the shortcut's dy, the sibling 1x1 branch of a CSPLayer): autograd's accumulation launch is gone.
 *     Stride-1 layers only (FRLW_ERR_UNSUPPORTED otherwise).
 *   Row strides in floats, multiples of 4, 0 = dense; pointers 16-byte aligned.  The sums are the same IEEE additions the separate
 *   launches made (a + b = b + a): results are bit-identical to the unfused sequence. */
typedef struct frlw_baseconv_fuse {
    int32_t struct_size;         /* sizeof(frlw_baseconv_fuse_t) */
    int32_t reserved;
    const float *residual;       /* forward; (B, Ho, Wo, Cout) rows */
    int64_t residual_row_stride;
    int64_t y_row_stride;        /* forward */
    const float *dx_add;         /* backward; (B, H, W, Cin) rows */
    int64_t dx_add_row_stride;
    /* split > 0: the call is TWO BaseConvs reading the same x (conv1 | conv2 of a CSPLayer, network_blocks.py:191-193), stacked
     * along the output channels: Cout = both blocks' channels, channels [0, split) are the first block's (w, gamma, beta, running
     * statistics, num_batches_tracked, y, dy: the call's own arguments; their rows are `split` wide by default), channels
     * [split, Cout) the second block's (the fields below).  ONE convolution, ONE statistics / BatchNorm pass, ONE data gradient
     * (dx is the sum over both blocks by construction) and ONE weight gradient do the work of two of each; z, dz, mean, var,
     * invstd, dw, dgamma, dbeta are stacked (Cout wide; dw = (Cout, Cin, k, k): the second block's rows start at split).
     * split % 4 == 0; no residual.  w_cache (when the caller lays the operands out itself): the operands of the STACKED weight. */
    int32_t split, reserved2;
    const float *w2;             /* (Cout - split, Cin, k, k) */
    const float *gamma2, *beta2;
    float *running_mean2, *running_var2;
    int64_t *num_batches_tracked2;
    float *y2;                   /* forward */
    int64_t y2_row_stride;
    const float *dy2;            /* backward */
    int64_t dy2_row_stride;
} frlw_baseconv_fuse_t;
int64_t frlw_baseconv_weight_cache_floats(int Cin, int Cout, int k, int precision);
int64_t frlw_baseconv_train_scratch_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride);
int frlw_baseconv_train_fwd(const float *x, const float *w, const float *gamma, const float *beta, float eps, int B, int H,
                            int W, int Cin, int Cout, int k, int stride, float *z, float *y, float *mean, float *var,
                            float *invstd, float *running_mean, float *running_var, float momentum,
                            int64_t *num_batches_tracked, float *w_cache, void *scratch, int64_t scratch_bytes,
                            int *splitk_counters, const frlw_baseconv_fuse_t *fuse, int precision, frlw_stream_t stream);
int frlw_baseconv_train_bwd(const float *dy, int64_t dy_row_stride, const float *x, const float *z, const float *w, const float *gamma,
                            const float *beta, const float *mean, const float *invstd, int B, int H, int W, int Cin,
                            int Cout, int k, int stride, float *dz, float *dx, float *dw, float *dgamma, float *dbeta,
                            const float *w_cache, void *scratch, int64_t scratch_bytes, int *splitk_counters,
                            const frlw_baseconv_fuse_t *fuse, int precision, frlw_stream_t stream);

/* ---- Visualization (csrc/render.hip): representation -> colour image -> boxes and tags, one launch per batch.
 *
 * frlw_render_frames paints n <= FRLW_RENDER_MAX_FRAMES frames.  src: uint8 volumes (n, C, h, w) at the stored shape, sampled to
 * the output shape (H, W) by the nearest rule of frlw_resize_nearest_u8, or -- mode FRLW_RENDER_BGR -- ready backgrounds
 * (n, H, W, 3) (then C = 3, h = H, w = W).  Backgrounds: TAF (C even, >= 2), SAE (C >= 1), ECI (C = 2), EV (C even, >= 2) as
 * DESIGN.md 3.16 defines them.  boxes: a DEVICE array of 32-byte records, box_offsets: a HOST array of n + 1 non-decreasing
 * offsets into it (frame i owns [box_offsets[i], box_offsets[i + 1]), at most FRLW_RENDER_MAX_BOXES of them); boxes may be NULL
 * when there is none.  A frame's boxes apply in array order, the last hit wins; per box: outline, tag fill, glyphs.  out:
 * (n, H, W, 3) uint8 BGR, must not overlap src.  Every output byte is written by exactly one thread: no atomics, bit-deterministic
 * alone or batched.  Argument errors (FRLW_ERR_ARG) are found on the host before anything is launched. */
#define FRLW_RENDER_MAX_FRAMES 64
#define FRLW_RENDER_MAX_BOXES 512
enum { FRLW_RENDER_TAF = 0, FRLW_RENDER_SAE = 1, FRLW_RENDER_ECI = 2, FRLW_RENDER_EV = 3, FRLW_RENDER_BGR = 4 };
typedef struct frlw_render_box {
    int32_t x1, y1, x2, y2;  /* inclusive corners, each within +-2^20 */
    uint8_t kind;            /* 0 ground truth, 1 detection: colour and tag width */
    uint8_t n_label, n_score, reserved;
    uint8_t label[8];        /* n_label <= 5 characters of the class name (a-z, 0-9, '.'; anything else is blank) */
    uint8_t score[4];        /* n_score <= 4 characters of the confidence */
} frlw_render_box_t;
int frlw_render_frames(const uint8_t *src, int n, int C, int h, int w, int mode, int H, int W, const frlw_render_box_t *boxes,
                       const int32_t *box_offsets, uint8_t *out, frlw_stream_t stream);
/* (n_pixels, 3) uint8 H, S, V -> B, G, R by the conversion the TAF / SAE / EV backgrounds go through (H in units of 2 degrees,
 * values above 180 wrap). */
int frlw_hsv_to_bgr_u8(const uint8_t *hsv, uint8_t *bgr, int64_t n_pixels, frlw_stream_t stream);

/* Measurement aid: a bare loop of v_mfma_f32_32x32x2_f32 (the instruction of every convolution here) on `blocks`
 * workgroups of four wavefronts, iters x 32 MFMAs (= iters x 131072 FLOP) per wavefront, operands = the 256 floats of
 * `seed` (device).  Timed by the caller (bench.py): the fp32 matrix rate the chip SUSTAINS on non-trivial data, which is
 * what the convolutions can approach -- the data-sheet peak assumes the maximum clock. */
int frlw_selftest_mfma_f32_rate(int blocks, int iters, const float *seed, float *sink, frlw_stream_t stream);

/* Library identification: "frlw_evd <version> gfx950". */
const char *frlw_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FRLW_EVD_H */
