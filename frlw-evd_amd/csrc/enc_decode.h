// enc_decode.h -- how one event becomes (tile, cell, window, value): Decode, Pos, place, the DAT8 and f64 decoders.
// Expects frlw_common.h above it (ST_*, kTileH / kTileHLog from frlw_consts.h, the HIP runtime); frlw_common.h includes it.
#pragma once

namespace frlw {
// How one event becomes (tile, cell, window, value).  Passed by value to the kernels.
struct Decode {
    const void *data;
    long long n;
    int row_stride;
    const uint16_t *xmap;
    const uint16_t *ymap;
    int map_w, map_h;
    int H, W;
    int twl;            // log2 of the tile width
    int tiles_x, n_tiles;
    long long t0;       // EV: t_end - window; SAE: now - window; TAF: t_start
    long long win;      // EV: window; TAF: window_us
    int n_windows;      // TAF
    int time_filter;    // DAT8 EV / SAE: drop t <= t0
    uint32_t win_magic; // floor(2^32 / win), TAF DAT8
    const float *tlut;  // TAF DAT8: tlut[r] = float(r / (win + 1e-8)) - 1 for r in [0, win], or NULL
};

struct Pos {
    int tile;      // < 0: not encoded
    uint32_t cell; // ((ly << twl | lx) << 1) | p
    int err;
};

// Bounds / polarity handling common to all layouts.
template <int KIND>
__device__ __forceinline__ Pos place(const Decode &P, int x, int y, int p)
{
    Pos r = {-1, 0u, 0};
    if ((unsigned)p > 1u) { r.err = ST_POLARITY; return r; }
    if ((unsigned)x >= (unsigned)P.W || (unsigned)y >= (unsigned)P.H) {
        // The reference indexes the FLAT pixel x + W*y (generate_eventvolume.py:32): x >= W aliases
        // into the next row and only a flat index outside [0, H*W) raises.  index_put_ (SAE,
        // generate_surfaceofactiveevents.py:49) checks each axis.
        if (KIND == KIND_SAE) { r.err = ST_INDEX; return r; }
        long long flat = (long long)x + (long long)P.W * y;
        if (flat < 0 || flat >= (long long)P.H * P.W) { r.err = ST_INDEX; return r; }
        y = (int)(flat / P.W);
        x = (int)(flat - (long long)y * P.W);
    }
    r.tile = (y >> kTileHLog) * P.tiles_x + (x >> P.twl);
    r.cell = (uint32_t)((((y & (kTileH - 1)) << P.twl) | (x & ((1 << P.twl) - 1))) << 1) | (uint32_t)p;
    return r;
}

// Position of a raw DAT record (src/io/dat_events_tools.py:96-98) incl. the optional coordinate
// maps and the time / range filters that drop an event without an error.
template <int KIND, bool HAS_MAP = true>
__device__ __forceinline__ Pos dat_pos(const Decode &P, uint2 r)
{
    int x = (int)(r.y & 16383u), y = (int)((r.y >> 14) & 16383u), p = (int)((r.y >> 28) & 1u);
    Pos o = {-1, 0u, 0};
    if (HAS_MAP && P.xmap) {
        if (x >= P.map_w || y >= P.map_h) { o.err = ST_INDEX; return o; }
        x = P.xmap[x];
        y = P.ymap[y];
    }
    if (KIND == KIND_SAE && (x >= P.W || y >= P.H)) return o; // generate_surfaceofactiveevents.py:72
    if ((KIND == KIND_EV || KIND == KIND_SAE) && P.time_filter && !((long long)r.x > P.t0)) return o;
    return place<KIND>(P, x, y, p);
}

// Window and f32 value of a raw DAT record.
template <int KIND>
__device__ __forceinline__ void dat_value(const Decode &P, uint2 r, int &window, float &val)
{
    window = 0;
    val = 0.0f;
    if (KIND == KIND_EV) {
        val = (float)((double)((long long)r.x - P.t0) / (double)P.win); // generate_eventvolume.py:141
    } else if (KIND == KIND_SAE) {
        val = (float)r.x; // float(t), generate_surfaceofactiveevents.py:76
    } else if (KIND == KIND_TAF) {
        // generate_taf.py:197-203: z = the last window i with start + i*w <= t <= start + (i+1)*w, else 0
        const long long rel = (long long)r.x - P.t0;
        const uint32_t winu = (uint32_t)P.win;
        double num;
        if (rel >= 0 && rel <= (long long)P.n_windows * P.win) {
            const uint32_t relu = (uint32_t)rel;
            uint32_t z = __umulhi(relu, P.win_magic); // floor(rel / win) - {0, 1, 2}
            uint32_t rem = relu - z * winu;
            if (rem >= winu) { ++z; rem -= winu; }
            if (rem >= winu) { ++z; rem -= winu; }
            if (z >= (uint32_t)P.n_windows) { z = (uint32_t)P.n_windows - 1u; rem = winu; } // t == end of the last window
            window = (int)z;
            if (P.tlut) { val = P.tlut[rem]; return; } // same f64 division, done once per distinct value
            num = (double)rem;
        } else {
            num = (double)rel; // outside the span: window 0, normalised time outside [0, 1]
        }
        const double tn = num / ((double)P.win + 1e-8); // generate_taf.py:215
        val = (float)tn - 1.0f;                         // t - 1, generate_taf.py:26
    }
}

// The reference's device tensor: (N, row_stride) float64 rows [x, y, t, p, ...].
template <int KIND>
__device__ __forceinline__ Pos f64_pos(const Decode &P, long long i, double &t)
{
    const double *r = (const double *)P.data + i * (long long)P.row_stride;
    const double xd = r[0], yd = r[1], pd = r[3];
    t = r[2];
    Pos o = {-1, 0u, 0};
    if (KIND == KIND_SAE && !(xd < (double)P.W && yd < (double)P.H)) return o;
    if (!(fabs(xd) < 1.0e9) || !(fabs(yd) < 1.0e9) || !(fabs(pd) < 1.0e9)) { o.err = ST_INDEX; return o; }
    return place<KIND>(P, (int)xd, (int)yd, (int)pd); // .long(): truncation toward zero
}

template <int KIND>
__device__ __forceinline__ float f64_value(double t)
{
    if (KIND == KIND_TAF) return (float)t - 1.0f; // generate_taf.py:26
    if (KIND == KIND_ECI) return 0.0f;
    return (float)t;
}
} // namespace frlw
