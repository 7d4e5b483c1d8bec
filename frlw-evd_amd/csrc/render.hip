// render.hip -- visualization (the reference's visualization.py): uint8 representation -> colour image -> boxes
// with tags, for up to 64 frames in ONE launch.  Output-driven: a thread owns four horizontally adjacent output pixels, computes
// their background from the stored volume (nearest sampling, nearest_src of frlw_common.h), walks the frame's boxes in list order
// (the last hit wins) and writes the 12 bytes as three dword stores.  No two threads write the same byte, nothing is accumulated:
// no atomics, and a frame's bytes do not depend on what else is in the batch.
//
// Tile: 128 x 8 pixels per workgroup of 256 threads = 32 thread columns x 8 rows, so a wavefront covers two rows of the tile and
// stores 2 x 384 contiguous bytes per dword slot; its source reads walk 2 rows of each channel plane.  Before the pixels, the
// workgroup compacts the frame's boxes whose footprint (box rectangle or tag rectangle) meets its tile into LDS, in order: ballot,
// popcount below the lane, the wave totals through four LDS words.  512 records of 32 bytes = 16 KB of LDS.  The pixel loop then
// runs over the same list for every lane of the workgroup (LDS broadcast reads).
//
// The TAF median does not sort: a bisection on the value finds the lower middle, one more pass the upper.  Up to 16 channels the
// pixel's bytes are read once and kept packed in four registers; above that every pass re-reads them (they stay in L1).  Either
// way there is no per-lane array, so nothing can land in scratch, and any even C works.

#include "frlw_common.h"

using namespace frlw;

namespace {

constexpr int kRenderTileW = 128, kRenderTileH = 8, kPixPerThread = 4, kThreads = (kRenderTileW / kPixPerThread) * kRenderTileH;
constexpr int kBoxWords = 8; // a frlw_render_box_t as dwords
static_assert(sizeof(frlw_render_box_t) == 4 * kBoxWords, "box record: 32 bytes");
static_assert(kThreads == 256 && kThreads % 64 == 0, "four whole wavefronts");

struct BoxOffsets { int32_t v[FRLW_RENDER_MAX_FRAMES + 1]; }; // by value in the kernel arguments: the host checked them

// ---- the glyph table: 35 bits a glyph, row r in bits [5 r, 5 r + 5), bit 4 of a row = leftmost column
constexpr unsigned long long glyph_bits(unsigned r0, unsigned r1, unsigned r2, unsigned r3, unsigned r4, unsigned r5, unsigned r6)
{
    return (unsigned long long)r0 | (unsigned long long)r1 << 5 | (unsigned long long)r2 << 10 | (unsigned long long)r3 << 15 |
           (unsigned long long)r4 << 20 | (unsigned long long)r5 << 25 | (unsigned long long)r6 << 30;
}
constexpr int kGlyphCount = 37; // a-z, 0-9, '.'
#define FRLW_GLYPH(ch, r0, r1, r2, r3, r4, r5, r6) glyph_bits(r0, r1, r2, r3, r4, r5, r6),
__constant__ unsigned long long kGlyphs[kGlyphCount + 1] = {
#include "render_font.h"
    0ull // blank: every other character
};
#undef FRLW_GLYPH
#define FRLW_GLYPH(ch, r0, r1, r2, r3, r4, r5, r6) ch,
constexpr char kGlyphChars[] = {
#include "render_font.h"
};
#undef FRLW_GLYPH
constexpr int glyph_index_of(unsigned ch)
{
    return ch >= 'a' && ch <= 'z' ? (int)(ch - 'a') : ch >= '0' && ch <= '9' ? 26 + (int)(ch - '0') : ch == '.' ? 36 : kGlyphCount;
}
constexpr bool glyph_order_ok()
{
    for (int i = 0; i < kGlyphCount; ++i)
        if (glyph_index_of((unsigned char)kGlyphChars[i]) != i) return false;
    return true;
}
static_assert(sizeof(kGlyphChars) == kGlyphCount && glyph_order_ok(), "render_font.h: a-z, 0-9, '.' in this order");

// ---- HSV -> BGR: H in units of 2 degrees, float32 inside, each channel x * 255 rounded to nearest-even and
// saturated.  Returns b | g << 8 | r << 16.
__device__ __forceinline__ uint32_t sat_rint_u8(float x)
{
    const float r = rintf(x);
    return r <= 0.0f ? 0u : r >= 255.0f ? 255u : (uint32_t)r;
}
__device__ __forceinline__ uint32_t hsv_to_bgr(uint32_t H, uint32_t S, uint32_t V)
{
    float h = (float)H * (6.0f / 180.0f);
    const float s = (float)S * (1.0f / 255.0f), v = (float)V * (1.0f / 255.0f);
    float b = v, g = v, r = v;
    if (s != 0.0f) {
        while (h < 0.0f) h += 6.0f;
        while (h >= 6.0f) h -= 6.0f;
        const float kf = floorf(h), f = h - kf;
        const int k = (int)kf;
        const float t0 = v, t1 = v * (1.0f - s), t2 = v * (1.0f - s * f), t3 = v * (1.0f - s * (1.0f - f));
        // sector table {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}: two bits per sector and channel, sector 0 lowest
        const uint32_t ib = (0x835u >> (2 * k)) & 3u, ig = (0x583u >> (2 * k)) & 3u, ir = (0x358u >> (2 * k)) & 3u;
        auto pick = [&](uint32_t i) { return i == 0 ? t0 : i == 1 ? t1 : i == 2 ? t2 : t3; };
        b = pick(ib); g = pick(ig); r = pick(ir);
    }
    return sat_rint_u8(b * 255.0f) | sat_rint_u8(g * 255.0f) << 8 | sat_rint_u8(r * 255.0f) << 16;
}

__global__ void k_hsv_to_bgr(const uint8_t *hsv, uint8_t *bgr, long long n)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const uint32_t c = hsv_to_bgr(hsv[3 * i], hsv[3 * i + 1], hsv[3 * i + 2]);
        bgr[3 * i] = (uint8_t)c;
        bgr[3 * i + 1] = (uint8_t)(c >> 8);
        bgr[3 * i + 2] = (uint8_t)(c >> 16);
    }
}

// ---- backgrounds: `vol` points at channel 0 of the pixel's source position, channel c lies c * plane bytes further
__device__ __forceinline__ uint32_t channel_max(const uint8_t *vol, int C, long long plane)
{
    uint32_t m = 0;
    for (int c = 0; c < C; ++c) {
        const uint32_t v = vol[c * plane];
        m = v > m ? v : m;
    }
    return m;
}
// H of the TAF and SAE images: u8(120 * (max / 255)) + 119
__device__ __forceinline__ uint32_t hue_of_max(uint32_t m) { return (uint32_t)(120.0f * ((float)m / 255.0f)) + 119u; }

// numpy's median of an even number C of bytes: the float32 mean of the two middle values.
__device__ __forceinline__ float channel_median(const uint8_t *vol, int C, long long plane)
{
    const int need = C / 2; // the lower middle is the smallest t with count(v <= t) >= C / 2
    int lo = 0;
    for (int step = 128; step >= 1; step >>= 1) { // eight halvings of [0, 255]
        const int mid = lo + step - 1;
        int cnt = 0;
        for (int c = 0; c < C; ++c) cnt += (int)vol[c * plane] <= mid ? 1 : 0;
        if (cnt < need) lo = mid + 1;
    }
    int cnt = 0, above = 255;
    for (int c = 0; c < C; ++c) {
        const int v = vol[c * plane];
        cnt += v <= lo ? 1 : 0;
        above = v > lo && v < above ? v : above;
    }
    const int hi = cnt > need ? lo : above; // the upper middle
    return ((float)lo + (float)hi) / 2.0f;
}

// The same for C <= 16 (every TAF volume this project writes: K <= 8) with ONE read of the pixel's bytes: they are packed into four
// registers, the missing ones as 255 -- the bisection never asks for v <= 255, and as a candidate for the upper middle 255 is
// the default anyway.  *max_out = the largest of the C bytes.
__device__ __forceinline__ int count_le(uint32_t w, int t)
{
    return ((int)(w & 255u) <= t ? 1 : 0) + ((int)(w >> 8 & 255u) <= t ? 1 : 0) + ((int)(w >> 16 & 255u) <= t ? 1 : 0) +
           ((int)(w >> 24) <= t ? 1 : 0);
}
__device__ __forceinline__ int min_above(uint32_t w, int lo, int best)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = (int)(w >> (8 * i) & 255u);
        best = v > lo && v < best ? v : best;
    }
    return best;
}
__device__ __forceinline__ float channel_median16(const uint8_t *vol, int C, long long plane, uint32_t *max_out)
{
    uint32_t w[4] = {~0u, ~0u, ~0u, ~0u}, m = 0; // constant indices after the unroll: registers
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (c < C) {
            const uint32_t v = vol[c * plane];
            m = v > m ? v : m;
            w[c >> 2] = (w[c >> 2] & ~(255u << (8 * (c & 3)))) | v << (8 * (c & 3));
        }
    *max_out = m;
    const int need = C / 2;
    int lo = 0;
    for (int step = 128; step >= 1; step >>= 1) {
        const int mid = lo + step - 1; // <= 254
        if (count_le(w[0], mid) + count_le(w[1], mid) + count_le(w[2], mid) + count_le(w[3], mid) < need) lo = mid + 1;
    }
    const int cnt = count_le(w[0], lo) + count_le(w[1], lo) + count_le(w[2], lo) + count_le(w[3], lo); // lo = 255 counts the padding: hi = lo either way
    const int above = min_above(w[3], lo, min_above(w[2], lo, min_above(w[1], lo, min_above(w[0], lo, 255))));
    const int hi = cnt > need ? lo : above;
    return ((float)lo + (float)hi) / 2.0f;
}

template <int MODE>
__device__ __forceinline__ uint32_t background(const uint8_t *vol, int C, long long plane)
{
    if (MODE == FRLW_RENDER_TAF) {
        uint32_t m;
        float t;
        if (C <= 16) { // workgroup-uniform
            t = channel_median16(vol, C, plane, &m);
        } else {
            m = channel_max(vol, C, plane);
            t = channel_median(vol, C, plane);
        }
        const uint32_t hue = hue_of_max(m);
        t = t / 180.0f * 255.0f;
        t = t > 255.0f ? 255.0f : t;
        return hsv_to_bgr(hue, 255u, (uint32_t)t);
    }
    if (MODE == FRLW_RENDER_SAE) return hsv_to_bgr(hue_of_max(channel_max(vol, C, plane)), 255u, 255u);
    if (MODE == FRLW_RENDER_ECI) {
        const float p = (float)vol[plane] / 255.0f, q = (float)vol[0] / 255.0f;
        const float pp = p > q ? p : 0.0f;
        const float qq = q > pp ? q : 0.0f;
        const float c = pp * 127.0f - qq * 127.0f;
        const uint32_t g = (127u + ((uint32_t)(int)c & 255u)) & 255u; // |c| <= 127: the conversion is exact truncation
        return g | g << 8 | g << 16;
    }
    // FRLW_RENDER_EV: the hue of the first bin that holds the pixel's largest count, its count as V
    const int B = C / 2;
    uint32_t hue = 119u, val = 0u, best = 0u;
    for (int i = 0; i < B; ++i) {
        const uint32_t a = vol[(B + i) * plane], b = vol[i * plane], c = a > b ? a : b;
        if (c > best) { hue = (uint32_t)(239 + 30 * i) & 255u; val = c; best = c; }
    }
    return hsv_to_bgr(hue, 255u, val);
}

// ---- boxes
constexpr uint32_t kColourGt = 0u | 255u << 8 | 149u << 16;   // BGR (0, 255, 149)
constexpr uint32_t kColourDt = 209u | 255u << 8 | 0u << 16;   // BGR (209, 255, 0)
__device__ __forceinline__ int tag_width(uint32_t kind) { return kind ? 75 : 35; }

__device__ __forceinline__ bool glyph_hit(int rx, int ry, unsigned long long chars, int n_chars)
{
    if (rx < 0 || rx >= 6 * n_chars) return false;
    const int ci = rx / 6, cx = rx - 6 * ci;
    if (cx >= 5) return false;
    const unsigned ch = (unsigned)(chars >> (8 * ci)) & 255u;
    return (kGlyphs[glyph_index_of(ch)] >> (5 * ry + 4 - cx)) & 1ull;
}

// One box over one pixel: outline, then tag fill, then glyphs.
__device__ __forceinline__ uint32_t paint(uint32_t px, int x, int y, int x1, int y1, int x2, int y2, uint32_t meta,
                                          unsigned long long label, uint32_t score)
{
    const uint32_t kind = meta & 255u;
    const uint32_t colour = kind ? kColourDt : kColourGt;
    const bool in_box = x >= x1 && x <= x2 && y >= y1 && y <= y2;
    const bool inner = x >= x1 + 2 && x <= x2 - 2 && y >= y1 + 2 && y <= y2 - 2;
    if (in_box && !inner) px = colour;
    if (x >= x1 && x <= x1 + tag_width(kind) && y >= y1 - 15 && y <= y1) {
        px = colour;
        const int ry = y - (y1 - 11);
        if (ry >= 0 && ry < 7) {
            const int n_label = min((int)(meta >> 8 & 255u), 5), n_score = min((int)(meta >> 16 & 255u), 4);
            if (glyph_hit(x - (x1 + 3), ry, label, n_label) || glyph_hit(x - (x1 + 40), ry, (unsigned long long)score, n_score))
                px = 0u;
        }
    }
    return px;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_render(const uint8_t *src, int C, int h, int w, int H, int W, float sh, float sw,
                                                     const uint32_t *boxes, BoxOffsets offs, uint8_t *out)
{
    __shared__ uint4 s_box[FRLW_RENDER_MAX_BOXES * 2];
    __shared__ int s_wave[kThreads / 64];
    const int f = blockIdx.z;
    const int tx0 = blockIdx.x * kRenderTileW, ty0 = blockIdx.y * kRenderTileH;
    const int tx1 = min(tx0 + kRenderTileW, W) - 1, ty1 = min(ty0 + kRenderTileH, H) - 1;
    const int first = offs.v[f], nb = offs.v[f + 1] - first;
    const int wave = threadIdx.x >> 6;

    // the frame's boxes whose footprint meets this tile, in order
    int kept = 0;
    for (int base = 0; base < nb; base += kThreads) {
        const int j = base + (int)threadIdx.x;
        bool hit = false;
        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
        if (j < nb) {
            const uint4 *rec = (const uint4 *)(boxes + (long long)kBoxWords * (first + j));
            lo = rec[0];
            hi = rec[1];
            const int x1 = (int)lo.x, y1 = (int)lo.y, x2 = (int)lo.z, y2 = (int)lo.w;
            const bool box = x1 <= tx1 && x2 >= tx0 && y1 <= ty1 && y2 >= ty0;
            const bool tag = x1 <= tx1 && x1 + tag_width(hi.x & 255u) >= tx0 && y1 - 15 <= ty1 && y1 >= ty0;
            hit = box || tag;
        }
        const unsigned long long m = __ballot(hit);
        if ((threadIdx.x & 63) == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int v = 0; v < kThreads / 64; ++v) {
            const int c = s_wave[v];
            before += v < wave ? c : 0;
            total += c;
        }
        if (hit) {
            const int pos = kept + before + __popcll(m & lanemask_lt());
            s_box[2 * pos] = lo;
            s_box[2 * pos + 1] = hi;
        }
        kept += total;
        __syncthreads(); // the records are visible; s_wave is free for the next round
    }

    const int y = ty0 + (int)(threadIdx.x >> 5), x0 = tx0 + (int)(threadIdx.x & 31) * kPixPerThread;
    if (y >= H || x0 >= W) return; // no barrier below
    const int nvalid = min(kPixPerThread, W - x0);

    uint32_t px[kPixPerThread];
    if (MODE == FRLW_RENDER_BGR) {
        const uint8_t *s = src + 3 * (((long long)f * H + y) * W + x0);
        if (nvalid == kPixPerThread && ((uintptr_t)s & 3) == 0) {
            const uint32_t d0 = ((const uint32_t *)s)[0], d1 = ((const uint32_t *)s)[1], d2 = ((const uint32_t *)s)[2];
            px[0] = d0 & 0xFFFFFFu;
            px[1] = (d0 >> 24 | d1 << 8) & 0xFFFFFFu;
            px[2] = (d1 >> 16 | d2 << 16) & 0xFFFFFFu;
            px[3] = d2 >> 8;
        } else {
#pragma unroll
            for (int i = 0; i < kPixPerThread; ++i)
                px[i] = i < nvalid ? (uint32_t)s[3 * i] | (uint32_t)s[3 * i + 1] << 8 | (uint32_t)s[3 * i + 2] << 16 : 0u;
        }
    } else {
        const long long plane = (long long)h * w;
        const uint8_t *row = src + (long long)f * C * plane + (long long)nearest_src(y, sh, h) * w;
#pragma unroll
        for (int i = 0; i < kPixPerThread; ++i)
            px[i] = i < nvalid ? background<MODE>(row + nearest_src(x0 + i, sw, w), C, plane) : 0u;
    }

    for (int j = 0; j < kept; ++j) {
        const uint4 lo = s_box[2 * j], hi = s_box[2 * j + 1];
        const unsigned long long label = (unsigned long long)hi.y | (unsigned long long)hi.z << 32;
#pragma unroll
        for (int i = 0; i < kPixPerThread; ++i)
            px[i] = paint(px[i], x0 + i, y, (int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, hi.x, label, hi.w);
    }

    uint8_t *o = out + 3 * (((long long)f * H + y) * W + x0);
    if (nvalid == kPixPerThread && ((uintptr_t)o & 3) == 0) {
        ((uint32_t *)o)[0] = px[0] | px[1] << 24;
        ((uint32_t *)o)[1] = px[1] >> 8 | px[2] << 16;
        ((uint32_t *)o)[2] = px[2] >> 16 | px[3] << 8;
    } else { // the ragged right edge, and rows of a width that does not keep them dword-aligned
#pragma unroll
        for (int i = 0; i < kPixPerThread; ++i)
            if (i < nvalid) {
                o[3 * i] = (uint8_t)px[i];
                o[3 * i + 1] = (uint8_t)(px[i] >> 8);
                o[3 * i + 2] = (uint8_t)(px[i] >> 16);
            }
    }
}

template <int MODE>
void launch_render(const uint8_t *src, int n, int C, int h, int w, int H, int W, const frlw_render_box_t *boxes,
                   const BoxOffsets &offs, uint8_t *out, hipStream_t st)
{
    const dim3 grid((unsigned)((W + kRenderTileW - 1) / kRenderTileW), (unsigned)((H + kRenderTileH - 1) / kRenderTileH), (unsigned)n);
    hipLaunchKernelGGL(k_render<MODE>, grid, dim3(kThreads), 0, st, src, C, h, w, H, W, (float)h / (float)H, (float)w / (float)W,
                       (const uint32_t *)boxes, offs, out);
}

} // namespace

extern "C" {

int frlw_render_frames(const uint8_t *src, int n, int C, int h, int w, int mode, int H, int W, const frlw_render_box_t *boxes,
                       const int32_t *box_offsets, uint8_t *out, frlw_stream_t stream)
{
    if (!src || !out || !box_offsets || n < 1 || n > FRLW_RENDER_MAX_FRAMES) return FRLW_ERR_ARG;
    if (C < 1 || h < 1 || w < 1 || H < 1 || W < 1) return FRLW_ERR_ARG;
    if ((H + kRenderTileH - 1) / kRenderTileH > 65535) return FRLW_ERR_ARG; // grid.y
    switch (mode) {
    case FRLW_RENDER_TAF: if (C < 2 || C % 2) return FRLW_ERR_ARG; break;
    case FRLW_RENDER_SAE: break;
    case FRLW_RENDER_ECI: if (C != 2) return FRLW_ERR_ARG; break;
    case FRLW_RENDER_EV: if (C < 2 || C % 2) return FRLW_ERR_ARG; break;
    case FRLW_RENDER_BGR: if (C != 3 || h != H || w != W) return FRLW_ERR_ARG; break;
    default: return FRLW_ERR_ARG;
    }
    BoxOffsets offs;
    if (box_offsets[0] < 0) return FRLW_ERR_ARG;
    for (int i = 0; i <= n; ++i) {
        offs.v[i] = box_offsets[i];
        if (i && (offs.v[i] < offs.v[i - 1] || offs.v[i] - offs.v[i - 1] > FRLW_RENDER_MAX_BOXES)) return FRLW_ERR_ARG;
    }
    for (int i = n + 1; i <= FRLW_RENDER_MAX_FRAMES; ++i) offs.v[i] = offs.v[n];
    if (offs.v[n] > offs.v[0] && (!boxes || ((uintptr_t)boxes & 15))) return FRLW_ERR_ARG; // the records are read as 16-byte halves
    const hipStream_t st = (hipStream_t)stream;
    (void)hipGetLastError(); // stale errors of other libraries
    switch (mode) {
    case FRLW_RENDER_TAF: launch_render<FRLW_RENDER_TAF>(src, n, C, h, w, H, W, boxes, offs, out, st); break;
    case FRLW_RENDER_SAE: launch_render<FRLW_RENDER_SAE>(src, n, C, h, w, H, W, boxes, offs, out, st); break;
    case FRLW_RENDER_ECI: launch_render<FRLW_RENDER_ECI>(src, n, C, h, w, H, W, boxes, offs, out, st); break;
    case FRLW_RENDER_EV: launch_render<FRLW_RENDER_EV>(src, n, C, h, w, H, W, boxes, offs, out, st); break;
    default: launch_render<FRLW_RENDER_BGR>(src, n, C, h, w, H, W, boxes, offs, out, st); break;
    }
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

int frlw_hsv_to_bgr_u8(const uint8_t *hsv, uint8_t *bgr, int64_t n_pixels, frlw_stream_t stream)
{
    if (!hsv || !bgr || n_pixels < 0) return FRLW_ERR_ARG;
    if (n_pixels == 0) return FRLW_OK;
    (void)hipGetLastError(); // stale errors of other libraries
    hipLaunchKernelGGL(k_hsv_to_bgr, dim3(grid_for(n_pixels, 256)), dim3(256), 0, (hipStream_t)stream, hsv, bgr,
                       (long long)n_pixels);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

} // extern "C"
