// leaky.h -- uint8(leaky_transform(.)) as a 256-level step function: the exact routine, the threshold and bucket look-ups, the table's layout.
// Expects frlw_common.h above it (f32_to_u8, the HIP runtime); frlw_common.h includes it.  leaky.hip builds the per-device table.
#pragma once

namespace frlw {
__device__ __forceinline__ float leaky_f(float v)
{
    float l = log1pf(-v);   // generate_taf.py:72
    l = 1.0f - l / 8.7f;    // :73
    if (l < 0.0f) l = 0.0f; // :74
    return l * 255.0f;      // :75
}

// uint8(leaky_transform(v)) is a non-increasing step function of x = -v >= 0 with at most 256 levels.
// thr[k] (k = 1..255) = bit pattern of the largest x with uint8(leaky_f(-x)) >= k, found by bisection on the
// SAME f32 pipeline (k_leaky_fill, leaky.hip); thr[0] = +inf.  The lookup below returns
// exactly what evaluating leaky_f would, for ~10 instructions instead of a log1pf per value.
constexpr int kLeakyLevels = 256;

__device__ __forceinline__ uint32_t leaky_threshold_bits(int k)
{
    uint32_t lo = 0u, hi = 0x7f000000u; // f(0) = 255 >= k always; f(huge) = 0
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((int)leaky_f(-__uint_as_float(mid)) >= k) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint8_t leaky_u8_lookup(float v, const uint32_t *thr)
{
    if (!(v <= 0.0f)) return f32_to_u8(leaky_f(v)); // outside the table's domain (events after the last window)
    const float x = fabsf(v); // v <= 0 here; fabsf also maps +0 to +0 (-(+0) = -0 would compare as a huge bit pattern)
    const uint32_t xb = __float_as_uint(x);
    // first guess from the hardware log2 (1 ulp-ish), then walk to the exact level
    float g = 255.0f * (1.0f - (__log2f(1.0f + x) * 0.69314718f) / 8.7f);
    int k = g < 0.0f ? 0 : (g > 255.0f ? 255 : (int)g);
    while (k < 255 && xb <= thr[k + 1]) ++k;
    while (k > 0 && xb > thr[k]) --k;
    return (uint8_t)k;
}

// The 256 thresholds are a constant of the device's f32 pipeline: built ONCE per device and process (leaky.hip) into a
// device-resident table, on the stream of the first encoder call; calls on other streams wait for that fill through an
// event until it has completed (no host synchronisation; inside a stream capture the fill becomes a node of the graph).
// nullptr: a HIP call failed.
const uint32_t *leaky_table(hipStream_t s);

// Out-of-line on purpose: it is the rare path of the batched look-up below, which would otherwise inline
// N copies of log1pf per cell.
__device__ __noinline__ uint8_t leaky_u8_exact(float v, const uint32_t *thr) { return leaky_u8_lookup(v, thr); }

// N look-ups at once: the first guess is off by at most one level, so thr[k] and thr[k + 1] decide it; both
// are read for all N values before any is used.  The (rare) values the pair does not pin down, and those
// outside the table's domain, take the exact scalar routine.
template <int N>
__device__ __forceinline__ void leaky_u8_lookup_n(const float (&v)[N], const uint32_t *thr, uint8_t (&out)[N])
{
    int k[N];
    uint32_t t0[N], t1[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float x = fabsf(v[i]);
        // first guess only (the table pair below decides): multiply instead of the exact routine's divide
        const float g = 255.0f - (__log2f(1.0f + x) * (255.0f * 0.69314718f / 8.7f));
        k[i] = g > 0.0f ? (g > 254.0f ? 254 : (int)g) : 0; // k + 1 stays inside the table
    }
#pragma unroll
    for (int i = 0; i < N; ++i) { t0[i] = thr[k[i]]; t1[i] = thr[k[i] + 1]; }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const uint32_t xb = __float_as_uint(fabsf(v[i]));
        // level k exactly: thr[k + 1] < x <= thr[k]  (thr[0] = +inf)
        out[i] = (uint8_t)k[i];
        if (!(v[i] <= 0.0f && xb > t1[i] && xb <= t0[i])) out[i] = leaky_u8_exact(v[i], thr);
    }
}

// The same step function through a bucket table (kf_taf_walk): the level changes by 20.3 per octave of 1 + x at most, so a bucket
// of 1/32 octave of x (the float's exponent and five mantissa bits) holds at most ONE threshold.  lut[b] = the level at the
// bucket's upper end; the level of x is lut[b] + (x <= thr[lut[b] + 1]): one byte and one word from LDS, a compare and an add --
// no transcendental, no first guess to repair.  Buckets start at 2^-6 (everything below shares bucket 0: level 254, or 255 for
// x <= thr[255], which the compare decides; thr[255] is not 0 but 2.5928e-7 on gfx950, bits 0x348b3334: below it 1 - l / 8.7
// rounds to 1) and end at 2^13 (level 0 from 6002 on).  k_leaky_fill builds lut[] from thr[] itself and
// CHECKS the one-threshold property for every bucket on the device's own table (word kLeakyOkWord); a device whose log1pf broke
// it would take the exact routine for every value.
constexpr int kLeakyBucketShift = 18;                         // 5 mantissa bits
constexpr int kLeakyBucket0 = (127 - 6) << 5;                 // bits(2^-6) >> 18
constexpr int kLeakyBuckets = ((127 + 13) << 5) - kLeakyBucket0; // 608
constexpr int kLeakyLutWord = kLeakyLevels;                   // lut bytes, four per word, behind the 256 thresholds
constexpr int kLeakyOkWord = kLeakyLutWord + kLeakyBuckets / 4;
constexpr int kLeakyTableWords = kLeakyOkWord + 1;            // 409 words: what leaky_table() points at

template <int N>
__device__ __forceinline__ void leaky_u8_bucket_n(const float (&v)[N], const uint32_t *tab, uint8_t (&out)[N])
{
    const uint8_t *lut = (const uint8_t *)(tab + kLeakyLutWord);
    const bool lut_ok = tab[kLeakyOkWord] != 0u; // (uniform)
    uint32_t xb[N], k[N], t1[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        xb[i] = __float_as_uint(fabsf(v[i]));
        int b = (int)(xb[i] >> kLeakyBucketShift) - kLeakyBucket0;
        b = b < 0 ? 0 : (b > kLeakyBuckets - 1 ? kLeakyBuckets - 1 : b);
        k[i] = lut[b];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) t1[i] = tab[k[i] + 1u];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        out[i] = (uint8_t)(k[i] + (xb[i] <= t1[i] ? 1u : 0u));
        if (!(v[i] <= 0.0f) || !lut_ok) out[i] = leaky_u8_exact(v[i], tab); // outside the table's domain (rare), or no valid lut
    }
}
} // namespace frlw
