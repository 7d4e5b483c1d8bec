// taf_mean.h -- the mean of one TAF cell and window, sum / ((float)n + 1e-8f) (generate_taf.py:27), without the division: for the
// small counts of kf_taf_walk the reciprocal comes from a table and the correctly rounded quotient from one product and two FMAs.
// No HIP header, no HIP type: tests/host/walk_mean_check.cpp includes this file into a host program and compares every input the
// walk can produce (and far more) bit for bit against the division (profiles/walk_mean_sweep.txt).
#pragma once

#ifndef FRLW_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRLW_HD __host__ __device__
#else
#define FRLW_HD
#endif
#endif

namespace frlw {
// Counts below kMeanTab take the table; a wavefront that holds a larger one divides (fifo_mean, taf_fifo.h).
constexpr int kMeanTab = 64;

// Entry n of the table: R[0] = +0 (a cell without records has sum = +0, and +0 / 1e-8f = +0), R[n] = RN(1 / n) behind it.
FRLW_HD inline float mean_recip_entry(int n) { return n > 0 ? 1.0f / (float)n : 0.0f; }

// RN(sum / nf) from R = RN(1 / nf), for nf = (float)n with 1 <= n < kMeanTab -- where (float)n + 1e-8f == (float)n, so this IS
// the reference's quotient -- and for n = 0 with sum = +-0:
//   q  = RN(sum * R)                  within one ulp of the quotient
//   r  = q * nf - sum                 exact in one FMA (the negated residual: no rounding, |r| < ulp(q) * nf)
//   q' = RN(q - r * R)                Markstein's correction step: the correctly rounded quotient
// The FMAs are explicit (the build has -ffp-contract=off, which only stops the compiler from contracting on its own).  The
// residual is kept NEGATED and negated again in the last step, which costs nothing (operand modifiers) and keeps the sign of a
// zero: an exact quotient leaves r = +0, and q - (+0) * R = q + (-0) = q also for q = -0, where q + (+0) * R would give +0.
FRLW_HD inline float mean_by_recip(float sum, float nf, float R)
{
    const float q = sum * R;
    const float r = __builtin_fmaf(q, nf, -sum);
    return __builtin_fmaf(-r, R, q);
}
} // namespace frlw
