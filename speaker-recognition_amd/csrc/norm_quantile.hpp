// norm_quantile.hpp -- the inverse of the standard normal distribution function in float64: Wichura's algorithm AS241, routine
// PPND16 (Applied Statistics 37 (1988) 477-484; relative accuracy about 1e-16).  One definition for both sides: featnorm.hip
// evaluates it on the device (per output, or once per table entry), sr_norm_quantile is its host instance.  It is the algorithm of
// Python's statistics.NormalDist().inv_cdf, which the tests' oracle uses; the Horner chains are written out operation by operation
// (the files that include this header are built without floating-point contraction).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define SR_NQ_HD __host__ __device__
#else
#define SR_NQ_HD
#endif

namespace sr {

// 0 < p < 1; anything else gives NaN
SR_NQ_HD inline double norm_quantile(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                              1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                              4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    if (!(p > 0.0 && p < 1.0)) return NAN;
    double r = q <= 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    double num, den;
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                   1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                   1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                 2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                   2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                   7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                 5.99832206555887937690e-1) * r + 1.0);
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

// The warped value of the doubled mid-rank r2 in 0 .. 2 N - 2: the quantile of (r2 + 1) / (2 N), taken through the lower half of
// the distribution -- a = r2 + 1 above N gives -quantile((2 N - a) / (2 N)), a == N gives 0 -- so that mirrored ranks give values
// that are each other's negatives to the bit (quantile(1 - p) rounds 1 - p first, and would not).
SR_NQ_HD inline double warp_value(int r2, int N) {
    const int a = r2 + 1, M = 2 * N;
    if (a == N) return 0.0;
    if (a < N) return norm_quantile((double)a / (double)M);
    return -norm_quantile((double)(M - a) / (double)M);
}

}  // namespace sr
