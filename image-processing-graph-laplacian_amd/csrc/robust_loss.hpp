// robust_loss.hpp -- the robust losses of the IRLS fit (graph_robust.hip) as functions of q = r^2 in f64: the multiplier
// u = psi(r) / r and the loss rho. Compiled into host_util.cpp (glf_robust_weight, the reference of the tests) and into the kernel's
// translation unit: k_graph_residual_weight forms its loss sum with the rho below.
#pragma once
#include <cmath>

#if defined(__HIP__) || defined(__CUDACC__)
#define GLF_ROBUST_HD __host__ __device__
#else
#define GLF_ROBUST_HD
#endif

namespace glf {

enum { ROBUST_HUBER = 0, ROBUST_CAUCHY = 1, ROBUST_TUKEY = 2, ROBUST_KINDS = 3 }; // = GLF_ROBUST_* (asserted in host_util.cpp)

// the tuning constant at which the estimator keeps 95 % efficiency under Gaussian noise
inline double robust_default_c(int kind) { return kind == ROBUST_HUBER ? 1.345 : kind == ROBUST_CAUCHY ? 2.385 : 4.685; }

GLF_ROBUST_HD inline double robust_u(int kind, double c, double q)
{
#ifdef __clang__
#pragma clang fp contract(off) // host and device round the same operations
#endif
    const double c2 = c * c;
    if (kind == ROBUST_HUBER) return q <= c2 ? 1.0 : c / sqrt(q);
    if (kind == ROBUST_CAUCHY) return 1.0 / (1.0 + q / c2);
    const double t = q / c2;
    return t < 1.0 ? (1.0 - t) * (1.0 - t) : 0.0;
}

GLF_ROBUST_HD inline double robust_rho(int kind, double c, double q)
{
#ifdef __clang__
#pragma clang fp contract(off) // host and device round the same operations
#endif
    const double c2 = c * c;
    if (kind == ROBUST_HUBER) return q <= c2 ? 0.5 * q : c * sqrt(q) - 0.5 * c2;
    if (kind == ROBUST_CAUCHY) return 0.5 * c2 * log1p(q / c2);
    const double t = q / c2, v = 1.0 - (t < 1.0 ? t : 1.0);
    return c2 / 6.0 * (1.0 - v * v * v);
}

} // namespace glf
