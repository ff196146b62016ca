// filter_rule.hpp -- the spectral filter z = ident y + gain Phi f(Pi) Phi^T y as a rule on the host, in f64: the response f per
// eigenvalue, the gain, the identity term and the sharpening weights. The whole-path driver (pipeline.hip) forms its filter
// weights with it and glf_filter_coeffs (graph.hip) its coefficients.
//   reference: z = y + gain Phi Pi^k Phi^T y (MatPow is a no-op there, hpc/utils.c:721 => k = 1);
//   PoC: z = y - Phi diag(mu + 5) Phi^T y (python/image_processing.py:304-305);
//   smoothing / sharpening (:197-241): z = Phi f(s) Phi^T y with s = 1 - mu the eigenvalues of W = I - L, f(s) = s or
//   (1 + beta) s^2 - beta s^3 -- no y term (the kernels subtract y from the correction: ysub = 1 - ident).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/glf.h"

namespace glf {

inline float filter_gain(const glf_options &opt) { return opt.filter_mode == GLF_FILTER_REFERENCE ? opt.gain : 1.0f; }
inline float filter_ident(const glf_options &opt) { return opt.filter_mode >= GLF_FILTER_SMOOTH ? 0.0f : 1.0f; }

// f(lambda) of the three diagonal modes (sharpening is not diagonal: sharpen_weights)
inline double filter_response(const glf_options &opt, double lambda)
{
    switch (opt.filter_mode) {
    case GLF_FILTER_POC: return -(lambda + 5.0);
    case GLF_FILTER_SMOOTH: return 1.0 - lambda;
    default: return std::pow(lambda, (double)(opt.filter_pow > 0 ? opt.filter_pow : 1));
    }
}

// Sharpening: (1 + beta) W^2 y - beta W^3 y with W = Phi L Phi^T applied factor by factor as the PoC does
// (python/image_processing.py:231-235): the extended eigenvectors are not orthonormal, so G = Phi^T Phi (rows of ldG doubles) sits
// between the factors -- out = (1 + beta) L G L c - beta L G L G L c, L = 1 - lambda, c = Phi^T y; the sums over j ascending.
inline void sharpen_weights(unsigned m, const double *lambda, const double *G, size_t ldG, double beta, const double *c, double *out)
{
    std::vector<double> t(m), u(m), v(m);
    auto LG = [&](const std::vector<double> &x, std::vector<double> &y) { // y = L (G x)
        for (unsigned i = 0; i < m; ++i) {
            double a = 0.0;
            for (unsigned j = 0; j < m; ++j) a += G[i * ldG + j] * x[j];
            y[i] = (1.0 - lambda[i]) * a;
        }
    };
    for (unsigned j = 0; j < m; ++j) t[j] = (1.0 - lambda[j]) * c[j];
    LG(t, u);
    LG(u, v);
    for (unsigned j = 0; j < m; ++j) out[j] = (1.0 + beta) * u[j] - beta * v[j];
}

// one row of the driver's filter weights: w[j] = fl32(f(lambda_j) c[j]), or the sharpening weights
inline void filter_weights_row(const glf_options &opt, unsigned m, const double *lambda, const double *G, size_t ldG, const double *c, float *w)
{
    if (opt.filter_mode == GLF_FILTER_SHARPEN) {
        std::vector<double> a(m);
        sharpen_weights(m, lambda, G, ldG, (double)opt.filter_beta, c, a.data());
        for (unsigned j = 0; j < m; ++j) w[j] = (float)a[j];
    } else {
        for (unsigned j = 0; j < m; ++j) w[j] = (float)(filter_response(opt, lambda[j]) * c[j]);
    }
}

} // namespace glf
