// Stand-alone check of the host-only half of the per-pixel quadratic forms (glf_fit_factor): built together with host_util.cpp under
// the address and undefined-behaviour sanitizers by `make quad_check`. CPU only; no device, no python.
// Exactly sized heap buffers, so that one element too far is reported, at m = 1, 2, 5, 33 and 70, with and without a penalty: R is
// upper triangular with a positive diagonal, R^T (G + diag(penalty)) R = I, two calls give the same bits, only G's lower triangle
// is read; and every refusal with R untouched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/glf.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// G = I + 0.3 B B^T / m with B uniform in [0, 1): symmetric, condition number below 1.4 + 0.3 m / 3
static std::vector<double> gram_case(unsigned m, uint64_t seed)
{
    std::vector<double> B((size_t)m * m), G((size_t)m * m);
    glf_random_vectors(B.data(), m, m, seed);
    for (unsigned i = 0; i < m; ++i)
        for (unsigned j = 0; j <= i; ++j) {
            double s = 0.0;
            for (unsigned k = 0; k < m; ++k) s += B[(size_t)i * m + k] * B[(size_t)j * m + k];
            G[(size_t)i * m + j] = G[(size_t)j * m + i] = (i == j ? 1.0 : 0.0) + 0.3 * s / m;
        }
    return G;
}

// max |R^T A R - I| with A [m][m]
static double congruence_defect(unsigned m, const std::vector<double> &R, const std::vector<double> &A)
{
    std::vector<double> AR((size_t)m * m, 0.0);
    for (unsigned i = 0; i < m; ++i)
        for (unsigned k = 0; k < m; ++k)
            for (unsigned j = 0; j < m; ++j) AR[(size_t)i * m + j] += A[(size_t)i * m + k] * R[(size_t)k * m + j];
    double worst = 0.0;
    for (unsigned i = 0; i < m; ++i)
        for (unsigned j = 0; j < m; ++j) {
            double s = 0.0;
            for (unsigned k = 0; k < m; ++k) s += R[(size_t)k * m + i] * AR[(size_t)k * m + j];
            worst = std::fmax(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
        }
    return worst;
}

int main()
{
    for (unsigned m : {1u, 2u, 5u, 33u, 70u}) {
        const std::vector<double> G = gram_case(m, 7 + m);
        std::vector<double> pen(m);
        glf_random_vectors(pen.data(), m, 1, 41 + m);
        for (double &x : pen) x = 0.5 * x + 0.01;
        const double tol = 64.0 * m * 0x1p-52 * 40.0;
        for (int with_pen = 0; with_pen < 2; ++with_pen) {
            std::vector<double> M(G), R((size_t)m * m, -9.0), R2((size_t)m * m, -8.0);
            for (unsigned i = 0; with_pen && i < m; ++i) M[(size_t)i * m + i] += pen[i];
            CHECK(glf_fit_factor(m, G.data(), with_pen ? pen.data() : nullptr, R.data()) == GLF_OK);
            CHECK(glf_fit_factor(m, G.data(), with_pen ? pen.data() : nullptr, R2.data()) == GLF_OK);
            CHECK(R == R2);
            for (unsigned i = 0; i < m; ++i) {
                CHECK(R[(size_t)i * m + i] > 0.0);
                for (unsigned j = 0; j < i; ++j) CHECK(R[(size_t)i * m + j] == 0.0);
            }
            CHECK(congruence_defect(m, R, M) <= tol);
            // the strict upper triangle of G is not read (glf_fit_coeffs' rule)
            std::vector<double> lower(G);
            for (unsigned i = 0; i < m; ++i)
                for (unsigned j = i + 1; j < m; ++j) lower[(size_t)i * m + j] = 123.0;
            CHECK(glf_fit_factor(m, lower.data(), with_pen ? pen.data() : nullptr, R2.data()) == GLF_OK);
            CHECK(R == R2);
        }
    }
    {   // a singular G made definite by the penalty alone
        const unsigned m = 3;
        const std::vector<double> zero((size_t)m * m, 0.0), pen{4.0, 0.25, 1.0};
        std::vector<double> R((size_t)m * m, -9.0);
        CHECK(glf_fit_factor(m, zero.data(), pen.data(), R.data()) == GLF_OK);
        CHECK(R[0] == 0.5 && R[4] == 2.0 && R[8] == 1.0 && R[1] == 0.0 && R[2] == 0.0 && R[5] == 0.0);
    }
    {   // refusals: R stays as it was
        const unsigned m = 5;
        const std::vector<double> G = gram_case(m, 3), pen(m, 0.1);
        std::vector<double> R((size_t)m * m, -7.0);
        std::vector<double> nanG(G), infG(G), indef(G), zero((size_t)m * m, 0.0), nanpen(pen), infpen(pen), negpen(pen);
        nanG[7] = NAN;
        infG[(size_t)m * m - 1] = INFINITY;
        indef[(size_t)3 * m + 3] = -1.0;
        nanpen[2] = NAN;
        infpen[4] = INFINITY;
        negpen[1] = -100.0;
        CHECK(glf_fit_factor(m, nullptr, pen.data(), R.data()) == GLF_ERR_INVALID);
        CHECK(glf_fit_factor(m, G.data(), pen.data(), nullptr) == GLF_ERR_INVALID);
        CHECK(glf_fit_factor(0, G.data(), pen.data(), R.data()) == GLF_ERR_INVALID);
        CHECK(glf_fit_factor(m, nanG.data(), pen.data(), R.data()) == GLF_ERR_INVALID);
        CHECK(glf_fit_factor(m, infG.data(), nullptr, R.data()) == GLF_ERR_INVALID);
        CHECK(glf_fit_factor(m, indef.data(), pen.data(), R.data()) == GLF_ERR_INVALID);
        CHECK(glf_fit_factor(m, zero.data(), nullptr, R.data()) == GLF_ERR_INVALID);
        CHECK(glf_fit_factor(m, G.data(), nanpen.data(), R.data()) == GLF_ERR_INVALID);
        CHECK(glf_fit_factor(m, G.data(), infpen.data(), R.data()) == GLF_ERR_INVALID);
        CHECK(glf_fit_factor(m, G.data(), negpen.data(), R.data()) == GLF_ERR_INVALID);
        for (double x : R) CHECK(x == -7.0);
    }
    if (failures) {
        std::fprintf(stderr, "quad_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("quad_host_check: ok\n");
    return 0;
}
