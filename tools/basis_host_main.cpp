// Stand-alone check of the host-only half of the change of basis (glf_basis_orthonormal): built together with host_util.cpp under
// the address and undefined-behaviour sanitizers by `make basis_check`. CPU only; no device, no python.
// Exactly sized heap buffers, so that one element too far is reported, at m = 1, 2, 5, 33 and 70; both modes; the identities
// T^T G T = I and T diag(1 - lam_new) T^T = diag(1 - lam); the order, the sign rule, two calls with the same bits, a tie of equal
// eigenvalues, and every refusal with its outputs untouched.
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

// max |T^T A T - diag(d)| with A [m][m]
static double congruence_defect(unsigned m, const std::vector<double> &T, const std::vector<double> &A, const std::vector<double> &d)
{
    std::vector<double> AT((size_t)m * m, 0.0);
    for (unsigned i = 0; i < m; ++i)
        for (unsigned k = 0; k < m; ++k)
            for (unsigned j = 0; j < m; ++j) AT[(size_t)i * m + j] += A[(size_t)i * m + k] * T[(size_t)k * m + j];
    double worst = 0.0;
    for (unsigned i = 0; i < m; ++i)
        for (unsigned j = 0; j < m; ++j) {
            double s = 0.0;
            for (unsigned k = 0; k < m; ++k) s += T[(size_t)k * m + i] * AT[(size_t)k * m + j];
            worst = std::fmax(worst, std::fabs(s - (i == j ? d[i] : 0.0)));
        }
    return worst;
}

int main()
{
    for (unsigned m : {1u, 2u, 5u, 33u, 70u}) {
        const std::vector<double> G = gram_case(m, 7 + m);
        std::vector<double> lam(m), ones(m, 1.0);
        glf_random_vectors(lam.data(), m, 1, 99 + m);
        for (double &x : lam) x = 0.6 + 0.5 * x;
        const double tol = 64.0 * m * 0x1p-52 * 40.0;
        {   // Cholesky mode: upper triangular, positive diagonal, T^T G T = I; lam_new may be NULL
            std::vector<double> T((size_t)m * m, -9.0), T2((size_t)m * m, -8.0);
            CHECK(glf_basis_orthonormal(m, G.data(), nullptr, T.data(), nullptr) == GLF_OK);
            CHECK(glf_basis_orthonormal(m, G.data(), nullptr, T2.data(), nullptr) == GLF_OK);
            CHECK(T == T2);
            for (unsigned i = 0; i < m; ++i) {
                CHECK(T[(size_t)i * m + i] > 0.0);
                for (unsigned j = 0; j < i; ++j) CHECK(T[(size_t)i * m + j] == 0.0);
            }
            CHECK(congruence_defect(m, T, G, ones) <= tol);
        }
        {   // Ritz mode
            std::vector<double> T((size_t)m * m, -9.0), T2((size_t)m * m, -8.0), ln(m, -9.0), ln2(m, -8.0);
            CHECK(glf_basis_orthonormal(m, G.data(), lam.data(), T.data(), ln.data()) == GLF_OK);
            CHECK(glf_basis_orthonormal(m, G.data(), lam.data(), T2.data(), ln2.data()) == GLF_OK);
            CHECK(T == T2 && ln == ln2);
            for (unsigned j = 1; j < m; ++j) CHECK(ln[j - 1] <= ln[j]);
            CHECK(congruence_defect(m, T, G, ones) <= tol);
            // T diag(1 - lam_new) T^T = diag(1 - lam), as a congruence of T^T
            std::vector<double> Tt((size_t)m * m), D((size_t)m * m, 0.0), want(m);
            for (unsigned i = 0; i < m; ++i) {
                D[(size_t)i * m + i] = 1.0 - ln[i];
                want[i] = 1.0 - lam[i];
                for (unsigned j = 0; j < m; ++j) Tt[(size_t)i * m + j] = T[(size_t)j * m + i];
            }
            CHECK(congruence_defect(m, Tt, D, want) <= tol);
        }
    }
    {   // G = I with equal eigenvalues: every theta ties, so the order is the original one and T = I
        const unsigned m = 4;
        std::vector<double> G((size_t)m * m, 0.0), T((size_t)m * m, -9.0), ln(m, -9.0);
        const std::vector<double> lam(m, 0.75);
        for (unsigned i = 0; i < m; ++i) G[(size_t)i * m + i] = 1.0;
        CHECK(glf_basis_orthonormal(m, G.data(), lam.data(), T.data(), ln.data()) == GLF_OK);
        for (unsigned i = 0; i < m; ++i) {
            CHECK(ln[i] == 0.75);
            for (unsigned j = 0; j < m; ++j) CHECK(T[(size_t)i * m + j] == (i == j ? 1.0 : 0.0));
        }
        // orthonormal already, eigenvalues unsorted: a permutation, ascending
        const std::vector<double> mixed{0.9, 0.7, 1.05, 0.8};
        CHECK(glf_basis_orthonormal(m, G.data(), mixed.data(), T.data(), ln.data()) == GLF_OK);
        CHECK(ln[0] == 1.0 - (1.0 - 0.7) && ln[1] == 1.0 - (1.0 - 0.8) && ln[2] == 1.0 - (1.0 - 0.9) && ln[3] == 1.0 - (1.0 - 1.05));
        CHECK(T[1 * m + 0] == 1.0 && T[3 * m + 1] == 1.0 && T[0 * m + 2] == 1.0 && T[2 * m + 3] == 1.0);
    }
    {   // refusals: the outputs stay as they were
        const unsigned m = 5;
        const std::vector<double> G = gram_case(m, 3), lam(m, 0.8);
        std::vector<double> T((size_t)m * m, -7.0), ln(m, -7.0);
        std::vector<double> nanG(G), infG(G), indef(G), zero((size_t)m * m, 0.0), nanlam(lam);
        nanG[7] = NAN;
        infG[(size_t)m * m - 1] = INFINITY;
        indef[(size_t)3 * m + 3] = -1.0;
        nanlam[2] = NAN;
        CHECK(glf_basis_orthonormal(m, nullptr, lam.data(), T.data(), ln.data()) == GLF_ERR_INVALID);
        CHECK(glf_basis_orthonormal(m, G.data(), lam.data(), nullptr, ln.data()) == GLF_ERR_INVALID);
        CHECK(glf_basis_orthonormal(m, G.data(), lam.data(), T.data(), nullptr) == GLF_ERR_INVALID);
        CHECK(glf_basis_orthonormal(0, G.data(), lam.data(), T.data(), ln.data()) == GLF_ERR_INVALID);
        CHECK(glf_basis_orthonormal(m, nanG.data(), lam.data(), T.data(), ln.data()) == GLF_ERR_INVALID);
        CHECK(glf_basis_orthonormal(m, infG.data(), nullptr, T.data(), nullptr) == GLF_ERR_INVALID);
        CHECK(glf_basis_orthonormal(m, indef.data(), lam.data(), T.data(), ln.data()) == GLF_ERR_INVALID);
        CHECK(glf_basis_orthonormal(m, zero.data(), nullptr, T.data(), nullptr) == GLF_ERR_INVALID);
        CHECK(glf_basis_orthonormal(m, G.data(), nanlam.data(), T.data(), ln.data()) == GLF_ERR_INVALID);
        for (double x : T) CHECK(x == -7.0);
        for (double x : ln) CHECK(x == -7.0);
    }
    if (failures) {
        std::fprintf(stderr, "basis_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("basis_host_check: ok\n");
    return 0;
}
