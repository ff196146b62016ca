// Stand-alone check of the host-only half of the robust fit (glf_robust_weight, glf_robust_scale): built together with
// host_util.cpp under the address and undefined-behaviour sanitizers by `make robust_check`. CPU only; no device, no python.
// It checks the table of the three losses at its branch points (q = c^2 one ulp below and above, q = 0, huge q), the median rule on
// even and odd counts and with zero weights, on exactly sized heap buffers so that one element too far is reported, and every refusal
// with the outputs untouched.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

static bool close_to(double got, double want) { return std::fabs(got - want) <= 8 * std::numeric_limits<double>::epsilon() * std::fabs(want); }

// the table restated, r = sqrt(q)
static void table(int kind, double c, double q, double *u, double *rho)
{
    const double c2 = c * c, r = std::sqrt(q);
    if (kind == GLF_ROBUST_HUBER) {
        *u = r <= c ? 1.0 : c / r;
        *rho = r <= c ? q / 2 : c * r - c2 / 2;
    } else if (kind == GLF_ROBUST_CAUCHY) {
        *u = 1.0 / (1.0 + q / c2);
        *rho = c2 / 2 * std::log1p(q / c2);
    } else {
        const double t = q < c2 ? q / c2 : 1.0;
        *u = (1 - t) * (1 - t);
        *rho = c2 / 6 * (1 - (1 - t) * (1 - t) * (1 - t));
    }
}

int main()
{
    const double defaults[3] = {1.345, 2.385, 4.685};
    for (int kind = 0; kind < 3; ++kind)
        for (double c : {0.0, 0.5, 1.0, 3.0, 1e-6, 1e18}) {
            const double cc = c == 0.0 ? defaults[kind] : c, c2 = cc * cc;
            const double below = std::nextafter(c2, 0.0), above = std::nextafter(c2, INFINITY);
            for (double q : {0.0, below, c2, above, 0.25 * c2, 4.0 * c2, 1e200}) {
                double u = -1.0, rho = -1.0, wu, wrho;
                CHECK(glf_robust_weight(kind, c, q, &u, &rho) == GLF_OK);
                table(kind, cc, q, &wu, &wrho);
                // (near q = c^2 Tukey's u is (1 - t)^2 with t within an ulp of 1: compare on the scale of 1)
                CHECK(std::fabs(u - wu) <= 1e-15 && (close_to(rho, wrho) || std::fabs(rho - wrho) <= 1e-15 * c2));
                CHECK(u >= 0.0 && u <= 1.0 && rho >= 0.0);
                double only_u = -1.0, only_rho = -1.0;
                CHECK(glf_robust_weight(kind, c, q, &only_u, nullptr) == GLF_OK && only_u == u);
                CHECK(glf_robust_weight(kind, c, q, nullptr, &only_rho) == GLF_OK && only_rho == rho);
            }
            double u = -1.0, rho = -1.0;
            // the branch points themselves
            CHECK(glf_robust_weight(kind, c, 0.0, &u, &rho) == GLF_OK && u == 1.0 && rho == 0.0);
            CHECK(glf_robust_weight(kind, c, c2, &u, &rho) == GLF_OK);
            if (kind == GLF_ROBUST_HUBER) CHECK(u == 1.0 && rho == 0.5 * c2);
            if (kind == GLF_ROBUST_CAUCHY) CHECK(u == 0.5);
            if (kind == GLF_ROBUST_TUKEY) CHECK(u == 0.0 && rho == c2 / 6.0);
            CHECK(glf_robust_weight(kind, c, below, &u, &rho) == GLF_OK);
            if (kind == GLF_ROBUST_HUBER) CHECK(u == 1.0);
            if (kind == GLF_ROBUST_TUKEY) CHECK(u >= 0.0 && u < 1e-30);
            CHECK(glf_robust_weight(kind, c, above, &u, &rho) == GLF_OK);
            if (kind == GLF_ROBUST_HUBER) CHECK(u <= 1.0 && u > 1.0 - 1e-15);
            if (kind == GLF_ROBUST_TUKEY) CHECK(u == 0.0 && rho == c2 / 6.0);
            CHECK(glf_robust_weight(kind, c, 1e200, &u, &rho) == GLF_OK && std::isfinite(rho));
            if (kind == GLF_ROBUST_TUKEY) CHECK(u == 0.0);
            else CHECK(u >= 0.0 && u < 1e-100 * (1.0 + c2));
        }
    {   // refusals: outputs untouched
        double u = -3.0, rho = -4.0;
        CHECK(glf_robust_weight(-1, 1.0, 1.0, &u, &rho) == GLF_ERR_INVALID);
        CHECK(glf_robust_weight(3, 1.0, 1.0, &u, &rho) == GLF_ERR_INVALID);
        CHECK(glf_robust_weight(GLF_ROBUST_HUBER, -1.0, 1.0, &u, &rho) == GLF_ERR_INVALID);
        CHECK(glf_robust_weight(GLF_ROBUST_HUBER, INFINITY, 1.0, &u, &rho) == GLF_ERR_INVALID);
        CHECK(glf_robust_weight(GLF_ROBUST_CAUCHY, NAN, 1.0, &u, &rho) == GLF_ERR_INVALID);
        CHECK(glf_robust_weight(GLF_ROBUST_TUKEY, 1.0, -1e-300, &u, &rho) == GLF_ERR_INVALID);
        CHECK(glf_robust_weight(GLF_ROBUST_TUKEY, 1.0, NAN, &u, &rho) == GLF_ERR_INVALID);
        CHECK(u == -3.0 && rho == -4.0);
        CHECK(glf_robust_weight(GLF_ROBUST_HUBER, 1.0, 1.0, nullptr, nullptr) == GLF_OK);
    }
    {   // the median rule: element floor((cnt - 1) / 2) of the ascending |res|
        double sigma = -1.0;
        const std::vector<double> odd{-5.0, 1.0, 3.0, -2.0, 4.0};            // |.| ascending 1 2 3 4 5 -> 3
        CHECK(glf_robust_scale(odd.data(), nullptr, odd.size(), &sigma) == GLF_OK && sigma == 1.4826 * 3.0);
        const std::vector<double> even{-5.0, 1.0, 3.0, -2.0, 4.0, 6.0};      // 1 2 3 4 5 6 -> element 2 = 3 (the lower median)
        CHECK(glf_robust_scale(even.data(), nullptr, even.size(), &sigma) == GLF_OK && sigma == 1.4826 * 3.0);
        const std::vector<double> two{7.0, -2.0};
        CHECK(glf_robust_scale(two.data(), nullptr, 2, &sigma) == GLF_OK && sigma == 1.4826 * 2.0);
        const std::vector<double> one{-0.5};
        CHECK(glf_robust_scale(one.data(), nullptr, 1, &sigma) == GLF_OK && sigma == 1.4826 * 0.5);
        // zero and negative weights drop their entries: 5 1 . 2 . 6 -> 1 2 5 6 -> element 1 = 2
        const std::vector<double> w{1.0, 0.5, 0.0, 2.0, -1.0, 1e-300};
        CHECK(glf_robust_scale(even.data(), w.data(), even.size(), &sigma) == GLF_OK && sigma == 1.4826 * 2.0);
        const std::vector<double> w1{0.0, 0.0, 0.0, 0.0, 0.0, 3.0};
        CHECK(glf_robust_scale(even.data(), w1.data(), even.size(), &sigma) == GLF_OK && sigma == 1.4826 * 6.0);
        // a larger, exactly sized buffer against a sort
        std::vector<double> big(1001), ww(1001);
        for (size_t i = 0; i < big.size(); ++i) {
            big[i] = (double)((i * 7919) % 1009) - 504.0;
            ww[i] = (double)(i % 3);
        }
        std::vector<double> kept;
        for (size_t i = 0; i < big.size(); ++i)
            if (ww[i] > 0.0) kept.push_back(std::fabs(big[i]));
        std::sort(kept.begin(), kept.end());
        CHECK(glf_robust_scale(big.data(), ww.data(), big.size(), &sigma) == GLF_OK && sigma == 1.4826 * kept[(kept.size() - 1) / 2]);
    }
    {   // refusals: sigma untouched
        double sigma = -9.0;
        const std::vector<double> res{1.0, 2.0, 3.0}, zeros{0.0, 0.0, 5.0}, w0{0.0, 0.0, 0.0}, wneg{-1.0, 0.0, -2.0};
        const std::vector<double> bad{1.0, NAN, 3.0}, inf{1.0, INFINITY, 3.0}, wbad{1.0, NAN, 1.0}, winf{1.0, INFINITY, 1.0};
        CHECK(glf_robust_scale(nullptr, nullptr, 3, &sigma) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(res.data(), nullptr, 3, nullptr) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(res.data(), nullptr, 0, &sigma) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(res.data(), w0.data(), 3, &sigma) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(res.data(), wneg.data(), 3, &sigma) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(bad.data(), nullptr, 3, &sigma) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(inf.data(), nullptr, 3, &sigma) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(bad.data(), w0.data(), 3, &sigma) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(res.data(), wbad.data(), 3, &sigma) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(res.data(), winf.data(), 3, &sigma) == GLF_ERR_INVALID);
        CHECK(glf_robust_scale(zeros.data(), nullptr, 3, &sigma) == GLF_ERR_INVALID); // the median is 0
        CHECK(sigma == -9.0);
    }
    if (failures) {
        std::fprintf(stderr, "robust_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("robust_host_check: ok\n");
    return 0;
}
