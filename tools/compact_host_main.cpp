// Stand-alone check of the host-only half of the compact graph handle (csrc/phi_compact.hpp: the exponent rule of a column and the
// folding of the column scales): built together with host_util.cpp under the address and undefined-behaviour sanitizers by
// `make compact_check`. CPU only; no device, no python.
// It checks the rule at its edges (a zero column, max_c at a power of two and one ulp to either side, max_c below 2^-100 down to
// the smallest subnormal, the largest admitted maximum, every refusal with the exponent untouched), that the multiplier is exact
// and puts the column's maximum into [2^14, 2^15), and the folding helpers on exactly sized heap buffers, so that one element too
// far is reported, against ldexp restated here.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../image-processing-graph-laplacian_amd/csrc/phi_compact.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

using namespace glf;

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    int32_t e = 777;
    // a column of zeros
    CHECK(compact_exponent(0.f, &e) && e == 0);
    CHECK(compact_multiplier(0) == 1.f);
    // powers of two and their neighbours: ilogb steps exactly at the power
    for (int k = -100; k <= 99; ++k) {
        const float p = std::ldexp(1.f, k), below = std::nextafter(p, 0.f), above = std::nextafter(p, inf);
        CHECK(compact_exponent(p, &e) && e == k - 14);
        CHECK(compact_exponent(above, &e) && e == k - 14);
        CHECK(compact_exponent(below, &e) && e == (k - 1 < -100 ? -100 : k - 1) - 14);
        // the multiplier is the exact power of two, and the scaled maximum lies in [2^14, 2^15)
        CHECK(compact_exponent(p, &e));
        const float mult = compact_multiplier(e);
        CHECK(mult == std::ldexp(1.f, -e) && std::isfinite(mult) && mult > 0.f);
        CHECK(p * mult == 16384.f);
        CHECK(compact_exponent(above, &e) && above * compact_multiplier(e) >= 16384.f && above * compact_multiplier(e) < 32768.f);
    }
    // below 2^-100 the exponent stays at -114: the column's halves are then smaller than 2^14, down to zero
    for (float x : {std::ldexp(1.f, -101), std::ldexp(1.f, -126), std::ldexp(1.f, -127), std::numeric_limits<float>::denorm_min()}) {
        CHECK(compact_exponent(x, &e) && e == -114);
        const float scaled = x * compact_multiplier(e);
        CHECK(scaled == std::ldexp(x, 114) && scaled < 16384.f); // exact: no overflow, the product of a subnormal and 2^114 is normal
    }
    // the largest admitted maximum, and the refusals: the exponent stays untouched
    CHECK(compact_exponent(std::nextafter(std::ldexp(1.f, 100), 0.f), &e) && e == 85);
    CHECK(compact_multiplier(85) == std::ldexp(1.f, -85) && compact_multiplier(-114) == std::ldexp(1.f, 114));
    e = 4242;
    CHECK(!compact_exponent(std::ldexp(1.f, 100), &e) && e == 4242);
    CHECK(!compact_exponent(std::numeric_limits<float>::max(), &e) && e == 4242);
    CHECK(!compact_exponent(inf, &e) && e == 4242);
    CHECK(!compact_exponent(nan, &e) && e == 4242);
    CHECK(!compact_exponent(-1.f, &e) && e == 4242);
    CHECK(!compact_exponent(1.f, nullptr));

    // the folding helpers on exactly sized buffers
    const unsigned m = 5;
    const std::vector<int32_t> ex = {-114, -24, 0, 3, 85};
    {
        std::vector<double> x(3 * m), want(3 * m);
        for (size_t i = 0; i < x.size(); ++i) x[i] = (i % 2 ? -1.0 : 1.0) * (1.0 + 0.37 * (double)i);
        for (size_t i = 0; i < x.size(); ++i) want[i] = std::ldexp(x[i], ex[i % m]);
        std::vector<double> y = x;
        compact_fold_cols(y.data(), 3, m, ex.data());
        for (size_t i = 0; i < x.size(); ++i) CHECK(y[i] == want[i]);
        compact_fold_cols(y.data(), 3, m, ex.data(), -1); // and back: powers of two, exact
        for (size_t i = 0; i < x.size(); ++i) CHECK(y[i] == x[i]);
        compact_fold_cols(y.data(), 3, m, nullptr); // no exponents (an f32 handle): nothing
        for (size_t i = 0; i < x.size(); ++i) CHECK(y[i] == x[i]);
        compact_fold_cols(y.data(), 0, m, ex.data());
        // a value that is not finite stays what it is: the calls' own refusals then see it
        std::vector<double> z = {inf, -inf, nan, 0.0, 1.0};
        compact_fold_cols(z.data(), 1, m, ex.data());
        CHECK(z[0] == inf && z[1] == -inf && std::isnan(z[2]) && z[3] == 0.0 && z[4] == std::ldexp(1.0, 85));
    }
    {
        std::vector<double> G((size_t)m * m), H;
        for (unsigned i = 0; i < m; ++i)
            for (unsigned j = 0; j < m; ++j) G[i * m + j] = 1.0 + (double)(i * j) / 7.0; // symmetric
        H = G;
        compact_fold_gram(H.data(), m, ex.data());
        for (unsigned i = 0; i < m; ++i)
            for (unsigned j = 0; j < m; ++j) {
                CHECK(H[i * m + j] == std::ldexp(G[i * m + j], ex[i] + ex[j]));
                CHECK(H[i * m + j] == H[j * m + i]); // stays exactly symmetric
            }
        compact_fold_gram(H.data(), m, nullptr);
        compact_fold_gram(H.data(), 0, ex.data());
    }
    if (failures) {
        std::fprintf(stderr, "compact_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("compact_host_check: ok\n");
    return 0;
}
