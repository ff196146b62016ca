// The power-of-two operand scale rule (csrc/scale_rule.hpp) against an independent statement in double precision, as a stand-alone
// host program (CPU only; built with the address and undefined-behaviour sanitizers by `make scale_rule_check`).
//
// The statement: for a finite m > 0, e = clamp(14 - ex, -100, 100) with m = f 2^ex, f in [0.5, 1) (std::frexp of the double, which
// holds every float, subnormal ones included, exactly); else e = 0. et: the same of the f32 product m * (float)nr. Then
// colscale = 2^e, inv = 2^(-e - 15), tscale = 2^clamp(et - e - 15, -126, 126), tinv = 2^(-et - 15) by std::ldexp. Every float is a
// double, so the comparison is exact equality.
// Inputs: every f32 exponent (and every leading bit of a subnormal) with the mantissas 1, 1 + 2^-23 and 2 - 2^-23; 0, the smallest and
// the largest subnormal, FLT_MAX, Inf, NaN and a negative value; each with nr = 1, 4, 304 and 1024. The values expected of the
// non-finite inputs are those of the host loops the rule replaced: e = 0.
#include "../image-processing-graph-laplacian_amd/csrc/scale_rule.hpp"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int expect_exponent(float v)
{
    if (!(v > 0.f) || !std::isfinite(v)) return 0;
    int ex = 0;
    (void)std::frexp((double)v, &ex);
    const int e = 14 - ex;
    return e > 100 ? 100 : e < -100 ? -100 : e;
}

static float from_bits(uint32_t u)
{
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

int main()
{
    std::vector<float> in;
    for (uint32_t b = 1; b <= 254; ++b)
        for (uint32_t frac : {0u, 1u, 0x7FFFFFu}) in.push_back(from_bits(b << 23 | frac));
    for (int k = 0; k < 23; ++k) // subnormals by leading bit: 2^k, 2^k + 1 (k > 0), 2^(k + 1) - 1
        for (uint32_t u : {1u << k, (1u << k) | (k ? 1u : 0u), (2u << k) - 1u}) in.push_back(from_bits(u));
    for (float v : {0.f, -0.f, from_bits(1u), from_bits(0x7FFFFFu), FLT_MAX, INFINITY, -INFINITY, NAN, -1.f, 0x1p-140f, 3e37f}) in.push_back(v);
    const int nrs[] = {1, 4, 304, 1024};
    long checked = 0, bad = 0;
    for (float m : in)
        for (int nr : nrs) {
            const glf::OperandScales s = glf::operand_scales(m, nr);
            const int e = expect_exponent(m), et = expect_exponent(m * (float)nr);
            int d = et - e - 15;
            d = d > 126 ? 126 : d < -126 ? -126 : d;
            const double want[4] = {std::ldexp(1.0, e), std::ldexp(1.0, -e - 15), std::ldexp(1.0, d), std::ldexp(1.0, -et - 15)};
            const double got[4] = {s.colscale, s.inv, s.tscale, s.tinv};
            ++checked;
            if (glf::scale_exponent(m) != e || std::memcmp(want, got, sizeof(want)) != 0) {
                if (bad++ < 10)
                    std::printf("scale_rule_host_check: m = %a nr = %d: e %d (want %d), scales %a %a %a %a (want %a %a %a %a)\n", (double)m, nr,
                                glf::scale_exponent(m), e, got[0], got[1], got[2], got[3], want[0], want[1], want[2], want[3]);
            }
        }
    // the edges by name: what the rule gives there is written down in DESIGN.md
    const bool edges = glf::scale_exponent(0.f) == 0 && glf::scale_exponent(INFINITY) == 0 && glf::scale_exponent(NAN) == 0 &&
                       glf::scale_exponent(0x1p-140f) == 100 && glf::scale_exponent(3e37f) == -100 &&
                       glf::operand_scales(3e37f, 304).tinv == 0x1p-15f /* the product overflows: et = 0 */;
    if (!edges) std::printf("scale_rule_host_check: a named edge moved\n");
    if (bad || !edges) {
        std::printf("scale_rule_host_check: %ld of %ld differ\n", bad, checked);
        return 1;
    }
    std::printf("scale_rule_host_check: ok (%ld cases)\n", checked);
    return 0;
}
