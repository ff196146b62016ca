// scale_rule.hpp -- the power-of-two operand scales of the split-f16 contractions, stated once for the host and the device
// (plain C++: tools/scale_rule_host_main.cpp compiles it without HIP).
//
// A column of the operand with maximum m = max |X[:, j]| is multiplied by 2^e so that |X| 2^e lies in [2^13, 2^14): both f16
// halves of the split then carry it. e = clamp(14 - exponent(m), -100, 100), with m = f 2^exponent, f in [0.5, 1), for a finite
// m > 0 (subnormal ones included), else 0. The kernel's entries carry 2^15 (NYS_F16_KSCALE_LOG2), so 2^(-e - 15) brings a sum
// back exactly. The factored forms hold an intermediate T with |T| <= nr m: the same rule on the f32 product m (float)nr gives et
// (0 where the product is no longer finite), T is rescaled by 2^(et - e - 15) as it arrives from the row pass, and 2^(-et - 15)
// brings the column pass' sum back. Integer arithmetic on the bits only: no frexp or ldexp whose edge cases could differ between
// the host's and the device's library.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GLF_SCALE_HD __host__ __device__
#else
#define GLF_SCALE_HD
#endif

namespace glf {

constexpr int SCALE_KSCALE_LOG2 = 15; // the 2^15 the kernels' entries carry (NYS_F16_KSCALE_LOG2)

// 2^e as a float, -126 <= e <= 127
GLF_SCALE_HD inline float scale_pow2(int e) { return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23); }

// e with m 2^e in [2^13, 2^14), clamped to [-100, 100]; 0 for m = 0, negative, infinite or NaN
GLF_SCALE_HD inline int scale_exponent(float m)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, m);
    if (!(m > 0.f) || (u >> 23) == 0xFFu) return 0;
    // frexp's exponent: biased exponent - 126; a subnormal's from its leading bit (bit k of the fraction: value 2^(k - 149))
    const int ex = (u >> 23) ? (int)(u >> 23) - 126 : (31 - __builtin_clz(u)) - 148;
    const int e = 14 - ex;
    return e > 100 ? 100 : e < -100 ? -100 : e;
}

struct OperandScales {
    float colscale; // 2^e: the operand column's scale
    float inv;      // 2^(-e - 15): a direct or band form's sum back (no intermediate)
    float tscale;   // 2^clamp(et - e - 15, -126, 126): the intermediate T as the row pass accumulated it, to its own scale 2^et
    float tinv;     // 2^(-et - 15): the column pass' sum back
};

// nr: the terms of the intermediate's sum (the sample grid's rows); 1 where there is no intermediate
GLF_SCALE_HD inline OperandScales operand_scales(float m, int nr)
{
    const int e = scale_exponent(m), et = scale_exponent(m * (float)nr);
    const int d = et - e - SCALE_KSCALE_LOG2;
    OperandScales s;
    s.colscale = scale_pow2(e);
    s.inv = scale_pow2(-e - SCALE_KSCALE_LOG2);
    s.tscale = scale_pow2(d > 126 ? 126 : d < -126 ? -126 : d);
    s.tinv = scale_pow2(-et - SCALE_KSCALE_LOG2);
    return s;
}

} // namespace glf
