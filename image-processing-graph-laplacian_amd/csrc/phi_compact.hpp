// phi_compact.hpp -- the host-only half of the compact graph handle (glf_graph_compact, include/glf.h): the exponent rule of a column
// and the folding of the column scales 2^e_c into the host-side operands and results of the handle's calls. Defined in
// host_util.cpp (no device code), so that `make compact_check` runs them under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace glf {

constexpr int COMPACT_E_FLOOR = -100; // ilogb(max_c) is taken no lower than this
constexpr int COMPACT_E_SHIFT = 14;   // a column's largest magnitude, scaled, lies in [2^14, 2^15)

// e_c of a column whose largest magnitude is max_c: max(ilogb(max_c), -100) - 14, and 0 for a column of zeros.
// false, *e untouched: max_c is negative, not finite, or >= 2^100.
bool compact_exponent(float max_c, int32_t *e);
// 2^-e as a float: the multiplier of the convert pass (exact for every e the rule gives, -114 <= e <= 85)
float compact_multiplier(int32_t e);
// x[r][c] <- x[r][c] 2^(sign e_c) for r < rows, c < cols, x of row pitch cols (f64: exact short of f64's own range); e NULL: nothing
void compact_fold_cols(double *x, size_t rows, unsigned cols, const int32_t *e, int sign = 1);
// G[i][j] <- G[i][j] 2^(e_i + e_j), G [m][m]
void compact_fold_gram(double *G, unsigned m, const int32_t *e);

} // namespace glf
