// host_util.cpp -- host-side stages of the C-ABI: sampling grid, X0 random block,
// synthetic benchmark images, the geometry and schedule of the band form, the centroid updates and
// the seedings (plain and weighted) of the spectral segmentation, the orthonormal change of basis of a
// graph handle from its Gram matrix, the loss table and the scale estimate of the robust fit, the exponent rule and the
// scale folding of the compact graph handle. No device code.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/glf.h"
#include "band_plan.hpp"
#include "phi_compact.hpp"
#include "robust_loss.hpp"

namespace {

inline uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }

struct Xoshiro256ss {
    uint64_t s[4];
    explicit Xoshiro256ss(uint64_t seed)
    {
        // splitmix64 expansion of the seed
        for (int i = 0; i < 4; ++i) {
            uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            s[i] = z ^ (z >> 31);
        }
    }
    uint64_t next()
    {
        const uint64_t result = rotl64(s[1] * 5, 7) * 9;
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0];
        s[3] ^= s[1];
        s[1] ^= s[2];
        s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl64(s[3], 45);
        return result;
    }
    double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); } // [0,1)
};

// The centroid update of one Lloyd iteration: the mean of a label's raw rows of Phi, moved into the embedding by scale. div is the
// label's count (glf_cluster_update) or its mass (glf_cluster_update_w: the weighted mean); a label with !(div_j > 0) keeps cent_prev_j.
template <class T>
int cluster_update(unsigned k, unsigned dim, const double *scale, const double *sums, const T *div, const double *cent_prev, double *cent)
{
    if (!sums || !div || !cent || k == 0 || dim == 0) return GLF_ERR_INVALID;
    if (!cent_prev)
        for (unsigned j = 0; j < k; ++j)
            if (!(div[j] > 0)) return GLF_ERR_INVALID;
    for (unsigned j = 0; j < k; ++j)
        for (unsigned c = 0; c < dim; ++c) {
            const size_t e = (size_t)j * dim + c;
            cent[e] = div[j] > 0 ? (scale ? scale[c] : 1.0) * sums[e] / (double)div[j] : cent_prev[e];
        }
    return GLF_OK;
}

// k-means++ (Arthur & Vassilvitskii 2007) on the library's own uniform stream, so that a seed names one set of centres. Every row's
// chance is multiplied by its weight w[i] (checked by the caller: >= 0 and finite), NULL meaning 1. A draw takes the first row, in
// row order, whose running sum of the chances exceeds u times their total; with all weights 1 the first centre is then row
// min(n - 1, floor(u n)), and 1.0 * D^2 is exact.
int cluster_seed(const double *rows, const double *w, size_t n, unsigned dim, unsigned k, uint64_t seed, double *cent)
{
    if (!rows || !cent || n == 0 || dim == 0 || k == 0 || k > n) return GLF_ERR_INVALID;
    auto wt = [&](size_t i) { return w ? w[i] : 1.0; };
    double wtotal = 0.0;
    for (size_t i = 0; i < n; ++i) wtotal += wt(i);
    if (!(wtotal > 0.0) || !std::isfinite(wtotal)) return GLF_ERR_INVALID;
    Xoshiro256ss rng(seed);
    std::vector<size_t> chosen(k);
    std::vector<double> d2(n);
    auto draw = [&](auto wd, double total) { // (total > 0: some wd[i] > 0)
        const double target = rng.uniform() * total;
        size_t pick = n;
        double run = 0.0;
        for (size_t i = 0; i < n && pick == n; ++i) {
            run += wd(i);
            if (run > target) pick = i;
        }
        if (pick == n) // (run ends at total; reached only where u total rounds up to total: the last row with a chance)
            for (pick = n - 1; pick > 0 && !(wd(pick) > 0.0);) --pick;
        return pick;
    };
    chosen[0] = draw(wt, wtotal);
    for (unsigned t = 1; t < k; ++t) {
        const double *c = rows + chosen[t - 1] * dim;
        double total = 0.0;
        for (size_t i = 0; i < n; ++i) {
            double d = 0.0;
            for (unsigned q = 0; q < dim; ++q) {
                const double x = rows[i * dim + q] - c[q];
                d += x * x;
            }
            d2[i] = t == 1 ? d : std::min(d2[i], d);
            total += wt(i) * d2[i];
        }
        if (!(total > 0.0) || !std::isfinite(total)) return GLF_ERR_INVALID; // fewer than k distinct rows of positive weight (or a NaN / Inf)
        chosen[t] = draw([&](size_t i) { return wt(i) * d2[i]; }, total);
    }
    for (unsigned t = 0; t < k; ++t) std::copy(rows + chosen[t] * dim, rows + (chosen[t] + 1) * dim, cent + (size_t)t * dim);
    return GLF_OK;
}

} // namespace

extern "C" {

// Spatially uniform grid sampling, same contract as the reference's
// Sampling()/UniformSampling() (hpc/sampling.c:6-33): the requested count is
// rewritten to the realised grid count; indices ascend in raster order; the
// grid pitch is floor(sqrt(floor(N / requested))) with unsigned integer
// division; the last image row and column are never sampled.
int glf_Sampling(int width, int height, unsigned *sample_size, unsigned **sample_indices)
{
    // width or height 1: `r < h - 1u` would wrap (the reference's loop bound `i < height - 1`, hpc/sampling.c:16-18, admits no
    // row either: no sample exists) -- rejected instead of counting forever
    if (!sample_size || !sample_indices || width < 2 || height < 2 || *sample_size == 0)
        return GLF_ERR_INVALID;
    const unsigned w = (unsigned)width, h = (unsigned)height;
    const unsigned pitch = (unsigned)std::sqrt((double)((w * h) / *sample_size));
    if (pitch == 0) return GLF_ERR_INVALID;
    const unsigned first = pitch / 2;
    unsigned nrows = 0, ncols = 0;
    for (unsigned r = first; r < h - 1u; r += pitch) ++nrows;
    for (unsigned c = first; c < w - 1u; c += pitch) ++ncols;
    const size_t count = (size_t)nrows * ncols;
    unsigned *idx = (unsigned *)std::malloc(sizeof(unsigned) * (count ? count : 1));
    if (!idx) return GLF_ERR_NOMEM;
    size_t k = 0;
    for (unsigned r = first; r < h - 1u; r += pitch)
        for (unsigned c = first; c < w - 1u; c += pitch) idx[k++] = w * r + c;
    *sample_size = (unsigned)count;
    *sample_indices = idx;
    return GLF_OK;
}

int glf_shard_rows(int height, int rank, int size, int *row0, int *row1)
{
    if (height < 0 || size < 1 || rank < 0 || rank >= size || !row0 || !row1) return GLF_ERR_INVALID;
    *row0 = (int)((long long)rank * height / size);
    *row1 = (int)((long long)(rank + 1) * height / size);
    return GLF_OK;
}

// X0 for the inverse subspace iteration: m vectors of length p, vector after
// vector, U[0,1) (the reference fills with PETSc's rand48 seeded by the MPI
// rank, hpc/inverse_power_it.c:27-34; that stream is third-party, so we fix our
// own and make it independent of the GPU count).
int glf_random_vectors(double *X0, unsigned p, unsigned m, uint64_t seed)
{
    if (!X0) return GLF_ERR_INVALID;
    Xoshiro256ss rng(seed);
    const size_t n = (size_t)p * m;
    for (size_t k = 0; k < n; ++k) X0[k] = rng.uniform();
    return GLF_OK;
}

// The PoC's random sampler (python/sampling/random.py:8-16): draw until `*sample_size` distinct pixels are there, sort.
int glf_RandomSampling(int width, int height, unsigned *sample_size, unsigned **sample_indices, uint64_t seed)
{
    if (!sample_size || !sample_indices || width <= 0 || height <= 0) return GLF_ERR_INVALID;
    const uint64_t N = (uint64_t)width * (uint64_t)height;
    const unsigned want = *sample_size;
    *sample_indices = nullptr;
    if (want == 0 || want > N) return GLF_ERR_INVALID;
    std::vector<uint8_t> taken(N, 0);
    Xoshiro256ss rng(0xA11CE5EEDull ^ seed);
    unsigned have = 0;
    while (have < want) {
        const uint64_t px = rng.next() % N;
        if (!taken[px]) {
            taken[px] = 1;
            ++have;
        }
    }
    unsigned *idx = static_cast<unsigned *>(std::malloc(sizeof(unsigned) * want));
    if (!idx) return GLF_ERR_NOMEM;
    unsigned k = 0;
    for (uint64_t px = 0; px < N; ++px)
        if (taken[px]) idx[k++] = (unsigned)px;
    *sample_indices = idx;
    return GLF_OK;
}

// Synthetic noisy benchmark image: smooth low-frequency shading +
// 64-px two-level checker + one diagonal edge, scaled into [40, 215], plus
// i.i.d. Gaussian noise sigma = 20 (Box-Muller), rounded and clipped to uint8.
int glf_synth_image(uint8_t *out, int width, int height, uint64_t seed)
{
    if (!out || width <= 0 || height <= 0) return GLF_ERR_INVALID;
    Xoshiro256ss rng(0x5EED0000ull + seed);
    const double two_pi = 6.283185307179586;
    for (int r = 0; r < height; ++r) {
        for (int c = 0; c < width; ++c) {
            const double u = (double)c / 512.0, v = (double)r / 512.0;
            double base = 0.5 * (std::sin(two_pi * 0.9 * u) + std::sin(two_pi * 0.6 * v + 1.0) +
                                 std::sin(two_pi * 0.4 * (u + v))) / 3.0;      // [-0.5, 0.5]
            base += (((r >> 6) + (c >> 6)) & 1) ? 0.22 : -0.22;                   // checker
            base += ((c - r) > (width - height) / 2 + 37) ? 0.15 : -0.15;         // diagonal edge
            double g = 127.5 + base * (175.0 / 1.74);                             // ~[40, 215]
            const double u1 = 1.0 - rng.uniform(), u2 = rng.uniform();
            g += 20.0 * std::sqrt(-2.0 * std::log(u1)) * std::cos(two_pi * u2);
            g = std::nearbyint(g);
            out[(size_t)r * width + c] = (uint8_t)(g < 0.0 ? 0.0 : (g > 255.0 ? 255.0 : g));
        }
    }
    return GLF_OK;
}

// The schedule of k_band's pixel-target instantiations, restated on the host from the same windows and the same pairing helpers
// (band_plan.hpp): what every wave executes, so that coverage can be checked without relying on the parity of outputs whose
// edge entries are below 2^-40 of the largest term.
int glf_band_plan(const int *rows, int nr, const int *cols, int nc, float h_loc, int width, int height, int row_begin, int row_end,
                  int pair_stride, int *rad, int *tile_px, int *ntiles, int *first_row, unsigned *units, uint64_t *ksteps)
{
    if (!rows || !cols || nr <= 0 || nc <= 0 || width <= 0 || height <= 0 || row_begin < 0 || row_end > height || row_begin > row_end ||
        !(h_loc > 0.f))
        return GLF_ERR_INVALID;
    const float s_loc = (float)(1.4426950408889634 / ((double)h_loc * (double)h_loc)); // (kernel_coef's)
    glf::BandGeom geom;
    if (!geom.init(rows, nr, cols, nc, (double)s_loc)) return GLF_ERR_UNSUPPORTED;
    static_assert(glf::BAND_NW == GLF_BAND_WG_ROWS, "glf.h documents the rows of a workgroup");
    const int tpx = 32 * glf::BAND_PB, nt = (width + tpx - 1) / tpx, NW = glf::BAND_NW;
    if (rad) *rad = geom.rad;
    if (tile_px) *tile_px = tpx;
    if (ntiles) *ntiles = nt;
    std::vector<unsigned> win((size_t)geom.rad * nt);
    for (int dr = 0; dr < geom.rad; ++dr)
        for (int t = 0; t < nt; ++t) win[(size_t)dr * nt + t] = geom.window(t * tpx, std::min(width, (t + 1) * tpx) - 1, dr, glf::BAND_HALF_SHIFT);
    uint64_t steps = 0;
    for (int trow0 = row_begin; trow0 < row_end; trow0 += NW) {
        const int ntw = std::min(NW, row_end - trow0);
        int alo = 0xFFFF, ahi = -1;
        for (int w = 0; w < ntw; ++w) {
            const unsigned rb = geom.band_of(trow0 + w);
            if (glf::band_win_live(rb)) {
                alo = std::min(alo, (int)(rb & 0xFFFFu));
                ahi = std::max(ahi, (int)(rb >> 16));
            }
        }
        const int nb = std::min(glf::BAND_MAXROWS, std::max(0, ahi - alo + 1)), npairs = (nb + glf::BAND_PAIR - 1) / glf::BAND_PAIR;
        if (units && npairs > pair_stride) return GLF_ERR_INVALID;
        for (int w = 0; w < ntw; ++w) {
            const size_t ro = (size_t)(trow0 + w - row_begin);
            if (first_row) first_row[ro] = nb > 0 ? alo : -1;
            for (int t = 0; t < nt; ++t) {
                unsigned *u = units ? units + (ro * nt + t) * (size_t)pair_stride : nullptr;
                for (int j = 0; u && j < pair_stride; ++j) u[j] = glf::BAND_EMPTY;
                for (int j = 0; j < npairs; ++j) {
                    unsigned h = glf::BAND_EMPTY;
                    for (int i = glf::BAND_PAIR * j; i < std::min(nb, glf::BAND_PAIR * (j + 1)); ++i) {
                        const int dr = std::abs(trow0 + w - geom.rows[alo + i]);
                        h = glf::band_win_hull(h, dr < geom.rad ? win[(size_t)dr * nt + t] : glf::BAND_EMPTY);
                    }
                    if (u) u[j] = h;
                    if (glf::band_win_live(h)) steps += (h >> 16) - (h & 0xFFFFu) + 1;
                }
            }
        }
    }
    if (ksteps) *ksteps = steps;
    return GLF_OK;
}

int glf_cluster_update(unsigned k, unsigned dim, const double *scale, const double *sums, const uint64_t *counts, const double *cent_prev,
                       double *cent)
{
    return cluster_update(k, dim, scale, sums, counts, cent_prev, cent);
}

int glf_cluster_update_w(unsigned k, unsigned dim, const double *scale, const double *sums, const double *mass, const double *cent_prev,
                         double *cent)
{
    return cluster_update(k, dim, scale, sums, mass, cent_prev, cent);
}

int glf_cluster_seed(const double *rows, size_t n, unsigned dim, unsigned k, uint64_t seed, double *cent)
{
    return cluster_seed(rows, nullptr, n, dim, k, seed, cent);
}

int glf_cluster_seed_w(const double *rows, const double *w, size_t n, unsigned dim, unsigned k, uint64_t seed, double *cent)
{
    for (size_t i = 0; w && i < n; ++i)
        if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return GLF_ERR_INVALID;
    return cluster_seed(rows, w, n, dim, k, seed, cent);
}

static_assert((int)GLF_ROBUST_HUBER == (int)glf::ROBUST_HUBER && (int)GLF_ROBUST_CAUCHY == (int)glf::ROBUST_CAUCHY && (int)GLF_ROBUST_TUKEY == (int)glf::ROBUST_TUKEY,
              "robust_loss.hpp restates the header's kinds");

int glf_robust_weight(int kind, double c, double q, double *u, double *rho)
{
    if (kind < 0 || kind >= glf::ROBUST_KINDS || !std::isfinite(c) || c < 0.0 || !(q >= 0.0)) return GLF_ERR_INVALID;
    if (c == 0.0) c = glf::robust_default_c(kind);
    if (u) *u = glf::robust_u(kind, c, q);
    if (rho) *rho = glf::robust_rho(kind, c, q);
    return GLF_OK;
}

int glf_robust_scale(const double *res, const double *w, size_t n, double *sigma)
{
    if (!res || !sigma || n == 0) return GLF_ERR_INVALID;
    std::vector<double> mag;
    mag.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(res[i]) || (w && !std::isfinite(w[i]))) return GLF_ERR_INVALID;
        if (!w || w[i] > 0.0) mag.push_back(std::fabs(res[i]));
    }
    if (mag.empty()) return GLF_ERR_INVALID;
    const size_t mid = (mag.size() - 1) / 2;
    std::nth_element(mag.begin(), mag.begin() + (std::ptrdiff_t)mid, mag.end());
    if (!(mag[mid] > 0.0)) return GLF_ERR_INVALID;
    *sigma = 1.4826 * mag[mid];
    return GLF_OK;
}

// The change of basis that makes Phi orthonormal, from its Gram matrix alone (the one-shot orthogonalisation of Fowlkes, Belongie,
// Chung and Malik, restated on Phi): G = L L^T, Q = Phi L^-T has orthonormal columns, and Phi diag(1 - lam) Phi^T = Q S Q^T with
// S = L^T diag(1 - lam) L. With S = U Theta U^T (cyclic Jacobi), Phi T with T = L^-T U is an orthonormal eigenbasis of the same
// operator with the eigenvalues 1 - theta. Everything is sequential f64 in a fixed order: two calls give the same bits.
int glf_basis_orthonormal(unsigned m, const double *G, const double *lam, double *T, double *lam_new)
{
    if (!G || !T || m == 0 || (lam && !lam_new)) return GLF_ERR_INVALID;
    const size_t n = m;
    for (size_t e = 0; e < n * n; ++e)
        if (!std::isfinite(G[e])) return GLF_ERR_INVALID;
    for (size_t i = 0; lam && i < n; ++i)
        if (!std::isfinite(lam[i])) return GLF_ERR_INVALID;
    // L L^T = G, row by row from G's lower triangle (glf_fit_coeffs' factorisation)
    std::vector<double> L(n * n, 0.0), Li(n * n, 0.0);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j <= i; ++j) {
            double s = G[i * n + j];
            for (size_t k = 0; k < j; ++k) s -= L[i * n + k] * L[j * n + k];
            if (i == j) {
                if (!(s > 0.0)) return GLF_ERR_INVALID;
                L[i * n + i] = std::sqrt(s);
            } else
                L[i * n + j] = s / L[j * n + j];
        }
    // Li = L^-1 (lower triangular), column by column: L Li = I
    for (size_t c = 0; c < n; ++c)
        for (size_t i = c; i < n; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (size_t k = c; k < i; ++k) s -= L[i * n + k] * Li[k * n + c];
            Li[i * n + c] = s / L[i * n + i];
        }
    std::vector<double> out(n * n, 0.0);
    if (!lam) {
        for (size_t k = 0; k < n; ++k)
            for (size_t j = k; j < n; ++j) out[k * n + j] = Li[j * n + k]; // L^-T
        std::copy(out.begin(), out.end(), T);
        return GLF_OK;
    }
    // S = L^T diag(1 - lam) L: the upper triangle, mirrored. Ut is U^T: a rotation then works on two rows of each matrix
    std::vector<double> S(n * n, 0.0), Ut(n * n, 0.0);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i; j < n; ++j) {
            double s = 0.0;
            for (size_t k = j; k < n; ++k) s += L[k * n + i] * (1.0 - lam[k]) * L[k * n + j];
            S[i * n + j] = S[j * n + i] = s;
        }
    for (size_t i = 0; i < n; ++i) Ut[i * n + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (size_t i = 0; i < n; ++i) {
            diag += S[i * n + i] * S[i * n + i];
            for (size_t j = i + 1; j < n; ++j) off += S[i * n + j] * S[i * n + j];
        }
        if (off <= 1e-32 * diag) break;
        for (size_t p = 0; p + 1 < n; ++p)
            for (size_t q = p + 1; q < n; ++q) {
                const double apq = S[p * n + q];
                if (apq == 0.0) continue;
                const double app = S[p * n + p], aqq = S[q * n + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                // S <- J^T S J: rows p and q (contiguous), the columns as their mirror, the 2 x 2 block in closed form
                double *sp = S.data() + p * n, *sq = S.data() + q * n;
                for (size_t k = 0; k < n; ++k) {
                    const double spk = sp[k], sqk = sq[k];
                    sp[k] = c * spk - s * sqk;
                    sq[k] = s * spk + c * sqk;
                }
                for (size_t k = 0; k < n; ++k) {
                    S[k * n + p] = sp[k];
                    S[k * n + q] = sq[k];
                }
                sp[p] = app - t * apq;
                sq[q] = aqq + t * apq;
                sp[q] = sq[p] = 0.0;
                double *up = Ut.data() + p * n, *uq = Ut.data() + q * n;
                for (size_t k = 0; k < n; ++k) {
                    const double upk = up[k], uqk = uq[k];
                    up[k] = c * upk - s * uqk;
                    uq[k] = s * upk + c * uqk;
                }
            }
    }
    // theta descending, the lower original index first on a tie
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return S[a * n + a] > S[b * n + b]; });
    for (size_t j = 0; j < n; ++j) {
        const size_t col = order[j];
        // sign: the entry of largest magnitude of the column of U is positive, the lowest index on a tie
        double big = 0.0;
        const double *u = Ut.data() + col * n;
        for (size_t i = 0; i < n; ++i)
            if (std::fabs(u[i]) > std::fabs(big)) big = u[i];
        const double sign = big < 0.0 ? -1.0 : 1.0;
        for (size_t k = 0; k < n; ++k) { // T = L^-T U
            double s = 0.0;
            for (size_t i = k; i < n; ++i) s += Li[i * n + k] * u[i];
            out[k * n + j] = sign * s;
        }
    }
    for (size_t e = 0; e < n * n; ++e)
        if (!std::isfinite(out[e])) return GLF_ERR_INVALID; // (a lam near the f64 range: nothing was written)
    std::copy(out.begin(), out.end(), T);
    for (size_t j = 0; j < n; ++j) lam_new[j] = 1.0 - S[order[j] * n + order[j]];
    return GLF_OK;
}

// R = L^-T of G + diag(penalty) = L L^T: glf_basis_orthonormal's Cholesky mode on the penalised matrix (its factorisation reads the
// lower triangle, as glf_fit_coeffs' does, so the two refuse the same systems)
int glf_fit_factor(unsigned m, const double *G, const double *penalty, double *R)
{
    if (!G || !R || m == 0) return GLF_ERR_INVALID;
    const size_t n = m;
    std::vector<double> M(G, G + n * n), out(n * n);
    for (size_t i = 0; penalty && i < n; ++i) {
        if (!std::isfinite(penalty[i])) return GLF_ERR_INVALID;
        M[i * n + i] += penalty[i];
    }
    const int rc = glf_basis_orthonormal(m, M.data(), nullptr, out.data(), nullptr);
    if (rc != GLF_OK) return rc;
    for (size_t e = 0; e < n * n; ++e)
        if (!std::isfinite(out[e])) return GLF_ERR_INVALID;
    std::copy(out.begin(), out.end(), R);
    return GLF_OK;
}

} // extern "C"

// ---- low-rank factor of the photometric table -----------------------------------------------------------------
// P[v][w] = exp2(-s_val (v - w)^2) over the 256 grey levels (the photometric factor of hpc/affinity.c:59-113 with
// s_val = log2(e) / h_val^2) is symmetric positive semi-definite with a rapidly decaying spectrum: at the reference's
// h_val = 30 its rank-32 eigen-expansion P ~= F F^T reproduces every entry to 1.5e-11. The factor is what the "rank"
// form of the grid-factored contractions carries instead of the 256 grey levels (nystroem_rank.inc).
// Computed in f64: pivoted Cholesky P ~= L L^T down to a residual diagonal of 1e-15 (r <= max_chol columns), then the
// eigen-decomposition of the small r x r matrix L^T L = Q diag(lambda) Q^T by cyclic Jacobi; F = L Q has the columns
// sqrt(lambda_k) u_k of the eigen-expansion, strongest first. Rows of F have sum_k F[v][k]^2 <= P[v][v] = 1.
namespace glf {

// F: [256][rank_out] row-major. Returns false when more than max_chol Cholesky columns are needed (sharp kernels).
bool photometric_factor(double s_val, int max_chol, std::vector<double> &F, int &rank_out)
{
    constexpr int n = 256;
    std::vector<double> L((size_t)n * max_chol, 0.0), d(n, 1.0);
    auto P = [&](int v, int w) { return std::exp2(-s_val * (double)(v - w) * (double)(v - w)); };
    int r = 0;
    for (; r < max_chol; ++r) {
        int piv = 0;
        for (int v = 1; v < n; ++v)
            if (d[v] > d[piv]) piv = v;
        if (d[piv] <= 1e-15) break;
        const double inv = 1.0 / std::sqrt(d[piv]);
        for (int v = 0; v < n; ++v) {
            double x = P(v, piv);
            for (int k = 0; k < r; ++k) x -= L[(size_t)v * max_chol + k] * L[(size_t)piv * max_chol + k];
            x *= inv;
            L[(size_t)v * max_chol + r] = x;
            d[v] -= x * x;
        }
        d[piv] = 0.0;
    }
    if (r == max_chol) {
        double worst = 0.0;
        for (int v = 0; v < n; ++v) worst = std::max(worst, d[v]);
        if (worst > 1e-15) return false;
    }
    // G = L^T L (r x r), Jacobi eigen-decomposition G = Q diag(lam) Q^T
    std::vector<double> G((size_t)r * r, 0.0), Q((size_t)r * r, 0.0);
    for (int i = 0; i < r; ++i)
        for (int j = i; j < r; ++j) {
            double x = 0.0;
            for (int v = 0; v < n; ++v) x += L[(size_t)v * max_chol + i] * L[(size_t)v * max_chol + j];
            G[(size_t)i * r + j] = G[(size_t)j * r + i] = x;
        }
    for (int i = 0; i < r; ++i) Q[(size_t)i * r + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < r; ++i) {
            diag += G[(size_t)i * r + i] * G[(size_t)i * r + i];
            for (int j = i + 1; j < r; ++j) off += G[(size_t)i * r + j] * G[(size_t)i * r + j];
        }
        if (off <= 1e-32 * diag) break;
        for (int pI = 0; pI < r - 1; ++pI)
            for (int q = pI + 1; q < r; ++q) {
                const double apq = G[(size_t)pI * r + q];
                if (apq == 0.0) continue;
                const double app = G[(size_t)pI * r + pI], aqq = G[(size_t)q * r + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < r; ++k) { // columns p, q
                    const double gkp = G[(size_t)k * r + pI], gkq = G[(size_t)k * r + q];
                    G[(size_t)k * r + pI] = c * gkp - s * gkq;
                    G[(size_t)k * r + q] = s * gkp + c * gkq;
                }
                for (int k = 0; k < r; ++k) { // rows p, q
                    const double gpk = G[(size_t)pI * r + k], gqk = G[(size_t)q * r + k];
                    G[(size_t)pI * r + k] = c * gpk - s * gqk;
                    G[(size_t)q * r + k] = s * gpk + c * gqk;
                }
                for (int k = 0; k < r; ++k) {
                    const double qkp = Q[(size_t)k * r + pI], qkq = Q[(size_t)k * r + q];
                    Q[(size_t)k * r + pI] = c * qkp - s * qkq;
                    Q[(size_t)k * r + q] = s * qkp + c * qkq;
                }
            }
    }
    std::vector<int> order(r);
    for (int i = 0; i < r; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return G[(size_t)a * r + a] > G[(size_t)b * r + b]; });
    F.assign((size_t)n * r, 0.0);
    for (int k = 0; k < r; ++k) {
        const int col = order[k];
        // sign convention: the entry of largest magnitude of every column is positive (the product F F^T does not care)
        double big = 0.0;
        for (int v = 0; v < n; ++v) {
            double x = 0.0;
            for (int j = 0; j < r; ++j) x += L[(size_t)v * max_chol + j] * Q[(size_t)j * r + col];
            F[(size_t)v * r + k] = x;
            if (std::fabs(x) > std::fabs(big)) big = x;
        }
        if (big < 0.0)
            for (int v = 0; v < n; ++v) F[(size_t)v * r + k] = -F[(size_t)v * r + k];
    }
    rank_out = r;
    return true;
}

// max over (v, w) of |sum_{k < R} F[v][k] F[w][k] - P[v][w]|
double photometric_factor_error(double s_val, const std::vector<double> &F, int rank, int R)
{
    constexpr int n = 256;
    double worst = 0.0;
    for (int v = 0; v < n; ++v)
        for (int w = v; w < n; ++w) {
            double x = 0.0;
            for (int k = 0; k < R && k < rank; ++k) x += F[(size_t)v * rank + k] * F[(size_t)w * rank + k];
            worst = std::max(worst, std::fabs(x - std::exp2(-s_val * (double)(v - w) * (double)(v - w))));
        }
    return worst;
}

// ---- band form: radius and windows -----------------------------------------------------------------------------
bool BandGeom::init(const int *grows, int nr, const int *gcols, int nc, double s_loc)
{
    if (!(s_loc > 0.0)) return false;
    D2 = 40.5 / s_loc; // 2^15 E(dr) E(dc) <= 2^-25.5: a zero f16 (hi, lo) pair whatever P is
    const double rr = std::floor(std::sqrt(D2)) + 1.0;
    if (rr > BAND_RMAX) return false;
    rad = (int)rr; // first integer distance with d^2 >= D2
    rows.assign(grows, grows + nr);
    cols.assign(gcols, gcols + nc);
    // largest |dc| inside the circle at row distance dr: dc^2 < D2 - dr^2
    dcmax.assign(rad, -1);
    for (int dr = 0; dr < rad; ++dr) {
        const double rem = D2 - (double)dr * dr;
        int d = (int)std::floor(std::sqrt(std::max(0.0, rem)));
        while (d > 0 && (double)d * d >= rem) --d;
        dcmax[dr] = rem > 0.0 ? d : -1;
    }
    return true;
}

unsigned BandGeom::band_of(int r) const
{
    const int lo = (int)(std::lower_bound(rows.begin(), rows.end(), r - rad + 1) - rows.begin());
    const int hi = (int)(std::upper_bound(rows.begin(), rows.end(), r + rad - 1) - rows.begin()) - 1;
    if (hi < lo) return 1u;
    return (unsigned)lo | ((unsigned)hi << 16);
}

unsigned BandGeom::window(int cmin, int cmax, int dr, int shift) const
{
    if (dcmax[dr] < 0) return BAND_EMPTY;
    int lo = 0, n = 0;
    band_cols_range(cols.data(), (int)cols.size(), cmin - dcmax[dr], cmax + dcmax[dr], &lo, &n);
    if (n <= 0) return BAND_EMPTY;
    return (unsigned)(lo >> shift) | ((unsigned)((lo + n - 1) >> shift) << 16);
}

// ---- compact graph handle: the exponent rule and the folding of the column scales -------------------------------
bool compact_exponent(float max_c, int32_t *e)
{
    if (!e || !(max_c >= 0.f) || !std::isfinite(max_c) || max_c >= std::ldexp(1.f, 100)) return false;
    *e = max_c == 0.f ? 0 : std::max(std::ilogb(max_c), COMPACT_E_FLOOR) - COMPACT_E_SHIFT;
    return true;
}

float compact_multiplier(int32_t e) { return std::ldexp(1.f, -e); }

void compact_fold_cols(double *x, size_t rows, unsigned cols, const int32_t *e, int sign)
{
    if (!e) return;
    for (size_t r = 0; r < rows; ++r)
        for (unsigned c = 0; c < cols; ++c) x[r * cols + c] = std::ldexp(x[r * cols + c], sign * e[c]);
}

void compact_fold_gram(double *G, unsigned m, const int32_t *e)
{
    if (!e) return;
    for (unsigned i = 0; i < m; ++i)
        for (unsigned j = 0; j < m; ++j) G[(size_t)i * m + j] = std::ldexp(G[(size_t)i * m + j], e[i] + e[j]);
}

} // namespace glf
