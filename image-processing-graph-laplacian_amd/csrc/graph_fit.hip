// graph_fit.hip -- the weighted normal equations of a least-squares fit on a graph handle: G = Phi^T diag(w) Phi and
// b_k = Phi^T diag(w) s_k in one pass over Phi (k_graph_normal), and the host-side Cholesky solve (glf_fit_coeffs).
#include "phi_tile.hpp"
#include "phi_compact.hpp"

#include <algorithm>
#include <cmath>

namespace glf {

// How the [ld][ld] matrix is cut. Tiles are 32 x 32 (one MFMA accumulator); only tiles (ti <= tj) are computed. The columns
// are grouped into superblocks of CW (64; 32 at ld 32) and blockIdx.y runs over the superblock pairs I <= J: a diagonal pair
// holds the tiles (2I, 2I), (2I, 2I + 1), (2I + 1, 2I + 1), an off-diagonal pair the four tiles (2I + a, 2J + b). A workgroup
// reads only its superblocks' columns of Phi: ld <= 64 is one pair and one pass; ld 128 reads 64 + 128 + 64 columns (Phi twice),
// ld 256 reads 4 x 64 + 6 x 128 columns (Phi four times). Every pair owns `slots` [32][32] f64 tiles of the result.
struct GnGeom {
    int cw, sb, ny, slots, xmax;
};
inline GnGeom gn_geom(unsigned ld)
{
    GnGeom g;
    g.cw = ld < 64 ? 32 : 64;
    g.sb = (int)ld / g.cw;
    g.ny = g.sb * (g.sb + 1) / 2;
    g.slots = ld >= 128 ? 4 : ld == 64 ? 3 : 1;
    g.xmax = ld == 32 ? 1024 : ld == 64 ? 512 : ld == 128 ? 256 : 128; // workgroups along the pixels (the rest by the grid stride)
    return g;
}
// superblock pair y -> (I, J), I <= J, row by row
__host__ __device__ inline void gn_pair(int sb, int y, int &I, int &J)
{
    for (I = 0; I < sb; ++I) {
        if (y < sb - I) break;
        y -= sb - I;
    }
    J = I + y;
}
// the tile (ti, tj) slot s of pair (I, J) holds; false: the slot is unused (a diagonal pair's fourth, written as zeros)
inline bool gn_slot_tile(unsigned ld, int I, int J, int s, int &ti, int &tj)
{
    if (ld == 32) {
        ti = tj = 0;
        return s == 0;
    }
    if (I == J) {
        ti = 2 * I + (s == 2);
        tj = 2 * I + (s >= 1);
        return s < 3;
    }
    ti = 2 * I + (s >> 1);
    tj = 2 * J + (s & 1);
    return true;
}

// partG[blockIdx.x][pair y][slot][32][32] (f64) = sum over the workgroup's pixels of fl32(w Phi[px][i]) Phi[px][j];
// partB[(blockIdx.x * 4 + wave) * 2 + half][k][LD] (f64) = sum over the wave's pixels of parity `half` of Phi[px][j] (w s_k)[px].
// The pixels are the contraction index (phi_tile.hpp: the unpadded image, the chain rule, the four-wave reduction): at step u lane
// (r, h) reads column r (and 32 + r) of pixel 2u + h for both operands. A = fl32(w phi), B = phi; w = 1 (no weight plane) leaves
// A = phi exactly. b: t = (double)w (double)s is exact, then fma((double)phi, t, acc) on the values the MFMAs read, one chain per
// (plane, column, pixel parity): it depends on no other plane, and G on no plane. Rows past N are staged as zeros (w and t too).
// ld <= 64 keeps two workgroups per CU (the k-steps of a diagonal pair are unrolled by 4, which holds the registers under 256);
// ld >= 128 carries four accumulator tiles and their f64 images and runs one wave per SIMD.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second loader, the same image).
template <int LD, class T = float>
__global__ __launch_bounds__(256, LD <= 64 ? 2 : 1) void k_graph_normal(const T *__restrict__ phi, int64_t N, const float *__restrict__ w,
                                                                         int nplanes, const float *__restrict__ planes,
                                                                         double *__restrict__ partG, double *__restrict__ partB)
{
    constexpr int CW = LD < 64 ? 32 : 64;
    constexpr int SB = LD / CW;
    constexpr int NY = SB * (SB + 1) / 2;
    constexpr int NP = LD >= 128 ? 4 : LD == 64 ? 3 : 1; // accumulator tiles of a workgroup
    constexpr int NIMG = LD >= 128 ? 2 : 1;               // staged images: superblock I, and J when it differs
    constexpr int RW = NIMG * 32 * CW > 2048 ? NIMG * 32 * CW : 2048; // floats of a wave's region (>= one f64 tile for the epilogue)
    __shared__ __attribute__((aligned(16))) float region[4][RW];
    __shared__ float w_sh[4][32];
    __shared__ double t_sh[4][GLF_MAX_SIGNALS][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    int I, J;
    gn_pair(SB, (int)blockIdx.y, I, J);
    const bool offd = NIMG > 1 && I != J;
    const bool do_b = !offd && nplanes > 0;
    const int cI = I * CW, cJ = J * CW;
    float *tw = region[wave];
    const float *ws = w_sh[wave];
    const double *ts = &t_sh[wave][0][0];
    const int64_t ntiles = (N + 31) / 32, tstride = (int64_t)gridDim.x * 4;

    f32x16 acc[NP];
    double dacc[NP][16];
    double bacc[GLF_MAX_SIGNALS][2];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            acc[p][g] = 0.f;
            dacc[p][g] = 0.0;
        }
#pragma unroll
    for (int k = 0; k < GLF_MAX_SIGNALS; ++k) bacc[k][0] = bacc[k][1] = 0.0;

    // what this lane stages of a tile
    tile_regs<T, CW> v[NIMG];
    float wv = 0.f, sv0 = 0.f, sv1 = 0.f;
    auto load_tile = [&](int64_t tile) {
#pragma unroll
        for (int img = 0; img < NIMG; ++img)
            if (img == 0 || offd) tile_load<CW>(v[img], phi, LD, img ? cJ : cI, N, tile, lane);
        const int64_t px = tile * 32 + r;
        const bool live = px < N;
        wv = live ? (w ? w[px] : 1.f) : 0.f;
        sv0 = do_b && live && h < nplanes ? planes[(size_t)h * N + px] : 0.f;
        sv1 = do_b && live && h + 2 < nplanes ? planes[(size_t)(h + 2) * N + px] : 0.f;
    };

    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile < ntiles) load_tile(tile);
    int chained = 0; // tiles in the running f32 chains
    for (; tile < ntiles; tile += tstride) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int img = 0; img < NIMG; ++img)
            if (img == 0 || offd) tile_put<CW, CW>(tw + img * 32 * CW, v[img], lane);
        if (h == 0) w_sh[wave][r] = wv;
        if (do_b) {
            if (h < nplanes) t_sh[wave][h][r] = (double)wv * (double)sv0;
            if (h + 2 < nplanes) t_sh[wave][h + 2][r] = (double)wv * (double)sv1;
        }
        __builtin_amdgcn_wave_barrier();
        // the next tile's loads fly under this tile's MFMAs
        if (tile + tstride < ntiles) load_tile(tile + tstride);
        if (offd) {
            if constexpr (NIMG > 1) {
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int px = 2 * u + h;
                    const float wp = ws[px];
                    const float a0 = wp * tw[px * CW + r], a1 = wp * tw[px * CW + 32 + r];
                    const float b0 = tw[32 * CW + px * CW + r], b1 = tw[32 * CW + px * CW + 32 + r];
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[3], 0, 0, 0);
                }
            }
        } else {
#pragma unroll 4
            for (int u = 0; u < 16; ++u) {
                const int px = 2 * u + h;
                const float wp = ws[px];
                const float q0 = tw[px * CW + r];
                const float a0 = wp * q0;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, q0, acc[0], 0, 0, 0);
                float q1 = 0.f;
                if constexpr (CW == 64) {
                    q1 = tw[px * CW + 32 + r];
                    const float a1 = wp * q1;
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, q1, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, q1, acc[2], 0, 0, 0);
                }
                if (do_b) {
#pragma unroll
                    for (int k = 0; k < GLF_MAX_SIGNALS; ++k)
                        if (k < nplanes) {
                            const double t = ts[k * 32 + px];
                            bacc[k][0] = fma((double)q0, t, bacc[k][0]);
                            if constexpr (CW == 64) bacc[k][1] = fma((double)q1, t, bacc[k][1]);
                        }
                }
            }
        }
        if (++chained == CHAIN_TILES) {
            chain_flush(acc, dacc);
            chained = 0;
        }
    }
    chain_flush(acc, dacc);

    double *const gout = partG + ((size_t)blockIdx.x * NY + blockIdx.y) * NP * 1024;
    wave_tiles_reduce(region, dacc, wave, r, h, [&](int p, int e, double s) { gout[(size_t)p * 1024 + e] = s; });
    if (do_b) {
        double *bout = partB + ((size_t)(blockIdx.x * 4 + wave) * 2 + h) * nplanes * LD;
#pragma unroll
        for (int k = 0; k < GLF_MAX_SIGNALS; ++k)
            if (k < nplanes) {
                bout[(size_t)k * LD + cI + r] = bacc[k][0];
                if constexpr (CW == 64) bout[(size_t)k * LD + cI + 32 + r] = bacc[k][1];
            }
    }
}

// h_G [m][m] and h_b [nplanes][m] of Phi [N][ld] (returns with the stream drained)
template <class T>
static int normal_equations(glf_ctx *ctx, const T *d_phi, int64_t N, unsigned m, unsigned ld, const float *d_w, int nplanes,
                           const float *d_planes, double *h_G, double *h_b)
{
    if (!valid_ld(ld) || N < 1 || m < 1 || m > ld || nplanes < 0 || nplanes > GLF_MAX_SIGNALS)
        return set_error(ctx, GLF_ERR_INVALID, "graph_normal_equations: ld=%u m=%u nplanes=%d", ld, m, nplanes);
    const GnGeom gm = gn_geom(ld);
    const unsigned nblk = (unsigned)std::min<int64_t>(ceil_div(ceil_div(N, 32), 4), gm.xmax);
    const size_t gcols = (size_t)gm.ny * gm.slots * 1024, bcols = (size_t)nplanes * ld;
    DevBuf<double> partG, partB, dG, dB;
    GLF_TRY(partG.alloc(ctx, (size_t)nblk * gcols));
    GLF_TRY(partB.alloc(ctx, (size_t)nblk * 8 * bcols));
    dispatch_ld(ld, [&](auto LD) { // (ld is valid)
        hipLaunchKernelGGL((k_graph_normal<LD.value, T>), dim3(nblk, (unsigned)gm.ny), dim3(256), 0, ctx->stream, d_phi, N, d_w, nplanes, d_planes, partG.p,
                           partB.p);
    });
    GLF_LAUNCH_CHECK(ctx);
    GLF_TRY(sum_partials(ctx, partG, (int)nblk, gcols, dG));
    if (nplanes > 0) GLF_TRY(sum_partials(ctx, partB, (int)nblk * 8, bcols, dB));
    std::vector<double> hG(gcols), hB(bcols);
    GLF_HIP(ctx, hipMemcpyAsync(hG.data(), dG.p, sizeof(double) * gcols, hipMemcpyDeviceToHost, ctx->stream));
    if (nplanes > 0) GLF_HIP(ctx, hipMemcpyAsync(hB.data(), dB.p, sizeof(double) * bcols, hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // the upper triangle from the tiles (of a diagonal tile, its own upper triangle), the lower as its mirror
    for (int y = 0; y < gm.ny; ++y) {
        int I, J;
        gn_pair(gm.sb, y, I, J);
        for (int s = 0; s < gm.slots; ++s) {
            int ti, tj;
            if (!gn_slot_tile(ld, I, J, s, ti, tj)) continue;
            const double *t = hG.data() + ((size_t)y * gm.slots + s) * 1024;
            for (unsigned i = 0; i < 32; ++i)
                for (unsigned j = ti == tj ? i : 0; j < 32; ++j) {
                    const unsigned gi = (unsigned)ti * 32 + i, gj = (unsigned)tj * 32 + j;
                    if (gi < m && gj < m) h_G[(size_t)gi * m + gj] = h_G[(size_t)gj * m + gi] = t[i * 32 + j];
                }
        }
    }
    for (int k = 0; k < nplanes; ++k)
        for (unsigned j = 0; j < m; ++j) h_b[(size_t)k * m + j] = hB[(size_t)k * ld + j];
    return GLF_OK;
}

int graph_normal_equations(glf_ctx *ctx, const float *d_phi, int64_t N, unsigned m, unsigned ld, const float *d_w, int nplanes,
                           const float *d_planes, double *h_G, double *h_b)
{
    return normal_equations(ctx, d_phi, N, m, ld, d_w, nplanes, d_planes, h_G, h_b);
}

int graph_normal_equations(const glf_graph *g, const float *d_w, int nplanes, const float *d_planes, double *h_G, double *h_b)
{
    const int64_t N = (int64_t)g->width * g->height;
    if (g->storage != GLF_PHI_F16) return normal_equations(g->ctx, g->phi, N, g->m, g->ld, d_w, nplanes, d_planes, h_G, h_b);
    GLF_TRY(normal_equations(g->ctx, static_cast<const __half *>(g->phi16), N, g->m, g->ld, d_w, nplanes, d_planes, h_G, h_b));
    compact_fold_gram(h_G, g->m, g->expo.data());
    if (nplanes > 0) compact_fold_cols(h_b, (size_t)nplanes, g->m, g->expo.data());
    return GLF_OK;
}

} // namespace glf

extern "C" int glf_fit_coeffs(unsigned m, const double *G, const double *penalty, int nrhs, const double *b, double *a)
{
    if (!G || !b || !a || m == 0 || nrhs < 1) return GLF_ERR_INVALID;
    for (size_t e = 0; e < (size_t)m * m; ++e)
        if (!std::isfinite(G[e])) return GLF_ERR_INVALID;
    if (penalty)
        for (unsigned i = 0; i < m; ++i)
            if (!std::isfinite(penalty[i])) return GLF_ERR_INVALID;
    // L L^T = G + diag(penalty), row by row from G's lower triangle
    std::vector<double> L((size_t)m * m, 0.0);
    for (unsigned i = 0; i < m; ++i) {
        for (unsigned j = 0; j <= i; ++j) {
            double s = G[(size_t)i * m + j];
            if (i == j && penalty) s += penalty[i];
            for (unsigned k = 0; k < j; ++k) s -= L[(size_t)i * m + k] * L[(size_t)j * m + k];
            if (i == j) {
                if (!(s > 0.0)) return GLF_ERR_INVALID;
                L[(size_t)i * m + i] = std::sqrt(s);
            } else
                L[(size_t)i * m + j] = s / L[(size_t)j * m + j];
        }
    }
    std::vector<double> x((size_t)nrhs * m);
    for (int q = 0; q < nrhs; ++q) {
        double *y = x.data() + (size_t)q * m;
        for (unsigned i = 0; i < m; ++i) { // L y = b
            double s = b[(size_t)q * m + i];
            for (unsigned k = 0; k < i; ++k) s -= L[(size_t)i * m + k] * y[k];
            y[i] = s / L[(size_t)i * m + i];
        }
        for (unsigned i = m; i-- > 0;) { // L^T a = y
            double s = y[i];
            for (unsigned k = i + 1; k < m; ++k) s -= L[(size_t)k * m + i] * y[k];
            y[i] = s / L[(size_t)i * m + i];
        }
    }
    std::copy(x.begin(), x.end(), a);
    return GLF_OK;
}
