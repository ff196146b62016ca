// graph_basis.hip -- change of basis on a graph handle: Phi <- Phi T in place on the device (k_graph_transform, glf_graph_transform)
// and the driver that makes the basis orthonormal with it (glf_graph_orthonormalize: G from k_graph_normal, T from the host solve
// glf_basis_orthonormal in host_util.cpp, then the transform). Nothing else in the library writes Phi.
// Out of scope: contexts with a communicator and glf_multi_* (handles refuse them), m > 256, changing ld, a flag of the host
// program, Rayleigh-Ritz against the true Laplacian (it needs L Phi over all pixels), a faster glf_graph_gram, and anything inside
// k_band, k_graph_synthesize, k_graph_normal and k_graph_cluster*.
#include "phi_tile.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace glf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the per-call operand of k_graph_transform (device): [LD][LD] float, fl32(T[k][j]) at [k][j], zero for k >= m and j >= m_new
inline size_t gt_operand_floats(unsigned ld) { return (size_t)ld * ld; }

// Phi'[px][j] = sum_k Phi[px][k] fl32(T[k][j]) for j < m_new, exact zeros for m_new <= j < LD, written over Phi.
// One wave per tile of 32 pixels, tiles strided over a resident grid in groups of four (one per wave of the workgroup).
// The pixels are the M index (A: Phi, one pixel per lane as float4s from the padded image of phi_tile.hpp) and 32 output columns
// the N index (B: T[k][32 t + r], 32 consecutive floats of one LDS row per half-wave: no conflict). A wave keeps all LD / 32
// accumulator tiles, so a float4 of Phi feeds 4 LD / 32 MFMAs. Register g of tile t holds, in the 32 lanes of half h, columns
// 32 t .. 32 t + 31 of pixel acc_row(g, h): a store instruction writes two 128-byte row segments. The other shape -- k_graph_synthesize's, the
// outputs as the M index -- leaves one column of 32 pixels per register and needs a transpose through LDS before any row segment
// can be stored; this one stores from the accumulator as it is.
// The contraction index is visited in k_graph_synthesize's order, which depends on LD alone -- chunk by chunk of CW columns,
// half-wave h taking columns h CW / 2 + s of the chunk at step s -- and every output column is its own k-ordered fma chain: its
// bits depend neither on m_new nor on the other columns of T.
// In place: tiles are disjoint, and a wave owns its tile. Every chunk of the tile -- all LD columns of its rows -- has been loaded
// (the last one into the LDS image, the earlier ones consumed from it) before the accumulators are complete, and the first store of
// the tile comes after that; the loads that fly under the last chunk's MFMAs belong to the wave's next tile, which nobody has
// written yet. phi is one pointer, read and written, and is not __restrict__. Rows past N are staged as zeros and neither read
// nor written.
// T: LD <= 128 keeps the whole operand in LDS (4, 16, 64 KB). At LD 256 it is 256 KB and does not fit: the 32 steps of a chunk are
// then cut into two halves of 16, and the workgroup keeps the 32 rows of T a half needs (rows 16 half + s and 32 + 16 half + s of
// the chunk, 32 KB) in one of two LDS buffers. While the waves run the 128 MFMAs of a half from one buffer, every thread holds the
// next half's rows in 8 float4 registers, loaded before the MFMAs so that the loads fly under them, and writes them to the other
// buffer afterwards; one workgroup barrier per half, which every wave reaches whether or not it has a tile, separates the reads
// of a buffer from the writes that replace it and those writes from the reads that follow. The halves of T cycle 0 .. 7 through
// every group of four tiles, so the buffer of a half is its parity. The order of the steps is the resident kernels'.
// Those loads are inline assembly with a hand-placed s_waitcnt vmcnt(0) before the LDS writes, between two scheduling barriers:
// written as plain loads the compiler moved every one of them below the MFMAs, each followed at once by its wait and its
// ds_write (the ISA showed it), and with the copy exposed the transform took 8.03 ms where it now takes 6.54 ms (2048^2, ld 256,
// profiles/graph_basis_time_cfg4.json). The compiler does not count these loads; its own waits only become stricter by them
// (the counter is in order), and nothing reads tv before the hand-placed wait. A wave without a tile runs the MFMAs of a half on
// whatever its image holds and stores nothing: under `if (live)` the MFMAs would sit in a block of their own, with the
// accumulators copied in and out of it.
template <int LD, int NT, int NU>
__device__ __forceinline__ void gt_steps(f32x16 (&acc)[NT], const float *arow, const float *tk)
{
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const float4 a = *reinterpret_cast<const float4 *>(arow + 4 * u);
        const float *bk = tk + (size_t)(4 * u) * LD;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bk[0 * LD + 32 * t], acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bk[1 * LD + 32 * t], acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bk[2 * LD + 32 * t], acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bk[3 * LD + 32 * t], acc[t], 0, 0, 0);
    }
}

template <int LD>
__global__ __launch_bounds__(256) void k_graph_transform(float *phi, int64_t N, int m_new, const float *__restrict__ operand)
{
    constexpr int CW = LD < 64 ? LD : 64; // columns staged per pass
    constexpr int NCH = LD / CW;
    constexpr int PITCH = CW + 4;
    constexpr int NT = LD / 32;           // accumulator tiles
    constexpr bool RESIDENT = LD <= 128;  // all of T in LDS
    constexpr int TROWS = RESIDENT ? LD : CW; // (streamed: two buffers of CW / 2 rows)
    constexpr int HALF = (CW / 2) * LD;   // floats of one buffer of the streamed T
    constexpr int NTV = RESIDENT ? 1 : HALF / 4 / 256; // float4s of a half per thread
    __shared__ __attribute__((aligned(16))) float t_sh[TROWS * LD];
    __shared__ __attribute__((aligned(16))) float tile_sh[4][32 * PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    // streamed T: half `half` of chunk ch, local row hh 16 + s = row ch CW + hh 32 + half 16 + s of T; thread t holds float4s
    // t, t + 256, ... of the half
    f32x4 tv[NTV];
#define GT_LOAD_HALF(ch_, half_)                                                                                          \
    _Pragma("unroll") for (int i = 0; i < NTV; ++i)                                                                       \
    {                                                                                                                     \
        const int e = i * 256 + (int)threadIdx.x, lr = e / (LD / 4), c4 = e % (LD / 4);                                   \
        const int row = (ch_) * CW + (lr >> 4) * (CW / 2) + (half_) * 16 + (lr & 15);                                     \
        const float *src = operand + (size_t)row * LD + c4 * 4;                                                           \
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(tv[i]) : "v"(src) : "memory");                              \
    }
#define GT_STORE_HALF(half_)                                                                                              \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    _Pragma("unroll") for (int i = 0; i < NTV; ++i) reinterpret_cast<f32x4 *>(t_sh + (half_) * HALF)[i * 256 + threadIdx.x] = tv[i];
    if constexpr (RESIDENT) {
        for (int e = threadIdx.x; e < LD * LD / 4; e += 256) reinterpret_cast<float4 *>(t_sh)[e] = reinterpret_cast<const float4 *>(operand)[e];
    } else {
        GT_LOAD_HALF(0, 0)
        GT_STORE_HALF(0)
    }
    __syncthreads();
    float *tw = tile_sh[wave];
    const int64_t ntiles = (N + 31) / 32, tstride = (int64_t)gridDim.x * 4;
    float4 v[CW / 8];
    if ((int64_t)blockIdx.x * 4 + wave < ntiles) tile_load<CW>(v, phi, LD, 0, N, (int64_t)blockIdx.x * 4 + wave, lane);
    for (int64_t group = (int64_t)blockIdx.x * 4; group < ntiles; group += tstride) {
        const int64_t tile = group + wave;
        const bool live = tile < ntiles; // (wave-uniform)
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc_clear(acc[t]);
#pragma unroll 1
        for (int ch = 0; ch < NCH; ++ch) {
            if (live) {
                tile_store<CW, PITCH>(tw, v, lane);
                // the next chunk's loads fly under this chunk's MFMAs
                if (ch + 1 < NCH) tile_load<CW>(v, phi, LD, (ch + 1) * CW, N, tile, lane);
                else if (tile + tstride < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile + tstride, lane);
            }
            if constexpr (RESIDENT) {
                if (live) gt_steps<LD, NT, CW / 8>(acc, tw + r * PITCH + h * (CW / 2), t_sh + (size_t)(ch * CW + h * (CW / 2)) * LD + r);
            } else {
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    // the half after this one (after the last of a group, the first again: the next group's)
                    const int nch = half == 0 ? ch : ch + 1 < NCH ? ch + 1 : 0;
                    GT_LOAD_HALF(nch, half ^ 1)
                    __builtin_amdgcn_sched_barrier(0);
                    // (not under `live`: see the kernel's header)
                    gt_steps<LD, NT, CW / 16>(acc, tw + r * PITCH + h * (CW / 2) + (CW / 4) * half, t_sh + half * HALF + (size_t)(h * (CW / 4)) * LD + r);
                    __builtin_amdgcn_sched_barrier(0);
                    GT_STORE_HALF(half ^ 1)
                    __syncthreads();
                }
            }
        }
        if (live) {
            // every column of the tile's rows has been read by now: the stores may begin
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int64_t px = tile * 32 + acc_row(g, h);
                if (px < N) {
                    float *row = phi + (size_t)px * LD + r;
#pragma unroll
                    for (int t = 0; t < NT; ++t) row[32 * t] = 32 * t + r < m_new ? acc[t][g] : 0.f;
                }
            }
        }
    }
}

#undef GT_LOAD_HALF
#undef GT_STORE_HALF

// max |G - I| of an [m][m] matrix
static double gram_defect(const std::vector<double> &G, unsigned m)
{
    double worst = 0.0;
    for (unsigned i = 0; i < m; ++i)
        for (unsigned j = 0; j < m; ++j) worst = std::max(worst, std::fabs(G[(size_t)i * m + j] - (i == j ? 1.0 : 0.0)));
    return worst;
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_transform(glf_graph *g, unsigned m_new, const double *h_T, const double *h_lam_new)
{
    if (!g || !h_T || !h_lam_new) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    const unsigned m = g->m, ld = g->ld;
    if (g->storage != GLF_PHI_F32)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "glf_graph_transform: the handle is compact (compaction is the last step of preparing a handle: transform first)");
    if (m_new == 0 || m_new > m) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_transform: m_new=%u (m=%u)", m_new, m);
    if (!all_finite(h_T, (size_t)m * m_new) || !all_finite(h_lam_new, m_new))
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_transform: an entry of T or lam_new that is not finite");
    std::vector<float> h_op(gt_operand_floats(ld), 0.f);
    for (unsigned k = 0; k < m; ++k)
        for (unsigned j = 0; j < m_new; ++j) {
            const double x = h_T[(size_t)k * m_new + j];
            if (std::fabs(x) > (double)std::numeric_limits<float>::max())
                return set_error(ctx, GLF_ERR_INVALID, "glf_graph_transform: T[%u][%u] does not fit a float", k, j);
            h_op[(size_t)k * ld + j] = (float)x;
        }
    const int64_t N = (int64_t)g->width * g->height;
    GLF_ENTER(ctx);
    DevBuf<float> op;
    GLF_TRY(upload_operand(ctx, op, h_op));
    // from here on a failure leaves Phi unspecified: the handle's cached Gram matrix goes first
    g->gram.clear();
    int rc = GLF_OK;
    if (!dispatch_ld(ld, [&](auto LD) { rc = launch_tiles(g, k_graph_transform<LD.value>, N, g->phi, N, (int)m_new, (const float *)op.p); }))
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_transform: ld=%u", ld);
    GLF_TRY(rc);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (h_op and op go out of scope)
    g->m = m_new;
    g->lam.assign(h_lam_new, h_lam_new + m_new);
    return GLF_OK;
}

int glf_graph_orthonormalize(glf_graph *g, int mode, int passes, int verify, glf_basis_stats *stats)
{
    if (!g) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    if (g->storage != GLF_PHI_F32)
        return set_error(ctx, GLF_ERR_UNSUPPORTED,
                         "glf_graph_orthonormalize: the handle is compact (compaction is the last step of preparing a handle: orthonormalize first)");
    if ((mode != GLF_BASIS_CHOLESKY && mode != GLF_BASIS_RITZ) || passes < 1 || passes > 2 || (stats && stats->struct_size != sizeof(glf_basis_stats)))
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_orthonormalize: mode=%d passes=%d struct_size=%u (want %zu)", mode, passes,
                         stats ? stats->struct_size : 0u, sizeof(glf_basis_stats));
    const unsigned m = g->m;
    const int64_t N = (int64_t)g->width * g->height;
    GLF_ENTER(ctx);
    std::vector<double> G((size_t)m * m), T((size_t)m * m), lam(m);
    double defect_in = 0.0, defect_out = std::numeric_limits<double>::quiet_NaN();
    for (int pass = 0; pass < passes; ++pass) {
        GLF_TRY(graph_normal_equations(ctx, g->phi, N, m, g->ld, nullptr, 0, nullptr, G.data(), nullptr));
        if (pass == 0) defect_in = gram_defect(G, m);
        // the second pass in Cholesky mode: an upper-triangular T keeps the Ritz order of the first
        const bool ritz = mode == GLF_BASIS_RITZ && pass == 0;
        if (glf_basis_orthonormal(m, G.data(), ritz ? g->lam.data() : nullptr, T.data(), ritz ? lam.data() : nullptr) != GLF_OK)
            return set_error(ctx, GLF_ERR_INVALID, "glf_graph_orthonormalize: Phi^T Phi is not positive definite (pass %d)", pass + 1);
        if (!ritz) lam = g->lam;
        GLF_TRY(glf_graph_transform(g, m, T.data(), lam.data()));
    }
    if (verify) {
        GLF_TRY(graph_normal_equations(ctx, g->phi, N, m, g->ld, nullptr, 0, nullptr, G.data(), nullptr));
        defect_out = gram_defect(G, m);
    }
    if (stats) {
        stats->passes = (uint32_t)passes;
        stats->defect_in = defect_in;
        stats->defect_out = defect_out;
    }
    return GLF_OK;
}

} // extern "C"
