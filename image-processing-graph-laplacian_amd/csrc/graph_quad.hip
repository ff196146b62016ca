// graph_quad.hip -- per-pixel quadratic forms on a graph handle: q_k(px) = |R^T phi_px - t_k|^2 for up to GLF_QUAD_MAX_CENTRES
// centres t_k under one shared R of up to GLF_QUAD_MAX_COLS columns, in one pass over Phi (k_graph_quadform). The leverage of a fit
// (R = L^-T of the penalised normal matrix, glf_fit_factor in host_util.cpp), the diffusion distance from seed pixels (R = diag(g))
// and the squared distances to centroids under a shared metric are this form. The contraction is k_graph_synthesize's; the new part
// is the epilogue, which squares and sums in registers and writes ncent planes instead of r.
// Out of scope: r > 64 per launch (the Python wrapper groups), per-centre metrics in one call, unit-length rows, soft memberships (a
// softmax over the output in torch), contexts with a communicator and glf_multi_* (handles refuse them), m > 256, a flag of the host
// program, and anything inside k_graph_synthesize, k_graph_normal and k_graph_residual_weight.
#include "phi_tile.hpp"
#include "phi_compact.hpp"

#include <algorithm>
#include <cmath>

// the arithmetic of the epilogue is pinned operation by operation (include/glf.h): nothing here is contracted into an fma that the
// text does not spell out
#pragma clang fp contract(off)

namespace glf {

constexpr int GQ_COLS = GLF_QUAD_MAX_COLS;     // columns of R in one launch: two accumulator tiles
constexpr int GQ_CENT = GLF_QUAD_MAX_CENTRES;  // centres of one launch
static_assert(GQ_COLS == 64 && GQ_CENT == 32, "two 32-row tiles of the M index; the centre image is [32][2][32] floats at most");

// the per-call operand block of k_graph_quadform<LD, T, NB> (device):
//   [NB][LD][32] float  fl32(R[j][32 b + cc]) at [b][j][cc], zero for columns >= r and rows >= m
//   [ncent][2][16 NB] float  the centres in register order: fl32(t_k[32 b + acc_row(g, h)]) at [k][h][16 b + g], zero for columns >= r
inline size_t gq_operand_floats(unsigned ld, int nb, unsigned ncent) { return (size_t)nb * ld * 32 + (size_t)ncent * 32 * nb; }

// out[k][px] (+)= sum_c (y_c(px) - t_k[c])^2, y_c(px) = sum_j Phi[px][j] fl32(R[j][c]), for the centres k < ncent in one pass over Phi.
// The contraction is k_graph_synthesize's, the same chunk_contract (phi_tile.hpp): the columns of R are the M index (A: NB operand
// blocks [LD][32] in LDS, one accumulator tile each), the pixels the N index. Register g of tile b of lane (r, h) then holds y_c of
// pixel r for c = 32 b + acc_row(g, h), with the bits glf_graph_synthesize gives for the coefficient column R[:, c] with no identity
// term. Epilogue, all lanes, in f32: per centre q = 0, then x = y_c - t_k[c], q = fmaf(x, x, q) over b ascending and g ascending
// (the lane's 16 NB columns; t from LDS in that order, four per read, the address uniform over a half-wave); the two half-waves are
// added by q + __shfl_xor(q, 32) (one f32 addition, commutative: both halves hold the same bits) and half 0 stores q, or out + q
// with one f32 addition under accumulate. The order depends on NB alone, not on ncent nor r: a column that is zero in R and in every
// t gives x = 0 and fmaf(0, 0, q) = q. No atomics. Rows past N are neither read nor stored.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second loader, the same image).
template <int LD, class T, int NB>
__global__ __launch_bounds__(256) void k_graph_quadform(const T *__restrict__ phi, int64_t N, int ncent, int accumulate,
                                                         const float *__restrict__ operand, float *__restrict__ out)
{
    constexpr int CW = LD < 64 ? LD : 64; // columns staged per pass
    constexpr int PITCH = CW + 4;
    constexpr int TL = 16 * NB;           // floats of one centre per half-wave
    __shared__ __attribute__((aligned(16))) float a_sh[NB * LD * 32];
    __shared__ __attribute__((aligned(16))) float tile_sh[4][32 * PITCH];
    __shared__ __attribute__((aligned(16))) float t_sh[GQ_CENT * 2 * TL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < NB * LD * 32; e += 256) a_sh[e] = operand[e];
    for (int e = threadIdx.x; e < ncent * 2 * TL; e += 256) t_sh[e] = operand[NB * LD * 32 + e];
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    float *tw = tile_sh[wave];
    const int64_t ntiles = (N + 31) / 32, tstride = (int64_t)gridDim.x * 4;
    tile_regs<T, CW> v;
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile, lane);
    for (; tile < ntiles; tile += tstride) {
        f32x16 acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc_clear(acc[b]);
#pragma unroll 1
        for (int ch = 0; ch < LD / CW; ++ch) {
            tile_store<CW, PITCH>(tw, v, lane);
            // the next chunk's loads fly under this chunk's MFMAs
            if (ch + 1 < LD / CW) tile_load<CW>(v, phi, LD, (ch + 1) * CW, N, tile, lane);
            else if (tile + tstride < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile + tstride, lane);
#pragma unroll
            for (int b = 0; b < NB; ++b) chunk_contract<CW, 32>(acc[b], tw, a_sh + (size_t)(b * LD + ch * CW) * 32, r, h);
        }
        const int64_t px = tile * 32 + r;
        const bool live = h == 0 && px < N;
#pragma unroll 1
        for (int k = 0; k < ncent; ++k) {
            const float4 *tk = reinterpret_cast<const float4 *>(t_sh + (size_t)(k * 2 + h) * TL);
            float q = 0.f;
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const float4 t = tk[b * 4 + g4];
                    const float x0 = acc[b][4 * g4 + 0] - t.x;
                    q = fmaf(x0, x0, q);
                    const float x1 = acc[b][4 * g4 + 1] - t.y;
                    q = fmaf(x1, x1, q);
                    const float x2 = acc[b][4 * g4 + 2] - t.z;
                    q = fmaf(x2, x2, q);
                    const float x3 = acc[b][4 * g4 + 3] - t.w;
                    q = fmaf(x3, x3, q);
                }
            q = q + __shfl_xor(q, 32);
            if (live) {
                float *o = out + (size_t)k * N + px;
                *o = accumulate ? *o + q : q;
            }
        }
    }
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_quadform(glf_graph *g, unsigned r, const double *h_R, unsigned ncent, const double *h_t, int accumulate, float *d_out)
{
    if (!g || !h_R || !d_out || r == 0 || r > (unsigned)GQ_COLS || ncent == 0 || ncent > (unsigned)GQ_CENT) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    const unsigned m = g->m, ld = g->ld;
    const int64_t N = (int64_t)g->width * g->height;
    // the coefficient vectors are the columns of R: rt[c][j] = R[j][c], 32 of them per operand block (a compact handle: the column
    // scales of Phi folded into the rows of R in f64, before their fl32: coeff_operand's rule; the centres live in the space of
    // R^T phi and take no scale)
    std::vector<double> rt((size_t)r * m);
    for (unsigned j = 0; j < m; ++j)
        for (unsigned c = 0; c < r; ++c) rt[(size_t)c * m + j] = h_R[(size_t)j * r + c];
    const int nb = r > 32 ? 2 : 1;
    std::vector<float> h_op(gq_operand_floats(ld, nb, ncent), 0.f);
    bool fits = !h_t || all_fl32_finite(h_t, (size_t)ncent * r);
    for (int b = 0; b < nb; ++b) {
        const size_t cols = std::min(r - 32u * b, 32u);
        const std::vector<double> a = coeff_operand(g, cols, rt.data() + (size_t)32 * b * m, 32, h_op.data() + (size_t)b * ld * 32);
        fits = fits && all_fl32_finite(a.data(), a.size());
    }
    if (!fits)
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_quadform: an entry of R (folded with its column's 2^e_c) or of t is not finite in f32");
    GLF_ENTER(ctx);
    float *t_op = h_op.data() + (size_t)nb * ld * 32;
    for (unsigned k = 0; h_t && k < ncent; ++k)
        for (int h = 0; h < 2; ++h)
            for (int b = 0; b < nb; ++b)
                for (int q = 0; q < 16; ++q) {
                    const unsigned c = 32u * b + (unsigned)acc_row(q, h);
                    if (c < r) t_op[((size_t)k * 2 + h) * 16 * nb + 16 * b + q] = (float)h_t[(size_t)k * r + c];
                }
    DevBuf<float> op;
    GLF_TRY(upload_operand(ctx, op, h_op));
    int rc = GLF_ERR_INVALID;
    dispatch_phi_ld(g, [&](auto LD, auto *phi, auto t) {
        rc = nb == 2 ? launch_tiles(g, k_graph_quadform<LD.value, decltype(t), 2>, N, phi, N, (int)ncent, (int)(accumulate != 0), (const float *)op.p, d_out)
                     : launch_tiles(g, k_graph_quadform<LD.value, decltype(t), 1>, N, phi, N, (int)ncent, (int)(accumulate != 0), (const float *)op.p, d_out);
    });
    GLF_TRY(rc);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (h_op and op go out of scope)
    return GLF_OK;
}

int glf_graph_rows(glf_graph *g, unsigned nrows, const int64_t *h_px, float *h_rows)
{
    if (!g || !h_px || !h_rows || nrows == 0 || nrows > (unsigned)GQ_CENT) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    const unsigned m = g->m;
    const int64_t N = (int64_t)g->width * g->height;
    for (unsigned i = 0; i < nrows; ++i)
        if (h_px[i] < 0 || h_px[i] >= N) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_rows: pixel %lld outside 0 .. %lld", (long long)h_px[i], (long long)N);
    GLF_ENTER(ctx);
    DevBuf<float> d_rows;
    GLF_TRY(d_rows.alloc(ctx, (size_t)nrows * m));
    GLF_TRY(graph_gather_rows(g, (int)m, nrows, h_px, d_rows.p));
    std::vector<float> rows((size_t)nrows * m);
    GLF_HIP(ctx, hipMemcpyAsync(rows.data(), d_rows.p, sizeof(float) * rows.size(), hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::copy(rows.begin(), rows.end(), h_rows);
    return GLF_OK;
}

} // extern "C"
