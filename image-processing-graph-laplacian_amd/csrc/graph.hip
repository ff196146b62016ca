// graph.hip -- the graph handle (glf_graph_*): the eigenbasis of one image built once, then any number of projections
// c = Phi^T s and syntheses out = ident s + Phi a on it. The build is the format's capture call with the handle's Phi as the
// capture target; Phi^T s and Phi^T Phi are filter.hip's phi_t_signals / phi_gram; the synthesis is the one new kernel.
#include "phi_tile.hpp"
#include "phi_compact.hpp"
#include "filter_rule.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>

namespace glf {

// the per-call operand block of k_graph_synthesize (device): the coefficients as the MFMA's A operand, then the identity terms
//   [LD][32] float  (float)a_j[k] at [k][j], zero for j >= nout and k >= m
//   [32] float      ident[j]
//   [32] int        plane[j] (-1: no identity term)
constexpr int GS_OUT = GLF_GRAPH_MAX_OUTPUTS;
inline size_t gs_operand_floats(unsigned ld) { return (size_t)ld * GS_OUT + 2 * GS_OUT; }

// Out[j][px] = ident[j] s_plane[j][px] + sum_k Phi[px][k] a_j[k] for all outputs j < nout in one pass over Phi.
// The outputs are the M index (A: the coefficients, from LDS), the pixels the N index (B: Phi, the padded image of phi_tile.hpp):
// register g of the accumulator holds, in the 32 lanes of half h, 32 consecutive pixels of output acc_row(g, h). The contraction index
// is visited chunk by chunk of CW columns in chunk_contract's order, which does not depend on nout, and every output is its own
// k-ordered fma chain: its bits do not depend on the outputs beside it. Rows past N are neither read nor stored.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second loader, the same image).
template <int LD, class T = float>
__global__ __launch_bounds__(256) void k_graph_synthesize(const T *__restrict__ phi, int64_t N, int nout, const float *__restrict__ operand,
                                                           const float *__restrict__ planes, float *__restrict__ out)
{
    constexpr int CW = LD < 64 ? LD : 64; // columns staged per pass
    constexpr int PITCH = CW + 4;
    __shared__ __attribute__((aligned(16))) float a_sh[LD * GS_OUT];
    __shared__ __attribute__((aligned(16))) float tile_sh[4][32 * PITCH];
    __shared__ float ident_sh[GS_OUT];
    __shared__ int plane_sh[GS_OUT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < LD * GS_OUT; e += 256) a_sh[e] = operand[e];
    if (threadIdx.x < GS_OUT) {
        ident_sh[threadIdx.x] = operand[LD * GS_OUT + threadIdx.x];
        plane_sh[threadIdx.x] = reinterpret_cast<const int *>(operand + LD * GS_OUT + GS_OUT)[threadIdx.x];
    }
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    float *tw = tile_sh[wave];
    const int64_t ntiles = (N + 31) / 32, tstride = (int64_t)gridDim.x * 4;
    tile_regs<T, CW> v;
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile, lane);
    for (; tile < ntiles; tile += tstride) {
        f32x16 acc;
        acc_clear(acc);
#pragma unroll 1
        for (int ch = 0; ch < LD / CW; ++ch) {
            tile_store<CW, PITCH>(tw, v, lane);
            // the next chunk's loads fly under this chunk's MFMAs
            if (ch + 1 < LD / CW) tile_load<CW>(v, phi, LD, (ch + 1) * CW, N, tile, lane);
            else if (tile + tstride < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile + tstride, lane);
            chunk_contract<CW, GS_OUT>(acc, tw, a_sh + (size_t)(ch * CW) * GS_OUT, r, h);
        }
        const int64_t px = tile * 32 + r;
        if (px < N) {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int j = acc_row(g, h);
                if (j < nout) {
                    float z = acc[g];
                    const int pl = plane_sh[j];
                    if (pl >= 0) z = fmaf(ident_sh[j], planes[(size_t)pl * N + px], z);
                    out[(size_t)j * N + px] = z;
                }
            }
        }
    }
}

template <class T>
__global__ void k_sample_rows(const T *__restrict__ phi, const int *__restrict__ expo, int64_t N, int ld, int dim, int nplanes,
                              const float *__restrict__ planes, const float *__restrict__ w, int wcol, int64_t ns, float *__restrict__ out)
{
    const int cols = dim + nplanes + wcol;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ns * cols) return;
    const int64_t i = e / cols;
    const int c = (int)(e % cols);
    const int64_t px = i * N / ns; // (i < ns <= N < 2^31)
    float x = 0.f;
    if (c < dim) {
        if constexpr (std::is_same<T, float>::value) x = phi[(size_t)px * ld + c];
        else x = ldexpf(__half2float(phi[(size_t)px * ld + c]), expo[c]); // Q, exact
    }
    out[e] = c < dim ? x : c < dim + nplanes ? planes[(size_t)(c - dim) * N + px] : w ? w[px] : 1.f;
}

int graph_sample_rows(glf_graph *g, int dim, int nplanes, const float *d_planes, const float *d_w, int wcol, int64_t ns, float *d_out)
{
    glf_ctx *ctx = g->ctx;
    const int64_t N = (int64_t)g->width * g->height, cnt = ns * (dim + nplanes + wcol);
    dispatch_phi(g, [&](auto *phi) {
        using T = phi_elem_t<decltype(phi)>;
        hipLaunchKernelGGL(k_sample_rows<T>, dim3((unsigned)ceil_div(cnt, 256)), dim3(256), 0, ctx->stream, phi, (const int *)g->d_expo, N, (int)g->ld, dim,
                           nplanes, d_planes, d_w, wcol, ns, d_out);
    });
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

int graph_gather_rows(glf_graph *g, int dim, unsigned nrows, const int64_t *h_px, float *d_out)
{
    glf_ctx *ctx = g->ctx;
    // the sample of one row of a one-row Phi that starts at the pixel: k_sample_rows' own reads, nothing new on the device
    dispatch_phi(g, [&](auto *phi) {
        using T = phi_elem_t<decltype(phi)>;
        for (unsigned i = 0; i < nrows; ++i)
            hipLaunchKernelGGL(k_sample_rows<T>, dim3((unsigned)ceil_div(dim, 256)), dim3(256), 0, ctx->stream, phi + (size_t)h_px[i] * g->ld,
                               (const int *)g->d_expo, (int64_t)1, (int)g->ld, dim, 0, (const float *)nullptr, (const float *)nullptr, 0, (int64_t)1,
                               d_out + (size_t)i * dim);
    });
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_destroy(glf_graph *g)
{
    if (!g) return GLF_OK;
    int rc = GLF_OK;
    if (g->phi) rc = glf_free(g->ctx, g->phi);
    if (g->phi16) {
        const int rc16 = glf_free(g->ctx, g->phi16);
        rc = rc != GLF_OK ? rc : rc16;
    }
    if (g->d_expo) {
        const int rce = glf_free(g->ctx, g->d_expo);
        rc = rc != GLF_OK ? rc : rce;
    }
    delete g;
    return rc;
}

int glf_graph_build(glf_ctx *ctx, const glf_options *opt_in, int pix, const void *d_img, int width, int height, glf_graph **graph,
                    glf_stats *stats)
{
    if (graph) *graph = nullptr;
    if (!ctx || !graph || !d_img || width <= 0 || height <= 0) return GLF_ERR_INVALID;
    if (pix < GLF_PIX_U8 || pix > GLF_PIX_RGBF32) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_build: pixel format %d", pix);
    if (ctx->has_comm || ctx->native)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "glf_graph_build: the context carries a communicator (row-sharded graph handles are not supported)");
    const PixGen gen = pixgen_of_pix(pix);
    GLF_ENTER(ctx);
    GLF_TRY(f32_admit(ctx, gen, static_cast<const uint8_t *>(d_img), width, height)); // (before the options can refuse, as in every whole-path call)
    pool_age(ctx);
    // the plan of the run below sizes Phi; its sample list stays in the handle (glf_graph_samples). Planned as the plain call, so that
    // more than 256 eigenpairs meet the handle's own refusal and not glf_capture's
    RunPlan plan;
    GLF_TRY(plan_run(ctx, opt_in, gen, width, height, false, false, &plan));
    const int64_t N = plan.N;
    const unsigned m = plan.m, ld = plan.ld;
    if (plan.wide)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "glf_graph_build: a graph handle takes at most %u eigenpairs (%u asked for)", PANEL_COLS, m);
    glf_graph *g = new (std::nothrow) glf_graph;
    if (!g) return set_error(ctx, GLF_ERR_NOMEM, "glf_graph_build: host allocation");
    g->ctx = ctx;
    g->pix = pix;
    g->width = width;
    g->height = height;
    g->lam.assign(m, 0.0);
    glf_stats S{};
    int rc;
    {
        void *d = nullptr;
        rc = glf_malloc(ctx, &d, sizeof(float) * (size_t)N * ld);
        g->phi = static_cast<float *>(d);
    }
    if (rc == GLF_OK) {
        DevBuf<uint8_t> img_out; // the call's filtered image: not kept
        rc = img_out.alloc(ctx, (size_t)N * pix_desc(gen).bytes);
        glf_capture cap{};
        cap.struct_size = sizeof(glf_capture);
        cap.d_phi = g->phi;
        cap.phi_floats = (size_t)N * ld;
        if (rc == GLF_OK) // (no float z: the handle keeps Phi and the eigenvalues only)
            rc = run_planned(ctx, plan, static_cast<const uint8_t *>(d_img), width, height, img_out.p, nullptr, g->lam.data(), &S, &cap, nullptr);
        if (rc == GLF_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = set_error(ctx, GLF_ERR_HIP, "glf_graph_build: synchronize");
    }
    if (rc != GLF_OK) {
        if (g->phi) (void)hipFree(g->phi); // (not glf_free: the failing call's message stays in last_error)
        delete g;
        return rc;
    }
    g->p = plan.p;
    g->m = m;
    g->ld = ld;
    g->samples = std::move(plan.samples);
    if (stats) *stats = S;
    *graph = g;
    return GLF_OK;
}

int glf_graph_get_info(const glf_graph *g, glf_graph_info *info)
{
    if (!g || !info || info->struct_size != sizeof(glf_graph_info)) return GLF_ERR_INVALID;
    info->pix = g->pix;
    info->width = g->width;
    info->height = g->height;
    info->p = g->p;
    info->m = g->m;
    info->ld = g->ld;
    info->d_phi = g->phi;
    info->phi_bytes = (g->storage == GLF_PHI_F16 ? sizeof(__half) : sizeof(float)) * (size_t)g->width * g->height * g->ld;
    return GLF_OK;
}

int glf_graph_eigenvalues(const glf_graph *g, double *lam)
{
    if (!g || !lam) return GLF_ERR_INVALID;
    std::memcpy(lam, g->lam.data(), sizeof(double) * g->m);
    return GLF_OK;
}

int glf_graph_gram(glf_graph *g, double *G)
{
    if (!g || !G) return GLF_ERR_INVALID;
    const unsigned m = g->m, ld = g->ld;
    if (g->gram.empty() && g->storage == GLF_PHI_F16) {
        // a compact handle: the normal-equations pass with w = NULL (no earlier bits to keep)
        GLF_ENTER(g->ctx);
        std::vector<double> hG((size_t)m * m);
        GLF_TRY(graph_normal_equations(g, nullptr, 0, nullptr, hG.data(), nullptr));
        g->gram.swap(hG);
    }
    if (g->gram.empty()) {
        glf_ctx *ctx = g->ctx;
        GLF_ENTER(ctx);
        DevBuf<double> dG;
        GLF_TRY(dG.alloc(ctx, (size_t)ld * ld));
        GLF_TRY(phi_gram(ctx, g->phi, 0, (int64_t)g->width * g->height, ld, dG.p));
        std::vector<double> hG((size_t)ld * ld);
        GLF_HIP(ctx, hipMemcpyAsync(hG.data(), dG.p, sizeof(double) * ld * ld, hipMemcpyDeviceToHost, ctx->stream));
        GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        g->gram.resize((size_t)m * m);
        for (unsigned i = 0; i < m; ++i)
            for (unsigned j = 0; j < m; ++j) g->gram[(size_t)i * m + j] = hG[(size_t)i * ld + j];
    }
    std::memcpy(G, g->gram.data(), sizeof(double) * m * m);
    return GLF_OK;
}

int glf_graph_project(glf_graph *g, int nplanes, const float *d_planes, double *h_c)
{
    if (!g || nplanes < 1 || nplanes > GLF_MAX_SIGNALS || !d_planes || !h_c) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    const unsigned m = g->m, ld = g->ld;
    const int64_t N = (int64_t)g->width * g->height;
    if (g->storage != GLF_PHI_F32)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "glf_graph_project: the handle is compact (its f64-chain kernel reads an f32 Phi): use glf_graph_project_wide");
    GLF_ENTER(ctx);
    DevBuf<double> c;
    GLF_TRY(c.alloc(ctx, (size_t)nplanes * ld));
    GLF_TRY(phi_t_signals(ctx, g->phi, d_planes, N, nplanes, 0, N, ld, c.p));
    std::vector<double> hc((size_t)nplanes * ld);
    GLF_HIP(ctx, hipMemcpyAsync(hc.data(), c.p, sizeof(double) * nplanes * ld, hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < nplanes; ++k)
        for (unsigned j = 0; j < m; ++j) h_c[(size_t)k * m + j] = hc[(size_t)k * ld + j];
    return GLF_OK;
}

int glf_graph_synthesize(glf_graph *g, int nout, const double *h_a, const float *ident, const int *plane, int nplanes, const float *d_planes,
                         float *d_out)
{
    if (!g || nout < 1 || nout > GLF_GRAPH_MAX_OUTPUTS || !h_a || !plane || !d_out || nplanes < 0) return GLF_ERR_INVALID;
    bool any_plane = false;
    if (ident_terms_check(nout, plane, nplanes, ident, d_planes, &any_plane) >= 0) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    const unsigned ld = g->ld;
    const int64_t N = (int64_t)g->width * g->height;
    GLF_ENTER(ctx);
    std::vector<float> h_op(gs_operand_floats(ld), 0.f);
    coeff_operand(g, (size_t)nout, h_a, GS_OUT, h_op.data());
    ident_terms_pack(nout, ident, plane, h_op.data() + (size_t)ld * GS_OUT);
    DevBuf<float> op;
    GLF_TRY(upload_operand(ctx, op, h_op));
    int rc = GLF_OK;
    if (!dispatch_phi_ld(g, [&](auto LD, auto *phi, auto t) {
            rc = launch_tiles(g, k_graph_synthesize<LD.value, decltype(t)>, N, phi, N, nout, (const float *)op.p, d_planes, d_out);
        }))
        return set_error(ctx, GLF_ERR_INVALID, "graph_synthesize: ld=%u", ld);
    GLF_TRY(rc);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (h_op and op go out of scope)
    return GLF_OK;
}

int glf_graph_normal_equations(glf_graph *g, const float *d_w, int nplanes, const float *d_planes, double *h_G, double *h_b)
{
    if (!g || !h_G || nplanes < 0 || nplanes > GLF_MAX_SIGNALS || (nplanes > 0 && (!d_planes || !h_b))) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    GLF_ENTER(ctx);
    return graph_normal_equations(g, d_w, nplanes, d_planes, h_G, h_b);
}

int glf_filter_coeffs(const glf_options *opt_in, unsigned m, const double *lam, const double *gram, const double *c, double *a, float *ident)
{
    if (!lam || !c || !a || !ident) return GLF_ERR_INVALID;
    glf_options opt;
    glf_options_default(&opt);
    if (opt_in) {
        if (opt_in->struct_size != sizeof(glf_options)) return GLF_ERR_INVALID;
        opt = *opt_in;
    }
    if (opt.filter_mode < GLF_FILTER_REFERENCE || opt.filter_mode > GLF_FILTER_SHARPEN) return GLF_ERR_INVALID;
    // the whole path's rule (filter_rule.hpp), the gain folded into the coefficients
    if (opt.filter_mode == GLF_FILTER_SHARPEN) {
        if (!gram) return GLF_ERR_INVALID;
        sharpen_weights(m, lam, gram, m, (double)opt.filter_beta, c, a);
    } else {
        const double gain = (double)filter_gain(opt);
        for (unsigned j = 0; j < m; ++j) a[j] = gain * filter_response(opt, lam[j]) * c[j];
    }
    *ident = filter_ident(opt);
    return GLF_OK;
}

} // extern "C"
