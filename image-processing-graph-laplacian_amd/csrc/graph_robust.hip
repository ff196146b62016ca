// graph_robust.hip -- the robust fit on a graph handle: iteratively reweighted least squares under Huber, Cauchy and Tukey losses.
// One iteration's device work (glf_graph_robust_step) is the per-pixel weight w_eff = w u(q) of the residuals at the previous
// iterate (k_graph_residual_weight: one pass over Phi on k_graph_synthesize's MFMA shape, the weight function as its epilogue), then
// graph_fit.hip's own pass over Phi with w_eff as the weight plane (graph_normal_equations, untouched). glf_graph_fit_robust drives
// the steps from the plain weighted fit; the host-only table and scale estimate (glf_robust_weight, glf_robust_scale) are in
// host_util.cpp, the losses as functions of q in robust_loss.hpp.
// Out of scope: per-plane independent weights in one call, a device-side median, L1 / total-variation terms, m > 256, contexts with a
// communicator and glf_multi_* (handles refuse them), a flag of the host program, and anything inside k_graph_normal,
// k_graph_synthesize, k_graph_cluster and k_graph_transform.
#include "phi_tile.hpp"
#include "phi_compact.hpp"
#include "robust_loss.hpp"

#include <algorithm>
#include <cmath>

// the arithmetic of the weight is pinned operation by operation (include/glf.h): nothing here is contracted into an fma that the
// text does not spell out
#pragma clang fp contract(off)

namespace glf {

constexpr int GR_OUT = GLF_MAX_SIGNALS; // residual planes = the first rows of the M index
static_assert(GR_OUT == 4, "accumulator registers 0..3 of half-wave 0 hold the planes");

// the constants of a step, by value
struct RobustConst {
    int kind;
    float cf, c2, ic2;   // fl32(c), fl32(c^2), fl32(1 / c^2)
    double c;
    float isig[GR_OUT];  // fl32(1 / sigma_k)
};

// u(q) in f32, selects only (no branch: it is inlined behind an unrolled MFMA region)
__device__ inline float robust_u32(int kind, float q, float cf, float c2, float ic2)
{
    const float huber = q <= c2 ? 1.f : cf / sqrtf(q);
    const float cauchy = 1.f / fmaf(q, ic2, 1.f);
    const float t = q * ic2;
    const float tukey = t < 1.f ? (1.f - t) * (1.f - t) : 0.f;
    return kind == ROBUST_HUBER ? huber : kind == ROBUST_CAUCHY ? cauchy : tukey;
}

// res_k[px] = s_k[px] - sum_c Phi[px][c] fl32(a_k[c]) for the planes k < nplanes, and from them the IRLS weight of the pixel, in one
// pass over Phi. The contraction is k_graph_synthesize's, the same chunk_contract (phi_tile.hpp): the planes are the M index (A: the
// coefficients, operand [LD][4] float with fl32(a_k[c]) at [c][k], read from LDS by the lanes r < 4, zero in the others), the pixels
// the N index. Register k of lane (r, 0) then holds d_k of pixel r with the bits glf_graph_synthesize gives for a_k with no
// identity term. Epilogue, lanes of half 0, in f32: res_k = s_k - d_k, x_k = res_k isig_k, q = fmaf(x_k, x_k, q) in ascending k,
// u = robust_u32(q), w_eff = w u; rho in f64 from (double) q (robust_rho, the host table's own statement), loss += (double) w rho and
// mass += (double) w_eff per lane. Rows past N are neither read nor stored nor summed.
// part[blockIdx.x][2] = (loss, mass) of the workgroup: the lanes of wave 0 first, in ascending lane order; no atomics, the
// workgroups are added by k_cols_sum.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second loader, the same image).
template <int LD, class T = float>
__global__ __launch_bounds__(256) void k_graph_residual_weight(const T *__restrict__ phi, int64_t N, int nplanes, const float *__restrict__ operand,
                                                                RobustConst rc, const float *__restrict__ w, const float *__restrict__ planes,
                                                                float *__restrict__ weight_out, float *__restrict__ res_out,
                                                                double *__restrict__ part)
{
    constexpr int CW = LD < 64 ? LD : 64; // columns staged per pass
    constexpr int PITCH = CW + 4;
    __shared__ __attribute__((aligned(16))) float a_sh[LD * GR_OUT];
    __shared__ __attribute__((aligned(16))) float tile_sh[4][32 * PITCH];
    __shared__ double red_sh[2][4][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < LD * GR_OUT; e += 256) a_sh[e] = operand[e];
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    float *tw = tile_sh[wave];
    const int64_t ntiles = (N + 31) / 32, tstride = (int64_t)gridDim.x * 4;
    double loss = 0.0, mass = 0.0;
    tile_regs<T, CW> v;
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile, lane);
    for (; tile < ntiles; tile += tstride) {
        // the pixel's planes and weight fly under the tile's MFMAs
        const int64_t px = tile * 32 + r;
        const bool live = h == 0 && px < N;
        float sv[GR_OUT], wv = 1.f;
#pragma unroll
        for (int k = 0; k < GR_OUT; ++k) sv[k] = live && k < nplanes ? planes[(size_t)k * N + px] : 0.f;
        if (live && w) wv = w[px];
        f32x16 acc;
        acc_clear(acc);
#pragma unroll 1
        for (int ch = 0; ch < LD / CW; ++ch) {
            tile_store<CW, PITCH>(tw, v, lane);
            // the next chunk's loads fly under this chunk's MFMAs
            if (ch + 1 < LD / CW) tile_load<CW>(v, phi, LD, (ch + 1) * CW, N, tile, lane);
            else if (tile + tstride < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile + tstride, lane);
            chunk_contract<CW, GR_OUT>(acc, tw, a_sh + (size_t)(ch * CW) * GR_OUT, r, h);
        }
        if (live) {
            float q = 0.f;
#pragma unroll
            for (int k = 0; k < GR_OUT; ++k)
                if (k < nplanes) {
                    const float res = sv[k] - acc[k];
                    if (res_out) res_out[(size_t)k * N + px] = res;
                    const float x = res * rc.isig[k];
                    q = fmaf(x, x, q);
                }
            const float weff = wv * robust_u32(rc.kind, q, rc.cf, rc.c2, rc.ic2);
            weight_out[px] = weff;
            const double lterm = (double)wv * robust_rho(rc.kind, rc.c, (double)q);
            loss += lterm;
            mass += (double)weff;
        }
    }
    if (h == 0) {
        red_sh[0][wave][r] = loss;
        red_sh[1][wave][r] = mass;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *x = &red_sh[threadIdx.x][0][0];
        double s = 0.0;
        for (int e = 0; e < 4 * 32; ++e) s += x[e];
        part[(size_t)blockIdx.x * 2 + threadIdx.x] = s;
    }
}

// what the step and the driver refuse alike, before any device work
static bool loss_shape_ok(const glf_robust_loss *loss, int nplanes, bool with_sigma)
{
    if (!loss || loss->struct_size != sizeof(glf_robust_loss) || loss->kind < 0 || loss->kind >= ROBUST_KINDS) return false;
    if (!std::isfinite(loss->c) || loss->c < 0.0) return false;
    for (int k = 0; with_sigma && k < nplanes; ++k)
        if (!std::isfinite(loss->sigma[k]) || !(loss->sigma[k] > 0.0)) return false;
    return true;
}

static RobustConst robust_const(int kind, double c, const double *sigma, int nplanes)
{
    RobustConst rc{};
    rc.kind = kind;
    rc.c = c == 0.0 ? robust_default_c(kind) : c;
    rc.cf = (float)rc.c;
    rc.c2 = (float)(rc.c * rc.c);
    rc.ic2 = (float)(1.0 / (rc.c * rc.c));
    for (int k = 0; k < nplanes; ++k) rc.isig[k] = (float)(1.0 / sigma[k]);
    return rc;
}

// one IRLS iteration's device work on checked arguments (returns with the stream drained)
static int robust_step(glf_graph *g, const RobustConst &rc, const float *d_w, int nplanes, const float *d_planes, const double *h_a, double *h_G,
                       double *h_b, double *h_loss, double *h_mass, float *d_weight_out, float *d_res_out)
{
    glf_ctx *ctx = g->ctx;
    const unsigned ld = g->ld;
    const int64_t N = (int64_t)g->width * g->height;
    // (a compact handle: the refusal of a coefficient that is not finite applies to the folded values)
    std::vector<float> h_op((size_t)ld * GR_OUT, 0.f);
    const std::vector<double> a = coeff_operand(g, (size_t)nplanes, h_a, GR_OUT, h_op.data());
    if (!all_finite(a.data(), a.size())) return set_error(ctx, GLF_ERR_INVALID, "robust step: a coefficient folded with its column's 2^e_c is not finite");
    DevBuf<float> op, weff;
    DevBuf<double> part, tot;
    GLF_TRY(upload_operand(ctx, op, h_op));
    if (!d_weight_out) {
        GLF_TRY(weff.alloc(ctx, (size_t)N));
        d_weight_out = weff.p;
    }
    int64_t nblk = 0;
    int rc_launch = GLF_ERR_INVALID;
    dispatch_phi_ld(g, [&](auto LD, auto *phi, auto t) {
        rc_launch = launch_tiles_partials(g, k_graph_residual_weight<LD.value, decltype(t)>, N, part, 2, &nblk, phi, N, nplanes, (const float *)op.p, rc, d_w,
                                          d_planes, d_weight_out, d_res_out);
    });
    GLF_TRY(rc_launch);
    std::vector<double> h_tot;
    GLF_TRY(sum_partials_to_host(ctx, part, (int)nblk, 2, tot, h_tot, false));
    // the second pass: G and b under w_eff, by the weighted fit's own kernel (it drains the stream; h_op and h_tot are then settled)
    GLF_TRY(graph_normal_equations(g, d_weight_out, nplanes, d_planes, h_G, h_b));
    if (h_loss) *h_loss = h_tot[0];
    if (h_mass) *h_mass = h_tot[1];
    return GLF_OK;
}

// The penalty's share of the objective the iteration decreases. The step a <- (G + diag(penalty))^-1 b minimises, plane by plane,
// sum_px w_eff res_k^2 + a_k^T diag(penalty) a_k: the penalty is in the units of the plain weighted fit (with every u = 1 the step is
// that fit). The loss counts a residual in units of sigma_k and halves its square (rho = q / 2 where u = 1), so in the loss's units
// the penalty of plane k is a_k^T diag(penalty) a_k / (2 sigma_k^2).
static double penalty_term(const double *penalty, const double *sigma, const double *a, unsigned m, int nplanes)
{
    double s = 0.0;
    for (int k = 0; penalty && k < nplanes; ++k) {
        double sk = 0.0;
        for (unsigned j = 0; j < m; ++j) sk += penalty[j] * a[(size_t)k * m + j] * a[(size_t)k * m + j];
        s += sk / (2.0 * sigma[k] * sigma[k]);
    }
    return s;
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_robust_step(glf_graph *g, const glf_robust_loss *loss, const float *d_w, int nplanes, const float *d_planes, const double *h_a,
                          double *h_G, double *h_b, double *h_loss, double *h_mass, float *d_weight_out, float *d_res_out)
{
    if (!g || !loss || !d_planes || !h_a || !h_G || !h_b || nplanes < 1 || nplanes > GLF_MAX_SIGNALS) return GLF_ERR_INVALID;
    if (!loss_shape_ok(loss, nplanes, true) || !all_finite(h_a, (size_t)nplanes * g->m))
        return set_error(g->ctx, GLF_ERR_INVALID,
                         "glf_graph_robust_step: struct_size=%u (want %zu) kind=%d c=%g, or a sigma that is not positive and finite, or a "
                         "coefficient that is not finite",
                         loss->struct_size, sizeof(glf_robust_loss), loss->kind, loss->c);
    GLF_ENTER(g->ctx);
    return robust_step(g, robust_const(loss->kind, loss->c, loss->sigma, nplanes), d_w, nplanes, d_planes, h_a, h_G, h_b, h_loss, h_mass,
                       d_weight_out, d_res_out);
}

int glf_graph_fit_robust(glf_graph *g, const glf_robust_options *opt, const float *d_w, int nplanes, const float *d_planes, double *h_a,
                         float *d_fit_out, float *d_weight_out, glf_robust_stats *stats)
{
    if (!g || !opt || !d_planes || !h_a || nplanes < 1 || nplanes > GLF_MAX_SIGNALS || opt->struct_size != sizeof(glf_robust_options)) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    const unsigned m = g->m;
    const int64_t N = (int64_t)g->width * g->height;
    const bool estimate = opt->estimate_sigma == 1;
    bool ok = (opt->estimate_sigma == 0 || estimate) && loss_shape_ok(&opt->loss, nplanes, !estimate) && std::isfinite(opt->tol) && opt->tol >= 0.0 &&
              (!stats || stats->struct_size == sizeof(glf_robust_stats));
    for (unsigned j = 0; ok && opt->penalty && j < m; ++j) ok = std::isfinite(opt->penalty[j]) && opt->penalty[j] >= 0.0;
    if (!ok)
        return set_error(ctx, GLF_ERR_INVALID,
                         "glf_graph_fit_robust: a struct_size, kind=%d c=%g estimate_sigma=%d tol=%g, or a sigma that is not positive and finite, "
                         "or a penalty that is negative or not finite",
                         opt->loss.kind, opt->loss.c, opt->estimate_sigma, opt->tol);
    const unsigned max_iter = opt->max_iter ? opt->max_iter : 20;
    const double tol = opt->tol > 0.0 ? opt->tol : 1e-6;
    GLF_ENTER(ctx);
    // a_0: the plain weighted fit
    const size_t na = (size_t)nplanes * m;
    std::vector<double> G((size_t)m * m), b(na), a(na), a_new(na);
    GLF_TRY(graph_normal_equations(g, d_w, nplanes, d_planes, G.data(), b.data()));
    if (glf_fit_coeffs(m, G.data(), opt->penalty, nplanes, b.data(), a.data()) != GLF_OK)
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_fit_robust: the plain weighted system is not positive definite (pass a penalty)");
    double sigma[GLF_MAX_SIGNALS] = {0.0, 0.0, 0.0, 0.0};
    if (estimate) {
        const int64_t ns = std::min<int64_t>(opt->sample_rows ? opt->sample_rows : 4096, N);
        const int cols = (int)m + nplanes + 1;
        const size_t cnt = (size_t)ns * cols;
        DevBuf<float> d_rows;
        GLF_TRY(d_rows.alloc(ctx, cnt));
        GLF_TRY(graph_sample_rows(g, (int)m, nplanes, d_planes, d_w, 1, ns, d_rows.p));
        std::vector<float> h_rows(cnt);
        GLF_HIP(ctx, hipMemcpyAsync(h_rows.data(), d_rows.p, sizeof(float) * cnt, hipMemcpyDeviceToHost, ctx->stream));
        GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<double> res((size_t)ns), ws((size_t)ns);
        for (int k = 0; k < nplanes; ++k) {
            for (int64_t i = 0; i < ns; ++i) {
                const float *row = h_rows.data() + (size_t)i * cols;
                double d = 0.0;
                for (unsigned c = 0; c < m; ++c) d += (double)row[c] * a[(size_t)k * m + c];
                res[(size_t)i] = (double)row[m + k] - d;
                ws[(size_t)i] = (double)row[m + nplanes];
            }
            if (glf_robust_scale(res.data(), ws.data(), (size_t)ns, &sigma[k]) != GLF_OK)
                return set_error(ctx, GLF_ERR_INVALID,
                                 "glf_graph_fit_robust: no scale for plane %d from %lld sampled rows (a median residual of 0, no sampled pixel of "
                                 "positive weight, or a value that is not finite): pass sigma",
                                 k, (long long)ns);
        }
    } else
        std::copy(opt->loss.sigma, opt->loss.sigma + nplanes, sigma);
    const RobustConst rc = robust_const(opt->loss.kind, opt->loss.c, sigma, nplanes);
    glf_robust_stats st{};
    st.struct_size = sizeof(glf_robust_stats);
    std::copy(sigma, sigma + GLF_MAX_SIGNALS, st.sigma);
    int status = GLF_OK;
    while (st.iterations < max_iter && !st.converged) {
        double loss = 0.0, mass = 0.0;
        GLF_TRY(robust_step(g, rc, d_w, nplanes, d_planes, a.data(), G.data(), b.data(), &loss, &mass, d_weight_out, nullptr));
        if (st.iterations < GLF_ROBUST_OBJECTIVES) st.objective[st.iterations] = loss + penalty_term(opt->penalty, sigma, a.data(), m, nplanes);
        st.mass = mass;
        ++st.iterations;
        if (glf_fit_coeffs(m, G.data(), opt->penalty, nplanes, b.data(), a_new.data()) != GLF_OK) {
            status = set_error(ctx, GLF_ERR_INVALID, "glf_graph_fit_robust: the reweighted system of step %u is not positive definite (mass %g): pass a penalty",
                               st.iterations, mass);
            break;
        }
        double dmax = 0.0, amax = 0.0;
        for (size_t e = 0; e < na; ++e) {
            dmax = std::max(dmax, std::fabs(a_new[e] - a[e]));
            amax = std::max(amax, std::fabs(a_new[e]));
        }
        a.swap(a_new);
        st.converged = dmax <= tol * amax;
    }
    std::copy(a.begin(), a.end(), h_a);
    if (stats) *stats = st;
    if (d_fit_out) {
        const int none[GLF_MAX_SIGNALS] = {-1, -1, -1, -1};
        GLF_TRY(glf_graph_synthesize(g, nplanes, a.data(), nullptr, none, 0, nullptr, d_fit_out));
    }
    return status;
}

} // extern "C"
