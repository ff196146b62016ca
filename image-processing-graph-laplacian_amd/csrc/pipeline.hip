// pipeline.hip -- the C-ABI stage entry points (mirror of hpc/*.h) and the whole
// approximate path glf_image_processing (hpc/image_processing.c:183-277).
#include "glf_internal.hpp"
#include "filter_rule.hpp"

#include <cmath>
#include <cstring>
#include <cstdlib>
#include <atomic>
#include <thread>

namespace glf {

static void shard_rows(const glf_ctx *ctx, int height, int *row0, int *row1)
{
    const int G = ctx->has_comm ? ctx->comm.size : 1, g = ctx->has_comm ? ctx->comm.rank : 0;
    (void)glf_shard_rows(height, g, G, row0, row1);
}

static int allreduce_f64(glf_ctx *ctx, double *d, size_t n)
{
    if (!ctx->has_comm) return GLF_OK;
    if (ctx->comm.allreduce_sum_f64(ctx->comm.user, d, n) != 0)
        return set_error(ctx, GLF_ERR_COMM, "allreduce_sum_f64 callback failed");
    return GLF_OK;
}

// Psi[i][j] = scale * Phi_A[i][j] * pinv[j]   (part_lower = phi_A * Pi^-1, hpc/nystroem.c:41; scale = -alpha)
// X[s][0] = y_s (the sample's pixel value) in a block of `ld` columns (the others stay zero)
__global__ void k_sample_values_column(const float4 *__restrict__ samples, unsigned p, unsigned ld, float *__restrict__ X)
{
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < p) X[(size_t)s * ld] = samples[s].z;
}

// t[s][0] = D_s y_s - t[s][0] / alpha: K_A y_A from (L_A y_A) with L_A = alpha (D - K_A)
__global__ void k_ka_from_la(const float4 *__restrict__ samples, const double *__restrict__ degree, unsigned p, unsigned ld, double inv_alpha,
                             float *__restrict__ T)
{
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < p) T[(size_t)s * ld] = (float)(degree[s] * (double)samples[s].z - (double)T[(size_t)s * ld] * inv_alpha);
}

// X[s][k] = s_k at sample s (block of `ld` columns, the others stay zero): the planes' sample values for t_s = K_A s_A
__global__ void k_sample_signal_columns(const uint32_t *__restrict__ idx, const float *__restrict__ sig, int64_t N, int nsig, unsigned p,
                                        unsigned ld, float *__restrict__ X)
{
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < p)
        for (int k = 0; k < nsig; ++k) X[(size_t)s * ld + k] = sig[(size_t)k * N + idx[s]];
}

__global__ void k_make_psi(const float *__restrict__ phiA, const float *__restrict__ pinv, unsigned p, unsigned ld, unsigned m,
                           float scale, float *__restrict__ psi)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned i = (unsigned)(e / ld), j = (unsigned)(e % ld);
    if (i >= p) return;
    psi[e] = (j < m) ? scale * (phiA[e] * pinv[j]) : 0.f;
}

// Jacobi preconditioner of L_A without the matrix: 1 / (alpha (D_i - K_ii)), K_ii = 1 (hpc/laplacian.c:31-35)
__global__ void k_dinv_from_degree(const double *__restrict__ degree, unsigned p, double alpha, float *__restrict__ dinv)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < p) dinv[i] = 1.0f / (float)(alpha * (degree[i] - 1.0));
}

__global__ void k_diag_inverse(const float *__restrict__ x, unsigned n, float *__restrict__ y)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = 1.0f / x[i]; // InverseDiagMat, hpc/utils.c:578-579
}

// 256-column panel q of a row-major [rows][ld_total] matrix <-> a contiguous [rows][256] block (m > 256, see eigen.hip "panels")
static int pack_panel(glf_ctx *ctx, const float *rm, int64_t ld_total, int64_t rows, unsigned q, float *panel)
{
    GLF_HIP(ctx, hipMemcpy2DAsync(panel, sizeof(float) * PANEL_COLS, rm + (size_t)q * PANEL_COLS, sizeof(float) * (size_t)ld_total,
                                  sizeof(float) * PANEL_COLS, (size_t)rows, hipMemcpyDeviceToDevice, ctx->stream));
    return GLF_OK;
}
static int unpack_panel(glf_ctx *ctx, const float *panel, int64_t ld_total, int64_t rows, unsigned q, float *rm)
{
    GLF_HIP(ctx, hipMemcpy2DAsync(rm + (size_t)q * PANEL_COLS, sizeof(float) * (size_t)ld_total, panel, sizeof(float) * PANEL_COLS,
                                  sizeof(float) * PANEL_COLS, (size_t)rows, hipMemcpyDeviceToDevice, ctx->stream));
    return GLF_OK;
}

static int sum_host(glf_ctx *ctx, const double *d_v, unsigned n, double *out)
{
    std::vector<double> h(n);
    GLF_HIP(ctx, hipMemcpyAsync(h.data(), d_v, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double s = 0.0;
    for (unsigned i = 0; i < n; ++i) s += h[i];
    *out = s;
    return GLF_OK;
}

int f32_admit(glf_ctx *ctx, PixGen gen, const uint8_t *d_img, int width, int height)
{
    if (!pix_desc(gen).is_float) return GLF_OK;
    bool finite = true;
    GLF_TRY(f32_all_finite(ctx, reinterpret_cast<const float *>(d_img), (int64_t)width * height * pix_desc(gen).channels, &finite));
    if (!finite) return set_error(ctx, GLF_ERR_INVALID, "the %s image holds a NaN or an Inf: finite values only", pix_desc(gen).name);
    return GLF_OK;
}

// The filter's weights from c = Phi^T y: fetches d_c ([k][ld] f64), forms k rows of ld f32 weights -- row(c_r, w_r) writes a row's
// live entries, the rest stay zero -- and uploads them to d_w; h_c0 (optional) takes a copy of the first row of c. Both copies synchronise.
template <class Row>
static int weights_from_c(glf_ctx *ctx, const double *d_c, int k, unsigned ld, Row row, float *d_w, double *h_c0 = nullptr)
{
    std::vector<double> hc((size_t)k * ld);
    GLF_TRY(glf_memcpy_d2h(ctx, hc.data(), d_c, sizeof(double) * hc.size()));
    if (h_c0) std::memcpy(h_c0, hc.data(), sizeof(double) * ld);
    std::vector<float> hw((size_t)k * ld, 0.f);
    for (int r = 0; r < k; ++r) row(hc.data() + (size_t)r * ld, hw.data() + (size_t)r * ld);
    return glf_memcpy_h2d(ctx, d_w, hw.data(), sizeof(float) * hw.size());
}

// OrthonormaliseVecs / NormaliseVecs for more than 256 vectors: row-major in, panels inside, row-major out
static int orthonormalise_wide(glf_ctx *ctx, glf_mat *X, double *norms, bool normalise_only)
{
    const unsigned n = (unsigned)X->rows, m = (unsigned)X->cols, ld = (unsigned)X->ld;
    if (!wide_ld(ld) || m > ld) return set_error(ctx, GLF_ERR_INVALID, "more than 256 vectors need ld = a multiple of 256 (ld = %u)", ld);
    const unsigned npan = (unsigned)ceil_div(m, PANEL_COLS), n32 = (unsigned)round_up(n, VEC_PAD);
    DevBuf<float> panels;
    GLF_TRY(panels.alloc(ctx, (size_t)npan * n32 * PANEL_COLS));
    GLF_HIP(ctx, hipMemsetAsync(panels.p, 0, sizeof(float) * (size_t)npan * n32 * PANEL_COLS, ctx->stream));
    for (unsigned q = 0; q < npan; ++q) GLF_TRY(pack_panel(ctx, X->data, ld, n, q, panels.p + (size_t)q * n32 * PANEL_COLS));
    GLF_TRY(orthonormalise_panels(ctx, panels.p, n, m, norms, normalise_only));
    for (unsigned q = 0; q < npan; ++q) GLF_TRY(unpack_panel(ctx, panels.p + (size_t)q * n32 * PANEL_COLS, ld, n, q, X->data));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

} // namespace glf

using namespace glf;

extern "C" {

// ------------------------------------------------------------------------------------------
// Stage API
// ------------------------------------------------------------------------------------------
// Throughput mode: a batch of equally sized tiles (BASELINE config 5)
// ------------------------------------------------------------------------------------------
// Every tile goes through glf_image_processing unchanged; nctx contexts (one stream and one host thread each) work
// concurrently and take the tiles from a shared counter, so the launch- and latency-bound stages of one tile (the
// eigensolver at 1024 x 1024: dozens of small kernels and a host round trip per outer iteration) overlap the wide
// kernels of the others. Replicas only: no data-path exchange between tiles, contexts must not carry a comm.
int glf_image_processing_batch(glf_ctx *const *ctxs, int nctx, const glf_options *opt, const uint8_t *d_imgs, int width, int height,
                               int ntiles, uint8_t *d_outs, float *d_zfs, glf_stats *stats)
{
    if (!ctxs || nctx < 1 || !ctxs[0]) return GLF_ERR_INVALID;
    if (ntiles < 0 || width <= 0 || height <= 0 || (ntiles > 0 && (!d_imgs || !d_outs)))
        return set_error(ctxs[0], GLF_ERR_INVALID, "glf_image_processing_batch: %d tiles of %dx%d", ntiles, width, height);
    for (int c = 0; c < nctx; ++c) {
        if (!ctxs[c]) return set_error(ctxs[0], GLF_ERR_INVALID, "glf_image_processing_batch: context %d is NULL", c);
        if (ctxs[c]->has_comm) return set_error(ctxs[0], GLF_ERR_INVALID, "glf_image_processing_batch: context %d has a comm (tiles are replicas)", c);
        for (int d = 0; d < c; ++d)
            if (ctxs[d] == ctxs[c]) return set_error(ctxs[0], GLF_ERR_INVALID, "glf_image_processing_batch: context %d listed twice", c);
    }
    const size_t N = (size_t)width * height;
    std::atomic<int> next{0}, status{GLF_OK}, failed{-1};
    auto worker = [&](int c) {
        if (hipSetDevice(ctxs[c]->device) != hipSuccess) {
            int expected = GLF_OK;
            if (status.compare_exchange_strong(expected, GLF_ERR_NODEVICE)) failed.store(c);
            return;
        }
        for (;;) {
            const int t = next.fetch_add(1);
            if (t >= ntiles || status.load() != GLF_OK) break;
            const int rc = glf_image_processing(ctxs[c], opt, d_imgs + (size_t)t * N, width, height, d_outs + (size_t)t * N,
                                                d_zfs ? d_zfs + (size_t)t * N : nullptr, nullptr, stats ? stats + t : nullptr);
            if (rc != GLF_OK) {
                int expected = GLF_OK;
                if (status.compare_exchange_strong(expected, rc)) failed.store(c);
                break;
            }
        }
    };
    std::vector<std::thread> threads;
    const int nworkers = std::min(nctx, std::max(1, ntiles));
    for (int c = 1; c < nworkers; ++c) threads.emplace_back(worker, c);
    worker(0);
    for (auto &th : threads) th.join();
    const int rc = status.load(), fc = failed.load();
    if (rc != GLF_OK && fc > 0) std::snprintf(ctxs[0]->last_error, sizeof(ctxs[0]->last_error), "context %d: %s", fc, ctxs[fc]->last_error);
    return rc;
}

// ------------------------------------------------------------------------------------------

int glf_ComputeAffinityMatrices(glf_ctx *ctx, glf_mat *K_A, glf_mat *K_B, const uint8_t *d_img, int width, int height,
                                unsigned sample_size, const unsigned *sample_indices, int kernel, float h_loc,
                                float h_val)
{
    if (!ctx || !K_B || !d_img || width <= 0 || height <= 0) return GLF_ERR_INVALID;
    if (kernel < GLF_KERNEL_BILATERAL || kernel > GLF_KERNEL_BILATERAL_RGBF32) return set_error(ctx, GLF_ERR_INVALID, "kernel %d", kernel);
    if (kernel == GLF_KERNEL_NLM && (width < 3 || height < 3)) // (nlm.hip reflects an out-of-image patch index once: valid from 3 pixels on)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "non-local-means kernel: the image must be at least 3 x 3 pixels (%d x %d)", width, height);
    GLF_ENTER(ctx);
    GLF_TRY(f32_admit(ctx, pixgen_of(kernel), d_img, width, height));
    const unsigned p = sample_size;
    SampleTables tb;
    GLF_TRY(build_sample_tables(ctx, d_img, width, height, p, sample_indices, tb, kernel)); // (RGB: d_img is [height][width][3]; U16: uint16_t; F32: float; RGBF32: float [height][width][3])
    const KernelCoef coef = make_coef(kernel, h_loc, h_val);
    DevBuf<double> deg;
    GLF_TRY(deg.alloc(ctx, p));
    int row0, row1;
    shard_rows(ctx, height, &row0, &row1);
    GLF_TRY(degree_rows_auto(ctx, d_img, width, height, row0, row1, tb.samples.p, p, sample_indices, coef, deg.p, 0, nullptr, tb.idx.p));
    GLF_TRY(allreduce_f64(ctx, deg.p, p));
    if (K_A) {
        const int64_t lda = round_up(p, VEC_PAD);
        GLF_TRY(glf_mat_create_dense(ctx, K_A, p, p, lda)); // zero-filled incl. padding
        GLF_TRY(build_sample_matrix(ctx, tb.samples.p, p, coef, K_A->data, lda, false, 0.0, nullptr, 0, 0, d_img, width, height, tb.idx.p));
    }
    std::memset(K_B, 0, sizeof(*K_B));
    K_B->kind = GLF_MAT_KERNEL_B;
    K_B->rows = p;
    K_B->cols = (int64_t)width * height - p;
    K_B->img = d_img;
    K_B->width = width;
    K_B->height = height;
    K_B->p = p;
    K_B->scale = 1.0f;
    K_B->h_loc = h_loc;
    K_B->h_val = h_val;
    K_B->kernel = kernel;
    K_B->samples = reinterpret_cast<const float *>(tb.samples.take());
    K_B->mask = tb.mask.take();
    K_B->idx = tb.idx.take();
    K_B->degree = deg.take();
    K_B->owns_desc = 1;
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

// The degree stage by itself: the tables, coefficients and dispatch of glf_ComputeAffinityMatrices over one rank's rows, with the whole
// path's window and sums (run_planned's degree_rows_auto and weighted_sums_grid calls), no all-reduce, and a report of what ran.
int glf_Degree_ex(glf_ctx *ctx, const void *d_img_v, int width, int height, unsigned sample_size, const unsigned *sample_indices,
                  int kernel, float h_loc, float h_val, int skip_exact_zeros, unsigned row0u, unsigned row1u, const float *d_plane,
                  double *h_degree, double *h_ysum, glf_degree_info *info)
{
    const uint8_t *d_img = static_cast<const uint8_t *>(d_img_v);
    if (!ctx || !d_img || !h_degree || width <= 0 || height <= 0) return GLF_ERR_INVALID;
    if (info && info->struct_size != sizeof(glf_degree_info))
        return set_error(ctx, GLF_ERR_INVALID, "degree: glf_degree_info.struct_size %u, expected %zu", info->struct_size, sizeof(glf_degree_info));
    if (kernel < GLF_KERNEL_BILATERAL || kernel > GLF_KERNEL_BILATERAL_RGBF32)
        return set_error(ctx, GLF_ERR_INVALID, "degree: kernel %d is not one of GLF_KERNEL_*", kernel);
    if (kernel == GLF_KERNEL_NLM && (width < 3 || height < 3))
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "non-local-means kernel: the image must be at least 3 x 3 pixels (%d x %d)", width, height);
    const bool all_rows = row0u == 0 && row1u == 0;
    if (!all_rows && (row0u >= row1u || row1u > (unsigned)height))
        return set_error(ctx, GLF_ERR_INVALID, "degree: image rows [%u, %u) are not a range of the %d rows", row0u, row1u, height);
    if (d_plane && h_ysum) return set_error(ctx, GLF_ERR_INVALID, "degree: a weight plane has no value-weighted sums (d_plane with h_ysum)");
    if (d_plane && !grey_levels_factor(kernel))
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "degree: the weighted sums take an 8-bit grey kernel (kernel %d)", kernel);
    if (h_ysum && !grey_levels_factor(kernel))
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "degree: only the grid-factored form has the value-weighted sums (kernel %d)", kernel);
    GLF_ENTER(ctx);
    GLF_TRY(f32_admit(ctx, pixgen_of(kernel), d_img, width, height));
    const unsigned p = sample_size;
    const int row0 = all_rows ? 0 : (int)row0u, row1 = all_rows ? height : (int)row1u;
    SampleTables tb;
    GLF_TRY(build_sample_tables(ctx, d_img, width, height, p, sample_indices, tb, kernel));
    const KernelCoef coef = make_coef(kernel, h_loc, h_val);
    const int window = skip_exact_zeros ? 1 : 0;
    DevBuf<double> deg;
    GLF_TRY(deg.alloc(ctx, (size_t)2 * p));
    bool have_ysum = false;
    if (d_plane) {
        float smax = 0.f;
        GLF_TRY(plane_absmax(ctx, d_plane + (size_t)row0 * width, (int64_t)(row1 - row0) * width, &smax));
        const int rc = weighted_sums_grid(ctx, d_img, width, height, row0, row1, tb.samples.p, p, sample_indices, coef, window, d_plane,
                                          (double)smax, deg.p);
        if (rc != GLF_OK) return rc == GLF_ERR_UNSUPPORTED ? set_error(ctx, GLF_ERR_UNSUPPORTED, "degree: weighted sums: no grid-factored degree for this sample set") : rc;
    } else {
        GLF_TRY(degree_rows_auto(ctx, d_img, width, height, row0, row1, tb.samples.p, p, sample_indices, coef, deg.p, window, nullptr,
                                 tb.idx.p, h_ysum ? deg.p + p : nullptr, &have_ysum));
        if (h_ysum && !have_ysum)
            return set_error(ctx, GLF_ERR_UNSUPPORTED, "degree: the form that ran (path %d) has no value-weighted sums", ctx->deg_note.path);
    }
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<double> h((size_t)2 * p); // (staged: a failing copy leaves the caller's buffers as they were)
    GLF_TRY(glf_memcpy_d2h(ctx, h.data(), deg.p, sizeof(double) * (have_ysum ? 2 : 1) * p));
    std::memcpy(h_degree, h.data(), sizeof(double) * p);
    if (h_ysum) std::memcpy(h_ysum, h.data() + p, sizeof(double) * p);
    if (info) {
        info->path = ctx->deg_note.path;
        info->shape = ctx->deg_note.shape;
        info->skipping = ctx->deg_note.skipping;
        info->chunks = ctx->deg_note.chunks;
        info->mgroups = ctx->deg_note.mgroups;
        info->row0 = (uint32_t)row0;
        info->row1 = (uint32_t)row1;
        info->entries_evaluated = ctx->deg_note.entries;
    }
    return GLF_OK;
}

int glf_ComputeLaplacianMatrix(glf_ctx *ctx, glf_mat *L_A, glf_mat *L_B, const glf_mat *K_A, const glf_mat *K_B,
                               double *alpha_out)
{
    if (!ctx || !L_A || !K_B || K_B->kind != GLF_MAT_KERNEL_B || !K_B->degree) return GLF_ERR_INVALID;
    GLF_ENTER(ctx);
    const unsigned p = K_B->p;
    if (K_A && (K_A->kind != GLF_MAT_DENSE || K_A->rows != p || K_A->cols != p))
        return set_error(ctx, GLF_ERR_INVALID, "K_A must be dense p x p");
    // alpha = 1 / VecMean(D_A), hpc/laplacian.c:29 + hpc/utils.c:378-388
    double sum = 0.0;
    GLF_TRY(sum_host(ctx, K_B->degree, p, &sum));
    const double alpha = 1.0 / (sum / (double)p);
    const int64_t lda = round_up(p, VEC_PAD);
    GLF_TRY(glf_mat_create_dense(ctx, L_A, p, p, lda));
    const KernelCoef coef = make_coef(K_B->kernel, K_B->h_loc, K_B->h_val);
    if (K_A)
        GLF_TRY(laplacian_from_KA(ctx, K_A->data, K_A->ld, p, L_A->data, lda, alpha, K_B->degree));
    else
        GLF_TRY(build_sample_matrix(ctx, reinterpret_cast<const float4 *>(K_B->samples), p, coef, L_A->data, lda, true,
                                    alpha, K_B->degree, 0, 0, K_B->img, K_B->width, K_B->height, K_B->idx));
    if (L_B) { // L_B = -alpha K_B, hpc/laplacian.c:37-38: same generator, other scale (shares tables)
        *L_B = *K_B;
        L_B->scale = (float)(-alpha);
        L_B->owns_desc = 0;
    }
    if (alpha_out) *alpha_out = alpha;
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

int glf_InversePowerIteration(glf_ctx *ctx, const glf_mat *A, unsigned m, glf_mat *eigenvectors, glf_mat *eigenvalues,
                              int optiGramSchmidt, double epsilon, double inner_rtol, int max_outer, const double *X0,
                              glf_eig_stats *stats)
{
    if (!ctx || !A || A->kind != GLF_MAT_DENSE || A->rows != A->cols) return GLF_ERR_INVALID;
    GLF_ENTER(ctx);
    const unsigned p = (unsigned)A->rows;
    if (m == 0 || m >= p) return set_error(ctx, GLF_ERR_INVALID, "need 0 < m < p (m=%u p=%u)", m, p);
    const unsigned ld = ld_total_for(m);
    const unsigned p32 = (unsigned)round_up(p, VEC_PAD);
    if (m > PANEL_COLS) { // panels of 256 vectors (the reference default m = p - 1, hpc/image_processing.c:96-108)
        const unsigned npan = ld / PANEL_COLS;
        glf_mat wide;
        GLF_TRY(glf_mat_create_dense(ctx, &wide, p32, m, ld));
        wide.rows = p;
        DevBuf<float> panels;
        GLF_TRY(panels.alloc(ctx, (size_t)npan * p32 * PANEL_COLS));
        std::vector<double> lamw(m);
        int rcw = inverse_power_iteration_panels(ctx, A->data, A->ld, p, m, X0, 1, optiGramSchmidt, epsilon, inner_rtol,
                                                 max_outer > 0 ? max_outer : 100000, panels.p, lamw.data(), stats, nullptr, nullptr);
        if (rcw != GLF_OK && rcw != GLF_ERR_NOCONV) {
            glf_mat_destroy(ctx, &wide);
            return rcw;
        }
        for (unsigned q = 0; q < npan; ++q) GLF_TRY(unpack_panel(ctx, panels.p + (size_t)q * p32 * PANEL_COLS, ld, p32, q, wide.data));
        GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (eigenvalues) {
            GLF_TRY(glf_mat_create_diag(ctx, eigenvalues, m));
            std::vector<float> lf(m);
            for (unsigned j = 0; j < m; ++j) lf[j] = (float)lamw[j];
            GLF_TRY(glf_memcpy_h2d(ctx, eigenvalues->data, lf.data(), sizeof(float) * m));
        }
        if (eigenvectors) *eigenvectors = wide;
        else glf_mat_destroy(ctx, &wide);
        return rcw;
    }
    glf_mat vecs;
    GLF_TRY(glf_mat_create_dense(ctx, &vecs, p32, m, ld));
    vecs.rows = p;
    std::vector<double> lam(m);
    int rc = inverse_power_iteration(ctx, A->data, A->ld, p, m, ld, X0, optiGramSchmidt, epsilon, inner_rtol,
                                     max_outer > 0 ? max_outer : 100000, vecs.data, lam.data(), stats);
    if (rc != GLF_OK && rc != GLF_ERR_NOCONV) {
        glf_mat_destroy(ctx, &vecs);
        return rc;
    }
    if (eigenvalues) {
        int rc2 = glf_mat_create_diag(ctx, eigenvalues, m);
        if (rc2 != GLF_OK) return rc2;
        std::vector<float> lf(m);
        for (unsigned j = 0; j < m; ++j) lf[j] = (float)lam[j];
        GLF_TRY(glf_memcpy_h2d(ctx, eigenvalues->data, lf.data(), sizeof(float) * m));
    }
    if (eigenvectors) *eigenvectors = vecs;
    else glf_mat_destroy(ctx, &vecs);
    return rc;
}

int glf_OrthonormaliseVecs(glf_ctx *ctx, glf_mat *X, double *norms)
{
    if (!ctx || !X || X->kind != GLF_MAT_DENSE) return GLF_ERR_INVALID;
    GLF_ENTER(ctx);
    if (X->cols > PANEL_COLS) return orthonormalise_wide(ctx, X, norms, false);
    return orthonormalise(ctx, X->data, (unsigned)X->rows, (unsigned)X->cols, (unsigned)X->ld, norms);
}

int glf_NormaliseVecs(glf_ctx *ctx, glf_mat *X, double *norms)
{
    if (!ctx || !X || X->kind != GLF_MAT_DENSE) return GLF_ERR_INVALID;
    GLF_ENTER(ctx);
    if (X->cols > PANEL_COLS) return orthonormalise_wide(ctx, X, norms, true);
    return normalise(ctx, X->data, (unsigned)X->rows, (unsigned)X->cols, (unsigned)X->ld, norms);
}

int glf_InverseDiagMat(glf_ctx *ctx, const glf_mat *x, glf_mat *inv)
{
    if (!ctx || !x || !inv || x->kind != GLF_MAT_DIAG) return GLF_ERR_INVALID;
    GLF_ENTER(ctx);
    GLF_TRY(glf_mat_create_diag(ctx, inv, x->rows));
    const unsigned n = (unsigned)x->rows;
    hipLaunchKernelGGL(k_diag_inverse, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, x->data, n, inv->data);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

int glf_Nystroem_ex(glf_ctx *ctx, const glf_mat *B, const glf_mat *phi_A, const glf_mat *Pi_A_Inv, int skip_exact_zeros, unsigned row0,
                    unsigned row1, glf_mat *phi, glf_nystroem_info *info)
{
    if (!ctx || !B || !phi_A || !Pi_A_Inv || !phi) return GLF_ERR_INVALID;
    GLF_ENTER(ctx);
    if (B->kind != GLF_MAT_KERNEL_B || phi_A->kind != GLF_MAT_DENSE || Pi_A_Inv->kind != GLF_MAT_DIAG)
        return set_error(ctx, GLF_ERR_INVALID, "Nystroem: B must be a KERNEL_B descriptor, phi_A dense, Pi_A_Inv diagonal");
    const unsigned p = B->p, m = (unsigned)phi_A->cols, ld = (unsigned)phi_A->ld;
    if (phi_A->rows != p || Pi_A_Inv->rows != m || !(valid_ld(ld) || wide_ld(ld)) || m > ld)
        return set_error(ctx, GLF_ERR_INVALID, "Nystroem: shape mismatch (p=%u, phi_A %lld x %u ld %u)", p,
                         (long long)phi_A->rows, m, ld);
    const int64_t N = (int64_t)B->width * B->height;
    const bool all_rows = row0 == 0 && row1 == 0, given = phi->data != nullptr;
    if (!all_rows && (row0 >= row1 || row1 > (unsigned)B->height))
        return set_error(ctx, GLF_ERR_INVALID, "Nystroem: image rows [%u, %u) are not a range of the %d rows", row0, row1, B->height);
    if (given && (phi->kind != GLF_MAT_DENSE || phi->rows != N || phi->cols != m || phi->ld != ld || phi->row_order != GLF_ROWS_SAMPLE_FIRST))
        return set_error(ctx, GLF_ERR_INVALID, "Nystroem: the given phi (%lld x %lld, ld %lld) is not a dense sample-first %lld x %u matrix of ld %u",
                         (long long)phi->rows, (long long)phi->cols, (long long)phi->ld, (long long)N, m, ld);
    if (wide_ld(ld) && (!all_rows || given))
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "Nystroem: more than 256 eigenpairs take all image rows and a phi allocated by the call");
    const int64_t pix0 = all_rows ? 0 : (int64_t)row0 * B->width, pix1 = all_rows ? N : (int64_t)row1 * B->width;
    const int window = skip_exact_zeros ? 1 : 0;
    int path = 0;
    uint64_t evaluated = 0;
    auto report = [&]() {
        if (!info) return;
        info->path = path;
        // (the colour, 16-bit and float formats' entry-by-entry kernels contract in f32 whatever the context's mode: glf_stats.contraction)
        info->contraction = (pixgen_of(B->kernel) != PixGen::Grey && path != 4) ? GLF_CONTRACT_F32_MFMA : ctx->contraction;
        info->skipping = ctx->nys_note.skipping;
        info->lut = ctx->nys_note.lut;
        info->row0 = all_rows ? 0u : row0;
        info->row1 = all_rows ? (unsigned)B->height : row1;
        info->entries_evaluated = (double)evaluated;
    };
    NysRequest rq; // (sample-first rows; the operand and Phi differ between the two branches below)
    rq.d_img = B->img; rq.width = B->width; rq.height = B->height;
    rq.d_mask = B->mask; rq.d_idx = B->idx;
    rq.d_samples = reinterpret_cast<const float4 *>(B->samples); rq.p = p; rq.coef = make_coef(B->kernel, B->h_loc, B->h_val);
    rq.window = window;
    rq.path = &path;
    if (wide_ld(ld)) { // more than 256 eigenvectors: one 256-column panel of Phi at a time (columns are independent)
        const unsigned npan = (unsigned)ceil_div(m, PANEL_COLS), p64 = (unsigned)round_up(p, NYS_PAD);
        DevBuf<float> pa, psiw, phip;
        GLF_TRY(pa.alloc(ctx, (size_t)p64 * PANEL_COLS));
        GLF_TRY(psiw.alloc(ctx, (size_t)p64 * PANEL_COLS));
        GLF_TRY(phip.alloc(ctx, (size_t)N * PANEL_COLS));
        GLF_TRY(glf_mat_create_dense(ctx, phi, N, m, ld));
        phi->row_order = GLF_ROWS_SAMPLE_FIRST;
        rq.pix1 = N;
        rq.d_psi = psiw.p; rq.ld = PANEL_COLS;
        rq.d_phi = phip.p;
        for (unsigned q = 0; q < npan; ++q) {
            const unsigned mq = std::min(PANEL_COLS, m - q * PANEL_COLS);
            GLF_HIP(ctx, hipMemsetAsync(pa.p, 0, sizeof(float) * (size_t)p64 * PANEL_COLS, ctx->stream));
            GLF_HIP(ctx, hipMemsetAsync(psiw.p, 0, sizeof(float) * (size_t)p64 * PANEL_COLS, ctx->stream));
            GLF_TRY(pack_panel(ctx, phi_A->data, ld, p, q, pa.p));
            hipLaunchKernelGGL(k_make_psi, dim3((unsigned)ceil_div((int64_t)p * PANEL_COLS, 256)), dim3(256), 0, ctx->stream, pa.p,
                               Pi_A_Inv->data + (size_t)q * PANEL_COLS, p, PANEL_COLS, mq, B->scale, psiw.p);
            GLF_LAUNCH_CHECK(ctx);
            uint64_t ev = 0;
            rq.m = mq; rq.entries_evaluated = &ev;
            GLF_TRY(nystroem_contract(ctx, rq));
            evaluated += ev; // (every panel evaluates K_B again)
            GLF_TRY(scatter_sample_rows(ctx, pa.p, p, PANEL_COLS, B->idx, phip.p, 0, B->img, nullptr, mq));
            GLF_TRY(unpack_panel(ctx, phip.p, ld, N, q, phi->data));
        }
        GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        report();
        return GLF_OK;
    }
    DevBuf<float> psi;
    GLF_TRY(psi.alloc(ctx, (size_t)round_up(p, NYS_PAD) * ld));
    GLF_HIP(ctx, hipMemsetAsync(psi.p, 0, sizeof(float) * (size_t)round_up(p, NYS_PAD) * ld, ctx->stream));
    hipLaunchKernelGGL(k_make_psi, dim3((unsigned)ceil_div((int64_t)p * ld, 256)), dim3(256), 0, ctx->stream, phi_A->data,
                       Pi_A_Inv->data, p, ld, m, B->scale, psi.p);
    GLF_LAUNCH_CHECK(ctx);
    if (!given) {
        GLF_TRY(glf_mat_create_dense(ctx, phi, N, m, ld));
        phi->row_order = GLF_ROWS_SAMPLE_FIRST;
    }
    rq.pix0 = pix0; rq.pix1 = pix1;
    rq.d_psi = psi.p; rq.m = m; rq.ld = ld;
    rq.d_phi = phi->data;
    rq.entries_evaluated = &evaluated;
    GLF_TRY(nystroem_contract(ctx, rq));
    GLF_TRY(scatter_sample_rows(ctx, phi_A->data, p, ld, B->idx, phi->data, 0, B->img, nullptr, m));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    report();
    return GLF_OK;
}

int glf_Nystroem(glf_ctx *ctx, const glf_mat *B, const glf_mat *phi_A, const glf_mat *Pi_A_Inv, glf_mat *phi)
{
    if (!phi) return GLF_ERR_INVALID;
    glf_mat out; // (phi is an output here, allocated by the call whatever the struct held; a refusal leaves it as it was)
    std::memset(&out, 0, sizeof(out));
    const int rc = glf_Nystroem_ex(ctx, B, phi_A, Pi_A_Inv, 0, 0, 0, &out, nullptr);
    if (out.data) *phi = out;
    return rc;
}

int glf_Permutation(glf_ctx *ctx, const glf_mat *in, const unsigned *sample_indices, unsigned num, glf_mat *out)
{
    if (!ctx || !in || !out || in->kind != GLF_MAT_DENSE || !sample_indices) return GLF_ERR_INVALID;
    GLF_ENTER(ctx);
    DevBuf<uint32_t> idx;
    GLF_TRY(idx.alloc(ctx, num));
    GLF_TRY(glf_memcpy_h2d(ctx, idx.p, sample_indices, sizeof(uint32_t) * num));
    GLF_TRY(glf_mat_create_dense(ctx, out, in->rows, in->cols, in->ld));
    out->row_order = GLF_ROWS_RASTER;
    if (wide_ld((unsigned)in->ld)) { // 256-column panels
        DevBuf<float> a, b;
        GLF_TRY(a.alloc(ctx, (size_t)in->rows * PANEL_COLS));
        GLF_TRY(b.alloc(ctx, (size_t)in->rows * PANEL_COLS));
        for (unsigned q = 0; q < (unsigned)(in->ld / PANEL_COLS); ++q) {
            GLF_TRY(pack_panel(ctx, in->data, in->ld, in->rows, q, a.p));
            GLF_TRY(permute_rows(ctx, a.p, b.p, in->rows, PANEL_COLS, idx.p, num));
            GLF_TRY(unpack_panel(ctx, b.p, in->ld, in->rows, q, out->data));
        }
        GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return GLF_OK;
    }
    GLF_TRY(permute_rows(ctx, in->data, out->data, in->rows, (unsigned)in->ld, idx.p, num));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

// ---- the filter stage: what the whole path's unfused filter and glf_Filter_ex both run ----------------------------------------------
// What the stage needs to know of a run: run_planned fills it from its RunPlan, glf_Filter_ex from its request.
struct FilterSpec {
    glf_options opt;   // filter_mode, filter_pow, filter_beta (filter_rule.hpp)
    PixGen gen;
    int64_t N;
    unsigned m, ld;
    float gain, ysub;
    const double *lam; // HOST [m]
    bool reduce;       // sum c and G over the ranks (the whole path; glf_Filter_ex is one rank's share)
};

// hG = Phi^T Phi over the pixels [pix0, pix1) (all ranks' when F.reduce): the sharpening weights' Gram matrix, f64 [ld][ld] on the host
static int filter_gram(glf_ctx *ctx, const FilterSpec &F, const float *phi_rows, int64_t pix0, int64_t pix1, std::vector<double> &hG)
{
    DevBuf<double> G;
    GLF_TRY(G.alloc(ctx, (size_t)F.ld * F.ld));
    GLF_TRY(phi_gram(ctx, phi_rows, pix0, pix1, F.ld, G.p));
    if (F.reduce) GLF_TRY(allreduce_f64(ctx, G.p, (size_t)F.ld * F.ld));
    hG.resize((size_t)F.ld * F.ld);
    return glf_memcpy_d2h(ctx, hG.data(), G.p, sizeof(double) * F.ld * F.ld);
}

// the 8-bit grey guide from its complete c = Phi^T y (device [ld]): the weights, then k_apply_filter over [pix0, pix1)
static int filter_grey(glf_ctx *ctx, const FilterSpec &F, const std::vector<double> &hG, const double *d_c, float *d_w, const float *phi_rows,
                       int64_t pix0, int64_t pix1, const uint8_t *d_img, uint8_t *d_out, float *d_zf, float *d_corr, double *h_c0)
{
    GLF_TRY(weights_from_c(ctx, d_c, 1, F.ld, [&](const double *hc, float *hw) {
        filter_weights_row(F.opt, F.m, F.lam, hG.data(), F.ld, hc, hw);
    }, d_w, h_c0));
    return apply_filter(ctx, d_img, phi_rows, pix0, pix1, F.m, F.ld, d_w, F.gain, F.ysub, d_out, d_zf, d_corr);
}

// one 256-column panel of more than 256 eigenpairs: its weights from its complete c (device [256]; mq live columns, lamq their
// eigenvalues), then its share of the correction into d_acc. d_pan: the panel's rows of the pixels [pix0, pix1)
static int filter_panel(glf_ctx *ctx, const glf_options &opt, unsigned mq, const double *lamq, const double *d_c, float *d_w, const float *d_pan,
                        int64_t pix0, int64_t pix1, float *d_acc, bool first)
{
    GLF_TRY(weights_from_c(ctx, d_c, 1, PANEL_COLS, [&](const double *hc, float *hw) {
        filter_weights_row(opt, mq, lamq, nullptr, 0, hc, hw);
    }, d_w));
    return filter_accumulate(ctx, d_pan, pix0, pix1, PANEL_COLS, d_w, d_acc, first);
}

// The planes of the filter stage over [pix0, pix1): the signal planes of an 8-bit grey guide (sig; sig_w: their weights where they
// are known already), or a colour / 16-bit / float guide's own channels (sig: the channels as float planes) with its extra planes
// (planes, optional: the guide's kernels then read the channels from the image). phi_rows: Phi's rows addressed by absolute pixel
// index. h_c_in (optional, HOST [rows][m]): stands in for the projection pass and its collective; h_c_out (optional): the
// projection as this call formed it. Rows: the guide's channels first, then the planes.
static int filter_planes_tail(glf_ctx *ctx, const FilterSpec &F, const std::vector<double> &hG, const float *phi_rows, int64_t pix0, int64_t pix1,
                              const uint8_t *d_img, const SignalPlanes *sig, const SignalPlanes *planes, const float *sig_w, uint8_t *d_out,
                              float *d_zf, const double *h_c_in = nullptr, double *h_c_out = nullptr)
{
    const unsigned m = F.m, ld = F.ld;
    const int64_t N = F.N;
    auto rule = [&](const double *hc, float *hw) { filter_weights_row(F.opt, m, F.lam, hG.data(), ld, hc, hw); };
    // c [rows][ld] on the device from the host's [rows][m], and back
    auto c_put = [&](double *d_c, int rows) -> int {
        std::vector<double> h((size_t)rows * ld, 0.0);
        for (int r = 0; r < rows; ++r) std::memcpy(h.data() + (size_t)r * ld, h_c_in + (size_t)r * m, sizeof(double) * m);
        return glf_memcpy_h2d(ctx, d_c, h.data(), sizeof(double) * h.size());
    };
    auto c_get = [&](const double *d_c, int rows) -> int {
        std::vector<double> h((size_t)rows * ld);
        GLF_TRY(glf_memcpy_d2h(ctx, h.data(), d_c, sizeof(double) * h.size()));
        for (int r = 0; r < rows; ++r) std::memcpy(h_c_out + (size_t)r * m, h.data() + (size_t)r * ld, sizeof(double) * m);
        return GLF_OK;
    };
    const int ns = sig->nsig;
    if (planes) { // colour or 16-bit guide with planes: c for the channels and the planes in one pass over Phi, the outputs in one more
        const int np = planes->nsig;
        DevBuf<double> ca; // [ns + np][ld]: the guide's channels, then the planes
        DevBuf<float> wa;
        GLF_TRY(ca.alloc(ctx, (size_t)(ns + np) * ld));
        GLF_TRY(wa.alloc(ctx, (size_t)(ns + np) * ld));
        double *cg = ca.p, *cp = ca.p + (size_t)ns * ld;
        if (h_c_in) GLF_TRY(c_put(ca.p, ns + np));
        else {
            GLF_TRY(phi_t_pix_signals(ctx, F.gen, phi_rows, d_img, planes->d_sig, N, np, pix0, pix1, ld, cg, cp));
            if (F.reduce) {
                GLF_TRY(allreduce_f64(ctx, cg, (size_t)ns * ld)); // the guide's collective, with the shape it has in the plain call
                GLF_TRY(allreduce_f64(ctx, cp, (size_t)np * ld)); // the planes' in one of their own (a ring's summation order may follow the layout)
            }
        }
        if (h_c_out) GLF_TRY(c_get(ca.p, ns + np));
        GLF_TRY(weights_from_c(ctx, ca.p, ns + np, ld, rule, wa.p));
        return apply_filter_pix_signals(ctx, F.gen, phi_rows, pix0, pix1, ld, np, wa.p, F.gain, F.ysub, d_img, d_out, d_zf, planes->d_sig,
                                        planes->d_out, N);
    }
    if (sig_w) // (its weights stand, c_s's collective is not repeated)
        return apply_filter_signals(ctx, phi_rows, pix0, pix1, ld, ns, sig_w, F.gain, F.ysub, sig->d_sig, sig->d_out, N);
    DevBuf<double> cs;
    DevBuf<float> ws;
    GLF_TRY(cs.alloc(ctx, (size_t)ns * ld));
    GLF_TRY(ws.alloc(ctx, (size_t)ns * ld));
    if (h_c_in) GLF_TRY(c_put(cs.p, ns));
    else {
        GLF_TRY(phi_t_signals(ctx, phi_rows, sig->d_sig, N, ns, pix0, pix1, ld, cs.p));
        if (F.reduce) GLF_TRY(allreduce_f64(ctx, cs.p, (size_t)ns * ld)); // c_k = Phi^T s_k over all ranks' pixels (a collective of its own)
    }
    if (h_c_out) GLF_TRY(c_get(cs.p, ns));
    GLF_TRY(weights_from_c(ctx, cs.p, ns, ld, rule, ws.p));
    if (F.gen != PixGen::Grey) // the outputs, clamped and cast as the grey d_out (16-bit: at 16 bits); the filter stage ends here
        return apply_filter_pix(ctx, F.gen, phi_rows, pix0, pix1, ld, ws.p, F.gain, F.ysub, d_img, d_out, d_zf, N);
    return apply_filter_signals(ctx, phi_rows, pix0, pix1, ld, ns, ws.p, F.gain, F.ysub, sig->d_sig, sig->d_out, N);
}

int glf_Filter_ex(glf_ctx *ctx, const glf_filter_request *rq, glf_filter_info *info)
{
    if (!ctx || !rq) return GLF_ERR_INVALID;
    if (rq->struct_size != sizeof(glf_filter_request))
        return set_error(ctx, GLF_ERR_INVALID, "filter: glf_filter_request.struct_size %u, expected %zu", rq->struct_size, sizeof(glf_filter_request));
    if (info && info->struct_size != sizeof(glf_filter_info))
        return set_error(ctx, GLF_ERR_INVALID, "filter: glf_filter_info.struct_size %u, expected %zu", info->struct_size, sizeof(glf_filter_info));
    const glf_mat *phi = rq->phi;
    if (!rq->d_img || !phi || !rq->lam || !rq->d_out || rq->width <= 0 || rq->height <= 0)
        return set_error(ctx, GLF_ERR_INVALID, "filter: a guide, phi, lam and d_out are required");
    if (rq->pix < GLF_PIX_U8 || rq->pix > GLF_PIX_RGBF32) return set_error(ctx, GLF_ERR_INVALID, "filter: pix %d is not one of GLF_PIX_*", rq->pix);
    if (rq->filter_mode < GLF_FILTER_REFERENCE || rq->filter_mode > GLF_FILTER_SHARPEN)
        return set_error(ctx, GLF_ERR_INVALID, "filter: filter_mode %d", rq->filter_mode);
    const PixGen gen = rq->pix == GLF_PIX_U8 ? PixGen::Grey : pixgen_of_pix(rq->pix);
    const bool grey = gen == PixGen::Grey;
    const int64_t N = (int64_t)rq->width * rq->height;
    if (N >= (int64_t)1 << 31) return set_error(ctx, GLF_ERR_UNSUPPORTED, "image too large");
    if (phi->kind != GLF_MAT_DENSE || !phi->data || phi->rows != N || phi->cols < 1)
        return set_error(ctx, GLF_ERR_INVALID, "filter: phi must be a dense N x m matrix (N = %lld)", (long long)N);
    if (phi->row_order == GLF_ROWS_SAMPLE_FIRST)
        return set_error(ctx, GLF_ERR_INVALID, "phi is in sample-first order: call glf_Permutation first (hpc/image_processing.c:250)");
    const unsigned m = (unsigned)phi->cols, ld = (unsigned)phi->ld;
    const bool wide = wide_ld(ld);
    if (!(valid_ld(ld) || wide)) return set_error(ctx, GLF_ERR_INVALID, "filter: ld = %u is not 32, 64, 128, 256 or a multiple of 256", ld);
    if (m > ld) return set_error(ctx, GLF_ERR_INVALID, "filter: m = %u columns in ld = %u", m, ld);
    const bool all_rows = rq->row0 == 0 && rq->row1 == 0;
    if (!all_rows && (rq->row0 >= rq->row1 || rq->row1 > (unsigned)rq->height))
        return set_error(ctx, GLF_ERR_INVALID, "filter: image rows [%u, %u) are not a range of the %d rows", rq->row0, rq->row1, rq->height);
    const int nsig = rq->nsig;
    if (nsig < 0 || nsig > GLF_MAX_SIGNALS || (nsig > 0 && (!rq->d_sig || !rq->d_sig_out)))
        return set_error(ctx, GLF_ERR_INVALID, "filter: nsig = %d planes (1 .. %d, with d_sig and d_sig_out)", nsig, GLF_MAX_SIGNALS);
    if (rq->d_corr && (!grey || wide)) return set_error(ctx, GLF_ERR_INVALID, "filter: d_corr is the 8-bit grey guide's correction (narrow ld)");
    if (wide && rq->filter_mode == GLF_FILTER_SHARPEN)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "the sharpening filter takes at most %u eigenpairs (%u asked for)", PANEL_COLS, m);
    if (wide && (nsig > 0 || !grey)) return set_error(ctx, GLF_ERR_UNSUPPORTED, "signal planes with more than 256 eigenpairs (%u asked for)", m);
    const bool sharpen = rq->filter_mode == GLF_FILTER_SHARPEN;
    if (sharpen && !all_rows && !(rq->row0 == 0 && rq->row1 == (unsigned)rq->height))
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "filter: the sharpening weights need Phi^T Phi over all image rows (rows [%u, %u))", rq->row0, rq->row1);
    GLF_ENTER(ctx);
    const uint8_t *d_img = static_cast<const uint8_t *>(rq->d_img);
    GLF_TRY(f32_admit(ctx, gen, d_img, rq->width, rq->height));
    FilterSpec F;
    glf_options_default(&F.opt);
    F.opt.filter_mode = rq->filter_mode;
    F.opt.filter_pow = rq->filter_pow;
    F.opt.filter_beta = rq->filter_beta;
    F.opt.gain = rq->gain;
    F.gen = gen;
    F.N = N;
    F.m = m;
    F.ld = ld;
    F.gain = filter_gain(F.opt);
    F.ysub = 1.0f - filter_ident(F.opt);
    F.lam = rq->lam;
    F.reduce = false;
    const int64_t pix0 = all_rows ? 0 : (int64_t)rq->row0 * rq->width, pix1 = all_rows ? N : (int64_t)rq->row1 * rq->width;
    ctx->flt_note = {};
    uint8_t *d_out = static_cast<uint8_t *>(rq->d_out);
    const int nch = pix_desc(gen).channels;
    std::vector<double> hc_out((size_t)(nch + nsig) * m), hG; // (staged: the host outputs are written once everything has run)
    if (wide) { // 256-column panels: right = phi^T y panel by panel, then the correction accumulated over the panels
        const unsigned npan = (unsigned)ceil_div(m, PANEL_COLS);
        const int64_t npix = pix1 - pix0;
        DevBuf<float> pan, wq, acc;
        DevBuf<double> cq;
        GLF_TRY(pan.alloc(ctx, (size_t)npix * PANEL_COLS));
        GLF_TRY(wq.alloc(ctx, PANEL_COLS));
        GLF_TRY(acc.alloc(ctx, (size_t)npix));
        GLF_TRY(cq.alloc(ctx, PANEL_COLS));
        std::vector<double> hq(PANEL_COLS);
        for (unsigned q = 0; q < npan; ++q) {
            const unsigned mq = std::min(PANEL_COLS, m - q * PANEL_COLS);
            GLF_TRY(pack_panel(ctx, phi->data + (size_t)pix0 * ld, ld, npix, q, pan.p));
            if (rq->h_c_in) {
                std::fill(hq.begin(), hq.end(), 0.0);
                std::memcpy(hq.data(), rq->h_c_in + (size_t)q * PANEL_COLS, sizeof(double) * mq);
                GLF_TRY(glf_memcpy_h2d(ctx, cq.p, hq.data(), sizeof(double) * PANEL_COLS));
            } else {
                GLF_TRY(phi_t_y(ctx, pan.p - (size_t)pix0 * PANEL_COLS, d_img, pix0, pix1, mq, PANEL_COLS, cq.p));
            }
            if (rq->h_c_out) {
                GLF_TRY(glf_memcpy_d2h(ctx, hq.data(), cq.p, sizeof(double) * PANEL_COLS));
                std::memcpy(hc_out.data() + (size_t)q * PANEL_COLS, hq.data(), sizeof(double) * mq);
            }
            GLF_TRY(filter_panel(ctx, F.opt, mq, rq->lam + (size_t)q * PANEL_COLS, cq.p, wq.p, pan.p, pix0, pix1, acc.p, q == 0));
        }
        GLF_TRY(filter_finish(ctx, d_img, acc.p, pix0, pix1, F.gain, F.ysub, d_out, rq->d_zf));
        ctx->flt_note.panels = npan;
    } else {
        const float *phi_rows = phi->data;
        if (sharpen) GLF_TRY(filter_gram(ctx, F, phi_rows, pix0, pix1, hG));
        SignalPlanes sig{nsig, rq->d_sig, rq->d_sig_out};
        if (grey) {
            DevBuf<double> c;
            DevBuf<float> w;
            GLF_TRY(c.alloc(ctx, ld));
            GLF_TRY(w.alloc(ctx, ld));
            if (rq->h_c_in) {
                std::vector<double> h(ld, 0.0);
                std::memcpy(h.data(), rq->h_c_in, sizeof(double) * m);
                GLF_TRY(glf_memcpy_h2d(ctx, c.p, h.data(), sizeof(double) * ld));
            } else {
                GLF_TRY(phi_t_y(ctx, phi_rows, d_img, pix0, pix1, m, ld, c.p)); // right = phi^T y, hpc/display.c:66
            }
            std::vector<double> h0(ld);
            GLF_TRY(filter_grey(ctx, F, hG, c.p, w.p, phi_rows, pix0, pix1, d_img, d_out, rq->d_zf, rq->d_corr, h0.data()));
            std::memcpy(hc_out.data(), h0.data(), sizeof(double) * m);
            if (nsig > 0)
                GLF_TRY(filter_planes_tail(ctx, F, hG, phi_rows, pix0, pix1, d_img, &sig, nullptr, nullptr, d_out, rq->d_zf,
                                           rq->h_c_in ? rq->h_c_in + m : nullptr, hc_out.data() + m));
        } else if (nsig > 0) {
            SignalPlanes guide{nch, nullptr, nullptr};
            GLF_TRY(filter_planes_tail(ctx, F, hG, phi_rows, pix0, pix1, d_img, &guide, &sig, nullptr, d_out, rq->d_zf, rq->h_c_in, hc_out.data()));
        } else { // the channels as float planes, as the whole path forms them
            DevBuf<float> gp;
            GLF_TRY(gp.alloc(ctx, (size_t)nch * N));
            GLF_TRY(pix_planes(ctx, gen, d_img, N, gp.p));
            SignalPlanes guide{nch, gp.p, nullptr};
            GLF_TRY(filter_planes_tail(ctx, F, hG, phi_rows, pix0, pix1, d_img, &guide, nullptr, nullptr, d_out, rq->d_zf, rq->h_c_in, hc_out.data()));
        }
    }
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rq->h_c_out) std::memcpy(rq->h_c_out, hc_out.data(), sizeof(double) * hc_out.size());
    if (rq->h_gram_out && sharpen)
        for (unsigned i = 0; i < m; ++i) std::memcpy(rq->h_gram_out + (size_t)i * m, hG.data() + (size_t)i * ld, sizeof(double) * m);
    if (info) {
        info->kernels = ctx->flt_note.kernels;
        info->ld = ctx->flt_note.ld;
        info->panels = ctx->flt_note.panels;
        info->proj_blocks = ctx->flt_note.proj_blocks;
        info->apply_blocks = ctx->flt_note.apply_blocks;
        info->grid_strided = ctx->flt_note.strided;
        info->reserved_ = 0;
        info->pix0 = (uint64_t)pix0;
        info->pix1 = (uint64_t)pix1;
    }
    return GLF_OK;
}

// glf_Filter_ex with its defaults: the reference filter z = y + gain Phi Pi Phi^T y on all rows (Pi: the DIAG matrix of f(eigenvalues))
int glf_ComputeResultFromLaplacian(glf_ctx *ctx, const uint8_t *d_img, const glf_mat *phi, const glf_mat *Pi, unsigned width,
                                   unsigned height, float gain, uint8_t *d_out, float *d_zf)
{
    if (!ctx || !d_img || !phi || !Pi || !d_out) return GLF_ERR_INVALID;
    GLF_ENTER(ctx);
    const int64_t N = (int64_t)width * height;
    const unsigned m = (unsigned)phi->cols, ld = (unsigned)phi->ld;
    if (phi->kind != GLF_MAT_DENSE || phi->rows != N || Pi->kind != GLF_MAT_DIAG || Pi->rows != m || !(valid_ld(ld) || wide_ld(ld)))
        return set_error(ctx, GLF_ERR_INVALID, "ComputeResultFromLaplacian: shape mismatch");
    std::vector<float> hp(m);
    GLF_TRY(glf_memcpy_d2h(ctx, hp.data(), Pi->data, sizeof(float) * m));
    const std::vector<double> lam(hp.begin(), hp.end()); // w = fl32(Pi c), left = phi Pi, hpc/display.c:64
    glf_filter_request rq{};
    rq.struct_size = sizeof(rq);
    rq.pix = GLF_PIX_U8;
    rq.d_img = d_img;
    rq.width = (int)width;
    rq.height = (int)height;
    rq.phi = phi;
    rq.lam = lam.data();
    rq.filter_mode = GLF_FILTER_REFERENCE;
    rq.filter_pow = 1;
    rq.gain = gain;
    rq.d_out = d_out;
    rq.d_zf = d_zf;
    return glf_Filter_ex(ctx, &rq, nullptr);
}

int glf_EntireComputation(glf_ctx *ctx, const uint8_t *d_img, int width, int height, int kernel, float h_loc, float h_val,
                          uint8_t *d_out, float *d_zf, double *alpha_out)
{
    if (!ctx || !d_img || !d_out || width <= 0 || height <= 0) return GLF_ERR_INVALID;
    if (kernel < GLF_KERNEL_BILATERAL || kernel > GLF_KERNEL_SPATIAL) return set_error(ctx, GLF_ERR_INVALID, "kernel %d", kernel);
    GLF_ENTER(ctx);
    return entire_computation(ctx, d_img, width, height, make_coef(kernel, h_loc, h_val), d_out, d_zf, alpha_out);
}

// ------------------------------------------------------------------------------------------
// Whole approximate path
// ------------------------------------------------------------------------------------------

// (an image of any format travels as a byte pointer)
static inline const uint8_t *bytes_of(const void *q) { return static_cast<const uint8_t *>(q); }
static inline uint8_t *bytes_of(void *q) { return static_cast<uint8_t *>(q); }

// Every typed entry point forwards to glf::image_processing_run with its format: the checks are there. (The float formats' output is
// z itself, interleaved as the image: no d_zf.)

int glf_image_processing(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_img, int width, int height, uint8_t *d_out, float *d_zf,
                         double *eigvals_out, glf_stats *stats)
{
    return image_processing_run(ctx, opt, PixGen::Grey, d_img, width, height, d_out, d_zf, eigvals_out, stats, nullptr, nullptr);
}

int glf_image_processing_capture(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_img, int width, int height, uint8_t *d_out,
                                 float *d_zf, double *eigvals_out, glf_stats *stats, glf_capture *cap)
{
    return image_processing_run(ctx, opt, PixGen::Grey, d_img, width, height, d_out, d_zf, eigvals_out, stats, cap, nullptr);
}

int glf_image_processing_signals(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_img, int width, int height, int nsig,
                                 const float *d_sig, float *d_sig_out, uint8_t *d_out, float *d_zf, double *eigvals_out,
                                 glf_stats *stats)
{
    const SignalPlanes sig{nsig, d_sig, d_sig_out};
    return image_processing_run(ctx, opt, PixGen::Grey, d_img, width, height, d_out, d_zf, eigvals_out, stats, nullptr, &sig);
}

int glf_image_processing_rgb(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_rgb, int width, int height, uint8_t *d_out_rgb,
                             float *d_zf, double *eigvals_out, glf_stats *stats)
{
    return image_processing_run(ctx, opt, PixGen::Rgb, d_rgb, width, height, d_out_rgb, d_zf, eigvals_out, stats, nullptr, nullptr);
}

int glf_image_processing_rgb_capture(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_rgb, int width, int height, uint8_t *d_out_rgb,
                                     float *d_zf, double *eigvals_out, glf_stats *stats, glf_capture *cap)
{
    return image_processing_run(ctx, opt, PixGen::Rgb, d_rgb, width, height, d_out_rgb, d_zf, eigvals_out, stats, cap, nullptr);
}

int glf_image_processing_u16(glf_ctx *ctx, const glf_options *opt, const uint16_t *d_img, int width, int height, uint16_t *d_out,
                             float *d_zf, double *eigvals_out, glf_stats *stats)
{
    return image_processing_run(ctx, opt, PixGen::U16, bytes_of(d_img), width, height, bytes_of(d_out), d_zf, eigvals_out, stats, nullptr, nullptr);
}

int glf_image_processing_u16_capture(glf_ctx *ctx, const glf_options *opt, const uint16_t *d_img, int width, int height, uint16_t *d_out,
                                     float *d_zf, double *eigvals_out, glf_stats *stats, glf_capture *cap)
{
    return image_processing_run(ctx, opt, PixGen::U16, bytes_of(d_img), width, height, bytes_of(d_out), d_zf, eigvals_out, stats, cap, nullptr);
}

int glf_image_processing_rgb_signals(glf_ctx *ctx, const glf_options *opt, const uint8_t *d_rgb, int width, int height, int nsig,
                                     const float *d_sig, float *d_sig_out, uint8_t *d_out_rgb, float *d_zf, double *eigvals_out,
                                     glf_stats *stats)
{
    const SignalPlanes sig{nsig, d_sig, d_sig_out};
    return image_processing_run(ctx, opt, PixGen::Rgb, d_rgb, width, height, d_out_rgb, d_zf, eigvals_out, stats, nullptr, &sig);
}

int glf_image_processing_u16_signals(glf_ctx *ctx, const glf_options *opt, const uint16_t *d_img, int width, int height, int nsig,
                                     const float *d_sig, float *d_sig_out, uint16_t *d_out, float *d_zf, double *eigvals_out,
                                     glf_stats *stats)
{
    const SignalPlanes sig{nsig, d_sig, d_sig_out};
    return image_processing_run(ctx, opt, PixGen::U16, bytes_of(d_img), width, height, bytes_of(d_out), d_zf, eigvals_out, stats, nullptr, &sig);
}

int glf_image_processing_f32(glf_ctx *ctx, const glf_options *opt, const float *d_img, int width, int height, float *d_out,
                             double *eigvals_out, glf_stats *stats)
{
    return image_processing_run(ctx, opt, PixGen::F32, bytes_of(d_img), width, height, bytes_of(d_out), nullptr, eigvals_out, stats, nullptr, nullptr);
}

int glf_image_processing_f32_capture(glf_ctx *ctx, const glf_options *opt, const float *d_img, int width, int height, float *d_out,
                                     double *eigvals_out, glf_stats *stats, glf_capture *cap)
{
    return image_processing_run(ctx, opt, PixGen::F32, bytes_of(d_img), width, height, bytes_of(d_out), nullptr, eigvals_out, stats, cap, nullptr);
}

int glf_image_processing_f32_signals(glf_ctx *ctx, const glf_options *opt, const float *d_img, int width, int height, int nsig,
                                     const float *d_sig, float *d_sig_out, float *d_out, double *eigvals_out, glf_stats *stats)
{
    const SignalPlanes sig{nsig, d_sig, d_sig_out};
    return image_processing_run(ctx, opt, PixGen::F32, bytes_of(d_img), width, height, bytes_of(d_out), nullptr, eigvals_out, stats, nullptr, &sig);
}

int glf_image_processing_rgbf32(glf_ctx *ctx, const glf_options *opt, const float *d_rgb, int width, int height, float *d_out_rgb,
                                double *eigvals_out, glf_stats *stats)
{
    return image_processing_run(ctx, opt, PixGen::RgbF32, bytes_of(d_rgb), width, height, bytes_of(d_out_rgb), nullptr, eigvals_out, stats, nullptr, nullptr);
}

int glf_image_processing_rgbf32_capture(glf_ctx *ctx, const glf_options *opt, const float *d_rgb, int width, int height,
                                        float *d_out_rgb, double *eigvals_out, glf_stats *stats, glf_capture *cap)
{
    return image_processing_run(ctx, opt, PixGen::RgbF32, bytes_of(d_rgb), width, height, bytes_of(d_out_rgb), nullptr, eigvals_out, stats, cap, nullptr);
}

int glf_image_processing_rgbf32_signals(glf_ctx *ctx, const glf_options *opt, const float *d_rgb, int width, int height, int nsig,
                                        const float *d_sig, float *d_sig_out, float *d_out_rgb, double *eigvals_out, glf_stats *stats)
{
    const SignalPlanes sig{nsig, d_sig, d_sig_out};
    return image_processing_run(ctx, opt, PixGen::RgbF32, bytes_of(d_rgb), width, height, bytes_of(d_out_rgb), nullptr, eigvals_out, stats, nullptr, &sig);
}

// ------------------------------------------------------------------------------------------
// The form L_A takes in the eigen-solve: decided here for the whole-path driver and for glf_operator_create alike
// ------------------------------------------------------------------------------------------
// For a tensor-grid sample set L_A is applied in grid-factored form and never stored (GLF_MV_PATH = grid | rank | band | dense |
// auto; auto: from 16 384 samples on -- below, streaming a small stored L_A is cheaper than the factored sweep's fixed cost).
// *out stays null where L_A is to be stored: not asked for, the NLM kernel, a colour / 16-bit / float guide wider than its band
// form's one block of 64 columns, or a form that does not apply (grid_op_create's GLF_ERR_UNSUPPORTED)
static int operator_factored(glf_ctx *ctx, const float4 *d_samples, const unsigned *h_idx, unsigned p, int width, int height, KernelCoef coef,
                             int kernel, unsigned ld, GridOp **out)
{
    *out = nullptr;
    const bool want = (ctx->tune.mv_path == 1 || ctx->tune.mv_path == 3 || ctx->tune.mv_path == 4) ? true : ctx->tune.mv_path == 2 ? false : p >= 16384;
    if (want && kernel != GLF_KERNEL_NLM && (pixgen_of(kernel) == PixGen::Grey || ld <= 64)) {
        const int rc = grid_op_create(ctx, d_samples, h_idx, p, width, height, coef, out);
        if (rc != GLF_OK && rc != GLF_ERR_UNSUPPORTED) return rc;
    }
    return GLF_OK;
}

struct OperatorStore {
    DevBuf<int4> kbox; // bounding boxes of the 64-sample chunks (exact-zero tile skipping of the stored split-f16 form)
    DevBuf<float> LA;  // the stored L_A: [p][lda], whole or (sharded) the column block [:, row0:row1)
    int64_t lda = 0;
};
// Completes the solve's MatShard (sharded: row0, row1 and rows_per_rank are the caller's) and builds what a stored L_A needs.
// Factored: alpha, the degree and the skipping window of the operator. Stored: the boxes and the radius of exact-zero tile
// skipping (|2^10 L_A[i][j]| = 2^10 alpha K < 2^-25 once t > 35 + log2(alpha)), lda and the matrix
static int operator_store(glf_ctx *ctx, GridOp *gop, const float4 *d_samples, const uint32_t *d_idx, unsigned p, KernelCoef coef, int kernel,
                          double alpha, const double *d_degree, int skip_exact_zeros, bool sharded, const uint8_t *d_img, int width, int height,
                          MatShard &shard, OperatorStore &st)
{
    if (gop) {
        shard.grid = gop;
        shard.grid_alpha = alpha;
        shard.grid_degree = d_degree;
        shard.grid_window = skip_exact_zeros;
    }
    if (!gop && skip_exact_zeros && coef.s_loc > 0.f && kernel != GLF_KERNEL_NLM && ctx->contraction == GLF_CONTRACT_F16_SPLIT) {
        const double t_zero = 35.5 + std::log2(alpha);
        GLF_TRY(st.kbox.alloc(ctx, (size_t)ceil_div(p, 64)));
        GLF_TRY(chunk_boxes(ctx, d_samples, p, st.kbox.p));
        shard.kbox = st.kbox.p;
        shard.radius = t_zero > 0.0 ? (int)std::floor(std::sqrt(t_zero / (double)coef.s_loc)) + 1 : 0;
    }
    const unsigned la_cols = sharded ? shard.row1 - shard.row0 : p;
    st.lda = sharded ? round_up(la_cols ? la_cols : 1, VEC_PAD) : round_up(p, VEC_PAD);
    if (!gop) {
        GLF_TRY(st.LA.alloc(ctx, (size_t)p * st.lda));
        if (la_cols) // writes every element of the p x lda block, padding columns included
            GLF_TRY(build_sample_matrix(ctx, d_samples, p, coef, st.LA.p, st.lda, true, alpha, d_degree, sharded ? shard.row0 : 0u, la_cols, d_img,
                                        width, height, d_idx));
    }
    return GLF_OK;
}
// what the solve hands to block_matvec: the shard where it says anything (rows, skipping boxes or a factored operator)
static inline const MatShard *shard_arg(const MatShard &shard) { return (shard.rows_per_rank || shard.kbox || shard.grid) ? &shard : nullptr; }

// ------------------------------------------------------------------------------------------
// One sweep of that operator on its own (glf_operator_*)
// ------------------------------------------------------------------------------------------
struct glf_operator {
    glf_ctx *ctx = nullptr;
    unsigned p = 0;
    PixGen gen = PixGen::Grey;
    GridOp *gop = nullptr;
    OperatorStore store;
    MatShard shard;
    unsigned row0 = 0, row1 = 0;
    int contraction = 0, mv_path = 0; // what the form was chosen (and a factored operator's tables built) under
    bool sweep_samples = false;
    double alpha = 0.0;               // of L_A = alpha (D - K_A), and the descriptor's degree: the Jacobi preconditioner of glf_operator_solve
    const double *degree = nullptr;
    ~glf_operator() { grid_op_destroy(gop); }
};

int glf_operator_create(glf_ctx *ctx, const glf_mat *L_B, int skip_exact_zeros, unsigned row0, unsigned row1, unsigned ld_hint, glf_operator **out)
{
    if (!ctx || !out) return GLF_ERR_INVALID;
    *out = nullptr;
    if (!L_B || L_B->kind != GLF_MAT_KERNEL_B || !L_B->degree || !L_B->samples || !L_B->idx || !L_B->img)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_create: L_B must be a KERNEL_B descriptor with its cached degree (glf_ComputeLaplacianMatrix's L_B)");
    GLF_ENTER(ctx);
    const unsigned p = L_B->p;
    const int kernel = L_B->kernel, width = L_B->width, height = L_B->height;
    if (p < 2 || kernel < GLF_KERNEL_BILATERAL || kernel > GLF_KERNEL_BILATERAL_RGBF32)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_create: p = %u, kernel %d", p, kernel);
    const bool ranged = !(row0 == 0 && row1 == p);
    if (ranged && !(row0 < row1 && row1 <= p)) return set_error(ctx, GLF_ERR_INVALID, "glf_operator_create: rows [%u, %u) of p = %u", row0, row1, p);
    const bool forced = ctx->tune.mv_path == 1 || ctx->tune.mv_path == 3 || ctx->tune.mv_path == 4;
    if (forced && kernel == GLF_KERNEL_NLM)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "glf_operator_create: the non-local-means kernel has no factored form (MV_PATH forces one)");
    if (ld_hint % 32 || ld_hint < 32 || ld_hint > 256)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_create: ld_hint %u (a multiple of 32 up to 256)", ld_hint);
    const KernelCoef coef = make_coef(kernel, L_B->h_loc, L_B->h_val);
    const float4 *samples = reinterpret_cast<const float4 *>(L_B->samples);
    std::vector<unsigned> h_idx(p);
    GLF_HIP(ctx, hipMemcpyAsync(h_idx.data(), L_B->idx, sizeof(unsigned) * p, hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // alpha = 1 / VecMean(D_A), as glf_ComputeLaplacianMatrix and the whole path compute it (L_B->scale holds it rounded to f32)
    double dsum = 0.0;
    GLF_TRY(sum_host(ctx, L_B->degree, p, &dsum));
    const double alpha = 1.0 / (dsum / (double)p);
    std::unique_ptr<glf_operator> op(new glf_operator);
    op->ctx = ctx;
    op->p = p;
    op->gen = pixgen_of(kernel);
    op->row0 = ranged ? row0 : 0u;
    op->row1 = ranged ? row1 : p;
    op->contraction = ctx->contraction;
    op->mv_path = ctx->tune.mv_path;
    op->sweep_samples = ctx->tune.sweep_samples;
    op->alpha = alpha;
    op->degree = L_B->degree;
    GLF_TRY(operator_factored(ctx, samples, h_idx.data(), p, width, height, coef, kernel, ld_hint, &op->gop));
    if (forced && !op->gop)
        return set_error(ctx, GLF_ERR_UNSUPPORTED,
                         "glf_operator_create: the forced MV_PATH does not apply (it needs a tensor grid of samples, the split-f16 contraction and, for a "
                         "colour, 16-bit or float guide, PIX_BAND with MV_PATH=band and ld_hint <= 64)");
    if (ranged) {
        if (op->gop) {
            const unsigned nc = (unsigned)grid_op_row_len(op->gop);
            if (row0 % nc || (row1 % nc && row1 != p))
                return set_error(ctx, GLF_ERR_INVALID, "glf_operator_create: rows [%u, %u) are not whole grid rows (%u samples each)", row0, row1, nc);
        } else {
            if (ctx->contraction != GLF_CONTRACT_F16_SPLIT)
                return set_error(ctx, GLF_ERR_UNSUPPORTED, "glf_operator_create: a row range of the stored L_A needs the split-f16 contraction");
            if (row0 % VEC_PAD) return set_error(ctx, GLF_ERR_INVALID, "glf_operator_create: row0 = %u of a stored L_A must be a multiple of %d", row0, VEC_PAD);
        }
        op->shard.row0 = row0;
        op->shard.row1 = row1;
        op->shard.rows_per_rank = (unsigned)round_up(row1 - row0, VEC_PAD); // (the all-gather block of a rank that owns these rows)
    }
    GLF_TRY(operator_store(ctx, op->gop, samples, L_B->idx, p, coef, kernel, alpha, L_B->degree, skip_exact_zeros, ranged, L_B->img, width, height,
                           op->shard, op->store));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = op.release();
    return GLF_OK;
}

int glf_operator_apply(glf_operator *op, const glf_mat *X, glf_mat *Y, glf_operator_info *info)
{
    if (!op || !op->ctx) return GLF_ERR_INVALID;
    glf_ctx *ctx = op->ctx;
    if (!X || !Y || X->kind != GLF_MAT_DENSE || Y->kind != GLF_MAT_DENSE || !X->data || !Y->data || X->data == Y->data)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_apply: X and Y must be two dense matrices");
    GLF_ENTER(ctx);
    const unsigned p = op->p;
    if (ctx->contraction != op->contraction || ctx->tune.mv_path != op->mv_path || ctx->tune.sweep_samples != op->sweep_samples)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_apply: the contraction mode, MV_PATH or SWEEP_COLPASS changed since glf_operator_create");
    if (X->rows < (int64_t)p || Y->rows < (int64_t)p)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_apply: X has %lld rows and Y %lld, fewer than p = %u", (long long)X->rows, (long long)Y->rows, p);
    if (X->ld != Y->ld || X->ld <= 0 || X->ld > 256)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_apply: X has ld %lld, Y ld %lld (equal, at most 256)", (long long)X->ld, (long long)Y->ld);
    const unsigned ld = (unsigned)X->ld;
    if (!op->gop && !valid_ld(ld)) return set_error(ctx, GLF_ERR_INVALID, "glf_operator_apply: the stored L_A takes ld 32, 64, 128 or 256 (ld = %u)", ld);
    if (op->gop && op->gen != PixGen::Grey && ld != 32 && ld != 64)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_apply: the %s band form takes ld 32 or 64 (ld = %u)", pix_desc(op->gen).name, ld);
    if (op->gop && ld != 32 && ld % 64) // (grid_op_apply walks the block 64 columns at a time from ld 64 on)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_apply: a factored form takes ld 32, 64, 128, 192 or 256 (ld = %u)", ld);
    GLF_TRY(block_matvec(ctx, op->store.LA.p, op->store.lda, p, X->data, Y->data, ld, shard_arg(op->shard)));
    GLF_TRY(mv_collect(ctx));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (info) {
        info->path = op->gop ? grid_op_path(op->gop) : 0;
        const bool f16s = !op->gop && ctx->contraction == GLF_CONTRACT_F16_SPLIT;
        info->ksplit = f16s ? mv_ksplit(ctx, p, op->row0, op->row1) : 0;
        info->skipping = op->gop ? (op->shard.grid_window && grid_op_can_skip(op->gop)) : (f16s && op->shard.kbox && op->shard.radius >= 0 && mv_can_skip(p));
        info->row0 = (int32_t)op->row0;
        info->row1 = (int32_t)op->row1;
    }
    return GLF_OK;
}

int glf_operator_solve(glf_operator *op, const glf_mat *B, glf_mat *X, glf_mat *R, unsigned m, double rtol, int max_it, glf_solve_info *info)
{
    if (!op || !op->ctx) return GLF_ERR_INVALID;
    glf_ctx *ctx = op->ctx;
    auto dense = [](const glf_mat *M) { return M && M->kind == GLF_MAT_DENSE && M->data; };
    if (!dense(B) || !dense(X) || (R && !dense(R)) || B->data == X->data || (R && (R->data == B->data || R->data == X->data)))
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_solve: B, X and R (or NULL) must be distinct dense matrices");
    GLF_ENTER(ctx);
    const unsigned p = op->p;
    if (ctx->contraction != op->contraction || ctx->tune.mv_path != op->mv_path || ctx->tune.sweep_samples != op->sweep_samples)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_solve: the contraction mode, MV_PATH or SWEEP_COLPASS changed since glf_operator_create");
    if (op->shard.rows_per_rank)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "glf_operator_solve: the operator was created for the rows [%u, %u) (the sharded solve needs a communicator)",
                         op->row0, op->row1);
    if (B->rows < (int64_t)p || X->rows < (int64_t)p || (R && R->rows < (int64_t)p))
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_solve: B has %lld rows, X %lld, R %lld, fewer than p = %u", (long long)B->rows,
                         (long long)X->rows, (long long)(R ? R->rows : p), p);
    if (B->ld != X->ld || (R && R->ld != B->ld) || B->ld <= 0 || B->ld > 256)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_solve: B has ld %lld, X ld %lld, R ld %lld (equal, at most 256)", (long long)B->ld,
                         (long long)X->ld, (long long)(R ? R->ld : B->ld));
    const unsigned ld = (unsigned)B->ld;
    if (!valid_ld(ld)) return set_error(ctx, GLF_ERR_INVALID, "glf_operator_solve: the block PCG takes ld 32, 64, 128 or 256 (ld = %u)", ld);
    if (op->gop && op->gen != PixGen::Grey && ld != 32 && ld != 64)
        return set_error(ctx, GLF_ERR_INVALID, "glf_operator_solve: the %s band form takes ld 32 or 64 (ld = %u)", pix_desc(op->gen).name, ld);
    if (m == 0 || m > ld) return set_error(ctx, GLF_ERR_INVALID, "glf_operator_solve: m = %u columns of ld = %u (0 < m <= ld)", m, ld);
    if (!(rtol > 0.0) || max_it < 0) return set_error(ctx, GLF_ERR_INVALID, "glf_operator_solve: rtol = %g, max_it = %d", rtol, max_it);
    // the whole path's Jacobi preconditioner, whatever the form: 1 / (alpha (D_i - 1)) from the degree
    DevBuf<float> dinv;
    GLF_TRY(dinv.alloc(ctx, p));
    hipLaunchKernelGGL(k_dinv_from_degree, dim3((p + 255) / 256), dim3(256), 0, ctx->stream, op->degree, p, op->alpha, dinv.p);
    GLF_LAUNCH_CHECK(ctx);
    GLF_TRY(mv_collect(ctx));
    const int mv_count0 = ctx->mv_count, narrow0 = ctx->narrow_sweeps;
    int iters = 0, unconverged = 0;
    const int rc = operator_solve(ctx, op->store.LA.p, op->store.lda, p, m, ld, shard_arg(op->shard), dinv.p, B->data, X->data, R ? R->data : nullptr,
                                  (unsigned)round_up(p, VEC_PAD), rtol, max_it, &iters, &unconverged);
    if (rc != GLF_OK && rc != GLF_ERR_NOCONV) return rc;
    GLF_TRY(mv_collect(ctx));
    if (info) {
        info->iters = iters;
        info->unconverged = unconverged;
        info->matvecs = ctx->mv_count - mv_count0;
        info->narrow_sweeps = ctx->narrow_sweeps - narrow0;
        info->path = op->gop ? grid_op_path(op->gop) : 0;
        info->reserved = 0;
    }
    return rc; // (GLF_ERR_NOCONV: block_pcg_work's message stands)
}

int glf_operator_stored(const glf_operator *op, glf_mat *view)
{
    if (!op || !op->ctx || !view) return GLF_ERR_INVALID;
    if (op->gop) return set_error(op->ctx, GLF_ERR_UNSUPPORTED, "glf_operator_stored: a factored form stores no matrix");
    std::memset(view, 0, sizeof(*view));
    view->kind = GLF_MAT_DENSE;
    view->rows = op->p;
    view->cols = op->row1 - op->row0;
    view->ld = op->store.lda;
    view->data = op->store.LA.p;
    return GLF_OK;
}

int glf_operator_destroy(glf_operator *op)
{
    if (!op) return GLF_OK;
    if (op->ctx && hipSetDevice(op->ctx->device) != hipSuccess) return GLF_ERR_HIP;
    delete op;
    return GLF_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------
// The whole-path driver: plan, affinity, Laplacian, eigenpairs, wide or narrow, fused or unfused, planes tail
// ------------------------------------------------------------------------------------------

int glf::plan_run(glf_ctx *ctx, const glf_options *opt_in, PixGen gen, int width, int height, bool has_capture, bool has_signals, RunPlan *plan)
{
    RunPlan &P = *plan;
    glf_options &opt = P.opt;
    glf_options_default(&opt);
    if (opt_in) {
        if (opt_in->struct_size != sizeof(glf_options))
            return set_error(ctx, GLF_ERR_INVALID, "glf_options.struct_size %u != %zu", opt_in->struct_size, sizeof(glf_options));
        opt = *opt_in;
    }
    // a kernel reads one pixel format: the colour and 16-bit entry points take their format's bilateral kernel only (for which
    // GLF_KERNEL_BILATERAL stands there), the 8-bit entry points no kernel of another format. The colour and 16-bit guides have no
    // 8-bit y: their values are filtered as planes (u8_guide false)
    P.gen = gen;
    P.u8_guide = gen == PixGen::Grey;
    if (!P.u8_guide && opt.kernel == GLF_KERNEL_BILATERAL) opt.kernel = pix_desc(gen).kernel;
    if (pixgen_of(opt.kernel) != gen) {
        if (!P.u8_guide) {
            const char *what = pix_desc(gen).name;
            return set_error(ctx, GLF_ERR_UNSUPPORTED, "%s filtering: kernel %d (the %s bilateral kernel only)", what, opt.kernel, what);
        }
        const PixDesc &k = pix_desc(pixgen_of(opt.kernel));
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "the %s kernel takes %s: %s", k.name, k.image, k.entry);
    }
    if (opt.kernel < GLF_KERNEL_BILATERAL || opt.kernel > GLF_KERNEL_BILATERAL_RGBF32) return set_error(ctx, GLF_ERR_INVALID, "kernel %d", opt.kernel);
    if (opt.kernel == GLF_KERNEL_NLM && (width < 3 || height < 3))
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "non-local-means kernel: the image must be at least 3 x 3 pixels (%d x %d)", width, height);
    if (opt.filter_mode < GLF_FILTER_REFERENCE || opt.filter_mode > GLF_FILTER_SHARPEN) return set_error(ctx, GLF_ERR_INVALID, "filter_mode %d", opt.filter_mode);
    P.gain = filter_gain(opt);
    P.ysub = 1.0f - filter_ident(opt);
    P.N = (int64_t)width * height;
    if (P.N >= (int64_t)1 << 31) return set_error(ctx, GLF_ERR_UNSUPPORTED, "image too large");
    // p = width*height*0.01 (truncating), hpc/image_processing.c:187; Sampling rewrites it, :191-193
    P.p = opt.num_samples ? opt.num_samples : (unsigned)((double)P.N * opt.sample_frac);
    {
        unsigned *h_idx = nullptr;
        const int rc = opt.sampling == GLF_SAMPLING_RANDOM ? glf_RandomSampling(width, height, &P.p, &h_idx, opt.sampling_seed)
                                                           : glf_Sampling(width, height, &P.p, &h_idx);
        if (rc == GLF_OK && h_idx) P.samples.assign(h_idx, h_idx + P.p);
        std::free(h_idx);
        if (rc != GLF_OK || P.p < 2) return set_error(ctx, GLF_ERR_INVALID, "sampling failed (requested %u samples on %dx%d)", P.p, width, height);
    }
    // GetNumberEigenvalues, hpc/image_processing.c:96-108
    P.m = opt.num_eigvals;
    if (P.m == 0 || P.m >= P.p) P.m = P.p - 1;
    P.wide = P.m > PANEL_COLS;
    if (P.wide && opt.filter_mode == GLF_FILTER_SHARPEN) // (its Gram matrix Phi^T Phi would couple the panels)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "the sharpening filter takes at most %u eigenpairs (%u asked for)", PANEL_COLS, P.m);
    if (P.wide && has_capture) return set_error(ctx, GLF_ERR_UNSUPPORTED, "glf_capture with more than 256 eigenpairs");
    if (P.wide && (has_signals || !P.u8_guide)) // (a colour, 16-bit or float guide's own values are planes)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "signal planes with more than 256 eigenpairs (%u asked for)", P.m);
    P.ld = P.wide ? PANEL_COLS : ld_for(P.m);
    P.p32 = (unsigned)round_up(P.p, VEC_PAD);
    P.coef = make_coef(opt.kernel, opt.h_loc, opt.h_val);
    return GLF_OK;
}

// [*i0, *i1): the samples (ascending pixel indices) among the pixels [pix0, pix1) of this shard
static void samples_among(const std::vector<unsigned> &idx, int64_t pix0, int64_t pix1, unsigned *i0, unsigned *i1)
{
    const unsigned p = (unsigned)idx.size();
    unsigned i = 0;
    while (i < p && (int64_t)idx[i] < pix0) ++i;
    *i0 = i;
    while (i < p && (int64_t)idx[i] < pix1) ++i;
    *i1 = i;
}

// Closes the last stage (ev[5]) and re-times the stages from `first` on (ev[i] opens stage i) and the total; then *stats = S
static int finish_stats(glf_ctx *ctx, glf_stats &S, int first, glf_stats *stats)
{
    float glf_stats::*const stage_ms[5] = {&glf_stats::ms_affinity, &glf_stats::ms_laplacian, &glf_stats::ms_eigen, &glf_stats::ms_nystroem,
                                           &glf_stats::ms_filter};
    GLF_HIP(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
    GLF_HIP(ctx, hipEventSynchronize(ctx->ev[5]));
    for (int i = first; i < 5; ++i) GLF_HIP(ctx, hipEventElapsedTime(&(S.*stage_ms[i]), ctx->ev[i], ctx->ev[i + 1]));
    GLF_HIP(ctx, hipEventElapsedTime(&S.ms_total, ctx->ev[0], ctx->ev[5]));
    if (stats) *stats = S;
    return GLF_OK;
}

// This rank's Nystroem request as far as the image, its pixel range and the sample tables settle it, Phi's rows at their pixels
// (raster); the operand, the outputs and the report are the caller's to name
static NysRequest nys_request(const uint8_t *d_img, int width, int height, int64_t pix0, int64_t pix1, const SampleTables &tb, unsigned p,
                              KernelCoef coef)
{
    NysRequest rq;
    rq.d_img = d_img; rq.width = width; rq.height = height;
    rq.pix0 = pix0; rq.pix1 = pix1;
    rq.d_mask = tb.mask.p; rq.d_idx = tb.idx.p; rq.raster = 1;
    rq.d_samples = tb.samples.p; rq.p = p; rq.coef = coef;
    return rq;
}

// More than 256 eigenpairs, from the eigenpairs on. Panels of 256 vectors: the eigen-solve once (eigen.hip "panels"), then Nystroem,
// Phi^T y and the filter's correction one panel at a time -- only one [pixels][256] block of Phi exists at any moment.
static int run_wide_panels(glf_ctx *ctx, const RunPlan &P, const uint8_t *d_img, int width, int height, int64_t pix0, int64_t pix1,
                           const SampleTables &tb, OperatorStore &store, const MatShard &shard, const float *d_dinv, double alpha, uint8_t *d_out,
                           float *d_zf, double *eigvals_out, glf_stats &S, glf_stats *stats)
{
    const glf_options &opt = P.opt;
    const unsigned p = P.p, m = P.m;
    hipStream_t st = ctx->stream;
    const unsigned npan = (unsigned)ceil_div(m, PANEL_COLS);
    const size_t pstride = (size_t)P.p32 * PANEL_COLS;
    DevBuf<float> vecs;
    GLF_TRY(vecs.alloc(ctx, pstride * npan));
    std::vector<double> lam(m);
    GLF_TRY(inverse_power_iteration_panels(ctx, store.LA.p, store.lda, p, m, nullptr, opt.seed, opt.opti_gs, opt.epsilon, opt.inner_rtol,
                                           opt.max_outer > 0 ? opt.max_outer : 100000, vecs.p, lam.data(), &S.eig, shard.grid ? &shard : nullptr,
                                           d_dinv));
    store.LA.release();
    if (eigvals_out)
        for (unsigned j = 0; j < m; ++j) eigvals_out[j] = lam[j];
    GLF_HIP(ctx, hipEventRecord(ctx->ev[3], st));
    const int64_t npix = pix1 - pix0;
    DevBuf<float> psi, pinv, phi, w, acc;
    DevBuf<double> c;
    const size_t psi_n = (size_t)round_up(p, NYS_PAD) * PANEL_COLS;
    GLF_TRY(psi.alloc(ctx, psi_n));
    GLF_TRY(pinv.alloc(ctx, PANEL_COLS));
    GLF_TRY(w.alloc(ctx, PANEL_COLS));
    GLF_TRY(c.alloc(ctx, PANEL_COLS));
    GLF_TRY(phi.alloc(ctx, (size_t)npix * PANEL_COLS));
    GLF_TRY(acc.alloc(ctx, (size_t)npix));
    float *phi_base = phi.p - (size_t)pix0 * PANEL_COLS;
    unsigned si0, si1;
    samples_among(P.samples, pix0, pix1, &si0, &si1);
    float kms_total = 0.f;
    for (unsigned q = 0; q < npan; ++q) {
        const unsigned mq = std::min(PANEL_COLS, m - q * PANEL_COLS);
        const float *vq = vecs.p + q * pstride;
        const double *lamq = lam.data() + q * PANEL_COLS;
        std::vector<float> hp(PANEL_COLS, 0.f);
        for (unsigned j = 0; j < mq; ++j) hp[j] = (float)(1.0 / lamq[j]); // InverseDiagMat, hpc/utils.c:559-586
        GLF_HIP(ctx, hipMemcpyAsync(pinv.p, hp.data(), sizeof(float) * PANEL_COLS, hipMemcpyHostToDevice, st));
        GLF_HIP(ctx, hipStreamSynchronize(st));
        GLF_HIP(ctx, hipMemsetAsync(psi.p, 0, sizeof(float) * psi_n, st));
        hipLaunchKernelGGL(k_make_psi, dim3((unsigned)ceil_div((int64_t)p * PANEL_COLS, 256)), dim3(256), 0, st, vq, pinv.p, p, PANEL_COLS, mq,
                           (float)(-alpha), psi.p);
        GLF_LAUNCH_CHECK(ctx);
        GLF_HIP(ctx, hipMemsetAsync(c.p, 0, sizeof(double) * PANEL_COLS, st));
        float kms = 0.f;
        uint64_t evaluated = 0;
        NysRequest rq = nys_request(d_img, width, height, pix0, pix1, tb, p, P.coef);
        rq.d_psi = psi.p; rq.m = mq; rq.ld = PANEL_COLS;
        rq.d_phi = phi_base; rq.d_c = c.p; rq.window = opt.skip_exact_zeros;
        rq.kernel_ms = &kms; rq.entries_evaluated = &evaluated; rq.path = &S.nystroem_path;
        GLF_TRY(nystroem_contract(ctx, rq));
        kms_total += kms;
        S.nystroem_evaluated += (double)evaluated;
        if (si1 > si0)
            GLF_TRY(scatter_sample_rows(ctx, vq + (size_t)si0 * PANEL_COLS, si1 - si0, PANEL_COLS, tb.idx.p + si0, phi_base, 1, d_img, c.p, mq));
        GLF_TRY(allreduce_f64(ctx, c.p, PANEL_COLS)); // right = phi^T y over all ranks' pixels (this panel's columns)
        GLF_TRY(filter_panel(ctx, opt, mq, lamq, c.p, w.p, phi.p, pix0, pix1, acc.p, q == 0));
    }
    GLF_HIP(ctx, hipEventRecord(ctx->ev[4], st));
    GLF_TRY(filter_finish(ctx, d_img, acc.p, pix0, pix1, P.gain, P.ysub, d_out, d_zf));
    S.nystroem_launches = (int)npan;
    S.nystroem_kernel_ms = kms_total;
    S.contraction = ctx->contraction;
    S.skip_exact_zeros = opt.skip_exact_zeros;
    return finish_stats(ctx, S, 0, stats);
}

// The signal planes through the guide's operator, after the guide is complete: its outputs, stats and collectives are those of the
// plain call. Phi is written for them on every path: the fused guide filter never writes it, so it is extended here with the guide's
// own Psi and contraction (unfused: phi_base, the rows the guide's filter read, addressed by absolute pixel index). Every rank comes
// here, so the collectives match. sig_w: the planes' weights where the band launch fell back after c_s was formed, null otherwise.
static int filter_planes(glf_ctx *ctx, const RunPlan &P, const uint8_t *d_img, int width, int height, int64_t pix0, int64_t pix1,
                         const SampleTables &tb, double alpha, const float *d_psi, const float *d_phiA, unsigned si0, unsigned si1,
                         const std::vector<double> &lam, const std::vector<double> &hG, bool fused, float *phi_base, const SignalPlanes *sig,
                         const SignalPlanes *planes, const float *sig_w, uint8_t *d_out, float *d_zf, glf_stats &S, glf_stats *stats)
{
    const unsigned p = P.p, m = P.m, ld = P.ld;
    DevBuf<float> phis;
    float *phi_rows = phi_base; // rows addressed by absolute pixel index
    if (fused) {
        GLF_TRY(phis.alloc(ctx, (size_t)(pix1 - pix0) * ld));
        phi_rows = phis.p - (size_t)pix0 * ld;
        NysRequest rq = nys_request(d_img, width, height, pix0, pix1, tb, p, P.coef);
        rq.d_psi = d_psi; rq.m = m; rq.ld = ld;
        rq.d_phi = phi_rows; rq.window = P.opt.skip_exact_zeros;
        GLF_TRY(nystroem_contract(ctx, rq));
        if (si1 > si0) GLF_TRY(scatter_sample_rows(ctx, d_phiA + (size_t)si0 * ld, si1 - si0, ld, tb.idx.p + si0, phi_rows, 1, d_img, nullptr, m));
    }
    const FilterSpec F{P.opt, P.gen, P.N, m, ld, P.gain, P.ysub, lam.data(), true};
    GLF_TRY(filter_planes_tail(ctx, F, hG, phi_rows, pix0, pix1, d_img, sig, planes, sig_w, d_out, d_zf));
    if (!P.u8_guide) return finish_stats(ctx, S, 4, stats); // (the guide's own values were planes: the filter stage ends here)
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

int glf::image_processing_run(glf_ctx *ctx, const glf_options *opt_in, PixGen gen, const uint8_t *d_img, int width, int height, uint8_t *d_out,
                              float *d_zf, double *eigvals_out, glf_stats *stats, glf_capture *cap, const SignalPlanes *sig)
{
    // (all of these answer GLF_ERR_INVALID and leave last_error alone)
    if (!ctx || !d_img || !d_out || width <= 0 || height <= 0) return GLF_ERR_INVALID;
    if (sig && (sig->nsig < 1 || sig->nsig > GLF_MAX_SIGNALS || !sig->d_sig || !sig->d_out)) return GLF_ERR_INVALID;
    if (cap && cap->struct_size != sizeof(glf_capture))
        return set_error(ctx, GLF_ERR_INVALID, "glf_capture.struct_size %u != %zu", cap->struct_size, sizeof(glf_capture));
    GLF_ENTER(ctx);
    GLF_TRY(f32_admit(ctx, gen, d_img, width, height)); // (before anything else)
    pool_age(ctx);
    RunPlan plan;
    GLF_TRY(plan_run(ctx, opt_in, gen, width, height, cap != nullptr, sig != nullptr, &plan));
    return run_planned(ctx, plan, d_img, width, height, d_out, d_zf, eigvals_out, stats, cap, sig);
}

int glf::run_planned(glf_ctx *ctx, const RunPlan &P, const uint8_t *d_img, int width, int height, uint8_t *d_out, float *d_zf,
                     double *eigvals_out, glf_stats *stats, glf_capture *cap, const SignalPlanes *sig)
{
    const glf_options &opt = P.opt;
    const PixGen gen = P.gen;
    const bool u8_guide = P.u8_guide;
    const int64_t N = P.N;
    const unsigned p = P.p, m = P.m, ld = P.ld, p32 = P.p32;
    const unsigned *h_idx = P.samples.data();
    const KernelCoef coef = P.coef;
    hipStream_t st = ctx->stream;
    glf_stats S{};
    DevBuf<float> guide_planes; // colour: the channels as float planes [3][N] (Phi^T x_c); 16-bit: the image as one plane
    SignalPlanes guide_sig{};
    const SignalPlanes *planes = nullptr; // a colour or 16-bit guide's extra planes (its own kernels read the channels from the image)
    if (!u8_guide) {
        const int nch = pix_desc(gen).channels;
        planes = sig;
        if (!planes) {
            GLF_TRY(guide_planes.alloc(ctx, (size_t)nch * N));
            GLF_TRY(pix_planes(ctx, gen, d_img, N, guide_planes.p));
        }
        guide_sig = SignalPlanes{nch, guide_planes.p, nullptr};
        sig = &guide_sig;
    }
    int row0, row1;
    shard_rows(ctx, height, &row0, &row1);
    const int64_t pix0 = (int64_t)row0 * width, pix1 = (int64_t)row1 * width;
    S.p = p;
    S.m = m;
    S.row0 = row0;
    S.row1 = row1;

    GLF_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    // ---- affinity: sample tables + degree (K_B generated on the fly) -------------------------
    SampleTables tb;
    GLF_TRY(build_sample_tables(ctx, d_img, width, height, p, h_idx, tb, opt.kernel));
    DevBuf<double> deg; // D_A [p], then (grid-factored degree only) the value-weighted sums U[s] = sum_px K(s, px) y[px] [p]
    GLF_TRY(deg.alloc(ctx, 2 * (size_t)p));
    bool have_ysum = false;
    GLF_TRY(degree_rows_auto(ctx, d_img, width, height, row0, row1, tb.samples.p, p, h_idx, coef, deg.p, opt.skip_exact_zeros,
                             &S.degree_evaluated, tb.idx.p, deg.p + p, &have_ysum));
    GLF_TRY(allreduce_f64(ctx, deg.p, have_ysum ? 2 * (size_t)p : p));
    GLF_HIP(ctx, hipEventRecord(ctx->ev[1], st));
    if (cap) {
        cap->ld = ld;
        if (cap->h_degree) {
            GLF_HIP(ctx, hipMemcpyAsync(cap->h_degree, deg.p, sizeof(double) * p, hipMemcpyDeviceToHost, st));
            GLF_HIP(ctx, hipStreamSynchronize(st));
        }
        if ((cap->d_phi_A && cap->phi_A_floats < (size_t)p32 * ld) || (cap->d_phi && cap->phi_floats < (size_t)(pix1 - pix0) * ld) ||
            (cap->d_corr && cap->corr_floats < (size_t)(pix1 - pix0)))
            return set_error(ctx, GLF_ERR_INVALID, "glf_capture: phi_A needs %zu floats, phi %zu", (size_t)p32 * ld, (size_t)(pix1 - pix0) * ld);
    }
    // ---- Laplacian ---------------------------------------------------------------------------
    double dsum = 0.0;
    GLF_TRY(sum_host(ctx, deg.p, p, &dsum));
    const double alpha = 1.0 / (dsum / (double)p);
    S.alpha = alpha;
    // With a communicator that can all-gather, L_A is sharded: rank g holds the column block
    // L_A[:, r0:r1) (= its row block transposed; L_A is symmetric) and computes rows [r0,r1) of every
    // mat-vec. Otherwise (single GPU, f32 contraction, or no allgather callback) L_A is whole.
    MatShard shard;
    bool shard_eig = ctx->has_comm && ctx->comm.allgather_f32 && ctx->contraction == GLF_CONTRACT_F16_SPLIT && !P.wide;
    // For a tensor-grid sample set L_A is applied in grid-factored form and never stored (GLF_MV_PATH = grid | dense | auto;
    // auto: from 16 384 samples on -- below, streaming a small stored L_A is cheaper than the factored sweep's fixed cost)
    struct GridOpGuard {
        GridOp *op = nullptr;
        ~GridOpGuard() { grid_op_destroy(op); }
    } gop;
    GLF_TRY(operator_factored(ctx, tb.samples.p, h_idx, p, width, height, coef, opt.kernel, ld, &gop.op));
    S.matvec_path = gop.op ? grid_op_path(gop.op) : 0;
    // With the band form a sweep costs less (0.19 ms at cfg4) than the all-gather of its 21.8 MB operand block over xGMI
    // (~0.2-0.4 ms), and the whole eigen-solve (4.8 ms) less than the sharded one's 12 all-gathers + ~46 small all-reduces:
    // every rank then runs the eigen-solve on all rows (bit-identical to one GPU, no collective) and only the pixel rows
    // -- degree, extension, filter -- are sharded. EIG_SHARD=1 forces the row-sharded solve, 0 the replicated one.
    if (shard_eig && ((S.matvec_path == 4 && ctx->tune.eig_shard != 1) || ctx->tune.eig_shard == 2)) shard_eig = false;
    S.eigen_sharded = shard_eig ? 1 : 0;
    if (shard_eig) {
        shard.rows_per_rank = gop.op ? grid_op_rows_per_rank(gop.op, ctx->comm.size) : shard_rows_per_rank(p, ctx->comm.size);
        const uint64_t b = (uint64_t)shard.rows_per_rank * (unsigned)ctx->comm.rank;
        shard.row0 = (unsigned)(b < p ? b : p);
        shard.row1 = (unsigned)(b + shard.rows_per_rank < p ? b + shard.rows_per_rank : p);
    }
    OperatorStore store; // the skipping boxes and the stored L_A (neither with a factored operator)
    GLF_TRY(operator_store(ctx, gop.op, tb.samples.p, tb.idx.p, p, coef, opt.kernel, alpha, deg.p, opt.skip_exact_zeros, shard_eig, d_img, width,
                           height, shard, store));
    DevBuf<float> &LA = store.LA;
    DevBuf<float> dinv;
    const int64_t lda = store.lda;
    GLF_TRY(dinv.alloc(ctx, p));
    hipLaunchKernelGGL(k_dinv_from_degree, dim3((p + 255) / 256), dim3(256), 0, st, deg.p, p, alpha, dinv.p);
    GLF_LAUNCH_CHECK(ctx);
    GLF_HIP(ctx, hipEventRecord(ctx->ev[2], st));
    // ---- eigenpairs --------------------------------------------------------------------------
    if (P.wide) return run_wide_panels(ctx, P, d_img, width, height, pix0, pix1, tb, store, shard, dinv.p, alpha, d_out, d_zf, eigvals_out, S, stats);
    DevBuf<float> phiA;
    GLF_TRY(phiA.alloc(ctx, (size_t)p32 * ld));
    std::vector<double> lam(m);
    {
        const float *d_x0 = nullptr; // seeded start block (hpc/inverse_power_it.c:12-47), cached per (p, m, ld, seed)
        GLF_TRY(start_block_cached(ctx, p, m, ld, opt.seed, &d_x0));
        GLF_TRY(inverse_power_iteration(ctx, LA.p, lda, p, m, ld, nullptr, opt.opti_gs, opt.epsilon, opt.inner_rtol,
                                        opt.max_outer > 0 ? opt.max_outer : 100000, phiA.p, lam.data(), &S.eig, shard_arg(shard), dinv.p, d_x0));
    }
    if (shard_eig || gop.op) LA.release(); // (a whole stored L_A is used once more below: K_A y_A for the fused filter)
    if (cap && cap->d_phi_A) GLF_HIP(ctx, hipMemcpyAsync(cap->d_phi_A, phiA.p, sizeof(float) * (size_t)p32 * ld, hipMemcpyDeviceToDevice, st));
    if (eigvals_out)
        for (unsigned j = 0; j < m; ++j) eigvals_out[j] = lam[j];
    GLF_HIP(ctx, hipEventRecord(ctx->ev[3], st));
    // ---- Nystroem extension, written straight in raster order (Permutation folded in) ----------
    DevBuf<float> psi, pinv, phi, w;
    DevBuf<double> c;
    GLF_TRY(psi.alloc(ctx, (size_t)round_up(p, NYS_PAD) * ld));
    GLF_HIP(ctx, hipMemsetAsync(psi.p, 0, sizeof(float) * (size_t)round_up(p, NYS_PAD) * ld, st));
    GLF_TRY(pinv.alloc(ctx, ld));
    GLF_TRY(w.alloc(ctx, ld));
    GLF_TRY(c.alloc(ctx, ld));
    {
        std::vector<float> hp(ld, 0.f);
        for (unsigned j = 0; j < m; ++j) hp[j] = (float)(1.0 / lam[j]); // InverseDiagMat, hpc/utils.c:559-586
        GLF_HIP(ctx, hipMemcpyAsync(pinv.p, hp.data(), sizeof(float) * ld, hipMemcpyHostToDevice, st));
        GLF_HIP(ctx, hipStreamSynchronize(st));
    }
    hipLaunchKernelGGL(k_make_psi, dim3((unsigned)ceil_div((int64_t)p * ld, 256)), dim3(256), 0, st, phiA.p, pinv.p, p, ld, m,
                       (float)(-alpha), psi.p);
    GLF_LAUNCH_CHECK(ctx);
    const int64_t npix = pix1 - pix0;
    float kms = 0.f;
    uint64_t evaluated = 0;
    RowpassStats rps;
    auto nystroem_stats = [&]() {
        S.nystroem_rowpass_launches = rps.launches;
        S.nystroem_rowpass_ms = rps.ms;
        S.nystroem_rowpass_flops = rps.flops;
        S.nystroem_colpass_launches = rps.col_launches;
        S.nystroem_colpass_ms = rps.col_ms;
        S.nystroem_colpass_flops = rps.col_flops;
        S.rank_terms = rps.rank_R;
        S.nystroem_launches = 1;
        S.nystroem_kernel_ms = kms;
        S.contraction = ctx->contraction;
        S.skip_exact_zeros = opt.skip_exact_zeros;
        S.nystroem_evaluated = (double)evaluated; // kernel entries generated (listed chunks x 64 x workgroup pixels)
    };
    unsigned si0, si1;
    samples_among(P.samples, pix0, pix1, &si0, &si1);
    // the filter's weights from c = Phi^T y (sharpening: with hG = Phi^T Phi, f64 [ld][ld] over all ranks' pixels, filled on the unfused path)
    std::vector<double> hG;
    auto rule = [&](const double *hc, float *hw) { filter_weights_row(opt, m, lam.data(), hG.data(), ld, hc, hw); };
    // ---- band form with the filter in the kernel's epilogue: Phi is never written -----------------------------------------
    // c = Phi^T y is needed before the extension then: it follows from the degree stage's value-weighted sums (c_from_ysum).
    // ---- joint filtering on the band form: the planes ride in k_band's epilogue, Phi is never written for them either --------
    // c_s = Phi^T s the way c is formed for y: U_s from the grid-factored degree with s as the histogram weight (all-reduced in
    // a collective of its own), t_s = K_A s_A from one more operator application (the guide's own application is untouched),
    // then c_from_ysum with s_A in place of y_A. The route is voted on every rank (have_ysum is decided per rank).
    const int nsig = sig ? sig->nsig : 0;
    bool sig_fused = false, sig_done = false;
    DevBuf<float> sig_w; // [nsig][ld] the planes' filter weights once c_s is known
    if (sig) {
        const bool elig = u8_guide && gop.op && ld <= 64 && opt.filter_mode != GLF_FILTER_SHARPEN && ctx->contraction == GLF_CONTRACT_F16_SPLIT &&
                          (ctx->tune.nys_path == 0 || ctx->tune.nys_path == 4) && !ctx->tune.no_fused_filter && (have_ysum || pix0 == pix1);
        DevBuf<double> vote;
        GLF_TRY(vote.alloc(ctx, 1));
        double hv = elig ? 1.0 : 0.0;
        GLF_HIP(ctx, hipMemcpyAsync(vote.p, &hv, sizeof(double), hipMemcpyHostToDevice, st));
        GLF_TRY(allreduce_f64(ctx, vote.p, 1));
        GLF_HIP(ctx, hipMemcpyAsync(&hv, vote.p, sizeof(double), hipMemcpyDeviceToHost, st));
        GLF_HIP(ctx, hipStreamSynchronize(st));
        sig_fused = hv == (double)(ctx->has_comm ? ctx->comm.size : 1);
    }
    if (sig_fused) {
        DevBuf<double> us, cs, zdeg;
        DevBuf<float> xs, ts;
        GLF_TRY(us.alloc(ctx, (size_t)nsig * p));
        for (int k = 0; k < nsig; ++k) {
            if (pix1 == pix0) {
                GLF_HIP(ctx, hipMemsetAsync(us.p + (size_t)k * p, 0, sizeof(double) * p, st));
                continue;
            }
            float smax = 0.f;
            GLF_TRY(plane_absmax(ctx, sig->d_sig + (size_t)k * N + pix0, pix1 - pix0, &smax));
            const int rc = weighted_sums_grid(ctx, d_img, width, height, row0, row1, tb.samples.p, p, h_idx, coef, opt.skip_exact_zeros,
                                              sig->d_sig + (size_t)k * N, (double)smax, us.p + (size_t)k * p);
            if (rc != GLF_OK) return rc == GLF_ERR_UNSUPPORTED ? set_error(ctx, GLF_ERR_INVALID, "weighted sums: no grid-factored degree") : rc;
        }
        GLF_TRY(allreduce_f64(ctx, us.p, (size_t)nsig * p));
        GLF_TRY(xs.alloc(ctx, (size_t)p32 * 32));
        GLF_TRY(ts.alloc(ctx, (size_t)p32 * 32));
        GLF_TRY(zdeg.alloc(ctx, p));
        GLF_TRY(cs.alloc(ctx, (size_t)nsig * ld));
        GLF_TRY(sig_w.alloc(ctx, (size_t)nsig * ld));
        GLF_HIP(ctx, hipMemsetAsync(xs.p, 0, sizeof(float) * (size_t)p32 * 32, st));
        GLF_HIP(ctx, hipMemsetAsync(ts.p, 0, sizeof(float) * (size_t)p32 * 32, st));
        GLF_HIP(ctx, hipMemsetAsync(zdeg.p, 0, sizeof(double) * p, st));
        hipLaunchKernelGGL(k_sample_signal_columns, dim3((p + 255) / 256), dim3(256), 0, st, tb.idx.p, sig->d_sig, (int64_t)N, nsig, p, 32u, xs.p);
        GLF_LAUNCH_CHECK(ctx);
        GLF_TRY(grid_op_apply(ctx, gop.op, xs.p, ts.p, 32, -1.0, zdeg.p, 0, p, 0)); // K_A s_A for every plane's column
        for (int k = 0; k < nsig; ++k)
            GLF_TRY(c_from_ysum(ctx, psi.p, phiA.p, us.p + (size_t)k * p, ts.p + k, 32, tb.samples.p, p, ld, cs.p + (size_t)k * ld, xs.p + k));
        GLF_TRY(weights_from_c(ctx, cs.p, nsig, ld, rule, sig_w.p));
    }
    bool fused = false;
    if (have_ysum && (gop.op || LA.p) && ld <= 64 && opt.filter_mode != GLF_FILTER_SHARPEN && !(cap && cap->d_phi) &&
        ctx->contraction == GLF_CONTRACT_F16_SPLIT && (ctx->tune.nys_path == 0 || ctx->tune.nys_path == 4) && !ctx->tune.no_fused_filter) {
        // t = K_A y_A (the sample pixels' share of the sums over all pixels): one 32-column application of the operator
        DevBuf<float> ya, t;
        DevBuf<double> zdeg;
        GLF_TRY(ya.alloc(ctx, (size_t)p32 * 32));
        GLF_TRY(t.alloc(ctx, (size_t)p32 * 32));
        GLF_TRY(zdeg.alloc(ctx, p));
        GLF_HIP(ctx, hipMemsetAsync(ya.p, 0, sizeof(float) * (size_t)p32 * 32, st));
        GLF_HIP(ctx, hipMemsetAsync(t.p, 0, sizeof(float) * (size_t)p32 * 32, st));
        GLF_HIP(ctx, hipMemsetAsync(zdeg.p, 0, sizeof(double) * p, st));
        hipLaunchKernelGGL(k_sample_values_column, dim3((p + 255) / 256), dim3(256), 0, st, tb.samples.p, p, 32u, ya.p);
        GLF_LAUNCH_CHECK(ctx);
        if (gop.op) GLF_TRY(grid_op_apply(ctx, gop.op, ya.p, t.p, 32, -1.0, zdeg.p, 0, p, 0)); // -(0 X - K_A X) = K_A y_A
        else { // stored L_A = alpha (D - K_A): K_A y_A = D y_A - L_A y_A / alpha
            GLF_TRY(block_matvec(ctx, LA.p, lda, p, ya.p, t.p, 32, shard.kbox ? &shard : nullptr));
            hipLaunchKernelGGL(k_ka_from_la, dim3((p + 255) / 256), dim3(256), 0, st, tb.samples.p, deg.p, p, 32u, 1.0 / alpha, t.p);
            GLF_LAUNCH_CHECK(ctx);
        }
        GLF_TRY(c_from_ysum(ctx, psi.p, phiA.p, deg.p + p, t.p, 32, tb.samples.p, p, ld, c.p));
        GLF_TRY(weights_from_c(ctx, c.p, 1, ld, rule, w.p, cap ? cap->h_c : nullptr));
        BandFilter flt;
        flt.w = w.p;
        flt.gain = P.gain;
        flt.ysub = P.ysub;
        flt.out = d_out;
        flt.zf = d_zf;
        flt.corr = cap ? cap->d_corr : nullptr;
        if (sig_fused) {
            flt.sig = BandSignals{nsig, sig_w.p, sig->d_sig, sig->d_out, (int64_t)N};
            GLF_TRY(filter_sample_rows_signals(ctx, phiA.p + (size_t)si0 * ld, si1 - si0, ld, tb.idx.p + si0, nsig, sig_w.p, P.gain, P.ysub,
                                               sig->d_sig, sig->d_out, N));
        }
        // the sample pixels from their rows of Phi_A first (k_band leaves them alone: the host work between the two launches --
        // grid detection, cached tables -- then overlaps a kernel instead of following the long one)
        GLF_TRY(filter_sample_rows(ctx, phiA.p + (size_t)si0 * ld, si1 - si0, ld, tb.idx.p + si0, d_img, w.p, P.gain, P.ysub, d_out, d_zf,
                                   cap ? cap->d_corr : nullptr, pix0));
        NysRequest rq = nys_request(d_img, width, height, pix0, pix1, tb, p, coef);
        rq.h_idx = h_idx;
        rq.d_psi = psi.p; rq.m = m; rq.ld = ld;
        rq.flt = &flt;
        rq.kernel_ms = &kms; rq.entries_evaluated = &evaluated; rq.mfma_flops = &S.nystroem_mfma_flops;
        rq.path = &S.nystroem_path; rq.rowpass = &rps;
        const int rc = nystroem_band_filter(ctx, rq);
        if (rc == GLF_OK) {
            nystroem_stats();
            S.filter_fused = 1;
            GLF_HIP(ctx, hipEventRecord(ctx->ev[4], st));
            fused = true;
            sig_done = sig_fused;
        } else if (rc != GLF_ERR_UNSUPPORTED) return rc;
    }
    LA.release();
    float *phi_base = nullptr; // unfused: Phi's rows addressed by absolute pixel index
    if (!fused) {
        GLF_TRY(phi.alloc(ctx, (size_t)npix * ld));
        phi_base = phi.p - (size_t)pix0 * ld;
        GLF_HIP(ctx, hipMemsetAsync(c.p, 0, sizeof(double) * ld, st));
        NysRequest rq = nys_request(d_img, width, height, pix0, pix1, tb, p, coef);
        rq.d_psi = psi.p; rq.m = m; rq.ld = ld;
        rq.d_phi = phi_base; rq.d_c = u8_guide ? c.p : nullptr; rq.window = opt.skip_exact_zeros;
        rq.kernel_ms = &kms; rq.entries_evaluated = &evaluated; rq.mfma_flops = &S.nystroem_mfma_flops;
        rq.path = &S.nystroem_path; rq.rowpass = &rps;
        GLF_TRY(nystroem_contract(ctx, rq));
        nystroem_stats();
        // sample rows of this shard <- Phi_A, and their share of c
        if (si1 > si0)
            GLF_TRY(scatter_sample_rows(ctx, phiA.p + (size_t)si0 * ld, si1 - si0, ld, tb.idx.p + si0, phi_base, 1, d_img, u8_guide ? c.p : nullptr, m));
        if (u8_guide) GLF_TRY(allreduce_f64(ctx, c.p, ld)); // right = phi^T y over all ranks' pixels
        GLF_HIP(ctx, hipEventRecord(ctx->ev[4], st));
        // ---- filter ------------------------------------------------------------------------------
        // (no 8-bit y: the channels / the 16-bit image are filtered in the planes tail; those formats' entry-by-entry kernel is f32, their
        // band form (PIX_BAND) split f16)
        if (!u8_guide && S.nystroem_path != 4) S.contraction = GLF_CONTRACT_F32_MFMA;
        const FilterSpec F{opt, gen, N, m, ld, P.gain, P.ysub, lam.data(), true};
        if (opt.filter_mode == GLF_FILTER_SHARPEN) // hG = Phi^T Phi over all ranks' pixels (the sharpening weights, here and in the tail)
            GLF_TRY(filter_gram(ctx, F, phi_base, pix0, pix1, hG));
        if (cap && cap->d_phi) GLF_HIP(ctx, hipMemcpyAsync(cap->d_phi, phi.p, sizeof(float) * (size_t)npix * ld, hipMemcpyDeviceToDevice, st));
        if (u8_guide)
            GLF_TRY(filter_grey(ctx, F, hG, c.p, w.p, phi_base, pix0, pix1, d_img, d_out, d_zf, cap ? cap->d_corr : nullptr,
                                cap ? cap->h_c : nullptr));
    }
    GLF_TRY(finish_stats(ctx, S, 0, u8_guide ? stats : nullptr));
    // ---- planes tail ----------------------------------------------------------------------------
    if (sig && !sig_done)
        return filter_planes(ctx, P, d_img, width, height, pix0, pix1, tb, alpha, psi.p, phiA.p, si0, si1, lam, hG, fused, phi_base, sig, planes,
                             sig_fused ? sig_w.p : nullptr, d_out, d_zf, S, stats);
    return GLF_OK;
}
