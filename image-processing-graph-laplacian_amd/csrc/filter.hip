// filter.hip -- spectral filter reconstruction (hpc/display.c:58-83):
//   right = Phi^T y                (m reductions over all pixels)
//   z     = y + gain * Phi (f(Pi) right);  z > 255 -> 255;  (png_byte) cast
// Both kernels stream Phi (N x ld floats) once: HBM-bandwidth bound,
// 4 N ld + N bytes each.
#include "glf_internal.hpp"

#include <algorithm>
#include <cstring>

namespace glf {

// glf_filter_info's report of an apply launch: its kernel, LD instantiation and grid, and whether the grid strides the range
void note_apply(glf_ctx *ctx, unsigned kernel, unsigned ld, int64_t npix, int ppb, int64_t nblk)
{
    ctx->flt_note.kernels |= kernel;
    ctx->flt_note.ld = ld;
    ctx->flt_note.apply_blocks = (unsigned)nblk;
    ctx->flt_note.strided = nblk * ppb < npix ? 1u : 0u;
}

// partial[blk][j] = sum_{pix in blk} Phi[pix][j] * y[pix]
__global__ __launch_bounds__(256) void k_phi_t_y(const float *__restrict__ phi, const uint8_t *__restrict__ img, int64_t pix0,
                                                  int64_t pix1, unsigned ld, double *__restrict__ partial)
{
    __shared__ double sh[256];
    const int col = threadIdx.x % ld, rl = threadIdx.x / ld, nrl = 256 / ld;
    const int64_t base = pix0 + (int64_t)blockIdx.x * 1024;
    float acc = 0.f;
    double s = 0.0;
    int cnt = 0;
    for (int64_t r = rl; r < 1024; r += nrl) {
        const int64_t px = base + r;
        if (px >= pix1) break;
        acc = fmaf(phi[(size_t)px * ld + col], (float)img[px], acc);
        if (++cnt == 32) { // bounded f32 chains, f64 across them
            s += (double)acc;
            acc = 0.f;
            cnt = 0;
        }
    }
    s += (double)acc;
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < ld) {
        double t = 0.0;
        for (int r = 0; r < nrl; ++r) t += sh[r * ld + col];
        partial[(size_t)blockIdx.x * ld + col] = t;
    }
}

__global__ void k_cols_sum(const double *__restrict__ in, int nrows, unsigned ld, double *__restrict__ out)
{
    // one workgroup per column chunk: 256 threads stride the rows, tree-reduce in LDS (fixed order)
    __shared__ double sh[256];
    const unsigned c = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < nrows; r += 256) s += in[(size_t)r * ld + c];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = sh[0];
}

int phi_t_y(glf_ctx *ctx, const float *d_phi, const uint8_t *d_img, int64_t pix0, int64_t pix1, unsigned /*m*/, unsigned ld,
            double *d_c)
{
    if (!valid_ld(ld) || pix0 > pix1) return set_error(ctx, GLF_ERR_INVALID, "phi_t_y: ld=%u", ld);
    if (pix0 == pix1) {
        GLF_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof(double) * ld, ctx->stream));
        return GLF_OK;
    }
    const int nblk = (int)ceil_div(pix1 - pix0, 1024);
    DevBuf<double> part;
    GLF_TRY(part.alloc(ctx, (size_t)nblk * ld));
    hipLaunchKernelGGL(k_phi_t_y, dim3(nblk), dim3(256), 0, ctx->stream, d_phi, d_img, pix0, pix1, ld, part.p);
    ctx->flt_note.kernels |= GLF_FK_PHI_T_Y;
    ctx->flt_note.proj_blocks = (unsigned)nblk;
    hipLaunchKernelGGL(k_cols_sum, dim3(ld), dim3(256), 0, ctx->stream, part.p, nblk, ld, d_c);
    GLF_LAUNCH_CHECK(ctx);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

// ---- c = Phi^T y without Phi (band form with the filter in the Nystroem kernel's epilogue) ---------------------------------
// Phi's rows are Phi_A at the sample pixels and sum_s K(px, s) Psi[s] elsewhere, so
//   c[n] = sum_s Phi_A[s][n] y_s + sum_s Psi[s][n] u_s,   u_s = sum over the NON-sample pixels of K(px, s) y[px]
// and u = (the degree stage's value-weighted sums over all pixels) - K_A y_A. f64 throughout; 128 samples per workgroup.
__global__ __launch_bounds__(256) void k_c_from_ysum(const float *__restrict__ psi, const float *__restrict__ phiA,
                                                      const double *__restrict__ ysum, const float *__restrict__ t, unsigned t_ld,
                                                      const float4 *__restrict__ samples, unsigned p, unsigned ld,
                                                      double *__restrict__ partial, const float *__restrict__ sval)
{
    __shared__ double sh[256];
    const int col = threadIdx.x % ld, rl = threadIdx.x / ld, nrl = 256 / ld;
    double acc = 0.0;
    const unsigned base = blockIdx.x * 128u;
    for (unsigned r = rl; r < 128u; r += nrl) {
        const unsigned s = base + r;
        if (s >= p) break;
        const double u = ysum[s] - (double)t[(size_t)s * t_ld];
        acc = fma((double)psi[(size_t)s * ld + col], u, acc);
        acc = fma((double)phiA[(size_t)s * ld + col], sval ? (double)sval[(size_t)s * t_ld] : (double)samples[s].z, acc);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < ld) {
        double tot = 0.0;
        for (int r = 0; r < nrl; ++r) tot += sh[r * ld + col];
        partial[(size_t)blockIdx.x * ld + col] = tot;
    }
}

int c_from_ysum(glf_ctx *ctx, const float *d_psi, const float *d_phiA, const double *d_ysum, const float *d_t, unsigned t_ld,
                const float4 *d_samples, unsigned p, unsigned ld, double *d_c, const float *d_sval)
{
    if (!valid_ld(ld)) return set_error(ctx, GLF_ERR_INVALID, "c_from_ysum: ld=%u", ld);
    const int nblk = (int)ceil_div(p, 128u);
    DevBuf<double> part;
    GLF_TRY(part.alloc(ctx, (size_t)nblk * ld));
    hipLaunchKernelGGL(k_c_from_ysum, dim3(nblk), dim3(256), 0, ctx->stream, d_psi, d_phiA, d_ysum, d_t, t_ld, d_samples, p, ld, part.p, d_sval);
    hipLaunchKernelGGL(k_cols_sum, dim3(ld), dim3(256), 0, ctx->stream, part.p, nblk, ld, d_c);
    GLF_LAUNCH_CHECK(ctx);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (part goes out of scope)
    return GLF_OK;
}

// partial[blk][i][j] = sum over the pixels of block blk of Phi[px][i] Phi[px][j] (blocks stride the range): the Gram matrix of
// the extended eigenvectors, which are not orthonormal -- what sits between the factors of the PoC's sharpening filter
// (python/image_processing.py:231-235). f32 products, f64 across chains of 32.
__global__ __launch_bounds__(256) void k_phi_gram(const float *__restrict__ phi, int64_t pix0, int64_t pix1, unsigned ld,
                                                   double *__restrict__ partial)
{
    extern __shared__ float tile[]; // [64 pixels][ld]
    const unsigned npair = ld * ld, e0 = blockIdx.y * 4096u; // this workgroup's 4096 pairs (i, j): 16 per thread
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0;
    for (int64_t base = pix0 + (int64_t)blockIdx.x * 64; base < pix1; base += (int64_t)gridDim.x * 64) {
        const int npx = (int)((pix1 - base) < 64 ? (pix1 - base) : 64);
        __syncthreads();
        for (unsigned e = threadIdx.x; e < 64 * ld; e += 256) tile[e] = e < (unsigned)npx * ld ? phi[(size_t)base * ld + e] : 0.f;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const unsigned e = e0 + q * 256 + threadIdx.x;
            if (e < npair) {
                const unsigned i = e / ld, j = e % ld;
                float a = 0.f;
                for (int r = 0; r < 64; ++r) a = fmaf(tile[r * ld + i], tile[r * ld + j], a);
                acc[q] += (double)a;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const unsigned e = e0 + q * 256 + threadIdx.x;
        if (e < npair) partial[(size_t)blockIdx.x * npair + e] = acc[q];
    }
}

// d_G[ld][ld] (f64) = Phi^T Phi over the pixels [pix0, pix1) of this rank
int phi_gram(glf_ctx *ctx, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, double *d_G)
{
    if (!valid_ld(ld) || pix0 > pix1) return set_error(ctx, GLF_ERR_INVALID, "phi_gram: ld=%u", ld);
    const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(512, ceil_div(pix1 - pix0, 64)));
    DevBuf<double> part;
    GLF_TRY(part.alloc(ctx, (size_t)nblk * ld * ld));
    ctx->flt_note.kernels |= GLF_FK_PHI_GRAM;
    hipLaunchKernelGGL(k_phi_gram, dim3(nblk, (unsigned)ceil_div((int64_t)ld * ld, 4096)), dim3(256), 64 * ld * sizeof(float), ctx->stream, d_phi,
                       pix0, pix1, ld, part.p);
    hipLaunchKernelGGL(k_cols_sum, dim3(ld * ld), dim3(256), 0, ctx->stream, part.p, nblk, ld * ld, d_G);
    GLF_LAUNCH_CHECK(ctx);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

// z[pix] = y + gain * sum_j Phi[pix][j] w[j]; LD/4 lanes per pixel, float4 each.
template <int LD>
__global__ __launch_bounds__(256) void k_apply_filter(const uint8_t *__restrict__ img, const float *__restrict__ phi,
                                                       int64_t pix0, int64_t pix1, const float *__restrict__ w, float gain, float ysub,
                                                       uint8_t *__restrict__ out, float *__restrict__ zf, float *__restrict__ corr)
{
    constexpr int LPP = LD / 4;       // lanes per pixel (8 .. 64)
    constexpr int PPB = 256 / LPP;    // pixels per block pass
    const int q = threadIdx.x % LPP, pl = threadIdx.x / LPP;
    const float4 wq = reinterpret_cast<const float4 *>(w)[q];
    for (int64_t px = pix0 + (int64_t)blockIdx.x * PPB + pl; px < pix1; px += (int64_t)gridDim.x * PPB) {
        const float4 f = reinterpret_cast<const float4 *>(phi + (size_t)px * LD)[q];
        float s = f.x * wq.x + f.y * wq.y + f.z * wq.z + f.w * wq.w;
#pragma unroll
        for (int o = LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (q == 0) {
            const int y = (int)img[px];
            // the correction 3.0 * Lapl_y, hpc/display.c:64-73; ysub = 1 for the filters without a y term (z = Phi f Phi^T y):
            // y is an integer, so y + floor(c - y) is the truncation of their z
            const float c = gain * s - ysub * (float)y;
            if (zf) zf[px] = (float)y + c;           // MatAXPY(z, 3.0, Lapl_y) as a float (resolves c to ulp(z) only)
            if (corr) corr[px - pix0] = c;
            out[px] = filter_output(y, c);
        }
    }
}

// the same for n sample pixels, each from its row of Phi_A: px = idx[i] (k_apply_filter's arithmetic)
template <int LD>
__global__ __launch_bounds__(256) void k_filter_sample_rows(const uint8_t *__restrict__ img, const float *__restrict__ phiA, unsigned n,
                                                             const uint32_t *__restrict__ idx, const float *__restrict__ w, float gain,
                                                             float ysub, uint8_t *__restrict__ out, float *__restrict__ zf,
                                                             float *__restrict__ corr, int64_t pix0)
{
    constexpr int LPP = LD / 4, PPB = 256 / LPP;
    const int q = threadIdx.x % LPP, pl = threadIdx.x / LPP;
    const float4 wq = reinterpret_cast<const float4 *>(w)[q];
    const unsigned i = blockIdx.x * PPB + pl;
    const bool live = i < n;
    const float4 f = live ? reinterpret_cast<const float4 *>(phiA + (size_t)i * LD)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    float s = f.x * wq.x + f.y * wq.y + f.z * wq.z + f.w * wq.w;
#pragma unroll
    for (int o = LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (q == 0 && live) {
        const int64_t px = (int64_t)idx[i];
        const int y = (int)img[px];
        const float c = gain * s - ysub * (float)y;
        if (zf) zf[px] = (float)y + c;
        if (corr) corr[px - pix0] = c;
        out[px] = filter_output(y, c);
    }
}

int filter_sample_rows(glf_ctx *ctx, const float *d_phiA, unsigned n, unsigned ld, const uint32_t *d_idx, const uint8_t *d_img,
                       const float *d_w, float gain, float ysub, uint8_t *d_out, float *d_zf, float *d_corr, int64_t pix0)
{
    if (n == 0) return GLF_OK;
    if (ld != 32 && ld != 64) return set_error(ctx, GLF_ERR_INVALID, "filter_sample_rows: ld=%u", ld);
    const unsigned ppb = 256 / (ld / 4);
    const dim3 grid((unsigned)ceil_div(n, ppb)), block(256);
    if (ld == 32) hipLaunchKernelGGL(k_filter_sample_rows<32>, grid, block, 0, ctx->stream, d_img, d_phiA, n, d_idx, d_w, gain, ysub, d_out, d_zf, d_corr, pix0);
    else hipLaunchKernelGGL(k_filter_sample_rows<64>, grid, block, 0, ctx->stream, d_img, d_phiA, n, d_idx, d_w, gain, ysub, d_out, d_zf, d_corr, pix0);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

int apply_filter(glf_ctx *ctx, const uint8_t *d_img, const float *d_phi, int64_t pix0, int64_t pix1, unsigned /*m*/,
                 unsigned ld, const float *d_w, float gain, float ysub, uint8_t *d_out, float *d_zf, float *d_corr)
{
    if (!valid_ld(ld) || pix0 > pix1) return set_error(ctx, GLF_ERR_INVALID, "apply_filter: ld=%u", ld);
    if (pix0 == pix1) return GLF_OK;
    const int ppb = 256 / (ld / 4);
    int64_t nblk = ceil_div(pix1 - pix0, ppb);
    if (nblk > 8192) nblk = 8192; // grid-stride the rest
    dim3 grid((unsigned)nblk), block(256);
    note_apply(ctx, GLF_FK_APPLY, ld, pix1 - pix0, ppb, nblk);
    switch (ld) {
    case 32: hipLaunchKernelGGL(k_apply_filter<32>, grid, block, 0, ctx->stream, d_img, d_phi, pix0, pix1, d_w, gain, ysub, d_out, d_zf, d_corr); break;
    case 64: hipLaunchKernelGGL(k_apply_filter<64>, grid, block, 0, ctx->stream, d_img, d_phi, pix0, pix1, d_w, gain, ysub, d_out, d_zf, d_corr); break;
    case 128: hipLaunchKernelGGL(k_apply_filter<128>, grid, block, 0, ctx->stream, d_img, d_phi, pix0, pix1, d_w, gain, ysub, d_out, d_zf, d_corr); break;
    case 256: hipLaunchKernelGGL(k_apply_filter<256>, grid, block, 0, ctx->stream, d_img, d_phi, pix0, pix1, d_w, gain, ysub, d_out, d_zf, d_corr); break;
    }
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// ---- extra signal planes through the guide's operator (glf_image_processing_signals) ------------------------------------
// Each plane s_k (float [N], replicated) goes through z_k = (1 - ysub) s_k + gain Phi w_k with w_k = f(Pi) Phi^T s_k. Every
// signal is its own accumulator chain in the same order whatever nsig is, so a plane's result does not depend on the others.

// partial[blk][k][j] = sum_{pix in blk} Phi[pix][j] * s_k[pix]: one read of Phi for all planes. The products are exact in
// f64 and summed in f64: a signed, zero-mean plane (chroma, a noise field) makes Phi^T s a sum with heavy cancellation, where
// k_phi_t_y's bounded f32 chains would lose ~1e-7 x sqrt(N) of it
__global__ __launch_bounds__(256) void k_phi_t_signals(const float *__restrict__ phi, const float *__restrict__ sig, int64_t N, int nsig,
                                                        int64_t pix0, int64_t pix1, unsigned ld, double *__restrict__ partial)
{
    __shared__ double sh[GLF_MAX_SIGNALS][256];
    const int col = threadIdx.x % ld, rl = threadIdx.x / ld, nrl = 256 / ld;
    const int64_t base = pix0 + (int64_t)blockIdx.x * 1024;
    double s[GLF_MAX_SIGNALS];
#pragma unroll
    for (int k = 0; k < GLF_MAX_SIGNALS; ++k) s[k] = 0.0;
    for (int64_t r = rl; r < 1024; r += nrl) {
        const int64_t px = base + r;
        if (px >= pix1) break;
        const double f = (double)phi[(size_t)px * ld + col];
#pragma unroll
        for (int k = 0; k < GLF_MAX_SIGNALS; ++k)
            if (k < nsig) s[k] = fma(f, (double)sig[(size_t)k * N + px], s[k]);
    }
#pragma unroll
    for (int k = 0; k < GLF_MAX_SIGNALS; ++k) sh[k][threadIdx.x] = s[k];
    __syncthreads();
    if (threadIdx.x < ld)
        for (int k = 0; k < nsig; ++k) {
            double t = 0.0;
            for (int r = 0; r < nrl; ++r) t += sh[k][r * ld + col];
            partial[((size_t)blockIdx.x * nsig + k) * ld + col] = t;
        }
}

int phi_t_signals(glf_ctx *ctx, const float *d_phi, const float *d_sig, int64_t N, int nsig, int64_t pix0, int64_t pix1, unsigned ld,
                  double *d_c)
{
    if (!valid_ld(ld) || pix0 > pix1 || nsig < 1 || nsig > GLF_MAX_SIGNALS)
        return set_error(ctx, GLF_ERR_INVALID, "phi_t_signals: ld=%u nsig=%d", ld, nsig);
    if (pix0 == pix1) {
        GLF_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof(double) * ld * nsig, ctx->stream));
        return GLF_OK;
    }
    const int nblk = (int)ceil_div(pix1 - pix0, 1024);
    DevBuf<double> part;
    GLF_TRY(part.alloc(ctx, (size_t)nblk * nsig * ld));
    hipLaunchKernelGGL(k_phi_t_signals, dim3(nblk), dim3(256), 0, ctx->stream, d_phi, d_sig, N, nsig, pix0, pix1, ld, part.p);
    ctx->flt_note.kernels |= GLF_FK_PHI_T_SIGNALS;
    ctx->flt_note.proj_blocks = (unsigned)nblk;
    hipLaunchKernelGGL(k_cols_sum, dim3(ld * nsig), dim3(256), 0, ctx->stream, part.p, nblk, ld * nsig, d_c);
    GLF_LAUNCH_CHECK(ctx);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

// out_k[pix] = s_k + (gain * sum_j Phi[pix][j] w_k[j] - ysub * s_k): k_apply_filter's per-pixel arithmetic with the plane's
// value in place of y, unclamped; each Phi row read once for all planes
template <int LD>
__global__ __launch_bounds__(256) void k_apply_filter_signals(const float *__restrict__ phi, int64_t pix0, int64_t pix1, int nsig,
                                                               const float *__restrict__ w, float gain, float ysub,
                                                               const float *__restrict__ sig, float *__restrict__ out, int64_t N)
{
    constexpr int LPP = LD / 4, PPB = 256 / LPP;
    const int q = threadIdx.x % LPP, pl = threadIdx.x / LPP;
    float4 wq[GLF_MAX_SIGNALS];
#pragma unroll
    for (int k = 0; k < GLF_MAX_SIGNALS; ++k)
        wq[k] = k < nsig ? reinterpret_cast<const float4 *>(w + (size_t)k * LD)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t px = pix0 + (int64_t)blockIdx.x * PPB + pl; px < pix1; px += (int64_t)gridDim.x * PPB) {
        const float4 f = reinterpret_cast<const float4 *>(phi + (size_t)px * LD)[q];
#pragma unroll
        for (int k = 0; k < GLF_MAX_SIGNALS; ++k) {
            if (k >= nsig) break;
            float s = f.x * wq[k].x + f.y * wq[k].y + f.z * wq[k].z + f.w * wq[k].w;
#pragma unroll
            for (int o = LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (q == 0) {
                const float v = sig[(size_t)k * N + px];
                const float c = gain * s - ysub * v;
                out[(size_t)k * N + px] = v + c;
            }
        }
    }
}

// max |s| over n floats (the f16 operand scale of the weighted histogram): non-negative floats order as their bit patterns
__global__ __launch_bounds__(256) void k_plane_absmax(const float *__restrict__ s, int64_t n, unsigned *__restrict__ out)
{
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, fabsf(s[i]));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}

int plane_absmax(glf_ctx *ctx, const float *d_s, int64_t n, float *h_max)
{
    *h_max = 0.f;
    if (n <= 0) return GLF_OK;
    DevBuf<unsigned> m;
    GLF_TRY(m.alloc(ctx, 1));
    GLF_HIP(ctx, hipMemsetAsync(m.p, 0, sizeof(unsigned), ctx->stream));
    hipLaunchKernelGGL(k_plane_absmax, dim3((unsigned)std::min<int64_t>(1024, ceil_div(n, 256))), dim3(256), 0, ctx->stream, d_s, n, m.p);
    GLF_LAUNCH_CHECK(ctx);
    unsigned bits = 0;
    GLF_HIP(ctx, hipMemcpyAsync(&bits, m.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_max, &bits, sizeof(float));
    return GLF_OK;
}

// the planes at n sample pixels px = idx[i], each from its row of Phi_A (k_filter_sample_rows' arithmetic per plane)
template <int LD>
__global__ __launch_bounds__(256) void k_filter_sample_rows_signals(const float *__restrict__ phiA, unsigned n, const uint32_t *__restrict__ idx,
                                                                     int nsig, const float *__restrict__ w, float gain, float ysub,
                                                                     const float *__restrict__ sig, float *__restrict__ out, int64_t N)
{
    constexpr int LPP = LD / 4, PPB = 256 / LPP;
    const int q = threadIdx.x % LPP, pl = threadIdx.x / LPP;
    const unsigned i = blockIdx.x * PPB + pl;
    const bool live = i < n;
    const float4 f = live ? reinterpret_cast<const float4 *>(phiA + (size_t)i * LD)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < nsig; ++k) {
        const float4 wq = reinterpret_cast<const float4 *>(w + (size_t)k * LD)[q];
        float s = f.x * wq.x + f.y * wq.y + f.z * wq.z + f.w * wq.w;
#pragma unroll
        for (int o = LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (q == 0 && live) {
            const int64_t px = (int64_t)idx[i];
            const float v = sig[(size_t)k * N + px];
            out[(size_t)k * N + px] = v + (gain * s - ysub * v);
        }
    }
}

int filter_sample_rows_signals(glf_ctx *ctx, const float *d_phiA, unsigned n, unsigned ld, const uint32_t *d_idx, int nsig, const float *d_w,
                               float gain, float ysub, const float *d_sig, float *d_out, int64_t N)
{
    if (n == 0) return GLF_OK;
    if ((ld != 32 && ld != 64) || nsig < 1 || nsig > GLF_MAX_SIGNALS)
        return set_error(ctx, GLF_ERR_INVALID, "filter_sample_rows_signals: ld=%u nsig=%d", ld, nsig);
    const unsigned ppb = 256 / (ld / 4);
    const dim3 grid((unsigned)ceil_div(n, ppb)), block(256);
    if (ld == 32) hipLaunchKernelGGL(k_filter_sample_rows_signals<32>, grid, block, 0, ctx->stream, d_phiA, n, d_idx, nsig, d_w, gain, ysub, d_sig, d_out, N);
    else hipLaunchKernelGGL(k_filter_sample_rows_signals<64>, grid, block, 0, ctx->stream, d_phiA, n, d_idx, nsig, d_w, gain, ysub, d_sig, d_out, N);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

int apply_filter_signals(glf_ctx *ctx, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, int nsig, const float *d_w, float gain,
                         float ysub, const float *d_sig, float *d_out, int64_t N)
{
    if (!valid_ld(ld) || pix0 > pix1 || nsig < 1 || nsig > GLF_MAX_SIGNALS)
        return set_error(ctx, GLF_ERR_INVALID, "apply_filter_signals: ld=%u nsig=%d", ld, nsig);
    if (pix0 == pix1) return GLF_OK;
    const int ppb = 256 / (ld / 4);
    int64_t nblk = ceil_div(pix1 - pix0, ppb);
    if (nblk > 8192) nblk = 8192; // grid-stride the rest
    dim3 grid((unsigned)nblk), block(256);
    note_apply(ctx, GLF_FK_APPLY_SIGNALS, ld, pix1 - pix0, ppb, nblk);
    switch (ld) {
    case 32: hipLaunchKernelGGL(k_apply_filter_signals<32>, grid, block, 0, ctx->stream, d_phi, pix0, pix1, nsig, d_w, gain, ysub, d_sig, d_out, N); break;
    case 64: hipLaunchKernelGGL(k_apply_filter_signals<64>, grid, block, 0, ctx->stream, d_phi, pix0, pix1, nsig, d_w, gain, ysub, d_sig, d_out, N); break;
    case 128: hipLaunchKernelGGL(k_apply_filter_signals<128>, grid, block, 0, ctx->stream, d_phi, pix0, pix1, nsig, d_w, gain, ysub, d_sig, d_out, N); break;
    case 256: hipLaunchKernelGGL(k_apply_filter_signals<256>, grid, block, 0, ctx->stream, d_phi, pix0, pix1, nsig, d_w, gain, ysub, d_sig, d_out, N); break;
    }
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// ---- the same filter for more than 256 eigenpairs: one 256-column panel of Phi at a time ------------------------------
__global__ __launch_bounds__(256) void k_filter_accum(const float *__restrict__ phi, int64_t pix0, int64_t pix1,
                                                       const float *__restrict__ w, float *__restrict__ acc, int first)
{
    constexpr int LD = 256, LPP = LD / 4, PPB = 256 / LPP;
    const int q = threadIdx.x % LPP, pl = threadIdx.x / LPP;
    const float4 wq = reinterpret_cast<const float4 *>(w)[q];
    for (int64_t px = pix0 + (int64_t)blockIdx.x * PPB + pl; px < pix1; px += (int64_t)gridDim.x * PPB) {
        const float4 f = reinterpret_cast<const float4 *>(phi + (size_t)(px - pix0) * LD)[q];
        float s = f.x * wq.x + f.y * wq.y + f.z * wq.z + f.w * wq.w;
#pragma unroll
        for (int o = LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (q == 0) acc[px - pix0] = first ? s : acc[px - pix0] + s;
    }
}

__global__ __launch_bounds__(256) void k_filter_finish(const uint8_t *__restrict__ img, const float *__restrict__ acc, int64_t pix0,
                                                        int64_t pix1, float gain, float ysub, uint8_t *__restrict__ out,
                                                        float *__restrict__ zf)
{
    const int64_t px = pix0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (px >= pix1) return;
    const int y = (int)img[px];
    const float c = gain * acc[px - pix0] - ysub * (float)y;
    if (zf) zf[px] = (float)y + c;
    out[px] = filter_output(y, c);
}

// d_phi: this panel's rows for the pixels [pix0, pix1), [pix1 - pix0][256]
int filter_accumulate(glf_ctx *ctx, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, const float *d_w, float *d_acc, bool first)
{
    if (ld != PANEL_COLS || pix0 > pix1) return set_error(ctx, GLF_ERR_INVALID, "filter_accumulate: ld=%u", ld);
    if (pix0 == pix1) return GLF_OK;
    int64_t nblk = ceil_div(pix1 - pix0, 4);
    if (nblk > 8192) nblk = 8192;
    note_apply(ctx, GLF_FK_ACCUM, ld, pix1 - pix0, 4, nblk);
    hipLaunchKernelGGL(k_filter_accum, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, d_phi, pix0, pix1, d_w, d_acc, first ? 1 : 0);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

int filter_finish(glf_ctx *ctx, const uint8_t *d_img, const float *d_acc, int64_t pix0, int64_t pix1, float gain, float ysub, uint8_t *d_out,
                  float *d_zf)
{
    if (pix0 >= pix1) return GLF_OK;
    ctx->flt_note.kernels |= GLF_FK_FINISH;
    hipLaunchKernelGGL(k_filter_finish, dim3((unsigned)ceil_div(pix1 - pix0, 256)), dim3(256), 0, ctx->stream, d_img, d_acc, pix0, pix1, gain,
                       ysub, d_out, d_zf);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

} // namespace glf
