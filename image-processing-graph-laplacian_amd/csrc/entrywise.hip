// entrywise.hip -- the pixel formats without a factored form behind the same stage API as the grey kernels: the colour bilateral
// affinity (glf_options.kernel = GLF_KERNEL_BILATERAL_RGB, image interleaved uint8 [height][width][3]) and the bilateral affinity
// on 16-bit grey values (GLF_KERNEL_BILATERAL_U16, image uint16_t [height][width]) and on float values (GLF_KERNEL_BILATERAL_F32, image
// float [height][width], any finite value), and the colour affinity on float channels (GLF_KERNEL_BILATERAL_RGBF32, image interleaved
// float [height][width][3]):
//
//   K(i, j) = Es(dr) Es(dc) P(v_i - v_j) = exp2(-(s_loc (dr^2 + dc^2) + s_val |v_i - v_j|^2))
//
// with v the pixel's colour, 16-bit or float value, read and compared through the format's policy Pix<G> (glf_internal.hpp). The
// photometric factor is at most 1, so every spatial bound of the grey kernels (the f32 underflow radius, the chunk boxes of the
// Nystroem window) holds unchanged. A colour guide has 2^24 values and a 16-bit guide 65 536, so the forms that factor the sums over
// the 256 grey levels (grid, rank, band) and the grey direct degree (a 256-entry table per sample) do not extend: those routes
// decline the kernel and the entry-by-entry kernels run --
//   k_degree_entrywise<G>               D[i] = sum over the rank's pixel rows of K(sample i, pixel)   lane = sample, pixel tiles in LDS
//   k_sample_matrix<G> (affinity.hip)   K_A / L_A from the sample records (U16 takes the grey instantiation: the same records)
//   k_nystroem<.., G> (nystroem.hip)    Phi = K_B^T Psi, f32 MFMA with the format's pixel read
//   k_apply_filter_pix<LD, G>           the outputs and z, dot products in f64
//   k_phi_t_pix_signals<G>, k_apply_filter_pix_signals<LD, G>   the same filter stage with 1-4 float planes riding along
//
// Arithmetic at 16 bits. dv = v_i - v_j is exact in f32 (|dv| < 2^16), dv^2 is not (up to 32 bits): it is rounded once (relative
// error <= 2^-24), and so is the exponent t = s_val dv^2 + s_loc q (q = dr^2 + dc^2 exact) in its fma, so t carries a relative error
// of at most ~2^-23 -- the same order as the f32 rounding of s_val itself, which the 8-bit kernels have too. exp2(-t) then moves by
// |dK| <= K t ln2 2^-23 <= (1/e) 2^-23 ~ 4.4e-8 absolute (the maximum of x e^-x at x = 1), and v_exp_f32 adds its own ~1 ulp: every
// entry of K_A and K_B is within ~1e-7 of the fp64 kernel, well inside 1e-6 of max|K| = 1. The colour distance is exact (integers
// below 2^18).
// Arithmetic on floats. dv is rounded once (2^-24 relative, exact when the two values are within a factor of two), dv^2 once more, the
// exponent's fma once: ~3 x 2^-24 on t, |dK| <= K t ln2 x 1.8e-7 <= 7e-8, inside the same 1e-7 per entry. Inputs are finite (the entry
// points check): P <= 1 and never NaN; a dv^2 that overflows gives exp2(-inf) = 0.
// Float colour. Each of the three differences is rounded once, its square once, the two fmas once each; all terms are positive, so
// dist2 carries at most ~5 x 2^-24 and an entry moves by at most K t ln2 x 3e-7 <= 1.1e-7. A sample's three channels do not fit its
// record: they sit in the value block behind the records (Pix<G>::HAS_VALUE_BLOCK, sample_value<G>).
#include "glf_internal.hpp"

#include <cmath>

namespace glf {

// ---- degree -------------------------------------------------------------------------------------------------------------
// A workgroup of 256 consecutive samples (ascending raster order: a band of sample rows) sweeps a chunk of EW_ROWS image rows in
// tiles of EW_ROWS x EW_COLS pixels staged in LDS as the format's {value, col} and read back as wave-wide broadcasts. Chunks beyond
// the f32 underflow radius of the block's sample rows, tiles beyond it from the block's sample columns (not even loaded) and from a
// wave's sample columns hold only entries that are exactly 0 (t > 150) and are not visited. Accumulation: f32 over one tile row,
// f64 across rows, chunks and the final reduction, in a fixed order. *evaluated += the (sample, pixel) entries the waves computed.
constexpr int EW_ROWS = 16, EW_COLS = 64;

template <PixGen G>
__global__ __launch_bounds__(256) void k_degree_entrywise(const uint8_t *__restrict__ img_bytes, int width, int row0, int row1,
                                                           const float4 *__restrict__ samples, unsigned p, float s_loc, float s_val,
                                                           int radius, double *__restrict__ partial, unsigned long long *__restrict__ evaluated)
{
    using P = Pix<G>;
    const typename P::In *img = reinterpret_cast<const typename P::In *>(img_bytes);
    __shared__ typename P::Tile tile[EW_ROWS * EW_COLS];
    __shared__ int wcols[2][4];
    const unsigned b0 = blockIdx.x * 256, i = b0 + threadIdx.x;
    const bool live = i < p;
    const float4 s = samples[live ? i : p - 1];
    const typename P::Val sv = sample_value<G>(samples, round_up_dev(p, NYS_PAD), live ? i : p - 1, s); // (a value block: one more 16-byte load)
    const int r_begin = row0 + (int)blockIdx.y * EW_ROWS, r_end = min(r_begin + EW_ROWS, row1);
    // rows of the block's samples: the first and last sample (ascending indices)
    const int brmin = (int)samples[b0].x, brmax = (int)samples[min(b0 + 255u, p - 1)].x;
    double total = 0.0;
    if (r_end > brmin - radius && r_begin <= brmax + radius) { // workgroup-uniform
        // columns of the wave's samples
        int wcmin = (int)s.y, wcmax = (int)s.y;
        for (int o = 32; o; o >>= 1) {
            wcmin = min(wcmin, __shfl_xor(wcmin, o, 64));
            wcmax = max(wcmax, __shfl_xor(wcmax, o, 64));
        }
        // columns of the block's samples: tiles out of their reach are not loaded at all
        if ((threadIdx.x & 63) == 0) {
            wcols[0][threadIdx.x >> 6] = wcmin;
            wcols[1][threadIdx.x >> 6] = wcmax;
        }
        __syncthreads();
        const int bcmin = min(min(wcols[0][0], wcols[0][1]), min(wcols[0][2], wcols[0][3]));
        const int bcmax = max(max(wcols[1][0], wcols[1][1]), max(wcols[1][2], wcols[1][3]));
        const int live_lanes = __popcll(__ballot(live));
        unsigned long long wave_entries = 0;
        for (int c0 = max(0, bcmin - radius) / EW_COLS * EW_COLS; c0 < width && c0 <= bcmax + radius; c0 += EW_COLS) {
            __syncthreads();
            for (int e = threadIdx.x; e < EW_ROWS * EW_COLS; e += 256) {
                const int rr = e / EW_COLS, cc = e % EW_COLS, r = r_begin + rr, c = c0 + cc;
                typename P::Tile v = P::outside();
                if (r < r_end && c < width) v = P::tile(img, (size_t)r * width + c, c);
                tile[e] = v;
            }
            __syncthreads();
            if (c0 + EW_COLS <= wcmin - radius || c0 > wcmax + radius) continue; // wave-uniform: only exact zeros here
            wave_entries += (unsigned long long)live_lanes * (unsigned long long)((r_end - r_begin) * min(EW_COLS, width - c0));
            for (int rr = 0; rr < r_end - r_begin; ++rr) {
                const float dr = s.x - (float)(r_begin + rr);
                const float qr = dr * dr;
                float acc = 0.f;
                const typename P::Tile *trow = tile + rr * EW_COLS;
#pragma unroll 8
                for (int cc = 0; cc < EW_COLS; ++cc) {
                    const typename P::Tile v = trow[cc];
                    const float dc = s.y - P::tile_col(v);
                    const float u = P::dist2(sv, P::tile_value(v));
                    acc += __builtin_amdgcn_exp2f(-fmaf(u, s_val, fmaf(dc, dc, qr) * s_loc));
                }
                total += (double)acc;
            }
        }
        if ((threadIdx.x & 63) == 0 && wave_entries) atomicAdd(evaluated, wave_entries);
    }
    if (live) partial[(size_t)blockIdx.y * p + i] = total;
}

int degree_rows_entrywise(glf_ctx *ctx, PixGen gen, const uint8_t *d_img, int width, int height, int row0, int row1,
                          const float4 *d_samples, unsigned p, KernelCoef coef, double *d_degree, double *evaluated)
{
    if (gen == PixGen::Grey) return set_error(ctx, GLF_ERR_INVALID, "degree_rows_entrywise: the 8-bit grey format has kernels of its own");
    if (row0 < 0 || row1 > height || row0 > row1) return set_error(ctx, GLF_ERR_INVALID, "bad row range");
    if (evaluated) *evaluated = 0.0;
    if (row0 == row1) {
        GLF_HIP(ctx, hipMemsetAsync(d_degree, 0, sizeof(double) * p, ctx->stream));
        return GLF_OK;
    }
    // t > 150 => exp2(-t) == 0 in f32 (the photometric term only adds to t); s_loc == 0 (never for these kernels): no window
    const int radius = coef.s_loc > 0.f ? (int)std::floor(std::sqrt(151.0 / (double)coef.s_loc)) + 1 : (width + height) * 2;
    const int nchunks = (int)ceil_div(row1 - row0, EW_ROWS);
    if (nchunks > 65535)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "image too tall for one %s degree launch", pix_desc(gen).name);
    DevBuf<double> partial;
    DevBuf<unsigned long long> count;
    GLF_TRY(partial.alloc(ctx, (size_t)nchunks * p));
    GLF_TRY(count.alloc(ctx, 1));
    GLF_HIP(ctx, hipMemsetAsync(count.p, 0, sizeof(unsigned long long), ctx->stream));
    const dim3 grid((unsigned)ceil_div(p, 256), nchunks);
    pix_dispatch_raw(gen, [&](auto t) {
        hipLaunchKernelGGL(k_degree_entrywise<t.G>, grid, dim3(256), 0, ctx->stream, d_img, width, row0, row1, d_samples, p, coef.s_loc,
                           coef.s_val, radius, partial.p, count.p);
    });
    GLF_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_reduce_partials, dim3((p + 255) / 256), dim3(256), 0, ctx->stream, partial.p, p, nchunks, d_degree);
    GLF_LAUNCH_CHECK(ctx);
    unsigned long long h_count = 0;
    GLF_HIP(ctx, hipMemcpyAsync(&h_count, count.p, sizeof(h_count), hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // partial is released at scope exit
    if (evaluated) *evaluated = (double)h_count;
    return GLF_OK;
}

// ---- whole path: the guide's channels as float planes [NCH][N] (c = Phi^T x_k with f64 sums, k_phi_t_signals) -------------
template <PixGen G>
__global__ void k_planes(const uint8_t *__restrict__ img_bytes, int64_t N, float *__restrict__ planes)
{
    using P = Pix<G>;
    const typename P::In *img = reinterpret_cast<const typename P::In *>(img_bytes);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int k = 0; k < P::NCH; ++k) planes[k * N + i] = (float)img[P::NCH * i + k];
}

int pix_planes(glf_ctx *ctx, PixGen gen, const uint8_t *d_img, int64_t N, float *d_planes)
{
    if (gen == PixGen::Grey) return set_error(ctx, GLF_ERR_INVALID, "pix_planes: the 8-bit grey format has kernels of its own");
    const dim3 grid((unsigned)ceil_div(N, 256));
    ctx->flt_note.kernels |= GLF_FK_PLANES;
    pix_dispatch_raw(gen, [&](auto t) { hipLaunchKernelGGL(k_planes<t.G>, grid, dim3(256), 0, ctx->stream, d_img, N, d_planes); });
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// ---- filter ---------------------------------------------------------------------------------------------------------------------
// Channel k of pixel px is x = img[NCH px + k], its correction c = gain * Phi[px] . w_k - ysub * x, the output P::output(x, c)
// (clamped and cast as the grey d_out, at the format's depth) and zf (optional) [NCH][N] = x + c. The dot product and c are formed in
// f64: with the smoothing filters (z = Phi w, no y term) the terms of Phi[px] . w cancel to ~1 % of their size, and an f32 sum
// leaves ~1.5e-5 of relative error in z where f64 leaves the f32 rounding of Phi and w alone.
template <int LD, PixGen G>
__global__ __launch_bounds__(256) void k_apply_filter_pix(const float *__restrict__ phi, int64_t pix0, int64_t pix1, const float *__restrict__ w,
                                                           float gain, float ysub, const uint8_t *__restrict__ img_bytes,
                                                           uint8_t *__restrict__ out_bytes, float *__restrict__ zf, int64_t N)
{
    using P = Pix<G>;
    constexpr int NCH = P::NCH, LPP = LD / 4, PPB = 256 / LPP;
    const typename P::In *img = reinterpret_cast<const typename P::In *>(img_bytes);
    typename P::Out *out = reinterpret_cast<typename P::Out *>(out_bytes);
    const int q = threadIdx.x % LPP, pl = threadIdx.x / LPP;
    float4 wq[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) wq[k] = reinterpret_cast<const float4 *>(w + (size_t)k * LD)[q];
    for (int64_t px = pix0 + (int64_t)blockIdx.x * PPB + pl; px < pix1; px += (int64_t)gridDim.x * PPB) {
        const float4 f = reinterpret_cast<const float4 *>(phi + (size_t)px * LD)[q];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            double s = (double)f.x * wq[k].x + (double)f.y * wq[k].y + (double)f.z * wq[k].z + (double)f.w * wq[k].w;
#pragma unroll
            for (int o = LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (q == 0) {
                const double x = (double)img[NCH * px + k];
                const double c = (double)gain * s - (double)ysub * x;
                if (zf) zf[(size_t)k * N + px] = (float)(x + c);
                out[NCH * px + k] = P::output(x, c);
            }
        }
    }
}

template <PixGen G>
static void launch_apply_filter_pix(unsigned ld, dim3 grid, hipStream_t st, const float *d_phi, int64_t pix0, int64_t pix1, const float *d_w,
                                    float gain, float ysub, const uint8_t *d_img, uint8_t *d_out, float *d_zf, int64_t N)
{
    switch (ld) {
    case 32: hipLaunchKernelGGL((k_apply_filter_pix<32, G>), grid, dim3(256), 0, st, d_phi, pix0, pix1, d_w, gain, ysub, d_img, d_out, d_zf, N); break;
    case 64: hipLaunchKernelGGL((k_apply_filter_pix<64, G>), grid, dim3(256), 0, st, d_phi, pix0, pix1, d_w, gain, ysub, d_img, d_out, d_zf, N); break;
    case 128: hipLaunchKernelGGL((k_apply_filter_pix<128, G>), grid, dim3(256), 0, st, d_phi, pix0, pix1, d_w, gain, ysub, d_img, d_out, d_zf, N); break;
    case 256: hipLaunchKernelGGL((k_apply_filter_pix<256, G>), grid, dim3(256), 0, st, d_phi, pix0, pix1, d_w, gain, ysub, d_img, d_out, d_zf, N); break;
    }
}

int apply_filter_pix(glf_ctx *ctx, PixGen gen, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, const float *d_w, float gain,
                     float ysub, const uint8_t *d_img, uint8_t *d_out, float *d_zf, int64_t N)
{
    if (gen == PixGen::Grey) return set_error(ctx, GLF_ERR_INVALID, "apply_filter_pix: the 8-bit grey format has kernels of its own");
    if (!valid_ld(ld) || pix0 > pix1) return set_error(ctx, GLF_ERR_INVALID, "apply_filter_pix: ld=%u", ld);
    if (pix0 == pix1) return GLF_OK;
    const int ppb = 256 / (ld / 4);
    int64_t nblk = ceil_div(pix1 - pix0, ppb);
    if (nblk > 8192) nblk = 8192; // grid-stride the rest
    const dim3 grid((unsigned)nblk);
    note_apply(ctx, GLF_FK_APPLY_PIX, ld, pix1 - pix0, ppb, nblk);
    pix_dispatch_raw(gen, [&](auto t) { launch_apply_filter_pix<t.G>(ld, grid, ctx->stream, d_phi, pix0, pix1, d_w, gain, ysub, d_img, d_out, d_zf, N); });
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// ---- joint filtering: float planes through the guide's filter (glf_image_processing_rgb_signals / _u16_signals) --------------------
// The filter stage with planes makes the two passes over Phi that it makes without them: one forms c for the guide's channels and
// the planes together, one forms every output. Each channel and each plane is an accumulator chain of its own, in the order it has
// when it runs alone: the guide's results keep the bits of the plain call, a plane's do not depend on the planes beside it.

// part_g[blk][k][j] = sum_{px in blk} Phi[px][j] * x_k[px] for the guide's NCH channels, part_s[blk][k][j] the same for the nsig
// planes: k_phi_t_signals' block partition (1024 pixels), f64 fma chains and LDS order per plane, one read of Phi for all of them.
// The guide's values are read from the image: (double)x is what the plain call's float plane holds.
template <PixGen G>
__global__ __launch_bounds__(256) void k_phi_t_pix_signals(const float *__restrict__ phi, const uint8_t *__restrict__ img_bytes,
                                                            const float *__restrict__ sig, int64_t N, int nsig, int64_t pix0, int64_t pix1,
                                                            unsigned ld, double *__restrict__ part_g, double *__restrict__ part_s)
{
    using P = Pix<G>;
    constexpr int NCH = P::NCH;
    const typename P::In *img = reinterpret_cast<const typename P::In *>(img_bytes);
    __shared__ double sh[NCH + GLF_MAX_SIGNALS][256];
    const int col = threadIdx.x % ld, rl = threadIdx.x / ld, nrl = 256 / ld;
    const int64_t base = pix0 + (int64_t)blockIdx.x * 1024;
    double g[NCH], s[GLF_MAX_SIGNALS];
#pragma unroll
    for (int k = 0; k < NCH; ++k) g[k] = 0.0;
#pragma unroll
    for (int k = 0; k < GLF_MAX_SIGNALS; ++k) s[k] = 0.0;
    for (int64_t r = rl; r < 1024; r += nrl) {
        const int64_t px = base + r;
        if (px >= pix1) break;
        const double f = (double)phi[(size_t)px * ld + col];
#pragma unroll
        for (int k = 0; k < NCH; ++k) g[k] = fma(f, (double)img[NCH * px + k], g[k]);
#pragma unroll
        for (int k = 0; k < GLF_MAX_SIGNALS; ++k)
            if (k < nsig) s[k] = fma(f, (double)sig[(size_t)k * N + px], s[k]);
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) sh[k][threadIdx.x] = g[k];
#pragma unroll
    for (int k = 0; k < GLF_MAX_SIGNALS; ++k) sh[NCH + k][threadIdx.x] = s[k];
    __syncthreads();
    if (threadIdx.x < ld)
        for (int k = 0; k < NCH + nsig; ++k) {
            double t = 0.0;
            for (int r = 0; r < nrl; ++r) t += sh[k][r * ld + col];
            if (k < NCH) part_g[((size_t)blockIdx.x * NCH + k) * ld + col] = t;
            else part_s[((size_t)blockIdx.x * nsig + (k - NCH)) * ld + col] = t;
        }
}

int phi_t_pix_signals(glf_ctx *ctx, PixGen gen, const float *d_phi, const uint8_t *d_img, const float *d_sig, int64_t N, int nsig,
                      int64_t pix0, int64_t pix1, unsigned ld, double *d_c, double *d_cs)
{
    if (gen == PixGen::Grey) return set_error(ctx, GLF_ERR_INVALID, "phi_t_pix_signals: the 8-bit grey format has kernels of its own");
    if (!valid_ld(ld) || pix0 > pix1 || nsig < 1 || nsig > GLF_MAX_SIGNALS)
        return set_error(ctx, GLF_ERR_INVALID, "phi_t_pix_signals: ld=%u nsig=%d", ld, nsig);
    const int nch = pix_desc(gen).channels;
    if (pix0 == pix1) {
        GLF_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof(double) * ld * nch, ctx->stream));
        GLF_HIP(ctx, hipMemsetAsync(d_cs, 0, sizeof(double) * ld * nsig, ctx->stream));
        return GLF_OK;
    }
    const int nblk = (int)ceil_div(pix1 - pix0, 1024);
    DevBuf<double> part_g, part_s;
    GLF_TRY(part_g.alloc(ctx, (size_t)nblk * nch * ld));
    GLF_TRY(part_s.alloc(ctx, (size_t)nblk * nsig * ld));
    ctx->flt_note.kernels |= GLF_FK_PHI_T_PIX_SIGNALS;
    ctx->flt_note.proj_blocks = (unsigned)nblk;
    pix_dispatch_raw(gen, [&](auto t) {
        hipLaunchKernelGGL(k_phi_t_pix_signals<t.G>, dim3(nblk), dim3(256), 0, ctx->stream, d_phi, d_img, d_sig, N, nsig, pix0, pix1, ld, part_g.p,
                           part_s.p);
    });
    GLF_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_cols_sum, dim3(ld * nch), dim3(256), 0, ctx->stream, part_g.p, nblk, ld * nch, d_c);
    hipLaunchKernelGGL(k_cols_sum, dim3(ld * nsig), dim3(256), 0, ctx->stream, part_s.p, nblk, ld * nsig, d_cs);
    GLF_LAUNCH_CHECK(ctx);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the partials are released at scope exit
    return GLF_OK;
}

// Each Phi row loaded once for the guide's channels and the planes. The channels: k_apply_filter_pix's arithmetic, statement for
// statement. Plane k of pixel px: out = (float)(s + (gain * Phi[px] . w_k - ysub * s)) in f64 (the dot product for the reason given
// above k_apply_filter_pix), not clamped. w [NCH + nsig][LD], the channels' weights first.
template <int LD, PixGen G>
__global__ __launch_bounds__(256) void k_apply_filter_pix_signals(const float *__restrict__ phi, int64_t pix0, int64_t pix1, int nsig,
                                                                   const float *__restrict__ w, float gain, float ysub,
                                                                   const uint8_t *__restrict__ img_bytes, uint8_t *__restrict__ out_bytes,
                                                                   float *__restrict__ zf, const float *__restrict__ sig,
                                                                   float *__restrict__ sig_out, int64_t N)
{
    using P = Pix<G>;
    constexpr int NCH = P::NCH, LPP = LD / 4, PPB = 256 / LPP;
    const typename P::In *img = reinterpret_cast<const typename P::In *>(img_bytes);
    typename P::Out *out = reinterpret_cast<typename P::Out *>(out_bytes);
    const int q = threadIdx.x % LPP, pl = threadIdx.x / LPP;
    float4 wq[NCH], ws[GLF_MAX_SIGNALS];
#pragma unroll
    for (int k = 0; k < NCH; ++k) wq[k] = reinterpret_cast<const float4 *>(w + (size_t)k * LD)[q];
#pragma unroll
    for (int k = 0; k < GLF_MAX_SIGNALS; ++k)
        ws[k] = k < nsig ? reinterpret_cast<const float4 *>(w + (size_t)(NCH + k) * LD)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t px = pix0 + (int64_t)blockIdx.x * PPB + pl; px < pix1; px += (int64_t)gridDim.x * PPB) {
        const float4 f = reinterpret_cast<const float4 *>(phi + (size_t)px * LD)[q];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            double s = (double)f.x * wq[k].x + (double)f.y * wq[k].y + (double)f.z * wq[k].z + (double)f.w * wq[k].w;
#pragma unroll
            for (int o = LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (q == 0) {
                const double x = (double)img[NCH * px + k];
                const double c = (double)gain * s - (double)ysub * x;
                if (zf) zf[(size_t)k * N + px] = (float)(x + c);
                out[NCH * px + k] = P::output(x, c);
            }
        }
#pragma unroll
        for (int k = 0; k < GLF_MAX_SIGNALS; ++k) {
            if (k >= nsig) break;
            double s = (double)f.x * ws[k].x + (double)f.y * ws[k].y + (double)f.z * ws[k].z + (double)f.w * ws[k].w;
#pragma unroll
            for (int o = LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (q == 0) {
                const double v = (double)sig[(size_t)k * N + px];
                sig_out[(size_t)k * N + px] = (float)(v + ((double)gain * s - (double)ysub * v));
            }
        }
    }
}

template <PixGen G>
static void launch_apply_filter_pix_signals(unsigned ld, dim3 grid, hipStream_t st, const float *d_phi, int64_t pix0, int64_t pix1, int nsig,
                                            const float *d_w, float gain, float ysub, const uint8_t *d_img, uint8_t *d_out, float *d_zf,
                                            const float *d_sig, float *d_sig_out, int64_t N)
{
    switch (ld) {
    case 32: hipLaunchKernelGGL((k_apply_filter_pix_signals<32, G>), grid, dim3(256), 0, st, d_phi, pix0, pix1, nsig, d_w, gain, ysub, d_img, d_out, d_zf, d_sig, d_sig_out, N); break;
    case 64: hipLaunchKernelGGL((k_apply_filter_pix_signals<64, G>), grid, dim3(256), 0, st, d_phi, pix0, pix1, nsig, d_w, gain, ysub, d_img, d_out, d_zf, d_sig, d_sig_out, N); break;
    case 128: hipLaunchKernelGGL((k_apply_filter_pix_signals<128, G>), grid, dim3(256), 0, st, d_phi, pix0, pix1, nsig, d_w, gain, ysub, d_img, d_out, d_zf, d_sig, d_sig_out, N); break;
    case 256: hipLaunchKernelGGL((k_apply_filter_pix_signals<256, G>), grid, dim3(256), 0, st, d_phi, pix0, pix1, nsig, d_w, gain, ysub, d_img, d_out, d_zf, d_sig, d_sig_out, N); break;
    }
}

int apply_filter_pix_signals(glf_ctx *ctx, PixGen gen, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, int nsig, const float *d_w,
                             float gain, float ysub, const uint8_t *d_img, uint8_t *d_out, float *d_zf, const float *d_sig, float *d_sig_out,
                             int64_t N)
{
    if (gen == PixGen::Grey) return set_error(ctx, GLF_ERR_INVALID, "apply_filter_pix_signals: the 8-bit grey format has kernels of its own");
    if (!valid_ld(ld) || pix0 > pix1 || nsig < 1 || nsig > GLF_MAX_SIGNALS)
        return set_error(ctx, GLF_ERR_INVALID, "apply_filter_pix_signals: ld=%u nsig=%d", ld, nsig);
    if (pix0 == pix1) return GLF_OK;
    const int ppb = 256 / (ld / 4);
    int64_t nblk = ceil_div(pix1 - pix0, ppb);
    if (nblk > 8192) nblk = 8192; // grid-stride the rest
    const dim3 grid((unsigned)nblk);
    note_apply(ctx, GLF_FK_APPLY_PIX_SIGNALS, ld, pix1 - pix0, ppb, nblk);
    pix_dispatch_raw(gen, [&](auto t) {
        launch_apply_filter_pix_signals<t.G>(ld, grid, ctx->stream, d_phi, pix0, pix1, nsig, d_w, gain, ysub, d_img, d_out, d_zf, d_sig, d_sig_out, N);
    });
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// ---- the float formats' admission check (float colour: N = its 3 x pixels floats) -------------------------------------------------------------------------------------
// *bad |= 1 where a value is NaN or Inf: exponent bits all ones. Grid-strided, one flag write per wave that saw one.
__global__ __launch_bounds__(256) void k_f32_nonfinite(const float *__restrict__ img, int64_t N, unsigned *__restrict__ bad)
{
    bool seen = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
        seen |= (__float_as_uint(img[i]) & 0x7f800000u) == 0x7f800000u;
    if (__ballot(seen) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

int f32_all_finite(glf_ctx *ctx, const float *d_img, int64_t N, bool *finite)
{
    DevBuf<unsigned> bad;
    GLF_TRY(bad.alloc(ctx, 1));
    GLF_HIP(ctx, hipMemsetAsync(bad.p, 0, sizeof(unsigned), ctx->stream));
    int64_t nblk = ceil_div(N, 256);
    if (nblk > 4096) nblk = 4096;
    hipLaunchKernelGGL(k_f32_nonfinite, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, d_img, N, bad.p);
    GLF_LAUNCH_CHECK(ctx);
    unsigned h_bad = 0;
    GLF_HIP(ctx, hipMemcpyAsync(&h_bad, bad.p, sizeof(h_bad), hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *finite = h_bad == 0;
    return GLF_OK;
}

} // namespace glf
