// u16.hip -- the bilateral affinity on 16-bit grey values (glf_options.kernel = GLF_KERNEL_BILATERAL_U16) behind the same stage
// API as the 8-bit kernels:
//
//   K(i, j) = Es(dr) Es(dc) P(dv) = exp2(-(s_loc (dr^2 + dc^2) + s_val (v_i - v_j)^2)),   v in 0..65535
//
// with the image read as uint16_t [height][width]. The photometric factor is at most 1, so every spatial bound of the grey kernels
// (the f32 underflow radius, the chunk boxes of the Nystroem window) holds unchanged. A 16-bit guide has 65 536 values, so the
// forms that factor the sums over the 256 grey levels (grid, rank, band) and the grey direct degree (a 256-entry table per sample)
// do not extend: those routes decline the kernel and the entry-by-entry kernels run --
//   k_degree_u16                       D[i] = sum over the rank's pixel rows of K(sample i, pixel)   lane = sample, pixel tiles in LDS
//   k_sample_matrix (affinity.hip)     K_A / L_A from the sample records alone: unchanged (no table, kernel_eval on record values)
//   k_nystroem<.., PixGen::U16>        Phi = K_B^T Psi, f32 MFMA with the 16-bit pixel read (nystroem.hip)
//   k_apply_filter_u16                 the 16-bit output and z, dot products in f64
// A sample record is the grey one, {row, col, value, 0}: a 16-bit value is exact in f32.
//
// Arithmetic. dv = v_i - v_j is exact in f32 (|dv| < 2^16), dv^2 is not (up to 32 bits): it is rounded once (relative error
// <= 2^-24), and so is the exponent t = s_val dv^2 + s_loc q (q = dr^2 + dc^2 exact) in its fma, so t carries a relative error
// of at most ~2^-23 -- the same order as the f32 rounding of s_val itself, which the 8-bit kernels have too. exp2(-t) then
// moves by |dK| <= K t ln2 2^-23 <= (1/e) 2^-23 ~ 4.4e-8 absolute (the maximum of x e^-x at x = 1), and v_exp_f32 adds its own
// ~1 ulp: every entry of K_A and K_B is within ~1e-7 of the fp64 kernel, well inside 1e-6 of max|K| = 1.
#include "glf_internal.hpp"

#include <cmath>
#include <vector>

namespace glf {

// ---- degree -------------------------------------------------------------------------------------------------------------
// k_degree_rgb's structure with a 16-bit grey pixel: a workgroup of 256 consecutive samples (ascending raster order: a band of
// sample rows) sweeps a chunk of U16_ROWS image rows in tiles of U16_ROWS x U16_COLS pixels staged in LDS as {value, col} and read
// back as wave-wide broadcasts. Chunks beyond the f32 underflow radius of the block's sample rows, tiles beyond it from the
// block's sample columns (not even loaded) and from a wave's sample columns hold only entries that are exactly 0 (t > 150) and
// are not visited. Accumulation: f32 over one tile row, f64 across rows, chunks and the final reduction, in a fixed order.
// *evaluated += the (sample, pixel) entries the waves computed.
constexpr int U16_ROWS = 16, U16_COLS = 64;

__global__ __launch_bounds__(256) void k_degree_u16(const uint16_t *__restrict__ img, int width, int row0, int row1,
                                                     const float4 *__restrict__ samples, unsigned p, float s_loc, float s_val, int radius,
                                                     double *__restrict__ partial, unsigned long long *__restrict__ evaluated)
{
    __shared__ float2 tile[U16_ROWS * U16_COLS];
    __shared__ int wcols[2][4];
    const unsigned b0 = blockIdx.x * 256, i = b0 + threadIdx.x;
    const bool live = i < p;
    const float4 s = samples[live ? i : p - 1];
    const int r_begin = row0 + (int)blockIdx.y * U16_ROWS, r_end = min(r_begin + U16_ROWS, row1);
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
        for (int c0 = max(0, bcmin - radius) / U16_COLS * U16_COLS; c0 < width && c0 <= bcmax + radius; c0 += U16_COLS) {
            __syncthreads();
            for (int e = threadIdx.x; e < U16_ROWS * U16_COLS; e += 256) {
                const int rr = e / U16_COLS, cc = e % U16_COLS, r = r_begin + rr, c = c0 + cc;
                float2 v = make_float2(0.f, -1e30f); // outside the chunk: a column no sample reaches (K = 0)
                if (r < r_end && c < width) v = make_float2((float)img[(size_t)r * width + c], (float)c);
                tile[e] = v;
            }
            __syncthreads();
            if (c0 + U16_COLS <= wcmin - radius || c0 > wcmax + radius) continue; // wave-uniform: only exact zeros here
            wave_entries += (unsigned long long)live_lanes * (unsigned long long)((r_end - r_begin) * min(U16_COLS, width - c0));
            for (int rr = 0; rr < r_end - r_begin; ++rr) {
                const float dr = s.x - (float)(r_begin + rr);
                const float qr = dr * dr;
                float acc = 0.f;
                const float2 *trow = tile + rr * U16_COLS;
#pragma unroll 8
                for (int cc = 0; cc < U16_COLS; ++cc) {
                    const float2 v = trow[cc];
                    const float dc = s.y - v.y, dv = s.z - v.x;
                    acc += __builtin_amdgcn_exp2f(-fmaf(dv * dv, s_val, fmaf(dc, dc, qr) * s_loc)); // kernel_eval's rounding
                }
                total += (double)acc;
            }
        }
        if ((threadIdx.x & 63) == 0 && wave_entries) atomicAdd(evaluated, wave_entries);
    }
    if (live) partial[(size_t)blockIdx.y * p + i] = total;
}

__global__ void k_u16_reduce(const double *__restrict__ partial, unsigned p, int nchunks, double *__restrict__ out)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p) return;
    double s = 0.0;
    for (int k = 0; k < nchunks; ++k) s += partial[(size_t)k * p + i];
    out[i] = s;
}

int u16_degree_rows(glf_ctx *ctx, const uint16_t *d_img, int width, int height, int row0, int row1, const float4 *d_samples, unsigned p,
                    KernelCoef coef, double *d_degree, double *evaluated)
{
    if (row0 < 0 || row1 > height || row0 > row1) return set_error(ctx, GLF_ERR_INVALID, "bad row range");
    if (evaluated) *evaluated = 0.0;
    if (row0 == row1) {
        GLF_HIP(ctx, hipMemsetAsync(d_degree, 0, sizeof(double) * p, ctx->stream));
        return GLF_OK;
    }
    // t > 150 => exp2(-t) == 0 in f32 (the photometric term only adds to t); s_loc == 0 (never for this kernel): no window
    const int radius = coef.s_loc > 0.f ? (int)std::floor(std::sqrt(151.0 / (double)coef.s_loc)) + 1 : (width + height) * 2;
    const int nchunks = (int)ceil_div(row1 - row0, U16_ROWS);
    if (nchunks > 65535) return set_error(ctx, GLF_ERR_UNSUPPORTED, "image too tall for one 16-bit degree launch");
    DevBuf<double> partial;
    DevBuf<unsigned long long> count;
    GLF_TRY(partial.alloc(ctx, (size_t)nchunks * p));
    GLF_TRY(count.alloc(ctx, 1));
    GLF_HIP(ctx, hipMemsetAsync(count.p, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_degree_u16, dim3((unsigned)ceil_div(p, 256), nchunks), dim3(256), 0, ctx->stream, d_img, width, row0, row1,
                       d_samples, p, coef.s_loc, coef.s_val, radius, partial.p, count.p);
    GLF_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_u16_reduce, dim3((p + 255) / 256), dim3(256), 0, ctx->stream, partial.p, p, nchunks, d_degree);
    GLF_LAUNCH_CHECK(ctx);
    unsigned long long h_count = 0;
    GLF_HIP(ctx, hipMemcpyAsync(&h_count, count.p, sizeof(h_count), hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // partial is released at scope exit
    if (evaluated) *evaluated = (double)h_count;
    return GLF_OK;
}

// ---- whole path: the image as one float plane (for c = Phi^T y with f64 sums, k_phi_t_signals) -------------------------------
__global__ void k_u16_plane(const uint16_t *__restrict__ img, int64_t N, float *__restrict__ plane)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) plane[i] = (float)img[i];
}

int u16_plane(glf_ctx *ctx, const uint16_t *d_img, int64_t N, float *d_plane)
{
    hipLaunchKernelGGL(k_u16_plane, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, d_img, N, d_plane);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// ---- filter ---------------------------------------------------------------------------------------------------------------------
// The grey d_out rule at 16 bits: clamp(x + floor(c), 0, 65535), NaN -> 0.
__device__ __forceinline__ uint16_t filter_output_u16(int x, double c)
{
    const double fc = floor(fmin(fmax(c, -1.0e6), 1.0e6));
    int zi = x + (int)fc;
    zi = zi > 65535 ? 65535 : zi;
    zi = (zi < 0 || !(c == c)) ? 0 : zi;
    return (uint16_t)zi;
}

// out[px] for pixel x = img[px]: its correction c = gain * Phi[px] . w - ysub * x and filter_output_u16(x, c); zf (optional) = x + c.
// The dot product and c are formed in f64 (as k_apply_filter_rgb: the smoothing filters' terms cancel to ~1 % of their size).
template <int LD>
__global__ __launch_bounds__(256) void k_apply_filter_u16(const float *__restrict__ phi, int64_t pix0, int64_t pix1, const float *__restrict__ w,
                                                           float gain, float ysub, const uint16_t *__restrict__ img, uint16_t *__restrict__ out,
                                                           float *__restrict__ zf)
{
    constexpr int LPP = LD / 4, PPB = 256 / LPP;
    const int q = threadIdx.x % LPP, pl = threadIdx.x / LPP;
    const float4 wq = reinterpret_cast<const float4 *>(w)[q];
    for (int64_t px = pix0 + (int64_t)blockIdx.x * PPB + pl; px < pix1; px += (int64_t)gridDim.x * PPB) {
        const float4 f = reinterpret_cast<const float4 *>(phi + (size_t)px * LD)[q];
        double s = (double)f.x * wq.x + (double)f.y * wq.y + (double)f.z * wq.z + (double)f.w * wq.w;
#pragma unroll
        for (int o = LPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (q == 0) {
            const int x = (int)img[px];
            const double c = (double)gain * s - (double)ysub * (double)x;
            if (zf) zf[px] = (float)((double)x + c);
            out[px] = filter_output_u16(x, c);
        }
    }
}

int apply_filter_u16(glf_ctx *ctx, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, const float *d_w, float gain, float ysub,
                     const uint16_t *d_img, uint16_t *d_out, float *d_zf)
{
    if (!valid_ld(ld) || pix0 > pix1) return set_error(ctx, GLF_ERR_INVALID, "apply_filter_u16: ld=%u", ld);
    if (pix0 == pix1) return GLF_OK;
    const int ppb = 256 / (ld / 4);
    int64_t nblk = ceil_div(pix1 - pix0, ppb);
    if (nblk > 8192) nblk = 8192; // grid-stride the rest
    dim3 grid((unsigned)nblk), block(256);
    switch (ld) {
    case 32: hipLaunchKernelGGL(k_apply_filter_u16<32>, grid, block, 0, ctx->stream, d_phi, pix0, pix1, d_w, gain, ysub, d_img, d_out, d_zf); break;
    case 64: hipLaunchKernelGGL(k_apply_filter_u16<64>, grid, block, 0, ctx->stream, d_phi, pix0, pix1, d_w, gain, ysub, d_img, d_out, d_zf); break;
    case 128: hipLaunchKernelGGL(k_apply_filter_u16<128>, grid, block, 0, ctx->stream, d_phi, pix0, pix1, d_w, gain, ysub, d_img, d_out, d_zf); break;
    case 256: hipLaunchKernelGGL(k_apply_filter_u16<256>, grid, block, 0, ctx->stream, d_phi, pix0, pix1, d_w, gain, ysub, d_img, d_out, d_zf); break;
    }
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

} // namespace glf
