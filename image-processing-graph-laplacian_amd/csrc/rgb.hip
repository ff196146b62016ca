// rgb.hip -- the colour bilateral affinity (glf_options.kernel = GLF_KERNEL_BILATERAL_RGB) behind the same stage API as the
// grey kernels:
//
//   K(i, j) = Es(dr) Es(dc) P(dR) P(dG) P(dB) = exp2(-(s_loc (dr^2 + dc^2) + s_val (dR^2 + dG^2 + dB^2)))
//
// with the image read as interleaved uint8 [height][width][3]. The colour factor is at most 1, so every spatial bound of
// the grey kernels (the f32 underflow radius, the chunk boxes of the Nystroem window) holds unchanged. A colour guide has
// 2^24 values, so the forms that factor the sums over the 256 grey levels (grid, rank, band) do not extend: those routes
// decline the kernel and the entry-by-entry kernels run --
//   k_degree_rgb       D[i] = sum over the rank's pixel rows of K(sample i, pixel)   lane = sample, pixel tiles in LDS
//   k_sample_matrix_rgb K_A / L_A                                                      lane = column sample
//   k_nystroem<.., RGB> (nystroem.hip) Phi = K_B^T Psi, f32 MFMA with the colour generator
// A sample record is {row, col, 0, R + 256 G + 65536 B} (the packed colour as an exact integer in f32).
#include "glf_internal.hpp"

#include <cmath>
#include <vector>

namespace glf {

__device__ __forceinline__ float rgb_dist2(unsigned a, float r, float g, float b)
{
    const float dr = ubyte_f32(a, 0) - r, dg = ubyte_f32(a, 1) - g,
                db = ubyte_f32(a, 2) - b;
    return fmaf(db, db, fmaf(dg, dg, dr * dr)); // exact: integers below 2^18
}

// ---- degree -------------------------------------------------------------------------------------------------------------
// A workgroup of 256 consecutive samples (ascending raster order: a band of sample rows) sweeps a chunk of RGB_ROWS image rows in
// tiles of RGB_ROWS x RGB_COLS pixels staged in LDS as {R, G, B, col} and read back as wave-wide broadcasts. Chunks beyond the
// f32 underflow radius of the block's sample rows, tiles beyond it from the block's sample columns (not even loaded) and from a
// wave's sample columns hold only entries that are exactly 0 (t > 150) and are not visited. Accumulation: f32 over one tile row,
// f64 across rows, chunks and the final reduction, in a fixed order. *evaluated += the (sample, pixel) entries the waves computed.
constexpr int RGB_ROWS = 16, RGB_COLS = 64;

__global__ __launch_bounds__(256) void k_degree_rgb(const uint8_t *__restrict__ img, int width, int row0, int row1,
                                                     const float4 *__restrict__ samples, unsigned p, float s_loc, float s_val, int radius,
                                                     double *__restrict__ partial, unsigned long long *__restrict__ evaluated)
{
    __shared__ float4 tile[RGB_ROWS * RGB_COLS];
    __shared__ int wcols[2][4];
    const unsigned b0 = blockIdx.x * 256, i = b0 + threadIdx.x;
    const bool live = i < p;
    const float4 s = samples[live ? i : p - 1];
    const unsigned sc = (unsigned)s.w;
    const float sr = ubyte_f32(sc, 0), sg = ubyte_f32(sc, 1), sb = ubyte_f32(sc, 2);
    const int r_begin = row0 + (int)blockIdx.y * RGB_ROWS, r_end = min(r_begin + RGB_ROWS, row1);
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
        for (int c0 = max(0, bcmin - radius) / RGB_COLS * RGB_COLS; c0 < width && c0 <= bcmax + radius; c0 += RGB_COLS) {
            __syncthreads();
            for (int e = threadIdx.x; e < RGB_ROWS * RGB_COLS; e += 256) {
                const int rr = e / RGB_COLS, cc = e % RGB_COLS, r = r_begin + rr, c = c0 + cc;
                float4 v = make_float4(0.f, 0.f, 0.f, -1e30f); // outside the chunk: a column no sample reaches (K = 0)
                if (r < r_end && c < width) {
                    const uint8_t *q = img + ((size_t)r * width + c) * 3;
                    v = make_float4((float)q[0], (float)q[1], (float)q[2], (float)c);
                }
                tile[e] = v;
            }
            __syncthreads();
            if (c0 + RGB_COLS <= wcmin - radius || c0 > wcmax + radius) continue; // wave-uniform: only exact zeros here
            wave_entries += (unsigned long long)live_lanes * (unsigned long long)((r_end - r_begin) * min(RGB_COLS, width - c0));
            for (int rr = 0; rr < r_end - r_begin; ++rr) {
                const float dr = s.x - (float)(r_begin + rr);
                const float qr = dr * dr;
                float acc = 0.f;
                const float4 *trow = tile + rr * RGB_COLS;
#pragma unroll 8
                for (int cc = 0; cc < RGB_COLS; ++cc) {
                    const float4 v = trow[cc];
                    const float dc = s.y - v.w, d0 = sr - v.x, d1 = sg - v.y, d2 = sb - v.z;
                    const float u = fmaf(d2, d2, fmaf(d1, d1, d0 * d0));
                    const float q = fmaf(dc, dc, qr);
                    acc += __builtin_amdgcn_exp2f(-fmaf(u, s_val, q * s_loc));
                }
                total += (double)acc;
            }
        }
        if ((threadIdx.x & 63) == 0 && wave_entries) atomicAdd(evaluated, wave_entries);
    }
    if (live) partial[(size_t)blockIdx.y * p + i] = total;
}

__global__ void k_rgb_reduce(const double *__restrict__ partial, unsigned p, int nchunks, double *__restrict__ out)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p) return;
    double s = 0.0;
    for (int k = 0; k < nchunks; ++k) s += partial[(size_t)k * p + i];
    out[i] = s;
}

int rgb_degree_rows(glf_ctx *ctx, const uint8_t *d_rgb, int width, int height, int row0, int row1, const float4 *d_samples, unsigned p,
                    KernelCoef coef, double *d_degree, double *evaluated)
{
    if (row0 < 0 || row1 > height || row0 > row1) return set_error(ctx, GLF_ERR_INVALID, "bad row range");
    if (evaluated) *evaluated = 0.0;
    if (row0 == row1) {
        GLF_HIP(ctx, hipMemsetAsync(d_degree, 0, sizeof(double) * p, ctx->stream));
        return GLF_OK;
    }
    // t > 150 => exp2(-t) == 0 in f32 (the colour term only adds to t); s_loc == 0 (never for this kernel): no window
    const int radius = coef.s_loc > 0.f ? (int)std::floor(std::sqrt(151.0 / (double)coef.s_loc)) + 1 : (width + height) * 2;
    const int nchunks = (int)ceil_div(row1 - row0, RGB_ROWS);
    if (nchunks > 65535) return set_error(ctx, GLF_ERR_UNSUPPORTED, "image too tall for one colour degree launch");
    DevBuf<double> partial;
    DevBuf<unsigned long long> count;
    GLF_TRY(partial.alloc(ctx, (size_t)nchunks * p));
    GLF_TRY(count.alloc(ctx, 1));
    GLF_HIP(ctx, hipMemsetAsync(count.p, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_degree_rgb, dim3((unsigned)ceil_div(p, 256), nchunks), dim3(256), 0, ctx->stream, d_rgb, width, row0, row1,
                       d_samples, p, coef.s_loc, coef.s_val, radius, partial.p, count.p);
    GLF_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_rgb_reduce, dim3((p + 255) / 256), dim3(256), 0, ctx->stream, partial.p, p, nchunks, d_degree);
    GLF_LAUNCH_CHECK(ctx);
    unsigned long long h_count = 0;
    GLF_HIP(ctx, hipMemcpyAsync(&h_count, count.p, sizeof(h_count), hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // partial is released at scope exit
    if (evaluated) *evaluated = (double)h_count;
    return GLF_OK;
}

// ---- K_A / L_A ------------------------------------------------------------------------------------------------------------------
// k_sample_matrix (affinity.hip) with the colour generator: out[i][jl] = K(sample i, sample col0 + jl), or the Laplacian form
// alpha (D_i delta_ij - K); padding columns up to ld are zeroed.
__global__ __launch_bounds__(256) void k_sample_matrix_rgb(const float4 *__restrict__ samples, unsigned p, float s_loc, float s_val,
                                                            float *__restrict__ out, int64_t ld, int laplacian, double alpha,
                                                            const double *__restrict__ degree, unsigned col0, unsigned ncols)
{
    const unsigned jl = blockIdx.x * 64 + (threadIdx.x & 63);
    const unsigned i0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 16;
    if (jl >= (unsigned)ld) return;
    if (jl >= ncols) {
        for (unsigned ii = 0; ii < 16 && i0 + ii < p; ++ii) out[(size_t)(i0 + ii) * ld + jl] = 0.f;
        return;
    }
    const unsigned j = col0 + jl;
    const float4 sj = samples[j];
    const unsigned cj = (unsigned)sj.w;
    const float rj = ubyte_f32(cj, 0), gj = ubyte_f32(cj, 1), bj = ubyte_f32(cj, 2);
    const float fscale = laplacian ? (float)(-alpha) : 1.0f;
    for (unsigned ii = 0; ii < 16; ++ii) {
        const unsigned i = i0 + ii;
        if (i >= p) break;
        const float4 si = samples[i];
        const float dr = si.x - sj.x, dc = si.y - sj.y;
        const float u = rgb_dist2((unsigned)si.w, rj, gj, bj);
        const float k = __builtin_amdgcn_exp2f(-fmaf(u, s_val, fmaf(dc, dc, dr * dr) * s_loc));
        float v = fscale * k;
        if (laplacian && i == j) v = (float)(alpha * (degree[i] - (double)k));
        out[(size_t)i * ld + jl] = v;
    }
}

int rgb_sample_matrix(glf_ctx *ctx, const float4 *d_samples, unsigned p, KernelCoef coef, float *d_out, int64_t ld, bool laplacian,
                      double alpha, const double *d_degree, unsigned col0, unsigned ncols)
{
    if (ncols == 0) {
        col0 = 0;
        ncols = p;
    }
    if (col0 + ncols > p) return set_error(ctx, GLF_ERR_INVALID, "rgb_sample_matrix: column range");
    hipLaunchKernelGGL(k_sample_matrix_rgb, dim3((unsigned)ceil_div(ld, 64), (p + 63) / 64), dim3(256), 0, ctx->stream, d_samples, p,
                       coef.s_loc, coef.s_val, d_out, ld, laplacian ? 1 : 0, alpha, d_degree, col0, ncols);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// ---- whole path: the channel planes of an interleaved RGB image (for Phi^T x_c) ---------------------------------------------------------------------
__global__ void k_rgb_planes(const uint8_t *__restrict__ rgb, int64_t N, float *__restrict__ planes)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    planes[i] = (float)rgb[3 * i];
    planes[N + i] = (float)rgb[3 * i + 1];
    planes[2 * N + i] = (float)rgb[3 * i + 2];
}

int rgb_planes(glf_ctx *ctx, const uint8_t *d_rgb, int64_t N, float *d_planes)
{
    hipLaunchKernelGGL(k_rgb_planes, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, d_rgb, N, d_planes);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

} // namespace glf
