// graph_compact.hip -- the compact graph handle (glf_graph_compact, glf_graph_storage, glf_graph_dequantize): Phi rewritten as
// __half [N][ld] with one power-of-two scale per column. Two pure streams do the compaction, the column maxima (k_phi_col_max) and
// the conversion (k_phi_to_half); the exponent rule between them is host code (compact_exponent, host_util.cpp). The six passes
// over a compact Phi are the f16 instances of the handle's own kernels (phi_tile.hpp: the second loader), the scales stay on the host.
#include "phi_tile.hpp"
#include "phi_compact.hpp"

#include <algorithm>
#include <cmath>

namespace glf {

// colmax[c] = max over the pixels of the bits of |Phi[px][c]| (colmax zeroed by the caller). The bit patterns of non-negative floats
// order as the values do, with +Inf and every NaN above all finite values: one unsigned maximum is the exact maximum of the
// magnitudes (what fmaxf gives on finite data, in any order) and the finiteness flag at once. A lane takes whole float4s at a
// grid stride that is a multiple of ld / 4, so it stays in its four columns; the workgroup's lanes of one column group meet in LDS
// and one lane per column issues the atomic maximum (a maximum: no order to fix).
__global__ __launch_bounds__(256) void k_phi_col_max(const float *__restrict__ phi, int64_t n4, int ld, unsigned *__restrict__ colmax)
{
    __shared__ uint4 sh[256];
    const int64_t stride = (int64_t)gridDim.x * 256;
    uint4 mx = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const uint4 x = reinterpret_cast<const uint4 *>(phi)[i];
        mx.x = max(mx.x, x.x & 0x7fffffffu);
        mx.y = max(mx.y, x.y & 0x7fffffffu);
        mx.z = max(mx.z, x.z & 0x7fffffffu);
        mx.w = max(mx.w, x.w & 0x7fffffffu);
    }
    sh[threadIdx.x] = mx;
    __syncthreads();
    const int groups = ld / 4; // column groups: lane t holds group t % groups (256 and the stride are multiples of it)
    if ((int)threadIdx.x < groups) {
        for (int t = threadIdx.x + groups; t < 256; t += groups) {
            mx.x = max(mx.x, sh[t].x);
            mx.y = max(mx.y, sh[t].y);
            mx.z = max(mx.z, sh[t].z);
            mx.w = max(mx.w, sh[t].w);
        }
        atomicMax(colmax + threadIdx.x * 4 + 0, mx.x);
        atomicMax(colmax + threadIdx.x * 4 + 1, mx.y);
        atomicMax(colmax + threadIdx.x * 4 + 2, mx.z);
        atomicMax(colmax + threadIdx.x * 4 + 3, mx.w);
    }
}

// out[px][c] = f16_rn(phi[px][c] mult[c]), mult[c] = 2^-e_c: a lane takes 8 consecutive columns of a row, two 16-byte loads and one
// 16-byte store; the product is exact (a power of two, no over- or underflow that the half would not round to the same value), the
// conversion is v_cvt_f16_f32, round to nearest even, subnormal results kept.
__global__ __launch_bounds__(256) void k_phi_to_half(const float *__restrict__ phi, int64_t n8, int ld, const float *__restrict__ mult,
                                                     __half *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int groups = ld / 8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const int c8 = (int)(i % groups);
        const float4 a = reinterpret_cast<const float4 *>(phi)[2 * i], b = reinterpret_cast<const float4 *>(phi)[2 * i + 1];
        const float4 ma = reinterpret_cast<const float4 *>(mult)[2 * c8], mb = reinterpret_cast<const float4 *>(mult)[2 * c8 + 1];
        f16x8 h;
        h[0] = (_Float16)(a.x * ma.x);
        h[1] = (_Float16)(a.y * ma.y);
        h[2] = (_Float16)(a.z * ma.z);
        h[3] = (_Float16)(a.w * ma.w);
        h[4] = (_Float16)(b.x * mb.x);
        h[5] = (_Float16)(b.y * mb.y);
        h[6] = (_Float16)(b.z * mb.z);
        h[7] = (_Float16)(b.w * mb.w);
        reinterpret_cast<uint4 *>(out)[i] = __builtin_bit_cast(uint4, h);
    }
}

// out[px][c] = 2^e_c half[px][c] (exact: ldexpf of a value of 11 significant bits, f32 subnormals kept)
__global__ __launch_bounds__(256) void k_phi_from_half(const __half *__restrict__ phi, int64_t n8, int ld, const int *__restrict__ expo,
                                                       float *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int groups = ld / 8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const int c = (int)(i % groups) * 8;
        const f16x8 h = __builtin_bit_cast(f16x8, reinterpret_cast<const uint4 *>(phi)[i]);
        reinterpret_cast<float4 *>(out)[2 * i] =
            make_float4(ldexpf((float)h[0], expo[c + 0]), ldexpf((float)h[1], expo[c + 1]), ldexpf((float)h[2], expo[c + 2]), ldexpf((float)h[3], expo[c + 3]));
        reinterpret_cast<float4 *>(out)[2 * i + 1] =
            make_float4(ldexpf((float)h[4], expo[c + 4]), ldexpf((float)h[5], expo[c + 5]), ldexpf((float)h[6], expo[c + 6]), ldexpf((float)h[7], expo[c + 7]));
    }
}

// workgroups of a stream over `items` lane items: enough to fill the device several times over, the rest by the grid stride
static unsigned stream_grid(const glf_ctx *ctx, int64_t items)
{
    const int64_t cus = ctx->prop.multiProcessorCount > 1 ? ctx->prop.multiProcessorCount : 1;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(items, 256), cus * 16));
}

static int graph_compact_f16(glf_graph *g)
{
    glf_ctx *ctx = g->ctx;
    const unsigned m = g->m, ld = g->ld;
    const int64_t N = (int64_t)g->width * g->height, cnt = N * ld;
    DevBuf<unsigned> colmax;
    GLF_TRY(colmax.alloc(ctx, ld));
    GLF_HIP(ctx, hipMemsetAsync(colmax.p, 0, sizeof(unsigned) * ld, ctx->stream));
    hipLaunchKernelGGL(k_phi_col_max, dim3(stream_grid(ctx, cnt / 4)), dim3(256), 0, ctx->stream, g->phi, cnt / 4, (int)ld, colmax.p);
    GLF_LAUNCH_CHECK(ctx);
    std::vector<unsigned> h_max(ld);
    GLF_HIP(ctx, hipMemcpyAsync(h_max.data(), colmax.p, sizeof(unsigned) * ld, hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> expo(ld, 0);
    std::vector<float> h_mult(ld, 1.f);
    for (unsigned c = 0; c < m; ++c) {
        float max_c;
        std::memcpy(&max_c, &h_max[c], sizeof(float));
        if (!compact_exponent(max_c, &expo[c]))
            return set_error(ctx, GLF_ERR_INVALID, "glf_graph_compact: the largest magnitude of column %u is %g (not finite, or >= 2^100)", c, (double)max_c);
        h_mult[c] = compact_multiplier(expo[c]);
    }
    DevBuf<float> mult;
    GLF_TRY(upload_operand(ctx, mult, h_mult));
    void *d16 = nullptr, *dex = nullptr;
    GLF_TRY(glf_malloc(ctx, &d16, sizeof(__half) * (size_t)cnt));
    int rc = glf_malloc(ctx, &dex, sizeof(int32_t) * ld);
    if (rc == GLF_OK && hipMemcpyAsync(dex, expo.data(), sizeof(int32_t) * ld, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = set_error(ctx, GLF_ERR_HIP, "glf_graph_compact: the upload of the exponents");
    if (rc == GLF_OK) {
        hipLaunchKernelGGL(k_phi_to_half, dim3(stream_grid(ctx, cnt / 8)), dim3(256), 0, ctx->stream, g->phi, cnt / 8, (int)ld, mult.p,
                           static_cast<__half *>(d16));
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = set_error(ctx, GLF_ERR_HIP, "glf_graph_compact: the conversion pass");
    }
    if (rc != GLF_OK) { // the handle is untouched and still f32 (hipFree, not glf_free: the failing call's message stays in last_error)
        (void)hipFree(d16);
        if (dex) (void)hipFree(dex);
        return rc;
    }
    GLF_TRY(glf_free(ctx, g->phi));
    g->phi = nullptr;
    g->phi16 = d16;
    g->d_expo = static_cast<int32_t *>(dex);
    g->expo.swap(expo);
    g->storage = GLF_PHI_F16;
    g->gram.clear();
    return GLF_OK;
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_compact(glf_graph *g, int storage)
{
    if (!g) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    if (storage != GLF_PHI_F32 && storage != GLF_PHI_F16) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_compact: storage %d", storage);
    if (storage == g->storage) return GLF_OK;
    if (storage == GLF_PHI_F32)
        return set_error(ctx, GLF_ERR_UNSUPPORTED, "glf_graph_compact: a compact handle does not go back to f32 (the f32 Phi was released: build the handle again)");
    GLF_ENTER(ctx);
    return graph_compact_f16(g);
}

int glf_graph_storage(const glf_graph *g, int *storage, int32_t *h_exponent)
{
    if (!g) return GLF_ERR_INVALID;
    if (storage) *storage = g->storage;
    if (h_exponent)
        for (unsigned c = 0; c < g->ld; ++c) h_exponent[c] = g->storage == GLF_PHI_F16 ? g->expo[c] : 0;
    return GLF_OK;
}

int glf_graph_dequantize(glf_graph *g, float *d_out)
{
    if (!g || !d_out) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    const int64_t cnt = (int64_t)g->width * g->height * g->ld;
    GLF_ENTER(ctx);
    if (g->storage == GLF_PHI_F16) {
        hipLaunchKernelGGL(k_phi_from_half, dim3(stream_grid(ctx, cnt / 8)), dim3(256), 0, ctx->stream, static_cast<const __half *>(g->phi16), cnt / 8,
                           (int)g->ld, g->d_expo, d_out);
        GLF_LAUNCH_CHECK(ctx);
    } else
        GLF_HIP(ctx, hipMemcpyAsync(d_out, g->phi, sizeof(float) * (size_t)cnt, hipMemcpyDeviceToDevice, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

} // extern "C"
