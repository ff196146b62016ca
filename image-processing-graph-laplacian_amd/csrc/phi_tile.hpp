// phi_tile.hpp -- what the graph-handle kernels share (graph.hip, graph_fit.hip, graph_cluster.hip, graph_basis.hip, graph_robust.hip,
// graph_project.hip, graph_quad.hip, graph_classify.hip, graph_edges.hip): staging a tile of Phi, the "outputs are M, pixels are N"
// contraction, the f32 chain rule, the four-wave f64 epilogue, and the host steps around a launch (the dispatch on storage and ld, the
// launch on a resident grid, the coefficient operand, the identity terms). Only pieces that at least two kernels use, as forceinlined
// templates and host inlines; each kernel keeps its index roles, its tile loop, its epilogue and its arithmetic contract in its own file
// (a shared tile loop was tried and cost time: DESIGN.md, profiles/graph_sweep_kernel_resources.txt).
//
// The tile. Every kernel gives one wave a tile of 32 pixels (32 rows of Phi), the tiles strided over the grid, and stages CW columns
// of it at a time: a lane loads CW / 8 float4s, whole 16-byte pieces in address order (piece e = q 64 + lane is row e / (CW / 4),
// float4 e % (CW / 4): each row's CW * 4 bytes contiguous), rows past N as zeros, which are never read from memory. The pieces go to
// the wave's own LDS image between two wave barriers -- the wave's reads of the previous image precede the writes, since LDS runs in
// order per wave, and no other wave touches the image -- and the next tile's (or chunk's) loads are issued right after, so that they
// fly under the MFMAs of this one. The image's row pitch decides how it is read back:
//   CW + 4  one pixel per lane as float4s (the pixels are the MFMA's N or M index): the 16 lanes of a ds_read_b128 group hit 64
//           different banks;
//   CW      one column per lane as floats (the pixels are the contraction index): at step u lane (r, h) reads column r of pixel
//           2 u + h, consecutive lanes, consecutive floats, no conflict at any pitch.
// The accumulator. v_mfma_f32_32x32x2_f32 leaves in register g of the lanes of half-wave h the row acc_row(g, h) of the 32 x 32 tile
// and in lane r its column r.
// The chain rule. Where the pixels are the contraction index, an accumulator is an f32 fma chain over at most GLF_GRAPH_NORMAL_CHAIN
// pixel terms (a whole number of tiles); it is then added into its f64 image and cleared (chain_flush).
// The reduction. No atomics: the four waves' f64 images are added through LDS in the fixed order ((w0 + w1) + w2) + w3
// (wave_tiles_reduce), the workgroups by filter.hip's k_cols_sum in an order that depends on their number alone (sum_partials).
#pragma once
#include "glf_internal.hpp"
#include "phi_compact.hpp"

#include <hip/hip_fp16.h>

#include <type_traits>

namespace glf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

static_assert(GLF_GRAPH_NORMAL_CHAIN % 32 == 0 && GLF_GRAPH_NORMAL_CHAIN >= 32 && GLF_GRAPH_NORMAL_CHAIN <= 256,
              "a chain is a whole number of 32-pixel tiles");
constexpr int CHAIN_TILES = GLF_GRAPH_NORMAL_CHAIN / 32; // 32-pixel tiles in one f32 chain

// the row of the 32 x 32 accumulator tile that register g holds in half-wave h
__host__ __device__ __forceinline__ constexpr int acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

__device__ __forceinline__ void acc_clear(f32x16 &acc)
{
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
}

// v <- this lane's pieces of columns [col0, col0 + CW) of tile `tile` of phi (row pitch ld floats)
template <int CW>
__device__ __forceinline__ void tile_load(float4 (&v)[CW / 8], const float *phi, int ld, int col0, int64_t N, int64_t tile, int lane)
{
    constexpr int FPR = CW / 4; // float4 pieces per staged row
    const int64_t base = tile * 32;
#pragma unroll
    for (int q = 0; q < CW / 8; ++q) {
        const int e = q * 64 + lane, row = e / FPR, c4 = e % FPR;
        v[q] = base + row < N ? *reinterpret_cast<const float4 *>(phi + (size_t)(base + row) * ld + col0 + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// the pieces into an image of row pitch PITCH, no barrier
template <int CW, int PITCH>
__device__ __forceinline__ void tile_put(float *img, const float4 (&v)[CW / 8], int lane)
{
    constexpr int FPR = CW / 4;
#pragma unroll
    for (int q = 0; q < CW / 8; ++q) {
        const int e = q * 64 + lane, row = e / FPR, c4 = e % FPR;
        *reinterpret_cast<float4 *>(img + row * PITCH + c4 * 4) = v[q];
    }
}

// The compact storage (a handle after glf_graph_compact: Phi as __half [N][ld], the column scales on the host). The same tile, the
// same image: a lane loads CW / 16 uint4s of 8 halves each, whole 16-byte pieces in address order (piece e = q 64 + lane is row
// e / (CW / 8), halves [8 (e % (CW / 8)), + 8): each row's CW * 2 bytes contiguous), rows past N as zeros, never read; tile_put
// converts a piece with v_cvt_f32_f16 (exact, f16 subnormals kept; no scale is applied on the device) and writes its two float4s
// where the f32 pieces of those columns go (neighbouring lanes' float4s then lie 32 bytes apart, a two-way conflict of the
// ds_write_b128 that the f32 put, 16 bytes apart, does not have: profiles/graph_compact_pmc_cluster.txt). Everything after the
// image is the f32 kernel's own.
template <class T>
struct phi_piece;
template <>
struct phi_piece<float> {
    typedef float4 type;
    static constexpr int elems = 4;
};
template <>
struct phi_piece<__half> {
    typedef uint4 type;
    static constexpr int elems = 8;
};
// the registers that hold a lane's pieces of CW columns of a tile
template <class T, int CW>
using tile_regs = typename phi_piece<T>::type[CW / (2 * phi_piece<T>::elems)];

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int CW>
__device__ __forceinline__ void tile_load(uint4 (&v)[CW / 16], const __half *phi, int ld, int col0, int64_t N, int64_t tile, int lane)
{
    constexpr int PPR = CW / 8; // 16-byte pieces per staged row
    const int64_t base = tile * 32;
#pragma unroll
    for (int q = 0; q < CW / 16; ++q) {
        const int e = q * 64 + lane, row = e / PPR, c8 = e % PPR;
        v[q] = base + row < N ? *reinterpret_cast<const uint4 *>(phi + (size_t)(base + row) * ld + col0 + c8 * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
}

template <int CW, int PITCH>
__device__ __forceinline__ void tile_put(float *img, const uint4 (&v)[CW / 16], int lane)
{
    constexpr int PPR = CW / 8;
#pragma unroll
    for (int q = 0; q < CW / 16; ++q) {
        const int e = q * 64 + lane, row = e / PPR, c8 = e % PPR;
        const f16x8 x = __builtin_bit_cast(f16x8, v[q]);
        float *dst = img + row * PITCH + c8 * 8;
        *reinterpret_cast<float4 *>(dst) = make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
        *reinterpret_cast<float4 *>(dst + 4) = make_float4((float)x[4], (float)x[5], (float)x[6], (float)x[7]);
    }
}

// the wave's image <- the pieces, between the two wave barriers. A kernel that stages more with the tile (a second image, weights,
// planes) writes all of it between two barriers of its own, the pieces with tile_put.
template <int CW, int PITCH, class V>
__device__ __forceinline__ void tile_store(float *img, const V &v, int lane)
{
    __builtin_amdgcn_wave_barrier();
    tile_put<CW, PITCH>(img, v, lane);
    __builtin_amdgcn_wave_barrier();
}

struct NoHook {
    __device__ __forceinline__ void operator()(int, const float4 &) const {}
};

// acc[acc_row(g, h)][pixel r] += sum_c a[c][row] img[r][c] over the CW columns of a staged chunk: the outputs are the M index (A: the
// operand a [CW][OUT] in LDS; OUT < 32: rows >= OUT are zeros and never read), the pixels the N index (B: the image, pitch CW + 4). The
// order depends on CW alone: half-wave h takes columns h CW / 2 + t at step t, and every output is its own fma chain in that order, so
// its bits do not depend on the outputs beside it nor on OUT. each(u, b) sees every float4 of the image after its four MFMAs.
// (The operand reads are written in two forms on purpose -- OUT 32 as the MFMAs' arguments, narrower operands as four masked reads
// first: either form alone moved the LDS reads of one group of instances, profiles/graph_phi_tile_kernel_resources.txt.)
template <int CW, int OUT, class Each = NoHook>
__device__ __forceinline__ void chunk_contract(f32x16 &acc, const float *img, const float *a, int r, int h, Each each = {})
{
    static_assert(OUT == 32 || (OUT < 32 && (OUT & (OUT - 1)) == 0), "a full tile of rows, or a power of two of them");
#pragma unroll
    for (int u = 0; u < CW / 8; ++u) {
        const float4 b = *reinterpret_cast<const float4 *>(img + r * (CW + 4) + h * (CW / 2) + 4 * u);
        const float *ak = a + (size_t)(h * (CW / 2) + 4 * u) * OUT + (r & (OUT - 1));
        if constexpr (OUT == 32) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[0 * OUT], b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[1 * OUT], b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[2 * OUT], b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ak[3 * OUT], b.w, acc, 0, 0, 0);
        } else {
            const bool arow = r < OUT; // this lane's row of A is an output
            const float a0 = arow ? ak[0 * OUT] : 0.f, a1 = arow ? ak[1 * OUT] : 0.f;
            const float a2 = arow ? ak[2 * OUT] : 0.f, a3 = arow ? ak[3 * OUT] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b.w, acc, 0, 0, 0);
        }
        each(u, b);
    }
}

// the end of an f32 chain: dacc += acc, acc <- 0
template <int NT>
__device__ __forceinline__ void chain_flush(f32x16 (&acc)[NT], double (&dacc)[NT][16])
{
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            dacc[t][g] += (double)acc[t][g];
            acc[t][g] = 0.f;
        }
}

// The workgroup's four waves, wave 0 first, tile by tile through the waves' regions (RW >= 2048 floats: one [32][32] f64 tile
// each): store(t, e, s) gets the sum s of element e = row * 32 + column of tile t, once per workgroup, and does the kernel's own
// guarded store.
template <int NT, int RW, class Store>
__device__ __forceinline__ void wave_tiles_reduce(float (&region)[4][RW], const double (&dacc)[NT][16], int wave, int r, int h, Store store)
{
    static_assert(RW >= 2048, "a region holds one f64 tile");
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        __syncthreads();
        double *mine = reinterpret_cast<double *>(region[wave]);
#pragma unroll
        for (int g = 0; g < 16; ++g) mine[acc_row(g, h) * 32 + r] = dacc[t][g];
        __syncthreads();
        for (int e = threadIdx.x; e < 1024; e += 256) {
            const double s = ((reinterpret_cast<const double *>(region[0])[e] + reinterpret_cast<const double *>(region[1])[e]) +
                              reinterpret_cast<const double *>(region[2])[e]) + reinterpret_cast<const double *>(region[3])[e];
            store(t, e, s);
        }
    }
}

// out[i] = [Phi[px_i][0 .. dim) | s_k[px_i], k < nplanes | w[px_i] if wcol (1 where w is NULL)], px_i = floor(i N / ns): the sample of
// rows a host-side seeding or scale estimate reads. A pure gather (graph.hip).
// expo: NULL on an f32 handle; on a compact one the column exponents (device int [ld]), and the gather writes Q = 2^e_c half.
template <class T>
__global__ void k_sample_rows(const T *__restrict__ phi, const int *__restrict__ expo, int64_t N, int ld, int dim, int nplanes,
                              const float *__restrict__ planes, const float *__restrict__ w, int wcol, int64_t ns, float *__restrict__ out);
// the gather on a handle of either storage (queued)
int graph_sample_rows(glf_graph *g, int dim, int nplanes, const float *d_planes, const float *d_w, int wcol, int64_t ns, float *d_out);

// f(phi) with the handle's Phi as const float * or const __half *, by its storage
template <class F>
inline void dispatch_phi(const glf_graph *g, F &&f)
{
    if (g->storage == GLF_PHI_F16) f(static_cast<const __half *>(g->phi16));
    else f(static_cast<const float *>(g->phi));
}

// the element type behind the pointer dispatch_phi hands over
template <class P>
using phi_elem_t = std::remove_cv_t<std::remove_pointer_t<P>>;

// f(std::integral_constant<int, LD>) for the ld of a graph handle; false: no such instance
template <class F>
inline bool dispatch_ld(unsigned ld, F &&f)
{
    switch (ld) {
    case 32: f(std::integral_constant<int, 32>{}); return true;
    case 64: f(std::integral_constant<int, 64>{}); return true;
    case 128: f(std::integral_constant<int, 128>{}); return true;
    case 256: f(std::integral_constant<int, 256>{}); return true;
    }
    return false;
}

// both: f(LD, phi, T{}) with the handle's Phi as const T *phi, so that a kernel instance is k<LD.value, decltype(t)>; false: no
// instance for the handle's ld
template <class F>
inline bool dispatch_phi_ld(const glf_graph *g, F &&f)
{
    bool found = false;
    dispatch_phi(g, [&](auto *phi) { found = dispatch_ld(g->ld, [&](auto LD) { f(LD, phi, phi_elem_t<decltype(phi)>{}); }); });
    return found;
}

// The launch of a kernel of the shape "one 32-pixel tile per wave, four waves, resident grid" over N pixels on the handle's stream
// (queued): resident_tile_grid, the launch, the check.
template <class Kernel, class... Args>
inline int launch_tiles(glf_graph *g, Kernel kernel, int64_t N, Args... args)
{
    int64_t nblk = 0;
    GLF_TRY(resident_tile_grid(g, kernel, N, &nblk));
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(256), 0, g->ctx->stream, args...);
    GLF_LAUNCH_CHECK(g->ctx);
    return GLF_OK;
}
// the same for a kernel with a reduction: its last argument is part, [workgroups][cols] f64 partials, sized here; *nblk: the
// workgroups (the rows sum_partials adds)
template <class Kernel, class... Args>
inline int launch_tiles_partials(glf_graph *g, Kernel kernel, int64_t N, DevBuf<double> &part, size_t cols, int64_t *nblk, Args... args)
{
    GLF_TRY(resident_tile_grid(g, kernel, N, nblk));
    GLF_TRY(part.alloc(g->ctx, (size_t)*nblk * cols));
    hipLaunchKernelGGL(kernel, dim3((unsigned)*nblk), dim3(256), 0, g->ctx->stream, args..., part.p);
    GLF_LAUNCH_CHECK(g->ctx);
    return GLF_OK;
}

// The coefficient operand of a pass that contracts Phi with `rows` coefficient vectors h_a ([rows][m], f64): the copy the handle's
// kernels take -- on a compact handle folded with the column scales in f64 (compact_fold_cols), before any fl32 -- is returned, and
// its fl32 written as the MFMA's A operand: a[j][c] at [c][j] of the [ld][OUT] block op, whose other entries stay as they are
// (zeros). Whether a value that is not finite is refused, as f64 or as f32, is the caller's rule.
inline std::vector<double> coeff_operand(const glf_graph *g, size_t rows, const double *h_a, int OUT, float *op)
{
    const unsigned m = g->m;
    std::vector<double> a(h_a, h_a + rows * m);
    if (g->storage == GLF_PHI_F16) compact_fold_cols(a.data(), rows, m, g->expo.data());
    for (size_t j = 0; j < rows; ++j)
        for (unsigned c = 0; c < m; ++c) op[(size_t)c * OUT + j] = (float)a[j * m + c];
    return a;
}

// The identity terms ident[j] s_plane[j] of synthesize's outputs and classify's scores, j < n <= 32. ident_terms_check: -1 if every
// plane[j] lies in -1 .. nplanes - 1 and ident and d_planes are there where one is >= 0 (*any_plane), else the first j out of range, or
// n for the missing pointers. ident_terms_pack: op <- [32] float ident[j] (0 without a term), [32] int plane[j] (-1 without one).
inline int ident_terms_check(int n, const int *plane, int nplanes, const float *ident, const float *d_planes, bool *any_plane)
{
    *any_plane = false;
    for (int j = 0; j < n; ++j) {
        if (plane[j] < -1 || plane[j] >= nplanes) return j;
        *any_plane = *any_plane || plane[j] >= 0;
    }
    return *any_plane && (!ident || !d_planes) ? n : -1;
}
inline void ident_terms_pack(int n, const float *ident, const int *plane, float *op)
{
    int h_plane[32];
    for (int j = 0; j < 32; ++j) {
        const bool term = j < n && plane[j] >= 0;
        op[j] = term ? ident[j] : 0.f;
        h_plane[j] = term ? plane[j] : -1;
    }
    std::memcpy(op + 32, h_plane, sizeof(h_plane));
}

// tot[c] = sum over r < nrows of part[r][c], c < ncols (queued)
inline int sum_partials(glf_ctx *ctx, const DevBuf<double> &part, int nrows, size_t ncols, DevBuf<double> &tot)
{
    GLF_TRY(tot.alloc(ctx, ncols));
    hipLaunchKernelGGL(k_cols_sum, dim3((unsigned)ncols), dim3(256), 0, ctx->stream, part.p, nrows, (unsigned)ncols, tot.p);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}
// ... and h_tot <- tot; sync false: the copy is queued, and h_tot and tot must outlive whatever drains the stream
inline int sum_partials_to_host(glf_ctx *ctx, const DevBuf<double> &part, int nrows, size_t ncols, DevBuf<double> &tot, std::vector<double> &h_tot,
                                bool sync = true)
{
    GLF_TRY(sum_partials(ctx, part, nrows, ncols, tot));
    h_tot.resize(ncols);
    GLF_HIP(ctx, hipMemcpyAsync(h_tot.data(), tot.p, sizeof(double) * ncols, hipMemcpyDeviceToHost, ctx->stream));
    if (sync) GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GLF_OK;
}

// op <- h_op (queued: h_op must outlive whatever drains the stream)
inline int upload_operand(glf_ctx *ctx, DevBuf<float> &op, const std::vector<float> &h_op)
{
    GLF_TRY(op.alloc(ctx, h_op.size()));
    GLF_HIP(ctx, hipMemcpyAsync(op.p, h_op.data(), sizeof(float) * h_op.size(), hipMemcpyHostToDevice, ctx->stream));
    return GLF_OK;
}

} // namespace glf
