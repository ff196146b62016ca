// graph_project.hip -- the wide projection of a graph handle: c_k = Phi^T diag(w) s_k for up to GLF_GRAPH_MAX_PLANES planes in one
// pass over Phi on the matrix pipe (k_graph_project_wide), the counterpart of k_graph_synthesize's 32 outputs. glf_graph_project and
// glf_graph_normal_equations keep their own f64 kernels and their bits.
#include "phi_tile.hpp"
#include "phi_compact.hpp"

#include <algorithm>

namespace glf {

constexpr int GPW_SLOTS = GLF_GRAPH_MAX_PLANES;   // plane slots of one call: one index of the 32 x 32 accumulator tile
constexpr int GPW_PITCH = 33;                     // floats between two planes of the staged plane image
static_assert(GPW_SLOTS == 32, "the plane slots are the M index of v_mfma_f32_32x32x2_f32");

// How the columns are cut and how many workgroups run along the pixels: fixed per ld, so that the pixel partition and with it the
// summation order depend on (N, ld) alone. cw columns per workgroup (blockIdx.y runs over the ld / cw groups), at most xmax
// workgroups along the pixels (the rest by the grid stride).
struct GpwGeom {
    int cw, ny, xmax;
};
inline GpwGeom gpw_geom(unsigned ld)
{
    GpwGeom g;
    g.cw = ld < 128 ? (int)ld : 128;
    g.ny = (int)ld / g.cw;
    g.xmax = ld == 32 ? 1024 : ld == 64 ? 512 : ld == 128 ? 256 : 128;
    return g;
}

// part[blockIdx.x][k][LD] (f64) = sum over the workgroup's pixels of t_k[px] Phi[px][j], t_k = fl32(w s_k) (w NULL: s_k itself), for the
// columns j of the workgroup's group and every plane k < nplanes.
//
// Arithmetic. The pixels are the contraction index (phi_tile.hpp: the unpadded image, the chain rule, the four-wave reduction):
// A = t (M index: the 32 plane slots), B = Phi as stored (N index: 32 columns), so the accumulator of lane (r, h) holds column r of the
// tile for the planes acc_row(g, h), g < 16. Every element is its own f32 fma chain over the wave's pixels in ascending order: it
// depends on no other plane and on no other column.
// Plane slots >= nplanes are staged as zeros and never read from memory; rows past N are staged as zeros (Phi, w and the planes).
//
// The split and the traffic. An accumulator tile and its f64 image are 48 registers per (32 columns x 32 planes): a wave holds at
// most four of them beside the staged pieces of the next tile, so the columns are cut into groups of CW = min(LD, 128) over blockIdx.y.
// A group reads its own columns of Phi only, and the planes and w once per group: Phi is read once at every ld, the planes once at
// ld <= 128 and twice at ld 256 (per pixel 4 LD + 128 (LD / CW) + 4 (LD / CW) bytes with all 32 planes and a weight plane).
//
// Staging the planes. A tile is 32 runs of 128 contiguous bytes, one per plane; lane (r, h) loads pixel r of the planes 2 q + h (a
// half-wave reads one run; dword loads, since a plane's start is only 4-byte aligned when N is odd) and writes t to
// img[plane * 33 + r]. The operand read is img[r * 33 + px], plane r of one pixel per half-wave. The bank of a ds_read_b32 /
// ds_write_b32 is the dword address mod 32 and only the 32 lanes of a half-wave conflict with one another: at a pitch of 32 the 32
// planes of one pixel would sit on one bank (32-way); at 33 the bank is (r + px) mod 32, one lane per bank, and the writes
// (consecutive r at a fixed plane) are consecutive dwords. So both directions are conflict-free.
//
// ld <= 64 runs two workgroups per CU; ld >= 128 carries four tiles and their images and runs one wave per SIMD.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second loader, the same image).
template <int LD, class T = float>
__global__ __launch_bounds__(256, LD < 128 ? 2 : 1) void k_graph_project_wide(const T *__restrict__ phi, int64_t N, const float *__restrict__ w,
                                                                                int nplanes, const float *__restrict__ planes,
                                                                                double *__restrict__ part)
{
    constexpr int CW = LD < 128 ? LD : 128;
    constexpr int NT = CW / 32;   // accumulator tiles of a wave
    constexpr int NPL = GPW_SLOTS / 2; // planes per lane: 32 slots / 2 half-waves
    constexpr int RW = 32 * CW + 32 * GPW_PITCH; // floats of a wave's region: the Phi image, then the plane image
    static_assert(RW >= 2048 && RW % 4 == 0, "a region holds one f64 tile for the epilogue and keeps the next one 16-byte aligned");
    __shared__ __attribute__((aligned(16))) float region[4][RW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int c0 = (int)blockIdx.y * CW;
    float *tw = region[wave];
    float *img = tw + 32 * CW;
    const int64_t ntiles = (N + 31) / 32, tstride = (int64_t)gridDim.x * 4;

    f32x16 acc[NT];
    double dacc[NT][16];
#pragma unroll
    for (int c = 0; c < NT; ++c)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            acc[c][g] = 0.f;
            dacc[c][g] = 0.0;
        }

    // what this lane stages of a tile
    tile_regs<T, CW> v;
    float sv[NPL];
    float wv = 0.f;
    auto load_tile = [&](int64_t tile) {
        tile_load<CW>(v, phi, LD, c0, N, tile, lane);
        const int64_t px = tile * 32 + r;
        const bool live = px < N;
        wv = live && w ? w[px] : 0.f;
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int k = 2 * q + h;
            sv[q] = live && k < nplanes ? planes[(size_t)k * N + px] : 0.f;
        }
    };

    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile < ntiles) load_tile(tile);
    int chained = 0; // tiles in the running f32 chains
    for (; tile < ntiles; tile += tstride) {
        __builtin_amdgcn_wave_barrier();
        tile_put<CW, CW>(tw, v, lane);
#pragma unroll
        for (int q = 0; q < NPL; ++q) img[(2 * q + h) * GPW_PITCH + r] = w ? wv * sv[q] : sv[q];
        __builtin_amdgcn_wave_barrier();
        // the next tile's loads fly under this tile's MFMAs
        if (tile + tstride < ntiles) load_tile(tile + tstride);
#pragma unroll 4
        for (int u = 0; u < 16; ++u) {
            const int px = 2 * u + h;
            const float a = img[r * GPW_PITCH + px];
#pragma unroll
            for (int c = 0; c < NT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, tw[px * CW + c * 32 + r], acc[c], 0, 0, 0);
        }
        if (++chained == CHAIN_TILES) {
            chain_flush(acc, dacc);
            chained = 0;
        }
    }
    chain_flush(acc, dacc);

    // one f64 tile [plane][column] per 32 columns
    double *const pout = part + (size_t)blockIdx.x * nplanes * LD + c0;
    wave_tiles_reduce(region, dacc, wave, r, h, [&](int c, int e, double s) {
        const int k = e >> 5, j = e & 31;
        if (k < nplanes) pout[(size_t)k * LD + c * 32 + j] = s;
    });
}

// h_c [nplanes][m] of Phi [N][ld] (returns with the stream drained; h_c is written only on success)
template <class T>
static int graph_project_wide(glf_ctx *ctx, const T *d_phi, int64_t N, unsigned m, unsigned ld, const float *d_w, int nplanes,
                              const float *d_planes, double *h_c)
{
    if (!valid_ld(ld) || N < 1 || m < 1 || m > ld || nplanes < 1 || nplanes > GPW_SLOTS)
        return set_error(ctx, GLF_ERR_INVALID, "graph_project_wide: ld=%u m=%u nplanes=%d", ld, m, nplanes);
    const GpwGeom gm = gpw_geom(ld);
    const unsigned nblk = (unsigned)std::min<int64_t>(ceil_div(ceil_div(N, 32), 4), gm.xmax);
    const size_t ncols = (size_t)nplanes * ld;
    DevBuf<double> part, tot;
    GLF_TRY(part.alloc(ctx, (size_t)nblk * ncols));
    dispatch_ld(ld, [&](auto LD) { // (ld is valid)
        hipLaunchKernelGGL((k_graph_project_wide<LD.value, T>), dim3(nblk, (unsigned)gm.ny), dim3(256), 0, ctx->stream, d_phi, N, d_w, nplanes, d_planes,
                           part.p);
    });
    GLF_LAUNCH_CHECK(ctx);
    std::vector<double> hc;
    GLF_TRY(sum_partials_to_host(ctx, part, (int)nblk, ncols, tot, hc));
    for (int k = 0; k < nplanes; ++k)
        for (unsigned j = 0; j < m; ++j) h_c[(size_t)k * m + j] = hc[(size_t)k * ld + j];
    return GLF_OK;
}

} // namespace glf

using namespace glf;

extern "C" int glf_graph_project_wide(glf_graph *g, const float *d_w, int nplanes, const float *d_planes, double *h_c)
{
    if (!g || nplanes < 1 || nplanes > GLF_GRAPH_MAX_PLANES || !d_planes || !h_c) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    GLF_ENTER(ctx);
    int rc = GLF_OK;
    dispatch_phi(g, [&](auto *phi) { rc = graph_project_wide(ctx, phi, (int64_t)g->width * g->height, g->m, g->ld, d_w, nplanes, d_planes, h_c); });
    // (a compact handle: c_k[c] 2^e_c, the column scale folded into the read-back in f64)
    if (rc == GLF_OK && g->storage == GLF_PHI_F16) compact_fold_cols(h_c, (size_t)nplanes, g->m, g->expo.data());
    return rc;
}
