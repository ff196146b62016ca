// graph_edges.hip -- the spectral edge map of a graph handle: out_d(px) = sum_{c < dim} (fl32(scale_c) (Phi[nb_d(px)][c] - Phi[px][c]))^2
// for the neighbours nb_d = E (row, col + 1), S (row + 1, col), SE (row + 1, col + 1), SW (row + 1, col - 1) of every pixel, the
// squared distance in the embedding between neighbouring pixels (k_graph_edges). The handle's first stencil kernel: every other call
// treats the rows of Phi as an unordered set, this one uses that they lie on the image raster. The staging is phi_tile.hpp's (the
// piece order, the LDS image at pitch CW + 4, the loads of the next image issued under the arithmetic); the new parts are a loader
// that takes a base pixel and a count (strip_load), the strip / row-block geometry and the pinned f32 chain (include/glf.h).
// Out of scope: a full (non-diagonal) metric, unit-length rows, filters wider than one pixel, non-maximum suppression, watershed,
// connected components, repairing the scale of Phi's sample rows (glf_graph_samples says where they are), contexts with a
// communicator and glf_multi_* (handles refuse them), m > 256, a flag of the host program, and anything inside phi_tile.hpp's
// existing functions or the existing kernels.
#include "phi_tile.hpp"
#include "phi_compact.hpp"

#include <cfloat>
#include <cmath>

// the arithmetic of a chain is pinned operation by operation (include/glf.h): nothing here is contracted into an fma that the
// text does not spell out
#pragma clang fp contract(off)

namespace glf {

constexpr int GE_STAGED = 64;            // pixels of an image row in a wave's LDS image: one per lane
constexpr int GE_STRIP = GE_STAGED - 2;  // of which the wave owns the inner 62 (one halo pixel on either side)
constexpr int GE_ROWS = 16;              // image rows of a row block: the wave reads one halo row below them

// v <- this lane's pieces of columns [col0, col0 + CW) of the 32 raster pixels px0 .. px0 + 31 of phi (row pitch ld elements), in
// tile_load's piece order (piece e = q 64 + lane is pixel e / pieces-per-row, 16 bytes in address order). Only the pixels px0 + j
// with lo <= j < hi are read; every other pixel is zeros and never read from memory (px0 + j may lie outside the array there).
template <int CW>
__device__ __forceinline__ void strip_load(float4 (&v)[CW / 8], const float *phi, int ld, int col0, int64_t px0, int lo, int hi, int lane)
{
    constexpr int FPR = CW / 4;
#pragma unroll
    for (int q = 0; q < CW / 8; ++q) {
        const int e = q * 64 + lane, j = e / FPR, c4 = e % FPR;
        v[q] = j >= lo && j < hi ? *reinterpret_cast<const float4 *>(phi + (size_t)(px0 + j) * ld + col0 + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
template <int CW>
__device__ __forceinline__ void strip_load(uint4 (&v)[CW / 16], const __half *phi, int ld, int col0, int64_t px0, int lo, int hi, int lane)
{
    constexpr int PPR = CW / 8;
#pragma unroll
    for (int q = 0; q < CW / 16; ++q) {
        const int e = q * 64 + lane, j = e / PPR, c8 = e % PPR;
        v[q] = j >= lo && j < hi ? *reinterpret_cast<const uint4 *>(phi + (size_t)(px0 + j) * ld + col0 + c8 * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
}

// one image row of a strip in flight: the pieces of its 64 staged pixels as two tiles of 32, and this lane's pixel's flag
template <class T, int CW>
struct strip_regs {
    tile_regs<T, CW> v[2];
    bool ok; // staged pixel `lane` lies inside the image and is valid
};

// r <- columns [col0, col0 + CW) of the staged pixels of image row y of the strip that starts at image column c0: staged pixel j is
// image column c0 - 1 + j. Columns outside [0, W) and rows >= H are zeros, never read, and not ok; the valid plane rides along.
template <int CW, class T>
__device__ __forceinline__ void strip_row_load(strip_regs<T, CW> &r, const T *phi, int ld, int col0, const uint8_t *valid, int W, int H, int c0,
                                               int y, int lane)
{
    const int lo = c0 == 0 ? 1 : 0;
    const int room = W - c0 + 1, hi = y < H ? (room < GE_STAGED ? room : GE_STAGED) : 0;
    const int64_t px0 = (int64_t)y * W + c0 - 1;
    strip_load<CW>(r.v[0], phi, ld, col0, px0, lo, hi, lane);
    strip_load<CW>(r.v[1], phi, ld, col0, px0 + 32, lo - 32, hi - 32, lane);
    const bool inside = lane >= lo && lane < hi;
    r.ok = inside && (valid == nullptr || valid[inside ? px0 + lane : 0] != 0);
}

// the wave's image <- the row in flight, between two wave barriers (tile_store's rule: the wave's reads of what the image held
// precede the writes, LDS runs in order per wave, and no other wave touches the image)
template <int CW, int PITCH, class T>
__device__ __forceinline__ void strip_row_store(float *img, const strip_regs<T, CW> &r, int lane)
{
    __builtin_amdgcn_wave_barrier();
    tile_put<CW, PITCH>(img, r.v[0], lane);
    tile_put<CW, PITCH>(img + 32 * PITCH, r.v[1], lane);
    __builtin_amdgcn_wave_barrier();
}

// q[k], k < ND, continued over n4 float4s of one staged chunk: per column d = b - a (one f32 subtraction), x = s d (one f32
// multiplication), q = fmaf(x, x, q), the columns ascending. The ND chains of a pixel (one per requested direction) share the loop:
// each is its own dependent chain in the pinned order, and they are independent of each other, so the fmas of one issue under the
// latency of the others'.
template <int ND>
__device__ __forceinline__ void edge_chains(const float *pa, const float *(&pb)[4], const float *s, int n4, float (&q)[4])
{
#pragma unroll 2
    for (int c4 = 0; c4 < n4; ++c4) {
        const float4 a = *reinterpret_cast<const float4 *>(pa + 4 * c4), sc = *reinterpret_cast<const float4 *>(s + 4 * c4);
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const float4 b = *reinterpret_cast<const float4 *>(pb[k] + 4 * c4);
            const float d0 = b.x - a.x;
            const float x0 = sc.x * d0;
            q[k] = fmaf(x0, x0, q[k]);
            const float d1 = b.y - a.y;
            const float x1 = sc.y * d1;
            q[k] = fmaf(x1, x1, q[k]);
            const float d2 = b.z - a.z;
            const float x2 = sc.z * d2;
            q[k] = fmaf(x2, x2, q[k]);
            const float d3 = b.w - a.w;
            const float x3 = sc.w * d3;
            q[k] = fmaf(x3, x3, q[k]);
        }
    }
}

// out[k][px] = sum_{c < dim} (scale[c] (Phi[nb][c] - Phi[px][c]))^2 for the k-th set bit of dirs (bit 0 E, 1 S, 2 SE, 3 SW), +0 where
// nb lies outside the image or either endpoint is not valid.
// Geometry: the image is cut into strips of GE_STRIP columns and blocks of GE_ROWS rows; a (strip, row block) unit belongs to one
// wave, the units strided over the resident grid, neighbouring waves on neighbouring strips. The wave marches down its rows with a
// ring of two LDS images (this row, the next) of GE_STAGED pixels at pitch CW + 4: lane j's staged pixel is image column c0 - 1 + j,
// lanes 1 .. GE_STRIP own their pixel and run its chains, reading their own and their neighbours' rows of the images as float4s.
// Each image row of a unit is loaded once per column chunk (plus the halo row below the block), and the load of the row after next
// (at a unit's last row: the first row of the wave's next pass) is issued before the arithmetic of this one.
// Column chunks (ld 128 / 256: CW = 64) are outermost over a unit: the partial sum of a live edge is stored to its output element
// after a chunk and reloaded by the same lane before the next, which keeps the chain's bits. Chunks at or beyond dim are not read.
// scale: device [LD], zeros from dim on (a zero scale gives x = +-0 and fmaf(x, x, q) = q). No atomics.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second put, the same image).
template <int LD, class T>
__global__ __launch_bounds__(256) void k_graph_edges(const T *__restrict__ phi, int W, int H, unsigned dirs, int dim, const float *__restrict__ scale,
                                                      const uint8_t *__restrict__ valid, float *out)
{
    constexpr int CW = LD < 64 ? LD : 64;
    constexpr int PITCH = CW + 4;
    __shared__ __attribute__((aligned(16))) float img_sh[4][2][GE_STAGED * PITCH];
    __shared__ __attribute__((aligned(16))) float s_sh[LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < LD; e += 256) s_sh[e] = scale[e];
    __syncthreads();
    const int nch = (dim + CW - 1) / CW;
    const int nstrips = (W + GE_STRIP - 1) / GE_STRIP, nblocks = (H + GE_ROWS - 1) / GE_ROWS;
    const int64_t N = (int64_t)W * H, units = (int64_t)nstrips * nblocks, ustride = (int64_t)gridDim.x * 4;
    // the staged pixels a lane reads as neighbours (clamped: lanes 0 and 63 own nothing and store nothing)
    const int east = lane < GE_STAGED - 1 ? lane + 1 : lane, west = lane > 0 ? lane - 1 : lane;
    // the requested directions in plane order: sel holds the k-th set bit of dirs in bits [2 k, 2 k + 2), nd their number
    unsigned sel = 0;
    int nd = 0;
#pragma unroll
    for (unsigned d = 0; d < 4; ++d)
        if (dirs >> d & 1u) sel |= d << (2 * nd++);
    strip_regs<T, CW> r;
    int64_t unit = (int64_t)blockIdx.x * 4 + wave;
    int ch = 0;
    if (unit < units) strip_row_load<CW>(r, phi, LD, 0, valid, W, H, (int)(unit % nstrips) * GE_STRIP, (int)(unit / nstrips) * GE_ROWS, lane);
    while (unit < units) {
        const int c0 = (int)(unit % nstrips) * GE_STRIP, y0 = (int)(unit / nstrips) * GE_ROWS, y1 = y0 + GE_ROWS < H ? y0 + GE_ROWS : H;
        const int64_t unit_next = ch + 1 < nch ? unit : unit + ustride; // the wave's next pass: the next chunk of this unit, or its next unit
        const int ch_next = ch + 1 < nch ? ch + 1 : 0;
        const int col0 = ch * CW, left = dim - col0, n4 = ((left < CW ? left : CW) + 3) / 4;
        const int col = c0 - 1 + lane;
        const bool owner = lane >= 1 && lane <= GE_STRIP && col < W;
        strip_row_store<CW, PITCH>(img_sh[wave][0], r, lane);
        bool ok_next = r.ok;
        strip_row_load<CW>(r, phi, LD, col0, valid, W, H, c0, y0 + 1, lane);
#pragma unroll 1
        for (int y = y0; y < y1; ++y) {
            const float *cur = img_sh[wave][(y - y0) & 1];
            float *nxt = img_sh[wave][(y - y0 + 1) & 1];
            const bool ok_cur = ok_next;
            strip_row_store<CW, PITCH>(nxt, r, lane);
            ok_next = r.ok;
            // the row after next, or the first row of the next pass, flies under this row's arithmetic
            if (y + 2 <= y1) strip_row_load<CW>(r, phi, LD, col0, valid, W, H, c0, y + 2, lane);
            else if (unit_next < units)
                strip_row_load<CW>(r, phi, LD, ch_next * CW, valid, W, H, (int)(unit_next % nstrips) * GE_STRIP, (int)(unit_next / nstrips) * GE_ROWS, lane);
            const int ok_c = ok_cur ? 1 : 0, ok_n = ok_next ? 1 : 0;
            const bool live_e = (ok_c & __shfl(ok_c, east)) != 0, live_s = (ok_c & ok_n) != 0;
            const bool live_se = (ok_c & __shfl(ok_n, east)) != 0, live_sw = (ok_c & __shfl(ok_n, west)) != 0;
            const float *pa = cur + lane * PITCH;
            const float *pb_e = cur + east * PITCH, *pb_s = nxt + lane * PITCH, *pb_se = nxt + east * PITCH, *pb_sw = nxt + west * PITCH;
            // plane k is direction sel_k (uniform selects: no indexed register arrays)
            const float *pb[4];
            bool live[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned d = sel >> (2 * k) & 3u;
                pb[k] = d == 0 ? pb_e : d == 1 ? pb_s : d == 2 ? pb_se : pb_sw;
                live[k] = d == 0 ? live_e : d == 1 ? live_s : d == 2 ? live_se : live_sw;
            }
            float *o = out + ((int64_t)y * W + (owner ? col : 0));
            float q[4] = {0.f, 0.f, 0.f, 0.f};
            if (ch > 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < nd && owner && live[k]) q[k] = o[(int64_t)k * N];
            }
            switch (nd) { // (uniform)
            case 1: edge_chains<1>(pa, pb, s_sh + col0, n4, q); break;
            case 2: edge_chains<2>(pa, pb, s_sh + col0, n4, q); break;
            case 3: edge_chains<3>(pa, pb, s_sh + col0, n4, q); break;
            default: edge_chains<4>(pa, pb, s_sh + col0, n4, q); break;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nd && owner) {
                    if (live[k]) o[(int64_t)k * N] = q[k];
                    else if (ch == 0) o[(int64_t)k * N] = 0.f;
                }
        }
        unit = unit_next;
        ch = ch_next;
    }
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_edges(glf_graph *g, unsigned dirs, unsigned dim, const double *h_scale, const uint8_t *d_valid, float *d_out)
{
    if (!g || !d_out) return g ? set_error(g->ctx, GLF_ERR_INVALID, "glf_graph_edges: d_out is NULL") : GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    const unsigned m = g->m, ld = g->ld;
    if (dirs == 0 || dirs > 15u) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_edges: dirs %u is not a union of GLF_EDGE_E | _S | _SE | _SW", dirs);
    if (dim == 0 || dim > m) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_edges: dim %u outside 1 .. m = %u", dim, m);
    // (a compact handle: the column scales of Phi folded into the scale in f64, before its fl32: compact_fold_cols' rule)
    std::vector<double> sc(dim, 1.0);
    if (h_scale) std::copy(h_scale, h_scale + dim, sc.begin());
    if (g->storage == GLF_PHI_F16) compact_fold_cols(sc.data(), 1, dim, g->expo.data());
    for (unsigned c = 0; c < dim; ++c)
        if (!(std::fabs(sc[c]) <= (double)FLT_MAX))
            return set_error(ctx, GLF_ERR_INVALID, "glf_graph_edges: scale[%u] (folded with its column's 2^e_c) is not finite in f32", c);
    GLF_ENTER(ctx);
    std::vector<float> h_op(ld, 0.f);
    for (unsigned c = 0; c < dim; ++c) h_op[c] = (float)sc[c];
    DevBuf<float> op;
    GLF_TRY(upload_operand(ctx, op, h_op));
    // one wave per (strip, row block) unit where resident_tile_grid counts one wave per 32-pixel tile
    const int64_t units = ceil_div(g->width, GE_STRIP) * ceil_div(g->height, GE_ROWS);
    int rc = GLF_ERR_INVALID;
    dispatch_phi_ld(g, [&](auto LD, auto *phi, auto t) {
        rc = launch_tiles(g, k_graph_edges<LD.value, decltype(t)>, units * 32, phi, g->width, g->height, dirs, (int)dim, (const float *)op.p, d_valid, d_out);
    });
    GLF_TRY(rc);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (h_op and op go out of scope)
    return GLF_OK;
}

int glf_graph_samples(const glf_graph *g, unsigned *h_idx)
{
    if (!g) return GLF_ERR_INVALID;
    if (!h_idx) return set_error(g->ctx, GLF_ERR_INVALID, "glf_graph_samples: h_idx is NULL (it takes p = %u entries)", g->p);
    std::copy(g->samples.begin(), g->samples.end(), h_idx);
    return GLF_OK;
}

} // extern "C"
