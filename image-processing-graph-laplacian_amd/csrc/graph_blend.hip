// graph_blend.hip -- per-pixel read-out of a bank of score planes on a graph handle: the nout * nlevels <= GLF_BLEND_MAX_SLOTS planes
// z_s = ident_s s_plane[s] + Phi a_s of glf_graph_synthesize, slot s = o * nlevels + b, are formed in registers in one pass over Phi
// (k_graph_blend) and read out per pixel by a level map t: output o gets the plane of level t(px) where t is an integer and the
// linear blend of the two neighbouring levels otherwise; the bank itself is never written. A filter whose strength varies over the
// image (a bank of responses, the strength map as the level), and the piecewise render out(px) = Phi[px] . a_label(px) of per-segment
// models both end in this step. The contraction is k_graph_synthesize's, the scores are k_graph_classify's; the new part is the
// epilogue after them.
// Out of scope: per-output level maps, more than 32 slots per launch, non-linear interpolation between levels, a derivative with
// respect to the level, evaluating a response per pixel and column instead of a bank, general mixture weights over all levels, an int32
// label input, a C driver for a piecewise fit, contexts with a communicator and glf_multi_* (handles refuse them), m > 256, a flag of
// the host program, and anything inside k_graph_synthesize, k_graph_classify and k_graph_softmax.
#include "phi_tile.hpp"
#include "phi_compact.hpp"

#include <cmath>

// the arithmetic of the epilogue is pinned operation by operation (include/glf.h): nothing here is contracted into an fma that the
// text does not spell out
#pragma clang fp contract(off)

namespace glf {

constexpr int GB_K = GLF_BLEND_MAX_SLOTS; // slots = the M index of one 32 x 32 accumulator
static_assert(GB_K == 32 && GB_K == GLF_GRAPH_MAX_OUTPUTS, "the slots fill exactly one MFMA tile, as synthesize's outputs do");
constexpr int GB_PITCH = GB_K + 1; // floats per pixel of the transposed scores: lane r's 33 r + s falls into bank (r + s) mod 32

// the per-call operand block of k_graph_blend (device): k_graph_synthesize's, then a header
//   [LD][32] float  (float)a_s[c] at [c][s], zero for s >= nout * nlevels and c >= m
//   [32] float      ident[s]
//   [32] int        plane[s] (-1: no identity term)
//   [4] int         nout, nlevels, 1 if any slot has an identity term, padding
inline size_t gb_operand_floats(unsigned ld) { return (size_t)ld * GB_K + 2 * GB_K + 4; }

// out_o[px] = the level-t(px) read-out of the scores z_s(px) = ident_s s_plane[s][px] + sum_c Phi[px][c] a_s[c], s = o nlevels + b, in one
// pass over Phi. The kernel is k_graph_classify up to and including the contraction (the same staging, chunk_contract in the same
// order, the prefetch of the next tile under the MFMAs): register g of lane (r, h) holds acc_s of pixel r for s = acc_row(g, h) -- slot
// s lives in half-wave (s >> 2) & 1 -- with glf_graph_synthesize's bits. The pixel's level is loaded before the tile's MFMAs and flies
// under them. Epilogue, in f32:
//   the wave's image of Phi is free once the last chunk is contracted (the next tile waits in registers): every lane writes its 16
//   accumulators to [pixel r][slot acc_row(g, h)] of it, pitch 33 (a half-wave's 32 stores fall into 32 banks), between two wave
//   barriers; a pixel's 32 scores then lie side by side and any of them is one indexed read -- no compare / select chain over 16
//   registers per value, no exchange between the half-waves, and no register beyond the accumulators;
//   tc = fminf(fmaxf(t, 0), nlevels - 1)  (a NaN level reads as 0);  i = min((int)tc, nlevels - 2);  f = tc - (float)i  (exact);
//   per output o, lo = o nlevels + i and hi = lo + 1: acc_lo and acc_hi by two reads of the pixel's row, the identity terms of these
//   two slots alone, z_s = plane[s] >= 0 ? fmaf(ident[s], planes[plane[s]][px], acc_s) : acc_s, with ident / plane read from LDS by
//   slot index (where no slot of the call has an identity term, a scalar test, the scores are the accumulators);
//   out = f == 0 ? z_lo : f == 1 ? z_hi : fmaf(f, z_hi, fmaf(-f, z_lo, z_lo)).
// The two scores are chosen by their index, never by arithmetic over the bank: a slot that a pixel does not take with a weight
// other than zero cannot reach it, whatever it holds. The outputs are shared between the half-waves, half h taking o = h, h + 2, ..:
// each stores 32 consecutive floats per output, synthesize's store pattern. No atomics. Rows past N are neither read nor stored,
// and level[px] is read for px < N only.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second loader, the same image).
template <int LD, class T>
__global__ __launch_bounds__(256) void k_graph_blend(const T *__restrict__ phi, int64_t N, const float *__restrict__ operand,
                                                      const float *__restrict__ planes, const float *__restrict__ level,
                                                      float *__restrict__ out)
{
    constexpr int CW = LD < 64 ? LD : 64; // columns staged per pass
    constexpr int PITCH = CW + 4;
    static_assert(32 * GB_PITCH <= 32 * PITCH, "the transposed scores fit the wave's image");
    __shared__ __attribute__((aligned(16))) float a_sh[LD * GB_K];
    __shared__ __attribute__((aligned(16))) float tile_sh[4][32 * PITCH];
    __shared__ __attribute__((aligned(8))) float2 slot_sh[GB_K]; // {ident, plane (an int)}: one read per slot
    // nout, nlevels and the has-planes flag: in LDS and made scalar per tile by a readfirstlane, not held as kernel-argument scalars
    // across the MFMA loop (as in k_graph_classify)
    __shared__ int par_sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < LD * GB_K; e += 256) a_sh[e] = operand[e];
    if (threadIdx.x < GB_K) slot_sh[threadIdx.x] = make_float2(operand[LD * GB_K + threadIdx.x], operand[LD * GB_K + GB_K + threadIdx.x]);
    if (threadIdx.x < 4) par_sh[threadIdx.x] = reinterpret_cast<const int *>(operand + LD * GB_K + 2 * GB_K)[threadIdx.x];
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    float *tw = tile_sh[wave];
    const int64_t ntiles = (N + 31) / 32, tstride = (int64_t)gridDim.x * 4;
    tile_regs<T, CW> v;
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile, lane);
    for (; tile < ntiles; tile += tstride) {
        const int64_t px = tile * 32 + r;
        const bool row = px < N; // (the same in both halves of the wave)
        const float t = row ? level[px] : 0.f; // in flight under the MFMAs
        f32x16 acc;
        acc_clear(acc);
#pragma unroll 1
        for (int ch = 0; ch < LD / CW; ++ch) {
            tile_store<CW, PITCH>(tw, v, lane);
            // the next chunk's loads fly under this chunk's MFMAs
            if (ch + 1 < LD / CW) tile_load<CW>(v, phi, LD, (ch + 1) * CW, N, tile, lane);
            else if (tile + tstride < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile + tstride, lane);
            chunk_contract<CW, GB_K>(acc, tw, a_sh + (size_t)(ch * CW) * GB_K, r, h);
        }
        // the scores, transposed: [pixel][slot] in the wave's own image (its reads above precede these writes: LDS runs in order
        // per wave, and the next tile's tile_store comes after the reads below)
        float *zr = tw + r * GB_PITCH;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int g = 0; g < 16; ++g) zr[acc_row(g, h)] = acc[g];
        __builtin_amdgcn_wave_barrier();
        const int nout = __builtin_amdgcn_readfirstlane(par_sh[0]), nlevels = __builtin_amdgcn_readfirstlane(par_sh[1]);
        const int has_planes = __builtin_amdgcn_readfirstlane(par_sh[2]);
        if (row) {
            const float tc = fminf(fmaxf(t, 0.f), (float)(nlevels - 1));
            const int it = (int)tc, i = it < nlevels - 2 ? it : nlevels - 2;
            const float f = tc - (float)i;
            for (int o = h; o < nout; o += 2) {
                const int lo = o * nlevels + i;
                float z_lo = zr[lo], z_hi = zr[lo + 1];
                if (has_planes) {
                    // a slot without a plane loads this pixel of plane 0 and does not use it: both loads are unconditional and in
                    // flight together
                    const float2 c_lo = slot_sh[lo], c_hi = slot_sh[lo + 1];
                    const int p_lo = __float_as_int(c_lo.y), p_hi = __float_as_int(c_hi.y);
                    const float x_lo = planes[(size_t)(p_lo > 0 ? p_lo : 0) * N + px], x_hi = planes[(size_t)(p_hi > 0 ? p_hi : 0) * N + px];
                    z_lo = p_lo >= 0 ? fmaf(c_lo.x, x_lo, z_lo) : z_lo;
                    z_hi = p_hi >= 0 ? fmaf(c_hi.x, x_hi, z_hi) : z_hi;
                }
                out[(size_t)o * N + px] = f == 0.f ? z_lo : f == 1.f ? z_hi : fmaf(f, z_hi, fmaf(-f, z_lo, z_lo));
            }
        }
    }
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_blend(glf_graph *g, int nout, int nlevels, const double *h_a, const float *ident, const int *plane, int nplanes,
                    const float *d_planes, const float *d_level, float *d_out)
{
    if (!g) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    if (nout < 1 || nlevels < 2 || (int64_t)nout * nlevels > GB_K)
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_blend: nout = %d, nlevels = %d outside nout >= 1, nlevels >= 2, nout * nlevels <= %d", nout,
                         nlevels, GB_K);
    if (!h_a || !plane || nplanes < 0) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_blend: h_a or plane is NULL, or nplanes < 0");
    if (!d_level || !d_out) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_blend: d_level or d_out is NULL");
    const int slots = nout * nlevels;
    bool any_plane = false;
    const int bad = ident_terms_check(slots, plane, nplanes, ident, d_planes, &any_plane);
    if (bad >= 0 && bad < slots)
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_blend: plane[%d] = %d outside -1 .. %d", bad, plane[bad], nplanes - 1);
    if (bad == slots) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_blend: identity planes without ident or d_planes");
    const unsigned ld = g->ld;
    const int64_t N = (int64_t)g->width * g->height;
    std::vector<float> h_op(gb_operand_floats(ld), 0.f);
    const std::vector<double> a = coeff_operand(g, (size_t)slots, h_a, GB_K, h_op.data());
    if (!all_fl32_finite(a.data(), a.size()))
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_blend: a coefficient (folded with its column's 2^e_c) is not finite in f32");
    GLF_ENTER(ctx);
    float *op_ident = h_op.data() + (size_t)ld * GB_K;
    ident_terms_pack(slots, ident, plane, op_ident);
    const int header[4] = {nout, nlevels, any_plane ? 1 : 0, 0};
    std::memcpy(op_ident + 2 * GB_K, header, sizeof(header));
    DevBuf<float> op;
    GLF_TRY(upload_operand(ctx, op, h_op));
    int rc = GLF_ERR_INVALID;
    dispatch_phi_ld(g, [&](auto LD, auto *phi, auto t) {
        rc = launch_tiles(g, k_graph_blend<LD.value, decltype(t)>, N, phi, N, (const float *)op.p, d_planes, d_level, d_out);
    });
    if (rc == GLF_ERR_INVALID) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_blend: ld=%u", ld);
    GLF_TRY(rc);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (h_op and op go out of scope)
    return GLF_OK;
}

} // extern "C"
