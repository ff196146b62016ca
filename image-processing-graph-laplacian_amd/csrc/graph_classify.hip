// graph_classify.hip -- label read-out on a graph handle: the k <= GLF_CLASSIFY_MAX score planes ident_j s_j + Phi a_j (+ bias_j) of
// glf_graph_synthesize are formed in registers in one pass over Phi (k_graph_classify) and reduced per pixel to the winning class,
// its score and its margin over the runner-up; the planes themselves are never written. Scribble propagation, the label map of
// graph-smoothed logits and the per-pixel choice among depth hypotheses all end in this step. The contraction is
// k_graph_synthesize's; the new part is the epilogue.
// Out of scope: per-class counts, k > 32 and merging across groups, a label input to the projection, contexts with a communicator
// and glf_multi_* (handles refuse them), m > 256, a flag of the host program, and anything inside k_graph_synthesize,
// k_graph_cluster and k_graph_quadform. (Softmax confidences and mean-field iterations: graph_softmax.hip.)
#include "phi_tile.hpp"
#include "phi_compact.hpp"

#include <cmath>

// the arithmetic of the epilogue is pinned operation by operation (include/glf.h): nothing here is contracted into an fma that the
// text does not spell out
#pragma clang fp contract(off)

namespace glf {

constexpr int GY_K = GLF_CLASSIFY_MAX; // classes = the M index of one 32 x 32 accumulator
static_assert(GY_K == 32 && GY_K == GLF_GRAPH_MAX_OUTPUTS, "the classes fill exactly one MFMA tile, as synthesize's outputs do");

// the per-call operand block of k_graph_classify (device): k_graph_synthesize's, then the biases
//   [LD][32] float  (float)a_j[c] at [c][j], zero for j >= k and c >= m
//   [32] float      ident[j]
//   [32] int        plane[j] (-1: no identity term)
//   [32] float      fl32(bias_j), zero for j >= k and where there is no bias
//   [4] int         [0]: GY_BIAS if the biases are added (h_bias was given) | GY_PLANES if any class has an identity term; the rest padding
inline size_t gy_operand_floats(unsigned ld) { return (size_t)ld * GY_K + 3 * GY_K + 4; }
enum { GY_BIAS = 1, GY_PLANES = 2 };

// the running top two of one lane: score s of class j after the classes before it (ascending j), strict >, so that a NaN never
// enters, the first of equal scores keeps the label and the second of them becomes the runner-up:
//   if (s > best) { second = best; best = s; label = j; } else if (s > second) second = s;
// written as selects; on: the slot takes part (j < k), otherwise nothing changes whatever s holds
__device__ __forceinline__ void top2_take(float &best, int &label, float &second, float s, int j, bool on)
{
    const bool first = on && s > best, runner = on && s > second;
    second = first ? best : runner ? s : second;
    label = first ? j : label;
    best = first ? s : best;
}

// label / best / margin of the scores z_j(px) = ident_j s_plane[j][px] + sum_c Phi[px][c] a_j[c] (+ bias_j), j < k, in one pass over
// Phi. The kernel is k_graph_synthesize up to and including the contraction (the same staging, chunk_contract in the same order, the
// prefetch of the next tile under the MFMAs): register g of lane (r, h) holds acc_j of pixel r for j = acc_row(g, h), with
// glf_graph_synthesize's bits. Epilogue, all lanes, in f32:
//   z_j = plane[j] >= 0 ? fmaf(ident[j], planes[plane[j]][px], acc_j) : acc_j   (synthesize's output j, bit for bit; the planes'
//         values are loaded before the scan, all in flight together, a class without a plane loading plane 0's and dropping it)
//   score_j = has_bias ? z_j + bias_j : z_j                                      (one f32 addition)
//   per lane (best, label, second) = (-inf, 0, -inf), then top2_take over g ascending -- ascending j within the half -- for the
//   slots j < k only (masked by index: whatever a slot >= k holds, it changes nothing). Register g holds class (g & 3) + 8 (g >> 2)
//   in half 0 and that + 4 in half 1: a register whose two classes are both >= k is skipped by a scalar branch, so the epilogue
//   costs what k classes cost; without identity planes and bias (a scalar test of the flags) the scores are the accumulators;
//   one __shfl_xor(.., 32) of the three values; with (b0, l0, s0) the lane's own and (b1, l1, s1) the other half's, the other half
//   wins if b1 > b0 or (b1 == b0 and l1 < l0), and second = max(min(b0, b1), max(s0, s1)) (no NaN reaches here); both halves hold
//   the same result;
//   margin = best == second ? +0 : best - second                                (one f32 subtraction; +inf where second = -inf)
// and half 0 stores the outputs that were asked for. No atomics. Rows past N are neither read nor stored.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second loader, the same image).
template <int LD, class T>
__global__ __launch_bounds__(256) void k_graph_classify(const T *__restrict__ phi, int64_t N, int k, const float *__restrict__ operand,
                                                         const float *__restrict__ planes, int32_t *__restrict__ label_out,
                                                         float *__restrict__ best_out, float *__restrict__ margin_out)
{
    constexpr int CW = LD < 64 ? LD : 64; // columns staged per pass
    constexpr int PITCH = CW + 4;
    __shared__ __attribute__((aligned(16))) float a_sh[LD * GY_K];
    __shared__ __attribute__((aligned(16))) float tile_sh[4][32 * PITCH];
    __shared__ __attribute__((aligned(16))) float4 class_sh[GY_K]; // {ident, plane (an int), bias, -}: one read per class
    __shared__ int flags_sh; // (in LDS, not a kernel-argument scalar: the widest f32 instance is short of scalar registers)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < LD * GY_K; e += 256) a_sh[e] = operand[e];
    if (threadIdx.x < GY_K)
        class_sh[threadIdx.x] = make_float4(operand[LD * GY_K + threadIdx.x], operand[LD * GY_K + GY_K + threadIdx.x],
                                            operand[LD * GY_K + 2 * GY_K + threadIdx.x], 0.f);
    if (threadIdx.x == 0) flags_sh = reinterpret_cast<const int *>(operand + LD * GY_K + 3 * GY_K)[0];
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    float *tw = tile_sh[wave];
    const int64_t ntiles = (N + 31) / 32, tstride = (int64_t)gridDim.x * 4;
    tile_regs<T, CW> v;
    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile, lane);
    for (; tile < ntiles; tile += tstride) {
        f32x16 acc;
        acc_clear(acc);
#pragma unroll 1
        for (int ch = 0; ch < LD / CW; ++ch) {
            tile_store<CW, PITCH>(tw, v, lane);
            // the next chunk's loads fly under this chunk's MFMAs
            if (ch + 1 < LD / CW) tile_load<CW>(v, phi, LD, (ch + 1) * CW, N, tile, lane);
            else if (tile + tstride < ntiles) tile_load<CW>(v, phi, LD, 0, N, tile + tstride, lane);
            chunk_contract<CW, GY_K>(acc, tw, a_sh + (size_t)(ch * CW) * GY_K, r, h);
        }
        const int64_t px = tile * 32 + r;
        const bool row = px < N; // (the same in both halves of the wave)
        float best = -INFINITY, second = -INFINITY;
        int label = 0;
        const int flags = __builtin_amdgcn_readfirstlane(flags_sh);
        // register g takes part in this lane where acc_row(g, 0) < k - 4 h. (Formed anew per tile behind an empty asm: as a loop
        // invariant the compiler keeps the 16 comparisons' masks in scalar registers across the MFMA loop and runs out of them.)
        int klane = k - 4 * h;
        asm volatile("" : "+v"(klane));
        if (row) {
            // label holds acc_row(g, 0) of the winning register, an immediate; the half's 4 h is added once at the end
            if (flags == 0) {
#pragma unroll
                for (int g = 0; g < 16; ++g)
                    if (acc_row(g, 0) < k) top2_take(best, label, second, acc[g], acc_row(g, 0), acc_row(g, 0) < klane);
            } else {
                // the identity planes' values first, all loads in flight together: a class without a plane (and a slot >= k: its
                // plane is -1) loads this pixel of plane 0 and does not use it -- an unconditional load the compiler can issue early
                float x[16];
#pragma unroll
                for (int g = 0; g < 16; ++g) x[g] = 0.f;
                if (flags & GY_PLANES) {
#pragma unroll
                    for (int g = 0; g < 16; ++g)
                        if (acc_row(g, 0) < k) {
                            const int pl = __float_as_int(class_sh[acc_row(g, h)].y);
                            x[g] = planes[(size_t)(pl > 0 ? pl : 0) * N + px];
                        }
                }
#pragma unroll
                for (int g = 0; g < 16; ++g)
                    if (acc_row(g, 0) < k) {
                        const float4 c = class_sh[acc_row(g, h)];
                        float z = acc[g];
                        z = __float_as_int(c.y) >= 0 ? fmaf(c.x, x[g], z) : z;
                        if (flags & GY_BIAS) z = z + c.z;
                        top2_take(best, label, second, z, acc_row(g, 0), acc_row(g, 0) < klane);
                    }
            }
            label = best > -INFINITY ? label + 4 * h : 0; // (a lane that took nothing keeps label 0)
        }
        const float b1 = __shfl_xor(best, 32), s1 = __shfl_xor(second, 32);
        const int l1 = __shfl_xor(label, 32);
        const float lo = fminf(best, b1), hi2 = fmaxf(second, s1);
        if (b1 > best || (b1 == best && l1 < label)) {
            best = b1;
            label = l1;
        }
        second = fmaxf(lo, hi2);
        if (row && h == 0) {
            if (label_out) label_out[px] = label;
            if (best_out) best_out[px] = best;
            if (margin_out) margin_out[px] = best == second ? 0.f : best - second;
        }
    }
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_classify(glf_graph *g, int k, const double *h_a, const float *ident, const int *plane, int nplanes, const float *d_planes,
                       const double *h_bias, int32_t *d_label, float *d_best, float *d_margin)
{
    if (!g) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    if (k < 1 || k > GY_K) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_classify: k = %d outside 1 .. %d", k, GY_K);
    if (!h_a || !plane || nplanes < 0) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_classify: h_a or plane is NULL, or nplanes < 0");
    if (!d_label && !d_best && !d_margin) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_classify: no output was asked for");
    bool any_plane = false;
    const int bad = ident_terms_check(k, plane, nplanes, ident, d_planes, &any_plane);
    if (bad >= 0 && bad < k)
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_classify: plane[%d] = %d outside -1 .. %d", bad, plane[bad], nplanes - 1);
    if (bad == k) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_classify: identity planes without ident or d_planes");
    const unsigned ld = g->ld;
    const int64_t N = (int64_t)g->width * g->height;
    std::vector<float> h_op(gy_operand_floats(ld), 0.f);
    const std::vector<double> a = coeff_operand(g, (size_t)k, h_a, GY_K, h_op.data());
    if (!all_fl32_finite(a.data(), a.size()))
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_classify: a coefficient (folded with its column's 2^e_c) is not finite in f32");
    if (h_bias && !all_fl32_finite(h_bias, (size_t)k)) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_classify: a bias is not finite in f32");
    GLF_ENTER(ctx);
    float *op_ident = h_op.data() + (size_t)ld * GY_K, *op_bias = op_ident + 2 * GY_K;
    ident_terms_pack(k, ident, plane, op_ident);
    for (int j = 0; h_bias && j < k; ++j) op_bias[j] = (float)h_bias[j];
    const int flags[4] = {(h_bias ? GY_BIAS : 0) | (any_plane ? GY_PLANES : 0), 0, 0, 0};
    std::memcpy(op_bias + GY_K, flags, sizeof(flags));
    DevBuf<float> op;
    GLF_TRY(upload_operand(ctx, op, h_op));
    int rc = GLF_ERR_INVALID;
    dispatch_phi_ld(g, [&](auto LD, auto *phi, auto t) {
        rc = launch_tiles(g, k_graph_classify<LD.value, decltype(t)>, N, phi, N, k, (const float *)op.p, d_planes, d_label, d_best, d_margin);
    });
    if (rc == GLF_ERR_INVALID) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_classify: ld=%u", ld);
    GLF_TRY(rc);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (h_op and op go out of scope)
    return GLF_OK;
}

} // extern "C"
