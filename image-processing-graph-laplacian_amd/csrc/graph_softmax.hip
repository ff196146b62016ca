// graph_softmax.hip -- softmax read-out on a graph handle: the k <= GLF_SOFTMAX_MAX score planes ident_j s_j + Phi a_j (+ bias_j) of
// glf_graph_classify are formed in registers in one pass over Phi (k_graph_softmax) and turned per pixel into the class
// probabilities p_j = exp(beta score_j) / sum_i exp(beta score_i), the log-sum-exp and the entropy; the scores themselves are never
// written. Per-pixel class probabilities, an uncertainty map, the soft memberships of a set of centres and one mean-field step of a
// dense CRF all end in this step. The contraction is k_graph_synthesize's, the scores are k_graph_classify's; the new part is the
// epilogue after them.
// Out of scope: k > 32 and merging across groups, unit-length rows in the memberships, subtracting the self-message of a mean-field
// step, a C driver for mean field, fusing the re-projection of the probabilities into this pass, repairing the scale of Phi's sample
// rows, contexts with a communicator and glf_multi_* (handles refuse them), m > 256, a flag of the host program, and anything inside
// k_graph_synthesize and k_graph_classify.
#include "phi_tile.hpp"
#include "phi_compact.hpp"

#include <cmath>

// the arithmetic of the epilogue is pinned operation by operation (include/glf.h): nothing here is contracted into an fma that the
// text does not spell out
#pragma clang fp contract(off)

namespace glf {

constexpr int GX_K = GLF_SOFTMAX_MAX; // classes = the M index of one 32 x 32 accumulator
static_assert(GX_K == 32 && GX_K == GLF_GRAPH_MAX_OUTPUTS, "the classes fill exactly one MFMA tile, as synthesize's outputs do");

// the per-call operand block of k_graph_softmax (device): k_graph_classify's, the last four words holding the scalars
//   [LD][32] float  (float)a_j[c] at [c][j], zero for j >= k and c >= m
//   [32] float      ident[j]
//   [32] int        plane[j] (-1: no identity term)
//   [32] float      fl32(bias_j), zero for j >= k and where there is no bias
//   [4] word        int GX_BIAS if the biases are added (h_bias was given) | GX_PLANES if any class has an identity term;
//                   float beta2 = fl32(beta log2 e); float fl32(beta); padding
inline size_t gx_operand_floats(unsigned ld) { return (size_t)ld * GX_K + 3 * GX_K + 4; }
enum { GX_BIAS = 1, GX_PLANES = 2 };

constexpr float GX_LN2 = 0.693147182464599609375f; // fl32(ln 2)

__device__ __forceinline__ float *lds_pointer(unsigned long long p) // a wave-uniform pointer read from LDS, as a scalar
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)p), hi = __builtin_amdgcn_readfirstlane((int)(unsigned)(p >> 32));
    return reinterpret_cast<float *>(((unsigned long long)hi << 32) | lo);
}

// p_j / lse / entropy of the scores score_j(px) = ident_j s_plane[j][px] + sum_c Phi[px][c] a_j[c] (+ bias_j), j < k, in one pass over
// Phi. The kernel is k_graph_classify up to and including the scores (the same staging, chunk_contract in the same order, the prefetch
// of the next tile under the MFMAs, the identity planes' values loaded together ahead of their use): register g of lane (r, h) holds
// score_j of pixel r for j = acc_row(g, h), with glf_graph_classify's bits. Epilogue, all lanes, in f32, register g of a lane taking
// part where its class is < k, masked by index: a register whose two classes are both >= k is skipped by a scalar branch, and a slot
// >= k beside a class < k in the other half-wave is set to -inf once and runs the same operations (it never becomes best, its e is
// +0, and S + (+0) and fmaf(+0, 0, A) change no bit of S and A, which are never -0), so that no per-register mask outlives the scores:
//   best = -inf; over g ascending: if (score > best) best = score;  one __shfl_xor(.., 32): if (other > best) best = other
//   per g ascending: d = score - best; t = beta2 * d; e = v_exp_f32(t); S = S + e; A = fmaf(e, e > 0 ? t : 0, A)   (S, A from +0;
//        A only where the entropy is asked for; e takes the score's place in the register)
//   S = S + __shfl_xor(S, 32); A = A + __shfl_xor(A, 32)                        (the same bits in both halves)
//   r = 1 / S (IEEE division); p_j = e_j * r, stored by the half-wave that holds class j: 32 consecutive floats per register,
//   synthesize's store pattern, the address a scalar plane base plus one per-lane offset formed per tile
//   L = v_log_f32(S); lse = fmaf(fl32(ln 2), L, fl32(beta) * best); entropy = fl32(ln 2) * (L - A * r), stored by half 0.
// The 16 v_exp_f32 of a lane come after its tile's MFMAs: a quarter-rate instruction costs an issue slot beside MFMAs and nothing
// more, and with two or more waves on a SIMD the other waves' MFMAs run under them (16 exps against LD / 2 MFMAs of 16 passes).
// No atomics. Rows past N are neither read nor stored; their lanes run the arithmetic on zeros. An output that was not asked for is
// not computed or touched.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second loader, the same image).
template <int LD, class T>
__global__ __launch_bounds__(256) void k_graph_softmax(const T *__restrict__ phi, int64_t N, int k, const float *__restrict__ operand,
                                                        const float *__restrict__ planes, float *prob_arg, float *lse_arg,
                                                        float *entropy_arg)
{
    constexpr int CW = LD < 64 ? LD : 64; // columns staged per pass
    constexpr int PITCH = CW + 4;
    __shared__ __attribute__((aligned(16))) float a_sh[LD * GX_K];
    __shared__ __attribute__((aligned(16))) float tile_sh[4][32 * PITCH];
    __shared__ __attribute__((aligned(16))) float4 class_sh[GX_K]; // {ident, plane (an int), bias, -}: one read per class
    // flags, beta2, beta and the three output pointers: in LDS and made scalar per tile by a readfirstlane, not held as
    // kernel-argument scalars across the MFMA loop (the widest f32 instances are short of scalar registers)
    __shared__ int par_sh[4];
    __shared__ unsigned long long out_sh[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < LD * GX_K; e += 256) a_sh[e] = operand[e];
    if (threadIdx.x < GX_K)
        class_sh[threadIdx.x] = make_float4(operand[LD * GX_K + threadIdx.x], operand[LD * GX_K + GX_K + threadIdx.x],
                                            operand[LD * GX_K + 2 * GX_K + threadIdx.x], 0.f);
    if (threadIdx.x < 4) par_sh[threadIdx.x] = reinterpret_cast<const int *>(operand + LD * GX_K + 3 * GX_K)[threadIdx.x];
    if (threadIdx.x == 0) {
        out_sh[0] = reinterpret_cast<unsigned long long>(prob_arg);
        out_sh[1] = reinterpret_cast<unsigned long long>(lse_arg);
        out_sh[2] = reinterpret_cast<unsigned long long>(entropy_arg);
    }
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
            chunk_contract<CW, GX_K>(acc, tw, a_sh + (size_t)(ch * CW) * GX_K, r, h);
        }
        const int64_t px = tile * 32 + r;
        const bool row = px < N; // (the same in both halves of the wave)
        const int flags = __builtin_amdgcn_readfirstlane(par_sh[0]);
        const float beta2 = __int_as_float(__builtin_amdgcn_readfirstlane(par_sh[1]));
        float *__restrict__ const prob_out = lds_pointer(out_sh[0]);
        float *__restrict__ const lse_out = lds_pointer(out_sh[1]);
        float *__restrict__ const entropy_out = lds_pointer(out_sh[2]);
        // register g takes part in this lane where acc_row(g, 0) < k - 4 h (formed anew per tile behind an empty asm, as in
        // k_graph_classify: as loop invariants the 16 masks would sit in scalar registers across the MFMA loop)
        int klane = k - 4 * h;
        asm volatile("" : "+v"(klane));
        if (flags != 0) {
            // classify's scores: the identity planes' values first, all loads in flight together (a class without a plane, and a
            // slot >= k, loads this pixel of plane 0 and does not use it)
            float x[16];
#pragma unroll
            for (int g = 0; g < 16; ++g) x[g] = 0.f;
            if ((flags & GX_PLANES) && row) {
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
                    if (flags & GX_BIAS) z = z + c.z;
                    acc[g] = z;
                }
        }
        // a slot >= k beside a class < k in the register's other half runs on a score of -inf from here on: it never becomes best, its
        // e is +0 (or a NaN where the pixel's outputs are NaN anyway) and changes no bit of S and A
#pragma unroll
        for (int g = 0; g < 16; ++g)
            if (acc_row(g, 0) < k) acc[g] = acc_row(g, 0) < klane ? acc[g] : -INFINITY;
        float best = -INFINITY;
#pragma unroll
        for (int g = 0; g < 16; ++g)
            if (acc_row(g, 0) < k) best = acc[g] > best ? acc[g] : best;
        {
            const float b1 = __shfl_xor(best, 32);
            best = b1 > best ? b1 : best;
        }
        float S = 0.f, A = 0.f;
        if (entropy_out) {
#pragma unroll
            for (int g = 0; g < 16; ++g)
                if (acc_row(g, 0) < k) {
                    const float d = acc[g] - best;
                    const float t = beta2 * d;
                    const float e = __builtin_amdgcn_exp2f(t);
                    S = S + e;
                    A = fmaf(e, e > 0.f ? t : 0.f, A);
                    acc[g] = e;
                }
            A = A + __shfl_xor(A, 32);
        } else {
#pragma unroll
            for (int g = 0; g < 16; ++g)
                if (acc_row(g, 0) < k) {
                    const float d = acc[g] - best;
                    const float t = beta2 * d;
                    const float e = __builtin_amdgcn_exp2f(t);
                    S = S + e;
                    acc[g] = e;
                }
        }
        S = S + __shfl_xor(S, 32);
        const float rs = 1.0f / S;
        if (prob_out && row) {
            // plane acc_row(g, 0) is a scalar base; the lane's part (its half's four planes, its pixel) is formed per tile behind an
            // empty asm, so that no per-class address is carried across the MFMA loop
            int kstore = k - 4 * h;
            int64_t lane_off = (int64_t)(4 * h) * N + px;
            asm volatile("" : "+v"(kstore), "+v"(lane_off));
            float *base = prob_out; // planes 8 q .. 8 q + 3 of register group q; opaque per group, so that four bases are live at a time
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                asm volatile("" : "+s"(base));
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (8 * q + i < k && 8 * q + i < kstore) (base + (size_t)i * N)[lane_off] = acc[4 * q + i] * rs;
                base += (size_t)8 * N;
            }
        }
        if (row && h == 0 && (lse_out || entropy_out)) {
            const float L = __builtin_amdgcn_logf(S);
            if (lse_out) {
                const float beta = __int_as_float(__builtin_amdgcn_readfirstlane(par_sh[2]));
                lse_out[px] = fmaf(GX_LN2, L, beta * best);
            }
            if (entropy_out) entropy_out[px] = GX_LN2 * (L - A * rs);
        }
    }
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_softmax(glf_graph *g, int k, const double *h_a, const float *ident, const int *plane, int nplanes, const float *d_planes,
                      const double *h_bias, double beta, float *d_prob, float *d_lse, float *d_entropy)
{
    if (!g) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    if (k < 1 || k > GX_K) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_softmax: k = %d outside 1 .. %d", k, GX_K);
    if (!h_a || !plane || nplanes < 0) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_softmax: h_a or plane is NULL, or nplanes < 0");
    if (!d_prob && !d_lse && !d_entropy) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_softmax: no output was asked for");
    const float beta32 = (float)beta, beta2 = (float)(beta * 1.4426950408889634074 /* log2 e */);
    if (!(beta32 > 0.f) || !std::isfinite(beta32) || !std::isfinite(beta2))
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_softmax: beta = %g is not finite and positive in f32, or beta log2 e is not finite in f32", beta);
    bool any_plane = false;
    const int bad = ident_terms_check(k, plane, nplanes, ident, d_planes, &any_plane);
    if (bad >= 0 && bad < k)
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_softmax: plane[%d] = %d outside -1 .. %d", bad, plane[bad], nplanes - 1);
    if (bad == k) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_softmax: identity planes without ident or d_planes");
    const unsigned ld = g->ld;
    const int64_t N = (int64_t)g->width * g->height;
    std::vector<float> h_op(gx_operand_floats(ld), 0.f);
    const std::vector<double> a = coeff_operand(g, (size_t)k, h_a, GX_K, h_op.data());
    if (!all_fl32_finite(a.data(), a.size()))
        return set_error(ctx, GLF_ERR_INVALID, "glf_graph_softmax: a coefficient (folded with its column's 2^e_c) is not finite in f32");
    if (h_bias && !all_fl32_finite(h_bias, (size_t)k)) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_softmax: a bias is not finite in f32");
    GLF_ENTER(ctx);
    float *op_ident = h_op.data() + (size_t)ld * GX_K, *op_bias = op_ident + 2 * GX_K;
    ident_terms_pack(k, ident, plane, op_ident);
    for (int j = 0; h_bias && j < k; ++j) op_bias[j] = (float)h_bias[j];
    const int flags = (h_bias ? GX_BIAS : 0) | (any_plane ? GX_PLANES : 0);
    std::memcpy(op_bias + GX_K, &flags, sizeof(flags));
    op_bias[GX_K + 1] = beta2;
    op_bias[GX_K + 2] = beta32;
    DevBuf<float> op;
    GLF_TRY(upload_operand(ctx, op, h_op));
    int rc = GLF_ERR_INVALID;
    dispatch_phi_ld(g, [&](auto LD, auto *phi, auto t) {
        rc = launch_tiles(g, k_graph_softmax<LD.value, decltype(t)>, N, phi, N, k, (const float *)op.p, d_planes, d_prob, d_lse, d_entropy);
    });
    if (rc == GLF_ERR_INVALID) return set_error(ctx, GLF_ERR_INVALID, "glf_graph_softmax: ld=%u", ld);
    GLF_TRY(rc);
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (h_op and op go out of scope)
    return GLF_OK;
}

} // extern "C"
