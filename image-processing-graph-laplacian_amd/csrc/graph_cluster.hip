// graph_cluster.hip -- spectral segmentation on a graph handle: k-means over the rows of Phi. One Lloyd iteration is one pass over
// Phi (k_graph_cluster: the assignment on k_graph_synthesize's MFMA shape, the per-label sums on k_graph_normal's), driven by
// glf_graph_cluster_step[_ex] and glf_graph_segment[_ex]; the host-only centroid update and k-means++ seeding are in host_util.cpp.
// Unit-length rows (the row-normalised embedding of Ng, Jordan and Weiss) and per-pixel weights are compile-time modes of that one
// kernel, chosen from the embedding the _ex entry points take; a plain embedding runs the plain mode.
// Out of scope: spherical k-means (renormalised centroids), a margin or confidence output, more than 64 embedding columns, k > 32,
// contexts with a communicator and glf_multi_* (handles refuse them), a flag of the host program, and anything inside k_band,
// k_graph_synthesize and k_graph_normal.
#include "phi_tile.hpp"
#include "phi_compact.hpp"

#include <algorithm>
#include <cmath>

namespace glf {

constexpr int GC_K = GLF_CLUSTER_MAX; // centroids = the M index of one 32 x 32 accumulator
static_assert(GC_K == 32, "the centroids fill exactly one MFMA tile");

// The modes of k_graph_cluster: the embedding is e(px) = rinv(px) scale o Phi[px], and pixel px enters the update with weight w(px).
//   GC_PLAIN   rinv = 1, w = 1
//   GC_WEIGHT  rinv = 1, w = the weight plane
//   GC_NORM    rinv = 1 / |scale o Phi[px]| (unit-length rows), w = the weight plane, or 1 where there is none (a run-time NULL check)
enum { GC_PLAIN = 0, GC_WEIGHT = 1, GC_NORM = 2, GC_MODES = 3 };

// the per-call operand block of k_graph_cluster (device):
//   [CW][32] float  fl32(scale_c cent_j[c]) at [c][j], zero for j >= k and c >= dim
//   [32] float      fl32(|cent_j|^2), zero for j >= k
//   [CW] float      fl32(scale_c), zero for c >= dim (GC_NORM only)
inline int gc_cw(unsigned ld) { return ld < 64 ? 32 : 64; }
inline size_t gc_operand_floats(int cw, int mode) { return (size_t)cw * GC_K + GC_K + (mode == GC_NORM ? cw : 0); }
// one workgroup's partial: [CW / 32][32 labels][32 columns] sums, then the tail of doubles: counts [32], changed, zero padding up to
// 64, and outside GC_PLAIN the mass [32]
constexpr int gc_tail(int mode) { return mode == GC_PLAIN ? 64 : 96; }
inline size_t gc_part_cols(int cw, int mode) { return (size_t)(cw / 32) * 1024 + gc_tail(mode); }

// One Lloyd iteration in one pass over the first CW columns of Phi (row pitch ld floats), on the padded image of phi_tile.hpp.
// Assignment: chunk_contract with the centroids as the M index (A: the operand block, from LDS) and the pixels as the N index:
// k_graph_synthesize's contraction order, every score its own fma chain. Register g of lane (r, h) then holds the dot product of pixel
// r with centroid j = acc_row(g, h); score = fmaf(-2 rinv, dot, |c_j|^2) (|e|^2 is the same for every j and is not formed). Each lane
// takes the argmin of its 16 registers in ascending j with a strict < (j >= k carries a bias of +inf and never wins), one exchange
// with the other half-wave decides between the two, the lower index winning a tie.
// Update: the wave's 32 labels go to LDS (-1 for rows past N), then the same MFMA with the pixels as the contraction index: at step
// u lane (r, h) gives A = (label[2u + h] == r ? t[2u + h] : 0), t(px) = fl32(w(px) rinv(px)), and B = Phi[2u + h][r] (and [32 + r])
// from the same image; the label is one address per group, a broadcast. sums_j = sum w rinv Phi[px][c] over the members of j, under
// the chain rule and the four-wave reduction of phi_tile.hpp. Lane (r, h) counts its own hits: the members of label r among the
// pixels of parity h, an exact integer; the lanes of half 0 count the labels that differ from prev.
// Rows past N are neither labelled nor counted. prev may be labels itself: a lane reads prev[px] before it writes labels[px], and no
// other lane touches that pixel.
// What the modes change (MODE is a template argument, nothing of another mode is left in an instance):
//   GC_PLAIN keeps the 16 biases |c_j|^2 of a lane in registers; t = 1, so A is 1 or 0 and the products are exact. In the other modes
//   the biases are read from LDS at every tile (bias_sh, +inf for j >= k; registers 4 q .. 4 q + 3 hold 16 consecutive bytes): with
//   them in registers, GC_NORM at CW 64 spilled 5 registers (profiles/graph_cluster_nw_kernel_resources.txt). The values, and so
//   every score's bits, are the same;
//   GC_NORM: lane (r, h) forms the squared length of its half row of pixel r from the float4s it reads anyway,
//   n2 = fmaf(x, x, n2), x = fl32(scale_c) phi_c (the scales in LDS, s_sh), in ascending column order; the halves are added through one
//   __shfl_xor(.., 32) (a commutative sum: both half-waves hold the same bits) and rinv = n2 > 0 ? 1 / sqrtf(n2) : 0 (a run-time
//   branch inside the unrolled contraction would cut it into one basic block per four MFMAs, and the LDS reads of the next step
//   would no longer be issued under the MFMAs of this one);
//   GC_WEIGHT and GC_NORM: t(px) and w(px) go to LDS beside the tile's 32 labels (w is loaded with the prefetch of the next tile,
//   as prev is), and lane (r, h) adds (double) w[p] over its hits: the mass of label r among the pixels of parity h. Counts and
//   changed stay integers.
// T: the element type of Phi (float, or __half on a compact handle: phi_tile.hpp's second loader, the same image).
template <int CW, int MODE, class T = float>
__global__ __launch_bounds__(256, 2) void k_graph_cluster(const T *__restrict__ phi, int64_t N, int ld, int k, const float *__restrict__ operand,
                                                          const float *__restrict__ weight, const int32_t *prev, int32_t *labels,
                                                          double *__restrict__ part)
{
    constexpr int PITCH = CW + 4;
    constexpr int NT = CW / 32;   // accumulator tiles of the sums
    constexpr int RW = 32 * PITCH > 2048 ? 32 * PITCH : 2048; // floats of a wave's region (>= one f64 tile for the epilogue)
    constexpr int TAIL = gc_tail(MODE);
    __shared__ __attribute__((aligned(16))) float a_sh[CW * GC_K];
    __shared__ __attribute__((aligned(16))) float region[4][RW];
    __shared__ __attribute__((aligned(16))) float s_sh[CW];      // GC_NORM
    __shared__ __attribute__((aligned(16))) float bias_sh[GC_K]; // not GC_PLAIN, as are t_sh, w_sh and mass_sh
    __shared__ int lab_sh[4][32];
    __shared__ float t_sh[4][32], w_sh[4][32];
    __shared__ unsigned cnt_sh[4][64], chg_sh[4][64];
    __shared__ double mass_sh[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    for (int e = threadIdx.x; e < CW * GC_K; e += 256) a_sh[e] = operand[e];
    auto centroid_of = [&](int g) { return acc_row(g, h); }; // the centroid of accumulator register g of this lane
    float bias[16];
    if constexpr (MODE == GC_PLAIN) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int j = centroid_of(g);
            bias[g] = j < k ? operand[CW * GC_K + j] : INFINITY;
        }
    } else if (threadIdx.x < GC_K)
        bias_sh[threadIdx.x] = (int)threadIdx.x < k ? operand[CW * GC_K + threadIdx.x] : INFINITY;
    if constexpr (MODE == GC_NORM)
        if (threadIdx.x < CW) s_sh[threadIdx.x] = operand[CW * GC_K + GC_K + threadIdx.x];
    __syncthreads();
    auto bias_of = [&](int g) {
        if constexpr (MODE == GC_PLAIN) return bias[g];
        else return bias_sh[centroid_of(g)];
    };
    float *tw = region[wave];
    const int *lab = lab_sh[wave];
    const int64_t ntiles = (N + 31) / 32, tstride = (int64_t)gridDim.x * 4;

    f32x16 acc[NT];
    double dacc[NT][16];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            acc[t][g] = 0.f;
            dacc[t][g] = 0.0;
        }
    unsigned cnt = 0, chg = 0;
    double mass = 0.0;

    // what this lane stages of a tile: rows past N as zeros
    tile_regs<T, CW> v;
    int pv = 0;
    float wv = 1.f;
    auto load_tile = [&](int64_t tile) {
        const int64_t base = tile * 32;
        tile_load<CW>(v, phi, ld, 0, N, tile, lane);
        if constexpr (MODE == GC_PLAIN) { // (prev first: with the other order the plain tile loop gains scalar work per tile)
            if (prev && h == 0 && base + r < N) pv = prev[base + r];
        } else if (h == 0 && base + r < N) {
            if (prev) pv = prev[base + r];
            if (weight) wv = weight[base + r];
        }
    };

    int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile < ntiles) load_tile(tile);
    int chained = 0; // tiles in the running f32 chains
    for (; tile < ntiles; tile += tstride) {
        tile_store<CW, PITCH>(tw, v, lane);
        const int pv_cur = pv;
        const float wv_cur = wv;
        // the next tile's loads fly under this tile's MFMAs
        if (tile + tstride < ntiles) load_tile(tile + tstride);

        f32x16 sc;
        acc_clear(sc);
        float n2 = 0.f;
        if constexpr (MODE == GC_NORM)
            chunk_contract<CW, GC_K>(sc, tw, a_sh, r, h, [&](int u, const float4 &b) {
                const float4 s = *reinterpret_cast<const float4 *>(s_sh + h * (CW / 2) + 4 * u);
                const float x0 = s.x * b.x, x1 = s.y * b.y, x2 = s.z * b.z, x3 = s.w * b.w;
                n2 = fmaf(x0, x0, n2);
                n2 = fmaf(x1, x1, n2);
                n2 = fmaf(x2, x2, n2);
                n2 = fmaf(x3, x3, n2);
            });
        else
            chunk_contract<CW, GC_K>(sc, tw, a_sh, r, h);
        float rinv = 1.f;
        if constexpr (MODE == GC_NORM) {
            n2 += __shfl_xor(n2, 32);
            rinv = n2 > 0.f ? 1.f / sqrtf(n2) : 0.f;
        }
        const float m2 = -2.f * rinv;
        // half 0 always holds centroid 0 < k, so a label is in [0, k) even if no comparison holds
        float best = INFINITY;
        int bj = h ? 0x7fffffff : 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const float s = fmaf(m2, sc[g], bias_of(g));
            if (s < best) {
                best = s;
                bj = centroid_of(g);
            }
        }
        const float ob = __shfl_xor(best, 32);
        const int oj = __shfl_xor(bj, 32);
        if (ob < best || (ob == best && oj < bj)) bj = oj;
        const int64_t px = tile * 32 + r;
        if (h == 0) {
            const bool live = px < N;
            lab_sh[wave][r] = live ? bj : -1;
            if constexpr (MODE != GC_PLAIN) {
                t_sh[wave][r] = wv_cur * rinv;
                w_sh[wave][r] = wv_cur;
            }
            if (live) {
                if (prev) chg += pv_cur != bj;
                labels[px] = bj;
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int p = 2 * u + h;
            const bool hit = lab[p] == r;
            float tp = 1.f, wp = 0.f;
            if constexpr (MODE != GC_PLAIN) tp = t_sh[wave][p], wp = w_sh[wave][p]; // (read whatever hit is: a branch here would cut the MFMA chain into blocks of two)
            const float a = hit ? tp : 0.f;
            cnt += hit;
            if constexpr (MODE != GC_PLAIN) mass += (double)(hit ? wp : 0.f);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, tw[p * PITCH + r], acc[0], 0, 0, 0);
            if constexpr (NT == 2) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, tw[p * PITCH + 32 + r], acc[1], 0, 0, 0);
        }
        if (++chained == CHAIN_TILES) {
            chain_flush(acc, dacc);
            chained = 0;
        }
    }
    chain_flush(acc, dacc);

    double *const pout = part + (size_t)blockIdx.x * (NT * 1024 + TAIL);
    wave_tiles_reduce(region, dacc, wave, r, h, [&](int t, int e, double s) { pout[(size_t)t * 1024 + e] = s; });
    cnt_sh[wave][lane] = cnt;
    chg_sh[wave][lane] = chg;
    if constexpr (MODE != GC_PLAIN) mass_sh[wave][lane] = mass;
    __syncthreads();
    if (threadIdx.x < TAIL) {
        const int t = threadIdx.x;
        double out = 0.0;
        if (t < 32) {
            unsigned s = 0;
            for (int w = 0; w < 4; ++w) s += cnt_sh[w][t] + cnt_sh[w][t + 32];
            out = (double)s;
        } else if (t == 32) {
            unsigned s = 0;
            for (int w = 0; w < 4; ++w)
                for (int l = 0; l < 32; ++l) s += chg_sh[w][l];
            out = (double)s;
        } else if (t >= 64) { // (TAIL is 64 in GC_PLAIN: never taken there)
            if constexpr (MODE != GC_PLAIN)
                for (int w = 0; w < 4; ++w) out += mass_sh[w][t - 64] + mass_sh[w][t - 32]; // wave 0 first, parity 0 before parity 1
        }
        pout[NT * 1024 + t] = out;
    }
}

// the six instances of a storage, at [CW == 64][mode]
template <class T>
using cluster_kernel = decltype(&k_graph_cluster<32, GC_PLAIN, T>);
template <class T>
static cluster_kernel<T> gc_kernel(int cw, int mode)
{
    static const cluster_kernel<T> kernels[2][GC_MODES] = {
        {k_graph_cluster<32, GC_PLAIN, T>, k_graph_cluster<32, GC_WEIGHT, T>, k_graph_cluster<32, GC_NORM, T>},
        {k_graph_cluster<64, GC_PLAIN, T>, k_graph_cluster<64, GC_WEIGHT, T>, k_graph_cluster<64, GC_NORM, T>}};
    return kernels[cw == 64][mode];
}

// what the steps and the drivers refuse alike, before any device work
static bool cluster_shape_ok(const glf_graph *g, unsigned k, unsigned dim, const double *scale)
{
    if (!g || k == 0 || k > (unsigned)GC_K || dim == 0 || dim > std::min(g->m, 64u)) return false;
    return !scale || all_finite(scale, dim);
}

static bool embed_ok(const glf_cluster_embed *emb)
{
    return !emb || (emb->struct_size == sizeof(glf_cluster_embed) && (emb->normalize == 0 || emb->normalize == 1));
}
static int embed_mode(const glf_cluster_embed *emb) { return !emb ? GC_PLAIN : emb->normalize ? GC_NORM : emb->d_weight ? GC_WEIGHT : GC_PLAIN; }

// one Lloyd iteration on checked arguments (returns with the stream drained). d_weight: NULL in GC_PLAIN, may be NULL in GC_NORM;
// h_mass may be NULL; GC_PLAIN reports mass = (double) counts.
static int cluster_step(glf_graph *g, int mode, const float *d_weight, unsigned k, unsigned dim, const double *h_cent, const double *scale,
                        const int32_t *d_prev, int32_t *d_labels, double *h_sums, uint64_t *h_counts, double *h_mass, uint64_t *changed)
{
    glf_ctx *ctx = g->ctx;
    const unsigned ld = g->ld;
    const int cw = gc_cw(ld);
    const int64_t N = (int64_t)g->width * g->height;
    // the scale operand as the kernel takes it: on a compact handle scale_c 2^e_c, the column scale folded in f64 before any fl32
    const bool compact = g->storage == GLF_PHI_F16;
    double sc[64];
    for (unsigned c = 0; c < dim; ++c) sc[c] = scale ? scale[c] : 1.0;
    if (compact) compact_fold_cols(sc, 1, dim, g->expo.data());
    if (!all_finite(sc, dim)) return set_error(ctx, GLF_ERR_INVALID, "cluster step: a scale entry folded with its column's 2^e_c is not finite");
    std::vector<float> h_op(gc_operand_floats(cw, mode), 0.f);
    for (unsigned j = 0; j < k; ++j) {
        double n2 = 0.0;
        for (unsigned c = 0; c < dim; ++c) {
            const double x = h_cent[(size_t)j * dim + c];
            h_op[(size_t)c * GC_K + j] = (float)(sc[c] * x);
            n2 += x * x;
        }
        h_op[(size_t)cw * GC_K + j] = (float)n2;
    }
    for (unsigned c = 0; mode == GC_NORM && c < dim; ++c) h_op[(size_t)cw * GC_K + GC_K + c] = (float)sc[c];
    DevBuf<float> op;
    DevBuf<double> part, tot;
    GLF_TRY(upload_operand(ctx, op, h_op));
    const size_t ncols = gc_part_cols(cw, mode);
    int64_t nblk = 0;
    int rc = GLF_OK;
    dispatch_phi(g, [&](auto *phi) {
        rc = launch_tiles_partials(g, gc_kernel<phi_elem_t<decltype(phi)>>(cw, mode), N, part, ncols, &nblk, phi, N, (int)ld, (int)k, (const float *)op.p,
                                   d_weight, d_prev, d_labels);
    });
    GLF_TRY(rc);
    std::vector<double> h_tot;
    GLF_TRY(sum_partials_to_host(ctx, part, (int)nblk, ncols, tot, h_tot)); // (the one read-back of an iteration; h_op and the buffers go out of scope)
    const double *tail = h_tot.data() + (size_t)(cw / 32) * 1024;
    for (unsigned j = 0; j < k; ++j) {
        for (unsigned c = 0; c < dim; ++c) h_sums[(size_t)j * dim + c] = h_tot[(size_t)(c / 32) * 1024 + j * 32 + c % 32];
        h_counts[j] = (uint64_t)tail[j];
        if (h_mass) h_mass[j] = mode == GC_PLAIN ? (double)h_counts[j] : tail[64 + j];
    }
    if (compact) compact_fold_cols(h_sums, k, dim, g->expo.data()); // (the raw-row sums of the halves times 2^e_c)
    *changed = d_prev ? (uint64_t)tail[32] : 0;
    return GLF_OK;
}

// The driver behind glf_graph_segment (emb and h_mass NULL) and glf_graph_segment_ex, errors reported under `name`: the seeding on
// a sample of rows (embedded in f64 as the kernel embeds them, with the sample's weights), then cluster_step + glf_cluster_update_w
// until a step moves no label. Without a weight plane the mass is the count, an integer below 2^53, and glf_cluster_update_w and
// glf_cluster_seed_w(w = NULL) are glf_cluster_update and glf_cluster_seed bit for bit.
static int segment_run(const char *name, glf_graph *g, const glf_segment_options *opt, const glf_cluster_embed *emb, int32_t *d_labels,
                       double *h_cent, glf_segment_stats *stats, double *h_mass)
{
    if (!g || !opt || !d_labels || !h_cent || opt->struct_size != sizeof(glf_segment_options)) return GLF_ERR_INVALID;
    glf_ctx *ctx = g->ctx;
    if (!embed_ok(emb))
        return set_error(ctx, GLF_ERR_INVALID, "%s: struct_size=%u (want %zu) normalize=%d", name, emb->struct_size, sizeof(glf_cluster_embed),
                         emb->normalize);
    const unsigned k = opt->k, dim = opt->dim;
    const double *scale = opt->scale;
    const int mode = embed_mode(emb);
    const bool normalize = mode == GC_NORM;
    const float *d_weight = emb ? emb->d_weight : nullptr;
    if (!cluster_shape_ok(g, k, dim, scale) || (opt->init != 0 && opt->init != 1) || (opt->init == 1 && !all_finite(h_cent, (size_t)k * dim)))
        return set_error(ctx, GLF_ERR_INVALID, "%s: k=%u dim=%u (m=%u) init=%d, or a centroid or scale entry that is not finite", name, k, dim, g->m,
                         opt->init);
    const unsigned max_iter = opt->max_iter ? opt->max_iter : 50;
    const int64_t N = (int64_t)g->width * g->height;
    GLF_ENTER(ctx);
    std::vector<double> cent((size_t)k * dim);
    if (opt->init == 0) {
        const int64_t ns = std::min<int64_t>(opt->sample_rows ? opt->sample_rows : 4096, N);
        const unsigned cols = dim + (d_weight ? 1 : 0); // a sampled row: its dim columns of Phi, then its weight
        const size_t cnt = (size_t)ns * cols;
        DevBuf<float> d_rows;
        GLF_TRY(d_rows.alloc(ctx, cnt));
        GLF_TRY(graph_sample_rows(g, (int)dim, 0, nullptr, d_weight, (int)(cols - dim), ns, d_rows.p));
        std::vector<float> h_rows(cnt);
        GLF_HIP(ctx, hipMemcpyAsync(h_rows.data(), d_rows.p, sizeof(float) * cnt, hipMemcpyDeviceToHost, ctx->stream));
        GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<double> rows((size_t)ns * dim), ws(d_weight ? (size_t)ns : 0);
        for (int64_t i = 0; i < ns; ++i) {
            double *row = rows.data() + (size_t)i * dim;
            double n2 = 0.0;
            for (unsigned c = 0; c < dim; ++c) {
                row[c] = (scale ? scale[c] : 1.0) * (double)h_rows[(size_t)i * cols + c];
                n2 += row[c] * row[c];
            }
            if (d_weight) ws[(size_t)i] = (double)h_rows[(size_t)i * cols + dim];
            const double rinv = n2 > 0.0 ? 1.0 / std::sqrt(n2) : 0.0;
            for (unsigned c = 0; normalize && c < dim; ++c) row[c] *= rinv;
        }
        if (glf_cluster_seed_w(rows.data(), d_weight ? ws.data() : nullptr, (size_t)ns, dim, k, opt->seed, cent.data()) != GLF_OK)
            return set_error(ctx, GLF_ERR_INVALID, "%s: the sample of %lld rows holds fewer than %u distinct rows%s", name, (long long)ns, k,
                             d_weight ? " of positive weight, or a weight that is negative or not finite" : "");
    } else
        std::copy(h_cent, h_cent + (size_t)k * dim, cent.begin());
    std::vector<double> sums((size_t)k * dim);
    uint64_t counts[GC_K] = {0}, changed = 0;
    double mass[GC_K] = {0.0};
    unsigned it = 0;
    int converged = 0;
    while (it < max_iter && !converged) {
        GLF_TRY(cluster_step(g, mode, d_weight, k, dim, cent.data(), scale, it ? d_labels : nullptr, d_labels, sums.data(), counts, mass, &changed));
        converged = it > 0 && changed == 0;
        ++it;
        GLF_TRY(glf_cluster_update_w(k, dim, scale, sums.data(), mass, cent.data(), cent.data()));
    }
    std::copy(cent.begin(), cent.end(), h_cent);
    if (stats) {
        stats->iterations = it;
        stats->converged = converged;
        stats->changed_last = changed;
        for (int j = 0; j < GC_K; ++j) stats->counts[j] = j < (int)k ? counts[j] : 0;
    }
    if (h_mass) std::copy(mass, mass + k, h_mass);
    return GLF_OK;
}

} // namespace glf

using namespace glf;

extern "C" {

int glf_graph_cluster_step(glf_graph *g, unsigned k, unsigned dim, const double *h_cent, const double *scale, const int32_t *d_prev,
                           int32_t *d_labels, double *h_sums, uint64_t *h_counts, uint64_t *changed)
{
    if (!g || !h_cent || !d_labels || !h_sums || !h_counts || !changed) return GLF_ERR_INVALID;
    if (!cluster_shape_ok(g, k, dim, scale) || !all_finite(h_cent, (size_t)k * dim))
        return set_error(g->ctx, GLF_ERR_INVALID, "glf_graph_cluster_step: k=%u dim=%u (m=%u), or a centroid or scale entry that is not finite", k, dim,
                         g->m);
    GLF_ENTER(g->ctx);
    return cluster_step(g, GC_PLAIN, nullptr, k, dim, h_cent, scale, d_prev, d_labels, h_sums, h_counts, nullptr, changed);
}

int glf_graph_cluster_step_ex(glf_graph *g, const glf_cluster_embed *emb, unsigned k, unsigned dim, const double *h_cent, const double *scale,
                              const int32_t *d_prev, int32_t *d_labels, double *h_sums, uint64_t *h_counts, double *h_mass, uint64_t *changed)
{
    if (!g || !h_cent || !d_labels || !h_sums || !h_counts || !h_mass || !changed) return GLF_ERR_INVALID;
    if (!embed_ok(emb))
        return set_error(g->ctx, GLF_ERR_INVALID, "glf_graph_cluster_step_ex: struct_size=%u (want %zu) normalize=%d", emb->struct_size,
                         sizeof(glf_cluster_embed), emb->normalize);
    if (!cluster_shape_ok(g, k, dim, scale) || !all_finite(h_cent, (size_t)k * dim))
        return set_error(g->ctx, GLF_ERR_INVALID, "glf_graph_cluster_step_ex: k=%u dim=%u (m=%u), or a centroid or scale entry that is not finite", k,
                         dim, g->m);
    GLF_ENTER(g->ctx);
    return cluster_step(g, embed_mode(emb), emb ? emb->d_weight : nullptr, k, dim, h_cent, scale, d_prev, d_labels, h_sums, h_counts, h_mass, changed);
}

int glf_graph_segment(glf_graph *g, const glf_segment_options *opt, int32_t *d_labels, double *h_cent, glf_segment_stats *stats)
{
    return segment_run("glf_graph_segment", g, opt, nullptr, d_labels, h_cent, stats, nullptr);
}

int glf_graph_segment_ex(glf_graph *g, const glf_segment_options *opt, const glf_cluster_embed *emb, int32_t *d_labels, double *h_cent,
                         glf_segment_stats *stats, double *h_mass)
{
    return segment_run("glf_graph_segment_ex", g, opt, emb, d_labels, h_cent, stats, h_mass);
}

} // extern "C"
