// glf_internal.hpp -- shared declarations of the HIP implementation behind include/glf.h.
// gfx950 (MI355X / CDNA4) only; wave = 64 lanes.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/glf.h"
#include "band_plan.hpp"

// Workspace pool of a context: device blocks released by DevBuf are kept and handed out again
// (same stream => ordering is safe). hipMalloc / hipFree of the multi-GB buffers on every call cost
// sporadic 1.7 s stalls (driver unmap of a 29 GB block) and a device-wide sync per hipFree.
struct glf_pool_block {
    void *p;
    size_t bytes;     // usable bytes (debug pool: the exact request rounded up to 256; a guard zone follows)
    bool in_use;
    unsigned last_call = 0; // glf_ctx::call_no of the public call that last took the block
};

// Which of several equivalent kernels implements a stage. Defaults (0 / false) = chosen from the problem size; every choice
// computes the same sums and is tested against the oracle and against the others. Set with glf_ctx_set_tuning, initialised at
// context creation from the environment variables GLF_<KEY> (read once, never per call).
struct glf_tuning {
    int nys_path = 0;            // NYS_PATH: 0 auto, 1 grid (factored Nystroem, all 256 grey levels), 2 direct (entry by entry), 3 rank (factored, photometric table as a rank-R expansion), 4 band (entry by entry, only the samples within the kernel's radius)
    int deg_path = 0;            // DEG_PATH: likewise for the degree
    int mv_path = 0;             // MV_PATH: 0 auto, 1 grid (L_A applied in factored form), 2 dense (stored L_A), 3 rank (factored, rank-R photometric table), 4 band (entry by entry within the radius, L_A never stored)
    int rowpass = 0;             // ROWPASS: row pass of the Nystroem passes: 0 / rt = row-tile form, 1 / v1 = one image row per wave
    int rowpass_op = 0;          // ROWPASS_OP: row pass of the L_A sweeps: 0 / v1, 1 / rt
    bool sweep_samples = false;  // SWEEP_COLPASS: rank-form L_A sweeps: false / segments = k_rank_colpass on the samples, true / samples = k_rank_samples
    int colpass = 0;             // COLPASS: rank-form column pass: 0 / ws = waves split into forming and contracting roles, 1 / v1 = every wave does both
    bool nys_no_lut = false;     // NYS_NO_LUT: direct Nystroem kernel generates entries with v_exp_f32 instead of LDS tables
    bool no_ecr = false;         // NO_ECR: column pass reads the per-column Ec fragment table instead of the compact one
    bool gs_seq = false;         // GS=seq: Gram-Schmidt as the column-by-column sweep instead of the Gram-matrix form
    bool residual_sweep = false; // RESIDUAL=sweep: residual from an explicit L_A sweep instead of the PCG state
    bool zmfma_groups = false;   // ZMFMA_GROUPS: degree row contraction in groups of five m-tiles (two n-tiles per wave) even when ten fit one wave
    int eig_shard = 0;           // EIG_SHARD: 0 auto (row-sharded eigen-solve unless the operator is in band form), 1 sharded, 2 replicated
    bool no_fused_filter = false; // NO_FUSED_FILTER: band form writes Phi and the filter runs as its own stage (k_apply_filter)
    int filter_form = 0;         // FILTER_FORM: the fused filter of the band form: 0 auto (sep where supported, else vec, else phi), 1 / sep = separable rank-R form (k_band_sep_*), 2 / vec = contracted with q = Psi w pair by pair, one column per plane (k_band_vec), 3 / phi = k_band's epilogue over the 64 columns of Phi
    bool band_noskip = false;    // BAND_NOSKIP: band-form Nystroem kernel executes every (row pair, half-block) of its workgroup's range, the exact zeros outside a wave's window included (same bits, more work: the check that the schedule loses no unit)
    bool pix_band = false;       // PIX_BAND: the colour and 16-bit bilateral kernels take the band form (Nystroem stage and operator) where the grey kernel would; off: entry by entry, L_A stored
    bool no_narrow = false;      // NO_NARROW: block PCG applies the operator to all columns of the block even when few still iterate
    bool operand_maxima_sweep = false; // OPERAND_MAXIMA=sweep: the operator finds its operand's column maxima itself (a pass over the block) even where block PCG carries them (ColMaxima); same bits either way: a max does not depend on the order
    bool verbose = false;        // VERBOSE: log every outer iteration on stderr (the reference does, hpc/inverse_power_it.c:164-181)
};

struct glf_native_comm; // comm.hip: RCCL / loopback communicator owned by a context

struct glf_ctx {
    std::vector<glf_pool_block> pool;
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    glf_comm comm{};
    bool has_comm = false;
    glf_native_comm *native = nullptr; // set by glf_ctx_set_comm_rccl / glf_multi_create: the library's own collectives
    bool force_comm = false;           // run the collectives even on a one-rank world (tests of the N > 1 plumbing)
    char last_error[512] = {0};
    hipDeviceProp_t prop{};
    // reusable events for stage timing
    hipEvent_t ev[8] = {};
    void *mv_scratch = nullptr; // split-f16 X fragments of the block mat-vec
    size_t mv_scratch_bytes = 0;
    // timing of the L_A sweeps (the HBM-bound kernel): a ring of event pairs, summed by mv_collect()
    static constexpr int MV_RING = 64;
    hipEvent_t mv_ev[2][MV_RING] = {};
    static constexpr int CP_RING = 16; // event pairs around the rank-form column-pass launches of one call (created on first use)
    hipEvent_t cp_ev[2][CP_RING] = {};
    int mv_pending = 0;
    unsigned call_no = 0; // public entry points so far (ages the cached work buffers: pool_get)
    int mv_count = 0;
    int narrow_sweeps = 0; // L_A sweeps applied to a packed block of the still-active columns (block PCG)
    double mv_ms = 0.0, mv_bytes = 0.0;
    // the seeded random start block of the eigensolver (hpc/inverse_power_it.c:12-47) as a device [p64][ld] f32 block:
    // it depends on (p, m, ld, seed) only, so images of one size reuse it (17 ms of host time at cfg4)
    float *x0_block = nullptr;
    unsigned x0_p = 0, x0_m = 0, x0_ld = 0;
    unsigned long long x0_seed = 0;
    // the same block after the solver's first Gram-Schmidt (inverse_power_iteration :95), with the norms |u_k| it found: the
    // result depends on the key above and on the Gram-Schmidt form in force, not on the image. x0_orth_form: 0 = none held,
    // else 1 + tune.gs_seq; x0_orth_fused: the Gram-matrix form ran (no fallback to the column sweep)
    float *x0_orth = nullptr;
    double *x0_orth_norms = nullptr; // device, x0_ld entries
    int x0_orth_form = 0;
    bool x0_orth_fused = false;
    int contraction = GLF_CONTRACT_F16_SPLIT; // how glf_Nystroem / glf_image_processing contract K_B^T Psi
    // what the last nystroem_contract launch ran with (glf_Nystroem_ex reports it): an exact-zero window (a SKIP instantiation, the
    // grid and rank forms' skipping passes, the band form's schedule), the table-driven generation of k_nystroem_f16s
    struct { int skipping = 0, lut = 0; } nys_note;
    // what the last degree sweep ran (glf_Degree_ex reports it): glf_degree_info's path, shape, skipping, chunks, mgroups, entries
    struct { int path = 0, shape = 0, skipping = 0, chunks = 0, mgroups = 0; double entries = 0.0; } deg_note;
    // what the filter stage's launchers ran since glf_Filter_ex cleared it (glf_filter_info): each launcher ORs its GLF_FK_* bit in
    // and notes its grid
    struct { unsigned kernels = 0, ld = 0, panels = 0, proj_blocks = 0, apply_blocks = 0, strided = 0; } flt_note;
    // one page of pinned, device-visible host memory the eigensolver's kernels write their flags and norms into (read
    // after a stream synchronise; no D2H copy launches, and no hipHostMalloc per image): see glf::ctx_pinned()
    void *pinned = nullptr;
    // rank form of the grid-factored contractions (nystroem_rank.inc): the factor F of the photometric table for one scale
    // band form (nystroem_band.inc): the geometry tables of the last (sample grid, kernel, image size), pixels / samples as targets
    // -- they depend on neither the image nor the operand, so consecutive images of one size reuse them (a plan)
    void *band_cache[2] = {nullptr, nullptr};
    bool rank_valid = false;
    float rank_s_val = 0.f;
    int rank_R = 0;             // terms of the expansion (0: the table is not low-rank enough, the exact form runs)
    void *rank_ftab = nullptr;  // f32 [R][256]
    void *rank_ff = nullptr;    // split-f16 A fragments of 2^15 F
    // debug pool (GLF_POOL_DEBUG=1): exact-size blocks + guard zone, NaN-filled floating-point buffers, no reuse
    bool pool_debug = false;
    int pool_violations = 0;
    glf_tuning tune;
};

// the graph handle of graph.hip (graph_cluster.hip reads it too)
struct glf_graph {
    glf_ctx *ctx = nullptr;
    int pix = 0, width = 0, height = 0;
    unsigned p = 0, m = 0, ld = 0;
    float *phi = nullptr;      // device [N][ld], raster rows (glf_malloc: not a block of the workspace pool); NULL once compact
    int storage = GLF_PHI_F32; // GLF_PHI_F16 after glf_graph_compact (graph_compact.hip): phi16, expo and d_expo then hold the handle's Phi
    void *phi16 = nullptr;     // device __half [N][ld], raster rows (glf_malloc)
    std::vector<int32_t> expo; // [ld] the column exponents e_c: the handle stands for Q[px][c] = 2^e_c phi16[px][c]
    int32_t *d_expo = nullptr; // device [ld], the same (glf_malloc): the row gathers of the drivers read it
    std::vector<double> lam;   // [m]
    std::vector<double> gram;  // [m][m] Phi^T Phi, filled by the first glf_graph_gram
    // resident workgroups per CU of the handle's tile kernels, by kernel (the host stub's address: one entry per instance, whatever its
    // storage, width or mode), asked of the runtime at a kernel's first launch (resident_tile_grid)
    std::vector<std::pair<const void *, int>> grid_cache;
    std::vector<unsigned> samples;       // [p] the sample pixels of the build call, ascending: its own sampler call's list (glf_graph_samples)
};

namespace glf {

constexpr int WAVE = 64;
constexpr int VEC_PAD = 64; // rows of vector blocks / lda of L_A are padded to a multiple of this (zeros)
constexpr int NYS_PAD = 64; // sample table and Psi are zero-padded to a multiple of this many rows

// pinned page layout (bytes): [0] PCG active-column counter (int), [64] Gram-Schmidt fallback flag (int),
// [128 .. 128 + 8 * 256) residual column sums (double[ld <= 256]), [3072] largest segment count of a row (rank form)
constexpr size_t PINNED_BYTES = 4096, PINNED_NACTIVE = 0, PINNED_GSFLAG = 64, PINNED_SUMS = 128, PINNED_RANKSEG = 3072, PINNED_BANDEVAL = 3136;
inline char *ctx_pinned(glf_ctx *ctx)
{
    if (!ctx->pinned && hipHostMalloc(&ctx->pinned, PINNED_BYTES, hipHostMallocDefault) != hipSuccess) ctx->pinned = nullptr;
    return static_cast<char *>(ctx->pinned);
}

inline int set_error(glf_ctx *ctx, int status, const char *fmt, ...)
{
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->last_error, sizeof(ctx->last_error), fmt, ap);
        va_end(ap);
    }
    return status;
}

#define GLF_HIP(ctx, call)                                                                    \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess)                                                                \
            return glf::set_error((ctx), e__ == hipErrorOutOfMemory ? GLF_ERR_NOMEM : GLF_ERR_HIP, \
                                  "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
    } while (0)

#define GLF_TRY(expr)                 \
    do {                              \
        int s__ = (expr);             \
        if (s__ != GLF_OK) return s__; \
    } while (0)

#define GLF_LAUNCH_CHECK(ctx) GLF_HIP(ctx, hipGetLastError())
// every public entry point: the calling thread's current device becomes the context's (two contexts on different GPUs in
// one process, or one host thread per GPU in glf_multi_*, would otherwise allocate and launch on the wrong device)
#define GLF_ENTER(ctx)                                 \
    do {                                               \
        GLF_HIP(ctx, hipSetDevice((ctx)->device));     \
        ++(ctx)->call_no;                              \
    } while (0)

inline int64_t round_up(int64_t x, int64_t q) { return (x + q - 1) / q * q; }
inline int64_t ceil_div(int64_t x, int64_t q) { return (x + q - 1) / q; }
// The grid of the graph-handle kernels that take one tile of 32 pixels per wave, four waves per workgroup, the tiles strided over
// a resident grid: min(ceil(ceil(N / 32) / 4), what fits the device at once), the rest of the tiles by the grid stride. The kernel's
// resident workgroups per CU come from the handle's grid_cache, asked of the runtime at the kernel's first launch.
template <class Kernel>
inline int resident_tile_grid(glf_graph *g, Kernel kernel, int64_t N, int64_t *nblk)
{
    glf_ctx *ctx = g->ctx;
    const void *key = reinterpret_cast<const void *>(kernel);
    int per_cu = 0;
    for (const auto &e : g->grid_cache)
        if (e.first == key) per_cu = e.second;
    if (per_cu <= 0) {
        GLF_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0));
        per_cu = per_cu > 1 ? per_cu : 1;
        g->grid_cache.emplace_back(key, per_cu);
    }
    const int64_t cus = ctx->prop.multiProcessorCount > 1 ? ctx->prop.multiProcessorCount : 1, tiles4 = ceil_div(ceil_div(N, 32), 4);
    *nblk = tiles4 < per_cu * cus ? tiles4 : per_cu * cus;
    return GLF_OK;
}
inline bool all_finite(const double *x, size_t n)
{
    for (size_t e = 0; e < n; ++e)
        if (!std::isfinite(x[e])) return false;
    return true;
}
// |x| fits an f32 (its fl32 is finite)
inline bool all_fl32_finite(const double *x, size_t n)
{
    for (size_t e = 0; e < n; ++e)
        if (!(std::fabs(x[e]) <= (double)std::numeric_limits<float>::max())) return false;
    return true;
}
// Leading dimension of vector blocks: m rounded up to a power of two in {32,64,128,256}
// (the column-reduction kernels map 256 threads onto 256/ld row lanes x ld columns).
inline unsigned ld_for(unsigned m) { unsigned ld = 32; while (ld < m) ld <<= 1; return ld; }
inline bool valid_ld(unsigned ld) { return ld == 32 || ld == 64 || ld == 128 || ld == 256; }
// More than 256 vectors: row-major matrices of the C-ABI carry ld = m rounded up to a multiple of 256; internally the
// vectors are processed as panels of 256 columns, each a contiguous [rows][256] block (eigen.hip, "panels").
constexpr unsigned PANEL_COLS = 256;
inline bool wide_ld(unsigned ld) { return ld > PANEL_COLS && ld % PANEL_COLS == 0; }
inline unsigned ld_total_for(unsigned m) { return m <= PANEL_COLS ? ld_for(m) : (unsigned)round_up(m, PANEL_COLS); }

constexpr size_t POOL_GUARD_BYTES = 4096;            // debug pool: canary bytes after every block
constexpr unsigned POOL_KEEP_CALLS = 64;             // an unused cached work buffer survives this many public calls without being taken
constexpr int POOL_CANARY = 0xA5;
// poison: the block holds floating-point data (debug pool: handed out filled with NaN; integer blocks with zeros)
void native_comm_release(glf_ctx *ctx);              // comm.hip
void *pool_get(glf_ctx *ctx, size_t bytes, bool poison_nan = false); // nullptr on failure (last_error set)
void pool_put(glf_ctx *ctx, void *ptr);              // back to the pool
void pool_forget(glf_ctx *ctx, void *ptr);           // ownership leaves the pool (caller hipFree's it)
void pool_free_all(glf_ctx *ctx, bool only_unused);
void pool_age(glf_ctx *ctx);                         // frees the cached blocks no call has taken for POOL_KEEP_CALLS public calls

// RAII device buffer from the context's workspace pool (returned to the pool at scope exit).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    glf_ctx *owner = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int alloc(glf_ctx *ctx, size_t count)
    {
        release();
        n = count;
        owner = ctx;
        if (count == 0) return GLF_OK;
        p = static_cast<T *>(pool_get(ctx, count * sizeof(T), std::is_floating_point<T>::value || std::is_same<T, _Float16>::value ||
                                                                  std::is_same<T, float4>::value));
        return p ? GLF_OK : GLF_ERR_NOMEM;
    }
    void release()
    {
        if (p) pool_put(owner, p);
        p = nullptr;
        n = 0;
    }
    T *take() // the block becomes a plain hipMalloc'd allocation owned by the caller
    {
        T *q = p;
        if (q) pool_forget(owner, q);
        p = nullptr;
        n = 0;
        return q;
    }
};

// Kernel-side description of the Gaussian kernel (hpc/affinity.c:59-121): the
// exponent is  -(dr^2+dc^2)/h_loc^2 - dv^2/h_val^2; we evaluate it as
// exp2(-(q*s_loc + u*s_val)) with s = log2(e)/h^2 so one v_exp_f32 does both
// reference exps. dr, dc, dv are exact small integers in f32.
struct KernelCoef {
    float s_loc; // log2(e) / h_loc^2 (0 for the photometric kernel)
    float s_val; // log2(e) / h_val^2 (0 for the spatial kernel); NLM: log2(e) / h^2 of the patch distance
    int kernel;  // GLF_KERNEL_*: NLM takes its own kernels (nlm.hip), the others share the positional ones
};
KernelCoef make_coef(int kernel, float h_loc, float h_val);
// host_util.cpp: P[v][w] = exp2(-s_val (v - w)^2) ~= F F^T in f64, F [256][rank] (strongest term first)
bool photometric_factor(double s_val, int max_chol, std::vector<double> &F, int &rank_out);
double photometric_factor_error(double s_val, const std::vector<double> &F, int rank, int R);

__device__ __forceinline__ float kernel_eval(float dr, float dc, float dv, float s_loc, float s_val)
{
    const float q = fmaf(dc, dc, dr * dr);
    const float t = fmaf(dv * dv, s_val, q * s_loc);
    return __builtin_amdgcn_exp2f(-t);
}

// byte k of a packed colour R + 256 G + 65536 B as f32 (v_cvt_f32_ubyte<k>)
__device__ __forceinline__ float ubyte_f32(unsigned v, int k) { return (float)((v >> (8 * k)) & 0xffu); }

// AboveXSetY(z, 255, 255) (hpc/display.c:76), negative -> 0 (survey quirk Q4) and the truncating (png_byte) cast
// (hpc/utils.c:525) of the reference's fp64 z = y + c, evaluated WITHOUT rounding the sum to f32 first: y is an integer, so
// trunc(y + c) = y + floor(c) wherever y + c >= 0. At 4096^2 |c| ~ 1e-3 grey levels: the f32 sum rounds y - 2e-6 up to y
// and 4 % of the pixels then miss the reference's y - 1.
__device__ __forceinline__ uint8_t filter_output(int y, float c)
{
    int zi = y + (int)floorf(fminf(fmaxf(c, -1.0e6f), 1.0e6f));
    zi = zi > 255 ? 255 : zi;
    zi = (zi < 0 || !(c == c)) ? 0 : zi; // (NaN -> 0)
    return (uint8_t)zi;
}
// the same rule at 16 bits, in f64: clamp(x + floor(c), 0, 65535), NaN -> 0
__device__ __forceinline__ uint16_t filter_output_u16(int x, double c)
{
    const double fc = floor(fmin(fmax(c, -1.0e6), 1.0e6));
    int zi = x + (int)fc;
    zi = zi > 65535 ? 65535 : zi;
    zi = (zi < 0 || !(c == c)) ? 0 : zi;
    return (uint16_t)zi;
}

// The pixel formats. Grey: uint8 [N] (GLF_KERNEL_BILATERAL and the other 8-bit kernels); Rgb: interleaved uint8 [N][3]
// (GLF_KERNEL_BILATERAL_RGB); U16: uint16 [N] (GLF_KERNEL_BILATERAL_U16); F32: float [N] (GLF_KERNEL_BILATERAL_F32, any finite
// value, h_val in the image's units); RgbF32: interleaved float [N][3] (GLF_KERNEL_BILATERAL_RGBF32, any finite values). The image
// travels as a byte pointer; the entry-by-entry
// kernels read it through the format's policy Pix<G>, which holds all that differs between the formats:
//   In, NCH        the image element and the channels per pixel: channel k of pixel px is img[NCH px + k]
//   Val, read      a pixel's value as the kernels compare it (its channels in f32, exact)
//   record, value  the sample record of pixel px and the value it carries. Grey, U16, F32: {row, col, v, 0};
//                  Rgb: {row, col, 0, R + 256 G + 65536 B} (the packed colour as an exact integer in f32);
//                  RgbF32: {row, col, 0, 0}: three floats do not fit the record, so HAS_VALUE_BLOCK is set and the sample table
//                  carries a value block of float4 {R, G, B, 0}, one per sample, behind its padded records (samples + p_pad, p_pad =
//                  round_up(p, NYS_PAD): one pointer, one allocation). value(record, entry) takes both; the formats without a
//                  block ignore the entry, and sample_value<G> does not load it for them
//   MATRIX_AS      (host side) the format whose k_sample_matrix reads the format's records: U16 and F32 records are Grey's {row, col, v, 0}
//   dist2          the squared photometric distance |a - b|^2 in a fixed operation order; the kernels take
//                  K = exp2(-fmaf(dist2, s_val, (dr^2 + dc^2) s_loc))
//   Tile, tile     the degree sweep's LDS element {value, col}; outside() lies in a column no sample reaches (K = 0)
//   Out, output    the output element of the apply kernel and its rule for channel x (passed exactly, as a double) with its
//                  f64 correction c: the grey d_out's rule, through f32 at 8 bits, in f64 at 16 bits; F32: (float)(x + c), the
//                  float z itself, no clamp and no floor (RgbF32 too)
// The factored forms over the 256 grey levels (grid, rank, the level-table degree) exist for Grey alone. The band form takes
// the others as well (k_band<.., G>: the photometric factor from dist2 and one v_exp_f32 per entry; RgbF32 with three u32 per sample in
// the chunk tails), behind the PIX_BAND key.
enum class PixGen { Grey, Rgb, U16, F32, RgbF32 };
template <PixGen G> struct Pix;
// one grey value per pixel, stored as T (Grey: uint8_t, U16: uint16_t, F32: float): the record {row, col, v, 0}
template <typename T> struct PixGreyValue {
    using In = T;
    using Val = float;
    static constexpr int NCH = 1;
    static constexpr bool HAS_VALUE_BLOCK = false;
    static constexpr PixGen MATRIX_AS = PixGen::Grey;
    __device__ __forceinline__ static Val read(const In *img, int64_t px) { return (float)img[px]; }
    __device__ __forceinline__ static float4 record(const In *img, uint32_t px, uint32_t width)
    {
        return make_float4((float)(px / width), (float)(px % width), (float)img[px], 0.f);
    }
    __device__ __forceinline__ static Val value(float4 s, float4) { return s.z; }
    __device__ __forceinline__ static float dist2(Val a, Val b) { const float d = a - b; return d * d; }
};
template <> struct Pix<PixGen::Grey> : PixGreyValue<uint8_t> {};
template <> struct Pix<PixGen::U16> : PixGreyValue<uint16_t> {
    using Tile = float2; // {v, col}
    using Out = uint16_t;
    __device__ __forceinline__ static Tile tile(const In *img, int64_t px, int c) { return make_float2(read(img, px), (float)c); }
    __device__ __forceinline__ static Tile outside() { return make_float2(0.f, -1e30f); }
    __device__ __forceinline__ static Val tile_value(Tile t) { return t.x; }
    __device__ __forceinline__ static float tile_col(Tile t) { return t.y; }
    __device__ __forceinline__ static Out output(double x, double c) { return filter_output_u16((int)x, c); }
};
// (the differences of two floats are rounded once, their squares once more; a dist2 that overflows gives exp2(-inf) = 0)
template <> struct Pix<PixGen::F32> : PixGreyValue<float> {
    using Tile = float2; // {v, col}
    using Out = float;
    __device__ __forceinline__ static Tile tile(const In *img, int64_t px, int c) { return make_float2(read(img, px), (float)c); }
    __device__ __forceinline__ static Tile outside() { return make_float2(0.f, -1e30f); }
    __device__ __forceinline__ static Val tile_value(Tile t) { return t.x; }
    __device__ __forceinline__ static float tile_col(Tile t) { return t.y; }
    __device__ __forceinline__ static Out output(double x, double c) { return (float)(x + c); }
};
template <> struct Pix<PixGen::Rgb> {
    using In = uint8_t;
    using Val = float3;
    using Tile = float4; // {R, G, B, col}
    using Out = uint8_t;
    static constexpr int NCH = 3;
    static constexpr bool HAS_VALUE_BLOCK = false;
    static constexpr PixGen MATRIX_AS = PixGen::Rgb;
    __device__ __forceinline__ static Val read(const In *img, int64_t px)
    {
        return make_float3((float)img[3 * px], (float)img[3 * px + 1], (float)img[3 * px + 2]);
    }
    __device__ __forceinline__ static float4 record(const In *img, uint32_t px, uint32_t width)
    {
        const In *q = img + (size_t)px * 3;
        return make_float4((float)(px / width), (float)(px % width), 0.f, (float)((unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16)));
    }
    __device__ __forceinline__ static Val value(float4 s, float4)
    {
        const unsigned v = (unsigned)s.w;
        return make_float3(ubyte_f32(v, 0), ubyte_f32(v, 1), ubyte_f32(v, 2));
    }
    __device__ __forceinline__ static float dist2(Val a, Val b)
    {
        const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z;
        return fmaf(d2, d2, fmaf(d1, d1, d0 * d0)); // exact: integers below 2^18
    }
    __device__ __forceinline__ static Tile tile(const In *img, int64_t px, int c)
    {
        const Val v = read(img, px);
        return make_float4(v.x, v.y, v.z, (float)c);
    }
    __device__ __forceinline__ static Tile outside() { return make_float4(0.f, 0.f, 0.f, -1e30f); }
    __device__ __forceinline__ static Val tile_value(Tile t) { return make_float3(t.x, t.y, t.z); }
    __device__ __forceinline__ static float tile_col(Tile t) { return t.w; }
    __device__ __forceinline__ static Out output(double x, double c) { return filter_output((int)x, (float)c); }
};
// three float channels per pixel: Rgb's tile and dist2 (its operation order) on float reads, F32's output rule; the sample's channels
// come from the value block. Each difference is rounded once, its square once, the two fmas once each: all terms positive, so dist2
// carries at most ~5 x 2^-24 of relative error; a dist2 that overflows gives exp2(-inf) = 0
template <> struct Pix<PixGen::RgbF32> {
    using In = float;
    using Val = float3;
    using Tile = float4; // {R, G, B, col}
    using Out = float;
    static constexpr int NCH = 3;
    static constexpr bool HAS_VALUE_BLOCK = true;
    static constexpr PixGen MATRIX_AS = PixGen::RgbF32;
    __device__ __forceinline__ static Val read(const In *img, int64_t px) { return make_float3(img[3 * px], img[3 * px + 1], img[3 * px + 2]); }
    __device__ __forceinline__ static float4 record(const In *, uint32_t px, uint32_t width)
    {
        return make_float4((float)(px / width), (float)(px % width), 0.f, 0.f);
    }
    __device__ __forceinline__ static float4 block_entry(const In *img, uint32_t px)
    {
        const In *q = img + (size_t)px * 3;
        return make_float4(q[0], q[1], q[2], 0.f);
    }
    __device__ __forceinline__ static Val value(float4, float4 e) { return make_float3(e.x, e.y, e.z); }
    __device__ __forceinline__ static float dist2(Val a, Val b)
    {
        const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z;
        return fmaf(d2, d2, fmaf(d1, d1, d0 * d0));
    }
    __device__ __forceinline__ static Tile tile(const In *img, int64_t px, int c)
    {
        const Val v = read(img, px);
        return make_float4(v.x, v.y, v.z, (float)c);
    }
    __device__ __forceinline__ static Tile outside() { return make_float4(0.f, 0.f, 0.f, -1e30f); }
    __device__ __forceinline__ static Val tile_value(Tile t) { return make_float3(t.x, t.y, t.z); }
    __device__ __forceinline__ static float tile_col(Tile t) { return t.w; }
    __device__ __forceinline__ static Out output(double x, double c) { return (float)(x + c); }
};
__device__ __forceinline__ unsigned round_up_dev(unsigned x, unsigned q) { return (x + q - 1) / q * q; }
// the value sample i carries: from its record s alone, or (HAS_VALUE_BLOCK) from entry i of the value block behind the p_pad records
template <PixGen G> __device__ __forceinline__ typename Pix<G>::Val sample_value(const float4 *__restrict__ samples, unsigned p_pad, unsigned i, float4 s)
{
    if constexpr (Pix<G>::HAS_VALUE_BLOCK) return Pix<G>::value(s, samples[(size_t)p_pad + i]);
    else return Pix<G>::value(s, s);
}

// ---- host side: the format table and the dispatchers ---------------------------------------------------------------------------
// What the host code knows of a format, one row per PixGen, built from Pix<G>: everything outside the kernels that differs between
// the formats is read from here (pix_desc) or instantiated through pix_dispatch / pix_dispatch_raw below.
struct PixDesc {
    int pix;              // the public GLF_PIX_*
    int kernel;           // the format's bilateral GLF_KERNEL_* (GLF_KERNEL_BILATERAL stands for it at the format's entry points)
    size_t bytes;         // per pixel, in and out
    int channels;         // per pixel; the float z planes of a call
    bool is_float;        // float elements: admitted after the finite check only, which runs over `channels` floats per pixel
    bool value_block;     // Pix<G>::HAS_VALUE_BLOCK: the sample table carries as many value-block entries behind its padded records
    int svals32_what;     // k_gridop_svals32's code for the sample values as u32: 0 the record's z as an integer, 1 the packed colour
                          // (its w), 2 the bit pattern of the float z, 3 three planes of bit patterns from the value block
    int svals32_planes;   // u32 values per sample in that image
    const char *name;     // the format in messages
    const char *image;    // "the <name> kernel takes <image>: <entry>": what the 8-bit entry points answer to another format's kernel
    const char *entry;    // the public entry point that message cites
};
template <PixGen G> constexpr PixDesc make_pix_desc(int pix, int kernel, const char *name, const char *image, const char *entry)
{
    using P = Pix<G>;
    constexpr bool flt = std::is_floating_point<typename P::In>::value;
    return {pix, kernel, sizeof(typename P::In) * P::NCH, P::NCH, flt, P::HAS_VALUE_BLOCK,
            P::HAS_VALUE_BLOCK ? 3 : flt ? 2 : P::NCH == 3 ? 1 : 0, P::HAS_VALUE_BLOCK ? P::NCH : 1, name, image, entry};
}
constexpr PixDesc PIX_TABLE[] = { // indexed by PixGen
    make_pix_desc<PixGen::Grey>(GLF_PIX_U8, GLF_KERNEL_BILATERAL, "8-bit", "an 8-bit image", "glf_image_processing"),
    make_pix_desc<PixGen::Rgb>(GLF_PIX_RGB8, GLF_KERNEL_BILATERAL_RGB, "colour", "an RGB image", "glf_image_processing_rgb"),
    make_pix_desc<PixGen::U16>(GLF_PIX_U16, GLF_KERNEL_BILATERAL_U16, "16-bit", "a 16-bit image", "glf_image_processing_u16"),
    make_pix_desc<PixGen::F32>(GLF_PIX_F32, GLF_KERNEL_BILATERAL_F32, "float", "a float image", "glf_image_processing_f32"),
    make_pix_desc<PixGen::RgbF32>(GLF_PIX_RGBF32, GLF_KERNEL_BILATERAL_RGBF32, "float colour", "a float RGB image", "glf_image_processing_rgbf32"),
};
constexpr int PIX_FORMATS = (int)(sizeof(PIX_TABLE) / sizeof(PIX_TABLE[0]));
inline const PixDesc &pix_desc(PixGen g) { return PIX_TABLE[(int)g]; }
// the format a kernel reads (every kernel that is not another format's bilateral kernel reads 8-bit grey), and the format of a
// GLF_PIX_* value (the caller has checked its range)
inline PixGen pixgen_of(int kernel)
{
    for (int g = 1; g < PIX_FORMATS; ++g)
        if (PIX_TABLE[g].kernel == kernel) return (PixGen)g;
    return PixGen::Grey;
}
inline PixGen pixgen_of_pix(int pix)
{
    for (int g = 1; g < PIX_FORMATS; ++g)
        if (PIX_TABLE[g].pix == pix) return (PixGen)g;
    return PixGen::Grey;
}
// f(PixTag<G>{}) for the runtime format g: inside a generic lambda `t.G` is the format as a constant (k_planes<t.G>, Pix<t.G>)
template <PixGen V> struct PixTag { static constexpr PixGen G = V; };
template <class F> inline void pix_dispatch(PixGen g, F &&f)
{
    switch (g) {
    case PixGen::Grey: f(PixTag<PixGen::Grey>{}); break;
    case PixGen::Rgb: f(PixTag<PixGen::Rgb>{}); break;
    case PixGen::U16: f(PixTag<PixGen::U16>{}); break;
    case PixGen::F32: f(PixTag<PixGen::F32>{}); break;
    case PixGen::RgbF32: f(PixTag<PixGen::RgbF32>{}); break;
    }
}
// the same over the formats without a factored form: Pix<Grey> has no Tile and no Out, so their kernels are never instantiated for
// it (Grey does nothing here: every caller has refused it before)
template <class F> inline void pix_dispatch_raw(PixGen g, F &&f)
{
    if (g != PixGen::Grey) pix_dispatch(g, [&](auto t) {
        if constexpr (decltype(t)::G != PixGen::Grey) f(t);
    });
}
// records the sample table allocates for p samples in the format: the padded records, and the value block behind them
inline size_t sample_table_records(PixGen g, unsigned p) { return (size_t)round_up(p, NYS_PAD) * (pix_desc(g).value_block ? 2 : 1); }
// whether the factored forms over the 256 grey levels apply to a kernel
inline bool grey_levels_factor(int kernel) { return kernel != GLF_KERNEL_NLM && pixgen_of(kernel) == PixGen::Grey; }
// the band form applies to a kernel: it factors over grey levels, or it is a colour / 16-bit / float bilateral kernel and PIX_BAND is set
inline bool band_form_applies(const glf_ctx *ctx, int kernel) { return grey_levels_factor(kernel) || (ctx->tune.pix_band && pixgen_of(kernel) != PixGen::Grey); }

// ---- LDS-DMA staging ---------------------------------------------------------------------------
// global_load_lds_dwordx4: 64 lanes x 16 B land at LDS byte offset (wave-uniform base) + lane * 16, no
// VGPRs. Issued from inline asm on purpose: with the builtin, hipcc (ROCm 7.2) cannot prove that the DMA
// into one staging buffer does not alias the ds_reads of the other and puts s_waitcnt vmcnt(0) in front
// of the MFMA loop; staged through a register array instead, the array became a stack object (scratch:
// tens of GB of HBM writes per launch). The issuing wave must call lds_dma_drain() before the barrier that
// hands the buffer to its readers.
__device__ __forceinline__ void lds_dma_16B(const void *gptr, unsigned lds_byte_offset)
{
    asm volatile("s_mov_b32 m0, %1\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, off"
                 :
                 : "v"(gptr), "s"(lds_byte_offset)
                 : "memory");
}
// the same with the global address as a wave-uniform base (scalar registers) + a 32-bit byte offset per lane: no 64-bit vector
// address arithmetic per instruction when only the base changes between calls
__device__ __forceinline__ void lds_dma_16B_base(const void *gbase_uniform, unsigned lane_byte_offset, unsigned lds_byte_offset)
{
    asm volatile("s_mov_b32 m0, %2\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %1"
                 :
                 : "v"(lane_byte_offset), "s"(gbase_uniform), "s"(lds_byte_offset)
                 : "memory");
}
__device__ __forceinline__ void lds_dma_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// f32 at an absolute LDS byte address (ds_read_b32 with a computed address)
__device__ __forceinline__ float lds_f32(unsigned lds_byte_addr)
{
    return *reinterpret_cast<const __attribute__((address_space(3))) float *>(lds_byte_addr);
}
__device__ __forceinline__ unsigned lds_offset_of(const void *lds_ptr)
{
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char *)(const char *)lds_ptr;
}
// copy `pieces` KiB-sized pieces global -> LDS, piece i handled by wave (i % NW) of an NW-wave workgroup
template <int NW = 4>
__device__ __forceinline__ void lds_dma_copy(const void *gsrc, void *ldst, int pieces, int wave, int lane)
{
    const char *g = reinterpret_cast<const char *>(gsrc);
    const unsigned base = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_offset_of(ldst)); // (wave-uniform: goes to m0)
    const int uw = __builtin_amdgcn_readfirstlane(wave);
    for (int i = uw; i < pieces; i += NW) lds_dma_16B(g + (size_t)i * 1024 + lane * 16, base + (unsigned)i * 1024u);
}

// ---- stage implementations (device pointers, all on ctx->stream) -----------------

// extra signal planes of the _signals entry points (nullptr: the guide alone): float [nsig][N] in and out, device pointers
// (comm.hip's multi_run takes the host planes of the glf_multi_ entry points in one)
struct SignalPlanes {
    int nsig;
    const float *d_sig;
    float *d_out;
};
// The whole approximate path behind every glf_image_processing_* and glf_multi_image_processing_* entry point and glf_graph_build
// (pipeline.hip). gen: the guide's pixel format; d_img and d_out are [N] pixels of it, d_zf (optional; null for the float formats,
// whose d_out is z itself) its [NCH][N] floats. It alone checks the pointers, the sizes, sig's plane count, the struct sizes and
// that a float guide is finite. A colour, 16-bit or float guide has no 8-bit y: its channels are filtered as planes (formed inside
// from the image) and written to d_out; sig there: float planes that ride along in the same two passes over Phi. (Hidden: an
// internal entry shared by three translation units, not one of the library's dynamic symbols.)
__attribute__((visibility("hidden"))) int image_processing_run(glf_ctx *ctx, const glf_options *opt_in, PixGen gen, const uint8_t *d_img,
                                                               int width, int height, uint8_t *d_out, float *d_zf, double *eigvals_out,
                                                               glf_stats *stats, glf_capture *cap, const SignalPlanes *sig);
// What follows from the options and the image size before any device work; const once plan_run has built it. image_processing_run
// is its checks, f32_admit, pool_age, plan_run and run_planned; glf_graph_build plans once itself, sizes Phi from the plan and keeps
// the sample list.
struct RunPlan {
    glf_options opt; // defaulted; GLF_KERNEL_BILATERAL at a non-grey entry point replaced by the format's kernel
    PixGen gen;
    bool u8_guide;   // an 8-bit grey guide: the only one with an 8-bit y (the others' values are filtered as planes)
    int64_t N;
    unsigned p;
    std::vector<unsigned> samples; // [p] pixel indices, ascending
    unsigned m;
    bool wide;       // more than 256 eigenpairs (the reference default m = p - 1): 256-column panels
    unsigned ld, p32;
    KernelCoef coef;
    float gain, ysub; // of the filter z = (1 - ysub) y + gain Phi f(Pi) Phi^T y (filter_rule.hpp)
};
// the validation of the options and the sizing, with the whole path's statuses and messages
__attribute__((visibility("hidden"))) int plan_run(glf_ctx *ctx, const glf_options *opt_in, PixGen gen, int width, int height, bool has_capture,
                                                   bool has_signals, RunPlan *plan);
__attribute__((visibility("hidden"))) int run_planned(glf_ctx *ctx, const RunPlan &plan, const uint8_t *d_img, int width, int height,
                                                      uint8_t *d_out, float *d_zf, double *eigvals_out, glf_stats *stats, glf_capture *cap,
                                                      const SignalPlanes *sig);
// the float formats admit finite values only: one pass over the image's floats before anything else (a no-op for the others)
__attribute__((visibility("hidden"))) int f32_admit(glf_ctx *ctx, PixGen gen, const uint8_t *d_img, int width, int height);

// Sample table: float4 {row, col, value, 0} per sample (float colour: and the value block behind the padded records) + mask + device idx.
struct SampleTables {
    DevBuf<float4> samples;
    DevBuf<uint8_t> mask;
    DevBuf<uint32_t> idx;
};
// d_img and the records in the format of `kernel` (Pix<pixgen_of(kernel)>)
int build_sample_tables(glf_ctx *ctx, const uint8_t *d_img, int width, int height, unsigned p,
                        const unsigned *h_idx, SampleTables &out, int kernel = GLF_KERNEL_BILATERAL);

// Partial degree D[i] = sum over pixels in rows [row0,row1) of K(sample i, pixel).
int degree_rows(glf_ctx *ctx, const uint8_t *d_img, int width, int height, int row0, int row1,
                const float4 *d_samples, unsigned p, KernelCoef coef, double *d_degree);

// Same sums, skipping pixels whose kernel entry underflows to exactly 0 in f32 for every sample of a block
// (h_idx: host sample indices, needed for the tile-major sample order). evaluated: entries executed.
// sums the pending mat-vec event pairs into ctx->mv_ms (synchronises on the last one)
int mv_collect(glf_ctx *ctx);
// device pointer to the cached start block X0 [round_up(p,64)][ld] for (p, m, ld, seed)
int start_block_cached(glf_ctx *ctx, unsigned p, unsigned m, unsigned ld, unsigned long long seed, const float **d_block);
int degree_rows_auto(glf_ctx *ctx, const uint8_t *d_img, int width, int height, int row0, int row1, const float4 *d_samples,
                     unsigned p, const unsigned *h_idx, KernelCoef coef, double *d_degree, int window, double *evaluated,
                     const uint32_t *d_idx = nullptr, double *d_ysum = nullptr, bool *have_ysum = nullptr);
int weighted_sums_grid(glf_ctx *ctx, const uint8_t *d_img, int width, int height, int row0, int row1, const float4 *d_samples, unsigned p,
                       const unsigned *h_idx, KernelCoef coef, int window, const float *d_plane, double wabs, double *d_out);
int degree_rows_windowed(glf_ctx *ctx, const uint8_t *d_img, int width, int height, int row0, int row1,
                         const float4 *d_samples, unsigned p, const unsigned *h_idx, KernelCoef coef,
                         double *d_degree, double *evaluated);

// -no_approx: z = clamp(y - L y) with the full N x N Laplacian, never stored (affinity.hip)
int entire_computation(glf_ctx *ctx, const uint8_t *d_img, int width, int height, KernelCoef coef, uint8_t *d_out, float *d_zf,
                       double *alpha_out);

// K_A (scale = 1, diag untouched) or L_A (scale = -alpha, diagonal alpha * D_i).
// columns [col0, col0 + ncols) only (ncols = 0: all p columns); out is [p][ld] with local column index
int build_sample_matrix(glf_ctx *ctx, const float4 *d_samples, unsigned p, KernelCoef coef,
                        float *d_out, int64_t ld, bool laplacian, double alpha, const double *d_degree,
                        unsigned col0 = 0, unsigned ncols = 0, const uint8_t *d_img = nullptr, int width = 0, int height = 0,
                        const uint32_t *d_idx = nullptr); // (image and device indices: needed by the NLM kernel only)
// non-local-means affinity (nlm.hip): same contracts as degree_rows / build_sample_matrix / nystroem_contract
int nlm_degree_rows(glf_ctx *ctx, const uint8_t *d_img, int width, int height, int row0, int row1, const uint32_t *d_idx, unsigned p,
                    KernelCoef coef, double *d_degree);
int nlm_sample_matrix(glf_ctx *ctx, const uint8_t *d_img, int width, int height, const uint32_t *d_idx, unsigned p, KernelCoef coef,
                      float *d_out, int64_t ld, bool laplacian, double alpha, const double *d_degree, unsigned col0, unsigned ncols);
struct NysRequest;
int nlm_nystroem(glf_ctx *ctx, const NysRequest &rq);
// out[i] = sum over the chunks k of partial[k][i], k ascending (affinity.hip)
__global__ void k_reduce_partials(const double *__restrict__ partial, unsigned p, int nchunks, double *__restrict__ out);
// the formats without a factored form (entrywise.hip, gen Rgb, U16, F32 or RgbF32; d_img in the format): the contract of degree_rows, the
// windowed entry-by-entry sweep (*evaluated = entries computed); the image's channels as float planes [NCH][N]; the outputs
// (d_w [NCH][ld]; d_img / d_out [N] pixels, rows [pix0, pix1) only; d_zf optional [NCH][N])
int degree_rows_entrywise(glf_ctx *ctx, PixGen gen, const uint8_t *d_img, int width, int height, int row0, int row1,
                          const float4 *d_samples, unsigned p, KernelCoef coef, double *d_degree, double *evaluated);
int pix_planes(glf_ctx *ctx, PixGen gen, const uint8_t *d_img, int64_t N, float *d_planes);
int apply_filter_pix(glf_ctx *ctx, PixGen gen, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, const float *d_w, float gain,
                     float ysub, const uint8_t *d_img, uint8_t *d_out, float *d_zf, int64_t N);
// joint filtering under a colour or 16-bit guide (glf_image_processing_rgb_signals / _u16_signals): the guide's channels and nsig
// float planes (d_sig / d_sig_out [nsig][N]) in two passes over Phi. phi_t_pix_signals: d_c [NCH][ld] and d_cs [nsig][ld] (f64) =
// Phi^T x over this rank's pixels, the guide's with the bits phi_t_signals gives on its float planes. apply_filter_pix_signals:
// d_w [NCH + nsig][ld], the guide's weights first; the guide's outputs are those of apply_filter_pix
int phi_t_pix_signals(glf_ctx *ctx, PixGen gen, const float *d_phi, const uint8_t *d_img, const float *d_sig, int64_t N, int nsig,
                      int64_t pix0, int64_t pix1, unsigned ld, double *d_c, double *d_cs);
int apply_filter_pix_signals(glf_ctx *ctx, PixGen gen, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, int nsig, const float *d_w,
                             float gain, float ysub, const uint8_t *d_img, uint8_t *d_out, float *d_zf, const float *d_sig, float *d_sig_out,
                             int64_t N);
// the float format admits finite values only: *finite = every one of the N floats is (one pass, synchronises)
int f32_all_finite(glf_ctx *ctx, const float *d_img, int64_t N, bool *finite);
int laplacian_from_KA(glf_ctx *ctx, const float *d_KA, int64_t ldk, unsigned p, float *d_LA, int64_t ld,
                      double alpha, const double *d_degree);

// Eigensolver pieces (eigen.hip)
// Row sharding of the symmetric p x p operator over the ranks of ctx->comm: this rank computes output
// rows [row0,row1) of A X and holds only the matching COLUMN block A[:, row0:row1) (= the transposed row
// block), stored [p][lda] with element (k, row) at A[k * lda + (row - row0)]. rows_per_rank is the
// all-gather block (a multiple of 64 >= ceil(p / size)); 0 = not sharded (A is the full matrix).
// the row-pass kernel of the grid-factored Nystroem contraction, timed launch by launch
struct RowpassStats {
    int launches = 0;
    float ms = 0.f;
    double flops = 0.0;
    // rank form: the fused T' + column-pass kernel, and the terms of the photometric expansion
    int col_launches = 0;
    float col_ms = 0.f;
    double col_flops = 0.0;
    int rank_R = 0;
};
struct GridOp; // L_A = alpha (D - K_A) applied in grid-factored form, never stored (nystroem_grid.inc)
int grid_op_create(glf_ctx *ctx, const float4 *d_samples, const unsigned *h_idx, unsigned p, int width, int height,
                   KernelCoef coef, GridOp **out); // GLF_ERR_UNSUPPORTED: not a tensor grid (or not the split-f16 mode)
void grid_op_destroy(GridOp *op);
unsigned grid_op_rows_per_rank(const GridOp *op, int size); // all-gather block: whole grid rows
void band_cache_free(glf_ctx *ctx);
// Filter applied in the epilogue of the band-form Nystroem kernel: z = y + gain Phi[px] . w - ysub y straight from the
// accumulators, Phi itself never written (hpc/display.c:60-78 fused into hpc/nystroem.c:41-42)
// joint filtering in k_band's epilogue: nsig float planes through the guide's filter (weights [nsig][ld], planes [nsig][N])
struct BandSignals {
    int nsig = 0;
    const float *w = nullptr;
    const float *s = nullptr;
    float *out = nullptr;
    int64_t N = 0;
};
// (the fused kernels take it by value: what only k_band_q / k_band_sep_g read -- w and sig.w -- sits behind what every lane stores with)
struct BandFilter {
    float gain = 0.f, ysub = 0.f;
    uint8_t *out = nullptr;   // [N] (absolute pixel index)
    float *zf = nullptr;      // [N] or null
    float *corr = nullptr;    // [pix1 - pix0] or null
    BandSignals sig;
    const float *w = nullptr; // [ld] filter weights x c (device)
};
// c = Psi^T (ysum - t) + Phi_A^T y_A  (ysum: the degree stage's value-weighted sums over all pixels; t = K_A y_A takes the
// sample pixels out again): Phi^T y without Phi. d_c [ld] f64.
int c_from_ysum(glf_ctx *ctx, const float *d_psi, const float *d_phiA, const double *d_ysum, const float *d_t, unsigned t_ld,
                const float4 *d_samples, unsigned p, unsigned ld, double *d_c, const float *d_sval = nullptr); // d_sval: s_A [p][t_ld] in place of y_A
// the sample pixels' outputs from their rows of Phi_A (the band kernel filters every pixel with its extended row)
int filter_sample_rows(glf_ctx *ctx, const float *d_phiA, unsigned n, unsigned ld, const uint32_t *d_idx, const uint8_t *d_img,
                       const float *d_w, float gain, float ysub, uint8_t *d_out, float *d_zf, float *d_corr, int64_t pix0);
int grid_op_path(const GridOp *op);                          // glf_stats.matvec_path: 1 exact grid form, 3 rank form
int grid_op_row_len(const GridOp *op);                       // samples per grid row (a row range of the operator is whole grid rows)
bool grid_op_can_skip(const GridOp *op);                     // the grid and rank forms' exact-zero skipping has something to skip (window != 0 turns it on)
// Column maxima of |X| that the kernel which wrote the operand X left behind, per block of its rows: part[b * ld + c], b < nblk,
// over ALL p rows (any partition of the rows gives the same max). With it a sweep skips its own pass over X for the scales.
struct ColMaxima {
    const float *part;
    int nblk;
};
// maxima: optional (band, grid and rank forms; ignored under OPERAND_MAXIMA=sweep)
int grid_op_apply(glf_ctx *ctx, GridOp *op, const float *X, float *Y, unsigned ld, double alpha, const double *d_degree,
                  unsigned row0, unsigned row1, int window, const ColMaxima *maxima = nullptr);

// Second level of the column reductions: out[v] = the sum (MAX: the maximum, of values >= 0) over b < nblk of
// part[(b * NV + v) * ld + col], in a fixed order. The kernel is launched with red2_grid(ld) workgroups of RED2_THREADS
// threads; a workgroup takes RED2_COLS columns, so at p = 85 264 (667 blocks of 128 rows) each of its 128 thread rows
// loads 6 blocks, all of them independent loads of one batch (a single workgroup over all the columns walked 6 - 21
// dependent batches: 8 - 16 us of L2 round trips between two sweeps of the solver). The thread rows are combined through
// LDS, 128 -> 16 -> 1. out[] is valid in threads t < RED2_COLS, for column blockIdx.x * RED2_COLS + t.
constexpr int RED2_COLS = 8, RED2_THREADS = 1024, RED2_BATCH = 8;
inline unsigned red2_grid(unsigned ld) { return ld / RED2_COLS; } // (ld is a multiple of 32)
template <typename T, int NV, bool MAX>
__device__ __forceinline__ void wg_reduce_partials(const T *__restrict__ part, int nblk, unsigned ld, T (&out)[NV],
                                                   T *sh /* LDS [NV][RED2_THREADS] */)
{
    constexpr int NP = RED2_THREADS / RED2_COLS, G = 16;
    const int t = threadIdx.x, c = t % RED2_COLS, row = t / RED2_COLS;
    const unsigned col = blockIdx.x * RED2_COLS + c;
    auto comb = [](T a, T b) {
        if constexpr (MAX) return a > b ? a : b;
        else return a + b;
    };
    T acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = T(0);
    for (int b0 = row; b0 < nblk; b0 += RED2_BATCH * NP) {
        T x[RED2_BATCH][NV]; // every load is issued (a block past the end re-reads the last one), then the valid ones are combined in order
#pragma unroll
        for (int u = 0; u < RED2_BATCH; ++u)
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int b = b0 + u * NP < nblk ? b0 + u * NP : nblk - 1;
                x[u][v] = part[((size_t)b * NV + v) * ld + col];
            }
#pragma unroll
        for (int u = 0; u < RED2_BATCH; ++u)
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if (b0 + u * NP < nblk) acc[v] = comb(acc[v], x[u][v]);
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) sh[v * RED2_THREADS + t] = acc[v];
    __syncthreads();
    if (t < RED2_COLS * G) // thread row g < G: rows g, g + G, ...
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            acc[v] = T(0);
            for (int r = row; r < NP; r += G) acc[v] = comb(acc[v], sh[v * RED2_THREADS + r * RED2_COLS + c]);
        }
    __syncthreads();
    if (t < RED2_COLS * G)
#pragma unroll
        for (int v = 0; v < NV; ++v) sh[v * RED2_THREADS + t] = acc[v];
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        T s = T(0);
        if (t < RED2_COLS)
            for (int g = 0; g < G; ++g) s = comb(s, sh[v * RED2_THREADS + g * RED2_COLS + c]);
        out[v] = s;
    }
    __syncthreads();
}

struct MatShard {
    unsigned row0 = 0, row1 = 0, rows_per_rank = 0;
    // when set, the operator is applied through the grid-factored form and `A` is not used (may be null)
    GridOp *grid = nullptr;
    double grid_alpha = 0.0;
    const double *grid_degree = nullptr;
    int grid_window = 0;
    // Exact-zero tile skipping of the split-f16 mat-vec (optional): kbox[c] = bounding box {rmin, rmax,
    // cmin, cmax} of samples [64 c, 64 c + 64); a (128-row block, 64-k tile) pair whose boxes are more
    // than `radius` pixels apart holds only entries with |2^10 A| < 2^-25, i.e. f16 hi = lo = 0.
    const int4 *kbox = nullptr;
    int radius = -1;
};
inline unsigned shard_rows_per_rank(unsigned p, int size) { return (unsigned)round_up(ceil_div(p, size), VEC_PAD); }
// rows to allocate for a p x ld vector block (zero padded) so that the all-gather blocks fit
inline unsigned vec_rows(unsigned p, const MatShard *sh, int size)
{
    const unsigned base = (unsigned)round_up(p, VEC_PAD);
    if (!sh || !sh->rows_per_rank) return base;
    const unsigned g = sh->rows_per_rank * (unsigned)size;
    return g > base ? g : base;
}
int block_matvec(glf_ctx *ctx, const float *A, int64_t lda, unsigned p, const float *X, float *Y,
                 unsigned mld, const MatShard *shard = nullptr, const ColMaxima *maxima = nullptr); // maxima: see ColMaxima (the stored forms ignore it)
// the stored split-f16 sweep's K slabs for the rows [row0, row1) (fills the 2-workgroups-per-CU residency evenly), and whether its
// tile list can hold p samples (exact-zero tile skipping)
int mv_ksplit(const glf_ctx *ctx, unsigned p, unsigned row0, unsigned row1);
bool mv_can_skip(unsigned p);
int orthonormalise(glf_ctx *ctx, float *X, unsigned n, unsigned m, unsigned ld, double *h_norms);
int normalise(glf_ctx *ctx, float *X, unsigned n, unsigned m, unsigned ld, double *h_norms);
int inverse_power_iteration(glf_ctx *ctx, const float *A, int64_t lda, unsigned p, unsigned m, unsigned ld,
                            const double *h_X0, int opti_gs, double epsilon, double inner_rtol, int max_outer,
                            float *d_eigvecs, double *h_eigvals, glf_eig_stats *stats,
                            const MatShard *shard = nullptr, const float *d_dinv = nullptr,
                            const float *d_X0_block = nullptr);

// one block solve L_A X = B by the solver's PCG, its state copied out (glf_operator_solve): see eigen.hip
int operator_solve(glf_ctx *ctx, const float *A, int64_t lda, unsigned p, unsigned m, unsigned ld, const MatShard *shard, const float *d_dinv,
                   const float *d_B, float *d_X, float *d_R, unsigned rows, double rtol, int max_it, int *iters, int *unconverged);

// m > 256 (the reference default m = p - 1): panel-major blocks, see eigen.hip
int inverse_power_iteration_panels(glf_ctx *ctx, const float *A, int64_t lda, unsigned p, unsigned m, const double *h_X0,
                                   unsigned long long seed, int opti_gs, double epsilon, double inner_rtol, int max_outer,
                                   float *d_eigvecs, double *h_eigvals, glf_eig_stats *stats, const MatShard *shard,
                                   const float *d_dinv);
int orthonormalise_panels(glf_ctx *ctx, float *X, unsigned n, unsigned m, double *h_norms, bool normalise_only);

// One Nystroem extension, as every form of it takes it (nystroem.hip): Phi[pix][j] = sum_i K(sample i, pix) * Psi[i][j] for the pixels
// [pix0, pix1). The caller names the fields it sets; the rest keep their defaults.
struct NysRequest {
    // the targets: [N] pixels in the format of coef.kernel; mask [N] != 0 and idx [p] (ascending) name the sample pixels
    const uint8_t *d_img = nullptr;
    int width = 0, height = 0;
    int64_t pix0 = 0, pix1 = 0;
    const uint8_t *d_mask = nullptr;
    const uint32_t *d_idx = nullptr;
    int raster = 0; // != 0: Phi's row = the pixel; else sample-first (the rows of the sample pixels are skipped)
    // the samples: records {row, col, value, 0}; h_idx: the host copy of d_idx when the caller has it
    const float4 *d_samples = nullptr;
    unsigned p = 0;
    KernelCoef coef{};
    const unsigned *h_idx = nullptr;
    // the operand: Psi [round_up(p, NYS_PAD)][ld] (the scale -alpha folded in), m <= ld columns in use
    const float *d_psi = nullptr;
    unsigned m = 0, ld = 0;
    // the outputs: Phi (row stride ld); d_c (optional): ld doubles, += the sum over the NON-sample pixels of Phi[pix][j] * y[pix];
    // flt (nystroem_band_filter only): the filter applied in the kernel's epilogue, Phi never written
    float *d_phi = nullptr;
    double *d_c = nullptr;
    const BandFilter *flt = nullptr;
    int window = 0; // != 0: pass over what is exactly zero (skip_exact_zeros)
    // the report, each field optional. path: 0 entry by entry, 1 exact grid form, 3 rank form, 4 band form
    float *kernel_ms = nullptr;
    uint64_t *entries_evaluated = nullptr;
    double *mfma_flops = nullptr;
    int *path = nullptr;
    RowpassStats *rowpass = nullptr;
};
int nystroem_contract(glf_ctx *ctx, const NysRequest &rq);
// The same extension with the filter fused into the band form (rq.flt set; d_phi, d_c, m, raster and window are not read).
// GLF_ERR_UNSUPPORTED: the band form does not apply (not a tensor grid, radius too large, or auto mode prefers a factored form)
int nystroem_band_filter(glf_ctx *ctx, const NysRequest &rq);
// box[c] = {rmin, rmax, cmin, cmax} of samples [64 c, 64 c + 64) (nystroem.hip)
int chunk_boxes(glf_ctx *ctx, const float4 *d_samples, unsigned p, int4 *d_box);
// Phi rows of the sample pixels <- Phi_A rows (hpc/nystroem.c:25-34 + hpc/utils.c:149-152)
int scatter_sample_rows(glf_ctx *ctx, const float *d_phiA, unsigned p, unsigned ld, const uint32_t *d_idx,
                        float *d_phi, int raster, const uint8_t *d_img, double *d_c, unsigned m);
int permute_rows(glf_ctx *ctx, const float *d_in, float *d_out, int64_t N, unsigned ld,
                 const uint32_t *d_idx, unsigned p);

// filter.hip
// out[c] = sum over the rows r of in[r][c], one workgroup per column, in an order that depends on nrows alone
__global__ void k_cols_sum(const double *__restrict__ in, int nrows, unsigned ld, double *__restrict__ out);
int phi_t_y(glf_ctx *ctx, const float *d_phi, const uint8_t *d_img, int64_t pix0, int64_t pix1, unsigned m,
            unsigned ld, double *d_c);
void note_apply(glf_ctx *ctx, unsigned kernel, unsigned ld, int64_t npix, int ppb, int64_t nblk); // (filter.hip; glf_filter_info)
int phi_gram(glf_ctx *ctx, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, double *d_G); // Phi^T Phi (f64 [ld][ld])
int apply_filter(glf_ctx *ctx, const uint8_t *d_img, const float *d_phi, int64_t pix0, int64_t pix1,
                 unsigned m, unsigned ld, const float *d_w, float gain, float ysub, uint8_t *d_out, float *d_zf,
                 float *d_corr = nullptr);
// extra signal planes (glf_image_processing_signals): d_sig / d_out [nsig][N] float, rows [pix0, pix1) only;
// d_c [nsig][ld] (f64) = Phi^T s_k over this rank's pixels; d_w [nsig][ld]
int phi_t_signals(glf_ctx *ctx, const float *d_phi, const float *d_sig, int64_t N, int nsig, int64_t pix0, int64_t pix1, unsigned ld,
                  double *d_c);
int plane_absmax(glf_ctx *ctx, const float *d_s, int64_t n, float *h_max); // max |s| of a device float array
int filter_sample_rows_signals(glf_ctx *ctx, const float *d_phiA, unsigned n, unsigned ld, const uint32_t *d_idx, int nsig, const float *d_w,
                               float gain, float ysub, const float *d_sig, float *d_out, int64_t N);
int apply_filter_signals(glf_ctx *ctx, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, int nsig, const float *d_w, float gain,
                         float ysub, const float *d_sig, float *d_out, int64_t N);
// the same filter panel by panel (m > 256): acc[px - pix0] (+)= sum_j Phi[px][j] w[j], then z = (1 - ysub) y + gain * acc
int filter_accumulate(glf_ctx *ctx, const float *d_phi, int64_t pix0, int64_t pix1, unsigned ld, const float *d_w, float *d_acc,
                      bool first);
int filter_finish(glf_ctx *ctx, const uint8_t *d_img, const float *d_acc, int64_t pix0, int64_t pix1, float gain, float ysub,
                  uint8_t *d_out, float *d_zf);

// graph_fit.hip: h_G [m][m] = Phi^T diag(w) Phi (exactly symmetric) and h_b [nplanes][m] = Phi^T diag(w) s_k of Phi [N][ld] in one pass
// (d_w NULL: w = 1; nplanes 0: no planes); returns with the stream drained
int graph_normal_equations(glf_ctx *ctx, const float *d_phi, int64_t N, unsigned m, unsigned ld, const float *d_w, int nplanes,
                           const float *d_planes, double *h_G, double *h_b);
// ... of a handle of either storage: on a compact one the f16 instance forms them on the stored halves, and the column scales are
// folded into the read-back in f64 (G[i][j] 2^(e_i + e_j), b_k[c] 2^e_c: the bits of the f32 pass over Q)
int graph_normal_equations(const glf_graph *g, const float *d_w, int nplanes, const float *d_planes, double *h_G, double *h_b);
// graph.hip: d_out[i] = Phi[h_px[i]][0 .. dim) (Q on a compact handle) for the pixels 0 <= h_px[i] < N the caller names, by the row
// gather of graph_sample_rows (queued)
int graph_gather_rows(glf_graph *g, int dim, unsigned nrows, const int64_t *h_px, float *d_out);

} // namespace glf
