// affinity_grid.inc -- the degree D_A = rowsum [K_A K_B] (hpc/laplacian.c:18-20) refactored for a tensor-grid sample
// set (samples (a, b) at grid row R_a, grid column C_b; hpc/sampling.c:6-23 always produces one).
// Included by affinity.hip inside namespace glf, after grid_common.inc.
//
//   D[(a,b)] = sum_{r,c} Er(r - R_a) Ec(c - C_b) P(|v_ab - img[r][c]|)
//            = sum_v P(|v_ab - v|) * Z[a][v][b],   Z[a][v][b] = sum_r Er(r - R_a) * Wt[r][v][b],
//   Wt[r][v][b] = sum_{c : img[r][c] = v} Ec(c - C_b)          (an Ec-weighted histogram of image row r).
//
// The same sum in another order (nothing truncated): p N kernel evaluations become N nc additions for Wt,
// nr H 256 nc f64 FMAs for Z and 256 p for the last step -- 1.4e12 -> about 1e11 operations at cfg4.
//   k_dgrid_hist : one workgroup per image row; pixels grouped by value (the counting sort of grid_common.inc);
//                  lane = grid column b; a group's Ec rows are added in ascending column order (f32). Round 3: the row's sorted
//                  columns in LDS and several pixels' gathers in flight (1.25 -> 0.94 ms), then each group of 64 columns walking
//                  only the contiguous run of a value's pixels within its reach (0.81). Tried and slower: a wave-uniform reach
//                  test per (pixel, group) (1.65 ms), the value's histogram row in LDS with one gather + one ds_add_f32 per pixel
//                  over the pixel's own window (5.0 ms), a conflict-free per-phase table for uniform grids (1.53 ms).
//   k_dgrid_zmfma: the row contraction Z = Er^T Wt as a split-f16 MFMA GEMM, f32 partial sums per chunk of 512 image rows
//                  (round 1: f64 FMAs on the vector pipe, 4.85 ms at cfg4). Exact-zero skipping drops the k-steps whose Er
//                  fragments are all zero -- their products would add +0 to every accumulator: bit-identical.
//   k_dgrid_final_parts: D[(a,b)] = sum_v P (sum_chunks Z) in f64, chunks and v ascending.
// All reductions run in a fixed order: bitwise reproducible, and identical between the dense and the skipping sweep.


// Wt[rl][v][b] for one image row. Ec(c - C_b) comes from an LDS copy of the factor table (index clamped to `ne - 1`,
// where the factor is exactly 0 or the table ends) -- reading the (W x nc) table row of every pixel instead cost 20 GB
// of L2 traffic per image (3.7 ms vs 1 ms at cfg4).
// WEIGHTED: every pixel's Ec term is multiplied by its value in the float plane `wplane` (rows from the shard's first row):
// Wt_s[r][v][b] = sum_{c : img[r][c] = v} s[r][c] Ec(c - C_b), the histogram of the value-weighted sums Phi^T s (joint filtering)
constexpr int DGRID_NE_MAX = 8192;
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_dgrid_hist(const float *__restrict__ etab, int ne, const int *__restrict__ gcol, int nc,
                                                     int ncp, const unsigned short *__restrict__ scol,
                                                     const unsigned *__restrict__ goff, int width, float *__restrict__ Wt,
                                                     const float *__restrict__ wplane, int pexp)
{
    extern __shared__ float etab_s[]; // [ne], then the row's value-sorted columns u16 [width] (WEIGHTED: then the row's weights)
    unsigned short *sc_s = reinterpret_cast<unsigned short *>(etab_s + ne);
    float *w_s = reinterpret_cast<float *>(etab_s + ne + (width + 1) / 2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = blockIdx.x;
    const unsigned short *sc = scol + (size_t)rl * width;
    const unsigned *go = goff + (size_t)rl * 257;
    for (int i = threadIdx.x; i < ne; i += 256) etab_s[i] = etab[i];
    // (the loop below walks a value's pixels one after the other: a global load of the column per pixel put its latency on
    // every step; from LDS, and with eight pixels' gathers in flight at a time, 1.25 -> 0.94 ms at cfg4)
    for (int i = threadIdx.x; i < width; i += 256) sc_s[i] = sc[i];
    if (WEIGHTED)
        for (int i = threadIdx.x; i < width; i += 256) w_s[i] = ldexpf(wplane[(size_t)rl * width + i], -pexp); // (pexp = 0: the plane's bits)
    __syncthreads();
    constexpr int NB = 10; // ncp <= 640
    int gc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) gc[i] = lane + 64 * i < nc ? gcol[lane + 64 * i] : -(1 << 28); // padding columns: factor 0
    // reach of each group of 64 grid columns (wave-uniform): with a table that ends in an exact zero (ne - 1 = the radius) a
    // pixel farther than that from every column of the group adds +0 to all of its 64 accumulators. A value's pixels are sorted
    // by column, so the ones within reach of a group are a contiguous run of the list: each group walks its own run (1 - 2 of
    // the 5 groups per pixel at cfg4) and the additions of a bin keep their ascending-column order -- the same sums.
    const bool zero_tail = __builtin_amdgcn_readfirstlane((int)(etab_s[ne - 1] == 0.f)) != 0;
    int glo[NB], ghi[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const bool have = 64 * i < nc;
        glo[i] = __builtin_amdgcn_readfirstlane(have ? (zero_tail ? gcol[64 * i] - (ne - 1) : -(1 << 28)) : (1 << 28));
        ghi[i] = __builtin_amdgcn_readfirstlane(have ? (zero_tail ? gcol[min(64 * i + 63, nc - 1)] + (ne - 1) : (1 << 28)) : -(1 << 28));
    }
    for (int v = wave; v < 256; v += 4) {
        const int g0 = (int)go[v], g1 = (int)go[v + 1];
        float acc[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[i] = 0.f;
        for (int kb = g0; kb < g1; kb += 64) { // 64 pixels of the value at a time: lane = pixel for the run search
            const int nk = min(64, g1 - kb);
            const int cl = lane < nk ? (int)sc_s[kb + lane] : (1 << 29);
#pragma unroll
            for (int i = 0; i < NB; ++i)
                if (64 * i < ncp) {
                    const unsigned long long in = __ballot(cl > glo[i] && cl < ghi[i]); // (a contiguous run of bits)
                    if (in == 0ull) continue;
                    const int k0 = kb + __builtin_ctzll(in), k1 = k0 + __builtin_popcountll(in);
                    int k = k0;
                    if (WEIGHTED) {
                        for (; k < k1; ++k) {
                            const int c0 = (int)sc_s[k];
                            acc[i] = fmaf(w_s[c0], etab_s[min(abs(c0 - gc[i]), ne - 1)], acc[i]);
                        }
                        continue;
                    }
                    for (; k + 4 <= k1; k += 4) { // (the additions stay in pixel order: only the gathers are hoisted)
                        const int c0 = (int)sc_s[k], c1 = (int)sc_s[k + 1], c2 = (int)sc_s[k + 2], c3 = (int)sc_s[k + 3]; // wave-uniform
                        const float e0 = etab_s[min(abs(c0 - gc[i]), ne - 1)], e1 = etab_s[min(abs(c1 - gc[i]), ne - 1)];
                        const float e2 = etab_s[min(abs(c2 - gc[i]), ne - 1)], e3 = etab_s[min(abs(c3 - gc[i]), ne - 1)];
                        acc[i] = (((acc[i] + e0) + e1) + e2) + e3;
                    }
                    for (; k < k1; ++k) acc[i] += etab_s[min(abs((int)sc_s[k] - gc[i]), ne - 1)];
                }
        }
        float *dst = Wt + ((size_t)rl * 256 + v) * ncp;
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (lane + 64 * i < ncp) dst[lane + 64 * i] = acc[i];
    }
}

// ---- the row contraction on the f16 matrix pipe ---------------------------------------------------------------------------
// Z[a][n] = sum_r Er(r - R_a) Wt[r][n] is a GEMM [nr x H] x [H x 256 ncp] (1.8e11 flop at cfg4: 4.85 ms as f64 FMAs on the vector
// pipe, the largest part of the affinity stage). Both operands split into f16 (hi, lo) pairs as everywhere else (2^15 Er from a
// fragment table, 2^wsh Wt split in registers), three v_mfma_f32_32x32x16_f16 per multiply-add, f32 accumulation over a chunk
// of DGZ_CHUNK image rows only: the chunk sums are written as f32 and added in f64 by k_dgrid_final, so the f32 rounding of an
// accumulator (~3e-7 relative after 32 k-steps) averages over chunks x values instead of growing with the image height
// (measured: D_A rel. error vs the fp64 oracle stays ~2e-8).
typedef _Float16 dg_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 dg_f16x2 __attribute__((ext_vector_type(2)));
typedef float dg_f32x2 __attribute__((ext_vector_type(2)));
typedef float dg_f32x16 __attribute__((ext_vector_type(16)));
constexpr int DGZ_CHUNK = 512; // image rows per f32 partial sum (32 k-steps)
constexpr int DGZ_MG = 5;      // m-tiles (32 grid rows each) per wave: with 2 n-tiles, 10 accumulators

// A fragments of 2^15 Er(r - R_a) with the GRID rows as the MFMA rows: [k-step][m-tile][hi, lo][lane][8 halves]; lane l holds grid
// row a = 32 mtile + l % 32 and image rows r = row0 + 16 kstep + 8 (l / 32) + j. kact[kstep * mgroups + g] = some entry of the
// m-tiles of group g (mg tiles: DGZ_MG, or 2 DGZ_MG in the single-group shape) in this k-step is non-zero.
__global__ __launch_bounds__(64) void k_dgrid_erfrag(const float *__restrict__ etab, const int *__restrict__ grow, int nr, int mtiles,
                                                      int row0, int nrows, _Float16 *__restrict__ Ef, unsigned short *__restrict__ kact,
                                                      int mgroups, int mg, const int *__restrict__ chunk_mt0)
{
    const int kstep = blockIdx.x, lane = threadIdx.x, half = lane >> 5;
    dg_f16x8 *out = reinterpret_cast<dg_f16x8 *>(Ef);
    for (int g = 0; g < mgroups; ++g) {
        unsigned bits = 0; // bit (mt - first m-tile of the group): some entry of that m-tile in this k-step is non-zero
        // (window shape: one group per chunk of image rows, starting at the chunk's first m-tile within the radius)
        const int gbase = chunk_mt0 ? chunk_mt0[kstep / (DGZ_CHUNK / 16)] : g * mg;
        for (int mt = gbase; mt < min(mtiles, gbase + mg); ++mt) {
            bool any = false;
            const int a = 32 * mt + (lane & 31);
            dg_f16x8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int rl = 16 * kstep + 8 * half + j;
                const float val = (a < nr && rl < nrows) ? 32768.f * etab[abs(row0 + rl - grow[a])] : 0.f;
                const _Float16 h = (_Float16)val;
                hi[j] = h;
                lo[j] = (_Float16)(val - (float)h);
                any |= val != 0.f;
            }
            out[(((size_t)kstep * mtiles + mt) * 2 + 0) * 64 + lane] = hi;
            out[(((size_t)kstep * mtiles + mt) * 2 + 1) * 64 + lane] = lo;
            if (__ballot(any)) bits |= 1u << (mt - gbase);
        }
        if (lane == 0) kact[(size_t)kstep * mgroups + g] = (unsigned short)bits;
    }
}

// grid (ncols / (64 NW), m-groups, chunks); NW waves, wave w takes the two 32-column n-tiles 2 (NW blockIdx.x + w) + {0, 1}.
// The A fragments of a k-step (DGZ_MG m-tiles, 10 KB) are shared by the NW waves: copied global -> LDS by LDS-DMA one k-step
// ahead (two buffers), so the matrix pipe never waits for the L2 round trip of its own operands (read straight from L2 per wave
// the contraction ran at a third of this rate). Zpart[chunk][a][n] (f32) = 2^-(15 + wsh) sum over the chunk's image rows.
// MG m-tiles (32 grid rows each) x NT n-tiles (32 columns) per wave: (5, 2), or (10, 1) when all the grid rows fit ten m-tiles --
// Wt is then read once instead of once per group of five m-tiles (2.4 -> 1.2 GB at cfg4: the kernel is bound by that stream).
template <bool SKIP, int NW, int MG, int NT>
__global__ __launch_bounds__(NW * 64) void k_dgrid_zmfma(const _Float16 *__restrict__ Ef, const unsigned short *__restrict__ kact,
                                                          const float *__restrict__ Wt, int ncols, int nrows, int nr, int mtiles,
                                                          int mgroups, float wscale, float outscale, float *__restrict__ Zpart,
                                                          const int *__restrict__ chunk_mt0)
{
    __shared__ __attribute__((aligned(16))) float4 abuf[2][MG * 2 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int n0 = (blockIdx.x * NW + wave) * (32 * NT); // (ncols is a multiple of 32 NT NW: checked on the host)
    const int g = blockIdx.y, mt0 = chunk_mt0 ? chunk_mt0[blockIdx.z] : g * MG, mtn = min(MG, mtiles - mt0);
    const int ks0 = blockIdx.z * (DGZ_CHUNK / 16), ks1 = min(ks0 + DGZ_CHUNK / 16, (nrows + 15) / 16);
    const float4 *Efv = reinterpret_cast<const float4 *>(Ef);
    dg_f32x16 acc[MG][NT];
#pragma unroll
    for (int mt = 0; mt < MG; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;
    // this lane's B entries of a k-step: rows r = 16 kstep + 8 half + j, columns n0 + 32 nt + l31 (clamped to the last row: the
    // A fragments of rows past the shard are zero)
    auto load_b = [&](float (&w)[NT][8], int kstep) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int rl = min(16 * kstep + 8 * half + j, nrows - 1);
            const float *row = Wt + (size_t)rl * ncols + n0 + l31;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) w[nt][j] = row[32 * nt];
        }
    };
    auto stage_a = [&](int kstep, int buf) { // the (hi, lo) KiB pieces of this k-step's m-tiles that have a non-zero entry
        const unsigned bits = (unsigned)__builtin_amdgcn_readfirstlane((int)kact[(size_t)kstep * mgroups + g]);
        const char *src = reinterpret_cast<const char *>(Efv + ((size_t)kstep * mtiles + mt0) * 2 * 64);
        const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_offset_of(abuf[buf]));
        for (int q = __builtin_amdgcn_readfirstlane(wave); q < mtn * 2; q += NW) // (wave-uniform)
            if ((bits >> (q >> 1)) & 1u)
                lds_dma_16B(src + (size_t)q * 1024 + lane * 16, (unsigned)__builtin_amdgcn_readfirstlane((int)(dst + (unsigned)q * 1024u)));
    };
    float wc[NT][8], wn[NT][8];
    if (ks0 < ks1) {
        stage_a(ks0, 0);
        load_b(wc, ks0);
    }
    lds_dma_drain();
    __syncthreads();
    for (int kstep = ks0; kstep < ks1; ++kstep) {
        const int buf = (kstep - ks0) & 1;
        if (kstep + 1 < ks1) { // in flight while this k-step is split and contracted
            stage_a(kstep + 1, buf ^ 1);
            load_b(wn, kstep + 1);
        }
        // m-tiles whose Er fragments are all zero in this k-step (the grid rows farther than the table's radius from all 16 image
        // rows: 4 of 5 at cfg4) are passed over: their MFMAs would add +0 to every accumulator -- the sums are bit-identical with or
        // without them, so this is not tied to glf_options.skip_exact_zeros (SKIP, which also drops the step's operand split)
        const unsigned bits = (unsigned)__builtin_amdgcn_readfirstlane((int)kact[(size_t)kstep * mgroups + g]);
        if (!SKIP || bits) {
            dg_f16x8 bh[NT], bl[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    dg_f32x2 yy;
                    yy[0] = wc[nt][j] * wscale;
                    yy[1] = wc[nt][j + 1] * wscale;
                    const dg_f16x2 h2 = __builtin_convertvector(yy, dg_f16x2);
                    dg_f32x2 res;
                    res[0] = yy[0] - (float)h2[0]; // exact in f32
                    res[1] = yy[1] - (float)h2[1];
                    const dg_f16x2 l2 = __builtin_convertvector(res, dg_f16x2);
                    bh[nt][j] = h2[0];
                    bh[nt][j + 1] = h2[1];
                    bl[nt][j] = l2[0];
                    bl[nt][j + 1] = l2[1];
                }
            const dg_f16x8 *af = reinterpret_cast<const dg_f16x8 *>(abuf[buf]);
#pragma unroll
            for (int mt = 0; mt < MG; ++mt) {
                if (mt < mtn && ((bits >> mt) & 1u)) { // uniform
                    const dg_f16x8 ah = af[(mt * 2 + 0) * 64 + lane];
                    const dg_f16x8 al = af[(mt * 2 + 1) * 64 + lane];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[nt], acc[mt][nt], 0, 0, 0);
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[nt], acc[mt][nt], 0, 0, 0);
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[nt], acc[mt][nt], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 8; ++j) wc[nt][j] = wn[nt][j];
        lds_dma_drain(); // this wave's pieces of the next k-step have landed ...
        __syncthreads(); // ... and everybody else's; buffer `buf` is free again
    }
    // C layout: register i of this lane is grid row 32 (mt0 + mt) + (i & 3) + 8 (i >> 2) + 4 half, column n0 + 32 nt + l31
    float *out = Zpart + (size_t)blockIdx.z * nr * ncols;
#pragma unroll
    for (int mt = 0; mt < MG; ++mt)
        if (mt < mtn)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int a = 32 * (mt0 + mt) + (i & 3) + 8 * (i >> 2) + 4 * half;
                if (a < nr) {
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) out[(size_t)a * ncols + n0 + 32 * nt + l31] = acc[mt][nt][i] * outscale;
                }
            }
}

// D[(a,b)] = sum_v P(|v_ab - v|) sum_chunks Zpart[chunk][a][v][b], both sums in f64 in a fixed order: 32 samples per workgroup,
// 8 threads per sample taking the values v = t, t + 8, ... (one thread per sample walked 2048 strided loads one after the other:
// 0.9 ms at cfg4), their partial sums added in thread order.
__global__ __launch_bounds__(256) void k_dgrid_final_parts(const float *__restrict__ Zpart, int nchunks, const float *__restrict__ ptab,
                                                            const float4 *__restrict__ samples, int nr, int nc, int ncp,
                                                            double *__restrict__ degree, double *__restrict__ ysum,
                                                            const int *__restrict__ grow, int row0, int radius, double dscale)
{
    // ysum (optional): U[s] = sum over the same pixels of K(s, px) y[px] -- the pixel's value rides along with its
    // histogram bin (y = v), so it is the same sum with v P in place of P: the whole of c = Phi^T y for the extended
    // rows then follows from Psi^T U without Phi (band form of the Nystroem stage with the filter in its epilogue)
    __shared__ double sh[8][32], shu[8][32];
    const int sl = threadIdx.x & 31, vl = threadIdx.x >> 5;
    const int s = blockIdx.x * 32 + sl;
    const bool live = s < nr * nc;
    double d = 0.0, u = 0.0;
    if (live) {
        const int a = s / nc, b = s % nc;
        const int sv = (int)samples[s].z;
        const size_t ncols = (size_t)256 * ncp, cstride = (size_t)nr * ncols;
        const float *z = Zpart + (size_t)a * ncols + b;
        // chunks of DGZ_CHUNK image rows all farther than the table's radius (its first exact zero) from this grid row hold
        // exact zeros (every Er fragment of theirs is zero): not read -- adding +0 leaves the sum as it is
        // A grid row out of reach above the shard (ra + radius - 1 < 0) has an empty range: its m-tile may lie below the first
        // one k_dgrid_zmfma stored for chunk 0 in window shape, so chunk 0 must not be read for it.
        const int ra = grow[a] - row0, hi = ra + radius - 1;
        const int c_lo = max(0, (ra - radius + 1) / DGZ_CHUNK), c_hi = hi < 0 ? -1 : min(nchunks - 1, hi / DGZ_CHUNK);
        for (int v = vl; v < 256; v += 8) {
            double zs = 0.0;
            for (int c = c_lo; c <= c_hi; ++c) zs += (double)z[(size_t)c * cstride + (size_t)v * ncp];
            const double pz = (double)ptab[abs(sv - v)] * zs;
            d = fma((double)ptab[abs(sv - v)], zs, d);
            u = fma((double)v, pz, u);
        }
    }
    sh[vl][sl] = d;
    shu[vl][sl] = u;
    __syncthreads();
    if (vl == 0 && live) {
        double t = sh[0][sl], tu = shu[0][sl];
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            t += sh[k][sl];
            tu += shu[k][sl];
        }
        degree[s] = t * dscale; // (1, or the power of two a far-scaled weight plane was divided by: exact)
        if (ysum) ysum[s] = tu;
    }
}

// GLF_ERR_UNSUPPORTED = not a grid (or too wide): the caller runs the direct sweep.
// d_wplane (joint filtering): d_degree receives U_s[(a,b)] = sum over the shard's pixels of K(sample, px) s[px] instead, with
// s = the float plane d_wplane [height][width] (absolute rows) and wabs >= max |s| (the f16 operand scale); d_ysum must be null.
static int degree_rows_grid(glf_ctx *ctx, const uint8_t *d_img, int width, int height, int row0, int row1,
                            const float4 *d_samples, unsigned p, const unsigned *h_idx, KernelCoef coef, double *d_degree,
                            int window, double *evaluated, double *d_ysum, const float *d_wplane = nullptr, double wabs = 1.0)
{
    if (!grid_path_wanted(ctx->tune.deg_path, width) || width > GRID_MAX_W || p < 4 || row0 >= row1 || !grey_levels_factor(coef.kernel))
        return GLF_ERR_UNSUPPORTED;
    std::vector<uint32_t> idx(h_idx, h_idx + p);
    GridInfo g;
    if (!detect_grid(idx, width, g) || round_up(g.nc, 4) > 640) return GLF_ERR_UNSUPPORTED;
    hipStream_t st = ctx->stream;
    GridTables gt;
    GLF_TRY(gt.build(ctx, g, coef, d_img, width, height, row0, row1));
    const int nrows = row1 - row0, ncols = 256 * gt.ncp;
    DevBuf<float> Wt;
    GLF_TRY(Wt.alloc(ctx, (size_t)nrows * ncols));
    // entries of the factor table the histogram needs: up to the first exact zero (kept as the clamp target)
    const int ne = std::min(gt.maxdim, gt.radius + 1);
    if (ne > DGRID_NE_MAX) return GLF_ERR_UNSUPPORTED; // (a kernel this wide on an image this large: the direct sweep runs)
    // A weight plane far from 1 (max |s| below 2^-40 or above 2^100) is divided by the power of two 2^pexp of its maximum as the
    // histogram reads it, and the sums are multiplied by it in f64 at the end: with the plane as it is, the f32 histogram sums and
    // the f32 chunk sums Zpart underflow below about 2^-60 (and 2^wsh overflows below 2^-113), and Zpart overflows above about
    // 2^118. Both scalings are exact, so U_s(2^k s) = 2^k U_s(s) bit for bit; a plane within the range keeps pexp = 0 and its bits.
    int pexp = 0;
    if (d_wplane && wabs > 0.0 && std::isfinite(wabs)) {
        int aexp = 0;
        (void)std::frexp(wabs, &aexp);
        if (aexp < -40 || aexp > 100) pexp = aexp;
    }
    if (d_wplane)
        hipLaunchKernelGGL(k_dgrid_hist<true>, dim3(nrows), dim3(256), (size_t)ne * sizeof(float) + (size_t)((width + 1) / 2) * 4 + (size_t)width * 4,
                           st, gt.etab(), ne, gt.gcol(), gt.nc, gt.ncp, gt.scol.p, gt.goff.p, width, Wt.p, d_wplane + (size_t)row0 * width, pexp);
    else
        hipLaunchKernelGGL(k_dgrid_hist<false>, dim3(nrows), dim3(256), (size_t)ne * sizeof(float) + (size_t)width * 2, st, gt.etab(), ne, gt.gcol(), gt.nc,
                           gt.ncp, gt.scol.p, gt.goff.p, width, Wt.p, (const float *)nullptr, 0);
    const bool skip = window && gt.can_skip(coef);
    // row contraction on the matrix pipe (k_dgrid_zmfma): Wt entries are sums of Ec over a row's pixels of one value, bounded by
    // the whole factor table's mass -> one power-of-two scale keeps 2^wsh Wt below the f16 range
    double wmax = 0.0;
    {
        const double s_loc = (double)coef.s_loc;
        for (int d = 1; d < width; ++d) wmax += std::exp2(-s_loc * (double)d * (double)d);
        wmax = 1.0 + 2.0 * wmax;
        if (d_wplane) wmax *= wabs > 0.0 ? std::ldexp(wabs, -pexp) : 1.0; // signed weights: |Wt_s| <= max |s| x the table's mass
    }
    int wexp = 0;
    (void)std::frexp(wmax, &wexp);       // wmax < 2^wexp
    const int wsh = 14 - wexp;           // 2^wsh wmax < 2^14
    const int mtiles = (int)ceil_div(gt.nr, 32);
    constexpr int ZNW = 8;
    // one group of up to ten m-tiles with one n-tile per wave when the grid rows fit (Wt read once), else groups of five with two
    const int ksteps = (int)ceil_div(nrows, 16), nchunks = (int)ceil_div(nrows, DGZ_CHUNK);
    // window shape: a chunk of 512 image rows reaches the grid rows within the table's radius only -- three or four m-tiles at
    // cfg4 -- so a wave carries four accumulators instead of ten (two workgroups per CU instead of one: the kernel is bound by
    // the latency of its k-steps), Wt is still read once, and the tiles out of reach are neither computed nor stored (the final
    // sums skip the same chunks by the same criterion)
    constexpr int ZWIN = 4;
    std::vector<int> h_mt0(nchunks, 0);
    bool window_ok = gt.radius < gt.maxdim && ncols % (32 * ZNW) == 0 && !ctx->tune.zmfma_groups;
    for (int c = 0; c < nchunks && window_ok; ++c) {
        const int r_lo = row0 + c * DGZ_CHUNK - (gt.radius - 1), r_hi = row0 + (c + 1) * DGZ_CHUNK - 1 + (gt.radius - 1); // (whole chunk, as k_dgrid_final_parts reckons)
        const int a_lo = (int)(std::lower_bound(g.rows.begin(), g.rows.end(), r_lo) - g.rows.begin());
        const int a_hi = (int)(std::upper_bound(g.rows.begin(), g.rows.end(), r_hi) - g.rows.begin()) - 1;
        h_mt0[c] = a_hi >= a_lo ? a_lo / 32 : 0;
        if (a_hi >= a_lo && a_hi / 32 - a_lo / 32 + 1 > ZWIN) window_ok = false;
    }
    const bool one_group = !window_ok && mtiles > DGZ_MG && mtiles <= 2 * DGZ_MG && ncols % (32 * ZNW) == 0 && !ctx->tune.zmfma_groups;
    const int mg = window_ok ? ZWIN : one_group ? 2 * DGZ_MG : DGZ_MG, ntw = (window_ok || one_group) ? 1 : 2;
    const int mgroups = window_ok ? 1 : (int)ceil_div(mtiles, mg);
    DevBuf<int> chunk_mt0;
    if (window_ok) {
        GLF_TRY(chunk_mt0.alloc(ctx, nchunks));
        GLF_HIP(ctx, hipMemcpyAsync(chunk_mt0.p, h_mt0.data(), sizeof(int) * nchunks, hipMemcpyHostToDevice, st)); // (h_mt0 outlives the synchronise below)
    }
    DevBuf<_Float16> Ef;
    DevBuf<unsigned short> kact;
    DevBuf<float> Zpart;
    GLF_TRY(Ef.alloc(ctx, (size_t)ksteps * mtiles * 2 * 64 * 8));
    GLF_TRY(kact.alloc(ctx, (size_t)ksteps * mgroups));
    GLF_TRY(Zpart.alloc(ctx, (size_t)nchunks * gt.nr * ncols));
    hipLaunchKernelGGL(k_dgrid_erfrag, dim3(ksteps), dim3(64), 0, st, gt.etab(), gt.grow(), gt.nr, mtiles, row0, nrows, Ef.p, kact.p, mgroups, mg,
                       window_ok ? chunk_mt0.p : nullptr);
    if (ncols % (32 * ntw * ZNW)) return set_error(ctx, GLF_ERR_INVALID, "grid degree: %d columns", ncols);
    const dim3 zgrid((unsigned)ceil_div(ncols, 32 * ntw * ZNW), (unsigned)mgroups, (unsigned)nchunks);
    const float wscale = std::ldexp(1.0f, wsh), outscale = std::ldexp(1.0f, -15 - wsh);
#define GLF_ZMFMA(SKIP_, MG_, NT_)                                                                                                          \
    hipLaunchKernelGGL((k_dgrid_zmfma<SKIP_, ZNW, MG_, NT_>), zgrid, dim3(ZNW * 64), 0, st, Ef.p, kact.p, Wt.p, ncols, nrows, gt.nr, mtiles, \
                       mgroups, wscale, outscale, Zpart.p, window_ok ? chunk_mt0.p : (const int *)nullptr)
    if (window_ok) {
        if (skip) GLF_ZMFMA(true, ZWIN, 1);
        else GLF_ZMFMA(false, ZWIN, 1);
    } else if (one_group) {
        if (skip) GLF_ZMFMA(true, 2 * DGZ_MG, 1);
        else GLF_ZMFMA(false, 2 * DGZ_MG, 1);
    } else {
        if (skip) GLF_ZMFMA(true, DGZ_MG, 2);
        else GLF_ZMFMA(false, DGZ_MG, 2);
    }
#undef GLF_ZMFMA
    hipLaunchKernelGGL(k_dgrid_final_parts, dim3((p + 31) / 32), dim3(256), 0, st, Zpart.p, nchunks, gt.ptab(), d_samples, gt.nr, gt.nc,
                       gt.ncp, d_degree, d_ysum, gt.grow(), row0, gt.radius < gt.maxdim ? gt.radius : (1 << 28), std::ldexp(1.0, pexp));
    GLF_LAUNCH_CHECK(ctx);
    GLF_HIP(ctx, hipStreamSynchronize(st));
    { // kernel entries represented by the factored sums
        double rows_in = (double)g.nr * nrows, cols_in = (double)g.nc * width;
        if (skip) { // (row, grid row) and (column, grid column) pairs closer than the exact-zero radius
            rows_in = cols_in = 0.0;
            for (int a = 0; a < g.nr; ++a)
                rows_in += std::max(0, std::min(row1, g.rows[a] + gt.radius) - std::max(row0, g.rows[a] - gt.radius + 1));
            for (int b = 0; b < g.nc; ++b)
                cols_in += std::max(0, std::min(width, g.cols[b] + gt.radius) - std::max(0, g.cols[b] - gt.radius + 1));
        }
        if (evaluated) *evaluated = rows_in * cols_in;
        // (what glf_Degree_ex reports: the shape of k_dgrid_zmfma that ran, its chunks of DGZ_CHUNK image rows and its m-groups)
        ctx->deg_note = {1, window_ok ? 2 : one_group ? 1 : 0, skip ? 1 : 0, nchunks, mgroups, rows_in * cols_in};
    }
    return GLF_OK;
}
