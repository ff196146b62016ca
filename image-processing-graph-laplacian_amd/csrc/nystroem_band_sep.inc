// Band form, fused filter in separable rank-R form (included from nystroem_grid.inc after nystroem_band_vec.inc, inside namespace glf).
//
// k_band_vec evaluates s[px] = sum_{a,b} Er(r - R_a) Ec(c - C_b) P(|v_px - v_ab|) q_ab pair by pair: one LDS gather of P and
// about five vector instructions per (pixel, sample). With the expansion P(|v - w|) = sum_{k < R} f_k(v) f_k(w) of the rank form
// (rank_tables, nystroem_rank.inc: f64 factor, R = 32 at h_val = 30, max error 1.5e-11, sum_k |f_k(v) f_k(w)| <= 1) every factor of a
// term depends on the pixel's row, its column or its value alone, and the sum factors:
//   G[a][b][k] = f_k(v_ab) q_ab                         k_band_sep_g     p R values per plane
//   S[r][b][k] = sum_a Er15(|r - R_a|) G[a][b][k]       k_band_sep_rows  one fmaf chain per element, a ascending
//   U_k[px]    = sum_b Ec(|c - C_b|) S[r][b][k]         k_band_sep_cols  one gather of Ec + R FMAs per (pixel, sample column)
//   s[px]      = sum_k f_k(v_px) U_k[px]                                 folded in f64, then band_filter_store
// In the column pass a wave is 64 pixels of one image row, so S[r][b][.] is wave-uniform: it is fetched by scalar loads and enters the
// FMAs as their scalar operand. No gather of P, no support test, no select: the support is the square |dr|, |dc| < rad (Er15 and
// Ec are exact zeros from rad on) instead of k_band_vec's circle -- the corners add terms below 2^-40 of the largest one.
// Layouts: G [plane][a][b][k], S [row][plane][b][k] (k fastest: a (row, b)'s terms are R consecutive floats = one or two scalar
// loads; a thread of the row pass owns one (plane, b, k) and walks a, so its loads and stores are contiguous over the wave).

constexpr int BSEP_RB = 8;                 // image rows a thread of the row pass holds (G is read once per block of rows)
constexpr int BSEP_ATILE = 128;            // band rows whose Er15 sit in LDS at a time (BAND_MAXROWS covers a block of rows at once)
constexpr size_t BSEP_S_BYTES = 256u << 20; // S of one chunk of image rows: the headline's 153 MB in one piece
static_assert(BSEP_RB == BAND_NW, "a block of the row pass is the rows of one workgroup of the column pass");
static_assert(BSEP_ATILE >= BAND_MAXROWS, "without BAND_NOSKIP one tile holds the band of a block of rows");

// q_k[s] = (float)(Psi[s] . w_k) as k_band_q has it (band_q_row), then G[k][s][t] = ftab[t][v_s] q_k[s]. One thread per sample.
template <int NC>
__global__ __launch_bounds__(256) void k_band_sep_g(const float *__restrict__ psi, unsigned p, unsigned ld, const float *__restrict__ w,
                                                    const float *__restrict__ sig_w, const uint8_t *__restrict__ svals,
                                                    const float *__restrict__ ftab, int R, float *__restrict__ G)
{
    const unsigned s = blockIdx.x * 256 + threadIdx.x;
    if (s >= p) return;
    double acc[NC];
    band_q_row<NC>(psi + (size_t)s * ld, ld, w, sig_w, acc);
    const int v = (int)svals[s];
    for (int t = 0; t < R; t += 4) {
        const float f0 = ftab[(t + 0) * 256 + v], f1 = ftab[(t + 1) * 256 + v], f2 = ftab[(t + 2) * 256 + v], f3 = ftab[(t + 3) * 256 + v];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const float q = (float)acc[k];
            *reinterpret_cast<float4 *>(G + ((size_t)k * p + s) * R + t) = make_float4(f0 * q, f1 * q, f2 * q, f3 * q);
        }
    }
}

// S of the image rows [row_begin, row_end), written at row - srow0. A workgroup: 256 consecutive elements (plane, b, k) of BSEP_RB
// consecutive image rows; E = planes x nc x R elements per row, ncR = nc x R. The band rows of the block (noskip: every band row)
// are walked in tiles of BSEP_ATILE, their Er15 per row of the block in LDS (a broadcast read); a row that a band row does not
// reach has Er15 = 0 there, an exact zero added.
__global__ __launch_bounds__(256) void k_band_sep_rows(const float *__restrict__ G, unsigned E, unsigned ncR, int nr, int row_begin, int row_end,
                                                       int srow0, const int *__restrict__ grow, const float *__restrict__ btab, int rad,
                                                       const unsigned *__restrict__ rowband, int noskip, float *__restrict__ S)
{
    __shared__ __attribute__((aligned(16))) float er_l[BSEP_ATILE][BSEP_RB];
    const int r0 = row_begin + blockIdx.y * BSEP_RB, nrb = min(BSEP_RB, row_end - r0);
    int alo, ahi;
    band_rows_hull(rowband, r0, nrb, &alo, &ahi);
    if (noskip) {
        alo = 0;
        ahi = nr - 1;
    }
    const unsigned e = blockIdx.x * 256 + threadIdx.x;
    const bool live = e < E;
    const unsigned plane = live ? e / ncR : 0u, rem = live ? e - plane * ncR : 0u;
    const float *g = G + (size_t)plane * nr * ncR + rem;
    float acc[BSEP_RB];
#pragma unroll
    for (int j = 0; j < BSEP_RB; ++j) acc[j] = 0.f;
    for (int a0 = alo; a0 <= ahi; a0 += BSEP_ATILE) {
        const int na = min(BSEP_ATILE, ahi - a0 + 1);
        __syncthreads();
        for (int i = threadIdx.x; i < na * BSEP_RB; i += 256) {
            const int dr = min(abs(r0 + i % BSEP_RB - grow[a0 + i / BSEP_RB]), rad);
            er_l[i / BSEP_RB][i % BSEP_RB] = btab[256 + rad + 1 + dr]; // (Er15[rad] = 0)
        }
        __syncthreads();
        if (live)
            for (int i = 0; i < na; ++i) {
                const float gv = g[(size_t)(a0 + i) * ncR];
                const float4 e0 = *reinterpret_cast<const float4 *>(&er_l[i][0]), e1 = *reinterpret_cast<const float4 *>(&er_l[i][4]);
                const float er[BSEP_RB] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
                for (int j = 0; j < BSEP_RB; ++j) acc[j] = fmaf(er[j], gv, acc[j]);
            }
    }
    if (live)
#pragma unroll
        for (int j = 0; j < BSEP_RB; ++j)
            if (j < nrb) S[(size_t)(r0 + j - srow0) * E + e] = acc[j];
}

// F transposed in LDS: [256][R + 1] (the odd pitch keeps lanes with different values off one bank) | Ec[rad + 1]
__host__ __device__ inline unsigned band_sep_lds_bytes(int R, int rad) { return 4u * (256u * (unsigned)(R + 1) + (unsigned)(rad + 1)); }

// 8 waves = 8 consecutive image rows x one tile of 64 columns, one lane per pixel, as k_band_vec. Every wave walks the sample
// columns within dc0 = dcmax[0] of the tile, ascending; per column one gather of Ec (exactly 0 from |dc| = rad on) and KB FMAs
// whose other operand is S[row][plane][b][k0 .. k0 + KB): wave-uniform, scalar loads. The KB accumulators of a (plane, block of
// terms) are folded with f_k(v_px) in f64. noskip: a wave without an image row walks too (with the last row's S) and writes nothing.
template <int NC, int KB>
__global__ __launch_bounds__(BAND_NW * 64) void k_band_sep_cols(const uint8_t *__restrict__ img, int width, int row_begin, int row_end, int srow0,
                                                                const int *__restrict__ gcol, int nc, const float *__restrict__ btab, int rad,
                                                                int dc0, const float *__restrict__ S, int R, const float *__restrict__ ftab,
                                                                const uint8_t *__restrict__ mask, BandFilter flt, int64_t fpix0, int noskip)
{
    constexpr int NW = BAND_NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char bsdyn[];
    float *ft = reinterpret_cast<float *>(bsdyn);  // [256][R + 1]
    float *elut = ft + 256 * (R + 1);              // [rad + 1]: Ec(d), 0 at d = rad
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int trow0 = row_begin + blockIdx.y * NW, ntw = min(NW, row_end - trow0);
    const int tc0 = blockIdx.x * 64, tc1 = min(width, tc0 + 64) - 1;
    for (int i = tid; i < 256 * R; i += NW * 64) ft[(i & 255) * (R + 1) + (i >> 8)] = ftab[i];
    for (int i = tid; i <= rad; i += NW * 64) elut[i] = btab[256 + i];
    // the tile's range of sample columns: within dc0 of it
    int Clo = 0, W = 0;
    if (dc0 >= 0) band_cols_range(gcol, nc, tc0 - dc0, tc1 + dc0, &Clo, &W);
    __syncthreads();
    if (wave >= ntw && !noskip) return;
    const int trow = min(trow0 + wave, row_end - 1), tcol = min(tc0 + lane, width - 1);
    const int pv = (int)img[(size_t)trow * width + tcol];
    const float *fpx = ft + pv * (R + 1);
    const size_t ncR = (size_t)nc * R;
    double tot[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        tot[k] = 0.0;
        const float *Srow = S + ((size_t)(trow - srow0) * NC + k) * ncR + (size_t)Clo * R;
        for (int k0 = 0; k0 < R; k0 += KB) {
            float U[KB];
#pragma unroll
            for (int t = 0; t < KB; ++t) U[t] = 0.f;
            for (int bb = 0; bb < W; ++bb) {
                const float ecv = elut[min(abs(tcol - gcol[Clo + bb]), rad)];
                const float *sp = Srow + (size_t)bb * R + k0;
#pragma unroll
                for (int t = 0; t < KB; ++t) U[t] = fmaf(ecv, sp[t], U[t]);
            }
#pragma unroll
            for (int t = 0; t < KB; ++t) tot[k] = fma((double)fpx[k0 + t], (double)U[t], tot[k]);
        }
    }

    // the filter, one lane per pixel (the sample pixels are filter_sample_rows' from Phi_A)
    if (wave >= ntw || tc0 + lane >= width) return;
    const int64_t px = (int64_t)trow * width + tcol;
    if (mask[px]) return;
    float sdot[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) sdot[k] = (float)(tot[k] * BAND_UNSCALE);
    band_filter_store<NC>(flt, fpix0, px, pv, sdot);
}

template <int NC, int KB>
static int band_sep_cols_launch(glf_ctx *ctx, const BandTables &bt, const uint8_t *d_img, int row0, int nrows, int srow0, const float *S, int R,
                                const float *ftab, unsigned lds, const uint8_t *d_mask, const BandFilter &flt, int64_t pix0)
{
    auto kern = k_band_sep_cols<NC, KB>;
    if (lds > 48u * 1024u) GLF_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)bt.ntiles_px, (unsigned)ceil_div(nrows, BAND_NW));
    hipLaunchKernelGGL(kern, grid, dim3(BAND_NW * 64), lds, ctx->stream, d_img, bt.width, row0, row0 + nrows, srow0, bt.gcol(), bt.nc, bt.tab(), bt.rad,
                       bt.dc0(), S, R, ftab, d_mask, flt, pix0, ctx->tune.band_noskip ? 1 : 0);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// The fused filter of the image rows [pix0 / width, pix1 / width) in separable rank-R form: G, then per chunk of image rows the row
// pass and the column pass. GLF_ERR_UNSUPPORTED: the photometric table has no expansion of at most RANK_MAX_R terms (R = 0: sharp
// kernels), or more planes than instantiated -- k_band_vec runs then.
static int launch_nystroem_band_sep(glf_ctx *ctx, const BandTables &bt, const uint8_t *d_img, int width, int64_t pix0, int64_t pix1,
                                    const float4 *d_samples, const uint8_t *d_mask, unsigned p, KernelCoef coef, const float *d_psi, unsigned ld,
                                    const BandFilter &flt, float *kernel_ms, uint64_t *entries_evaluated, double *mfma_flops, RowpassStats *stats)
{
    const int row0 = (int)(pix0 / width), row1 = (int)(pix1 / width), nrows = row1 - row0;
    const int ncol = 1 + flt.sig.nsig;
    if (ncol < 1 || ncol > BANDV_MAXNC || bt.width != width || p != (unsigned)bt.nr * (unsigned)bt.nc) return GLF_ERR_UNSUPPORTED;
    int R = 0;
    const float *ftab = nullptr;
    const _Float16 *Ff = nullptr;
    GLF_TRY(rank_tables(ctx, coef, &R, &ftab, &Ff));
    if (R <= 0) return GLF_ERR_UNSUPPORTED;
    const unsigned lds = band_sep_lds_bytes(R, bt.rad);
    if (lds > BANDV_LDS_MAX) return GLF_ERR_UNSUPPORTED; // (R = 64: the F table alone is 66 KB)
    // S in chunks of whole workgroups' rows: everything at once where BSEP_S_BYTES and the pool allow, else halved
    const size_t row_bytes = sizeof(float) * (size_t)bt.nc * R * ncol;
    int chunk = (int)std::min<size_t>((size_t)round_up(nrows, BAND_NW), std::max<size_t>(BAND_NW, BSEP_S_BYTES / row_bytes / BAND_NW * BAND_NW));
    DevBuf<uint8_t> svals;
    DevBuf<float> G, S;
    GLF_TRY(G.alloc(ctx, (size_t)ncol * p * R));
    while (S.alloc(ctx, (size_t)chunk * bt.nc * R * ncol) != GLF_OK) {
        if (chunk <= BAND_NW) return GLF_ERR_NOMEM;
        chunk = (int)round_up(chunk / 2, BAND_NW);
    }
    GLF_TRY(band_svals(ctx, d_samples, p, svals));
    hipStream_t st = ctx->stream;
    hipEvent_t e0 = ctx->ev[6], e1 = ctx->ev[7];
    const bool noskip = ctx->tune.band_noskip;
    GLF_TRY(band_dispatch_planes(ncol, [&](auto nc_) -> int {
        constexpr int NC = decltype(nc_)::value;
        hipLaunchKernelGGL(k_band_sep_g<NC>, dim3((p + 255) / 256), dim3(256), 0, st, d_psi, p, ld, flt.w, flt.sig.w, svals.p, ftab, R, G.p);
        GLF_LAUNCH_CHECK(ctx);
        const unsigned ncR = (unsigned)bt.nc * (unsigned)R, E = ncR * NC;
        GLF_HIP(ctx, hipEventRecord(e0, st));
        for (int c0 = 0; c0 < nrows; c0 += chunk) {
            const int r0 = row0 + c0, n = std::min(chunk, nrows - c0);
            hipLaunchKernelGGL(k_band_sep_rows, dim3((E + 255) / 256, (unsigned)ceil_div(n, BSEP_RB)), dim3(256), 0, st, G.p, E, ncR, bt.nr, r0, r0 + n, r0,
                               bt.grow(), bt.tab(), bt.rad, bt.rowband_px(), noskip ? 1 : 0, S.p);
            GLF_LAUNCH_CHECK(ctx);
            if (R % 32 == 0) GLF_TRY((band_sep_cols_launch<NC, 32>(ctx, bt, d_img, r0, n, r0, S.p, R, ftab, lds, d_mask, flt, pix0)));
            else GLF_TRY((band_sep_cols_launch<NC, 16>(ctx, bt, d_img, r0, n, r0, S.p, R, ftab, lds, d_mask, flt, pix0)));
        }
        GLF_HIP(ctx, hipEventRecord(e1, st));
        return GLF_OK;
    }));
    GLF_HIP(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    GLF_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    if (kernel_ms) *kernel_ms = ms;
    if (entries_evaluated) {
        // lane-entries covered by the windows, from the plan: 64 x sum over the walking waves of (columns walked x band rows feeding them)
        uint64_t cols = 0, rows = 0;
        for (int t = 0; t < bt.ntiles_px; ++t) cols += (uint64_t)bt.cols_near_tile(t);
        if (noskip) rows = (uint64_t)ceil_div(nrows, BAND_NW) * BAND_NW * (uint64_t)bt.nr; // every wave, every band row
        else
            for (int r = row0; r < row1; ++r) {
                int alo, ahi;
                band_rows_hull(bt.h_rowband_px.data(), r, 1, &alo, &ahi);
                rows += (uint64_t)std::max(0, ahi - alo + 1);
            }
        *entries_evaluated = 64ull * cols * rows;
    }
    if (mfma_flops) *mfma_flops = 0.0;
    band_stats(stats, bt, row0, row1, 1, ms, (unsigned)ncol, R);
    return GLF_OK;
}
