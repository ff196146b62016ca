// Band form, fused filter in separable rank-R form (included from nystroem_grid.inc after nystroem_band_vec.inc, inside namespace glf).
//
// k_band_vec evaluates s[px] = sum_{a,b} Er(r - R_a) Ec(c - C_b) P(|v_px - v_ab|) q_ab pair by pair: one LDS gather of P and
// about five vector instructions per (pixel, sample). With the expansion P(|v - w|) = sum_{k < R} f_k(v) f_k(w) of the rank form
// (rank_tables, nystroem_rank.inc: f64 factor, R = 32 at h_val = 30, max error 1.5e-11, sum_k |f_k(v) f_k(w)| <= 1) every factor of a
// term depends on the pixel's row, its column or its value alone, and the sum factors:
//   G[a][b][k] = f_k(v_ab) q_ab                         k_band_sep_g     p R values per plane
//   S[r][b][k] = sum_a Er15(|r - R_a|) G[a][b][k]       k_band_sep_rows  one fmaf chain per element, a ascending
//   U_k[px]    = sum_b S[r][b][k] Ec(|c - C_b|)         k_band_sep_cols_mfma  a banded GEMM on the matrix pipe (split f16, f32 accumulate)
//   s[px]      = sum_k f_k(v_px) U_k[px]                                 folded in f64, then band_filter_store
// The column pass is M = term k, N = pixel, K = sample column b: S arrives as the MFMA's A operand through coalesced vector loads,
// scaled by one power of two per plane (k_band_sep_scales, from the block maxima of |q| that k_band_sep_g leaves) and split into
// f16 (hi, lo) in registers; 2^12 Ec is the B operand, formed once per workgroup in LDS. No gather of P, no support test, no select:
// the support is the square |dr|, |dc| < rad (Er15 and Ec are exact zeros from rad on) instead of k_band_vec's circle -- the
// corners add terms below 2^-40 of the largest one.
// Layouts: G [plane][a][b][k], S [row][plane][b][k] (k fastest: the 32 terms of a term tile at one (row, b) are 128 contiguous
// bytes, one half-wave's load; a thread of the row pass owns one (plane, b, k) and walks a, so its loads and stores are contiguous
// over the wave).

constexpr int BSEP_RB = 8;                 // image rows a thread of the row pass holds (G is read once per block of rows)
constexpr int BSEP_ATILE = 128;            // band rows whose Er15 sit in LDS at a time (BAND_MAXROWS covers a block of rows at once)
constexpr size_t BSEP_S_BYTES = 256u << 20; // S of one chunk of image rows: the headline's 153 MB in one piece
static_assert(BSEP_RB == BAND_NW, "a block of the row pass is the rows of one workgroup of the column pass");
static_assert(BSEP_ATILE >= BAND_MAXROWS, "without BAND_NOSKIP one tile holds the band of a block of rows");

// q_k[s] = (float)(Psi[s] . w_k) as k_band_q has it (band_q_row), then G[k][s][t] = ftab[t][v_s] q_k[s]. One thread per sample.
// qpart [blocks][NC]: max |q_k| over the block's samples.
template <int NC>
__global__ __launch_bounds__(256) void k_band_sep_g(const float *__restrict__ psi, unsigned p, unsigned ld, const float *__restrict__ w,
                                                    const float *__restrict__ sig_w, const uint8_t *__restrict__ svals,
                                                    const float *__restrict__ ftab, int R, float *__restrict__ G, float *__restrict__ qpart)
{
    __shared__ float qm[4][NC];
    const unsigned s = blockIdx.x * 256 + threadIdx.x;
    const bool live = s < p;
    double acc[NC];
    if (live) band_q_row<NC>(psi + (size_t)s * ld, ld, w, sig_w, acc);
    // the block's max |q| per plane (q as it enters G), for the column pass' operand scale: k_band_sep_scales
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        float m = live ? fabsf((float)acc[k]) : 0.f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if ((threadIdx.x & 63) == 0) qm[threadIdx.x >> 6][k] = m;
    }
    __syncthreads();
    if (threadIdx.x < NC) qpart[(size_t)blockIdx.x * NC + threadIdx.x] = fmaxf(fmaxf(qm[0][threadIdx.x], qm[1][threadIdx.x]), fmaxf(qm[2][threadIdx.x], qm[3][threadIdx.x]));
    if (!live) return;
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

// The operand scale of S, one power of two per plane: |S| <= max |q| er15_rowsum (|f_k| <= 1, BandTables::er15_rowsum), so with
// 2^e max |q| er15_rowsum in [2^13, 2^14) the f16 (hi, lo) halves of 2^e S neither overflow nor lose their low bits. One workgroup:
// the block maxima of |q| that k_band_sep_g left, then scl[k] = 2^e and scl[BANDV_MAXNC + k] = 2^(-e - BSEP_EC_LOG2) (a plane
// whose q is all zero: e = 0), as k_band_absmax_scales does for the sweeps' operands.
constexpr int BSEP_EC_LOG2 = 12; // the Ec operand is split as 2^12 Ec: its f16 halves reach down to 2^-36 Ec(0)
__global__ __launch_bounds__(256) void k_band_sep_scales(const float *__restrict__ qpart, int nblk, int ncol, float er15_rowsum, float *__restrict__ scl)
{
    __shared__ float sh[256];
    for (int k = 0; k < ncol; ++k) {
        float m = 0.f;
        for (int i = threadIdx.x; i < nblk; i += 256) m = fmaxf(m, qpart[(size_t)i * ncol + k]);
        __syncthreads();
        sh[threadIdx.x] = m;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] = fmaxf(sh[threadIdx.x], sh[threadIdx.x + o]);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float mx = sh[0] * er15_rowsum;
            int e = 0;
            if (mx > 0.f && isfinite(mx)) {
                int ex;
                (void)frexpf(mx, &ex);
                e = 14 - ex;
            }
            e = max(-90, min(90, e));
            scl[k] = ldexpf(1.0f, e);
            scl[BANDV_MAXNC + k] = ldexpf(1.0f, -e - BSEP_EC_LOG2);
        }
    }
}

#ifndef BSEP_PT_X
#define BSEP_PT_X 4
#endif
constexpr int BSEP_PT = BSEP_PT_X; // pixel tiles of 32 per wave of the column pass: one fragment of S feeds all of them
constexpr int BSEP_KCH = 4;        // k-steps whose Ec fragments sit in LDS at a time (the headline's tiles have 2 or 3)
static_assert(BSEP_PT % 2 == 0 && BSEP_PT >= 2 && BSEP_PT <= 8, "a lane ends with BSEP_PT / 2 pixels");

// F transposed in LDS: [256][R + 1] (the odd pitch keeps lanes with different values off one bank) | Ec[rad + 1]
__host__ __device__ inline unsigned band_sep_lds_bytes(int R, int rad) { return 4u * (256u * (unsigned)(R + 1) + (unsigned)(rad + 1)); }
// ... | (16-byte aligned) the B fragments of BSEP_KCH k-steps: [k-step][pixel tile][hi | lo][lane][8] f16
__host__ __device__ inline unsigned band_sep_frag_offset(int R, int rad) { return (band_sep_lds_bytes(R, rad) + 15u) & ~15u; }
__host__ __device__ inline unsigned band_sep_mfma_lds_bytes(int R, int rad) { return band_sep_frag_offset(R, rad) + (unsigned)(BSEP_KCH * BSEP_PT) * 2048u; }

// The column pass as a banded GEMM on the matrix pipe: U[k][px] = sum_b S[r][b][k] Ec(|c_px - C_b|) with M = term k, N = pixel,
// K = sample column b, split-f16 (hi hi + hi lo + lo hi, f32 accumulate) on v_mfma_f32_32x32x16_f16.
// 8 waves = 8 consecutive image rows x one tile of 32 PT columns. The tile's sample columns (band_sep_tile_cols: within dc0 of it)
// go in k-steps of 16, ascending.
// B = 2^12 Ec is the same for the 8 rows, every plane and every term tile: its (hi, lo) fragments are formed once per workgroup
// into LDS (lane l of pixel tile t: pixel 32 t + (l & 31), entries 8 (l >> 5) + j of the k-step; an entry past the range, or rad or
// more away, is an exact zero in both halves). A tile with more than BSEP_KCH k-steps re-forms them per (plane, term tile).
// A = scl[plane] S[row][plane][b][k]: lane l holds term k0 + (l & 31) of columns b0 + 8 (l >> 5) + j, eight coalesced loads, scaled
// and split in registers; a term from R on (R = 16, 48: the last term tile is half full) is a zero that is never loaded, a column
// past the range is loaded from a clamped index and meets a zero of B.
// A (k-step, pixel tile) whose block of Ec is zero throughout (band_sep_block_dead) is passed over unless noskip: it adds exact
// zeros. The accumulator has the pixel on the lane and 16 of the tile's 32 terms in its registers, so the fold sum_k f_k(v_px) U_k
// is per-lane f64 FMAs against F in LDS -- registers ascending, term tiles ascending -- and one exchange between the half-waves,
// half 0 + half 1; lane l then owns pixel l of each 64 of the tile. Every wave stays to the end (the barriers); one without an
// image row loads nothing and stores nothing unless noskip, where it walks with the last row's S.
template <int NC, int PT>
__global__ __launch_bounds__(BAND_NW * 64) void k_band_sep_cols_mfma(const uint8_t *__restrict__ img, int width, int row_begin, int row_end, int srow0,
                                                                     const int *__restrict__ gcol, int nc, const float *__restrict__ btab, int rad,
                                                                     int dc0, const float *__restrict__ S, int R, const float *__restrict__ ftab,
                                                                     const float *__restrict__ scl, const uint8_t *__restrict__ mask, BandFilter flt,
                                                                     int64_t fpix0, int noskip)
{
    constexpr int NW = BAND_NW, NI = PT / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char bsdyn[];
    float *ft = reinterpret_cast<float *>(bsdyn);  // [256][R + 1]
    float *elut = ft + 256 * (R + 1);              // [rad + 1]: Ec(d), 0 at d = rad
    f16x8 *bfrag = reinterpret_cast<f16x8 *>(bsdyn + band_sep_frag_offset(R, rad)); // [BSEP_KCH][PT][2][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), half = lane >> 5, l31 = lane & 31;
    const int trow0 = row_begin + blockIdx.y * NW, ntw = min(NW, row_end - trow0);
    const int tc0 = blockIdx.x * (32 * PT);
    for (int i = tid; i < 256 * R; i += NW * 64) ft[(i & 255) * (R + 1) + (i >> 8)] = ftab[i];
    for (int i = tid; i <= rad; i += NW * 64) elut[i] = btab[256 + i];
    int Clo, W;
    band_sep_tile_cols(gcol, nc, width, tc0, 32 * PT, dc0, &Clo, &W);
    const int nks = band_sep_ksteps(W);
    const bool walk = wave < ntw || noskip;
    const int trow = min(trow0 + wave, row_end - 1);
    int pv[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) pv[t] = (int)img[(size_t)trow * width + min(tc0 + 32 * t + l31, width - 1)];
    __syncthreads();
    // the (hi, lo) fragments of 2^12 Ec of the k-steps [ks0, ks0 + BSEP_KCH)
    auto form = [&](int ks0) {
        for (int i = tid; i < BSEP_KCH * PT * 64; i += NW * 64) {
            const int ln = i & 63, t = (i >> 6) % PT, ks = ks0 + (i >> 6) / PT;
            if (ks >= nks) break;
            const int cpx = tc0 + 32 * t + (ln & 31);
            f16x8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = BSEP_KSTEP * ks + 8 * (ln >> 5) + j;
                const float ec = elut[min(abs(cpx - gcol[band_sep_col(Clo, e, nc)]), rad)];
                const float v = e < W ? ec * (float)(1 << BSEP_EC_LOG2) : 0.f;
                hi[j] = (_Float16)v;
                lo[j] = (_Float16)(v - (float)hi[j]);
            }
            bfrag[((i >> 6) * 2 + 0) * 64 + ln] = hi;
            bfrag[((i >> 6) * 2 + 1) * 64 + ln] = lo;
        }
    };
    const bool once = nks <= BSEP_KCH;
    if (once) {
        form(0);
        __syncthreads();
    }
    const size_t ncR = (size_t)nc * R;
    float sdot[NI][NC];
#pragma unroll 1 // (one plane at a time: unrolled, the planes' loads are hoisted over each other and the registers grow by 12 per plane)
    for (int k = 0; k < NC; ++k) {
        const float sc = scl[k];
        const float *Srow = S + ((size_t)(trow - srow0) * NC + k) * ncR;
        double tot[PT];
#pragma unroll
        for (int t = 0; t < PT; ++t) tot[t] = 0.0;
        for (int k0 = 0; k0 < R; k0 += 32) {
            f32x16 acc[PT];
#pragma unroll
            for (int t = 0; t < PT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
            const bool kin = k0 + l31 < R;
            const float *Sk = Srow + min(k0 + l31, R - 1);
            for (int ks0 = 0; ks0 < nks; ks0 += BSEP_KCH) {
                if (!once) {
                    __syncthreads();
                    form(ks0);
                    __syncthreads();
                }
                if (!walk) continue;
                // (the next k-step's eight loads are in flight under this one's MFMAs)
                const int ks1 = min(ks0 + BSEP_KCH, nks);
                float sv[8], sn[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) sn[j] = Sk[(size_t)band_sep_col(Clo, BSEP_KSTEP * ks0 + 8 * half + j, nc) * R];
                for (int ks = ks0; ks < ks1; ++ks) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) sv[j] = sn[j];
                    if (ks + 1 < ks1)
#pragma unroll
                        for (int j = 0; j < 8; ++j) sn[j] = Sk[(size_t)band_sep_col(Clo, BSEP_KSTEP * (ks + 1) + 8 * half + j, nc) * R];
                    f16x8 ah, al;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float v = kin ? sv[j] * sc : 0.f;
                        ah[j] = (_Float16)v;
                        al[j] = (_Float16)(v - (float)ah[j]);
                    }
                    const f16x8 *bf = bfrag + (size_t)(ks - ks0) * PT * 128 + lane;
#pragma unroll
                    for (int t = 0; t < PT; ++t) {
                        if (!noskip && band_sep_block_dead(gcol, nc, Clo, W, ks, tc0 + 32 * t, tc0 + 32 * t + 31, rad)) continue; // (wave-uniform)
                        const f16x8 bh = bf[t * 128], bl = bf[t * 128 + 64];
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[t], 0, 0, 0);
                    }
                }
            }
            // register q of a lane: term k0 + (q & 3) + 8 (q >> 2) + 4 half of pixel l31 of each pixel tile
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (k0 + 8 * (q >> 2) >= R) continue; // (the empty half of a last term tile: R is a multiple of 16)
                const int kk = k0 + (q & 3) + 8 * (q >> 2) + 4 * half;
#pragma unroll
                for (int t = 0; t < PT; ++t) tot[t] = fma((double)ft[pv[t] * (R + 1) + kk], (double)acc[t][q], tot[t]);
            }
        }
        // half 0 + half 1: lane l ends with pixel tile 2 i + half, i.e. pixel tc0 + 64 i + l
        const double unscale = BAND_UNSCALE * (double)scl[BANDV_MAXNC + k];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const double s0 = tot[2 * i] + __shfl_xor(tot[2 * i], 32, 64), s1 = tot[2 * i + 1] + __shfl_xor(tot[2 * i + 1], 32, 64);
            const float r = (float)((half ? s1 : s0) * unscale);
#pragma unroll
            for (int kk = 0; kk < NC; ++kk) // (k is not a constant: the planes' loop is not unrolled)
                if (kk == k) sdot[i][kk] = r;
        }
    }

    // the filter, one lane per pixel (the sample pixels are filter_sample_rows' from Phi_A)
    if (wave >= ntw) return;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int col = tc0 + 64 * i + lane;
        if (col >= width) continue;
        const int64_t px = (int64_t)trow * width + col;
        if (mask[px]) continue;
        band_filter_store<NC>(flt, fpix0, px, (int)img[px], sdot[i]);
    }
}

template <int NC>
static int band_sep_cols_launch(glf_ctx *ctx, const BandTables &bt, const uint8_t *d_img, int row0, int nrows, int srow0, const float *S, int R,
                                const float *ftab, const float *scl, const uint8_t *d_mask, const BandFilter &flt, int64_t pix0)
{
    auto kern = k_band_sep_cols_mfma<NC, BSEP_PT>;
    const unsigned lds = band_sep_mfma_lds_bytes(R, bt.rad);
    if (lds > 48u * 1024u) GLF_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)ceil_div(bt.width, 32 * BSEP_PT), (unsigned)ceil_div(nrows, BAND_NW));
    hipLaunchKernelGGL(kern, grid, dim3(BAND_NW * 64), lds, ctx->stream, d_img, bt.width, row0, row0 + nrows, srow0, bt.gcol(), bt.nc, bt.tab(), bt.rad,
                       bt.dc0(), S, R, ftab, scl, d_mask, flt, pix0, ctx->tune.band_noskip ? 1 : 0);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// The fused filter of the image rows [pix0 / width, pix1 / width) in separable rank-R form: G, then per chunk of image rows the row
// pass and the column pass. GLF_ERR_UNSUPPORTED: the photometric table has no expansion of at most RANK_MAX_R terms (R = 0: sharp
// kernels), or more planes than instantiated -- k_band_vec runs then.
static int launch_nystroem_band_sep(glf_ctx *ctx, const NysRequest &rq, const BandTables &bt)
{
    const int row0 = (int)(rq.pix0 / rq.width), row1 = (int)(rq.pix1 / rq.width), nrows = row1 - row0;
    const BandFilter &flt = *rq.flt;
    const int ncol = 1 + flt.sig.nsig;
    if (ncol < 1 || ncol > BANDV_MAXNC || bt.width != rq.width || rq.p != (unsigned)bt.nr * (unsigned)bt.nc) return GLF_ERR_UNSUPPORTED;
    int R = 0;
    const float *ftab = nullptr;
    const _Float16 *Ff = nullptr;
    GLF_TRY(rank_tables(ctx, rq.coef, &R, &ftab, &Ff));
    if (R <= 0) return GLF_ERR_UNSUPPORTED;
    if (band_sep_lds_bytes(R, bt.rad) > BANDV_LDS_MAX) return GLF_ERR_UNSUPPORTED; // (R = 64: the F table alone is 66 KB)
    // S in chunks of whole workgroups' rows: everything at once where BSEP_S_BYTES and the pool allow, else halved
    const size_t row_bytes = sizeof(float) * (size_t)bt.nc * R * ncol;
    int chunk = (int)std::min<size_t>((size_t)round_up(nrows, BAND_NW), std::max<size_t>(BAND_NW, BSEP_S_BYTES / row_bytes / BAND_NW * BAND_NW));
    DevBuf<uint8_t> svals;
    DevBuf<float> G, S, qpart, scl;
    const unsigned gblocks = (rq.p + 255) / 256;
    GLF_TRY(qpart.alloc(ctx, (size_t)gblocks * ncol));
    GLF_TRY(scl.alloc(ctx, 2 * BANDV_MAXNC));
    GLF_TRY(G.alloc(ctx, (size_t)ncol * rq.p * R));
    while (S.alloc(ctx, (size_t)chunk * bt.nc * R * ncol) != GLF_OK) {
        if (chunk <= BAND_NW) return GLF_ERR_NOMEM;
        chunk = (int)round_up(chunk / 2, BAND_NW);
    }
    GLF_TRY(band_svals(ctx, rq.d_samples, rq.p, svals));
    hipStream_t st = ctx->stream;
    hipEvent_t e0 = ctx->ev[6], e1 = ctx->ev[7];
    const bool noskip = ctx->tune.band_noskip;
    GLF_TRY(band_dispatch_planes(ncol, [&](auto nc_) -> int {
        constexpr int NC = decltype(nc_)::value;
        hipLaunchKernelGGL(k_band_sep_g<NC>, dim3(gblocks), dim3(256), 0, st, rq.d_psi, rq.p, rq.ld, flt.w, flt.sig.w, svals.p, ftab, R, G.p, qpart.p);
        GLF_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_band_sep_scales, dim3(1), dim3(256), 0, st, qpart.p, (int)gblocks, NC, (float)bt.er15_rowsum, scl.p);
        GLF_LAUNCH_CHECK(ctx);
        const unsigned ncR = (unsigned)bt.nc * (unsigned)R, E = ncR * NC;
        GLF_HIP(ctx, hipEventRecord(e0, st));
        for (int c0 = 0; c0 < nrows; c0 += chunk) {
            const int r0 = row0 + c0, n = std::min(chunk, nrows - c0);
            hipLaunchKernelGGL(k_band_sep_rows, dim3((E + 255) / 256, (unsigned)ceil_div(n, BSEP_RB)), dim3(256), 0, st, G.p, E, ncR, bt.nr, r0, r0 + n, r0,
                               bt.grow(), bt.tab(), bt.rad, bt.rowband_px(), noskip ? 1 : 0, S.p);
            GLF_LAUNCH_CHECK(ctx);
            GLF_TRY(band_sep_cols_launch<NC>(ctx, bt, rq.d_img, r0, n, r0, S.p, R, ftab, scl.p, rq.d_mask, flt, rq.pix0));
        }
        GLF_HIP(ctx, hipEventRecord(e1, st));
        return GLF_OK;
    }));
    GLF_HIP(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    GLF_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    if (rq.kernel_ms) *rq.kernel_ms = ms;
    if (rq.entries_evaluated) {
        // entries covered by the windows, from the plan: sum over the walking waves of (the 16 x 32 blocks of Ec the column pass
        // executes x band rows feeding them)
        uint64_t cols = 0, rows = 0;
        for (int tc0 = 0; tc0 < rq.width; tc0 += 32 * BSEP_PT)
            cols += band_sep_tile_entries(bt.geom.cols.data(), bt.nc, rq.width, tc0, 32 * BSEP_PT, bt.dc0(), bt.rad, noskip);
        if (noskip) rows = (uint64_t)ceil_div(nrows, BAND_NW) * BAND_NW * (uint64_t)bt.nr; // every wave, every band row
        else
            for (int r = row0; r < row1; ++r) {
                int alo, ahi;
                band_rows_hull(bt.h_rowband_px.data(), r, 1, &alo, &ahi);
                rows += (uint64_t)std::max(0, ahi - alo + 1);
            }
        *rq.entries_evaluated = cols * rows;
    }
    if (rq.mfma_flops) *rq.mfma_flops = 0.0;
    band_stats(rq.rowpass, bt, row0, row1, 1, ms, (unsigned)ncol, R);
    return GLF_OK;
}
