// Band form of the sample-side contractions (included from nystroem_grid.inc, inside namespace glf).
//
// Both sums of the path that run over the samples -- the Nystroem extension Phi[px] = sum_s K(px, s) Psi[s] (hpc/nystroem.c:118-162)
// and the operator sweep (K_A X)[s'] = sum_s K(s', s) X[s] of the eigen-solve (hpc/inverse_power_it.c:63-117 with the
// matrix of hpc/laplacian.c:20-71) -- carry the bilateral kernel K = E(dr) E(dc) P(|dv|) as 2^15 K split into an f16
// (hi, lo) pair. 2^15 E(dr) E(dc) <= 2^-25 leaves a zero pair: every sample farther than rad = sqrt(40.5 / s_loc) pixels
// from the target contributes exactly nothing in this arithmetic (211 px at cfg4: 961 of the 85 264 samples of the
// 292 x 292 grid, 1.1 %). The grid-factored forms (exact: T per grey level; rank: S per expansion term) were built to carry
// ALL samples and move 10 - 80 GB of intermediates per image for it. This form evaluates the entries inside the radius
// directly and nothing else:
//   per target row r and grid row a with |r - R_a| < rad (<= 31 rows at cfg4), per block of 16 sample columns that
//   reaches into the circle of a tile of 32 PB targets (2 - 4 blocks), one MFMA k-step: the 32 x 16 entries
//   y = (Er15(dr) Ec(dc)) P(|dv|) are generated on the vector pipe from three LDS tables (Ec hoisted out of the loop
//   over the grid rows: it depends on the target and the sample column only), split into f16 hi + lo, and contracted
//   with the (hi, lo) fragments of Psi -- staged once per workgroup by LDS-DMA -- on v_mfma_f32_32x32x16_f16.
// No intermediate reaches HBM; the operand is 21.8 MB per 64 columns.
// With the pixels as targets the unit is finer: a half-block of 8 sample columns in two consecutive band rows per k-step (the two
// lane-halves of the MFMA's k), which covers the circle with 0.835 of the k-steps (see k_band and band_plan.hpp).
//
// The colour and 16-bit bilateral kernels take the same form (k_band<.., PixGen::Rgb | U16>, behind the PIX_BAND tuning key): the
// spatial factor, the windows and the contraction are the grey ones, and P is generated from the raw values -- dist2 of the pixel
// policy and one v_exp_f32 per entry -- instead of gathered from the 256-level table.
//
// Tables (host-built, BandTables): win[dr][tile] = the blocks (sample targets) or half-blocks (pixel targets) of sample columns whose
// entries can be non-zero for a tile of targets at row distance dr (the circle narrows with dr); rowband[r] = the grid rows within the radius of target row r.

#ifndef BAND_SETPRIO
#define BAND_SETPRIO 1
#endif
#ifndef BAND_PCOPY
#define BAND_PCOPY 16 // copies of the photometric table in LDS (32 = one per bank of a 32-lane pass; 16 measured the same and leaves LDS for the row-major stages of the sweeps)
#endif
#ifndef BAND_NBUF
#define BAND_NBUF 2   // stage buffers (2: the next stage in flight; 3: two ahead)
#endif
constexpr unsigned BAND_PSTRIDE = 4u * BAND_PCOPY; // bytes between consecutive entries of the replicated table
#ifndef BAND_GROWS
#define BAND_GROWS 4
#endif
constexpr int BAND_G = BAND_GROWS;         // grid rows staged together (one barrier per stage)
// (BAND_MAXROWS, BAND_RMAX, BAND_EMPTY, BAND_PB, BAND_NW and the window helpers: band_plan.hpp, shared with the host-side plan)
__host__ __device__ constexpr inline int band_chunk_bytes(int mb) { return mb * 2048 + 256; }
constexpr int BAND_WB = 6; // sample targets: blocks of a grid row staged together (row-major stage order)
__host__ __device__ constexpr inline int band_stage_chunks(bool samples)
{
    return samples && 2 * BAND_WB > BAND_NBUF * BAND_G ? 2 * BAND_WB : BAND_NBUF * BAND_G;
}
// (plut: the replicated photometric table -- the grey instantiations; the colour and 16-bit ones generate the factor instead)
__host__ __device__ inline unsigned band_lds_bytes(int mb, int nw, int rad, int ksc, bool samples, bool plut = true)
{
    return (plut ? 256u * BAND_PSTRIDE : 0u) + (unsigned)band_stage_chunks(samples) * (unsigned)band_chunk_bytes(mb) + 4u * (unsigned)(rad + 1) + 64u * (unsigned)ksc + 4u * BAND_MAXROWS * (unsigned)(1 + 2 * nw) + 16u;
}

// operand chunks: per (grid row a, block of 16 sample columns): the MFMA B fragments of X[(a, b)][c0 .. c0 + 32 MB) colscale,
// [n-tile j][hi | lo][lane = 32 (k / 8) + n][k % 8] f16 (1 KiB each), then 128 v of the 16 samples as u32 (the row
// stride of the replicated photometric table) and padding to 256 B. Sample columns past nc: zeros.
// RAW (the colour and 16-bit formats): svals is the u32 image of the sample values (the 16-bit value, or the packed colour
// R + 256 G + 65536 B) and the tail carries it as it is. NCH = 3 (float colour): svals is three such planes [3][nr][nc], the bit
// patterns of R, G and B, and the tail carries R at +0, G at +64 and B at +128.
template <bool RAW, int NCH = 1>
__global__ __launch_bounds__(256) void k_band_prep(const float *__restrict__ X, unsigned x_ld, const float *__restrict__ colscale,
                                                    const void *__restrict__ svals_, int nr, int nc, int ksc, int mb,
                                                    unsigned char *__restrict__ chunks)
{
    const std::conditional_t<RAW, unsigned, uint8_t> *__restrict__ svals = static_cast<const std::conditional_t<RAW, unsigned, uint8_t> *>(svals_);
    // one thread per 16-byte fragment piece pair (hi, lo): (grid row a, block, n-tile jb, half h, column rr) -> the 8 samples
    // 16 blk + 8 h + j of column 32 jb + rr: 32 lanes read 128 contiguous bytes of a sample's row, and write 512 contiguous bytes
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)nr * ksc * mb * 64;
    if (e >= total) return;
    const unsigned rr = (unsigned)(e & 31), h = (unsigned)((e >> 5) & 1);
    const size_t q = e >> 6;
    const unsigned jb = (unsigned)(q % (unsigned)mb);
    const size_t ab = q / (unsigned)mb;
    const int blk = (int)(ab % (unsigned)ksc), a = (int)(ab / (unsigned)ksc);
    const unsigned c = 32u * jb + rr;
    const float sc = colscale[c];
    f16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int bcol = 16 * blk + 8 * (int)h + j;
        const float v = bcol < nc ? X[((size_t)a * nc + bcol) * x_ld + c] * sc : 0.f;
        hi[j] = (_Float16)v;
        lo[j] = (_Float16)(v - (float)hi[j]);
    }
    unsigned char *ch = chunks + ((size_t)a * ksc + blk) * band_chunk_bytes(mb);
    f16x8 *f = reinterpret_cast<f16x8 *>(ch);
    f[(size_t)(jb * 2 + 0) * 64 + h * 32 + rr] = hi;
    f[(size_t)(jb * 2 + 1) * 64 + h * 32 + rr] = lo;
    if (jb == 0 && rr < 8) {
        const int k = 8 * (int)h + (int)rr, bcol = 16 * blk + k;
        if constexpr (NCH == 1)
            reinterpret_cast<unsigned *>(ch + mb * 2048)[k] = bcol < nc ? (RAW ? 1u : BAND_PSTRIDE) * (unsigned)svals[(size_t)a * nc + bcol] : 0u;
        else {
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                reinterpret_cast<unsigned *>(ch + mb * 2048)[16 * c + k] = bcol < nc ? (unsigned)svals[((size_t)c * nr + a) * nc + bcol] : 0u;
        }
    }
}

// second level of the column maxima (k_col_absmax_part's block maxima) and the scales in one launch:
// colscale[j] = 2^e with |X[:, j]| 2^e in [2^13, 2^14); inv[j] = 2^(-e - 15) takes it and the 2^15 of the kernel out again
// (red2_grid(ld) workgroups of RED2_THREADS threads: wg_reduce_partials)
__global__ __launch_bounds__(RED2_THREADS) void k_band_absmax_scales(const float *__restrict__ part, int nblk, unsigned ld,
                                                                      float *__restrict__ colscale, float *__restrict__ inv)
{
    __shared__ float sh[RED2_THREADS];
    float mx[1];
    wg_reduce_partials<float, 1, true>(part, nblk, ld, mx, sh);
    if (threadIdx.x < RED2_COLS) {
        const unsigned col = blockIdx.x * RED2_COLS + threadIdx.x;
        const OperandScales s = operand_scales(mx[0], 1); // (scale_rule.hpp)
        colscale[col] = s.colscale;
        inv[col] = s.inv;
    }
}
// the column maxima of X, then colscale / inv (two launches; one where the writer of X carried the block maxima along)
static void band_scales(hipStream_t st, const float *X, unsigned p, unsigned ld, float *scratch, float *colscale, float *inv,
                        const ColMaxima *carried = nullptr)
{
    const float *part = scratch;
    int nblk = (int)ceil_div(p, CAM_ROWS);
    if (carried) {
        part = carried->part;
        nblk = carried->nblk;
    } else {
        hipLaunchKernelGGL(k_col_absmax_part, dim3(nblk), dim3(256), 0, st, X, p, ld, scratch);
    }
    hipLaunchKernelGGL(k_band_absmax_scales, dim3(red2_grid(ld)), dim3(RED2_THREADS), 0, st, part, nblk, ld, colscale, inv);
}

// The filter of one pixel px that is no sample, from sdot[k] = Phi[px] . w_k (k = 0: the guide, then the planes of joint filtering):
// hpc/display.c:64-78 as k_apply_filter has it, Phi never written. The one store of every form of the fused filter -- k_band's
// epilogue, k_band_vec, k_band_sep_cols_mfma; y: the guide's value at px.
template <int NC>
__device__ __forceinline__ void band_filter_store(const BandFilter &f, int64_t pix0, int64_t px, int y, const float (&sdot)[NC])
{
    const float cc = f.gain * sdot[0] - f.ysub * (float)y;
    if (f.zf) f.zf[px] = (float)y + cc;
    if (f.corr) f.corr[px - pix0] = cc;
    f.out[px] = filter_output(y, cc);
#pragma unroll
    for (int k = 1; k < NC; ++k) {
        const float v = f.sig.s[(size_t)(k - 1) * f.sig.N + px];
        f.sig.out[(size_t)(k - 1) * f.sig.N + px] = v + (f.gain * sdot[k] - f.ysub * v);
    }
}
// k_band_vec and k_band_sep_cols_mfma sum with the Er15 table, which carries k_band's 2^15 (k_band's inv[] takes it out); their f64
// totals lose it here
constexpr double BAND_UNSCALE = 1.0 / 32768.0;
static_assert(NYS_F16_KSCALE_LOG2 == 15.0f, "BAND_UNSCALE takes the scale of the Er15 table out again");

// the fused filter's columns: the guide and up to GLF_MAX_SIGNALS planes, one instantiation of its kernels per count
constexpr int BANDV_MAXNC = 1 + GLF_MAX_SIGNALS;
template <class F> static int band_dispatch_planes(int n, F &&f)
{
    static_assert(BANDV_MAXNC == 5, "one instantiation per column count");
    switch (n) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    default: return GLF_ERR_UNSUPPORTED;
    }
}

// MB: n-tiles of 32 columns; PB: tiles of 32 targets per wave; NW: waves per workgroup. The waves of a workgroup take the
// same tile of columns in NW consecutive target rows: they need the same blocks of the same grid rows (all but a row at the
// ends of the band), so every staged chunk serves every wave. (Waves side by side in one row shared a third of their
// chunks less and idled through the stages outside their own window: 2.4x slower.)
// SAMPLES = false: targets = the pixels of image rows [row_begin, row_begin + gridDim.y): out = Phi (+ column offset), epilogue
//   as k_nystroem_f16s (sample pixels skipped unless raster; c += Phi^T y per workgroup).
// SAMPLES = true: targets = the samples of grid rows [row_begin, ..): out = Y = alpha (D X - K_A X).
// fw set: the filter in the epilogue (band_filter_store) instead of Phi. NS > 0 (joint filtering): NS float planes through the
//   same filter, fsig.w [NS][LD] their weights
// G: the pixel format. Grey: the photometric factor is one LDS gather per entry from the 256-level table. Rgb, U16, F32: tval is the
//   image in the format (pixel targets) or the u32 image of the sample values (sample targets), the chunk tails carry the raw u32
//   values (F32: the float's bit pattern), and the factor is P = exp2(pix_nsval dist2) with Pix<G>::dist2 and one v_exp_f32 per entry (pix_nsval = -s_val); no
//   table in LDS. Er Ec stays a separate factor, so an entry outside the radius is still an exact zero pair. These
//   instantiations write Phi (or Y): no filter in the epilogue, no c.
//   RgbF32: three u32 per sample (the bit patterns of R, G, B): tval for the sample targets is three planes [3][nr][nc], and the tail
//   carries R at +0, G at +64, B at +128 -- a k-step reads its 8 samples' channels as three pairs of uint4. With the pixels as targets
//   the tail piece of a slot is assembled by lanes 0 - 11 of its one DMA instruction (four lanes per channel) in the same layout.
template <PixGen G> __device__ __forceinline__ typename Pix<G>::Val band_pix_value(unsigned v)
{
    if constexpr (G == PixGen::Rgb) return make_float3(ubyte_f32(v, 0), ubyte_f32(v, 1), ubyte_f32(v, 2));
    else if constexpr (G == PixGen::F32) return __uint_as_float(v); // (the float's bit pattern)
    else return (float)v;
}
// (float colour: the three bit patterns of a value)
__device__ __forceinline__ float3 band_pix_value3(unsigned r, unsigned g, unsigned b)
{
    return make_float3(__uint_as_float(r), __uint_as_float(g), __uint_as_float(b));
}
template <int MB, int PB, int NW, bool SAMPLES, int NS = 0, PixGen G = PixGen::Grey>
__global__ __launch_bounds__(NW * 64) void k_band(const uint8_t *__restrict__ tval, int width, int row_begin, const int *__restrict__ grow,
                                                   const int *__restrict__ gcol, int nr, int nc, int ksc, const float *__restrict__ btab,
                                                   const float *__restrict__ pexp, int rad, const unsigned *__restrict__ rowband, const unsigned *__restrict__ win,
                                                   int ntiles, const unsigned char *__restrict__ chunks, const float *__restrict__ inv,
                                                   float *__restrict__ out, int out_ld, const uint8_t *__restrict__ mask,
                                                   const uint32_t *__restrict__ idx, unsigned p, int raster, double *__restrict__ cpartial,
                                                   const float *__restrict__ X, int x_ld, const double *__restrict__ degree, float alpha,
                                                   unsigned long long *__restrict__ evaluated, int row_end, const float *__restrict__ fw,
                                                   float fgain, float fysub, uint8_t *__restrict__ fout, float *__restrict__ fzf,
                                                   float *__restrict__ fcorr, int64_t fpix0, BandSignals fsig, int noskip, float pix_nsval)
{
    static_assert(!SAMPLES || PB == 1, "sample targets: one tile of 32 per wave");
    static_assert(G == PixGen::Grey || NS == 0, "the colour and 16-bit instantiations have no filter epilogue");
    constexpr bool GREY = G == PixGen::Grey, TRI = G == PixGen::RgbF32; // (TRI: three u32 per sample value)
    constexpr unsigned PLUT_BYTES = GREY ? 256 * BAND_PSTRIDE : 0u;
    constexpr int LD = 32 * MB, CHB = band_chunk_bytes(MB), NPIECE = MB * 2 + 1; // (the last piece is the 256-byte tail)
    // Pixel targets: a unit of work is (pair of consecutive band rows, half-block of 8 sample columns): lanes 0 - 31 of the MFMA's
    // k hold the 8 columns in the pair's first row, lanes 32 - 63 the same columns in its second row. The pairs are aligned to the
    // workgroup's first band row, so every wave shares a stage; windows and positions `blk` are in half-blocks. The circle is covered
    // at 8 columns x 1 row instead of 16 x 1: 0.835 of the k-steps. A half outside its own window generates exact zeros.
    // Sample targets: (one band row, block of 16 columns) as before.
    constexpr int RP = SAMPLES ? 1 : BAND_PAIR;
    extern __shared__ __attribute__((aligned(16))) unsigned char bdyn[];
    float *plut = reinterpret_cast<float *>(bdyn); // [256][32]: the photometric table, one copy per bank (Grey only)
    unsigned char *stage = bdyn + PLUT_BYTES; // [BAND_NBUF][BAND_G][CHB]
    float *elut = reinterpret_cast<float *>(stage + band_stage_chunks(SAMPLES) * CHB); // [rad + 1]: Ec(d), 0 at d = rad
    int *gcs = reinterpret_cast<int *>(elut + (rad + 1));              // [16 ksc]: the sample columns (far away past nc)
    float *er_s = reinterpret_cast<float *>(gcs + 16 * ksc);           // [NW][BAND_MAXROWS]: 2^15 Er of the band rows, per wave
    unsigned *gwin = reinterpret_cast<unsigned *>(er_s + NW * BAND_MAXROWS); // [BAND_MAXROWS]: blocks any wave needs of a band row
    unsigned *wwin = gwin + BAND_MAXROWS;                              // [NW][BAND_MAXROWS]: blocks each wave needs
    int *misc = reinterpret_cast<int *>(wwin + NW * BAND_MAXROWS);     // first and last block of the workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), half = lane >> 5, l31 = lane & 31;
    const int trow0 = row_begin + blockIdx.y * NW; // target row of wave 0 (image row / grid row)
    const int tile = blockIdx.x, ntw = min(NW, row_end - trow0); // waves with a target row
    // band of the workgroup: the grid rows within the radius of any of its target rows
    int alo, ahi;
    band_rows_hull(rowband, trow0, ntw, &alo, &ahi);
    const int nb = min(BAND_MAXROWS, max(0, ahi - alo + 1));

    // the replicated photometric table arrives by LDS-DMA from its expanded image in the tables blob (256 BAND_PCOPY floats, after
    // the grid coordinates), 1 KiB per instruction: 21 load + store rounds per thread otherwise
    if constexpr (GREY) {
        constexpr int PIECES = 256 * BAND_PCOPY * 4 / 1024;
        const unsigned char *src = reinterpret_cast<const unsigned char *>(pexp);
        const unsigned dst0 = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_offset_of(plut));
        for (int q = wave; q < PIECES; q += NW) lds_dma_16B(src + (size_t)q * 1024 + lane * 16, dst0 + (unsigned)q * 1024u);
    }
    for (int i = tid; i <= rad; i += NW * 64) elut[i] = btab[256 + i];
    for (int i = tid; i < 16 * ksc; i += NW * 64) gcs[i] = i < nc ? gcol[i] : -(1 << 28);
    // per unit of RP band rows (entry RP u of the arrays): what each wave needs of it -- the hull of its rows' windows -- and what any does
    for (int i0 = RP * tid; i0 < nb; i0 += RP * NW * 64) {
        unsigned g = BAND_EMPTY;
        for (int w = 0; w < NW; ++w) {
            const int rw = w < ntw ? (SAMPLES ? grow[trow0 + w] : trow0 + w) : (1 << 28);
            unsigned u = BAND_EMPTY;
            for (int i = i0; i < min(i0 + RP, nb); ++i) {
                const int dr = abs(rw - grow[alo + i]);
                er_s[w * BAND_MAXROWS + i] = dr < rad ? btab[256 + rad + 1 + dr] : 0.f;
                u = band_win_hull(u, dr < rad ? win[(size_t)dr * ntiles + tile] : BAND_EMPTY);
            }
            wwin[w * BAND_MAXROWS + i0] = u;
            g = band_win_hull(g, u);
        }
        gwin[i0] = g;
    }
    if constexpr (GREY) lds_dma_drain(); // (this wave's pieces of the photometric table)
    __syncthreads();
    if (tid == 0) {
        int blo = 0xFFFF, bhi = -1;
        for (int i = 0; i < nb; i += RP) {
            const unsigned u = gwin[i];
            if (band_win_live(u)) {
                blo = min(blo, (int)(u & 0xFFFFu));
                bhi = max(bhi, (int)(u >> 16));
            }
        }
        misc[0] = blo;
        misc[1] = bhi;
    }
    __syncthreads();
    const int Blo = misc[0], Bhi = misc[1];

    // this wave's targets: column and 128 value per lane and tile
    const bool wvalid = wave < ntw;
    const int trow = min(trow0 + wave, row_end - 1);
    int tc[PB];
    unsigned pv128[PB];
    typename Pix<G>::Val pvv[PB]; // (Rgb, U16: the target's value as the policy compares it)
#pragma unroll
    for (int b = 0; b < PB; ++b) {
        if (SAMPLES) {
            const int bb = min(tile * 32 + l31, nc - 1);
            tc[b] = gcol[bb];
            if constexpr (GREY) pv128[b] = BAND_PSTRIDE * (unsigned)tval[(size_t)trow * nc + bb];
            else if constexpr (TRI) {
                const unsigned *tv = reinterpret_cast<const unsigned *>(tval) + (size_t)trow * nc + bb;
                const size_t plane = (size_t)nr * nc;
                pvv[b] = band_pix_value3(tv[0], tv[plane], tv[2 * plane]);
            } else pvv[b] = band_pix_value<G>(reinterpret_cast<const unsigned *>(tval)[(size_t)trow * nc + bb]);
        } else {
            const int cc = min((tile * PB + b) * 32 + l31, width - 1);
            tc[b] = cc;
            if constexpr (GREY) pv128[b] = BAND_PSTRIDE * (unsigned)tval[(size_t)trow * width + cc];
            else pvv[b] = Pix<G>::read(reinterpret_cast<const typename Pix<G>::In *>(tval), (int64_t)trow * width + cc);
        }
    }
    const unsigned pbase = lds_offset_of(plut) + 4u * (unsigned)(lane % BAND_PCOPY);
    f32x16 acc[PB][MB];
#pragma unroll
    for (int b = 0; b < PB; ++b)
#pragma unroll
        for (int j = 0; j < MB; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[b][j][q] = 0.f;

    // stages: ((half-)block, group of BAND_G units of RP band rows) in block-major order; a stage no wave needs anything of is passed
    // over (noskip: none is, and every wave executes every unit of the workgroup's range -- the skipped ones add exact zeros)
    auto stage_live = [&](int blk, int g0) -> bool {
        bool any = noskip != 0;
        for (int i = g0; i < min(g0 + RP * BAND_G, nb); i += RP) any = any || band_win_has(gwin[i], blk);
        return any;
    };
    auto advance = [&](int &blk, int &g0) { // to the next live stage (blk > Bhi: none)
        for (;;) {
            g0 += RP * BAND_G;
            if (g0 >= nb) {
                g0 = 0;
                ++blk;
            }
            if (blk > Bhi || stage_live(blk, g0)) return;
        }
    };
    // pixel targets: byte offsets of a lane's 16 bytes within a DMA instruction, from the chunk of the pair's first row: the piece's
    // half for lanes 0 - 31 and the same of the next band row (ksc chunks on) for lanes 32 - 63; of the tail, lanes 0 - 1 and 2 - 3
    const unsigned dma_off_row = 16u * (unsigned)l31, dma_off = dma_off_row + (half ? (unsigned)ksc * CHB : 0u);
    // (TRI: lanes 4 c .. 4 c + 3 the same of channel c, 64 c bytes on in the tail and in the slot)
    constexpr int TAIL_LANES = TRI ? 12 : 4;
    const unsigned dma_toff_row = 16u * (unsigned)(lane & 1) + (TRI ? 64u * (unsigned)(lane >> 2) : 0u),
                   dma_toff = dma_toff_row + ((lane >> 1) & 1 ? (unsigned)ksc * CHB : 0u);
    auto issue = [&](int blk, int g0, int buf) -> int { // returns the DMA instructions this wave issued
        int n = 0;
        for (int q = wave; q < BAND_G * NPIECE; q += NW) { // (wave-uniform)
            const int slot = q / NPIECE, k = q % NPIECE, i = g0 + RP * slot;
            if (i >= nb) break;
            if (!noskip && !band_win_has(gwin[i], blk)) continue;
            const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_offset_of(stage + (size_t)(buf * BAND_G + slot) * CHB + k * 1024));
            if constexpr (SAMPLES) {
                const unsigned char *src = chunks + ((size_t)(alo + i) * ksc + blk) * CHB + k * 1024 + lane * 16;
                if (k < NPIECE - 1 || lane < 16) lds_dma_16B(src, dst);
            } else {
                // the slot is assembled by the DMA itself (it writes dst + 16 lane from per-lane addresses): lanes 0 - 31 bring half
                // (blk & 1) of block blk >> 1 of band row i, lanes 32 - 63 the same half of row i + 1; of the tail, 32 bytes
                // of sample values each. A row past the end of the band: row i again (its Er is 0).
                // (wave-uniform base + per-lane 32-bit offsets fixed for the launch: one vector instruction per DMA)
                const unsigned char *ch = chunks + ((size_t)(alo + i) * ksc + (blk >> 1)) * CHB + k * 1024;
                const bool both = i + 1 < nb;
                if (k < NPIECE - 1) lds_dma_16B_base(ch + 512 * (blk & 1), both ? dma_off : dma_off_row, dst);
                else if (lane < TAIL_LANES) lds_dma_16B_base(ch + 32 * (blk & 1), both ? dma_toff : dma_toff_row, dst);
            }
            ++n;
        }
        return n;
    };
    // wait until at most n of this wave's DMA instructions are outstanding (they complete in order: everything issued before
    // the last n has landed)
    auto dma_wait = [&](int n) {
        switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break; // (more than 4 per stage: waits for more than it must)
        }
    };

    f32x2 ec[PB][4]; // Ec of this lane's target(s) at its 8 samples of the current block (pairs: the products below are packed)
    // one k-step: the 32 PB x 16 entries of (targets, the 16 samples of chunk `sl`) generated, split, contracted
    auto kstep = [&](const unsigned char *sl, float era, const f32x2 (&ec)[PB][4]) __attribute__((always_inline)) {
        const uint4 s0 = *reinterpret_cast<const uint4 *>(sl + MB * 2048 + 32 * half);
        const uint4 s1 = *reinterpret_cast<const uint4 *>(sl + MB * 2048 + 32 * half + 16);
        const unsigned sv128[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        // all the photometric gathers of the step first (their latency overlaps), then the products and the split.
        // (A software pipeline over the steps of a stage -- the next step's generation placed between this step's MFMAs with
        // sched_group_barrier -- needs 212 VGPRs: two waves per SIMD instead of four, 14.7 ms instead of 9.8; held to 128
        // registers it spills 236. Four waves per SIMD overlapping each other's phases is the better trade here. Placing one
        // tile's MFMAs between the vector instructions of the next tile's generation inside a step costs no registers and
        // measured 2 % slower; tiles of 32 or 128 columns per wave (PB = 1, 4): 11.6 / 11.1 ms against 9.2.)
        float pp[PB][8];
        if constexpr (TRI) {
            // the sample's three channels from the tail (G 64 bytes, B 128 bytes behind R): Pix<G>::dist2 in its own operation order,
            // fmaf(dB, dB, fmaf(dG, dG, dR dR)), taken channel by channel over the step's entries so that one channel's 8 values are live
            // at a time (all 24 at once cost the kernel a wave per SIMD), then one v_exp_f32 per entry
            const unsigned char *tl = sl + MB * 2048 + 32 * half;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float sr = __uint_as_float(sv128[e]);
#pragma unroll
                for (int b = 0; b < PB; ++b) {
                    const float d = pvv[b].x - sr;
                    pp[b][e] = d * d;
                }
            }
            {
                const uint4 g0 = *reinterpret_cast<const uint4 *>(tl + 64), g1 = *reinterpret_cast<const uint4 *>(tl + 80);
                const unsigned sg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = __uint_as_float(sg[e]);
#pragma unroll
                    for (int b = 0; b < PB; ++b) {
                        const float d = pvv[b].y - v;
                        pp[b][e] = fmaf(d, d, pp[b][e]);
                    }
                }
            }
            {
                const uint4 b0 = *reinterpret_cast<const uint4 *>(tl + 128), b1 = *reinterpret_cast<const uint4 *>(tl + 144);
                const unsigned sb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = __uint_as_float(sb[e]);
#pragma unroll
                    for (int b = 0; b < PB; ++b) {
                        const float d = pvv[b].z - v;
                        pp[b][e] = __builtin_amdgcn_exp2f(fmaf(d, d, pp[b][e]) * pix_nsval);
                    }
                }
            }
        } else if constexpr (GREY) {
#pragma unroll
            for (int b = 0; b < PB; ++b)
#pragma unroll
                for (int e = 0; e < 8; ++e) pp[b][e] = lds_f32(sad_u32(pv128[b], sv128[e], pbase));
        } else {
            // the policy's squared distance (exact integer terms, the sum rounded once) and one v_exp_f32 per entry; a sample's
            // value is unpacked once for the PB targets
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const typename Pix<G>::Val sv = band_pix_value<G>(sv128[e]);
#pragma unroll
                for (int b = 0; b < PB; ++b) pp[b][e] = __builtin_amdgcn_exp2f(Pix<G>::dist2(pvv[b], sv) * pix_nsval);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        f16x8 ah[PB], al[PB];
#if defined(BAND_EXP) && BAND_EXP == 2 // (profiling build: no generation -- the gathers stay, their values go unused)
#pragma unroll
        for (int b = 0; b < PB; ++b)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                ah[b][e] = (_Float16)pp[b][0];
                al[b][e] = (_Float16)era;
            }
#else
#pragma unroll
        for (int b = 0; b < PB; ++b) {
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                f32x2 y; // (scalar products on purpose: v_pk_mul_f32 measured 8 % slower beside the MFMAs, as v_pk_add_f32 in k_nystroem_f16s)
                y[0] = (era * ec[b][e >> 1][0]) * pp[b][e];
                y[1] = (era * ec[b][e >> 1][1]) * pp[b][e + 1];
                const f16x2 h2 = __builtin_convertvector(y, f16x2);
                f32x2 res;
                res[0] = y[0] - (float)h2[0];
                res[1] = y[1] - (float)h2[1];
                const f16x2 l2 = __builtin_convertvector(res, f16x2);
                ah[b][e] = h2[0];
                ah[b][e + 1] = h2[1];
                al[b][e] = l2[0];
                al[b][e + 1] = l2[1];
            }
        }
#endif
#if defined(BAND_EXP) && BAND_EXP == 1 // (profiling build: no MFMAs -- the entries are folded into one accumulator register)
#pragma unroll
        for (int b = 0; b < PB; ++b)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[b][0][e] += (float)ah[b][e] + (float)al[b][e];
        return;
#endif
        if (BAND_SETPRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < MB; ++j) {
            const f16x8 bh = *reinterpret_cast<const f16x8 *>(sl + (j * 2 + 0) * 1024 + lane * 16);
            const f16x8 bl = *reinterpret_cast<const f16x8 *>(sl + (j * 2 + 1) * 1024 + lane * 16);
#pragma unroll
            for (int b = 0; b < PB; ++b) {
                acc[b][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[b], bh, acc[b][j], 0, 0, 0);
                acc[b][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[b], bl, acc[b][j], 0, 0, 0);
                acc[b][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[b], bh, acc[b][j], 0, 0, 0);
            }
        }
        if (BAND_SETPRIO) __builtin_amdgcn_s_setprio(0);
    };
    int cur_blk = -1;
    unsigned long long nsteps = 0;
    int blk = Blo, g0 = -BAND_G;
    bool row_major = false;
    if constexpr (SAMPLES) {
        // Sample targets, row-major stages: a stage is one band row with all its blocks (contiguous chunks: up to BAND_WB), every
        // wave takes a k-step of each -- 38 full stages per workgroup instead of ~50 part-filled ones in block-major order, where a
        // stage's few k-steps of one 32-target tile per wave left the DMA latency of the next stage exposed. Ec of all the window's
        // blocks stays in registers (the targets are fixed).
        row_major = nb > 0 && Bhi >= Blo && Bhi - Blo + 1 <= BAND_WB;
        if (row_major) {
            f32x2 ecs[BAND_WB][PB][4];
#pragma unroll
            for (int bq = 0; bq < BAND_WB; ++bq)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int cb = Blo + bq <= Bhi ? gcs[16 * (Blo + bq) + 8 * half + e] : -(1 << 28);
#pragma unroll
                    for (int b = 0; b < PB; ++b) ecs[bq][b][e >> 1][e & 1] = elut[min(abs(tc[b] - cb), rad)];
                }
            auto live = [&](int i) -> bool {
                const unsigned u = gwin[i];
                return (u & 0xFFFFu) <= (u >> 16);
            };
            auto next_row = [&](int i) -> int {
                do ++i;
                while (i < nb && !live(i));
                return i;
            };
            auto issue_row = [&](int i, int bf) {
                const unsigned u = gwin[i];
                const int lo = (int)(u & 0xFFFFu), bytes = ((int)(u >> 16) - lo + 1) * CHB; // (a multiple of 256)
                const unsigned char *src = chunks + ((size_t)(alo + i) * ksc + lo) * CHB;
                const unsigned dst0 = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_offset_of(stage + (size_t)bf * BAND_WB * CHB));
                for (int q = wave; q * 1024 < bytes; q += NW) // (wave-uniform)
                    if (lane * 16 < bytes - q * 1024)
                        lds_dma_16B(src + (size_t)q * 1024 + lane * 16, (unsigned)__builtin_amdgcn_readfirstlane((int)(dst0 + (unsigned)q * 1024u)));
            };
            int i = live(0) ? 0 : next_row(0), bf = 0;
            if (i < nb) issue_row(i, 0);
            lds_dma_drain();
            __syncthreads();
            while (i < nb) {
                const int inext = next_row(i);
                if (inext < nb) issue_row(inext, bf ^ 1);
                if (wvalid) {
                    const unsigned ug = gwin[i];
                    const unsigned uw = (unsigned)__builtin_amdgcn_readfirstlane((int)wwin[wave * BAND_MAXROWS + i]);
                    const int glo = (int)(ug & 0xFFFFu), wlo = (int)(uw & 0xFFFFu), whi = (int)(uw >> 16);
                    const float era = er_s[wave * BAND_MAXROWS + i];
                    const unsigned char *sb = stage + (size_t)bf * BAND_WB * CHB;
#pragma unroll
                    for (int bq = 0; bq < BAND_WB; ++bq) {
                        const int bk = Blo + bq;
                        if (bk >= wlo && bk <= whi) { // (wave-uniform)
                            kstep(sb + (size_t)(bk - glo) * CHB, era, ecs[bq]);
                            ++nsteps;
                        }
                    }
                }
                lds_dma_drain();
                __syncthreads();
                i = inext;
                bf ^= 1;
            }
            blk = Bhi + 1; // (the block-major loop below has nothing left to do)
        }
    }
    if (row_major) {
    } else if (nb > 0 && Bhi >= Blo) {
        --blk;
        g0 = nb; // (advance steps to (Blo, 0) first)
        advance(blk, g0);
    } else blk = Bhi + 1;
    // ring of BAND_NBUF stage buffers: stages s + 1 .. s + BAND_NBUF - 1 are in flight while stage s is contracted
    int qblk[BAND_NBUF], qg0[BAND_NBUF], buf = 0, last_issued = 0; // qblk[d]: the stage d ahead of the current one
    qblk[0] = blk;
    qg0[0] = g0;
#pragma unroll
    for (int d = 1; d < BAND_NBUF; ++d) {
        qblk[d] = qblk[d - 1];
        qg0[d] = qg0[d - 1];
        if (qblk[d] <= Bhi) advance(qblk[d], qg0[d]);
    }
#pragma unroll
    for (int d = 0; d < BAND_NBUF - 1; ++d)
        if (qblk[d] <= Bhi) last_issued = issue(qblk[d], qg0[d], d);
    // (the first stage must have landed; with three buffers the second may still be in flight)
    if (BAND_NBUF > 2 && qblk[BAND_NBUF - 2] <= Bhi && BAND_NBUF - 2 > 0) dma_wait(last_issued);
    else lds_dma_drain();
    __syncthreads();
    while (blk <= Bhi) {
        int issued = 0;
        if (qblk[BAND_NBUF - 1] <= Bhi) issued = issue(qblk[BAND_NBUF - 1], qg0[BAND_NBUF - 1], (buf + BAND_NBUF - 1) % BAND_NBUF);
        if (wvalid || noskip) { // (noskip: a wave without a target row walks too, as in k_band_vec and k_band_sep_cols_mfma -- its Er15 is 0 and it writes nothing)
            if (blk != cur_blk) {
                cur_blk = blk;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int cb = SAMPLES ? gcs[16 * blk + 8 * half + e] : gcs[8 * blk + e]; // (pixel targets: the same 8 columns in both lane-halves)
#pragma unroll
                    for (int b = 0; b < PB; ++b) ec[b][e >> 1][e & 1] = elut[min(abs(tc[b] - cb), rad)];
                }
            }
#pragma unroll 1
            for (int slot = 0; slot < BAND_G; ++slot) {
                const int i = g0 + RP * slot;
                if (i >= nb) break;
                const unsigned u = (unsigned)__builtin_amdgcn_readfirstlane((int)wwin[wave * BAND_MAXROWS + i]);
                if (!noskip && !band_win_has(u, blk)) continue;
                ++nsteps;
                const unsigned char *sl = stage + (size_t)(buf * BAND_G + slot) * CHB;
                // (pixel targets: each lane-half its own row of the pair; 0 past the end of the band)
                const int ie = SAMPLES ? i : i + half;
                const float era = ie < nb ? er_s[wave * BAND_MAXROWS + ie] : 0.f;
                kstep(sl, era, ec);
            }
        }
        // the next stage's chunks have landed (what was issued above may stay in flight when there is a buffer to spare)
        if (BAND_NBUF > 2) dma_wait(issued);
        else lds_dma_drain();
        __syncthreads();
#pragma unroll
        for (int d = 0; d < BAND_NBUF - 1; ++d) {
            qblk[d] = qblk[d + 1];
            qg0[d] = qg0[d + 1];
        }
        if (qblk[BAND_NBUF - 1] <= Bhi) advance(qblk[BAND_NBUF - 1], qg0[BAND_NBUF - 1]);
        blk = qblk[0];
        g0 = qg0[0];
        buf = (buf + 1) % BAND_NBUF;
    }
    if (evaluated && lane == 0 && nsteps) atomicAdd(evaluated, nsteps * (unsigned long long)(16 * 32 * PB));

    // ---- epilogue: accumulator register q of a lane is target (q & 3) + 8 (q >> 2) + 4 half of the tile, column l31 of the n-tile
    float iv[MB], csum[MB];
#pragma unroll
    for (int j = 0; j < MB; ++j) {
        iv[j] = inv[32 * j + l31];
        csum[j] = 0.f;
    }
    if (GREY && !SAMPLES && fw) {
        // filter in the epilogue: s_k = Phi[px] . w_k (the guide's w, then the planes' fsig.w [NS][LD]), each summed over the 32 lanes
        // that hold the pixel's columns, then band_filter_store; Phi is not written. (The filter arrives as loose scalars and becomes a
        // BandFilter here: taken by value it moved the registers of the instantiations that write Phi or Y.)
        if (wvalid) {
            BandFilter flt;
            flt.sig = fsig;
            flt.w = fw;
            flt.gain = fgain;
            flt.ysub = fysub;
            flt.out = fout;
            flt.zf = fzf;
            flt.corr = fcorr;
            float wv[1 + NS][MB];
#pragma unroll
            for (int k = 0; k <= NS; ++k)
#pragma unroll
                for (int j = 0; j < MB; ++j) wv[k][j] = (k == 0 ? flt.w[32 * j + l31] : flt.sig.w[(k - 1) * LD + 32 * j + l31]) * iv[j];
#pragma unroll
            for (int b = 0; b < PB; ++b) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    float sdot[1 + NS];
#pragma unroll
                    for (int k = 0; k <= NS; ++k) {
                        sdot[k] = 0.f;
#pragma unroll
                        for (int j = 0; j < MB; ++j) sdot[k] = fmaf(acc[b][j][q], wv[k][j], sdot[k]);
#pragma unroll
                        for (int o = 16; o > 0; o >>= 1) sdot[k] += __shfl_xor(sdot[k], o, 64);
                    }
                    const int col = (tile * PB + b) * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
                    if (l31 == 0 && col < width) {
                        const int64_t px = (int64_t)trow * width + col;
                        if (mask[px]) continue; // (a sample: filter_sample_rows and filter_sample_rows_signals write it from Phi_A)
                        band_filter_store<1 + NS>(flt, fpix0, px, (int)tval[px], sdot);
                    }
                }
            }
        }
        return;
    }
    if (wvalid) {
#pragma unroll
        for (int b = 0; b < PB; ++b) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int t = (q & 3) + 8 * (q >> 2) + 4 * half;
                if (SAMPLES) {
                    const int bi = tile * 32 + t;
                    if (bi >= nc) continue;
                    const size_t s = (size_t)trow * nc + bi;
                    const float dg = (float)degree[s];
#pragma unroll
                    for (int j = 0; j < MB; ++j)
                        out[s * out_ld + 32 * j + l31] = alpha * fmaf(dg, X[s * x_ld + 32 * j + l31], -(acc[b][j][q] * iv[j]));
                } else {
                    const int col = (tile * PB + b) * 32 + t;
                    if (col >= width) continue;
                    const int64_t px = (int64_t)trow * width + col;
                    const bool is_sample = mask[px] != 0;
                    int64_t dst;
                    if (raster) dst = px;
                    else {
                        if (is_sample) continue;
                        dst = (int64_t)p + px - (int64_t)samples_before(idx, p, (uint32_t)px);
                    }
                    const float yv = (!GREY || is_sample) ? 0.f : (float)tval[px]; // (Rgb, U16: no 8-bit y, no c)
#pragma unroll
                    for (int j = 0; j < MB; ++j) {
                        const float v = acc[b][j][q] * iv[j];
                        out[(size_t)dst * out_ld + 32 * j + l31] = v;
                        csum[j] = fmaf(v, yv, csum[j]);
                    }
                }
            }
        }
    }
    if (GREY && !SAMPLES && cpartial) {
        __syncthreads();
        float *red = reinterpret_cast<float *>(stage); // [NW][LD]
#pragma unroll
        for (int j = 0; j < MB; ++j) {
            const float v = csum[j] + __shfl_xor(csum[j], 32, 64);
            if (half == 0) red[wave * LD + 32 * j + l31] = v;
        }
        __syncthreads();
        if (tid < LD) {
            double tot = 0.0;
            for (int w = 0; w < NW; ++w) tot += (double)red[w * LD + tid];
            cpartial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * LD + tid] = tot;
        }
    }
}

// Host-built geometry of the band for one sample grid and kernel: which grid rows lie within the radius of a target row, and
// which blocks of sample columns can reach a tile of targets at a given row distance (BandGeom, band_plan.hpp) -- half-blocks
// of 8 columns for the pixel targets (win_px), blocks of 16 for the sample targets (win_s).
struct BandTables {
    int rad = 0, nr = 0, nc = 0, ksc = 0, width = 0;
    int tile_px = 0, ntiles_px = 0, ntiles_s = 0; // pixels per wave tile (32 PB); wave tiles per image row / per grid row
    bool ok = false;
    // one device blob (one upload): P[256] Ec[rad + 1] Er15[rad + 1] | P replicated as in LDS | grow[nr] gcol[nc] | rowband_px win_px | rowband_s win_s | dcmax[rad]
    DevBuf<unsigned> blob;
    size_t o_pexp = 0, o_grid = 0, o_rb_px = 0, o_win_px = 0, o_rb_s = 0, o_win_s = 0, o_dcmax = 0;
    const float *tab() const { return reinterpret_cast<const float *>(blob.p); }
    const float *pexp() const { return reinterpret_cast<const float *>(blob.p + o_pexp); } // P replicated BAND_PCOPY-fold, as it sits in LDS
    const int *grow() const { return reinterpret_cast<const int *>(blob.p + o_grid); }
    const int *gcol() const { return grow() + nr; }
    const unsigned *rowband_px() const { return blob.p + o_rb_px; }
    const unsigned *win_px() const { return blob.p + o_win_px; }
    const unsigned *rowband_s() const { return blob.p + o_rb_s; }
    const unsigned *win_s() const { return blob.p + o_win_s; }
    const int *dcmax() const { return reinterpret_cast<const int *>(blob.p + o_dcmax); } // geom.dcmax (k_band_vec's support)
    std::vector<unsigned> h_rowband_px; // host copy of rowband_px (the launchers' window plans)
    double er15_rowsum = 0.0;           // max over the image rows r of sum_a Er15(|r - R_a|): |S| <= max |q| times this (the separable form's operand scale)
    int dc0() const { return geom.dcmax.empty() ? -1 : geom.dcmax[0]; } // the circle's half-width in a sample's own row (-1: none)
    int cols_near_tile(int t) const // sample columns within dc0 of pixel tile t: what k_band_vec walks at most
    {
        int lo = 0, n = 0;
        if (dc0() >= 0) band_cols_range(geom.cols.data(), nc, t * tile_px - dc0(), std::min(width, (t + 1) * tile_px) - 1 + dc0(), &lo, &n);
        return n;
    }
    std::vector<double> pairs_dr;   // per row distance: (target column, sample column) pairs inside the circle, pixels as targets
    std::vector<double> pairs_dr_s; // ... the samples as targets
    std::vector<int> hrows;
    BandGeom geom;
    unsigned band_of(int r) const { return geom.band_of(r); }
    double pairs_rows(const std::vector<double> &per_dr, int r) const
    {
        const unsigned rb = band_of(r);
        double tot = 0.0;
        for (int a = (int)(rb & 0xFFFFu); a <= (int)(rb >> 16); ++a) tot += per_dr[std::abs(r - hrows[a])];
        return tot;
    }
    mutable int memo_r0 = -1, memo_r1 = -1;
    mutable double memo_pairs = 0.0;
    double pairs_px(int row0, int row1) const // (pixel, sample) pairs inside the radius for the image rows [row0, row1)
    {
        if (row0 == memo_r0 && row1 == memo_r1) return memo_pairs;
        double tot = 0.0;
        for (int r = row0; r < row1; ++r) tot += pairs_rows(pairs_dr, r);
        memo_r0 = row0;
        memo_r1 = row1;
        memo_pairs = tot;
        return tot;
    }
    double pairs_s(int a0, int a1) const // (sample, sample) pairs inside the radius for the grid rows [a0, a1) as targets
    {
        double tot = 0.0;
        for (int t = a0; t < a1; ++t) tot += pairs_rows(pairs_dr_s, hrows[t]);
        return tot;
    }
    // GLF_ERR_UNSUPPORTED: no spatial factor, or a radius / band beyond what the kernel's LDS tables hold
    int build(glf_ctx *ctx, const GridInfo &g, KernelCoef coef, int width_, int height, int tile_px_, bool want_px, bool want_s)
    {
        ok = false;
        if (!geom.init(g.rows.data(), g.nr, g.cols.data(), g.nc, (double)coef.s_loc)) return GLF_ERR_UNSUPPORTED;
        rad = geom.rad;
        nr = g.nr;
        nc = g.nc;
        ksc = (int)ceil_div(nc, 16);
        width = width_;
        tile_px = tile_px_;
        hrows = g.rows;
        if (nr > 65535 || ksc > 65535) return GLF_ERR_UNSUPPORTED;
        ntiles_px = want_px ? (int)ceil_div(width, tile_px) : 0;
        ntiles_s = want_s ? (int)ceil_div(nc, 32) : 0;
        const size_t n_tab = 256 + 2 * (size_t)(rad + 1);
        o_pexp = (n_tab + 3) / 4 * 4; // (16-byte aligned: copied by global_load_lds_dwordx4)
        o_grid = o_pexp + 256 * (size_t)BAND_PCOPY;
        o_rb_px = o_grid + (size_t)nr + nc;
        o_win_px = o_rb_px + (want_px ? (size_t)height : 0);
        o_rb_s = o_win_px + (size_t)rad * ntiles_px;
        o_win_s = o_rb_s + (want_s ? (size_t)nr : 0);
        o_dcmax = o_win_s + (size_t)rad * ntiles_s;
        std::vector<unsigned> h(o_dcmax + (size_t)rad);
        float *htab = reinterpret_cast<float *>(h.data());
        for (int e = 0; e < 256; ++e) htab[e] = (float)std::exp2(-(double)coef.s_val * e * e);
        for (int d = 0; d <= rad; ++d) {
            const double t = (double)coef.s_loc * (double)d * (double)d;
            htab[256 + d] = d < rad ? (float)std::exp2(-t) : 0.f;
            htab[256 + rad + 1 + d] = d < rad ? (float)std::exp2((double)NYS_F16_KSCALE_LOG2 - t) : 0.f;
        }
        for (int i = 0; i < 256 * BAND_PCOPY; ++i) reinterpret_cast<float *>(h.data())[o_pexp + i] = htab[i / BAND_PCOPY];
        for (int a = 0; a < nr; ++a) h[o_grid + a] = (unsigned)g.rows[a];
        for (int b = 0; b < nc; ++b) h[o_grid + nr + b] = (unsigned)g.cols[b];
        const std::vector<int> &dcmax = geom.dcmax;
        for (int dr = 0; dr < rad; ++dr) h[o_dcmax + dr] = (unsigned)dcmax[dr];
        int maxband = 0;
        if (want_px) {
            for (int r = 0; r < height; ++r) {
                const unsigned rb = band_of(r);
                h[o_rb_px + r] = rb;
                maxband = std::max(maxband, (int)(rb >> 16) - (int)(rb & 0xFFFF) + 1);
            }
            h_rowband_px.assign(h.begin() + o_rb_px, h.begin() + o_win_px);
            er15_rowsum = 0.0;
            for (int r = 0; r < height; ++r) {
                const unsigned rb = h[o_rb_px + r];
                double s = 0.0;
                for (int a = (int)(rb & 0xFFFFu); a <= (int)(rb >> 16); ++a) s += (double)htab[256 + rad + 1 + std::min(std::abs(r - g.rows[a]), rad)];
                er15_rowsum = std::max(er15_rowsum, s);
            }
            for (int dr = 0; dr < rad; ++dr)
                for (int t = 0; t < ntiles_px; ++t) h[o_win_px + (size_t)dr * ntiles_px + t] = geom.window(t * tile_px, std::min(width, (t + 1) * tile_px) - 1, dr, BAND_HALF_SHIFT);
            pairs_dr.assign(rad, 0.0);
            for (int dr = 0; dr < rad; ++dr) {
                if (dcmax[dr] < 0) continue;
                double n = 0.0;
                for (int b = 0; b < nc; ++b) n += (double)(std::min(width - 1, g.cols[b] + dcmax[dr]) - std::max(0, g.cols[b] - dcmax[dr]) + 1);
                pairs_dr[dr] = n;
            }
        }
        if (want_s) {
            for (int a = 0; a < nr; ++a) {
                const unsigned rb = band_of(g.rows[a]);
                h[o_rb_s + a] = rb;
                maxband = std::max(maxband, (int)(rb >> 16) - (int)(rb & 0xFFFF) + 1);
            }
            for (int dr = 0; dr < rad; ++dr)
                for (int t = 0; t < ntiles_s; ++t) h[o_win_s + (size_t)dr * ntiles_s + t] = geom.window(g.cols[t * 32], g.cols[std::min(nc, (t + 1) * 32) - 1], dr, BAND_BLOCK_SHIFT);
            pairs_dr_s.assign(rad, 0.0);
            for (int dr = 0; dr < rad; ++dr) {
                if (dcmax[dr] < 0) continue;
                double n = 0.0;
                int lo = 0, hi = 0; // (two pointers: the columns ascend)
                for (int b = 0; b < nc; ++b) {
                    while (lo < nc && g.cols[lo] < g.cols[b] - dcmax[dr]) ++lo;
                    while (hi < nc && g.cols[hi] <= g.cols[b] + dcmax[dr]) ++hi;
                    n += (double)(hi - lo);
                }
                pairs_dr_s[dr] = n;
            }
        }
        if (maxband + 8 > BAND_MAXROWS) return GLF_ERR_UNSUPPORTED; // (a workgroup: the union over its target rows)
        GLF_TRY(blob.alloc(ctx, h.size()));
        GLF_HIP(ctx, hipMemcpyAsync(blob.p, h.data(), sizeof(unsigned) * h.size(), hipMemcpyHostToDevice, ctx->stream));
        GLF_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (pageable host vector)
        ok = true;
        return GLF_OK;
    }
    // is the band a small part of the grid? (auto mode: otherwise the factored forms, which carry all samples, do less work)
    bool narrow(int height) const { return 2.0 * rad < 0.5 * std::min(width, height); }
};

// the context's cached tables for (grid, kernel, image size, targets); rebuilt when any of them differs from the last call's
struct BandCacheEntry {
    BandTables bt;
    std::vector<int> rows, cols;
    float s_loc = 0.f, s_val = 0.f;
    int width = 0, height = 0, tile_px = 0;
};
static void band_cache_delete(void *e) { delete reinterpret_cast<BandCacheEntry *>(e); }
static int band_tables_cached(glf_ctx *ctx, const GridInfo &g, KernelCoef coef, int width, int height, int tile_px, bool px, const BandTables **out)
{
    using Entry = BandCacheEntry;
    Entry *&e = reinterpret_cast<Entry *&>(ctx->band_cache[px ? 0 : 1]);
    if (e && e->bt.ok && e->rows == g.rows && e->cols == g.cols && e->s_loc == coef.s_loc && e->s_val == coef.s_val && e->width == width &&
        e->height == height && e->tile_px == tile_px) {
        *out = &e->bt;
        return GLF_OK;
    }
    delete e;
    e = new Entry;
    e->rows = g.rows;
    e->cols = g.cols;
    e->s_loc = coef.s_loc;
    e->s_val = coef.s_val;
    e->width = width;
    e->height = height;
    e->tile_px = tile_px;
    const int rc = e->bt.build(ctx, g, coef, width, height, tile_px, px, !px);
    if (rc != GLF_OK) {
        delete e;
        e = nullptr;
        return rc;
    }
    *out = &e->bt;
    return GLF_OK;
}

#ifndef BAND_NW_S_X
#define BAND_NW_S_X 8
#endif
constexpr int BAND_NW_S = BAND_NW_S_X;                // sample targets: 32 per wave, 8 grid rows per workgroup

// G: the pixel format of d_img (Rgb, U16: Phi is written; no filter, no c; nsval = -s_val of the kernel)
template <int MB, int NS = 0, PixGen G = PixGen::Grey>
static int launch_band_px(glf_ctx *ctx, const BandTables &bt, const uint8_t *d_img, int row0, int nrows, const unsigned char *chunks,
                          const float *inv, float *phi, int phi_ld, const uint8_t *d_mask, const uint32_t *d_idx, unsigned p, int raster,
                          double *cpartial, unsigned long long *evaluated, const BandFilter *flt = nullptr, int64_t pix0 = 0, float nsval = 0.f)
{
    if constexpr (G != PixGen::Grey)
        if (flt || cpartial) return set_error(ctx, GLF_ERR_INVALID, "k_band: the colour and 16-bit formats have no filter epilogue");
    if constexpr (NS == 0 && G == PixGen::Grey) // the planes ride in the filter's epilogue: one instantiation per plane count
        if (flt && flt->sig.nsig > 0) {
            if (flt->sig.nsig >= BANDV_MAXNC) return set_error(ctx, GLF_ERR_INVALID, "k_band: %d signal planes", flt->sig.nsig);
            return band_dispatch_planes(1 + flt->sig.nsig, [&](auto nc) -> int {
                return launch_band_px<MB, decltype(nc)::value - 1>(ctx, bt, d_img, row0, nrows, chunks, inv, phi, phi_ld, d_mask, d_idx, p, raster,
                                                                   cpartial, evaluated, flt, pix0);
            });
        }
    auto kern = k_band<MB, BAND_PB, BAND_NW, false, NS, G>;
    const unsigned lds = band_lds_bytes(MB, BAND_NW, bt.rad, bt.ksc, false, G == PixGen::Grey);
    GLF_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)bt.ntiles_px, (unsigned)ceil_div(nrows, BAND_NW));
    hipLaunchKernelGGL(kern, grid, dim3(BAND_NW * 64), lds, ctx->stream, d_img, bt.width, row0, bt.grow(), bt.gcol(), bt.nr, bt.nc,
                       bt.ksc, bt.tab(), bt.pexp(), bt.rad, bt.rowband_px(), bt.win_px(), bt.ntiles_px, chunks, inv, phi, phi_ld, d_mask, d_idx, p, raster,
                       cpartial, (const float *)nullptr, 0, (const double *)nullptr, 0.f, evaluated, row0 + nrows, flt ? flt->w : (const float *)nullptr,
                       flt ? flt->gain : 0.f, flt ? flt->ysub : 0.f, flt ? flt->out : (uint8_t *)nullptr, flt ? flt->zf : (float *)nullptr,
                       flt ? flt->corr : (float *)nullptr, pix0, flt ? flt->sig : BandSignals{}, ctx->tune.band_noskip ? 1 : 0, nsval);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}
inline size_t band_px_wgs(const BandTables &bt, int nrows) { return (size_t)bt.ntiles_px * (size_t)ceil_div(nrows, BAND_NW); }

// (Rgb, U16: svals is the u32 image of the sample values, passed as bytes)
template <int MB, PixGen G = PixGen::Grey>
static int launch_band_samples(glf_ctx *ctx, const BandTables &bt, const uint8_t *svals, int a0, int nrows, const unsigned char *chunks,
                               const float *inv, float *Y, int y_ld, const float *X, int x_ld, const double *degree, float alpha,
                               unsigned long long *evaluated, float nsval = 0.f)
{
    auto kern = k_band<MB, 1, BAND_NW_S, true, 0, G>;
    const unsigned lds = band_lds_bytes(MB, BAND_NW_S, bt.rad, bt.ksc, true, G == PixGen::Grey);
    GLF_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)bt.ntiles_s, (unsigned)ceil_div(nrows, BAND_NW_S));
    hipLaunchKernelGGL(kern, grid, dim3(BAND_NW_S * 64), lds, ctx->stream, svals, bt.nc, a0, bt.grow(), bt.gcol(), bt.nr, bt.nc, bt.ksc,
                       bt.tab(), bt.pexp(), bt.rad, bt.rowband_s(), bt.win_s(), bt.ntiles_s, chunks, inv, Y, y_ld, (const uint8_t *)nullptr,
                       (const uint32_t *)nullptr, 0u, 1, (double *)nullptr, X, x_ld, degree, alpha, evaluated, a0 + nrows, (const float *)nullptr, 0.f,
                       0.f, (uint8_t *)nullptr, (float *)nullptr, (float *)nullptr, (int64_t)0, BandSignals{}, 0, nsval);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// svals: uint8 [nr][nc] (raw = false) or u32 [nr][nc] (raw: the colour and 16-bit formats)
// (nch = 3: float colour, three planes)
static int band_prep(glf_ctx *ctx, const float *X, unsigned x_ld, const float *colscale, const void *svals, bool raw, int nr, int nc, int ksc, int mb,
                     unsigned char *chunks, int nch = 1)
{
    const size_t total = (size_t)nr * ksc * mb * 64;
    auto kern = raw && nch == 3 ? k_band_prep<true, 3> : raw ? k_band_prep<true> : k_band_prep<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div((int64_t)total, 256)), dim3(256), 0, ctx->stream, X, x_ld, colscale, svals, nr, nc, ksc, mb, chunks);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

// What the launchers of the three forms share. The sample values as bytes [p]:
static int band_svals(glf_ctx *ctx, const float4 *d_samples, unsigned p, DevBuf<uint8_t> &svals)
{
    GLF_TRY(svals.alloc(ctx, p));
    hipLaunchKernelGGL(k_gridop_svals, dim3((p + 255) / 256), dim3(256), 0, ctx->stream, d_samples, p, svals.p);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}
// the kernels' counter of evaluated entries: zeroed on the stream; read back (through the pinned block) with the stream synchronised
static int band_eval_zero(glf_ctx *ctx, DevBuf<unsigned long long> &dev_eval)
{
    GLF_TRY(dev_eval.alloc(ctx, 1));
    GLF_HIP(ctx, hipMemsetAsync(dev_eval.p, 0, sizeof(unsigned long long), ctx->stream));
    return GLF_OK;
}
static int band_eval_read(glf_ctx *ctx, const DevBuf<unsigned long long> &dev_eval, unsigned long long *h_eval)
{
    unsigned long long *pin_eval = ctx_pinned(ctx) ? reinterpret_cast<unsigned long long *>(ctx_pinned(ctx) + PINNED_BANDEVAL) : nullptr;
    GLF_HIP(ctx, hipMemcpyAsync(pin_eval ? pin_eval : h_eval, dev_eval.p, sizeof(*h_eval), hipMemcpyDeviceToHost, ctx->stream));
    GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (pin_eval) *h_eval = *pin_eval;
    return GLF_OK;
}
// the launch as the statistics report it: `launches` launches of ms in all over `cols` columns (Phi's, or one per plane), R expansion terms
static void band_stats(RowpassStats *stats, const BandTables &bt, int row0, int row1, int launches, float ms, unsigned cols, int R)
{
    if (!stats) return;
    stats->col_launches = launches;
    stats->col_ms = ms;
    stats->col_flops = 2.0 * bt.pairs_px(row0, row1) * cols; // algorithmic: the (pixel, sample) pairs inside the radius (memoised), one multiply-add per column
    stats->rank_R = R;
}

// (nystroem_band_vec.inc: the fused filter contracted with q = Psi w, one column per plane)
static int launch_nystroem_band_vec(glf_ctx *ctx, const NysRequest &rq, const BandTables &bt);
// (nystroem_band_sep.inc: the same sum in separable form, the photometric table as its rank-R expansion)
static int launch_nystroem_band_sep(glf_ctx *ctx, const NysRequest &rq, const BandTables &bt);

// Nystroem extension of the image rows [pix0 / width, pix1 / width) in band form (see the head of this file). With rq.flt the
// request names no Phi and no c (nystroem_band_filter sees to it).
static int launch_nystroem_band(glf_ctx *ctx, const NysRequest &rq, const GridInfo &g, bool forced)
{
    const BandTables *btp = nullptr;
    GLF_TRY(band_tables_cached(ctx, g, rq.coef, rq.width, rq.height, 32 * BAND_PB, true, &btp));
    const BandTables &bt = *btp;
    if (!forced && !bt.narrow(rq.height)) return GLF_ERR_UNSUPPORTED;
    hipStream_t st = ctx->stream;
    const int row0 = (int)(rq.pix0 / rq.width), row1 = (int)(rq.pix1 / rq.width), nrows = row1 - row0;
    const unsigned LD = rq.ld >= 64 ? 64u : 32u, nblocks = rq.ld / LD;
    const int mb = (int)LD / 32;
    DevBuf<float> colscale, inv, camx;
    DevBuf<uint8_t> svals;
    DevBuf<unsigned> svals32; // (Rgb, U16, F32: the sample values as u32; float colour: three planes)
    DevBuf<unsigned char> chunks;
    DevBuf<double> cpart;
    const PixGen gen = pixgen_of(rq.coef.kernel);
    const bool raw = gen != PixGen::Grey;
    if (raw && (rq.flt || rq.d_c)) return GLF_ERR_UNSUPPORTED; // (no 8-bit y: the filter stays a stage of its own)
    if (rq.flt && rq.ld > 64) return GLF_ERR_UNSUPPORTED; // (the filter's dot product with w runs over one block of at most 64 columns)
    // FILTER_FORM: sep (separable rank-R form) where the photometric table has an expansion, else vec (pair by pair, one column per
    // plane instead of Phi's), else -- its LDS window too large -- k_band's epilogue
    if (rq.flt && ctx->tune.filter_form <= 1) {
        const int rc = launch_nystroem_band_sep(ctx, rq, bt);
        if (rc != GLF_ERR_UNSUPPORTED) return rc;
    }
    if (rq.flt && ctx->tune.filter_form <= 2) {
        const int rc = launch_nystroem_band_vec(ctx, rq, bt);
        if (rc != GLF_ERR_UNSUPPORTED) return rc;
    }
    DevBuf<unsigned long long> dev_eval;
    ctx->nys_note.skipping = ctx->tune.band_noskip ? 0 : 1; // (the band is a window by construction; BAND_NOSKIP executes all of it)
    GLF_TRY(colscale.alloc(ctx, rq.ld));
    GLF_TRY(inv.alloc(ctx, rq.ld));
    GLF_TRY(camx.alloc(ctx, (size_t)ceil_div(rq.p, CAM_ROWS) * rq.ld));
    if (raw) GLF_TRY(svals32.alloc(ctx, (size_t)pix_desc(gen).svals32_planes * rq.p));
    GLF_TRY(chunks.alloc(ctx, (size_t)bt.nr * bt.ksc * band_chunk_bytes(mb)));
    const size_t wgs = band_px_wgs(bt, nrows);
    if (rq.d_c) GLF_TRY(cpart.alloc(ctx, wgs * LD));
    GLF_TRY(band_eval_zero(ctx, dev_eval));
    band_scales(st, rq.d_psi, rq.p, rq.ld, camx.p, colscale.p, inv.p);
    if (raw) {
        hipLaunchKernelGGL(k_gridop_svals32, dim3((rq.p + 255) / 256), dim3(256), 0, st, rq.d_samples, rq.p, pix_desc(gen).svals32_what, svals32.p);
        GLF_LAUNCH_CHECK(ctx);
    } else GLF_TRY(band_svals(ctx, rq.d_samples, rq.p, svals));
    if (rq.kernel_ms) GLF_HIP(ctx, hipEventRecord(ctx->ev[6], st));
    float band_ms = 0.f;
    CpTimer timer{ctx, rq.rowpass != nullptr};
    for (unsigned cb = 0; cb < nblocks; ++cb) {
        const unsigned c0 = cb * LD;
        GLF_TRY(band_prep(ctx, rq.d_psi + c0, rq.ld, colscale.p + c0, raw ? (const void *)svals32.p : (const void *)svals.p, raw, bt.nr, bt.nc, bt.ksc, mb, chunks.p, pix_desc(gen).svals32_planes));
        GLF_TRY(timer.start());
        if (raw) {
            float *po = rq.d_phi + c0;
            const float nsval = -rq.coef.s_val;
            int rc = GLF_OK;
            pix_dispatch_raw(gen, [&](auto t) { // (these formats' k_band exists for one and two column blocks only)
                rc = mb == 2 ? launch_band_px<2, 0, t.G>(ctx, bt, rq.d_img, row0, nrows, chunks.p, inv.p + c0, po, (int)rq.ld, rq.d_mask, rq.d_idx, rq.p, rq.raster,
                                                         nullptr, dev_eval.p, nullptr, rq.pix0, nsval)
                             : launch_band_px<1, 0, t.G>(ctx, bt, rq.d_img, row0, nrows, chunks.p, inv.p + c0, po, (int)rq.ld, rq.d_mask, rq.d_idx, rq.p, rq.raster,
                                                         nullptr, dev_eval.p, nullptr, rq.pix0, nsval);
            });
            GLF_TRY(rc);
        } else if (mb == 2)
            GLF_TRY(launch_band_px<2>(ctx, bt, rq.d_img, row0, nrows, chunks.p, inv.p + c0, rq.flt ? nullptr : rq.d_phi + c0, (int)rq.ld, rq.d_mask, rq.d_idx, rq.p,
                                      rq.raster, rq.d_c ? cpart.p : nullptr, dev_eval.p, rq.flt, rq.pix0));
        else
            GLF_TRY(launch_band_px<1>(ctx, bt, rq.d_img, row0, nrows, chunks.p, inv.p + c0, rq.flt ? nullptr : rq.d_phi + c0, (int)rq.ld, rq.d_mask, rq.d_idx, rq.p,
                                      rq.raster, rq.d_c ? cpart.p : nullptr, dev_eval.p, rq.flt, rq.pix0));
        GLF_TRY(timer.stop());
        if (rq.d_c) GLF_TRY(sum_rows(ctx, cpart.p, (int64_t)wgs, LD, rq.d_c + c0, true)); // synchronises
    }
    if (rq.kernel_ms) GLF_HIP(ctx, hipEventRecord(ctx->ev[7], st));
    unsigned long long h_eval = 0;
    GLF_TRY(band_eval_read(ctx, dev_eval, &h_eval)); // (synchronises)
    GLF_TRY(timer.total(&band_ms));
    if (rq.kernel_ms) GLF_HIP(ctx, hipEventElapsedTime(rq.kernel_ms, ctx->ev[6], ctx->ev[7]));
    // (every column block evaluates the same entries: per block, h_eval / nblocks)
    if (rq.entries_evaluated) *rq.entries_evaluated = (uint64_t)(h_eval / std::max(1u, nblocks));
    if (rq.mfma_flops) *rq.mfma_flops = 6.0 * (double)h_eval * LD; // three split products per entry and column
    band_stats(rq.rowpass, bt, row0, row1, (int)nblocks, band_ms, rq.ld, 0);
    return GLF_OK;
}
