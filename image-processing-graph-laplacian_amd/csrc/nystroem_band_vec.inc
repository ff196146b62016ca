// Band form with the filter collapsed to one column (included from nystroem_grid.inc after nystroem_band.inc, inside namespace glf).
//
// With the filter in the epilogue the only thing kept of a pixel's 64 columns of Phi is s[px] = sum_n Phi[px][n] w[n]
// = sum_s K(px, s) q[s] with q = Psi w, a p-vector known before the launch (w = f(lambda) c, c from c_from_ysum). So the
// launch contracts K with one column (NC = 1 + the signal planes of joint filtering, one q_k = Psi w_k each) instead of 64:
// no MFMA, no f16 split, no operand chunks, no cross-lane reduction. One lane owns one pixel: a wave is 64 pixels of one
// image row, a sample is wave-uniform, and the circle is cut per single sample column.
//   per sample column b of the workgroup's range (outer) and band row a (inner):
//     address = |64 v_px - 64 v_s| + table (v_sad_u32), P = one ds_read_b32, zeroed where |dc| > dcmax[dr] (the
//     support, per lane), t = P Er15(dr_a), inner += t q[s]; Ec(|dc|) -- one LDS gather per (lane, b) -- multiplies the inner
//     sum once, and the product is folded into the pixel's total in f64.
// The wave-uniform Er15(dr_a) and dcmax[dr_a] of 16 band rows sit in scalar registers (the rows are walked in chunks of 16,
// fully unrolled), so an entry costs two LDS reads: the sample's (64 v_s, q) at a wave-uniform address and the gather of P.
// Within a chunk the rows go in groups of eight without a branch between them, so that the eight gathers are in flight together;
// a group's samples come in 16-byte LDS reads. The table of P is k_band's 16-fold image (BAND_PCOPY): lanes l and l + 16 of a
// ds_read_b32 share a bank, so a gather whose two lanes differ takes a second LDS cycle; 32 copies would be conflict-free but cost a
// workgroup per CU (DESIGN section 4).
// Support: a (pixel, sample) pair contributes iff dr < rad and |dc| <= dcmax[dr] (band_plan.hpp) -- the set BandTables::pairs_px
// counts. k_band instead flushes the individual entries whose product rounds to a zero f16 pair: terms below 2^-40 of the
// largest one, which enter here with full f32 relative precision.

constexpr int BANDV_CHUNK = 16, BANDV_GROUP = 8;          // band rows per set of scalar registers / per branch-free group
static_assert(BANDV_GROUP % 4 == 0 && BANDV_CHUNK % BANDV_GROUP == 0, "a group's samples are read 16 bytes at a time");
static_assert(32 * BAND_PB == 64, "k_band_vec: one lane per pixel of a 64-column tile (BandTables' tile_px)");
constexpr unsigned BANDV_LDS_MAX = 64u * 1024u;           // what a workgroup may take

// [wcap][nbcap] samples of 1 + nc dwords | Ec[rad + 1] | columns[wcap] | Er15[NW][nbcap] | dcmax[NW][nbcap] | rows per column [NW][wcap] | misc
__host__ __device__ inline unsigned band_vec_lds_bytes(int ncol, int rad, int wcap, int nbcap)
{
    return 256u * BAND_PSTRIDE + 4u * ((unsigned)wcap * (unsigned)nbcap * (unsigned)(1 + ncol) + (unsigned)(rad + 1) + (unsigned)wcap +
                                       2u * BAND_NW * (unsigned)nbcap + BAND_NW * (unsigned)wcap + 4u);
}

// out[k] = sum_n row[n] w_k[n] over one sample's row of Psi, in f64 (the callers round once). w_0 = w, w_k = sig_w[k - 1]; a zero
// weight skips its column, so the padded columns of Psi never enter. (Summed in locals and copied out: accumulating through the
// reference costs both callers 4 - 8 VGPRs, and their NC = 5 a wave per SIMD.)
template <int NC>
__device__ __forceinline__ void band_q_row(const float *psi_row, unsigned ld, const float *w, const float *sig_w, double (&out)[NC])
{
    double acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.0;
    const float4 *row = reinterpret_cast<const float4 *>(psi_row);
    for (unsigned n = 0; n < ld; n += 4) {
        const float4 x4 = row[n / 4];
        const float x[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const float wv = k == 0 ? w[n + u] : sig_w[(size_t)(k - 1) * ld + n + u];
                if (wv != 0.f) acc[k] = fma((double)x[u], (double)wv, acc[k]);
            }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) out[k] = acc[k];
}

// q[k][s] = (float)(Psi[s] . w_k), [NC][p32] zero-padded
template <int NC>
__global__ __launch_bounds__(256) void k_band_q(const float *__restrict__ psi, unsigned p, unsigned p32, unsigned ld, const float *__restrict__ w,
                                                const float *__restrict__ sig_w, float *__restrict__ q)
{
    const unsigned s = blockIdx.x * 256 + threadIdx.x;
    if (s >= p32) return;
    double acc[NC] = {};
    if (s < p) band_q_row<NC>(psi + (size_t)s * ld, ld, w, sig_w, acc);
#pragma unroll
    for (int k = 0; k < NC; ++k) q[(size_t)k * p32 + s] = (float)acc[k];
}

// 8 waves = 8 consecutive image rows x one tile of 64 columns, one lane per pixel (k_band's pixel-target workgroup: rowband, grow,
// gcol, btab and pexp are its tables). wcap, nbcap: the widest range of sample columns / the most band rows (a multiple of
// BANDV_GROUP) of any workgroup of the launch -- the host sizes the LDS window from them.
template <int NC>
__global__ __launch_bounds__(BAND_NW * 64) void k_band_vec(const uint8_t *__restrict__ img, int width, int row_begin, int row_end,
                                                           const int *__restrict__ grow, const int *__restrict__ gcol, int nc,
                                                           const float *__restrict__ btab, const float *__restrict__ pexp, int rad,
                                                           const unsigned *__restrict__ rowband, const int *__restrict__ dcmax,
                                                           const uint8_t *__restrict__ svals, const float *__restrict__ q, unsigned q_ld, int wcap,
                                                           int nbcap, const uint8_t *__restrict__ mask, BandFilter flt, int64_t fpix0, int noskip,
                                                           unsigned long long *__restrict__ evaluated)
{
    constexpr int NW = BAND_NW, EW = 1 + NC;
    constexpr unsigned PLUT_BYTES = 256 * BAND_PSTRIDE;
    extern __shared__ __attribute__((aligned(16))) unsigned char bvdyn[];
    float *plut = reinterpret_cast<float *>(bvdyn);                       // the photometric table, BAND_PCOPY copies
    unsigned *smp = reinterpret_cast<unsigned *>(bvdyn + PLUT_BYTES);     // [wcap][nbcap][EW]: 64 v_s, q_0 .. q_{NC-1}
    float *elut = reinterpret_cast<float *>(smp + (size_t)wcap * nbcap * EW); // [rad + 1]: Ec(d), 0 at d = rad
    int *gcs = reinterpret_cast<int *>(elut + (rad + 1));                 // [wcap]: the sample columns of the range
    float *er_s = reinterpret_cast<float *>(gcs + wcap);                  // [NW][nbcap]: 2^15 Er of the band rows, per wave
    int *dcm = reinterpret_cast<int *>(er_s + NW * nbcap);                // [NW][nbcap]: dcmax[dr] of the band rows, per wave (-1: outside)
    unsigned *irange = reinterpret_cast<unsigned *>(dcm + NW * nbcap);    // [NW][wcap]: first | last << 16 band row a wave needs of a column
    int *misc = reinterpret_cast<int *>(irange + NW * wcap);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int trow0 = row_begin + blockIdx.y * NW, ntw = min(NW, row_end - trow0);
    const int tc0 = blockIdx.x * 64, tc1 = min(width, tc0 + 64) - 1;
    int alo, ahi;
    band_rows_hull(rowband, trow0, ntw, &alo, &ahi);
    const int nb = min(nbcap, max(0, ahi - alo + 1)), nbp = (nb + BANDV_GROUP - 1) / BANDV_GROUP * BANDV_GROUP; // (nbcap is a multiple of the group)
    { // (the replicated table as it sits in the tables blob, 1 KiB per instruction)
        constexpr int PIECES = 256 * BAND_PCOPY * 4 / 1024;
        const unsigned char *src = reinterpret_cast<const unsigned char *>(pexp);
        const unsigned dst0 = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_offset_of(plut));
        for (int piece = wave; piece < PIECES; piece += NW) lds_dma_16B(src + (size_t)piece * 1024 + lane * 16, dst0 + (unsigned)piece * 1024u);
    }
    for (int i = tid; i <= rad; i += NW * 64) elut[i] = btab[256 + i];
    if (tid == 0) misc[0] = -1;
    __syncthreads();
    // per (wave, band row): Er15 and the half-width of the circle; the widest half-width of the workgroup
    for (int i = tid; i < nbp; i += NW * 64) {
        int mx = -1;
        for (int w = 0; w < NW; ++w) {
            const int dr = i < nb && w < ntw ? abs(trow0 + w - grow[alo + i]) : rad;
            er_s[w * nbcap + i] = dr < rad ? btab[256 + rad + 1 + dr] : 0.f;
            const int dm = dr < rad ? dcmax[dr] : -1;
            dcm[w * nbcap + i] = dm;
            mx = max(mx, dm);
        }
        if (mx >= 0) atomicMax(&misc[0], mx);
    }
    __syncthreads();
    // the workgroup's range of sample columns: within the widest half-width of the tile
    const int dmx = __builtin_amdgcn_readfirstlane(misc[0]);
    int Clo = 0, W = 0;
    if (dmx >= 0) {
        band_cols_range(gcol, nc, tc0 - dmx, tc1 + dmx, &Clo, &W);
        W = min(wcap, W);
    }
    // the samples, once: column-major so that the band rows of a column are contiguous; rows nb .. nbp - 1 are zeros
    for (int e = tid; e < W * nbp; e += NW * 64) {
        const int i = e / W, bb = e - i * W;
        unsigned *ent = smp + ((size_t)bb * nbcap + i) * EW;
        if (i < nb) {
            const size_t s = (size_t)(alo + i) * nc + Clo + bb;
            ent[0] = BAND_PSTRIDE * (unsigned)svals[s];
#pragma unroll
            for (int k = 0; k < NC; ++k) ent[1 + k] = __float_as_uint(q[(size_t)k * q_ld + s]);
        } else {
#pragma unroll
            for (int k = 0; k < EW; ++k) ent[k] = 0u;
        }
    }
    for (int bb = tid; bb < W; bb += NW * 64) gcs[bb] = gcol[Clo + bb];
    // per (wave, column): the band rows whose circle reaches the column from some pixel of the tile (contiguous: the half-width
    // falls with dr). noskip: every band row of the workgroup for every column of its range, for every wave -- one without an image
    // row included (its Er15 is 0 and its dcmax -1: the walk adds nothing and it writes nothing).
    for (int t = tid; t < NW * W; t += NW * 64) {
        const int w = t / W, bb = t - w * W, gc = gcol[Clo + bb], dist = max(0, max(tc0 - gc, gc - tc1));
        int i0 = 0xFFFF, i1 = 0;
        if (noskip && nb > 0) {
            i0 = 0;
            i1 = nb - 1;
        } else if (w < ntw) {
            for (int i = 0; i < nb; ++i)
                if (dcm[w * nbcap + i] >= dist) {
                    i0 = min(i0, i);
                    i1 = max(i1, i);
                }
        }
        irange[w * wcap + bb] = (unsigned)i0 | ((unsigned)i1 << 16);
    }
    lds_dma_drain();
    __syncthreads();

    if (wave >= ntw && !noskip) return;
    const int trow = min(trow0 + wave, row_end - 1), tcol = min(tc0 + lane, width - 1);
    const unsigned pv = BAND_PSTRIDE * (unsigned)img[(size_t)trow * width + tcol];
    const unsigned pbase = lds_offset_of(plut) + 4u * (unsigned)(lane % BAND_PCOPY);
    double tot[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) tot[k] = 0.0;
    unsigned long long nsteps = 0;
    for (int c0 = 0; c0 < nb; c0 += BANDV_CHUNK) {
        float era[BANDV_CHUNK]; // (wave-uniform: scalar registers)
        int dmr[BANDV_CHUNK];
#pragma unroll
        for (int j = 0; j < BANDV_CHUNK; ++j) {
            const bool in = c0 + j < nb;
            era[j] = in ? __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(er_s[wave * nbcap + c0 + j]))) : 0.f;
            dmr[j] = in ? __builtin_amdgcn_readfirstlane(dcm[wave * nbcap + c0 + j]) : -1;
        }
        for (int bb = 0; bb < W; ++bb) {
            const unsigned r = (unsigned)__builtin_amdgcn_readfirstlane((int)irange[wave * wcap + bb]);
            const int i0 = (int)(r & 0xFFFFu), i1 = (int)(r >> 16);
            if (i0 > i1 || i1 < c0 || i0 >= c0 + BANDV_CHUNK) continue;
            const int adc = abs(tcol - gcs[bb]);
            const float ecv = elut[min(adc, rad)];
            const unsigned *col = smp + (size_t)bb * nbcap * EW;
            float inner[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) inner[k] = 0.f;
#pragma unroll
            for (int g = 0; g < BANDV_CHUNK; g += BANDV_GROUP) {
                const int ib = c0 + g; // (a live group lies below nbp: ib <= i1 < nb, and nbp is a multiple of the group)
                if (ib + BANDV_GROUP - 1 < i0 || ib > i1) continue;
                nsteps += BANDV_GROUP;
                unsigned ent[BANDV_GROUP * EW]; // (the group starts at a multiple of 16 EW bytes)
#pragma unroll
                for (int e = 0; e < BANDV_GROUP * EW / 4; ++e) {
                    const uint4 v = reinterpret_cast<const uint4 *>(col + ib * EW)[e];
                    ent[4 * e] = v.x, ent[4 * e + 1] = v.y, ent[4 * e + 2] = v.z, ent[4 * e + 3] = v.w;
                }
                float pp[BANDV_GROUP];
#pragma unroll
                for (int u = 0; u < BANDV_GROUP; ++u) pp[u] = lds_f32(sad_u32(pv, ent[u * EW], pbase));
#pragma unroll
                for (int u = 0; u < BANDV_GROUP; ++u) {
                    const float t = (adc <= dmr[g + u] ? pp[u] : 0.f) * era[g + u];
#pragma unroll
                    for (int k = 0; k < NC; ++k) inner[k] = fmaf(t, __uint_as_float(ent[u * EW + 1 + k]), inner[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < NC; ++k) tot[k] += (double)(ecv * inner[k]);
        }
    }
    if (evaluated && lane == 0 && nsteps) atomicAdd(evaluated, nsteps * 64ull);

    // the filter, one lane per pixel (the sample pixels are filter_sample_rows' from Phi_A)
    if (wave >= ntw || tc0 + lane >= width) return;
    const int64_t px = (int64_t)trow * width + tcol;
    if (mask[px]) return;
    float sdot[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) sdot[k] = (float)(tot[k] * BAND_UNSCALE);
    band_filter_store<NC>(flt, fpix0, px, (int)img[px], sdot);
}

// the LDS window of a launch over the image rows [row0, row1): the most band rows of a workgroup (rounded up to the group) and the
// widest range of sample columns of a tile
static void band_vec_caps(const BandTables &bt, int row0, int row1, int *wcap, int *nbcap)
{
    int nbmax = 0, wmax = 0;
    for (int r = row0; r < row1; r += BAND_NW) {
        int alo, ahi;
        band_rows_hull(bt.h_rowband_px.data(), r, std::min(BAND_NW, row1 - r), &alo, &ahi);
        nbmax = std::max(nbmax, ahi - alo + 1);
    }
    for (int t = 0; t < bt.ntiles_px; ++t) wmax = std::max(wmax, bt.cols_near_tile(t));
    *wcap = std::max(1, wmax);
    *nbcap = std::max(BANDV_GROUP, (std::min(nbmax, BAND_MAXROWS) + BANDV_GROUP - 1) / BANDV_GROUP * BANDV_GROUP);
}

// The fused filter of the image rows [pix0 / width, pix1 / width) through k_band_vec: the sample values, q = Psi w (and the planes'),
// one launch. GLF_ERR_UNSUPPORTED: the window of samples does not fit the LDS (the caller takes k_band's epilogue then).
static int launch_nystroem_band_vec(glf_ctx *ctx, const NysRequest &rq, const BandTables &bt)
{
    const int row0 = (int)(rq.pix0 / rq.width), row1 = (int)(rq.pix1 / rq.width), nrows = row1 - row0;
    const BandFilter &flt = *rq.flt;
    const int ncol = 1 + flt.sig.nsig;
    if (ncol < 1 || ncol > BANDV_MAXNC || bt.width != rq.width) return GLF_ERR_UNSUPPORTED;
    int wcap = 0, nbcap = 0;
    band_vec_caps(bt, row0, row1, &wcap, &nbcap);
    const unsigned lds = band_vec_lds_bytes(ncol, bt.rad, wcap, nbcap);
    if (lds > BANDV_LDS_MAX) return GLF_ERR_UNSUPPORTED;
    hipStream_t st = ctx->stream;
    const unsigned p32 = (unsigned)round_up(rq.p, VEC_PAD);
    DevBuf<uint8_t> svals;
    DevBuf<float> q;
    DevBuf<unsigned long long> dev_eval;
    GLF_TRY(q.alloc(ctx, (size_t)ncol * p32));
    GLF_TRY(band_eval_zero(ctx, dev_eval));
    GLF_TRY(band_svals(ctx, rq.d_samples, rq.p, svals));
    hipEvent_t e0 = ctx->ev[6], e1 = ctx->ev[7];
    GLF_TRY(band_dispatch_planes(ncol, [&](auto nc_) -> int {
        constexpr int NC = decltype(nc_)::value;
        hipLaunchKernelGGL(k_band_q<NC>, dim3((p32 + 255) / 256), dim3(256), 0, st, rq.d_psi, rq.p, p32, rq.ld, flt.w, flt.sig.w, q.p);
        const dim3 grid((unsigned)bt.ntiles_px, (unsigned)ceil_div(nrows, BAND_NW));
        (void)hipEventRecord(e0, st);
        hipLaunchKernelGGL(k_band_vec<NC>, grid, dim3(BAND_NW * 64), lds, st, rq.d_img, bt.width, row0, row1, bt.grow(), bt.gcol(), bt.nc, bt.tab(), bt.pexp(),
                           bt.rad, bt.rowband_px(), bt.dcmax(), svals.p, q.p, p32, wcap, nbcap, rq.d_mask, flt, rq.pix0, ctx->tune.band_noskip ? 1 : 0, dev_eval.p);
        (void)hipEventRecord(e1, st);
        return GLF_OK;
    }));
    GLF_LAUNCH_CHECK(ctx);
    unsigned long long h_eval = 0;
    GLF_TRY(band_eval_read(ctx, dev_eval, &h_eval));
    float ms = 0.f;
    GLF_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    if (rq.kernel_ms) *rq.kernel_ms = ms;
    if (rq.entries_evaluated) *rq.entries_evaluated = (uint64_t)h_eval; // wave-level entry steps x 64 lanes
    if (rq.mfma_flops) *rq.mfma_flops = 0.0;
    band_stats(rq.rowpass, bt, row0, row1, 1, ms, (unsigned)ncol, 0);
    return GLF_OK;
}
