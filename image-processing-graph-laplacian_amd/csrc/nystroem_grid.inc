// nystroem_grid.inc -- the Nystroem contraction refactored for a sample set that is a full tensor grid
// (what hpc/sampling.c:6-23 always produces): samples s = (a, b), a < nr grid rows R_a, b < nc grid columns C_b.
// Included by nystroem.hip inside namespace glf.
//
//   Phi[px][n] = sum_s K(px, s) Psi[s][n],     K = Er(r - R_a) * Ec(c - C_b) * P(|v - v_ab|)     (px = (r, c), value v)
//              = sum_b Ec(c - C_b) * T[r][v][b][n],
//   T[r][v][b][n] = sum_a P(|v - v_ab|) * Er(r - R_a) * Psi[(a, b)][n].
//
// The same sum in another order -- nothing is truncated or approximated -- but T depends on the pixel only
// through its image row and its u8 value, so the p-term inner sum is shared by every pixel of a row that has the
// same value: 2 H 256 nc nr m flops (1.1e13 at cfg4) instead of 2 N p m (1.8e14), plus 2 N nc m for the outer sum.
//
//   row pass  (k_grid_rowpass_rt for the Nystroem passes: see "row-tile form" below; k_grid_rowpass for the L_A sweeps):
//             k_grid_rowpass: for a sample column b and a block of 64 values v, the GEMM
//             T[r][v][b][:] = Pm_b[v][a] * (Er_r[a] Psi_b[a][:]) on the f16 matrix pipe with the split-f16 scheme of
//             k_nystroem_f16s (both operands hi + lo, three v_mfma_f32_32x32x16_f16, f32 accumulate). Pm_b (256 x nr,
//             independent of r) is prepared once as MFMA A fragments and stays in LDS together with Psi_b; a wave
//             takes one image row at a time, scales Psi_b by Er_r in registers straight into the B-fragment layout.
//   col pass  (k_grid_colpass): one workgroup per image row; pixels are grouped by value (k_grid_rowsort: a stable
//             counting sort of the row); per chunk of up to 32 pixels of a group the small GEMM [pixels x nc] x [nc x m]
//             runs on the matrix pipe too (Ec fragments from a table, T[r][v] streamed once and split in registers);
//             writes Phi rows and the Phi^T y partial sums like the direct kernel's epilogue.
// T is the only large intermediate (256 nc m 4 B per image row: 19 MB at cfg4); it is produced and consumed in
// passes over blocks of image rows sized to GRID_T_BYTES of HBM.
// Exact-zero skipping: Er_r[a] = +0 beyond the f32 underflow radius makes whole 16-sample-row k-steps of the row
// pass exactly zero, and Ec = +0 bounds the sample columns a pixel chunk needs; both are skipped without changing
// a bit of the result.

constexpr int GRID_MT = 2;                    // MFMA m-tiles (32 values each) per row-pass workgroup (4 spills: 46 vs 37 ms)
constexpr int GRID_NW = 16;                   // waves per row-pass workgroup (four per SIMD at 127 VGPRs; 12 measured 2-5 % slower)
constexpr int GRID_KS_BLDS = 19;              // k-steps (16 grid rows each) up to which A and Psi_b slices both fit the LDS: nr <= 304
constexpr int ER_PIECE = 64;                  // floats of an Er row per LDS-DMA piece of the dense v1 row pass (4 k-steps)
constexpr int GRID_MAX_KS = 38;               // beyond, up to nr <= 608, Psi_b is read from global memory (L2) instead
constexpr size_t GRID_T_BYTES = 16ull << 30;  // HBM for T per pass
constexpr int GRID_RT_MT = 2, GRID_RT_NW = 8; // m-tiles per wave and group, waves per workgroup of the row-tile row pass
constexpr int GRID_RT_TCAP = 3;               // x GRID_T_BYTES of HBM for T in the row-tile form

// ---- operand preparation ---------------------------------------------------------------------------

// A fragments of Pm_b[v][a] = 2^15 P(|v - v_ab|): [b][m-tile (8)][k-step][hi, lo][lane][8 halves]; lane l holds
// row v = 32 mt + l % 32, k = 16 kstep + 8 (l / 32) + j.
__global__ __launch_bounds__(256) void k_grid_afrag(const float *__restrict__ ptab, const float4 *__restrict__ samples, int nr,
                                                     int nc, int ks, _Float16 *__restrict__ Af)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nc * 8 * ks * 64) return;
    const int lane = (int)(e % 64), kstep = (int)((e / 64) % ks), mt = (int)((e / 64 / ks) % 8), b = (int)(e / 64 / ks / 8);
    const int v = mt * 32 + (lane & 31);
    f16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int a = kstep * 16 + 8 * (lane >> 5) + j;
        float val = 0.f;
        if (a < nr) {
            const int sv = (int)samples[(size_t)a * nc + b].z;
            val = 32768.f * ptab[abs(v - sv)];
        }
        const _Float16 h = (_Float16)val;
        hi[j] = h;
        lo[j] = (_Float16)(val - (float)h);
    }
    f16x8 *out = reinterpret_cast<f16x8 *>(Af);
    const size_t frag = (((size_t)b * 8 + mt) * ks + kstep) * 2;
    out[(frag + 0) * 64 + lane] = hi;
    out[(frag + 1) * 64 + lane] = lo;
}

// Psi_b[a][n] * colscale[n] in the order the row pass reads it: [b][k-step][n-tile][h][q][n % 32][4 floats],
// a = 16 kstep + 8 h + 4 q + (0..3): a lane's 8 k values are two conflict-free 16-B reads.
__global__ __launch_bounds__(256) void k_grid_bprep(const float *__restrict__ psi, unsigned ld, const float *__restrict__ colscale,
                                                     int nr, int nc, int ks, int nt_count, float *__restrict__ Bp)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; // one float4
    if (e >= (size_t)nc * ks * nt_count * 2 * 2 * 32) return;
    const int n = (int)(e % 32), q = (int)((e / 32) % 2), h = (int)((e / 64) % 2), nt = (int)((e / 128) % nt_count);
    const int kstep = (int)((e / 128 / nt_count) % ks), b = (int)(e / 128 / nt_count / ks);
    const int col = nt * 32 + n;
    const float sc = colscale[col];
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int a = kstep * 16 + 8 * h + 4 * q + u;
        v[u] = a < nr ? psi[((size_t)a * nc + b) * ld + col] * sc : 0.f;
    }
    reinterpret_cast<float4 *>(Bp)[e] = make_float4(v[0], v[1], v[2], v[3]);
}

// one ER_PIECE-float piece of an Er row -> LDS at a wave-uniform byte offset (4 bytes per lane; lanes beyond the row stay out)
__device__ __forceinline__ void lds_dma_er(const float *row, int piece, int kp, unsigned lds_byte_offset, int lane)
{
    const int i = piece * ER_PIECE + lane;
    if (i < kp)
        asm volatile("s_mov_b32 m0, %1\n\t"
                     "s_nop 0\n\t"
                     "global_load_lds_dword %0, off"
                     :
                     : "v"(row + i), "s"(lds_byte_offset)
                     : "memory");
}

// ---- row pass ------------------------------------------------------------------------------------------
// grid (nc, 8 / MT, splits); GRID_NW = 16 waves (four per SIMD: the operand slices fill the LDS, so the extra waves
// have to come from the same workgroup; 127 VGPRs allow four); wave w takes the rows w, w + GRID_NW, ... of its split.
// MT = m-tiles (32 values each) per workgroup; BLDS: the Psi_b slice sits in LDS beside the A slice (nr <= 304 at MT = 2),
// else it is read from global memory (L2) and the A slice alone fills the LDS.
// OP only tags the instantiation (false: Nystroem passes over image rows, true: L_A sweeps over grid rows) so that
// profilers list the two uses of the kernel separately.
template <int NT, bool SKIP, int MT, bool BLDS, bool OP>
__global__ __launch_bounds__(GRID_NW * 64) void k_grid_rowpass(const _Float16 *__restrict__ Af, const float *__restrict__ Bp,
                                                                const float *__restrict__ ermat,
                                                                const unsigned long long *__restrict__ active_ks, int nc, int ks,
                                                                int row_off, int nrows_pass, int rows_per_wg,
                                                                const unsigned *__restrict__ pmask, float *__restrict__ T)
{
    extern __shared__ __attribute__((aligned(16))) float4 dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.x, vq = blockIdx.y;
    // LDS: A slice [MT m-tiles][ks][2][64] x 16 B, and for MT = 2 the B slice [ks][NT][2][2][32] x 16 B
    f16x8 *As = reinterpret_cast<f16x8 *>(dyn);
    lds_dma_copy<GRID_NW>(reinterpret_cast<const float4 *>(Af) + ((size_t)b * 8 + MT * vq) * ks * 128, As, ks * 2 * MT, wave, lane);
    const float4 *Bs = reinterpret_cast<const float4 *>(Bp) + (size_t)b * ks * NT * 128;
    if (BLDS) {
        float4 *Bl = dyn + MT * ks * 2 * 64;
        lds_dma_copy<GRID_NW>(Bs, Bl, ks * NT * 2, wave, lane);
        Bs = Bl;
    }
    // Er of the dense sweep goes through a per-wave ring of two 256-byte pieces (4 k-steps each) behind the slices,
    // one LDS-DMA instruction per piece: as two 16-byte global loads per lane and k-step the same 32 bytes cost a
    // quarter of the kernel (the vector-memory path returns 2 KiB per wave and k-step for 64 distinct bytes).
    constexpr bool ERL = BLDS && !SKIP;
    const float *er_ring = reinterpret_cast<const float *>(dyn + MT * ks * 2 * 64 + ks * NT * 2 * 64) + wave * (2 * ER_PIECE);
    const unsigned er_ring_lds = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_offset_of(er_ring));
    lds_dma_drain();
    __syncthreads();

    const int kp = ks * 16;
    const int r_end = min((int)(blockIdx.z + 1) * rows_per_wg, nrows_pass);
    const int r_first = blockIdx.z * rows_per_wg + wave;
    const int npieces = (kp + ER_PIECE - 1) / ER_PIECE;
    unsigned piece_no = 0; // pieces consumed by this wave so far: piece i of the stream lives in ring slot i & 1
    if (ERL && r_first < r_end) lds_dma_er(ermat + (size_t)(row_off + r_first) * kp, 0, kp, er_ring_lds, lane);
    for (int rl = r_first; rl < r_end; rl += GRID_NW) {
        // Er_r over the grid rows: this lane's 8 k values of a step are 32 contiguous bytes of the row's table
        const float *er_row = ermat + (size_t)(row_off + rl) * kp + 8 * half;
        const unsigned long long active = SKIP ? active_ks[row_off + rl] : 0ull;
        // The values of this block of 64 that occur in the row, packed: position j holds the j-th present value (the absent
        // ones fill up from the top), so that a row with at most 32 of them needs one m-tile, not two (73 % of the tiles at
        // cfg4's L_A sweeps, where a grid row's 292 samples carry ~125 distinct values). A lane knows the rank of ITS value
        // among the present ones from the row's presence words (mbcnt), sends its value to the lane of that position
        // (ds_permute), and the MFMA A fragment of position l31 of tile mt is then the fragment of the value found there.
        static_assert(MT == 2, "the value positions of a workgroup are the 64 lanes of a wave");
        const unsigned pm_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)pmask[(size_t)(row_off + rl) * 8 + vq * MT + 0]);
        const unsigned pm_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)pmask[(size_t)(row_off + rl) * 8 + vq * MT + 1]);
        const int npresent = __builtin_popcount(pm_lo) + __builtin_popcount(pm_hi);
        const int mt_n = (npresent + 31) >> 5; // m-tiles holding a present value (wave-uniform)
        int perm;                              // the value (0..63 within the block) at position `lane`
        {
            const unsigned rank = __builtin_amdgcn_mbcnt_hi(pm_hi, __builtin_amdgcn_mbcnt_lo(pm_lo, 0u)); // present values below this lane's
            const bool mine = ((lane < 32 ? pm_lo : pm_hi) >> (lane & 31)) & 1u;
            const unsigned dst = mine ? rank : 63u - ((unsigned)lane - rank);
            perm = __builtin_amdgcn_ds_permute((int)(dst * 4u), lane);
        }
        int a_idx[MT]; // As index of this lane's A fragment of k-step 0, hi, per tile
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int pv = __builtin_amdgcn_ds_bpermute((mt * 32 + l31) * 4, perm);
            a_idx[mt] = (pv >> 5) * ks * 2 * 64 + 32 * half + (pv & 31);
        }
        f32x16 acc[MT][NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;
        // dense sweep: Er of the next k-step is fetched (L2) while this one is contracted
        float4 en0, en1;
        if (!ERL) {
            en0 = *reinterpret_cast<const float4 *>(er_row);
            en1 = *reinterpret_cast<const float4 *>(er_row + 4);
        }
        for (int kstep = 0; kstep < ks; ++kstep) {
            if (SKIP && !((active >> kstep) & 1ull)) continue; // every B entry of the step is exactly +0
            float4 e0, e1;
            if (ERL) {
                constexpr int SPP = ER_PIECE / 16; // k-steps per piece
                if (kstep % SPP == 0) {
                    // the piece of this k-step has landed (the wave's only other vector-memory traffic is the T stores of
                    // the row before; leaving those in flight with a counted wait measured no faster); the other slot was
                    // last read a piece ago: refill it with the piece after this one, which at the end of a row is the
                    // first of the wave's next row
                    lds_dma_drain();
                    const int pc = kstep / SPP + 1;
                    const unsigned slot = ((piece_no + 1) & 1u) * (ER_PIECE * 4);
                    if (pc < npieces)
                        lds_dma_er(ermat + (size_t)(row_off + rl) * kp, pc, kp, er_ring_lds + slot, lane);
                    else if (rl + GRID_NW < r_end)
                        lds_dma_er(ermat + (size_t)(row_off + rl + GRID_NW) * kp, 0, kp, er_ring_lds + slot, lane);
                }
                const float *ep = er_ring + (piece_no & 1u) * ER_PIECE + (kstep % SPP) * 16 + 8 * half;
                e0 = *reinterpret_cast<const float4 *>(ep);
                e1 = *reinterpret_cast<const float4 *>(ep + 4);
                if (kstep % SPP == SPP - 1 || kstep == ks - 1) ++piece_no;
            } else if (SKIP) {
                e0 = *reinterpret_cast<const float4 *>(er_row + kstep * 16);
                e1 = *reinterpret_cast<const float4 *>(er_row + kstep * 16 + 4);
            } else {
                e0 = en0;
                e1 = en1;
                if (kstep + 1 < ks) {
                    en0 = *reinterpret_cast<const float4 *>(er_row + (kstep + 1) * 16);
                    en1 = *reinterpret_cast<const float4 *>(er_row + (kstep + 1) * 16 + 4);
                }
            }
            f16x8 bh[NT], bl[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float4 p0 = Bs[(((kstep * NT + nt) * 2 + half) * 2 + 0) * 32 + l31];
                const float4 p1 = Bs[(((kstep * NT + nt) * 2 + half) * 2 + 1) * 32 + l31];
                const float y[8] = {e0.x * p0.x, e0.y * p0.y, e0.z * p0.z, e0.w * p0.w,
                                    e1.x * p1.x, e1.y * p1.y, e1.z * p1.z, e1.w * p1.w};
                // (scalar multiplies: the packed v_pk_mul_f32 form of these, and v_fma_mixlo/hi_f16 writing the f16 halves
                // directly, both measured slower beside the MFMAs -- tools/valu_probe.hip has the issue costs)
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    f32x2 yy;
                    yy[0] = y[j];
                    yy[1] = y[j + 1];
                    const f16x2 h2 = __builtin_convertvector(yy, f16x2);
                    f32x2 res;
                    res[0] = yy[0] - (float)h2[0]; // exact in f32
                    res[1] = yy[1] - (float)h2[1];
                    const f16x2 l2 = __builtin_convertvector(res, f16x2);
                    bh[nt][j] = h2[0];
                    bh[nt][j + 1] = h2[1];
                    bl[nt][j] = l2[0];
                    bl[nt][j + 1] = l2[1];
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if (mt >= mt_n) break;
                const f16x8 ah = As[a_idx[mt] + (kstep * 2 + 0) * 64];
                const f16x8 al = As[a_idx[mt] + (kstep * 2 + 1) * 64];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[nt], acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[nt], acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[nt], acc[mt][nt], 0, 0, 0);
                }
            }
        }
        // T[rl][v][b][n] as accumulated (the column pass takes the operand scales out), each row of a tile at the value its
        // position holds. Positions beyond the present values are not written (the column pass never reads those rows): their
        // lanes store beyond the range of the row's buffer descriptor, which the hardware drops -- no branches, and no wait
        // between the stores (under `if (present)` every global store waited for the one before).
        const float *Trow = T + (((size_t)rl * 256 + (size_t)vq * MT * 32) * nc + b) * (32 * NT);
        const uintptr_t tb = (uintptr_t)Trow;
        const uintptr_t tbu = ((uintptr_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(tb >> 32)) << 32) |
                              (uintptr_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)tb);
        const unsigned vstride = (unsigned)nc * (32 * NT) * (unsigned)sizeof(float); // bytes between consecutive values
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)tbu, 0, (int)(MT * 32 * vstride), 0x00020000);
        const unsigned lane_off = (unsigned)l31 * (unsigned)sizeof(float);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (mt >= mt_n) break;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int pos = mt * 32 + (i & 3) + 8 * (i >> 2); // of half 0; half 1 holds the position 4 further
                const int v0 = __builtin_amdgcn_readlane(perm, pos), v1 = __builtin_amdgcn_readlane(perm, pos + 4);
                const unsigned val = (unsigned)(half ? v1 : v0);
                const unsigned off = pos + 4 * half < npresent ? lane_off + val * vstride : 0x80000000u;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[mt][nt][i]), rsrc, (int)off + 128 * nt, 0,
                                                              0);
            }
        }
    }
}

// ---- row pass, row-tile form -------------------------------------------------------------------------
// The same GEMM with the roles of the operands exchanged: for a sample column b and a value v,
//   T[r][v][b][:] = sum_a Er(r - R_a) * (P(|v - v_ab|) Psi_b[a][:]),
// M = target rows, K = grid rows, N = m. The A operand (2^15 Er, split hi + lo) does not depend on (b, v): it is a
// table of MFMA fragments per 32-row m-tile built once (k_grid_erfrag, a few MB, L2 resident). The B operand of a
// (b, v) pair is scaled and split ONCE per workgroup into LDS and then serves every row tile of the pass, so the
// VALU work per MFMA is ~64x smaller than in k_grid_rowpass (which re-splits Er_r Psi_b for every image row and block of
// 64 values). A workgroup holds VT values of one sample column; wave w takes the groups of MT m-tiles w, w + NW, ...
// and multiplies each A fragment with the VT x NT B fragments.
//
// A fragments: [m-tile][k-step][hi, lo][lane][8 halves]; lane l holds target row 32 mtile + l % 32 and
// k = 16 kstep + 8 (l / 32) + j; tact[mtile] = bit mask of the k-steps that hold a non-zero.
__global__ __launch_bounds__(64) void k_grid_erfrag(const float *__restrict__ etab, const int *__restrict__ grow, int nr, int ks,
                                                     int row0, int nrows, const int *__restrict__ rowlist,
                                                     _Float16 *__restrict__ Erf, unsigned long long *__restrict__ tact)
{
    const int mtile = blockIdx.x, lane = threadIdx.x, rl = 32 * mtile + (lane & 31), half = lane >> 5;
    const bool valid = rl < nrows;
    const int r = valid ? (rowlist ? rowlist[rl] : row0 + rl) : 0;
    f16x8 *out = reinterpret_cast<f16x8 *>(Erf);
    unsigned long long act = 0;
    for (int kstep = 0; kstep < ks; ++kstep) {
        f16x8 hi, lo;
        bool nz = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int a = kstep * 16 + 8 * half + j;
            const float val = (valid && a < nr) ? 32768.f * etab[abs(r - grow[a])] : 0.f;
            const _Float16 h = (_Float16)val;
            hi[j] = h;
            lo[j] = (_Float16)(val - (float)h);
            nz |= val != 0.f;
        }
        out[(((size_t)mtile * ks + kstep) * 2 + 0) * 64 + lane] = hi;
        out[(((size_t)mtile * ks + kstep) * 2 + 1) * 64 + lane] = lo;
        if (__ballot(nz)) act |= 1ull << kstep;
    }
    if (lane == 0) tact[mtile] = act;
}

// presence masks by (m-tile, value): bit j of pmT[mtile][v] = row 32 mtile + j of the shard holds a pixel of value v
__global__ __launch_bounds__(256) void k_grid_pmask_t(const unsigned *__restrict__ pmask, int nrows, int ntiles,
                                                       unsigned *__restrict__ pmT)
{
    const int mtile = blockIdx.x, v = threadIdx.x;
    if (mtile >= ntiles) return;
    unsigned word = 0;
    for (int j = 0; j < 32; ++j) {
        const int rl = 32 * mtile + j;
        if (rl < nrows && ((pmask[(size_t)rl * 8 + (v >> 5)] >> (v & 31)) & 1u)) word |= 1u << j;
    }
    pmT[(size_t)mtile * 256 + v] = word;
}

// svalT[b][a] = value of sample (a, b): what a row-pass workgroup (one grid column b) reads to build P(|v - v_ab|)
__global__ __launch_bounds__(256) void k_grid_svalt(const float4 *__restrict__ samples, int nr, int nc, int kp, uint8_t *__restrict__ svalT)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nc * kp) return;
    const int b = e / kp, a = e - b * kp;
    svalT[e] = a < nr ? (uint8_t)samples[(size_t)a * nc + b].z : (uint8_t)0;
}

__device__ __forceinline__ void split_f16x8(const float (&y)[8], f16x8 &hi, f16x8 &lo)
{
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        f32x2 yy;
        yy[0] = y[j];
        yy[1] = y[j + 1];
        const f16x2 h2 = __builtin_convertvector(yy, f16x2);
        f32x2 res;
        res[0] = yy[0] - (float)h2[0]; // exact in f32
        res[1] = yy[1] - (float)h2[1];
        const f16x2 l2 = __builtin_convertvector(res, f16x2);
        hi[j] = h2[0];
        hi[j + 1] = h2[1];
        lo[j] = l2[0];
        lo[j + 1] = l2[1];
    }
}

// grid (nc, 256 / VT, splits of the m-tile groups); NW waves.
// tile0 = first m-tile of the pass in the fragment table, ntiles = m-tiles of the pass; T rows are pass-relative.
// RANK: the "rank" form (nystroem_rank.inc): the workgroup's VT "values" are VT terms k of the low-rank expansion
// P(|v - w|) ~= sum_k f_k(v) f_k(w) of the photometric table; ptab then holds f_k(w) as [k][256], the output is
// S[r][n-tile][b][k][32] = sum_a Er(r - R_a) f_k(v_ab) Psi[(a, b)][n] (every row is stored: nothing depends on the image),
// and blockIdx.y counts blocks of VT terms (gridDim.y = R / VT).
template <int NT, bool SKIP, int VT, int MT, int NW, bool OP, bool RANK = false>
__global__ __launch_bounds__(NW * 64) void k_grid_rowpass_rt(const _Float16 *__restrict__ Erf,
                                                              const unsigned long long *__restrict__ tact,
                                                              const float *__restrict__ Bp, const float *__restrict__ ptab,
                                                              const uint8_t *__restrict__ svalT, int nr, int nc, int ks, int tile0,
                                                              int ntiles, int groups_per_wg,
                                                              const unsigned *__restrict__ pmT, float *__restrict__ T,
                                                              int rank_r, int rank_ncs, const float *__restrict__ rank_scale)
{
    constexpr int LDN = 32 * NT;
    extern __shared__ __attribute__((aligned(16))) float4 dyn[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), half = lane >> 5, l31 = lane & 31;
    // RANK: blockIdx.y = n-tile * (R / VT) + block of VT terms; one n-tile of 32 columns per workgroup (NT = 1), its own Bp
    static_assert(!RANK || (VT == 4 && NT == 1), "rank form: four terms of one n-tile per workgroup (16-byte stores of S)");
    const int rank_kq = RANK ? rank_r / VT : 1, rank_nt = RANK ? (int)blockIdx.y / rank_kq : 0, rank_ntt = RANK ? (int)gridDim.y / rank_kq : 1;
    const int b = blockIdx.x, v0 = (RANK ? (int)blockIdx.y % rank_kq : (int)blockIdx.y) * VT, kp = ks * 16;
    if (RANK) Bp += (size_t)rank_nt * nc * ks * NT * 512;
    // LDS: B fragments [VT][ks][NT][hi, lo][64 lanes] x 16 B, then P(|v - v_ab|) over the grid rows [VT][kp]
    f16x8 *Bl = reinterpret_cast<f16x8 *>(dyn);
    float *Pv = reinterpret_cast<float *>(dyn + (size_t)VT * ks * NT * 2 * 64);
    for (int a = threadIdx.x; a < kp; a += NW * 64) { // one contiguous read of the column's sample values, VT table reads
        const int sv = svalT[(size_t)b * kp + a];
#pragma unroll
        for (int vi = 0; vi < VT; ++vi)
            Pv[vi * kp + a] = a < nr ? (RANK ? ptab[(v0 + vi) * 256 + sv] : ptab[abs(v0 + vi - sv)]) : 0.f;
    }
    __syncthreads();
    {
        const float4 *Bs = reinterpret_cast<const float4 *>(Bp) + (size_t)b * ks * NT * 128;
        const int units = ks * NT; // (k-step, n-tile) pieces of Psi_b, each read once and scaled for the VT values
        constexpr int UPW = 5; // units of a wave per round: all 38 of ks = 19, NT = 2 in one round of loads
        for (int u0 = wave; u0 < units; u0 += UPW * NW) {
            float4 p0[UPW], p1[UPW];
#pragma unroll
            for (int q = 0; q < UPW; ++q) {
                const int u = min(u0 + q * NW, units - 1);
                p0[q] = Bs[((u * 2 + half) * 2 + 0) * 32 + l31];
                p1[q] = Bs[((u * 2 + half) * 2 + 1) * 32 + l31];
            }
#pragma unroll
            for (int q = 0; q < UPW; ++q) {
                const int u = u0 + q * NW;
                if (u >= units) break;
                const int kstep = u / NT, nt = u - kstep * NT;
#pragma unroll
                for (int vi = 0; vi < VT; ++vi) {
                    const float4 f0 = *reinterpret_cast<const float4 *>(Pv + vi * kp + kstep * 16 + 8 * half);
                    const float4 f1 = *reinterpret_cast<const float4 *>(Pv + vi * kp + kstep * 16 + 8 * half + 4);
                    const float y[8] = {f0.x * p0[q].x, f0.y * p0[q].y, f0.z * p0[q].z, f0.w * p0[q].w,
                                        f1.x * p1[q].x, f1.y * p1[q].y, f1.z * p1[q].z, f1.w * p1[q].w};
                    f16x8 hi, lo;
                    split_f16x8(y, hi, lo);
                    Bl[(((vi * ks + kstep) * NT + nt) * 2 + 0) * 64 + lane] = hi;
                    Bl[(((vi * ks + kstep) * NT + nt) * 2 + 1) * 64 + lane] = lo;
                }
            }
        }
    }
    __syncthreads();

    const f16x8 *Ef = reinterpret_cast<const f16x8 *>(Erf);
    const int ngroups = (ntiles + MT - 1) / MT;
    const int g_end = min((int)(blockIdx.z + 1) * groups_per_wg, ngroups);
    // floats between consecutive rows of T (RANK: of S[r][n-tile][b (rank_ncs slots)][k / 4][32 columns][4 terms])
    const size_t rowstride = RANK ? (size_t)rank_ntt * rank_ncs * rank_r * 32 : (size_t)256 * nc * LDN;
    // One flat loop over the (group, k-step) pairs of this wave. The fragments of the next pair (A from L2, B from LDS) are
    // fetched while the current pair is contracted, across group boundaries too; the epilogue of a group sits inside the
    // loop, so the loop has a single back edge and the compiler's wait counts stay exact (with a separate loop per group it
    // merged the entry state into the steady state and waited for the loads it had just issued).
    auto group_mask = [&](int g) -> unsigned long long {
        if (g >= g_end) return 0ull;
        if (!SKIP) return (1ull << ks) - 1ull;
        unsigned long long m = 0;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            if (g * MT + mt < ntiles) m |= tact[tile0 + g * MT + mt];
        m = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(m >> 32)) << 32) |
            (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)m); // (the builtin returns int)
        return m ? m : 1ull; // a group without a non-zero Er still owes its rows of zeros: one (all-zero) k-step
    };
    int gC = blockIdx.z * groups_per_wg + wave, gF = gC;
    unsigned long long maskC = group_mask(gC), maskF = maskC;
    f16x8 A0[MT][2], A1[MT][2], B0[VT][NT][2], B1[VT][NT][2];
    if (gC >= g_end) return; // (no barrier below)
    const int g_first = gC;
    // Every call issues the same loads whether or not a pair is left to fetch (past the end it re-reads the wave's first
    // fragments): with conditional loads the compiler's wait counts have to cover the path without them and end up waiting
    // for the loads just issued.
    auto fetch_a = [&](f16x8(&dst)[MT][2]) {
        const bool valid = gF < g_end;
        const int g = valid ? gF : g_first, kstep = valid ? __builtin_ctzll(maskF) : 0;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            dst[mt][0] = Ef[(((size_t)(tile0 + g * MT + mt) * ks + kstep) * 2 + 0) * 64 + lane];
            dst[mt][1] = Ef[(((size_t)(tile0 + g * MT + mt) * ks + kstep) * 2 + 1) * 64 + lane];
        }
        if (valid) {
            maskF &= maskF - 1ull;
            if (!maskF) {
                gF += NW;
                maskF = group_mask(gF);
            }
        }
    };
    auto fetch_b = [&](f16x8(&dst)[VT][NT][2], int kstep) {
#pragma unroll
        for (int vi = 0; vi < VT; ++vi)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                dst[vi][nt][0] = Bl[(((vi * ks + kstep) * NT + nt) * 2 + 0) * 64 + lane];
                dst[vi][nt][1] = Bl[(((vi * ks + kstep) * NT + nt) * 2 + 1) * 64 + lane];
            }
    };
    fetch_a(A0);
    fetch_b(B0, __builtin_ctzll(maskC));
    // RANK: S leaves the row pass ready for the T' GEMM of the column pass -- scaled by the power of two that brings the
    // column below 2^14 and split into its f16 (hi, lo) pair, packed in one dword: every workgroup of the column pass that
    // reads the element (one per segment of the row: ~9 at cfg4) then assembles its B fragments with one v_perm per element
    // instead of re-doing the scaling and the split (7 vector instructions per element: the column pass was VALU-bound).
    float rsc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) rsc[nt] = RANK ? rank_scale[32 * (rank_nt + nt) + l31] * (1.0f / 128.f) : 1.f; // (RANK_S_SCALE)
    // bytes of T one (m-tile, value) block of a wave spans: the buffer descriptor's range (masked lanes store out of range)
    const unsigned blk_bytes = (unsigned)((size_t)32 * rowstride * sizeof(float));
    f32x16 acc[MT][VT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int vi = 0; vi < VT; ++vi)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][vi][nt][i] = 0.f;
    // one (group, k-step) pair: contracts the fragments in (a, bf) and fetches those of the next pair into (af, bn), the
    // buffers the previous step used; returns false after the wave's last pair
    auto step = [&](const f16x8(&a)[MT][2], f16x8(&af)[MT][2], const f16x8(&bf)[VT][NT][2], f16x8(&bn)[VT][NT][2])
                    __attribute__((always_inline)) -> bool {
        maskC &= maskC - 1ull;
        fetch_a(af);
        {
            const unsigned long long mnext = maskC ? maskC : group_mask(gC + NW);
            fetch_b(bn, mnext ? __builtin_ctzll(mnext) : 0);
        }
        // three split products; consecutive MFMAs go to different accumulators
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int vi = 0; vi < VT; ++vi)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][vi][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mt][s == 2 ? 1 : 0], bf[vi][nt][s == 1 ? 1 : 0],
                                                                                 acc[mt][vi][nt], 0, 0, 0);
        if (maskC) return true;
        // Last k-step of the group: T[row][v][b][n] as accumulated (the column pass takes the operand scales out). (row, value) pairs that do
        // not occur in the image are never read by the column pass and are not written: their lanes store beyond the range
        // of the block's buffer descriptor, which the hardware drops (no branches). Register i of a lane is row
        // (i & 3) + 8 (i >> 2) + 4 half of the m-tile.
        const int t_rel = gC * MT, t_abs = tile0 + t_rel; // the fragment table is padded to whole groups
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (RANK && t_rel + mt < ntiles) {
                // S[row][n-tile][b][k / 4][n][4 terms]: the lane's four terms of (row, n) are one 16-byte store, the 32 lanes of a
                // half 512 contiguous bytes; every element scaled and split (see rsc)
                const float *Sblk = T + (size_t)(t_rel + mt) * 32 * rowstride + (size_t)rank_nt * rank_ncs * rank_r * 32 +
                                    ((size_t)b * rank_kq + (v0 / VT)) * 128;
                const uintptr_t tb = (uintptr_t)Sblk;
                const uintptr_t tbu = ((uintptr_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(tb >> 32)) << 32) |
                                      (uintptr_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)tb);
                const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)tbu, 0, (int)blk_bytes, 0x00020000);
                const unsigned lane_off = (unsigned)(((size_t)(4 * half) * rowstride + 4 * l31) * sizeof(float));
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int rit = (i & 3) + 8 * (i >> 2);
                    u32x4 w4;
#pragma unroll
                    for (int vi = 0; vi < VT; ++vi) {
                        const float x = acc[mt][vi][0][i] * rsc[0];
                        const _Float16 xh = (_Float16)x;
                        const _Float16 xl = (_Float16)(x - (float)xh);
                        w4[vi] = (unsigned)__builtin_bit_cast(unsigned short, xh) | ((unsigned)__builtin_bit_cast(unsigned short, xl) << 16);
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(w4, rsrc, (int)(lane_off + (unsigned)((size_t)rit * rowstride * sizeof(float))), 0, 0);
                }
            } else if (t_rel + mt < ntiles) {
#pragma unroll
                for (int vi = 0; vi < VT; ++vi) {
                    const unsigned present = pmT[(size_t)(t_abs + mt) * 256 + v0 + vi] >> (4 * half);
                    const float *Tblk = T + ((size_t)(t_rel + mt) * 32 * 256 + (size_t)(v0 + vi)) * nc * LDN + (size_t)b * LDN;
                    const uintptr_t tb = (uintptr_t)Tblk;
                    const uintptr_t tbu = ((uintptr_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(tb >> 32)) << 32) |
                                          (uintptr_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)tb);
                    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)tbu, 0, (int)blk_bytes, 0x00020000);
                    const unsigned lane_off = (unsigned)(((size_t)(4 * half) * rowstride + l31) * sizeof(float));
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int rit = (i & 3) + 8 * (i >> 2);
                        const unsigned off =
                            ((present >> rit) & 1u) ? lane_off + (unsigned)((size_t)rit * rowstride * sizeof(float)) : 0x80000000u;
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[mt][vi][nt][i]), rsrc, (int)off + 128 * nt, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int vi = 0; vi < VT; ++vi)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[mt][vi][nt][i] = 0.f;
        }
        gC += NW;
        maskC = group_mask(gC);
        return gC < g_end;
    };
    while (true) { // two sets of fragment buffers, exchanged by unrolling (register copies would have to wait for the loads)
        if (!step(A0, A1, B0, B1)) break;
        if (!step(A1, A0, B1, B0)) break;
    }
}

// ---- column pass ---------------------------------------------------------------------------------------
// Phi[px][n] = sum_b Ec(c_px - C_b) T[r][v][b][n] for the pixels of one (image row, value) group: a small GEMM
// [pixels x nc] x [nc x m] per group, again on the f16 matrix pipe with split operands. A = 2^15 Ec comes ready-split
// from a per-column fragment table (k_grid_ecfrag; no VALU), B = T[r][v] is streamed from HBM exactly once per
// chunk of up to 32 pixels (lane = column n, 8 sample columns per lane and k-step) and split in registers after an
// exact power-of-two scaling (|T[..][n]| <= nr max|Psi[:, n]|, so the scale is known beforehand).
// One workgroup (4 waves) per image row; the row's chunks are dealt round-robin to the waves.
constexpr int GRID_PCT = 32; // pixels per chunk = one MFMA m-tile
constexpr int GRID_T_PAD = 16; // sample columns of padding behind T: the last k-step of the column pass reads past nc
constexpr int GRID_COLPASS_SPLIT = 2;    // workgroups per image row (Nystroem: ~840 rows per pass)
constexpr int GRID_COLPASS_SPLIT_OP = 16; // workgroups per grid row (L_A sweep: only nr rows)

// A fragments of 2^15 Ec(c - C_b): [c][k-step][hi, lo][h][8 halves], b = 16 kstep + 8 h + j (0 beyond nc)
// Table rows: the pixel columns 0 .. ncols-1, or (collist) the listed columns (the grid columns for the L_A operator).
__global__ __launch_bounds__(256) void k_grid_ecfrag(const float *__restrict__ etab, const int *__restrict__ gcol, int ncols,
                                                      const int *__restrict__ collist, int nc, int ksc,
                                                      _Float16 *__restrict__ ecf)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; // one (table row, kstep, h)
    if (e >= (size_t)ncols * ksc * 2) return;
    const int h = (int)(e % 2), kstep = (int)((e / 2) % ksc), ci = (int)(e / 2 / ksc);
    const int c = collist ? collist[ci] : ci;
    f16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = kstep * 16 + 8 * h + j;
        const float val = b < nc ? 32768.f * etab[abs(c - gcol[b])] : 0.f;
        const _Float16 x = (_Float16)val;
        hi[j] = x;
        lo[j] = (_Float16)(val - (float)x);
    }
    f16x8 *out = reinterpret_cast<f16x8 *>(ecf);
    out[(((size_t)ci * ksc + kstep) * 2 + 0) * 2 + h] = hi;
    out[(((size_t)ci * ksc + kstep) * 2 + 1) * 2 + h] = lo;
}

// The same fragments for a UNIFORM sample grid (C_b = C_0 + dist b, what hpc/sampling.c:15-21 produces) from a table
// 20x smaller: with c - C_0 = dist Q + r (0 <= r < dist), Ec(c - C_b) = E(|dist (Q - b) + r|) depends on (r, Q - b)
// only, so the 8 entries b = 16 kstep + 8 h + j of a fragment are 8 consecutive entries G_r[s + j], s = 16 kstep + 8 h - Q,
// G_r[i] = 2^15 E(|r - dist i|). ecr[r][phase][e / 8][hi, lo][e % 8] = G_r[e + phase - off] holds every 16-byte alignment of every
// window (8 phases): 0.3 MB at cfg4 against the 5 MB of the per-column table, which did not survive in L2 next to the
// T stream (the column pass fetched 1.56 bytes per byte of T). Entries for b >= nc are not zero here; their T is.
__global__ __launch_bounds__(256) void k_grid_ecr(const float *__restrict__ etab, int maxdim, int dist, int len, int off,
                                                   _Float16 *__restrict__ ecr)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)dist * 8 * len) return;
    const int i = (int)(e % len), ph = (int)((e / len) % 8), r = (int)(e / len / 8);
    const int d = abs(r - dist * (i + ph - off));
    const float val = d < maxdim ? 32768.f * etab[d] : 0.f;
    const _Float16 x = (_Float16)val;
    // hi and lo windows of 8 entries side by side: the two half-waves of a pixel read one 64-byte block per k-step
    const size_t w8 = ((size_t)(r * 8 + ph) * (len / 8) + i / 8) * 2;
    ecr[(w8 + 0) * 8 + i % 8] = x;
    ecr[(w8 + 1) * 8 + i % 8] = (_Float16)(val - (float)x);
}

// dynamic LDS of the column pass: group offsets [257] | sorted columns [width] | sample mask [width]
__host__ __device__ constexpr inline unsigned colpass_lds_sc() { return 1040u; }
__host__ __device__ inline unsigned colpass_lds_mask(int width) { return colpass_lds_sc() + (unsigned)((2 * width + 15) / 16 * 16); }
__host__ __device__ inline unsigned colpass_lds_bytes(int width) { return colpass_lds_mask(width) + (unsigned)width; }

// SAMPLES: the targets are the samples of one grid row instead of the pixels of one image row (the L_A operator of the
// eigensolver): scol lists grid-column indices b, the A table is indexed by b, and the epilogue writes
// Y[s][n] = alpha (D_s X[s][n] - (K_A X)[s][n]) for the sample s = row * nc + b.
// ECR: the A fragments come from the compact table of a uniform grid (k_grid_ecr; ecf = that table, ecr_* its geometry).
template <int NT, bool SKIP, bool SAMPLES, bool ECR = false>
__global__ __launch_bounds__(256, 2) void k_grid_colpass(const float *__restrict__ T, const _Float16 *__restrict__ ecf, int nc, int ksc,
                                                       const int *__restrict__ gcol, int radius,
                                                       const unsigned short *__restrict__ scol, const unsigned *__restrict__ goff,
                                                       const uint8_t *__restrict__ img, const uint8_t *__restrict__ mask,
                                                       const uint32_t *__restrict__ idx, unsigned p, int width, int row_begin,
                                                       int sort_row0, const float *__restrict__ tscale,
                                                       const float *__restrict__ tinv, float *__restrict__ phi, int phi_ld,
                                                       int raster, double *__restrict__ cpartial, const float *__restrict__ xin,
                                                       const double *__restrict__ degree, float alpha, int ecr_dist = 0,
                                                       int ecr_c0 = 0, int ecr_len = 0, int ecr_off = 0)
{
    constexpr int LDN = 32 * NT;
    __shared__ int cpre[257];
    __shared__ float red[4 * 2 * LDN];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int rl = blockIdx.x, r = row_begin + rl;
    // The row's sorted columns, group offsets and sample mask are staged in LDS: inside the chunk loop the only
    // vector-memory traffic is then the T stream, the A fragments and the output stores, so a wait for one of the small
    // reads never drains the T loads in flight behind it (the counter is in order).
    // A chunk is up to CT m-tiles of 32 pixels of one (row, value) group, contracted against one pass over T[r][v]. Image
    // rows take two: at cfg4 28 % of the one-tile chunks were the second or third of their group and re-read its T block after
    // it had left L2 (40 GB fetched per launch for the 30.6 GB of T that occur; 38 GB with the chunks dealt round-robin to the
    // waves). The second tile costs 48 registers (accumulators, A fragments), which the stream pays for by fetching T one slot
    // ahead instead of two (228 VGPRs, two waves per SIMD as before): 6.75 -> 6.25 ms per launch; with T two slots ahead the
    // kernel spills (8.8 ms), with the A fragments fetched in the slot that uses them 6.55. The groups of the L_A sweeps (the
    // samples of a grid row with one value) hold one or two samples: one tile, T two slots ahead.
    constexpr int CT = SAMPLES ? 1 : 2, CPX = GRID_PCT * CT;
    constexpr int TAHEAD = CT == 1 ? 2 : 1; // slots T is fetched ahead of its use (TAHEAD + 1 register sets)
    extern __shared__ __attribute__((aligned(16))) unsigned char cdyn[];
    unsigned *go = reinterpret_cast<unsigned *>(cdyn);
    unsigned short *sc = reinterpret_cast<unsigned short *>(cdyn + colpass_lds_sc());
    unsigned char *mk = cdyn + colpass_lds_mask(width);
    {
        const unsigned short *scg = scol + (size_t)(r - sort_row0) * width;
        const unsigned *gog = goff + (size_t)(r - sort_row0) * 257;
        for (int t = threadIdx.x; t < 257; t += 256) go[t] = gog[t];
        for (int t = threadIdx.x; t < width; t += 256) sc[t] = scg[t];
        if (!SAMPLES)
            for (int t = threadIdx.x; t < width; t += 256) mk[t] = mask[(size_t)r * width + t];
        __syncthreads();
    }
    const f16x8 *ecfv = reinterpret_cast<const f16x8 *>(ecf);
    {
        const int t = threadIdx.x;
        cpre[t + 1] = ((int)go[t + 1] - (int)go[t] + CPX - 1) / CPX;
        if (t == 0) cpre[0] = 0;
        __syncthreads();
        if (t == 0)
            for (int v = 0; v < 256; ++v) cpre[v + 1] += cpre[v];
        __syncthreads();
    }
    const int nchunks = cpre[256];
    float bsc[NT], osc[NT], csum[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        bsc[nt] = tscale[32 * nt + l31];
        osc[nt] = tinv[32 * nt + l31];
        csum[nt] = 0.f;
    }
    // gridDim.y workgroups share the row, each with a contiguous range of its chunks; the chunks of one value group re-read
    // the same T[r][v]
    // (dealt over all the row's waves, workgroups included, they ran at unrelated times: 19.8 GB fetched per 15.3 GB of T;
    // one wave taking a contiguous range read the second chunk of a group a whole L2 turnover after the first: 40 GB per
    // 30.6 GB at cfg4, where 28 % of the chunks are such seconds.) Within the workgroup's range the chunks go round-robin
    // to its four waves, which start together and spend the same time per chunk: the chunks of a group are streamed by
    // neighbouring waves at about the same time and all but the first find T[r][v] in L2.
    const int wg_lo = (int)(((long long)nchunks * blockIdx.y) / gridDim.y);
    const int ci_end = (int)(((long long)nchunks * (blockIdx.y + 1)) / gridDim.y);
    // One flat loop over the (chunk, k-step) pairs of this wave, like the row pass: the T block of the next pair is in
    // flight while the current pair is split and contracted, across chunk boundaries too, and the parameters of the
    // chunk after the current one (its value, pixels and fragment pointers: a chain of dependent loads) are worked out
    // one chunk ahead. With a loop per chunk every chunk began with that chain plus one exposed HBM latency -- a third
    // of its streaming time -- and ended with two re-fetches of its last k-step.
    struct Chunk {
        const float *Tv; // T[r][v]
        const f16x8 *ap[CT]; // this lane's A fragments of k-step k, per m-tile: ap[k * 4] (hi) and ap[k * 4 + ALO] (lo)
        int cm[CT];          // column of the pixel this lane feeds into the A operand of the m-tile (-1: none)
        int v, cs, npx, ks_lo, ks_hi;
        // The stream is counted in slots: a chunk has max(k-steps, 2) of them, so that two slots ahead of any slot of a
        // chunk lies in that chunk or the next. Slot j is k-step ks_lo + j; a padding slot (a chunk with one k-step)
        // re-reads that k-step and contracts it with A zeroed.
        __device__ int slots() const { return max(ks_hi - ks_lo, 2); }
        __device__ int kstep_of(int j) const { return min(ks_lo + j, ks_hi - 1); }
    };
    constexpr int ALO = ECR ? 1 : 2;
    auto setup = [&](int ci) -> Chunk {
        Chunk c;
        ci = min(ci, nchunks - 1); // past the wave's last chunk: some valid chunk, fetched from once and never contracted
        {
            int lo = 0, hi = 256; // last v with cpre[v] <= ci
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (cpre[mid] <= ci) lo = mid;
                else hi = mid;
            }
            c.v = __builtin_amdgcn_readfirstlane(lo); // (the chunk is the wave's: scalar registers from here on)
        }
        const int g1 = __builtin_amdgcn_readfirstlane((int)go[c.v + 1]);
        c.Tv = T + ((size_t)rl * 256 + c.v) * nc * LDN;
        c.cs = __builtin_amdgcn_readfirstlane((int)go[c.v] + (ci - cpre[c.v]) * CPX);
        c.npx = min(CPX, g1 - c.cs);
#pragma unroll
        for (int mt = 0; mt < CT; ++mt) {
            const int cm = 32 * mt + l31 < c.npx ? (int)sc[c.cs + 32 * mt + l31] : -1;
            c.cm[mt] = cm;
            c.ap[mt] = ecfv;
            if (ECR) {
                const int u = max(cm, 0) - ecr_c0;
                const int Q = u >= 0 ? u / ecr_dist : -((-u + ecr_dist - 1) / ecr_dist), rr = u - Q * ecr_dist, ph = (-Q) & 7;
                c.ap[mt] = ecfv + ((size_t)(rr * 8 + ph) * (ecr_len / 8) + (size_t)((-Q - ph + ecr_off) / 8 + half)) * 2;
            } else if (cm >= 0) {
                c.ap[mt] = ecfv + (size_t)cm * ksc * 4 + half;
            }
        }
        c.ks_lo = 0;
        c.ks_hi = ksc;
        if (SKIP) { // k-steps holding a sample column with a non-zero Ec for some pixel of the chunk
            const int c_first = SAMPLES ? gcol[sc[c.cs]] : (int)sc[c.cs];
            const int c_last = SAMPLES ? gcol[sc[c.cs + c.npx - 1]] : (int)sc[c.cs + c.npx - 1];
            int lo = 0, hi = nc;
            while (lo < hi) { // first b with C_b > c_first - radius
                const int mid = (lo + hi) >> 1;
                if (gcol[mid] > c_first - radius) hi = mid;
                else lo = mid + 1;
            }
            c.ks_lo = lo >> 4;
            hi = nc;
            while (lo < hi) { // first b with C_b >= c_last + radius
                const int mid = (lo + hi) >> 1;
                if (gcol[mid] >= c_last + radius) hi = mid;
                else lo = mid + 1;
            }
            c.ks_hi = (lo + 15) >> 4;
            if (c.ks_lo >= c.ks_hi) { // nothing within reach: the chunk still owes its rows of zeros -- one k-step, A zeroed
                c.ks_lo = 0;
                c.ks_hi = 1;
#pragma unroll
                for (int mt = 0; mt < CT; ++mt) c.cm[mt] = -1;
            }
        }
        return c;
    };
    f16x8 zero8;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero8[j] = (_Float16)0.f;
    // Every load is unconditional so that the compiler's wait counts stay exact.
    struct TFrag {
        float t[NT][8];
    };
    struct AFrag {
        f16x8 ah[CT], al[CT];
    };
    auto fetch_t = [&](TFrag &f, const Chunk &c, int kstep) {
        // (the last k-step reads up to 15 sample columns past the block's nc: the next block, or the padding behind the
        // last one -- zeroed in contract(); one lane offset and immediates instead of sixteen clamped addresses)
        const float *tl = c.Tv + (unsigned)((kstep * 16 + 8 * half) * LDN + l31);
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) f.t[nt][j] = tl[j * LDN + 32 * nt];
    };
    auto fetch_a = [&](AFrag &f, const Chunk &c, int kstep) {
#pragma unroll
        for (int mt = 0; mt < CT; ++mt) {
            f.ah[mt] = c.ap[mt][kstep * 4];
            f.al[mt] = c.ap[mt][kstep * 4 + ALO];
        }
    };
    f32x16 acc[CT][NT];
#pragma unroll
    for (int mt = 0; mt < CT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;
    // real: not a padding slot; the second m-tile is contracted only when the chunk reaches into it (wave-uniform)
    auto contract = [&](const TFrag &f, const AFrag &fa, const Chunk &c, bool real, int kstep) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            f16x8 bh, bl;
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                f32x2 yy;
                yy[0] = (kstep * 16 + 8 * half + j < nc ? f.t[nt][j] : 0.f) * bsc[nt];
                yy[1] = (kstep * 16 + 8 * half + j + 1 < nc ? f.t[nt][j + 1] : 0.f) * bsc[nt];
                const f16x2 h2 = __builtin_convertvector(yy, f16x2);
                f32x2 res;
                res[0] = yy[0] - (float)h2[0]; // exact in f32
                res[1] = yy[1] - (float)h2[1];
                const f16x2 l2 = __builtin_convertvector(res, f16x2);
                bh[j] = h2[0];
                bh[j + 1] = h2[1];
                bl[j] = l2[0];
                bl[j + 1] = l2[1];
            }
#pragma unroll
            for (int mt = 0; mt < CT; ++mt) {
                if (mt > 0 && c.npx <= 32 * mt) break;
                const bool live = real && c.cm[mt] >= 0;
                const f16x8 ah = live ? fa.ah[mt] : zero8, al = live ? fa.al[mt] : zero8;
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[mt][nt], 0, 0, 0);
            }
        }
    };
    // C layout: register i of this lane is pixel m = (i & 3) + 8 (i >> 2) + 4 half of the chunk, column n = l31
    auto epilogue = [&](const Chunk &c) {
#pragma unroll
        for (int mt = 0; mt < CT; ++mt) {
            if (mt > 0 && c.npx <= 32 * mt) break;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = 32 * mt + (i & 3) + 8 * (i >> 2) + 4 * half;
                if (m < c.npx && SAMPLES) {
                    // (K_A X)[s][n] only: alpha (D_s X - .) is applied by k_gridop_finish afterwards -- reading D and X
                    // here would put loads into the epilogue, and waiting for them drains the T stream of the next chunk
                    const size_t srow = (size_t)r * nc + sc[c.cs + m]; // sample index (r = grid row)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) phi[srow * phi_ld + 32 * nt + l31] = acc[mt][nt][i] * osc[nt];
                } else if (m < c.npx) {
                    const int col = sc[c.cs + m];
                    const int64_t px = (int64_t)r * width + col;
                    const bool is_sample = mk[col] != 0;
                    size_t row = (size_t)px;
                    if (!raster) row = (size_t)p + (size_t)px - samples_before(idx, p, (uint32_t)px);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const float val = acc[mt][nt][i] * osc[nt];
                        if (raster || !is_sample) phi[row * phi_ld + 32 * nt + l31] = val;
                        if (!is_sample) csum[nt] = fmaf(val, (float)c.v, csum[nt]);
                    }
                }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;
        }
    };
    int ci = wg_lo + wave;
    if (ci < ci_end) {
        Chunk cur = setup(ci), nxt = setup(ci + 4);
        int slot = 0; // of cur
        // the stream position d slots ahead of (cur, slot), d <= 2: its chunk (cur or nxt) and k-step
        auto ahead = [&](int d, Chunk &c) -> int {
            const int jj = slot + d, n = cur.slots();
            c = cur;
            if (jj >= n) c = nxt;
            return jj >= n ? nxt.kstep_of(jj - n) : cur.kstep_of(jj);
        };
        // T is fetched TAHEAD slots ahead (TAHEAD + 1 register sets), the A fragments -- a few hundred KB that stay in L2 --
        // one slot ahead (two sets): with one k-step of T in flight per wave the twelve waves of a CU held ~70 KB in flight,
        // short of what the HBM latency asks for at 6 TB/s.
        TFrag t0, t1, t2;
        AFrag a0, a1;
        {
            Chunk c;
            int k = ahead(0, c);
            fetch_t(t0, c, k);
            fetch_a(a0, c, k);
            if (TAHEAD == 2) {
                k = ahead(1, c);
                fetch_t(t1, c, k);
            }
        }
        // one slot: contracts it from (tc, ac), fetches T of the slot TAHEAD ahead into tf and A of the next slot into af;
        // false after the wave's last slot
        auto step = [&](const TFrag &tc, TFrag &tf, const AFrag &ac, AFrag &af) __attribute__((always_inline)) -> bool {
            {
                Chunk c;
                int k = ahead(TAHEAD, c);
                fetch_t(tf, c, k);
                if (TAHEAD != 1) k = ahead(1, c);
                fetch_a(af, c, k);
            }
            contract(tc, ac, cur, cur.ks_lo + slot < cur.ks_hi, cur.kstep_of(slot));
            if (++slot < cur.slots()) return true;
            epilogue(cur);
            if ((ci += 4) >= ci_end) return false;
            cur = nxt;
            nxt = setup(ci + 4);
            slot = 0;
            return true;
        };
        while (true) { // the register sets are exchanged by unrolling: T with period TAHEAD + 1, A with period 2
            if (TAHEAD == 1) {
                if (!step(t0, t1, a0, a1)) break;
                if (!step(t1, t0, a1, a0)) break;
                continue;
            }
            if (!step(t0, t2, a0, a1)) break;
            if (!step(t1, t0, a1, a0)) break;
            if (!step(t2, t1, a0, a1)) break;
            if (!step(t0, t2, a1, a0)) break;
            if (!step(t1, t0, a0, a1)) break;
            if (!step(t2, t1, a1, a0)) break;
        }
    }
    if (cpartial) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) red[(wave * 2 + half) * LDN + 32 * nt + l31] = csum[nt];
        __syncthreads();
        if (threadIdx.x < LDN) {
            double tot = 0.0;
            for (int w = 0; w < 8; ++w) tot += (double)red[w * LDN + threadIdx.x];
            cpartial[((size_t)rl * gridDim.y + blockIdx.y) * LDN + threadIdx.x] = tot;
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------

// Operands of the row-tile row pass that depend on the target rows only: Er fragments, their k-step masks and the
// (m-tile, value) presence masks.
struct RowTiles {
    int tiles = 0; // m-tiles of the shard, padded to a multiple of 4 (whole groups)
    DevBuf<_Float16> Erf;
    DevBuf<unsigned long long> tact;
    DevBuf<unsigned> pmT;
    DevBuf<uint8_t> svalT; // [nc][16 ks]: the values of the samples of a grid column, contiguous (0 behind the last grid row)
    int build(glf_ctx *ctx, const float *etab, const int *grow, int nr, int ks, int row0, int nrows, const int *rowlist,
              const unsigned *pmask, const float4 *d_samples, int nc)
    {
        tiles = (int)round_up(ceil_div(nrows, 32), 4);
        GLF_TRY(svalT.alloc(ctx, (size_t)nc * ks * 16));
        hipLaunchKernelGGL(k_grid_svalt, dim3((unsigned)ceil_div((int64_t)nc * ks * 16, 256)), dim3(256), 0, ctx->stream, d_samples, nr, nc,
                           ks * 16, svalT.p);
        GLF_TRY(Erf.alloc(ctx, (size_t)tiles * ks * 2 * 64 * 8));
        GLF_TRY(tact.alloc(ctx, (size_t)tiles));
        GLF_TRY(pmT.alloc(ctx, (size_t)tiles * 256));
        hipLaunchKernelGGL(k_grid_erfrag, dim3(tiles), dim3(64), 0, ctx->stream, etab, grow, nr, ks, row0, nrows, rowlist, Erf.p, tact.p);
        hipLaunchKernelGGL(k_grid_pmask_t, dim3(tiles), dim3(256), 0, ctx->stream, pmask, nrows, tiles, pmT.p);
        GLF_LAUNCH_CHECK(ctx);
        return GLF_OK;
    }
};

inline bool rowpass_rt_wanted(const glf_ctx *ctx) { return ctx->tune.rowpass == 0; } // rt (default) | v1 (k_grid_rowpass: one image row per wave)

constexpr int GRID_RT_ROWS = 2048; // rows per pass of the row-tile form (T: 39 GB at cfg4): the B operand of a workgroup serves 4 groups per wave; its Er fragments (2.4 MB at ks = 19) still stay in L2

template <int NT, bool SKIP, int VT, int MT, int NW, bool OP>
static int launch_rowpass_rt_cfg(glf_ctx *ctx, const RowTiles &rt, const float *Bp, const float *ptab, int nr,
                                 int nc, int ks, int row_off, int nrp, float *T)
{
    auto kern = k_grid_rowpass_rt<NT, SKIP, VT, MT, NW, OP>;
    const size_t lds = (size_t)VT * ks * NT * 2048 + (size_t)VT * ks * 16 * sizeof(float);
    GLF_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int ntiles = (int)ceil_div(nrp, 32), ngroups = (int)ceil_div(ntiles, MT);
    const int nwg_base = nc * (256 / VT);
    int splits = std::max(1, std::min((int)ceil_div(ngroups, NW), (int)ceil_div(256 * 8, nwg_base)));
    const int gpw = (int)ceil_div(ngroups, splits);
    splits = (int)ceil_div(ngroups, gpw);
    hipLaunchKernelGGL(kern, dim3(nc, 256 / VT, splits), dim3(NW * 64), lds, ctx->stream, rt.Erf.p, rt.tact.p, Bp, ptab, rt.svalT.p, nr, nc,
                       ks, row_off / 32, ntiles, gpw, rt.pmT.p, T, 0, 0, nullptr);
    return GLF_OK;
}

// row_off (a multiple of 32) = first target row of the pass within the shard, nrp = its rows
template <int NT, bool OP>
static int launch_rowpass_rt(glf_ctx *ctx, bool skip, const RowTiles &rt, const float *Bp, const float *ptab, int nr, int nc, int ks,
                             int row_off, int nrp, float *T)
{
    const bool two = (size_t)2 * ks * NT * 2048 + (size_t)2 * ks * 64 <= 160 * 1024; // two values' B fragments fit the LDS
#define GLF_RT_GO(VT, MT, NW)                                                                                                          \
    return skip ? launch_rowpass_rt_cfg<NT, true, VT, MT, NW, OP>(ctx, rt, Bp, ptab, nr, nc, ks, row_off, nrp, T)  \
                : launch_rowpass_rt_cfg<NT, false, VT, MT, NW, OP>(ctx, rt, Bp, ptab, nr, nc, ks, row_off, nrp, T)
    if (!two) { GLF_RT_GO(1, 2, 8); }
    GLF_RT_GO(2, GRID_RT_MT, GRID_RT_NW);
#undef GLF_RT_GO
}

// The first row pass (k_grid_rowpass) of the target rows [rb, rb + nrp): its LDS, the instantiation, the split of the rows
// over workgroups. OP: the L_A operator's sweep (the targets are grid rows).
template <int NT, bool OP>
static int launch_rowpass_v1(glf_ctx *ctx, bool skip, const _Float16 *Af, const float *Bp, const float *ermat, const unsigned long long *active,
                             int nc, int ks, int rb, int nrp, const unsigned *pmask, float *T)
{
    constexpr int MT = GRID_MT;
    const bool blds = ks <= GRID_KS_BLDS && GRID_MT <= 2;
    const size_t lds = (size_t)ks * 2048 * MT + (blds ? (size_t)ks * NT * 2048 + GRID_NW * 2 * ER_PIECE * sizeof(float) : 0);
    auto kern = blds ? (skip ? k_grid_rowpass<NT, true, MT, true, OP> : k_grid_rowpass<NT, false, MT, true, OP>)
                     : (skip ? k_grid_rowpass<NT, true, MT, false, OP> : k_grid_rowpass<NT, false, MT, false, OP>);
    GLF_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // splits: enough workgroups to fill the chip several times over, at least one row per wave each
    const int nwg_base = nc * (8 / MT);
    int splits = std::max(1, std::min((int)ceil_div(nrp, GRID_NW), (int)ceil_div(256 * 8, nwg_base)));
    const int rows_per_wg = (int)round_up((int)ceil_div(nrp, splits), GRID_NW); // whole rounds of the waves
    splits = (int)ceil_div(nrp, rows_per_wg);
    hipLaunchKernelGGL(kern, dim3(nc, 8 / MT, splits), dim3(GRID_NW * 64), lds, ctx->stream, Af, Bp, ermat, active, nc, ks, rb, nrp, rows_per_wg,
                       pmask, T);
    return GLF_OK;
}

// The Ec fragments of a column pass: per target column (the image's columns, or the listed ones: the grid's own for the L_A
// operator), or -- a uniform grid of at most 32 pixels' pitch, unless NO_ECR -- the compact table, one fragment set per residue of
// the pitch (hpc/sampling.c always yields a uniform grid; any tensor grid is accepted). zfrag: what a lane without a pixel reads.
struct EcTable {
    int dist = 0, off = 0, len = 0; // compact: the pitch (0: per column), the table's centre and length
    DevBuf<_Float16> frag, zfrag;
    int build(glf_ctx *ctx, const GridInfo &g, const float *etab, int maxdim, const int *d_gcol, int ntargets, const int *d_targets, bool compact)
    {
        const int nc = g.nc, ksc = (int)ceil_div(nc, 16);
        dist = compact && nc >= 2 ? g.cols[1] - g.cols[0] : 0;
        for (int b = 1; b < nc && dist > 0; ++b)
            if (g.cols[b] != g.cols[0] + dist * b) dist = 0;
        if (dist > 32 || ctx->tune.no_ecr) dist = 0;
        off = (int)round_up(ntargets / std::max(1, dist) + 16, 8);
        len = off + 16 * ksc + 16;
        if (dist > 0) {
            GLF_TRY(frag.alloc(ctx, (size_t)dist * 8 * 2 * len));
            hipLaunchKernelGGL(k_grid_ecr, dim3((unsigned)ceil_div((int64_t)dist * 8 * len, 256)), dim3(256), 0, ctx->stream, etab, maxdim, dist, len,
                               off, frag.p);
        } else {
            GLF_TRY(frag.alloc(ctx, (size_t)ntargets * ksc * 2 * 2 * 8));
            hipLaunchKernelGGL(k_grid_ecfrag, dim3((unsigned)ceil_div((int64_t)ntargets * ksc * 2, 256)), dim3(256), 0, ctx->stream, etab, d_gcol,
                               ntargets, d_targets, nc, ksc, frag.p);
        }
        return GLF_OK;
    }
    int build_zfrag(glf_ctx *ctx, int ksc)
    {
        GLF_TRY(zfrag.alloc(ctx, (size_t)(ksc * 4 + 4) * 8));
        GLF_HIP(ctx, hipMemsetAsync(zfrag.p, 0, (size_t)(ksc * 4 + 4) * 16, ctx->stream));
        return GLF_OK;
    }
};

// The row passes of one Nystroem call timed launch by launch through the context's event ring (idle here: the eigensolver is
// done). The ring's totals belong to the eigensolver's sweeps: end() (a timer that is on) takes this call's share back out.
struct MvRingTimer {
    glf_ctx *ctx;
    bool on;
    double ms0 = 0.0;
    int count0 = 0;
    int begin()
    {
        if (on) GLF_TRY(mv_collect(ctx));
        ms0 = ctx->mv_ms;
        count0 = ctx->mv_count;
        return GLF_OK;
    }
    int start()
    {
        if (on && ctx->mv_pending == glf_ctx::MV_RING) GLF_TRY(mv_collect(ctx));
        if (on) GLF_HIP(ctx, hipEventRecord(ctx->mv_ev[0][ctx->mv_pending], ctx->stream));
        return GLF_OK;
    }
    int stop()
    {
        if (on) GLF_HIP(ctx, hipEventRecord(ctx->mv_ev[1][ctx->mv_pending++], ctx->stream));
        return GLF_OK;
    }
    int end(float *ms)
    {
        GLF_TRY(mv_collect(ctx));
        *ms = (float)(ctx->mv_ms - ms0);
        ctx->mv_ms = ms0;
        ctx->mv_count = count0;
        return GLF_OK;
    }
};
// The column-pass (band form: k_band) launches of one call, the first CP_RING of them timed by event pairs of their own, created on
// first use. total(): with the stream synchronised.
struct CpTimer {
    glf_ctx *ctx;
    bool on;
    int n = 0;
    bool timing = false;
    int start()
    {
        timing = on && n < glf_ctx::CP_RING;
        for (int q = 0; timing && q < 2; ++q)
            if (!ctx->cp_ev[q][n]) GLF_HIP(ctx, hipEventCreate(&ctx->cp_ev[q][n]));
        if (timing) GLF_HIP(ctx, hipEventRecord(ctx->cp_ev[0][n], ctx->stream));
        return GLF_OK;
    }
    int stop()
    {
        if (timing) GLF_HIP(ctx, hipEventRecord(ctx->cp_ev[1][n++], ctx->stream));
        return GLF_OK;
    }
    int total(float *sum)
    {
        for (int q = 0; q < n; ++q) {
            float ms = 0.f;
            GLF_HIP(ctx, hipEventElapsedTime(&ms, ctx->cp_ev[0][q], ctx->cp_ev[1][q]));
            *sum += ms;
        }
        return GLF_OK;
    }
};

// GLF_ERR_UNSUPPORTED = the caller runs the direct kernel instead (no error is recorded).
// rq.ld = row stride of Psi and Phi; the contraction runs per block of LD = 32 NT columns (rq.ld / LD blocks share
// the grid tables, the A fragments and the T buffer).
template <int NT>
static int launch_nystroem_grid(glf_ctx *ctx, const NysRequest &rq, const GridInfo &g)
{
    constexpr unsigned LD = 32 * NT;
    const unsigned nblocks = rq.ld / LD;
    hipStream_t st = ctx->stream;
    const int nr = g.nr, nc = g.nc, ks = (int)ceil_div(nr, 16);
    const int row0 = (int)(rq.pix0 / rq.width), row1 = (int)(rq.pix1 / rq.width), nrows = row1 - row0;

    // column scales of Psi (as launch_nystroem_f16s): |Psi| T_j < 2^14; and of T: |T[..][n]| <= nr max|Psi[:, n]|. T is stored as
    // the row pass accumulated it (Psi scaled by 2^e, Er by 2^15): the column pass takes both out together with its own scale 2^et
    // -- one power of two (the row pass' 128 multiplies per epilogue were a seventh of its stores' cost)
    OperandScaleBufs sc;
    GLF_TRY(sc.reserve(ctx, rq.p, rq.ld));
    sc.run(st, rq.d_psi, rq.p, rq.ld, nr);
    GLF_LAUNCH_CHECK(ctx);

    GridTables gt;
    GLF_TRY(gt.build(ctx, g, rq.coef, rq.d_img, rq.width, rq.height, row0, row1));
    const int radius = gt.radius;
    const int *d_gcol = gt.gcol();
    // operands that do not depend on the column block: Pm_b A fragments, Ec fragment table
    const int ksc = (int)ceil_div(nc, 16);
    DevBuf<_Float16> Af;
    DevBuf<float> Bp;
    GLF_TRY(Af.alloc(ctx, (size_t)nc * 8 * ks * 2 * 64 * 8));
    GLF_TRY(Bp.alloc(ctx, (size_t)nc * ks * NT * 512));
    hipLaunchKernelGGL(k_grid_afrag, dim3((unsigned)ceil_div((int64_t)nc * 8 * ks * 64, 256)), dim3(256), 0, st, gt.ptab(), rq.d_samples,
                       nr, nc, ks, Af.p);
    EcTable ec;
    GLF_TRY(ec.build(ctx, g, gt.etab(), gt.maxdim, d_gcol, rq.width, nullptr, true));
    GLF_LAUNCH_CHECK(ctx);

    const bool use_rt = rowpass_rt_wanted(ctx);
    RowTiles rtl;
    if (use_rt) GLF_TRY(rtl.build(ctx, gt.etab(), gt.grow(), nr, ks, row0, nrows, nullptr, gt.pmask.p, rq.d_samples, nc));

    // passes over blocks of image rows
    const size_t t_row_bytes = (size_t)256 * nc * LD * sizeof(float);
    int rows_pass = (int)std::max<size_t>(4, std::min<size_t>((size_t)nrows, (use_rt ? GRID_RT_TCAP : 1) * GRID_T_BYTES / t_row_bytes));
    if (use_rt) rows_pass = std::max(64, std::min(GRID_RT_ROWS, rows_pass / 64 * 64)); // whole groups of m-tiles
    DevBuf<float> T;
    DevBuf<double> cpart;
    while (T.alloc(ctx, (size_t)round_up(rows_pass, 32) * 256 * nc * LD + GRID_T_PAD * LD) != GLF_OK) { // less HBM free than GRID_T_BYTES: smaller passes
        if (rows_pass <= (use_rt ? 64 : 4)) return GLF_ERR_NOMEM;
        rows_pass = use_rt ? std::max(64, rows_pass / 128 * 64) : std::max(4, rows_pass / 2);
    }
    constexpr int CSPLIT = GRID_COLPASS_SPLIT; // workgroups per image row in the column pass
    if (rq.d_c) GLF_TRY(cpart.alloc(ctx, (size_t)nrows * CSPLIT * LD));
    const bool skip = rq.window && gt.can_skip(rq.coef);
    ctx->nys_note.skipping = skip;
    auto colpass = ec.dist > 0 ? (skip ? k_grid_colpass<NT, true, false, true> : k_grid_colpass<NT, false, false, true>)
                               : (skip ? k_grid_colpass<NT, true, false, false> : k_grid_colpass<NT, false, false, false>);
    MvRingTimer row_timer{ctx, rq.rowpass != nullptr};
    GLF_TRY(row_timer.begin());
    if (rq.kernel_ms) GLF_HIP(ctx, hipEventRecord(ctx->ev[6], st));
    for (unsigned cb = 0; cb < nblocks; ++cb) {
        const unsigned c0 = cb * LD;
        hipLaunchKernelGGL(k_grid_bprep, dim3((unsigned)ceil_div((int64_t)nc * ks * NT * 128, 256)), dim3(256), 0, st, rq.d_psi + c0,
                           rq.ld, sc.colscale.p + c0, nr, nc, ks, NT, Bp.p);
        for (int rb = 0; rb < nrows; rb += rows_pass) {
            const int nrp = std::min(rows_pass, nrows - rb);
            GLF_TRY(row_timer.start());
            if (use_rt)
                GLF_TRY((launch_rowpass_rt<NT, false>(ctx, skip, rtl, Bp.p, gt.ptab(), nr, nc, ks, rb, nrp, T.p)));
            else
                GLF_TRY((launch_rowpass_v1<NT, false>(ctx, skip, Af.p, Bp.p, gt.ermat.p, gt.active.p, nc, ks, rb, nrp, gt.pmask.p, T.p)));
            GLF_TRY(row_timer.stop());
            if (rq.rowpass) {
                ++rq.rowpass->launches;
                rq.rowpass->flops += 2.0 * nrp * 256.0 * nc * nr * LD;
            }
            hipLaunchKernelGGL(colpass, dim3(nrp, CSPLIT), dim3(256), colpass_lds_bytes(rq.width), st, T.p, ec.frag.p, nc, ksc, d_gcol, radius, gt.scol.p, gt.goff.p, rq.d_img,
                               rq.d_mask, rq.d_idx, rq.p, rq.width, row0 + rb, row0, sc.tscale.p + c0, sc.tinv.p + c0, rq.d_phi + c0, (int)rq.ld,
                               rq.raster, rq.d_c ? cpart.p + (size_t)rb * CSPLIT * LD : nullptr, nullptr, nullptr, 0.f, ec.dist, g.cols[0],
                               ec.len, ec.off);
            GLF_LAUNCH_CHECK(ctx);
        }
        if (rq.d_c) GLF_TRY(sum_rows(ctx, cpart.p, (int64_t)nrows * CSPLIT, LD, rq.d_c + c0, true)); // synchronises: cpart is reused by the next block
    }
    if (rq.kernel_ms) GLF_HIP(ctx, hipEventRecord(ctx->ev[7], st));
    GLF_HIP(ctx, hipStreamSynchronize(st));
    if (rq.kernel_ms) GLF_HIP(ctx, hipEventElapsedTime(rq.kernel_ms, ctx->ev[6], ctx->ev[7]));
    if (rq.rowpass) GLF_TRY(row_timer.end(&rq.rowpass->ms));

    // work accounting (host side, from the grid geometry; closed forms, the loops are over grid rows / columns only)
    double ksteps = (double)ks * nrows, entries = (double)nr * nrows * (double)nc * rq.width;
    if (skip) {
        double sum_cols = 0.0;
        for (int b = 0; b < nc; ++b)
            sum_cols += std::max(0, std::min(rq.width, g.cols[b] + radius) - std::max(0, g.cols[b] - radius + 1));
        double rows_in = 0.0;
        ksteps = 0.0;
        for (int kk = 0; kk < ks; ++kk) { // image rows for which k-step kk holds a non-zero Er: within radius of one of its grid rows
            const int a_lo = kk * 16, a_hi = std::min(nr, a_lo + 16) - 1;
            int covered = row0; // union of the (ascending) intervals [R_a - radius + 1, R_a + radius) clipped to the pass
            for (int a = a_lo; a <= a_hi; ++a) {
                const int lo = std::max(covered, g.rows[a] - radius + 1), hi = std::min(row1, g.rows[a] + radius);
                if (hi > lo) {
                    ksteps += hi - lo;
                    covered = hi;
                }
            }
        }
        for (int a = 0; a < nr; ++a) rows_in += std::max(0, std::min(row1, g.rows[a] + radius) - std::max(row0, g.rows[a] - radius + 1));
        entries = rows_in * sum_cols;
    }
    if (rq.entries_evaluated) *rq.entries_evaluated = (uint64_t)entries; // kernel entries represented by the factored sums
    if (rq.mfma_flops) // row pass + column pass (every pixel takes part in one 32-row m-tile of its chunk), 3 split products
        *rq.mfma_flops = nblocks * 3.0 * 2.0 * LD * 16.0 * (ksteps * nc * 256.0 + (double)nrows * rq.width * (double)ksc);
    return GLF_OK;
}

// rank form (nystroem_rank.inc): the photometric table as a rank-R expansion, T' formed in LDS
static int launch_nystroem_rank(glf_ctx *ctx, const NysRequest &rq, const GridInfo &g);

// band form (nystroem_band.inc): entry by entry, only the samples within the kernel's radius of each pixel. forced: NYS_PATH = band
// (auto takes it only where the band is narrow); rq.flt: the filter fused into it
static int launch_nystroem_band(glf_ctx *ctx, const NysRequest &rq, const GridInfo &g, bool forced);

// the sample indices on the host (the caller's copy, or read back) as a tensor grid; false: they are none
static int nys_detect_grid(glf_ctx *ctx, const NysRequest &rq, GridInfo &g, bool *is_grid)
{
    std::vector<uint32_t> hidx(rq.p);
    if (rq.h_idx) std::copy(rq.h_idx, rq.h_idx + rq.p, hidx.begin());
    else {
        GLF_HIP(ctx, hipMemcpyAsync(hidx.data(), rq.d_idx, sizeof(uint32_t) * rq.p, hipMemcpyDeviceToHost, ctx->stream));
        GLF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *is_grid = detect_grid(hidx, rq.width, g);
    return GLF_OK;
}

// *path: 1 = exact grid form, 3 = rank form, 4 = band form
static int nystroem_contract_grid(glf_ctx *ctx, const NysRequest &rq)
{
    const int nys_path = ctx->tune.nys_path;
    if (ctx->contraction != GLF_CONTRACT_F16_SPLIT || !grid_path_wanted(nys_path, rq.width) || !band_form_applies(ctx, rq.coef.kernel))
        return GLF_ERR_UNSUPPORTED;
    // the colour and 16-bit kernels (PIX_BAND): the band form or nothing, one block of at most 64 columns, no c = Phi^T y
    const bool band_only = !grey_levels_factor(rq.coef.kernel);
    if (band_only && (!(nys_path == 0 || nys_path == 4) || rq.ld > 64 || rq.d_c)) return GLF_ERR_UNSUPPORTED;
    if (rq.pix0 % rq.width || rq.pix1 % rq.width || rq.width > GRID_MAX_W || rq.p < 4) return GLF_ERR_UNSUPPORTED;
    GridInfo g;
    bool is_grid = false;
    GLF_TRY(nys_detect_grid(ctx, rq, g, &is_grid));
    if (!is_grid || ceil_div(g.nr, 16) > GRID_MAX_KS) return GLF_ERR_UNSUPPORTED;
    // a form that answers GLF_ERR_UNSUPPORTED leaves the request to the next one
    auto ran = [&](int rc, int path) {
        if (rc != GLF_ERR_UNSUPPORTED && rq.path) *rq.path = path;
        return rc != GLF_ERR_UNSUPPORTED;
    };
    if (rq.path) *rq.path = 1;
    int rc = GLF_ERR_UNSUPPORTED;
    if (nys_path == 0 || nys_path == 4) // auto | band: only the samples within the radius of each pixel
        if (ran(rc = launch_nystroem_band(ctx, rq, g, nys_path == 4), 4)) return rc;
    if (band_only) return GLF_ERR_UNSUPPORTED;
    if (nys_path == 0 || nys_path == 3) // auto | rank: the rank form when the photometric table allows it
        if (ran(rc = launch_nystroem_rank(ctx, rq, g), 3)) return rc;
    // 64 columns at a time (ld = 128, 256: two or four column blocks)
    return rq.ld >= 64 ? launch_nystroem_grid<2>(ctx, rq, g) : launch_nystroem_grid<1>(ctx, rq, g);
}

int nystroem_band_filter(glf_ctx *ctx, const NysRequest &rq_in)
{
    const int nys_path = ctx->tune.nys_path;
    if (!rq_in.flt) return set_error(ctx, GLF_ERR_INVALID, "nystroem_band_filter: no filter");
    NysRequest rq = rq_in; // (Phi is not written and c was needed before this launch: c_from_ysum)
    rq.d_phi = nullptr;
    rq.d_c = nullptr;
    rq.raster = 1;
    if (ctx->contraction != GLF_CONTRACT_F16_SPLIT || !(nys_path == 0 || nys_path == 4) || !grey_levels_factor(rq.coef.kernel) ||
        !grid_path_wanted(nys_path, rq.width) || rq.ld > 64)
        return GLF_ERR_UNSUPPORTED;
    if (rq.pix0 % rq.width || rq.pix1 % rq.width || rq.width > GRID_MAX_W || rq.p < 4 || rq.pix0 >= rq.pix1) return GLF_ERR_UNSUPPORTED;
    GridInfo g;
    bool is_grid = false;
    GLF_TRY(nys_detect_grid(ctx, rq, g, &is_grid));
    if (!is_grid) return GLF_ERR_UNSUPPORTED;
    const int rc = launch_nystroem_band(ctx, rq, g, nys_path == 4);
    if (rc == GLF_OK && rq.path) *rq.path = 4;
    return rc;
}

// ---- the sample-sample operator L_A = alpha (D - K_A) in the same factored form ---------------------------------
// (K_A X)[(a,b)][n] = sum_{a',b'} Er(R_a - R_a') Ec(C_b - C_b') P(|v_ab - v_a'b'|) X[(a',b')][n]: the Nystroem sums with
// the samples themselves as targets -- nr target rows instead of H image rows, so a sweep costs nr / H of a Nystroem row
// pass (T: 5.6 GB at cfg4) instead of streaming the 29 GB of a stored L_A, and L_A is not stored at all.

// Y[s][n] = alpha (D_s X[s][n] - Y[s][n]) for the samples s in [s0, s1): Y holds (K_A X) from the column pass
__global__ __launch_bounds__(256) void k_gridop_finish(float *__restrict__ Y, const float *__restrict__ X,
                                                        const double *__restrict__ degree, unsigned s0, unsigned s1, unsigned ld,
                                                        float alpha)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; // one float4
    const unsigned q = ld / 4;
    if (e >= (size_t)(s1 - s0) * q) return;
    const unsigned srow = s0 + (unsigned)(e / q);
    const float dg = (float)degree[srow];
    const size_t o = (size_t)srow * q + e % q;
    const float4 x = reinterpret_cast<const float4 *>(X)[o];
    float4 y = reinterpret_cast<float4 *>(Y)[o];
    y.x = alpha * fmaf(dg, x.x, -y.x);
    y.y = alpha * fmaf(dg, x.y, -y.y);
    y.z = alpha * fmaf(dg, x.z, -y.z);
    y.w = alpha * fmaf(dg, x.w, -y.w);
    reinterpret_cast<float4 *>(Y)[o] = y;
}

// sample values as an nr x nc byte image (what k_grid_rowsort sorts per target row)
__global__ __launch_bounds__(256) void k_gridop_svals(const float4 *__restrict__ samples, unsigned p, uint8_t *__restrict__ svals)
{
    const unsigned s = blockIdx.x * 256 + threadIdx.x;
    if (s < p) svals[s] = (uint8_t)samples[s].z;
}

// the colour, 16-bit and float formats' sample values as u32 [nr][nc]. what = 0: the 16-bit value (record's z); 1: the packed colour
// (its w); 2: the bit pattern of the float value (its z); 3 (float colour): three planes [3][nr][nc], the bit patterns of R, G and B
// from the value block behind the padded records. The host takes `what` and the planes from the format table (PixDesc::svals32_*)
__global__ __launch_bounds__(256) void k_gridop_svals32(const float4 *__restrict__ samples, unsigned p, int what, unsigned *__restrict__ svals)
{
    const unsigned s = blockIdx.x * 256 + threadIdx.x;
    if (s >= p) return;
    if (what == 3) {
        const float4 e = samples[(size_t)round_up_dev(p, NYS_PAD) + s];
        svals[s] = __float_as_uint(e.x);
        svals[(size_t)p + s] = __float_as_uint(e.y);
        svals[2 * (size_t)p + s] = __float_as_uint(e.z);
    } else
        svals[s] = what == 2 ? __float_as_uint(samples[s].z) : (unsigned)(what == 1 ? samples[s].w : samples[s].z);
}

#include "nystroem_rank.inc"
#include "nystroem_band.inc"
#include "nystroem_band_vec.inc"
#include "nystroem_band_sep.inc"

} // namespace glf (GridOp is declared at global scope in glf_internal.hpp)

struct glf::GridOp {
    glf::GridInfo g;
    unsigned p = 0;
    int ksc = 0;
    bool can_skip = false;
    // the factored forms' tables (none in band form): the Nystroem passes' own, over the nr x nc byte image of the sample values
    // with the grid rows as target rows; the Ec fragments per grid column
    glf::GridTables gt;
    glf::EcTable ec;
    glf::OperandScaleBufs sc;
    glf::DevBuf<float> T, Bp;
    glf::DevBuf<_Float16> Af;
    glf::DevBuf<uint8_t> svals;
    glf::DevBuf<unsigned> svals32; // the colour, 16-bit and float formats (band form only): the sample values as u32, in place of svals (float colour: three planes)
    glf::PixGen gen = glf::PixGen::Grey;
    float nsval = 0.f;             // -s_val (the generated photometric factor of those formats)
    glf::RowTiles rtl; // row-tile form of the row pass: the grid rows [rtl_a0, rtl_a0 + rtl_rows) as target rows
    int rtl_a0 = -1, rtl_rows = 0;
    // rank form (nystroem_rank.inc): R terms of the photometric expansion (0: exact form), the context's tables, the
    // segments of the value-sorted grid rows and the intermediate S [rows][n-tile][b][k][32]
    int rank_R = 0;
    const float *rank_ftab = nullptr;
    const _Float16 *rank_Ff = nullptr;
    glf::RankSegments rank_sg;
    glf::DevBuf<float> rank_S;
    unsigned rank_ld = 0;
    int rank_nt = 0; // n-tiles per row of S the padding columns were last zeroed for
    // band form (nystroem_band.inc): only the samples within the kernel's radius of each target
    bool use_band = false;
    const glf::BandTables *band = nullptr; // (the context's cached tables)
    glf::DevBuf<unsigned char> band_chunks;
    glf::DevBuf<float> band_inv;
    const float4 *d_samples = nullptr;
    unsigned work_ld = 0;
};

namespace glf {

int grid_op_create(glf_ctx *ctx, const float4 *d_samples, const unsigned *h_idx, unsigned p, int width, int height,
                   KernelCoef coef, GridOp **out)
{
    *out = nullptr;
    if (ctx->contraction != GLF_CONTRACT_F16_SPLIT || p < 4 || !band_form_applies(ctx, coef.kernel)) return GLF_ERR_UNSUPPORTED;
    const bool band_only = !grey_levels_factor(coef.kernel); // the colour and 16-bit kernels (PIX_BAND): the band form or nothing
    if (band_only && !(ctx->tune.mv_path == 0 || ctx->tune.mv_path == 4)) return GLF_ERR_UNSUPPORTED;
    std::vector<uint32_t> idx(h_idx, h_idx + p);
    GridInfo g;
    if (!detect_grid(idx, width, g) || ceil_div(g.nr, 16) > GRID_MAX_KS || g.nc > GRID_MAX_W) return GLF_ERR_UNSUPPORTED;
    std::unique_ptr<GridOp> op(new GridOp);
    hipStream_t st = ctx->stream;
    op->g = g;
    op->p = p;
    const int nr = g.nr, nc = g.nc;
    op->ksc = (int)ceil_div(nc, 16);
    op->gen = pixgen_of(coef.kernel);
    op->nsval = -coef.s_val;
    if (band_only) {
        GLF_TRY(op->svals32.alloc(ctx, (size_t)pix_desc(op->gen).svals32_planes * p));
        hipLaunchKernelGGL(k_gridop_svals32, dim3((p + 255) / 256), dim3(256), 0, st, d_samples, p, pix_desc(op->gen).svals32_what, op->svals32.p);
    } else {
        GLF_TRY(op->svals.alloc(ctx, p));
        hipLaunchKernelGGL(k_gridop_svals, dim3((p + 255) / 256), dim3(256), 0, st, d_samples, p, op->svals.p);
    }
    GLF_LAUNCH_CHECK(ctx);
    if (ctx->tune.mv_path == 0 || ctx->tune.mv_path == 4) { // auto | band
        const int rc = band_tables_cached(ctx, g, coef, width, height, 32 * BAND_PB, false, &op->band);
        if (rc != GLF_OK && rc != GLF_ERR_UNSUPPORTED) return rc;
        op->use_band = rc == GLF_OK && (ctx->tune.mv_path == 4 || op->band->narrow(height));
        if (ctx->tune.mv_path == 4 && !op->use_band) return GLF_ERR_UNSUPPORTED;
    }
    if (band_only && !op->use_band) {
        GLF_HIP(ctx, hipStreamSynchronize(st));
        return GLF_ERR_UNSUPPORTED;
    }
    if (op->use_band) {
        op->d_samples = d_samples;
        GLF_HIP(ctx, hipStreamSynchronize(st));
        *out = op.release();
        return GLF_OK;
    }
    GridTables &gt = op->gt;
    GLF_TRY(gt.build(ctx, op->g, coef, std::max(width, height), GridTargets{op->svals.p, nc, 0, nr, true}, false));
    op->can_skip = gt.can_skip(coef);
    GLF_TRY(op->Af.alloc(ctx, (size_t)nc * 8 * gt.ks * 2 * 64 * 8));
    hipLaunchKernelGGL(k_grid_afrag, dim3((unsigned)ceil_div((int64_t)nc * 8 * gt.ks * 64, 256)), dim3(256), 0, st, gt.ptab(), d_samples, nr, nc,
                       gt.ks, op->Af.p);
    GLF_TRY(op->ec.build(ctx, op->g, gt.etab(), gt.maxdim, gt.gcol(), nc, gt.gcol(), false));
    GLF_LAUNCH_CHECK(ctx);
    if ((ctx->tune.mv_path == 0 || ctx->tune.mv_path == 3) && gt.ks <= GRID_KS_BLDS) { // auto | rank
        GLF_TRY(rank_tables(ctx, coef, &op->rank_R, &op->rank_ftab, &op->rank_Ff));
        if (op->rank_R && !ctx->tune.sweep_samples) { // (only the value-grouped column pass needs the segments of the grid rows)
            GLF_TRY(op->rank_sg.build(ctx, gt.scol.p, gt.goff.p, nr, nc, gt.gcol(), nc, op->ksc, true, gt.radius16, nullptr, 0, 0, 0, 0));
            GLF_TRY(op->ec.build_zfrag(ctx, op->ksc));
        }
    }
    op->d_samples = d_samples; // the sample table outlives the operator (both belong to one image_processing call)
    GLF_HIP(ctx, hipStreamSynchronize(st)); // (the one of the call: the tables' uploads from op->g and gt.htab included)
    *out = op.release();
    return GLF_OK;
}

void grid_op_destroy(GridOp *op) { delete op; }

void band_cache_free(glf_ctx *ctx)
{
    for (int q = 0; q < 2; ++q) {
        band_cache_delete(ctx->band_cache[q]);
        ctx->band_cache[q] = nullptr;
    }
}

unsigned grid_op_rows_per_rank(const GridOp *op, int size) { return (unsigned)(ceil_div(op->g.nr, size) * op->g.nc); }
int grid_op_path(const GridOp *op) { return op->use_band ? 4 : op->rank_R ? 3 : 1; }
int grid_op_row_len(const GridOp *op) { return op->g.nc; }
bool grid_op_can_skip(const GridOp *op) { return !op->use_band && op->can_skip; }

// Y[s][:] = alpha (D_s X[s][:] - (K_A X)[s][:]) for the samples s in [row0, row1) (whole grid rows); X holds all p rows.
template <int NT>
static int grid_op_apply_nt(glf_ctx *ctx, GridOp *op, const float *X, float *Y, unsigned ld_total, double alpha,
                            const double *d_degree, unsigned row0, unsigned row1, int window, const ColMaxima *maxima)
{
    if (ctx->tune.operand_maxima_sweep) maxima = nullptr;
    constexpr unsigned LD = 32 * NT;
    hipStream_t st = ctx->stream;
    const GridTables &gt = op->gt;
    const int nr = op->g.nr, nc = op->g.nc, ks = gt.ks, ksc = op->ksc;
    const int a0 = (int)(row0 / nc), a1 = (int)(row1 / nc), nrows = a1 - a0;
    if (nrows <= 0) return GLF_OK;
    if (op->use_band) { // scales, operand chunks, one launch per 32 NT columns: Y = alpha (D X - K_A X) in the kernel's epilogue
        if (op->work_ld < ld_total) {
            GLF_TRY(op->sc.reserve(ctx, op->p, ld_total));
            GLF_TRY(op->band_inv.alloc(ctx, ld_total));
            GLF_TRY(op->band_chunks.alloc(ctx, (size_t)nr * ksc * band_chunk_bytes(2)));
            op->work_ld = ld_total;
        }
        band_scales(st, X, op->p, ld_total, op->sc.camx.p, op->sc.colscale.p, op->band_inv.p, maxima);
        for (unsigned c0 = 0; c0 < ld_total; c0 += LD) {
            const bool raw = op->gen != PixGen::Grey;
            const uint8_t *sv = raw ? reinterpret_cast<const uint8_t *>(op->svals32.p) : op->svals.p;
            GLF_TRY(band_prep(ctx, X + c0, ld_total, op->sc.colscale.p + c0, sv, raw, nr, nc, ksc, NT, op->band_chunks.p, pix_desc(op->gen).svals32_planes));
            int rc = GLF_OK;
            pix_dispatch(op->gen, [&](auto t) {
                rc = launch_band_samples<NT, t.G>(ctx, *op->band, sv, a0, nrows, op->band_chunks.p, op->band_inv.p + c0, Y + c0, (int)ld_total, X + c0,
                                                  (int)ld_total, d_degree, (float)alpha, nullptr, op->nsval);
            });
            GLF_TRY(rc);
        }
        return GLF_OK;
    }
    if (op->work_ld < ld_total) { // (a narrower block -- the packed sweeps of block PCG -- reuses the wider block's buffers)
        GLF_TRY(op->sc.reserve(ctx, op->p, ld_total));
        GLF_TRY(op->Bp.alloc(ctx, (size_t)nc * ks * NT * 512));
        if (!op->rank_R) GLF_TRY(op->T.alloc(ctx, (size_t)nr * 256 * nc * LD + GRID_T_PAD * LD));
        op->work_ld = ld_total;
    }
    // per-column power-of-two scales from max |X[:, n]| (device side: no host round trip inside the PCG loop)
    op->sc.run(st, X, op->p, ld_total, nr, maxima);
    const bool skip = window && op->can_skip;
    auto colpass = skip ? k_grid_colpass<NT, true, true> : k_grid_colpass<NT, false, true>;
    const int *gcol = gt.gcol();
    const bool use_rank = op->rank_R > 0;
    const bool use_rt = use_rank || ctx->tune.rowpass_op == 1; // rt | v1 (default: the sweeps have few target rows per B operand)
    const int ncs = ksc * 16;
    if (use_rank && op->rank_ld < ld_total) {
        GLF_TRY(op->rank_S.alloc(ctx, (size_t)round_up(nr, 64) * NT * ncs * op->rank_R * 32));
        op->rank_ld = ld_total;
        op->rank_nt = 0;
    }
    if (use_rank && op->rank_nt != NT) { // the padding columns sit elsewhere when a narrower block reuses the buffer (row stride NT ncs R 32)
        GLF_TRY(rank_zero_pad(ctx, op->rank_S.p, (int)round_up(nr, 64), NT, nc, ncs, op->rank_R));
        op->rank_nt = NT;
    }
    if (use_rt && (op->rtl_a0 != a0 || op->rtl_rows != nrows)) { // a rank applies the operator to the same grid rows every time
        GLF_TRY(op->rtl.build(ctx, gt.etab(), gt.grow(), nr, ks, 0, nrows, gt.grow() + a0, gt.pmask.p + (size_t)a0 * 8, op->d_samples, nc));
        op->rtl_a0 = a0;
        op->rtl_rows = nrows;
    }
    for (unsigned c0 = 0; c0 < ld_total; c0 += LD) {
        if (use_rank) // one operand image per n-tile of 32 columns (the rank row pass takes one n-tile per workgroup)
            for (int t = 0; t < NT; ++t)
                hipLaunchKernelGGL(k_grid_bprep, dim3((unsigned)ceil_div((int64_t)nc * ks * 128, 256)), dim3(256), 0, st, X + c0 + 32 * t, ld_total,
                                   op->sc.colscale.p + c0 + 32 * t, nr, nc, ks, 1, op->Bp.p + (size_t)t * nc * ks * 512);
        else
            hipLaunchKernelGGL(k_grid_bprep, dim3((unsigned)ceil_div((int64_t)nc * ks * NT * 128, 256)), dim3(256), 0, st, X + c0, ld_total,
                               op->sc.colscale.p + c0, nr, nc, ks, NT, op->Bp.p);
        if (use_rank) {
            // S[a'][n-tile][b][k][32] for the grid rows of this rank, then T' and the Ec contraction per (grid row, segment)
            GLF_TRY((launch_rowpass_rank<true>(ctx, skip, op->rtl, op->Bp.p, op->rank_ftab, op->rank_R, NT, nr, nc, ks, ncs, 0, nrows,
                                                   op->rank_S.p, op->sc.tscale.p + c0)));
            if (!ctx->tune.sweep_samples) // (default) the value-grouped column pass of the Nystroem stage on the samples
                GLF_TRY((launch_rank_colpass<true>(ctx, op->rank_R, false, op->rank_S.p, ncs, NT, op->rank_Ff, op->ec.frag.p, op->ec.zfrag.p, nc, ksc,
                                                   op->rank_sg, a0, nrows, nullptr, op->p, nc, a0, op->sc.tinv.p + c0, Y + c0, (int)ld_total, 1,
                                                   nullptr)));
            else
                GLF_TRY(launch_rank_samples(ctx, op->rank_R, op->rank_S.p, ncs, NT, op->rank_ftab, op->svals.p, gt.etab(), gcol, nc, a0,
                                            nrows, op->sc.tinv.p + c0, Y + c0, (int)ld_total));
            continue;
        }
        if (use_rt)
            GLF_TRY((launch_rowpass_rt<NT, true>(ctx, skip, op->rtl, op->Bp.p, gt.ptab(), nr, nc, ks, 0, nrows, op->T.p)));
        else
            GLF_TRY((launch_rowpass_v1<NT, true>(ctx, skip, op->Af.p, op->Bp.p, gt.ermat.p, gt.active.p, nc, ks, a0, nrows, gt.pmask.p, op->T.p)));
        hipLaunchKernelGGL(colpass, dim3(nrows, GRID_COLPASS_SPLIT_OP), dim3(256), colpass_lds_bytes(nc), st, op->T.p, op->ec.frag.p, nc, ksc, gcol, gt.radius, gt.scol.p, gt.goff.p,
                           nullptr, nullptr, nullptr, op->p, nc, a0, 0, op->sc.tscale.p + c0, op->sc.tinv.p + c0, Y + c0, (int)ld_total, 1,
                           nullptr, X + c0, d_degree, (float)alpha, 0, 0, 0, 0);
    }
    hipLaunchKernelGGL(k_gridop_finish, dim3((unsigned)ceil_div((int64_t)nrows * nc * (ld_total / 4), 256)), dim3(256), 0, st, Y, X,
                       d_degree, (unsigned)a0 * nc, (unsigned)a1 * nc, ld_total, (float)alpha);
    GLF_LAUNCH_CHECK(ctx);
    return GLF_OK;
}

int grid_op_apply(glf_ctx *ctx, GridOp *op, const float *X, float *Y, unsigned ld, double alpha, const double *d_degree,
                  unsigned row0, unsigned row1, int window, const ColMaxima *maxima)
{
    if (row0 % op->g.nc || (row1 % op->g.nc && row1 != op->p))
        return set_error(ctx, GLF_ERR_INVALID, "grid_op_apply: rows [%u, %u) are not whole grid rows", row0, row1);
    if (ld >= 64) return grid_op_apply_nt<2>(ctx, op, X, Y, ld, alpha, d_degree, row0, row1, window, maxima);
    return grid_op_apply_nt<1>(ctx, op, X, Y, ld, alpha, d_degree, row0, row1, window, maxima);
}
