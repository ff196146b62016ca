// grid_common.inc -- pieces shared by the grid-factored Nystroem contraction (nystroem_grid.inc) and the grid-factored
// degree (affinity_grid.inc): detection of a tensor-grid sample set, the factor tables, the per-row counting sort.
// Included inside namespace glf; everything has internal linkage (the file is included by two translation units).
namespace {

constexpr int GRID_MAX_W = 16384; // an image row is staged in LDS by the sort
constexpr int GRID_MIN_W = 1024;  // below this width the direct kernels win (the factored forms always sweep all 256 values)

// tuning NYS_PATH / DEG_PATH = grid | direct | auto (default): force or forbid the grid-factored form
inline bool grid_path_wanted(int setting, int width)
{
    if (setting == 1 || setting == 3 || setting == 4) return true; // grid | rank (the rank form of the grid-factored contraction) | band
    if (setting == 2) return false;
    return width >= GRID_MIN_W;
}

// first distance from which 2^15 E(d) is a zero f16 (hi, lo) pair (the spatial factor as the split-f16 kernels carry it):
// 2^15 E <= 2^-25 rounds to a zero f16 and leaves nothing for the lo half either
inline int f16_zero_radius(const float *etab, int maxdim)
{
    for (int d = 0; d < maxdim; ++d)
        if (etab[d] <= 0x1p-40f) return d;
    return maxdim;
}

struct GridInfo {
    int nr = 0, nc = 0;
    std::vector<int> rows, cols;
};

static bool detect_grid(const std::vector<uint32_t> &idx, int width, GridInfo &g)
{
    const size_t p = idx.size();
    if (p == 0) return false;
    const uint32_t r0 = idx[0] / (uint32_t)width;
    size_t nc = 0;
    while (nc < p && idx[nc] / (uint32_t)width == r0) ++nc;
    if (nc == 0 || p % nc) return false;
    const size_t nr = p / nc;
    g.nr = (int)nr;
    g.nc = (int)nc;
    g.rows.resize(nr);
    g.cols.resize(nc);
    for (size_t b = 0; b < nc; ++b) {
        g.cols[b] = (int)(idx[b] % (uint32_t)width);
        if (b && g.cols[b] <= g.cols[b - 1]) return false;
    }
    for (size_t a = 0; a < nr; ++a) {
        g.rows[a] = (int)(idx[a * nc] / (uint32_t)width);
        if (a && g.rows[a] <= g.rows[a - 1]) return false;
    }
    for (size_t a = 0; a < nr; ++a)
        for (size_t b = 0; b < nc; ++b)
            if (idx[a * nc + b] != (uint32_t)g.rows[a] * (uint32_t)width + (uint32_t)g.cols[b]) return false;
    return true;
}

// ermat[rl][k] = Er(row0 + rl - R_k) (0 for the padding k >= nr); active[rl] = bit mask of the 16-row k-steps
// that hold a non-zero (all of them matter to the dense sweep; the skipping sweep visits only these)
__global__ __launch_bounds__(64) void k_grid_ermat(const float *__restrict__ etab, const int *__restrict__ grow, int nr, int kp,
                                                    int row0, const int *__restrict__ rowlist, float *__restrict__ ermat,
                                                    unsigned long long *__restrict__ active)
{
    // target rows: the image rows row0 + rl, or (rowlist) the listed rows (the grid rows themselves for the L_A operator)
    const int rl = blockIdx.x, r = rowlist ? rowlist[rl] : row0 + rl, lane = threadIdx.x;
    unsigned long long act = 0;
    for (int i = 0; i * 64 < kp; ++i) {
        const int k = lane + 64 * i;
        float e = 0.f;
        if (k < nr) e = etab[abs(r - grow[k])];
        if (k < kp) ermat[(size_t)rl * kp + k] = e;
        const unsigned long long nz = __ballot(e != 0.f);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if ((nz >> (16 * q)) & 0xFFFFull) act |= 1ull << (4 * i + q);
    }
    if (lane == 0) active[rl] = act;
}

// Stable counting sort of one image row by pixel value: scol = columns ordered by (value, column),
// goff[v] .. goff[v + 1] = the group of value v. One workgroup of four waves per row; wave w owns the w-th quarter of the
// columns. Counts per (quarter, value) by LDS atomics, then every wave walks its quarter 64 columns at a time: a lane's
// rank among the lanes of the batch with its value (eight ballots give the mask of those lanes) is its offset behind the
// running position of (quarter, value), which the first lane of each value then advances. The sorted row is assembled in
// LDS and written out in whole lines. (Every thread scanning the whole row twice for its own value took 0.69 ms per
// 4096 x 4096 image, three times per step.)
__global__ __launch_bounds__(256) void k_grid_rowsort(const uint8_t *__restrict__ img, int width, int row0,
                                                       unsigned short *__restrict__ scol, unsigned *__restrict__ goff,
                                                       unsigned *__restrict__ pmask)
{
    __shared__ __attribute__((aligned(16))) uint8_t rowb[GRID_MAX_W];
    __shared__ __attribute__((aligned(16))) unsigned short sorted[GRID_MAX_W];
    __shared__ unsigned pos[4][256]; // counts, then running positions, per (quarter, value)
    __shared__ unsigned cnt[257];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint8_t *src = img + (size_t)(row0 + blockIdx.x) * width;
    for (int c = t; c < width; c += 256) rowb[c] = src[c];
#pragma unroll
    for (int q = 0; q < 4; ++q) pos[q][t] = 0;
    __syncthreads();
    const int seg = ((width + 3) / 4 + 63) / 64 * 64, c_lo = wave * seg, c_hi = min(width, c_lo + seg);
    for (int c = c_lo + lane; c < c_hi; c += 64) atomicAdd(&pos[wave][rowb[c]], 1u);
    __syncthreads();
    const unsigned n = pos[0][t] + pos[1][t] + pos[2][t] + pos[3][t]; // pixels of value t in the row
    cnt[t] = n;
    __syncthreads();
    if (t == 0) {
        unsigned s = 0;
        for (int v = 0; v < 256; ++v) {
            const unsigned k = cnt[v];
            cnt[v] = s;
            s += k;
        }
        cnt[256] = s;
    }
    __syncthreads();
    {
        unsigned s = cnt[t];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned k = pos[q][t];
            pos[q][t] = s;
            s += k;
        }
    }
    __syncthreads();
    volatile unsigned *mypos = pos[wave];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c0 = c_lo; c0 < c_hi; c0 += 64) { // (wave-uniform bounds)
        const int c = c0 + lane;
        const bool valid = c < c_hi;
        const unsigned v = valid ? rowb[c] : 0u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned long long b = __ballot((v >> k) & 1u);
            peers &= ((v >> k) & 1u) ? b : ~b;
        }
        const unsigned rank = (unsigned)__popcll(peers & below);
        unsigned base = 0;
        if (valid) {
            base = mypos[v];
            sorted[base + rank] = (unsigned short)c;
        }
        __builtin_amdgcn_wave_barrier(); // every lane has read the running position before the leaders advance it
        if (valid && rank == 0) mypos[v] = base + (unsigned)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    unsigned short *dst = scol + (size_t)blockIdx.x * width;
    for (int c = t; c < width; c += 256) dst[c] = sorted[c];
    goff[(size_t)blockIdx.x * 257 + t] = cnt[t];
    if (t == 0) goff[(size_t)blockIdx.x * 257 + 256] = cnt[256];
    // presence mask of the row: bit (v % 32) of word v / 32 = some pixel of the row has value v
    const unsigned long long present = __ballot(n != 0);
    if ((t & 63) == 0) {
        pmask[(size_t)blockIdx.x * 8 + t / 32] = (unsigned)present;
        pmask[(size_t)blockIdx.x * 8 + t / 32 + 1] = (unsigned)(present >> 32);
    }
}


// The target rows of the tables: nrows rows of a byte image with `stride` columns, from its row `first` on. They stand at the image
// rows first + rl -- or, at_grid_rows, at the sample grid's own rows: the L_A operator, whose image is the nr x nc image of the
// sample values.
struct GridTargets {
    const uint8_t *img;
    int stride, first, nrows;
    bool at_grid_rows;
};
// Device-side tables of one (sample grid, kernel, target rows): P and E factor tables (correctly rounded from f64), grid
// coordinates, Er per (target row, grid row) with the non-zero k-step mask, and the value-sorted columns of every target row.
struct GridTables {
    int nr = 0, nc = 0, ks = 0, kp = 0, ncp = 0, radius = 0, radius16 = 0, row0 = 0, nrows = 0, maxdim = 0;
    std::vector<float> htab; // (pageable: kept while its upload may be in flight)
    DevBuf<float> tab, ermat;
    DevBuf<int> grid;
    DevBuf<unsigned long long> active;
    DevBuf<unsigned> goff, pmask;
    DevBuf<unsigned short> scol;
    const float *ptab() const { return tab.p; }
    const float *etab() const { return tab.p + 256; }
    const int *grow() const { return grid.p; }
    const int *gcol() const { return grid.p + nr; }
    // maxdim: the distances the E table covers (the larger side of the image). g outlives the call's stream work; sync = false
    // leaves the stream to the caller, who synchronises before the tables are used from another stream or g goes away.
    int build(glf_ctx *ctx, const GridInfo &g, KernelCoef coef, int maxdim_, const GridTargets &t, bool sync = true)
    {
        hipStream_t st = ctx->stream;
        nr = g.nr;
        nc = g.nc;
        ks = (int)ceil_div(nr, 16);
        kp = ks * 16;
        ncp = (int)round_up(nc, 4);
        row0 = t.first;
        nrows = t.nrows;
        maxdim = maxdim_;
        htab.resize(256 + (size_t)maxdim);
        for (int e = 0; e < 256; ++e) htab[e] = (float)std::exp2(-(double)coef.s_val * e * e);
        for (int d = 0; d < maxdim; ++d) htab[256 + d] = (float)std::exp2(-(double)coef.s_loc * (double)d * (double)d);
        radius = maxdim; // first distance at which the spatial factor is exactly +0 in f32
        for (int d = 0; d < maxdim; ++d)
            if (htab[256 + d] == 0.f) {
                radius = d;
                break;
            }
        radius16 = f16_zero_radius(htab.data() + 256, maxdim);
        GLF_TRY(tab.alloc(ctx, htab.size()));
        GLF_TRY(grid.alloc(ctx, (size_t)nr + nc));
        GLF_HIP(ctx, hipMemcpyAsync(tab.p, htab.data(), sizeof(float) * htab.size(), hipMemcpyHostToDevice, st));
        GLF_HIP(ctx, hipMemcpyAsync(grid.p, g.rows.data(), sizeof(int) * nr, hipMemcpyHostToDevice, st));
        GLF_HIP(ctx, hipMemcpyAsync(grid.p + nr, g.cols.data(), sizeof(int) * nc, hipMemcpyHostToDevice, st));
        GLF_TRY(ermat.alloc(ctx, (size_t)nrows * kp));
        GLF_TRY(active.alloc(ctx, (size_t)nrows));
        GLF_TRY(scol.alloc(ctx, (size_t)nrows * t.stride));
        GLF_TRY(goff.alloc(ctx, (size_t)nrows * 257));
        GLF_TRY(pmask.alloc(ctx, (size_t)nrows * 8));
        hipLaunchKernelGGL(k_grid_rowsort, dim3(nrows), dim3(256), 0, st, t.img, t.stride, row0, scol.p, goff.p, pmask.p);
        hipLaunchKernelGGL(k_grid_ermat, dim3(nrows), dim3(64), 0, st, etab(), grow(), nr, kp, row0, t.at_grid_rows ? grow() : nullptr, ermat.p,
                           active.p);
        GLF_LAUNCH_CHECK(ctx);
        if (sync) GLF_HIP(ctx, hipStreamSynchronize(st));
        return GLF_OK;
    }
    // the image rows [r0, r1) of d_img as targets (the Nystroem passes, the degree)
    int build(glf_ctx *ctx, const GridInfo &g, KernelCoef coef, const uint8_t *d_img, int width, int height, int r0, int r1)
    {
        return build(ctx, g, coef, std::max(width, height), GridTargets{d_img, width, r0, r1 - r0, false});
    }
    bool can_skip(KernelCoef coef) const { return coef.s_loc > 0.f && radius < maxdim; }
};

} // namespace
