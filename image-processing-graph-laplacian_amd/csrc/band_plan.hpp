// band_plan.hpp -- geometry and schedule of the band form (nystroem_band.inc) that needs no device: the radius, the windows of
// sample columns a tile of targets can reach at a row distance, and how k_band's pixel-target instantiations pair band rows.
// Compiled into host_util.cpp (glf_band_plan, what tests/test_band_plan.py checks) and into the kernels' translation unit:
// the window helpers below are the ones the kernel itself schedules with.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIP__) || defined(__CUDACC__)
#define GLF_BAND_HD __host__ __device__
#else
#define GLF_BAND_HD
#endif

namespace glf {

#ifndef BAND_MAXROWS_X
#define BAND_MAXROWS_X 128
#endif
constexpr int BAND_MAXROWS = BAND_MAXROWS_X; // grid rows within the radius of one target row
constexpr int BAND_RMAX = 1023;              // largest radius (the Ec table sits in LDS)
constexpr unsigned BAND_EMPTY = 0x0000FFFFu; // lo = 0xFFFF, hi = 0: no block
#ifndef BAND_PB_X
#define BAND_PB_X 2
#endif
#ifndef BAND_NW_X
#define BAND_NW_X 8
#endif
constexpr int BAND_PB = BAND_PB_X, BAND_NW = BAND_NW_X; // pixel targets: 64 columns per wave, 8 image rows per workgroup
// Pixel targets: the unit of work is a half-block of 8 sample columns (what one lane-half of v_mfma_f32_32x32x16_f16 holds of
// k) in two consecutive band rows, pairs aligned to the workgroup's first band row. Sample targets: 16 columns of one band row.
constexpr int BAND_HALF_SHIFT = 3, BAND_BLOCK_SHIFT = 4, BAND_PAIR = 2;

// windows: lo | hi << 16 in units of (half-)blocks, lo > hi: empty
GLF_BAND_HD inline bool band_win_live(unsigned u) { return (u & 0xFFFFu) <= (u >> 16); }
GLF_BAND_HD inline bool band_win_has(unsigned u, int c) { return c >= (int)(u & 0xFFFFu) && c <= (int)(u >> 16); }
// smallest window holding both (the windows of one tile are nested -- the circle narrows with dr -- so this is their union)
GLF_BAND_HD inline unsigned band_win_hull(unsigned u, unsigned v)
{
    if (!band_win_live(u)) return v;
    if (!band_win_live(v)) return u;
    const unsigned lo = (u & 0xFFFFu) < (v & 0xFFFFu) ? (u & 0xFFFFu) : (v & 0xFFFFu);
    const unsigned hi = (u >> 16) > (v >> 16) ? (u >> 16) : (v >> 16);
    return lo | (hi << 16);
}
// hull of the bands (rowband[r] = BandGeom::band_of(r)) of the n target rows from r0; *alo = 0xFFFF > *ahi = -1: none of them has one
GLF_BAND_HD inline void band_rows_hull(const unsigned *rowband, int r0, int n, int *alo, int *ahi)
{
    int lo = 0xFFFF, hi = -1;
    for (int w = 0; w < n; ++w) {
        const unsigned rb = rowband[r0 + w];
        if (!band_win_live(rb)) continue;
        lo = (int)(rb & 0xFFFFu) < lo ? (int)(rb & 0xFFFFu) : lo;
        hi = (int)(rb >> 16) > hi ? (int)(rb >> 16) : hi;
    }
    *alo = lo;
    *ahi = hi;
}
// the ascending sample columns gcol[0 .. nc) inside [cmin, cmax]: *lo = the first one >= cmin, *count of them (0 where cmax < cmin)
GLF_BAND_HD inline void band_cols_range(const int *gcol, int nc, int cmin, int cmax, int *lo, int *count)
{
    int l = 0, h = nc; // first column >= cmin
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (gcol[mid] < cmin) l = mid + 1;
        else h = mid;
    }
    const int first = l;
    h = nc; // first column > cmax, from there on
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (gcol[mid] <= cmax) l = mid + 1;
        else h = mid;
    }
    *lo = first;
    *count = l - first;
}

// Column pass of the separable form on the matrix pipe (k_band_sep_cols_mfma, nystroem_band_sep.inc). A wave's tile is `tile_px`
// pixels of one image row = tile_px / 32 pixel tiles of the MFMA's N; the sample columns within d of the tile (band_cols_range,
// clipped at the image width) are walked in k-steps of BSEP_KSTEP: entry i of the range is column clo + i, k-step i / 16, and
// entries from the count on are dead (their Ec operand is zero, their index clamped inside the grid).
constexpr int BSEP_KSTEP = 16;
GLF_BAND_HD inline void band_sep_tile_cols(const int *gcol, int nc, int width, int tc0, int tile_px, int d, int *clo, int *count)
{
    *clo = 0;
    *count = 0;
    const int tc1 = (tc0 + tile_px < width ? tc0 + tile_px : width) - 1;
    if (d >= 0 && tc1 >= tc0) band_cols_range(gcol, nc, tc0 - d, tc1 + d, clo, count);
}
GLF_BAND_HD inline int band_sep_ksteps(int count) { return (count + BSEP_KSTEP - 1) / BSEP_KSTEP; }
// index (into gcol, and of S's sample column) of entry i >= 0 of a range from clo: inside [0, nc) whatever i
GLF_BAND_HD inline int band_sep_col(int clo, int i, int nc) { return clo + i < nc - 1 ? clo + i : nc - 1; }
// do the live entries of k-step ks (16 ks < count) all lie rad or more from every pixel of [p0, p1]? Then the block of Ec is zero
// throughout (the table is an exact zero from rad on) and the k-step adds exact zeros to that pixel tile.
GLF_BAND_HD inline bool band_sep_block_dead(const int *gcol, int nc, int clo, int count, int ks, int p0, int p1, int rad)
{
    const int i1 = BSEP_KSTEP * ks + BSEP_KSTEP - 1 < count - 1 ? BSEP_KSTEP * ks + BSEP_KSTEP - 1 : count - 1;
    const int first = gcol[band_sep_col(clo, BSEP_KSTEP * ks, nc)], last = gcol[band_sep_col(clo, i1, nc)];
    return first - p1 >= rad || p0 - last >= rad;
}
// 16 x 32 entries per (k-step, pixel tile) the column pass executes for the tile from tc0 (all: none is passed over)
GLF_BAND_HD inline uint64_t band_sep_tile_entries(const int *gcol, int nc, int width, int tc0, int tile_px, int d, int rad, bool all)
{
    int clo, count;
    band_sep_tile_cols(gcol, nc, width, tc0, tile_px, d, &clo, &count);
    uint64_t n = 0;
    for (int ks = 0; ks < band_sep_ksteps(count); ++ks)
        for (int pt = 0; pt < tile_px / 32; ++pt)
            if (all || !band_sep_block_dead(gcol, nc, clo, count, ks, tc0 + 32 * pt, tc0 + 32 * pt + 31, rad)) n += (uint64_t)BSEP_KSTEP * 32u;
    return n;
}

// radius and windows of one (sample grid, spatial coefficient)
struct BandGeom {
    int rad = 0;
    double D2 = 0.0;
    std::vector<int> rows, cols, dcmax; // dcmax[dr]: largest |dc| inside the circle at row distance dr (-1: none)
    // false: no spatial factor, or a radius beyond BAND_RMAX
    bool init(const int *grows, int nr, const int *gcols, int nc, double s_loc);
    // grid rows with |r - R_a| < rad (the rows ascend): lo | hi << 16 (lo > hi: none)
    unsigned band_of(int r) const;
    // sample columns within dcmax[dr] of the targets [cmin, cmax], in units of 2^shift columns
    unsigned window(int cmin, int cmax, int dr, int shift) const;
};

} // namespace glf
