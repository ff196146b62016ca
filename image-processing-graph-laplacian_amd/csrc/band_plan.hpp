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
