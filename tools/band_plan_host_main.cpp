// Stand-alone check of the window plan the three forms of the fused band filter share (band_plan.hpp: band_rows_hull, band_cols_range)
// and of BandGeom::window / band_of beside them: built together with host_util.cpp under the address and undefined-behaviour
// sanitizers by `make band_plan_check`. CPU only; no device, no python.
// A few hundred random ascending grids in exactly sized heap buffers (one element too far is reported), one-column grids among them;
// tiles inside the grid, wholly left and wholly right of every column; d = -1 (a range narrower than the tile, inverted for one
// pixel; as dcmax[dr] it means no column at all, which the callers' guard and BandGeom::window decide); blocks of rows that no
// band reaches.
// The k-step plan of the matrix-pipe column pass (band_sep_tile_cols, band_sep_ksteps, band_sep_col, band_sep_block_dead,
// band_sep_tile_entries) against a brute-force enumeration of the (pixel, sample column) pairs of a tile: every pair within d of
// each other sits in exactly one live entry of a block that is not dead, every index the kernel forms lies inside the grid, a dead
// block holds no pair nearer than the radius. Widths that are no multiple of the tile, fewer than 16 columns and counts that are no
// multiple of 16, radii larger than the image, tiles clipped at either image edge.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../image-processing-graph-laplacian_amd/csrc/band_plan.hpp"

using namespace glf;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static std::vector<int> ascending(std::mt19937 &rng, int n, int first, int max_pitch)
{
    std::vector<int> v(n);
    for (int i = 0, x = first; i < n; ++i) {
        v[i] = x;
        x += 1 + (int)(rng() % (unsigned)max_pitch);
    }
    return v;
}

// band_cols_range against std::lower_bound / std::upper_bound (a range with cmax < cmin holds no column)
static void check_cols(const std::vector<int> &cols, int cmin, int cmax, int *lo_out, int *n_out)
{
    int lo = -7, n = -7;
    band_cols_range(cols.data(), (int)cols.size(), cmin, cmax, &lo, &n);
    const int lb = (int)(std::lower_bound(cols.begin(), cols.end(), cmin) - cols.begin());
    const int ub = (int)(std::upper_bound(cols.begin(), cols.end(), cmax) - cols.begin());
    CHECK(lo == lb);
    CHECK(n == std::max(0, ub - lb));
    *lo_out = lo;
    *n_out = n;
}

// the column pass' plan for every tile of `tile_px` pixels of an image `width` wide; returns the k-steps of the widest tile
static int check_sep_tiles(const std::vector<int> &cols, int width, int tile_px, int d, int rad, int *dead_blocks, int *part_steps)
{
    const int nc = (int)cols.size();
    int most = 0;
    for (int tc0 = 0; tc0 < width; tc0 += tile_px) {
        int clo = -7, count = -7;
        band_sep_tile_cols(cols.data(), nc, width, tc0, tile_px, d, &clo, &count);
        const int tc1 = std::min(width, tc0 + tile_px) - 1, nks = band_sep_ksteps(count);
        CHECK(count >= 0 && clo >= 0 && clo + count <= nc);
        CHECK(nks * BSEP_KSTEP >= count && (nks - 1) * BSEP_KSTEP < std::max(count, 1));
        most = std::max(most, nks);
        *part_steps += count % BSEP_KSTEP != 0;
        // every column within d of a pixel of the (clipped) tile is an entry of the range, and nothing else is
        for (int b = 0; b < nc; ++b) {
            bool near = false;
            for (int c = tc0; c <= tc1 && !near; ++c) near = std::abs(c - cols[b]) <= d;
            CHECK(near == (b >= clo && b < clo + count));
        }
        uint64_t live_blocks = 0;
        for (int ks = 0; ks < nks; ++ks) {
            // the indices the kernel forms for the 16 entries of the k-step, dead ones included
            for (int j = 0; j < BSEP_KSTEP; ++j) {
                const int i = BSEP_KSTEP * ks + j, b = band_sep_col(clo, i, nc);
                CHECK(b >= 0 && b < nc);
                if (i < count) CHECK(b == clo + i);
            }
            for (int pt = 0; pt < tile_px / 32; ++pt) { // (pixel tiles past the width among them: their lanes compute too)
                const int p0 = tc0 + 32 * pt, p1 = p0 + 31;
                bool any = false;
                for (int i = BSEP_KSTEP * ks; i < std::min(count, BSEP_KSTEP * (ks + 1)); ++i)
                    for (int c = p0; c <= p1; ++c) any = any || std::abs(c - cols[clo + i]) < rad;
                const bool dead = band_sep_block_dead(cols.data(), nc, clo, count, ks, p0, p1, rad);
                CHECK(!dead || !any); // (judged by the k-step's first and last column: a block it keeps may still be all zero)
                if (count >= BSEP_KSTEP * (ks + 1) && cols[clo + BSEP_KSTEP * ks + 15] - cols[clo + BSEP_KSTEP * ks] < rad) CHECK(dead == !any);
                live_blocks += !dead;
                *dead_blocks += dead;
            }
        }
        CHECK(band_sep_tile_entries(cols.data(), nc, width, tc0, tile_px, d, rad, false) == live_blocks * BSEP_KSTEP * 32u);
        CHECK(band_sep_tile_entries(cols.data(), nc, width, tc0, tile_px, d, rad, true) == (uint64_t)nks * (tile_px / 32) * BSEP_KSTEP * 32u);
    }
    return most;
}

int main()
{
    std::mt19937 rng(20240607u);
    int grids = 0, empty_ranges = 0, empty_hulls = 0, closed_circles = 0, sep_most = 0, sep_dead = 0, sep_part = 0;
    for (int trial = 0; trial < 400; ++trial) {
        const int nc = trial % 5 == 0 ? 1 : 1 + (int)(rng() % 40u), nr = trial % 7 == 0 ? 1 : 1 + (int)(rng() % 40u);
        const std::vector<int> cols = ascending(rng, nc, (int)(rng() % 30u), 1 + (int)(rng() % 20u));
        const std::vector<int> rows = ascending(rng, nr, (int)(rng() % 30u), 1 + (int)(rng() % 20u));
        const double D2 = 0.3 + (double)(rng() % 3000u) * (trial % 3 == 0 ? 0.01 : 1.0); // radius 1 .. 55
        BandGeom g;
        CHECK(g.init(rows.data(), nr, cols.data(), nc, 40.5 / D2));
        CHECK(g.rad >= 1 && (int)g.dcmax.size() == g.rad && g.dcmax[0] >= 0);
        ++grids;
        // tiles: inside the grid, straddling its ends, wholly left and wholly right of every column; one pixel wide among them
        const int width = cols.back() + 1 + (int)(rng() % 100u);
        for (int t = 0; t < 24; ++t) {
            int c0, c1;
            if (t == 0) c0 = cols.front() - 3 * g.rad - 70, c1 = c0 + 63;   // left of every column, beyond the radius
            else if (t == 1) c0 = cols.back() + 3 * g.rad + 5, c1 = c0 + 63; // right of every column
            else c0 = (int)(rng() % (unsigned)width) - 10, c1 = c0 + (t % 4 == 0 ? 0 : (int)(rng() % 64u));
            const int ds[4] = {-1, 0, g.dcmax[0], (int)(rng() % 70u)};
            for (int d : ds) {
                int lo, n;
                check_cols(cols, c0 - d, c1 + d, &lo, &n);
                empty_ranges += n == 0;
            }
            if (t < 2) {
                int lo, n;
                check_cols(cols, c0 - g.dcmax[0], c1 + g.dcmax[0], &lo, &n);
                CHECK(n == 0);
            }
            // BandGeom::window is the same interval: in columns (shift 0) and in half-blocks of 8. dcmax[dr] = -1 (the circle ends
            // exactly at dr): no column at all, the guard every caller of band_cols_range has
            for (int dr = 0; dr < g.rad; dr += 1 + dr / 4) {
                int lo, n;
                check_cols(cols, c0 - g.dcmax[dr], c1 + g.dcmax[dr], &lo, &n);
                if (g.dcmax[dr] < 0) n = 0, ++closed_circles;
                const unsigned w0 = g.window(c0, c1, dr, 0), w3 = g.window(c0, c1, dr, BAND_HALF_SHIFT);
                CHECK(w0 == (n > 0 ? (unsigned)lo | ((unsigned)(lo + n - 1) << 16) : BAND_EMPTY));
                CHECK(w3 == (n > 0 ? (unsigned)(lo >> 3) | ((unsigned)((lo + n - 1) >> 3) << 16) : BAND_EMPTY));
                CHECK(band_win_live(w0) == (n > 0));
            }
        }
        // the hull of a block of target rows against a brute-force walk over the grid rows; image rows far below the last grid row
        // have no band
        const int height = rows.back() + 3 * g.rad + 20;
        std::vector<unsigned> rowband(height);
        for (int r = 0; r < height; ++r) rowband[r] = g.band_of(r);
        for (int t = 0; t < 24; ++t) {
            const int n = t == 0 ? 0 : 1 + (int)(rng() % (unsigned)BAND_NW);
            const int r0 = t == 1 ? height - n : (int)(rng() % (unsigned)(height - n + 1));
            int alo = -7, ahi = -7, blo = 0xFFFF, bhi = -1;
            band_rows_hull(rowband.data(), r0, n, &alo, &ahi);
            for (int r = r0; r < r0 + n; ++r)
                for (int a = 0; a < nr; ++a)
                    if (std::abs(r - rows[a]) < g.rad) {
                        blo = std::min(blo, a);
                        bhi = std::max(bhi, a);
                    }
            CHECK(alo == blo && ahi == bhi);
            empty_hulls += ahi < alo;
        }
        // the column pass' k-steps: the trial's own grid and radius (often larger than the image), tiles of 64, 128 and 256 pixels
        // over a width that is no multiple of them; d = -1 (no column at all) among the distances
        for (int tile_px : {64, 128, 256}) {
            const int w2 = trial % 2 ? width : cols.back() + 1; // (the last column on the last pixel: the range clipped at the right edge)
            for (int d : {g.dcmax[0], -1, 0}) {
                const int most = check_sep_tiles(cols, w2, tile_px, d, g.rad, &sep_dead, &sep_part);
                if (d < 0) CHECK(most == 0);
                sep_most = std::max(sep_most, most);
            }
        }
    }
    // dense grids under a small radius: three and more k-steps per tile, ranges that start past column 0 and end before the last one
    for (int trial = 0; trial < 60; ++trial) {
        const int nc = 16 + (int)(rng() % 200u);
        const std::vector<int> cols = ascending(rng, nc, (int)(rng() % 4u), 1 + (int)(rng() % 3u));
        const std::vector<int> rows = ascending(rng, 3, 0, 5);
        const int rad_want = 8 + (int)(rng() % 60u);
        BandGeom g;
        CHECK(g.init(rows.data(), 3, cols.data(), nc, 40.5 / ((double)rad_want * rad_want)));
        for (int tile_px : {64, 128, 256}) sep_most = std::max(sep_most, check_sep_tiles(cols, cols.back() + 1 + (int)(rng() % 70u), tile_px, g.dcmax[0], g.rad, &sep_dead, &sep_part));
    }
    CHECK(sep_most >= 3 && sep_dead > 0 && sep_part > 0);
    CHECK(empty_ranges > 0 && empty_hulls > 0 && closed_circles > 0);
    if (failures) {
        std::fprintf(stderr, "band_plan_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("band_plan_check: %d grids, %d empty column ranges, %d empty hulls; column pass: up to %d k-steps, %d dead blocks: ok\n", grids,
                empty_ranges, empty_hulls, sep_most, sep_dead);
    return 0;
}
