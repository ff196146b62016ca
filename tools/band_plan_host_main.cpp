// Stand-alone check of the window plan the three forms of the fused band filter share (band_plan.hpp: band_rows_hull, band_cols_range)
// and of BandGeom::window / band_of beside them: built together with host_util.cpp under the address and undefined-behaviour
// sanitizers by `make band_plan_check`. CPU only; no device, no python.
// A few hundred random ascending grids in exactly sized heap buffers (one element too far is reported), one-column grids among them;
// tiles inside the grid, wholly left and wholly right of every column; d = -1 (a range narrower than the tile, inverted for one
// pixel; as dcmax[dr] it means no column at all, which the callers' guard and BandGeom::window decide); blocks of rows that no
// band reaches.
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

int main()
{
    std::mt19937 rng(20240607u);
    int grids = 0, empty_ranges = 0, empty_hulls = 0, closed_circles = 0;
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
    }
    CHECK(empty_ranges > 0 && empty_hulls > 0 && closed_circles > 0);
    if (failures) {
        std::fprintf(stderr, "band_plan_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("band_plan_check: %d grids, %d empty column ranges, %d empty hulls: ok\n", grids, empty_ranges, empty_hulls);
    return 0;
}
