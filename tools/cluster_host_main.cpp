// Stand-alone check of the host-only half of the spectral segmentation (glf_cluster_seed, glf_cluster_update and their weighted
// forms glf_cluster_seed_w, glf_cluster_update_w): built together
// with host_util.cpp under the address and undefined-behaviour sanitizers by `make cluster_check`. CPU only; no device, no python.
// It walks the edges where an index could leave its array: n = k, k = 1, duplicate rows, the refusals, empty clusters, cent
// aliasing cent_prev, and exactly sized heap buffers so that one element too far is reported.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/glf.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// the restatement of the seeding rule on the uniforms glf_random_vectors exposes
static std::vector<size_t> seed_rule(const std::vector<double> &rows, size_t n, unsigned dim, unsigned k, uint64_t seed)
{
    std::vector<double> u(k);
    glf_random_vectors(u.data(), k, 1, seed);
    std::vector<size_t> pick{(size_t)(u[0] * (double)n)};
    std::vector<double> d2(n, INFINITY);
    for (unsigned t = 1; t < k; ++t) {
        double total = 0.0;
        for (size_t i = 0; i < n; ++i) {
            double d = 0.0;
            for (unsigned q = 0; q < dim; ++q) d += (rows[i * dim + q] - rows[pick.back() * dim + q]) * (rows[i * dim + q] - rows[pick.back() * dim + q]);
            d2[i] = d < d2[i] ? d : d2[i];
            total += d2[i];
        }
        double run = 0.0;
        size_t i = 0;
        for (; i < n; ++i) {
            run += d2[i];
            if (run > u[t] * total) break;
        }
        pick.push_back(i);
    }
    return pick;
}

int main()
{
    // lattice points: every distance and running sum is exact
    for (unsigned dim : {1u, 3u, 64u})
        for (size_t n : {(size_t)1, (size_t)5, (size_t)32, (size_t)257})
            for (unsigned k : {1u, 2u, 5u, 32u}) {
                if (k > n) continue;
                std::vector<double> rows(n * dim);
                for (size_t i = 0; i < n; ++i)
                    for (unsigned q = 0; q < dim; ++q) rows[i * dim + q] = (double)((i * 7 + q * 3 + (i * i) % 5) % 11) + (q == 0 ? 16.0 * (double)i : 0.0);
                for (uint64_t seed : {(uint64_t)0, (uint64_t)1, (uint64_t)12345}) {
                    std::vector<double> cent((size_t)k * dim, -1.0);
                    CHECK(glf_cluster_seed(rows.data(), n, dim, k, seed, cent.data()) == GLF_OK);
                    const std::vector<size_t> want = seed_rule(rows, n, dim, k, seed);
                    for (unsigned t = 0; t < k; ++t)
                        for (unsigned q = 0; q < dim; ++q) CHECK(cent[(size_t)t * dim + q] == rows[want[t] * dim + q]);
                }
            }
    {   // duplicates: 3 distinct rows among 6
        const std::vector<double> rows{1, 1, 2, 2, 1, 1, 3, 3, 2, 2, 3, 3};
        std::vector<double> cent(8, -7.0);
        CHECK(glf_cluster_seed(rows.data(), 6, 2, 3, 4, cent.data()) == GLF_OK);
        CHECK(glf_cluster_seed(rows.data(), 6, 2, 4, 4, cent.data()) == GLF_ERR_INVALID);
        CHECK(cent[6] == -7.0 && cent[7] == -7.0);
        std::vector<double> one(2, -7.0);
        CHECK(glf_cluster_seed(rows.data(), 6, 2, 7, 4, cent.data()) == GLF_ERR_INVALID); // k > n
        CHECK(glf_cluster_seed(rows.data(), 0, 2, 1, 4, one.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed(rows.data(), 6, 0, 1, 4, one.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed(rows.data(), 6, 2, 0, 4, one.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed(nullptr, 6, 2, 1, 4, one.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed(rows.data(), 6, 2, 1, 4, nullptr) == GLF_ERR_INVALID);
        CHECK(one[0] == -7.0 && one[1] == -7.0);
        std::vector<double> bad(rows);
        bad[5] = NAN;
        CHECK(glf_cluster_seed(bad.data(), 6, 2, 2, 4, cent.data()) == GLF_ERR_INVALID);
    }
    {   // update: means, scale, an empty cluster, in place
        const unsigned k = 3, dim = 2;
        const std::vector<double> sums{2, 4, 0, 0, 9, 3}, scale{2, 0}, prev{5, 6, 7, 8, 9, 10};
        const std::vector<uint64_t> counts{2, 0, 3};
        std::vector<double> cent(6, -1.0);
        CHECK(glf_cluster_update(k, dim, scale.data(), sums.data(), counts.data(), prev.data(), cent.data()) == GLF_OK);
        CHECK(cent[0] == 2.0 && cent[1] == 0.0 && cent[2] == 7.0 && cent[3] == 8.0 && cent[4] == 6.0 && cent[5] == 0.0);
        std::vector<double> inplace(prev);
        CHECK(glf_cluster_update(k, dim, nullptr, sums.data(), counts.data(), inplace.data(), inplace.data()) == GLF_OK);
        CHECK(inplace[0] == 1.0 && inplace[1] == 2.0 && inplace[2] == 7.0 && inplace[3] == 8.0 && inplace[4] == 3.0 && inplace[5] == 1.0);
        std::vector<double> keep(6, -1.0);
        CHECK(glf_cluster_update(k, dim, nullptr, sums.data(), counts.data(), nullptr, keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update(0, dim, nullptr, sums.data(), counts.data(), prev.data(), keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update(k, 0, nullptr, sums.data(), counts.data(), prev.data(), keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update(k, dim, nullptr, nullptr, counts.data(), prev.data(), keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update(k, dim, nullptr, sums.data(), nullptr, prev.data(), keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update(k, dim, nullptr, sums.data(), counts.data(), prev.data(), nullptr) == GLF_ERR_INVALID);
        for (double x : keep) CHECK(x == -1.0);
    }
    // weighted seeding: w NULL and w = 1 ... on lattice points, doubled weights, zero weights, the refusals
    for (unsigned dim : {1u, 3u, 64u})
        for (size_t n : {(size_t)1, (size_t)5, (size_t)32, (size_t)257})
            for (unsigned k : {1u, 2u, 5u, 32u}) {
                if (k > n) continue;
                std::vector<double> rows(n * dim), w(n), w2(n);
                for (size_t i = 0; i < n; ++i) {
                    for (unsigned q = 0; q < dim; ++q) rows[i * dim + q] = (double)((i * 7 + q * 3 + (i * i) % 5) % 11) + (q == 0 ? 16.0 * (double)i : 0.0);
                    w[i] = (double)(1 + (i * 5) % 4); // small integers: every running sum is exact
                    w2[i] = 2.0 * w[i];
                }
                for (uint64_t seed : {(uint64_t)0, (uint64_t)1, (uint64_t)12345}) {
                    std::vector<double> plain((size_t)k * dim, -1.0), viaw((size_t)k * dim, -2.0), a((size_t)k * dim, -3.0), b((size_t)k * dim, -4.0);
                    CHECK(glf_cluster_seed(rows.data(), n, dim, k, seed, plain.data()) == GLF_OK);
                    CHECK(glf_cluster_seed_w(rows.data(), nullptr, n, dim, k, seed, viaw.data()) == GLF_OK);
                    CHECK(plain == viaw);
                    CHECK(glf_cluster_seed_w(rows.data(), w.data(), n, dim, k, seed, a.data()) == GLF_OK);
                    CHECK(glf_cluster_seed_w(rows.data(), w2.data(), n, dim, k, seed, b.data()) == GLF_OK);
                    CHECK(a == b);
                    for (unsigned t = 0; t < k; ++t) { // every centre is one of the rows, and no row is taken twice
                        size_t hits = 0;
                        for (size_t i = 0; i < n; ++i) hits += a[(size_t)t * dim] == rows[i * dim];
                        CHECK(hits == 1);
                        for (unsigned t2 = 0; t2 < t; ++t2) CHECK(a[(size_t)t * dim] != a[(size_t)t2 * dim]);
                    }
                }
            }
    {   // rows of weight 0 are never chosen; too few rows of positive weight, bad weights and a zero total are refused
        const std::vector<double> rows{0, 0, 1, 0, 2, 0, 3, 0, 4, 0, 5, 0};
        const std::vector<double> w{0, 1, 0, 2, 0, 0};
        for (uint64_t seed = 0; seed < 16; ++seed) {
            std::vector<double> cent(4, -7.0);
            CHECK(glf_cluster_seed_w(rows.data(), w.data(), 6, 2, 2, seed, cent.data()) == GLF_OK);
            CHECK((cent[0] == 1.0 && cent[2] == 3.0) || (cent[0] == 3.0 && cent[2] == 1.0));
            std::vector<double> one(2, -7.0);
            CHECK(glf_cluster_seed_w(rows.data(), w.data(), 6, 2, 1, seed, one.data()) == GLF_OK);
            CHECK(one[0] == 1.0 || one[0] == 3.0);
        }
        std::vector<double> keep(6, -7.0);
        CHECK(glf_cluster_seed_w(rows.data(), w.data(), 6, 2, 3, 1, keep.data()) == GLF_ERR_INVALID); // only 2 rows carry weight
        std::vector<double> bad(w);
        bad[2] = -1.0;
        CHECK(glf_cluster_seed_w(rows.data(), bad.data(), 6, 2, 2, 1, keep.data()) == GLF_ERR_INVALID);
        bad[2] = NAN;
        CHECK(glf_cluster_seed_w(rows.data(), bad.data(), 6, 2, 2, 1, keep.data()) == GLF_ERR_INVALID);
        bad[2] = INFINITY;
        CHECK(glf_cluster_seed_w(rows.data(), bad.data(), 6, 2, 2, 1, keep.data()) == GLF_ERR_INVALID);
        const std::vector<double> zero(6, 0.0);
        CHECK(glf_cluster_seed_w(rows.data(), zero.data(), 6, 2, 1, 1, keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed_w(nullptr, w.data(), 6, 2, 1, 1, keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed_w(rows.data(), w.data(), 6, 2, 1, 1, nullptr) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed_w(rows.data(), w.data(), 0, 2, 1, 1, keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed_w(rows.data(), w.data(), 6, 0, 1, 1, keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed_w(rows.data(), w.data(), 6, 2, 0, 1, keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_seed_w(rows.data(), w.data(), 6, 2, 7, 1, keep.data()) == GLF_ERR_INVALID);
        for (double x : keep) CHECK(x == -7.0);
    }
    {   // weighted update: means by mass, scale, a cluster of mass 0 (and of NaN mass) keeps its centroid, in place
        const unsigned k = 3, dim = 2;
        const std::vector<double> sums{2, 4, 5, 5, 9, 3}, scale{2, 0}, prev{5, 6, 7, 8, 9, 10};
        const std::vector<double> mass{0.5, 0.0, 3.0};
        std::vector<double> cent(6, -1.0);
        CHECK(glf_cluster_update_w(k, dim, scale.data(), sums.data(), mass.data(), prev.data(), cent.data()) == GLF_OK);
        CHECK(cent[0] == 8.0 && cent[1] == 0.0 && cent[2] == 7.0 && cent[3] == 8.0 && cent[4] == 6.0 && cent[5] == 0.0);
        std::vector<double> inplace(prev);
        CHECK(glf_cluster_update_w(k, dim, nullptr, sums.data(), mass.data(), inplace.data(), inplace.data()) == GLF_OK);
        CHECK(inplace[0] == 4.0 && inplace[1] == 8.0 && inplace[2] == 7.0 && inplace[3] == 8.0 && inplace[4] == 3.0 && inplace[5] == 1.0);
        const std::vector<double> nanmass{0.5, NAN, 3.0};
        std::vector<double> c2(6, -1.0);
        CHECK(glf_cluster_update_w(k, dim, nullptr, sums.data(), nanmass.data(), prev.data(), c2.data()) == GLF_OK);
        CHECK(c2[2] == 7.0 && c2[3] == 8.0);
        std::vector<double> keep(6, -1.0);
        CHECK(glf_cluster_update_w(k, dim, nullptr, sums.data(), mass.data(), nullptr, keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update_w(k, dim, nullptr, sums.data(), nanmass.data(), nullptr, keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update_w(0, dim, nullptr, sums.data(), mass.data(), prev.data(), keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update_w(k, 0, nullptr, sums.data(), mass.data(), prev.data(), keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update_w(k, dim, nullptr, nullptr, mass.data(), prev.data(), keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update_w(k, dim, nullptr, sums.data(), nullptr, prev.data(), keep.data()) == GLF_ERR_INVALID);
        CHECK(glf_cluster_update_w(k, dim, nullptr, sums.data(), mass.data(), prev.data(), nullptr) == GLF_ERR_INVALID);
        for (double x : keep) CHECK(x == -1.0);
    }
    if (failures) {
        std::fprintf(stderr, "cluster_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("cluster_host_check: ok\n");
    return 0;
}
