// C++ test of icebin::VectorMultivec (icebin_amd/host/icebin_hip.hpp): add, append_weighted from a 3-row matrix's product,
// to_dense_scale and to_dense on one small case, against the reference's loops (multivec.cpp:35-81) run here on the same numbers.
// Exit code 0 = pass, 3 = no GPU (the no-fallback error path was verified instead).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "host_test.h"

using namespace icebin;

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

int main() {
    const int nvar = 2, nE = 6;
    try {
        VectorMultivec mv(nvar);
        REQUIRE(mv.nvar() == nvar && mv.size() == 0);
        mv.add(4, std::vector<double>{1.5, -2.0}, 0.25);
        const double v1[2] = {std::numeric_limits<double>::quiet_NaN(), 8.0};
        mv.add(1, v1, 3.0);

        // a 3 x 3 diagonal matrix: dims are identities, wM as given; its field-major product B[ivar][row]
        const int32_t rc[3] = {0, 1, 2};
        const double ones[3] = {1., 1., 1.}, wM[3] = {0.5, 0.75, 2.0};
        ibh_weighted *h = nullptr;
        check(ibh_weighted_from_coo(3, 3, 3, rc, rc, ones, wM, ones, 1, 0, &h));
        linear::Weighted M(h);
        const double B[2][4] = {{0.1, 0.2, 0.3, -7.}, {10., 20., 30., -7.}};      // row stride 4
        mv.append_weighted(M, &B[0][0], nvar, 4);
        REQUIRE(mv.size() == 5);

        const std::vector<long> index = mv.index();
        const std::vector<double> weights = mv.weights(), vals = mv.vals();
        const long want_index[5] = {4, 1, 0, 1, 2};
        const double want_w[5] = {0.25, 3.0, 0.5, 0.75, 2.0};
        const double want_v[10] = {1.5, -2.0, v1[0], 8.0, 0.1, 10., 0.2, 20., 0.3, 30.};
        for (int i = 0; i < 5; ++i) REQUIRE(index[i] == want_index[i] && same_bits(weights[i], want_w[i]));
        for (int i = 0; i < 10; ++i) REQUIRE(same_bits(vals[i], want_v[i]));
        REQUIRE(same_bits(mv.val(1, 3), 20.));

        // multivec.cpp:35-50
        std::vector<double> want_scale(nE, 0.0), scale(nE, -1.0);
        for (int i = 0; i < 5; ++i) want_scale[want_index[i]] += want_w[i];
        for (int iE = 0; iE < nE; ++iE) want_scale[iE] = 1. / want_scale[iE];
        mv.to_dense_scale(scale);
        for (int iE = 0; iE < nE; ++iE) REQUIRE(same_bits(scale[iE], want_scale[iE]));
        REQUIRE(std::isinf(scale[3]) && std::isinf(scale[5]));

        // multivec.cpp:55-81, one variable at a time and all at once
        const double fill = -9.0;
        const std::vector<double> all = mv.to_dense(scale, fill);
        for (int ivar = 0; ivar < nvar; ++ivar) {
            std::vector<double> want(nE, std::numeric_limits<double>::quiet_NaN()), got(nE, 0.0);
            for (int i = 0; i < 5; ++i) {
                const long iE = want_index[i];
                const double p = want_v[i * nvar + ivar] * want_scale[iE];
                if (std::isnan(want[iE])) want[iE] = p; else want[iE] += p;
            }
            for (int iE = 0; iE < nE; ++iE) if (std::isnan(want[iE])) want[iE] = fill;
            mv.to_dense(ivar, scale, fill, got);
            for (int iE = 0; iE < nE; ++iE) REQUIRE(same_bits(got[iE], want[iE]) && same_bits(all[ivar * nE + iE], want[iE]));
        }

        VectorMultivec other(nvar);
        other.add(5, std::vector<double>{1., 2.}, 1.0);
        VectorMultivec cat = concatenate({&mv, &other});
        REQUIRE(cat.size() == 6 && cat.index()[5] == 5);
        VectorMultivec three(3);
        try { concatenate({&mv, &three}); REQUIRE(false); }
        catch (Exception const &e) { REQUIRE(e.code == IBH_EINVAL && std::strstr(e.what(), "nvar") != nullptr); }
        std::vector<double> too_short(4);
        try { cat.to_dense_scale(too_short); REQUIRE(false); }
        catch (Exception const &e) { REQUIRE(e.code == IBH_EINVAL && std::strstr(e.what(), "entry 0") != nullptr); }
        SparseSetT dimE0;
        cat.add_dense_to(dimE0);
        REQUIRE(dimE0.dense_extent() == 5 && dimE0.to_sparse(0) == 4 && dimE0.to_sparse(1) == 1 && dimE0.to_sparse(4) == 5);
    } catch (std::exception const &e) {
        if (std::strstr(e.what(), "no CPU fallback")) { std::printf("no GPU: %s\n", e.what()); return 3; }
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
