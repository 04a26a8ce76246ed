// Drives MOIHGPRegression::samplePathsAhead (include/moihgp_cxx/moihgp_regression.hpp) for tests/test_forecast_paths.py.
// stdin: kern M L dt nticks nahead nsamples seed | params[np] | Y[nticks][M]   (kern 0 = Matern-3/2, 1 = Matern-5/2; NaN = missing output)
// stdout: the paths, one tick ahead per line, sample after sample.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "moihgp_cxx/moihgp_regression.hpp"

using Vec = std::vector<double>;
static bool rd(Vec& v) {
    char tok[64];
    for (auto& e : v) {
        if (scanf("%63s", tok) != 1) return false;
        e = (!strcmp(tok, "nan") || !strcmp(tok, "NaN")) ? NAN : strtod(tok, nullptr);
    }
    return true;
}

template <class SS> int run(size_t M, size_t L, double dt) {
    int nt, na, ns;
    unsigned long long seed;
    if (scanf("%d %d %d %llu", &nt, &na, &ns, &seed) != 4) return 2;
    moihgp::MOIHGPRegression<SS> reg(dt, M, L, (size_t)nt, false);
    Vec p0(reg.getNumParam()), g;
    if (!rd(p0)) return 2;
    std::vector<Vec> Y((size_t)nt, Vec(M));
    for (auto& y : Y) if (!rd(y)) return 2;
    reg.objective().apply_params = true;
    reg.objective()(p0, g);                                        // installs p0 (update) without fitting
    for (const std::vector<Vec>& plane : reg.samplePathsAhead(Y, (size_t)na, (size_t)ns, seed))
        for (const Vec& ys : plane) {
            for (double e : ys) printf("%.17g ", e);
            printf("\n");
        }
    return 0;
}

int main() {
    int kern; size_t M, L; double dt;
    if (scanf("%d %zu %zu %lf", &kern, &M, &L, &dt) != 4) return 2;
    return kern == 0 ? run<moihgp::Matern32StateSpace>(M, L, dt) : run<moihgp::Matern52StateSpace>(M, L, dt);
}
