// Drives MOIHGPRegression::predictLagged (include/moihgp_cxx/moihgp_regression.hpp) for tests/test_lagged.py.
// stdin: kern M L dt lag nticks | params[np] | Y[nticks][M]   (kern 0 = Matern-3/2, 1 = Matern-5/2; NaN = missing output)
// stdout: the outputs smoothed with the fixed lag at every tick, one tick per line.
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
    int lag, nt;
    if (scanf("%d %d", &lag, &nt) != 2) return 2;
    moihgp::MOIHGPRegression<SS> reg(dt, M, L, (size_t)nt, false);
    Vec p0(reg.getNumParam()), g;
    if (!rd(p0)) return 2;
    std::vector<Vec> Y((size_t)nt, Vec(M));
    for (auto& y : Y) if (!rd(y)) return 2;
    reg.objective().apply_params = true;
    reg.objective()(p0, g);                                        // installs p0 (update) without fitting
    for (const Vec& ys : reg.predictLagged(Y, lag)) {
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
