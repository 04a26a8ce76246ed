// Drives MOIHGPRegression::predictSlope (include/moihgp_cxx/moihgp_regression.hpp) for tests/test_slope.py.
// stdin: kern M L dt frac past nticks | params[np] | Y[nticks][M]   (kern 0 = Matern-3/2, 1 = Matern-5/2; past 0 / 1; NaN = missing output)
// stdout: the outputs' rate of change at time (t + frac) dt for every tick t, one tick per line.  A frac outside [0, 1) must throw
// std::invalid_argument before anything runs: the program then prints "invalid_argument" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
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
    double frac; int past, nt;
    if (scanf("%lf %d %d", &frac, &past, &nt) != 3) return 2;
    moihgp::MOIHGPRegression<SS> reg(dt, M, L, (size_t)nt, false);
    Vec p0(reg.getNumParam()), g;
    if (!rd(p0)) return 2;
    std::vector<Vec> Y((size_t)nt, Vec(M));
    for (auto& y : Y) if (!rd(y)) return 2;
    reg.objective().apply_params = true;
    reg.objective()(p0, g);                                        // installs p0 (update) without fitting
    try {
        for (const Vec& ys : reg.predictSlope(Y, frac, past != 0)) {
            for (double e : ys) printf("%.17g ", e);
            printf("\n");
        }
    } catch (const std::invalid_argument&) {
        printf("invalid_argument\n");
    }
    return 0;
}

int main() {
    int kern; size_t M, L; double dt;
    if (scanf("%d %zu %zu %lf", &kern, &M, &L, &dt) != 4) return 2;
    return kern == 0 ? run<moihgp::Matern32StateSpace>(M, L, dt) : run<moihgp::Matern52StateSpace>(M, L, dt);
}
