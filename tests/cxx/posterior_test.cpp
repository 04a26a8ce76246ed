// Drives MOIHGPRegression::predictPosterior (include/moihgp_cxx/moihgp_regression.hpp) for tests/test_posterior.py.
// stdin: kern M L dt nticks | params[np] | Y[nticks][M] | nvar | ticks[nvar]   (kern 0 = Matern-3/2, 1 = Matern-5/2; NaN = missing output)
// stdout: the posterior means of the outputs, one tick per line, the output variances, one requested tick per line, and the latents' nll on one line.
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
    int nt, nv;
    if (scanf("%d", &nt) != 1) return 2;
    moihgp::MOIHGPRegression<SS> reg(dt, M, L, (size_t)nt, false);
    Vec p0(reg.getNumParam()), g;
    if (!rd(p0)) return 2;
    std::vector<Vec> Y((size_t)nt, Vec(M));
    for (auto& y : Y) if (!rd(y)) return 2;
    if (scanf("%d", &nv) != 1) return 2;
    std::vector<long> ticks((size_t)nv);
    for (auto& t : ticks) if (scanf("%ld", &t) != 1) return 2;
    reg.objective().apply_params = true;
    reg.objective()(p0, g);                                        // installs p0 (update) without fitting
    std::vector<Vec> varY;
    Vec nll;
    for (const Vec& ys : reg.predictPosterior(Y, ticks, &varY, &nll)) {
        for (double e : ys) printf("%.17g ", e);
        printf("\n");
    }
    for (const Vec& v : varY) {
        for (double e : v) printf("%.17g ", e);
        printf("\n");
    }
    for (double e : nll) printf("%.17g ", e);
    printf("\n");
    return 0;
}

int main() {
    int kern; size_t M, L; double dt;
    if (scanf("%d %zu %zu %lf", &kern, &M, &L, &dt) != 4) return 2;
    return kern == 0 ? run<moihgp::Matern32StateSpace>(M, L, dt) : run<moihgp::Matern52StateSpace>(M, L, dt);
}
