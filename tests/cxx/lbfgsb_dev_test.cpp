// Drives moihgp::opt::DevLBFGSBSolver and DevBFGSMat (include/moihgp_cxx/lbfgsb_dev.hpp) next to the host LBFGSBSolver / BFGSMat
// (lbfgsb.hpp) on analytic problems; tests/test_device_learner.py feeds the cases.  Linked with libmoihgp the vectors live on the GPU;
// linked with tests/cxx/dvec_cpu.cpp instead, the same program runs on the CPU with the summation order of the reductions chosen by `order`.
// The objective is evaluated on the host in both solvers (download, evaluate, upload on the device side), so only the vector arithmetic
// differs; the host solver runs in a second thread and hands every evaluation point over, so that each one is compared and none is stored.
// Modes (first token on stdin):
//   solve prob n maxit order dump
//        prob 0: Rosenbrock, box [-2, 2], ub[0] = 0.5, x0 = 0   1: tridiagonal quadratic, box [-0.7, 0.9], x0 = 0
//             2: separable quadratic sum 0.5 c_i (x_i - t_i)^2, c_i = 1 + i % 97, t_i = 1.5 sin(0.37 (i % 1013)), box [-0.7, 0.9], x0 = 0
//        solver: m = 6, epsilon = 1e-10, epsilon_rel = 0, past = 0, max_iterations = maxit (0: 300, which no problem here comes near)
//        -> "host iterations evaluations fx" | "dev iterations evaluations fx" | "points compared worst|x_host - x_dev| unmatched" | backend
//           and, when `dump` is not "-", the two final iterates as raw doubles in that file (host's, then the device solver's)
//   bfgs n order
//        m = 4, 7 corrections (the cyclic storage wraps).  Per leg "name err_dev err_host scale outside": largest |dev - ld|, |host - ld|
//        against a long-double two-loop recursion, the largest |ld| entry, and the number of non-zero device entries outside the mask.
//        Then "copy <1 if a copy taken before reset() still gives the same bits>".
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>
#include "moihgp_cxx/lbfgsb_dev.hpp"

using moihgp::opt::Vector;
using moihgp::opt::DVec;
using moihgp::opt::DevOps;

extern "C" int dvec_cpu_order __attribute__((weak));      // defined by dvec_cpu.cpp only

struct Rosenbrock {
    double operator()(const Vector& x, Vector& g) {
        const size_t n = x.size();
        double f = 0.0;
        for (size_t i = 0; i < n; i++) g[i] = 0.0;
        for (size_t i = 0; i + 1 < n; i++) {
            const double a = x[i + 1] - x[i] * x[i], b = 1.0 - x[i];
            f += 100.0 * a * a + b * b;
            g[i] += -400.0 * a * x[i] - 2.0 * b;
            g[i + 1] += 200.0 * a;
        }
        return f;
    }
};
struct Quadratic {            // f = 1/2 x'Ax - b'x,  A = tridiag(-1, 2.5, -1),  b_i = 3 sin(i + 1)   (as tests/cxx/lbfgsb_test.cpp)
    double operator()(const Vector& x, Vector& g) {
        const size_t n = x.size();
        if (b.size() != n) { b.resize(n); for (size_t i = 0; i < n; i++) b[i] = 3.0 * std::sin((double)(i + 1)); }
        double f = 0.0;
        for (size_t i = 0; i < n; i++) {
            const double ax = 2.5 * x[i] - (i > 0 ? x[i - 1] : 0.0) - (i + 1 < n ? x[i + 1] : 0.0);
            g[i] = ax - b[i];
            f += 0.5 * x[i] * ax - b[i] * x[i];
        }
        return f;
    }
    Vector b;
};
struct Separable {
    double operator()(const Vector& x, Vector& g) {
        const size_t n = x.size();
        if (t.size() != n) { t.resize(n); for (size_t i = 0; i < n; i++) t[i] = 1.5 * std::sin(0.37 * (double)(i % 1013)); }
        double f = 0.0;
        for (size_t i = 0; i < n; i++) {
            const double c = 1.0 + (double)(i % 97), d = x[i] - t[i];
            g[i] = c * d;
            f += 0.5 * c * d * d;
        }
        return f;
    }
    Vector t;
};

// the host solver's evaluation points, handed to the device side one by one
struct Trace {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Vector> q;
    bool done = false;
    void push(const Vector& x) {
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return q.size() < 2; });
        q.push_back(x);
        cv.notify_all();
    }
    void finish() { std::lock_guard<std::mutex> lock(mu); done = true; cv.notify_all(); }
    bool pop(Vector& x) {
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [&] { return !q.empty() || done; });
        if (q.empty()) return false;
        x.swap(q.front());
        q.pop_front();
        cv.notify_all();
        return true;
    }
};
template <class F> struct HostSide {
    F f; Trace* tr; long evals = 0;
    double operator()(const Vector& x, Vector& g) { evals++; tr->push(x); return f(x, g); }
};
template <class F> struct DevSide {
    F f; Trace* tr; DevOps* ops; long evals = 0, compared = 0, unmatched = 0; double worst = 0.0;
    Vector hx, hg, ref;
    double operator()(const DVec& x, DVec& grad) {
        evals++;
        ops->download(x, hx);
        if (tr->pop(ref) && ref.size() == hx.size()) {
            compared++;
            for (size_t i = 0; i < hx.size(); i++) { const double d = std::fabs(hx[i] - ref[i]); if (!(d <= worst)) worst = d; }    // (a NaN stays)
        } else unmatched++;
        hg.resize(hx.size());
        const double fx = f(hx, hg);
        ops->upload(hg, grad);
        return fx;
    }
};

template <class F> int solve(int prob, size_t n, int maxit, const char* dump) {
    Vector lb(n, prob == 0 ? -2.0 : -0.7), ub(n, prob == 0 ? 2.0 : 0.9), x0(n, 0.0);
    if (prob == 0) ub[0] = 0.5;
    moihgp::opt::LBFGSBParam prm;
    prm.m = 6; prm.epsilon = 1e-10; prm.epsilon_rel = 0.0; prm.past = 0; prm.max_iterations = maxit ? maxit : 300;       // (the uncapped problems take 22, 16 and 124; the cap ends a run whose kernels are wrong)
    Trace tr;
    HostSide<F> hs{F(), &tr};
    Vector xh = x0;
    double fh = 0.0; int ith = 0;
    std::thread host([&] {
        moihgp::opt::LBFGSBSolver solver(prm);
        ith = solver.minimize(hs, xh, fh, lb, ub);
        tr.finish();
    });
    DevOps ops;
    DevSide<F> ds{F(), &tr, &ops};
    DVec x, dlb, dub;
    ops.upload(x0, x); ops.upload(lb, dlb); ops.upload(ub, dub);
    double fd = 0.0; int itd = -1;
    try {
        moihgp::opt::DevLBFGSBSolver solver(prm, &ops);
        itd = solver.minimize(ds, x, fd, dlb, dub);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); }
    Vector rest;
    while (tr.pop(rest)) ds.unmatched++;                           // (also lets the host thread end when the device side stopped early)
    host.join();
    if (itd < 0) return 3;
    Vector xd;
    ops.download(x, xd);
    printf("host %d %ld %.17g\n", ith, hs.evals, fh);
    printf("dev %d %ld %.17g\n", itd, ds.evals, fd);
    printf("points %ld %.17g %ld\n", ds.compared, ds.worst, ds.unmatched);
    printf("%s\n", &dvec_cpu_order ? "cpu" : "device");
    if (strcmp(dump, "-")) {
        FILE* fp = fopen(dump, "wb");
        if (!fp) return 4;
        fwrite(xh.data(), sizeof(double), n, fp); fwrite(xd.data(), sizeof(double), n, fp);
        fclose(fp);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------- BFGS matrix
static unsigned long long g_lcg = 0x2545F4914F6CDD1DULL;
static double unif() { g_lcg = g_lcg * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(g_lcg >> 11) / 9007199254740992.0 * 2.0 - 1.0; }

// a H v in long double over the stored pairs (newest last); mask == nullptr: apply_Hv (theta of the newest pair, no pair skipped);
// otherwise apply_Hv_free (pairs with s.y <= eps y.y on the face skipped, theta from the newest one kept)
static std::vector<long double> two_loop_ld(const std::vector<Vector>& S, const std::vector<Vector>& Y, const Vector& v, double a, const std::vector<char>* mask) {
    const size_t n = v.size(), k = S.size();
    auto in = [&](size_t q) { return !mask || (*mask)[q]; };
    std::vector<long double> r(n), alpha(k, 0.0L), ys(k, 0.0L);
    std::vector<char> use(k, 1);
    for (size_t q = 0; q < n; q++) r[q] = in(q) ? (long double)a * v[q] : 0.0L;
    long double theta = 1.0L;
    bool have = false;
    for (size_t j = k; j-- > 0;) {
        long double yy = 0.0L, sr = 0.0L;
        for (size_t q = 0; q < n; q++) if (in(q)) { ys[j] += (long double)S[j][q] * Y[j][q]; yy += (long double)Y[j][q] * Y[j][q]; }
        if (mask) use[j] = ys[j] > (long double)std::numeric_limits<double>::epsilon() * yy;
        if (!use[j]) continue;
        if (!have) { theta = yy / ys[j]; have = true; }
        for (size_t q = 0; q < n; q++) if (in(q)) sr += (long double)S[j][q] * r[q];
        alpha[j] = sr / ys[j];
        for (size_t q = 0; q < n; q++) if (in(q)) r[q] -= alpha[j] * Y[j][q];
    }
    for (size_t q = 0; q < n; q++) r[q] /= theta;
    for (size_t j = 0; j < k; j++) {
        if (!use[j]) continue;
        long double b = 0.0L;
        for (size_t q = 0; q < n; q++) if (in(q)) b += (long double)Y[j][q] * r[q];
        b /= ys[j];
        for (size_t q = 0; q < n; q++) if (in(q)) r[q] += (alpha[j] - b) * S[j][q];
    }
    return r;
}

static void leg(const char* name, const Vector& dev, const Vector& host, const std::vector<long double>& ld, const std::vector<char>* mask) {
    double ed = 0.0, eh = 0.0, scale = 0.0; long outside = 0;
    for (size_t q = 0; q < ld.size(); q++) {
        const double d = (double)fabsl((long double)dev[q] - ld[q]), h = (double)fabsl((long double)host[q] - ld[q]);
        if (!(d <= ed)) ed = d;
        if (!(h <= eh)) eh = h;
        scale = std::max(scale, (double)fabsl(ld[q]));
        if (mask && !(*mask)[q] && !(dev[q] == 0.0)) outside++;
    }
    printf("%s %.17g %.17g %.17g %ld\n", name, ed, eh, scale, outside);
}

static int bfgs(size_t n) {
    const int m = 4, nc = 7;
    DevOps ops;
    moihgp::opt::BFGSMat H;
    moihgp::opt::DevBFGSMat D;
    H.reset((int)n, m); D.reset(&ops, n, m);
    std::vector<Vector> S, Y;
    DVec ds, dy;
    for (int c = 0; c < nc; c++) {
        Vector s(n), y(n);
        for (size_t q = 0; q < n; q++) {
            s[q] = unif();
            y[q] = (0.5 + 0.25 * (double)(q % 11)) * s[q] + 0.05 * unif();
            if ((c == 4 && q % 5 == 0) || (c == 6 && q % 5 == 1)) y[q] = -2.0 * s[q];      // pair 4 bends the wrong way on the face q % 5 == 0, pair 6 (the newest) on q % 5 == 1
        }
        H.add_correction(s, y);
        ops.upload(s, ds); ops.upload(y, dy);
        D.add_correction(ds, dy);
        if (c >= nc - m) { S.push_back(s); Y.push_back(y); }
    }
    Vector v(n), hres, dres;
    for (size_t q = 0; q < n; q++) v[q] = unif();
    DVec dv, dr;
    ops.upload(v, dv);
    const double a = 0.37;
    H.apply_Hv(v, a, hres); D.apply_Hv(dv, a, dr); ops.download(dr, dres);
    leg("apply_Hv", dres, hres, two_loop_ld(S, Y, v, a, nullptr), nullptr);
    const Vector first = dres;

    // masks reach the device through active_set alone: x on lb with g > 0 where the variable is to be fixed
    unsigned char* dmask = moihgp_dvec_alloc_mask(n);
    if (!dmask) return 4;
    const char* names[4] = {"free_60", "free_skip_mid", "free_skip_newest", "free_none"};
    for (int k = 0; k < 4; k++) {
        std::vector<char> mask(n);
        for (size_t q = 0; q < n; q++) mask[q] = k == 0 ? (unif() < 0.2) : k == 1 ? (q % 5 == 0) : k == 2 ? (q % 5 == 1) : 0;
        Vector x(n), g(n, 1.0), lb(n, 0.0), ub(n, 1.0);
        for (size_t q = 0; q < n; q++) x[q] = mask[q] ? 0.5 : 0.0;
        DVec dx, dg, dlb, dub;
        ops.upload(x, dx); ops.upload(g, dg); ops.upload(lb, dlb); ops.upload(ub, dub);
        moihgp::opt::dv_check(moihgp_dvec_active_set(ops.ctx(), n, dx.data(), dg.data(), dlb.data(), dub.data(), dmask), "active_set");
        H.apply_Hv_free(v, mask, hres); D.apply_Hv_free(dv, dmask, dr); ops.download(dr, dres);
        leg(names[k], dres, hres, two_loop_ld(S, Y, v, 1.0, &mask), &mask);
    }
    ops.sync();
    moihgp_dvec_free(dmask);

    moihgp::opt::DevBFGSMat kept = D;                               // shares the pairs with D ...
    D.reset(&ops, n, m);                                           // ... which now lets go of them
    ops.upload(v, ds); ops.upload(Y[0], dy);
    D.add_correction(ds, dy);
    kept.apply_Hv(dv, a, dr); ops.download(dr, dres);
    printf("copy %d\n", (int)(memcmp(dres.data(), first.data(), n * sizeof(double)) == 0));
    return 0;
}

int main() {
    char mode[16];
    if (scanf("%15s", mode) != 1) return 2;
    try {
        if (!strcmp(mode, "solve")) {
            int prob, maxit, order; size_t n; char dump[512];
            if (scanf("%d %zu %d %d %511s", &prob, &n, &maxit, &order, dump) != 5) return 2;
            if (&dvec_cpu_order) dvec_cpu_order = order;
            if (prob == 0) return solve<Rosenbrock>(prob, n, maxit, dump);
            if (prob == 1) return solve<Quadratic>(prob, n, maxit, dump);
            if (prob == 2) return solve<Separable>(prob, n, maxit, dump);
        }
        if (!strcmp(mode, "bfgs")) {
            size_t n; int order;
            if (scanf("%zu %d", &n, &order) != 2) return 2;
            if (&dvec_cpu_order) dvec_cpu_order = order;
            return bfgs(n);
        }
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 3; }
    return 2;
}
