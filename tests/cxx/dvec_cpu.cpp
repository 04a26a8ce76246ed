// dvec_cpu.cpp -- test-only CPU stand-in for the `moihgp_dvec_*` entries of libmoihgp (include/moihgp.h "device vectors", csrc/vecops.hip):
// plain loops over malloc'ed memory.  Linked in place of the library it runs the host logic of include/moihgp_cxx/lbfgsb_dev.hpp
// (DevBFGSMat, DevLBFGSBSolver) on a machine without a GPU, and `dvec_cpu_order` chooses the order in which the reductions add their terms,
// so that a test can tell what rounding order alone does to the solver from what a defect does:
//   0  sequential, as the host solver (lbfgsb.hpp)          1  sequential in long double, rounded once
//   2  sequential from the last term to the first           3  the device's own order (below), element-wise kernels fused as on the device
// The device's order (vecops.hip): 1024 x 256 threads; thread g adds the terms g, g + 262144, .. with one fma each; per workgroup a butterfly
// over each 64 lanes (lane 0 of `v += shfl_xor(v, o)`, o = 32 .. 1, is the tree v[l] += v[l + o] for l < o) and the 4 wavefront sums in
// order; the finish adds the partials t, t + 256, t + 512, t + 768 per thread, then the same butterfly and 4 wavefront sums.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
#include "moihgp.h"
}

extern "C" int dvec_cpu_order;
int dvec_cpu_order = 0;

namespace {

constexpr size_t kBlocks = 1024, kThreads = 256, kGrid = kBlocks * kThreads;

double wave_sum(double* v) {                       // 64 lanes, the value lane 0 ends with
    for (int o = 32; o > 0; o >>= 1) for (int l = 0; l < o; l++) v[l] += v[l + o];
    return v[0];
}
double block_sum(double* v) {                      // 256 threads
    double r = 0.0;
    for (int w = 0; w < 4; w++) r += wave_sum(v + 64 * w);
    return r;
}
double wave_max(double* v) {
    for (int o = 32; o > 0; o >>= 1) for (int l = 0; l < o; l++) { const double u = v[l + o]; v[l] = (u > v[l] || u != u) ? u : v[l]; }
    return v[0];
}
double block_max(double* v) {
    double r = 0.0;
    for (int w = 0; w < 4; w++) { const double u = wave_max(v + 64 * w); r = (u > r || u != u) ? u : r; }
    return r;
}
double finish(const std::vector<double>& partial, bool is_max) {
    double acc[kThreads];
    for (size_t t = 0; t < kThreads; t++) {
        double a = 0.0;
        for (size_t i = t; i < kBlocks; i += kThreads) { const double v = partial[i]; if (is_max) a = (v > a || v != v) ? v : a; else a += v; }
        acc[t] = a;
    }
    return is_max ? block_max(acc) : block_sum(acc);
}

// sum_i term(i) in the chosen order; `fused(i, acc)` is the device thread's `acc = fma(.., .., acc)` for the same term
template <typename Term, typename Fused>
double reduce_sum(size_t n, Term term, Fused fused) {
    switch (dvec_cpu_order) {
    case 1: { long double s = 0.0L; for (size_t i = 0; i < n; i++) s += (long double)term(i); return (double)s; }
    case 2: { double s = 0.0; for (size_t i = n; i-- > 0;) s += term(i); return s; }
    case 3: {
        std::vector<double> partial(kBlocks, 0.0);
        double acc[kThreads];
        for (size_t b = 0; b < kBlocks && b * kThreads < n; b++) {       // (a workgroup whose threads all start past n holds +0.0)
            for (size_t t = 0; t < kThreads; t++) {
                double a = 0.0;
                for (size_t i = b * kThreads + t; i < n; i += kGrid) a = fused(i, a);
                acc[t] = a;
            }
            partial[b] = block_sum(acc);
        }
        return finish(partial, false);
    }
    default: { double s = 0.0; for (size_t i = 0; i < n; i++) s += term(i); return s; }
    }
}

char g_error[64] = "";

}  // namespace

struct moihgp_dvec_ctx { int unused; };

extern "C" {

const char* moihgp_last_error(void) { return g_error; }
moihgp_dvec_ctx* moihgp_dvec_ctx_new(void) { return new moihgp_dvec_ctx(); }
void moihgp_dvec_ctx_del(moihgp_dvec_ctx* c) { delete c; }
void* moihgp_dvec_ctx_stream(moihgp_dvec_ctx*) { return nullptr; }
double* moihgp_dvec_alloc(size_t n) { return static_cast<double*>(std::malloc((n ? n : 1) * sizeof(double))); }
unsigned char* moihgp_dvec_alloc_mask(size_t n) { return static_cast<unsigned char*>(std::malloc(n ? n : 1)); }
void moihgp_dvec_free(void* p) { std::free(p); }
void moihgp_dvec_trim(void) {}
void moihgp_dvec_cache_limit(size_t) {}
int moihgp_dvec_upload(moihgp_dvec_ctx*, double* dst, const double* src, size_t n) { std::memcpy(dst, src, n * sizeof(double)); return 0; }
int moihgp_dvec_download(moihgp_dvec_ctx*, double* dst, const double* src, size_t n) { std::memcpy(dst, src, n * sizeof(double)); return 0; }
int moihgp_dvec_copy(moihgp_dvec_ctx*, double* dst, const double* src, size_t n) { std::memmove(dst, src, n * sizeof(double)); return 0; }
int moihgp_dvec_sync(moihgp_dvec_ctx*) { return 0; }

int moihgp_dvec_dot(moihgp_dvec_ctx*, size_t n, const double* a, const double* b, const unsigned char* mask, double* result) {
    *result = reduce_sum(n, [&](size_t i) { return (!mask || mask[i]) ? a[i] * b[i] : 0.0; },
                         [&](size_t i, double acc) { return (!mask || mask[i]) ? std::fma(a[i], b[i], acc) : acc; });
    return 0;
}
int moihgp_dvec_axpy(moihgp_dvec_ctx*, size_t n, double alpha, const double* x, double* y, const unsigned char* mask) {
    const bool fused = dvec_cpu_order == 3;
    for (size_t i = 0; i < n; i++) if (!mask || mask[i]) y[i] = fused ? std::fma(alpha, x[i], y[i]) : y[i] + alpha * x[i];
    return 0;
}
int moihgp_dvec_scale(moihgp_dvec_ctx*, size_t n, double alpha, const double* x, double* y, const unsigned char* mask) {
    for (size_t i = 0; i < n; i++) y[i] = (!mask || mask[i]) ? alpha * x[i] : 0.0;
    return 0;
}
int moihgp_dvec_sub(moihgp_dvec_ctx*, size_t n, const double* a, const double* b, double* out) {
    for (size_t i = 0; i < n; i++) out[i] = a[i] - b[i];
    return 0;
}
int moihgp_dvec_clamp(moihgp_dvec_ctx*, size_t n, double* x, const double* lb, const double* ub) {
    for (size_t i = 0; i < n; i++) x[i] = std::fmin(std::fmax(x[i], lb[i]), ub[i]);
    return 0;
}
int moihgp_dvec_active_set(moihgp_dvec_ctx*, size_t n, const double* x, const double* g, const double* lb, const double* ub, unsigned char* free_var) {
    for (size_t i = 0; i < n; i++) free_var[i] = !((x[i] <= lb[i] && g[i] > 0.0) || (x[i] >= ub[i] && g[i] < 0.0) || lb[i] == ub[i]) ? 1 : 0;
    return 0;
}
int moihgp_dvec_proj_step(moihgp_dvec_ctx*, size_t n, const double* xp, const double* drt, double step, const double* lb, const double* ub, const double* gradp,
                          double* xt, double* dec) {
    const bool fused = dvec_cpu_order == 3;
    for (size_t i = 0; i < n; i++) xt[i] = std::fmin(std::fmax(fused ? std::fma(step, drt[i], xp[i]) : xp[i] + step * drt[i], lb[i]), ub[i]);
    *dec = reduce_sum(n, [&](size_t i) { return gradp[i] * (xt[i] - xp[i]); },
                      [&](size_t i, double acc) { return std::fma(gradp[i], xt[i] - xp[i], acc); });
    return 0;
}
int moihgp_dvec_proj_grad_norm(moihgp_dvec_ctx*, size_t n, const double* x, const double* g, const double* lb, const double* ub, double* result) {
    auto term = [&](size_t i) { double v = x[i] - g[i]; v = v < lb[i] ? lb[i] : v; v = v > ub[i] ? ub[i] : v; return std::fabs(v - x[i]); };   // (a NaN stays one)
    if (dvec_cpu_order != 3) {                      // (a maximum does not depend on the order; NaN sticks as on the device)
        double r = 0.0;
        for (size_t i = 0; i < n; i++) { const double d = term(i); r = (d > r || d != d) ? d : r; }
        *result = r;
        return 0;
    }
    std::vector<double> partial(kBlocks, 0.0);
    double acc[kThreads];
    for (size_t b = 0; b < kBlocks && b * kThreads < n; b++) {
        for (size_t t = 0; t < kThreads; t++) {
            double a = 0.0;
            for (size_t i = b * kThreads + t; i < n; i += kGrid) { const double d = term(i); a = (d > a || d != d) ? d : a; }
            acc[t] = a;
        }
        partial[b] = block_max(acc);
    }
    *result = finish(partial, true);
    return 0;
}

}  // extern "C"
