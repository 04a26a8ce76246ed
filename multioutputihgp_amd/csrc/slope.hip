// slope.hip -- slopes of whole series-major streams: the rate of change of every latent per unit of time (include/moihgp.h moihgp_slope_stream /
// _variances).
//
// Per latent, with the off-grid smoother's A_phi, B_phi, P_phi (interp.hip), M_phi = P_phi - Pinf and the smoother's two passes (xf forward, s backward),
// for offsets phi_0 .. phi_{K-1} in [0, 1):
//   given all ticks      slope[k][t] = a_k . xf[t] + gd_k . s[t+1],   a_k = e1^T A_phi_k,  gd_k = e0^T (F M_phi_k - Pinf F^T) B_phi_k^T P^-1
//                        var[k]      = (P_phi_k)_11 + gd_k (Ps - P) gd_k^T
//   given the ticks <= t slope[k][t] = a_k . xf[t],                   var[k] = (P_phi_k)_11
// the derivative with respect to time of interp.hip's fine[k][t] (of the forecast phi_k dt ahead of tick t in the second form) and that derivative's
// own posterior variance.  gd_k is d/dtau of interp.hip's row g_k (d M_phi / dtau = F M_phi + M_phi F^T, d B_phi^T / dtau = -F^T B_phi^T); it is NOT
// row 1 of G_phi where F Pinf + Pinf F^T has a non-zero first row, as with the reference's Matern-5/2.
//
// The planes have the shape of interp.hip's, a_k . xf[t] + g_k . s[t+1] with other rows, so this file holds only the kernel that builds the rows into an
// IT<D> block; the sweeps are interp.hip's kernels, launched by interp.hip's launch functions: both sweeps given all ticks, the forward sweep alone
// given the past (its rows g_k are zero, so interp_serial_kernel, which supplies the status words, the serial-route latents and the failed rows,
// leaves the planes of its backward walk as they are).
#include "stream_tables.h"

// ---- the tables: fp64, written for accuracy (no contraction, as interp.hip's) -------------------------------------------------------------------
#pragma clang fp contract(off)
#include "stationary_common.h"

namespace moihgp {
namespace {

template <int D>
__global__ void __launch_bounds__(64) slope_tables_kernel(int kernel, const double* __restrict__ cb64, const double* __restrict__ sm, size_t L,
                                                          double dt, InterpFracs fracs, int K, int given, double* __restrict__ it) {
    using S = SM<D>;
    using C = CB<D>;
    using W = IT<D>;
    constexpr int NN = D * D;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t l = idx / (size_t)K;
    const int k = (int)(idx % (size_t)K);
    if (l >= L) return;
    const double* cb = cb64 + l * C::SIZE;
    const double* s = sm + l * (size_t)S::SIZE;
    double* o = it + l * (size_t)W::SIZE;
    const bool failed = s[S::STATUS] != 0.0;
    double prm[3] = {cb[C::PARAMS + 0], cb[C::PARAMS + 1], cb[C::PARAMS + 2]};
    SS<D> ss;
    ss_build<D>(kernel, prm, ss);
    const double phi = fracs.f[k];
    double Fa[NN], Ap[NN], ApT[NN], T1[NN], T2[NN], Pp[NN];
    for (int i = 0; i < NN; i++) Fa[i] = ss.F[i] * (phi * dt);
    expm<D>(Fa, Ap);
    mt<D>(Ap, ApT);
    // P_phi = A_phi PF A_phi^T + Pinf - A_phi Pinf A_phi^T
    mm<D>(Ap, s + S::PF, T1); mm<D>(T1, ApT, Pp);
    mm<D>(Ap, ss.Pinf, T1); mm<D>(T1, ApT, T2);
    for (int i = 0; i < NN; i++) Pp[i] = Pp[i] + ss.Pinf[i] - T2[i];
    double g[D], q = 0.0;
    for (int j = 0; j < D; j++) g[j] = 0.0;
    if (given == 0) {
        // gd^T = P^-1 B_phi (F M_phi - Pinf F^T)^T e0 (P is symmetric): column 0 of the solve
        double Bp[NN], P[NN], X[NN];
        for (int i = 0; i < NN; i++) { Fa[i] = ss.F[i] * ((1.0 - phi) * dt); P[i] = s[S::P + i]; }
        expm<D>(Fa, Bp);
        for (int i = 0; i < NN; i++) T1[i] = Pp[i] - ss.Pinf[i];
        mm<D>(ss.F, T1, T1);                       // F M_phi
        mt<D>(ss.F, T2); mm<D>(ss.Pinf, T2, T2);   // Pinf F^T
        for (int i = 0; i < NN; i++) T1[i] = T1[i] - T2[i];
        mt<D>(T1, T1);
        mm<D>(Bp, T1, T1);
        lu_solve<D>(P, T1, X);
        for (int j = 0; j < D; j++) g[j] = X[j * D];
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) q += g[i] * (s[S::PS + i * D + j] - P[i * D + j]) * g[j];
    }
    const double nan = __builtin_nan("");
    for (int j = 0; j < D; j++) {
        o[W::AROW + k * D + j] = failed ? nan : Ap[D + j];
        o[W::GROW + k * D + j] = failed ? nan : g[j];
    }
    o[W::VAR + k] = failed ? nan : Pp[D + 1] + q;
    if (k == K - 1)
        for (int kk = K; kk < kInterpMaxPoints; kk++) {
            for (int j = 0; j < D; j++) { o[W::AROW + kk * D + j] = 0.0; o[W::GROW + kk * D + j] = 0.0; }
            o[W::VAR + kk] = 0.0;
        }
    if (k == 0) o[W::STATUS] = failed ? 1.0 : 0.0;
}

}  // namespace

void launch_slope_tables(int kernel, int d, const double* cb64, const double* sm, size_t L, double dt, const InterpFracs& fracs, int K, int given,
                         double* it, hipStream_t stream) {
    if (L == 0) return;
    dim3 block(64), grid((unsigned)((L * (size_t)K + 63) / 64));
    dispatch_dim(d, [&](auto dim) {
        hipLaunchKernelGGL((slope_tables_kernel<decltype(dim)::value>), grid, block, 0, stream, kernel, cb64, sm, L, dt, fracs, K, given, it);
    });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_slope_stream(int d, const SweepIo& io, const double* sm, const double* it, const SweepPlanes& out, int* status, int path, int given) {
    if (given == 0) launch_interp_stream(d, io, sm, it, out, status, path);
    else launch_interp_forward(d, io, sm, it, out, status, path);
}

}  // namespace moihgp
