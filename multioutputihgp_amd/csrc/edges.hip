// edges.hip -- exact-edge smoothing of whole streams (include/moihgp.h moihgp_smooth_stream_exact): the rank-d correction that turns the
// steady-state sweeps of smoother.hip, run from a zero start state, into the smoother of the same model under the model's own prior on the
// first state, and the time-varying smoothed variance at the two ends of the stream.
//
// The steady sweeps are the exact smoother under x_0 ~ N(0, P); the model says x_0 ~ N(0, Pinf).  Per latent, with the smoother's tables
// G, P, PF, Ps (SM<D>) and s[0] from the backward sweep:
//   Ps_t :  Ps_{T-1} = PF,  Ps_t = PF + G (Ps_{t+1} - P) G^T        (backward; reaches Ps once T - 1 - t >= TAIL)
//   E = Pinf^-1 - P^-1,     Z = -(I + E Ps_0)^-1 E,   c = Z s[0]
//   r_t = e0^T Ps_t (G^T)^t                                          (below 2^-60 of its size once t >= HEAD)
//   ys[t] += r_t c,   var[t] = (Ps_t)_00 + r_t Z r_t^T,   x_end += PF (G^T)^(T-1) c
// Ticks in [HEAD, T - TAIL) are not touched: ys keeps the sweeps' bits and var is the steady value.
//
// Kernels
//   edge_tables_kernel    one lane per latent, fp64: E, the row e0^T Ps, HEAD and TAIL by walking the powers of G, a status.  Launch-latency work,
//                         once per parameter set (capi.cpp builds it lazily beside the smoother's tables).
//   smooth_edges_kernel   two wavefronts per latent behind the two sweeps, one for the tail and one for the head and the coalesced fill of the
//                         interior of var: away from each other the two edges are independent.  The recursions are serial in t and every
//                         lane carries them (the same registers in all 64 lanes: no divergence, no broadcast); per tile of kEdgeTile ticks
//                         the values go through LDS and the 64 lanes read and write the rows coalesced.  When the two edges of a latent
//                         overlap (HEAD + TAIL > T) the head needs row 0 of the tail's Ps_t: the tail's wavefront then walks both, leaving
//                         the rows in `scratch` [L][T][D] (T <= kEdgeScratchTicks; status 3 beyond) and reading them back in the head
//                         walk, and the head's wavefront leaves at once.
// Written for accuracy like the tables kernels (fp64, no contraction): the work is (HEAD + TAIL) O(d^3) per latent.
#pragma clang fp contract(off)
#include "stationary_common.h"
#include "stream_tables.h"

namespace moihgp {
namespace {

constexpr int kEdgeTile = 128;
constexpr double kEdgeEps = 0x1p-60;

template <int D>
__global__ void __launch_bounds__(64) edge_tables_kernel(int kernel, const double* __restrict__ cb64, const double* __restrict__ sm, size_t L,
                                                         double* __restrict__ et) {
    using B = SM<D>;
    using C = CB<D>;
    using Eb = ET<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* cb = cb64 + l * C::SIZE;
    const double* tb = sm + l * B::SIZE;
    double* o = et + l * Eb::SIZE;
    double prm[3] = {cb[C::PARAMS + 0], cb[C::PARAMS + 1], cb[C::PARAMS + 2]};
    SS<D> s;
    ss_build<D>(kernel, prm, s);
    double P[NN], G[NN], I[NN], Pinv[NN], Pinfinv[NN], E[NN];
    for (int i = 0; i < NN; i++) { P[i] = tb[B::P + i]; G[i] = tb[B::G + i]; I[i] = (i % (D + 1)) == 0 ? 1.0 : 0.0; }
    lu_solve<D>(s.Pinf, I, Pinfinv);
    lu_solve<D>(P, I, Pinv);
    bool fin = true;
    for (int i = 0; i < NN; i++) { E[i] = Pinfinv[i] - Pinv[i]; fin = fin && isfinite(E[i]) && isfinite(G[i]) && isfinite(tb[B::PS + i]) && isfinite(tb[B::PF + i]); }
    // HEAD: the smallest n with |G^n|inf <= 2^-60; TAIL: the smallest k with |G^k|inf^2 <= 2^-60 (one walk: TAIL comes first)
    int head = kEdgeCap, tail = kEdgeCap;
    if (fin && tb[B::STATUS] == 0.0) {
        double M[NN];
        for (int i = 0; i < NN; i++) M[i] = I[i];
#pragma nounroll
        for (int n = 1; n < kEdgeCap; n++) {
            mm<D>(G, M, M);
            const double nrm = norm_inf<D>(M);
            if (!isfinite(nrm)) { fin = false; break; }
            if (tail == kEdgeCap && nrm * nrm <= kEdgeEps) tail = n;
            if (nrm <= kEdgeEps) { head = n; break; }
        }
    }
    for (int i = 0; i < NN; i++) o[Eb::E + i] = E[i];
    for (int i = 0; i < D; i++) o[Eb::PSROW + i] = tb[B::PS + i];
    o[Eb::HEAD] = (double)head;
    o[Eb::TAIL] = (double)tail;
    o[Eb::STATUS] = tb[B::STATUS] != 0.0 ? 1.0 : (fin ? 0.0 : 4.0);
}

// Ps <- PF + G (Ps - P) G^T
template <int D>
__device__ __forceinline__ void tail_step(const double* G, const double* GT, const double* P, const double* PF, double* Ps) {
    double Df[D * D], T1[D * D];
    for (int i = 0; i < D * D; i++) Df[i] = Ps[i] - P[i];
    mm<D>(G, Df, T1);
    mm<D>(T1, GT, T1);
    for (int i = 0; i < D * D; i++) Ps[i] = PF[i] + T1[i];
}

template <typename Tv, int D>
__global__ void __launch_bounds__(64) smooth_edges_kernel(size_t T, const double* __restrict__ sm, const double* __restrict__ et,
                                                          const double* __restrict__ s0, double* scratch, Tv* ys, Tv* var, size_t ld_out, Tv* x,
                                                          int* status) {
    using B = SM<D>;
    using Eb = ET<D>;
    constexpr int NN = D * D;
    __shared__ double rowb[kEdgeTile * D];      // row 0 of Ps_t of the tile's ticks
    __shared__ double corb[kEdgeTile];          // the tile's corrections of ys
    __shared__ double varb[kEdgeTile];          // the tile's variances
    const size_t l = blockIdx.x >> 1;
    const bool head_role = blockIdx.x & 1;      // two wavefronts per latent: the tail's (it walks the head too where the edges overlap) and the head's
    const int lane = threadIdx.x;
    const double* tb = sm + l * B::SIZE;
    const double* eb = et + l * Eb::SIZE;
    Tv* yrow = ys + l * ld_out;
    Tv* vrow = var ? var + l * ld_out : nullptr;
    if (tb[B::STATUS] != 0.0) {                 // the Kalman DARE failed: the sweeps wrote the NaN row, the NaN end state and status 1
        if (vrow && !head_role)
            for (size_t t = lane; t < T; t += 64) vrow[t] = (Tv)__builtin_nan("");
        return;
    }
    const size_t head = (size_t)eb[Eb::HEAD], tail = (size_t)eb[Eb::TAIL];
    const bool overlap = head >= (size_t)kEdgeCap || tail >= (size_t)kEdgeCap || head + tail > T;
    const int code = eb[Eb::STATUS] != 0.0 ? 4 : (overlap && (T > (size_t)kEdgeScratchTicks || !scratch)) ? 3 : 0;
    const Tv vsteady = (Tv)tb[B::VARS];
    if (code != 0) {                            // the steady sweeps' row and end state stay; the steady variance
        if (head_role) return;
        if (status && lane == 0) status[l] = code;
        if (vrow)
            for (size_t t = lane; t < T; t += 64) vrow[t] = vsteady;
        return;
    }
    const size_t n_head = head < T ? head : T, n_tail = tail < T ? tail : T;
    const size_t t_tail = T - n_tail;           // ticks t_tail .. T - 1 take Ps_t from the recursion
    if (head_role && overlap) return;
    if (vrow && head_role)                      // the interior (there is none where the edges overlap)
        for (size_t t = n_head + lane; t < t_tail; t += 64) vrow[t] = vsteady;

    double G[NN], GT[NN], P[NN], PF[NN], Pst[NN], psrow[D];
    for (int i = 0; i < NN; i++) { G[i] = tb[B::G + i]; P[i] = tb[B::P + i]; PF[i] = tb[B::PF + i]; Pst[i] = PF[i]; }
    for (int i = 0; i < D; i++) psrow[i] = eb[Eb::PSROW + i];
    mt<D>(G, GT);
    double* srow = scratch ? scratch + l * T * D : nullptr;

    // ---- the tail, from tick T - 1 down to t_tail: var where the head does not reach, row 0 of Ps_t into scratch where it does
    for (size_t k0 = 0; k0 < (head_role ? 0 : n_tail); k0 += kEdgeTile) {
        const int n = (int)(n_tail - k0 < (size_t)kEdgeTile ? n_tail - k0 : (size_t)kEdgeTile);
        for (int i = 0; i < n; i++) {
            if (k0 + i > 0) tail_step<D>(G, GT, P, PF, Pst);
            if (lane == 0) {
                varb[i] = Pst[0];
                for (int j = 0; j < D; j++) rowb[i * D + j] = Pst[j];
            }
        }
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            const size_t t = T - 1 - (k0 + i);
            if (t >= n_head) { if (vrow) vrow[t] = (Tv)varb[i]; }
            else if (srow)
                for (int j = 0; j < D; j++) srow[t * D + j] = rowb[i * D + j];
        }
        __syncthreads();
    }
    if (n_head == 0 || (!head_role && !overlap)) return;
    __threadfence_block();

    // ---- Z and c = Z s[0], with Ps_0 from the tail where it reaches tick 0
    double Ps0[NN], E[NN], I[NN], T1[NN], Z[NN], c[D], sv[D];
    for (int i = 0; i < NN; i++) { Ps0[i] = t_tail == 0 ? Pst[i] : tb[B::PS + i]; E[i] = eb[Eb::E + i]; I[i] = (i % (D + 1)) == 0 ? 1.0 : 0.0; }
    for (int i = 0; i < D; i++) sv[i] = s0[l * D + i];
    mm<D>(E, Ps0, T1);
    for (int i = 0; i < NN; i++) T1[i] = I[i] + T1[i];
    lu_solve<D>(T1, E, Z);
    for (int i = 0; i < NN; i++) Z[i] = -Z[i];
    mv<D>(Z, sv, c);

    // ---- the head, from tick 0 up to n_head - 1.  Apart from the tail, row 0 of Ps_t is the tables' at every tick and r_t = r_{t-1} G^T is a vector
    // recursion; where the edges overlap the rows come from the tail and r_t = row_t (G^T)^t needs the matrix power.
    double M[NN], xc[D], r[D];                  // M = (G^T)^t
    for (int i = 0; i < NN; i++) M[i] = I[i];
    for (int i = 0; i < D; i++) { xc[i] = 0.0; r[i] = psrow[i]; }
    for (size_t t0 = 0; t0 < n_head; t0 += kEdgeTile) {
        const int n = (int)(n_head - t0 < (size_t)kEdgeTile ? n_head - t0 : (size_t)kEdgeTile);
        if (overlap)
            for (int i = lane; i < n * D; i += 64) {
                const size_t t = t0 + i / D;
                rowb[i] = (t >= t_tail && srow) ? srow[t * D + i % D] : psrow[i % D];
            }
        __syncthreads();
        for (int i = 0; i < n; i++) {
            double row0 = psrow[0], rz[D];
            if (overlap) {
                double row[D];
                for (int j = 0; j < D; j++) row[j] = rowb[i * D + j];
                for (int j = 0; j < D; j++) { double a = 0.0; for (int k = 0; k < D; k++) a += row[k] * M[k * D + j]; r[j] = a; }
                row0 = row[0];
            }
            for (int j = 0; j < D; j++) { double a = 0.0; for (int k = 0; k < D; k++) a += r[k] * Z[k * D + j]; rz[j] = a; }
            double cor = 0.0, q = 0.0;
            for (int j = 0; j < D; j++) { cor += r[j] * c[j]; q += rz[j] * r[j]; }
            if (overlap && t0 + i == T - 1) {   // the end state, where the head reaches the last tick: PF (G^T)^(T-1) c
                double PM[NN];
                mm<D>(PF, M, PM);
                mv<D>(PM, c, xc);
            }
            if (lane == 0) { corb[i] = cor; varb[i] = row0 + q; }
            if (overlap) mm<D>(M, GT, M);
            else {
                double rn[D];
                for (int j = 0; j < D; j++) { double a = 0.0; for (int k = 0; k < D; k++) a += r[k] * GT[k * D + j]; rn[j] = a; }
                for (int j = 0; j < D; j++) r[j] = rn[j];
            }
        }
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            const size_t t = t0 + i;
            yrow[t] = (Tv)((double)yrow[t] + corb[i]);
            if (vrow) vrow[t] = (Tv)varb[i];
        }
        __syncthreads();
    }
    if (overlap && n_head == T && lane < D) x[l * D + lane] = (Tv)((double)x[l * D + lane] + xc[lane]);
}

}  // namespace

void launch_edge_tables(int kernel, int d, const double* cb64, const double* sm, size_t L, double* et, hipStream_t stream) {
    if (L == 0) return;
    dim3 block(64), grid((unsigned)((L + 63) / 64));
    dispatch_dim(d, [&](auto dim) { hipLaunchKernelGGL((edge_tables_kernel<decltype(dim)::value>), grid, block, 0, stream, kernel, cb64, sm, L, et); });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_smooth_edges(int d, const SweepIo& io, const double* sm, const double* et, const double* s0, double* scratch, void* var, int* status) {
    if (io.L == 0 || io.T == 0) return;
    dispatch_stream(d, io.dtype, [&](auto tv, auto dim) {
        using Tv = decltype(tv);
        hipLaunchKernelGGL((smooth_edges_kernel<Tv, decltype(dim)::value>), dim3((unsigned)(2 * io.L)), dim3(64), 0, io.stream, io.T, sm, et, s0, scratch,
                           (Tv*)io.yhat, (Tv*)var, io.ld_out, (Tv*)io.x, status);
    });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

}  // namespace moihgp
