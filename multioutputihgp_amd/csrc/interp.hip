// interp.hip -- off-grid smoothing of whole series-major streams: the smoothed mean between ticks (include/moihgp.h moihgp_interp_stream /
// _variances).
//
// Per latent, with the smoother's tables (A, K, G, P, PF, Ps of SM<D>), Pinf and F of the model and the smoother's two passes
//   forward   xp[t] = A xf[t-1];  p[t] = xp[t]_0;  v[t] = y[t] - p[t] (0 where y[t] is NaN);  xf[t] = xp[t] + K v[t]
//   backward  s[T] = 0;  s[t] = G s[t+1] + K v[t];  ys[t] = p[t] + s[t]_0
// for fractions phi_0 .. phi_{K-1} in [0, 1):
//   A_phi = expm(F phi dt);  B_phi = expm(F (1 - phi) dt);  P_phi = A_phi PF A_phi^T + Pinf - A_phi Pinf A_phi^T;  G_phi = P_phi B_phi^T P^-1
//   fine[k][t] = a_k . xf[t] + g_k . s[t+1],   a_k = H A_phi_k,  g_k = H G_phi_k          the mean at time (t + phi_k) dt given the whole stream
//   var[k]     = ( P_phi + G_phi (Ps - P) G_phi^T )_00
// i.e. the RTS smoother with an unobserved point inserted between ticks t and t + 1 (the predicted covariance at t + 1 through it is again P).
//
// Kernels
//   interp_tables_kernel   fp64, one lane per (latent, offset): the two exponentials (expm of stationary_common.h), P_phi, G_phi through an LU solve
//                          on P, the rows a_k, g_k and var[k]; NaN where the smoother's status is non-zero.  Built per call: the rows depend on the
//                          call's offsets.
//   interp_fwd_kernel      the smoother's forward sweep (chunk maps, scan, replay: scan_sweep.h) whose replay also writes q_k[t] = a_k . xf[t] into
//                          plane k.  y is staged and scanned once per segment; more than KG offsets repeat the replay from the lane's start state
//                          per group of KG planes, and p replaces y in the last group.
//   interp_bwd_kernel      one wavefront per latent, segments from the last to the first with the lane order mirrored, every chunk's map G^kScanChunk,
//                          as smooth_bwd_kernel.  v = y - p is staged once per segment (p stays in registers, for the store) and scanned once: one
//                          state s serves all offsets.  Per group of KG planes the lane replays its chunk from the state that enters it: at tick t it
//                          holds s[t+1] -- from the neighbouring lane at the chunk's last tick, from the segment to the right at the segment's last,
//                          zero at tick T - 1 -- adds g_k . s[t+1] to q_k[t] in the staged plane, then steps to s[t].  The last group writes s_0 over
//                          v, which leaves as ys = p + s_0.
//   interp_serial_kernel   one lane per latent, fp64, tick by tick: the latents the scan kernels leave (growth bound failed, option "interp_path" = 1),
//                          every status word, and the NaN rows of failed latents when it walks all.
// slope.hip builds other rows into the same IT<D> block and launches these sweeps for them (launch_interp_stream; launch_interp_forward: the
// forward sweep and the serial kernel alone, for rows g_k = 0).
// Arithmetic is fp64 for both stream types, as the smoother's; fp32 streams are staged in fp32 (v and the planes are rounded to the stream's own
// precision) and narrowed on store.
#include "scan_sweep.h"

namespace moihgp {
namespace {

// Tv: the stream's scalar and that of the staged planes; KG: planes staged per replay.  sm: the smoother's blocks, it: the call's IT<D> blocks.
template <typename Tv, int D, int KG>
__global__ void __launch_bounds__(64) interp_fwd_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ sm,
                                                        const double* __restrict__ it, int K, const Tv* x_in, Tv* x_out, Tv* __restrict__ p_out,
                                                        Tv* __restrict__ fine, size_t ld_out, size_t plane_stride, int path) {
    using B = SM<D>;
    using W = IT<D>;
    constexpr int NN = D * D;
    extern __shared__ double interp_lds[];
    __shared__ double buf[kScanPlane];                 // y of the segment, then p
    Tv* qb = reinterpret_cast<Tv*>(interp_lds);        // [KG][64][kScanPitch] q_k of the group
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const double* tb = sm + l * B::SIZE;
    const double* tw = it + l * W::SIZE;
    const Tv* yrow = Ty + l * ld_in;
    Tv* prow = p_out + l * ld_out;
    Tv* frow = fine + l * ld_out;
    const Route route = latent_route(tb[B::STATUS], tb[B::GROWTH], scan_growth_bound<double>(), path);
    if (route == Route::kFailed) {
        write_failed<Tv, D>(prow, 0, 1, T, x_out + l * D, lane, 64);
        write_failed<Tv, D>(frow, plane_stride, K, T, x_out + l * D, lane, 64);
    }
    if (route != Route::kScan) return;
    double A[NN], AKHA[NN], MF[NN], Kg[D];
#pragma unroll
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; AKHA[i] = tb[B::AKHA + i]; MF[i] = tb[B::MF + i]; }
#pragma unroll
    for (int i = 0; i < D; i++) Kg[i] = tb[B::K + i];
    double xseg[D];
#pragma unroll
    for (int i = 0; i < D; i++) xseg[i] = (double)x_in[l * D + i];
    double* my = buf + lane * kScanPitch;
    for (size_t seg0 = 0; seg0 < T; seg0 += kScanSeg) {
        stage_in(yrow, seg0, T, lane, buf);
        __syncthreads();
        bool regular;
        const int n = lane_ticks(my, seg0, T, lane, regular);
        // 1. the chunk's map from a zero state; 2. scan over the lanes: the state before this lane's chunk
        double Phi[NN], r[D], xs[D];
        chunk_map<double, D>(my, n, regular, A, AKHA, MF, Kg, Phi, r);
        scan_maps<double, D, true>(Phi, r, lane);
        start_states<double, D, true>(Phi, r, xseg, xs, lane);
        // 3. replay per group of planes: q_k = a_k . xf into the lane's rows of qb; the last group leaves p in place of y
        for (int k0 = 0; k0 < K; k0 += KG) {
            const bool last = k0 + KG >= K;
            double a[KG][D], xr[D];
#pragma unroll
            for (int kk = 0; kk < KG; kk++)
#pragma unroll
                for (int j = 0; j < D; j++) a[kk][j] = tw[W::AROW + (k0 + kk) * D + j];   // (k0 + kk < kInterpMaxPoints: KG divides it)
#pragma unroll
            for (int j = 0; j < D; j++) xr[j] = xs[j];
            for (int i = 0; i < n; i++) {
                double xp[D];
                matvec<double, D>(A, xr, xp);
                const double y = my[i], p = xp[0];
                const double v = isnan(y) ? 0.0 : y - p;
#pragma unroll
                for (int j = 0; j < D; j++) xr[j] = fma(Kg[j], v, xp[j]);
#pragma unroll
                for (int kk = 0; kk < KG; kk++) {
                    double q = 0.0;
#pragma unroll
                    for (int j = 0; j < D; j++) q = fma(a[kk][j], xr[j], q);
                    qb[kk * kScanPlane + lane * kScanPitch + i] = (Tv)q;
                }
                if (last) my[i] = p;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KG; kk++)
                if (k0 + kk < K) stage_out(qb + kk * kScanPlane, frow + (size_t)(k0 + kk) * plane_stride, seg0, T, lane);
            if (last) stage_out(buf, prow, seg0, T, lane);
            __syncthreads();
        }
    }
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)xseg[i];
}

template <typename Tv, int D, int KG>
__global__ void __launch_bounds__(64) interp_bwd_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ sm,
                                                        const double* __restrict__ it, int K, Tv* ys, Tv* fine, size_t ld_out, size_t plane_stride,
                                                        int path) {
    using B = SM<D>;
    using W = IT<D>;
    constexpr int NN = D * D;
    extern __shared__ double interp_lds[];
    Tv* vb = reinterpret_cast<Tv*>(interp_lds);        // [64][kScanPitch] v of the segment, then s_0
    Tv* qb = vb + kScanPlane;                          // [KG] ... q_k of the group, then fine
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const double* tb = sm + l * B::SIZE;
    const double* tw = it + l * W::SIZE;
    if (latent_route(tb[B::STATUS], tb[B::GROWTH], scan_growth_bound<double>(), path) != Route::kScan) return;
    double G[NN], MB[NN], Kg[D];
#pragma unroll
    for (int i = 0; i < NN; i++) { G[i] = tb[B::G + i]; MB[i] = tb[B::MB + i]; }
#pragma unroll
    for (int i = 0; i < D; i++) Kg[i] = tb[B::K + i];
    double sseg[D];
#pragma unroll
    for (int i = 0; i < D; i++) sseg[i] = 0.0;
    const Tv* yrow = Ty + l * ld_in;
    Tv* prow = ys + l * ld_out;
    Tv* frow = fine + l * ld_out;
    Tv* v = vb + lane * kScanPitch;
    const size_t nseg = (T + kScanSeg - 1) / kScanSeg;
    for (size_t sg = nseg; sg-- > 0;) {
        const size_t seg0 = sg * kScanSeg;
        Tv pseg[kScanChunk];                    // p at the ticks this lane loads and stores (the same coalesced walk): it never goes through LDS
#pragma unroll
        for (int k = 0; k < kScanChunk; k++) {   // as smooth_bwd_kernel, of v = y - p
            const int tl = k * 64 + lane;
            const size_t t = seg0 + tl;
            Tv y = 0, p = 0;
            if (t < T) { y = yrow[t]; p = prow[t]; }
            vb[scan_slot(tl)] = (t < T && !isnan(y)) ? (Tv)((double)y - (double)p) : (Tv)0;
            pseg[k] = p;
        }
        __syncthreads();
        // 1. the chunk's response from a zero state at its end (its map is G^kScanChunk for every lane); 2. mirrored scan: s0 is the state that
        // enters this lane's chunk from the right, s[t+1] of the chunk's last tick (the carry of the segment to the right in lane 63, zero at T)
        double Phi[NN], r[D], s0[D];
#pragma unroll
        for (int i = 0; i < NN; i++) Phi[i] = MB[i];
        chunk_response_bwd<double, D, Tv>(v, G, Kg, r);
        scan_maps<double, D, false>(Phi, r, lane);
        start_states<double, D, false>(Phi, r, sseg, s0, lane);
        for (int k0 = 0; k0 < K; k0 += KG) {
            const bool last = k0 + KG >= K;
#pragma unroll
            for (int kk = 0; kk < KG; kk++)
                if (k0 + kk < K) stage_in(frow + (size_t)(k0 + kk) * plane_stride, seg0, T, lane, qb + kk * kScanPlane);
            __syncthreads();
            // 3. replay per group: fine = q + g_k . s[t+1] in place of q, then the step to s[t]; the last group leaves s_0 in place of v
            double g[KG][D], s[D];
#pragma unroll
            for (int kk = 0; kk < KG; kk++)
#pragma unroll
                for (int j = 0; j < D; j++) g[kk][j] = tw[W::GROW + (k0 + kk) * D + j];   // (rows past K are zero)
#pragma unroll
            for (int j = 0; j < D; j++) s[j] = s0[j];
            for (int i = kScanChunk - 1; i >= 0; i--) {
#pragma unroll
                for (int kk = 0; kk < KG; kk++) {
                    Tv* qv = qb + kk * kScanPlane + lane * kScanPitch;
                    double c = (double)qv[i];
#pragma unroll
                    for (int j = 0; j < D; j++) c = fma(g[kk][j], s[j], c);
                    qv[i] = (Tv)c;
                }
                tick_step<double, D>(G, Kg, (double)v[i], s);
                if (last) v[i] = (Tv)s[0];
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KG; kk++)
                if (k0 + kk < K) stage_out(qb + kk * kScanPlane, frow + (size_t)(k0 + kk) * plane_stride, seg0, T, lane);
            if (last) {
#pragma unroll
                for (int k = 0; k < kScanChunk; k++) {
                    const int tl = k * 64 + lane;
                    const size_t t = seg0 + tl;
                    if (t < T) prow[t] = pseg[k] + vb[scan_slot(tl)];   // ys = p + s_0
                }
            }
            __syncthreads();
        }
    }
}

// Tick by tick, one lane per latent: the latents the scan kernels do not take, the NaN rows of failed latents when they do not run, every status word.
template <typename Tv, int D>
__global__ void __launch_bounds__(64) interp_serial_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ sm,
                                                           const double* __restrict__ it, size_t L, int K, const Tv* x_in, Tv* x_out, Tv* ys, Tv* fine,
                                                           size_t ld_out, size_t plane_stride, int* status, int path) {
    using B = SM<D>;
    using W = IT<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* tb = sm + l * B::SIZE;
    const double* tw = it + l * W::SIZE;
    const Route route = latent_route(tb[B::STATUS], tb[B::GROWTH], scan_growth_bound<double>(), path);
    if (status) status[l] = route == Route::kFailed ? 1 : 0;
    Tv* prow = ys + l * ld_out;
    Tv* frow = fine + l * ld_out;
    if (route == Route::kFailed && path == 1) {   // (else interp_fwd_kernel wrote them)
        write_failed<Tv, D>(prow, 0, 1, T, x_out + l * D, 0, 1);
        write_failed<Tv, D>(frow, plane_stride, K, T, x_out + l * D, 0, 1);
    }
    if (route != Route::kSerial) return;
    double A[NN], G[NN], Kg[D], x[D];
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; G[i] = tb[B::G + i]; }
    for (int i = 0; i < D; i++) { Kg[i] = tb[B::K + i]; x[i] = (double)x_in[l * D + i]; }
    const Tv* yrow = Ty + l * ld_in;
    for (size_t t = 0; t < T; t++) {
        double xp[D];
        matvec<double, D>(A, x, xp);
        const double y = (double)yrow[t], p = xp[0];
        const double v = isnan(y) ? 0.0 : y - p;
        for (int j = 0; j < D; j++) x[j] = fma(Kg[j], v, xp[j]);
        prow[t] = (Tv)p;
        for (int k = 0; k < K; k++) {
            double q = 0.0;
            for (int j = 0; j < D; j++) q = fma(tw[W::AROW + k * D + j], x[j], q);
            frow[(size_t)k * plane_stride + t] = (Tv)q;
        }
    }
    for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)x[i];
    double s[D];
    for (int i = 0; i < D; i++) s[i] = 0.0;
    for (size_t t = T; t-- > 0;) {
        for (int k = 0; k < K; k++) {
            double c = (double)frow[(size_t)k * plane_stride + t];
            for (int j = 0; j < D; j++) c = fma(tw[W::GROW + k * D + j], s[j], c);
            frow[(size_t)k * plane_stride + t] = (Tv)c;
        }
        const double y = (double)yrow[t], p = (double)prow[t];
        const double v = isnan(y) ? 0.0 : y - p;
        tick_step<double, D>(G, Kg, v, s);
        prow[t] = (Tv)(p + s[0]);
    }
}

}  // namespace
}  // namespace moihgp

// ---- the tables: fp64, written for accuracy (no contraction, as smoother.hip's) ---------------------------------------------------------------
#pragma clang fp contract(off)
#include "stationary_common.h"

namespace moihgp {
namespace {

template <int D>
__global__ void __launch_bounds__(64) interp_tables_kernel(int kernel, const double* __restrict__ cb64, const double* __restrict__ sm, size_t L,
                                                           double dt, InterpFracs fracs, int K, double* __restrict__ it) {
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
    double Fa[NN], Fb[NN], Ap[NN], Bp[NN], ApT[NN], T1[NN], T2[NN], Pp[NN], P[NN], X[NN];
    for (int i = 0; i < NN; i++) { Fa[i] = ss.F[i] * (phi * dt); Fb[i] = ss.F[i] * ((1.0 - phi) * dt); P[i] = s[S::P + i]; }
    expm<D>(Fa, Ap);
    expm<D>(Fb, Bp);
    mt<D>(Ap, ApT);
    // P_phi = A_phi PF A_phi^T + Pinf - A_phi Pinf A_phi^T
    mm<D>(Ap, s + S::PF, T1); mm<D>(T1, ApT, Pp);
    mm<D>(Ap, ss.Pinf, T1); mm<D>(T1, ApT, T2);
    for (int i = 0; i < NN; i++) Pp[i] = Pp[i] + ss.Pinf[i] - T2[i];
    // G_phi^T = P^-1 B_phi P_phi (P and P_phi are symmetric): row 0 of G_phi is column 0 of the solve
    mm<D>(Bp, Pp, T1);
    lu_solve<D>(P, T1, X);
    double g[D];
    for (int j = 0; j < D; j++) g[j] = X[j * D];
    double q = 0.0;
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) q += g[i] * (s[S::PS + i * D + j] - P[i * D + j]) * g[j];
    const double nan = __builtin_nan("");
    for (int j = 0; j < D; j++) {
        o[W::AROW + k * D + j] = failed ? nan : Ap[j];
        o[W::GROW + k * D + j] = failed ? nan : g[j];
    }
    o[W::VAR + k] = failed ? nan : Pp[0] + q;
    if (k == K - 1)
        for (int kk = K; kk < kInterpMaxPoints; kk++) {
            for (int j = 0; j < D; j++) { o[W::AROW + kk * D + j] = 0.0; o[W::GROW + kk * D + j] = 0.0; }
            o[W::VAR + kk] = 0.0;
        }
    if (k == 0) o[W::STATUS] = failed ? 1.0 : 0.0;
}

}  // namespace

void launch_interp_tables(int kernel, int d, const double* cb64, const double* sm, size_t L, double dt, const InterpFracs& fracs, int K, double* it,
                          hipStream_t stream) {
    if (L == 0) return;
    dim3 block(64), grid((unsigned)((L * (size_t)K + 63) / 64));
    dispatch_dim(d, [&](auto dim) {
        hipLaunchKernelGGL((interp_tables_kernel<decltype(dim)::value>), grid, block, 0, stream, kernel, cb64, sm, L, dt, fracs, K, it);
    });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

// The call's record and its planes are unpacked here, at the launch lines.
template <typename Tv, int D, int KG>
static void launch_scan_kg(const SweepIo& io, const double* sm, const double* it, const SweepPlanes& out, int path, bool backward) {
    const size_t lds = sizeof(Tv) * (size_t)KG * kScanPlane;
    hipLaunchKernelGGL((interp_fwd_kernel<Tv, D, KG>), dim3((unsigned)io.L), dim3(64), lds, io.stream, (const Tv*)io.Ty, io.T, io.ld, sm, it, out.K,
                       (const Tv*)io.xin, (Tv*)io.x, (Tv*)io.yhat, (Tv*)out.base, io.ld_out, out.stride, path);
    MOIHGP_HIP_FATAL(hipGetLastError());
    if (!backward) return;
    hipLaunchKernelGGL((interp_bwd_kernel<Tv, D, KG>), dim3((unsigned)io.L), dim3(64), lds + sizeof(Tv) * kScanPlane, io.stream, (const Tv*)io.Ty, io.T,
                       io.ld, sm, it, out.K, (Tv*)io.yhat, (Tv*)out.base, io.ld_out, out.stride, path);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

// backward = false: the forward sweep alone (slope.hip, given the past: the rows g_k of `it` are zero)
static void launch_sweeps(int d, const SweepIo& io, const double* sm, const double* it, const SweepPlanes& out, int* status, int path, bool backward) {
    if (io.L == 0) return;
    dispatch_stream(d, io.dtype, [&](auto tv, auto dim) {
        using Tv = decltype(tv);
        constexpr int D = decltype(dim)::value;
        if (io.T > 0 && path != 1) {
            // planes staged per replay: one for a single offset, else two (at fp64 26 KB of LDS per wavefront in either sweep, at fp32 17 KB and 13 KB)
            if (out.K == 1) launch_scan_kg<Tv, D, 1>(io, sm, it, out, path, backward);
            else launch_scan_kg<Tv, D, 2>(io, sm, it, out, path, backward);
        }
        hipLaunchKernelGGL((interp_serial_kernel<Tv, D>), dim3((unsigned)((io.L + 63) / 64)), dim3(64), 0, io.stream, (const Tv*)io.Ty, io.T, io.ld, sm, it,
                           io.L, out.K, (const Tv*)io.xin, (Tv*)io.x, (Tv*)io.yhat, (Tv*)out.base, io.ld_out, out.stride, status, io.T > 0 ? path : 1);
    });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_interp_stream(int d, const SweepIo& io, const double* sm, const double* it, const SweepPlanes& out, int* status, int path) {
    launch_sweeps(d, io, sm, it, out, status, path, true);
}

void launch_interp_forward(int d, const SweepIo& io, const double* sm, const double* it, const SweepPlanes& out, int* status, int path) {
    launch_sweeps(d, io, sm, it, out, status, path, false);
}

}  // namespace moihgp
