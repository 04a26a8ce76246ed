// smoother.hip -- steady-state Rauch-Tung-Striebel smoothing of whole series-major streams (include/moihgp.h moihgp_smooth_stream).
//
// Per latent the model of the handle's hyper-parameters (CB::PARAMS) and its transition A (CB::A), with the TEXTBOOK Kalman DARE
// (the learners' tables keep the reference's literal one, ihgp.h:125):
//   Q = sym(Pinf - A Pinf A^T);  P = A P A^T - A P H^T (H P H^T + R)^-1 H P A^T + Q;  S = P00 + R;  K = P H^T / S;  PF = P - K H P
//   G = PF A^T P^-1;  Ps = G Ps G^T + PF - G P G^T;  var_filtered = PF00, var_smoothed = Ps00
// and two sweeps with x_in the state before tick 0:
//   forward   xp[t] = A xf[t-1];  p[t] = xp[t]_0;  v[t] = y[t] - p[t] (0 where y[t] is NaN);  xf[t] = xp[t] + K v[t]
//   backward  s[T] = 0;  s[t] = G s[t+1] + K v[t];  ys[t] = p[t] + s[t]_0
// (the RTS form xs[t] = xf[t] + G (xs[t+1] - A xf[t]) with xf[t+1] - A xf[t] = K v[t+1]).
//
// Kernels
//   smoother_tables_kernel   one lane per latent, fp64: Pinf from the model code (stationary_common.h), the DARE by structure-preserving
//                            doubling and two Newton steps (relative residual <= 1e-12 or status 1), the d^2 x d^2 Stein solve for Ps, chunk powers
//                            and a growth bound.  Launch-latency work.
//   smooth_fwd_kernel        one wavefront per latent, 64 x kScanChunk-tick segments staged through LDS (coalesced in and out): each lane
//                            takes kScanChunk consecutive ticks, computes its chunk's affine map from a zero state, a Kogge-Stone scan of the
//                            maps over the 64 lanes gives every lane its true start state, and the lane replays its chunk writing p[t].
//                            Missing ticks (x <- A x) and the ragged tail (identity) make a lane's map its own product of tick maps.
//                            Its STATE_AT instance is the forward pass of the fixed-lag smoother (lagged.hip, launch_smooth_forward).
//   smooth_bwd_kernel        the same from the last segment to the first with the lane order mirrored: the map of every chunk is G^kScanChunk
//                            (the backward recursion is time-invariant even across missing ticks, v = 0 there; ticks past T carry v = 0
//                            into s[T] = 0, which is exact).  Reads y and p, writes ys (which may alias p).
//   smooth_serial_kernel     one lane per latent, fp64, tick by tick: the latents the scan kernels leave (growth bound failed, option
//                            "smoother_path" = 1), and the status word of every latent.  The NaN row of a latent whose DARE did not converge
//                            is written by smooth_fwd_kernel (by this kernel when it walks every latent).
// The S0 instances of the backward and the serial kernel also hand out s[0], the state the backward sweep holds when it leaves tick 0 (fp64 [L][d]):
// exact-edge smoothing (edges.hip) corrects the head of the row from it.
// Arithmetic is fp64 throughout; fp32 streams are widened on load and narrowed on store.  The chunk-scan machinery of the two sweep kernels is
// scan_sweep.h (shared with forecast.hip and sampler.hip; the backward chunk response is its chunk_response_bwd), the block layout SM<D>
// stream_tables.h, the Stein solve (stein_solve) and the chunk powers of the tables kernel stationary_common.h.
#include "scan_sweep.h"

namespace moihgp {
namespace {

// STATE_AT (the fixed-lag smoother's forward pass): x_out receives the filtered state after tick T_state - 1 (<= T; 0: x_in), from the replay of
// the lane that holds that tick, instead of the state that leaves the last segment.  A smooth is the instance without it.
template <typename Tv, int D, bool STATE_AT>
__global__ void __launch_bounds__(64) smooth_fwd_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ tabs,
                                                        const Tv* x_in, Tv* x_out, Tv* __restrict__ p_out, size_t ld_out, int path, size_t T_state) {
    using B = SM<D>;
    constexpr int NN = D * D;
    __shared__ double buf[kScanPlane];
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const double* tb = tabs + l * B::SIZE;
    const Tv* yrow = Ty + l * ld_in;
    Tv* prow = p_out + l * ld_out;
    const Route route = latent_route(tb[B::STATUS], tb[B::GROWTH], scan_growth_bound<double>(), path);
    if (route == Route::kFailed) write_failed<Tv, D>(prow, 0, 1, T, x_out + l * D, lane, 64);   // written coalesced here
    if (route != Route::kScan) return;
    double A[NN], AKHA[NN], MF[NN], K[D];
#pragma unroll
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; AKHA[i] = tb[B::AKHA + i]; MF[i] = tb[B::MF + i]; }
#pragma unroll
    for (int i = 0; i < D; i++) K[i] = tb[B::K + i];
    double xseg[D];
#pragma unroll
    for (int i = 0; i < D; i++) xseg[i] = (double)x_in[l * D + i];
    if (STATE_AT && T_state == 0 && lane == 0)
#pragma unroll
        for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)xseg[i];
    double* my = buf + lane * kScanPitch;
    for (size_t seg0 = 0; seg0 < T; seg0 += kScanSeg) {
        stage_in(yrow, seg0, T, lane, buf);
        __syncthreads();
        bool regular;
        const int n = lane_ticks(my, seg0, T, lane, regular);
        // 1. the chunk's map from a zero state; 2. scan over the lanes: the state before this lane's chunk
        double Phi[NN], r[D], xs[D];
        chunk_map<double, D>(my, n, regular, A, AKHA, MF, K, Phi, r);
        scan_maps<double, D, true>(Phi, r, lane);
        start_states<double, D, true>(Phi, r, xseg, xs, lane);
        // 3. replay: predicted means into the lane's row of buf (in place of y)
        for (int i = 0; i < n; i++) {
            double xp[D];
            matvec<double, D>(A, xs, xp);
            const double y = my[i], p = xp[0];
            const double v = isnan(y) ? 0.0 : y - p;
#pragma unroll
            for (int j = 0; j < D; j++) xs[j] = fma(K[j], v, xp[j]);
            my[i] = p;
            if (STATE_AT && seg0 + (size_t)lane * kScanChunk + i + 1 == T_state)
#pragma unroll
                for (int j = 0; j < D; j++) x_out[l * D + j] = (Tv)xs[j];
        }
        __syncthreads();
        stage_out(buf, prow, seg0, T, lane);
        __syncthreads();
    }
    if (!STATE_AT && lane == 0)
#pragma unroll
        for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)xseg[i];
}

// S0 (exact-edge smoothing, edges.hip): s0 [L][D] receives the state s[0] the sweep holds when it leaves tick 0.  A smooth is the instance without it.
template <typename Tv, int D, bool S0>
__global__ void __launch_bounds__(64) smooth_bwd_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ tabs,
                                                        Tv* ys, size_t ld_out, int path, double* s0) {
    using B = SM<D>;
    constexpr int NN = D * D;
    __shared__ double vb[kScanPlane];
    __shared__ double pb[kScanPlane];
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const double* tb = tabs + l * B::SIZE;
    if (latent_route(tb[B::STATUS], tb[B::GROWTH], scan_growth_bound<double>(), path) != Route::kScan) return;
    double G[NN], MB[NN], K[D];
#pragma unroll
    for (int i = 0; i < NN; i++) { G[i] = tb[B::G + i]; MB[i] = tb[B::MB + i]; }
#pragma unroll
    for (int i = 0; i < D; i++) K[i] = tb[B::K + i];
    double sseg[D];
#pragma unroll
    for (int i = 0; i < D; i++) sseg[i] = 0.0;
    const Tv* yrow = Ty + l * ld_in;
    Tv* prow = ys + l * ld_out;
    const double* v = vb + lane * kScanPitch;
    double* pw = pb + lane * kScanPitch;
    const size_t nseg = (T + kScanSeg - 1) / kScanSeg;
    for (size_t sg = nseg; sg-- > 0;) {
        const size_t seg0 = sg * kScanSeg;
#pragma unroll
        for (int k = 0; k < kScanChunk; k++) {   // as stage_in, of v = y - p and p
            const int tl = k * 64 + lane;
            const size_t t = seg0 + tl;
            double y = 0.0, p = 0.0;
            if (t < T) { y = (double)yrow[t]; p = (double)prow[t]; }
            vb[scan_slot(tl)] = (t < T && !isnan(y)) ? y - p : 0.0;
            pb[scan_slot(tl)] = p;
        }
        __syncthreads();
        // 1. the chunk's response from a zero state at its end (its map is G^kScanChunk for every lane)
        double Phi[NN], r[D], s[D];
#pragma unroll
        for (int i = 0; i < NN; i++) Phi[i] = MB[i];
        chunk_response_bwd<double, D>(v, G, K, r);
        // 2. mirrored scan: the state entering this lane's chunk from the right
        scan_maps<double, D, false>(Phi, r, lane);
        start_states<double, D, false>(Phi, r, sseg, s, lane);
        // 3. replay: ys = p + s_0 (in place of p)
        for (int i = kScanChunk - 1; i >= 0; i--) {
            tick_step<double, D>(G, K, v[i], s);
            pw[i] += s[0];
        }
        __syncthreads();
        stage_out(pb, prow, seg0, T, lane);
        __syncthreads();
    }
    if (S0 && lane == 0)
#pragma unroll
        for (int i = 0; i < D; i++) s0[l * D + i] = sseg[i];
}

// Tick by tick, one lane per latent: the latents the scan kernels do not take, the NaN rows of latents whose DARE failed, every status word.
template <typename Tv, int D, bool S0>
__global__ void __launch_bounds__(64) smooth_serial_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ tabs, size_t L,
                                                           const Tv* x_in, Tv* x_out, Tv* ys, size_t ld_out, int* status, int path, double* s0) {
    using B = SM<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* tb = tabs + l * B::SIZE;
    const Route route = latent_route(tb[B::STATUS], tb[B::GROWTH], scan_growth_bound<double>(), path);
    if (status) status[l] = route == Route::kFailed ? 1 : 0;
    Tv* prow = ys + l * ld_out;
    if (route == Route::kFailed && path == 1) write_failed<Tv, D>(prow, 0, 1, T, x_out + l * D, 0, 1);   // (else smooth_fwd_kernel wrote them)
    if (route != Route::kSerial) return;
    double A[NN], G[NN], K[D], x[D];
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; G[i] = tb[B::G + i]; }
    for (int i = 0; i < D; i++) { K[i] = tb[B::K + i]; x[i] = (double)x_in[l * D + i]; }
    const Tv* yrow = Ty + l * ld_in;
    for (size_t t = 0; t < T; t++) {
        double xp[D];
        matvec<double, D>(A, x, xp);
        const double y = (double)yrow[t], p = xp[0];
        const double v = isnan(y) ? 0.0 : y - p;
        for (int j = 0; j < D; j++) x[j] = fma(K[j], v, xp[j]);
        prow[t] = (Tv)p;
    }
    for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)x[i];
    double s[D];
    for (int i = 0; i < D; i++) s[i] = 0.0;
    for (size_t t = T; t-- > 0;) {
        const double y = (double)yrow[t], p = (double)prow[t];
        const double v = isnan(y) ? 0.0 : y - p;
        tick_step<double, D>(G, K, v, s);
        prow[t] = (Tv)(p + s[0]);
    }
    if (S0)
        for (int i = 0; i < D; i++) s0[l * D + i] = s[i];
}

}  // namespace
}  // namespace moihgp

// ---- the tables: fp64, one lane per latent, written for accuracy (no contraction, as stationary.hip) -------------------------------------
#pragma clang fp contract(off)
#include "stationary_common.h"

namespace moihgp {
namespace {

template <int D>
__global__ void __launch_bounds__(64) smoother_tables_kernel(int kernel, const double* __restrict__ cb64, size_t L, double* __restrict__ tabs) {
    using B = SM<D>;
    using C = CB<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* cb = cb64 + l * C::SIZE;
    double* o = tabs + l * B::SIZE;
    double prm[3] = {cb[C::PARAMS + 0], cb[C::PARAMS + 1], cb[C::PARAMS + 2]};
    SS<D> s;
    ss_build<D>(kernel, prm, s);
    const double R = s.R;
    double A[NN], AT[NN], T1[NN], T2[NN], Q[NN];
    for (int i = 0; i < NN; i++) A[i] = cb[C::A + i];
    mt<D>(A, AT);
    mm<D>(A, s.Pinf, T1); mm<D>(T1, AT, T2);
    for (int i = 0; i < NN; i++) T1[i] = s.Pinf[i] - T2[i];
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) Q[i * D + j] = (T1[i * D + j] + T1[j * D + i]) / 2.0;

    // Kalman DARE by structure-preserving doubling on the dual (control) form with A_c = A^T, B_c = H^T:
    //   Ak+1 = Ak W Ak,  Gk+1 = Gk + Ak W Gk Ak^T,  Hk+1 = Hk + Ak^T Hk W Ak,  W = (I + Gk Hk)^-1;  A0 = A^T, G0 = H^T H / R, H0 = Q;  Hk -> P
    double Ak[NN], Gk[NN], Hk[NN], I[NN];
    for (int i = 0; i < NN; i++) { Ak[i] = AT[i]; Gk[i] = 0.0; Hk[i] = Q[i]; I[i] = (i % (D + 1)) == 0 ? 1.0 : 0.0; }
    Gk[0] = 1.0 / R;
    for (int it = 0; it < 64; it++) {
        double Den[NN], WA[NN], WG[NN], An[NN], Gn[NN], Hn[NN], AkT[NN];
        mm<D>(Gk, Hk, T1);
        for (int i = 0; i < NN; i++) Den[i] = I[i] + T1[i];
        lu_solve<D>(Den, Ak, WA);                 // W Ak
        lu_solve<D>(Den, Gk, WG);                 // W Gk
        mt<D>(Ak, AkT);
        mm<D>(Ak, WA, An);
        mm<D>(Ak, WG, T1); mm<D>(T1, AkT, T2);
        for (int i = 0; i < NN; i++) Gn[i] = Gk[i] + T2[i];
        mm<D>(AkT, Hk, T1); mm<D>(T1, WA, T2);
        for (int i = 0; i < NN; i++) Hn[i] = Hk[i] + T2[i];
        double dif = 0.0;
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) {
                const double h = (Hn[i * D + j] + Hn[j * D + i]) / 2.0, g = (Gn[i * D + j] + Gn[j * D + i]) / 2.0;
                dif = fmax(dif, fabs(h - Hk[i * D + j]));
                T1[i * D + j] = h; T2[i * D + j] = g;
            }
        for (int i = 0; i < NN; i++) { Ak[i] = An[i]; Hk[i] = T1[i]; Gk[i] = T2[i]; }
        if (!(dif > 1e-16 * max_abs<D>(Hk))) break;   // (NaN stops too; the residual below decides)
    }
    double P[NN];
    for (int i = 0; i < NN; i++) P[i] = Hk[i];
    // Kalman-form residual  Res(P) = A P A^T - A P H^T H P A^T / S + Q - P  (max |.|, relative to max |P|)
    auto residual = [&](double* Res) {
        const double Sr = P[0] + R;
        double AP[NN], APAt[NN];
        mm<D>(A, P, AP); mm<D>(AP, AT, APAt);
        double m = 0.0;
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) {
                Res[i * D + j] = APAt[i * D + j] - AP[i * D] * AP[j * D] / Sr + Q[i * D + j] - P[i * D + j];
                m = fmax(m, fabs(Res[i * D + j]));
            }
        const double pm = max_abs<D>(P);
        return pm > 0.0 ? m / pm : m;
    };
    // Doubling alone leaves up to ~1e-10 on these models (Q = Pinf - A Pinf A^T is indefinite for Matern-5/2 with the reference's
    // lam = sqrt(3)/l): two Newton steps in residual form take P to rounding.  The step dP solves dP = Ac dP Ac^T + Res(P), the Riccati
    // map linearised at P, with the closed loop Ac = A - A P H^T H / S (exact d^2 x d^2 solve, as for Ps below).
    for (int step = 0; step < 2; step++) {
        double Res[NN];
        const double r = residual(Res);
        if (!(r > 0.0) || !isfinite(r)) break;
        const double Sr = P[0] + R;
        double Ac[NN], AP0[D];
        for (int i = 0; i < D; i++) { double t = 0.0; for (int k = 0; k < D; k++) t += A[i * D + k] * P[k * D]; AP0[i] = t; }
        for (int i = 0; i < NN; i++) Ac[i] = A[i];
        for (int i = 0; i < D; i++) Ac[i * D] -= AP0[i] / Sr;
        double dP[NN];
        stein_solve<D>(Ac, Res, dP);
        double Pn[NN];
        bool fin = true;
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) { Pn[i * D + j] = P[i * D + j] + dP[i * D + j]; fin = fin && isfinite(Pn[i * D + j]); }
        if (!fin) break;
        for (int i = 0; i < NN; i++) P[i] = Pn[i];
    }
    double Res[NN];
    const double res = residual(Res);
    const double S = P[0] + R;
    double K[D];
    for (int i = 0; i < D; i++) K[i] = P[i * D] / S;
    const bool ok = isfinite(res) && res <= 1e-12 && isfinite(S) && S > 0.0;

    double PF[NN], HA[D], AKHA[NN], Pinv[NN], G[NN], Ps[NN];
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) PF[i * D + j] = P[i * D + j] - K[i] * P[j];
    for (int j = 0; j < D; j++) HA[j] = A[j];
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) AKHA[i * D + j] = A[i * D + j] - K[i] * HA[j];
    lu_solve<D>(P, I, Pinv);
    mm<D>(PF, AT, T1); mm<D>(T1, Pinv, G);
    // Ps = G Ps G^T + PF - G P G^T
    mm<D>(G, P, T1); mt<D>(G, T2); mm<D>(T1, T2, T1);
    for (int i = 0; i < NN; i++) T1[i] = PF[i] - T1[i];
    stein_solve<D>(G, T1, Ps);
    // chunk powers and the growth figure (inf-norm of G^k and AKHA^k, k <= 2 kScanChunk)
    double MB[NN], MF[NN];
    const double growth = fmax(chunk_powers<D, kScanChunk>(G, MB, T1), chunk_powers<D, kScanChunk>(AKHA, MF, T1));
    for (int i = 0; i < NN; i++) {
        o[B::A + i] = A[i]; o[B::AKHA + i] = AKHA[i]; o[B::G + i] = G[i]; o[B::MF + i] = MF[i]; o[B::MB + i] = MB[i];
        o[B::P + i] = P[i]; o[B::PF + i] = PF[i]; o[B::PS + i] = Ps[i];
    }
    for (int i = 0; i < D; i++) o[B::K + i] = K[i];
    o[B::VARF] = PF[0];
    o[B::VARS] = Ps[0];
    o[B::GROWTH] = growth;
    o[B::RESID] = res;
    bool fin = isfinite(Ps[0]) && isfinite(PF[0]);
    for (int i = 0; i < NN; i++) fin = fin && isfinite(G[i]) && isfinite(Ps[i]);
    o[B::STATUS] = (ok && fin) ? 0.0 : 1.0;
}

}  // namespace

void launch_smoother_tables(int kernel, int d, const double* cb64, size_t L, double* tabs, hipStream_t stream) {
    if (L == 0) return;
    dim3 block(64), grid((unsigned)((L + 63) / 64));
    dispatch_dim(d, [&](auto dim) { hipLaunchKernelGGL((smoother_tables_kernel<decltype(dim)::value>), grid, block, 0, stream, kernel, cb64, L, tabs); });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

// The call's record is unpacked here, at the launch lines: forward and backward scan sweeps for the latents that take them, then the serial kernel
// for the rest and the status words.  S0: the instances that hand out s[0] (exact-edge smoothing).
template <typename Tv, int D, bool S0>
static void launch_smooth_t(const SweepIo& io, const double* tabs, int* status, int path, double* s0) {
    const Tv *Ty = (const Tv*)io.Ty, *x_in = (const Tv*)io.xin;
    Tv *x = (Tv*)io.x, *ys = (Tv*)io.yhat;
    const size_t T = io.T, L = io.L;
    if (T > 0 && path != 1) {
        hipLaunchKernelGGL((smooth_fwd_kernel<Tv, D, false>), dim3((unsigned)L), dim3(64), 0, io.stream, Ty, T, io.ld, tabs, x_in, x, ys, io.ld_out, path, T);
        MOIHGP_HIP_FATAL(hipGetLastError());
        hipLaunchKernelGGL((smooth_bwd_kernel<Tv, D, S0>), dim3((unsigned)L), dim3(64), 0, io.stream, Ty, T, io.ld, tabs, ys, io.ld_out, path, s0);
        MOIHGP_HIP_FATAL(hipGetLastError());
    }
    hipLaunchKernelGGL((smooth_serial_kernel<Tv, D, S0>), dim3((unsigned)((L + 63) / 64)), dim3(64), 0, io.stream, Ty, T, io.ld, tabs, L, x_in, x, ys, io.ld_out,
                       status, T > 0 ? path : 1, s0);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_smooth_stream(int d, const SweepIo& io, const double* tabs, int* status, int path, double* s0) {
    if (io.L == 0) return;
    dispatch_stream(d, io.dtype, [&](auto tv, auto dim) {
        if (s0) launch_smooth_t<decltype(tv), decltype(dim)::value, true>(io, tabs, status, path, s0);
        else launch_smooth_t<decltype(tv), decltype(dim)::value, false>(io, tabs, status, path, nullptr);
    });
}

void launch_smooth_forward(int d, const SweepIo& io, const double* tabs, size_t T_state, int path) {
    if (io.L == 0 || io.T == 0) return;
    dispatch_stream(d, io.dtype, [&](auto tv, auto dim) {
        using Tv = decltype(tv);
        hipLaunchKernelGGL((smooth_fwd_kernel<Tv, decltype(dim)::value, true>), dim3((unsigned)io.L), dim3(64), 0, io.stream, (const Tv*)io.Ty, io.T, io.ld,
                           tabs, (const Tv*)io.xin, (Tv*)io.x, (Tv*)io.yhat, io.ld_out, path, T_state);
    });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

}  // namespace moihgp
