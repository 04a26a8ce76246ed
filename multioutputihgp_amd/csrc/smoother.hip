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
//   smooth_fwd_kernel        one wavefront per latent, 64 x kSmChunk-tick segments staged through LDS (coalesced in and out): each lane
//                            takes kSmChunk consecutive ticks, computes its chunk's affine map from a zero state, a Kogge-Stone scan of the
//                            maps over the 64 lanes gives every lane its true start state, and the lane replays its chunk writing p[t].
//                            Missing ticks (x <- A x) and the ragged tail (identity) make a lane's map its own product of tick maps.
//   smooth_bwd_kernel        the same from the last segment to the first with the lane order mirrored: the map of every chunk is G^kSmChunk
//                            (the backward recursion is time-invariant even across missing ticks, v = 0 there; ticks past T carry v = 0
//                            into s[T] = 0, which is exact).  Reads y and p, writes ys (which may alias p).
//   smooth_serial_kernel     one lane per latent, fp64, tick by tick: the latents the scan kernels leave (growth bound failed, option
//                            "smoother_path" = 1), and the status word of every latent.  The NaN row of a latent whose DARE did not converge
//                            is written by smooth_fwd_kernel (by this kernel when it walks every latent).
// Arithmetic is fp64 throughout; fp32 streams are widened on load and narrowed on store.
#include "common.h"

namespace moihgp {
namespace {

constexpr int kSmChunk = 16;                    // ticks per lane per segment (1024-tick segments)
constexpr int kSmSeg = 64 * kSmChunk;
constexpr int kSmPitch = kSmChunk + 1;          // LDS row pitch of one lane's chunk (odd: no bank conflicts between lanes)

// per-latent smoother block (fp64), offsets in doubles
template <int D>
struct SM {
    static constexpr int NN = D * D;
    static constexpr int A = 0, AKHA = A + NN, K = AKHA + NN, G = K + D;   // AKHA = A - K H A
    static constexpr int MF = G + NN;           // AKHA^kSmChunk
    static constexpr int MB = MF + NN;          // G^kSmChunk
    static constexpr int P = MB + NN, PF = P + NN, PS = PF + NN;
    static constexpr int VARF = PS + NN, VARS = VARF + 1, GROWTH = VARS + 1, RESID = GROWTH + 1, STATUS = RESID + 1;
    static constexpr int SIZE = (STATUS + 1 + 1) / 2 * 2;
};

// a latent's scan kernels are usable when its DARE converged and no power of G or AKHA up to 2 kSmChunk exceeds this (inf-norm): the
// zero-state chunk responses then lose at most ~log10(bound) digits to cancellation
constexpr double kSmGrowthBound = 1e4;

__device__ inline bool scan_ok(const double* tb, int status_off, int growth_off) {
    return tb[status_off] == 0.0 && tb[growth_off] <= kSmGrowthBound;
}

template <int D>
__device__ inline void matvec(const double* M, const double* x, double* y) {
#pragma unroll
    for (int i = 0; i < D; i++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < D; k++) s = fma(M[i * D + k], x[k], s);
        y[i] = s;
    }
}
template <int D>
__device__ inline void matmul(const double* X, const double* Y, double* Z) {
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
        for (int j = 0; j < D; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < D; k++) s = fma(X[i * D + k], Y[k * D + j], s);
            Z[i * D + j] = s;
        }
}

// Inclusive Kogge-Stone scan of affine maps (Phi, r) over the wavefront.  FWD: lane j ends with the composition of lanes 0..j (lane 0 first);
// otherwise lanes j..63 with lane 63 first (the backward sweep walks time from the end).
template <int D, bool FWD>
__device__ inline void scan_maps(double* Phi, double* r, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        double Po[D * D], ro[D];
#pragma unroll
        for (int i = 0; i < D * D; i++) Po[i] = FWD ? __shfl_up(Phi[i], off, 64) : __shfl_down(Phi[i], off, 64);
#pragma unroll
        for (int i = 0; i < D; i++) ro[i] = FWD ? __shfl_up(r[i], off, 64) : __shfl_down(r[i], off, 64);
        const bool has = FWD ? lane >= off : lane + off < 64;
        if (has) {
            double Pn[D * D], rn[D];
            matmul<D>(Phi, Po, Pn);
            matvec<D>(Phi, ro, rn);
#pragma unroll
            for (int i = 0; i < D * D; i++) Phi[i] = Pn[i];
#pragma unroll
            for (int i = 0; i < D; i++) r[i] += rn[i];
        }
    }
}

template <typename Tv, int D>
__global__ void __launch_bounds__(64) smooth_fwd_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ tabs,
                                                        const Tv* x_in, Tv* x_out, Tv* __restrict__ p_out, size_t ld_out, int path) {
    using B = SM<D>;
    constexpr int NN = D * D;
    __shared__ double buf[64 * kSmPitch];
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const double* tb = tabs + l * B::SIZE;
    if (path == 1) return;                                                              // smooth_serial_kernel's
    if (tb[B::STATUS] != 0.0) {   // DARE not converged: NaN row and end state, written coalesced here
        const Tv nan = (Tv)__builtin_nan("");
        for (size_t t = lane; t < T; t += 64) p_out[l * ld_out + t] = nan;
        if (lane < D) x_out[l * D + lane] = nan;
        return;
    }
    if (path == -1 && !scan_ok(tb, B::STATUS, B::GROWTH)) return;                      // smooth_serial_kernel's
    double A[NN], AKHA[NN], MF[NN], K[D];
#pragma unroll
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; AKHA[i] = tb[B::AKHA + i]; MF[i] = tb[B::MF + i]; }
#pragma unroll
    for (int i = 0; i < D; i++) K[i] = tb[B::K + i];
    double xseg[D];
#pragma unroll
    for (int i = 0; i < D; i++) xseg[i] = (double)x_in[l * D + i];
    const Tv* yrow = Ty + l * ld_in;
    Tv* prow = p_out + l * ld_out;
    for (size_t seg0 = 0; seg0 < T; seg0 += kSmSeg) {
        // coalesced load: tick seg0 + k*64 + lane lands in lane (k*64+lane)/kSmChunk's row
#pragma unroll
        for (int k = 0; k < kSmChunk; k++) {
            const int tl = k * 64 + lane;
            const size_t t = seg0 + tl;
            buf[(tl / kSmChunk) * kSmPitch + tl % kSmChunk] = t < T ? (double)yrow[t] : 0.0;
        }
        __syncthreads();
        const double* my = buf + lane * kSmPitch;
        const size_t t0 = seg0 + (size_t)lane * kSmChunk;
        const int n = t0 >= T ? 0 : (int)((T - t0) < (size_t)kSmChunk ? (T - t0) : (size_t)kSmChunk);   // valid ticks of this lane
        bool regular = n == kSmChunk;
        for (int i = 0; i < n; i++) regular &= !isnan(my[i]);
        // 1. the chunk's map from a zero state
        double Phi[NN], r[D];
#pragma unroll
        for (int i = 0; i < D; i++) r[i] = 0.0;
        if (regular) {
#pragma unroll
            for (int i = 0; i < NN; i++) Phi[i] = MF[i];
            for (int i = 0; i < kSmChunk; i++) {
                double rn[D];
                matvec<D>(AKHA, r, rn);
                const double y = my[i];
#pragma unroll
                for (int j = 0; j < D; j++) r[j] = fma(K[j], y, rn[j]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NN; i++) Phi[i] = (i % (D + 1)) == 0 ? 1.0 : 0.0;
            for (int i = 0; i < n; i++) {
                const double y = my[i];
                const bool miss = isnan(y);
                const double* M = miss ? A : AKHA;
                double rn[D], Pn[NN];
                matvec<D>(M, r, rn);
                matmul<D>(M, Phi, Pn);
#pragma unroll
                for (int j = 0; j < D; j++) r[j] = miss ? rn[j] : fma(K[j], y, rn[j]);
#pragma unroll
                for (int j = 0; j < NN; j++) Phi[j] = Pn[j];
            }
        }
        // 2. scan over the lanes; the state before this lane's chunk is the inclusive map of lane - 1 applied to xseg
        scan_maps<D, true>(Phi, r, lane);
        double xs[D], xe[D];
        matvec<D>(Phi, xseg, xe);
#pragma unroll
        for (int i = 0; i < D; i++) xe[i] += r[i];
#pragma unroll
        for (int i = 0; i < D; i++) {
            const double prev = __shfl_up(xe[i], 1, 64);
            xs[i] = lane == 0 ? xseg[i] : prev;
            xseg[i] = __shfl(xe[i], 63, 64);
        }
        // 3. replay: predicted means into the lane's row of buf (in place of y)
        double* myw = buf + lane * kSmPitch;
        for (int i = 0; i < n; i++) {
            double xp[D];
            matvec<D>(A, xs, xp);
            const double y = myw[i], p = xp[0];
            const double v = isnan(y) ? 0.0 : y - p;
#pragma unroll
            for (int j = 0; j < D; j++) xs[j] = fma(K[j], v, xp[j]);
            myw[i] = p;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSmChunk; k++) {
            const int tl = k * 64 + lane;
            const size_t t = seg0 + tl;
            if (t < T) prow[t] = (Tv)buf[(tl / kSmChunk) * kSmPitch + tl % kSmChunk];
        }
        __syncthreads();
    }
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)xseg[i];
}

template <typename Tv, int D>
__global__ void __launch_bounds__(64) smooth_bwd_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ tabs,
                                                        Tv* ys, size_t ld_out, int path) {
    using B = SM<D>;
    constexpr int NN = D * D;
    __shared__ double vb[64 * kSmPitch];
    __shared__ double pb[64 * kSmPitch];
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const double* tb = tabs + l * B::SIZE;
    if (path == 1 || tb[B::STATUS] != 0.0 || (path == -1 && !scan_ok(tb, B::STATUS, B::GROWTH))) return;
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
    const size_t nseg = (T + kSmSeg - 1) / kSmSeg;
    for (size_t sg = nseg; sg-- > 0;) {
        const size_t seg0 = sg * kSmSeg;
#pragma unroll
        for (int k = 0; k < kSmChunk; k++) {
            const int tl = k * 64 + lane;
            const size_t t = seg0 + tl;
            double y = 0.0, p = 0.0;
            if (t < T) { y = (double)yrow[t]; p = (double)prow[t]; }
            const int o = (tl / kSmChunk) * kSmPitch + tl % kSmChunk;
            vb[o] = (t < T && !isnan(y)) ? y - p : 0.0;
            pb[o] = p;
        }
        __syncthreads();
        const double* v = vb + lane * kSmPitch;
        // 1. the chunk's response from a zero state at its end (its map is G^kSmChunk for every lane)
        double Phi[NN], r[D];
#pragma unroll
        for (int i = 0; i < NN; i++) Phi[i] = MB[i];
#pragma unroll
        for (int i = 0; i < D; i++) r[i] = 0.0;
        for (int i = kSmChunk - 1; i >= 0; i--) {
            double rn[D];
            matvec<D>(G, r, rn);
            const double vi = v[i];
#pragma unroll
            for (int j = 0; j < D; j++) r[j] = fma(K[j], vi, rn[j]);
        }
        // 2. mirrored scan: the state entering this lane's chunk from the right is the inclusive map of lane + 1 applied to sseg
        scan_maps<D, false>(Phi, r, lane);
        double s[D], se[D];
        matvec<D>(Phi, sseg, se);
#pragma unroll
        for (int i = 0; i < D; i++) se[i] += r[i];
#pragma unroll
        for (int i = 0; i < D; i++) {
            const double nxt = __shfl_down(se[i], 1, 64);
            s[i] = lane == 63 ? sseg[i] : nxt;
            sseg[i] = __shfl(se[i], 0, 64);
        }
        // 3. replay: ys = p + s_0 (in place of p)
        double* pw = pb + lane * kSmPitch;
        for (int i = kSmChunk - 1; i >= 0; i--) {
            double sn[D];
            matvec<D>(G, s, sn);
            const double vi = v[i];
#pragma unroll
            for (int j = 0; j < D; j++) s[j] = fma(K[j], vi, sn[j]);
            pw[i] += s[0];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSmChunk; k++) {
            const int tl = k * 64 + lane;
            const size_t t = seg0 + tl;
            if (t < T) prow[t] = (Tv)pb[(tl / kSmChunk) * kSmPitch + tl % kSmChunk];
        }
        __syncthreads();
    }
}

// Tick by tick, one lane per latent: the latents the scan kernels do not take, the NaN rows of latents whose DARE failed, every status word.
template <typename Tv, int D>
__global__ void __launch_bounds__(64) smooth_serial_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ tabs, size_t L,
                                                           const Tv* x_in, Tv* x_out, Tv* ys, size_t ld_out, int* status, int path) {
    using B = SM<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* tb = tabs + l * B::SIZE;
    const bool failed = tb[B::STATUS] != 0.0;
    if (status) status[l] = failed ? 1 : 0;
    Tv* prow = ys + l * ld_out;
    if (failed) {   // (with the scan kernels running, smooth_fwd_kernel writes this row coalesced)
        if (path == 1) {
            const Tv nan = (Tv)__builtin_nan("");
            for (size_t t = 0; t < T; t++) prow[t] = nan;
            for (int i = 0; i < D; i++) x_out[l * D + i] = nan;
        }
        return;
    }
    if (!(path == 1 || (path == -1 && !scan_ok(tb, B::STATUS, B::GROWTH)))) return;
    double A[NN], G[NN], K[D], x[D];
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; G[i] = tb[B::G + i]; }
    for (int i = 0; i < D; i++) { K[i] = tb[B::K + i]; x[i] = (double)x_in[l * D + i]; }
    const Tv* yrow = Ty + l * ld_in;
    for (size_t t = 0; t < T; t++) {
        double xp[D];
        matvec<D>(A, x, xp);
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
        double sn[D];
        matvec<D>(G, s, sn);
        for (int j = 0; j < D; j++) s[j] = fma(K[j], v, sn[j]);
        prow[t] = (Tv)(p + s[0]);
    }
}

}  // namespace
}  // namespace moihgp

// ---- the tables: fp64, one lane per latent, written for accuracy (no contraction, as stationary.hip) -------------------------------------
#pragma clang fp contract(off)
#include "stationary_common.h"

namespace moihgp {
namespace {

template <int D>
__device__ double max_abs(const double* X) {
    double m = 0.0;
    for (int i = 0; i < D * D; i++) m = fmax(m, fabs(X[i]));
    return m;
}
template <int D>
__device__ double norm_inf(const double* X) {
    double m = 0.0;
    for (int i = 0; i < D; i++) {
        double s = 0.0;
        for (int j = 0; j < D; j++) s += fabs(X[i * D + j]);
        m = fmax(m, s);
    }
    return m;
}

template <int D>
__global__ void __launch_bounds__(64) smoother_tables_kernel(int kernel, const double* __restrict__ cb64, size_t L, double* __restrict__ tabs) {
    using B = SM<D>;
    using C = CB<D>;
    constexpr int NN = D * D, N2 = NN * NN;
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
        double M[NN * NN], rhs[NN * NN], sol[NN * NN];
        for (int i = 0; i < NN * NN; i++) { M[i] = 0.0; rhs[i] = 0.0; }
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) {
                const int row = i * D + j;
                rhs[row * NN] = Res[row];
                for (int k = 0; k < D; k++)
                    for (int m = 0; m < D; m++) M[row * NN + k * D + m] = (row == k * D + m ? 1.0 : 0.0) - Ac[i * D + k] * Ac[j * D + m];
            }
        lu_solve<NN>(M, rhs, sol);
        double Pn[NN];
        bool fin = true;
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) { Pn[i * D + j] = P[i * D + j] + (sol[(i * D + j) * NN] + sol[(j * D + i) * NN]) / 2.0; fin = fin && isfinite(Pn[i * D + j]); }
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
    {   // Ps: (I - G (x) G) vec(Ps) = vec(PF - G P G^T), row-major vec
        double M[N2], rhs[N2], sol[N2];
        mm<D>(G, P, T1); mt<D>(G, T2); mm<D>(T1, T2, T1);
        for (int i = 0; i < N2; i++) { M[i] = 0.0; rhs[i] = 0.0; }
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) {
                const int row = i * D + j;
                rhs[row * NN] = PF[row] - T1[row];
                for (int k = 0; k < D; k++)
                    for (int m = 0; m < D; m++) M[row * NN + k * D + m] = (row == k * D + m ? 1.0 : 0.0) - G[i * D + k] * G[j * D + m];
            }
        lu_solve<NN>(M, rhs, sol);
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) Ps[i * D + j] = (sol[(i * D + j) * NN] + sol[(j * D + i) * NN]) / 2.0;
    }
    // chunk powers and the growth bound (inf-norm of G^k and AKHA^k, k <= 2 kSmChunk)
    double Gp[NN], Fp[NN], MB[NN], MF[NN], growth = 0.0;
    for (int i = 0; i < NN; i++) { Gp[i] = G[i]; Fp[i] = AKHA[i]; }
    for (int k = 1; k <= 2 * kSmChunk; k++) {
        if (k == kSmChunk) for (int i = 0; i < NN; i++) { MB[i] = Gp[i]; MF[i] = Fp[i]; }
        growth = fmax(growth, fmax(norm_inf<D>(Gp), norm_inf<D>(Fp)));
        if (!isfinite(growth)) growth = INFINITY;
        mm<D>(G, Gp, Gp); mm<D>(AKHA, Fp, Fp);
    }
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

int sm_size(int d) { return d == 2 ? SM<2>::SIZE : SM<3>::SIZE; }

void sm_offsets(int d, int* off) {
    // A AKHA K G MF MB P PF PS VARF VARS GROWTH RESID STATUS
    if (d == 2) { using B = SM<2>; const int o[] = {B::A, B::AKHA, B::K, B::G, B::MF, B::MB, B::P, B::PF, B::PS, B::VARF, B::VARS, B::GROWTH, B::RESID, B::STATUS}; for (int i = 0; i < 14; i++) off[i] = o[i]; }
    else        { using B = SM<3>; const int o[] = {B::A, B::AKHA, B::K, B::G, B::MF, B::MB, B::P, B::PF, B::PS, B::VARF, B::VARS, B::GROWTH, B::RESID, B::STATUS}; for (int i = 0; i < 14; i++) off[i] = o[i]; }
}

void launch_smoother_tables(int kernel, int d, const double* cb64, size_t L, double* tabs, hipStream_t stream) {
    if (L == 0) return;
    dim3 block(64), grid((unsigned)((L + 63) / 64));
    if (d == 2) hipLaunchKernelGGL((smoother_tables_kernel<2>), grid, block, 0, stream, kernel, cb64, L, tabs);
    else hipLaunchKernelGGL((smoother_tables_kernel<3>), grid, block, 0, stream, kernel, cb64, L, tabs);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

template <typename Tv, int D>
static void launch_smooth_t(const Tv* Ty, size_t T, size_t ld_in, size_t L, const double* tabs, const Tv* x_in, Tv* x, Tv* ys, size_t ld_out,
                            int* status, int path, hipStream_t stream) {
    if (T > 0 && path != 1) {
        hipLaunchKernelGGL((smooth_fwd_kernel<Tv, D>), dim3((unsigned)L), dim3(64), 0, stream, Ty, T, ld_in, tabs, x_in, x, ys, ld_out, path);
        MOIHGP_HIP_FATAL(hipGetLastError());
        hipLaunchKernelGGL((smooth_bwd_kernel<Tv, D>), dim3((unsigned)L), dim3(64), 0, stream, Ty, T, ld_in, tabs, ys, ld_out, path);
        MOIHGP_HIP_FATAL(hipGetLastError());
    }
    hipLaunchKernelGGL((smooth_serial_kernel<Tv, D>), dim3((unsigned)((L + 63) / 64)), dim3(64), 0, stream, Ty, T, ld_in, tabs, L, x_in, x, ys, ld_out,
                       status, T > 0 ? path : 1);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_smooth_stream(int d, int dtype, const void* Ty, size_t T, size_t ld_in, size_t L, const double* tabs, const void* x_in, void* x,
                          void* ys, size_t ld_out, int* status, int path, hipStream_t stream) {
    if (L == 0) return;
    if (dtype == 0) {
        if (d == 2) launch_smooth_t<double, 2>((const double*)Ty, T, ld_in, L, tabs, (const double*)x_in, (double*)x, (double*)ys, ld_out, status, path, stream);
        else launch_smooth_t<double, 3>((const double*)Ty, T, ld_in, L, tabs, (const double*)x_in, (double*)x, (double*)ys, ld_out, status, path, stream);
    } else {
        if (d == 2) launch_smooth_t<float, 2>((const float*)Ty, T, ld_in, L, tabs, (const float*)x_in, (float*)x, (float*)ys, ld_out, status, path, stream);
        else launch_smooth_t<float, 3>((const float*)Ty, T, ld_in, L, tabs, (const float*)x_in, (float*)x, (float*)ys, ld_out, status, path, stream);
    }
}

}  // namespace moihgp
