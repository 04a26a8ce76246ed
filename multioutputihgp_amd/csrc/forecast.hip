// forecast.hip -- multi-horizon forecasts of whole series-major streams (include/moihgp.h moihgp_forecast_stream / _tail / _variances).
//
// Per latent, with A the handle's transition, H = e0 and gains (K, M): the smoother's Kalman-form K with M = A - K H A (gains 0), or the
// handle's own K and AKHA (gains 1, the learners' filter):
//   x[t] = M x[t-1] + K y[t]   (x[t] = A x[t-1] where y[t] is NaN; x[-1] = x_in)
//   fc[k][t] = c_k . x[t],  c_k = H A^h_k          the mean at tick t + h_k given ticks <= t, stored at the tick the forecast is made at
//   var[k]   = Pinf_00 - c_k (Pinf - PF) c_k^T     (Kalman gains only)
//
// Kernels
//   forecast_tables_kernel   fp64, one lane per (latent, horizon): c_k by binary powering and var[k]; the lane of horizon 0 also copies A, M, K,
//                            builds M^kFcChunk and the growth figure the sweep's choice of path rests on.  An fp32 copy of the block is
//                            written next to the fp64 one.  Built per call: the rows depend on the call's horizons.
//   forecast_sweep_kernel    one wavefront per latent, 64 x kFcChunk-tick segments staged through LDS, as smooth_fwd_kernel: chunk maps from a
//                            zero state, a Kogge-Stone scan over the lanes, then each lane replays its chunk from its start state and writes
//                            KG dot products c_k . x[t] per tick into KG LDS planes, which leave coalesced.  More than KG horizons: the
//                            replay (not the scan) is repeated per group of KG.  Arithmetic in the stream's own precision.
//   forecast_serial_kernel   one lane per latent, fp64, tick by tick: latents whose M fails the growth bound (rho(AKHA) > 1 occurs with the
//                            handle's gains), option "forecast_path" = 1, and every status word.
//   forecast_tail_kernel     tail[l][j] = H A^(j+1) x_l, fp64: each lane powers A to its first index and then strides by A^64.
#include "common.h"

namespace moihgp {
namespace {

constexpr int kFcChunk = 16;                    // ticks per lane per segment (1024-tick segments)
constexpr int kFcSeg = 64 * kFcChunk;
constexpr int kFcPitch = kFcChunk + 1;          // LDS row pitch of one lane's chunk (odd: no bank conflicts between lanes)
constexpr int kFcPlane = 64 * kFcPitch;         // elements of one staged plane

// per-latent forecast block, offsets in scalars (the same in the fp64 and the fp32 copy)
template <int D>
struct FT {
    static constexpr int NN = D * D;
    static constexpr int A = 0, M = A + NN, K = M + NN, MF = K + D;   // MF = M^kFcChunk
    static constexpr int C = MF + NN;                                 // [kFcMaxHorizons][D]  c_k = H A^h_k (rows past the call's K are zero)
    static constexpr int VAR = C + kFcMaxHorizons * D;                // [kFcMaxHorizons]
    static constexpr int GROWTH = VAR + kFcMaxHorizons, STATUS = GROWTH + 1;
    static constexpr int SIZE = (STATUS + 1 + 3) / 4 * 4;
};

// The scan is used for a latent when no power of M up to 2 kFcChunk, nor M^kFcSeg, exceeds this in the inf-norm (the smoother's figure also
// covers its G, which no forecast uses: it is not consulted): the zero-state chunk responses and the composed maps of one segment then lose
// at most log10(bound) digits to cancellation.  fp64 keeps the smoother's bound; fp32 arithmetic (7 digits, 3 needed) affords two.
template <typename Ta> __host__ __device__ constexpr double fc_growth_bound() { return sizeof(Ta) == 8 ? 1e4 : 1e2; }

__device__ inline bool fc_scan_ok(const double* tb, int status_off, int growth_off, double bound) {
    return tb[status_off] == 0.0 && tb[growth_off] <= bound;
}

template <typename Ta> __device__ inline Ta fc_fma(Ta a, Ta b, Ta c);
template <> __device__ inline double fc_fma<double>(double a, double b, double c) { return fma(a, b, c); }
template <> __device__ inline float fc_fma<float>(float a, float b, float c) { return fmaf(a, b, c); }

template <typename Ta, int D>
__device__ inline void fc_matvec(const Ta* M, const Ta* x, Ta* y) {
#pragma unroll
    for (int i = 0; i < D; i++) {
        Ta s = 0;
#pragma unroll
        for (int k = 0; k < D; k++) s = fc_fma<Ta>(M[i * D + k], x[k], s);
        y[i] = s;
    }
}
template <typename Ta, int D>
__device__ inline void fc_matmul(const Ta* X, const Ta* Y, Ta* Z) {
#pragma unroll
    for (int i = 0; i < D; i++)
#pragma unroll
        for (int j = 0; j < D; j++) {
            Ta s = 0;
#pragma unroll
            for (int k = 0; k < D; k++) s = fc_fma<Ta>(X[i * D + k], Y[k * D + j], s);
            Z[i * D + j] = s;
        }
}

// Inclusive Kogge-Stone scan of affine maps (Phi, r) over the wavefront: lane j ends with the composition of lanes 0..j (lane 0 first).
template <typename Ta, int D>
__device__ inline void fc_scan_maps(Ta* Phi, Ta* r, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        Ta Po[D * D], ro[D];
#pragma unroll
        for (int i = 0; i < D * D; i++) Po[i] = __shfl_up(Phi[i], off, 64);
#pragma unroll
        for (int i = 0; i < D; i++) ro[i] = __shfl_up(r[i], off, 64);
        if (lane >= off) {
            Ta Pn[D * D], rn[D];
            fc_matmul<Ta, D>(Phi, Po, Pn);
            fc_matvec<Ta, D>(Phi, ro, rn);
#pragma unroll
            for (int i = 0; i < D * D; i++) Phi[i] = Pn[i];
#pragma unroll
            for (int i = 0; i < D; i++) r[i] += rn[i];
        }
    }
}

// Tv: the stream's scalar; Ta: the arithmetic (= Tv); KG: horizons staged per replay.  tabs: the Ta copy of the blocks; tabs64 decides the path.
// (waves per SIMD: at fp32 four, so that 16 wavefronts per CU hold 4096 latents in one round -- 128 VGPRs at d = 3, no scratch)
template <typename Tv, typename Ta, int D, int KG>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(sizeof(Ta) == 4 ? 4 : 2))) forecast_sweep_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const Ta* __restrict__ tabs,
                                                            const double* __restrict__ tabs64, const Tv* x_in, Tv* x_out, Tv* __restrict__ fc,
                                                            size_t ld_out, size_t plane_stride, int K, int path) {
    using B = FT<D>;
    constexpr int NN = D * D;
    extern __shared__ double fc_lds[];
    Ta* ybuf = reinterpret_cast<Ta*>(fc_lds);                  // [64][kFcPitch] the segment's y
    Ta* obuf = ybuf + kFcPlane;                                // [KG][64][kFcPitch] the group's planes
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const Ta* tb = tabs + l * B::SIZE;
    const double* tb64 = tabs64 + l * B::SIZE;
    if (path == 1) return;                                                                              // forecast_serial_kernel's
    if (tb64[B::STATUS] != 0.0) {   // Kalman DARE not converged: NaN rows and end state, written coalesced here
        const Tv nan = (Tv)__builtin_nan("");
        for (int k = 0; k < K; k++)
            for (size_t t = lane; t < T; t += 64) fc[(size_t)k * plane_stride + l * ld_out + t] = nan;
        if (lane < D) x_out[l * D + lane] = nan;
        return;
    }
    if (path == -1 && !fc_scan_ok(tb64, B::STATUS, B::GROWTH, fc_growth_bound<Ta>())) return;           // forecast_serial_kernel's
    Ta A[NN], M[NN], MF[NN], Kg[D];
#pragma unroll
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; M[i] = tb[B::M + i]; MF[i] = tb[B::MF + i]; }
#pragma unroll
    for (int i = 0; i < D; i++) Kg[i] = tb[B::K + i];
    Ta xseg[D];
#pragma unroll
    for (int i = 0; i < D; i++) xseg[i] = (Ta)x_in[l * D + i];
    const Tv* yrow = Ty + l * ld_in;
    Tv* frow = fc + l * ld_out;
    const Ta* my = ybuf + lane * kFcPitch;
    for (size_t seg0 = 0; seg0 < T; seg0 += kFcSeg) {
        // coalesced load: tick seg0 + k*64 + lane lands in lane (k*64+lane)/kFcChunk's row
#pragma unroll
        for (int k = 0; k < kFcChunk; k++) {
            const int tl = k * 64 + lane;
            const size_t t = seg0 + tl;
            ybuf[(tl / kFcChunk) * kFcPitch + tl % kFcChunk] = t < T ? (Ta)yrow[t] : (Ta)0;
        }
        __syncthreads();
        const size_t t0 = seg0 + (size_t)lane * kFcChunk;
        const int n = t0 >= T ? 0 : (int)((T - t0) < (size_t)kFcChunk ? (T - t0) : (size_t)kFcChunk);   // valid ticks of this lane
        bool regular = n == kFcChunk;
        for (int i = 0; i < n; i++) regular &= !isnan(my[i]);
        // 1. the chunk's map from a zero state
        Ta Phi[NN], r[D];
#pragma unroll
        for (int i = 0; i < D; i++) r[i] = 0;
        if (regular) {
#pragma unroll
            for (int i = 0; i < NN; i++) Phi[i] = MF[i];
            for (int i = 0; i < kFcChunk; i++) {
                Ta rn[D];
                fc_matvec<Ta, D>(M, r, rn);
                const Ta y = my[i];
#pragma unroll
                for (int j = 0; j < D; j++) r[j] = fc_fma<Ta>(Kg[j], y, rn[j]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NN; i++) Phi[i] = (i % (D + 1)) == 0 ? (Ta)1 : (Ta)0;
            for (int i = 0; i < n; i++) {
                const Ta y = my[i];
                const bool miss = isnan(y);
                const Ta* Mt = miss ? A : M;
                Ta rn[D], Pn[NN];
                fc_matvec<Ta, D>(Mt, r, rn);
                fc_matmul<Ta, D>(Mt, Phi, Pn);
#pragma unroll
                for (int j = 0; j < D; j++) r[j] = miss ? rn[j] : fc_fma<Ta>(Kg[j], y, rn[j]);
#pragma unroll
                for (int j = 0; j < NN; j++) Phi[j] = Pn[j];
            }
        }
        // 2. scan over the lanes; the state before this lane's chunk is the inclusive map of lane - 1 applied to xseg
        fc_scan_maps<Ta, D>(Phi, r, lane);
        Ta xs0[D], xe[D];
        fc_matvec<Ta, D>(Phi, xseg, xe);
#pragma unroll
        for (int i = 0; i < D; i++) xe[i] += r[i];
#pragma unroll
        for (int i = 0; i < D; i++) {
            const Ta prev = __shfl_up(xe[i], 1, 64);
            xs0[i] = lane == 0 ? xseg[i] : prev;
            xseg[i] = __shfl(xe[i], 63, 64);
        }
        // 3. replay per group of KG horizons: c_k . x[t] into the group's planes, which then leave coalesced
        for (int k0 = 0; k0 < K; k0 += KG) {
            Ta c[KG][D];
#pragma unroll
            for (int kk = 0; kk < KG; kk++)
#pragma unroll
                for (int j = 0; j < D; j++) c[kk][j] = tb[B::C + (k0 + kk) * D + j];   // (k0 + kk < kFcMaxHorizons: KG divides it)
            Ta xs[D];
#pragma unroll
            for (int j = 0; j < D; j++) xs[j] = xs0[j];
            Ta* ow = obuf + lane * kFcPitch;
            if (regular) {   // a whole chunk without missing ticks: fixed trip count, no selects
#pragma unroll
                for (int i = 0; i < kFcChunk; i++) {
                    Ta xm[D];
                    fc_matvec<Ta, D>(M, xs, xm);
                    const Ta y = my[i];
#pragma unroll
                    for (int j = 0; j < D; j++) xs[j] = fc_fma<Ta>(Kg[j], y, xm[j]);
#pragma unroll
                    for (int kk = 0; kk < KG; kk++) {
                        Ta s = 0;
#pragma unroll
                        for (int j = 0; j < D; j++) s = fc_fma<Ta>(c[kk][j], xs[j], s);
                        ow[kk * kFcPlane + i] = s;
                    }
                }
            } else {
                for (int i = 0; i < n; i++) {
                    const Ta y = my[i];
                    const bool miss = isnan(y);
                    const Ta* Mt = miss ? A : M;
                    Ta xn[D];
                    fc_matvec<Ta, D>(Mt, xs, xn);
#pragma unroll
                    for (int j = 0; j < D; j++) xs[j] = miss ? xn[j] : fc_fma<Ta>(Kg[j], y, xn[j]);
#pragma unroll
                    for (int kk = 0; kk < KG; kk++) {
                        Ta s = 0;
#pragma unroll
                        for (int j = 0; j < D; j++) s = fc_fma<Ta>(c[kk][j], xs[j], s);
                        ow[kk * kFcPlane + i] = s;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KG; kk++) {
                if (k0 + kk < K) {
                    Tv* prow = frow + (size_t)(k0 + kk) * plane_stride;
#pragma unroll
                    for (int k = 0; k < kFcChunk; k++) {
                        const int tl = k * 64 + lane;
                        const size_t t = seg0 + tl;
                        if (t < T) prow[t] = (Tv)obuf[kk * kFcPlane + (tl / kFcChunk) * kFcPitch + tl % kFcChunk];
                    }
                }
            }
            __syncthreads();
        }
    }
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)xseg[i];
}

// Tick by tick, one lane per latent, fp64: the latents the sweep does not take, the NaN rows of failed latents when it does not run, every status word.
template <typename Tv, int D>
__global__ void __launch_bounds__(64) forecast_serial_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ tabs, size_t L,
                                                             const Tv* x_in, Tv* x_out, Tv* fc, size_t ld_out, size_t plane_stride, int K,
                                                             int* status, int path, double bound) {
    using B = FT<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* tb = tabs + l * B::SIZE;
    const bool failed = tb[B::STATUS] != 0.0;
    if (status) status[l] = failed ? 1 : 0;
    Tv* frow = fc + l * ld_out;
    if (failed) {   // (with the sweep running, forecast_sweep_kernel writes these rows coalesced)
        if (path == 1) {
            const Tv nan = (Tv)__builtin_nan("");
            for (int k = 0; k < K; k++)
                for (size_t t = 0; t < T; t++) frow[(size_t)k * plane_stride + t] = nan;
            for (int i = 0; i < D; i++) x_out[l * D + i] = nan;
        }
        return;
    }
    if (!(path == 1 || (path == -1 && !fc_scan_ok(tb, B::STATUS, B::GROWTH, bound)))) return;
    double A[NN], M[NN], Kg[D], x[D], c[kFcMaxHorizons][D];
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; M[i] = tb[B::M + i]; }
    for (int i = 0; i < D; i++) { Kg[i] = tb[B::K + i]; x[i] = (double)x_in[l * D + i]; }
    for (int k = 0; k < kFcMaxHorizons; k++)
        for (int j = 0; j < D; j++) c[k][j] = tb[B::C + k * D + j];
    const Tv* yrow = Ty + l * ld_in;
    for (size_t t = 0; t < T; t++) {
        const double y = (double)yrow[t];
        double xn[D];
        if (isnan(y)) {
            fc_matvec<double, D>(A, x, xn);
            for (int j = 0; j < D; j++) x[j] = xn[j];
        } else {
            fc_matvec<double, D>(M, x, xn);
            for (int j = 0; j < D; j++) x[j] = fma(Kg[j], y, xn[j]);
        }
#pragma unroll
        for (int k = 0; k < kFcMaxHorizons; k++) {
            if (k < K) {
                double s = 0.0;
                for (int j = 0; j < D; j++) s = fma(c[k][j], x[j], s);
                frow[(size_t)k * plane_stride + t] = (Tv)s;
            }
        }
    }
    for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)x[i];
}

// row <- row X  (row vector times matrix)
template <int D>
__device__ inline void fc_rowmat(const double* row, const double* X, double* out) {
    double t[D];
    for (int j = 0; j < D; j++) {
        double s = 0.0;
        for (int i = 0; i < D; i++) s = fma(row[i], X[i * D + j], s);
        t[j] = s;
    }
    for (int j = 0; j < D; j++) out[j] = t[j];
}
// c = e0^T A^h by binary powering
template <int D>
__device__ inline void fc_power_row(const double* A, unsigned long long h, double* c) {
    double P[D * D], Pn[D * D];
    for (int i = 0; i < D * D; i++) P[i] = A[i];
    for (int j = 0; j < D; j++) c[j] = j == 0 ? 1.0 : 0.0;
    while (h) {
        if (h & 1ull) fc_rowmat<D>(c, P, c);
        h >>= 1;
        if (h) {
            fc_matmul<double, D>(P, P, Pn);
            for (int i = 0; i < D * D; i++) P[i] = Pn[i];
        }
    }
}

// grid.y = latent, each block 1024 indices: lane starts at j = base + lane and strides by 64 (row <- row A^64)
template <typename Tv, int D>
__global__ void __launch_bounds__(64) forecast_tail_kernel(const double* __restrict__ cb64, int cb_size, int cb_A, const Tv* __restrict__ x, size_t n,
                                                           Tv* __restrict__ tail, size_t ld_out) {
    constexpr int NN = D * D;
    const size_t l = blockIdx.y;
    const size_t j0 = (size_t)blockIdx.x * kFcSeg + threadIdx.x;
    if (j0 >= n) return;
    double A[NN], A64[NN], Pn[NN], xv[D], c[D];
    for (int i = 0; i < NN; i++) { A[i] = cb64[l * (size_t)cb_size + cb_A + i]; A64[i] = A[i]; }
    for (int s = 0; s < 6; s++) {
        fc_matmul<double, D>(A64, A64, Pn);
        for (int i = 0; i < NN; i++) A64[i] = Pn[i];
    }
    for (int i = 0; i < D; i++) xv[i] = (double)x[l * D + i];
    fc_power_row<D>(A, (unsigned long long)j0 + 1ull, c);
    for (int i = 0; i < kFcChunk; i++) {
        const size_t j = j0 + (size_t)i * 64;
        if (j >= n) break;
        double s = 0.0;
        for (int k = 0; k < D; k++) s = fma(c[k], xv[k], s);
        tail[l * ld_out + j] = (Tv)s;
        fc_rowmat<D>(c, A64, c);
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
__device__ double fc_norm_inf(const double* X) {
    double m = 0.0;
    for (int i = 0; i < D; i++) {
        double s = 0.0;
        for (int j = 0; j < D; j++) s += fabs(X[i * D + j]);
        m = fmax(m, s);
    }
    return m;
}

// sm: the smoother's blocks (gains 0) with the offsets of its K, AKHA, PF, STATUS in smo[0, 1, 2, 4] and its block size in smo[5]; unused for gains 1
struct FcSmOffsets { int o[6]; };

template <int D>
__global__ void __launch_bounds__(64) forecast_tables_kernel(int kernel, const double* __restrict__ cb64, const double* __restrict__ sm, FcSmOffsets smo,
                                                             size_t L, FcHorizons hz, int K, int gains, double* __restrict__ t64,
                                                             float* __restrict__ t32) {
    using B = FT<D>;
    using C = CB<D>;
    constexpr int NN = D * D;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t l = idx / (size_t)K;
    const int k = (int)(idx % (size_t)K);
    if (l >= L) return;
    const double* cb = cb64 + l * C::SIZE;
    const double* s = gains == 0 ? sm + l * (size_t)smo.o[5] : nullptr;
    double* o = t64 + l * B::SIZE;
    float* of = t32 + l * B::SIZE;
    auto put = [&](int at, double v) { o[at] = v; of[at] = (float)v; };
    double A[NN], c[D];
    for (int i = 0; i < NN; i++) A[i] = cb[C::A + i];
    const bool failed = gains == 0 && s[smo.o[4]] != 0.0;
    fc_power_row<D>(A, (unsigned long long)hz.h[k], c);
    for (int j = 0; j < D; j++) put(B::C + k * D + j, c[j]);
    double var = 0.0;
    if (gains == 0) {
        // Pinf_00 - c (Pinf - PF) c^T, Pinf from the model code as the smoother's tables take it
        double prm[3] = {cb[C::PARAMS + 0], cb[C::PARAMS + 1], cb[C::PARAMS + 2]};
        SS<D> ss;
        ss_build<D>(kernel, prm, ss);
        double q = 0.0;
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) q += c[i] * (ss.Pinf[i * D + j] - s[smo.o[2] + i * D + j]) * c[j];
        var = failed ? __builtin_nan("") : ss.Pinf[0] - q;
    }
    put(B::VAR + k, var);
    if (k == K - 1)
        for (int kk = K; kk < kFcMaxHorizons; kk++) {
            for (int j = 0; j < D; j++) put(B::C + kk * D + j, 0.0);
            put(B::VAR + kk, 0.0);
        }
    if (k != 0) return;
    double M[NN], Kg[D], Mp[NN], MF[NN], growth = 0.0;
    for (int i = 0; i < NN; i++) M[i] = gains == 0 ? s[smo.o[1] + i] : cb[C::AKHA + i];
    for (int i = 0; i < D; i++) Kg[i] = gains == 0 ? s[smo.o[0] + i] : cb[C::K + i];
    for (int i = 0; i < NN; i++) Mp[i] = M[i];
    for (int p = 1; p <= 2 * kFcChunk; p++) {              // Mp = M^p
        if (p == kFcChunk) for (int i = 0; i < NN; i++) MF[i] = Mp[i];
        growth = fmax(growth, fc_norm_inf<D>(Mp));
        if (p < 2 * kFcChunk) mm<D>(M, Mp, Mp);
    }
    for (int q = 2 * kFcChunk; q < kFcSeg; q *= 2) mm<D>(Mp, Mp, Mp);   // M^kFcSeg: what one segment's scan composes
    growth = fmax(growth, fc_norm_inf<D>(Mp));
    if (!isfinite(growth)) growth = INFINITY;              // (fmax drops a NaN operand: test the parts)
    for (int i = 0; i < NN; i++) if (!isfinite(Mp[i]) || !isfinite(MF[i])) growth = INFINITY;
    for (int i = 0; i < NN; i++) { put(B::A + i, A[i]); put(B::M + i, M[i]); put(B::MF + i, MF[i]); }
    for (int i = 0; i < D; i++) put(B::K + i, Kg[i]);
    put(B::GROWTH, growth);
    put(B::STATUS, failed ? 1.0 : 0.0);
}

}  // namespace

int fc_size(int d) { return d == 2 ? FT<2>::SIZE : FT<3>::SIZE; }
int fc_var_offset(int d) { return d == 2 ? FT<2>::VAR : FT<3>::VAR; }

void launch_forecast_tables(int kernel, int d, const double* cb64, const double* sm, size_t L, const FcHorizons& hz, int K, int gains, double* t64,
                            float* t32, hipStream_t stream) {
    if (L == 0) return;
    FcSmOffsets smo{};
    if (gains == 0) {
        int off[14];
        sm_offsets(d, off);   // A AKHA K G MF MB P PF PS VARF VARS GROWTH RESID STATUS
        smo.o[0] = off[2]; smo.o[1] = off[1]; smo.o[2] = off[7]; smo.o[4] = off[13]; smo.o[5] = sm_size(d);
    }
    dim3 block(64), grid((unsigned)((L * (size_t)K + 63) / 64));
    if (d == 2) hipLaunchKernelGGL((forecast_tables_kernel<2>), grid, block, 0, stream, kernel, cb64, sm, smo, L, hz, K, gains, t64, t32);
    else hipLaunchKernelGGL((forecast_tables_kernel<3>), grid, block, 0, stream, kernel, cb64, sm, smo, L, hz, K, gains, t64, t32);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

template <typename Tv, int D, int KG>
static void launch_sweep_kg(const Tv* Ty, size_t T, size_t ld_in, size_t L, const Tv* tabs, const double* t64, const Tv* x_in, Tv* x, Tv* fc,
                            size_t ld_out, size_t plane_stride, int K, int path, hipStream_t stream) {
    const size_t lds = sizeof(Tv) * (size_t)(1 + KG) * kFcPlane;
    hipLaunchKernelGGL((forecast_sweep_kernel<Tv, Tv, D, KG>), dim3((unsigned)L), dim3(64), lds, stream, Ty, T, ld_in, tabs, t64, x_in, x, fc, ld_out,
                       plane_stride, K, path);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

template <typename Tv, int D>
static void launch_forecast_t(const Tv* Ty, size_t T, size_t ld_in, size_t L, const double* t64, const float* t32, const Tv* x_in, Tv* x, Tv* fc,
                              size_t ld_out, size_t plane_stride, int K, int* status, int path, hipStream_t stream) {
    const Tv* tabs;
    if constexpr (sizeof(Tv) == 8) tabs = t64; else tabs = t32;
    if (T > 0 && path != 1) {
        // horizons staged per replay: one for a single horizon, else two (three LDS planes per wavefront: 13 KB at fp32, 26 KB at fp64)
        if (K == 1) launch_sweep_kg<Tv, D, 1>(Ty, T, ld_in, L, tabs, t64, x_in, x, fc, ld_out, plane_stride, K, path, stream);
        else launch_sweep_kg<Tv, D, 2>(Ty, T, ld_in, L, tabs, t64, x_in, x, fc, ld_out, plane_stride, K, path, stream);
    }
    hipLaunchKernelGGL((forecast_serial_kernel<Tv, D>), dim3((unsigned)((L + 63) / 64)), dim3(64), 0, stream, Ty, T, ld_in, t64, L, x_in, x, fc, ld_out,
                       plane_stride, K, status, T > 0 ? path : 1, fc_growth_bound<Tv>());
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_forecast_stream(int d, int dtype, const void* Ty, size_t T, size_t ld_in, size_t L, const double* t64, const float* t32, const void* x_in,
                            void* x, void* fc, size_t ld_out, size_t plane_stride, int K, int* status, int path, hipStream_t stream) {
    if (L == 0) return;
    if (dtype == 0) {
        if (d == 2) launch_forecast_t<double, 2>((const double*)Ty, T, ld_in, L, t64, t32, (const double*)x_in, (double*)x, (double*)fc, ld_out, plane_stride, K, status, path, stream);
        else launch_forecast_t<double, 3>((const double*)Ty, T, ld_in, L, t64, t32, (const double*)x_in, (double*)x, (double*)fc, ld_out, plane_stride, K, status, path, stream);
    } else {
        if (d == 2) launch_forecast_t<float, 2>((const float*)Ty, T, ld_in, L, t64, t32, (const float*)x_in, (float*)x, (float*)fc, ld_out, plane_stride, K, status, path, stream);
        else launch_forecast_t<float, 3>((const float*)Ty, T, ld_in, L, t64, t32, (const float*)x_in, (float*)x, (float*)fc, ld_out, plane_stride, K, status, path, stream);
    }
}

void launch_forecast_tail(int d, int dtype, const double* cb64, size_t L, const void* x, size_t n, void* tail, size_t ld_out, hipStream_t stream) {
    if (L == 0 || n == 0) return;
    dim3 block(64), grid((unsigned)((n + kFcSeg - 1) / kFcSeg), (unsigned)L);
    const int cbs = cb_size(d);
    if (dtype == 0) {
        if (d == 2) hipLaunchKernelGGL((forecast_tail_kernel<double, 2>), grid, block, 0, stream, cb64, cbs, CB<2>::A, (const double*)x, n, (double*)tail, ld_out);
        else hipLaunchKernelGGL((forecast_tail_kernel<double, 3>), grid, block, 0, stream, cb64, cbs, CB<3>::A, (const double*)x, n, (double*)tail, ld_out);
    } else {
        if (d == 2) hipLaunchKernelGGL((forecast_tail_kernel<float, 2>), grid, block, 0, stream, cb64, cbs, CB<2>::A, (const float*)x, n, (float*)tail, ld_out);
        else hipLaunchKernelGGL((forecast_tail_kernel<float, 3>), grid, block, 0, stream, cb64, cbs, CB<3>::A, (const float*)x, n, (float*)tail, ld_out);
    }
    MOIHGP_HIP_FATAL(hipGetLastError());
}

}  // namespace moihgp
