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
//                            builds M^kScanChunk and the growth figure the sweep's choice of path rests on.  An fp32 copy of the block is
//                            written next to the fp64 one.  Built per call: the rows depend on the call's horizons.
//   forecast_sweep_kernel    one wavefront per latent, 64 x kScanChunk-tick segments staged through LDS, as smooth_fwd_kernel: chunk maps from a
//                            zero state, a Kogge-Stone scan over the lanes, then each lane replays its chunk from its start state and writes
//                            KG dot products c_k . x[t] per tick into KG LDS planes, which leave coalesced.  More than KG horizons: the
//                            replay (not the scan) is repeated per group of KG.  Arithmetic in the stream's own precision.
//   forecast_serial_kernel   one lane per latent, fp64, tick by tick: latents whose M fails the growth bound (rho(AKHA) > 1 occurs with the
//                            handle's gains), option "forecast_path" = 1, and every status word.
//   forecast_tail_kernel     tail[l][j] = H A^(j+1) x_l, fp64: each lane powers A to its first index and then strides by A^64.
//   forecast_score_kernel    moihgp_forecast_scores: the sweep's scan and replay, but where that one stores c_k . x[t] this one forms the error
//                            e = y[t + h_k] - c_k . x[t] and adds e, e^2 and a count into per-lane fp64 sums; no planes leave.  One shuffle
//                            reduction per latent at the end, plain stores, no atomics: the summation order is fixed.
//   forecast_score_serial_kernel   its serial twin, which also writes every status word and predictive variance var + R.
// The chunk-scan machinery of the sweep is scan_sweep.h (shared with smoother.hip and sampler.hip), the block layout FT<D> stream_tables.h.  The
// growth figure is the largest inf-norm of the powers of M up to 2 kScanChunk and of M^kScanSeg (segment_growth, stationary_common.h, shared with
// sampler.hip; the smoother's figure also covers its G, which no forecast uses: it is not consulted), held against scan_growth_bound<Ta>().
#include "scan_sweep.h"

namespace moihgp {
namespace {

// Tv: the stream's scalar; Ta: the arithmetic (= Tv); KG: horizons staged per replay.  tabs: the Ta copy of the blocks; tabs64 decides the path.
// (waves per SIMD: at fp32 four, so that 16 wavefronts per CU hold 4096 latents in one round -- 128 VGPRs at d = 3, no scratch)
template <typename Tv, typename Ta, int D, int KG>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(sizeof(Ta) == 4 ? 4 : 2))) forecast_sweep_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const Ta* __restrict__ tabs,
                                                            const double* __restrict__ tabs64, const Tv* x_in, Tv* x_out, Tv* __restrict__ fc,
                                                            size_t ld_out, size_t plane_stride, int K, int path) {
    using B = FT<D>;
    constexpr int NN = D * D;
    extern __shared__ double fc_lds[];
    Ta* ybuf = reinterpret_cast<Ta*>(fc_lds);                  // [64][kScanPitch] the segment's y
    Ta* obuf = ybuf + kScanPlane;                              // [KG][64][kScanPitch] the group's planes
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const Ta* tb = tabs + l * B::SIZE;
    const double* tb64 = tabs64 + l * B::SIZE;
    const Tv* yrow = Ty + l * ld_in;
    Tv* frow = fc + l * ld_out;
    const Route route = latent_route(tb64[B::STATUS], tb64[B::GROWTH], scan_growth_bound<Ta>(), path);
    if (route == Route::kFailed) write_failed<Tv, D>(frow, plane_stride, K, T, x_out + l * D, lane, 64);   // written coalesced here
    if (route != Route::kScan) return;
    Ta A[NN], M[NN], MF[NN], Kg[D];
#pragma unroll
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; M[i] = tb[B::M + i]; MF[i] = tb[B::MF + i]; }
#pragma unroll
    for (int i = 0; i < D; i++) Kg[i] = tb[B::K + i];
    Ta xseg[D];
#pragma unroll
    for (int i = 0; i < D; i++) xseg[i] = (Ta)x_in[l * D + i];
    const Ta* my = ybuf + lane * kScanPitch;
    for (size_t seg0 = 0; seg0 < T; seg0 += kScanSeg) {
        stage_in(yrow, seg0, T, lane, ybuf);
        __syncthreads();
        bool regular;
        const int n = lane_ticks(my, seg0, T, lane, regular);
        // 1. the chunk's map from a zero state; 2. scan over the lanes: the state before this lane's chunk
        Ta Phi[NN], r[D], xs0[D];
        chunk_map<Ta, D>(my, n, regular, A, M, MF, Kg, Phi, r);
        scan_maps<Ta, D, true>(Phi, r, lane);
        start_states<Ta, D, true>(Phi, r, xseg, xs0, lane);
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
            Ta* ow = obuf + lane * kScanPitch;
            if (regular) {   // a whole chunk without missing ticks: fixed trip count, no selects
#pragma unroll
                for (int i = 0; i < kScanChunk; i++) {
                    Ta xm[D];   // (tick_step's loop, kept here: through the helper the fp32 sweeps come out rescheduled)
                    matvec<Ta, D>(M, xs, xm);
                    const Ta y = my[i];
#pragma unroll
                    for (int j = 0; j < D; j++) xs[j] = fma(Kg[j], y, xm[j]);
#pragma unroll
                    for (int kk = 0; kk < KG; kk++) {
                        Ta s = 0;
#pragma unroll
                        for (int j = 0; j < D; j++) s = fma(c[kk][j], xs[j], s);
                        ow[kk * kScanPlane + i] = s;
                    }
                }
            } else {
                for (int i = 0; i < n; i++) {
                    const Ta y = my[i];
                    const bool miss = isnan(y);
                    const Ta* Mt = miss ? A : M;
                    Ta xn[D];
                    matvec<Ta, D>(Mt, xs, xn);
#pragma unroll
                    for (int j = 0; j < D; j++) xs[j] = miss ? xn[j] : fma(Kg[j], y, xn[j]);
#pragma unroll
                    for (int kk = 0; kk < KG; kk++) {
                        Ta s = 0;
#pragma unroll
                        for (int j = 0; j < D; j++) s = fma(c[kk][j], xs[j], s);
                        ow[kk * kScanPlane + i] = s;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KG; kk++) {   // (stage_out's loop, kept here: called with obuf + kk * kScanPlane it costs the KG = 2 kernels 16 VGPRs)
                if (k0 + kk < K) {
                    Tv* prow = frow + (size_t)(k0 + kk) * plane_stride;
#pragma unroll
                    for (int k = 0; k < kScanChunk; k++) {
                        const int tl = k * 64 + lane;
                        const size_t t = seg0 + tl;
                        if (t < T) prow[t] = (Tv)obuf[kk * kScanPlane + scan_slot(tl)];
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
    const Route route = latent_route(tb[B::STATUS], tb[B::GROWTH], bound, path);
    if (status) status[l] = route == Route::kFailed ? 1 : 0;
    Tv* frow = fc + l * ld_out;
    if (route == Route::kFailed && path == 1) write_failed<Tv, D>(frow, plane_stride, K, T, x_out + l * D, 0, 1);   // (else forecast_sweep_kernel wrote them)
    if (route != Route::kSerial) return;
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
            matvec<double, D>(A, x, xn);
            for (int j = 0; j < D; j++) x[j] = xn[j];
        } else {
            matvec<double, D>(M, x, xn);
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

// ---- backtest scores (include/moihgp.h moihgp_forecast_scores): the forecast sweep's replay with the planes reduced on the spot -----------------
// Horizons per replay of the kernels that stage their targets, and whether fp64 streams take the row-direct form instead (all horizons in one
// replay).  Overridable from XFLAGS for measurements.
#ifndef MOIHGP_SCORE_KG
#define MOIHGP_SCORE_KG 2
#endif
#ifndef MOIHGP_SCORE_DIRECT64
#define MOIHGP_SCORE_DIRECT64 1
#endif

// One scored pair: the forecast s against its target yt, which is NaN where the pair does not count.  The error is formed in the precision
// both are held in and widened once; the sums are fp64.
template <typename Ta>
__device__ __forceinline__ void score_add(Ta s, Ta yt, double& se, double& sq, unsigned& cnt) {
    const bool ok = !isnan(yt);
    const double e = (double)(ok ? yt - s : (Ta)0);
    se += e;
    sq = fma(e, e, sq);
    cnt += ok ? 1u : 0u;
}

// The targets of the segment's origins at horizon h into a plane, coalesced as stage_in loads y: the slot of origin tick t holds y[t + h], or NaN
// where the pair does not count -- an origin before t_first, a target at or past T (never read there), a missing target as it stands.
template <typename Tv, typename Ta>
__device__ __forceinline__ void stage_targets(const Tv* row, size_t seg0, size_t h, size_t T, size_t t_first, int lane, Ta* plane) {
    const Ta nan = (Ta)__builtin_nan("");
#pragma unroll
    for (int k = 0; k < kScanChunk; k++) {
        const int tl = k * 64 + lane;
        const size_t t = seg0 + tl;
        plane[scan_slot(tl)] = (t + h < T && t >= t_first) ? (Ta)row[t + h] : nan;
    }
}

// forecast_sweep_kernel with its planes replaced by per-lane fp64 sums: KG horizons per replay, NG groups of them (KG NG >= K; every group's sums
// stay in registers until the stream's end, so the groups are unrolled), then a shuffle reduction in a fixed order and one lane's plain stores.
// STAGED: LDS holds the segment's y and the KG target planes of the group in hand; the first group's are loaded together with y, ahead of the
// scan.  Otherwise a pair's target is read straight from the row (under t + h < T and t >= t_first) and LDS is the one plane of y.
// Only the latents the scan takes; the serial kernel below sees to the others.
template <typename Tv, typename Ta, int D, int KG, int NG, bool STAGED>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) forecast_score_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const Ta* __restrict__ tabs,
                                                            const double* __restrict__ tabs64, const Tv* x_in, Tv* x_out, FcHorizons hz, int K,
                                                            size_t t_first, size_t L, long long* __restrict__ n_out, double* __restrict__ sum_err,
                                                            double* __restrict__ sum_sq, int path) {
    using B = FT<D>;
    constexpr int NN = D * D;
    constexpr int NK = KG * NG;
    extern __shared__ double fc_lds[];
    Ta* ybuf = reinterpret_cast<Ta*>(fc_lds);                  // [64][kScanPitch] the segment's y
    Ta* tbuf = ybuf + kScanPlane;                              // STAGED: [KG][64][kScanPitch] the group's targets y[t + h]
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const Ta* tb = tabs + l * B::SIZE;
    const double* tb64 = tabs64 + l * B::SIZE;
    const Tv* yrow = Ty + l * ld_in;
    if (latent_route(tb64[B::STATUS], tb64[B::GROWTH], scan_growth_bound<Ta>(), path) != Route::kScan) return;
    Ta A[NN], M[NN], MF[NN], Kg[D];
#pragma unroll
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; M[i] = tb[B::M + i]; MF[i] = tb[B::MF + i]; }
#pragma unroll
    for (int i = 0; i < D; i++) Kg[i] = tb[B::K + i];
    Ta xseg[D];
#pragma unroll
    for (int i = 0; i < D; i++) xseg[i] = (Ta)x_in[l * D + i];
    double se[NK], sq[NK];
    unsigned cnt[NK];
#pragma unroll
    for (int j = 0; j < NK; j++) { se[j] = 0.0; sq[j] = 0.0; cnt[j] = 0u; }
    const Ta* my = ybuf + lane * kScanPitch;
    const Ta* tg = tbuf + lane * kScanPitch;
    for (size_t seg0 = 0; seg0 < T; seg0 += kScanSeg) {
        const bool scored = seg0 + kScanSeg > t_first;   // else the segment ends before t_first: only the state moves on
        stage_in(yrow, seg0, T, lane, ybuf);
        if (STAGED && scored) {
#pragma unroll
            for (int kk = 0; kk < KG; kk++) stage_targets(yrow, seg0, (size_t)hz.h[kk], T, t_first, lane, tbuf + kk * kScanPlane);
        }
        __syncthreads();
        bool regular;
        const int n = lane_ticks(my, seg0, T, lane, regular);
        Ta Phi[NN], r[D], xs0[D];
        chunk_map<Ta, D>(my, n, regular, A, M, MF, Kg, Phi, r);
        scan_maps<Ta, D, true>(Phi, r, lane);
        start_states<Ta, D, true>(Phi, r, xseg, xs0, lane);
        const size_t t0 = seg0 + (size_t)lane * kScanChunk;
        if (scored) {
#pragma unroll
            for (int g = 0; g < NG; g++) {
                if (g * KG < K) {
                    Ta c[KG][D];
#pragma unroll
                    for (int kk = 0; kk < KG; kk++)
#pragma unroll
                        for (int j = 0; j < D; j++) c[kk][j] = tb[B::C + (g * KG + kk) * D + j];   // (g KG + kk < kFcMaxHorizons; rows past K are zero and their sums are never stored)
                    if (STAGED && g > 0) {   // the planes of the group before have been read
                        __syncthreads();
#pragma unroll
                        for (int kk = 0; kk < KG; kk++) stage_targets(yrow, seg0, (size_t)hz.h[g * KG + kk], T, t_first, lane, tbuf + kk * kScanPlane);
                        __syncthreads();
                    }
                    Ta xs[D];
#pragma unroll
                    for (int j = 0; j < D; j++) xs[j] = xs0[j];
                    // the forecasts made at tick i of the chunk from the state xs after it, against their targets
                    auto score = [&](int i) {
#pragma unroll
                        for (int kk = 0; kk < KG; kk++) {
                            Ta s = 0;
#pragma unroll
                            for (int j = 0; j < D; j++) s = fma(c[kk][j], xs[j], s);
                            Ta yt;
                            if constexpr (STAGED) {
                                yt = tg[kk * kScanPlane + i];
                            } else {
                                const size_t t = t0 + i, tt = t + (size_t)hz.h[g * KG + kk];
                                yt = (tt < T && t >= t_first) ? (Ta)yrow[tt] : (Ta)__builtin_nan("");
                            }
                            score_add<Ta>(s, yt, se[g * KG + kk], sq[g * KG + kk], cnt[g * KG + kk]);
                        }
                    };
                    auto step = [&](int i) {   // a tick of a chunk without missing ticks: no selects
                        Ta xm[D];
                        matvec<Ta, D>(M, xs, xm);
                        const Ta y = my[i];
#pragma unroll
                        for (int j = 0; j < D; j++) xs[j] = fma(Kg[j], y, xm[j]);
                        score(i);
                    };
                    if (regular) {   // fixed trip count; unrolled where the targets wait in LDS (row-direct, the loads of an unrolled chunk spill from two horizons on)
                        if constexpr (STAGED || KG == 1) {
#pragma unroll
                            for (int i = 0; i < kScanChunk; i++) step(i);
                        } else {
#pragma nounroll
                            for (int i = 0; i < kScanChunk; i++) step(i);
                        }
                    } else {
                        for (int i = 0; i < n; i++) {
                            const Ta y = my[i];
                            const bool miss = isnan(y);
                            const Ta* Mt = miss ? A : M;
                            Ta xn[D];
                            matvec<Ta, D>(Mt, xs, xn);
#pragma unroll
                            for (int j = 0; j < D; j++) xs[j] = miss ? xn[j] : fma(Kg[j], y, xn[j]);
                            score(i);
                        }
                    }
                }
            }
        }
        __syncthreads();   // the next segment restages every plane
    }
    // over the wavefront in a fixed order, then lane 0 stores the latent's K results
#pragma unroll
    for (int j = 0; j < NK; j++) {
        double a = se[j], b = sq[j];
        long long c = (long long)cnt[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_down(a, off, 64);
            b += __shfl_down(b, off, 64);
            c += __shfl_down(c, off, 64);
        }
        if (lane == 0 && j < K) {
            n_out[(size_t)j * L + l] = c;
            if (sum_err) sum_err[(size_t)j * L + l] = a;
            sum_sq[(size_t)j * L + l] = b;
        }
    }
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)xseg[i];
}

// The serial twin, one lane per latent, fp64: every status word and predictive variance (var + R, R the latent's noise parameter), the NaN results
// of failed latents, and the walk of the latents the sweep does not take.
template <typename Tv, int D>
__global__ void __launch_bounds__(64) forecast_score_serial_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ tabs,
                                                                   const double* __restrict__ cb64, size_t L, const Tv* x_in, Tv* x_out, FcHorizons hz,
                                                                   int K, size_t t_first, long long* __restrict__ n_out, double* __restrict__ sum_err,
                                                                   double* __restrict__ sum_sq, double* __restrict__ pvar, int* status, int path,
                                                                   double bound) {
    using B = FT<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* tb = tabs + l * B::SIZE;
    const Route route = latent_route(tb[B::STATUS], tb[B::GROWTH], bound, path);
    const bool failed = route == Route::kFailed;
    const double nan = __builtin_nan("");
    if (status) status[l] = failed ? 1 : 0;
    if (pvar) {
        const double R = cb64[l * CB<D>::SIZE + CB<D>::PARAMS + 2];
#pragma unroll
        for (int k = 0; k < kFcMaxHorizons; k++)
            if (k < K) pvar[(size_t)k * L + l] = failed ? nan : tb[B::VAR + k] + R;
    }
    if (failed) {
#pragma unroll
        for (int k = 0; k < kFcMaxHorizons; k++)
            if (k < K) {
                n_out[(size_t)k * L + l] = 0;
                if (sum_err) sum_err[(size_t)k * L + l] = nan;
                sum_sq[(size_t)k * L + l] = nan;
            }
        for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)nan;
    }
    if (route != Route::kSerial) return;
    double A[NN], M[NN], Kg[D], x[D], c[kFcMaxHorizons][D], se[kFcMaxHorizons], sq[kFcMaxHorizons];
    unsigned long long cnt[kFcMaxHorizons];
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; M[i] = tb[B::M + i]; }
    for (int i = 0; i < D; i++) { Kg[i] = tb[B::K + i]; x[i] = (double)x_in[l * D + i]; }
#pragma unroll
    for (int k = 0; k < kFcMaxHorizons; k++) {
        for (int j = 0; j < D; j++) c[k][j] = tb[B::C + k * D + j];
        se[k] = 0.0; sq[k] = 0.0; cnt[k] = 0ull;
    }
    const Tv* yrow = Ty + l * ld_in;
    for (size_t t = 0; t < T; t++) {
        const double y = (double)yrow[t];
        double xn[D];
        if (isnan(y)) {
            matvec<double, D>(A, x, xn);
            for (int j = 0; j < D; j++) x[j] = xn[j];
        } else {
            matvec<double, D>(M, x, xn);
            for (int j = 0; j < D; j++) x[j] = fma(Kg[j], y, xn[j]);
        }
        if (t < t_first) continue;
#pragma unroll
        for (int k = 0; k < kFcMaxHorizons; k++) {
            if (k < K) {
                double s = 0.0;
                for (int j = 0; j < D; j++) s = fma(c[k][j], x[j], s);
                const size_t tt = t + (size_t)hz.h[k];
                unsigned one = 0u;
                score_add<double>(s, tt < T ? (double)yrow[tt] : nan, se[k], sq[k], one);
                cnt[k] += one;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kFcMaxHorizons; k++)
        if (k < K) {
            n_out[(size_t)k * L + l] = (long long)cnt[k];
            if (sum_err) sum_err[(size_t)k * L + l] = se[k];
            sum_sq[(size_t)k * L + l] = sq[k];
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
            matmul<double, D>(P, P, Pn);
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
    const size_t j0 = (size_t)blockIdx.x * kScanSeg + threadIdx.x;
    if (j0 >= n) return;
    double A[NN], A64[NN], Pn[NN], xv[D], c[D];
    for (int i = 0; i < NN; i++) { A[i] = cb64[l * (size_t)cb_size + cb_A + i]; A64[i] = A[i]; }
    for (int s = 0; s < 6; s++) {
        matmul<double, D>(A64, A64, Pn);
        for (int i = 0; i < NN; i++) A64[i] = Pn[i];
    }
    for (int i = 0; i < D; i++) xv[i] = (double)x[l * D + i];
    fc_power_row<D>(A, (unsigned long long)j0 + 1ull, c);
    for (int i = 0; i < kScanChunk; i++) {
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
__global__ void __launch_bounds__(64) forecast_tables_kernel(int kernel, const double* __restrict__ cb64, const double* __restrict__ sm,
                                                             size_t L, FcHorizons hz, int K, int gains, double* __restrict__ t64,
                                                             float* __restrict__ t32) {
    using B = FT<D>;
    using C = CB<D>;
    using S = SM<D>;   // the smoother's blocks (gains 0: Kalman-form K, A - K H A, PF); unused for gains 1
    constexpr int NN = D * D;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t l = idx / (size_t)K;
    const int k = (int)(idx % (size_t)K);
    if (l >= L) return;
    const double* cb = cb64 + l * C::SIZE;
    const double* s = gains == 0 ? sm + l * (size_t)S::SIZE : nullptr;
    double* o = t64 + l * B::SIZE;
    float* of = t32 + l * B::SIZE;
    auto put = [&](int at, double v) { o[at] = v; of[at] = (float)v; };
    double A[NN], c[D];
    for (int i = 0; i < NN; i++) A[i] = cb[C::A + i];
    const bool failed = gains == 0 && s[S::STATUS] != 0.0;
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
            for (int j = 0; j < D; j++) q += c[i] * (ss.Pinf[i * D + j] - s[S::PF + i * D + j]) * c[j];
        var = failed ? __builtin_nan("") : ss.Pinf[0] - q;
    }
    put(B::VAR + k, var);
    if (k == K - 1)
        for (int kk = K; kk < kFcMaxHorizons; kk++) {
            for (int j = 0; j < D; j++) put(B::C + kk * D + j, 0.0);
            put(B::VAR + kk, 0.0);
        }
    if (k != 0) return;
    double M[NN], Kg[D], Mp[NN], MF[NN];
    for (int i = 0; i < NN; i++) M[i] = gains == 0 ? s[S::AKHA + i] : cb[C::AKHA + i];
    for (int i = 0; i < D; i++) Kg[i] = gains == 0 ? s[S::K + i] : cb[C::K + i];
    double growth = segment_growth<D, kScanChunk, kScanSeg>(M, MF, Mp);   // Mp = M^kScanSeg: what one segment's scan composes
    if (!isfinite(growth)) growth = INFINITY;              // (fmax drops a NaN operand: test the parts)
    for (int i = 0; i < NN; i++) if (!isfinite(Mp[i]) || !isfinite(MF[i])) growth = INFINITY;
    for (int i = 0; i < NN; i++) { put(B::A + i, A[i]); put(B::M + i, M[i]); put(B::MF + i, MF[i]); }
    for (int i = 0; i < D; i++) put(B::K + i, Kg[i]);
    put(B::GROWTH, growth);
    put(B::STATUS, failed ? 1.0 : 0.0);
}

}  // namespace

void launch_forecast_tables(int kernel, int d, const double* cb64, const double* sm, size_t L, const FcHorizons& hz, int K, int gains, double* t64,
                            float* t32, hipStream_t stream) {
    if (L == 0) return;
    dim3 block(64), grid((unsigned)((L * (size_t)K + 63) / 64));
    dispatch_dim(d, [&](auto dim) {
        hipLaunchKernelGGL((forecast_tables_kernel<decltype(dim)::value>), grid, block, 0, stream, kernel, cb64, sm, L, hz, K, gains, t64, t32);
    });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

// The call's record and its planes are unpacked here, at the launch lines.
template <typename Tv, int D, int KG>
static void launch_sweep_kg(const SweepIo& io, const Tv* tabs, const double* t64, const SweepPlanes& fc, int path) {
    const size_t lds = sizeof(Tv) * (size_t)(1 + KG) * kScanPlane;
    hipLaunchKernelGGL((forecast_sweep_kernel<Tv, Tv, D, KG>), dim3((unsigned)io.L), dim3(64), lds, io.stream, (const Tv*)io.Ty, io.T, io.ld, tabs, t64,
                       (const Tv*)io.xin, (Tv*)io.x, (Tv*)fc.base, io.ld_out, fc.stride, fc.K, path);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

template <typename Tv, int D>
static void launch_forecast_t(const SweepIo& io, const double* t64, const float* t32, const SweepPlanes& fc, int* status, int path) {
    const Tv* tabs;
    if constexpr (sizeof(Tv) == 8) tabs = t64; else tabs = t32;
    if (io.T > 0 && path != 1) {
        // horizons staged per replay: one for a single horizon, else two (three LDS planes per wavefront: 13 KB at fp32, 26 KB at fp64)
        if (fc.K == 1) launch_sweep_kg<Tv, D, 1>(io, tabs, t64, fc, path);
        else launch_sweep_kg<Tv, D, 2>(io, tabs, t64, fc, path);
    }
    hipLaunchKernelGGL((forecast_serial_kernel<Tv, D>), dim3((unsigned)((io.L + 63) / 64)), dim3(64), 0, io.stream, (const Tv*)io.Ty, io.T, io.ld, t64, io.L,
                       (const Tv*)io.xin, (Tv*)io.x, (Tv*)fc.base, io.ld_out, fc.stride, fc.K, status, io.T > 0 ? path : 1, scan_growth_bound<Tv>());
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_forecast_stream(int d, const SweepIo& io, const double* t64, const float* t32, const SweepPlanes& fc, int* status, int path) {
    if (io.L == 0) return;
    dispatch_stream(d, io.dtype, [&](auto tv, auto dim) { launch_forecast_t<decltype(tv), decltype(dim)::value>(io, t64, t32, fc, status, path); });
}

// KG horizons per replay, NG groups.  Staged targets: K = 1 and 2 are their own group, more take MOIHGP_SCORE_KG at a time.  Row-direct (fp64
// streams): 1, 2, 4 or all kFcMaxHorizons rows of the table in one replay.
template <typename Tv, int D, int KG, int NG, bool STAGED = true>
static void launch_score_kg(const SweepIo& io, const Tv* tabs, const double* t64, const FcHorizons& hz, int K, size_t t_first, const ScoreSums& out, int path) {
    const size_t lds = sizeof(Tv) * (size_t)(1 + (STAGED ? KG : 0)) * kScanPlane;
    hipLaunchKernelGGL((forecast_score_kernel<Tv, Tv, D, KG, NG, STAGED>), dim3((unsigned)io.L), dim3(64), lds, io.stream, (const Tv*)io.Ty, io.T, io.ld, tabs, t64,
                       (const Tv*)io.xin, (Tv*)io.x, hz, K, t_first, io.L, out.n, out.sum_err, out.sum_sq, path);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

template <typename Tv, int D>
static void launch_scores_t(const SweepIo& io, const double* t64, const float* t32, const double* cb64, const FcHorizons& hz, int K, size_t t_first,
                            const ScoreSums& out, int* status, int path) {
    constexpr int KG = MOIHGP_SCORE_KG;
    static_assert(KG == 2 || KG == 4 || KG == 8, "MOIHGP_SCORE_KG divides kFcMaxHorizons");
    const Tv* tabs;
    if constexpr (sizeof(Tv) == 8) tabs = t64; else tabs = t32;
    if (io.T > 0 && path != 1) {
        if constexpr (sizeof(Tv) == 8 && MOIHGP_SCORE_DIRECT64) {
            if (K == 1) launch_score_kg<Tv, D, 1, 1, false>(io, tabs, t64, hz, K, t_first, out, path);
            else if (K == 2) launch_score_kg<Tv, D, 2, 1, false>(io, tabs, t64, hz, K, t_first, out, path);
            else if (K <= 4) launch_score_kg<Tv, D, 4, 1, false>(io, tabs, t64, hz, K, t_first, out, path);
            else launch_score_kg<Tv, D, kFcMaxHorizons, 1, false>(io, tabs, t64, hz, K, t_first, out, path);
        }
        else if (K == 1) launch_score_kg<Tv, D, 1, 1>(io, tabs, t64, hz, K, t_first, out, path);
        else if (K == 2) launch_score_kg<Tv, D, 2, 1>(io, tabs, t64, hz, K, t_first, out, path);
        else if (K <= KG) launch_score_kg<Tv, D, KG, 1>(io, tabs, t64, hz, K, t_first, out, path);
        else if (K <= 2 * KG) launch_score_kg<Tv, D, KG, (KG < 8 ? 2 : 1)>(io, tabs, t64, hz, K, t_first, out, path);
        else launch_score_kg<Tv, D, KG, (KG < 4 ? 4 : 1)>(io, tabs, t64, hz, K, t_first, out, path);
    }
    hipLaunchKernelGGL((forecast_score_serial_kernel<Tv, D>), dim3((unsigned)((io.L + 63) / 64)), dim3(64), 0, io.stream, (const Tv*)io.Ty, io.T, io.ld, t64, cb64,
                       io.L, (const Tv*)io.xin, (Tv*)io.x, hz, K, t_first, out.n, out.sum_err, out.sum_sq, out.pvar, status, io.T > 0 ? path : 1,
                       scan_growth_bound<Tv>());
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_forecast_scores(int d, const SweepIo& io, const double* t64, const float* t32, const double* cb64, const FcHorizons& hz, int K, size_t t_first,
                            const ScoreSums& out, int* status, int path) {
    if (io.L == 0) return;
    dispatch_stream(d, io.dtype, [&](auto tv, auto dim) {
        launch_scores_t<decltype(tv), decltype(dim)::value>(io, t64, t32, cb64, hz, K, t_first, out, status, path);
    });
}

void launch_forecast_tail(int d, int dtype, const double* cb64, size_t L, const void* x, size_t n, void* tail, size_t ld_out, hipStream_t stream) {
    if (L == 0 || n == 0) return;
    dim3 block(64), grid((unsigned)((n + kScanSeg - 1) / kScanSeg), (unsigned)L);
    dispatch_stream(d, dtype, [&](auto tv, auto dim) {
        using Tv = decltype(tv);
        constexpr int D = decltype(dim)::value;
        hipLaunchKernelGGL((forecast_tail_kernel<Tv, D>), grid, block, 0, stream, cb64, CB<D>::SIZE, CB<D>::A, (const Tv*)x, n, (Tv*)tail, ld_out);
    });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

}  // namespace moihgp
