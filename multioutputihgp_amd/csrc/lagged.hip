// lagged.hip -- fixed-lag smoothing of whole series-major streams (include/moihgp.h moihgp_lagged_stream / _variances).
//
// Per latent, with the smoother's tables (A, K, G, PF, Ps of SM<D>) and its forward pass (p[t], v[t] = y[t] - p[t], 0 where y[t] is NaN), for lags
// l_0 .. l_{K-1}:
//   lag[k][t] = p[t] + ( sum_{j=0..l_k, t+j<T} G^j K v[t+j] )_0      the mean at tick t given the ticks <= min(t + l_k, T - 1)
//   var[k]    = ( Ps + G^l_k (PF - Ps) (G^l_k)^T )_00
// The windowed sum is the backward recursion (v = 0 at and past T, s_k[T] = 0)
//   s_k[t] = G s_k[t+1] + K v[t] - w_k v[t + l_k + 1],   w_k = G^(l_k + 1) K,   lag[k][t] = p[t] + s_k[t]_0
// with the smoother's map G for every lag: only the second input, a copy of v shifted by l_k + 1 ticks, and its gain differ.
//
// Kernels
//   lagged_tables_kernel   fp64, one lane per (latent, lag): G^l_k by binary powering, w_k and var[k] from the latent's SM<D> block; the lane of
//                          lag 0 marks a latent whose smoother status is non-zero.  Built per call: the rows depend on the call's lags.
//   smooth_fwd_kernel      (smoother.hip, its STATE_AT instance) writes p into ypred and the filtered state after tick T_state - 1 into x.
//   lagged_bwd_kernel      one wavefront per latent, 64 x kScanChunk-tick segments from the last to the first with the lane order mirrored, as
//                          smooth_bwd_kernel.  A segment's v is staged once (its p stays in registers, for the store) and kept for the next segment
//                          to the left; per group of KG lags one more plane per lag holds v shifted by l_k + 1: copied from the two staged
//                          segments while l_k < kScanSeg, else from y and p read coalesced at the shifted offset (zero past T and at NaN).  Every chunk's map is G^kScanChunk, the
//                          same in every lane and for every lag, so the Kogge-Stone scan never composes maps: stage `off` applies G^(kScanChunk off),
//                          six matrices that are built once per wavefront and kept in LDS, and only the KG response vectors are scanned.  A chunk's
//                          response is the smoother's (once per segment) less that of the shifted plane (per lag).  Each lane then replays its
//                          chunk once per lag and writes s_0 over the shifted plane, which leaves coalesced with p added.  More than KG lags repeat the
//                          shifted loads, the response scan and the replay per group, not the loads of y and p or the smoother's response.
//   lagged_serial_kernel   one lane per latent, fp64, tick by tick, forward and then once backward per lag: the latents the scan kernels leave
//                          (growth bound failed, option "lagged_path" = 1), every status word, and the NaN rows of failed latents when it walks all.
// Arithmetic is fp64 for both stream types, as the smoother's (the window's two inputs cancel: at lag 0 what is left of the smoother's sum is its
// first term); fp32 streams are staged in fp32, i.e. v is rounded once to the stream's own precision, and narrowed on store.
#include "scan_sweep.h"

namespace moihgp {
namespace {

constexpr int kLagStages = 6;   // Kogge-Stone stages over 64 lanes

// Inclusive mirrored scan (lane 63 first) of NR response vectors whose chunks all have the map MB: stage s composes with MB^(2^s) = pw[s] in every
// lane that takes part (a lane that has a partner `off` lanes up holds exactly `off` chunks).  pw: [kLagStages][D * D], the same for all lanes.
template <int D, int NR>
__device__ __forceinline__ void scan_responses_bwd(const double* pw, double (*r)[D], int lane) {
#pragma unroll
    for (int st = 0; st < kLagStages; st++) {
        const int off = 1 << st;
        double P[D * D];
#pragma unroll
        for (int i = 0; i < D * D; i++) P[i] = pw[st * D * D + i];
#pragma unroll
        for (int k = 0; k < NR; k++) {
            double ro[D], rn[D];
#pragma unroll
            for (int i = 0; i < D; i++) ro[i] = __shfl_down(r[k][i], off, 64);
            matvec<double, D>(P, ro, rn);
            if (lane + off < 64)
#pragma unroll
                for (int i = 0; i < D; i++) r[k][i] += rn[i];
        }
    }
}

// Tv: the stream's scalar and that of the staged planes; KG: lags staged per replay.  sm: the smoother's blocks, lt: the call's LT<D> blocks.
template <typename Tv, int D, int KG>
__global__ void __launch_bounds__(64) lagged_bwd_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ sm,
                                                        const double* __restrict__ lt, LagList lags, int K, const Tv* __restrict__ ypred,
                                                        Tv* __restrict__ out, size_t ld_out, size_t plane_stride, Tv* x_out, int path) {
    using B = SM<D>;
    using W = LT<D>;
    constexpr int NN = D * D;
    extern __shared__ double lag_lds[];
    __shared__ double pw[kLagStages * NN];          // G^(kScanChunk 2^s)
    __shared__ double sseg[kLagMaxLags * D];         // per lag, the state that enters the segment from the right
    Tv* vpl = reinterpret_cast<Tv*>(lag_lds);        // [2][64][kScanPitch] v of the segment and of the segment to its right, taking turns
    Tv* sb = vpl + 2 * kScanPlane;                   // [KG] ... v shifted by the lag + 1, then s_0 of the lag
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const double* tb = sm + l * B::SIZE;
    const double* tw = lt + l * W::SIZE;
    const Route route = latent_route(tb[B::STATUS], tb[B::GROWTH], scan_growth_bound<double>(), path);
    Tv* orow = out + l * ld_out;
    if (route == Route::kFailed) write_failed<Tv, D>(orow, plane_stride, K, T, x_out + l * D, lane, 64);   // (ypred's row: smooth_fwd_kernel)
    if (route != Route::kScan) return;
    double G[NN], Kg[D];
#pragma unroll
    for (int i = 0; i < NN; i++) G[i] = tb[B::G + i];
#pragma unroll
    for (int i = 0; i < D; i++) Kg[i] = tb[B::K + i];
    {
        double P[NN], Pn[NN];
#pragma unroll
        for (int i = 0; i < NN; i++) P[i] = tb[B::MB + i];
#pragma unroll
        for (int st = 0; st < kLagStages; st++) {
            if (lane == 0)
#pragma unroll
                for (int i = 0; i < NN; i++) pw[st * NN + i] = P[i];
            matmul<double, D>(P, P, Pn);
#pragma unroll
            for (int i = 0; i < NN; i++) P[i] = Pn[i];
        }
        if (lane < kLagMaxLags * D) sseg[lane] = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * kScanPlane; k += 64)   // v past the end of the stream is zero
            if (k + lane < 2 * kScanPlane) vpl[k + lane] = (Tv)0;
    }
    const Tv* yrow = Ty + l * ld_in;
    const Tv* prow = ypred + l * ld_out;
    const size_t nseg = (T + kScanSeg - 1) / kScanSeg;
    for (size_t sg = nseg; sg-- > 0;) {
        const size_t seg0 = sg * kScanSeg;
        Tv* vb = vpl + (sg & 1) * kScanPlane;
        const Tv* vr = vpl + ((sg & 1) ^ 1) * kScanPlane;   // the segment at seg0 + kScanSeg, staged by the iteration before (zeros at the stream's end)
        const Tv* v = vb + lane * kScanPitch;
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
        // the smoother's part of every lag's chunk response, from a zero state at the chunk's end
        double ra[D];
        chunk_response_bwd<double, D, Tv>(v, G, Kg, ra);
        for (int k0 = 0; k0 < K; k0 += KG) {
#pragma unroll
            for (int kk = 0; kk < KG; kk++) {
                const size_t sh = k0 + kk < K ? (size_t)lags.lag[k0 + kk] + 1 : 0;
                if (sh == 0) {                      // an idle plane of the last group
#pragma unroll
                    for (int k = 0; k < kScanChunk; k++) sb[kk * kScanPlane + scan_slot(k * 64 + lane)] = (Tv)0;
                } else if (sh <= (size_t)kScanSeg) {   // the shifted ticks lie in the two staged segments: no second trip to memory
#pragma unroll
                    for (int k = 0; k < kScanChunk; k++) {
                        const int tl = k * 64 + lane, ts = tl + (int)sh;
                        sb[kk * kScanPlane + scan_slot(tl)] = ts < kScanSeg ? vb[scan_slot(ts)] : vr[scan_slot(ts - kScanSeg)];
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < kScanChunk; k++) {
                        const int tl = k * 64 + lane;
                        const size_t t = seg0 + tl + sh;
                        Tv y = 0, p = 0;
                        if (t < T) { y = yrow[t]; p = prow[t]; }
                        sb[kk * kScanPlane + scan_slot(tl)] = (t < T && !isnan(y)) ? (Tv)((double)y - (double)p) : (Tv)0;
                    }
                }
            }
            __syncthreads();
            // 1. per lag the chunk's response: the smoother's less the shifted plane's under w_k (rows past K are zero: a copy of the smoother)
            double wn[KG][D], r[KG][D], s[KG][D];
#pragma unroll
            for (int kk = 0; kk < KG; kk++) {
#pragma unroll
                for (int j = 0; j < D; j++) wn[kk][j] = -tw[W::W + (k0 + kk) * D + j];   // (k0 + kk < kLagMaxLags: KG divides it)
                chunk_response_bwd<double, D, Tv>(sb + kk * kScanPlane + lane * kScanPitch, G, wn[kk], r[kk]);
                double se[D], in[D];
#pragma unroll
                for (int j = 0; j < D; j++) se[j] = sseg[(k0 + kk) * D + j];
                matvec<double, D>(pw, se, in);   // the state that enters from the right, through lane 63's chunk
#pragma unroll
                for (int j = 0; j < D; j++) {
                    r[kk][j] += ra[j];
                    if (lane == 63) r[kk][j] += in[j];
                    s[kk][j] = se[j];
                }
            }
            // 2. mirrored scan of the responses: r becomes the state that leaves this lane's chunk on the left
            scan_responses_bwd<D, KG>(pw, r, lane);
#pragma unroll
            for (int kk = 0; kk < KG; kk++)
#pragma unroll
                for (int j = 0; j < D; j++) {
                    const double nb = __shfl_down(r[kk][j], 1, 64), left = __shfl(r[kk][j], 0, 64);
                    if (lane != 63) s[kk][j] = nb;
                    if (lane == 0) sseg[(k0 + kk) * D + j] = left;
                }
            // 3. replay per lag: s_0 in place of the shifted plane
#pragma unroll
            for (int kk = 0; kk < KG; kk++) {
                Tv* sv = sb + kk * kScanPlane + lane * kScanPitch;
                for (int i = kScanChunk - 1; i >= 0; i--) {
                    double sn[D];
                    matvec<double, D>(G, s[kk], sn);
                    const double e = (double)v[i], es = (double)sv[i];
#pragma unroll
                    for (int j = 0; j < D; j++) s[kk][j] = fma(Kg[j], e, fma(wn[kk][j], es, sn[j]));
                    sv[i] = (Tv)s[kk][0];
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KG; kk++) {
                if (k0 + kk < K) {
                    Tv* krow = orow + (size_t)(k0 + kk) * plane_stride;
#pragma unroll
                    for (int k = 0; k < kScanChunk; k++) {
                        const int tl = k * 64 + lane;
                        const size_t t = seg0 + tl;
                        if (t < T) krow[t] = pseg[k] + sb[kk * kScanPlane + scan_slot(tl)];   // lag = p + s_0
                    }
                }
            }
            __syncthreads();
        }
    }
}

// Tick by tick, one lane per latent: the latents the scan kernels do not take, the NaN rows of failed latents when they do not run, every status word.
template <typename Tv, int D>
__global__ void __launch_bounds__(64) lagged_serial_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ sm,
                                                           const double* __restrict__ lt, size_t L, const Tv* x_in, Tv* x_out, size_t T_state,
                                                           LagList lags, int K, Tv* ypred, Tv* out, size_t ld_out, size_t plane_stride, int* status,
                                                           int path) {
    using B = SM<D>;
    using W = LT<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* tb = sm + l * B::SIZE;
    const double* tw = lt + l * W::SIZE;
    const Route route = latent_route(tb[B::STATUS], tb[B::GROWTH], scan_growth_bound<double>(), path);
    if (status) status[l] = route == Route::kFailed ? 1 : 0;
    Tv* prow = ypred + l * ld_out;
    Tv* orow = out + l * ld_out;
    if (route == Route::kFailed && path == 1) {   // (else smooth_fwd_kernel and lagged_bwd_kernel wrote them)
        write_failed<Tv, D>(prow, 0, 1, T, x_out + l * D, 0, 1);
        write_failed<Tv, D>(orow, plane_stride, K, T, x_out + l * D, 0, 1);
    }
    if (route != Route::kSerial) return;
    double A[NN], G[NN], Kg[D], x[D];
    for (int i = 0; i < NN; i++) { A[i] = tb[B::A + i]; G[i] = tb[B::G + i]; }
    for (int i = 0; i < D; i++) { Kg[i] = tb[B::K + i]; x[i] = (double)x_in[l * D + i]; }
    const Tv* yrow = Ty + l * ld_in;
    if (T_state == 0)
        for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)x[i];
    for (size_t t = 0; t < T; t++) {
        double xp[D];
        matvec<double, D>(A, x, xp);
        const double y = (double)yrow[t], p = xp[0];
        const double v = isnan(y) ? 0.0 : y - p;
        for (int j = 0; j < D; j++) x[j] = fma(Kg[j], v, xp[j]);
        prow[t] = (Tv)p;
        if (t + 1 == T_state)
            for (int i = 0; i < D; i++) x_out[l * D + i] = (Tv)x[i];
    }
    for (int k = 0; k < K; k++) {
        const size_t sh = (size_t)lags.lag[k] + 1;
        double wn[D], s[D];
        for (int i = 0; i < D; i++) { wn[i] = -tw[W::W + k * D + i]; s[i] = 0.0; }
        Tv* krow = orow + (size_t)k * plane_stride;
        for (size_t t = T; t-- > 0;) {
            const double y = (double)yrow[t], p = (double)prow[t];
            const double v = isnan(y) ? 0.0 : y - p;
            double vs = 0.0;
            if (t + sh < T) {
                const double y2 = (double)yrow[t + sh], p2 = (double)prow[t + sh];
                vs = isnan(y2) ? 0.0 : y2 - p2;
            }
            double sn[D];
            matvec<double, D>(G, s, sn);
            for (int j = 0; j < D; j++) s[j] = fma(Kg[j], v, fma(wn[j], vs, sn[j]));
            krow[t] = (Tv)(p + s[0]);
        }
    }
}

}  // namespace
}  // namespace moihgp

// ---- the tables: fp64, written for accuracy (no contraction, as smoother.hip's) ---------------------------------------------------------------
#pragma clang fp contract(off)

namespace moihgp {
namespace {

template <int D>
__global__ void __launch_bounds__(64) lagged_tables_kernel(const double* __restrict__ sm, size_t L, LagList lags, int K, double* __restrict__ lt) {
    using S = SM<D>;
    using W = LT<D>;
    constexpr int NN = D * D;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t l = idx / (size_t)K;
    const int k = (int)(idx % (size_t)K);
    if (l >= L) return;
    const double* s = sm + l * (size_t)S::SIZE;
    double* o = lt + l * (size_t)W::SIZE;
    const bool failed = s[S::STATUS] != 0.0;
    double G[NN], P[NN], Gl[NN], Pn[NN];
    for (int i = 0; i < NN; i++) { G[i] = s[S::G + i]; P[i] = G[i]; Gl[i] = (i % (D + 1)) == 0 ? 1.0 : 0.0; }
    unsigned h = (unsigned)lags.lag[k];
    while (h) {   // Gl = G^lag by binary powering
        if (h & 1u) {
            matmul<double, D>(Gl, P, Pn);
            for (int i = 0; i < NN; i++) Gl[i] = Pn[i];
        }
        h >>= 1;
        if (h) {
            matmul<double, D>(P, P, Pn);
            for (int i = 0; i < NN; i++) P[i] = Pn[i];
        }
    }
    // w = G^lag (G K)
    double gk[D];
    for (int i = 0; i < D; i++) {
        double t = 0.0;
        for (int j = 0; j < D; j++) t += G[i * D + j] * s[S::K + j];
        gk[i] = t;
    }
    for (int i = 0; i < D; i++) {
        double t = 0.0;
        for (int j = 0; j < D; j++) t += Gl[i * D + j] * gk[j];
        o[W::W + k * D + i] = t;
    }
    // Ps_00 + row_0(G^lag) (PF - Ps) row_0(G^lag)^T
    double q = 0.0;
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) q += Gl[i] * (s[S::PF + i * D + j] - s[S::PS + i * D + j]) * Gl[j];
    o[W::VAR + k] = failed ? __builtin_nan("") : s[S::PS] + q;
    if (k == K - 1)
        for (int kk = K; kk < kLagMaxLags; kk++) {
            for (int j = 0; j < D; j++) o[W::W + kk * D + j] = 0.0;
            o[W::VAR + kk] = 0.0;
        }
    if (k == 0) o[W::STATUS] = failed ? 1.0 : 0.0;
}

}  // namespace

void launch_lagged_tables(int d, const double* sm, size_t L, const LagList& lags, int K, double* lt, hipStream_t stream) {
    if (L == 0) return;
    dim3 block(64), grid((unsigned)((L * (size_t)K + 63) / 64));
    dispatch_dim(d, [&](auto dim) { hipLaunchKernelGGL((lagged_tables_kernel<decltype(dim)::value>), grid, block, 0, stream, sm, L, lags, K, lt); });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

// The call's record and its planes are unpacked here, at the launch lines.
template <typename Tv, int D, int KG>
static void launch_bwd_kg(const SweepIo& io, const double* sm, const double* lt, const LagList& lags, const SweepPlanes& out, int path) {
    const size_t lds = sizeof(Tv) * (size_t)(2 + KG) * kScanPlane;
    hipLaunchKernelGGL((lagged_bwd_kernel<Tv, D, KG>), dim3((unsigned)io.L), dim3(64), lds, io.stream, (const Tv*)io.Ty, io.T, io.ld, sm, lt, lags, out.K,
                       (const Tv*)io.yhat, (Tv*)out.base, io.ld_out, out.stride, (Tv*)io.x, path);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_lagged_stream(int d, const SweepIo& io, const double* sm, const double* lt, size_t T_state, const LagList& lags, const SweepPlanes& out,
                          int* status, int path) {
    if (io.L == 0) return;
    if (io.T > 0 && path != 1) launch_smooth_forward(d, io, sm, T_state, path);
    dispatch_stream(d, io.dtype, [&](auto tv, auto dim) {
        using Tv = decltype(tv);
        constexpr int D = decltype(dim)::value;
        if (io.T > 0 && path != 1) {
            // lags staged per replay: one for a single lag, else two (four LDS planes per wavefront: 17 KB at fp32, 35 KB at fp64)
            if (out.K == 1) launch_bwd_kg<Tv, D, 1>(io, sm, lt, lags, out, path);
            else launch_bwd_kg<Tv, D, 2>(io, sm, lt, lags, out, path);
        }
        hipLaunchKernelGGL((lagged_serial_kernel<Tv, D>), dim3((unsigned)((io.L + 63) / 64)), dim3(64), 0, io.stream, (const Tv*)io.Ty, io.T, io.ld, sm, lt,
                           io.L, (const Tv*)io.xin, (Tv*)io.x, T_state, lags, out.K, (Tv*)io.yhat, (Tv*)out.base, io.ld_out, out.stride, status,
                           io.T > 0 ? path : 1);
    });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

}  // namespace moihgp
