// sampler.hip -- seeded steady-state posterior sampling of whole series-major streams (include/moihgp.h moihgp_sample_stream).
//
// A sample is the smoother's mean plus a stationary deviation process whose scalar autocovariance is that of the steady-state posterior,
//   r[k] = H G^k Ps H^T     (G, Ps: the smoother's tables, SM<D>),
// drawn through its innovations realization (one scalar normal per tick; the state-form backward sampler does not exist here, its noise
// covariance PF - G P G^T is indefinite for Matern-5/2).  Per latent, with h = e0, N = Ps h, r0 = Ps_00, Sigma solves
//   sigma^2 = r0 - Sigma_00      B = G (N - Sigma h) / sigma^2      Sigma = G Sigma G^T + sigma^2 B B^T
// and per sample, backward in time, with n[t] and g the normals of sample_normals4 below:
//   u[T-1] = Lc g;   e = sigma n[t];   o[t] = u[t]_0 + e;   u[t-1] = G u[t] + B e;   sample[t] = ysmooth[t] + o[t]
//
// Kernels
//   sampler_tables_kernel   one lane per latent, fp64: Sigma by 64 fixed-point steps from zero and up to 8 Newton steps (the d^2 x d^2 Stein solve
//                           of the closed loop G - B h^T), accepted by the autocovariance it reproduces (SP<D>::ERR <= 1e-9 or status 2), the
//                           Cholesky factor Lc, and the growth figure of G (powers up to 2 kScanChunk, and G^kScanSeg).  Launch-latency work.
//   sample_sweep_kernel     one wavefront per (latent, group of kSampleGroup samples) walks the kScanSeg-tick segments from the end: the segment of
//                           ysmooth is staged once per group; per sample every lane draws the 16 normals of its chunk (four Philox blocks) into
//                           its own row of the out plane, a mirrored Kogge-Stone scan of the chunk maps (G^kScanChunk, the chunk's response to its noise) gives the
//                           lane its entering state, and the replay emits ysmooth + u_0 + e into a plane that is staged out coalesced.  The
//                           states carried from segment to segment live in LDS (kSampleGroup x D doubles).  No noise touches memory.
//   sample_serial_kernel    one lane per (latent, sample), tick by tick: the latents the sweep leaves (growth bound failed, option "sample_path"
//                           = 1), the NaN rows of failed latents and every status word.
//   sample_noise_kernel     the generator alone (moihgp_sample_noise), through the same sample_normals4.
// Arithmetic is fp64 for both stream types (G exceeds the fp32 growth bound on ordinary parameters); the normals are formed in fp32.  The
// chunk-scan machinery of the sweep is scan_sweep.h (its backward half, chunk_response_bwd and the mirrored scan, shared with smooth_bwd_kernel);
// the Stein solve (stein_solve) and the growth figure (segment_growth) of the tables kernel are stationary_common.h's.
#include "scan_sweep.h"
#include "philox_normals.h"

namespace moihgp {
namespace {

constexpr int kSampleGroup = 8;   // samples per wavefront of sample_sweep_kernel

// ---- the generator: philox_normals.h (sample_normals4, shared with paths.hip) ----------------------------------------------------------------------
// u[T-1] = Lc g (Lc lower triangular, g_0 .. g_{D-1} of the start block)
template <int D>
__device__ __forceinline__ void start_state(const double* Lc, unsigned long long seed, uint32_t latent, uint32_t sample, double* u) {
    float g[4];
    sample_normals4(seed, 0u, latent, sample, 1u, g);
#pragma unroll
    for (int i = 0; i < D; i++) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j <= i; j++) t = fma(Lc[i * D + j], (double)g[j], t);
        u[i] = t;
    }
}

// 0 ok, 1 the Kalman DARE failed, 2 the realization failed; Route of the latents that are left (the growth figure is the sampler's: G alone)
__device__ __forceinline__ int sample_status(double sm_status, double sp_status) { return sm_status != 0.0 ? 1 : (sp_status != 0.0 ? 2 : 0); }

// ---- the sweep ---------------------------------------------------------------------------------------------------------------------------------
template <typename Tv, int D>
__global__ void __launch_bounds__(64) sample_sweep_kernel(const double* __restrict__ sm, const double* __restrict__ sp, size_t T,
                                                          const Tv* __restrict__ ysm, size_t ld_out, Tv* __restrict__ samples, size_t plane_stride,
                                                          int nsamples, unsigned long long seed, uint32_t sample0, uint32_t latent0, int path) {
    using BM = SM<D>;
    using BP = SP<D>;
    constexpr int NN = D * D;
    __shared__ double yb[kScanPlane];
    __shared__ double ob[kScanPlane];
    __shared__ double carry[kSampleGroup * D];
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x;
    const int s0 = (int)blockIdx.y * kSampleGroup;
    const int ns = nsamples - s0 < kSampleGroup ? nsamples - s0 : kSampleGroup;
    const double* tm = sm + l * BM::SIZE;
    const double* tp = sp + l * BP::SIZE;
    if (sample_status(tm[BM::STATUS], tp[BP::STATUS]) != 0) return;
    if (latent_route(0.0, tp[BP::GROWTH], scan_growth_bound<double>(), path) != Route::kScan) return;
    double G[NN], MB[NN], Bv[D];
#pragma unroll
    for (int i = 0; i < NN; i++) { G[i] = tm[BM::G + i]; MB[i] = tm[BM::MB + i]; }
#pragma unroll
    for (int i = 0; i < D; i++) Bv[i] = tp[BP::B + i];
    const double sigma = tp[BP::SIGMA];
    const uint32_t lat = latent0 + (uint32_t)l;
    if (lane < ns) {
        double Lc[NN], u[D];
#pragma unroll
        for (int i = 0; i < NN; i++) Lc[i] = tp[BP::LC + i];
        start_state<D>(Lc, seed, lat, sample0 + (uint32_t)(s0 + lane), u);
#pragma unroll
        for (int i = 0; i < D; i++) carry[lane * D + i] = u[i];
    }
    __syncthreads();
    const Tv* yrow = ysm + l * ld_out;
    const double* my = yb + lane * kScanPitch;
    double* mo = ob + lane * kScanPitch;
    const size_t nseg = (T + kScanSeg - 1) / kScanSeg;
    for (size_t sg = nseg; sg-- > 0;) {
        const size_t seg0 = sg * kScanSeg;
        stage_in(yrow, seg0, T, lane, yb);
        __syncthreads();
        // this lane's ticks t0 .. t0 + n (the ragged tail is the identity: the state that enters the last segment is u[T-1])
        const size_t t0 = seg0 + (size_t)lane * kScanChunk;
        const int n = lane_tick_count(seg0, T, lane);
        double Pn[NN];                          // G^n, the same for every sample
        if (n == kScanChunk) {
#pragma unroll
            for (int i = 0; i < NN; i++) Pn[i] = MB[i];
        } else {
#pragma unroll
            for (int i = 0; i < NN; i++) Pn[i] = (i % (D + 1)) == 0 ? 1.0 : 0.0;
            for (int i = 0; i < n; i++) {
                double t[NN];
                matmul<double, D>(G, Pn, t);
#pragma unroll
                for (int j = 0; j < NN; j++) Pn[j] = t[j];
            }
        }
        for (int s = 0; s < ns; s++) {
            // the lane's 16 normals, four Philox blocks, as e = sigma n into its row of the out plane (zero past T)
#pragma nounroll
            for (int b = 0; b < kScanChunk / 4; b++) {
                float nz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (4 * b < n) sample_normals4(seed, (uint32_t)(t0 >> 2) + b, lat, sample0 + (uint32_t)(s0 + s), 0u, nz);   // (none past T)
#pragma unroll
                for (int j = 0; j < 4; j++) mo[4 * b + j] = 4 * b + j < n ? sigma * (double)nz[j] : 0.0;
            }
            // 1. the chunk's response to its noise from a zero state at its end (ticks past T come first and leave it zero)
            double Phi[NN], r[D], u[D], useg[D];
#pragma unroll
            for (int i = 0; i < NN; i++) Phi[i] = Pn[i];
            chunk_response_bwd<double, D>(mo, G, Bv, r);
            // 2. mirrored scan: the state entering this lane's chunk from the right
#pragma unroll
            for (int i = 0; i < D; i++) useg[i] = carry[s * D + i];
            scan_maps<double, D, false>(Phi, r, lane);
            start_states<double, D, false>(Phi, r, useg, u, lane);
            if (lane == 0)
#pragma unroll
                for (int i = 0; i < D; i++) carry[s * D + i] = useg[i];
            // 3. replay: sample = ysmooth + u_0 + e (in place of e)
            for (int i = n - 1; i >= 0; i--) {
                const double e = mo[i];
                mo[i] = my[i] + (u[0] + e);
                tick_step<double, D>(G, Bv, e, u);
            }
            __syncthreads();
            stage_out(ob, samples + (size_t)(s0 + s) * plane_stride + l * ld_out, seg0, T, lane);
            __syncthreads();
        }
    }
}

// Tick by tick, one lane per (latent, sample): the latents the sweep does not take, the NaN rows of failed latents, every status word.
template <typename Tv, int D>
__global__ void __launch_bounds__(64) sample_serial_kernel(const double* __restrict__ sm, const double* __restrict__ sp, size_t L, size_t T,
                                                           const Tv* __restrict__ ysm, size_t ld_out, Tv* __restrict__ samples, size_t plane_stride,
                                                           int nsamples, unsigned long long seed, uint32_t sample0, uint32_t latent0, int* status,
                                                           int path) {
    using BM = SM<D>;
    using BP = SP<D>;
    constexpr int NN = D * D;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= L * (size_t)nsamples) return;
    const size_t l = idx % L;
    const int s = (int)(idx / L);
    const double* tm = sm + l * BM::SIZE;
    const double* tp = sp + l * BP::SIZE;
    const int st = sample_status(tm[BM::STATUS], tp[BP::STATUS]);
    if (status && s == 0) status[l] = st;
    Tv* row = samples + (size_t)s * plane_stride + l * ld_out;
    if (st != 0) {
        const Tv nan = (Tv)__builtin_nan("");
        for (size_t t = 0; t < T; t++) row[t] = nan;
        return;
    }
    if (latent_route(0.0, tp[BP::GROWTH], scan_growth_bound<double>(), path) != Route::kSerial) return;
    double G[NN], Lc[NN], Bv[D], u[D];
    for (int i = 0; i < NN; i++) { G[i] = tm[BM::G + i]; Lc[i] = tp[BP::LC + i]; }
    for (int i = 0; i < D; i++) Bv[i] = tp[BP::B + i];
    const double sigma = tp[BP::SIGMA];
    const uint32_t lat = latent0 + (uint32_t)l, smp = sample0 + (uint32_t)s;
    start_state<D>(Lc, seed, lat, smp, u);
    const Tv* yrow = ysm + l * ld_out;
    float nz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (size_t t = T; t-- > 0;) {
        const int k = (int)(t & 3);
        if (k == 3 || t == T - 1) sample_normals4(seed, (uint32_t)(t >> 2), lat, smp, 0u, nz);
        const double e = sigma * (double)(k == 0 ? nz[0] : k == 1 ? nz[1] : k == 2 ? nz[2] : nz[3]);
        row[t] = (Tv)((double)yrow[t] + (u[0] + e));
        tick_step<double, D>(G, Bv, e, u);
    }
}

// noise [S][L][ld]: n[t] of (latent0 + l, sample0 + s); start [S][L][4] or null: g_0 .. g_3.  One lane per block of four ticks.
__global__ void __launch_bounds__(256) sample_noise_kernel(unsigned long long seed, uint32_t latent0, size_t L, uint32_t sample0, size_t S, size_t T,
                                                           float* __restrict__ noise, size_t ld, float* __restrict__ start) {
    const size_t nq = (T + 3) / 4 + 1;          // the last one is the start block
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S * L * nq) return;
    const size_t q = idx % nq, row = idx / nq, l = row % L, s = row / L;
    float n[4];
    if (q == nq - 1) {
        if (!start) return;
        sample_normals4(seed, 0u, latent0 + (uint32_t)l, sample0 + (uint32_t)s, 1u, n);
        for (int i = 0; i < 4; i++) start[row * 4 + i] = n[i];
        return;
    }
    sample_normals4(seed, (uint32_t)q, latent0 + (uint32_t)l, sample0 + (uint32_t)s, 0u, n);
    for (int i = 0; i < 4; i++)
        if (4 * q + i < T) noise[row * ld + 4 * q + i] = n[i];
}

}  // namespace
}  // namespace moihgp

// ---- the tables: fp64, one lane per latent, written for accuracy (no contraction, as the smoother's) -------------------------------------------
#pragma clang fp contract(off)
#include "stationary_common.h"

namespace moihgp {
namespace {

template <int D>
__global__ void __launch_bounds__(64) sampler_tables_kernel(const double* __restrict__ sm, size_t L, double* __restrict__ sp) {
    using BM = SM<D>;
    using BP = SP<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* tm = sm + l * BM::SIZE;
    double* o = sp + l * BP::SIZE;
    double G[NN], GT[NN], N[D], Sg[NN], F[NN], Bv[D], T1[NN], T2[NN];
    for (int i = 0; i < NN; i++) { G[i] = tm[BM::G + i]; Sg[i] = 0.0; }
    for (int i = 0; i < D; i++) N[i] = tm[BM::PS + i * D];
    const double r0 = tm[BM::PS];
    mt<D>(G, GT);
    // sigma^2, B and the residual F(Sigma) = G Sigma G^T + sigma^2 B B^T - Sigma (symmetrised) at the current Sigma
    auto parts = [&]() {
        const double s2 = r0 - Sg[0];
        double w[D];
        for (int i = 0; i < D; i++) w[i] = N[i] - Sg[i * D];
        mv<D>(G, w, Bv);
        for (int i = 0; i < D; i++) Bv[i] /= s2;
        mm<D>(G, Sg, T1); mm<D>(T1, GT, T2);
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) T1[i * D + j] = T2[i * D + j] + s2 * Bv[i] * Bv[j] - Sg[i * D + j];
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) F[i * D + j] = (T1[i * D + j] + T1[j * D + i]) / 2.0;
        return s2;
    };
    // the limit of the iteration from zero ...
#pragma nounroll
    for (int it = 0; it < 64; it++) {
        parts();
        for (int i = 0; i < NN; i++) Sg[i] += F[i];
    }
    // ... polished (or, where the iteration is slow, reached) by Newton steps dSigma = Ac dSigma Ac^T + F(Sigma), Ac = G - B h^T.  The stopping
    // rule is relative to max |Sigma|: its derivative components are orders of magnitude above r0.
#pragma nounroll
    for (int step = 0; step < 8; step++) {
        parts();
        double fm = 0.0, m = 0.0;
        for (int i = 0; i < NN; i++) { fm = fmax(fm, fabs(F[i])); m = fmax(m, fabs(Sg[i])); }
        if (!isfinite(m) || !(fm > 1e-15 * m)) break;
        double Ac[NN], dS[NN];
        for (int i = 0; i < NN; i++) Ac[i] = G[i];
        for (int i = 0; i < D; i++) Ac[i * D] -= Bv[i];
        stein_solve<D>(Ac, F, dS);
        bool fin = true;
        for (int i = 0; i < NN; i++) fin = fin && isfinite(dS[i]);
        if (!fin) break;
        for (int i = 0; i < NN; i++) Sg[i] += dS[i];
    }
    const double s2 = parts();
    // acceptance: the autocovariance the realization reproduces against r[k] = (G^k N)_0, k < 64
    double v[D], w[D], h0[D];
    for (int i = 0; i < D; i++) { v[i] = N[i]; h0[i] = Sg[i * D]; }
    mv<D>(G, h0, w);
    for (int i = 0; i < D; i++) w[i] += s2 * Bv[i];
    double err = fabs(Sg[0] + s2 - r0);
#pragma nounroll
    for (int k = 1; k < 64; k++) {
        mv<D>(G, v, v);
        const double d = fabs(w[0] - v[0]);
        err = (d > err || isnan(d)) ? d : err;
        mv<D>(G, w, w);
    }
    err /= r0;
    bool ok = isfinite(err) && err <= 1e-9 && s2 > 0.0 && isfinite(s2);
    for (int i = 0; i < NN; i++) ok = ok && isfinite(Sg[i]);
    for (int i = 0; i < D; i++) ok = ok && isfinite(Bv[i]);
    // Lc: lower Cholesky factor of Sigma; a pivot <= 0 gives a zero column
    double Lc[NN];
    for (int i = 0; i < NN; i++) Lc[i] = 0.0;
    for (int j = 0; j < D; j++) {
        double p = Sg[j * D + j];
        for (int k = 0; k < j; k++) p -= Lc[j * D + k] * Lc[j * D + k];
        if (!(p > 0.0)) continue;
        const double dj = sqrt(p);
        Lc[j * D + j] = dj;
        for (int i = j + 1; i < D; i++) {
            double t = Sg[i * D + j];
            for (int k = 0; k < j; k++) t -= Lc[i * D + k] * Lc[j * D + k];
            Lc[i * D + j] = t / dj;
        }
    }
    for (int i = 0; i < NN; i++) ok = ok && isfinite(Lc[i]);
    // growth of the sweep's maps: G^1 .. G^(2 kScanChunk), and what a whole segment composes, G^kScanSeg
    const double growth = segment_growth<D, kScanChunk, kScanSeg>(G, T1, T2);
    for (int i = 0; i < NN; i++) ok = ok && isfinite(T2[i]);
    for (int i = 0; i < NN; i++) { o[BP::LC + i] = Lc[i]; o[BP::SG + i] = Sg[i]; }
    for (int i = 0; i < D; i++) o[BP::B + i] = Bv[i];
    o[BP::SIGMA] = s2 > 0.0 ? sqrt(s2) : 0.0;
    o[BP::SIGMA2] = s2;
    o[BP::ERR] = err;
    o[BP::GROWTH] = growth;
    o[BP::STATUS] = tm[BM::STATUS] != 0.0 ? 1.0 : (ok ? 0.0 : 2.0);
}

}  // namespace

void launch_sampler_tables(int d, const double* sm, size_t L, double* sp, hipStream_t stream) {
    if (L == 0) return;
    dim3 block(64), grid((unsigned)((L + 63) / 64));
    dispatch_dim(d, [&](auto dim) { hipLaunchKernelGGL((sampler_tables_kernel<decltype(dim)::value>), grid, block, 0, stream, sm, L, sp); });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

// The call's record and its planes are unpacked here, at the launch lines.
void launch_sample_stream(int d, const SweepIo& io, const double* sm, const double* sp, const SweepPlanes& samples, unsigned long long seed,
                          unsigned sample0, unsigned latent0, int* status, int path) {
    if (io.L == 0) return;
    dispatch_stream(d, io.dtype, [&](auto tv, auto dim) {
        using Tv = decltype(tv);
        constexpr int D = decltype(dim)::value;
        const int nsamples = samples.K;
        if (io.T > 0 && path != 1) {
            const dim3 grid((unsigned)io.L, (unsigned)((nsamples + kSampleGroup - 1) / kSampleGroup));
            hipLaunchKernelGGL((sample_sweep_kernel<Tv, D>), grid, dim3(64), 0, io.stream, sm, sp, io.T, (const Tv*)io.yhat, io.ld_out, (Tv*)samples.base,
                               samples.stride, nsamples, seed, sample0, latent0, path);
            MOIHGP_HIP_FATAL(hipGetLastError());
        }
        const size_t n = io.L * (size_t)nsamples;
        hipLaunchKernelGGL((sample_serial_kernel<Tv, D>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, io.stream, sm, sp, io.L, io.T, (const Tv*)io.yhat,
                           io.ld_out, (Tv*)samples.base, samples.stride, nsamples, seed, sample0, latent0, status, io.T > 0 ? path : 1);
        MOIHGP_HIP_FATAL(hipGetLastError());
    });
}

void launch_sample_noise(unsigned long long seed, unsigned latent0, size_t L, unsigned sample0, size_t S, size_t T, float* noise, size_t ld, float* start,
                         hipStream_t stream) {
    const size_t n = S * L * ((T + 3) / 4 + 1);
    if (n == 0) return;
    hipLaunchKernelGGL(sample_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed, latent0, L, sample0, S, T, noise, ld, start);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

}  // namespace moihgp
