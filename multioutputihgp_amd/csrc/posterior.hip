// posterior.hip -- exact smoothing across missing ticks (include/moihgp.h moihgp_posterior_stream): the time-varying Kalman filter from the model's
// own prior N(0, Pinf) and the RTS backward pass, with no update at a NaN tick.  For any pattern of missing ticks this is the GP posterior at
// every tick, and the forward pass sums the exact log marginal likelihood.  No DARE and no steady-state gain anywhere.
//
// The covariance recursion is a Riccati map, not an affine one: the chunk scan of scan_sweep.h does not apply and the walk is serial in time.
// The parallelism is across latents, one latent per lane, 64 latents per wavefront (one wavefront per workgroup).
//
// Kernels
//   posterior_tables_kernel   one lane per latent, fp64: the block PT<D> (A from the constant block, Pinf and R from the model, Q = sym(Pinf - A Pinf A^T)).
//                             Launch-latency work, once per parameter set (capi.cpp builds it lazily).
//   posterior_fwd_kernel      the filter.  The 64 rows go through LDS in tiles of kPostTile ticks (loads coalesced along time, odd pitch), each lane
//                             walks its own row.  Every kPostBlock ticks the lanes store a checkpoint (xf, upper triangle of PF) to scratch laid out
//                             [block][component][L] (coalesced across lanes).  At the end: x, P_end, nll and the breakdown flag.
//   posterior_bwd_kernel      the smoother.  Tiles from the end; per block of a tile the forward recursion is recomputed from the block's checkpoint
//                             with (xf, PF) of every tick kept in LDS, then the block is walked backward: P[t+1] and xp[t+1] are recomputed from
//                             (xf, PF)[t], G = PF[t] A^T P[t+1]^-1 by pivoted elimination (Q is indefinite for Matern-5/2: no Cholesky).  Means
//                             and variances leave through LDS tiles, so global stores run along time.  A latent that broke down (status 5) gets
//                             its NaN rows, end state, P_end and nll here.
// Whether a tick is observed differs from lane to lane: the update is computed by every lane and chosen by selects, and a breakdown is a sticky
// per-lane flag.  Lanes past the last latent walk a copy of the last latent and store nothing.  fp64 arithmetic for both stream dtypes, no
// contraction: the two kernels must produce the same (xf, PF) from the same lines.
#pragma clang fp contract(off)
#include "stationary_common.h"
#include "stream_tables.h"

namespace moihgp {
namespace {

constexpr int kPostPitch = kPostTile + 1;       // LDS row pitch of one latent's tile (odd: the lanes' walks hit different banks)
static_assert(kPostTile % kPostBlock == 0, "a tile holds whole blocks");

template <int D>
struct PostModel {
    double A[D * D], AT[D * D], Q[D * D], Pinf[D * D], R;
};

template <int D>
__device__ __forceinline__ void post_load_model(const double* __restrict__ pt, size_t l, PostModel<D>& m) {
    using B = PT<D>;
    const double* b = pt + l * B::SIZE;
    for (int i = 0; i < D * D; i++) { m.A[i] = b[B::A + i]; m.Q[i] = b[B::Q + i]; m.Pinf[i] = b[B::PINF + i]; }
    m.R = b[B::R];
    mt<D>(m.A, m.AT);
}

template <int D>
__device__ __forceinline__ void sym(double* X) {
    for (int i = 0; i < D; i++)
        for (int j = i + 1; j < D; j++) {
            const double a = (X[i * D + j] + X[j * D + i]) / 2.0;
            X[i * D + j] = a; X[j * D + i] = a;
        }
}

template <int D>
__device__ __forceinline__ bool all_finite(const double* x, const double* P) {
    bool ok = true;
    for (int i = 0; i < D; i++) ok = ok && isfinite(x[i]);
    for (int i = 0; i < D * D; i++) ok = ok && isfinite(P[i]);
    return ok;
}

// xp = A xf, P = sym(A PF A^T + Q); the first tick takes the prior (first is the same in every lane)
template <int D>
__device__ __forceinline__ void post_predict(const PostModel<D>& m, bool first, const double* xf, const double* PF, double* xp, double* P) {
    double T1[D * D];
    mv<D>(m.A, xf, xp);
    mm<D>(m.A, PF, T1);
    mm<D>(T1, m.AT, T1);
    for (int i = 0; i < D * D; i++) P[i] = T1[i] + m.Q[i];
    sym<D>(P);
    if (first) {
        for (int i = 0; i < D; i++) xp[i] = 0.0;
        for (int i = 0; i < D * D; i++) P[i] = m.Pinf[i];
    }
}

// The update of one tick, chosen per lane by selects: observed (y is not NaN) or missing.  bad is sticky.  NLL: the likelihood term too (the forward
// kernel; the backward kernel's recompute leaves it out -- the (xf, PF) lines are the same in both).
template <int D, bool NLL>
__device__ __forceinline__ void post_update(const PostModel<D>& m, double y, const double* xp, const double* P, double* xf, double* PF, double& nll,
                                            bool& bad) {
    const bool obs = !isnan(y);
    const double S = P[0] + m.R, v = y - xp[0];
    double K[D], U[D * D];
    for (int i = 0; i < D; i++) K[i] = P[i * D] / S;
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) U[i * D + j] = P[i * D + j] - K[i] * P[j];
    sym<D>(U);
    for (int i = 0; i < D; i++) xf[i] = obs ? xp[i] + K[i] * v : xp[i];
    for (int i = 0; i < D * D; i++) PF[i] = obs ? U[i] : P[i];
    if (NLL) {
        const double term = 0.5 * (log(2.0 * M_PI * S) + v * v / S);
        nll += obs ? term : 0.0;
        bad = bad || !isfinite(nll);
    }
    bad = bad || (obs && !(S > 0.0)) || !all_finite<D>(xf, PF);
}

// one tile of the 64 rows, global -> LDS as doubles: row r of the tile is latent l0 + r, a row past the last latent reads as missing ticks
template <typename Tv>
__device__ __forceinline__ void post_load_tile(const Tv* __restrict__ Ty, size_t ld_in, size_t l0, size_t L, size_t t0, int n, int lane, double* tile) {
    for (int r = 0; r < 64; r++)
        if (lane < n) tile[r * kPostPitch + lane] = l0 + r < L ? (double)Ty[(l0 + r) * ld_in + t0 + lane] : __builtin_nan("");
}
// ... and LDS -> global: ticks t0 .. t0 + n - 1 of the rows of the latents that exist, nothing else
template <typename Tv>
__device__ __forceinline__ void post_store_tile(const double* tile, Tv* out, size_t ld_out, size_t l0, size_t L, size_t t0, int n, int lane) {
    for (int r = 0; r < 64; r++)
        if (lane < n && l0 + r < L) out[(l0 + r) * ld_out + t0 + lane] = (Tv)tile[r * kPostPitch + lane];
}

template <int D>
__global__ void __launch_bounds__(64) posterior_tables_kernel(int kernel, const double* __restrict__ cb64, size_t L, double* __restrict__ pt) {
    using C = CB<D>;
    using B = PT<D>;
    constexpr int NN = D * D;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double* cb = cb64 + l * C::SIZE;
    double* o = pt + l * B::SIZE;
    double prm[3] = {cb[C::PARAMS + 0], cb[C::PARAMS + 1], cb[C::PARAMS + 2]};
    SS<D> s;
    ss_build<D>(kernel, prm, s);
    double A[NN], AT[NN], T1[NN], Q[NN];
    for (int i = 0; i < NN; i++) A[i] = cb[C::A + i];
    mt<D>(A, AT);
    mm<D>(A, s.Pinf, T1);
    mm<D>(T1, AT, T1);
    for (int i = 0; i < NN; i++) Q[i] = s.Pinf[i] - T1[i];
    sym<D>(Q);
    for (int i = 0; i < NN; i++) { o[B::A + i] = A[i]; o[B::Q + i] = Q[i]; o[B::PINF + i] = s.Pinf[i]; }
    o[B::R] = s.R;
    for (int i = B::R + 1; i < B::SIZE; i++) o[i] = 0.0;
}

// upper triangle <-> full symmetric matrix
template <int D>
__device__ __forceinline__ void sym_pack(const double* P, double* u) {
    int c = 0;
    for (int i = 0; i < D; i++)
        for (int j = i; j < D; j++) u[c++] = P[i * D + j];
}
template <int D>
__device__ __forceinline__ void sym_unpack(const double* u, double* P) {
    int c = 0;
    for (int i = 0; i < D; i++)
        for (int j = i; j < D; j++) { P[i * D + j] = u[c]; P[j * D + i] = u[c]; c++; }
}

template <typename Tv, int D>
__global__ void __launch_bounds__(64) posterior_fwd_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ pt, size_t L,
                                                           double* __restrict__ ckpt, int* __restrict__ badw, Tv* __restrict__ x,
                                                           double* __restrict__ P_end, double* __restrict__ nll_out) {
    constexpr int NN = D * D, NS = D * (D + 1) / 2, NC = D + NS;
    __shared__ double tile[64 * kPostPitch];
    const int lane = threadIdx.x;
    const size_t l0 = (size_t)blockIdx.x * 64, l = l0 + lane;
    const bool live = l < L;
    PostModel<D> m;
    post_load_model<D>(pt, live ? l : L - 1, m);
    double xf[D], PF[NN], xp[D], P[NN], nll = 0.0;
    bool bad = false;
    // the state "before tick 0" is the prior: what a call of no ticks hands out
    for (int i = 0; i < D; i++) xf[i] = 0.0;
    for (int i = 0; i < NN; i++) PF[i] = m.Pinf[i];
    for (size_t t0 = 0; t0 < T; t0 += kPostTile) {
        const int n = (int)(T - t0 < (size_t)kPostTile ? T - t0 : (size_t)kPostTile);
        __syncthreads();
        post_load_tile<Tv>(Ty, ld_in, l0, L, t0, n, lane, tile);
        __syncthreads();
        for (int i = 0; i < n; i++) {
            const size_t t = t0 + i;
            post_predict<D>(m, t == 0, xf, PF, xp, P);
            post_update<D, true>(m, tile[lane * kPostPitch + i], xp, P, xf, PF, nll, bad);
            if ((t + 1) % kPostBlock == 0 && t + 1 < T && live) {      // the state block (t + 1) / kPostBlock starts from
                double u[NS];
                sym_pack<D>(PF, u);
                double* c = ckpt + ((t + 1) / kPostBlock - 1) * (size_t)NC * L + l;
                for (int k = 0; k < D; k++) c[(size_t)k * L] = xf[k];
                for (int k = 0; k < NS; k++) c[(size_t)(D + k) * L] = u[k];
            }
        }
    }
    bad = bad || !all_finite<D>(xf, PF);           // (T == 0: a model that is not finite)
    if (!live) return;
    badw[l] = bad ? 1 : 0;
    for (int i = 0; i < D; i++) x[l * D + i] = (Tv)xf[i];
    if (P_end)
        for (int i = 0; i < NN; i++) P_end[l * NN + i] = PF[i];
    if (nll_out) nll_out[l] = nll;
}

template <typename Tv, int D>
__global__ void __launch_bounds__(64) posterior_bwd_kernel(const Tv* __restrict__ Ty, size_t T, size_t ld_in, const double* __restrict__ pt, size_t L,
                                                           const double* __restrict__ ckpt, const int* __restrict__ badw, Tv* mean, Tv* var,
                                                           size_t ld_out, Tv* x, double* P_end, double* nll_out, int* status) {
    constexpr int NN = D * D, NS = D * (D + 1) / 2, NC = D + NS;
    extern __shared__ double post_lds[];
    double* ym = post_lds;                          // the tile: the stream going in, the means going out
    double* yv = ym + 64 * kPostPitch;              // the tile's variances
    double* st = yv + 64 * kPostPitch;              // [kPostBlock][NC][64]: (xf, upper triangle of PF) of the block's ticks
    int* flag = reinterpret_cast<int*>(st + (size_t)kPostBlock * NC * 64);    // [64] the lanes' breakdown flags, for the row-wise NaN fill
    const int lane = threadIdx.x;
    const size_t l0 = (size_t)blockIdx.x * 64, l = l0 + lane;
    const bool live = l < L;
    PostModel<D> m;
    post_load_model<D>(pt, live ? l : L - 1, m);
    bool bad = badw[live ? l : L - 1] != 0;
    double xs[D], Ps[NN];
    for (int i = 0; i < D; i++) xs[i] = 0.0;
    for (int i = 0; i < NN; i++) Ps[i] = 0.0;
    const size_t ntiles = (T + kPostTile - 1) / kPostTile;
    for (size_t it = ntiles; it-- > 0;) {
        const size_t t0 = it * kPostTile;
        const int n = (int)(T - t0 < (size_t)kPostTile ? T - t0 : (size_t)kPostTile);
        __syncthreads();
        post_load_tile<Tv>(Ty, ld_in, l0, L, t0, n, lane, ym);
        __syncthreads();
        for (int b0 = (n - 1) / kPostBlock * kPostBlock; b0 >= 0; b0 -= kPostBlock) {
            const size_t tb = t0 + b0;                                  // the block's first tick
            const int nb = n - b0 < kPostBlock ? n - b0 : kPostBlock;
            // ---- the block again, forward from its checkpoint
            double xf[D], PF[NN], xp[D], P[NN], nll = 0.0;
            if (tb == 0) {
                for (int i = 0; i < D; i++) xf[i] = 0.0;
                for (int i = 0; i < NN; i++) PF[i] = m.Pinf[i];
            } else {
                double u[NS];
                const double* c = ckpt + (tb / kPostBlock - 1) * (size_t)NC * L + (live ? l : L - 1);
                for (int k = 0; k < D; k++) xf[k] = c[(size_t)k * L];
                for (int k = 0; k < NS; k++) u[k] = c[(size_t)(D + k) * L];
                sym_unpack<D>(u, PF);
            }
            for (int i = 0; i < nb; i++) {
                post_predict<D>(m, tb + i == 0, xf, PF, xp, P);
                post_update<D, false>(m, ym[lane * kPostPitch + b0 + i], xp, P, xf, PF, nll, bad);
                double u[NS];
                sym_pack<D>(PF, u);
                double* s = st + (size_t)i * NC * 64 + lane;
                for (int k = 0; k < D; k++) s[k * 64] = xf[k];
                for (int k = 0; k < NS; k++) s[(D + k) * 64] = u[k];
            }
            // ---- and backward (each lane reads back what it wrote: no barrier)
            for (int i = nb - 1; i >= 0; i--) {
                double u[NS];
                const double* s = st + (size_t)i * NC * 64 + lane;
                for (int k = 0; k < D; k++) xf[k] = s[k * 64];
                for (int k = 0; k < NS; k++) u[k] = s[(D + k) * 64];
                sym_unpack<D>(u, PF);
                if (tb + i == T - 1) {
                    for (int k = 0; k < D; k++) xs[k] = xf[k];
                    for (int k = 0; k < NN; k++) Ps[k] = PF[k];
                } else {
                    double APF[NN], GT[NN], G[NN], dx[D], Gdx[D], Dm[NN], T1[NN];
                    post_predict<D>(m, false, xf, PF, xp, P);           // xp[t+1], P[t+1]
                    mm<D>(m.A, PF, APF);
                    lu_solve<D>(P, APF, GT);                            // G^T = P[t+1]^-1 A PF[t]
                    mt<D>(GT, G);
                    for (int k = 0; k < D; k++) dx[k] = xs[k] - xp[k];
                    mv<D>(G, dx, Gdx);
                    for (int k = 0; k < D; k++) xs[k] = xf[k] + Gdx[k];
                    for (int k = 0; k < NN; k++) Dm[k] = Ps[k] - P[k];
                    mm<D>(G, Dm, T1);
                    mm<D>(T1, GT, T1);
                    for (int k = 0; k < NN; k++) Ps[k] = PF[k] + T1[k];
                    sym<D>(Ps);
                }
                bad = bad || !all_finite<D>(xs, Ps);
                ym[lane * kPostPitch + b0 + i] = xs[0];
                yv[lane * kPostPitch + b0 + i] = Ps[0];
            }
        }
        __syncthreads();
        post_store_tile<Tv>(ym, mean, ld_out, l0, L, t0, n, lane);
        if (var) post_store_tile<Tv>(yv, var, ld_out, l0, L, t0, n, lane);
    }
    // ---- status words; a latent that broke down: NaN rows, end state, P_end and nll
    __syncthreads();
    flag[lane] = bad && live ? 1 : 0;
    __syncthreads();
    if (live) {
        if (status) status[l] = bad ? 5 : 0;
        if (bad) {
            for (int i = 0; i < D; i++) x[l * D + i] = (Tv)__builtin_nan("");
            if (P_end)
                for (int i = 0; i < NN; i++) P_end[l * NN + i] = __builtin_nan("");
            if (nll_out) nll_out[l] = __builtin_nan("");
        }
    }
    for (int r = 0; r < 64; r++) {
        if (!flag[r]) continue;                     // (the same word in every lane)
        for (size_t t = lane; t < T; t += 64) {
            mean[(l0 + r) * ld_out + t] = (Tv)__builtin_nan("");
            if (var) var[(l0 + r) * ld_out + t] = (Tv)__builtin_nan("");
        }
    }
}

template <int D>
constexpr size_t post_bwd_lds_bytes() {
    return sizeof(double) * (2 * 64 * kPostPitch + (size_t)kPostBlock * post_ckpt_doubles(D) * 64) + sizeof(int) * 64;
}

}  // namespace

void launch_posterior_tables(int kernel, int d, const double* cb64, size_t L, double* pt, hipStream_t stream) {
    if (L == 0) return;
    dim3 block(64), grid((unsigned)((L + 63) / 64));
    dispatch_dim(d, [&](auto dim) { hipLaunchKernelGGL((posterior_tables_kernel<decltype(dim)::value>), grid, block, 0, stream, kernel, cb64, L, pt); });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

int launch_posterior_stream(int d, const SweepIo& io, const double* pt, double* scratch, double* P_end, void* var, double* nll, int* status) {
    if (io.L == 0) return 0;
    const size_t L = io.L, T = io.T;
    int rc = 0;
    dispatch_stream(d, io.dtype, [&](auto tv, auto dim) {
        using Tv = decltype(tv);
        constexpr int D = decltype(dim)::value;
        double* ckpt = scratch;
        int* badw = reinterpret_cast<int*>(scratch + (T + kPostBlock - 1) / kPostBlock * (size_t)post_ckpt_doubles(D) * L);
        const dim3 grid((unsigned)((L + 63) / 64)), block(64);
        constexpr size_t smem = post_bwd_lds_bytes<D>();
        auto bwd = posterior_bwd_kernel<Tv, D>;
        // (more dynamic LDS than the default limit needs the attribute; set at every launch: it belongs to the device that is current)
        const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(bwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (attr != hipSuccess) { set_last_error("posterior_bwd_kernel: %zu bytes of LDS refused: %s", smem, hipGetErrorString(attr)); rc = 2; return; }
        hipLaunchKernelGGL((posterior_fwd_kernel<Tv, D>), grid, block, 0, io.stream, (const Tv*)io.Ty, T, io.ld, pt, L, ckpt, badw, (Tv*)io.x, P_end, nll);
        MOIHGP_HIP_FATAL(hipGetLastError());
        hipLaunchKernelGGL(bwd, grid, block, smem, io.stream, (const Tv*)io.Ty, T, io.ld, pt, L, (const double*)ckpt, (const int*)badw, (Tv*)io.yhat, (Tv*)var,
                           io.ld_out, (Tv*)io.x, P_end, nll, status);
        MOIHGP_HIP_FATAL(hipGetLastError());
    });
    return rc;
}

}  // namespace moihgp
