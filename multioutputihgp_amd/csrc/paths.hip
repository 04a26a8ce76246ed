// paths.hip -- seeded forecast paths: joint draws of the ticks beyond the end of a stream (include/moihgp.h moihgp_forecast_paths).
//
// Per latent the innovations form of the steady-state one-step predictor, with the handle's A and the smoother's K, P (SM<D>) and the noise
// parameter R of the constant block: Sv = P_00 + R, and per sample, from the start state u[-1], with q = step0 + j and n[q] the normals of
// sample_normals4 (tag 2):
//   e = sqrt(Sv) n[q];   u[j] = A u[j-1] + K e;   paths[s][l][j] = u[j]_0 + (1 - K_0) e
// (the state-form x <- A x + chol(Q) n does not exist here: Q is indefinite for Matern-5/2).
//
// Kernels
//   paths_kernel         one lane per (sample, latent) row, rows sample-major, tick by tick: a horizon is short next to a stream and the
//                        parallelism is in the S L rows, so there is no scan, no growth bound and no second route.  One Philox block gives the
//                        normals of four consecutive steps.  The planes are [S][L][ld_out]: a lane's ticks are contiguous, its neighbours' are
//                        ld_out apart, so every wavefront keeps 64 rows x kPathBlock ticks in LDS (the stream's type; row pitch kPathBlock + 1,
//                        so the lanes' column writes fall on different banks) and writes the tile out row by row with 16-byte stores; the ragged
//                        last block stores scalars.  NaN rows and states of failed latents go through the same tile; every status word is
//                        written by the rows of sample 0.
//   paths_noise_kernel   the generator alone (moihgp_forecast_paths_noise), through the same sample_normals4.
// Arithmetic is fp64 for both stream types, every product and sum an explicit fma in a fixed order: a walk continued from its fp64 end state
// repeats the single walk bit for bit.  The value is rounded once, at the store into the tile.
#include "scan_sweep.h"
#include "philox_normals.h"

namespace moihgp {
namespace {

constexpr int kPathBlock = 32;                  // ticks per tile
constexpr int kPathPitch = kPathBlock + 1;      // row pitch of the tile, in scalars
constexpr size_t kNoRow = ~(size_t)0;

template <typename Tv, int D>
__global__ void __launch_bounds__(64) paths_kernel(const double* __restrict__ sm, const double* __restrict__ cb64, size_t L, size_t nrows,
                                                   const Tv* __restrict__ x, const double* states_in, double* states_out, size_t n, size_t step0,
                                                   unsigned long long seed, uint32_t sample0, uint32_t latent0, Tv* __restrict__ paths,
                                                   size_t ld_out, size_t plane_stride, int* __restrict__ status) {
    using B = SM<D>;
    using CBD = CB<D>;
    using Vec = typename VecOf<Tv>::type;
    constexpr int NN = D * D;
    constexpr int V = 16 / (int)sizeof(Tv);     // scalars per 16-byte store
    constexpr int LPR = kPathBlock / V;         // lanes per row of the tile
    constexpr int RPP = 64 / LPR;               // rows per pass
    __shared__ Tv tile[64 * kPathPitch];
    __shared__ size_t rowoff[64];               // where each row of the tile starts in the planes (kNoRow past the last row)
    const int lane = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * 64 + lane;
    const bool active = row < nrows;
    const size_t s = active ? row / L : 0, l = active ? row % L : 0;
    rowoff[lane] = active ? s * plane_stride + l * ld_out : kNoRow;
    const double* tb = sm + l * B::SIZE;
    const bool failed = tb[B::STATUS] != 0.0;
    if (active && status && s == 0) status[l] = failed ? 1 : 0;
    double A[NN], K[D], u[D];
#pragma unroll
    for (int i = 0; i < NN; i++) A[i] = tb[B::A + i];
#pragma unroll
    for (int i = 0; i < D; i++) K[i] = tb[B::K + i];
    const double sv = sqrt(tb[B::P] + cb64[l * CBD::SIZE + CBD::PARAMS + 2]), omk = 1.0 - K[0];
#pragma unroll
    for (int i = 0; i < D; i++) u[i] = !active ? 0.0 : (states_in ? states_in[row * D + i] : (double)x[l * D + i]);
    const uint32_t lat = latent0 + (uint32_t)l, smp = sample0 + (uint32_t)s;
    const Tv nan = (Tv)__builtin_nan("");
    Tv* mine = tile + lane * kPathPitch;
    float nz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    __syncthreads();
    for (size_t j0 = 0; j0 < n; j0 += kPathBlock) {
        const int nb = n - j0 < (size_t)kPathBlock ? (int)(n - j0) : kPathBlock;
        if (active) {
            for (int jj = 0; jj < nb; jj++) {
                const size_t q = step0 + j0 + jj;
                const int k = (int)(q & 3);
                if (k == 0 || (j0 == 0 && jj == 0)) sample_normals4(seed, (uint32_t)(q >> 2), lat, smp, 2u, nz);
                const double e = sv * (double)(k == 0 ? nz[0] : k == 1 ? nz[1] : k == 2 ? nz[2] : nz[3]);
                tick_step<double, D>(A, K, e, u);
                mine[jj] = failed ? nan : (Tv)fma(omk, e, u[0]);
            }
        }
        __syncthreads();
        if (nb == kPathBlock) {
            // rows of 128 (fp32) or 256 (fp64) contiguous bytes, one 16-byte store per lane: ld_out and plane_stride are multiples of 16 bytes
            // and j0 one of kPathBlock, so every run is aligned
#pragma unroll
            for (int p = 0; p < 64 / RPP; p++) {
                const int r = p * RPP + lane / LPR, c = (lane % LPR) * V;
                const size_t off = rowoff[r];
                if (off != kNoRow) {
                    Tv v[V];
#pragma unroll
                    for (int i = 0; i < V; i++) v[i] = tile[r * kPathPitch + c + i];
                    *reinterpret_cast<Vec*>(paths + off + j0 + c) = pack<Tv>(v);
                }
            }
        } else {
            for (int p = 0; p < 64 / RPP; p++) {
                const int r = p * RPP + lane / LPR, c = (lane % LPR) * V;
                const size_t off = rowoff[r];
                if (off != kNoRow)
                    for (int i = 0; i < V; i++)
                        if (c + i < nb) paths[off + j0 + c + i] = tile[r * kPathPitch + c + i];
            }
        }
        __syncthreads();
    }
    if (active && states_out)
#pragma unroll
        for (int i = 0; i < D; i++) states_out[row * D + i] = failed ? __builtin_nan("") : u[i];
}

// noise [S][L][ld]: n[step0 + j] of (latent0 + l, sample0 + s) at [s][l][j], j < n.  One lane per Philox block of four steps.
__global__ void __launch_bounds__(256) paths_noise_kernel(unsigned long long seed, uint32_t latent0, size_t L, uint32_t sample0, size_t S, size_t step0,
                                                          size_t n, float* __restrict__ noise, size_t ld) {
    const size_t q0 = step0 >> 2, nq = ((step0 + n + 3) >> 2) - q0;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S * L * nq) return;
    const size_t q = q0 + idx % nq, row = idx / nq, l = row % L, s = row / L;
    float nz[4];
    sample_normals4(seed, (uint32_t)q, latent0 + (uint32_t)l, sample0 + (uint32_t)s, 2u, nz);
    for (int i = 0; i < 4; i++) {
        const size_t step = 4 * q + i;
        if (step >= step0 && step < step0 + n) noise[row * ld + (step - step0)] = nz[i];
    }
}

}  // namespace

// x [L][d] (dtype) or states_in [S][L][d]: exactly one of them; paths.K planes of L rows.  The caller has validated every size.
void launch_forecast_paths(int d, int dtype, const double* sm, const double* cb64, size_t L, const void* x, const double* states_in, double* states_out,
                           size_t n, size_t step0, unsigned long long seed, unsigned sample0, unsigned latent0, const SweepPlanes& paths, size_t ld_out,
                           int* status, hipStream_t stream) {
    const size_t nrows = L * (size_t)paths.K;
    if (nrows == 0) return;
    dispatch_stream(d, dtype, [&](auto tv, auto dim) {
        using Tv = decltype(tv);
        hipLaunchKernelGGL((paths_kernel<Tv, decltype(dim)::value>), dim3((unsigned)((nrows + 63) / 64)), dim3(64), 0, stream, sm, cb64, L, nrows,
                           (const Tv*)x, states_in, states_out, n, step0, seed, sample0, latent0, (Tv*)paths.base, ld_out, paths.stride, status);
    });
    MOIHGP_HIP_FATAL(hipGetLastError());
}

void launch_forecast_paths_noise(unsigned long long seed, unsigned latent0, size_t L, unsigned sample0, size_t S, size_t step0, size_t n, float* noise,
                                 size_t ld, hipStream_t stream) {
    if (n == 0 || S * L == 0) return;
    const size_t cnt = S * L * (((step0 + n + 3) >> 2) - (step0 >> 2));
    hipLaunchKernelGGL(paths_noise_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, seed, latent0, L, sample0, S, step0, n, noise, ld);
    MOIHGP_HIP_FATAL(hipGetLastError());
}

}  // namespace moihgp
