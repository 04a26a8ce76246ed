// scan_sweep.h -- device machinery of the chunk-scan sweeps over whole streams (smoother.hip: smooth_fwd_kernel, smooth_bwd_kernel;
// forecast.hip: forecast_sweep_kernel; sampler.hip: sample_sweep_kernel; lagged.hip: lagged_bwd_kernel; interp.hip: interp_fwd_kernel, interp_bwd_kernel).  One wavefront per latent walks the stream in segments of
// 64 x kScanChunk ticks staged through LDS (coalesced in and out): each lane takes kScanChunk consecutive ticks, computes its chunk's affine map
// from a zero state, a Kogge-Stone scan of the maps over the 64 lanes gives every lane its true start state, and the lane replays its chunk from
// there.  Both directions live here: forward in time (chunk_map, lane 0 first) and backward (chunk_response_bwd, lane 63 first, a chunk walked
// from its last tick to its first); scan_maps and start_states take the direction as FWD.  What a sweep does in its replay stays in its kernel.
// Ta: the arithmetic (the smoother's and the sampler's double, the forecasts' stream scalar); D: the state dimension.
#pragma once
#include "kernels_common.h"
#include "stream_tables.h"

namespace moihgp {
namespace {

// ---- which kernel takes a latent ----------------------------------------------------------------------------------------------------------
// The scan is usable for a latent when its DARE converged and no power of its maps that the tables kernel looked at exceeds this in the
// inf-norm: the zero-state chunk responses and the composed maps then lose at most log10(bound) digits to cancellation.  fp64 arithmetic
// affords four; fp32 (7 digits, 3 needed) two.
template <typename Ta> __host__ __device__ constexpr double scan_growth_bound() { return sizeof(Ta) == 8 ? 1e4 : 1e2; }

// kFailed: the DARE did not converge (NaN row and end state, no sweep); kScan: the chunk-scan kernels' latent; kSerial: the tick-by-tick kernel's.
// path: -1 automatic (the growth bound decides), 0 scan, 1 serial.
enum class Route { kFailed, kScan, kSerial };
__device__ __forceinline__ Route latent_route(double status, double growth, double bound, int path) {
    if (status != 0.0) return Route::kFailed;
    if (path == 1 || (path == -1 && !(growth <= bound))) return Route::kSerial;
    return Route::kScan;
}

// NaN rows (K planes plane_stride apart, row: the latent's row of plane 0) and NaN end state of a failed latent, by the lanes first, first + step, ...
template <typename Tv, int D>
__device__ __forceinline__ void write_failed(Tv* row, size_t plane_stride, int K, size_t T, Tv* x_out, int first, int step) {
    const Tv nan = (Tv)__builtin_nan("");
    for (int k = 0; k < K; k++)
        for (size_t t = first; t < T; t += step) row[(size_t)k * plane_stride + t] = nan;
    for (int i = first; i < D; i += step) x_out[i] = nan;
}

// ---- small dense helpers --------------------------------------------------------------------------------------------------------------------
template <typename Ta, int D>
__device__ __forceinline__ void matvec(const Ta* M, const Ta* x, Ta* y) {
#pragma unroll
    for (int i = 0; i < D; i++) y[i] = 0;
    matvec_acc<Ta, D>(M, x, y);
}

// one tick x <- M x + K e (the backward sweeps and the serial kernels; the forward chunk maps and replays keep their loops)
template <typename Ta, int D>
__device__ __forceinline__ void tick_step(const Ta* M, const Ta* K, Ta e, Ta* x) {
    Ta xn[D];
    matvec<Ta, D>(M, x, xn);
#pragma unroll
    for (int j = 0; j < D; j++) x[j] = fma(K[j], e, xn[j]);
}

// ---- segment staging ------------------------------------------------------------------------------------------------------------------------
// Tick seg0 + tl of a segment (tl = k*64 + lane in a coalesced walk, k < kScanChunk) belongs to lane tl / kScanChunk's row of a staged plane
__device__ __forceinline__ int scan_slot(int tl) { return (tl / kScanChunk) * kScanPitch + tl % kScanChunk; }

// coalesced load of the segment at seg0 of a stream's row into a plane (zeros past the stream's end), and one plane back to a row of the stream
// (a plain lambda for the sweep's conversion costs the forecast's fp32 sweeps a wave per SIMD: the backward sweep, which stages y - p and p,
// keeps its own loop)
template <typename Tv, typename Ta>
__device__ __forceinline__ void stage_in(const Tv* row, size_t seg0, size_t T, int lane, Ta* plane) {
#pragma unroll
    for (int k = 0; k < kScanChunk; k++) {
        const int tl = k * 64 + lane;
        const size_t t = seg0 + tl;
        plane[scan_slot(tl)] = t < T ? (Ta)row[t] : (Ta)0;
    }
}
template <typename Tv, typename Ta>
__device__ __forceinline__ void stage_out(const Ta* plane, Tv* row, size_t seg0, size_t T, int lane) {
#pragma unroll
    for (int k = 0; k < kScanChunk; k++) {
        const int tl = k * 64 + lane;
        const size_t t = seg0 + tl;
        if (t < T) row[t] = (Tv)plane[scan_slot(tl)];
    }
}

// ticks of this lane's chunk that lie inside the stream
__device__ __forceinline__ int lane_tick_count(size_t seg0, size_t T, int lane) {
    const size_t t0 = seg0 + (size_t)lane * kScanChunk;
    return t0 >= T ? 0 : (int)((T - t0) < (size_t)kScanChunk ? (T - t0) : (size_t)kScanChunk);
}
// ... of this lane's chunk my[]; regular: a whole chunk without missing ticks
template <typename Ta>
__device__ __forceinline__ int lane_ticks(const Ta* my, size_t seg0, size_t T, int lane, bool& regular) {
    const int n = lane_tick_count(seg0, T, lane);
    regular = n == kScanChunk;
    for (int i = 0; i < n; i++) regular &= !isnan(my[i]);
    return n;
}

// ---- the chunk's map, the scan, the start states -----------------------------------------------------------------------------------------------
// The affine map (Phi, r) of the chunk y[0 .. n) from a zero state under x <- M x + K y (x <- A x where y is NaN; the ragged tail is the
// identity).  MF = M^kScanChunk is the map of a regular chunk; any other is its own product of tick maps.
template <typename Ta, int D>
__device__ __forceinline__ void chunk_map(const Ta* y, int n, bool regular, const Ta* A, const Ta* M, const Ta* MF, const Ta* K, Ta* Phi, Ta* r) {
    constexpr int NN = D * D;
#pragma unroll
    for (int i = 0; i < D; i++) r[i] = 0;
    if (regular) {
#pragma unroll
        for (int i = 0; i < NN; i++) Phi[i] = MF[i];
        for (int i = 0; i < kScanChunk; i++) {   // (tick_step's loop, kept here: through the helper the forecasts' fp32 sweeps come out rescheduled)
            Ta rn[D];
            matvec<Ta, D>(M, r, rn);
            const Ta yi = y[i];
#pragma unroll
            for (int j = 0; j < D; j++) r[j] = fma(K[j], yi, rn[j]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < NN; i++) Phi[i] = (i % (D + 1)) == 0 ? (Ta)1 : (Ta)0;
        for (int i = 0; i < n; i++) {
            const Ta yi = y[i];
            const bool miss = isnan(yi);
            const Ta* Mt = miss ? A : M;
            Ta rn[D], Pn[NN];
            matvec<Ta, D>(Mt, r, rn);
            matmul<Ta, D>(Mt, Phi, Pn);
#pragma unroll
            for (int j = 0; j < D; j++) r[j] = miss ? rn[j] : fma(K[j], yi, rn[j]);
#pragma unroll
            for (int j = 0; j < NN; j++) Phi[j] = Pn[j];
        }
    }
}

// Backward: the response r of the whole chunk e[0 .. kScanChunk) under s <- G s + K e[i], walked from its last tick to its first from a zero
// state at its end (the recursion is time-invariant, so the chunk's map is a power of G that the caller holds; entries past the stream's end
// are zero, come first and leave the state zero).  Te: the scalar the chunk is staged in (the fixed-lag sweep stages fp32 streams in fp32).
template <typename Ta, int D, typename Te = Ta>
__device__ __forceinline__ void chunk_response_bwd(const Te* e, const Ta* G, const Ta* K, Ta* r) {
#pragma unroll
    for (int i = 0; i < D; i++) r[i] = 0;
    for (int i = kScanChunk - 1; i >= 0; i--) tick_step<Ta, D>(G, K, (Ta)e[i], r);
}

// Inclusive Kogge-Stone scan of affine maps (Phi, r) over the wavefront.  FWD: lane j ends with the composition of lanes 0..j (lane 0 first);
// otherwise lanes j..63 with lane 63 first (a backward sweep walks time from the end).
template <typename Ta, int D, bool FWD>
__device__ __forceinline__ void scan_maps(Ta* Phi, Ta* r, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        Ta Po[D * D], ro[D];
#pragma unroll
        for (int i = 0; i < D * D; i++) Po[i] = FWD ? __shfl_up(Phi[i], off, 64) : __shfl_down(Phi[i], off, 64);
#pragma unroll
        for (int i = 0; i < D; i++) ro[i] = FWD ? __shfl_up(r[i], off, 64) : __shfl_down(r[i], off, 64);
        const bool has = FWD ? lane >= off : lane + off < 64;
        if (has) {
            Ta Pn[D * D], rn[D];
            matmul<Ta, D>(Phi, Po, Pn);
            matvec<Ta, D>(Phi, ro, rn);
#pragma unroll
            for (int i = 0; i < D * D; i++) Phi[i] = Pn[i];
#pragma unroll
            for (int i = 0; i < D; i++) r[i] += rn[i];
        }
    }
}

// The scanned map applied to the state xseg that enters the segment: xs <- the state that enters this lane's chunk (the end state of the lane
// before it in the sweep's direction, xseg for the first), xseg <- the state that leaves the segment.
template <typename Ta, int D, bool FWD>
__device__ __forceinline__ void start_states(const Ta* Phi, const Ta* r, Ta* xseg, Ta* xs, int lane) {
    Ta xe[D];
    matvec<Ta, D>(Phi, xseg, xe);
#pragma unroll
    for (int i = 0; i < D; i++) xe[i] += r[i];
#pragma unroll
    for (int i = 0; i < D; i++) {
        const Ta nb = FWD ? __shfl_up(xe[i], 1, 64) : __shfl_down(xe[i], 1, 64);
        xs[i] = lane == (FWD ? 0 : 63) ? xseg[i] : nb;
        xseg[i] = __shfl(xe[i], FWD ? 63 : 0, 64);
    }
}

}  // namespace
}  // namespace moihgp
