// stream_tables.h -- the per-latent table blocks of the whole-stream smoother (smoother.hip), its exact edges (edges.hip), the exact posterior (posterior.hip), forecasts (forecast.hip), fixed-lag smoother (lagged.hip), off-grid smoother (interp.hip) and sampler (sampler.hip), the
// chunk geometry their chunk powers are built for, and the (d, dtype) dispatch of their launchers.  Read by those files and by capi.cpp.
#pragma once
#include "common.h"
#include <type_traits>

namespace moihgp {

// chunk geometry of the chunk-scan sweeps (scan_sweep.h); MF / MB below are powers for exactly this chunk length
constexpr int kScanChunk = 16;                  // ticks per lane per segment
constexpr int kScanSeg = 64 * kScanChunk;       // ticks per segment (one wavefront)
constexpr int kScanPitch = kScanChunk + 1;      // LDS row pitch of one lane's chunk (odd: no bank conflicts between lanes)
constexpr int kScanPlane = 64 * kScanPitch;     // elements of one staged plane

// per-latent smoother block (fp64), offsets in doubles
template <int D>
struct SM {
    static constexpr int NN = D * D;
    static constexpr int A = 0, AKHA = A + NN, K = AKHA + NN, G = K + D;   // AKHA = A - K H A
    static constexpr int MF = G + NN;           // AKHA^kScanChunk
    static constexpr int MB = MF + NN;          // G^kScanChunk
    static constexpr int P = MB + NN, PF = P + NN, PS = PF + NN;
    static constexpr int VARF = PS + NN, VARS = VARF + 1, GROWTH = VARS + 1, RESID = GROWTH + 1, STATUS = RESID + 1;
    static constexpr int SIZE = (STATUS + 1 + 1) / 2 * 2;
};

// per-latent forecast block, offsets in scalars (the same in the fp64 and the fp32 copy)
template <int D>
struct FT {
    static constexpr int NN = D * D;
    static constexpr int A = 0, M = A + NN, K = M + NN, MF = K + D;   // MF = M^kScanChunk
    static constexpr int C = MF + NN;                                 // [kFcMaxHorizons][D]  c_k = H A^h_k (rows past the call's K are zero)
    static constexpr int VAR = C + kFcMaxHorizons * D;                // [kFcMaxHorizons]
    static constexpr int GROWTH = VAR + kFcMaxHorizons, STATUS = GROWTH + 1;
    static constexpr int SIZE = (STATUS + 1 + 3) / 4 * 4;
};

// per-latent fixed-lag block (fp64), offsets in doubles, next to the latent's SM<D> block (which holds G, G^kScanChunk, K and the growth figure)
template <int D>
struct LT {
    static constexpr int W = 0;                                       // [kLagMaxLags][D]  w_k = G^(l_k + 1) K (rows past the call's K are zero)
    static constexpr int VAR = W + kLagMaxLags * D;                   // [kLagMaxLags]
    static constexpr int STATUS = VAR + kLagMaxLags;
    static constexpr int SIZE = (STATUS + 1 + 1) / 2 * 2;
};

// per-latent off-grid block (fp64), offsets in doubles, next to the latent's SM<D> block: per offset phi_k the two rows of
// fine[k][t] = a_k . xf[t] + g_k . s[t+1] (interp.hip); slope.hip fills the same block with the rows of the rate of change
template <int D>
struct IT {
    static constexpr int AROW = 0;                                    // [kInterpMaxPoints][D]  a_k = H A_phi_k (rows past the call's K are zero)
    static constexpr int GROW = AROW + kInterpMaxPoints * D;          // [kInterpMaxPoints][D]  g_k = H G_phi_k
    static constexpr int VAR = GROW + kInterpMaxPoints * D;           // [kInterpMaxPoints]
    static constexpr int STATUS = VAR + kInterpMaxPoints;
    static constexpr int SIZE = (STATUS + 1 + 1) / 2 * 2;
};

// per-latent sampler block (fp64), offsets in doubles: the innovations realization of the smoother's steady-state autocovariance (sampler.hip),
// next to the latent's SM<D> block (which holds G, G^kScanChunk and Ps)
template <int D>
struct SP {
    static constexpr int NN = D * D;
    static constexpr int B = 0, LC = B + D, SG = LC + NN;       // B, Lc = chol(Sigma), Sigma
    static constexpr int SIGMA = SG + NN, SIGMA2 = SIGMA + 1;
    static constexpr int ERR = SIGMA2 + 1;                      // max_{k < 64} |r^[k] - r[k]| / r0, the acceptance figure
    static constexpr int GROWTH = ERR + 1;                      // max inf-norm of G^k, k <= 2 kScanChunk, and of G^kScanSeg
    static constexpr int STATUS = GROWTH + 1;                   // 0 ok, 1 the Kalman DARE failed, 2 the realization failed
    static constexpr int SIZE = (STATUS + 1 + 1) / 2 * 2;
};

// per-latent edge block (fp64), offsets in doubles, next to the latent's SM<D> block (which holds G, P, PF, Ps): what exact-edge smoothing (edges.hip)
// needs of the model beside it
constexpr int kEdgeCap = 1 << 20;               // HEAD and TAIL are capped here; the cap means "never reached"
constexpr int kEdgeScratchTicks = 4096;         // overlapping edges are walked in streams of at most this many ticks
template <int D>
struct ET {
    static constexpr int NN = D * D;
    static constexpr int E = 0;                                 // Pinf^-1 - P^-1
    static constexpr int PSROW = E + NN;                        // [D] e0^T Ps
    static constexpr int HEAD = PSROW + D, TAIL = HEAD + 1;     // the smallest n with |G^n|inf <= 2^-60, the smallest k with |G^k|inf^2 <= 2^-60 (as doubles)
    static constexpr int STATUS = TAIL + 1;                     // 0 ok, 1 the Kalman DARE failed, 4 Pinf or P could not be inverted / something is not finite
    static constexpr int SIZE = (STATUS + 1 + 1) / 2 * 2;
};

// per-latent model block (fp64), offsets in doubles: what the exact posterior (posterior.hip) walks with.  No DARE: the handle's A and the model's own
// Pinf and R, and Q = sym(Pinf - A Pinf A^T)
template <int D>
struct PT {
    static constexpr int NN = D * D;
    static constexpr int A = 0, Q = A + NN, PINF = Q + NN, R = PINF + NN;
    static constexpr int SIZE = (R + 1 + 1) / 2 * 2;
};
// The walk of posterior.hip: the forward kernel leaves a checkpoint (xf, PF) every kPostBlock ticks, the backward kernel recomputes a block from
// it; both move the rows through LDS in tiles of kPostTile ticks (a multiple of kPostBlock).  A checkpoint holds xf and the upper triangle of PF.
constexpr int kPostBlock = 16;
constexpr int kPostTile = 32;
constexpr int post_ckpt_doubles(int d) { return d + d * (d + 1) / 2; }
// doubles of scratch a call of T ticks and L latents needs: the checkpoints [ceil(T / kPostBlock)][post_ckpt_doubles(d)][L], then one word per
// latent (the forward walk's breakdown flag)
constexpr size_t post_scratch_doubles(int d, size_t T, size_t L) { return ((T + kPostBlock - 1) / kPostBlock * (size_t)post_ckpt_doubles(d) + 1) * L; }

constexpr int sm_size(int d) { return d == 2 ? SM<2>::SIZE : SM<3>::SIZE; }
constexpr int et_size(int d) { return d == 2 ? ET<2>::SIZE : ET<3>::SIZE; }
constexpr int pt_size(int d) { return d == 2 ? PT<2>::SIZE : PT<3>::SIZE; }
constexpr int fc_size(int d) { return d == 2 ? FT<2>::SIZE : FT<3>::SIZE; }
constexpr int sp_size(int d) { return d == 2 ? SP<2>::SIZE : SP<3>::SIZE; }
constexpr int lt_size(int d) { return d == 2 ? LT<2>::SIZE : LT<3>::SIZE; }
constexpr int it_size(int d) { return d == 2 ? IT<2>::SIZE : IT<3>::SIZE; }

// f(std::integral_constant<int, D>) for the state dimension d (2 or 3); f(Tv(), std::integral_constant<int, D>) for the stream's scalar too
template <typename F>
inline void dispatch_dim(int d, F&& f) {
    if (d == 2) f(std::integral_constant<int, 2>());
    else f(std::integral_constant<int, 3>());
}
template <typename F>
inline void dispatch_stream(int d, int dtype, F&& f) {
    dispatch_dim(d, [&](auto dim) {
        if (dtype == 0) f(double(), dim);
        else f(float(), dim);
    });
}

}  // namespace moihgp
