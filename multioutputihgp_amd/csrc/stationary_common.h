// stationary_common.h -- small dense helpers shared by stationary.hip, stationary_x.hip and the tables kernels of smoother.hip, forecast.hip and
// sampler.hip (one lane per latent, fp64): matrix products, chunk powers and growth figures, the LU and Stein solves, Eigen-style Pade matrix
// exponential, and the literal fixed-point solvers of the reference's utils/dare.h.
// Include AFTER `#pragma clang fp contract(off)`: the iteration counts of DARE/DLyap must agree with a plain-C evaluation.
#pragma once
#include "common.h"

namespace moihgp {
namespace {

template <int N>
__device__ inline void mm(const double* A, const double* B, double* C) {
    double T[N * N];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            double s = 0.0;
            for (int k = 0; k < N; k++) s += A[i * N + k] * B[k * N + j];
            T[i * N + j] = s;
        }
    for (int i = 0; i < N * N; i++) C[i] = T[i];
}
template <int N>
__device__ inline void mt(const double* A, double* At) {
    double T[N * N];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) T[j * N + i] = A[i * N + j];
    for (int i = 0; i < N * N; i++) At[i] = T[i];
}
template <int N>
__device__ inline void mv(const double* A, const double* x, double* y) {
    double T[N];
    for (int i = 0; i < N; i++) {
        double s = 0.0;
        for (int k = 0; k < N; k++) s += A[i * N + k] * x[k];
        T[i] = s;
    }
    for (int i = 0; i < N; i++) y[i] = T[i];
}
template <int N>
__device__ inline double norm_inf(const double* X) {
    double m = 0.0;
    for (int i = 0; i < N; i++) {
        double s = 0.0;
        for (int j = 0; j < N; j++) s += fabs(X[i * N + j]);
        m = fmax(m, s);
    }
    return m;
}
// Xc <- X^C and Xp <- X^(2C) by repeated multiplication from the left; returns the largest inf-norm of X^1 .. X^(2C) (fmax drops a NaN
// operand: a caller that must notice one tests the powers)
template <int N, int C>
__device__ inline double chunk_powers(const double* X, double* Xc, double* Xp) {
    double growth = 0.0;
    for (int i = 0; i < N * N; i++) Xp[i] = X[i];
#pragma nounroll
    for (int p = 1;; p++) {
        if (p == C) for (int i = 0; i < N * N; i++) Xc[i] = Xp[i];
        growth = fmax(growth, norm_inf<N>(Xp));
        if (p == 2 * C) return growth;
        mm<N>(X, Xp, Xp);
    }
}
// The growth figure of a whole segment of SEG ticks walked in chunks of C: Xc <- X^C, Xs <- X^SEG (SEG = 2C times a power of two); returns the
// largest inf-norm of X^1 .. X^(2C) and of X^SEG (NaN operands drop out as in chunk_powers: the caller tests Xc and Xs)
template <int N, int C, int SEG>
__device__ inline double segment_growth(const double* X, double* Xc, double* Xs) {
    const double growth = chunk_powers<N, C>(X, Xc, Xs);
    for (int p = 2 * C; p < SEG; p *= 2) mm<N>(Xs, Xs, Xs);
    return fmax(growth, norm_inf<N>(Xs));
}
template <int N>
__device__ inline bool all_zero(const double* A) {
    for (int i = 0; i < N * N; i++)
        if (A[i] != 0.0) return false;
    return true;
}

template <int D>
struct SS {
    double F[D * D], Pinf[D * D], H[D], R;
    double dF[3][D * D], dPinf[3][D * D], dR[3];
};

// matern32ss.h:40-64 (D == 2) and matern52ss.h:38-75 (D == 3), including `lam = sqrt(3)/l` there.
template <int D>
__device__ void ss_build(int kernel, const double* params, SS<D>& s) {
    for (int i = 0; i < D * D; i++) {
        s.F[i] = 0.0; s.Pinf[i] = 0.0;
        for (int p = 0; p < 3; p++) { s.dF[p][i] = 0.0; s.dPinf[p][i] = 0.0; }
    }
    for (int i = 0; i < D; i++) s.H[i] = 0.0;
    s.H[0] = 1.0;
    double magnitude = params[0], lengthscale = params[1];
    s.R = params[2];
    s.dR[0] = 0.0; s.dR[1] = 0.0; s.dR[2] = 1.0;
    if constexpr (D == 2) {
        double lam = sqrt(3.0) / lengthscale, lam2 = lam * lam;
        double len3 = 6.0 / (lengthscale * lengthscale * lengthscale);
        s.F[1] = 1.0;
        s.F[2] = -lam2;
        s.F[3] = -2.0 * lam;
        s.Pinf[0] = magnitude;
        s.Pinf[3] = magnitude * lam2;
        s.dF[1][2] = len3;
        s.dF[1][3] = 2.0 * lam / lengthscale;
        s.dPinf[0][0] = 1.0;
        s.dPinf[0][3] = lam2;
        s.dPinf[1][3] = -magnitude * len3;
    } else {
        double lam = sqrt(3.0) / lengthscale;
        double lam2 = lam * lam, len2 = lengthscale * lengthscale, len3 = len2 * lengthscale, len4 = len2 * len2;
        double kappa = 5.0 / 3.0 * magnitude / len2, kappa2 = -2.0 * kappa / lengthscale, sq5 = sqrt(5.0);
        s.F[1] = 1.0; s.F[5] = 1.0;
        s.F[6] = -lam2 * lam; s.F[7] = -3.0 * lam2; s.F[8] = -3.0 * lam;
        s.Pinf[0] = magnitude; s.Pinf[8] = 25.0 * magnitude / len4; s.Pinf[4] = kappa;
        s.Pinf[6] = -kappa; s.Pinf[2] = -kappa;
        s.dF[1][6] = 15.0 * sq5 / len4; s.dF[1][7] = 30.0 / len3; s.dF[1][8] = sq5 * lam2;
        for (int i = 0; i < 9; i++) s.dPinf[0][i] = s.Pinf[i] / magnitude;
        s.dPinf[1][4] = kappa2; s.dPinf[1][6] = -kappa2; s.dPinf[1][2] = -kappa2;
        s.dPinf[1][8] = -100.0 * magnitude / len2 / len3;
    }
    (void)kernel;
}

// X = Den^-1 Num, partial pivoting (Eigen partialPivLu().solve)
template <int N>
__device__ void lu_solve(const double* Ain, const double* Bin, double* X) {
    double A[N * N], B[N * N];
    for (int i = 0; i < N * N; i++) { A[i] = Ain[i]; B[i] = Bin[i]; }
    for (int k = 0; k < N; k++) {
        int p = k;
        double best = fabs(A[k * N + k]);
        for (int i = k + 1; i < N; i++)
            if (fabs(A[i * N + k]) > best) { best = fabs(A[i * N + k]); p = i; }
        if (p != k)
            for (int j = 0; j < N; j++) {
                double t = A[k * N + j]; A[k * N + j] = A[p * N + j]; A[p * N + j] = t;
                t = B[k * N + j]; B[k * N + j] = B[p * N + j]; B[p * N + j] = t;
            }
        for (int i = k + 1; i < N; i++) {
            double f = A[i * N + k] / A[k * N + k];
            for (int j = k; j < N; j++) A[i * N + j] -= f * A[k * N + j];
            for (int j = 0; j < N; j++) B[i * N + j] -= f * B[k * N + j];
        }
    }
    for (int j = 0; j < N; j++)
        for (int i = N - 1; i >= 0; i--) {
            double s = B[i * N + j];
            for (int k = i + 1; k < N; k++) s -= A[i * N + k] * X[k * N + j];
            X[i * N + j] = s / A[i * N + i];
        }
}

template <int D>
__device__ double max_abs(const double* X) {
    double m = 0.0;
    for (int i = 0; i < D * D; i++) m = fmax(m, fabs(X[i]));
    return m;
}
// S = sym(X) with (I - Ac (x) Ac) vec(X) = vec(RHS), row-major vec: the solution of the Stein equation X = Ac X Ac^T + RHS (exact d^2 x d^2 solve).
// (forceinline: inlined after it was optimised on its own, it costs smoother_tables_kernel<2> a wave per SIMD)
template <int D>
__device__ __forceinline__ void stein_solve(const double* Ac, const double* RHS, double* S) {
    constexpr int NN = D * D, N2 = NN * NN;
    double M[N2], rhs[N2], sol[N2];
    for (int i = 0; i < N2; i++) { M[i] = 0.0; rhs[i] = 0.0; }
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) {
            const int row = i * D + j;
            rhs[row * NN] = RHS[row];
            for (int k = 0; k < D; k++)
                for (int m = 0; m < D; m++) M[row * NN + k * D + m] = (row == k * D + m ? 1.0 : 0.0) - Ac[i * D + k] * Ac[j * D + m];
        }
    lu_solve<NN>(M, rhs, sol);
    for (int i = 0; i < D; i++)
        for (int j = 0; j < D; j++) S[i * D + j] = (sol[(i * D + j) * NN] + sol[(j * D + i) * NN]) / 2.0;
}

// E = exp(Ain): Pade approximant of degree 3/5/7/9/13 by 1-norm, scaling & squaring for the last.
template <int N>
__device__ void expm(const double* Ain, double* E) {
    constexpr int NN = N * N;
    double A[NN], A2[NN], A4[NN], A6[NN], U[NN], V[NN], T[NN];
    double l1 = 0.0;
    for (int j = 0; j < N; j++) {
        double s = 0.0;
        for (int i = 0; i < N; i++) s += fabs(Ain[i * N + j]);
        if (s > l1) l1 = s;
    }
    for (int i = 0; i < NN; i++) A[i] = Ain[i];
    int squarings = 0;
    if (l1 < 1.495585217958292e-002) {
        const double b[] = {120., 60., 12., 1.};
        mm<N>(A, A, A2);
        for (int i = 0; i < NN; i++) T[i] = b[3] * A2[i];
        for (int i = 0; i < N; i++) T[i * N + i] += b[1];
        mm<N>(A, T, U);
        for (int i = 0; i < NN; i++) V[i] = b[2] * A2[i];
        for (int i = 0; i < N; i++) V[i * N + i] += b[0];
    } else if (l1 < 2.539398330063230e-001) {
        const double b[] = {30240., 15120., 3360., 420., 30., 1.};
        mm<N>(A, A, A2); mm<N>(A2, A2, A4);
        for (int i = 0; i < NN; i++) T[i] = b[5] * A4[i] + b[3] * A2[i];
        for (int i = 0; i < N; i++) T[i * N + i] += b[1];
        mm<N>(A, T, U);
        for (int i = 0; i < NN; i++) V[i] = b[4] * A4[i] + b[2] * A2[i];
        for (int i = 0; i < N; i++) V[i * N + i] += b[0];
    } else if (l1 < 9.504178996162932e-001) {
        const double b[] = {17297280., 8648640., 1995840., 277200., 25200., 1512., 56., 1.};
        mm<N>(A, A, A2); mm<N>(A2, A2, A4); mm<N>(A4, A2, A6);
        for (int i = 0; i < NN; i++) T[i] = b[7] * A6[i] + b[5] * A4[i] + b[3] * A2[i];
        for (int i = 0; i < N; i++) T[i * N + i] += b[1];
        mm<N>(A, T, U);
        for (int i = 0; i < NN; i++) V[i] = b[6] * A6[i] + b[4] * A4[i] + b[2] * A2[i];
        for (int i = 0; i < N; i++) V[i * N + i] += b[0];
    } else if (l1 < 2.097847961257068e+000) {
        const double b[] = {17643225600., 8821612800., 2075673600., 302702400., 30270240., 2162160., 110880., 3960., 90., 1.};
        double A8[NN];
        mm<N>(A, A, A2); mm<N>(A2, A2, A4); mm<N>(A4, A2, A6); mm<N>(A6, A2, A8);
        for (int i = 0; i < NN; i++) T[i] = b[9] * A8[i] + b[7] * A6[i] + b[5] * A4[i] + b[3] * A2[i];
        for (int i = 0; i < N; i++) T[i * N + i] += b[1];
        mm<N>(A, T, U);
        for (int i = 0; i < NN; i++) V[i] = b[8] * A8[i] + b[6] * A6[i] + b[4] * A4[i] + b[2] * A2[i];
        for (int i = 0; i < N; i++) V[i * N + i] += b[0];
    } else {
        const double b[] = {64764752532480000., 32382376266240000., 7771770303897600., 1187353796428800.,
                            129060195264000., 10559470521600., 670442572800., 33522128640., 1323241920.,
                            40840800., 960960., 16380., 182., 1.};
        const double maxnorm = 5.371920351148152;
        frexp(l1 / maxnorm, &squarings);
        if (squarings < 0) squarings = 0;
        double sc = ldexp(1.0, -squarings);
        for (int i = 0; i < NN; i++) A[i] *= sc;
        mm<N>(A, A, A2); mm<N>(A2, A2, A4); mm<N>(A4, A2, A6);
        for (int i = 0; i < NN; i++) V[i] = b[13] * A6[i] + b[11] * A4[i] + b[9] * A2[i];
        mm<N>(A6, V, T);
        for (int i = 0; i < NN; i++) T[i] += b[7] * A6[i] + b[5] * A4[i] + b[3] * A2[i];
        for (int i = 0; i < N; i++) T[i * N + i] += b[1];
        mm<N>(A, T, U);
        for (int i = 0; i < NN; i++) T[i] = b[12] * A6[i] + b[10] * A4[i] + b[8] * A2[i];
        mm<N>(A6, T, V);
        for (int i = 0; i < NN; i++) V[i] += b[6] * A6[i] + b[4] * A4[i] + b[2] * A2[i];
        for (int i = 0; i < N; i++) V[i * N + i] += b[0];
    }
    for (int i = 0; i < NN; i++) { double u = U[i], v = V[i]; A2[i] = u + v; A4[i] = -u + v; }
    lu_solve<N>(A4, A2, E);
    for (int s = 0; s < squarings; s++) mm<N>(E, E, E);
}

// exp of the block lower triangular matrix [[X, 0], [Y, X]] (2N x 2N), returned as its blocks [[EX, 0], [EY, EX]]: the matrix
// ihgp.h:163-167 exponentiates to get dA = EY.  Same algorithm as expm<2N> above (degree by the 1-norm of the whole matrix, the
// same Pade coefficients, scaling and squaring), carried out on the blocks: a product of two such matrices is three N x N
// products instead of eight, and the linear solve is two N x N solves.  Equal to the dense evaluation up to rounding (the dense
// LU may pivot across the blocks); a third of its instructions, which is what this straight-line code is bound by.
template <int N>
struct BltPair { double x[N * N], y[N * N]; };
template <int N>
__device__ inline void blt_mul(const BltPair<N>& a, const BltPair<N>& b, BltPair<N>& c) {
    double t1[N * N], t2[N * N], tx[N * N];
    mm<N>(a.x, b.x, tx);
    mm<N>(a.y, b.x, t1);
    mm<N>(a.x, b.y, t2);
    for (int i = 0; i < N * N; i++) { c.x[i] = tx[i]; c.y[i] = t1[i] + t2[i]; }
}
template <int N>
__device__ void expm_blt(const double* X, const double* Y, double* EX, double* EY) {
    constexpr int NN = N * N;
    BltPair<N> A, A2, A4, A6, U, V, T;
    double l1 = 0.0;
    for (int j = 0; j < N; j++) {                      // columns j < N carry both blocks: they bound the others
        double s = 0.0;
        for (int i = 0; i < N; i++) s += fabs(X[i * N + j]);
        for (int i = 0; i < N; i++) s += fabs(Y[i * N + j]);
        if (s > l1) l1 = s;
    }
    for (int i = 0; i < NN; i++) { A.x[i] = X[i]; A.y[i] = Y[i]; }
    int squarings = 0;
    // T = sum_k c_k P_k (+ d I), on both blocks
    auto comb = [&](BltPair<N>& out, double c3, const BltPair<N>* p3, double c2, const BltPair<N>* p2, double c1, const BltPair<N>* p1, double diag, bool accumulate) {
        for (int i = 0; i < NN; i++) {
            double vx = accumulate ? out.x[i] : 0.0, vy = accumulate ? out.y[i] : 0.0;
            if (p3) { vx += c3 * p3->x[i]; vy += c3 * p3->y[i]; }
            if (p2) { vx += c2 * p2->x[i]; vy += c2 * p2->y[i]; }
            if (p1) { vx += c1 * p1->x[i]; vy += c1 * p1->y[i]; }
            out.x[i] = vx; out.y[i] = vy;
        }
        for (int i = 0; i < N; i++) out.x[i * N + i] += diag;
    };
    if (l1 < 1.495585217958292e-002) {
        const double b[] = {120., 60., 12., 1.};
        blt_mul<N>(A, A, A2);
        comb(T, 0, nullptr, 0, nullptr, b[3], &A2, b[1], false);
        blt_mul<N>(A, T, U);
        comb(V, 0, nullptr, 0, nullptr, b[2], &A2, b[0], false);
    } else if (l1 < 2.539398330063230e-001) {
        const double b[] = {30240., 15120., 3360., 420., 30., 1.};
        blt_mul<N>(A, A, A2); blt_mul<N>(A2, A2, A4);
        comb(T, 0, nullptr, b[5], &A4, b[3], &A2, b[1], false);
        blt_mul<N>(A, T, U);
        comb(V, 0, nullptr, b[4], &A4, b[2], &A2, b[0], false);
    } else if (l1 < 9.504178996162932e-001) {
        const double b[] = {17297280., 8648640., 1995840., 277200., 25200., 1512., 56., 1.};
        blt_mul<N>(A, A, A2); blt_mul<N>(A2, A2, A4); blt_mul<N>(A4, A2, A6);
        comb(T, b[7], &A6, b[5], &A4, b[3], &A2, b[1], false);
        blt_mul<N>(A, T, U);
        comb(V, b[6], &A6, b[4], &A4, b[2], &A2, b[0], false);
    } else if (l1 < 2.097847961257068e+000) {
        const double b[] = {17643225600., 8821612800., 2075673600., 302702400., 30270240., 2162160., 110880., 3960., 90., 1.};
        BltPair<N> A8;
        blt_mul<N>(A, A, A2); blt_mul<N>(A2, A2, A4); blt_mul<N>(A4, A2, A6); blt_mul<N>(A6, A2, A8);
        comb(T, b[7], &A6, b[5], &A4, b[3], &A2, 0.0, false);
        comb(T, 0, nullptr, 0, nullptr, b[9], &A8, b[1], true);
        blt_mul<N>(A, T, U);
        comb(V, b[6], &A6, b[4], &A4, b[2], &A2, 0.0, false);
        comb(V, 0, nullptr, 0, nullptr, b[8], &A8, b[0], true);
    } else {
        const double b[] = {64764752532480000., 32382376266240000., 7771770303897600., 1187353796428800.,
                            129060195264000., 10559470521600., 670442572800., 33522128640., 1323241920.,
                            40840800., 960960., 16380., 182., 1.};
        const double maxnorm = 5.371920351148152;
        frexp(l1 / maxnorm, &squarings);
        if (squarings < 0) squarings = 0;
        double sc = ldexp(1.0, -squarings);
        for (int i = 0; i < NN; i++) { A.x[i] *= sc; A.y[i] *= sc; }
        blt_mul<N>(A, A, A2); blt_mul<N>(A2, A2, A4); blt_mul<N>(A4, A2, A6);
        comb(V, b[13], &A6, b[11], &A4, b[9], &A2, 0.0, false);
        blt_mul<N>(A6, V, T);
        comb(T, b[7], &A6, b[5], &A4, b[3], &A2, b[1], true);
        blt_mul<N>(A, T, U);
        comb(T, b[12], &A6, b[10], &A4, b[8], &A2, 0.0, false);
        blt_mul<N>(A6, T, V);
        comb(V, b[6], &A6, b[4], &A4, b[2], &A2, b[0], true);
    }
    // (V - U) R = V + U on the blocks: P Rx = Nx ; P Ry = Ny - S Rx, with P, S the blocks of V - U
    double Px[NN], Sy[NN], Nx[NN], Ny[NN], Rx[NN], Ry[NN], t[NN];
    for (int i = 0; i < NN; i++) { Px[i] = -U.x[i] + V.x[i]; Sy[i] = -U.y[i] + V.y[i]; Nx[i] = U.x[i] + V.x[i]; Ny[i] = U.y[i] + V.y[i]; }
    lu_solve<N>(Px, Nx, Rx);
    mm<N>(Sy, Rx, t);
    for (int i = 0; i < NN; i++) Ny[i] -= t[i];
    lu_solve<N>(Px, Ny, Ry);
    BltPair<N> E;
    for (int i = 0; i < NN; i++) { E.x[i] = Rx[i]; E.y[i] = Ry[i]; }
    for (int s = 0; s < squarings; s++) blt_mul<N>(E, E, E);
    for (int i = 0; i < NN; i++) { EX[i] = E.x[i]; EY[i] = E.y[i]; }
}

constexpr double kDareTol = 1e-8;   // utils/dare.h:7
constexpr int kDareMaxIter = 100;   // utils/dare.h:8

// utils/dare.h:10-33, Bd = H^T
template <int D>
__device__ int dare(const double* Ad, const double* Bd, const double* Q, double R, double* P) {
    double AdT[D * D], Pn[D * D], T1[D * D], PB[D], APB[D], BtP[D], BPA[D];
    mt<D>(Ad, AdT);
    for (int i = 0; i < D * D; i++) P[i] = Q[i];
    for (int it = 0; it < kDareMaxIter; it++) {
        mm<D>(AdT, P, T1); mm<D>(T1, Ad, Pn);
        mv<D>(P, Bd, PB);
        double g = R;
        for (int i = 0; i < D; i++) g += Bd[i] * PB[i];
        mv<D>(AdT, PB, APB);
        for (int j = 0; j < D; j++) { double s = 0.0; for (int i = 0; i < D; i++) s += Bd[i] * P[i * D + j]; BtP[j] = s; }
        for (int j = 0; j < D; j++) { double s = 0.0; for (int k = 0; k < D; k++) s += BtP[k] * Ad[k * D + j]; BPA[j] = s; }
        double ginv = 1.0 / g;
        double diff = -INFINITY;
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) {
                double v = Pn[i * D + j] - APB[i] * ginv * BPA[j] + Q[i * D + j];   // dare.h:23
                Pn[i * D + j] = v;
                double dlt = v - P[i * D + j];
                if (dlt > diff) diff = dlt;                                       // maxCoeff, dare.h:25
            }
        diff = fabs(diff);
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) P[i * D + j] = (Pn[i * D + j] + Pn[j * D + i]) / 2.0;   // dare.h:26
        if (diff < kDareTol) return it + 1;
    }
    return kDareMaxIter;
}

// utils/dare.h:36-58 (literal `AdT P Ad - P + Q`)
template <int D>
__device__ int dlyap(const double* Ad, const double* Q, double* P) {
    double AdT[D * D], Pn[D * D], T1[D * D];
    mt<D>(Ad, AdT);
    for (int i = 0; i < D * D; i++) P[i] = Q[i];
    for (int it = 0; it < kDareMaxIter; it++) {
        mm<D>(AdT, P, T1); mm<D>(T1, Ad, Pn);
        double diff = -INFINITY;
        for (int i = 0; i < D * D; i++) {
            double v = Pn[i] - P[i] + Q[i];
            Pn[i] = v;
            double dlt = v - P[i];
            if (dlt > diff) diff = dlt;
        }
        diff = fabs(diff);
        for (int i = 0; i < D; i++)
            for (int j = 0; j < D; j++) P[i * D + j] = (Pn[i * D + j] + Pn[j * D + i]) / 2.0;
        if (diff < kDareTol) return it + 1;
    }
    return kDareMaxIter;
}

}  // namespace
}  // namespace moihgp
