/* moihgp.h -- C ABI of libmoihgp.so (MI355X / gfx950 HIP implementation).
 *
 * Part 1 is the drop-in boundary: the exact 26 symbols the reference exports from
 * moihgp/src/wrapper.cpp and that moihgp/pywrapper.py binds through ctypes
 * (pywrapper.py:28-94).  Signatures, buffer layouts and ownership are the reference's:
 * every pointer is a caller-owned host buffer of C-contiguous doubles, valid for the
 * duration of the call only.
 *     x, xnew   [L][d]          (wrapper.cpp:63,84)
 *     dx, dxnew [L][P][d]       (wrapper.cpp:69,90)
 *     y, yhat   [M]
 *     params, grad [M*L + L + 1 + L*P] = U row-major | S | sigma | (magnitude, lengthscale, noise) x L
 *                               (moihgp.h:93, :431-457, :721-738)
 * All arithmetic behind these symbols runs in HIP kernels on the current device; there is no
 * CPU fallback.  If no usable GPU is present `*_new` returns NULL and moihgp_last_error()
 * says why.  A later HIP failure (a launch, copy or allocation that fails) inside one of the
 * reference entries prints the error and aborts -- they are all void / value returns, the
 * reference ABI has no status channel (wrapper.cpp:31-326).  The additive entries of part 2
 * that return int report it instead: rc 1 = invalid argument, 2 = HIP failure, 3 = unsupported
 * input (a window whose missing outputs exceed the limits of moihgp_project_stream), 4 = host memory; moihgp_last_error() holds
 * the text.  Nothing ever unwinds across the ABI.
 *
 * Part 2 is additive: batched entry points over whole time streams (the per-tick ABI costs one
 * FFI crossing + several launches per tick and cannot amortise them), taking DEVICE pointers.
 *
 * Citations `file:line` are into the reference tree /root/reference/moihgp/.
 */
#ifndef MOIHGP_C_API_H_
#define MOIHGP_C_API_H_

#include <stddef.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ Part 1: reference ABI */
/* Opaque handle; the reference returns `GP32*` / `GP52*` (src/wrapper.cpp:21-22).            */
typedef struct moihgp_gp moihgp_gp;

/* replaces src/wrapper.cpp:31-34  (MOIHGP ctor, include/moihgp/moihgp.h:81-136).  `threading` selects the
 * reference's per-call pthread fan-out (moihgp.h:184-214), which the GPU replaces -- but the flag is OBSERVABLE in
 * the reference and is honoured here: the gradient overload of negLogLikelihood adds the per-latent losses only
 * on its threaded branch (moihgp.h:590); the serial branch (:597-607) computes the per-latent gradients and drops
 * the losses.  So with threading == false (the default of pywrapper.py:12, online_learning.py:12, example.py:37;
 * forced for num_latent < 2 by moihgp.h:128-135) gpXX_lik1 returns 1/2 log(sum S) + 1/2 (M-L)+ log sigma +
 * 1/2 ||(I-UU^T)y|| / sigma alone, with threading == true the same plus sum_l 1/2 (v_l^2/S_l + log S_l) (= gpXX_lik2).
 * The gradient is the same in both.  MOIHGP_LIK1_FULL_LOSS=1 (read at construction) selects the summed form
 * regardless of the flag. */
moihgp_gp* gp32_new(double dt, size_t num_output, size_t num_latent, bool threading);
/* replaces src/wrapper.cpp:37-40 (which runs the destructor but leaks the object; we free it) */
void   gp32_del(moihgp_gp* gp);
/* replaces src/wrapper.cpp:43-94   -> MOIHGP::step overload 1, moihgp.h:148-226 */
void   gp32_step1(moihgp_gp* gp, double* x, double* y, double* dx, double* xnew, double* yhat, double* dxnew);
/* replaces src/wrapper.cpp:97-145  -> MOIHGP::step overload 2, moihgp.h:229-301 */
void   gp32_step2(moihgp_gp* gp, double* x, double* y, double* dx, double* xnew, double* dxnew);
/* replaces src/wrapper.cpp:148-184 -> MOIHGP::step overload 3, moihgp.h:304-378 */
void   gp32_step3(moihgp_gp* gp, double* x, double* y, double* xnew, double* yhat);
/* replaces src/wrapper.cpp:187-220 -> MOIHGP::step overload 4, moihgp.h:381-428 */
void   gp32_step4(moihgp_gp* gp, double* x, double* xnew, double* yhat);
/* replaces src/wrapper.cpp:223-228 -> MOIHGP::update, moihgp.h:431-457 (+ IHGP::update, ihgp.h:117-201) */
void   gp32_update(moihgp_gp* gp, double* params);
/* replaces src/wrapper.cpp:231-268 -> MOIHGP::negLogLikelihood(x,y,dx,grad), moihgp.h:460-611 */
double gp32_lik1(moihgp_gp* gp, double* x, double* y, double* dx, double* grad);
/* replaces src/wrapper.cpp:271-296 -> MOIHGP::negLogLikelihood(x,y), moihgp.h:614-688 */
double gp32_lik2(moihgp_gp* gp, double* x, double* y);
/* replaces src/wrapper.cpp:299-307 -> MOIHGP::getParams, moihgp.h:721-738 */
void   gp32_get_params(moihgp_gp* gp, double* params);
/* replace src/wrapper.cpp:310-325 */
size_t gp32_igp_dim(moihgp_gp* gp);
size_t gp32_num_param(moihgp_gp* gp);
size_t gp32_num_igp_param(moihgp_gp* gp);

/* replaces src/wrapper.cpp:329-624.  NOTE: in the reference `GP52` is a typedef of the
 * Matern-3/2 model (typo alias, wrapper.cpp:22), so gp52_* behave exactly like gp32_*.
 * That behaviour is kept by default.  Set the environment variable MOIHGP_GP52_MATERN52=1
 * (read at gp52_new) to get the real Matern-5/2 model of include/moihgp/matern52ss.h, or
 * use moihgp_new(MOIHGP_MATERN52, ...). */
moihgp_gp* gp52_new(double dt, size_t num_output, size_t num_latent, bool threading);
void   gp52_del(moihgp_gp* gp);
void   gp52_step1(moihgp_gp* gp, double* x, double* y, double* dx, double* xnew, double* yhat, double* dxnew);
void   gp52_step2(moihgp_gp* gp, double* x, double* y, double* dx, double* xnew, double* dxnew);
void   gp52_step3(moihgp_gp* gp, double* x, double* y, double* xnew, double* yhat);
void   gp52_step4(moihgp_gp* gp, double* x, double* xnew, double* yhat);
void   gp52_update(moihgp_gp* gp, double* params);
double gp52_lik1(moihgp_gp* gp, double* x, double* y, double* dx, double* grad);
double gp52_lik2(moihgp_gp* gp, double* x, double* y);
void   gp52_get_params(moihgp_gp* gp, double* params);
size_t gp52_igp_dim(moihgp_gp* gp);
size_t gp52_num_param(moihgp_gp* gp);
size_t gp52_num_igp_param(moihgp_gp* gp);

/* ------------------------------------------------------------------ Part 2: additive ABI */
enum { MOIHGP_MATERN32 = 0, MOIHGP_MATERN52 = 1 };
enum { MOIHGP_F64 = 0, MOIHGP_F32 = 1 };
/* Stacked state: the sum of J Matern components observed through one output (state dim J*2 or J*3 up to 12; BASELINE.json's
 * d = 6 / d = 12 shapes).  The reference ships no such model; it is what its IHGP<StateSpace> template (ihgp.h:17-35)
 * computes for a StateSpace with F, Pinf block-diagonal in the reference's component models and H = [H_1 .. H_J].
 * J in {2, 3, 4}.  Hyper-parameters per latent: [magnitude_1, lengthscale_1, .., magnitude_J, lengthscale_J, noise]
 * (P = 2J + 1).  Accepted everywhere a kernel id is: latent banks (moihgp_new_latents / moihgp_update_latents /
 * moihgp_filter_stream / moihgp_grad_stream / moihgp_get_latent) and full objects (moihgp_new: OILMM mixing, the gpXX_* per-tick
 * entries on the handle, moihgp_project_stream / moihgp_unproject_stream, the window objective), with params / grad laid out as
 * [U row-major | S | sigma | P values per latent] (moihgp.h:93 with num_igp_param = 2J + 1).  The sensitivities of IHGP::update
 * (ihgp.h:136-200) are computed from the first call that needs them on. */
#define MOIHGP_STACK(base, J) ((base) | ((J) << 4))

/* Thread-local message of the last failure ("" if none). */
const char* moihgp_last_error(void);
/* Number of usable HIP devices (0 if none / runtime missing). */
int         moihgp_device_count(void);
/* Library/ABI version: major*10000 + minor*100 + patch. */
int         moihgp_version(void);

/* Same object as gp32_new/gp52_new with an explicit kernel (the StateSpace template argument of
 * moihgp::MOIHGP<SS>, include/moihgp/moihgp.h:76).  Returns NULL on failure. */
moihgp_gp*  moihgp_new(int kernel, double dt, size_t num_output, size_t num_latent);
void        moihgp_del(moihgp_gp* gp);
size_t      moihgp_num_output(moihgp_gp* gp);
size_t      moihgp_num_latent(moihgp_gp* gp);
/* The `threading` constructor argument of moihgp.h:81 for objects made by moihgp_new (which start with it off), with the
 * override of moihgp.h:128-135 (num_latent < 2: always off).  It decides the value gpXX_lik1 / moihgp_window_eval return
 * (see gp32_new above). */
void        moihgp_set_threading(moihgp_gp* gp, int threading);
int         moihgp_get_threading(moihgp_gp* gp);
/* Newton-Schulz steps the last update() / construction took for the polar factor of the mixing (moihgp.h:433-447 computes it by SVD;
 * DESIGN.md 3.6): one symmetric Gram product and one M x L x L product each.  0 for small models (single-workgroup kernel). */
int         moihgp_polar_iterations(moihgp_gp* gp);

/* Deterministic counterpart of the ctor's random U (moihgp.h:103-125 uses std::random_device):
 * reseeds and redraws U = polar(I + N(0,1e-3)) from a fixed 64-bit seed. */
void        moihgp_reseed_U(moihgp_gp* gp, unsigned long long seed);

/* Latent-sharded construction: the object owns latents [l0, l0+nl) only and takes only
 * their (magnitude, lengthscale, noise) triples; no mixing matrix.  Used by one rank per GPU.
 * params_LP is a HOST array [nl][P], P = 3 (2J + 1 for a stacked kernel). */
moihgp_gp*  moihgp_new_latents(int kernel, double dt, size_t num_latent_local, const double* params_LP);
/* Re-run IHGP::update (ihgp.h:117-201) for every owned latent from HOST params [nl][P]. */
int         moihgp_update_latents(moihgp_gp* gp, const double* params_LP);

/* Set the mixing of a full object directly, WITHOUT the polar-factor step of update() (moihgp.h:433-447): U [M][L] row-major,
 * S [L], sigma, all HOST.  For latent shards of a bigger model: rank r builds an object with its L_r latents and hands it the
 * columns [lo_r, hi_r) of the global orthonormal factor, so that moihgp_project_stream / moihgp_unproject_stream compute this
 * rank's part of S^-1/2 U^T y and of U S^1/2 Ty (sharded.py).  Combine with moihgp_update_latents for the per-latent parameters. */
int         moihgp_set_mixing(moihgp_gp* gp, const double* U, const double* S, double sigma);

/* Copy the stationary matrices of latent l (ihgp.h:243-254) to HOST buffers (any may be NULL):
 * A[d*d] K[d] S[1] HA[d] AKHA[d*d] dA[P*d*d] dS[P] dK[P*d] dAKHA[P*d*d] HdA[P*d], row-major;
 * iters[1+P] = DARE iteration count followed by the P DLyap counts (utils/dare.h returns are ignored
 * by the reference; exposed here for diagnosis). */
int         moihgp_get_latent(moihgp_gp* gp, size_t l, double* A, double* K, double* S, double* HA, double* AKHA,
                              double* dA, double* dS, double* dK, double* dAKHA, double* HdA, int* iters);

/* ---- ordering contract of the batched entries ---------------------------------------------------
 * moihgp_filter_stream(_io), moihgp_grad_stream, moihgp_project_stream and moihgp_unproject_stream (and their _tiled forms) are ASYNCHRONOUS on the
 * stream the caller passes and read the handle's per-latent tables and mixing.  gpXX_update, moihgp_update_latents,
 * moihgp_set_mixing and moihgp_reseed_U rewrite those; they (a) first make their internal stream wait for everything enqueued so
 * far on every stream that carried batched work of this handle, so a rewrite never overtakes a sweep that is still in flight,
 * and (b) return only when the new tables are complete, so batched work enqueued afterwards on any stream sees them.  Buffers
 * the caller owns (streams, states, nll, grad) are ordered by the caller's own stream discipline as usual.  A handle is not
 * thread-safe (as the reference object, moihgp.h:431-457 mutates shared matrices): one host thread at a time.
 * The sweeps also use small scratch areas that belong to the handle (flags and hand-over records of their second passes, per-slice
 * partial sums): batched work of ONE handle must be ordered among itself -- keep it on one stream, or order the streams with events.
 * Different handles are independent. */

/* Hand a stream back before destroying it.  The handle remembers (by value) every stream that carried batched work since its last
 * table rewrite and records an event on each of them at the next rewrite; a stream destroyed in between would be a dangling handle
 * there.  moihgp_release_stream orders the handle's own stream behind everything enqueued on `stream` so far and forgets it.  Streams
 * that live as long as the handle (torch's pool, the default stream) never need this. */
int moihgp_release_stream(moihgp_gp* gp, void* stream);

/* Options of a handle (tuning / test hooks; defaults come from the environment variables of the same meaning, read ONCE when the
 * handle is created -- nothing below consults the environment per launch):
 *   "filter_split"    0 = automatic time split for few latents, 1 = off, n > 1 = n slices      (env MOIHGP_FILTER_SPLIT)
 *   "filter_team"     few latents: -1 = automatic, 0 = never, 1 = always take a one-workgroup-per-latent kernel when the stream fits one
 *                     (2 .. 8 segments of 1024 .. 2048 ticks), 2 = the 2048-tick form only -- stacked models; the reference's own models have
 *                     no such form and take the chunk-templated kernel under 2 as under 1                        (env MOIHGP_FILTER_TEAM)
 *   "filter_plain_x"  Matern-3/2 and -5/2 through the stacked filter's kernels (one component): -1 = automatic, 0 = never, 1 = always
 *   "filter_maxlinks" -1 = automatic; chunks with a gap per segment that the stacked filter's second pass takes as broken links
 *                                                                                               (env MOIHGP_FILTER_MAXLINKS)
 *   "filter_impute"   stacked models, 1024 latents and more: latents whose stream holds missing ticks are swept twice without gaps around a scalar
 *                     recursion over their gaps (exact imputation, csrc/recursion_x.hip: filter_x_gaps_a / _b_kernel) instead of by the second
 *                     pass's broken links / tick-by-tick walk, which keeps the latents whose filter remembers more than 1024 ticks:
 *                     -1 = automatic (state dimension >= 8; below it if no latent's filter is that slow), 0 = never, 1 = always.  (env MOIHGP_GAP_TRACE=1: one line per sweep on stderr with the
 *                     number of latents taken, solved and not, and why not; synchronises the stream)
 *   "polar_warm_start" 0 (default) / 1: update() starts the deflation of outlying singular values (csrc/polar_deflate.hip) from the subspace the
 *                     previous update() of this handle found -- consecutive objective evaluations of a learner differ by one line-search step,
 *                     and one pass over the Gram matrix is saved.  The factor is the same to rounding (<= 1e-12), but no longer a function of
 *                     the argument alone bit for bit: off unless asked (include/moihgp_cxx/lbfgsb_dev.hpp asks).
 *   "filter_variant"  kernel tiling probes; accepted only by a library built with -DMOIHGP_TUNING (make TUNING=1), rc 1 otherwise:
 *                     the probe instantiations (some of which do no arithmetic) are not part of the shipped library.
 * Returns 0, or 1 for an unknown name / a value out of range. */
int moihgp_set_option(moihgp_gp* gp, const char* name, long value);

/* ---- batched recursion over pre-projected streams (DEVICE pointers) -------------------------
 * The stream is SERIES-MAJOR: Ty[l*ld + t], l < L (latents owned by gp), t < T, element type per
 * `dtype`.  Requirements: base pointers 16-byte aligned; ld*sizeof(elem) a multiple of 16 and
 * ld >= T rounded up to a multiple of 16/sizeof(elem).
 *
 * For every latent, sequentially in t (order of moihgp_online.h:61-70 / moihgp_regression.h:45-49):
 *     v = y_t - HA x            (pre-step state; ihgp.h:206)
 *     nll += 1/2 (v^2/S + log S)                       (ihgp.h:207)
 *     x <- AKHA x + K y_t ;  yhat_t = x[0]             (ihgp.h:90-91)
 * A NaN y_t takes the missing-data branch x <- A x (ihgp.h:83-87) and contributes no NLL term.
 *
 *   x        [L][d]  in: state before tick 0; out: state after tick T-1   (dtype)
 *   yhat     [L][ld] or NULL                                              (dtype)
 *   nll      [L] doubles or NULL: per-latent sum of ihgp.h:207 terms (always fp64)
 *   stream   hipStream_t (NULL = default stream).  The call is asynchronous.
 * Returns 0 on success, nonzero on invalid arguments (see moihgp_last_error()).            */
int moihgp_filter_stream(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld,
                         void* x, void* yhat, double* nll, void* stream);
/* The same sweep with the start state read from x_in and the end state written to x (x_in == x is the form above).  A caller
 * that sweeps again and again from one fixed state -- the learners restart every objective evaluation from the same x
 * (moihgp_regression.h:38, moihgp_online.h:57) -- keeps that state in a buffer of its own and saves a reset per sweep.
 * nll_total (DEVICE double, may be NULL; needs nll): the sum over the latents of nll[], the scalar the optimiser consumes
 * (moihgp.h:684), added in a fixed order by a one-wavefront kernel queued right behind the sweep. */
int moihgp_filter_stream_io(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld,
                            const void* x_in, void* x, void* yhat, double* nll, double* nll_total, void* stream);

/* The same sweep with a row stride of its own for yhat (ld_out, same rules as ld: a multiple of 16 bytes, >= T rounded up), so that the
 * filtered means can land in a buffer shaped differently from the stream -- a compact [L][T'] array next to a column slice of a wider
 * slab, say.  The two entries above hand yhat the stream's stride, which the library cannot check against the caller's allocation: an
 * output buffer narrower than the stream's rows is then written out of bounds.  Prefer this entry whenever Ty and yhat are not
 * allocated alike.  yhat may be NULL (ld_out is then ignored). */
int moihgp_filter_stream_v2(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in,
                            const void* x_in, void* x, void* yhat, size_t ld_out, double* nll, double* nll_total, void* stream);

/* ---- segment-major streams (round 4) -------------------------------------------------------------------------------------------------
 * The same sweep over streams laid out [ceil(T / SEG)][L][SEG], SEG = 4096 / sizeof(scalar) ticks (1024 fp32, 512 fp64): segment s of every
 * latent side by side, tile (s, l) at ((s L + l) SEG) scalars from the base, the last tile allocated whole (its ticks past T are ignored on
 * input and unspecified on output).  The wavefronts of a launch move through the segments together, so the chip reads and writes one
 * contiguous front instead of L row streams: a cold stream moves ~12 % faster.  For the reference's own models (d = 2, 3);
 * stacked models return 3.  x_in / x / nll / nll_total / stream as moihgp_filter_stream_io; yhat (may be NULL) in the same layout.
 * moihgp_stream_retile copies between the two layouts (to_tiled != 0: src series-major with row stride ld, dst segment-major); a stream that
 * comes from observations and goes back to outputs needs no such copy: moihgp_project_stream_tiled / moihgp_unproject_stream_tiled below. */
int moihgp_filter_stream_tiled(moihgp_gp* gp, int dtype, const void* Ty_tiled, size_t T, const void* x_in, void* x, void* yhat_tiled, double* nll,
                               double* nll_total, void* stream);
int moihgp_stream_retile(int dtype, const void* src, void* dst, size_t L, size_t T, size_t ld, int to_tiled, void* stream);

/* ---- steady-state RTS smoothing of whole streams (not in the reference; its IHGP::backwardSmoother, ihgp.h:103-114, is dead code) ----------
 * The posterior of every latent at every tick given ALL the ticks of the stream, where moihgp_filter_stream* gives the filtered means (ticks
 * up to their own).  A separate estimator of the same model: the learners' filter, NLL and gradients keep the reference's literal gains.
 * Per latent, from the handle's hyper-parameters: A = expm(dt F) (the handle's A), Q = sym(Pinf - A Pinf A^T), H = e0, R = the noise parameter,
 *     P   solves  P = A P A^T - A P H^T (H P H^T + R)^-1 H P A^T + Q     (the Kalman form, by structure-preserving doubling and two Newton
 *                                                                        steps, relative residual <= 1e-12 or status 1; NOT the un-transposed
 *                                                                        DARE of ihgp.h:125, whose gain below diverges)
 *     S = H P H^T + R,  K = P H^T / S,  PF = P - K H P,  G = PF A^T P^-1
 *     Ps  solves  Ps = G Ps G^T + PF - G P G^T                           (exact d^2 x d^2 linear solve)
 *     var_filtered = H PF H^T,  var_smoothed = H Ps H^T
 * and, with x_in the state before tick 0:
 *     forward:   xp[t] = A xf[t-1] (xf[-1] = x_in);  p[t] = H xp[t];  v[t] = y[t] - p[t] (0 where y[t] is NaN);  xf[t] = xp[t] + K v[t]
 *     backward:  s[T] = 0;  s[t] = G s[t+1] + K v[t];  ysmooth[t] = p[t] + s[t]_0
 * (the RTS form xs[t] = xf[t] + G (xs[t+1] - A xf[t]); xs[T-1] = xf[T-1]).  The gains are the steady-state ones: in the interior of a long
 * gap-free stream the result is the exact GP posterior mean (and var_smoothed its variance); within a few correlation lengths of the two ends
 * and of missing ticks it is the IHGP approximation, not the exact posterior.
 * moihgp_smooth_stream: Ty [L][ld_in] series-major (dtype), ysmooth [L][ld_out] (dtype; must not overlap Ty), same stride and alignment rules as
 *   moihgp_filter_stream_v2.  The forward sweep writes the predicted means into ysmooth and the backward sweep smooths them in place.
 *   x_in [L][d] state before tick 0; x [L][d] end state (filtered = smoothed at T-1; may alias x_in).  status: DEVICE int [L] or NULL
 *   (0 ok, 1 Kalman DARE not converged: that latent's row and end state are NaN).  No NLL: the learners' objective stays moihgp_filter_stream*'s.
 *   Asynchronous on `stream`, which joins the handle's set of streams that carry batched work.  The smoother's tables are built on the first
 *   smooth after a table rewrite (gpXX_update, moihgp_update_latents, ...), on that call's stream: the rewrites themselves do no extra work.
 *   Option "smoother_path" (moihgp_set_option): -1 automatic (the time-parallel scan kernels, a serial fp64 walk for latents whose G or A - K H A
 *   fails a growth bound), 0 scan kernels for every latent, 1 serial fp64 walk for every latent.  Stacked models: 3.
 * moihgp_get_smoother: latent l's P [d*d], K [d], G [d*d], Ps [d*d] (row-major), var_filtered, var_smoothed, to HOST buffers (any may be NULL).
 * moihgp_latent_variances: var_filtered [L], var_smoothed [L] to HOST buffers (either may be NULL).  Both synchronise. */
int moihgp_smooth_stream(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in, const void* x_in, void* x,
                         void* ysmooth, size_t ld_out, int* status, void* stream);
int moihgp_get_smoother(moihgp_gp* gp, size_t l, double* P, double* K, double* G, double* Ps,
                        double* var_filtered, double* var_smoothed);
int moihgp_latent_variances(moihgp_gp* gp, double* var_filtered, double* var_smoothed);

/* ---- exact-edge smoothing of whole streams, with per-tick variances (not in the reference) ------------------------------------------------
 * The steady sweeps of moihgp_smooth_stream are the exact smoother of the model under the prior x_0 ~ N(A x_in, P) on the first state; the model's
 * own prior is N(0, Pinf).  Swapping a Gaussian prior on a d-dimensional state is a rank-d update of the whole smoothed trajectory, and the
 * steady smoothed variance is wrong at both ends of a stream (the backward recursion starts from PF, not Ps).  Per latent, take the smoother's
 * tables A, K, G, P, PF, Ps and the model's Pinf, and run moihgp_smooth_stream's two passes from a ZERO start state: p[t], v[t], xf[t], s[t],
 * ys[t] = p[t] + s[t]_0.  Then:
 *     Ps_t :  Ps_{T-1} = PF,   Ps_t = PF + G (Ps_{t+1} - P) G^T            (backward; reaches the tables' Ps away from the end)
 *     E  = Pinf^-1 - P^-1,     Z = -(I + E Ps_0)^-1 E                       (d x d, symmetric; no inverse of Ps)
 *     r_t = e0^T Ps_t (G^T)^t                                               (row vector, decays like G^t)
 *     ysmooth[t] = ys[t] + r_t Z s[0]
 *     var[t]     = (Ps_t)_00 + r_t Z r_t^T                                  (variance of the latent FUNCTION, no noise)
 *     x          = xf[T-1] + PF (G^T)^(T-1) Z s[0]
 * s[0] is the full d-vector the backward pass holds when it leaves tick 0 (with a zero start, the smoothed state at tick 0).  For a gap-free
 * stream these formulas are the GP posterior at every tick, for any T >= 1.  With missing ticks the steady sweeps are themselves approximate
 * near the gaps, as in moihgp_smooth_stream; the correction is applied unchanged and no exactness is claimed there.  Start states are not taken:
 * the start is the prior.
 * Edge lengths, per latent, from the tables: head is the smallest n with |G^n|inf <= 2^-60, tail the smallest k with |G^k|inf^2 <= 2^-60; both are
 * capped at 2^20, and the cap means "never reached".  Ticks in [head, T - tail) are not touched: there ysmooth holds the bits moihgp_smooth_stream
 * writes (from a zero start state) and var the stream-dtype rounding of var_smoothed; x is corrected only when T <= head.  When the two edges of
 * a latent overlap (head + tail > T) the head needs the tail's Ps_t, which goes through a scratch buffer of 8 d T L bytes on the handle, for
 * streams of at most 4096 ticks.
 * moihgp_smooth_stream_exact: Ty, ld_in, ysmooth, ld_out, alignment, overlap rules, asynchrony and stream bookkeeping as moihgp_smooth_stream.
 *   x [L][d] receives the end state (output only).  var [L][ld_out] (dtype) or NULL: a second row-shaped output that may overlap neither Ty nor
 *   ysmooth; NULL writes no variance.  status: DEVICE int [L] or NULL: 0 ok; 1 Kalman DARE not converged (rows and end state NaN, as
 *   moihgp_smooth_stream); 3 the edges overlap in a stream longer than 4096 ticks (ysmooth and x are moihgp_smooth_stream's, var is
 *   var_smoothed at every tick); 4 the edge tables failed (Pinf or P could not be inverted, or something is not finite; the rows as for 3).
 *   Honours the option "smoother_path".  The edge tables are built with the smoother's, on the first call after a table rewrite; that call also
 *   reads the largest head + tail back once and so synchronises.  Stacked models: 3.
 * moihgp_edge_lengths: head [L], tail [L] to HOST buffers (either may be NULL).  Synchronises. */
int moihgp_smooth_stream_exact(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in, void* x, void* ysmooth, void* var, size_t ld_out,
                               int* status, void* stream);
int moihgp_edge_lengths(moihgp_gp* gp, int* head, int* tail);

/* ---- exact smoothing across missing ticks: the GP posterior at every tick (not in the reference) ------------------------------------------
 * Every other whole-stream estimator runs on steady-state gains, and moihgp_smooth_stream_exact corrects them at the two ends of a stream only:
 * inside a gap its variance does not widen.  This entry runs the time-varying recursion instead.  Per latent, in fp64: A the handle's, Pinf the
 * model's, Q = sym(Pinf - A Pinf A^T), H = e0^T, R the noise parameter; sym(X) = (X + X^T) / 2.  A NaN in Ty marks a missing tick, and nothing
 * else does.
 *     forward   xp[0] = 0, P[0] = Pinf;   t > 0: xp[t] = A xf[t-1],  P[t] = sym(A PF[t-1] A^T + Q)
 *               observed: S = P[t]_00 + R, v = y[t] - xp[t]_0, K = P[t] e0 / S, xf[t] = xp[t] + K v, PF[t] = sym(P[t] - K (e0^T P[t]))
 *                         nll += (log(2 pi S) + v^2 / S) / 2
 *               missing:  xf[t] = xp[t], PF[t] = P[t]
 *     backward  xs[T-1] = xf[T-1], Ps[T-1] = PF[T-1]
 *               G = PF[t] A^T P[t+1]^-1      (pivoted elimination, not Cholesky: Q is indefinite for Matern-5/2)
 *               xs[t] = xf[t] + G (xs[t+1] - xp[t+1]),  Ps[t] = sym(PF[t] + G (Ps[t+1] - P[t+1]) G^T)
 *     outputs   mean[t] = xs[t]_0,  var[t] = Ps[t]_00 (the latent FUNCTION, no noise),  x = xf[T-1],  P_end = PF[T-1],  nll
 * For any pattern of missing ticks mean and var are the GP posterior given the observed ticks, nll is -log N(y_obs; 0, C_oo + R I), and (x, P_end)
 * is the filtering distribution at the last tick.  No DARE is involved, so the entry also serves latents whose Kalman DARE does not converge.
 * An all-missing row gives mean 0, var Pinf_00 and nll 0.  T = 0: nothing is written to the rows, x = 0, P_end = Pinf, nll = 0.
 * status per latent: 0 ok; 5 the recursion broke down (S <= 0, a pivot of P[t+1] was zero, or a non-finite quantity arose -- a +-Inf
 * observation among them): the latent's mean and var rows, x, P_end and nll are NaN, no other latent is affected.  Codes 1 to 4 keep their
 * meanings and do not occur here.
 * moihgp_posterior_stream: Ty, ld_in, mean, ld_out, alignment, overlap rules, asynchrony and stream bookkeeping as moihgp_smooth_stream_exact
 *   (mean in ysmooth's place).  x [L][d] (dtype) receives the end state: an output only, the start is the prior.  P_end: DEVICE fp64 [L][d*d] or
 *   NULL.  var [L][ld_out] (dtype) or NULL: shape and rules as mean, may overlap neither Ty nor mean.  nll: DEVICE fp64 [L] or NULL.  status:
 *   DEVICE int [L] or NULL.  The arithmetic is fp64 for both stream dtypes.  Series-major only.  Stacked models: 3.
 *   Scratch: one buffer on the handle, grown on demand (a failed allocation returns 2 with the message; nothing falls back):
 *       8 * ((d + d (d + 1) / 2) * ceil(T / 16) + 1) * L bytes
 *   -- a checkpoint (xf, upper triangle of PF) every 16 ticks, 4.5 bytes per tick and latent at d = 3, and one word per latent. */
int moihgp_posterior_stream(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in, void* x, double* P_end, void* mean, void* var,
                            size_t ld_out, double* nll, int* status, void* stream);

/* ---- multi-horizon forecasts of whole streams, with variances (not in the reference, whose only route is the per-tick ABI: one step(x, y) and
 * then h prediction-only step(x) calls per tick and per horizon, ihgp.h:96-100) --------------------------------------------------------------
 * Per latent, A the handle's A, H = e0, and gains (K, M):
 *     gains = MOIHGP_GAINS_KALMAN (0, the default of the host wrappers): K of the smoother's tables (the Kalman-form DARE of moihgp_smooth_stream),
 *                                  M = A - K H A;
 *     gains = MOIHGP_GAINS_HANDLE (1): the handle's K and AKHA (what moihgp_get_latent returns; the learners' filter, the reference's literal DARE).
 * With x[-1] = x_in:   x[t] = M x[t-1] + K y[t],   or x[t] = A x[t-1] where y[t] is NaN.   For horizons h_0 .. h_{K-1}
 * (0 <= h <= 2^20, 1 <= K <= MOIHGP_FORECAST_MAX_HORIZONS, need not be sorted or distinct):
 *     fc[k][l][t] = H A^{h_k} x_l[t]        0 <= t < T
 * i.e. plane k holds, AT THE INDEX OF THE TICK THE FORECAST WAS MADE AT, the mean of the latent at tick t + h_k given the ticks <= t.  h = 0 is the
 * filtered mean (with gains = 1 it is moihgp_filter_stream's yhat).  A forecast is written at missing ticks too.  With the Kalman gains the interior
 * of a long gap-free stream gives the exact GP predictive mean; the handle's gains give exactly "the reference's step followed by h prediction-only
 * steps", which is off the GP predictive mean by what the literal DARE is off the Kalman one.
 * Variances belong to the Kalman gains only (they are NOT the error of the literal-gain estimator):
 *     var[k][l] = (Pinf - A^{h_k} (Pinf - PF) A^{h_k}^T)_00        Pinf the model's stationary covariance, PF the smoother's filtered covariance
 * the steady-state variance of the latent FUNCTION at t + h given the ticks <= t; add R for an observation.  h = 0 equals var_filtered of
 * moihgp_latent_variances; it rises monotonically to Pinf_00.
 * moihgp_forecast_stream: Ty, x_in, x, ld_in, ld_out, alignment, asynchrony and stream bookkeeping as moihgp_smooth_stream (x_in == x allowed; fc
 *   must not overlap Ty).  horizons: HOST int [K], read before the call returns.  Plane k starts k * plane_stride elements after fc;
 *   plane_stride >= L * ld_out and a multiple of 16 bytes.  status: DEVICE int [L] or NULL.  gains = 0: a latent whose Kalman DARE did not converge
 *   gets status 1, NaN in all its K rows and a NaN end state; the smoother's tables are built on the first such call after a table rewrite, exactly
 *   as by a smooth.  gains = 1: status is all zero (the rows are whatever the handle's own tables give, as moihgp_filter_stream), and the smoother's
 *   tables are neither needed nor built.  fp32 streams are swept in fp32 arithmetic, fp64 streams in fp64.  Returns 1 (and launches nothing) for K or
 *   a horizon out of range, bad strides or alignment, an overlap, unknown gains; 3 for stacked models.
 *   Option "forecast_path" (moihgp_set_option): -1 automatic (the time-parallel scan kernel; a serial fp64 walk for latents whose M fails a
 *   growth bound -- the smoother's for fp64 streams, a tighter one for fp32; rho(AKHA) > 1 does occur with the handle's gains), 0 scan for every
 *   latent, 1 serial fp64 walk for every latent.
 * moihgp_forecast_tail: from any state x [L][d] (dtype), tail[l][j] = H A^{j+1} x_l, 0 <= j < n <= 2^20, tail [L][ld_out] (dtype): the forecast beyond
 *   the end of a stream (depends on A only).  Asynchronous on `stream`.
 * moihgp_forecast_variances: var [K][L] to a HOST buffer (NaN for a latent whose Kalman DARE did not converge).  Synchronises. */
#define MOIHGP_FORECAST_MAX_HORIZONS 8
enum { MOIHGP_GAINS_KALMAN = 0, MOIHGP_GAINS_HANDLE = 1 };
int moihgp_forecast_stream(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in, const void* x_in, void* x,
                           const int* horizons, size_t K, void* fc, size_t ld_out, size_t plane_stride,
                           int gains, int* status, void* stream);
int moihgp_forecast_tail(moihgp_gp* gp, int dtype, const void* x, size_t n, void* tail, size_t ld_out, void* stream);
int moihgp_forecast_variances(moihgp_gp* gp, const int* horizons, size_t K, double* var);

/* ---- forecast scores: backtest errors of those forecasts on the stream itself, per latent and horizon (not in the reference) ---------------------
 * The gains, the recursion x[t] and fc[k][l][t] = H A^{h_k} x_l[t] are exactly moihgp_forecast_stream's, and so are the rules for the horizons
 * (1 .. MOIHGP_FORECAST_MAX_HORIZONS integers in 0 .. 2^20, in any order, repeats allowed).  No plane is written: every forecast is held against the
 * observation it predicts and only sums leave.  For each horizon k and latent l, over the origins t_first <= t < T:
 *     e = y[t + h_k] - fc[k][l][t]           scored iff t + h_k < T and y[t + h_k] is not NaN
 *     n[k][l] = number of scored origins,   sum_err[k][l] = sum of e,   sum_sq[k][l] = sum of e^2
 * The origin tick itself may be missing: the forecast is made there anyway, as moihgp_forecast_stream makes it.  t_first skips the start-up
 * transient of a zero start state.  h = 0 scores the in-sample residual y[t] - H x[t], the observation against the filtered mean it has already
 * moved: that is NOT a prediction error.  The states and the forecasts are computed in the stream's own precision, as the forecast sweep computes
 * them, and e is formed in it; the sums are accumulated in fp64 for both stream types, in a fixed order: two calls with the same arguments give
 * the same bits.
 * With the Kalman gains also
 *     pvar[k][l] = var[k][l] + R_l           var of moihgp_forecast_variances, R_l the latent's noise parameter
 * the steady-state predictive variance of an OBSERVATION at t + h_k given the ticks <= t, for h_k >= 1 (at h = 1 it is S = P_00 + R of the smoother's
 * tables, exactly: Pinf - A (Pinf - PF) A^T = P).  sum_sq / (n pvar) is then ~ 1 for a calibrated model, and
 * -1/2 (n log(2 pi pvar) + sum_sq / pvar) at h = 1 is the steady-state marginal log likelihood of the textbook Kalman filter over the scored ticks
 * (the learners' NLL, which keeps the reference's literal DARE, is moihgp_filter_stream's and is not this).
 * moihgp_forecast_scores: n (long long), sum_err, sum_sq, pvar (double) are DEVICE arrays [K][L]; sum_err and pvar may be NULL.  Ty, x_in, x, ld_in,
 *   alignment, asynchrony and stream bookkeeping as moihgp_forecast_stream; x receives the end state (x_in == x allowed).  horizons: HOST int [K],
 *   read before the call returns.  status: DEVICE int [L] or NULL.  The smoother's tables are built when moihgp_forecast_stream would build them.
 *   gains = 0: a latent whose Kalman DARE did not converge gets status 1, n = 0, NaN sums, NaN pvar and a NaN end state.  gains = 1: status is all
 *   zero, pvar must be NULL (the variances belong to the Kalman gains), and an unstable latent's sums are whatever the arithmetic gives (inf or NaN
 *   allowed).  T = 0 gives zeros and x = x_in.  Option "forecast_path" governs the route as it does for moihgp_forecast_stream (latents that fail the
 *   growth bound take the serial fp64 walk).  Returns 1 (and launches nothing) for K or a horizon out of range, unknown gains, t_first > T, a NULL n
 *   or sum_sq, pvar given with MOIHGP_GAINS_HANDLE; 3 for stacked models. */
int moihgp_forecast_scores(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in, const void* x_in, void* x,
                           const int* horizons, size_t K, size_t t_first, int gains,
                           long long* n, double* sum_err, double* sum_sq, double* pvar, int* status, void* stream);

/* ---- fixed-lag smoothing of whole streams, with variances (not in the reference) -------------------------------------------------------------
 * The mean of every latent at tick t given the ticks up to t + l: what an online caller knows about tick t once it has waited l more ticks.  It
 * is the member of the family between the filtered mean (l = 0: moihgp_forecast_stream with h = 0 and the Kalman gains) and the smoothed one
 * (l >= T: moihgp_smooth_stream) -- a forecast with a negative horizon.
 * Per latent, take the smoother's tables A, K, G, P, PF, Ps (moihgp_smooth_stream), S = P_00 + R, and its forward pass:
 *     xp[t] = A xf[t-1] (xf[-1] = x_in);  p[t] = H xp[t];  v[t] = y[t] - p[t] (0 where y[t] is NaN);  xf[t] = xp[t] + K v[t]
 * For lags l_0 .. l_{K-1} (0 <= l <= 2^20, 1 <= K <= MOIHGP_LAGGED_MAX_LAGS, need not be sorted or distinct):
 *     lag[k][l][t] = p[t] + ( sum_{j=0..l_k, t+j<T} G^j K v[t+j] )_0          0 <= t < T
 *     var[k][l]    = ( Ps + G^l_k (PF - Ps) (G^l_k)^T )_00
 * i.e. plane k holds, AT THE INDEX OF THE TICK IT ESTIMATES, the mean of the latent at tick t given the ticks <= min(t + l_k, T - 1); an online
 * caller has it at tick t + l_k.  The variance is the steady-state one of the latent FUNCTION (add R for an observation): var_filtered at l = 0,
 * falling monotonically to var_smoothed (PF - Ps = sum_{j>=1} G^j (K S K^T) (G^j)^T).  The windowed sum is computed by the exact backward recursion
 *     s_k[t] = G s_k[t+1] + K v[t] - (G^{l_k+1} K) v[t+l_k+1]      (v = 0 at and past T; s_k[T] = 0),      lag[k][l][t] = p[t] + s_k[t]_0
 * Missing ticks and the two ends are treated as the smoother treats them: the gains are the steady-state ones, so in the interior of a long gap-free
 * stream the result is the exact GP conditional mean and variance given y[0 .. t + l]; within a few correlation lengths of the start of the stream
 * and of missing ticks it is the IHGP approximation.
 * moihgp_lagged_stream: Ty, x_in, ld_in, ld_out, alignment, asynchrony and stream bookkeeping as moihgp_forecast_stream.  lags: HOST int [K], read
 *   before the call returns.  ypred [L][ld_out] (dtype) is required and receives p; out holds K planes [L][ld_out], plane k starting k * plane_stride
 *   elements after out (plane_stride >= L * ld_out and a multiple of 16 bytes).  out, ypred and Ty must be mutually disjoint.  x [L][d] receives the
 *   FILTERED state after tick T_state - 1, T_state <= T: T_state = T is the ordinary end state, T_state = 0 returns x_in (x may alias x_in).  A stream
 *   that arrives in slabs is smoothed exactly, without being held whole, by calling on each slab [t0, t1) followed by max(lags) ticks of lookahead
 *   with T_state = t1 - t0, keeping the first t1 - t0 ticks of every plane and carrying x into the next call.  status: DEVICE int [L] or NULL; a
 *   latent whose Kalman DARE did not converge gets status 1 and NaN in all its K rows, in its row of ypred and in x.  The smoother's tables are
 *   built on the first such call after a table rewrite, exactly as by a smooth.  Arithmetic is fp64 for both stream types (an fp32 stream's v is
 *   rounded once to fp32, its results are narrowed on store).  Returns 1 (and launches nothing) for K or a lag out of range, T_state > T, bad strides or alignment, an
 *   overlap; 3 for stacked models.
 *   Option "lagged_path" (moihgp_set_option): -1 automatic (the time-parallel scan kernels; a serial fp64 walk for latents whose G or A - K H A
 *   fails the smoother's growth bound), 0 scan kernels for every latent, 1 serial fp64 walk for every latent.
 * moihgp_lagged_variances: var [K][L] to a HOST buffer (NaN for a latent whose Kalman DARE did not converge).  Synchronises. */
#define MOIHGP_LAGGED_MAX_LAGS 8
int moihgp_lagged_stream(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in, const void* x_in, void* x, size_t T_state,
                         const int* lags, size_t K, void* ypred, void* out, size_t ld_out, size_t plane_stride,
                         int* status, void* stream);
int moihgp_lagged_variances(moihgp_gp* gp, const int* lags, size_t K, double* var);

/* ---- off-grid smoothing of whole streams: means between ticks, with variances (not in the reference) -----------------------------------------
 * The posterior mean of every latent at times BETWEEN the ticks given the whole stream: the smoothed signal upsampled, for resampling, for
 * alignment with another clock, for plotting.  (Smoothing a NaN-padded stream with a bank at dt / n is n times the work and is not this: the
 * steady-state gains of that bank assume an observation every dt / n.)
 * Per latent, take the smoother's tables A, K, G, P, PF, Ps (moihgp_smooth_stream), Pinf and F of the model, H = e0, and its two passes:
 *     forward    xp[t] = A xf[t-1] (xf[-1] = x_in);  p[t] = H xp[t];  v[t] = y[t] - p[t] (0 where y[t] is NaN);  xf[t] = xp[t] + K v[t]
 *     backward   s[T] = 0;  s[t] = G s[t+1] + K v[t];  ys[t] = p[t] + s[t]_0
 * For fractions phi_0 .. phi_{K-1} (finite, 0 <= phi < 1, 1 <= K <= MOIHGP_INTERP_MAX_POINTS, need not be sorted or distinct):
 *     A_phi = expm(F phi dt);  B_phi = expm(F (1 - phi) dt);  P_phi = A_phi PF A_phi^T + Pinf - A_phi Pinf A_phi^T;  G_phi = P_phi B_phi^T P^-1
 *     fine[k][l][t] = a_k . xf[t] + g_k . s[t+1],   a_k = H A_phi_k,  g_k = H G_phi_k          0 <= t < T
 *     var[k][l]     = ( P_phi + G_phi (Ps - P) G_phi^T )_00
 * i.e. plane k holds at index t the mean of the latent at time (t + phi_k) dt given all T ticks: the RTS smoother with an unobserved point
 * inserted between ticks t and t + 1 (the predicted covariance at t + 1 through that point is again P, so nothing else changes).  At phi = 0 it
 * is ys[t] (A_0 = I, G_0 = G); at the last tick s[T] = 0, so the value is the forecast phi dt past the end, H A_phi xf[T-1].  The variance is the
 * steady-state one of the latent FUNCTION (add R for an observation): var_smoothed at phi = 0.  Missing ticks and the two ends are treated as the
 * smoother treats them: in the interior of a long gap-free stream the result is the exact GP conditional mean and variance; within a few
 * correlation lengths of the ends and of missing ticks it is the IHGP approximation.
 * moihgp_interp_stream: Ty, x_in, ld_in, ld_out, alignment, asynchrony and stream bookkeeping as moihgp_lagged_stream.  fracs: HOST double [K], read
 *   before the call returns.  ysmooth [L][ld_out] (dtype) is required and receives ys, equal to moihgp_smooth_stream's to rounding; fine holds K
 *   planes [L][ld_out], plane k starting k * plane_stride elements after fine (plane_stride >= L * ld_out and a multiple of 16 bytes).  fine,
 *   ysmooth and Ty must be mutually disjoint.  x [L][d] receives the end state (x may alias x_in).  status: DEVICE int [L] or NULL; a latent whose
 *   Kalman DARE did not converge gets status 1 and NaN in all its K rows, in its row of ysmooth and in x.  T = 0 writes x and status only.  The
 *   smoother's tables are built on the first such call after a table rewrite, exactly as by a smooth.  Arithmetic is fp64 for both stream types (an
 *   fp32 stream's v and planes are rounded to fp32 between the two passes, its results are narrowed on store).  Returns 1 (and launches nothing)
 *   for K or an offset out of range, bad strides or alignment, an overlap; 3 for stacked models.
 *   Option "interp_path" (moihgp_set_option): -1 automatic (the time-parallel scan kernels; a serial fp64 walk for latents whose G or A - K H A
 *   fails the smoother's growth bound), 0 scan kernels for every latent, 1 serial fp64 walk for every latent.
 * moihgp_interp_variances: var [K][L] to a HOST buffer (NaN for a latent whose Kalman DARE did not converge).  Synchronises. */
#define MOIHGP_INTERP_MAX_POINTS 8
int moihgp_interp_stream(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in, const void* x_in, void* x,
                         const double* fracs, size_t K, void* ysmooth, void* fine, size_t ld_out, size_t plane_stride,
                         int* status, void* stream);
int moihgp_interp_variances(moihgp_gp* gp, const double* fracs, size_t K, double* var);

/* ---- slopes of whole streams: the rate of change of every latent, with variances (not in the reference) ----------------------------------------
 * The derivative with respect to TIME (the unit of dt, not ticks) of the posterior mean of every latent, on or between the ticks, and the posterior
 * variance of that derivative: for trends, turning points and "is it rising, and are we sure" bands.  (Differencing moihgp_interp_stream's planes
 * gives a mean but the wrong variance, and none for the real-time case.)
 * Take A_phi, B_phi, P_phi, G_phi of moihgp_interp_stream above, M_phi = P_phi - Pinf, H = e0, and the smoother's two passes (xf, p, v forward; s
 * backward).  For offsets phi_0 .. phi_{K-1} (as moihgp_interp_stream's: finite, 0 <= phi < 1, 1 <= K <= MOIHGP_INTERP_MAX_POINTS):
 *     given all ticks (MOIHGP_SLOPE_ALL):         slope[k][l][t] = a_k . xf[t] + gd_k . s[t+1]
 *                                                 a_k = e1^T A_phi_k       gd_k = e0^T (F M_phi_k - Pinf F^T) B_phi_k^T P^-1
 *                                                 var[k][l] = (P_phi_k)_11 + gd_k (Ps - P) gd_k^T
 *     given the ticks <= t (MOIHGP_SLOPE_PAST):   slope[k][l][t] = a_k . xf[t]          var[k][l] = (P_phi_k)_11
 * slope[k][l][t] is d/dtau of the posterior mean of latent l at time tau = (t + phi_k) dt.  With ALL it is the derivative with respect to phi dt of
 * moihgp_interp_stream's plane; with PAST the derivative of the forecast phi dt ahead of tick t, at phi = 0 the real-time slope estimate.
 * gd = d g_phi / dtau, since d M_phi / dtau = F M_phi + M_phi F^T and d B_phi^T / dtau = -F^T B_phi^T; equivalently
 *     gd = e1^T G_phi - e0^T (F Pinf + Pinf F^T) B_phi^T P^-1.
 * The second term vanishes where Pinf solves the Lyapunov equation of F (Matern-3/2).  The reference's Matern-5/2, reproduced literally here, has a
 * Pinf that does not (row 0 of F Pinf + Pinf F^T has a non-zero entry (0, 2)): there component 1 of the smoothed state is NOT the slope of the
 * smoothed curve, and the rows e1^T G_phi would be wrong by a third to two thirds of the slope's scale.  The variance is the mixed second derivative,
 * at phi' = phi, of the smoothed covariance of f between two points of one interval, [P_phi A_(phi'-phi)^T + G_phi (Ps - P) G_phi'^T]_00; its first
 * term comes to (P_phi)_11 for both models.  The variance is positive and below the prior's Pinf_11.  At the last tick s[T] = 0, so both forms give
 * the slope of the forecast.  Missing ticks and the two ends are the smoother's steady-state approximation, as everywhere: in the interior of a long
 * gap-free stream mean and variance are those of the exact GP posterior of f' (given all ticks, or the ticks <= t).
 * moihgp_slope_stream: every argument and check as moihgp_interp_stream's (offsets, strides, alignment, overlap, asynchrony, status, T = 0, failed
 *   latents, stacked models rc 3); slope holds the K planes.  given other than the two constants returns 1; a bad call launches nothing.  ysmooth
 *   [L][ld_out] is required: with MOIHGP_SLOPE_ALL it receives the smoothed means, as moihgp_interp_stream's; with MOIHGP_SLOPE_PAST it is scratch of
 *   unspecified content (only the forward sweep runs).  The sweeps are moihgp_interp_stream's kernels, so the option "interp_path" governs the
 *   route here too.  The call's tables live in a buffer of their own: a slope call and an off-grid call on two streams do not wait for each other.
 * moihgp_slope_variances: var [K][L] to a HOST buffer (NaN for a latent whose Kalman DARE did not converge).  Synchronises. */
#define MOIHGP_SLOPE_ALL 0
#define MOIHGP_SLOPE_PAST 1
int moihgp_slope_stream(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in, const void* x_in, void* x,
                        const double* fracs, size_t K, int given, void* ysmooth, void* slope, size_t ld_out, size_t plane_stride,
                        int* status, void* stream);
int moihgp_slope_variances(moihgp_gp* gp, const double* fracs, size_t K, int given, double* var);

/* ---- seeded steady-state posterior samples of whole streams (not in the reference) -----------------------------------------------------------
 * Joint draws over time of every latent given ALL the ticks of the stream: the smoother's mean plus a stationary deviation process with the
 * steady-state posterior's covariance across time.  The textbook backward sampler (x~[t] = xf[t] + G (x~[t+1] - A xf[t]) + w, w ~ N(0, PF - G P G^T))
 * does not exist for these models: the reference's Matern-5/2 (lam = sqrt(3)/l, matern52ss.h:42) makes Q and PF - G P G^T indefinite.  The SCALAR
 * output process is valid all the same: with the smoother's G and Ps, r[k] = H G^k Ps H^T is the posterior covariance between interior ticks k apart,
 * and the sampler draws from its innovations realization, one scalar normal per tick.  Per latent, with h = e0, N = Ps h, r0 = Ps_00:
 *     Sigma  solves   sigma^2 = r0 - Sigma_00,   B = G (N - Sigma h) / sigma^2,   Sigma = G Sigma G^T + sigma^2 B B^T
 * (the limit of the iteration from Sigma = 0; 64 such steps, then up to 8 Newton steps dSigma - Ac dSigma Ac^T = F(Sigma), Ac = G - B h^T).  It is
 * accepted by what it reproduces: with r^[0] = Sigma_00 + sigma^2, r^[k] = (G^{k-1} (G Sigma h + sigma^2 B))_0,
 *     acov_err = max_{k < 64} |r^[k] - r[k]| / r0 <= 1e-9,  sigma^2 > 0 and everything finite, or that latent gets status 2.
 * Lc is the lower Cholesky factor of sym(Sigma) (a pivot <= 0 gives a zero column).
 * Noise: Philox4x32-10 (Random123's constants), key = (seed low word, seed high word), counter = (q, latent0 + l, sample0 + s, tag):
 *     tag 0, q = t / 4: the four words give the normals n[4q] .. n[4q+3];  tag 1, q = 0: the start normals g_0 .. g_3.
 * A pair of words (a, b) -- words (0, 1) and words (2, 3) -- gives two normals, in fp32 whatever the stream's type (an fp32 and an fp64 stream see
 * the same noise), with the accurate library functions:
 *     u1 = ((a >> 8) + 0.5) 2^-24,  u2 = ((b >> 8) + 0.5) 2^-24,  rho = sqrtf(-2 logf(u1)),  normals  rho cosf(2 pi u2),  rho sinf(2 pi u2).
 * Per sample s and latent l, backward in time (fp64 arithmetic for both stream types):
 *     u[T-1] = Lc g;    for t = T-1 .. 0:   e = sigma n[t];   o[t] = u[t]_0 + e;   u[t-1] = G u[t] + B e
 *     samples[s][l][t] = ysmooth[l][t] + o[t]
 * with ysmooth exactly what moihgp_smooth_stream writes for the same arguments: missing ticks and the start state act through the mean only.
 * The deviation process is stationary and independent of the data: it is the exact posterior covariance in the interior of a long gap-free stream;
 * within a few correlation lengths of the two ends and of missing ticks it is under-dispersed (at the last tick the exact variance is var_filtered,
 * not var_smoothed).  This is the same steady-state approximation the smoother's var_smoothed already makes.  Latents are independent a posteriori
 * under the OILMM, so un-projecting plane s (moihgp_unproject_stream) gives a joint sample of all outputs (of the function f; no observation noise).
 * moihgp_sample_stream: Ty, x_in, x, ld_in as moihgp_smooth_stream.  ysmooth [L][ld_out] is required and is written by the smoothing the call runs;
 *   samples [S][L][ld_out], plane s starting s * plane_stride elements after samples; strides and alignment as moihgp_forecast_stream.  ysmooth and
 *   samples must not overlap Ty or each other.  seed: 64 bits; sample0, latent0: offsets of this call's samples and latents in the counter, so that
 *   calls for ranges of samples, or banks that hold ranges of latents, reproduce the rows of one large call bit for bit.  status: DEVICE int [L] or
 *   NULL: 0 ok; 1 Kalman DARE not converged (as the smoother: ysmooth row, end state and sample rows NaN); 2 realization not accepted (sample rows
 *   NaN; ysmooth row and end state the smoother's).  Returns 1 (and launches nothing) for nsamples outside 1 .. 65535, bad strides or alignment, an
 *   overlap; 3 for stacked models.  Asynchronous on `stream`, with the handle's stream bookkeeping as for a smooth; the realization's tables are
 *   built behind the smoother's, on the first call that needs them after a table rewrite.
 *   Option "sample_path" (moihgp_set_option): -1 automatic (the time-parallel scan kernel; a serial fp64 walk for latents whose G fails the
 *   smoother's growth bound), 0 scan for every latent, 1 serial fp64 walk for every latent.
 * moihgp_sample_noise: the normals above without a handle -- noise [S][L][ld] (DEVICE float, n[t] of latent latent0 + l and sample sample0 + s at
 *   [s][l][t], t < T <= ld) and start [S][L][4] (DEVICE float or NULL: g_0 .. g_3).  Asynchronous on `stream`.  The way to audit a draw.
 * moihgp_get_sampler: latent l's B [d], sigma^2, Sigma [d*d], Lc [d*d] (row-major), acov_err and status, to HOST buffers (any may be NULL).
 *   Synchronises. */
int moihgp_sample_stream(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld_in, const void* x_in, void* x,
                         size_t nsamples, unsigned long long seed, unsigned sample0, unsigned latent0,
                         void* ysmooth, size_t ld_out, void* samples, size_t plane_stride, int* status, void* stream);
int moihgp_sample_noise(unsigned long long seed, unsigned latent0, size_t L, unsigned sample0, size_t S, size_t T,
                        float* noise, size_t ld, float* start, void* stream);
int moihgp_get_sampler(moihgp_gp* gp, size_t l, double* B, double* sigma2, double* Sigma, double* Lc, double* acov_err, int* status);

/* ---- seeded forecast paths: joint draws of the ticks beyond a stream (not in the reference) ------------------------------------------------------
 * moihgp_forecast_tail gives the means past the end of a stream and moihgp_forecast_variances the variance of every horizon; neither says how the
 * horizons vary together (the sum over the next n ticks, the largest of them, a set of scenarios).  These are whole trajectories whose covariance
 * across horizons is the GP predictive one.  The textbook recursion x <- A x + chol(Q) n does not exist for these models: the reference's
 * Matern-5/2 makes Q = Pinf - A Pinf A^T indefinite.  The innovations form of the steady-state predictor is always valid: one scalar normal per
 * tick with variance Sv = P_00 + R > 0.  It draws what will be OBSERVED (the latent's projected observation, noise included): the quantity
 * moihgp_forecast_scores scores, with pvar its variance.
 * Per latent, with the handle's A, the smoother's K and P (moihgp_get_smoother), the noise parameter R and Sv = P_00 + R; per sample s, with u[-1]
 * the start state and q = step0 + j the absolute step index, for j = 0 .. n-1 (fp64 arithmetic for both stream types, rounded once at the store):
 *     e = sqrt(Sv) n[q];    u[j] = A u[j-1] + K e;    paths[s][l][j] = u[j]_0 + (1 - K_0) e
 * i.e. the one-step predicted mean (A u[j-1])_0 plus the innovation e, the filtered state then carried on as if paths[s][l][j] had been observed.
 * states_out[s][l] = u[n-1] (the start state when n = 0).
 * Noise: Philox4x32-10 exactly as the sampler's (the same key, Box-Muller in fp32), counter = (q / 4, latent0 + l, sample0 + s, tag 2), element
 * q % 4; tags 0 and 1 are the sampler's, so the draws inside a stream and the draws of its future are independent for one seed.  Nothing of the
 * noise is stored.
 * What the draws are: their mean over draws is H A^{j+1} x (moihgp_forecast_tail); their covariance is C = Sv Lam Lam^T with Lam lower-triangular
 * Toeplitz, taps lam_0 = 1, lam_k = (A^k K)_0 -- the GP predictive covariance of y[T .. T+n) given a long past -- and
 * C_jj = moihgp_forecast_variances([j+1]) + R.  They are draws given the data up to the end state and nothing else: they are NOT jointly consistent
 * with a moihgp_sample_stream draw of the same stream.  Un-projected through the mixing (moihgp_unproject_stream per plane) they are draws of the
 * outputs' observation process inside the mixing's span, with the latents' noise; the sigma^2 component outside the span is not drawn.
 * Not offered: draws of the noise-free function ahead (no recursive realization without a positive semi-definite Q); stacked models (return 3, as
 * everywhere else); a time-parallel scan (a horizon is short next to a stream and the parallelism is in the S L rows: one lane walks one row).
 * moihgp_forecast_paths: exactly one of x ([L][d], dtype, the start of every sample: a stream's end state) and states_in ([S][L][d], fp64 DEVICE:
 *   the states_out of an earlier call) is non-NULL.  states_out [S][L][d] fp64 DEVICE or NULL; it may equal states_in.  n <= 2^20,
 *   step0 + n <= 2^32, nsamples 1 .. 65535.  paths [S][L][ld_out] (dtype), plane s starting s * plane_stride elements after paths; strides and
 *   alignment as moihgp_forecast_stream's fc; paths must not overlap x or the states (NULL is allowed when n = 0).  status: DEVICE int [L] or NULL:
 *   0 ok; 1 Kalman DARE not converged (that latent's rows and states_out NaN for every sample).  Returns 1 (and launches nothing) for bad
 *   arguments; 3 for stacked models.  Asynchronous on `stream`, with the handle's stream bookkeeping as for a forecast; the smoother's tables are
 *   built on the first call that needs them after a table rewrite.
 *   Chaining: a call for n1 steps followed by a call with its states_out as states_in, step0 = n1 and n2 steps reproduces one call of n1 + n2
 *   steps bit for bit, for any n1 (hence the fp64 states and step0): S x L x n can be generated in slabs.  Ranges of samples (sample0) and banks
 *   that hold ranges of latents (latent0) reproduce the rows of one large call likewise.
 * moihgp_forecast_paths_noise: the normals above without a handle -- noise [S][L][ld] (DEVICE float), n[step0 + j] of latent latent0 + l and
 *   sample sample0 + s at [s][l][j], j < n <= ld.  Asynchronous on `stream`.  The way to audit a path. */
int moihgp_forecast_paths(moihgp_gp* gp, int dtype, const void* x, const double* states_in, double* states_out,
                          size_t n, size_t step0, size_t nsamples, unsigned long long seed, unsigned sample0, unsigned latent0,
                          void* paths, size_t ld_out, size_t plane_stride, int* status, void* stream);
int moihgp_forecast_paths_noise(unsigned long long seed, unsigned latent0, size_t L, unsigned sample0, size_t S,
                                size_t step0, size_t n, float* noise, size_t ld, void* stream);

/* As above plus the hyper-parameter sensitivities (ihgp.h:54) and the per-latent NLL gradient
 * (ihgp.h:216-220), summed over ticks:
 *   dx   [L][P][d] in/out (dtype);  grad [L][P] doubles out. */
int moihgp_grad_stream(moihgp_gp* gp, int dtype, const void* Ty, size_t T, size_t ld,
                       void* x, void* dx, void* yhat, double* nll, double* grad, void* stream);

/* ---- OILMM projection over whole streams (DEVICE pointers) ----------------------------------
 * Y is TICK-MAJOR [T][M] (a stream of observation vectors, as the reference's callers hold it,
 * example.py:40-42); the projected stream comes out series-major [L][ld] ready for the recursion:
 *     Ty[l][t] = S_l^-1/2 * sum_m U[m][l] Y[t][m]                 (moihgp.h:181)
 * and back:  Yhat[t][m] = sum_l U[m][l] S_l^1/2 Tyhat[l][t]       (moihgp.h:222-225)
 * A tick whose observation vector holds NaN (missing outputs) is projected as the reference does it, by least squares over the observed
 * rows (moihgp.h:167-178): Ty[:, t] = S^-1/2 (U0^T U0)^-1 U0^T y_obs -- evaluated through the k x k system of the k missing rows
 * (U^T U = I for the polar factor update() installs: U0^T U0 = I - U_miss^T U_miss), the same vector to rounding.  It needs
 * orthonormal columns (checked when the mixing comes from moihgp_set_mixing), at most 64 missing outputs in the tick, at least L
 * observed ones, and L <= 15040 (the tick's U^T y lives in the workgroup's LDS); otherwise the NaN propagates into Ty[:, t], i.e. the
 * recursion treats the whole tick as missing (use the per-tick ABI for such ticks). */
int moihgp_project_stream(moihgp_gp* gp, int dtype, const void* Y, size_t T, void* Ty, size_t ld, void* stream);
/* The same least-squares projection when the latents are split over ranks (one object per rank holding ITS columns of the global orthonormal
 * factor, moihgp_set_mixing): (U0^T U0)^-1 couples all latents, but by Woodbury only sums over the latent columns cross the shards.
 *   1. project the stream with the NaNs replaced by zeros (moihgp_project_stream on the zero-filled Y): Ty = S^-1/2 U_r^T y0, column-local;
 *   2. moihgp_ls_shard_gram:  per affected tick (ticks: DEVICE int32 [n], ascending) this rank's part of [U_miss r | U_miss U_miss^T] into
 *      packed [n][kmax + kmax^2] doubles (zero padded; kmax = the largest number of missing outputs in one tick, <= 64);
 *   3. the caller all-reduces (SUM) `packed` over the ranks -- the path's one extra exchange;
 *   4. moihgp_ls_shard_apply: solves the k x k systems (identical on every rank) and corrects this rank's rows of Ty in place.
 * Y is the ORIGINAL stream (with its NaNs: they name the missing outputs). */
int moihgp_ls_shard_gram(moihgp_gp* gp, int dtype, const void* Y, const int* ticks, size_t n, int kmax, const void* Ty, size_t ld, double* packed, void* stream);
int moihgp_ls_shard_apply(moihgp_gp* gp, int dtype, const void* Y, const int* ticks, size_t n, int kmax, const double* packed, void* Ty, size_t ld, void* stream);
int moihgp_unproject_stream(moihgp_gp* gp, int dtype, const void* Tyhat, size_t T, size_t ld, void* Yhat, void* stream);
/* The same two products with the stream in the SEGMENT-MAJOR layout of moihgp_filter_stream_tiled ("segment-major streams" above:
 * [ceil(T / SEG)][L][SEG], tile (s, l) at ((s L + l) SEG) scalars from the base, the last tile allocated whole), so that
 *     Y [T][M]  ->  moihgp_project_stream_tiled  ->  moihgp_filter_stream_tiled  ->  moihgp_unproject_stream_tiled  ->  Yhat [T][M]
 * runs without a moihgp_stream_retile pass on either side.  The arithmetic, its order and the results are those of the series-major entries
 * bit for bit; only the addresses differ.  Everything else is theirs too: a full object, asynchronous on `stream` under the ordering contract,
 * the least-squares projection of ticks with missing outputs with the same limits (beyond them the tick's NaN column stands).
 * Ticks past T in the last tile: UNSPECIFIED after the projection (it never writes them -- whatever the buffer held stays), IGNORED by the
 * un-projection (it never reads them: they may hold NaN).  The projection applies to stacked models as well; their sweep takes series-major
 * streams only.  Returns 1 for an unknown dtype, a null pointer or a segment-major base that is not 16-byte aligned (T > 0); T == 0 returns 0
 * and touches nothing. */
int moihgp_project_stream_tiled(moihgp_gp* gp, int dtype, const void* Y, size_t T, void* Ty_tiled, void* stream);
int moihgp_unproject_stream_tiled(moihgp_gp* gp, int dtype, const void* Tyhat_tiled, size_t T, void* Yhat, void* stream);

/* ---- the learners' windowed objective as one call (HOST pointers, fp64) -----------------------------
 * One evaluation of the loop of moihgp_online.h:61-70 / moihgp_regression.h:42-50 / online_learning.py:83-89:
 *     for t < W:  step(x, y_t, dx, xnew, dxnew);  loss += negLogLikelihood(x, y_t, dx, g);  grad += g;  x = xnew;  dx = dxnew
 * with the object's current parameters (set them with gpXX_update first, moihgp_online.h:43).  `loss` is the sum of what
 * gpXX_lik1 returns per tick, i.e. it follows the object's `threading` flag (moihgp.h:590 vs :597-607, see gp32_new).
 * moihgp_window_set uploads the window Y [W][M] (tick-major, already de-meaned by the caller) once; it stays
 * resident for all evaluations of one L-BFGS solve.
 * Ticks with missing outputs (NaN in y_t) are projected by least squares over the observed rows, as moihgp_project_stream does it
 * (moihgp.h:485-494, same k x k Woodbury form and the same limits: at most 64 missing outputs per tick, at least L observed, orthonormal
 * mixing, L <= 15040; moihgp_window_set returns 3 beyond them: use the per-tick ABI for such windows).  Everything else of such a tick is
 * the reference's own arithmetic on a vector that holds NaN (moihgp.h:499-563: (I - U U^T) y, y^T U dU^T y, pv with raw y(l) are dense
 * products with y): the loss and the U / S / sigma part of the gradient come out NaN, the per-latent part (which only sees the projected
 * stream, moihgp.h:565-607) and the carried state are finite -- exactly what gpXX_lik1 / gpXX_step1 return tick by tick.
 * moihgp_window_eval:  x [L][d], dx [L][P][d] state before the window;  *loss, grad [M*L+L+1+L*P] summed over the
 * W ticks;  xnew / dxnew (may be NULL) state after the window. */
int moihgp_window_set(moihgp_gp* gp, const double* Y, size_t W);
int moihgp_window_eval(moihgp_gp* gp, const double* x, const double* dx, double* loss, double* grad, double* xnew, double* dxnew);

/* ---- the same objective without PCIe in the optimiser's inner loop (DEVICE pointers, fp64) ------------------------------------
 * gpXX_update and moihgp_window_eval move the parameter and gradient vectors (8 (M L + ..) bytes each: 134 MB at M = L = 4096) across
 * PCIe on every objective evaluation.  An optimiser that keeps theta, its gradient and its correction pairs on the device calls these
 * instead: params / grad are DEVICE arrays laid out exactly as the host ones ([U row-major | S | sigma | P values per latent],
 * moihgp.h:93); x, dx, xnew, dxnew, loss are DEVICE arrays / a DEVICE scalar.  moihgp_update_dev == gpXX_update (moihgp.h:431-457; the
 * small tail S | sigma | per-latent values is mirrored to the host for getParams, the mixing is not copied until somebody asks);
 * moihgp_window_eval_dev == moihgp_window_eval on the window moihgp_window_set installed.  Both run on the handle's own stream and
 * return when the results are complete (like their host forms), so the caller's streams need no extra ordering AFTER the call.  The
 * input arrays must be complete when the call is made: synchronise (or otherwise finish) the stream that produced them first -- the
 * handle's stream does not wait for caller streams it has never seen.
 * Same values as the host forms, bit for bit (same kernels). */
int moihgp_update_dev(moihgp_gp* gp, const double* params_dev);
int moihgp_window_eval_dev(moihgp_gp* gp, const double* x_dev, const double* dx_dev, double* loss_dev, double* grad_dev,
                           double* xnew_dev, double* dxnew_dev);
/* The same two entries for callers that produce the operands on a stream of their own (`stream`: a hipStream_t; NULL = the default
 * stream).  The handle's stream is ordered BEHIND everything queued on `stream` at the time of the call (an event, no host
 * synchronisation): operands written by kernels or copies still in flight there are fine.
 *   moihgp_window_eval_dev_on does not synchronise the host at all: `stream` is made to wait for the results, so whatever the caller
 *     queues on it afterwards (an axpy of the gradient, the download of the loss) sees them; other streams need their own ordering.
 *   moihgp_update_dev_on returns, like gpXX_update, when the new tables are complete (the polar factor's step count is decided on the
 *     host, and the tail S | sigma | per-latent values is mirrored there), so only the ordering of its INPUT changes.
 * Values bit-identical to the forms above (tests/test_gpu_configs.py::test_dev_entries_take_the_callers_stream). */
int moihgp_update_dev_on(moihgp_gp* gp, const double* params_dev, void* stream);
int moihgp_window_eval_dev_on(moihgp_gp* gp, const double* x_dev, const double* dx_dev, double* loss_dev, double* grad_dev,
                              double* xnew_dev, double* dxnew_dev, void* stream);
/* getParams (moihgp.h:721-738) into a DEVICE array [num_param]. */
int moihgp_get_params_dev(moihgp_gp* gp, double* params_dev);

/* ---- device vectors: what a bound-constrained L-BFGS needs to keep theta, the gradient and its correction pairs on the device ---------
 * (include/moihgp_cxx/lbfgsb_dev.hpp is such an optimiser; with moihgp_update_dev / moihgp_window_eval_dev one iteration of the learners'
 * loop, moihgp_online.h:40-72 + LBFGSB.h:117-241, then moves no parameter-sized vector across PCIe).  fp64, DEVICE pointers; a context owns
 * a stream, the scratch of the reductions and a page-locked result word.  Element-wise entries are asynchronous on the context's stream;
 * the reductions (dot, proj_step, proj_grad_norm) are deterministic (fixed grid, fixed order) and return their scalar after
 * synchronising it.  mask (unsigned char [n], may be NULL): entries whose byte is 0 are skipped (the free-variable set of the active-set
 * method).  Return codes as for the other additive entries. */
typedef struct moihgp_dvec_ctx moihgp_dvec_ctx;
moihgp_dvec_ctx* moihgp_dvec_ctx_new(void);
void    moihgp_dvec_ctx_del(moihgp_dvec_ctx* c);
void*   moihgp_dvec_ctx_stream(moihgp_dvec_ctx* c);                   /* the context's hipStream_t (for the `_on` entries above) */
double* moihgp_dvec_alloc(size_t n);                                  /* n doubles of device memory (NULL on failure) */
unsigned char* moihgp_dvec_alloc_mask(size_t n);
void    moihgp_dvec_free(void* p);                                    /* as hipFree for the caller; blocks of 1 MB and more are kept for the next alloc of that size */
void    moihgp_dvec_trim(void);                                       /* hand the kept blocks back to the driver */
void    moihgp_dvec_cache_limit(size_t bytes);                        /* most the cache may hold (default 8 GB, or MOIHGP_DVEC_CACHE_GB; 0: keep nothing); trims if over */
int moihgp_dvec_upload(moihgp_dvec_ctx* c, double* dst_dev, const double* src_host, size_t n);     /* synchronous */
int moihgp_dvec_download(moihgp_dvec_ctx* c, double* dst_host, const double* src_dev, size_t n);   /* synchronous */
int moihgp_dvec_copy(moihgp_dvec_ctx* c, double* dst_dev, const double* src_dev, size_t n);
int moihgp_dvec_sync(moihgp_dvec_ctx* c);
int moihgp_dvec_dot(moihgp_dvec_ctx* c, size_t n, const double* a, const double* b, const unsigned char* mask, double* result);
int moihgp_dvec_axpy(moihgp_dvec_ctx* c, size_t n, double alpha, const double* x, double* y, const unsigned char* mask);     /* y += alpha x */
int moihgp_dvec_scale(moihgp_dvec_ctx* c, size_t n, double alpha, const double* x, double* y, const unsigned char* mask);    /* y = alpha x (0 where masked out) */
int moihgp_dvec_sub(moihgp_dvec_ctx* c, size_t n, const double* a, const double* b, double* out);                           /* out = a - b */
int moihgp_dvec_clamp(moihgp_dvec_ctx* c, size_t n, double* x, const double* lb, const double* ub);
/* free_var[i] = 0 where x sits at a bound with the gradient pointing out of the box, or lb == ub; 1 elsewhere */
int moihgp_dvec_active_set(moihgp_dvec_ctx* c, size_t n, const double* x, const double* g, const double* lb, const double* ub, unsigned char* free_var);
/* xt = clamp(xp + step drt, lb, ub);  *dec = sum gradp (xt - xp)   (projected search point and its Armijo decrease) */
int moihgp_dvec_proj_step(moihgp_dvec_ctx* c, size_t n, const double* xp, const double* drt, double step, const double* lb, const double* ub, const double* gradp,
                          double* xt, double* dec);
/* max |clamp(x - g, lb, ub) - x|   (projected-gradient norm, LBFGSB.h:64-67) */
int moihgp_dvec_proj_grad_norm(moihgp_dvec_ctx* c, size_t n, const double* x, const double* g, const double* lb, const double* ub, double* result);

/* Kernel-exact timing of moihgp_filter_stream launches (bench / diagnosis).  After
 * moihgp_profile_enable(gp, n) the next n launches on this handle are bracketed by a HIP event pair
 * attached to the dispatch itself (hipExtLaunchKernel), not to the stream.  The pair brackets the sweep's FIRST (dominant) kernel --
 * the one rocprofv3 lists as filter_scan_kernel / filter_x_kernel; the small kernels queued behind it (the NLL total, the slice sums,
 * and for streams with missing ticks the second pass of the stacked filter) are outside it: time such streams with the wall clock.  moihgp_profile_read waits
 * for them, writes the per-launch durations in milliseconds, rearms the slots and returns the count.
 * moihgp_profile_enable(gp, 0) turns it off.  An event pair makes the dispatch it brackets wait for its predecessor and costs
 * 3-6 us of launch overlap; moihgp_profile_stride(gp, k) attaches pairs to every k-th launch only (default 1), so a timed loop
 * can sample its kernel durations without slowing every pass. */
int moihgp_profile_enable(moihgp_gp* gp, int max_launches);
int moihgp_profile_stride(moihgp_gp* gp, int stride);
int moihgp_profile_read(moihgp_gp* gp, float* ms, int n);

/* Page-lock a caller-owned HOST buffer that is passed again and again to the reference ABI (the params / grad staging arrays
 * of pywrapper.py:146-149 are 8*(M*L+..) bytes: 134 MB at M = L = 4096), so that the copies behind gpXX_update / gpXX_lik1 /
 * moihgp_window_eval run at PCIe rate instead of the pageable rate.  The buffer must outlive the handle (it is unregistered
 * in *_del).  Optional: everything works without it. */
int moihgp_pin_host_buffer(moihgp_gp* gp, void* ptr, size_t bytes);

/* Stream synchronisation helper for callers without a HIP runtime binding. */
int moihgp_stream_sync(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOIHGP_C_API_H_ */
