// moihgp_regression.hpp -- Eigen-free C++ batch learner over libmoihgp.so, mirroring the reference's
// moihgp::RegressionObjective<SS> / moihgp::MOIHGPRegression<SS> (reference moihgp/include/moihgp/moihgp_regression.h:17-202):
// fit(Y) minimises the summed negative log-likelihood of the whole series from a zero start state, predict(Y) filters it.
// Like the reference (moihgp_regression.h:34-52) the objective does NOT call update(params): literal, including the
// consequence that the model's parameters never change during fit().  Set `apply_params = true` to evaluate the objective at
// the parameters it is given.  Host-side differences from the reference: std::vector containers, one device call per objective
// evaluation (moihgp_window_*), this repo's optimiser (lbfgsb.hpp) instead of LBFGS++.
#ifndef MOIHGP_CXX_MOIHGP_REGRESSION_HPP_
#define MOIHGP_CXX_MOIHGP_REGRESSION_HPP_

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "lbfgsb.hpp"
#include "moihgp.hpp"

namespace moihgp {

template <typename StateSpace>
class RegressionObjective {
public:
    typedef std::vector<double> Vector;
    RegressionObjective(const size_t& num_data, MOIHGP<StateSpace>* gp) {                            // moihgp_regression.h:22-31
        _gp = gp;
        _dim = _gp->getIGPDim();
        _num_param = _gp->getNumParam();
        _igp_num_param = _gp->getNumIGPParam();
        _num_latent = _gp->getNumLatent();
        _num_output = _gp->getNumOutput();
        _num_data = num_data;
        Y.reserve(_num_data);
    }
    double operator()(const Vector& params, Vector& grad) {                                          // moihgp_regression.h:34-52
        if (apply_params) _gp->update(params);
        grad.assign(_num_param, 0.0);
        if (Y.empty()) return 0.0;
        if (_dirty) {
            _Yflat.resize(Y.size() * _num_output);
            for (size_t t = 0; t < Y.size(); t++) for (size_t m = 0; m < _num_output; m++) _Yflat[t * _num_output + m] = Y[t][m];
            const int rc = moihgp_window_set(_gp->handle(), _Yflat.data(), Y.size());
            if (rc != 0 && rc != 3) throw std::runtime_error(std::string("moihgp_window_set: ") + moihgp_last_error());
            _per_tick = rc == 3;          // missing outputs beyond the batched kernel's limits: the reference's loop, tick by tick
            _dirty = false;
        }
        Vector x(_num_latent * _dim, 0.0), dx(_num_latent * _igp_num_param * _dim, 0.0);            // :38-39 zero start
        if (_per_tick) return window_loop_per_tick(_gp->handle(), _Yflat.data(), Y.size(), _num_output, x, dx, grad);
        double loss = 0.0;
        if (moihgp_window_eval(_gp->handle(), x.data(), dx.data(), &loss, grad.data(), nullptr, nullptr) != 0)
            throw std::runtime_error(std::string("moihgp_window_eval: ") + moihgp_last_error());
        return loss;
    }
    void set_data(const std::vector<Vector>& data) { Y = data; _dirty = true; }
    std::vector<Vector> Y;
    bool apply_params = false;

private:
    size_t _dim, _num_param, _igp_num_param, _num_latent, _num_output, _num_data;
    MOIHGP<StateSpace>* _gp;
    Vector _Yflat;
    bool _dirty = true, _per_tick = false;
};

template <typename StateSpace>
class MOIHGPRegression {
public:
    typedef std::vector<double> Vector;
    MOIHGPRegression(const double& dt, const size_t& num_output, const size_t& num_latent, const size_t& num_data,
                     const bool& threading) {                                                      // moihgp_regression.h:80-108
        _dt = dt; _num_output = num_output; _num_latent = num_latent; _num_data = num_data; _threading = threading;
        _moihgp = new MOIHGP<StateSpace>(dt, num_output, num_latent, threading);
        _dim = _moihgp->getIGPDim();
        _num_param = _moihgp->getNumParam();
        _igp_num_param = _moihgp->getNumIGPParam();
        _lb.assign(_num_param, 0.0); _ub.assign(_num_param, 0.0);
        const size_t nu = _num_output * _num_latent;
        for (size_t i = 0; i < nu; i++) { _lb[i] = -1e+4; _ub[i] = 1e+4; }
        for (size_t i = nu; i < nu + _num_latent; i++) { _lb[i] = 1e-4; _ub[i] = 1e+4; }
        for (size_t i = nu + _num_latent; i < _num_param; i++) { _lb[i] = 1e-4; _ub[i] = 1e+2; }
        _params = _moihgp->getParams();
        _LBFGSB_param.max_iterations = 1000;                                                        // :100-105
        _LBFGSB_param.m = 10;
        _LBFGSB_param.max_linesearch = 20;
        _LBFGSB_param.ftol = 1e-8;
        _LBFGSB_param.epsilon = 1e-8;
        _LBFGSB_param.epsilon_rel = 1e-8;
        _solver = new opt::LBFGSBSolver(_LBFGSB_param);
        _obj = new RegressionObjective<StateSpace>(_num_data, _moihgp);
    }
    ~MOIHGPRegression() { delete _obj; delete _solver; delete _moihgp; }
    MOIHGPRegression(const MOIHGPRegression&) = delete;
    MOIHGPRegression& operator=(const MOIHGPRegression&) = delete;

    int fit(const std::vector<Vector>& Y) {                                                         // :118-124
        _obj->set_data(Y);
        double fx;
        int num_iter = _solver->minimize(*_obj, _params, fx, _lb, _ub);
        _params = _moihgp->getParams();
        return num_iter;
    }
    std::vector<Vector> predict(const std::vector<Vector>& Y) {                                     // :127-139
        std::vector<Vector> Yhat;
        Yhat.reserve(Y.size());
        Vector x(_num_latent * _dim, 0.0), xnew(x.size()), yhat(_num_output), y(_num_output);
        for (size_t t = 0; t < Y.size(); t++) {
            y = Y[t];
            gp32_step3(_moihgp->handle(), x.data(), y.data(), xnew.data(), yhat.data());
            Yhat.push_back(yhat);
            x = xnew;
        }
        return Yhat;
    }
    // (not in the reference) The steady-state RTS smoother of the whole series with the current parameters (include/moihgp.h
    // moihgp_smooth_stream): the posterior mean of every output at every tick given ALL of Y, from a zero start state, where predict()
    // returns filtered means.  fp64 on the device: project_stream -> smooth_stream -> unproject_stream.  Throws std::runtime_error if a latent's
    // Kalman DARE did not converge (status 1: its row would be NaN).  Missing outputs (NaN) go through moihgp_project_stream's least-squares
    // projection, which has limits predict() does not: a tick with more than 64 missing outputs, or fewer than num_latent observed ones, is
    // treated as missing as a whole (the smoother then carries the state across it).
    std::vector<Vector> predictSmoothed(const std::vector<Vector>& Y) {
        const size_t T = Y.size(), M = _num_output, L = _num_latent, ld = (T + 1) / 2 * 2;
        std::vector<Vector> Ys(T, Vector(M, 0.0));
        if (T == 0) return Ys;
        Vector flat(T * M), zeros(L * _dim, 0.0);
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) flat[t * M + m] = Y[t][m];
        moihgp_dvec_ctx* ctx = moihgp_dvec_ctx_new();
        const size_t nst = (L + 1) / 2;                             // status words: L ints in doubles' storage
        double *dY = moihgp_dvec_alloc(T * M), *dTy = moihgp_dvec_alloc(L * ld), *dys = moihgp_dvec_alloc(L * ld), *dx = moihgp_dvec_alloc(L * _dim),
               *dst = moihgp_dvec_alloc(nst);
        int rc = (ctx && dY && dTy && dys && dx && dst) ? 0 : 4;
        Vector st(nst, 0.0);
        void* s = ctx ? moihgp_dvec_ctx_stream(ctx) : nullptr;
        moihgp_gp* h = _moihgp->handle();
        if (!rc) rc = moihgp_dvec_upload(ctx, dY, flat.data(), T * M);
        if (!rc) rc = moihgp_dvec_upload(ctx, dx, zeros.data(), L * _dim);
        if (!rc) rc = moihgp_project_stream(h, MOIHGP_F64, dY, T, dTy, ld, s);
        if (!rc) rc = moihgp_smooth_stream(h, MOIHGP_F64, dTy, T, ld, dx, dx, dys, ld, reinterpret_cast<int*>(dst), s);
        if (!rc) rc = moihgp_unproject_stream(h, MOIHGP_F64, dys, T, ld, dY, s);
        if (!rc) rc = moihgp_dvec_download(ctx, flat.data(), dY, T * M);
        if (!rc) rc = moihgp_dvec_download(ctx, st.data(), dst, nst);
        if (ctx) { moihgp_dvec_sync(ctx); moihgp_release_stream(h, s); }
        for (double* p : {dY, dTy, dys, dx, dst}) if (p) moihgp_dvec_free(p);
        if (ctx) moihgp_dvec_ctx_del(ctx);
        if (rc) throw std::runtime_error(std::string("predictSmoothed: ") + moihgp_last_error());
        std::vector<int> status(2 * nst, 0);
        std::memcpy(status.data(), st.data(), sizeof(double) * nst);
        for (size_t l = 0; l < L; l++)
            if (status[l] != 0) throw std::runtime_error("predictSmoothed: the Kalman DARE of latent " + std::to_string(l) + " did not converge");
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) Ys[t][m] = flat[t * M + m];
        return Ys;
    }
    // (not in the reference) Seeded joint posterior samples of the whole series with the current parameters (include/moihgp.h
    // moihgp_sample_stream): element [s][t] is sample s of every output at tick t given ALL of Y -- the smoothed mean of predictSmoothed() plus a
    // draw of the steady-state deviation process (exact covariance in the interior of a long gap-free series, under-dispersed near its ends and
    // missing ticks), from a zero start state.  The same seed gives the same samples.  fp64 on the device: project_stream -> sample_stream ->
    // unproject_stream per sample.  Throws std::invalid_argument for nsamples outside 1 .. 65535 and std::runtime_error on a non-zero status
    // (1 Kalman DARE not converged, 2 sampling realization not accepted).  Missing outputs (NaN) are projected as in predictSmoothed().
    std::vector<std::vector<Vector>> sampleSmoothed(const std::vector<Vector>& Y, size_t nsamples, unsigned long long seed = 0) {
        if (nsamples < 1 || nsamples > 65535) throw std::invalid_argument("sampleSmoothed: nsamples must be 1 .. 65535");
        const size_t T = Y.size(), M = _num_output, L = _num_latent, ld = (T + 1) / 2 * 2, S = nsamples;
        std::vector<std::vector<Vector>> Ys(S, std::vector<Vector>(T, Vector(M, 0.0)));
        if (T == 0) return Ys;
        Vector flat(T * M), zeros(L * _dim, 0.0);
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) flat[t * M + m] = Y[t][m];
        moihgp_dvec_ctx* ctx = moihgp_dvec_ctx_new();
        const size_t nst = (L + 1) / 2;                             // status words: L ints in doubles' storage
        double *dY = moihgp_dvec_alloc(T * M), *dTy = moihgp_dvec_alloc(L * ld), *dys = moihgp_dvec_alloc(L * ld), *dsm = moihgp_dvec_alloc(S * L * ld),
               *dx = moihgp_dvec_alloc(L * _dim), *dst = moihgp_dvec_alloc(nst);
        int rc = (ctx && dY && dTy && dys && dsm && dx && dst) ? 0 : 4;
        Vector st(nst, 0.0);
        void* s = ctx ? moihgp_dvec_ctx_stream(ctx) : nullptr;
        moihgp_gp* h = _moihgp->handle();
        if (!rc) rc = moihgp_dvec_upload(ctx, dY, flat.data(), T * M);
        if (!rc) rc = moihgp_dvec_upload(ctx, dx, zeros.data(), L * _dim);
        if (!rc) rc = moihgp_project_stream(h, MOIHGP_F64, dY, T, dTy, ld, s);
        if (!rc) rc = moihgp_sample_stream(h, MOIHGP_F64, dTy, T, ld, dx, dx, S, seed, 0, 0, dys, ld, dsm, L * ld, reinterpret_cast<int*>(dst), s);
        if (!rc) rc = moihgp_dvec_download(ctx, st.data(), dst, nst);
        for (size_t k = 0; k < S && !rc; k++) {
            rc = moihgp_unproject_stream(h, MOIHGP_F64, dsm + k * L * ld, T, ld, dY, s);
            if (!rc) rc = moihgp_dvec_download(ctx, flat.data(), dY, T * M);
            if (!rc) rc = moihgp_dvec_sync(ctx);
            if (!rc) for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) Ys[k][t][m] = flat[t * M + m];
        }
        if (ctx) { moihgp_dvec_sync(ctx); moihgp_release_stream(h, s); }
        for (double* p : {dY, dTy, dys, dsm, dx, dst}) if (p) moihgp_dvec_free(p);
        if (ctx) moihgp_dvec_ctx_del(ctx);
        if (rc) throw std::runtime_error(std::string("sampleSmoothed: ") + moihgp_last_error());
        std::vector<int> status(2 * nst, 0);
        std::memcpy(status.data(), st.data(), sizeof(double) * nst);
        for (size_t l = 0; l < L; l++)
            if (status[l] != 0) throw std::runtime_error("sampleSmoothed: latent " + std::to_string(l) + " has status " + std::to_string(status[l]) +
                                                         (status[l] == 1 ? " (the Kalman DARE did not converge)" : " (the sampling realization was not accepted)"));
        return Ys;
    }
    // (not in the reference) Forecasts `horizon` ticks ahead at every tick of the series with the current parameters (include/moihgp.h
    // moihgp_forecast_stream, Kalman-form gains): element t is the mean of every output at tick t + horizon given Y[0..t], from a zero start
    // state, where the reference would call step(x, y) and then `horizon` prediction-only steps per tick.  fp64 on the device:
    // project_stream -> forecast_stream -> unproject_stream.  Throws std::invalid_argument for a horizon outside 0 .. 2^20 and std::runtime_error
    // if a latent's Kalman DARE did not converge (status 1: its row would be NaN).  Missing outputs (NaN) are projected as in predictSmoothed().
    std::vector<Vector> predictAhead(const std::vector<Vector>& Y, int horizon) {
        if (horizon < 0 || horizon > (1 << 20)) throw std::invalid_argument("predictAhead: horizon must be 0 .. 2^20");
        const size_t T = Y.size(), M = _num_output, L = _num_latent, ld = (T + 1) / 2 * 2;
        std::vector<Vector> Yf(T, Vector(M, 0.0));
        if (T == 0) return Yf;
        Vector flat(T * M), zeros(L * _dim, 0.0);
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) flat[t * M + m] = Y[t][m];
        moihgp_dvec_ctx* ctx = moihgp_dvec_ctx_new();
        const size_t nst = (L + 1) / 2;                             // status words: L ints in doubles' storage
        double *dY = moihgp_dvec_alloc(T * M), *dTy = moihgp_dvec_alloc(L * ld), *dfc = moihgp_dvec_alloc(L * ld), *dx = moihgp_dvec_alloc(L * _dim),
               *dst = moihgp_dvec_alloc(nst);
        int rc = (ctx && dY && dTy && dfc && dx && dst) ? 0 : 4;
        Vector st(nst, 0.0);
        void* s = ctx ? moihgp_dvec_ctx_stream(ctx) : nullptr;
        moihgp_gp* h = _moihgp->handle();
        if (!rc) rc = moihgp_dvec_upload(ctx, dY, flat.data(), T * M);
        if (!rc) rc = moihgp_dvec_upload(ctx, dx, zeros.data(), L * _dim);
        if (!rc) rc = moihgp_project_stream(h, MOIHGP_F64, dY, T, dTy, ld, s);
        if (!rc) rc = moihgp_forecast_stream(h, MOIHGP_F64, dTy, T, ld, dx, dx, &horizon, 1, dfc, ld, L * ld, MOIHGP_GAINS_KALMAN,
                                             reinterpret_cast<int*>(dst), s);
        if (!rc) rc = moihgp_unproject_stream(h, MOIHGP_F64, dfc, T, ld, dY, s);
        if (!rc) rc = moihgp_dvec_download(ctx, flat.data(), dY, T * M);
        if (!rc) rc = moihgp_dvec_download(ctx, st.data(), dst, nst);
        if (ctx) { moihgp_dvec_sync(ctx); moihgp_release_stream(h, s); }
        for (double* p : {dY, dTy, dfc, dx, dst}) if (p) moihgp_dvec_free(p);
        if (ctx) moihgp_dvec_ctx_del(ctx);
        if (rc) throw std::runtime_error(std::string("predictAhead: ") + moihgp_last_error());
        std::vector<int> status(2 * nst, 0);
        std::memcpy(status.data(), st.data(), sizeof(double) * nst);
        for (size_t l = 0; l < L; l++)
            if (status[l] != 0) throw std::runtime_error("predictAhead: the Kalman DARE of latent " + std::to_string(l) + " did not converge");
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) Yf[t][m] = flat[t * M + m];
        return Yf;
    }
    // (not in the reference) Fixed-lag smoothing of the series with the current parameters (include/moihgp.h moihgp_lagged_stream): element t is the
    // mean of every output at tick t given Y[0 .. min(t + lag, T - 1)], from a zero start state -- predictAhead(Y, 0) at lag 0, predictSmoothed(Y)
    // once lag >= T.  fp64 on the device: project_stream -> lagged_stream -> unproject_stream.  Throws std::invalid_argument for a lag outside
    // 0 .. 2^20 and std::runtime_error if a latent's Kalman DARE did not converge (status 1: its row would be NaN).  Missing outputs (NaN) are
    // projected as in predictSmoothed().
    std::vector<Vector> predictLagged(const std::vector<Vector>& Y, int lag) {
        if (lag < 0 || lag > (1 << 20)) throw std::invalid_argument("predictLagged: lag must be 0 .. 2^20");
        const size_t T = Y.size(), M = _num_output, L = _num_latent, ld = (T + 1) / 2 * 2;
        std::vector<Vector> Yl(T, Vector(M, 0.0));
        if (T == 0) return Yl;
        Vector flat(T * M), zeros(L * _dim, 0.0);
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) flat[t * M + m] = Y[t][m];
        moihgp_dvec_ctx* ctx = moihgp_dvec_ctx_new();
        const size_t nst = (L + 1) / 2;                             // status words: L ints in doubles' storage
        double *dY = moihgp_dvec_alloc(T * M), *dTy = moihgp_dvec_alloc(L * ld), *dyp = moihgp_dvec_alloc(L * ld), *dlg = moihgp_dvec_alloc(L * ld),
               *dx = moihgp_dvec_alloc(L * _dim), *dst = moihgp_dvec_alloc(nst);
        int rc = (ctx && dY && dTy && dyp && dlg && dx && dst) ? 0 : 4;
        Vector st(nst, 0.0);
        void* s = ctx ? moihgp_dvec_ctx_stream(ctx) : nullptr;
        moihgp_gp* h = _moihgp->handle();
        if (!rc) rc = moihgp_dvec_upload(ctx, dY, flat.data(), T * M);
        if (!rc) rc = moihgp_dvec_upload(ctx, dx, zeros.data(), L * _dim);
        if (!rc) rc = moihgp_project_stream(h, MOIHGP_F64, dY, T, dTy, ld, s);
        if (!rc) rc = moihgp_lagged_stream(h, MOIHGP_F64, dTy, T, ld, dx, dx, T, &lag, 1, dyp, dlg, ld, L * ld, reinterpret_cast<int*>(dst), s);
        if (!rc) rc = moihgp_unproject_stream(h, MOIHGP_F64, dlg, T, ld, dY, s);
        if (!rc) rc = moihgp_dvec_download(ctx, flat.data(), dY, T * M);
        if (!rc) rc = moihgp_dvec_download(ctx, st.data(), dst, nst);
        if (ctx) { moihgp_dvec_sync(ctx); moihgp_release_stream(h, s); }
        for (double* p : {dY, dTy, dyp, dlg, dx, dst}) if (p) moihgp_dvec_free(p);
        if (ctx) moihgp_dvec_ctx_del(ctx);
        if (rc) throw std::runtime_error(std::string("predictLagged: ") + moihgp_last_error());
        std::vector<int> status(2 * nst, 0);
        std::memcpy(status.data(), st.data(), sizeof(double) * nst);
        for (size_t l = 0; l < L; l++)
            if (status[l] != 0) throw std::runtime_error("predictLagged: the Kalman DARE of latent " + std::to_string(l) + " did not converge");
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) Yl[t][m] = flat[t * M + m];
        return Yl;
    }
    // (not in the reference) predict() as ONE pass over the whole series on the device (include/moihgp.h): project -> filter -> un-project in
    // fp64 from a zero start state, where predict() makes one gp32_step3 round trip per tick; element t is what predict() returns at tick t, to
    // rounding.  tiled = true runs the segment-major entries (moihgp_project_stream_tiled -> moihgp_filter_stream_tiled ->
    // moihgp_unproject_stream_tiled: the layout of the many-latent sweep, no copy between layouts); tiled = false the series-major ones.  The
    // two agree bit for bit above 1024 latents and to rounding below (there the series-major sweep splits a stream over wavefronts).
    // Limits against predict(): missing outputs (NaN) go through moihgp_project_stream's least-squares projection -- a tick with more than 64
    // missing outputs, or fewer than num_latent observed ones, is treated as missing as a whole (the filter predicts across it), where predict()
    // projects any tick with at least one observed output.  Stacked models refuse tiled = true (std::runtime_error, the library's return
    // code 3): their sweep takes series-major streams only.
    std::vector<Vector> predictStream(const std::vector<Vector>& Y, bool tiled = false) {
        const size_t T = Y.size(), M = _num_output, L = _num_latent, seg = 512 /* fp64 ticks per tile */;
        const size_t ld = (T + 1) / 2 * 2, n = tiled ? (T + seg - 1) / seg * L * seg : L * ld;
        std::vector<Vector> Yhat(T, Vector(M, 0.0));
        if (T == 0) return Yhat;
        Vector flat(T * M), zeros(L * _dim, 0.0);
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) flat[t * M + m] = Y[t][m];
        moihgp_dvec_ctx* ctx = moihgp_dvec_ctx_new();
        double *dY = moihgp_dvec_alloc(T * M), *dTy = moihgp_dvec_alloc(n), *dyh = moihgp_dvec_alloc(n), *dx = moihgp_dvec_alloc(L * _dim);
        int rc = (ctx && dY && dTy && dyh && dx) ? 0 : 4;
        void* s = ctx ? moihgp_dvec_ctx_stream(ctx) : nullptr;
        moihgp_gp* h = _moihgp->handle();
        if (!rc) rc = moihgp_dvec_upload(ctx, dY, flat.data(), T * M);
        if (!rc) rc = moihgp_dvec_upload(ctx, dx, zeros.data(), L * _dim);
        if (tiled) {
            if (!rc) rc = moihgp_project_stream_tiled(h, MOIHGP_F64, dY, T, dTy, s);
            if (!rc) rc = moihgp_filter_stream_tiled(h, MOIHGP_F64, dTy, T, dx, dx, dyh, nullptr, nullptr, s);
            if (!rc) rc = moihgp_unproject_stream_tiled(h, MOIHGP_F64, dyh, T, dY, s);
        } else {
            if (!rc) rc = moihgp_project_stream(h, MOIHGP_F64, dY, T, dTy, ld, s);
            if (!rc) rc = moihgp_filter_stream_v2(h, MOIHGP_F64, dTy, T, ld, dx, dx, dyh, ld, nullptr, nullptr, s);
            if (!rc) rc = moihgp_unproject_stream(h, MOIHGP_F64, dyh, T, ld, dY, s);
        }
        if (!rc) rc = moihgp_dvec_download(ctx, flat.data(), dY, T * M);
        const std::string err = rc ? moihgp_last_error() : "";
        if (ctx) { moihgp_dvec_sync(ctx); moihgp_release_stream(h, s); }
        for (double* p : {dY, dTy, dyh, dx}) if (p) moihgp_dvec_free(p);
        if (ctx) moihgp_dvec_ctx_del(ctx);
        if (rc) throw std::runtime_error("predictStream: " + err);
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) Yhat[t][m] = flat[t * M + m];
        return Yhat;
    }
    Vector getParams() { return _moihgp->getParams(); }
    size_t getNumParam() { return _num_param; }
    size_t getNumOutput() { return _num_output; }
    size_t getNumLatent() { return _num_latent; }
    size_t getNumIGPParam() { return _igp_num_param; }
    size_t getIGPDim() { return _dim; }
    size_t getNumData() { return _num_data; }
    RegressionObjective<StateSpace>& objective() { return *_obj; }   // (not in the reference)

private:
    MOIHGP<StateSpace>* _moihgp;
    bool _threading;
    double _dt;
    size_t _num_output, _num_latent, _num_data, _num_param, _igp_num_param, _dim;
    Vector _params, _lb, _ub;
    opt::LBFGSBParam _LBFGSB_param;
    opt::LBFGSBSolver* _solver;
    RegressionObjective<StateSpace>* _obj;
};

}  // namespace moihgp

#endif
