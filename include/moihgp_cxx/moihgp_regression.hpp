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
        const size_t T = Y.size(), L = _num_latent, ld = (T + 1) / 2 * 2;
        if (T == 0) return std::vector<Vector>();
        return streamRoundTrip("predictSmoothed", Y, {L * ld, L * ld}, [&](StreamTrip& d) {
            int rc = d.project();
            if (!rc) rc = moihgp_smooth_stream(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, d.x, d.buf[1], ld, d.status, d.s);
            return rc ? rc : d.fetch(d.buf[1]);
        }, [](size_t l, int) { return "the Kalman DARE of latent " + std::to_string(l) + " did not converge"; })[0];
    }
    // (not in the reference) predictSmoothed() with exact edges (include/moihgp.h moihgp_smooth_stream_exact): the posterior mean of every output
    // at every tick given ALL of Y under the model's own prior on the first state -- for a series without missing outputs the GP posterior at
    // every tick, where predictSmoothed() is approximate near the start.  varY (if not null) receives, per entry of `ticks` (negative: counted
    // from the end), the posterior variance of the latent FUNCTION behind every output at that tick, without the observation noise:
    // (*varY)[k][m] = sum_l U[m][l]^2 S_l var[l][ticks[k]].  fp64 on the device: project_stream -> smooth_stream_exact -> unproject_stream.
    // Throws std::invalid_argument for a tick outside -T .. T - 1 and std::runtime_error on a non-zero status (1 Kalman DARE not converged, 3 a
    // latent's edges overlap in a series longer than 4096 ticks, 4 its edge tables failed).  Missing outputs (NaN) are projected as in
    // predictSmoothed(); no exactness is claimed near them.
    std::vector<Vector> predictSmoothedExact(const std::vector<Vector>& Y, const std::vector<long>& ticks = std::vector<long>(),
                                             std::vector<Vector>* varY = nullptr) {
        const size_t T = Y.size(), L = _num_latent, M = _num_output, ld = (T + 1) / 2 * 2;
        for (long t : ticks)
            if (t < -(long)T || t >= (long)T) throw std::invalid_argument("predictSmoothedExact: ticks must lie in -T .. T - 1");
        if (varY) varY->assign(ticks.size(), Vector(M, 0.0));
        if (T == 0) return std::vector<Vector>();
        Vector var(varY ? L * ld : 0);
        std::vector<Vector> Ys = streamRoundTrip("predictSmoothedExact", Y, {L * ld, L * ld, L * ld}, [&](StreamTrip& d) {
            int rc = d.project();
            if (!rc) rc = moihgp_smooth_stream_exact(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, d.buf[1], varY ? d.buf[2] : nullptr, ld, d.status, d.s);
            if (!rc && varY) rc = moihgp_dvec_download(d.ctx, var.data(), d.buf[2], L * ld);
            return rc ? rc : d.fetch(d.buf[1]);
        }, [](size_t l, int status) {
            return "latent " + std::to_string(l) + " has status " + std::to_string(status) +
                   (status == 1 ? " (the Kalman DARE did not converge)"
                    : status == 3 ? " (its edges overlap in a series longer than 4096 ticks)" : " (its edge tables failed)");
        })[0];
        if (varY) {
            const Vector prm = _moihgp->getParams();                 // [U row-major | S | ...]
            for (size_t k = 0; k < ticks.size(); k++) {
                const size_t t = (size_t)(ticks[k] < 0 ? ticks[k] + (long)T : ticks[k]);
                for (size_t m = 0; m < M; m++) {
                    double a = 0.0;
                    for (size_t l = 0; l < L; l++) a += prm[m * L + l] * prm[m * L + l] * (prm[M * L + l] * var[l * ld + t]);
                    (*varY)[k][m] = a;
                }
            }
        }
        return Ys;
    }
    // (not in the reference) The GP posterior across missing ticks (include/moihgp.h moihgp_posterior_stream): the posterior mean of every output at
    // every tick given ALL of Y, by the time-varying Kalman recursion from the model's own prior, with no update at a missing tick -- exact for
    // any pattern of wholly missing ticks, where predictSmoothed() and predictSmoothedExact() run on steady-state gains.  varY (if not null)
    // receives, per entry of `ticks` (negative: counted from the end), the posterior variance of the latent FUNCTION behind every output at that
    // tick, without the observation noise: (*varY)[k][m] = sum_l U[m][l]^2 S_l var[l][ticks[k]]; it widens inside a gap.  nll (if not null)
    // receives the latents' exact -log marginal likelihoods of their projected series [L].  fp64 on the device: project_stream ->
    // posterior_stream -> unproject_stream.  Throws std::invalid_argument for a tick outside -T .. T - 1 and std::runtime_error on a non-zero
    // status (5: a latent's recursion broke down).  Missing outputs (NaN) are projected as in predictSmoothed().
    std::vector<Vector> predictPosterior(const std::vector<Vector>& Y, const std::vector<long>& ticks = std::vector<long>(),
                                         std::vector<Vector>* varY = nullptr, Vector* nll = nullptr) {
        const size_t T = Y.size(), L = _num_latent, M = _num_output, ld = (T + 1) / 2 * 2;
        for (long t : ticks)
            if (t < -(long)T || t >= (long)T) throw std::invalid_argument("predictPosterior: ticks must lie in -T .. T - 1");
        if (varY) varY->assign(ticks.size(), Vector(M, 0.0));
        if (nll) nll->assign(L, 0.0);
        if (T == 0) return std::vector<Vector>();
        Vector var(varY ? L * ld : 0);
        std::vector<Vector> Ys = streamRoundTrip("predictPosterior", Y, {L * ld, L * ld, L * ld, L}, [&](StreamTrip& d) {
            int rc = d.project();
            if (!rc) rc = moihgp_posterior_stream(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, nullptr, d.buf[1], varY ? d.buf[2] : nullptr, ld,
                                                  nll ? d.buf[3] : nullptr, d.status, d.s);
            if (!rc && varY) rc = moihgp_dvec_download(d.ctx, var.data(), d.buf[2], L * ld);
            if (!rc && nll) rc = moihgp_dvec_download(d.ctx, nll->data(), d.buf[3], L);
            return rc ? rc : d.fetch(d.buf[1]);
        }, [](size_t l, int status) {
            return "latent " + std::to_string(l) + " has status " + std::to_string(status) + " (its recursion broke down)";
        })[0];
        if (varY) {
            const Vector prm = _moihgp->getParams();                 // [U row-major | S | ...]
            for (size_t k = 0; k < ticks.size(); k++) {
                const size_t t = (size_t)(ticks[k] < 0 ? ticks[k] + (long)T : ticks[k]);
                for (size_t m = 0; m < M; m++) {
                    double a = 0.0;
                    for (size_t l = 0; l < L; l++) a += prm[m * L + l] * prm[m * L + l] * (prm[M * L + l] * var[l * ld + t]);
                    (*varY)[k][m] = a;
                }
            }
        }
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
        const size_t T = Y.size(), L = _num_latent, ld = (T + 1) / 2 * 2, S = nsamples;
        if (T == 0) return std::vector<std::vector<Vector>>(S);
        return streamRoundTrip("sampleSmoothed", Y, {L * ld, L * ld, S * L * ld}, [&](StreamTrip& d) {
            int rc = d.project();
            if (!rc) rc = moihgp_sample_stream(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, d.x, S, seed, 0, 0, d.buf[1], ld, d.buf[2], L * ld, d.status, d.s);
            for (size_t k = 0; k < S && !rc; k++) rc = d.fetch(d.buf[2] + k * L * ld);
            return rc;
        }, [](size_t l, int status) {
            return "latent " + std::to_string(l) + " has status " + std::to_string(status) +
                   (status == 1 ? " (the Kalman DARE did not converge)" : " (the sampling realization was not accepted)");
        });
    }
    // (not in the reference) Forecasts `horizon` ticks ahead at every tick of the series with the current parameters (include/moihgp.h
    // moihgp_forecast_stream, Kalman-form gains): element t is the mean of every output at tick t + horizon given Y[0..t], from a zero start
    // state, where the reference would call step(x, y) and then `horizon` prediction-only steps per tick.  fp64 on the device:
    // project_stream -> forecast_stream -> unproject_stream.  Throws std::invalid_argument for a horizon outside 0 .. 2^20 and std::runtime_error
    // if a latent's Kalman DARE did not converge (status 1: its row would be NaN).  Missing outputs (NaN) are projected as in predictSmoothed().
    std::vector<Vector> predictAhead(const std::vector<Vector>& Y, int horizon) {
        if (horizon < 0 || horizon > (1 << 20)) throw std::invalid_argument("predictAhead: horizon must be 0 .. 2^20");
        const size_t T = Y.size(), L = _num_latent, ld = (T + 1) / 2 * 2;
        if (T == 0) return std::vector<Vector>();
        return streamRoundTrip("predictAhead", Y, {L * ld, L * ld}, [&](StreamTrip& d) {
            int rc = d.project();
            if (!rc) rc = moihgp_forecast_stream(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, d.x, &horizon, 1, d.buf[1], ld, L * ld, MOIHGP_GAINS_KALMAN, d.status, d.s);
            return rc ? rc : d.fetch(d.buf[1]);
        }, [](size_t l, int) { return "the Kalman DARE of latent " + std::to_string(l) + " did not converge"; })[0];
    }
    // (not in the reference) Seeded joint draws of the n ticks beyond the series with the current parameters (include/moihgp.h
    // moihgp_forecast_paths): element [s][j] is draw s of every output's observation at tick T + j given ALL of Y -- whole trajectories whose
    // covariance across horizons is the GP predictive one, inside the mixing's span and with the latents' noise -- from a zero start state.  The
    // same seed gives the same paths; they are not jointly consistent with sampleSmoothed() of the same series.  fp64 on the device:
    // project_stream -> the end state with the Kalman gains (forecast_scores, which writes no plane) -> forecast_paths -> unproject_stream per
    // sample.  Throws std::invalid_argument for an empty series, n outside 0 .. 2^20 or nsamples outside 1 .. 65535, and std::runtime_error if a
    // latent's Kalman DARE did not converge (status 1: its rows would be NaN).  Missing outputs (NaN) are projected as in predictSmoothed().
    std::vector<std::vector<Vector>> samplePathsAhead(const std::vector<Vector>& Y, size_t n, size_t nsamples, unsigned long long seed = 0) {
        if (nsamples < 1 || nsamples > 65535) throw std::invalid_argument("samplePathsAhead: nsamples must be 1 .. 65535");
        if (n > ((size_t)1 << 20)) throw std::invalid_argument("samplePathsAhead: n must be 0 .. 2^20");
        if (Y.empty()) throw std::invalid_argument("samplePathsAhead: the series is empty");
        const size_t T = Y.size(), L = _num_latent, M = _num_output, ld = (T + 1) / 2 * 2, ldn = (n + 1) / 2 * 2, S = nsamples;
        if (n == 0) return std::vector<std::vector<Vector>>(S);
        const int one = 1;
        return streamRoundTrip("samplePathsAhead", Y, {L * ld, 2 * L, S * L * ldn, n * M}, [&](StreamTrip& d) {
            int rc = d.project();
            if (!rc) rc = moihgp_forecast_scores(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, d.x, &one, 1, 0, MOIHGP_GAINS_KALMAN,
                                                 reinterpret_cast<long long*>(d.buf[1]), nullptr, d.buf[1] + L, nullptr, d.status, d.s);
            if (!rc) rc = moihgp_forecast_paths(d.h, MOIHGP_F64, d.x, nullptr, nullptr, n, 0, S, seed, 0, 0, d.buf[2], ldn, L * ldn, d.status, d.s);
            for (size_t k = 0; k < S && !rc; k++) rc = d.fetchAhead(d.buf[2] + k * L * ldn, n, ldn, d.buf[3]);
            return rc;
        }, [](size_t l, int) { return "the Kalman DARE of latent " + std::to_string(l) + " did not converge"; });
    }
    // (not in the reference) Fixed-lag smoothing of the series with the current parameters (include/moihgp.h moihgp_lagged_stream): element t is the
    // mean of every output at tick t given Y[0 .. min(t + lag, T - 1)], from a zero start state -- predictAhead(Y, 0) at lag 0, predictSmoothed(Y)
    // once lag >= T.  fp64 on the device: project_stream -> lagged_stream -> unproject_stream.  Throws std::invalid_argument for a lag outside
    // 0 .. 2^20 and std::runtime_error if a latent's Kalman DARE did not converge (status 1: its row would be NaN).  Missing outputs (NaN) are
    // projected as in predictSmoothed().
    std::vector<Vector> predictLagged(const std::vector<Vector>& Y, int lag) {
        if (lag < 0 || lag > (1 << 20)) throw std::invalid_argument("predictLagged: lag must be 0 .. 2^20");
        const size_t T = Y.size(), L = _num_latent, ld = (T + 1) / 2 * 2;
        if (T == 0) return std::vector<Vector>();
        return streamRoundTrip("predictLagged", Y, {L * ld, L * ld, L * ld}, [&](StreamTrip& d) {
            int rc = d.project();
            if (!rc) rc = moihgp_lagged_stream(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, d.x, T, &lag, 1, d.buf[1], d.buf[2], ld, L * ld, d.status, d.s);
            return rc ? rc : d.fetch(d.buf[2]);
        }, [](size_t l, int) { return "the Kalman DARE of latent " + std::to_string(l) + " did not converge"; })[0];
    }
    // (not in the reference) Off-grid smoothing of the series with the current parameters (include/moihgp.h moihgp_interp_stream): element t is the
    // mean of every output at time (t + frac) dt given ALL of Y, from a zero start state -- predictSmoothed(Y) at frac 0; the last element is the
    // forecast frac dt past the end.  fp64 on the device: project_stream -> interp_stream -> unproject_stream.  Throws std::invalid_argument for a
    // frac outside [0, 1) (NaN included) and std::runtime_error if a latent's Kalman DARE did not converge (status 1: its row would be NaN).
    // Missing outputs (NaN) are projected as in predictSmoothed().
    std::vector<Vector> predictBetween(const std::vector<Vector>& Y, double frac) {
        if (!(frac >= 0.0 && frac < 1.0)) throw std::invalid_argument("predictBetween: frac must be in [0, 1)");
        const size_t T = Y.size(), L = _num_latent, ld = (T + 1) / 2 * 2;
        if (T == 0) return std::vector<Vector>();
        return streamRoundTrip("predictBetween", Y, {L * ld, L * ld, L * ld}, [&](StreamTrip& d) {
            int rc = d.project();
            if (!rc) rc = moihgp_interp_stream(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, d.x, &frac, 1, d.buf[1], d.buf[2], ld, L * ld, d.status, d.s);
            return rc ? rc : d.fetch(d.buf[2]);
        }, [](size_t l, int) { return "the Kalman DARE of latent " + std::to_string(l) + " did not converge"; })[0];
    }
    // (not in the reference) Rate of change of the series with the current parameters (include/moihgp.h moihgp_slope_stream): element t is the
    // derivative with respect to time (the unit of dt) of the mean of every output at time (t + frac) dt, from a zero start state -- given ALL of Y,
    // or with past = true given the ticks up to t only (at frac 0 the real-time slope estimate).  fp64 on the device: project_stream ->
    // slope_stream -> unproject_stream.  Throws as predictBetween does.
    std::vector<Vector> predictSlope(const std::vector<Vector>& Y, double frac = 0.0, bool past = false) {
        if (!(frac >= 0.0 && frac < 1.0)) throw std::invalid_argument("predictSlope: frac must be in [0, 1)");
        const size_t T = Y.size(), L = _num_latent, ld = (T + 1) / 2 * 2;
        if (T == 0) return std::vector<Vector>();
        return streamRoundTrip("predictSlope", Y, {L * ld, L * ld, L * ld}, [&](StreamTrip& d) {
            int rc = d.project();
            if (!rc) rc = moihgp_slope_stream(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, d.x, &frac, 1, past ? MOIHGP_SLOPE_PAST : MOIHGP_SLOPE_ALL, d.buf[1],
                                              d.buf[2], ld, L * ld, d.status, d.s);
            return rc ? rc : d.fetch(d.buf[2]);
        }, [](size_t l, int) { return "the Kalman DARE of latent " + std::to_string(l) + " did not converge"; })[0];
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
        const size_t T = Y.size(), L = _num_latent, seg = 512 /* fp64 ticks per tile */;
        const size_t ld = (T + 1) / 2 * 2, n = tiled ? (T + seg - 1) / seg * L * seg : L * ld;
        if (T == 0) return std::vector<Vector>();
        return streamRoundTrip("predictStream", Y, {n, n}, [&](StreamTrip& d) {
            int rc;
            if (tiled) {
                rc = moihgp_project_stream_tiled(d.h, MOIHGP_F64, d.Y, T, d.buf[0], d.s);
                if (!rc) rc = moihgp_filter_stream_tiled(d.h, MOIHGP_F64, d.buf[0], T, d.x, d.x, d.buf[1], nullptr, nullptr, d.s);
                if (!rc) rc = moihgp_unproject_stream_tiled(d.h, MOIHGP_F64, d.buf[1], T, d.Y, d.s);
                return rc ? rc : d.take();
            }
            rc = d.project();
            if (!rc) rc = moihgp_filter_stream_v2(d.h, MOIHGP_F64, d.buf[0], T, ld, d.x, d.x, d.buf[1], ld, nullptr, nullptr, d.s);
            return rc ? rc : d.fetch(d.buf[1]);
        }, [](size_t, int) { return std::string(); })[0];      // (the filter reports no status: the words stay zero)
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
    // One device round trip of the whole-stream methods above, as its sweep sees it: the handle, the context's stream, and the device vectors --
    // Y [T][M] the observations, x [L][dim] a zero start state, status L zeroed ints, buf[] the vectors the call named by size (buf[0]: the stream).
    // Every call of take() adds one [T][M] plane to the method's result.
    struct StreamTrip {
        moihgp_gp* h; moihgp_dvec_ctx* ctx; void* s;
        size_t T, M, ld;
        double *Y, *x; int* status;
        std::vector<double*> buf;
        Vector flat;
        std::vector<std::vector<Vector>> planes;
        int project() { return moihgp_project_stream(h, MOIHGP_F64, Y, T, buf[0], ld, s); }          // Y -> buf[0], series-major rows of ld
        int take() { return takeFrom(Y, T); }                                                        // Y -> the next plane of the result
        int takeFrom(const double* src, size_t n) {                                                   // n ticks [n][M] at src -> the next plane
            if (flat.size() < n * M) flat.resize(n * M);
            if (int rc = moihgp_dvec_download(ctx, flat.data(), src, n * M)) return rc;
            planes.push_back(std::vector<Vector>(n, Vector(M)));
            for (size_t t = 0; t < n; t++) for (size_t m = 0; m < M; m++) planes.back()[t][m] = flat[t * M + m];
            return 0;
        }
        int fetch(const double* rows) {                                                               // un-project series-major rows, then take()
            const int rc = moihgp_unproject_stream(h, MOIHGP_F64, rows, T, ld, Y, s);
            return rc ? rc : take();
        }
        int fetchAhead(const double* rows, size_t n, size_t ldn, double* Yn) {                        // ... n ticks past the series, through Yn [n][M]
            const int rc = moihgp_unproject_stream(h, MOIHGP_F64, rows, n, ldn, Yn, s);
            return rc ? rc : takeFrom(Yn, n);
        }
    };
    // The round trip itself, fp64 from a zero start state: flatten Y, create the context and the device vectors (Y, x, the status words, and one per
    // entry of `sizes`, in doubles), upload, run sweep(trip) -- which projects, issues the method's sweep and takes the result plane by plane --
    // download the status words, free everything on every path, then throw: on a non-zero return code with moihgp_last_error() as it stood when
    // the failure was seen (the cleanup calls may overwrite it), on a non-zero status word of latent l with statusText(l, word).
    template <typename Sweep, typename StatusText>
    std::vector<std::vector<Vector>> streamRoundTrip(const char* who, const std::vector<Vector>& Y, std::initializer_list<size_t> sizes, Sweep&& sweep,
                                                     StatusText&& statusText) {
        const size_t T = Y.size(), M = _num_output, L = _num_latent, nst = (L + 1) / 2;               // status words: L ints in doubles' storage
        StreamTrip d{_moihgp->handle(), moihgp_dvec_ctx_new(), nullptr, T, M, (T + 1) / 2 * 2, nullptr, nullptr, nullptr, {}, Vector(T * M), {}};
        for (size_t t = 0; t < T; t++) for (size_t m = 0; m < M; m++) d.flat[t * M + m] = Y[t][m];
        Vector zeros(L * _dim, 0.0), st(nst, 0.0);
        std::vector<double*> all = {d.Y = moihgp_dvec_alloc(T * M), d.x = moihgp_dvec_alloc(L * _dim), moihgp_dvec_alloc(nst)};
        d.status = reinterpret_cast<int*>(all[2]);
        for (size_t n : sizes) { d.buf.push_back(moihgp_dvec_alloc(n)); all.push_back(d.buf.back()); }
        int rc = d.ctx ? 0 : 4;
        for (double* p : all) if (!p) rc = 4;
        if (d.ctx) d.s = moihgp_dvec_ctx_stream(d.ctx);
        if (!rc) rc = moihgp_dvec_upload(d.ctx, d.Y, d.flat.data(), T * M);
        if (!rc) rc = moihgp_dvec_upload(d.ctx, d.x, zeros.data(), L * _dim);
        if (!rc) rc = moihgp_dvec_upload(d.ctx, all[2], st.data(), nst);
        if (!rc) rc = sweep(d);
        if (!rc) rc = moihgp_dvec_download(d.ctx, st.data(), all[2], nst);
        const std::string err = rc ? moihgp_last_error() : "";
        if (d.ctx) { moihgp_dvec_sync(d.ctx); moihgp_release_stream(d.h, d.s); }
        for (double* p : all) if (p) moihgp_dvec_free(p);
        if (d.ctx) moihgp_dvec_ctx_del(d.ctx);
        if (rc) throw std::runtime_error(std::string(who) + ": " + err);
        std::vector<int> status(2 * nst, 0);
        std::memcpy(status.data(), st.data(), sizeof(double) * nst);
        for (size_t l = 0; l < L; l++)
            if (status[l] != 0) throw std::runtime_error(std::string(who) + ": " + statusText(l, status[l]));
        return std::move(d.planes);
    }

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
