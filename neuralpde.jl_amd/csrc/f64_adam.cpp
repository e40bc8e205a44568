// f64_adam.cpp — the resident optimiser loop of the float64 evaluation mode (pinn_adam_* on a handle in float64 mode).
#include "f64_internal.hpp"

namespace pe {

// ---- the resident optimiser loop in float64 (pinn_adam_* on a handle in float64 mode; r05): theta, moments, points and every kernel of the
// iteration in double on the device — redraw (the fp32 samplers' points, converted on the device: the reference's StochasticTraining /
// QuasiRandomTraining(resampling = true) with Float64 parameters, src/training_strategies.jl:271-282, 365-389) -> evaluate -> Adam.
// The iterate has its OWN buffer (d_opt_theta): evaluations between two pinn_adam_steps calls (adaptive reweighting, callbacks) do not touch it ----
// Adam's bias corrections 1 / (1 - beta^t) at step t
static void adam_bias(double beta1, double beta2, long long t, double& c1, double& c2) {
    c1 = 1.0 / (1.0 - std::pow(beta1, (double)t));
    c2 = 1.0 / (1.0 - std::pow(beta2, (double)t));
}
int f64_adam_init(pinn_engine& E, const double* theta) {
    F64State& S = state(E);
    const int64_t P = E.ntheta;
    const int K = (int)E.terms.size();
    if (!S.d_m) {
        S.d_m = (double*)plat_malloc(sizeof(double) * P);
        S.d_v = (double*)plat_malloc(sizeof(double) * P);
        S.d_opt_theta = (double*)plat_malloc(sizeof(double) * (P + pk::F64S_PAD_THETA));
        if (S.d_opt_theta) plat_memset(S.d_opt_theta, 0, sizeof(double) * (P + pk::F64S_PAD_THETA), E.stream);
        S.d_w_over_n = (double*)plat_malloc(sizeof(double) * K);
        if (!S.d_m || !S.d_v || !S.d_w_over_n || !S.d_opt_theta) return fail("device allocation failed (float64 optimiser state)");
    }
    if (plat_h2d(S.d_opt_theta, theta, sizeof(double) * P, E.stream)) return fail("H2D copy of theta failed");
    plat_memset(S.d_m, 0, sizeof(double) * P, E.stream);
    plat_memset(S.d_v, 0, sizeof(double) * P, E.stream);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    S.opt_ready = true;
    E.opt_t = 0;
    return 0;
}
int f64_adam_get(pinn_engine& E, double* theta) {
    F64State& S = state(E);
    if (!S.opt_ready) return fail("pinn_adam_get: no float64 optimiser state (call pinn_adam_init after switching to precision f64)");
    if (plat_d2h(theta, S.d_opt_theta, sizeof(double) * E.ntheta, E.stream) || plat_sync(E.stream)) return fail("D2H copy failed");
    return 0;
}
int f64_adam_steps(pinn_engine& E, int nsteps, double lr, double beta1, double beta2, double eps, const float* term_w, double* loss_history) {
    pinn_engine* es[1] = {&E};
    return f64_adam_steps_comm(es, 1, nsteps, lr, beta1, beta2, eps, term_w, loss_history);
}
// the resident float64 Adam loop over a communicator (r06): per iteration every rank / device evaluates its shards, ONE all-reduce of [P + K] doubles,
// the identical update on every rank.  ndev == 1: a one-process-per-GPU communicator (or none); ndev > 1: the handles of a pinn_comm_init_all communicator
int f64_adam_steps_comm(pinn_engine** es, int ndev, int nsteps, double lr, double beta1, double beta2, double eps, const float* term_w, double* loss_history) {
    const int K = (int)es[0]->terms.size();
    const int P = (int)es[0]->ntheta;
    const std::vector<double> w = f64_widen_weights(term_w, K);
    std::vector<double> won(K);
    for (int k = 0; k < K; ++k) won[k] = w[k] / (double)es[0]->terms[k].n_norm;
    std::vector<double*> vec(ndev);
    for (int i = 0; i < ndev; ++i) {
        pinn_engine& E = *es[i];
        DeviceScope scope(E.device);
        F64State& S = state(E);
        if (!S.opt_ready) return fail("pinn_adam_steps: call pinn_adam_init first (float64 mode keeps its own optimiser state)");
        plat_h2d(S.d_w_over_n, won.data(), sizeof(double) * K, E.stream);
        if (!dev_grow(S.d_hist, S.hist_cap, (size_t)nsteps, E.stream)) return fail("device allocation failed (loss history)");
        vec[i] = S.d_grad;
    }
    const bool collective = ndev > 1 || es[0]->comm != nullptr;
    for (int s = 0; s < nsteps; ++s) {
        for (int i = 0; i < ndev; ++i) {
            pinn_engine& E = *es[i];
            DeviceScope scope(E.device);
            F64State& S = state(E);
            for (size_t t = 0; t < E.terms.size(); ++t) {
                Term& T = E.terms[t];
                if (T.sampler == 0) continue;
                redraw_term(E, T, false);                        // (engine.cpp: the fp32 sampler kernels, rank-specific seeds, draw counter advanced)
                if (f64_points_from_device(E, (int)t)) return 1;
            }
            if (f64_eval_device(E, S.d_opt_theta, S.d_grad, S.d_sumsq, w.data())) return 1;
        }
        if (collective && comm_all_reduce_f64(es, ndev, vec.data(), (int64_t)P + K)) return 1;
        for (int i = 0; i < ndev; ++i) {
            pinn_engine& E = *es[i];
            DeviceScope scope(E.device);
            F64State& S = state(E);
            ++E.opt_t;
            double c1, c2;
            adam_bias(beta1, beta2, E.opt_t, c1, c2);
            pk::launch_f64_adam_total(S.d_opt_theta, S.d_m, S.d_v, S.d_grad, P, lr, beta1, beta2, eps, c1, c2, S.d_hist, s, S.d_sumsq, S.d_w_over_n, K, E.stream);
        }
    }
    {
        pinn_engine& E0 = *es[0];
        DeviceScope scope(E0.device);
        F64State& S0 = state(E0);
        if (loss_history && plat_d2h(loss_history, S0.d_hist, sizeof(double) * nsteps, E0.stream)) return fail("D2H copy failed");
    }
    for (int i = 0; i < ndev; ++i) {
        DeviceScope scope(es[i]->device);
        if (plat_sync(es[i]->stream)) return fail(std::string("device error: ") + plat_last_error());
    }
    return 0;
}
// one Adam update of the float64 state from a caller-supplied host vector [gradient (P) | raw per-term sums (K)] (pinn_adam_apply in float64 mode)
int f64_adam_apply(pinn_engine& E, const double* grad_and_sums, double lr, double beta1, double beta2, double eps, const float* term_w, double* loss) {
    F64State& S = state(E);
    if (!S.opt_ready) return fail("pinn_adam_apply: call pinn_adam_init first (float64 mode keeps its own optimiser state)");
    const int K = (int)E.terms.size();
    const int P = (int)E.ntheta;
    if (plat_h2d(S.d_grad, grad_and_sums, sizeof(double) * P, E.stream)) return fail("H2D copy failed");
    ++E.opt_t;
    double c1, c2;
    adam_bias(beta1, beta2, E.opt_t, c1, c2);
    pk::launch_f64_adam(S.d_opt_theta, S.d_m, S.d_v, S.d_grad, P, lr, beta1, beta2, eps, c1, c2, E.stream);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    if (loss) {
        const std::vector<double> w = f64_widen_weights(term_w, K);
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += w[k] * grad_and_sums[P + k] / (double)E.terms[k].n_norm;
        *loss = s;
    }
    return 0;
}

}  // namespace pe
