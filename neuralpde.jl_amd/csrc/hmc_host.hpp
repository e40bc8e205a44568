// hmc_host.hpp — the target set-up the two samplers share (hmc.cpp: pinn_hmc_init; hmc_chains.cpp: pinn_hmc_chains_init; only these two include
// it): the checks of the posterior's description, and the tables and constants of hmc::Args the kernels read it from.
#pragma once
#include "resident.hpp"
#include "hmc_rules.hpp"

namespace pe {

// "<who>: <what> must be positive and finite"
inline int hmc_need_positive(const char* who, const char* what, double x) {
    if (!(x > 0.0) || !std::isfinite(x)) return fail(std::string(who) + ": " + what + " must be positive and finite");
    return 0;
}

// the posterior's description against the handle: one standard deviation per loss term, the weight prior, the parameter priors of the last n_prior
// elements of theta.  inv_metric: pinn_hmc_chains_init's diagonal [p] (null: none to check), between the standard deviations and the weight prior,
// where that call has always checked it.
inline int hmc_check_target(const pinn_engine& E, const char* who, int64_t p, const double* stds, int k, const double* inv_metric, double nn_mu, double nn_sigma,
                            int n_prior, const int* prior_kind, const double* prior_mu, const double* prior_sigma) {
    const int K = (int)E.terms.size();
    if (k != K) return fail(std::string(who) + ": " + std::to_string(k) + " standard deviations for " + std::to_string(K) + " loss terms");
    for (int j = 0; j < K; ++j)
        if (!(stds[j] > 0.0) || !std::isfinite(stds[j])) return fail(std::string(who) + ": standard deviations must be positive");
    for (int64_t i = 0; inv_metric && i < p; ++i)
        if (hmc_need_positive(who, "the inverse metric", inv_metric[i])) return 1;
    if (!(nn_sigma > 0.0) || !std::isfinite(nn_sigma) || !std::isfinite(nn_mu)) return fail(std::string(who) + ": the weight prior needs a finite mean and a positive standard deviation");
    if (n_prior < 0 || n_prior > p) return fail(std::string(who) + ": n_prior must be in 0..P");
    if (n_prior > 0 && (!prior_kind || !prior_mu || !prior_sigma)) return fail(std::string(who) + ": null prior table");
    for (int j = 0; j < n_prior; ++j) {
        if (prior_kind[j] != hmc::PRIOR_NORMAL && prior_kind[j] != hmc::PRIOR_LOGNORMAL) return fail(std::string(who) + ": prior kind must be 0 (Normal) or 1 (LogNormal)");
        if (!(prior_sigma[j] > 0.0) || !std::isfinite(prior_sigma[j]) || !std::isfinite(prior_mu[j])) return fail(std::string(who) + ": a parameter prior needs a finite mu and a positive sigma");
    }
    return 0;
}

// The checked description on the device: d_tab = [prior mu | prior sigma | lik_c | lik_d | lik_n] and d_kind (the caller's state owns and frees both),
// `a` zeroed and its constants filled (P, K, nn, n_prior, nn_*, the table pointers), w = the evaluation's term weights N_k / (2 s_k^2).  The caller
// adds the pointers of its own state to `a`.
inline int hmc_target_setup(pinn_engine& E, const char* who, int64_t p, const double* stds, double nn_mu, double nn_sigma, int n_prior, const int* prior_kind,
                            const double* prior_mu, const double* prior_sigma, double*& d_tab, int*& d_kind, hmc::Args& a, std::vector<double>& w) {
    const int K = (int)E.terms.size();
    std::vector<double> tb((size_t)(2 * n_prior + 3 * K));
    d_tab = (double*)plat_malloc(sizeof(double) * tb.size());
    d_kind = (int*)plat_malloc(sizeof(int) * (size_t)std::max(n_prior, 1));
    if (!d_tab || !d_kind) return fail(std::string(who) + ": device allocation failed");
    w.resize((size_t)K);
    for (int j = 0; j < n_prior; ++j) { tb[j] = prior_mu[j]; tb[n_prior + j] = prior_sigma[j]; }
    for (int j = 0; j < K; ++j) {
        const double N = (double)E.terms[j].n, Nn = (double)E.terms[j].n_norm, sd = stds[j];
        w[j] = Nn / (2.0 * sd * sd);
        tb[2 * n_prior + j] = -0.5 * N * std::log(2.0 * 3.14159265358979323846) - N * std::log(sd);      // (loglik_from_sse's constants, same order of operations)
        tb[2 * n_prior + K + j] = 2.0 * sd * sd;
        tb[2 * n_prior + 2 * K + j] = Nn;
    }
    std::memset(&a, 0, sizeof a);
    a.P = (int)p; a.K = K; a.n_prior = n_prior; a.nn = (int)p - n_prior;
    a.nn_mu = nn_mu; a.nn_sigma = nn_sigma; a.nn_var = nn_sigma * nn_sigma;
    a.nn_const = (double)a.nn * (std::log(nn_sigma) + 0.5 * std::log(2.0 * 3.14159265358979323846));
    a.pr_mu = d_tab; a.pr_sigma = d_tab + n_prior; a.lik_c = d_tab + 2 * n_prior; a.lik_d = a.lik_c + K; a.lik_n = a.lik_d + K;
    a.pr_kind = d_kind;
    const std::vector<int> kinds(prior_kind, prior_kind + n_prior);
    if (plat_h2d(d_tab, tb.data(), sizeof(double) * tb.size(), E.stream) || (n_prior > 0 && plat_h2d(d_kind, kinds.data(), sizeof(int) * kinds.size(), E.stream)))
        return fail(std::string(who) + ": H2D copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());      // (the host images end with this call)
    return 0;
}

}  // namespace pe
