// hmc.cpp — resident HMC (pinn_hmc_init / _set_metric / _draws / _get): the transition loop of
// neuralpde.jl_amd/bpinn.py `_hmc` with the chain on the device; and its warm-up (pinn_hmc_find_stepsize / _warmup; section 4.11): the initial
// step-size search, dual averaging and the windowed diagonal metric of `_hmc_device`.
// A leapfrog step = the handle's resident evaluation (resident.hpp: ResidentEval) + ONE update launch (hmc_kernels.hpp); nothing is read back
// before the single download that ends pinn_hmc_draws.
// pinn_nuts_draws (section 4.14): No-U-Turn transitions of the same chain — slots of one evaluation + one state-machine launch
// (nuts_kernels.hpp), queued in chunks of "nuts_chunk"; the control block is all the host reads between chunks.
// The state has buffers of its own: evaluations and optimiser runs between two calls do not touch the chain, and the chain does not touch them.
#include "resident.hpp"
#include "nuts_kernels.hpp"

using namespace pe;

struct pe::HmcState {
    hmc::Args a;
    ResidentEval ev;                     // term weights N_k / (2 s_k^2), as pinn_loglik_grad forms them
    double* d_state = nullptr;           // [6 P + SC_COUNT]: th_cur | th_prop | r | g_cur | g_prop | minv | scalars
    double* d_tab = nullptr;             // [3 n_prior + 3 K]: prior mu | prior sigma | lik_c | lik_d | lik_n (+ kinds as ints in d_kind)
    int* d_kind = nullptr;
    double* d_samples = nullptr; double* d_stat = nullptr; double* d_mom = nullptr; double* d_uni = nullptr;
    double* d_r0 = nullptr; double* d_steps = nullptr;      // the search's momentum [P]; the warm-up's step sizes [n_adapts + 1]
    size_t samples_cap = 0, stat_cap = 0, mom_cap = 0, uni_cap = 0, r0_cap = 0, steps_cap = 0;
    unsigned long long draws = 0;        // draw counter of the generator (advanced per completed draw, whatever supplies momenta and uniforms)
    // NUTS (allocated by the first pinn_nuts_draws)
    double* d_tree = nullptr;            // [(12 + 2 MAX_DEPTH) P]: edges (theta, r, g) x 2 | candidates (theta, g) x 2 | rho | rho_sub | r_ck | rho_ck
    nuts::Ctl* d_nctl = nullptr;
    int* d_istat = nullptr;              // [3 ndraws]: tree_depth | n_leapfrog | divergent
    size_t istat_cap = 0;
};

namespace {

void hmc_release(HmcState* H) {
    if (!H) return;
    H->ev.release();
    plat_free(H->d_state); plat_free(H->d_tab); plat_free(H->d_kind);
    plat_free(H->d_samples); plat_free(H->d_stat); plat_free(H->d_mom); plat_free(H->d_uni);
    plat_free(H->d_r0); plat_free(H->d_steps);
    plat_free(H->d_tree); plat_free(H->d_nctl); plat_free(H->d_istat);
    delete H;
}

// what every pinn_hmc_* call after init checks first; leaves the handle as it is
int hmc_ready(pinn_engine& E, const char* who) {
    if (!E.hmc) return fail(std::string(who) + ": no sampler state (call pinn_hmc_init first)");
    return E.hmc->ev.ready(E, who, "pinn_hmc_init");
}
int hmc_refuse_target(pinn_engine& E, const char* who) {
    return resident_refuse_target(E, who, "the resident sampler runs single-device chains only", "HMC needs a fixed target");
}
// the update launch after an evaluation at the proposal (from_eval), or the opening half kick
void hmc_leap(pinn_engine& E, HmcState& H, bool from_eval, double kick, double eps, int drift) {
    if (H.ev.f64) hmc::launch_leap<double>(H.a, from_eval ? H.ev.out<double>() : nullptr, kick, eps, drift, E.stream);
    else hmc::launch_leap<float>(H.a, from_eval ? H.ev.out<float>() : nullptr, kick, eps, drift, E.stream);
}
// the same with the step size read from the scalar block on the device: kick = kfac * eps
void hmc_leap_dev(pinn_engine& E, HmcState& H, bool from_eval, double kfac, int drift) {
    if (H.ev.f64) hmc::launch_leap_dev<double>(H.a, from_eval ? H.ev.out<double>() : nullptr, kfac, drift, E.stream);
    else hmc::launch_leap_dev<float>(H.a, from_eval ? H.ev.out<float>() : nullptr, kfac, drift, E.stream);
}

}  // namespace

void pe::hmc_free(pinn_engine& E) {
    hmc_release(E.hmc);
    E.hmc = nullptr;
}

extern "C" {

int pinn_hmc_init(pinn_handle h, const double* theta, int64_t p, const double* stds, int k, double nn_mu, double nn_sigma,
                  int n_prior, const int* prior_kind, const double* prior_mu, const double* prior_sigma) {
    const char* who = "pinn_hmc_init";
    if (!h || !theta || !stds) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    const int K = (int)E.terms.size();
    if (k != K) return fail(std::string(who) + ": " + std::to_string(k) + " standard deviations for " + std::to_string(K) + " loss terms");
    for (int j = 0; j < K; ++j)
        if (!(stds[j] > 0.0) || !std::isfinite(stds[j])) return fail(std::string(who) + ": standard deviations must be positive");
    if (!(nn_sigma > 0.0) || !std::isfinite(nn_sigma) || !std::isfinite(nn_mu)) return fail(std::string(who) + ": the weight prior needs a finite mean and a positive standard deviation");
    if (n_prior < 0 || n_prior > p) return fail(std::string(who) + ": n_prior must be in 0..P");
    if (n_prior > 0 && (!prior_kind || !prior_mu || !prior_sigma)) return fail(std::string(who) + ": null prior table");
    for (int j = 0; j < n_prior; ++j) {
        if (prior_kind[j] != hmc::PRIOR_NORMAL && prior_kind[j] != hmc::PRIOR_LOGNORMAL) return fail(std::string(who) + ": prior kind must be 0 (Normal) or 1 (LogNormal)");
        if (!(prior_sigma[j] > 0.0) || !std::isfinite(prior_sigma[j]) || !std::isfinite(prior_mu[j])) return fail(std::string(who) + ": a parameter prior needs a finite mu and a positive sigma");
    }
    if (hmc_refuse_target(E, who)) return 1;
    DeviceScope scope(E.device);
    if (!E.f64 && ensure_points(E)) return 1;
    const size_t P = (size_t)p;
    std::unique_ptr<HmcState, void (*)(HmcState*)> H(new HmcState, hmc_release);
    H->d_state = (double*)plat_malloc(sizeof(double) * (6 * P + hmc::SC_COUNT));
    H->d_tab = (double*)plat_malloc(sizeof(double) * (size_t)(2 * n_prior + 3 * K));
    H->d_kind = (int*)plat_malloc(sizeof(int) * (size_t)std::max(n_prior, 1));
    if (!H->d_state || !H->d_tab || !H->d_kind) return fail(std::string(who) + ": device allocation failed");
    // tables: prior, likelihood constants, the evaluation's term weights
    std::vector<double> tb((size_t)(2 * n_prior + 3 * K)), w((size_t)K);
    for (int j = 0; j < n_prior; ++j) { tb[j] = prior_mu[j]; tb[n_prior + j] = prior_sigma[j]; }
    for (int j = 0; j < K; ++j) {
        const double N = (double)E.terms[j].n, Nn = (double)E.terms[j].n_norm, sd = stds[j];
        w[j] = Nn / (2.0 * sd * sd);
        tb[2 * n_prior + j] = -0.5 * N * std::log(2.0 * 3.14159265358979323846) - N * std::log(sd);      // (loglik_from_sse's constants, same order of operations)
        tb[2 * n_prior + K + j] = 2.0 * sd * sd;
        tb[2 * n_prior + 2 * K + j] = Nn;
    }
    if (H->ev.init(E, who, w.data(), K)) return 1;
    const bool f64 = H->ev.f64;
    hmc::Args& a = H->a;
    std::memset(&a, 0, sizeof a);
    a.P = (int)p; a.K = K; a.n_prior = n_prior; a.nn = (int)p - n_prior;
    a.sse_roundtrip = f64 ? 1 : 0;
    a.th_cur = H->d_state; a.th_prop = a.th_cur + P; a.r = a.th_prop + P; a.g_cur = a.r + P; a.g_prop = a.g_cur + P;
    double* minv = a.g_prop + P;
    a.minv = minv; a.sc = minv + P;
    a.nn_mu = nn_mu; a.nn_sigma = nn_sigma; a.nn_var = nn_sigma * nn_sigma;
    a.nn_const = (double)a.nn * (std::log(nn_sigma) + 0.5 * std::log(2.0 * 3.14159265358979323846));
    double* tab = H->d_tab;
    a.pr_mu = tab; a.pr_sigma = tab + n_prior; a.lik_c = tab + 2 * n_prior; a.lik_d = a.lik_c + K; a.lik_n = a.lik_d + K;
    a.pr_kind = H->d_kind;
    a.th_eval64 = H->ev.theta64(E);
    a.th_eval32 = H->ev.theta32();
    // host image of the state: theta twice, zero momentum and gradients, unit metric
    std::vector<double> st(6 * P + hmc::SC_COUNT, 0.0);
    std::copy(theta, theta + P, st.begin());
    std::copy(theta, theta + P, st.begin() + P);
    std::fill(st.begin() + 5 * P, st.begin() + 6 * P, 1.0);
    std::vector<int> kinds(prior_kind, prior_kind + n_prior);
    if (plat_h2d(H->d_state, st.data(), sizeof(double) * st.size(), E.stream) || plat_h2d(H->d_tab, tb.data(), sizeof(double) * tb.size(), E.stream) ||
        (n_prior > 0 && plat_h2d(H->d_kind, kinds.data(), sizeof(int) * kinds.size(), E.stream)))
        return fail(std::string(who) + ": H2D copy failed");
    if (f64) {
        if (plat_h2d(a.th_eval64, theta, sizeof(double) * P, E.stream)) return fail(std::string(who) + ": H2D copy failed");
    } else {
        std::vector<float> t32(P);
        for (size_t i = 0; i < P; ++i) t32[i] = (float)theta[i];
        if (plat_h2d(a.th_eval32, t32.data(), sizeof(float) * P, E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": H2D copy failed");
    }
    // logp and its gradient at theta: one evaluation, the update kernel with a zero kick (gradient only), the energy kernel at zero momentum
    if (H->ev.eval(E)) return 1;
    hmc_leap(E, *H, true, 0.0, 0.0, 0);
    hmc::launch_energy(a, 1, H->ev.sums(P), E.stream);
    plat_d2d(a.g_cur, a.g_prop, sizeof(double) * P, E.stream);
    plat_d2d(a.sc + hmc::SC_LP_CUR, a.sc + hmc::SC_LP_PROP, sizeof(double), E.stream);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    hmc_free(E);
    E.hmc = H.release();
    return 0;
}

int pinn_hmc_set_metric(pinn_handle h, const double* inv_metric, int64_t p) {
    const char* who = "pinn_hmc_set_metric";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p)) return 1;
    HmcState& H = *E.hmc;
    std::vector<double> m((size_t)p, 1.0);
    for (int64_t i = 0; inv_metric && i < p; ++i) {
        if (!(inv_metric[i] > 0.0) || !std::isfinite(inv_metric[i])) return fail(std::string(who) + ": the inverse metric must be positive and finite");
        m[(size_t)i] = inv_metric[i];
    }
    DeviceScope scope(E.device);
    if (plat_h2d((double*)H.a.minv, m.data(), sizeof(double) * (size_t)p, E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": H2D copy failed");
    return 0;
}

int pinn_hmc_draws(pinn_handle h, int ndraws, int n_leapfrog, double eps, uint64_t seed, const double* momenta, const double* uniforms,
                   double* samples, int64_t p, double* accept_prob, double* logp) {
    const char* who = "pinn_hmc_draws";
    if (!h || !accept_prob || !logp) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p) || hmc_refuse_target(E, who)) return 1;
    if (ndraws < 1) return fail(std::string(who) + ": ndraws must be at least 1");
    if (n_leapfrog < 1) return fail(std::string(who) + ": n_leapfrog must be at least 1");
    if (!(eps > 0.0) || !std::isfinite(eps)) return fail(std::string(who) + ": the step size eps must be positive and finite");
    HmcState& H = *E.hmc;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    const size_t P = (size_t)p, nd = (size_t)ndraws;
    if ((samples && !dev_grow(H.d_samples, H.samples_cap, nd * P, E.stream)) || !dev_grow(H.d_stat, H.stat_cap, 2 * nd, E.stream) ||
        (momenta && !dev_grow(H.d_mom, H.mom_cap, nd * P, E.stream)) || (uniforms && !dev_grow(H.d_uni, H.uni_cap, nd, E.stream)))
        return fail(std::string(who) + ": device allocation failed");
    if ((momenta && plat_h2d(H.d_mom, momenta, sizeof(double) * nd * P, E.stream)) || (uniforms && plat_h2d(H.d_uni, uniforms, sizeof(double) * nd, E.stream)))
        return fail(std::string(who) + ": H2D copy failed");
    double* d_acc = H.d_stat;
    double* d_lp = H.d_stat + nd;
    for (int d = 0; d < ndraws; ++d) {
        const unsigned ctr = (unsigned)H.draws;
        hmc::launch_momentum(H.a, momenta ? H.d_mom + (size_t)d * P : nullptr, seed, ctr, E.stream);
        hmc::launch_energy(H.a, 0, nullptr, E.stream);
        hmc_leap(E, H, false, 0.5 * eps, eps, 1);
        for (int s = 0; s < n_leapfrog; ++s) {
            if (H.ev.eval(E)) return 1;                 // (the current state only changes in the accept launch: a failed call leaves the chain at its last completed draw)
            const bool last = s == n_leapfrog - 1;
            hmc_leap(E, H, true, last ? 0.5 * eps : eps, eps, last ? 0 : 1);
        }
        hmc::launch_energy(H.a, 1, H.ev.sums(P), E.stream);
        hmc::launch_accept(H.a, d, uniforms ? H.d_uni : nullptr, seed, ctr, samples ? H.d_samples : nullptr, d_acc, d_lp, E.stream);
        ++H.draws;
    }
    if ((samples && plat_d2h(samples, H.d_samples, sizeof(double) * nd * P, E.stream)) || plat_d2h(accept_prob, d_acc, sizeof(double) * nd, E.stream) ||
        plat_d2h(logp, d_lp, sizeof(double) * nd, E.stream))
        return fail(std::string(who) + ": D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

int pinn_nuts_draws(pinn_handle h, int ndraws, int max_depth, double eps, double delta_max, uint64_t seed, const double* normals, const double* uniforms,
                    double* samples, int64_t p, double* accept_stat, double* logp, int* tree_depth, int* n_leapfrog, int* divergent) {
    const char* who = "pinn_nuts_draws";
    if (!h || !accept_stat || !logp || !tree_depth || !n_leapfrog || !divergent) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p) || hmc_refuse_target(E, who)) return 1;
    if (ndraws < 1) return fail(std::string(who) + ": ndraws must be at least 1");
    if (max_depth < 1 || max_depth > nuts::MAX_DEPTH) return fail(std::string(who) + ": max_depth must be in 1.." + std::to_string(nuts::MAX_DEPTH));
    if (!(eps > 0.0) || !std::isfinite(eps)) return fail(std::string(who) + ": the step size eps must be positive and finite");
    if (!(delta_max > 0.0) || !std::isfinite(delta_max)) return fail(std::string(who) + ": delta_max must be positive and finite");
    HmcState& H = *E.hmc;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    const size_t P = (size_t)p, nd = (size_t)ndraws, nu = (size_t)(2 * max_depth + (1 << max_depth) - 1);
    if (!H.d_tree) H.d_tree = (double*)plat_malloc(sizeof(double) * (12 + 2 * nuts::MAX_DEPTH) * P);
    if (!H.d_nctl) H.d_nctl = (nuts::Ctl*)plat_malloc(sizeof(nuts::Ctl));
    if (!H.d_tree || !H.d_nctl || (samples && !dev_grow(H.d_samples, H.samples_cap, nd * P, E.stream)) || !dev_grow(H.d_stat, H.stat_cap, 2 * nd, E.stream) ||
        !dev_grow(H.d_istat, H.istat_cap, 3 * nd, E.stream) ||
        (normals && !dev_grow(H.d_mom, H.mom_cap, nd * P, E.stream)) || (uniforms && !dev_grow(H.d_uni, H.uni_cap, nd * nu, E.stream)))
        return fail(std::string(who) + ": device allocation failed");
    nuts::Ctl ctl;
    std::memset(&ctl, 0, sizeof ctl);
    ctl.status = nuts::ST_RUN;
    ctl.fresh = 1;
    if ((normals && plat_h2d(H.d_mom, normals, sizeof(double) * nd * P, E.stream)) || (uniforms && plat_h2d(H.d_uni, uniforms, sizeof(double) * nd * nu, E.stream)) ||
        plat_h2d(H.d_nctl, &ctl, sizeof ctl, E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    nuts::Tree q;
    std::memset(&q, 0, sizeof q);
    q.ctl = H.d_nctl;
    double* v = H.d_tree;
    for (double** f : {&q.th_l, &q.r_l, &q.g_l, &q.th_r, &q.r_r, &q.g_r, &q.th_sc, &q.g_sc, &q.th_tc, &q.g_tc, &q.rho, &q.rho_sub}) { *f = v; v += P; }
    q.r_ck = v; q.rho_ck = v + nuts::MAX_DEPTH * P;
    q.normals = normals ? H.d_mom : nullptr; q.uniforms = uniforms ? H.d_uni : nullptr;
    q.samples = samples ? H.d_samples : nullptr; q.accept_stat = H.d_stat; q.logp = H.d_stat + nd;
    q.tree_depth = H.d_istat; q.n_leapfrog = H.d_istat + nd; q.divergent = H.d_istat + 2 * nd;
    q.ndraws = ndraws; q.max_depth = max_depth; q.nu = (int)nu;
    q.eps = eps; q.delta_max = delta_max;
    q.seed_lo = (unsigned)seed; q.seed_hi = (unsigned)(seed >> 32); q.ctr0 = (unsigned)H.draws;
    auto step = [&] {
        if (H.ev.f64) nuts::launch_step<double>(H.a, q, H.ev.out<double>(), H.ev.sums(P), E.stream);
        else nuts::launch_step<float>(H.a, q, H.ev.out<float>(), H.ev.sums(P), E.stream);
    };
    auto read_ctl = [&] { return plat_d2h(&ctl, H.d_nctl, sizeof ctl, E.stream) || plat_sync(E.stream); };
    step();                                              // the first draw's momentum and first leaf; every slot after it: evaluation, then judge + propose
    const long long max_slots = (long long)ndraws * ((1 << max_depth) - 1);      // (a draw has at most 2^D - 1 leaves)
    for (long long slots = 0; ctl.status == nuts::ST_RUN;) {
        if (slots >= max_slots) return fail(std::string(who) + ": the transitions did not end within ndraws (2^max_depth - 1) leapfrog steps");
        for (int s = 0; s < E.nuts_chunk; ++s, ++slots) {
            if (H.ev.eval(E)) {                          // (the current state only changes when a transition ends: the chain is at its last completed draw)
                if (!read_ctl()) H.draws += (unsigned long long)ctl.draw;
                return 1;
            }
            step();
        }
        if (read_ctl()) return fail(std::string("device error: ") + plat_last_error());
    }
    H.draws += nd;
    if ((samples && plat_d2h(samples, H.d_samples, sizeof(double) * nd * P, E.stream)) || plat_d2h(accept_stat, q.accept_stat, sizeof(double) * nd, E.stream) ||
        plat_d2h(logp, q.logp, sizeof(double) * nd, E.stream) || plat_d2h(tree_depth, q.tree_depth, sizeof(int) * nd, E.stream) ||
        plat_d2h(n_leapfrog, q.n_leapfrog, sizeof(int) * nd, E.stream) || plat_d2h(divergent, q.divergent, sizeof(int) * nd, E.stream))
        return fail(std::string(who) + ": D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

int pinn_hmc_find_stepsize(pinn_handle h, double eps0, uint64_t seed, const double* normals, int64_t p, double* eps, int* ntrials) {
    const char* who = "pinn_hmc_find_stepsize";
    if (!h || !eps) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p) || hmc_refuse_target(E, who)) return 1;
    if (!(eps0 > 0.0) || !std::isfinite(eps0)) return fail(std::string(who) + ": the step size eps0 must be positive and finite");
    HmcState& H = *E.hmc;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    const size_t P = (size_t)p;
    if (!dev_grow(H.d_r0, H.r0_cap, P, E.stream) || (normals && !dev_grow(H.d_mom, H.mom_cap, P, E.stream)))
        return fail(std::string(who) + ": device allocation failed");
    if (normals && plat_h2d(H.d_mom, normals, sizeof(double) * P, E.stream)) return fail(std::string(who) + ": H2D copy failed");
    // r0 and h0 = -logp(current) + 1/2 sum minv r0^2; the current state, its gradient and logp are only read from here on
    hmc::launch_momentum_z(H.a, normals ? H.d_mom : nullptr, seed, 0xFFFFFFFFu, E.stream);
    hmc::launch_energy(H.a, 0, nullptr, E.stream);
    plat_d2d(H.d_r0, H.a.r, sizeof(double) * P, E.stream);
    const double log08 = std::log(0.8);
    double e = eps0, direction = 0.0;
    int trials = 0;
    for (int t = 0; t <= 40; ++t) {
        if (t > 0) {
            e *= direction > 0 ? 2.0 : 0.5;
            plat_d2d(H.a.r, H.d_r0, sizeof(double) * P, E.stream);
        }
        hmc_leap(E, H, false, 0.5 * e, e, 1);
        if (H.ev.eval(E)) return 1;
        hmc_leap(E, H, true, 0.5 * e, e, 0);
        hmc::launch_energy(H.a, 1, H.ev.sums(P), E.stream);
        double hh[2];                                    // H_old, H_new: neighbours in the scalar block
        if (plat_d2h(hh, H.a.sc + hmc::SC_H_OLD, sizeof hh, E.stream) || plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        double d = hh[0] - hh[1];
        ++trials;
        if (t == 0) {
            direction = (std::isfinite(d) && d > log08) ? 1.0 : -1.0;
            continue;
        }
        if (!std::isfinite(d)) d = -INFINITY;
        if ((direction > 0) == (d <= log08)) break;
    }
    *eps = e;
    if (ntrials) *ntrials = trials;
    return 0;
}

int pinn_hmc_warmup(pinn_handle h, int n_adapts, int n_leapfrog, double eps0, double target, uint64_t seed, const double* normals, const double* uniforms,
                    double* samples, int64_t p, double* accept_prob, double* logp, double* step_sizes, double* eps_final, double* inv_metric) {
    const char* who = "pinn_hmc_warmup";
    if (!h || !accept_prob || !logp || !eps_final) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p) || hmc_refuse_target(E, who)) return 1;
    if (n_adapts < 1) return fail(std::string(who) + ": n_adapts must be at least 1");
    if (n_leapfrog < 1) return fail(std::string(who) + ": n_leapfrog must be at least 1");
    if (!(eps0 > 0.0) || !std::isfinite(eps0)) return fail(std::string(who) + ": the step size eps0 must be positive and finite");
    if (!(target > 0.0) || !(target < 1.0)) return fail(std::string(who) + ": the target acceptance rate must be in (0, 1)");
    HmcState& H = *E.hmc;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    const size_t P = (size_t)p, nd = (size_t)n_adapts;
    if (!dev_grow(H.d_samples, H.samples_cap, nd * P, E.stream) || !dev_grow(H.d_stat, H.stat_cap, 2 * nd, E.stream) ||
        !dev_grow(H.d_steps, H.steps_cap, nd + 1, E.stream) ||
        (normals && !dev_grow(H.d_mom, H.mom_cap, nd * P, E.stream)) || (uniforms && !dev_grow(H.d_uni, H.uni_cap, nd, E.stream)))
        return fail(std::string(who) + ": device allocation failed");
    // eps, mu, hbar, log_eps_bar, m: neighbours in the scalar block; step_sizes[0]
    const double sc0[5] = {eps0, std::log(10.0 * eps0), 0.0, 0.0, 0.0};
    if ((normals && plat_h2d(H.d_mom, normals, sizeof(double) * nd * P, E.stream)) || (uniforms && plat_h2d(H.d_uni, uniforms, sizeof(double) * nd, E.stream)) ||
        plat_h2d(H.a.sc + hmc::SC_EPS, sc0, sizeof sc0, E.stream) || plat_h2d(H.d_steps, sc0, sizeof(double), E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    const int w0 = (int)(0.15 * (double)n_adapts), w1 = (int)(0.9 * (double)n_adapts);      // the variance window of the metric
    const bool metric_event = w1 - w0 >= 8 && n_adapts >= 100;
    double* d_acc = H.d_stat;
    double* d_lp = H.d_stat + nd;
    for (int d = 0; d < n_adapts; ++d) {
        const unsigned ctr = (unsigned)H.draws;
        hmc::launch_momentum_z(H.a, normals ? H.d_mom + (size_t)d * P : nullptr, seed, ctr, E.stream);
        hmc::launch_energy(H.a, 0, nullptr, E.stream);
        hmc_leap_dev(E, H, false, 0.5, 1);
        for (int s = 0; s < n_leapfrog; ++s) {
            if (H.ev.eval(E)) return 1;                 // (the chain is at its last completed draw, under the metric in force there)
            const bool last = s == n_leapfrog - 1;
            hmc_leap_dev(E, H, true, last ? 0.5 : 1.0, last ? 0 : 1);
        }
        hmc::launch_energy(H.a, 1, H.ev.sums(P), E.stream);
        const bool restart = metric_event && d == w1 - 1;
        const int flags = (restart ? hmc::ADAPT_RESTART : 0) | (d == n_adapts - 1 ? hmc::ADAPT_LAST : 0);
        hmc::launch_accept_adapt(H.a, d, uniforms ? H.d_uni : nullptr, seed, ctr, H.d_samples, d_acc, d_lp, target, flags, H.d_steps, E.stream);
        if (restart) hmc::launch_window_metric(H.a, H.d_samples, w0, w1, E.stream);
        ++H.draws;
    }
    if ((samples && plat_d2h(samples, H.d_samples, sizeof(double) * nd * P, E.stream)) || plat_d2h(accept_prob, d_acc, sizeof(double) * nd, E.stream) ||
        plat_d2h(logp, d_lp, sizeof(double) * nd, E.stream) || (step_sizes && plat_d2h(step_sizes, H.d_steps, sizeof(double) * nd, E.stream)) ||
        plat_d2h(eps_final, H.d_steps + nd, sizeof(double), E.stream) || (inv_metric && plat_d2h(inv_metric, H.a.minv, sizeof(double) * P, E.stream)))
        return fail(std::string(who) + ": D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

int pinn_hmc_get(pinn_handle h, double* theta, int64_t p, double* logp, double* grad) {
    const char* who = "pinn_hmc_get";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p)) return 1;
    HmcState& H = *E.hmc;
    DeviceScope scope(E.device);
    if (plat_d2h(theta, H.a.th_cur, sizeof(double) * (size_t)p, E.stream) || (logp && plat_d2h(logp, H.a.sc + hmc::SC_LP_CUR, sizeof(double), E.stream)) ||
        (grad && plat_d2h(grad, H.a.g_cur, sizeof(double) * (size_t)p, E.stream)) || plat_sync(E.stream))
        return fail(std::string(who) + ": D2H copy failed");
    return 0;
}

}  // extern "C"
