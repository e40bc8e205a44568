// hmc.cpp — resident HMC (pinn_hmc_init / _set_metric / _draws / _get): the transition loop of
// neuralpde.jl_amd/bpinn.py `_hmc` with the chain on the device; and its warm-up (pinn_hmc_find_stepsize / _warmup; section 4.11): the initial
// step-size search, dual averaging and the windowed diagonal metric of `_hmc_device`.
// A leapfrog step = the handle's resident evaluation (resident.hpp: ResidentEval) + ONE update launch (hmc_kernels.hpp); nothing is read back
// before the single download that ends pinn_hmc_draws.
// pinn_nuts_draws (section 4.14): No-U-Turn transitions of the same chain — slots of one evaluation + one state-machine launch
// (nuts_kernels.hpp), queued in chunks of "nuts_chunk"; the control block is all the host reads between chunks.
// pinn_hmc_set_metric_dense / _get_metric_dense (section 4.16): the same chain under a full inverse metric M^-1 = L L^T (hmc_dense_kernels.hpp).
// The trajectory is written once, in Run below: the entry points queue momentum, trajectory and metric event through it and do not ask which
// metric the chain holds.
// The state has buffers of its own: evaluations and optimiser runs between two calls do not touch the chain, and the chain does not touch them.
#include "hmc_host.hpp"
#include "nuts_kernels.hpp"
#include "hmc_dense_kernels.hpp"

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
    // the dense metric (allocated by the first pinn_hmc_set_metric_dense; section 4.16)
    bool dense = false;                  // which metric the chain holds
    hmc::Dense dn{};
    double* d_dmat = nullptr;            // [4 ld ld]: M^-1 | L | staged M^-1 | staged L
    double* d_dvec = nullptr;            // [5 P]: second momentum | second proposal (the ping-pong partners of a.r, a.th_prop) | v | mu | diag
    int* d_dflag = nullptr;
};

namespace {

void hmc_release(HmcState* H) {
    if (!H) return;
    H->ev.release();
    plat_free(H->d_state); plat_free(H->d_tab); plat_free(H->d_kind);
    plat_free(H->d_samples); plat_free(H->d_stat); plat_free(H->d_mom); plat_free(H->d_uni);
    plat_free(H->d_r0); plat_free(H->d_steps);
    plat_free(H->d_tree); plat_free(H->d_nctl); plat_free(H->d_istat);
    plat_free(H->d_dmat); plat_free(H->d_dvec); plat_free(H->d_dflag);
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

// stage -> factorise -> commit, all on the stream; the caller reads the flag when it wants to know
void dense_refactor(pinn_engine& E, HmcState& H) {
    hmc::launch_chol(H.dn, H.a.P, E.stream);
    hmc::launch_commit(H.a, H.dn, E.stream);
}

// One call's launches, under the metric the chain holds.  Diagonal: momentum and proposal stay in a.r and a.th_prop.  Dense: they ping-pong between
// (a.r, a.th_prop) and their partners in d_dvec, every leap flipping the side.  `args()` is the argument block whose r / th_prop are the current
// ones, for the energy and accept launches.
struct Run {
    pinn_engine& E; HmcState& H;
    int rc = 0, tc = 0;
    double* rb(int k) const { return k ? H.d_dvec : H.a.r; }
    double* tb(int k) const { return k ? H.d_dvec + H.a.P : H.a.th_prop; }
    double* r() const { return rb(rc); }
    hmc::Args args() const { hmc::Args b = H.a; b.r = rb(rc); b.th_prop = tb(tc); return b; }
    // the update launch, T the evaluation's element type: DMODE_EVAL after an evaluation at the proposal, DMODE_FIRST the opening half kick
    template <class T> void leap_as(int mode, double kick, double eps, int from_sc, int drift) {
        const T* ev = mode == hmc::DMODE_EVAL ? H.ev.out<T>() : nullptr;
        if (!H.dense) return hmc::launch_leap<T>(H.a, ev, kick, eps, from_sc, drift, E.stream);
        const hmc::LeapIO io{tb(tc), tb(1 - tc), rb(rc), rb(1 - rc)};
        hmc::launch_dense_leap<T>(H.a, H.dn, ev, io, mode, kick, eps, from_sc, drift, E.stream);
        if (mode != hmc::DMODE_PRODUCT) rc = 1 - rc;
        if (drift) tc = 1 - tc;
    }
    void leap(int mode, double kick, double eps, int from_sc, int drift) {
        if (H.ev.f64) leap_as<double>(mode, kick, eps, from_sc, drift);
        else leap_as<float>(mode, kick, eps, from_sc, drift);
    }
    // mode 0: H_old.  mode 1: logp(proposal) from the last evaluation's sums, H_new
    void energy(int mode) {
        hmc::launch_energy(args(), mode, mode ? H.ev.sums((size_t)H.a.P) : nullptr, H.dense ? H.dn.v : nullptr, E.stream);
    }
    // the momentum from z (a device row of standard normals, or the generator) under the metric, or the caller's momentum as given; then H_old.
    // Dense: r = L^-T z, and the product launch v = M^-1 r the energy reads
    void momentum(const double* z, const double* given, uint64_t seed, unsigned ctr) {
        if (!H.dense) hmc::launch_momentum(H.a, z, given, seed, ctr, E.stream);
        else {
            if (given) plat_d2d(r(), given, sizeof(double) * (size_t)H.a.P, E.stream);
            else hmc::launch_dense_momentum(H.a, H.dn, z, seed, ctr, r(), E.stream);
            leap(hmc::DMODE_PRODUCT, 0.0, 0.0, 0, 0);
        }
        energy(0);
    }
    // the trajectory after the momentum: eps from the host, or (from_sc) from the scalar block with kick factors 1/2, 1
    int trajectory(int n_leapfrog, double eps, int from_sc) {
        const double half = from_sc ? 0.5 : 0.5 * eps, full = from_sc ? 1.0 : eps;
        leap(hmc::DMODE_FIRST, half, eps, from_sc, 1);
        for (int s = 0; s < n_leapfrog; ++s) {
            if (H.ev.eval(E)) return 1;                 // (the current state only changes in the accept launch: a failed call leaves the chain at its last completed draw)
            const bool last = s == n_leapfrog - 1;
            leap(hmc::DMODE_EVAL, last ? half : full, eps, from_sc, last ? 0 : 1);
        }
        energy(1);
        return 0;
    }
    // the warm-up's metric event from rows [w0, w1) of the sample buffer.  Dense: the window's regularised covariance, staged; a bad pivot keeps the old metric
    void metric_event(int w0, int w1) {
        if (!H.dense) return hmc::launch_window_metric(H.a, H.d_samples, w0, w1, E.stream);
        hmc::launch_cov(H.a, H.dn, H.d_samples, w0, w1, E.stream);
        dense_refactor(E, H);
    }
};

// the staging of a call of nd draws: the sample buffer when wanted, the statistic | logp pair, `rows` [nd][P] momenta or normals and `uni` [nd][nu]
// uniforms uploaded (null: the generator's)
int hmc_stage(pinn_engine& E, HmcState& H, const char* who, size_t nd, const double* rows, const double* uni, size_t nu, bool want_samples) {
    const size_t P = (size_t)H.a.P;
    if ((want_samples && !dev_grow(H.d_samples, H.samples_cap, nd * P, E.stream)) || !dev_grow(H.d_stat, H.stat_cap, 2 * nd, E.stream) ||
        (rows && !dev_grow(H.d_mom, H.mom_cap, nd * P, E.stream)) || (uni && !dev_grow(H.d_uni, H.uni_cap, nd * nu, E.stream)))
        return fail(std::string(who) + ": device allocation failed");
    if ((rows && plat_h2d(H.d_mom, rows, sizeof(double) * nd * P, E.stream)) || (uni && plat_h2d(H.d_uni, uni, sizeof(double) * nd * nu, E.stream)))
        return fail(std::string(who) + ": H2D copy failed");
    return 0;
}
// samples (when asked for) | statistic | logp of the nd draws to the host; the caller synchronises
int hmc_download(pinn_engine& E, HmcState& H, const char* who, size_t nd, double* samples, double* stat, double* logp) {
    if ((samples && plat_d2h(samples, H.d_samples, sizeof(double) * nd * (size_t)H.a.P, E.stream)) || plat_d2h(stat, H.d_stat, sizeof(double) * nd, E.stream) ||
        plat_d2h(logp, H.d_stat + nd, sizeof(double) * nd, E.stream))
        return fail(std::string(who) + ": D2H copy failed");
    return 0;
}

}  // namespace

int pe::hmc_refuse_dense(const pinn_engine& E, const char* who, const char* why) {
    if (E.hmc && E.hmc->dense) return fail(std::string(who) + ": the handle's chain holds a dense metric (pinn_hmc_set_metric_dense); " + why + " (pinn_hmc_set_metric returns to a diagonal one)");
    return 0;
}

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
    if (hmc_check_target(E, who, p, stds, k, nullptr, nn_mu, nn_sigma, n_prior, prior_kind, prior_mu, prior_sigma) || hmc_refuse_target(E, who)) return 1;
    DeviceScope scope(E.device);
    if (!E.f64 && ensure_points(E)) return 1;
    const size_t P = (size_t)p;
    std::unique_ptr<HmcState, void (*)(HmcState*)> H(new HmcState, hmc_release);
    H->d_state = (double*)plat_malloc(sizeof(double) * (6 * P + hmc::SC_COUNT));
    if (!H->d_state) return fail(std::string(who) + ": device allocation failed");
    hmc::Args& a = H->a;
    std::vector<double> w;                               // the evaluation's term weights
    if (hmc_target_setup(E, who, p, stds, nn_mu, nn_sigma, n_prior, prior_kind, prior_mu, prior_sigma, H->d_tab, H->d_kind, a, w) || H->ev.init(E, who, w.data(), k)) return 1;
    const bool f64 = H->ev.f64;
    a.sse_roundtrip = f64 ? 1 : 0;
    a.th_cur = H->d_state; a.th_prop = a.th_cur + P; a.r = a.th_prop + P; a.g_cur = a.r + P; a.g_prop = a.g_cur + P;
    double* minv = a.g_prop + P;
    a.minv = minv; a.sc = minv + P;
    a.th_eval64 = H->ev.theta64(E);
    a.th_eval32 = H->ev.theta32();
    // host image of the state: theta twice, zero momentum and gradients, unit metric
    std::vector<double> st(6 * P + hmc::SC_COUNT, 0.0);
    std::copy(theta, theta + P, st.begin());
    std::copy(theta, theta + P, st.begin() + P);
    std::fill(st.begin() + 5 * P, st.begin() + 6 * P, 1.0);
    if (plat_h2d(H->d_state, st.data(), sizeof(double) * st.size(), E.stream)) return fail(std::string(who) + ": H2D copy failed");
    if (f64) {
        if (plat_h2d(a.th_eval64, theta, sizeof(double) * P, E.stream)) return fail(std::string(who) + ": H2D copy failed");
    } else {
        std::vector<float> t32(P);
        for (size_t i = 0; i < P; ++i) t32[i] = (float)theta[i];
        if (plat_h2d(a.th_eval32, t32.data(), sizeof(float) * P, E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": H2D copy failed");
    }
    // logp and its gradient at theta: one evaluation, the update kernel with a zero kick (gradient only), the energy kernel at zero momentum
    if (H->ev.eval(E)) return 1;
    Run R{E, *H};
    R.leap(hmc::DMODE_EVAL, 0.0, 0.0, 0, 0);
    R.energy(1);
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
        if (hmc_need_positive(who, "the inverse metric", inv_metric[i])) return 1;
        m[(size_t)i] = inv_metric[i];
    }
    DeviceScope scope(E.device);
    if (plat_h2d((double*)H.a.minv, m.data(), sizeof(double) * (size_t)p, E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": H2D copy failed");
    H.dense = false;
    return 0;
}

int pinn_hmc_set_metric_dense(pinn_handle h, const double* inv_metric, int64_t p) {
    const char* who = "pinn_hmc_set_metric_dense";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p) || hmc_refuse_target(E, who)) return 1;
    if (p > hmc::DENSE_MAX_P) return fail(std::string(who) + ": " + std::to_string(p) + " parameters; the dense metric is limited to P <= " + std::to_string(hmc::DENSE_MAX_P));
    HmcState& H = *E.hmc;
    const size_t P = (size_t)p, ld = (size_t)hmc::dense_ld((int)p);
    std::vector<double> img(ld * ld, 0.0);               // the padded image: pads zero
    double amax = 0.0;
    for (size_t i = 0; i < P; ++i)
        for (size_t j = 0; j < P; ++j) {
            const double x = inv_metric ? inv_metric[i * P + j] : (i == j ? 1.0 : 0.0);
            if (!std::isfinite(x)) return fail(std::string(who) + ": the inverse metric has a non-finite entry at (" + std::to_string(i) + ", " + std::to_string(j) + ")");
            amax = std::max(amax, std::fabs(x));
            img[i * ld + j] = x;
        }
    for (size_t i = 0; i < P; ++i)
        for (size_t j = 0; j < i; ++j)
            if (std::fabs(img[i * ld + j] - img[j * ld + i]) > 1e-12 * amax)
                return fail(std::string(who) + ": the inverse metric is not symmetric at (" + std::to_string(i) + ", " + std::to_string(j) + ")");
    DeviceScope scope(E.device);
    if (!H.d_dmat) {
        double* mat = (double*)plat_malloc(sizeof(double) * 4 * ld * ld);
        double* vec = (double*)plat_malloc(sizeof(double) * 5 * P);
        int* flg = (int*)plat_malloc(sizeof(int) * hmc::DF_COUNT);
        if (!mat || !vec || !flg) { plat_free(mat); plat_free(vec); plat_free(flg); return fail(std::string(who) + ": device allocation failed"); }
        H.d_dmat = mat; H.d_dvec = vec; H.d_dflag = flg;
        H.dn.ld = (int)ld;
        H.dn.M = mat; H.dn.L = mat + ld * ld; H.dn.Mn = mat + 2 * ld * ld; H.dn.Ln = mat + 3 * ld * ld;
        H.dn.v = vec + 2 * P; H.dn.mu = vec + 3 * P; H.dn.diag = vec + 4 * P;
        H.dn.flag = flg;
    }
    int flag[hmc::DF_COUNT] = {0, -1, 0, -1};
    if (plat_h2d(H.dn.Mn, img.data(), sizeof(double) * ld * ld, E.stream) || plat_h2d(H.dn.flag, flag, sizeof flag, E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    dense_refactor(E, H);
    if (plat_d2h(flag, H.dn.flag, sizeof flag, E.stream) || plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    if (flag[hmc::DF_STATUS] != 0)
        return fail(std::string(who) + ": the inverse metric is not positive definite: pivot " + std::to_string(flag[hmc::DF_INDEX]) + " of its Cholesky factorisation is not positive and finite");
    H.dense = true;
    return 0;
}

int pinn_hmc_get_metric_dense(pinn_handle h, double* inv_metric, double* chol, int64_t p) {
    const char* who = "pinn_hmc_get_metric_dense";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p)) return 1;
    HmcState& H = *E.hmc;
    if (!H.dense) return fail(std::string(who) + ": the handle's chain holds a diagonal metric (pinn_hmc_set_metric_dense sets a dense one)");
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, ld = (size_t)H.dn.ld;
    std::vector<double> img(ld * ld);
    const double* src[2] = {H.dn.M, H.dn.L};
    double* dst[2] = {inv_metric, chol};
    for (int q = 0; q < 2; ++q) {
        if (!dst[q]) continue;
        if (plat_d2h(img.data(), src[q], sizeof(double) * ld * ld, E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": D2H copy failed");
        for (size_t i = 0; i < P; ++i) std::copy(img.begin() + i * ld, img.begin() + i * ld + P, dst[q] + i * P);
    }
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
    if (hmc_need_positive(who, "the step size eps", eps)) return 1;
    HmcState& H = *E.hmc;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    const size_t P = (size_t)p, nd = (size_t)ndraws;
    if (hmc_stage(E, H, who, nd, momenta, uniforms, 1, samples != nullptr)) return 1;
    Run R{E, H};
    for (int d = 0; d < ndraws; ++d) {
        const unsigned ctr = (unsigned)H.draws;
        R.momentum(nullptr, momenta ? H.d_mom + (size_t)d * P : nullptr, seed, ctr);
        if (R.trajectory(n_leapfrog, eps, 0)) return 1;
        hmc::launch_accept(R.args(), d, uniforms ? H.d_uni : nullptr, seed, ctr, samples ? H.d_samples : nullptr, H.d_stat, H.d_stat + nd, E.stream);
        ++H.draws;
    }
    if (hmc_download(E, H, who, nd, samples, accept_prob, logp)) return 1;
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

int pinn_nuts_draws(pinn_handle h, int ndraws, int max_depth, double eps, double delta_max, uint64_t seed, const double* normals, const double* uniforms,
                    double* samples, int64_t p, double* accept_stat, double* logp, int* tree_depth, int* n_leapfrog, int* divergent) {
    const char* who = "pinn_nuts_draws";
    if (!h || !accept_stat || !logp || !tree_depth || !n_leapfrog || !divergent) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p) || hmc_refuse_target(E, who) || hmc_refuse_dense(E, who, "the U-turn test runs under a diagonal metric")) return 1;
    if (ndraws < 1) return fail(std::string(who) + ": ndraws must be at least 1");
    if (max_depth < 1 || max_depth > nuts::MAX_DEPTH) return fail(std::string(who) + ": max_depth must be in 1.." + std::to_string(nuts::MAX_DEPTH));
    if (hmc_need_positive(who, "the step size eps", eps) || hmc_need_positive(who, "delta_max", delta_max)) return 1;
    HmcState& H = *E.hmc;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    const size_t P = (size_t)p, nd = (size_t)ndraws, nu = (size_t)(2 * max_depth + (1 << max_depth) - 1);
    if (!H.d_tree) H.d_tree = (double*)plat_malloc(sizeof(double) * (12 + 2 * nuts::MAX_DEPTH) * P);
    if (!H.d_nctl) H.d_nctl = (nuts::Ctl*)plat_malloc(sizeof(nuts::Ctl));
    if (!H.d_tree || !H.d_nctl || !dev_grow(H.d_istat, H.istat_cap, 3 * nd, E.stream)) return fail(std::string(who) + ": device allocation failed");
    if (hmc_stage(E, H, who, nd, normals, uniforms, nu, samples != nullptr)) return 1;
    nuts::Ctl ctl;
    std::memset(&ctl, 0, sizeof ctl);
    ctl.status = nuts::ST_RUN;
    ctl.fresh = 1;
    if (plat_h2d(H.d_nctl, &ctl, sizeof ctl, E.stream)) return fail(std::string(who) + ": H2D copy failed");
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
    if (hmc_download(E, H, who, nd, samples, accept_stat, logp)) return 1;
    if (plat_d2h(tree_depth, q.tree_depth, sizeof(int) * nd, E.stream) || plat_d2h(n_leapfrog, q.n_leapfrog, sizeof(int) * nd, E.stream) ||
        plat_d2h(divergent, q.divergent, sizeof(int) * nd, E.stream))
        return fail(std::string(who) + ": D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

int pinn_hmc_find_stepsize(pinn_handle h, double eps0, uint64_t seed, const double* normals, int64_t p, double* eps, int* ntrials) {
    const char* who = "pinn_hmc_find_stepsize";
    if (!h || !eps) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (hmc_ready(E, who) || check_theta(E, who, p) || hmc_refuse_target(E, who)) return 1;
    if (hmc_need_positive(who, "the step size eps0", eps0)) return 1;
    HmcState& H = *E.hmc;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    const size_t P = (size_t)p;
    if (!dev_grow(H.d_r0, H.r0_cap, P, E.stream) || (normals && !dev_grow(H.d_mom, H.mom_cap, P, E.stream)))
        return fail(std::string(who) + ": device allocation failed");
    if (normals && plat_h2d(H.d_mom, normals, sizeof(double) * P, E.stream)) return fail(std::string(who) + ": H2D copy failed");
    // r0 and h0 = -logp(current) + 1/2 sum minv r0^2; the current state, its gradient and logp are only read from here on
    Run R{E, H};
    R.momentum(normals ? H.d_mom : nullptr, nullptr, seed, 0xFFFFFFFFu);
    plat_d2d(H.d_r0, R.r(), sizeof(double) * P, E.stream);
    const double log08 = std::log(0.8);
    double e = eps0, direction = 0.0;
    int trials = 0;
    for (int t = 0; t <= 40; ++t) {
        if (t > 0) {
            e *= direction > 0 ? 2.0 : 0.5;
            plat_d2d(R.r(), H.d_r0, sizeof(double) * P, E.stream);
        }
        if (R.trajectory(1, e, 0)) return 1;
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
    if (hmc_need_positive(who, "the step size eps0", eps0)) return 1;
    if (!(target > 0.0) || !(target < 1.0)) return fail(std::string(who) + ": the target acceptance rate must be in (0, 1)");
    HmcState& H = *E.hmc;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    const size_t P = (size_t)p, nd = (size_t)n_adapts;
    if (!dev_grow(H.d_steps, H.steps_cap, nd + 1, E.stream)) return fail(std::string(who) + ": device allocation failed");
    if (hmc_stage(E, H, who, nd, normals, uniforms, 1, true)) return 1;      // (the sample buffer whether or not the caller wants it: the metric's window)
    // eps, mu, hbar, log_eps_bar, m: neighbours in the scalar block; step_sizes[0]
    const double sc0[5] = {eps0, std::log(10.0 * eps0), 0.0, 0.0, 0.0};
    if (plat_h2d(H.a.sc + hmc::SC_EPS, sc0, sizeof sc0, E.stream) || plat_h2d(H.d_steps, sc0, sizeof(double), E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    const int w0 = (int)(0.15 * (double)n_adapts), w1 = (int)(0.9 * (double)n_adapts);      // the variance window of the metric
    const bool metric_event = w1 - w0 >= 8 && n_adapts >= 100;
    Run R{E, H};
    int dflag[hmc::DF_COUNT] = {0, -1, 0, -1};
    if (H.dense && plat_h2d(H.dn.flag, dflag, sizeof dflag, E.stream)) return fail(std::string(who) + ": H2D copy failed");
    for (int d = 0; d < n_adapts; ++d) {
        const unsigned ctr = (unsigned)H.draws;
        R.momentum(normals ? H.d_mom + (size_t)d * P : nullptr, nullptr, seed, ctr);
        if (R.trajectory(n_leapfrog, 0.0, 1)) return 1;  // (on failure the chain is at its last completed draw, under the metric in force there)
        const bool restart = metric_event && d == w1 - 1;
        const int flags = (restart ? hmc::ADAPT_RESTART : 0) | (d == n_adapts - 1 ? hmc::ADAPT_LAST : 0);
        hmc::launch_accept_adapt(R.args(), d, uniforms ? H.d_uni : nullptr, seed, ctr, H.d_samples, H.d_stat, H.d_stat + nd, target, flags, H.d_steps, E.stream);
        if (restart) R.metric_event(w0, w1);
        ++H.draws;
    }
    if (hmc_download(E, H, who, nd, samples, accept_prob, logp)) return 1;
    if ((step_sizes && plat_d2h(step_sizes, H.d_steps, sizeof(double) * nd, E.stream)) ||
        plat_d2h(eps_final, H.d_steps + nd, sizeof(double), E.stream) ||
        (inv_metric && plat_d2h(inv_metric, H.dense ? H.dn.diag : H.a.minv, sizeof(double) * P, E.stream)) ||
        (H.dense && plat_d2h(dflag, H.dn.flag, sizeof dflag, E.stream)))
        return fail(std::string(who) + ": D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    if (dflag[hmc::DF_REJECTED] != 0) {                  // the run is complete and its outputs are valid: a report, not a failure
        fail(std::string(who) + ": the window covariance was not positive definite (pivot " + std::to_string(dflag[hmc::DF_REJECTED_INDEX]) + "); the metric before the window was kept");
        return PINN_HMC_METRIC_KEPT;
    }
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
