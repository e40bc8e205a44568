// lbfgs.cpp — the L-BFGS finishers of the C ABI: pinn_lbfgs (iteration on the host, evaluations on the device) and the resident loop
// pinn_lbfgs_init / _steps / _get.  Both use the noise-floor switch of resident.hpp (GemmFloorSwitch).
#include "qn_host.hpp"
#include "lbfgs_kernels.hpp"

using namespace pe;

extern "C" {

int pinn_lbfgs(pinn_handle h, double* theta, int64_t p, int maxiters, int history, double gtol, const float* term_w, double* loss_history,
               int* iters_done) {
    if (!h || !theta) return fail("pinn_lbfgs: null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (p != E.ntheta) return fail("pinn_lbfgs: theta length " + std::to_string(p) + " != ntheta " + std::to_string(E.ntheta));
    if (maxiters <= 0 || history <= 0 || history > 64) return fail("pinn_lbfgs: maxiters must be positive and history in 1..64");
    for (auto& T : E.terms)
        if (T.sampler != 0) return fail("pinn_lbfgs: a term redraws its points on the device; L-BFGS needs a fixed objective (fixed point sets)");
    if (ensure_points(E)) return 1;
    const int K = (int)E.terms.size();
    const size_t P = (size_t)p;
    std::vector<float> th32(P);
    std::vector<double> g(P), x(theta, theta + P), xn(P), gn(P), d(P), q(P);
    // one device evaluation: fused loss + gradient, or (grad == nullptr) the loss-only launch — a rejected line-search trial needs the
    // objective only, at about a third of the cost
    auto eval = [&](const std::vector<double>& at, std::vector<double>* grad, double& f) -> int {
        if (E.f64) {                                     // float64 mode: the objective and its gradient in double, no fp32 noise floor
            std::vector<double> w(K, 1.0), L(K);
            if (term_w) for (int k = 0; k < K; ++k) w[k] = term_w[k];
            if (f64_eval(E, at.data(), w.data(), L.data(), grad ? grad->data() : nullptr)) return 1;
            f = 0.0;
            for (int k = 0; k < K; ++k) f += w[k] * L[k];
            return 0;
        }
        for (size_t i = 0; i < P; ++i) th32[i] = (float)at[i];
        if (upload_theta(E, th32.data(), p)) return 1;
        if (grad) {
            if (eval_and_sync(E, E.hp_out, term_w, E.hp_raw, false)) return 1;
        } else {
            EvalRequest rq = EvalRequest::host_entry(E, term_w);
            rq.loss_only = true;
            if (run_loss_grad(E, rq)) return 1;
            if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        }
        f = 0.0;
        for (int k = 0; k < K; ++k) f += (double)(term_w ? term_w[k] : 1.0f) * E.hp_raw[k] / (double)E.terms[k].n_norm;
        if (grad)
            for (size_t i = 0; i < P; ++i) (*grad)[i] = (double)E.hp_out[i];
        return 0;
    };
    auto dot = [&](const std::vector<double>& a, const std::vector<double>& b) { double s = 0.0; for (size_t i = 0; i < P; ++i) s += a[i] * b[i]; return s; };
    double f = 0.0;
    if (eval(x, &g, f)) return 1;
    std::deque<std::vector<double>> S, Y;
    std::deque<double> RHO;
    GemmFloorSwitch floor_switch(E);
    int it = 0;
    for (; it < maxiters; ++it) {
        double gmax = 0.0;
        for (size_t i = 0; i < P; ++i) gmax = std::max(gmax, std::fabs(g[i]));
        if (!(gmax > gtol)) break;
        // two-loop recursion: d = -H g
        q = g;
        std::vector<double> alpha(S.size());
        for (int i = (int)S.size() - 1; i >= 0; --i) {
            alpha[i] = RHO[i] * dot(S[i], q);
            for (size_t j = 0; j < P; ++j) q[j] -= alpha[i] * Y[i][j];
        }
        double gamma = 1.0;
        if (!S.empty()) gamma = dot(S.back(), Y.back()) / dot(Y.back(), Y.back());
        for (size_t j = 0; j < P; ++j) q[j] *= gamma;
        for (size_t i = 0; i < S.size(); ++i) {
            const double beta = RHO[i] * dot(Y[i], q);
            for (size_t j = 0; j < P; ++j) q[j] += (alpha[i] - beta) * S[i][j];
        }
        for (size_t j = 0; j < P; ++j) d[j] = -q[j];
        double gd = dot(g, d);
        if (!(gd < 0.0)) {                               // not a descent direction (stale curvature): restart from steepest descent
            S.clear(); Y.clear(); RHO.clear();
            for (size_t j = 0; j < P; ++j) d[j] = -g[j];
            gd = dot(g, d);
        }
        // backtracking line search (Armijo, c1 = 1e-4); first iteration: step 1 / |g|_1-ish scale
        double t = S.empty() ? std::min(1.0, 1.0 / std::sqrt(dot(g, g))) : 1.0;
        double fn = f;
        bool ok = false;
        // the first trial (accepted most of the time) is a full evaluation: its gradient is the next iterate's; after a rejection the
        // trials are loss-only evaluations and the accepted point gets its gradient from one more full evaluation
        for (int ls = 0; ls < 30; ++ls) {
            for (size_t j = 0; j < P; ++j) xn[j] = x[j] + t * d[j];
            if (eval(xn, ls == 0 ? &gn : nullptr, fn)) return 1;
            if (std::isfinite(fn) && fn <= f + 1e-4 * t * gd) {
                if (ls > 0 && eval(xn, &gn, fn)) return 1;
                ok = true;
                break;
            }
            t *= 0.5;
        }
        if (!ok) {
            // no decrease along a descent direction: the evaluation's noise floor (GemmFloorSwitch)
            if (floor_switch.eligible()) {
                const int sw = floor_switch.engage();
                if (sw == 1) return 1;
                if (sw == 2) break;
                if (floor_switch.switched) {
                    if (eval(x, &g, f)) return 1;
                    S.clear(); Y.clear(); RHO.clear();   // curvature pairs carry the other arithmetic's gradient noise
                    --it;
                    continue;
                }
            }
            break;
        }
        std::vector<double> sv(P), yv(P);
        for (size_t j = 0; j < P; ++j) { sv[j] = xn[j] - x[j]; yv[j] = gn[j] - g[j]; }
        const double sy = dot(sv, yv);
        if (sy > 1e-10 * std::sqrt(dot(sv, sv) * dot(yv, yv))) {
            S.push_back(std::move(sv)); Y.push_back(std::move(yv)); RHO.push_back(1.0 / sy);
            if ((int)S.size() > history) { S.pop_front(); Y.pop_front(); RHO.pop_front(); }
        }
        x.swap(xn); g.swap(gn); f = fn;
        if (loss_history) loss_history[it] = f;
    }
    if (loss_history) for (int i = it; i < maxiters; ++i) loss_history[i] = f;
    if (iters_done) *iters_done = it;
    for (size_t i = 0; i < P; ++i) theta[i] = x[i];
    return floor_switch.finish();
}

}  // extern "C"

// Resident L-BFGS (pinn_lbfgs_init / _steps / _get): pinn_lbfgs's iteration with the iterate, the curvature rings and the
// line search on the device.  A SLOT = one lbfgs::k_lbfgs_step launch (judge the evaluation just finished, propose the next point) + one full
// resident evaluation (resident.hpp: ResidentEval).  The driver is qn_host.hpp's; this unit adds the rings' buffer and the slot's launch.
// The state has buffers of its own: evaluations, optimiser runs and HMC draws between two calls do not touch it, and it does not touch them.
struct pe::LbfgsState : QnState<lbfgs::Args, lbfgs::Ctl> {
    static constexpr const char *NAME = "L-BFGS", *INIT = "pinn_lbfgs_init";
    static constexpr int LOAD = lbfgs::MODE_LOAD, ADOPT = lbfgs::MODE_ADOPT;
    double* d_state = nullptr;           // [4 P + 2 m P + m]: x | g | xn | d | S | Y | rho
    ~LbfgsState() { plat_free(d_state); }
    void launch(pinn_engine& E, int mode, int it0, int it_end, double gtol) {
        typed([&](auto* out) { lbfgs::launch_step(a, out, mode, it0, it_end, gtol, E.stream); });
    }
    void slot(pinn_engine& E, int it0, int it_end, double gtol) { launch(E, lbfgs::MODE_SLOT, it0, it_end, gtol); }
};

void pe::lbfgs_free(pinn_engine& E) {
    delete E.lbfgs;
    E.lbfgs = nullptr;
    E.lbfgs_history = 0;
}

extern "C" {

int pinn_lbfgs_init(pinn_handle h, const double* theta, int64_t p, int history, const float* term_w) {
    const char* who = "pinn_lbfgs_init";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    if (history < 1 || history > lbfgs::MAX_HISTORY) return fail(std::string(who) + ": history must be in 1.." + std::to_string(lbfgs::MAX_HISTORY));
    if (qn_refuse_target<LbfgsState>(E, who)) return 1;
    DeviceScope scope(E.device);
    if (!E.f64 && ensure_points(E)) return 1;
    const size_t P = (size_t)p, m = (size_t)history;
    std::unique_ptr<LbfgsState> H(new LbfgsState);
    const size_t nstate = 4 * P + 2 * m * P + m;
    H->d_state = (double*)plat_malloc(sizeof(double) * nstate);
    if (!H->d_state) return fail(std::string(who) + ": device allocation failed");
    lbfgs::Args& a = H->a;
    a.m = history;
    a.x = H->d_state; a.g = a.x + P; a.xn = a.g + P; a.d = a.xn + P; a.S = a.d + P; a.Y = a.S + m * P; a.rho = a.Y + m * P;
    plat_memset(H->d_state, 0, sizeof(double) * nstate, E.stream);
    if (qn_init(E, *H, who, theta, term_w)) return 1;
    lbfgs_free(E);
    E.lbfgs = H.release();
    E.lbfgs_history = history;
    return 0;
}

int pinn_lbfgs_steps(pinn_handle h, int maxiters, int max_evals, double gtol, double* loss_history, int* iters_done, int* evals_done, int* status) {
    const char* who = "pinn_lbfgs_steps";
    if (!h) return fail(std::string(who) + ": null argument");
    return qn_steps(*h, h->lbfgs, who, maxiters, max_evals, gtol, loss_history, iters_done, evals_done, status);
}

int pinn_lbfgs_get(pinn_handle h, double* theta, int64_t p, double* f, double* grad) {
    const char* who = "pinn_lbfgs_get";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    return qn_get(*h, h->lbfgs, who, theta, p, f, grad);
}

}  // extern "C"
