// lbfgs.cpp — the L-BFGS finishers of the C ABI: pinn_lbfgs (iteration on the host, evaluations on the device) and the resident loop
// pinn_lbfgs_init / _steps / _get.  Both use the noise-floor switch of resident.hpp (GemmFloorSwitch).
#include "resident.hpp"
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
            if (run_loss_grad(E, E.d_theta, E.hp_out, term_w, -1, false, E.hp_raw, false, true)) return 1;
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
// resident evaluation (resident.hpp: ResidentEval).
// Slots are queued in chunks of "lbfgs_chunk"; the host reads the control block after a chunk and nothing else before the call's end.
// The state has buffers of its own: evaluations, optimiser runs and HMC draws between two calls do not touch it, and it does not touch them.
struct pe::LbfgsState {
    lbfgs::Args a;
    lbfgs::Ctl ctl;                      // host mirror of the control block as of the last download
    ResidentEval ev;                     // the term weights, fixed at init (the curvature pairs belong to one objective)
    double* d_state = nullptr;           // [4 P + 2 m P + m]: x | g | xn | d | S | Y | rho
    lbfgs::Ctl* d_ctl = nullptr;
    double* d_tab = nullptr;             // [2 K]: weights | n_norm
    double* d_hist = nullptr;
    size_t hist_cap = 0;
};

namespace {

void lbfgs_release(LbfgsState* H) {
    if (!H) return;
    H->ev.release();
    plat_free(H->d_state); plat_free(H->d_ctl); plat_free(H->d_tab); plat_free(H->d_hist);
    delete H;
}

// what pinn_lbfgs_steps / _get check first; leaves the handle as it is
int lbfgs_ready(pinn_engine& E, const char* who) {
    if (!E.lbfgs) return fail(std::string(who) + ": no optimiser state (call pinn_lbfgs_init first)");
    return E.lbfgs->ev.ready(E, who, "pinn_lbfgs_init");
}
int lbfgs_refuse_target(pinn_engine& E, const char* who) {
    return resident_refuse_target(E, who, "the resident L-BFGS loop runs on a single device only", "L-BFGS needs a fixed objective");
}
void lbfgs_step(pinn_engine& E, LbfgsState& H, int mode, int it0, int it_end, double gtol) {
    if (H.ev.f64) lbfgs::launch_step<double>(H.a, H.ev.out<double>(), mode, it0, it_end, gtol, E.stream);
    else lbfgs::launch_step<float>(H.a, H.ev.out<float>(), mode, it0, it_end, gtol, E.stream);
}
// (f, g) at x from one evaluation; rings cleared, nothing pending (init, and after the noise-floor switch); downloads the control block
int lbfgs_adopt(pinn_engine& E, LbfgsState& H) {
    lbfgs_step(E, H, lbfgs::MODE_LOAD, 0, 0, 0.0);
    if (H.ev.eval(E)) return 1;
    lbfgs_step(E, H, lbfgs::MODE_ADOPT, 0, 0, 0.0);
    if (plat_d2h(&H.ctl, H.d_ctl, sizeof(lbfgs::Ctl), E.stream)) return fail("D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

}  // namespace

void pe::lbfgs_free(pinn_engine& E) {
    lbfgs_release(E.lbfgs);
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
    if (lbfgs_refuse_target(E, who)) return 1;
    DeviceScope scope(E.device);
    if (!E.f64 && ensure_points(E)) return 1;
    const size_t P = (size_t)p, m = (size_t)history;
    const int K = (int)E.terms.size();
    std::unique_ptr<LbfgsState, void (*)(LbfgsState*)> H(new LbfgsState, lbfgs_release);
    const size_t nstate = 4 * P + 2 * m * P + m;
    H->d_state = (double*)plat_malloc(sizeof(double) * nstate);
    H->d_ctl = (lbfgs::Ctl*)plat_malloc(sizeof(lbfgs::Ctl));
    H->d_tab = (double*)plat_malloc(sizeof(double) * (size_t)(2 * K));
    if (!H->d_state || !H->d_ctl || !H->d_tab) return fail(std::string(who) + ": device allocation failed");
    std::vector<double> tb((size_t)(2 * K));             // weights (the caller's floats, widened) | n_norm
    for (int k = 0; k < K; ++k) {
        tb[k] = term_w ? (double)term_w[k] : 1.0;
        tb[K + k] = (double)E.terms[k].n_norm;
    }
    if (H->ev.init(E, who, tb.data(), K)) return 1;
    lbfgs::Args& a = H->a;
    std::memset(&a, 0, sizeof a);
    a.P = (int)p; a.K = K; a.m = history; a.f64form = H->ev.f64 ? 1 : 0;
    a.x = H->d_state; a.g = a.x + P; a.xn = a.g + P; a.d = a.xn + P; a.S = a.d + P; a.Y = a.S + m * P; a.rho = a.Y + m * P;
    a.ctl = H->d_ctl;
    a.w = H->d_tab; a.nrm = H->d_tab + K;
    a.sums = H->ev.sums(P);
    a.th_eval64 = H->ev.theta64(E);
    a.th_eval32 = H->ev.theta32();
    std::memset(&H->ctl, 0, sizeof H->ctl);
    plat_memset(H->d_state, 0, sizeof(double) * nstate, E.stream);
    if (plat_h2d(a.x, theta, sizeof(double) * P, E.stream) || plat_h2d(H->d_tab, tb.data(), sizeof(double) * tb.size(), E.stream) ||
        plat_h2d(H->d_ctl, &H->ctl, sizeof(lbfgs::Ctl), E.stream) || plat_sync(E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    if (lbfgs_adopt(E, *H)) return 1;
    lbfgs_free(E);
    E.lbfgs = H.release();
    E.lbfgs_history = history;
    return 0;
}

int pinn_lbfgs_steps(pinn_handle h, int maxiters, int max_evals, double gtol, double* loss_history, int* iters_done, int* evals_done, int* status) {
    const char* who = "pinn_lbfgs_steps";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (lbfgs_ready(E, who) || lbfgs_refuse_target(E, who)) return 1;
    if (maxiters < 1) return fail(std::string(who) + ": maxiters must be at least 1");
    if (max_evals < 1) return fail(std::string(who) + ": max_evals must be at least 1");
    LbfgsState& H = *E.lbfgs;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    if (!dev_grow(H.d_hist, H.hist_cap, (size_t)maxiters, E.stream)) return fail(std::string(who) + ": device allocation failed");
    H.a.loss_hist = H.d_hist;
    if (H.ctl.status >= lbfgs::ST_CONVERGED) {           // a terminal state ends a call, not the optimisation: the next call tests again
        H.ctl.status = lbfgs::ST_RUN;
        if (plat_h2d(H.d_ctl, &H.ctl, sizeof(lbfgs::Ctl), E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": H2D copy failed");
    }
    const int it0 = H.ctl.it, it_end = it0 + maxiters, ev0 = H.ctl.evals;
    GemmFloorSwitch floor_switch(E);
    for (;;) {
        const int left = max_evals - (H.ctl.evals - ev0);
        if (left <= 0) break;
        const int n = std::min(E.lbfgs_chunk, left);     // (a slot proposes at most one trial point)
        for (int s = 0; s < n; ++s) {
            lbfgs_step(E, H, lbfgs::MODE_SLOT, it0, it_end, gtol);
            if (H.ev.eval(E)) return 1;
        }
        if (plat_d2h(&H.ctl, H.d_ctl, sizeof(lbfgs::Ctl), E.stream)) return fail(std::string(who) + ": D2H copy failed");
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        if (H.ctl.status < lbfgs::ST_CONVERGED) continue;
        if (H.ctl.status == lbfgs::ST_STALLED && floor_switch.eligible()) {
            const int sw = floor_switch.engage();
            if (sw == 1) return 1;
            if (sw == 0 && floor_switch.switched) {      // go on from the same iterate; curvature pairs carry the other arithmetic's gradient noise
                if (lbfgs_adopt(E, H)) return 1;
                continue;
            }
        }
        break;
    }
    const int done = H.ctl.it - it0;
    if (loss_history) {
        if (done > 0 && (plat_d2h(loss_history, H.d_hist, sizeof(double) * (size_t)done, E.stream) || plat_sync(E.stream))) return fail(std::string(who) + ": D2H copy failed");
        for (int i = done; i < maxiters; ++i) loss_history[i] = H.ctl.f;
    }
    if (iters_done) *iters_done = done;
    if (evals_done) *evals_done = H.ctl.evals - ev0;
    if (status) *status = H.ctl.status;
    return floor_switch.finish();
}

int pinn_lbfgs_get(pinn_handle h, double* theta, int64_t p, double* f, double* grad) {
    const char* who = "pinn_lbfgs_get";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (lbfgs_ready(E, who) || check_theta(E, who, p)) return 1;
    LbfgsState& H = *E.lbfgs;
    DeviceScope scope(E.device);
    if (plat_d2h(theta, H.a.x, sizeof(double) * (size_t)p, E.stream) || (grad && plat_d2h(grad, H.a.g, sizeof(double) * (size_t)p, E.stream)) || plat_sync(E.stream))
        return fail(std::string(who) + ": D2H copy failed");
    if (f) *f = H.ctl.f;
    return 0;
}

}  // extern "C"
