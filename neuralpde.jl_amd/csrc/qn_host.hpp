// qn_host.hpp — the host driver the two resident quasi-Newton finishers share (lbfgs.cpp, bfgs.cpp; only these two include it): the state
// around the common control block, the checks every call makes first, the weights | n_norm table, the wiring of the evaluation lane into the
// kernels' arguments, the slot loop with the noise-floor switch, and the common part of _get.
// A solver's state S derives from QnState<its Args, its Ctl> and adds:
//   static constexpr const char *NAME, *INIT    "L-BFGS", "pinn_lbfgs_init": the solver's words in the messages
//   static constexpr int LOAD, ADOPT            the control kernel's two phases outside a slot
//   void launch(E, phase, it0, it_end, gtol)    one launch of the control kernel
//   void slot(E, it0, it_end, gtol)             the launches of one slot before its evaluation
// and frees its own buffers in its destructor.
#pragma once
#include "resident.hpp"
#include "qn_kernels.hpp"

namespace pe {

template <class A, class K> struct QnState {
    A a{};
    K ctl{};                             // host mirror of the control block as of the last download
    K* d_ctl = nullptr;
    ResidentEval ev;                     // the term weights, fixed at init (the curvature belongs to one objective)
    double* d_tab = nullptr;             // [2 K]: weights | n_norm
    double* d_hist = nullptr;
    size_t hist_cap = 0;
    QnState() = default;
    QnState(const QnState&) = delete;
    ~QnState() { ev.release(); plat_free(d_ctl); plat_free(d_tab); plat_free(d_hist); }
    // one launch with the evaluation's output in its element type: f(const double*) in float64 mode, f(const float*) otherwise
    template <class F> void typed(F f) { if (ev.f64) f(ev.out<double>()); else f(ev.out<float>()); }
};

// what _steps / _get check first; leaves the handle as it is
template <class S> int qn_ready(const pinn_engine& E, const S* H, const char* who) {
    if (!H) return fail(std::string(who) + ": no optimiser state (call " + S::INIT + " first)");
    return H->ev.ready(E, who, S::INIT);
}
template <class S> int qn_refuse_target(const pinn_engine& E, const char* who) {
    return resident_refuse_target(E, who, (std::string("the resident ") + S::NAME + " loop runs on a single device only").c_str(),
                                  (std::string(S::NAME) + " needs a fixed objective").c_str());
}

// (f, g) at x from one evaluation; curvature cleared, nothing pending (init, and after the noise-floor switch); downloads the control block
template <class S> int qn_adopt(pinn_engine& E, S& H) {
    H.launch(E, S::LOAD, 0, 0, 0.0);
    if (H.ev.eval(E)) return 1;
    H.launch(E, S::ADOPT, 0, 0, 0.0);
    if (plat_d2h(&H.ctl, H.d_ctl, sizeof H.ctl, E.stream)) return fail("D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

// the second half of _init, after the solver has allocated and zeroed its buffers and pointed a.x, a.g, a.xn, a.d and its own arguments at
// them: the control block, the table, the evaluation lane, the common arguments; x <- theta; the first evaluation
template <class S> int qn_init(pinn_engine& E, S& H, const char* who, const double* theta, const float* term_w) {
    const size_t P = (size_t)E.ntheta;
    const int K = (int)E.terms.size();
    H.d_ctl = (decltype(H.d_ctl))plat_malloc(sizeof H.ctl);
    H.d_tab = (double*)plat_malloc(sizeof(double) * (size_t)(2 * K));
    if (!H.d_ctl || !H.d_tab) return fail(std::string(who) + ": device allocation failed");
    std::vector<double> tb((size_t)(2 * K));             // weights (the caller's floats, widened) | n_norm
    for (int k = 0; k < K; ++k) {
        tb[k] = term_w ? (double)term_w[k] : 1.0;
        tb[K + k] = (double)E.terms[k].n_norm;
    }
    if (H.ev.init(E, who, tb.data(), K)) return 1;
    qn::Args& a = H.a;
    a.P = (int)P; a.K = K; a.f64form = H.ev.f64 ? 1 : 0;
    a.w = H.d_tab; a.nrm = H.d_tab + K;
    a.sums = H.ev.sums(P);
    a.th_eval64 = H.ev.theta64(E);
    a.th_eval32 = H.ev.theta32();
    H.a.ctl = H.d_ctl;
    if (plat_h2d(a.x, theta, sizeof(double) * P, E.stream) || plat_h2d(H.d_tab, tb.data(), sizeof(double) * tb.size(), E.stream) ||
        plat_h2d(H.d_ctl, &H.ctl, sizeof H.ctl, E.stream) || plat_sync(E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    return qn_adopt(E, H);
}

// pinn_lbfgs_steps / pinn_bfgs_steps.  Slots are queued in chunks of "lbfgs_chunk"; the host reads the control block after a chunk and nothing
// else before the call's end.
template <class S> int qn_steps(pinn_engine& E, S* Hp, const char* who, int maxiters, int max_evals, double gtol, double* loss_history, int* iters_done,
                                int* evals_done, int* status) {
    if (qn_ready(E, Hp, who) || qn_refuse_target<S>(E, who)) return 1;
    if (maxiters < 1) return fail(std::string(who) + ": maxiters must be at least 1");
    if (max_evals < 1) return fail(std::string(who) + ": max_evals must be at least 1");
    S& H = *Hp;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    if (!dev_grow(H.d_hist, H.hist_cap, (size_t)maxiters, E.stream)) return fail(std::string(who) + ": device allocation failed");
    H.a.loss_hist = H.d_hist;
    if (H.ctl.status >= qn::ST_CONVERGED) {              // a terminal state ends a call, not the optimisation: the next call tests again
        H.ctl.status = qn::ST_RUN;
        if (plat_h2d(H.d_ctl, &H.ctl, sizeof H.ctl, E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": H2D copy failed");
    }
    const int it0 = H.ctl.it, it_end = it0 + maxiters, ev0 = H.ctl.evals;
    GemmFloorSwitch floor_switch(E);
    for (;;) {
        const int left = max_evals - (H.ctl.evals - ev0);
        if (left <= 0) break;
        const int n = std::min(E.lbfgs_chunk, left);     // (a slot proposes at most one trial point)
        for (int s = 0; s < n; ++s) {
            H.slot(E, it0, it_end, gtol);
            if (H.ev.eval(E)) return 1;
        }
        if (plat_d2h(&H.ctl, H.d_ctl, sizeof H.ctl, E.stream)) return fail(std::string(who) + ": D2H copy failed");
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        if (H.ctl.status < qn::ST_CONVERGED) continue;
        if (H.ctl.status == qn::ST_STALLED && floor_switch.eligible()) {
            const int sw = floor_switch.engage();
            if (sw == 1) return 1;
            if (sw == 0 && floor_switch.switched) {      // go on from the same iterate; the curvature carries the other arithmetic's gradient noise
                if (qn_adopt(E, H)) return 1;
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

// theta, f and (when asked for) the gradient of the current iterate
template <class S> int qn_get(pinn_engine& E, S* Hp, const char* who, double* theta, int64_t p, double* f, double* grad) {
    if (qn_ready(E, Hp, who) || check_theta(E, who, p)) return 1;
    S& H = *Hp;
    DeviceScope scope(E.device);
    if (plat_d2h(theta, H.a.x, sizeof(double) * (size_t)p, E.stream) || (grad && plat_d2h(grad, H.a.g, sizeof(double) * (size_t)p, E.stream)) || plat_sync(E.stream))
        return fail(std::string(who) + ": D2H copy failed");
    if (f) *f = H.ctl.f;
    return 0;
}

}  // namespace pe
