// bfgs.cpp — the resident dense BFGS finisher of the C ABI: pinn_bfgs_init / _steps / _get.  The library's own BFGS with
// the iterate, the inverse-Hessian approximation H and the line search on the device.  A SLOT = bfgs::k_bfgs_ctl (judge the evaluation just
// finished), k_bfgs_matvec, k_bfgs_ctl (the update's scalar c), k_bfgs_update (rank-two update fused with the next direction), k_bfgs_ctl (propose
// the next point) + one full resident evaluation (resident.hpp: ResidentEval).  The matrix kernels are launched in every slot and return at once
// when the control block gives them nothing to do.
// Slots are queued in chunks of "lbfgs_chunk"; the host reads the control block after a chunk and nothing else before the call's end.
// The state has buffers of its own: evaluations, optimiser runs and HMC draws between two calls do not touch it, and it does not touch them.
#include "resident.hpp"
#include "bfgs_kernels.hpp"

using namespace pe;

struct pe::BfgsState {
    bfgs::Args a;
    bfgs::Ctl ctl;                       // host mirror of the control block as of the last download
    ResidentEval ev;                     // the term weights, fixed at init (H belongs to one objective)
    double* d_vec = nullptr;             // [7 ld]: x | g | xn | d | s | y | u, pads zero
    double* d_H = nullptr;               // [P][ld]
    bfgs::Ctl* d_ctl = nullptr;
    double* d_tab = nullptr;             // [2 K]: weights | n_norm
    double* d_hist = nullptr;
    size_t hist_cap = 0;
};

namespace {

void bfgs_release(BfgsState* H) {
    if (!H) return;
    H->ev.release();
    plat_free(H->d_vec); plat_free(H->d_H); plat_free(H->d_ctl); plat_free(H->d_tab); plat_free(H->d_hist);
    delete H;
}

// what pinn_bfgs_steps / _get check first; leaves the handle as it is
int bfgs_ready(pinn_engine& E, const char* who) {
    if (!E.bfgs) return fail(std::string(who) + ": no optimiser state (call pinn_bfgs_init first)");
    return E.bfgs->ev.ready(E, who, "pinn_bfgs_init");
}
int bfgs_refuse_target(pinn_engine& E, const char* who) {
    return resident_refuse_target(E, who, "the resident BFGS loop runs on a single device only", "BFGS needs a fixed objective");
}
void bfgs_ctl(pinn_engine& E, BfgsState& H, int phase, int it0, int it_end, double gtol) {
    if (H.ev.f64) bfgs::launch_ctl<double>(H.a, H.ev.out<double>(), phase, it0, it_end, gtol, E.stream);
    else bfgs::launch_ctl<float>(H.a, H.ev.out<float>(), phase, it0, it_end, gtol, E.stream);
}
// (f, g) at x from one evaluation; H = I, nothing pending (init, and after the noise-floor switch); downloads the control block
int bfgs_adopt(pinn_engine& E, BfgsState& H) {
    bfgs_ctl(E, H, bfgs::PH_LOAD, 0, 0, 0.0);
    if (H.ev.eval(E)) return 1;
    bfgs_ctl(E, H, bfgs::PH_ADOPT, 0, 0, 0.0);
    if (plat_d2h(&H.ctl, H.d_ctl, sizeof(bfgs::Ctl), E.stream)) return fail("D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}
// the most parameters pinn_bfgs_init takes: bfgs::MAX_P, or less by $PINN_BFGS_MAX_P (a device shared with other work)
int bfgs_cap() {
    int cap = bfgs::MAX_P;
    if (const char* e = std::getenv("PINN_BFGS_MAX_P")) {
        char* end = nullptr;
        const long q = std::strtol(e, &end, 10);
        if (end != e && !*end && q >= 1 && q < cap) cap = (int)q;
    }
    return cap;
}

}  // namespace

void pe::bfgs_free(pinn_engine& E) {
    bfgs_release(E.bfgs);
    E.bfgs = nullptr;
}
int pe::bfgs_params(const pinn_engine& E) { return E.bfgs ? E.bfgs->a.P : 0; }

extern "C" {

int pinn_bfgs_init(pinn_handle h, const double* theta, int64_t p, const float* term_w) {
    const char* who = "pinn_bfgs_init";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    if (bfgs_refuse_target(E, who)) return 1;
    const int cap = bfgs_cap();
    const size_t P = (size_t)p, ld = p <= bfgs::MAX_P ? (size_t)bfgs::padded_ld((int)p) : P, hbytes = sizeof(double) * P * ld;
    if (p > cap)
        return fail(std::string(who) + ": P = " + std::to_string(p) + " parameters exceed the cap of " + std::to_string(cap) + " (the dense inverse-Hessian matrix would take " +
                    std::to_string(hbytes) + " bytes; use the resident L-BFGS, pinn_lbfgs_init)");
    DeviceScope scope(E.device);
    if (!E.f64 && ensure_points(E)) return 1;
    const int K = (int)E.terms.size();
    std::unique_ptr<BfgsState, void (*)(BfgsState*)> H(new BfgsState, bfgs_release);
    H->d_H = (double*)plat_malloc(hbytes);
    if (!H->d_H) return fail(std::string(who) + ": the dense inverse-Hessian matrix cannot be allocated: P = " + std::to_string(p) + ", " + std::to_string(hbytes) + " bytes");
    H->d_vec = (double*)plat_malloc(sizeof(double) * 7 * ld);
    H->d_ctl = (bfgs::Ctl*)plat_malloc(sizeof(bfgs::Ctl));
    H->d_tab = (double*)plat_malloc(sizeof(double) * (size_t)(2 * K));
    if (!H->d_vec || !H->d_ctl || !H->d_tab) return fail(std::string(who) + ": device allocation failed");
    std::vector<double> tb((size_t)(2 * K));             // weights (the caller's floats, widened) | n_norm
    for (int k = 0; k < K; ++k) {
        tb[k] = term_w ? (double)term_w[k] : 1.0;
        tb[K + k] = (double)E.terms[k].n_norm;
    }
    if (H->ev.init(E, who, tb.data(), K)) return 1;
    bfgs::Args& a = H->a;
    std::memset(&a, 0, sizeof a);
    a.P = (int)p; a.K = K; a.ld = (int)ld; a.f64form = H->ev.f64 ? 1 : 0;
    a.x = H->d_vec; a.g = a.x + ld; a.xn = a.g + ld; a.d = a.xn + ld; a.s = a.d + ld; a.y = a.s + ld; a.u = a.y + ld;
    a.H = H->d_H;
    a.ctl = H->d_ctl;
    a.w = H->d_tab; a.nrm = H->d_tab + K;
    a.sums = H->ev.sums(P);
    a.th_eval64 = H->ev.theta64(E);
    a.th_eval32 = H->ev.theta32();
    std::memset(&H->ctl, 0, sizeof H->ctl);
    plat_memset(H->d_vec, 0, sizeof(double) * 7 * ld, E.stream);      // (H itself is first written by k_bfgs_update, whole rows, pads included)
    if (plat_h2d(a.x, theta, sizeof(double) * P, E.stream) || plat_h2d(H->d_tab, tb.data(), sizeof(double) * tb.size(), E.stream) ||
        plat_h2d(H->d_ctl, &H->ctl, sizeof(bfgs::Ctl), E.stream) || plat_sync(E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    if (bfgs_adopt(E, *H)) return 1;
    bfgs_free(E);
    E.bfgs = H.release();
    return 0;
}

int pinn_bfgs_steps(pinn_handle h, int maxiters, int max_evals, double gtol, double* loss_history, int* iters_done, int* evals_done, int* status) {
    const char* who = "pinn_bfgs_steps";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (bfgs_ready(E, who) || bfgs_refuse_target(E, who)) return 1;
    if (maxiters < 1) return fail(std::string(who) + ": maxiters must be at least 1");
    if (max_evals < 1) return fail(std::string(who) + ": max_evals must be at least 1");
    BfgsState& H = *E.bfgs;
    DeviceScope scope(E.device);
    H.a.th_eval64 = H.ev.theta64(E);
    if (!dev_grow(H.d_hist, H.hist_cap, (size_t)maxiters, E.stream)) return fail(std::string(who) + ": device allocation failed");
    H.a.loss_hist = H.d_hist;
    if (H.ctl.status >= bfgs::ST_CONVERGED) {            // a terminal state ends a call, not the optimisation: the next call tests again
        H.ctl.status = bfgs::ST_RUN;
        if (plat_h2d(H.d_ctl, &H.ctl, sizeof(bfgs::Ctl), E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": H2D copy failed");
    }
    const int it0 = H.ctl.it, it_end = it0 + maxiters, ev0 = H.ctl.evals;
    GemmFloorSwitch floor_switch(E);
    for (;;) {
        const int left = max_evals - (H.ctl.evals - ev0);
        if (left <= 0) break;
        const int n = std::min(E.lbfgs_chunk, left);     // (a slot proposes at most one trial point)
        for (int s = 0; s < n; ++s) {
            bfgs_ctl(E, H, bfgs::PH_JUDGE, it0, it_end, gtol);
            bfgs::launch_matvec(H.a, E.stream);
            bfgs_ctl(E, H, bfgs::PH_MID, it0, it_end, gtol);
            bfgs::launch_update(H.a, E.stream);
            bfgs_ctl(E, H, bfgs::PH_PROPOSE, it0, it_end, gtol);
            if (H.ev.eval(E)) return 1;
        }
        if (plat_d2h(&H.ctl, H.d_ctl, sizeof(bfgs::Ctl), E.stream)) return fail(std::string(who) + ": D2H copy failed");
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        if (H.ctl.status < bfgs::ST_CONVERGED) continue;
        if (H.ctl.status == bfgs::ST_STALLED && floor_switch.eligible()) {
            const int sw = floor_switch.engage();
            if (sw == 1) return 1;
            if (sw == 0 && floor_switch.switched) {      // go on from the same iterate; H carries the other arithmetic's gradient noise: H = I
                if (bfgs_adopt(E, H)) return 1;
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

int pinn_bfgs_get(pinn_handle h, double* theta, int64_t p, double* f, double* grad, double* hinv) {
    const char* who = "pinn_bfgs_get";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (bfgs_ready(E, who) || check_theta(E, who, p)) return 1;
    BfgsState& H = *E.bfgs;
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, ld = (size_t)H.a.ld;
    if (plat_d2h(theta, H.a.x, sizeof(double) * P, E.stream) || (grad && plat_d2h(grad, H.a.g, sizeof(double) * P, E.stream)) || plat_sync(E.stream))
        return fail(std::string(who) + ": D2H copy failed");
    if (f) *f = H.ctl.f;
    if (hinv && H.ctl.ident) {                           // H = gamma I: the matrix on the device is not in use
        std::fill(hinv, hinv + P * P, 0.0);
        for (size_t i = 0; i < P; ++i) hinv[i * P + i] = H.ctl.gamma;
    } else if (hinv && ld == P) {
        if (plat_d2h(hinv, H.d_H, sizeof(double) * P * P, E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": D2H copy failed");
    } else if (hinv) {                                   // the padded rows, then their first P columns
        std::vector<double> full(P * ld);
        if (plat_d2h(full.data(), H.d_H, sizeof(double) * P * ld, E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": D2H copy failed");
        for (size_t i = 0; i < P; ++i) std::copy(full.begin() + i * ld, full.begin() + i * ld + P, hinv + i * P);
    }
    return 0;
}

}  // extern "C"
