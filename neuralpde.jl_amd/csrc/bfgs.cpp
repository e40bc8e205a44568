// bfgs.cpp — the resident dense BFGS finisher of the C ABI: pinn_bfgs_init / _steps / _get.  The library's own BFGS with
// the iterate, the inverse-Hessian approximation H and the line search on the device.  A SLOT = bfgs::k_bfgs_ctl (judge the evaluation just
// finished), k_bfgs_matvec, k_bfgs_ctl (the update's scalar c), k_bfgs_update (rank-two update fused with the next direction), k_bfgs_ctl (propose
// the next point) + one full resident evaluation (resident.hpp: ResidentEval).  The matrix kernels are launched in every slot and return at once
// when the control block gives them nothing to do.  The driver is qn_host.hpp's; this unit adds the matrix, its cap and the slot's launches.
// The state has buffers of its own: evaluations, optimiser runs and HMC draws between two calls do not touch it, and it does not touch them.
#include "qn_host.hpp"
#include "bfgs_kernels.hpp"

using namespace pe;

struct pe::BfgsState : QnState<bfgs::Args, bfgs::Ctl> {
    static constexpr const char *NAME = "BFGS", *INIT = "pinn_bfgs_init";
    static constexpr int LOAD = bfgs::PH_LOAD, ADOPT = bfgs::PH_ADOPT;
    double* d_vec = nullptr;             // [7 ld]: x | g | xn | d | s | y | u, pads zero
    double* d_H = nullptr;               // [P][ld]
    ~BfgsState() { plat_free(d_vec); plat_free(d_H); }
    void launch(pinn_engine& E, int phase, int it0, int it_end, double gtol) {
        typed([&](auto* out) { bfgs::launch_ctl(a, out, phase, it0, it_end, gtol, E.stream); });
    }
    void slot(pinn_engine& E, int it0, int it_end, double gtol) {
        launch(E, bfgs::PH_JUDGE, it0, it_end, gtol);
        bfgs::launch_matvec(a, E.stream);
        launch(E, bfgs::PH_MID, it0, it_end, gtol);
        bfgs::launch_update(a, E.stream);
        launch(E, bfgs::PH_PROPOSE, it0, it_end, gtol);
    }
};

namespace {

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
    delete E.bfgs;
    E.bfgs = nullptr;
}
int pe::bfgs_params(const pinn_engine& E) { return E.bfgs ? E.bfgs->a.P : 0; }

extern "C" {

int pinn_bfgs_init(pinn_handle h, const double* theta, int64_t p, const float* term_w) {
    const char* who = "pinn_bfgs_init";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    if (qn_refuse_target<BfgsState>(E, who)) return 1;
    const int cap = bfgs_cap();
    const size_t P = (size_t)p, ld = p <= bfgs::MAX_P ? (size_t)bfgs::padded_ld((int)p) : P, hbytes = sizeof(double) * P * ld;
    if (p > cap)
        return fail(std::string(who) + ": P = " + std::to_string(p) + " parameters exceed the cap of " + std::to_string(cap) + " (the dense inverse-Hessian matrix would take " +
                    std::to_string(hbytes) + " bytes; use the resident L-BFGS, pinn_lbfgs_init)");
    DeviceScope scope(E.device);
    if (!E.f64 && ensure_points(E)) return 1;
    std::unique_ptr<BfgsState> H(new BfgsState);
    H->d_H = (double*)plat_malloc(hbytes);
    if (!H->d_H) return fail(std::string(who) + ": the dense inverse-Hessian matrix cannot be allocated: P = " + std::to_string(p) + ", " + std::to_string(hbytes) + " bytes");
    H->d_vec = (double*)plat_malloc(sizeof(double) * 7 * ld);
    if (!H->d_vec) return fail(std::string(who) + ": device allocation failed");
    bfgs::Args& a = H->a;
    a.ld = (int)ld;
    a.x = H->d_vec; a.g = a.x + ld; a.xn = a.g + ld; a.d = a.xn + ld; a.s = a.d + ld; a.y = a.s + ld; a.u = a.y + ld;
    a.H = H->d_H;
    plat_memset(H->d_vec, 0, sizeof(double) * 7 * ld, E.stream);      // (H itself is first written by k_bfgs_update, whole rows, pads included)
    if (qn_init(E, *H, who, theta, term_w)) return 1;
    bfgs_free(E);
    E.bfgs = H.release();
    return 0;
}

int pinn_bfgs_steps(pinn_handle h, int maxiters, int max_evals, double gtol, double* loss_history, int* iters_done, int* evals_done, int* status) {
    const char* who = "pinn_bfgs_steps";
    if (!h) return fail(std::string(who) + ": null argument");
    return qn_steps(*h, h->bfgs, who, maxiters, max_evals, gtol, loss_history, iters_done, evals_done, status);
}

int pinn_bfgs_get(pinn_handle h, double* theta, int64_t p, double* f, double* grad, double* hinv) {
    const char* who = "pinn_bfgs_get";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (qn_get(E, E.bfgs, who, theta, p, f, grad)) return 1;
    BfgsState& H = *E.bfgs;
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, ld = (size_t)H.a.ld;
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
