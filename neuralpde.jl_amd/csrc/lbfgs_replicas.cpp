// lbfgs_replicas.cpp — replica-resident L-BFGS (pinn_lbfgs_replicas_init / _steps / _get): the quasi-Newton finisher of
// nrep trainings of the handle's discretised problem, one workgroup each, whole slots (evaluation, judgement, proposal) inside ONE launch
// (lbfgs_replica_kernels.hpp: k_lbfgs_replicas, reached through SpecInfo::lbfgs_replicas).  The state has buffers of its own — per replica:
// x | g | xn | d in double, the rings S, Y, rho, a control block, a weight image, a parameter row, record scratch, a gradient slab, loss partials
// — so evaluations, pinn_adam_*, pinn_adam_replicas_*, pinn_hmc_* and the single-training quasi-Newton loops on the same handle leave it alone,
// and it leaves them alone; the handle's kernel plan is read afresh by every call.  The term weights are fixed at init: the curvature belongs to
// one objective.  Between two launches of a call the host reads the nrep control blocks and nothing else.
#include <cstring>
#include <memory>

#include "resident.hpp"

using namespace pe;

struct pe::LbfgsReplicaState {
    int nrep = 0, K = 0, m = 0;
    int64_t P = 0;
    const pk::SpecInfo* spec = nullptr;  // the kernel the buffers were sized for
    std::vector<lbfgs::Ctl> ctl;         // host mirror of the control blocks as of the last download
    std::vector<float> term_w;           // the term weights of every evaluation
    double* d_state = nullptr; double* d_rings = nullptr; lbfgs::Ctl* d_ctl = nullptr; double* d_sums = nullptr; double* d_tab = nullptr;
    float* d_packed = nullptr; float* d_params = nullptr; float* d_slabs = nullptr; double* d_losspart = nullptr; float* d_scratch = nullptr;
    int* d_call = nullptr; double* d_hist = nullptr;
    size_t hist_cap = 0;
};

namespace {

constexpr size_t LDS_GFX950 = 160 * 1024;    // bytes of LDS a gfx950 workgroup can hold

void release(LbfgsReplicaState* R) {
    if (!R) return;
    plat_free(R->d_state); plat_free(R->d_rings); plat_free(R->d_ctl); plat_free(R->d_sums); plat_free(R->d_tab);
    plat_free(R->d_packed); plat_free(R->d_params); plat_free(R->d_slabs); plat_free(R->d_losspart); plat_free(R->d_scratch);
    plat_free(R->d_call); plat_free(R->d_hist);
    delete R;
}

// the set-ups the kernel's evaluation covers (resident.hpp: shared with the chain-resident sampler and the replica-resident Adam), and the room
// its LDS state needs
int eligible(pinn_engine& E, const char* who) {
    if (wg_resident_eligible(E, who, "the replica-resident L-BFGS", "the replicas finish on one fixed discretisation", "lbfgs replica",
                             [](const pk::SpecInfo& s) { return s.lbfgs_replicas != nullptr; }, (int64_t)pk::REPLICA_MAX_P)) return 1;
    const size_t eval_bytes = 4 * (size_t)E.groups[0].spec->LDS_WG, all_bytes = 4 * (size_t)pk::lbfgs_replica_lds(E.groups[0].spec->LDS_WG);
    if (all_bytes > LDS_GFX950)
        return fail(std::string(who) + ": the evaluation's " + std::to_string(eval_bytes) + " bytes of LDS and the finisher's state's " +
                    std::to_string(all_bytes - eval_bytes) + " are more than the " + std::to_string(LDS_GFX950) + " of a workgroup");
    if ((int)E.terms.size() > pk::LBFGS_REPLICA_MAX_TERMS)
        return fail(std::string(who) + ": more than " + std::to_string(pk::LBFGS_REPLICA_MAX_TERMS) + " loss terms are not covered by the replica-resident L-BFGS");
    return 0;
}
int ready(pinn_engine& E, const char* who) {
    if (!E.lbfgs_replicas) return fail(std::string(who) + ": no optimiser state (call pinn_lbfgs_replicas_init first)");
    if (eligible(E, who)) return 1;
    const LbfgsReplicaState& R = *E.lbfgs_replicas;
    if (E.groups[0].spec != R.spec || E.ntheta != R.P || (int)E.terms.size() != R.K)
        return fail(std::string(who) + ": the handle's kernel plan changed since pinn_lbfgs_replicas_init (call pinn_lbfgs_replicas_init again)");
    return ensure_points(E);
}

// one launch over every replica: `call` = [nrep][3] it0, it_end, slots
int launch(pinn_engine& E, LbfgsReplicaState& R, int mode, const std::vector<int>& call, double gtol, int hist_stride) {
    if (plat_h2d(R.d_call, call.data(), sizeof(int) * call.size(), E.stream)) return fail("H2D copy failed");
    const float* w = R.term_w.empty() ? nullptr : R.term_w.data();
    const pk::GroupArgs ga = wg_resident_group_args(E, w, R.d_packed, R.d_params, R.d_slabs, R.d_losspart, R.d_scratch);
    pk::LbfgsReplicaArgs la;
    std::memset(&la, 0, sizeof la);
    la.r.packed = R.d_packed; la.r.params = R.d_params; la.r.defaults = E.d_defaults;
    la.r.row_ptr = E.d_gr_ptr; la.r.row_ent = E.d_gr_ent; la.r.inv_ptr = E.d_inv_ptr; la.r.inv_pos = E.d_inv_pos;
    la.r.P = (int)R.P; la.r.K = R.K; la.r.np = E.np; la.r.ne = E.ne; la.r.p_off = E.p_theta_off;
    la.state = R.d_state; la.rings = R.d_rings; la.ctl = R.d_ctl; la.sums = R.d_sums; la.hist = R.d_hist; la.tab = R.d_tab; la.call = R.d_call;
    la.m = R.m; la.mode = mode; la.hist_stride = hist_stride; la.gtol = gtol;
    E.groups[0].spec->lbfgs_replicas(ga, la, R.nrep, E.stream);
    if (plat_d2h(R.ctl.data(), R.d_ctl, sizeof(lbfgs::Ctl) * R.ctl.size(), E.stream)) return fail("D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());      // (`call` is a pageable temporary)
    return 0;
}

}  // namespace

void pe::lbfgs_replicas_free(pinn_engine& E) {
    release(E.lbfgs_replicas);
    E.lbfgs_replicas = nullptr;
}

extern "C" {

int pinn_lbfgs_replicas_init(pinn_handle h, int nrep, const double* theta, int64_t p, int history, const float* term_w) {
    const char* who = "pinn_lbfgs_replicas_init";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    if (nrep < 1 || nrep > pk::REPLICA_MAX_REPLICAS) return fail(std::string(who) + ": nrep must be in 1.." + std::to_string(pk::REPLICA_MAX_REPLICAS));
    if (history < 1 || history > lbfgs::MAX_HISTORY) return fail(std::string(who) + ": history must be in 1.." + std::to_string(lbfgs::MAX_HISTORY));
    if (eligible(E, who)) return 1;
    DeviceScope scope(E.device);
    if (ensure_points(E)) return 1;
    const pk::SpecInfo& S = *E.groups[0].spec;
    const int K = (int)E.terms.size();
    const size_t P = (size_t)p, nr = (size_t)nrep, m = (size_t)history, nring = nr * (2 * m * P + m);
    std::unique_ptr<LbfgsReplicaState, void (*)(LbfgsReplicaState*)> R(new LbfgsReplicaState, release);
    R->nrep = nrep; R->K = K; R->m = history; R->P = p; R->spec = &S;
    R->ctl.assign(nr, lbfgs::Ctl{});
    if (term_w) R->term_w.assign(term_w, term_w + K);
    R->d_state = (double*)plat_malloc(sizeof(double) * nr * 4 * P);
    R->d_rings = (double*)plat_malloc(sizeof(double) * nring);
    R->d_ctl = (lbfgs::Ctl*)plat_malloc(sizeof(lbfgs::Ctl) * nr);
    R->d_sums = (double*)plat_malloc(sizeof(double) * nr * (size_t)K);
    R->d_tab = (double*)plat_malloc(sizeof(double) * 2 * (size_t)K);
    R->d_packed = (float*)plat_malloc(sizeof(float) * nr * (size_t)S.PACKED);
    R->d_params = (float*)plat_malloc(sizeof(float) * nr * pk::MAX_PARAMS);
    R->d_slabs = (float*)plat_malloc(sizeof(float) * nr * (size_t)S.SLAB);
    R->d_losspart = (double*)plat_malloc(sizeof(double) * nr * 4 * (size_t)K);
    R->d_scratch = (float*)plat_malloc(sizeof(float) * std::max<size_t>(nr * 4 * (size_t)S.SCR, 1));      // (register-resident records: SCR = 0)
    R->d_call = (int*)plat_malloc(sizeof(int) * nr * 3);
    if (!R->d_state || !R->d_rings || !R->d_ctl || !R->d_sums || !R->d_tab || !R->d_packed || !R->d_params || !R->d_slabs || !R->d_losspart ||
        !R->d_scratch || !R->d_call || !dev_grow(R->d_hist, R->hist_cap, nr, E.stream))
        return fail(std::string(who) + ": device allocation failed");
    // host image of the vectors: per replica x = theta | g = xn = d = 0; the table weights (the caller's floats, widened) | n_norm
    std::vector<double> st(nr * 4 * P, 0.0), tb(2 * (size_t)K);
    for (size_t r = 0; r < nr; ++r) std::copy(theta + r * P, theta + (r + 1) * P, st.begin() + r * 4 * P);
    for (int k = 0; k < K; ++k) {
        tb[k] = term_w ? (double)term_w[k] : 1.0;
        tb[K + k] = (double)E.terms[k].n_norm;
    }
    if (plat_h2d(R->d_state, st.data(), sizeof(double) * st.size(), E.stream) || plat_h2d(R->d_tab, tb.data(), sizeof(double) * tb.size(), E.stream) ||
        plat_h2d(R->d_ctl, R->ctl.data(), sizeof(lbfgs::Ctl) * nr, E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    // the images' padding and the parameter rows start at zero (aux::k_pack writes zeros where no parameter lands); the rings are empty
    plat_memset(R->d_packed, 0, sizeof(float) * nr * (size_t)S.PACKED, E.stream);
    plat_memset(R->d_params, 0, sizeof(float) * nr * pk::MAX_PARAMS, E.stream);
    plat_memset(R->d_sums, 0, sizeof(double) * nr * (size_t)K, E.stream);
    plat_memset(R->d_rings, 0, sizeof(double) * nring, E.stream);
    // (f, g) at x from one evaluation per replica
    if (launch(E, *R, pk::LBFGS_REPLICA_ADOPT, std::vector<int>(nr * 3, 0), 0.0, 1)) return 1;
    lbfgs_replicas_free(E);
    E.lbfgs_replicas = R.release();
    return 0;
}

int pinn_lbfgs_replicas_steps(pinn_handle h, int maxiters, int max_evals, double gtol, double* loss_history, int* iters_done, int* evals_done,
                              int* status) {
    const char* who = "pinn_lbfgs_replicas_steps";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (ready(E, who)) return 1;
    if (maxiters < 1) return fail(std::string(who) + ": maxiters must be at least 1");
    if (max_evals < 1) return fail(std::string(who) + ": max_evals must be at least 1");
    LbfgsReplicaState& R = *E.lbfgs_replicas;
    const size_t nr = (size_t)R.nrep;
    if (!dev_grow(R.d_hist, R.hist_cap, nr * (size_t)maxiters, E.stream)) return fail(std::string(who) + ": device allocation failed");
    // a terminal state ends a call, not the optimisation: the next call tests again
    bool reset = false;
    for (auto& c : R.ctl)
        if (c.status >= qn::ST_CONVERGED) { c.status = qn::ST_RUN; reset = true; }
    if (reset && (plat_h2d(R.d_ctl, R.ctl.data(), sizeof(lbfgs::Ctl) * nr, E.stream) || plat_sync(E.stream))) return fail(std::string(who) + ": H2D copy failed");
    std::vector<int> it0(nr), ev0(nr), call(nr * 3);
    for (size_t r = 0; r < nr; ++r) { it0[r] = R.ctl[r].it; ev0[r] = R.ctl[r].evals; }
    // launches of at most LBFGS_REPLICA_MAX_SLOTS slots while a replica is not terminal and has evaluations left (a slot proposes one trial
    // point, so the slot bound is the replica's max_evals); a launch ends with the state in its HBM rows, where the next one picks it up
    for (;;) {
        bool any = false;
        for (size_t r = 0; r < nr; ++r) {
            const lbfgs::Ctl& c = R.ctl[r];
            const int left = c.status >= qn::ST_CONVERGED ? 0 : std::min(pk::LBFGS_REPLICA_MAX_SLOTS, max_evals - (c.evals - ev0[r]));
            call[3 * r] = it0[r]; call[3 * r + 1] = it0[r] + maxiters; call[3 * r + 2] = std::max(left, 0);
            any = any || left > 0;
        }
        if (!any) break;
        if (launch(E, R, pk::LBFGS_REPLICA_SLOTS, call, gtol, maxiters)) return 1;
    }
    if (loss_history) {
        if (plat_d2h(loss_history, R.d_hist, sizeof(double) * nr * (size_t)maxiters, E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": D2H copy failed");
        for (size_t r = 0; r < nr; ++r)
            for (int i = R.ctl[r].it - it0[r]; i < maxiters; ++i) loss_history[r * (size_t)maxiters + i] = R.ctl[r].f;
    }
    for (size_t r = 0; r < nr; ++r) {
        if (iters_done) iters_done[r] = R.ctl[r].it - it0[r];
        if (evals_done) evals_done[r] = R.ctl[r].evals - ev0[r];
        if (status) status[r] = R.ctl[r].status;
    }
    return 0;
}

int pinn_lbfgs_replicas_get(pinn_handle h, int nrep, int64_t p, double* theta, double* f, double* grad) {
    const char* who = "pinn_lbfgs_replicas_get";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (!E.lbfgs_replicas) return fail(std::string(who) + ": no optimiser state (call pinn_lbfgs_replicas_init first)");
    LbfgsReplicaState& R = *E.lbfgs_replicas;
    if (p != R.P || nrep != R.nrep) return fail(std::string(who) + ": nrep / theta length differ from pinn_lbfgs_replicas_init's");
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, nr = (size_t)nrep;
    if (theta || grad) {                                 // one download of the vectors
        std::vector<double> st(nr * 4 * P);
        if (plat_d2h(st.data(), R.d_state, sizeof(double) * st.size(), E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": D2H copy failed");
        double* const out[2] = {theta, grad};
        for (size_t j = 0; j < 2; ++j)
            for (size_t r = 0; out[j] && r < nr; ++r) std::copy(st.begin() + (r * 4 + j) * P, st.begin() + (r * 4 + j + 1) * P, out[j] + r * P);
    }
    for (size_t r = 0; f && r < nr; ++r) f[r] = R.ctl[r].f;
    return 0;
}

}  // extern "C"
