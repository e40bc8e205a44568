// adam_replicas.cpp — replica-resident Adam (pinn_adam_replicas_init / _steps / _get): nrep independent Adam trainings of
// the handle's discretised problem, one workgroup each, whole iterations inside ONE launch (adam_replica_kernels.hpp: k_adam_replicas, reached
// through SpecInfo::replicas).  The state has buffers of its own — per replica: theta | m | v in float, a weight image, a parameter row, record
// scratch, a gradient slab, loss partials — so evaluations, pinn_adam_*, pinn_hmc_* and the quasi-Newton loops on the same handle leave it alone,
// and it leaves them alone; the handle's kernel plan (launch arguments, reduce map, inverse pack map) is read afresh by every call.
#include <cstring>
#include <memory>

#include "resident.hpp"
#include "adam_host.hpp"

using namespace pe;

struct pe::ReplicaState {
    int nrep = 0, K = 0;
    int64_t P = 0;
    long long t = 0;                     // Adam steps taken since pinn_adam_replicas_init: the bias correction runs on across calls
    const pk::SpecInfo* spec = nullptr;  // the kernel the buffers were sized for
    float* d_state = nullptr; float* d_packed = nullptr; float* d_params = nullptr; double* d_sse = nullptr;
    float* d_slabs = nullptr; double* d_losspart = nullptr; float* d_scratch = nullptr;
    float* d_lr = nullptr; float* d_wn = nullptr; float* d_c12 = nullptr; double* d_hist = nullptr;
    size_t c12_cap = 0, hist_cap = 0;
};

namespace {

constexpr size_t LDS_GFX950 = 160 * 1024;    // bytes of LDS a gfx950 workgroup can hold

void replicas_release(ReplicaState* R) {
    if (!R) return;
    plat_free(R->d_state); plat_free(R->d_packed); plat_free(R->d_params); plat_free(R->d_sse);
    plat_free(R->d_slabs); plat_free(R->d_losspart); plat_free(R->d_scratch);
    plat_free(R->d_lr); plat_free(R->d_wn); plat_free(R->d_c12); plat_free(R->d_hist);
    delete R;
}

// the set-ups the kernel's evaluation covers (resident.hpp: shared with the chain-resident sampler), and the room its LDS state needs
int replicas_eligible(pinn_engine& E, const char* who) {
    if (wg_resident_eligible(E, who, "the replica-resident Adam", "the replicas train on one fixed discretisation", "replica",
                             [](const pk::SpecInfo& s) { return s.replicas != nullptr; }, (int64_t)pk::REPLICA_MAX_P)) return 1;
    const size_t eval_floats = (size_t)E.groups[0].spec->LDS_WG, state_floats = 3 * (size_t)pk::REPLICA_MAX_P;
    if (4 * (eval_floats + state_floats) > LDS_GFX950)
        return fail(std::string(who) + ": the evaluation's " + std::to_string(4 * eval_floats) + " bytes of LDS and the optimiser state's " +
                    std::to_string(4 * state_floats) + " are more than the " + std::to_string(LDS_GFX950) + " of a workgroup");
    return 0;
}
int replicas_ready(pinn_engine& E, const char* who) {
    if (!E.replicas) return fail(std::string(who) + ": no optimiser state (call pinn_adam_replicas_init first)");
    if (replicas_eligible(E, who)) return 1;
    if (E.groups[0].spec != E.replicas->spec || E.ntheta != E.replicas->P || (int)E.terms.size() != E.replicas->K)
        return fail(std::string(who) + ": the handle's kernel plan changed since pinn_adam_replicas_init (call pinn_adam_replicas_init again)");
    return ensure_points(E);
}

}  // namespace

void pe::replicas_free(pinn_engine& E) {
    replicas_release(E.replicas);
    E.replicas = nullptr;
}

extern "C" {

int pinn_adam_replicas_init(pinn_handle h, int nrep, const float* theta, int64_t p) {
    const char* who = "pinn_adam_replicas_init";
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    if (nrep < 1 || nrep > pk::REPLICA_MAX_REPLICAS) return fail(std::string(who) + ": nrep must be in 1.." + std::to_string(pk::REPLICA_MAX_REPLICAS));
    if (replicas_eligible(E, who)) return 1;
    DeviceScope scope(E.device);
    if (ensure_points(E)) return 1;
    const pk::SpecInfo& S = *E.groups[0].spec;
    const int K = (int)E.terms.size();
    const size_t P = (size_t)p, nr = (size_t)nrep;
    std::unique_ptr<ReplicaState, void (*)(ReplicaState*)> R(new ReplicaState, replicas_release);
    R->nrep = nrep; R->K = K; R->P = p; R->spec = &S;
    R->d_state = (float*)plat_malloc(sizeof(float) * nr * 3 * P);
    R->d_packed = (float*)plat_malloc(sizeof(float) * nr * (size_t)S.PACKED);
    R->d_params = (float*)plat_malloc(sizeof(float) * nr * pk::MAX_PARAMS);
    R->d_sse = (double*)plat_malloc(sizeof(double) * nr * (size_t)K);
    R->d_slabs = (float*)plat_malloc(sizeof(float) * nr * (size_t)S.SLAB);
    R->d_losspart = (double*)plat_malloc(sizeof(double) * nr * 4 * (size_t)K);
    R->d_scratch = (float*)plat_malloc(sizeof(float) * std::max<size_t>(nr * 4 * (size_t)S.SCR, 1));      // (register-resident records: SCR = 0)
    R->d_lr = (float*)plat_malloc(sizeof(float) * nr);
    R->d_wn = (float*)plat_malloc(sizeof(float) * (size_t)K);
    if (!R->d_state || !R->d_packed || !R->d_params || !R->d_sse || !R->d_slabs || !R->d_losspart || !R->d_scratch || !R->d_lr || !R->d_wn)
        return fail(std::string(who) + ": device allocation failed");
    // host image of the state: per replica theta | m = 0 | v = 0
    std::vector<float> st(nr * 3 * P, 0.f);
    for (size_t r = 0; r < nr; ++r) std::copy(theta + r * P, theta + (r + 1) * P, st.begin() + r * 3 * P);
    if (plat_h2d(R->d_state, st.data(), sizeof(float) * st.size(), E.stream)) return fail(std::string(who) + ": H2D copy failed");
    // the images' padding and the parameter rows start at zero (aux::k_pack writes zeros where no parameter lands); every launch writes the
    // rest from the replica's theta before its first evaluation
    plat_memset(R->d_packed, 0, sizeof(float) * nr * (size_t)S.PACKED, E.stream);
    plat_memset(R->d_params, 0, sizeof(float) * nr * pk::MAX_PARAMS, E.stream);
    plat_memset(R->d_sse, 0, sizeof(double) * nr * (size_t)K, E.stream);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    replicas_free(E);
    E.replicas = R.release();
    return 0;
}

int pinn_adam_replicas_steps(pinn_handle h, int nsteps, const float* lr, float beta1, float beta2, float eps, const float* term_w, double* loss_history) {
    const char* who = "pinn_adam_replicas_steps";
    if (!h || !lr) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (replicas_ready(E, who)) return 1;
    if (nsteps < 1) return fail(std::string(who) + ": nsteps must be at least 1");
    ReplicaState& R = *E.replicas;
    for (int r = 0; r < R.nrep; ++r)
        if (!(lr[r] > 0.f) || !std::isfinite(lr[r])) return fail(std::string(who) + ": the learning rate of replica " + std::to_string(r) + " must be positive and finite");
    const int K = R.K;
    const size_t nr = (size_t)R.nrep;
    if (!dev_grow(R.d_c12, R.c12_cap, 2 * (size_t)nsteps, E.stream) || !dev_grow(R.d_hist, R.hist_cap, nr * (size_t)nsteps, E.stream))
        return fail(std::string(who) + ": device allocation failed");
    // the bias corrections of steps t + 1 .. t + nsteps and the history's weights, as pinn_adam_steps forms them (adam.cpp: upload_c12, adam_prepare)
    std::vector<float> c12(2 * (size_t)nsteps), wn((size_t)K);
    for (int s = 0; s < nsteps; ++s) {
        c12[2 * s] = adam_bias(beta1, R.t + s + 1);
        c12[2 * s + 1] = adam_bias(beta2, R.t + s + 1);
    }
    for (int k = 0; k < K; ++k) wn[k] = (term_w ? term_w[k] : 1.0f) / (float)E.terms[k].n_norm;
    if (plat_h2d(R.d_c12, c12.data(), sizeof(float) * c12.size(), E.stream) || plat_h2d(R.d_wn, wn.data(), sizeof(float) * wn.size(), E.stream) ||
        plat_h2d(R.d_lr, lr, sizeof(float) * nr, E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    const Group& G = E.groups[0];
    const pk::GroupArgs ga = wg_resident_group_args(E, term_w, R.d_packed, R.d_params, R.d_slabs, R.d_losspart, R.d_scratch);
    pk::ReplicaArgs ra;
    std::memset(&ra, 0, sizeof ra);
    ra.state = R.d_state; ra.packed = R.d_packed; ra.params = R.d_params; ra.sse = R.d_sse;
    ra.lr = R.d_lr; ra.w_over_n = R.d_wn; ra.defaults = E.d_defaults;
    ra.row_ptr = E.d_gr_ptr; ra.row_ent = E.d_gr_ent; ra.inv_ptr = E.d_inv_ptr; ra.inv_pos = E.d_inv_pos;
    ra.P = (int)R.P; ra.K = K; ra.np = E.np; ra.ne = E.ne; ra.p_off = E.p_theta_off;
    ra.hist_stride = nsteps;
    ra.b1 = beta1; ra.b2 = beta2; ra.eps = eps;
    // launches of at most REPLICA_MAX_STEPS steps: a launch ends with the state in its HBM rows, where the next one picks it up
    for (int s0 = 0; s0 < nsteps; s0 += pk::REPLICA_MAX_STEPS) {
        ra.nsteps = std::min(pk::REPLICA_MAX_STEPS, nsteps - s0);
        ra.c12 = R.d_c12 + 2 * (size_t)s0;
        ra.hist = R.d_hist + s0;
        G.spec->replicas(ga, ra, R.nrep, E.stream);
    }
    if (loss_history && plat_d2h(loss_history, R.d_hist, sizeof(double) * nr * (size_t)nsteps, E.stream)) return fail(std::string(who) + ": D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());      // (c12, wn are pageable temporaries)
    R.t += nsteps;
    return 0;
}

int pinn_adam_replicas_get(pinn_handle h, int nrep, int64_t p, float* theta, float* m, float* v, double* term_sums) {
    const char* who = "pinn_adam_replicas_get";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (!E.replicas) return fail(std::string(who) + ": no optimiser state (call pinn_adam_replicas_init first)");
    ReplicaState& R = *E.replicas;
    if (p != R.P || nrep != R.nrep) return fail(std::string(who) + ": nrep / theta length differ from pinn_adam_replicas_init's");
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, nr = (size_t)nrep;
    if (theta || m || v) {                               // one download of the state block
        std::vector<float> st(nr * 3 * P);
        if (plat_d2h(st.data(), R.d_state, sizeof(float) * st.size(), E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": D2H copy failed");
        float* const out[3] = {theta, m, v};
        for (size_t j = 0; j < 3; ++j)
            for (size_t r = 0; out[j] && r < nr; ++r) std::copy(st.begin() + (r * 3 + j) * P, st.begin() + (r * 3 + j + 1) * P, out[j] + r * P);
    }
    if (term_sums && plat_d2h(term_sums, R.d_sse, sizeof(double) * nr * (size_t)R.K, E.stream)) return fail(std::string(who) + ": D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

}  // extern "C"
