// hmc_chains.cpp — chain-resident HMC (pinn_hmc_chains_init / _draws / _get): nchains chains of a BPINN posterior, one
// workgroup each, whole trajectories inside ONE launch (hmc_chain_kernels.hpp: k_hmc_chains, reached through SpecInfo::chains).
// The state has buffers of its own — per chain: theta / momentum / gradients / energies in double, a weight image, a parameter row, record
// scratch, a gradient slab, loss partials — so evaluations, pinn_adam_* and pinn_hmc_* on the same handle leave it alone, and it leaves them
// alone; the handle's kernel plan (launch arguments, reduce map, inverse pack map) is read afresh by every call.
#include "hmc_host.hpp"

using namespace pe;

struct pe::ChainsState {
    int nchains = 0, n_leapfrog = 0, K = 0, n_prior = 0;
    int64_t P = 0;
    double eps = 0.0;
    uint64_t seed = 0;
    unsigned long long draws = 0;        // draw counter of the generator, shared by the chains
    const pk::SpecInfo* spec = nullptr;  // the kernel the buffers were sized for
    hmc::Args a;                         // shared tables (device pointers into d_tab / d_kind / d_minv)
    std::vector<float> scale;            // [K] reverse-sweep seeds 2 w_k / N_k with w_k = N_k / (2 s_k^2)
    double* d_state = nullptr; double* d_minv = nullptr; double* d_tab = nullptr; int* d_kind = nullptr;
    float* d_packed = nullptr; float* d_params = nullptr; float* d_ev = nullptr; double* d_sse = nullptr;
    float* d_slabs = nullptr; double* d_losspart = nullptr; float* d_scratch = nullptr;
    double* d_samples = nullptr; double* d_stat = nullptr; double* d_mom = nullptr; double* d_uni = nullptr;
    size_t samples_cap = 0, stat_cap = 0, mom_cap = 0, uni_cap = 0;
    int last_ndraws = 0;
};

namespace {

void chains_release(ChainsState* C) {
    if (!C) return;
    plat_free(C->d_state); plat_free(C->d_minv); plat_free(C->d_tab); plat_free(C->d_kind);
    plat_free(C->d_packed); plat_free(C->d_params); plat_free(C->d_ev); plat_free(C->d_sse);
    plat_free(C->d_slabs); plat_free(C->d_losspart); plat_free(C->d_scratch);
    plat_free(C->d_samples); plat_free(C->d_stat); plat_free(C->d_mom); plat_free(C->d_uni);
    delete C;
}

// the set-ups the kernel's evaluation covers (resident.hpp: shared with the replica-resident Adam)
int chains_eligible(pinn_engine& E, const char* who) {
    return wg_resident_eligible(E, who, "the chain-resident sampler", "HMC needs a fixed target", "chain",
                                [](const pk::SpecInfo& s) { return s.chains != nullptr; }, 256 * (int64_t)pk::CHAIN_MAX_ELEMS);
}
int chains_ready(pinn_engine& E, const char* who) {
    if (!E.chains) return fail(std::string(who) + ": no sampler state (call pinn_hmc_chains_init first)");
    if (chains_eligible(E, who)) return 1;
    if (E.groups[0].spec != E.chains->spec || E.ntheta != E.chains->P || (int)E.terms.size() != E.chains->K)
        return fail(std::string(who) + ": the handle's kernel plan changed since pinn_hmc_chains_init (call pinn_hmc_chains_init again)");
    return ensure_points(E);
}

// one launch: the group's launch arguments with the chains' buffers in place of the handle's, the handle's maps as they are now
void chains_launch(pinn_engine& E, ChainsState& C, pk::ChainArgs& ca) {
    const Group& G = E.groups[0];
    pk::GroupArgs ga = G.ga;
    for (size_t j = 0; j < G.terms.size(); ++j) ga.terms[j].scale = C.scale[(size_t)G.terms[j]];
    ga.packed = C.d_packed; ga.params = C.d_params; ga.slabs = C.d_slabs; ga.losspart = C.d_losspart; ga.scratch = C.d_scratch;
    ga.chain = 0;
    ca.a = C.a;
    ca.state = C.d_state; ca.packed = C.d_packed; ca.params = C.d_params; ca.ev = C.d_ev; ca.sse = C.d_sse;
    ca.defaults = E.d_defaults;
    ca.row_ptr = E.d_gr_ptr; ca.row_ent = E.d_gr_ent; ca.inv_ptr = E.d_inv_ptr; ca.inv_pos = E.d_inv_pos;
    ca.np = E.np; ca.ne = E.ne; ca.p_off = E.p_theta_off;
    G.spec->chains(ga, ca, C.nchains, E.stream);
}

}  // namespace

void pe::chains_free(pinn_engine& E) {
    chains_release(E.chains);
    E.chains = nullptr;
}

extern "C" {

int pinn_hmc_chains_init(pinn_handle h, int nchains, const double* theta, int64_t p, double eps, const double* inv_metric, const double* stds, int k,
                         double nn_mu, double nn_sigma, int n_prior, const int* prior_kind, const double* prior_mu, const double* prior_sigma,
                         int n_leapfrog, uint64_t seed) {
    const char* who = "pinn_hmc_chains_init";
    if (!h || !theta || !stds) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p) || hmc_refuse_dense(E, who, "the chain kernel keeps a diagonal metric in LDS")) return 1;
    if (nchains < 1 || nchains > pk::CHAIN_MAX_CHAINS) return fail(std::string(who) + ": nchains must be in 1.." + std::to_string(pk::CHAIN_MAX_CHAINS));
    if (n_leapfrog < 1) return fail(std::string(who) + ": n_leapfrog must be at least 1");
    if (hmc_need_positive(who, "the step size eps", eps)) return 1;
    if (hmc_check_target(E, who, p, stds, k, inv_metric, nn_mu, nn_sigma, n_prior, prior_kind, prior_mu, prior_sigma)) return 1;
    if (chains_eligible(E, who)) return 1;
    DeviceScope scope(E.device);
    if (ensure_points(E)) return 1;
    const pk::SpecInfo& S = *E.groups[0].spec;
    const int K = (int)E.terms.size();
    const size_t P = (size_t)p, nc = (size_t)nchains, row = 5 * P + hmc::SC_COUNT;
    std::unique_ptr<ChainsState, void (*)(ChainsState*)> C(new ChainsState, chains_release);
    C->nchains = nchains; C->n_leapfrog = n_leapfrog; C->K = K; C->n_prior = n_prior; C->P = p; C->eps = eps; C->seed = seed; C->spec = &S;
    C->d_state = (double*)plat_malloc(sizeof(double) * nc * row);
    C->d_minv = (double*)plat_malloc(sizeof(double) * P);
    C->d_packed = (float*)plat_malloc(sizeof(float) * nc * (size_t)S.PACKED);
    C->d_params = (float*)plat_malloc(sizeof(float) * nc * pk::MAX_PARAMS);
    C->d_ev = (float*)plat_malloc(sizeof(float) * nc * P);
    C->d_sse = (double*)plat_malloc(sizeof(double) * nc * (size_t)K);
    C->d_slabs = (float*)plat_malloc(sizeof(float) * nc * (size_t)S.SLAB);
    C->d_losspart = (double*)plat_malloc(sizeof(double) * nc * 4 * (size_t)K);
    C->d_scratch = (float*)plat_malloc(sizeof(float) * std::max<size_t>(nc * 4 * (size_t)S.SCR, 1));      // (register-resident records: SCR = 0)
    if (!C->d_state || !C->d_minv || !C->d_packed || !C->d_params || !C->d_ev || !C->d_sse || !C->d_slabs || !C->d_losspart || !C->d_scratch)
        return fail(std::string(who) + ": device allocation failed");
    // the target's tables; the reverse sweep's seeds from the evaluation's term weights, narrowed as the evaluation takes them
    hmc::Args& a = C->a;
    std::vector<double> w;
    if (hmc_target_setup(E, who, p, stds, nn_mu, nn_sigma, n_prior, prior_kind, prior_mu, prior_sigma, C->d_tab, C->d_kind, a, w)) return 1;
    C->scale.resize((size_t)K);
    for (int j = 0; j < K; ++j) C->scale[(size_t)j] = (float)(2.0 * (double)(float)w[(size_t)j] / (double)E.terms[j].n_norm);      // (adam.cpp train_common's expression)
    a.minv = C->d_minv;
    // host image of the state: per chain theta as current state, everything else zero; the metric (ones when null)
    std::vector<double> st(nc * row, 0.0), minv(P, 1.0);
    for (size_t c = 0; c < nc; ++c) std::copy(theta + c * P, theta + (c + 1) * P, st.begin() + c * row);
    if (inv_metric) std::copy(inv_metric, inv_metric + P, minv.begin());
    if (plat_h2d(C->d_state, st.data(), sizeof(double) * st.size(), E.stream) || plat_h2d(C->d_minv, minv.data(), sizeof(double) * P, E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    // the images' padding and the parameter rows start at zero (aux::k_pack writes zeros where no parameter lands)
    plat_memset(C->d_packed, 0, sizeof(float) * nc * (size_t)S.PACKED, E.stream);
    plat_memset(C->d_params, 0, sizeof(float) * nc * pk::MAX_PARAMS, E.stream);
    pk::ChainArgs ca;
    std::memset(&ca, 0, sizeof ca);
    ca.init = 1;
    chains_launch(E, *C, ca);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    chains_free(E);
    E.chains = C.release();
    return 0;
}

int pinn_hmc_chains_draws(pinn_handle h, int ndraws, const double* momenta, const double* uniforms) {
    const char* who = "pinn_hmc_chains_draws";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (chains_ready(E, who) || hmc_refuse_dense(E, who, "the chain kernel keeps a diagonal metric in LDS")) return 1;
    if (ndraws < 1) return fail(std::string(who) + ": ndraws must be at least 1");
    ChainsState& C = *E.chains;
    const size_t P = (size_t)C.P, n = (size_t)C.nchains * (size_t)ndraws;
    if (!dev_grow(C.d_samples, C.samples_cap, n * P, E.stream) || !dev_grow(C.d_stat, C.stat_cap, 2 * n, E.stream) ||
        (momenta && !dev_grow(C.d_mom, C.mom_cap, n * P, E.stream)) || (uniforms && !dev_grow(C.d_uni, C.uni_cap, n, E.stream)))
        return fail(std::string(who) + ": device allocation failed");
    if ((momenta && plat_h2d(C.d_mom, momenta, sizeof(double) * n * P, E.stream)) || (uniforms && plat_h2d(C.d_uni, uniforms, sizeof(double) * n, E.stream)))
        return fail(std::string(who) + ": H2D copy failed");
    pk::ChainArgs ca;
    std::memset(&ca, 0, sizeof ca);
    ca.ndraws = ndraws; ca.n_leapfrog = C.n_leapfrog; ca.eps = C.eps;
    ca.momenta = momenta ? C.d_mom : nullptr; ca.uniforms = uniforms ? C.d_uni : nullptr;
    ca.samples = C.d_samples; ca.accept_prob = C.d_stat; ca.logp = C.d_stat + n;
    ca.seed_lo = (unsigned)C.seed; ca.seed_hi = (unsigned)(C.seed >> 32); ca.ctr0 = (unsigned)C.draws;
    C.last_ndraws = 0;
    chains_launch(E, C, ca);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    C.draws += (unsigned long long)ndraws;
    C.last_ndraws = ndraws;
    return 0;
}

int pinn_hmc_chains_get(pinn_handle h, int nchains, int ndraws, int64_t p, double* samples, double* accept_prob, double* logp,
                        double* theta, double* logp_cur, double* grad) {
    const char* who = "pinn_hmc_chains_get";
    if (!h) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (!E.chains) return fail(std::string(who) + ": no sampler state (call pinn_hmc_chains_init first)");
    ChainsState& C = *E.chains;
    if (p != C.P || nchains != C.nchains) return fail(std::string(who) + ": nchains / theta length differ from pinn_hmc_chains_init's");
    if ((samples || accept_prob || logp) && ndraws != C.last_ndraws)
        return fail(std::string(who) + ": ndraws is not the last pinn_hmc_chains_draws call's (" + std::to_string(C.last_ndraws) + ")");
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, nc = (size_t)nchains, n = nc * (size_t)ndraws, row = 5 * P + hmc::SC_COUNT;
    if ((samples && plat_d2h(samples, C.d_samples, sizeof(double) * n * P, E.stream)) || (accept_prob && plat_d2h(accept_prob, C.d_stat, sizeof(double) * n, E.stream)) ||
        (logp && plat_d2h(logp, C.d_stat + n, sizeof(double) * n, E.stream)))
        return fail(std::string(who) + ": D2H copy failed");
    if (theta || logp_cur || grad) {                     // the chains' current states: one download of the state block
        std::vector<double> st(nc * row);
        if (plat_d2h(st.data(), C.d_state, sizeof(double) * st.size(), E.stream) || plat_sync(E.stream)) return fail(std::string(who) + ": D2H copy failed");
        for (size_t c = 0; c < nc; ++c) {
            const double* s = st.data() + c * row;
            if (theta) std::copy(s, s + P, theta + c * P);
            if (grad) std::copy(s + 3 * P, s + 4 * P, grad + c * P);
            if (logp_cur) logp_cur[c] = s[5 * P + hmc::SC_LP_CUR];
        }
    }
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

}  // extern "C"
