// nuts_emu_check.cpp — stand-alone check of the resident NUTS kernel's body (csrc/nuts_kernels.hpp, with hmc_kernels.hpp and the contexts of
// qn_kernels.hpp) in its serial emulation under the host sanitizers.  Nothing of the engine is linked: the "evaluation" is written by this
// program for the target  loglik = -1/2 sum a_i x_i^2  (one term: raw sum = sum a_i x_i^2, lik_d = 2; ev = [a_i x_i | .]), with the N(0, 2^2)
// prior on all but the last parameter and a LogNormal(0, 1) prior on the last, and the slot loop of hmc.cpp (pinn_nuts_draws) is restated
// around nuts::launch_step.  Every buffer has exactly the size hmc.cpp gives it, so an index out of range is the sanitizer's to report.
// Cases: P = 5 and P = 321 (two strides of the 256 "threads"); max_depth 1, 5 and 10 (the last checkpoint slot in use); the generator and
// supplied normals / uniforms; both element types; a step so large that draws diverge.  Exit status 0 iff every draw of every run completes
// with finite outputs, 0 <= tree_depth <= D, 1 <= n_leapfrog <= 2^D - 1, accept_stat in [0, 1], the state equal to the last sample row, and a
// run repeated with the generator's own values supplied is bit-equal.  A CPU program: from the repository root
//   g++ -std=c++17 -DPINN_EMU -g -fsanitize=address,undefined -Ineuralpde.jl_amd/csrc tools/micro/nuts_emu_check.cpp -o /tmp/nuts_emu_check && /tmp/nuts_emu_check
#include "nuts_kernels.hpp"
#include <cstdio>
#include <vector>

struct Out {
    std::vector<double> samples, acc, lp, state;
    std::vector<int> depth, nleap, div;
    int slots = 0;
    bool operator==(const Out& o) const { return samples == o.samples && acc == o.acc && lp == o.lp && state == o.state && depth == o.depth && nleap == o.nleap && div == o.div; }
};

template <class T> static int run(int P, int D, int ndraws, double eps, bool supplied, Out& out) {
    const int K = 1, n_prior = 1, nu = 2 * D + (1 << D) - 1;
    std::vector<double> state((size_t)6 * P + hmc::SC_COUNT, 0.0), tab(2 * n_prior + 3 * K), tree((size_t)(12 + 2 * nuts::MAX_DEPTH) * P, 0.0);
    std::vector<int> kind(n_prior, hmc::PRIOR_LOGNORMAL);
    std::vector<T> th(P), ev(P + K);
    std::vector<double> sse(K), curv(P);
    for (int i = 0; i < P; ++i) curv[i] = 0.5 + 3.0 * ((i * 7) % 11) / 11.0;
    hmc::Args a;
    std::memset(&a, 0, sizeof a);
    a.P = P; a.K = K; a.n_prior = n_prior; a.nn = P - n_prior; a.sse_roundtrip = sizeof(T) == 8;
    a.th_cur = state.data(); a.th_prop = a.th_cur + P; a.r = a.th_prop + P; a.g_cur = a.r + P; a.g_prop = a.g_cur + P;
    double* minv = a.g_prop + P;
    a.minv = minv; a.sc = minv + P;
    a.nn_mu = 0.0; a.nn_sigma = 2.0; a.nn_var = 4.0; a.nn_const = a.nn * (std::log(2.0) + 0.5 * std::log(2.0 * 3.14159265358979323846));
    tab[0] = 0.0; tab[1] = 1.0; tab[2] = 0.0; tab[3] = 2.0; tab[4] = 1.0;
    a.pr_mu = tab.data(); a.pr_sigma = tab.data() + 1; a.lik_c = tab.data() + 2; a.lik_d = tab.data() + 3; a.lik_n = tab.data() + 4;
    a.pr_kind = kind.data();
    if constexpr (sizeof(T) == 8) a.th_eval64 = th.data();
    else a.th_eval32 = th.data();
    auto evaluate = [&] {
        double s = 0.0;
        for (int i = 0; i < P; ++i) { const double x = (double)th[i]; ev[i] = (T)(curv[i] * x); s += curv[i] * x * x; }
        ev[P] = (T)s;
        sse[0] = s;
    };
    // the chain's start as pinn_hmc_init leaves it: theta, its gradient and logp
    for (int i = 0; i < P; ++i) { a.th_cur[i] = a.th_prop[i] = 0.3 + 0.1 * ((i % 5) - 2); th[i] = (T)a.th_cur[i]; minv[i] = 0.5 + ((i * 3) % 7) / 7.0; }
    evaluate();
    for (int i = 0; i < P; ++i) hmc::leap_body<T>(i, a, ev.data(), 0.0, 0.0, 0);
    hmc::launch_energy(a, 1, sse.data(), nullptr);
    for (int i = 0; i < P; ++i) a.g_cur[i] = a.g_prop[i];
    a.sc[hmc::SC_LP_CUR] = a.sc[hmc::SC_LP_PROP];

    const uint64_t seed = (1ull << 40) + 77;
    std::vector<double> z, u;
    if (supplied) {                                      // the generator's own values, through the same functions
        z.resize((size_t)ndraws * P); u.resize((size_t)ndraws * nu);
        for (int d = 0; d < ndraws; ++d) {
            const unsigned key = hmc::rng_key((unsigned)seed, (unsigned)(seed >> 32), (unsigned)d);
            for (int i = 0; i < P; ++i) z[(size_t)d * P + i] = hmc::rng_normal(key, (unsigned)i);
            for (int k = 0; k < nu; ++k) u[(size_t)d * nu + k] = hmc::rng_uniform(key, (unsigned)(P + k));
        }
    }
    out.samples.assign((size_t)ndraws * P, 0.0); out.acc.assign(ndraws, 0.0); out.lp.assign(ndraws, 0.0);
    out.depth.assign(ndraws, -1); out.nleap.assign(ndraws, -1); out.div.assign(ndraws, -1);
    nuts::Ctl ctl;
    std::memset(&ctl, 0, sizeof ctl);
    ctl.status = nuts::ST_RUN; ctl.fresh = 1;
    nuts::Tree q;
    std::memset(&q, 0, sizeof q);
    q.ctl = &ctl;
    double* v = tree.data();
    for (double** f : {&q.th_l, &q.r_l, &q.g_l, &q.th_r, &q.r_r, &q.g_r, &q.th_sc, &q.g_sc, &q.th_tc, &q.g_tc, &q.rho, &q.rho_sub}) { *f = v; v += P; }
    q.r_ck = v; q.rho_ck = v + (size_t)nuts::MAX_DEPTH * P;
    q.normals = supplied ? z.data() : nullptr; q.uniforms = supplied ? u.data() : nullptr;
    q.samples = out.samples.data(); q.accept_stat = out.acc.data(); q.logp = out.lp.data();
    q.tree_depth = out.depth.data(); q.n_leapfrog = out.nleap.data(); q.divergent = out.div.data();
    q.ndraws = ndraws; q.max_depth = D; q.nu = nu; q.eps = eps; q.delta_max = 1000.0;
    q.seed_lo = (unsigned)seed; q.seed_hi = (unsigned)(seed >> 32); q.ctr0 = 0;
    nuts::launch_step<T>(a, q, ev.data(), sse.data(), nullptr);
    const long long max_slots = (long long)ndraws * ((1 << D) - 1);
    for (out.slots = 0; ctl.status == nuts::ST_RUN && out.slots < max_slots; ++out.slots) {
        evaluate();
        nuts::launch_step<T>(a, q, ev.data(), sse.data(), nullptr);
    }
    out.state.assign(a.th_cur, a.th_cur + P);
    int bad = ctl.status != nuts::ST_DONE || ctl.draw != ndraws;
    long long leaves = 0;
    for (int d = 0; d < ndraws; ++d) {
        bad += !(out.depth[d] >= 0 && out.depth[d] <= D) || !(out.nleap[d] >= 1 && out.nleap[d] <= (1 << D) - 1) || !(out.div[d] == 0 || out.div[d] == 1);
        bad += !(out.acc[d] >= 0.0 && out.acc[d] <= 1.0) || !hmc::is_finite(out.lp[d]);
        for (int i = 0; i < P; ++i) bad += !hmc::is_finite(out.samples[(size_t)d * P + i]);
        leaves += out.nleap[d];
    }
    bad += leaves != out.slots;                          // one slot per leaf, none behind the last draw in this loop
    for (int i = 0; i < P; ++i) bad += out.state[i] != out.samples[(size_t)(ndraws - 1) * P + i];
    bad += !(out.state[P - 1] > 0.0);                    // the LogNormal parameter never leaves its support
    int ndiv = 0, dmax = 0;
    for (int d = 0; d < ndraws; ++d) { ndiv += out.div[d]; dmax = out.depth[d] > dmax ? out.depth[d] : dmax; }
    std::printf("nuts %-6s P=%3d D=%2d eps %-5g %-9s draws %d  leaves %5lld  deepest %2d  divergent %d  accept_stat[0] %.4f  %s\n", sizeof(T) == 8 ? "double" : "float", P, D,
                eps, supplied ? "supplied" : "generator", ndraws, leaves, dmax, ndiv, out.acc[0], bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

template <class T> static int both(int P, int D, int ndraws, double eps) {
    Out g, s;
    int bad = run<T>(P, D, ndraws, eps, false, g) + run<T>(P, D, ndraws, eps, true, s);
    if (!(g == s)) { std::printf("the run supplied with the generator's values differs from the generator's run\n"); ++bad; }
    return bad;
}

int main() {
    int bad = 0;
    for (int P : {5, 321}) {
        bad += both<double>(P, 1, 4, 0.05) + both<float>(P, 1, 4, 0.05);
        bad += both<double>(P, 5, 4, 0.05) + both<float>(P, 5, 4, 0.05);
        bad += both<double>(P, 10, 3, 0.002) + both<float>(P, 10, 3, 0.002);
        bad += both<double>(P, 4, 3, 5.0);
    }
    if (bad) { std::printf("nuts_emu_check: %d run(s) FAILED\n", bad); return 1; }
    std::puts("nuts_emu_check: ok");
    return 0;
}
