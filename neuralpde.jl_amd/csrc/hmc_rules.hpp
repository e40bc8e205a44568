// hmc_rules.hpp — the bodies of the resident HMC transition, written once: hmc_kernels.hpp launches them one kernel per
// phase (pinn_hmc_*), hmc_dense_kernels.hpp forms the same gradient and energy under a dense metric (section 4.16), hmc_chain_kernels.hpp runs
// them inside one workgroup per chain (pinn_hmc_chains_*; section 4.15).  The generator, the priors, the momentum, gradient, update, energy and
// accept bodies, their argument block and the emulation's wave butterfly; see hmc_kernels.hpp for what each restates.
#pragma once
#include <cmath>
#include <cstdint>
#include "plat.hpp"
#include "sample_rules.hpp"

namespace hmc {

#ifdef PINN_EMU
#define HMC_DEV inline
#else
#define HMC_DEV __device__ __forceinline__
#endif
#if defined(__clang__)
#define HMC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HMC_NO_CONTRACT
#endif

enum { SC_LP_CUR = 0, SC_H_OLD = 1, SC_H_NEW = 2, SC_LP_PROP = 3,
       SC_EPS = 4, SC_MU = 5, SC_HBAR = 6, SC_LOG_EPS_BAR = 7, SC_M = 8,      // the warm-up's step size and dual-averaging state (m as a double)
       SC_COUNT = 9 };
enum { ADAPT_RESTART = 1, ADAPT_LAST = 2 };
enum { PRIOR_NORMAL = 0, PRIOR_LOGNORMAL = 1 };
constexpr int BLOCK = 256;

struct Args {
    int P, K, nn, n_prior;               // nn = P - n_prior network weights under N(nn_mu, nn_sigma^2); then n_prior PDE parameters
    int sse_roundtrip;                   // float64 mode: the host path forms SSE_k as (sum / N_k) * N_k — restated so that logp is the same number
    double* th_cur; double* th_prop;     // [P] current state, proposal
    double* r;                           // [P] momentum
    double* g_cur; double* g_prop;       // [P] log-posterior gradient at th_cur / th_prop
    const double* minv;                  // [P] diagonal inverse metric
    double* sc;                          // [SC_COUNT] logp(current), H_old, H_new, logp(proposal); eps, mu, hbar, log_eps_bar, m of a warm-up
    double nn_mu, nn_sigma, nn_var, nn_const;      // nn_var = sigma^2, nn_const = nn (log sigma + 1/2 log 2 pi)
    const int* pr_kind; const double* pr_mu; const double* pr_sigma;      // [n_prior]
    const double* lik_c; const double* lik_d; const double* lik_n;        // [K] -N/2 log 2 pi - N log s | 2 s^2 | N_norm
    double* th_eval64; float* th_eval32; // where the next evaluation reads theta (one of them is null)
};

// ---- the generator (include/pinn_hip.h: pinn_hmc_draws) ----
HMC_DEV unsigned rng_key(unsigned seed_lo, unsigned seed_hi, unsigned draw) {
    const unsigned base = aux::mix32(seed_lo + 0x9E3779B9U * seed_hi);
    return aux::mix32(base ^ (draw * 0x85EBCA6BU + 0xC2B2AE35U));
}
HMC_DEV unsigned rng_word(unsigned key, unsigned e, unsigned j) { return aux::mix32(key ^ aux::mix32((2u * e + j) * 0x9E3779B9U + 0x165667B1U)); }
HMC_DEV double rng_normal(unsigned key, unsigned e) {
    const double u1 = ((double)rng_word(key, e, 0u) + 1.0) * (1.0 / 4294967296.0);      // (0, 1]
    const double u2 = (double)rng_word(key, e, 1u) * (1.0 / 4294967296.0);              // [0, 1)
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
HMC_DEV double rng_uniform(unsigned key, unsigned e) { return (double)rng_word(key, e, 0u) * (1.0 / 4294967296.0); }

HMC_DEV bool is_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }      // (false for NaN)

// log-density and its derivative of parameter prior j at x (bpinn.py: Normal / LogNormal .logpdf_grad)
HMC_DEV void prior_logpdf_grad(const Args& a, int j, double x, double& l, double& d) {
    HMC_NO_CONTRACT
    const double mu = a.pr_mu[j], sg = a.pr_sigma[j];
    if (a.pr_kind[j] == PRIOR_LOGNORMAL) {
        if (!(x > 0.0)) { l = -INFINITY; d = 0.0; return; }
        const double z = (log(x) - mu) / sg;
        l = -log(x * sg * 2.5066282746310002) - 0.5 * z * z;
        d = -1.0 / x - z / (sg * x);
    } else {
        const double z = (x - mu) / sg;
        l = -log(sg * 2.5066282746310002) - 0.5 * z * z;
        d = -z / sg;
    }
}

// `given`: row i of the caller's finished momenta; else z (the caller's standard normals, or the generator) under the metric in force
HMC_DEV void momentum_body(int i, const Args& a, const double* z, const double* given, unsigned key) {
    a.r[i] = given ? given[i] : (z ? z[i] : rng_normal(key, (unsigned)i)) / sqrt(a.minv[i]);
}

// element i of the gradient of logp at x: ev = the evaluation's [gradient of sum_k w_k L_k | ...] there, whose sign-flipped value is
// d loglik / d theta; then the weight prior's or the parameter prior's part
template <class T> HMC_DEV double logp_grad(int i, const Args& a, const T* ev, double x) {
    HMC_NO_CONTRACT
    double g = -(double)ev[i];
    if (i < a.nn) g -= (x - a.nn_mu) / a.nn_var;
    else {
        double l, d;
        prior_logpdf_grad(a, i - a.nn, x, l, d);
        g += d;
    }
    return g;
}

// ev == nullptr: the first half kick of a trajectory, from the stored gradient at the current state; otherwise ev = the evaluation at th_prop
template <class T> HMC_DEV void leap_body(int i, const Args& a, const T* ev, double kick, double eps, int drift) {
    HMC_NO_CONTRACT
    double g, x;
    if (!ev) {
        g = a.g_cur[i];
        x = a.th_cur[i];
    } else {
        x = a.th_prop[i];
        g = logp_grad<T>(i, a, ev, x);
        a.g_prop[i] = g;
    }
    const double r = a.r[i] + kick * g;
    a.r[i] = r;
    if (drift) {
        x = x + eps * a.minv[i] * r;
        a.th_prop[i] = x;
        if (a.th_eval64) a.th_eval64[i] = x;
        if (a.th_eval32) a.th_eval32[i] = (float)x;
    }
}

// thread t of BLOCK: its part of sum minv r^2 (DENSE: of sum r v, v = M^-1 r under a dense metric) and (with_prior) of sum ((w - mu) / sigma)^2
// over the network weights of the proposal.  The choice is made outside the loop, at compile time: a caller without v — the chain kernel —
// compiles to the diagonal loop alone
template <bool DENSE = false> HMC_DEV void energy_partial(int t, const Args& a, int with_prior, double& kin, double& pri, const double* v = nullptr) {
    HMC_NO_CONTRACT
    kin = 0.0; pri = 0.0;
    for (int i = t; i < a.P; i += BLOCK) {
        const double r = a.r[i];
        if constexpr (DENSE) kin += r * v[i];
        else kin += a.minv[i] * r * r;
        if (with_prior && i < a.nn) {
            const double z = (a.th_prop[i] - a.nn_mu) / a.nn_sigma;
            pri += z * z;
        }
    }
}
// logp(proposal) from the K sums of squares `sse`, the weights' sum of squares `pri` and the parameter priors at th_prop
HMC_DEV double logp_from_sums(const Args& a, double pri, const double* sse) {
    HMC_NO_CONTRACT
    double ll = 0.0;
    for (int k = 0; k < a.K; ++k) {
        double s = sse[k];
        if (a.sse_roundtrip) s = s / a.lik_n[k] * a.lik_n[k];
        ll += a.lik_c[k] - s / a.lik_d[k];
    }
    double lp = ll - 0.5 * pri - a.nn_const;
    for (int j = 0; j < a.n_prior; ++j) {
        double l, d;
        prior_logpdf_grad(a, j, a.th_prop[a.nn + j], l, d);
        lp += l;
    }
    return lp;
}
// mode 0: H_old = -logp(current) + kin / 2.  mode 1: logp(proposal) from the K sums of squares `sse` and the priors, H_new.
HMC_DEV void energy_finish(const Args& a, int mode, double kin, double pri, const double* sse) {
    HMC_NO_CONTRACT
    if (mode == 0) {
        a.sc[SC_H_OLD] = -a.sc[SC_LP_CUR] + 0.5 * kin;
        return;
    }
    const double lp = logp_from_sums(a, pri, sse);
    a.sc[SC_LP_PROP] = lp;
    a.sc[SC_H_NEW] = -lp + 0.5 * kin;
}

#ifdef PINN_EMU
// the device's 64-lane xor butterfly (32, 16, ... 1), restated: every lane adds its partner's value; lane 0's sum
inline double wave_butterfly(double* v) {
    for (int m = 32; m >= 1; m >>= 1) {
        double n[64];
        for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ m];
        for (int l = 0; l < 64; ++l) v[l] = n[l];
    }
    return v[0];
}
#endif

HMC_DEV void accept_body(int i, const Args& a, int draw, const double* uniforms, unsigned key, double* samples, double* accept_prob, double* logp) {
    const double h_old = a.sc[SC_H_OLD], h_new = a.sc[SC_H_NEW];
    double d = h_old - h_new;
    if (d > 0.0) d = 0.0;
    const double prob = is_finite(h_new) ? exp(d) : 0.0;
    const double u = uniforms ? uniforms[draw] : rng_uniform(key, (unsigned)a.P);
    const bool acc = u < prob;
    double x = a.th_cur[i];
    if (acc) {
        x = a.th_prop[i];
        a.th_cur[i] = x;
        a.g_cur[i] = a.g_prop[i];
    }
    if (samples) samples[(size_t)draw * a.P + i] = x;
    if (i == 0) {                                        // (nobody reads sc[SC_LP_CUR] in this launch)
        const double lp = acc ? a.sc[SC_LP_PROP] : a.sc[SC_LP_CUR];
        a.sc[SC_LP_CUR] = lp;
        accept_prob[draw] = prob;
        logp[draw] = lp;
    }
}

}  // namespace hmc
