// hmc_kernels.hpp — the device-resident HMC transition of a Bayesian PINN (pinn_hmc_*): everything of a draw that is
// not the evaluation of the physics / data likelihood.  theta, momentum, inverse metric, log-posterior gradient and the energies live on the
// device in double; the host queues   momentum -> energy(old) -> [update -> evaluation] x n_leapfrog -> update -> energy(new) -> accept
// per draw and reads nothing back before the call's single download.
//   k_hmc_momentum : r_i = z_i / sqrt(minv_i), z from the counter-based generator below (or row i of the caller's momenta)
//   k_hmc_leap<T>  : ONE launch per leapfrog step: log-posterior gradient from the evaluation's [gradient | sums] vector (T = double in float64
//                    mode, float otherwise) + the priors' gradient at theta_i, kick, drift, the copy of theta the next evaluation reads
//   k_hmc_energy   : kinetic energy, log-prior, log-likelihood (from the K sums of squares) and H, one workgroup; double sums in a FIXED order:
//                    thread t takes elements t, t + 256, ...; per-wave butterfly (xor 32, 16, ... 1); the four waves in order.  No atomics.
//   k_hmc_accept   : a = exp(min(0, H_old - H_new)) (0 when H_new is not finite), u < a, elementwise selection of theta / gradient / logp,
//                    row `draw` of the sample buffer, accept_prob[draw], logp[draw]
// The warm-up (pinn_hmc_find_stepsize / pinn_hmc_warmup) adds, with the same bodies where a body exists:
//   k_hmc_momentum_z      : r_i = z_i / sqrt(minv_i) with z from the caller's standard normals (or the generator): the metric changes inside the call
//   k_hmc_leap_dev<T>     : leap_body with eps read from the scalar block (a uniform load), kick = kfac * eps, kfac in {1/2, 1} from the host
//   k_hmc_accept_adapt    : accept_body; element 0 then runs adapt_body — dual averaging of eps (bpinn.py `_hmc_device`), the restart after a
//                           metric event, the final average — and writes the next draw's eps to the scalar block and to step_sizes[draw + 1]
//   k_hmc_window_metric   : minv_i = (k / (k + 5)) var_i + 1e-3 (5 / (k + 5)), var_i the population variance of column i over sample rows
//                           [w0, w1): mean first, then squared deviations, rows in order (numpy.var's two passes); one thread per parameter
// The arithmetic restates neuralpde.jl_amd/bpinn.py (`_hmc`, `logp_grad`, `Normal` / `LogNormal`) operation by operation, with floating-point
// contraction off: elementwise results equal the host sampler's bit for bit, sums to their order.
// Every body exists once; the PINN_EMU build runs the same bodies serially (the energy sums in the device's order).
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

HMC_DEV void momentum_body(int i, const Args& a, const double* row, unsigned key) {
    a.r[i] = row ? row[i] : rng_normal(key, (unsigned)i) / sqrt(a.minv[i]);
}

// ev == nullptr: the first half kick of a trajectory, from the stored gradient at the current state; otherwise ev = the evaluation's
// [gradient of sum_k w_k L_k | ...] at th_prop, whose sign-flipped value is d loglik / d theta
template <class T> HMC_DEV void leap_body(int i, const Args& a, const T* ev, double kick, double eps, int drift) {
    HMC_NO_CONTRACT
    double g, x;
    if (!ev) {
        g = a.g_cur[i];
        x = a.th_cur[i];
    } else {
        x = a.th_prop[i];
        g = -(double)ev[i];
        if (i < a.nn) g -= (x - a.nn_mu) / a.nn_var;
        else {
            double l, d;
            prior_logpdf_grad(a, i - a.nn, x, l, d);
            g += d;
        }
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

// thread t of BLOCK: its part of sum minv r^2 and (with_prior) of sum ((w - mu) / sigma)^2 over the network weights of the proposal
HMC_DEV void energy_partial(int t, const Args& a, int with_prior, double& kin, double& pri) {
    HMC_NO_CONTRACT
    kin = 0.0; pri = 0.0;
    for (int i = t; i < a.P; i += BLOCK) {
        const double r = a.r[i];
        kin += a.minv[i] * r * r;
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

// ---- the warm-up ----
HMC_DEV void momentum_z_body(int i, const Args& a, const double* z, unsigned key) {
    a.r[i] = (z ? z[i] : rng_normal(key, (unsigned)i)) / sqrt(a.minv[i]);
}

// bpinn.py `_hmc_device`, the adaptation after a draw with acceptance probability `acc`, in its order of operations; element 0 of the accept
// launch only.  flags: what the host knows from (draw, n_adapts) alone.  `next` = step_sizes[draw + 1] (the final step size after the last draw).
HMC_DEV void adapt_body(const Args& a, double acc, double target, int flags, double* next) {
    HMC_NO_CONTRACT
    const double t0 = 10.0, gamma = 0.05, kappa = 0.75;
    double mu = a.sc[SC_MU], hbar = a.sc[SC_HBAR], leb = a.sc[SC_LOG_EPS_BAR], m = a.sc[SC_M];
    m = m + 1.0;
    hbar = (1.0 - 1.0 / (m + t0)) * hbar + (target - acc) / (m + t0);
    const double log_eps = mu - sqrt(m) / gamma * hbar;
    const double eta = pow(m, -kappa);
    leb = eta * log_eps + (1.0 - eta) * leb;
    double eps = exp(log_eps);
    if (flags & ADAPT_RESTART) {                         // a new metric follows this launch: search again from the step just found
        mu = log(10.0 * eps);
        hbar = 0.0; leb = 0.0; m = 0.0;
    }
    if ((flags & ADAPT_LAST) && m > 0.0) eps = exp(leb);
    a.sc[SC_MU] = mu; a.sc[SC_HBAR] = hbar; a.sc[SC_LOG_EPS_BAR] = leb; a.sc[SC_M] = m;
    a.sc[SC_EPS] = eps;                                  // (its first readers are the next draw's launches)
    *next = eps;
}

HMC_DEV void window_metric_body(int i, const Args& a, double* minv, const double* samples, int w0, int w1) {
    HMC_NO_CONTRACT
    const double k = (double)(w1 - w0);
    double s = 0.0;
    for (int row = w0; row < w1; ++row) s += samples[(size_t)row * a.P + i];
    const double mean = s / k;
    double q = 0.0;
    for (int row = w0; row < w1; ++row) {
        const double d = samples[(size_t)row * a.P + i] - mean;
        q += d * d;
    }
    minv[i] = (k / (k + 5.0)) * (q / k) + 1e-3 * (5.0 / (k + 5.0));
}

#ifdef PINN_EMU
inline void launch_momentum(const Args& a, const double* row, uint64_t seed, unsigned draw, plat_stream) {
    const unsigned key = rng_key((unsigned)seed, (unsigned)(seed >> 32), draw);
    for (int i = 0; i < a.P; ++i) momentum_body(i, a, row, key);
}
template <class T> inline void launch_leap(const Args& a, const T* ev, double kick, double eps, int drift, plat_stream) {
    for (int i = 0; i < a.P; ++i) leap_body<T>(i, a, ev, kick, eps, drift);
}
inline void launch_energy(const Args& a, int mode, const double* sse, plat_stream) {
    double tot[2] = {0.0, 0.0};
    for (int w = 0; w < BLOCK / 64; ++w) {
        double v[2][64];
        for (int l = 0; l < 64; ++l) energy_partial(w * 64 + l, a, mode == 1, v[0][l], v[1][l]);
        for (int q = 0; q < 2; ++q) {
            for (int m = 32; m >= 1; m >>= 1) {          // the device's butterfly: every lane adds its partner's value
                double n[64];
                for (int l = 0; l < 64; ++l) n[l] = v[q][l] + v[q][l ^ m];
                for (int l = 0; l < 64; ++l) v[q][l] = n[l];
            }
            tot[q] = w == 0 ? v[q][0] : tot[q] + v[q][0];
        }
    }
    energy_finish(a, mode, tot[0], tot[1], sse);
}
inline void launch_accept(const Args& a, int draw, const double* uniforms, uint64_t seed, unsigned ctr, double* samples, double* accept_prob, double* logp, plat_stream) {
    const unsigned key = rng_key((unsigned)seed, (unsigned)(seed >> 32), ctr);
    for (int i = a.P - 1; i >= 0; --i) accept_body(i, a, draw, uniforms, key, samples, accept_prob, logp);      // (element 0 last: it overwrites logp(current))
}
inline void launch_momentum_z(const Args& a, const double* z, uint64_t seed, unsigned draw, plat_stream) {
    const unsigned key = rng_key((unsigned)seed, (unsigned)(seed >> 32), draw);
    for (int i = 0; i < a.P; ++i) momentum_z_body(i, a, z, key);
}
template <class T> inline void launch_leap_dev(const Args& a, const T* ev, double kfac, int drift, plat_stream) {
    HMC_NO_CONTRACT
    const double eps = a.sc[SC_EPS];
    for (int i = 0; i < a.P; ++i) leap_body<T>(i, a, ev, kfac * eps, eps, drift);
}
inline void launch_accept_adapt(const Args& a, int draw, const double* uniforms, uint64_t seed, unsigned ctr, double* samples, double* accept_prob, double* logp,
                                double target, int flags, double* step_sizes, plat_stream) {
    const unsigned key = rng_key((unsigned)seed, (unsigned)(seed >> 32), ctr);
    for (int i = a.P - 1; i >= 0; --i) accept_body(i, a, draw, uniforms, key, samples, accept_prob, logp);
    adapt_body(a, accept_prob[draw], target, flags, step_sizes + draw + 1);
}
inline void launch_window_metric(const Args& a, const double* samples, int w0, int w1, plat_stream) {
    for (int i = 0; i < a.P; ++i) window_metric_body(i, a, const_cast<double*>(a.minv), samples, w0, w1);
}
#else
__global__ void __launch_bounds__(BLOCK) k_hmc_momentum(const Args a, const double* row, unsigned seed_lo, unsigned seed_hi, unsigned draw) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < a.P) momentum_body(i, a, row, rng_key(seed_lo, seed_hi, draw));
}
template <class T> __global__ void __launch_bounds__(BLOCK) k_hmc_leap(const Args a, const T* ev, double kick, double eps, int drift) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < a.P) leap_body<T>(i, a, ev, kick, eps, drift);
}
__global__ void __launch_bounds__(BLOCK) k_hmc_energy(const Args a, int mode, const double* sse) {
    __shared__ double sh[2][BLOCK / 64];
    double kin, pri;
    energy_partial((int)threadIdx.x, a, mode == 1, kin, pri);
    for (int m = 32; m >= 1; m >>= 1) {
        kin += __shfl_xor(kin, m, 64);
        pri += __shfl_xor(pri, m, 64);
    }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = kin; sh[1][threadIdx.x >> 6] = pri; }
    __syncthreads();
    if (threadIdx.x == 0) {
        kin = sh[0][0]; pri = sh[1][0];
        for (int w = 1; w < BLOCK / 64; ++w) { kin += sh[0][w]; pri += sh[1][w]; }
        energy_finish(a, mode, kin, pri, sse);
    }
}
__global__ void __launch_bounds__(BLOCK) k_hmc_accept(const Args a, int draw, const double* uniforms, unsigned seed_lo, unsigned seed_hi, unsigned ctr,
                                                      double* samples, double* accept_prob, double* logp) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < a.P) accept_body(i, a, draw, uniforms, rng_key(seed_lo, seed_hi, ctr), samples, accept_prob, logp);
}
__global__ void __launch_bounds__(BLOCK) k_hmc_momentum_z(const Args a, const double* z, unsigned seed_lo, unsigned seed_hi, unsigned draw) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < a.P) momentum_z_body(i, a, z, rng_key(seed_lo, seed_hi, draw));
}
template <class T> __global__ void __launch_bounds__(BLOCK) k_hmc_leap_dev(const Args a, const T* ev, double kfac, int drift) {
    HMC_NO_CONTRACT
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    const double eps = a.sc[SC_EPS];                     // (the same address in every lane)
    if (i < a.P) leap_body<T>(i, a, ev, kfac * eps, eps, drift);
}
__global__ void __launch_bounds__(BLOCK) k_hmc_accept_adapt(const Args a, int draw, const double* uniforms, unsigned seed_lo, unsigned seed_hi, unsigned ctr,
                                                            double* samples, double* accept_prob, double* logp, double target, int flags, double* step_sizes) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < a.P) accept_body(i, a, draw, uniforms, rng_key(seed_lo, seed_hi, ctr), samples, accept_prob, logp);
    if (i == 0) adapt_body(a, accept_prob[draw], target, flags, step_sizes + draw + 1);      // (nobody reads the adaptation scalars in this launch)
}
__global__ void __launch_bounds__(BLOCK) k_hmc_window_metric(const Args a, double* minv, const double* samples, int w0, int w1) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < a.P) window_metric_body(i, a, minv, samples, w0, w1);
}
inline void launch_momentum(const Args& a, const double* row, uint64_t seed, unsigned draw, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_momentum, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, row, (unsigned)seed, (unsigned)(seed >> 32), draw);
}
template <class T> inline void launch_leap(const Args& a, const T* ev, double kick, double eps, int drift, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_leap<T>, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, ev, kick, eps, drift);
}
inline void launch_energy(const Args& a, int mode, const double* sse, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_energy, dim3(1), dim3(BLOCK), 0, st, a, mode, sse);
}
inline void launch_accept(const Args& a, int draw, const double* uniforms, uint64_t seed, unsigned ctr, double* samples, double* accept_prob, double* logp, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_accept, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, draw, uniforms, (unsigned)seed, (unsigned)(seed >> 32), ctr,
                       samples, accept_prob, logp);
}
inline void launch_momentum_z(const Args& a, const double* z, uint64_t seed, unsigned draw, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_momentum_z, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, z, (unsigned)seed, (unsigned)(seed >> 32), draw);
}
template <class T> inline void launch_leap_dev(const Args& a, const T* ev, double kfac, int drift, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_leap_dev<T>, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, ev, kfac, drift);
}
inline void launch_accept_adapt(const Args& a, int draw, const double* uniforms, uint64_t seed, unsigned ctr, double* samples, double* accept_prob, double* logp,
                                double target, int flags, double* step_sizes, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_accept_adapt, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, draw, uniforms, (unsigned)seed, (unsigned)(seed >> 32), ctr,
                       samples, accept_prob, logp, target, flags, step_sizes);
}
inline void launch_window_metric(const Args& a, const double* samples, int w0, int w1, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_window_metric, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, const_cast<double*>(a.minv), samples, w0, w1);
}
#endif

}  // namespace hmc
