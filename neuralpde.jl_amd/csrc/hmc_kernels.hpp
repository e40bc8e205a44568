// hmc_kernels.hpp — the device-resident HMC transition of a Bayesian PINN (pinn_hmc_*): everything of a draw that is
// not the evaluation of the physics / data likelihood.  theta, momentum, inverse metric, log-posterior gradient and the energies live on the
// device in double; the host queues   momentum -> energy(old) -> [update -> evaluation] x n_leapfrog -> update -> energy(new) -> accept
// per draw and reads nothing back before the call's single download.
//   k_hmc_momentum : r_i = z_i / sqrt(minv_i), z from the counter-based generator (hmc_rules.hpp) or the caller's standard normals — the
//                    warm-up's metric changes inside the call —, or row i of the caller's finished momenta as given
//   k_hmc_leap<T>  : ONE launch per leapfrog step: log-posterior gradient from the evaluation's [gradient | sums] vector (T = double in float64
//                    mode, float otherwise) + the priors' gradient at theta_i, kick, drift, the copy of theta the next evaluation reads.
//                    from_sc (the warm-up; a template flag of the kernel): eps read from the scalar block (a uniform load), kick = kfac * eps,
//                    kfac in {1/2, 1} from the host
//   k_hmc_energy   : kinetic energy (sum minv r^2, or sum r v with v = M^-1 r of hmc_dense_kernels.hpp), log-prior, log-likelihood (from the K
//                    sums of squares) and H, one workgroup; double sums in a FIXED order: thread t takes elements t, t + 256, ...; per-wave
//                    butterfly (xor 32, 16, ... 1); the four waves in order.  No atomics.
//   k_hmc_accept   : a = exp(min(0, H_old - H_new)) (0 when H_new is not finite), u < a, elementwise selection of theta / gradient / logp,
//                    row `draw` of the sample buffer, accept_prob[draw], logp[draw]
// The warm-up (pinn_hmc_find_stepsize / pinn_hmc_warmup) adds, with the same bodies where a body exists:
//   k_hmc_accept_adapt    : accept_body; element 0 then runs adapt_body — dual averaging of eps (bpinn.py `_hmc_device`), the restart after a
//                           metric event, the final average — and writes the next draw's eps to the scalar block and to step_sizes[draw + 1]
//   k_hmc_window_metric   : minv_i = (k / (k + 5)) var_i + 1e-3 (5 / (k + 5)), var_i the population variance of column i over sample rows
//                           [w0, w1): mean first, then squared deviations, rows in order (numpy.var's two passes); one thread per parameter
// The arithmetic restates neuralpde.jl_amd/bpinn.py (`_hmc`, `logp_grad`, `Normal` / `LogNormal`) operation by operation, with floating-point
// contraction off: elementwise results equal the host sampler's bit for bit, sums to their order.
// Every body exists once; the PINN_EMU build runs the same bodies serially (the energy sums in the device's order).
#pragma once
#include "hmc_rules.hpp"

namespace hmc {

// ---- the warm-up ----
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
inline void launch_momentum(const Args& a, const double* z, const double* given, uint64_t seed, unsigned draw, plat_stream) {
    const unsigned key = rng_key((unsigned)seed, (unsigned)(seed >> 32), draw);
    for (int i = 0; i < a.P; ++i) momentum_body(i, a, z, given, key);
}
template <class T> inline void launch_leap(const Args& a, const T* ev, double kick, double eps, int from_sc, int drift, plat_stream) {
    HMC_NO_CONTRACT
    if (from_sc) { eps = a.sc[SC_EPS]; kick = kick * eps; }
    for (int i = 0; i < a.P; ++i) leap_body<T>(i, a, ev, kick, eps, drift);
}
inline void launch_energy(const Args& a, int mode, const double* sse, const double* v, plat_stream) {
    double tot[2] = {0.0, 0.0};
    for (int w = 0; w < BLOCK / 64; ++w) {
        double part[2][64];
        for (int l = 0; l < 64; ++l) {
            if (v) energy_partial<true>(w * 64 + l, a, mode == 1, part[0][l], part[1][l], v);
            else energy_partial(w * 64 + l, a, mode == 1, part[0][l], part[1][l]);
        }
        for (int q = 0; q < 2; ++q) {
            const double s = wave_butterfly(part[q]);
            tot[q] = w == 0 ? s : tot[q] + s;
        }
    }
    energy_finish(a, mode, tot[0], tot[1], sse);
}
inline void launch_accept(const Args& a, int draw, const double* uniforms, uint64_t seed, unsigned ctr, double* samples, double* accept_prob, double* logp, plat_stream) {
    const unsigned key = rng_key((unsigned)seed, (unsigned)(seed >> 32), ctr);
    for (int i = a.P - 1; i >= 0; --i) accept_body(i, a, draw, uniforms, key, samples, accept_prob, logp);      // (element 0 last: it overwrites logp(current))
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
__global__ void __launch_bounds__(BLOCK) k_hmc_momentum(const Args a, const double* z, const double* given, unsigned seed_lo, unsigned seed_hi, unsigned draw) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < a.P) momentum_body(i, a, z, given, rng_key(seed_lo, seed_hi, draw));
}
// FROM_SC is a compile-time flag: the kernel of pinn_hmc_draws carries neither the load nor the branch
template <class T, int FROM_SC> __global__ void __launch_bounds__(BLOCK) k_hmc_leap(const Args a, const T* ev, double kick, double eps, int drift) {
    HMC_NO_CONTRACT
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (FROM_SC) {
        eps = a.sc[SC_EPS];                              // (the same address in every lane)
        kick = kick * eps;
    }
    if (i < a.P) leap_body<T>(i, a, ev, kick, eps, drift);
}
__global__ void __launch_bounds__(BLOCK) k_hmc_energy(const Args a, int mode, const double* sse, const double* v) {
    __shared__ double sh[2][BLOCK / 64];
    double kin, pri;
    if (v) energy_partial<true>((int)threadIdx.x, a, mode == 1, kin, pri, v);      // (the same v in every thread)
    else energy_partial((int)threadIdx.x, a, mode == 1, kin, pri);
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
inline void launch_momentum(const Args& a, const double* z, const double* given, uint64_t seed, unsigned draw, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_momentum, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, z, given, (unsigned)seed, (unsigned)(seed >> 32), draw);
}
template <class T> inline void launch_leap(const Args& a, const T* ev, double kick, double eps, int from_sc, int drift, plat_stream st) {
    const dim3 grid((a.P + BLOCK - 1) / BLOCK);
    if (from_sc) hipLaunchKernelGGL((k_hmc_leap<T, 1>), grid, dim3(BLOCK), 0, st, a, ev, kick, eps, drift);
    else hipLaunchKernelGGL((k_hmc_leap<T, 0>), grid, dim3(BLOCK), 0, st, a, ev, kick, eps, drift);
}
inline void launch_energy(const Args& a, int mode, const double* sse, const double* v, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_energy, dim3(1), dim3(BLOCK), 0, st, a, mode, sse, v);
}
inline void launch_accept(const Args& a, int draw, const double* uniforms, uint64_t seed, unsigned ctr, double* samples, double* accept_prob, double* logp, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_accept, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, draw, uniforms, (unsigned)seed, (unsigned)(seed >> 32), ctr,
                       samples, accept_prob, logp);
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
