// lbfgs_kernels.hpp — the device-resident L-BFGS finisher (pinn_lbfgs_init / _steps / _get): everything of the
// quasi-Newton iteration that is not the evaluation of the objective.  The iterate x, its gradient g, the trial point xn, the direction d, the
// curvature rings S[m][P], Y[m][P], rho[m] (a RING with a head index and a count: pairs are never shifted) and a small control block live on
// the device in double.  The host queues SLOTS back to back and reads nothing inside a chunk of them:
//     one slot = ONE k_lbfgs_step<T> launch + ONE full evaluation (objective and gradient) at the evaluation's copy of theta
// (T = the evaluation's element type: double in float64 mode, float otherwise; the evaluation is the handle's resident path, untouched).
// k_lbfgs_step<T> is one workgroup of 256 threads and a state machine on the control block:
//   JUDGE (when an evaluation is pending)   fn = sum_k w_k sums_k / n_norm_k as pinn_lbfgs's `eval` forms it; Armijo: isfinite(fn) && fn <= f + 1e-4 t gd.
//       accept: s = xn - x, y = gn - g; sy, ss, yy; the pair is pushed iff sy > 1e-10 sqrt(ss yy) (the oldest pair beyond `history` is evicted);
//               x <- xn, g <- gn, f <- fn, loss_hist[it++] = f
//       reject: t *= 0.5; after 30 trials status STALLED (terminal), otherwise status RETRY
//   PROPOSE   RETRY: only xn = x + t d and the evaluation's copy.  Otherwise: gmax > gtol or CONVERGED; it < the call's limit or MAXITER; the
//             two-loop recursion newest pair first, gamma = sy / yy of the newest pair; restart to -g with cleared rings when gd >= 0; first step
//             min(1, 1 / sqrt(g.g)) when the rings are empty, 1 otherwise; xn and the evaluation's copy.
//   In a terminal state (CONVERGED / STALLED / MAXITER) the launch does nothing.
// The arithmetic restates pinn_lbfgs (lbfgs.cpp) operation by operation with floating-point contraction off.  Every dot product has the fixed
// order of hmc::k_hmc_energy: thread t takes elements t, t + 256, ...; per-wave butterfly (xor 32, 16, ... 1); the four waves in order.  No
// atomics: the launch is bit-reproducible.  alpha and rho are held in LDS (<= 64 doubles each).  Every thread only ever touches the elements
// i = t (mod 256) of the vectors, so the vector passes need no barrier; a ring pair's address is base + slot * P + i with a workgroup-uniform
// slot, and every load in the ring loops is unconditional.
// THE ONE DIFFERENCE from pinn_lbfgs: a rejected trial costs a FULL evaluation here (the host routine runs rejected trials loss-only and
// re-evaluates the accepted point with a gradient); an accepted trial never needs re-evaluation.  The iterates are the same algorithm.
// The body exists once (step_body over a context); the PINN_EMU build runs it serially with the sums in the device's order.
#pragma once
#include <cmath>
#include <cstdint>
#include "plat.hpp"

namespace lbfgs {

#if defined(__clang__)
#define LBFGS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define LBFGS_NO_CONTRACT
#endif
#ifdef PINN_EMU
#define LBFGS_DEV inline
#else
#define LBFGS_DEV __device__ __forceinline__
#endif

enum { ST_RUN = 0, ST_RETRY = 1, ST_CONVERGED = 2, ST_STALLED = 3, ST_MAXITER = 4 };
enum { MODE_SLOT = 0, MODE_LOAD = 1, MODE_ADOPT = 2 };
constexpr int BLOCK = 256;
constexpr int MAX_HISTORY = 64;
constexpr int MAX_TRIALS = 30;

struct Ctl {                             // the control block: all the host ever downloads inside pinn_lbfgs_steps
    double f, t, gd;                     // objective at x; step and g.d of the running line search
    int status, ls, it, evals;           // ST_*; trials of the running line search; iterations / trial evaluations since pinn_lbfgs_init
    int head, count, pending, pad;       // ring: oldest pair's slot, pairs held; pending = an evaluation at xn awaits its judgement
};

struct Args {
    int P, K, m;                         // m = history
    int f64form;                         // objective formed as w_k * (sums_k / n_k) (float64 mode's eval) or (w_k * sums_k) / n_k (fp32 mode's)
    double* x; double* g; double* xn; double* d;      // [P]
    double* S; double* Y; double* rho;   // [m][P], [m][P], [m]
    Ctl* ctl;
    double* loss_hist;                   // objective after iteration it0 + i of the running call
    const double* w; const double* nrm;  // [K] term weights, n_norm
    const double* sums;                  // [K] raw sums of the evaluation, double
    double* th_eval64; float* th_eval32; // where the next evaluation reads theta (one of them is null)
};

LBFGS_DEV bool is_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }      // (false for NaN)

// C: the execution context — each(n, f): f(i) for the elements of this thread; sum(n, f) / amax(n, f): workgroup-uniform reductions of f(i);
// lead(): the one thread that writes scalars; sync(): workgroup barrier; al / rh: the LDS arrays
template <class T, class C> LBFGS_DEV void step_body(C& c, const Args& a, const T* ev, int mode, int it0, int it_end, double gtol) {
    LBFGS_NO_CONTRACT
    const int P = a.P, m = a.m;
    Ctl k = *a.ctl;                                      // every thread reads the block before anyone writes it (the barrier below)
    for (int j = c.first(); j < m; j += c.stride()) c.rh[j] = a.rho[j];
    c.sync();
    auto store_eval = [&](int i, double v) {
        if (a.th_eval64) a.th_eval64[i] = v;
        if (a.th_eval32) a.th_eval32[i] = (float)v;
    };
    auto objective = [&]() {
        LBFGS_NO_CONTRACT
        double fn = 0.0;
        for (int q = 0; q < a.K; ++q) fn += a.f64form ? a.w[q] * (a.sums[q] / a.nrm[q]) : a.w[q] * a.sums[q] / a.nrm[q];
        return fn;
    };
    if (mode == MODE_LOAD) {                             // the evaluation's copy <- x
        c.each(P, [&](int i) { store_eval(i, a.x[i]); });
        return;
    }
    if (mode == MODE_ADOPT) {                            // (f, g) <- the evaluation at x; rings cleared; nothing pending
        c.each(P, [&](int i) { a.g[i] = (double)ev[i]; });
        k.f = objective();
        k.status = ST_RUN; k.ls = 0; k.head = 0; k.count = 0; k.pending = 0; k.t = 0.0; k.gd = 0.0;
        if (c.lead()) *a.ctl = k;
        return;
    }
    if (k.status >= ST_CONVERGED) return;
    if (k.pending) {
        k.pending = 0;
        const double fn = objective();
        if (is_finite(fn) && fn <= k.f + 1e-4 * k.t * k.gd) {
            auto sv = [&](int i) { return a.xn[i] - a.x[i]; };
            auto yv = [&](int i) { return (double)ev[i] - a.g[i]; };
            const double sy = c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return sv(i) * yv(i); });
            const double ss = c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return sv(i) * sv(i); });
            const double yy = c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return yv(i) * yv(i); });
            const bool push = sy > 1e-10 * sqrt(ss * yy);
            int slot = k.head + k.count;
            if (slot >= m) slot -= m;                    // (count == m: the oldest pair's slot, overwritten)
            double* Sn = a.S + (size_t)slot * P;
            double* Yn = a.Y + (size_t)slot * P;
            c.each(P, [&](int i) {
                const double xi = a.xn[i], gi = (double)ev[i];
                if (push) { Sn[i] = xi - a.x[i]; Yn[i] = gi - a.g[i]; }
                a.x[i] = xi; a.g[i] = gi;
            });
            if (push) {
                if (c.lead()) { c.rh[slot] = 1.0 / sy; a.rho[slot] = 1.0 / sy; }
                if (k.count == m) { k.head = k.head + 1 == m ? 0 : k.head + 1; } else ++k.count;
                c.sync();
            }
            k.f = fn;
            if (c.lead()) a.loss_hist[k.it - it0] = fn;
            ++k.it;
            k.status = ST_RUN;
        } else {
            k.t *= 0.5;
            ++k.ls;
            k.status = k.ls >= MAX_TRIALS ? ST_STALLED : ST_RETRY;
        }
    }
    if (k.status == ST_RUN) {
        const double gmax = c.amax(P, [&](int i) { return a.g[i]; });
        if (!(gmax > gtol)) k.status = ST_CONVERGED;
        else if (!(k.it < it_end)) k.status = ST_MAXITER;
        else {
            // two-loop recursion: d = -H g, q held in d
            c.each(P, [&](int i) { a.d[i] = a.g[i]; });
            for (int j = k.count - 1; j >= 0; --j) {
                int slot = k.head + j;
                if (slot >= m) slot -= m;
                const double* Sj = a.S + (size_t)slot * P;
                const double* Yj = a.Y + (size_t)slot * P;
                const double al = c.rh[slot] * c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return Sj[i] * a.d[i]; });
                if (c.lead()) c.al[j] = al;
                c.each(P, [&](int i) { LBFGS_NO_CONTRACT a.d[i] -= al * Yj[i]; });
            }
            double gamma = 1.0;
            if (k.count > 0) {
                int slot = k.head + k.count - 1;
                if (slot >= m) slot -= m;
                const double* Sj = a.S + (size_t)slot * P;
                const double* Yj = a.Y + (size_t)slot * P;
                const double sy = c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return Sj[i] * Yj[i]; });
                const double yy = c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return Yj[i] * Yj[i]; });
                gamma = sy / yy;
            }
            c.each(P, [&](int i) { LBFGS_NO_CONTRACT a.d[i] *= gamma; });
            c.sync();                                    // (alpha of every pair is in LDS)
            for (int j = 0; j < k.count; ++j) {
                int slot = k.head + j;
                if (slot >= m) slot -= m;
                const double* Sj = a.S + (size_t)slot * P;
                const double* Yj = a.Y + (size_t)slot * P;
                const double beta = c.rh[slot] * c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return Yj[i] * a.d[i]; });
                const double ab = c.al[j] - beta;
                c.each(P, [&](int i) { LBFGS_NO_CONTRACT a.d[i] += ab * Sj[i]; });
            }
            c.each(P, [&](int i) { a.d[i] = -a.d[i]; });
            k.gd = c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return a.g[i] * a.d[i]; });
            if (!(k.gd < 0.0)) {                         // not a descent direction (stale curvature): restart from steepest descent
                k.head = 0; k.count = 0;
                c.each(P, [&](int i) { a.d[i] = -a.g[i]; });
                k.gd = c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return a.g[i] * a.d[i]; });
            }
            k.t = 1.0;
            if (k.count == 0) {
                const double gg = c.sum(P, [&](int i) { LBFGS_NO_CONTRACT return a.g[i] * a.g[i]; });
                const double r = 1.0 / sqrt(gg);
                k.t = r < 1.0 ? r : 1.0;                 // std::min(1.0, r)
            }
            k.ls = 0;
        }
    }
    if (k.status == ST_RUN || k.status == ST_RETRY) {
        const double t = k.t;
        c.each(P, [&](int i) {
            LBFGS_NO_CONTRACT
            const double v = a.x[i] + t * a.d[i];
            a.xn[i] = v;
            store_eval(i, v);
        });
        k.pending = 1;
        ++k.evals;
    }
    if (c.lead()) *a.ctl = k;
}

#ifdef PINN_EMU
struct EmuCtx {
    double al[MAX_HISTORY], rh[MAX_HISTORY];
    int first() const { return 0; }
    int stride() const { return 1; }
    bool lead() const { return true; }
    void sync() {}
    template <class F> void each(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
    template <class F> double sum(int n, F f) {          // the device's order: strided partials, per-wave butterfly, the waves in order
        LBFGS_NO_CONTRACT
        double tot = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) {
            double v[64];
            for (int l = 0; l < 64; ++l) {
                double s = 0.0;
                for (int i = w * 64 + l; i < n; i += BLOCK) s += f(i);
                v[l] = s;
            }
            for (int msk = 32; msk >= 1; msk >>= 1) {
                double nx[64];
                for (int l = 0; l < 64; ++l) nx[l] = v[l] + v[l ^ msk];
                for (int l = 0; l < 64; ++l) v[l] = nx[l];
            }
            tot = w == 0 ? v[0] : tot + v[0];
        }
        return tot;
    }
    template <class F> double amax(int n, F f) {
        double mx = 0.0;
        for (int i = 0; i < n; ++i) mx = fmax(mx, fabs(f(i)));
        return mx;
    }
};
template <class T> inline void launch_step(const Args& a, const T* ev, int mode, int it0, int it_end, double gtol, plat_stream) {
    EmuCtx c;
    step_body<T>(c, a, ev, mode, it0, it_end, gtol);
}
#else
struct DevCtx {
    double* al; double* rh; double* sh;
    int t;
    __device__ __forceinline__ int first() const { return t; }
    __device__ __forceinline__ int stride() const { return BLOCK; }
    __device__ __forceinline__ bool lead() const { return t == 0; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    template <class F> __device__ __forceinline__ void each(int n, F f) { for (int i = t; i < n; i += BLOCK) f(i); }
    template <class F> __device__ __forceinline__ double sum(int n, F f) {
        LBFGS_NO_CONTRACT
        double v = 0.0;
        for (int i = t; i < n; i += BLOCK) v += f(i);
        for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk, 64);
        if ((t & 63) == 0) sh[t >> 6] = v;
        __syncthreads();
        v = sh[0];
        for (int w = 1; w < BLOCK / 64; ++w) v += sh[w];
        __syncthreads();                                 // (sh is free for the next reduction)
        return v;
    }
    template <class F> __device__ __forceinline__ double amax(int n, F f) {
        double v = 0.0;
        for (int i = t; i < n; i += BLOCK) v = fmax(v, fabs(f(i)));
        for (int msk = 32; msk >= 1; msk >>= 1) v = fmax(v, __shfl_xor(v, msk, 64));
        if ((t & 63) == 0) sh[t >> 6] = v;
        __syncthreads();
        v = sh[0];
        for (int w = 1; w < BLOCK / 64; ++w) v = fmax(v, sh[w]);
        __syncthreads();
        return v;
    }
};
template <class T> __global__ void __launch_bounds__(BLOCK) k_lbfgs_step(const Args a, const T* ev, int mode, int it0, int it_end, double gtol) {
    __shared__ double al[MAX_HISTORY], rh[MAX_HISTORY], sh[BLOCK / 64];
    DevCtx c{al, rh, sh, (int)threadIdx.x};
    step_body<T>(c, a, ev, mode, it0, it_end, gtol);
}
template <class T> inline void launch_step(const Args& a, const T* ev, int mode, int it0, int it_end, double gtol, plat_stream st) {
    hipLaunchKernelGGL(k_lbfgs_step<T>, dim3(1), dim3(BLOCK), 0, st, a, ev, mode, it0, it_end, gtol);
}
#endif

}  // namespace lbfgs
