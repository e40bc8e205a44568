// qn_kernels.hpp — what the two device-resident quasi-Newton finishers share on the device (lbfgs_kernels.hpp, DESIGN.md section 4.8;
// bfgs_kernels.hpp, section 4.12; these two and the host driver qn_host.hpp include it, and nuts_kernels.hpp for the execution contexts DevCtx / EmuCtx alone): everything of the iteration except how the direction d = -H g and the curvature
// update are formed.  The iterate x, its gradient g, the trial point xn, the direction d and a small control block live on the device in double.
// A control kernel is ONE workgroup of 256 threads and a state machine on the control block:
//   JUDGE (when an evaluation is pending)   fn = sum_k w_k sums_k / n_norm_k as pinn_lbfgs's `eval` forms it; Armijo: isfinite(fn) && fn <= f + 1e-4 t gd.
//       accept: s = xn - x, y = gn - g; the solver's curvature update is due iff s.y > 1e-10 sqrt(s.s y.y); x <- xn, g <- gn, f <- fn, loss_hist[it++] = f
//       reject: t *= 0.5; after 30 trials status STALLED (terminal), otherwise status RETRY
//   PROPOSE   RETRY: only xn = x + t d and the evaluation's copy.  RUN: max |g_i| > gtol or CONVERGED (a NaN entry is skipped); it < the call's
//             limit or MAXITER; the solver's d; gd = g.d; not gd < 0: restart, d = -g; t = 1, or min(1, 1 / sqrt(g.g)) while H is the unscaled
//             identity; xn and the evaluation's copy.
//   In a terminal state (CONVERGED / STALLED / MAXITER) the launch does nothing.
// The arithmetic restates pinn_lbfgs (lbfgs.cpp) operation by operation with floating-point contraction off (the pragma is repeated in every
// lambda that multiplies and adds: a lambda's body does not inherit it).  Every dot product has the fixed order of hmc::k_hmc_energy: thread t
// takes elements t, t + 256, ...; per-wave butterfly (xor 32, 16, ... 1); the four waves in order.  No atomics: a launch is bit-reproducible.
// Every thread only ever touches the elements i = t (mod 256) of the vectors, so the vector passes need no barrier.
// Each body exists once, over a context: DevCtx on the device, EmuCtx (PINN_EMU) serially with the sums in the device's order.
#pragma once
#include <cmath>
#include <cstdint>
#include "plat.hpp"

namespace qn {

#if defined(__clang__)
#define QN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define QN_NO_CONTRACT
#endif
#ifdef PINN_EMU
#define QN_DEV inline
#else
#define QN_DEV __device__ __forceinline__
#endif

enum { ST_RUN = 0, ST_RETRY = 1, ST_CONVERGED = 2, ST_STALLED = 3, ST_MAXITER = 4 };
constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int MAX_TRIALS = 30;

struct Ctl {                             // the common part of a control block (a solver's Ctl derives from it and is all the host downloads inside _steps)
    double f, t, gd;                     // objective at x; step and g.d of the running line search
    int status, ls, it, evals;           // ST_*; trials of the running line search; iterations / trial evaluations since _init
    int pending;                         // an evaluation at xn awaits its judgement
};

struct Args {                            // the common part of a control kernel's arguments
    int P, K;
    int f64form;                         // objective formed as w_k * (sums_k / n_k) (float64 mode's eval) or (w_k * sums_k) / n_k (fp32 mode's)
    double* x; double* g; double* xn; double* d;      // [P] (their spacing is the solver's)
    const double* w; const double* nrm;  // [K] term weights, n_norm
    const double* sums;                  // [K] raw sums of the evaluation, double
    double* loss_hist;                   // objective after iteration it0 + i of the running call
    double* th_eval64; float* th_eval32; // where the next evaluation reads theta (one of them is null)
};

QN_DEV bool is_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }      // (false for NaN)

// C, the execution context — first() / stride(): this thread's elements of a short array; each(n, f): f(i) for the elements of this thread;
// sum(n, f) / amax(n, f): workgroup-uniform reductions of f(i); lead(): the one thread that writes scalars; sync(): workgroup barrier
#ifdef PINN_EMU
// the xor butterfly 32, 16, ... 1 over one wave's 64 values, restated serially: the sum as every lane of the device holds it
inline double butterfly(double* v) {
    QN_NO_CONTRACT
    for (int msk = 32; msk >= 1; msk >>= 1) {
        double nx[WAVE];
        for (int l = 0; l < WAVE; ++l) nx[l] = v[l] + v[l ^ msk];
        for (int l = 0; l < WAVE; ++l) v[l] = nx[l];
    }
    return v[0];
}
struct EmuCtx {
    int first() const { return 0; }
    int stride() const { return 1; }
    bool lead() const { return true; }
    void sync() {}
    template <class F> void each(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
    template <class F> double sum(int n, F f) {          // the device's order: strided partials, per-wave butterfly, the waves in order
        QN_NO_CONTRACT
        double tot = 0.0;
        for (int w = 0; w < BLOCK / WAVE; ++w) {
            double v[WAVE];
            for (int l = 0; l < WAVE; ++l) {
                double s = 0.0;
                for (int i = w * WAVE + l; i < n; i += BLOCK) s += f(i);
                v[l] = s;
            }
            const double r = butterfly(v);
            tot = w == 0 ? r : tot + r;
        }
        return tot;
    }
    template <class F> double amax(int n, F f) {
        double mx = 0.0;
        for (int i = 0; i < n; ++i) mx = fmax(mx, fabs(f(i)));
        return mx;
    }
};
#else
struct DevCtx {
    double* sh;                          // LDS, one double per wave
    int t;
    __device__ __forceinline__ int first() const { return t; }
    __device__ __forceinline__ int stride() const { return BLOCK; }
    __device__ __forceinline__ bool lead() const { return t == 0; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    template <class F> __device__ __forceinline__ void each(int n, F f) { for (int i = t; i < n; i += BLOCK) f(i); }
    template <class F> __device__ __forceinline__ double sum(int n, F f) {
        QN_NO_CONTRACT
        double v = 0.0;
        for (int i = t; i < n; i += BLOCK) v += f(i);
        for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk, WAVE);
        if ((t & 63) == 0) sh[t >> 6] = v;
        __syncthreads();
        v = sh[0];
        for (int w = 1; w < BLOCK / WAVE; ++w) v += sh[w];
        __syncthreads();                                 // (sh is free for the next reduction)
        return v;
    }
    template <class F> __device__ __forceinline__ double amax(int n, F f) {
        double v = 0.0;
        for (int i = t; i < n; i += BLOCK) v = fmax(v, fabs(f(i)));
        for (int msk = 32; msk >= 1; msk >>= 1) v = fmax(v, __shfl_xor(v, msk, WAVE));
        if ((t & 63) == 0) sh[t >> 6] = v;
        __syncthreads();
        v = sh[0];
        for (int w = 1; w < BLOCK / WAVE; ++w) v = fmax(v, sh[w]);
        __syncthreads();
        return v;
    }
};
#endif

// ---- the shared steps of a control kernel's body.  c: the context; a: the common arguments; k: the thread's copy of the control block
QN_DEV void store_eval(const Args& a, int i, double v) {
    if (a.th_eval64) a.th_eval64[i] = v;
    if (a.th_eval32) a.th_eval32[i] = (float)v;
}
QN_DEV double objective(const Args& a) {
    QN_NO_CONTRACT
    double fn = 0.0;
    for (int q = 0; q < a.K; ++q) fn += a.f64form ? a.w[q] * (a.sums[q] / a.nrm[q]) : a.w[q] * a.sums[q] / a.nrm[q];
    return fn;
}
// LOAD: the evaluation's copy <- x
template <class C> QN_DEV void load(C& c, const Args& a) {
    c.each(a.P, [&](int i) { store_eval(a, i, a.x[i]); });
}
// ADOPT: (f, g) <- the evaluation at x; nothing pending (the solver clears its curvature and writes the block)
template <class T, class C> QN_DEV void adopt(C& c, const Args& a, Ctl& k, const T* ev) {
    c.each(a.P, [&](int i) { a.g[i] = (double)ev[i]; });
    k.f = objective(a);
    k.status = ST_RUN; k.ls = 0; k.pending = 0; k.t = 0.0; k.gd = 0.0;
}
QN_DEV bool armijo(const Ctl& k, double fn) {
    QN_NO_CONTRACT
    return is_finite(fn) && fn <= k.f + 1e-4 * k.t * k.gd;
}
QN_DEV void reject(Ctl& k) {
    k.t *= 0.5;
    ++k.ls;
    k.status = k.ls >= MAX_TRIALS ? ST_STALLED : ST_RETRY;
}
// the accepted point's bookkeeping (x and g are the solver's to move: it may still need the old ones)
template <class C> QN_DEV void accepted(C& c, const Args& a, Ctl& k, double fn, int it0) {
    k.f = fn;
    if (c.lead()) a.loss_hist[k.it - it0] = fn;
    ++k.it;
    k.status = ST_RUN;
}
// s.y, s.s and y.y of the accepted step, sv(i) and yv(i) its elements; true when the pair is fit for a curvature update
template <class C, class S, class Y> QN_DEV bool curvature(C& c, int P, S sv, Y yv, double& sy, double& yy) {
    QN_NO_CONTRACT
    sy = c.sum(P, [&](int i) { QN_NO_CONTRACT return sv(i) * yv(i); });
    const double ss = c.sum(P, [&](int i) { QN_NO_CONTRACT return sv(i) * sv(i); });
    yy = c.sum(P, [&](int i) { QN_NO_CONTRACT return yv(i) * yv(i); });
    return sy > 1e-10 * sqrt(ss * yy);
}
// the stop tests of a RUN state; true when there is an iteration to start
template <class C> QN_DEV bool go_on(C& c, const Args& a, Ctl& k, int it_end, double gtol) {
    const double gmax = c.amax(a.P, [&](int i) { return a.g[i]; });
    if (!(gmax > gtol)) k.status = ST_CONVERGED;
    else if (!(k.it < it_end)) k.status = ST_MAXITER;
    return k.status == ST_RUN;
}
// gd = g.d of the solver's direction; not a descent direction (stale curvature): d = -g, and true — the solver drops its curvature
template <class C> QN_DEV bool restart_if_uphill(C& c, const Args& a, Ctl& k) {
    k.gd = c.sum(a.P, [&](int i) { QN_NO_CONTRACT return a.g[i] * a.d[i]; });
    if (k.gd < 0.0) return false;
    c.each(a.P, [&](int i) { a.d[i] = -a.g[i]; });
    k.gd = c.sum(a.P, [&](int i) { QN_NO_CONTRACT return a.g[i] * a.d[i]; });
    return true;
}
// the first step of a line search: 1, or min(1, 1 / sqrt(g.g)) while H is the unscaled identity
template <class C> QN_DEV void first_step(C& c, const Args& a, Ctl& k, bool unscaled) {
    k.t = 1.0;
    if (unscaled) {
        const double gg = c.sum(a.P, [&](int i) { QN_NO_CONTRACT return a.g[i] * a.g[i]; });
        const double r = 1.0 / sqrt(gg);
        k.t = r < 1.0 ? r : 1.0;                         // std::min(1.0, r)
    }
    k.ls = 0;
}
// xn = x + t d into the evaluation's copy
template <class C> QN_DEV void propose(C& c, const Args& a, Ctl& k) {
    const double t = k.t;
    c.each(a.P, [&](int i) {
        QN_NO_CONTRACT
        const double v = a.x[i] + t * a.d[i];
        a.xn[i] = v;
        store_eval(a, i, v);
    });
    k.pending = 1;
    ++k.evals;
}

}  // namespace qn
