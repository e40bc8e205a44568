// lbfgs_kernels.hpp — the device-resident L-BFGS finisher (pinn_lbfgs_init / _steps / _get).  The state machine, the line
// search, the reductions and their fixed order are qn_kernels.hpp's; this header adds the limited-memory curvature: the rings S[m][P], Y[m][P],
// rho[m] (a RING with a head index and a count: pairs are never shifted) and the two-loop recursion.  The host queues SLOTS back to back and
// reads nothing inside a chunk of them:
//     one slot = ONE k_lbfgs_step<T> launch + ONE full evaluation (objective and gradient) at the evaluation's copy of theta
// (T = the evaluation's element type: double in float64 mode, float otherwise; the evaluation is the handle's resident path, untouched).
//   JUDGE, on acceptance: the pair (s, y) is pushed iff it passes qn::curvature (the oldest pair beyond `history` is evicted)
//   PROPOSE, RUN: the two-loop recursion newest pair first, gamma = sy / yy of the newest pair; a restart clears the rings; the first step is
//             scaled while the rings are empty.
// alpha and rho are held in LDS (<= 64 doubles each).  A ring pair's address is base + slot * P + i with a workgroup-uniform slot, and every
// load in the ring loops is unconditional.
// THE ONE DIFFERENCE from pinn_lbfgs: a rejected trial costs a FULL evaluation here (the host routine runs rejected trials loss-only and
// re-evaluates the accepted point with a gradient); an accepted trial never needs re-evaluation.  The iterates are the same algorithm.
#pragma once
#include "qn_kernels.hpp"

namespace lbfgs {

using namespace qn;

enum { MODE_SLOT = 0, MODE_LOAD = 1, MODE_ADOPT = 2 };
constexpr int MAX_HISTORY = 64;

struct Ctl : qn::Ctl {
    int head, count;                     // ring: oldest pair's slot, pairs held
};

struct Args : qn::Args {
    int m;                               // history
    double* S; double* Y; double* rho;   // [m][P], [m][P], [m]
    Ctl* ctl;
};

// al / rh: alpha of the running recursion and rho of the ring, [MAX_HISTORY] each, shared by the workgroup (LDS)
template <class T, class C> QN_DEV void step_body(C& c, double* al, double* rh, const Args& a, const T* ev, int mode, int it0, int it_end, double gtol) {
    QN_NO_CONTRACT
    const int P = a.P, m = a.m;
    Ctl k = *a.ctl;                                      // every thread reads the block before anyone writes it (the barrier below)
    for (int j = c.first(); j < m; j += c.stride()) rh[j] = a.rho[j];
    c.sync();
    if (mode == MODE_LOAD) {
        load(c, a);
        return;
    }
    if (mode == MODE_ADOPT) {                            // rings cleared
        adopt(c, a, k, ev);
        k.head = 0; k.count = 0;
        if (c.lead()) *a.ctl = k;
        return;
    }
    if (k.status >= ST_CONVERGED) return;
    if (k.pending) {
        k.pending = 0;
        const double fn = objective(a);
        if (armijo(k, fn)) {
            double sy, yy;
            const bool push = curvature(c, P, [&](int i) { return a.xn[i] - a.x[i]; }, [&](int i) { return (double)ev[i] - a.g[i]; }, sy, yy);
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
                if (c.lead()) { rh[slot] = 1.0 / sy; a.rho[slot] = 1.0 / sy; }
                if (k.count == m) { k.head = k.head + 1 == m ? 0 : k.head + 1; } else ++k.count;
                c.sync();
            }
            accepted(c, a, k, fn, it0);
        } else reject(k);
    }
    if (k.status == ST_RUN && go_on(c, a, k, it_end, gtol)) {
        // two-loop recursion: d = -H g, q held in d
        c.each(P, [&](int i) { a.d[i] = a.g[i]; });
        for (int j = k.count - 1; j >= 0; --j) {
            int slot = k.head + j;
            if (slot >= m) slot -= m;
            const double* Sj = a.S + (size_t)slot * P;
            const double* Yj = a.Y + (size_t)slot * P;
            const double alpha = rh[slot] * c.sum(P, [&](int i) { QN_NO_CONTRACT return Sj[i] * a.d[i]; });
            if (c.lead()) al[j] = alpha;
            c.each(P, [&](int i) { QN_NO_CONTRACT a.d[i] -= alpha * Yj[i]; });
        }
        double gamma = 1.0;
        if (k.count > 0) {
            int slot = k.head + k.count - 1;
            if (slot >= m) slot -= m;
            const double* Sj = a.S + (size_t)slot * P;
            const double* Yj = a.Y + (size_t)slot * P;
            const double sy = c.sum(P, [&](int i) { QN_NO_CONTRACT return Sj[i] * Yj[i]; });
            const double yy = c.sum(P, [&](int i) { QN_NO_CONTRACT return Yj[i] * Yj[i]; });
            gamma = sy / yy;
        }
        c.each(P, [&](int i) { QN_NO_CONTRACT a.d[i] *= gamma; });
        c.sync();                                        // (alpha of every pair is in LDS)
        for (int j = 0; j < k.count; ++j) {
            int slot = k.head + j;
            if (slot >= m) slot -= m;
            const double* Sj = a.S + (size_t)slot * P;
            const double* Yj = a.Y + (size_t)slot * P;
            const double beta = rh[slot] * c.sum(P, [&](int i) { QN_NO_CONTRACT return Yj[i] * a.d[i]; });
            const double ab = al[j] - beta;
            c.each(P, [&](int i) { QN_NO_CONTRACT a.d[i] += ab * Sj[i]; });
        }
        c.each(P, [&](int i) { a.d[i] = -a.d[i]; });
        if (restart_if_uphill(c, a, k)) { k.head = 0; k.count = 0; }
        first_step(c, a, k, k.count == 0);
    }
    if (k.status == ST_RUN || k.status == ST_RETRY) propose(c, a, k);
    if (c.lead()) *a.ctl = k;
}

#ifdef PINN_EMU
template <class T> inline void launch_step(const Args& a, const T* ev, int mode, int it0, int it_end, double gtol, plat_stream) {
    EmuCtx c;
    double al[MAX_HISTORY], rh[MAX_HISTORY];
    step_body<T>(c, al, rh, a, ev, mode, it0, it_end, gtol);
}
#else
template <class T> __global__ void __launch_bounds__(BLOCK) k_lbfgs_step(const Args a, const T* ev, int mode, int it0, int it_end, double gtol) {
    __shared__ double al[MAX_HISTORY], rh[MAX_HISTORY], sh[BLOCK / WAVE];
    DevCtx c{sh, (int)threadIdx.x};
    step_body<T>(c, al, rh, a, ev, mode, it0, it_end, gtol);
}
template <class T> inline void launch_step(const Args& a, const T* ev, int mode, int it0, int it_end, double gtol, plat_stream st) {
    hipLaunchKernelGGL(k_lbfgs_step<T>, dim3(1), dim3(BLOCK), 0, st, a, ev, mode, it0, it_end, gtol);
}
#endif

}  // namespace lbfgs
