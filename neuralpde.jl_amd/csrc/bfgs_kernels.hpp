// bfgs_kernels.hpp — the device-resident dense BFGS finisher (pinn_bfgs_init / _steps / _get).  The state machine, the
// line search, the reductions and their fixed order are qn_kernels.hpp's; this header adds the dense curvature: the last step s = xn - x, the
// gradient difference y, u = H y, the inverse-Hessian approximation H[P][ld] (full symmetric storage, row-major) and the two matrix kernels.
// The pair (ident, gamma) of the control block stands for H = gamma I without touching the matrix: neither the start nor a restart costs a
// pass over it.
// LEADING DIMENSION.  ld = P rounded up to a multiple of 128 = 64 lanes x 2 doubles: every row starts on a 16-byte boundary for any P (odd P
// included), and every lane of a wave makes the same ld / 128 unconditional 16-byte loads per row.  The vectors are [ld] too.  The pad entries of
// the vectors are zero from pinn_bfgs_init on and never written; the pad columns of H are written by k_bfgs_update only, as products with those
// zeros: they add +0 to a row sum.  Rows >= P do not exist.
// The host queues SLOTS back to back and reads nothing inside a chunk of them:
//     one slot = k_bfgs_ctl<T>(JUDGE), k_bfgs_matvec, k_bfgs_ctl<T>(MID), k_bfgs_update, k_bfgs_ctl<T>(PROPOSE), ONE full evaluation
// (T = the evaluation's element type: double in float64 mode, float otherwise; the evaluation is the handle's resident path, untouched).
//   JUDGE, on acceptance: s and y are stored; when the pair passes qn::curvature the update is due: rho = 1 / s.y.  H a matrix: mv = MV_U,
//             upd = UPD_MATRIX.  H = gamma I: gamma = s.y / y.y (Nocedal-Wright 6.20), u = gamma y, c = rho (1 + rho y.u) at once,
//             upd = UPD_IDENT, ident = 0.  Update skipped and H a matrix: mv = MV_D (d = -H g).
//   MID       mv == MV_U: c = rho (1 + rho y.u) from the u the matrix-vector kernel has just written
//   PROPOSE   clears mv and upd.  RUN: d = -gamma g while ident (a matrix H: d is what the matrix kernels left); a restart sets ident = 1,
//             gamma = 1; the first step is scaled while H is the unscaled identity.
// THE MATRIX KERNELS are launched in every slot.  Each reads ONE word of the control block first (mv / upd) and returns at once when it is 0
// (a rejected trial, a terminal state, H = gamma I).  That word was written by a k_bfgs_ctl of an EARLIER launch: kernel boundaries on the one
// stream are the only ordering — no grid barrier, no spin-wait, no atomics, no cooperative launch.
//   k_bfgs_matvec   out = +-H v (u = H y, or d = -H g).  One WAVE owns a row (4 rows per workgroup of 256, ceil(P / 4) workgroups).  Lane l
//                   takes the column pairs (2 l + 128 k, 2 l + 1 + 128 k), k = 0, 1, ..., with one 16-byte load of H and one of v each; it keeps
//                   one partial for its even and one for its odd columns, adds the odd one to the even one, then the xor butterfly 32, 16, ... 1.
//                   A row's sum is one wave's in that order: it does not depend on the grid, the number of CUs or "lbfgs_chunk".
//   k_bfgs_update   H[i][j] <- (H[i][j] - rho (s_i u_j + u_i s_j)) + c (s_i s_j), every product rounded on its own (contraction off).  s_i u_j +
//                   u_i s_j and s_i s_j are the same doubles at [i][j] and [j][i] (products and the sum commute), so H stays BIT-SYMMETRIC.
//                   The wave that holds the new row multiplies it by the new g and reduces in the order above: d_i = -sum_j H[i][j] g_j in the
//                   same pass.  An accepted, updated iteration is one read pass (u = H y) and one read + write pass.  UPD_IDENT reads nothing
//                   of H: the old entry is gamma delta_ij.
// Indexing into H is size_t; addresses in the column loops are affine and the loads unconditional.
#pragma once
#include "qn_kernels.hpp"

namespace bfgs {

using namespace qn;

enum { PH_JUDGE = 0, PH_MID = 1, PH_PROPOSE = 2, PH_LOAD = 3, PH_ADOPT = 4 };
enum { MV_NONE = 0, MV_U = 1, MV_D = 2 };                // k_bfgs_matvec: nothing | u = H y | d = -H g
enum { UPD_NONE = 0, UPD_MATRIX = 1, UPD_IDENT = 2 };    // k_bfgs_update: nothing | H a matrix | H = gamma I (write only)
constexpr int ROWS_PER_BLOCK = BLOCK / WAVE;
constexpr int LD_ALIGN = 2 * WAVE;                       // doubles one wave takes per step of the column loop
constexpr int MAX_P = 32768;                             // H = 8 GiB there

struct Ctl : qn::Ctl {
    int ident, mv, upd;                  // H = gamma I; what the matrix kernels of this slot do
    double gamma, rho, c;                // H = gamma I while ident; the scalars of the pending rank-two update
};

struct Args : qn::Args {
    int ld;
    double* s; double* y; double* u;     // [ld] like x, g, xn, d; pads zero
    double* H;                           // [P][ld]
    Ctl* ctl;
};

inline int padded_ld(int P) { return (P + LD_ALIGN - 1) / LD_ALIGN * LD_ALIGN; }

struct dbl2 { double x, y; };
QN_DEV dbl2 load2(const double* p) {
#ifdef PINN_EMU
    return dbl2{p[0], p[1]};
#else
    const double2 v = *reinterpret_cast<const double2*>(p);
    return dbl2{v.x, v.y};
#endif
}
QN_DEV void store2(double* p, dbl2 v) {
#ifdef PINN_EMU
    p[0] = v.x; p[1] = v.y;
#else
    *reinterpret_cast<double2*>(p) = make_double2(v.x, v.y);
#endif
}

// ---- the control kernel's body
template <class T, class C> QN_DEV void ctl_body(C& c, const Args& a, const T* ev, int phase, int it0, int it_end, double gtol) {
    QN_NO_CONTRACT
    const int P = a.P;
    Ctl k = *a.ctl;
    c.sync();                                            // every thread has read the block before anyone writes it
    if (phase == PH_LOAD) {
        load(c, a);
        return;
    }
    if (phase == PH_ADOPT) {                             // H = I
        adopt(c, a, k, ev);
        k.ident = 1; k.gamma = 1.0; k.rho = 0.0; k.c = 0.0; k.mv = MV_NONE; k.upd = UPD_NONE;
        if (c.lead()) *a.ctl = k;
        return;
    }
    if (k.status >= ST_CONVERGED) return;
    if (phase == PH_JUDGE) {
        if (!k.pending) return;
        k.pending = 0;
        const double fn = objective(a);
        if (armijo(k, fn)) {
            c.each(P, [&](int i) {
                const double xi = a.xn[i], gi = (double)ev[i];
                a.s[i] = xi - a.x[i]; a.y[i] = gi - a.g[i];
                a.x[i] = xi; a.g[i] = gi;
            });
            double sy, yy;
            if (curvature(c, P, [&](int i) { return a.s[i]; }, [&](int i) { return a.y[i]; }, sy, yy)) {
                k.rho = 1.0 / sy;
                if (k.ident) {                           // leaving H = gamma I: u and c need no matrix pass
                    const double gamma = sy / yy;
                    k.gamma = gamma;
                    c.each(P, [&](int i) { QN_NO_CONTRACT a.u[i] = gamma * a.y[i]; });
                    const double yu = c.sum(P, [&](int i) { QN_NO_CONTRACT return a.y[i] * a.u[i]; });
                    k.c = k.rho * (1.0 + k.rho * yu);
                    k.ident = 0;
                    k.upd = UPD_IDENT;
                } else {
                    k.mv = MV_U;
                    k.upd = UPD_MATRIX;
                }
            } else if (!k.ident) k.mv = MV_D;            // update skipped: the next direction from the matrix as it is
            accepted(c, a, k, fn, it0);
        } else reject(k);
        if (c.lead()) *a.ctl = k;
        return;
    }
    if (phase == PH_MID) {
        if (k.mv != MV_U) return;
        const double yu = c.sum(P, [&](int i) { QN_NO_CONTRACT return a.y[i] * a.u[i]; });
        k.c = k.rho * (1.0 + k.rho * yu);
        if (c.lead()) *a.ctl = k;
        return;
    }
    // PH_PROPOSE
    k.mv = MV_NONE; k.upd = UPD_NONE;
    if (k.status == ST_RUN && go_on(c, a, k, it_end, gtol)) {
        if (k.ident) {
            const double gamma = k.gamma;
            c.each(P, [&](int i) { QN_NO_CONTRACT a.d[i] = -(gamma * a.g[i]); });
        }
        if (restart_if_uphill(c, a, k)) { k.ident = 1; k.gamma = 1.0; }
        first_step(c, a, k, k.ident && k.gamma == 1.0);
    }
    if (k.status == ST_RUN || k.status == ST_RETRY) propose(c, a, k);
    if (c.lead()) *a.ctl = k;
}

// ---- the matrix kernels' bodies, one row each.  W: wave_sum(f): the sum of f(lane) over the 64 lanes by the xor butterfly, in every lane;
// lane0(): the lane that writes the row's scalar
template <class W> QN_DEV void matvec_row(W& w, const Args& a, int row, int mode) {
    const double* Hr = a.H + (size_t)row * (size_t)a.ld;
    const double* v = mode == MV_U ? a.y : a.g;
    const int nstep = a.ld / LD_ALIGN;
    const double r = w.wave_sum([&](int lane) {
        QN_NO_CONTRACT
        const double* hp = Hr + 2 * lane;
        const double* vp = v + 2 * lane;
        double a0 = 0.0, a1 = 0.0;
        for (int q = 0; q < nstep; ++q, hp += LD_ALIGN, vp += LD_ALIGN) {
            const dbl2 h = load2(hp), z = load2(vp);
            a0 += h.x * z.x;
            a1 += h.y * z.y;
        }
        return a0 + a1;
    });
    if (w.lane0()) {
        if (mode == MV_U) a.u[row] = r;
        else a.d[row] = -r;
    }
}

template <bool FROM_IDENT, class W> QN_DEV void update_row(W& w, const Args& a, int row, double gamma, double rho, double cc) {
    double* Hr = a.H + (size_t)row * (size_t)a.ld;
    const double si = a.s[row], ui = a.u[row];
    const int nstep = a.ld / LD_ALIGN;
    const double r = w.wave_sum([&](int lane) {
        QN_NO_CONTRACT
        double* hp = Hr + 2 * lane;
        const double* sp = a.s + 2 * lane;
        const double* up = a.u + 2 * lane;
        const double* gp = a.g + 2 * lane;
        int j = 2 * lane;
        double a0 = 0.0, a1 = 0.0;
        for (int q = 0; q < nstep; ++q, hp += LD_ALIGN, sp += LD_ALIGN, up += LD_ALIGN, gp += LD_ALIGN, j += LD_ALIGN) {
            const dbl2 sj = load2(sp), uj = load2(up), gj = load2(gp);
            dbl2 h;
            if (FROM_IDENT) { h.x = j == row ? gamma : 0.0; h.y = j + 1 == row ? gamma : 0.0; }
            else h = load2(hp);
            const double px = si * uj.x, qx = ui * sj.x, rx = si * sj.x;
            const double py = si * uj.y, qy = ui * sj.y, ry = si * sj.y;
            h.x = (h.x - rho * (px + qx)) + cc * rx;
            h.y = (h.y - rho * (py + qy)) + cc * ry;
            store2(hp, h);
            a0 += h.x * gj.x;
            a1 += h.y * gj.y;
        }
        return a0 + a1;
    });
    if (w.lane0()) a.d[row] = -r;
}

#ifdef PINN_EMU
struct EmuWave {
    bool lane0() const { return true; }
    template <class F> double wave_sum(F f) {
        QN_NO_CONTRACT
        double v[WAVE];
        for (int l = 0; l < WAVE; ++l) v[l] = f(l);
        return butterfly(v);
    }
};
template <class T> inline void launch_ctl(const Args& a, const T* ev, int phase, int it0, int it_end, double gtol, plat_stream) {
    EmuCtx c;
    ctl_body<T>(c, a, ev, phase, it0, it_end, gtol);
}
inline void launch_matvec(const Args& a, plat_stream) {
    const int mode = a.ctl->mv;
    if (mode == MV_NONE) return;
    EmuWave w;
    for (int row = 0; row < a.P; ++row) matvec_row(w, a, row, mode);
}
inline void launch_update(const Args& a, plat_stream) {
    const int mode = a.ctl->upd;
    if (mode == UPD_NONE) return;
    const double gamma = a.ctl->gamma, rho = a.ctl->rho, cc = a.ctl->c;
    EmuWave w;
    for (int row = 0; row < a.P; ++row) {
        if (mode == UPD_IDENT) update_row<true>(w, a, row, gamma, rho, cc);
        else update_row<false>(w, a, row, gamma, rho, cc);
    }
}
#else
struct DevWave {
    int lane;
    __device__ __forceinline__ bool lane0() const { return lane == 0; }
    template <class F> __device__ __forceinline__ double wave_sum(F f) {
        QN_NO_CONTRACT
        double v = f(lane);
        for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk, WAVE);
        return v;
    }
};
template <class T> __global__ void __launch_bounds__(BLOCK) k_bfgs_ctl(const Args a, const T* ev, int phase, int it0, int it_end, double gtol) {
    __shared__ double sh[BLOCK / WAVE];
    DevCtx c{sh, (int)threadIdx.x};
    ctl_body<T>(c, a, ev, phase, it0, it_end, gtol);
}
__global__ void __launch_bounds__(BLOCK) k_bfgs_matvec(const Args a) {
    const int mode = a.ctl->mv;                          // written by a k_bfgs_ctl of an earlier launch
    if (mode == MV_NONE) return;
    const int row = (int)blockIdx.x * ROWS_PER_BLOCK + ((int)threadIdx.x >> 6);
    if (row >= a.P) return;
    DevWave w{(int)threadIdx.x & 63};
    matvec_row(w, a, row, mode);
}
__global__ void __launch_bounds__(BLOCK) k_bfgs_update(const Args a) {
    const int mode = a.ctl->upd;                         // written by a k_bfgs_ctl of an earlier launch
    if (mode == UPD_NONE) return;
    const int row = (int)blockIdx.x * ROWS_PER_BLOCK + ((int)threadIdx.x >> 6);
    if (row >= a.P) return;
    const double gamma = a.ctl->gamma, rho = a.ctl->rho, cc = a.ctl->c;
    DevWave w{(int)threadIdx.x & 63};
    if (mode == UPD_IDENT) update_row<true>(w, a, row, gamma, rho, cc);
    else update_row<false>(w, a, row, gamma, rho, cc);
}
inline int row_blocks(int P) { return (P + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK; }
template <class T> inline void launch_ctl(const Args& a, const T* ev, int phase, int it0, int it_end, double gtol, plat_stream st) {
    hipLaunchKernelGGL(k_bfgs_ctl<T>, dim3(1), dim3(BLOCK), 0, st, a, ev, phase, it0, it_end, gtol);
}
inline void launch_matvec(const Args& a, plat_stream st) { hipLaunchKernelGGL(k_bfgs_matvec, dim3(row_blocks(a.P)), dim3(BLOCK), 0, st, a); }
inline void launch_update(const Args& a, plat_stream st) { hipLaunchKernelGGL(k_bfgs_update, dim3(row_blocks(a.P)), dim3(BLOCK), 0, st, a); }
#endif

}  // namespace bfgs
