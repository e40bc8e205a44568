// cub_kernels.hpp — h-adaptive cubature of one term's squared residual, resident on the device (pinn_cubature_refine):
// everything of a refinement round that is not the evaluation of the residual.  The region list (centres, half-widths, volume shares, estimates),
// the rule's nodes, the split decisions and the emitted point set live in device memory; the host reads one Rec per round.
//   k_cub_nodes<T>    : one thread per (pending box, node): the Genz-Malik degree-7 node set of the box as points [n][d] in T
//   k_cub_estimate<T> : ONE WAVE PER BOX, lane = node (at most 57 of 64): I7, |I7 - I5| and the split axis (largest fourth difference)
//   k_cub_plan        : one workgroup: I = sum I7, E = sum err (thread t takes boxes t, t + 256, ...; per-wave butterfly; the waves in order), the
//                       tolerance, the exit decision, split flags and their exclusive scan (the children's slots)
//   k_cub_split       : one thread per box: child A in place, child B at its scanned slot, both pending
//   k_cub_emit<T>     : one thread per (leaf, tensor Gauss-Legendre node): the point in T (and its float copy), the factor float(sqrt(w n_norm))
// The rule on [-1, 1]^n, weights as fractions of the mean; node order = lane order:
//   0 the centre | +-l2 e_i (i = 0..n-1, + before -) | +-l3 e_i | (+-l4, +-l4) on axis pairs i < j, lexicographic, signs ++ +- -+ -- |
//   the 2^n corners l5 (+-1, ..), axis 0 the most significant bit, + before -
// Floating-point contraction is off: node coordinates, fourth differences and per-box estimates are the same numbers on every build; sums over
// lanes / boxes differ from a serial sum by their order only.  Every body exists once; the PINN_EMU build runs the same bodies serially, the
// sums in the device's order.
#pragma once
#include <cmath>
#include <cstdint>
#include "plat.hpp"

namespace cub {

#ifdef PINN_EMU
#define CUB_DEV inline
#else
#define CUB_DEV __device__ __forceinline__
#endif
#if defined(__clang__)
#define CUB_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CUB_NO_CONTRACT
#endif

constexpr int BLOCK = 256;
constexpr int MAX_FREE = 4;              // free axes of a box
constexpr int MAX_D = 4;                 // coordinates of a term's point: the engine plans no term with more (plan.cpp), so every free axis has a slot
static_assert(MAX_D <= MAX_FREE, "a free axis per coordinate");
constexpr int MAX_GAUSS = 8;             // Gauss-Legendre nodes per axis per leaf
enum { ST_CONVERGED = 0, ST_MAX_REGIONS = 1, ST_MAX_ROUNDS = 2, ST_NONFINITE = 3, ST_SPLIT = -1 };      // Rec::status; ST_SPLIT: the round goes on with k_cub_split

constexpr double L2 = 0.35856858280031809199;      // sqrt(9 / 70)
constexpr double L3 = 0.94868329805051379960;      // sqrt(9 / 10) (= l4)
constexpr double L5 = 0.68824720161168529772;      // sqrt(9 / 19)

// what the host reads once per round
struct Rec {
    int status, nboxes, npending, pad;   // nboxes / npending: AFTER the split when status == ST_SPLIT, the list as it stands otherwise
    double I, E, tau;
};

struct Args {
    int nf, d, M, nb, npend;             // free axes, coordinates per point, nodes of the rule, boxes in the list, pending boxes
    int free_ax[MAX_FREE];               // coordinate of free axis k
    double fixed[MAX_D];                 // value of a coordinate the term holds fixed (free coordinates: unused)
    double w7[5], w5[5];                 // weights per node class: centre, l2, l3, pairs, corners
    double* c; double* h;                // [cap][MAX_FREE] centres, half-widths
    double* share;                       // [cap] vol(box) / vol(domain)
    double* I7; double* err;             // [cap]
    int* axis; int* slot; int* pend;     // [cap] split axis; slot of child B (-1: not split); the pending boxes' indices
    Rec* rec;
};

constexpr int node_count(int nf) { return 1 + 4 * nf + 2 * nf * (nf - 1) + (1 << nf); }      // 7, 17, 33, 57 (constexpr: host and device)
CUB_DEV int node_class(int nf, int j) {
    if (j == 0) return 0;
    if (j < 1 + 2 * nf) return 1;
    if (j < 1 + 4 * nf) return 2;
    if (j < 1 + 4 * nf + 2 * nf * (nf - 1)) return 3;
    return 4;
}
// coordinate k of node j on [-1, 1]^nf
CUB_DEV double node_coord(int nf, int j, int k) {
    if (j == 0) return 0.0;
    j -= 1;
    if (j < 2 * nf) return (j >> 1) == k ? ((j & 1) ? -L2 : L2) : 0.0;
    j -= 2 * nf;
    if (j < 2 * nf) return (j >> 1) == k ? ((j & 1) ? -L3 : L3) : 0.0;
    j -= 2 * nf;
    const int npair = nf * (nf - 1) / 2;
    if (j < 4 * npair) {
        int q = j >> 2;
        const int s = j & 3;
        for (int a = 0; a < nf; ++a)
            for (int b = a + 1; b < nf; ++b, --q)
                if (q == 0) return k == a ? ((s & 2) ? -L3 : L3) : (k == b ? ((s & 1) ? -L3 : L3) : 0.0);
        return 0.0;
    }
    j -= 4 * npair;
    return ((j >> (nf - 1 - k)) & 1) ? -L5 : L5;
}

template <class T> CUB_DEV void nodes_body(int q, const Args& a, T* pts) {
    CUB_NO_CONTRACT
    const int p = q / a.M, j = q - p * a.M, box = a.pend[p];
    T* out = pts + (size_t)q * a.d;
    for (int i = 0; i < a.d; ++i) out[i] = (T)a.fixed[i];
    for (int k = 0; k < a.nf; ++k) {
        const double x = a.c[box * MAX_FREE + k] + a.h[box * MAX_FREE + k] * node_coord(a.nf, j, k);
        out[a.free_ax[k]] = (T)x;
    }
}

// lane j of the wave of pending box p: v_j = r_j^2 and the two weighted terms (lanes beyond the rule: zeros)
template <class T> CUB_DEV void estimate_lane(int p, int lane, const Args& a, const T* r, double& v, double& t7, double& t5) {
    CUB_NO_CONTRACT
    v = 0.0; t7 = 0.0; t5 = 0.0;
    if (lane >= a.M) return;
    const double x = (double)r[(size_t)p * a.M + lane];
    v = x * x;
    const int cls = node_class(a.nf, lane);
    t7 = a.w7[cls] * v;
    t5 = a.w5[cls] * v;
}
CUB_DEV double fourth_diff(double v0, double p2, double m2, double p3, double m3) {
    CUB_NO_CONTRACT
    return fabs((p2 + m2 - 2.0 * v0) - (p3 + m3 - 2.0 * v0) / 7.0);
}
// lane 0: the box's record from the wave's sums and the axis' fourth differences D[0..nf)
CUB_DEV void estimate_finish(int p, const Args& a, double s7, double s5, const double* D) {
    CUB_NO_CONTRACT
    const int box = a.pend[p];
    const double sh = a.share[box];
    const double i7 = sh * s7, i5 = sh * s5;
    int ax = 0;
    for (int k = 1; k < a.nf; ++k) if (D[k] > D[ax]) ax = k;      // (lowest index on ties)
    a.I7[box] = i7;
    a.err[box] = fabs(i7 - i5);
    a.axis[box] = ax;
}

// thread t of BLOCK: its part of sum I7 and sum err
CUB_DEV void plan_partial(int t, const Args& a, double& si, double& se) {
    CUB_NO_CONTRACT
    si = 0.0; se = 0.0;
    for (int i = t; i < a.nb; i += BLOCK) { si += a.I7[i]; se += a.err[i]; }
}
CUB_DEV double plan_tau(double I, double reltol, double abstol) {
    CUB_NO_CONTRACT
    const double rt = reltol * fabs(I);
    return abstol > rt ? abstol : rt;
}
CUB_DEV bool plan_flag(const Args& a, int i, double tau) {
    CUB_NO_CONTRACT
    return a.err[i] > tau * a.share[i];
}
// boxes [t per, (t + 1) per) are thread t's part of the scan
CUB_DEV int plan_per(const Args& a) { return (a.nb + BLOCK - 1) / BLOCK; }
CUB_DEV int plan_count(int t, const Args& a, double tau) {
    const int per = plan_per(a);
    int n = 0;
    for (int i = t * per; i < (t + 1) * per && i < a.nb; ++i) n += plan_flag(a, i, tau) ? 1 : 0;
    return n;
}
CUB_DEV void plan_slots(int t, const Args& a, double tau, int first) {
    const int per = plan_per(a);
    for (int i = t * per; i < (t + 1) * per && i < a.nb; ++i) a.slot[i] = plan_flag(a, i, tau) ? first++ : -1;
}
CUB_DEV void plan_finish(const Args& a, double I, double E, double tau, int nsplit, int max_regions, int may_split) {
    Rec r;
    r.pad = 0; r.I = I; r.E = E; r.tau = tau;
    r.nboxes = a.nb; r.npending = 0;
    const double big = 1.7976931348623157e308;
    if (!(fabs(I) <= big) || !(fabs(E) <= big)) r.status = ST_NONFINITE;      // a NaN / Inf residual somewhere: no comparison below means anything
    else if (E <= tau || nsplit == 0) r.status = ST_CONVERGED;      // (nsplit == 0 with E > tau: the shares' rounding; nothing is left to split)
    else if (a.nb + nsplit > max_regions) r.status = ST_MAX_REGIONS;
    else if (!may_split) r.status = ST_MAX_ROUNDS;
    else { r.status = ST_SPLIT; r.nboxes = a.nb + nsplit; r.npending = 2 * nsplit; }
    *a.rec = r;
}

CUB_DEV void split_body(int i, const Args& a) {
    CUB_NO_CONTRACT
    const int s = a.slot[i];
    if (s < 0) return;
    const int j = a.nb + s, ax = a.axis[i];
    const double hh = 0.5 * a.h[i * MAX_FREE + ax], cc = a.c[i * MAX_FREE + ax], sh = 0.5 * a.share[i];
    for (int k = 0; k < MAX_FREE; ++k) { a.c[j * MAX_FREE + k] = a.c[i * MAX_FREE + k]; a.h[j * MAX_FREE + k] = a.h[i * MAX_FREE + k]; }
    a.c[i * MAX_FREE + ax] = cc - hh; a.h[i * MAX_FREE + ax] = hh;
    a.c[j * MAX_FREE + ax] = cc + hh; a.h[j * MAX_FREE + ax] = hh;
    a.share[i] = sh; a.share[j] = sh;
    a.pend[2 * s] = i; a.pend[2 * s + 1] = j;
}

struct EmitArgs {
    int G, npl;                          // Gauss-Legendre nodes per axis, points per leaf = G^nf
    double gx[MAX_GAUSS], gw[MAX_GAUSS]; // nodes on [-1, 1]; weights as fractions of the mean (they sum to 1)
    double n_norm;                       // = the emitted point count
    float* pts32;                        // T = double: the fp32 kernels' copy of the points (nullptr: none)
    float* pw;                           // [n] float(sqrt(w n_norm)), w rounded to float first: what pinn_set_point_weights stores for float(w)
};
// point q = leaf * npl + (i_0 + G i_1 + ...), i_k the Gauss node on free axis k; w = share * gw[i_0] * gw[i_1] * ...
template <class T> CUB_DEV void emit_body(int q, const Args& a, const EmitArgs& e, T* pts) {
    CUB_NO_CONTRACT
    const int box = q / e.npl;
    int r = q - box * e.npl;
    T* out = pts + (size_t)q * a.d;
    float* out32 = e.pts32 ? e.pts32 + (size_t)q * a.d : nullptr;
    for (int i = 0; i < a.d; ++i) {
        out[i] = (T)a.fixed[i];
        if (out32) out32[i] = (float)a.fixed[i];
    }
    double w = a.share[box];
    for (int k = 0; k < a.nf; ++k) {
        const int ik = r % e.G;
        r /= e.G;
        const double x = a.c[box * MAX_FREE + k] + a.h[box * MAX_FREE + k] * e.gx[ik];
        out[a.free_ax[k]] = (T)x;
        if (out32) out32[a.free_ax[k]] = (float)x;
        w = w * e.gw[ik];
    }
    e.pw[q] = (float)sqrt((double)(float)w * e.n_norm);
}

#ifdef PINN_EMU
template <class T> inline void launch_nodes(const Args& a, T* pts, plat_stream) {
    for (int q = 0; q < a.npend * a.M; ++q) nodes_body<T>(q, a, pts);
}
inline void butterfly(double* v) {                       // the device's 64-lane xor butterfly: every lane adds its partner's value
    for (int m = 32; m >= 1; m >>= 1) {
        double n[64];
        for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ m];
        for (int l = 0; l < 64; ++l) v[l] = n[l];
    }
}
template <class T> inline void launch_estimate(const Args& a, const T* r, plat_stream) {
    for (int p = 0; p < a.npend; ++p) {
        double v[64], t7[64], t5[64], D[MAX_FREE];
        for (int l = 0; l < 64; ++l) estimate_lane<T>(p, l, a, r, v[l], t7[l], t5[l]);
        for (int k = 0; k < a.nf; ++k) D[k] = fourth_diff(v[0], v[1 + 2 * k], v[2 + 2 * k], v[1 + 2 * a.nf + 2 * k], v[2 + 2 * a.nf + 2 * k]);
        butterfly(t7);
        butterfly(t5);
        estimate_finish(p, a, t7[0], t5[0], D);
    }
}
inline void launch_plan(const Args& a, double reltol, double abstol, int max_regions, int may_split, plat_stream) {
    double tot[2] = {0.0, 0.0};
    for (int w = 0; w < BLOCK / 64; ++w) {
        double v[2][64];
        for (int l = 0; l < 64; ++l) plan_partial(w * 64 + l, a, v[0][l], v[1][l]);
        butterfly(v[0]);
        butterfly(v[1]);
        for (int q = 0; q < 2; ++q) tot[q] = w == 0 ? v[q][0] : tot[q] + v[q][0];
    }
    const double tau = plan_tau(tot[0], reltol, abstol);
    int first = 0;
    for (int t = 0; t < BLOCK; ++t) {
        const int n = plan_count(t, a, tau);
        plan_slots(t, a, tau, first);
        first += n;
    }
    plan_finish(a, tot[0], tot[1], tau, first, max_regions, may_split);
}
inline void launch_split(const Args& a, plat_stream) {
    for (int i = 0; i < a.nb; ++i) split_body(i, a);
}
template <class T> inline void launch_emit(const Args& a, const EmitArgs& e, T* pts, plat_stream) {
    for (int q = 0; q < a.nb * e.npl; ++q) emit_body<T>(q, a, e, pts);
}
#else
template <class T> __global__ void __launch_bounds__(BLOCK) k_cub_nodes(const Args a, T* pts) {
    const int q = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (q < a.npend * a.M) nodes_body<T>(q, a, pts);
}
template <class T> __global__ void __launch_bounds__(BLOCK) k_cub_estimate(const Args a, const T* r) {
    const int p = (int)(blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    if (p >= a.npend) return;                            // (the whole wave: p is uniform in it)
    double v, t7, t5;
    estimate_lane<T>(p, lane, a, r, v, t7, t5);
    double D[MAX_FREE];
    const double v0 = __shfl(v, 0, 64);
    for (int k = 0; k < MAX_FREE; ++k) {                 // (every lane takes part in every shuffle; the lanes read stay below 1 + 4 MAX_FREE)
        const int kk = k < a.nf ? k : 0;
        const double p2 = __shfl(v, 1 + 2 * kk, 64), m2 = __shfl(v, 2 + 2 * kk, 64);
        const double p3 = __shfl(v, 1 + 2 * a.nf + 2 * kk, 64), m3 = __shfl(v, 2 + 2 * a.nf + 2 * kk, 64);
        D[k] = fourth_diff(v0, p2, m2, p3, m3);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        t7 += __shfl_xor(t7, m, 64);
        t5 += __shfl_xor(t5, m, 64);
    }
    if (lane == 0) estimate_finish(p, a, t7, t5, D);
}
__global__ void __launch_bounds__(BLOCK) k_cub_plan(const Args a, double reltol, double abstol, int max_regions, int may_split) {
    __shared__ double sh[2][BLOCK / 64];
    __shared__ double sh_tau;
    __shared__ int cnt[BLOCK];
    const int t = (int)threadIdx.x;
    double si, se;
    plan_partial(t, a, si, se);
    for (int m = 32; m >= 1; m >>= 1) {
        si += __shfl_xor(si, m, 64);
        se += __shfl_xor(se, m, 64);
    }
    if ((t & 63) == 0) { sh[0][t >> 6] = si; sh[1][t >> 6] = se; }
    __syncthreads();
    if (t == 0) {
        si = sh[0][0]; se = sh[1][0];
        for (int w = 1; w < BLOCK / 64; ++w) { si += sh[0][w]; se += sh[1][w]; }
        sh[0][0] = si; sh[1][0] = se;
        sh_tau = plan_tau(si, reltol, abstol);
    }
    __syncthreads();
    const double tau = sh_tau;
    cnt[t] = plan_count(t, a, tau);
    __syncthreads();
    int first = 0;
    for (int u = 0; u < t; ++u) first += cnt[u];          // (256 counts in LDS: every thread sums its predecessors', an exclusive scan)
    plan_slots(t, a, tau, first);
    if (t == BLOCK - 1) plan_finish(a, sh[0][0], sh[1][0], tau, first + cnt[t], max_regions, may_split);
}
__global__ void __launch_bounds__(BLOCK) k_cub_split(const Args a) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < a.nb) split_body(i, a);
}
template <class T> __global__ void __launch_bounds__(BLOCK) k_cub_emit(const Args a, const EmitArgs e, T* pts) {
    const int q = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (q < a.nb * e.npl) emit_body<T>(q, a, e, pts);
}
template <class T> inline void launch_nodes(const Args& a, T* pts, plat_stream st) {
    hipLaunchKernelGGL(k_cub_nodes<T>, dim3((a.npend * a.M + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, pts);
}
template <class T> inline void launch_estimate(const Args& a, const T* r, plat_stream st) {
    hipLaunchKernelGGL(k_cub_estimate<T>, dim3((a.npend + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, st, a, r);
}
inline void launch_plan(const Args& a, double reltol, double abstol, int max_regions, int may_split, plat_stream st) {
    hipLaunchKernelGGL(k_cub_plan, dim3(1), dim3(BLOCK), 0, st, a, reltol, abstol, max_regions, may_split);
}
inline void launch_split(const Args& a, plat_stream st) {
    hipLaunchKernelGGL(k_cub_split, dim3((a.nb + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a);
}
template <class T> inline void launch_emit(const Args& a, const EmitArgs& e, T* pts, plat_stream st) {
    hipLaunchKernelGGL(k_cub_emit<T>, dim3((a.nb * e.npl + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, e, pts);
}
#endif

}  // namespace cub
