// ens_kernels.hpp — ensemble prediction (pinn_phi_ensemble): the trial function of ONE network at S parameter vectors
// and n points, and the posterior mean / standard deviation over the S predictions, without a host round trip per sample.
//   k_ens_forward<T> : preds[s][i] = phi_net(x_i; theta_s), T = double (float64 mode) or float.  One workgroup = one (sample s, block of
//                      `ppb` points) pair, one LANE per point.  The sample is uniform across the workgroup, so every weight is read at a
//                      wave-uniform address straight from theta_s (ComponentArrays order, W_l column-major then b_l, as family 4) — no packed
//                      image, no size limit on the parameters.  A layer's activations live in LDS in two ping-pong images [neuron][point],
//                      the point index fastest: the 64 lanes of a wave touch consecutive words (conflict-free) and a lane only ever touches
//                      its own column, so there is no barrier.  Layer widths, depth and activation are RUN-TIME values (one kernel per T).
//                      Per output neuron the dot product is the k-ascending vfma chain of f64_point's channel 0 (pinn_kernels4.hpp), MB
//                      neurons share every activation read; blocking changes no bit.  The ragged last block repeats the last point
//                      (unconditional loads, affine addresses) and drops the store with a per-lane select; nothing exits early.
//   k_ens_stats      : one thread per point: mean_i = (sum_s preds[s][i]) / S, std_i = sqrt(sum_s (preds[s][i] - mean_i)^2 / (S - ddof)), both
//                      sums in double in the fixed order s = 0 .. S-1 (two passes: what numpy.mean / numpy.std restate).  No atomics: the
//                      result is bit-reproducible and does not depend on how the host chunks the points.
//   k_ens_jet<T, J>  : (pinn_derivative_ensemble) the same geometry carrying a Taylor jet: an image row is (neuron, channel),
//                      an image [wmax * C][ppb].  J is one of five channel STRUCTURES (JetSet of pinn_kernels.hpp): the line jets u, d_a u, ..,
//                      d_a^K u for K = 1 .. 4 (C = 2 .. 5) and the two-axis jet u, d_a u, d_b u, d_a d_b u (C = 4); the axes a, b are RUN-TIME
//                      values (J's own axes 0 / 1 stand for them: they only pick the columns of W_0 that seed the first layer).  The rules are
//                      act_value / act_record / act_derivs_n / jet_forward of pinn_kernels.hpp under a workgroup-uniform branch on the activation
//                      class.  Channel 0 is forward_point's chain (bias first, vfma over k ascending), the other channels start from zero in the
//                      same order: channel 0 of every pass is bit-equal to k_ens_forward's prediction.  The two images live in LDS, or — when they
//                      would leave a CU fewer than four workgroups, or exceed its LDS (ensemble.cpp decides) — in a per-workgroup region of a device scratch buffer in the same [row][point]
//                      layout (coalesced; a lane only touches its own column): the body takes the image pointer and is the same either way.  The
//                      grid walks the (sample, block) pairs in a grid-stride loop, so the scratch is bounded by the grid, not by S x blocks.
// Every body exists once; the PINN_EMU build runs the same bodies serially, in the same summation order.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>
#include <vector>
#include "pinn_kernels.hpp"
#include "plat.hpp"

namespace ens {

#ifdef PINN_EMU
#define ENS_DEV inline
#else
#define ENS_DEV __device__ __forceinline__
#endif
#if defined(__clang__)
#define ENS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ENS_NO_CONTRACT
#endif

constexpr int MAX_LAYERS = 16;             // Dense layers including the output layer (family 4's limit)
constexpr int MB = 8;                      // output neurons per register block
constexpr int STATS_BLOCK = 256;
constexpr int MIN_PPB = 64, MAX_PPB = 256; // points per block: a multiple of the wave size
constexpr size_t LDS_MAX = 160 * 1024;     // LDS of a gfx950 CU: what one workgroup may take at most
constexpr size_t LDS_TARGET = 32 * 1024;   // ... and what it takes when the network allows it (several workgroups per CU)

struct Net {
    int nl;                                // Dense layers
    int sizes[MAX_LAYERS + 1];             // n_0 .. n_nl, n_nl == 1
    int act, act_layers;                   // as pe::Net: one kind for all hidden layers, or ACT_MIXED with the kind of hidden layer l in bits 4l .. 4l+3
    int theta0;                            // the network's slice of a parameter vector
    int wmax;                              // widest layer, inputs and output included: rows of one LDS image
};

// bytes of LDS one workgroup of `ppb` points takes: two images [wmax * C][ppb] (C jet channels per neuron; the value kernel: 1)
inline size_t lds_bytes(const Net& n, int ppb, size_t elem, int C = 1) { return 2 * (size_t)n.wmax * (size_t)C * (size_t)ppb * elem; }
// points per block for this network: the largest of 256 / 128 / 64 within LDS_TARGET, else 64 within LDS_MAX, else 0 (the value kernel's
// caller refuses; the jet kernel's takes the scratch storage)
inline int pick_ppb(const Net& n, size_t elem, int C = 1) {
    for (int ppb = MAX_PPB; ppb >= MIN_PPB; ppb >>= 1)
        if (lds_bytes(n, ppb, elem, C) <= LDS_TARGET) return ppb;
    return lds_bytes(n, MIN_PPB, elem, C) <= LDS_MAX ? MIN_PPB : 0;
}

// activation of hidden layer l at z: the rules of pinn_kernels.hpp (the emulation's float rules are 64 lanes wide: lane 0 of a broadcast)
template <class T> ENS_DEV T act_apply(const Net& n, int l, T z);
template <> ENS_DEV double act_apply<double>(const Net& n, int l, double z) {
    if (n.act == pk::ACT_SIN) return pk::act_value<pk::ACLS_Z_SIN, false, double>(n.act, z);
    if (n.act == pk::ACT_SWISH) return pk::act_value<pk::ACLS_Z_SWISH, false, double>(n.act, z);
    return pk::act_value<pk::ACLS_A, false, double>(n.act == pk::ACT_MIXED ? ((n.act_layers >> (4 * l)) & 15) : n.act, z);
}
template <> ENS_DEV float act_apply<float>(const Net& n, int l, float z) {
#ifdef PINN_EMU
    const wv::vfloat v(z);
    auto one = [](const wv::vfloat& a) { return a.v[0]; };
#else
    const float v = z;
    auto one = [](float a) { return a; };
#endif
    if (n.act == pk::ACT_SIN) return one(pk::act_value<pk::ACLS_Z_SIN>(n.act, v));
    if (n.act == pk::ACT_SWISH) return one(pk::act_value<pk::ACLS_Z_SWISH>(n.act, v));
    return one(pk::act_value<pk::ACLS_A>(n.act == pk::ACT_MIXED ? ((n.act_layers >> (4 * l)) & 15) : n.act, v));
}

// the point of lane `t` of a block of `ppb` points: th = the network's parameters of the block's sample, x = the point's n_0 coordinates,
// img = the block's two LDS images (element (row, t) at img[row * ppb + t]).  Returns phi.
template <class T> ENS_DEV T forward_point(const Net& n, const T* __restrict__ th, const T* __restrict__ x, T* img, int ppb, int t) {
    const int half = n.wmax * ppb;
    for (int i = 0; i < n.sizes[0]; ++i) img[i * ppb + t] = x[i];
    int o = 0;
    for (int l = 0; l < n.nl; ++l) {
        const int n_in = n.sizes[l], n_out = n.sizes[l + 1];
        const T* W = th + o;                             // (n_out x n_in, column-major)
        const T* B = W + n_out * n_in;
        o += n_out * n_in + n_out;
        const T* in = img + (l & 1) * half + t;
        T* out = img + ((l + 1) & 1) * half + t;
        const bool hidden = l + 1 < n.nl;
        for (int m0 = 0; m0 < n_out; m0 += MB) {
            T z[MB];
            int mj[MB];
            PINN_UNROLL for (int j = 0; j < MB; ++j) {
                mj[j] = (m0 + j < n_out) ? m0 + j : n_out - 1;       // (the tail of the last block repeats the last neuron; never stored)
                z[j] = B[mj[j]];
            }
            for (int k = 0; k < n_in; ++k) {
                const T a = in[k * ppb];
                PINN_UNROLL for (int j = 0; j < MB; ++j) z[j] = wv::vfma(W[mj[j] + k * n_out], a, z[j]);
            }
            PINN_UNROLL for (int j = 0; j < MB; ++j)
                if (m0 + j < n_out) out[(m0 + j) * ppb] = hidden ? act_apply<T>(n, l, z[j]) : z[j];
        }
    }
    return img[(n.nl & 1) * half + t];
}

// ---- jets (pinn_derivative_ensemble) ----
// the five channel structures: JetSet instances for axis 0 or axes (0, 1); the run-time axes of a pass stand in for them
using JetLine1 = pk::JetSet<1u, 0ull, 0, 0u>;            // u, d_a u
using JetLine2 = pk::JetSet<1u, 0ull, 1, 0u>;            // .., d_a^2 u
using JetLine3 = pk::JetSet<1u, 0ull, 1, 3u>;            // .., d_a^3 u
using JetLine4 = pk::JetSet<1u, 0ull, 1, 4u>;            // .., d_a^4 u
using JetPair = pk::JetSet<3u, 0x10ull, 1, 0u>;          // u, d_a u, d_b u, d_a d_b u
static_assert(JetLine1::C == 2 && JetLine2::C == 3 && JetLine3::C == 4 && JetLine4::C == 5 && JetPair::C == 4, "channel counts of the five structures");
constexpr int JET_PAIR = 5;                              // JetPass::kind: 1 .. 4 = the line jet of that order, 5 = the two-axis jet
constexpr int JET_MAX_C = 5;
constexpr int jet_mb(int C) { return C <= 3 ? 8 : 4; }   // neurons per register block (MB * C accumulators), as f64_point
inline int jet_channels(int kind) { return kind == JET_PAIR ? 4 : kind + 1; }

// one jet pass: the structure, its run-time axes and, per channel, the request whose slab [S][ld] takes that channel (-1: none)
struct JetPass {
    int kind;
    int axis[2];                                         // a (line jets), a and b (two-axis jet)
    int dst[JET_MAX_C];
};

// the activation and its jet rule on one neuron's channels, in place: z[0] = the pre-activation value, z[k > 0] = the pre-activation channels
template <class J, int ACLS, class V> ENS_DEV void jet_act_v(int kind, V (&z)[J::C]) {
    const V a0 = pk::act_value<ACLS, false, V>(kind, z[0]);
    z[0] = pk::act_record<ACLS>(z[0], a0);
    V dd[pk::ND];
    pk::act_derivs_n<J::NORD - 1, ACLS, false, V>(kind, z[0], dd);
    pk::jet_forward<J>(z, dd);
    z[0] = a0;
}
// ... on the MB neurons of a register block
template <class J, int ACLS, class T, int MB_> ENS_DEV void jet_act(int kind, T (&z)[MB_][J::C]) {
#ifdef PINN_EMU
    if constexpr (std::is_same_v<T, float>) {            // (the emulation's float rules are 64 lanes wide: neuron j of the block rides in lane j)
        wv::vfloat v[J::C];
        for (int c = 0; c < J::C; ++c) { v[c] = wv::vfloat(0.f); for (int j = 0; j < MB_; ++j) v[c].v[j] = z[j][c]; }
        jet_act_v<J, ACLS>(kind, v);
        for (int c = 0; c < J::C; ++c) for (int j = 0; j < MB_; ++j) z[j][c] = v[c].v[j];
        return;
    } else
#endif
    { PINN_UNROLL for (int j = 0; j < MB_; ++j) jet_act_v<J, ACLS>(kind, z[j]); }
}

// forward_point with jets: u[c] = channel c of the trial function at the point of lane t.  img = the block's two images, element (neuron m,
// channel c, t) at img[(m * C + c) * ppb + t]; the coordinates take rows 0 .. n_0 - 1 of image 0.  The first layer seeds the derivative channels
// from columns axis[..] of W_0 (f64_point); the output layer is linear in every channel.
template <class T, class J> ENS_DEV void jet_point(const Net& n, const int* axis, const T* __restrict__ th, const T* __restrict__ x, T* img, int ppb, int t, T (&u)[J::C]) {
    constexpr int C = J::C, MBJ = jet_mb(C);
    const int half = n.wmax * C * ppb;
    for (int i = 0; i < n.sizes[0]; ++i) img[i * ppb + t] = x[i];
    int o = 0;
    for (int l = 0; l < n.nl; ++l) {
        const int n_in = n.sizes[l], n_out = n.sizes[l + 1];
        const T* W = th + o;                             // (n_out x n_in, column-major)
        const T* B = W + n_out * n_in;
        o += n_out * n_in + n_out;
        const T* in = img + (l & 1) * half + t;
        T* out = img + ((l + 1) & 1) * half + t;
        const bool hidden = l + 1 < n.nl;
        const int kind = n.act == pk::ACT_MIXED ? ((n.act_layers >> (4 * l)) & 15) : n.act;
        for (int m0 = 0; m0 < n_out; m0 += MBJ) {
            T z[MBJ][C];
            int mj[MBJ];
            PINN_UNROLL for (int j = 0; j < MBJ; ++j) {
                mj[j] = (m0 + j < n_out) ? m0 + j : n_out - 1;       // (the tail of the last block repeats the last neuron; never stored)
                z[j][0] = B[mj[j]];
                PINN_UNROLL for (int c = 1; c < C; ++c) z[j][c] = T(0);
            }
            if (l == 0) {
                for (int k = 0; k < n_in; ++k) {
                    const T a = in[k * ppb];
                    PINN_UNROLL for (int j = 0; j < MBJ; ++j) z[j][0] = wv::vfma(W[mj[j] + k * n_out], a, z[j][0]);
                }
                PINN_UNROLL for (int j = 0; j < MBJ; ++j)
                    PINN_UNROLL for (int kf = 0; kf < J::NFIRST; ++kf) z[j][J::CH_FIRST + kf] = W[mj[j] + axis[J::first_axis(kf)] * n_out];
            } else {
                for (int k = 0; k < n_in; ++k) {
                    T ak[C];
                    PINN_UNROLL for (int c = 0; c < C; ++c) ak[c] = in[(k * C + c) * ppb];
                    PINN_UNROLL for (int j = 0; j < MBJ; ++j) {
                        const T w = W[mj[j] + k * n_out];
                        PINN_UNROLL for (int c = 0; c < C; ++c) z[j][c] = wv::vfma(w, ak[c], z[j][c]);
                    }
                }
            }
            if (hidden) {                                // (the class is uniform across the workgroup)
                if (n.act == pk::ACT_SIN) jet_act<J, pk::ACLS_Z_SIN>(kind, z);
                else if (n.act == pk::ACT_SWISH) jet_act<J, pk::ACLS_Z_SWISH>(kind, z);
                else jet_act<J, pk::ACLS_A>(kind, z);
            }
            PINN_UNROLL for (int j = 0; j < MBJ; ++j)
                if (m0 + j < n_out) { PINN_UNROLL for (int c = 0; c < C; ++c) out[((m0 + j) * C + c) * ppb] = z[j][c]; }
        }
    }
    PINN_UNROLL for (int c = 0; c < C; ++c) u[c] = img[(n.nl & 1) * half + c * ppb + t];
}

// lane t of the (sample, block) pair `pair` of a pass: the jet, then channel c into its request's slab preds[dst[c]][s][i] (dropped past n)
template <class T, class J> ENS_DEV void jet_pair_lane(const Net& net, const JetPass& ps, const T* __restrict__ thetas, int nblk, size_t P, const T* __restrict__ pts, int n, int S,
                                                       double* __restrict__ preds, size_t ld, T* img, int ppb, int pair, int t) {
    const int s = pair / nblk, b = pair - s * nblk;
    const int i = b * ppb + t, ic = i < n ? i : n - 1;
    T u[J::C];
    jet_point<T, J>(net, ps.axis, thetas + (size_t)s * P + net.theta0, pts + (size_t)ic * net.sizes[0], img, ppb, t, u);
    PINN_UNROLL for (int c = 0; c < J::C; ++c)
        if (ps.dst[c] >= 0 && i < n) preds[((size_t)ps.dst[c] * (size_t)S + (size_t)s) * ld + i] = (double)u[c];
}
// elements of one workgroup's region of the scratch storage: two images of ppb points
inline size_t jet_region(const Net& n, int C, int ppb) { return 2 * (size_t)n.wmax * (size_t)C * (size_t)ppb; }

// thread i of the statistics: column i of preds [S][ld]
ENS_DEV void stats_point(const double* __restrict__ preds, size_t ld, int S, int ddof, size_t i, double* mean, double* sd) {
    ENS_NO_CONTRACT
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += preds[(size_t)s * ld + i];
    const double m = sum / (double)S;
    double sq = 0.0;
    for (int s = 0; s < S; ++s) {
        const double d = preds[(size_t)s * ld + i] - m;
        sq += d * d;
    }
    mean[i] = m;
    sd[i] = sqrt(sq / (double)(S - ddof));
}

#ifdef PINN_EMU
template <class T> inline int launch_forward(const Net& net, const T* thetas, int S, size_t P, const T* pts, int n, double* preds, size_t ld, int ppb, plat_stream) {
    const int nblk = (n + ppb - 1) / ppb;
    std::vector<T> img(2 * (size_t)net.wmax * ppb);
    for (int s = 0; s < S; ++s)
        for (int b = 0; b < nblk; ++b)
            for (int t = 0; t < ppb; ++t) {
                const int i = b * ppb + t, ic = i < n ? i : n - 1;
                const T u = forward_point<T>(net, thetas + (size_t)s * P + net.theta0, pts + (size_t)ic * net.sizes[0], img.data(), ppb, t);
                if (i < n) preds[(size_t)s * ld + i] = (double)u;
            }
    return 0;
}
inline int launch_stats(const double* preds, size_t ld, int S, int ddof, int n, double* mean, double* sd, plat_stream) {
    for (int i = 0; i < n; ++i) stats_point(preds, ld, S, ddof, (size_t)i, mean, sd);
    return 0;
}
// scratch == nullptr: the images in "LDS" (a local block, one workgroup per pair); else `grid` workgroups, each with its region, stride over the pairs
template <class T, class J> inline int launch_jet_t(const Net& net, const JetPass& ps, const T* thetas, int S, size_t P, const T* pts, int n, double* preds, size_t ld, int ppb,
                                                    T* scratch, int grid, plat_stream) {
    const int nblk = (n + ppb - 1) / ppb, npairs = S * nblk;
    const size_t region = jet_region(net, J::C, ppb);
    std::vector<T> lds(scratch ? 0 : region);
    const int G = scratch ? (grid < npairs ? grid : npairs) : npairs;
    for (int wg = 0; wg < G; ++wg) {
        T* img = scratch ? scratch + (size_t)wg * region : lds.data();
        for (int pair = wg; pair < npairs; pair += G)
            for (int t = 0; t < ppb; ++t) jet_pair_lane<T, J>(net, ps, thetas, nblk, P, pts, n, S, preds, ld, img, ppb, pair, t);
    }
    return 0;
}
#else
// grid: S x nblk workgroups of ppb threads, sample-major; dynamic LDS = lds_bytes(net, ppb, sizeof(T))
template <class T> __global__ void __launch_bounds__(MAX_PPB) k_ens_forward(const Net net, const T* __restrict__ thetas, int nblk, size_t P,
                                                                            const T* __restrict__ pts, int n, double* __restrict__ preds, size_t ld) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ens_lds[];
    T* img = reinterpret_cast<T*>(ens_lds);
    const int s = (int)(blockIdx.x / (unsigned)nblk), b = (int)(blockIdx.x - (unsigned)s * (unsigned)nblk);
    const int ppb = (int)blockDim.x, t = (int)threadIdx.x;
    const int i = b * ppb + t, ic = i < n ? i : n - 1;
    const T u = forward_point<T>(net, thetas + (size_t)s * P + net.theta0, pts + (size_t)ic * net.sizes[0], img, ppb, t);
    if (i < n) preds[(size_t)s * ld + i] = (double)u;
}
__global__ void __launch_bounds__(STATS_BLOCK) k_ens_stats(const double* __restrict__ preds, size_t ld, int S, int ddof, int n, double* __restrict__ mean,
                                                           double* __restrict__ sd) {
    const int i = (int)(blockIdx.x * STATS_BLOCK + threadIdx.x);
    if (i < n) stats_point(preds, ld, S, ddof, (size_t)i, mean, sd);
}
// (both return nonzero when the launch was not accepted: a launch error would otherwise pass unnoticed, the stream staying healthy)
template <class T> inline int launch_forward(const Net& net, const T* thetas, int S, size_t P, const T* pts, int n, double* preds, size_t ld, int ppb, plat_stream st) {
    const int nblk = (n + ppb - 1) / ppb;
    const size_t lds = lds_bytes(net, ppb, sizeof(T));
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)k_ens_forward<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 1;
    hipLaunchKernelGGL(k_ens_forward<T>, dim3((unsigned)S * (unsigned)nblk), dim3(ppb), lds, st, net, thetas, nblk, P, pts, n, preds, ld);
    return hipGetLastError() != hipSuccess;
}
inline int launch_stats(const double* preds, size_t ld, int S, int ddof, int n, double* mean, double* sd, plat_stream st) {
    hipLaunchKernelGGL(k_ens_stats, dim3((n + STATS_BLOCK - 1) / STATS_BLOCK), dim3(STATS_BLOCK), 0, st, preds, ld, S, ddof, n, mean, sd);
    return hipGetLastError() != hipSuccess;
}
// grid: min(npairs, what the launcher bounds it by) workgroups of ppb threads striding over the npairs = S x nblk (sample, block) pairs, sample-major;
// scratch == nullptr: the images in dynamic LDS (lds_bytes with C); else workgroup w owns scratch[w * region, (w + 1) * region)
template <class T, class J> __global__ void __launch_bounds__(MAX_PPB) k_ens_jet(const Net net, const JetPass ps, const T* __restrict__ thetas, int nblk, int npairs, size_t P,
                                                                                 const T* __restrict__ pts, int n, int S, double* __restrict__ preds, size_t ld,
                                                                                 T* __restrict__ scratch, size_t region) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ens_lds[];
    T* img = scratch ? scratch + (size_t)blockIdx.x * region : reinterpret_cast<T*>(ens_lds);
    const int ppb = (int)blockDim.x, t = (int)threadIdx.x;
    for (int pair = (int)blockIdx.x; pair < npairs; pair += (int)gridDim.x)
        jet_pair_lane<T, J>(net, ps, thetas, nblk, P, pts, n, S, preds, ld, img, ppb, pair, t);
}
template <class T, class J> inline int launch_jet_t(const Net& net, const JetPass& ps, const T* thetas, int S, size_t P, const T* pts, int n, double* preds, size_t ld, int ppb,
                                                    T* scratch, int grid, plat_stream st) {
    const int nblk = (n + ppb - 1) / ppb, npairs = S * nblk;
    const size_t lds = scratch ? 0 : lds_bytes(net, ppb, sizeof(T), J::C);
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)k_ens_jet<T, J>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 1;
    const int G = scratch ? (grid < npairs ? grid : npairs) : npairs;
    hipLaunchKernelGGL((k_ens_jet<T, J>), dim3((unsigned)G), dim3(ppb), lds, st, net, ps, thetas, nblk, npairs, P, pts, n, S, preds, ld, scratch, jet_region(net, J::C, ppb));
    return hipGetLastError() != hipSuccess;
}
#endif

// one jet pass of the (sample, block) pairs of `n` points; scratch / grid: see launch_jet_t
template <class T> inline int launch_jet(const Net& net, const JetPass& ps, const T* thetas, int S, size_t P, const T* pts, int n, double* preds, size_t ld, int ppb,
                                         T* scratch, int grid, plat_stream st) {
    switch (ps.kind) {
    case 1: return launch_jet_t<T, JetLine1>(net, ps, thetas, S, P, pts, n, preds, ld, ppb, scratch, grid, st);
    case 2: return launch_jet_t<T, JetLine2>(net, ps, thetas, S, P, pts, n, preds, ld, ppb, scratch, grid, st);
    case 3: return launch_jet_t<T, JetLine3>(net, ps, thetas, S, P, pts, n, preds, ld, ppb, scratch, grid, st);
    case 4: return launch_jet_t<T, JetLine4>(net, ps, thetas, S, P, pts, n, preds, ld, ppb, scratch, grid, st);
    case JET_PAIR: return launch_jet_t<T, JetPair>(net, ps, thetas, S, P, pts, n, preds, ld, ppb, scratch, grid, st);
    }
    return 1;
}

}  // namespace ens
