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
// Every body exists once; the PINN_EMU build runs the same bodies serially, in the same summation order.
#pragma once
#include <cmath>
#include <cstdint>
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

// bytes of LDS one workgroup of `ppb` points takes: two images [wmax][ppb]
inline size_t lds_bytes(const Net& n, int ppb, size_t elem) { return 2 * (size_t)n.wmax * (size_t)ppb * elem; }
// points per block for this network: the largest of 256 / 128 / 64 within LDS_TARGET, else 64 within LDS_MAX, else 0 (the caller refuses)
inline int pick_ppb(const Net& n, size_t elem) {
    for (int ppb = MAX_PPB; ppb >= MIN_PPB; ppb >>= 1)
        if (lds_bytes(n, ppb, elem) <= LDS_TARGET) return ppb;
    return lds_bytes(n, MIN_PPB, elem) <= LDS_MAX ? MIN_PPB : 0;
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
#endif

}  // namespace ens
