// adam_kernels.hpp — the kernels only the resident fp32 Adam loop launches (adam.cpp is the one unit that includes this header):
//   k_adam       : the Adam step of every theta element
//   k_total_loss : the evaluation's total weighted loss into the history
//   k_adam_fused : both, and the new parameters scattered into the packed weight images: one launch per step instead of three
//   k_resample   : every redrawn term of a problem and its source channels in one launch (sample_rules.hpp: ResampleTerm)
// The samplers, k_src, k_embed and k_pack serve the evaluation path as well: they stay in aux_kernels.hpp and the loop reaches them through
// engine.cpp (pe::redraw_term, pe::pack_all).
#pragma once
#include "aux_limits.hpp"
#include "plat.hpp"
#include "update_rules.hpp"
#include "sample_rules.hpp"

namespace aux {

// ---- resident-theta training loop ----
// the Adam rule itself lives in update_rules.hpp (shared with the persistent training kernel, pinn_train.hpp)
using ur::adam_update;
AUX_DEV void adam_body(int i, float* theta, float* m, float* v, const float* grad, float lr, float b1, float b2, float eps, float c1, float c2) {
    float mi = m[i], vi = v[i];
    const float t = adam_update(theta[i], mi, vi, grad[i], lr, b1, b2, eps, c1, c2);
    m[i] = mi;
    v[i] = vi;
    theta[i] = t;
}
// the resident loop's update kernel: Adam step of element i, its new value scattered into the packed weight images (inverse pack
// map), and — one thread — the evaluation's total weighted loss into the history: one launch instead of total_loss + adam + pack
struct AdamFusedArgs {
    float* theta; float* m; float* v; const float* out;      // out = [P gradient | K raw per-term sums]
    int P, K;
    float lr, b1, b2, eps, c1, c2;
    const int* inv_ptr; const int* inv_pos;
    float* packed[MAX_PACK_NETS];
    double* hist; int step; const float* w_over_n;
};
AUX_DEV void adam_fused_body(int i, const AdamFusedArgs& a) {
    if (i == 0) {
        double s = 0.0;
        for (int k = 0; k < a.K; ++k) s += (double)a.out[a.P + k] * (double)a.w_over_n[k];
        a.hist[a.step] = s;
    }
    if (i >= a.P) return;
    float mi = a.m[i], vi = a.v[i];
    const float t = adam_update(a.theta[i], mi, vi, a.out[i], a.lr, a.b1, a.b2, a.eps, a.c1, a.c2);
    a.m[i] = mi;
    a.v[i] = vi;
    a.theta[i] = t;
    for (int q = a.inv_ptr[i]; q < a.inv_ptr[i + 1]; ++q) {
        const int pos = a.inv_pos[q];
        a.packed[pos >> 24][pos & 0xFFFFFF] = t;
    }
}
// total weighted loss of one evaluation from the raw per-term sums in out[P..P+K)
AUX_DEV void total_loss_body(double* hist, int step, const float* out, int P, int K, const float* w_over_n) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += (double)out[P + k] * (double)w_over_n[k];
    hist[step] = s;
}

#ifdef PINN_EMU
inline void launch_adam(float* theta, float* m, float* v, const float* grad, int P, float lr, float b1, float b2, float eps, float c1, float c2, plat_stream) {
    for (int i = 0; i < P; ++i) adam_body(i, theta, m, v, grad, lr, b1, b2, eps, c1, c2);
}
inline void launch_total_loss(double* hist, int step, const float* out, int P, int K, const float* w_over_n, plat_stream) {
    total_loss_body(hist, step, out, P, K, w_over_n);
}
inline void launch_adam_fused(const AdamFusedArgs& a, plat_stream) {
    for (int i = 0; i < (a.P > 1 ? a.P : 1); ++i) adam_fused_body(i, a);
}
inline void launch_resample(const ResampleTerm* samp, int nsamp, int max_n, int step, plat_stream) {
    for (int p = 0; p < max_n; ++p) resample_point_sets(samp, nsamp, p, max_n, step);
}
#else
__global__ void k_adam(float* theta, float* m, float* v, const float* grad, int P, float lr, float b1, float b2, float eps, float c1, float c2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P) adam_body(i, theta, m, v, grad, lr, b1, b2, eps, c1, c2);
}
__global__ void k_total_loss(double* hist, int step, const float* out, int P, int K, const float* w_over_n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) total_loss_body(hist, step, out, P, K, w_over_n);
}
inline void launch_adam(float* theta, float* m, float* v, const float* grad, int P, float lr, float b1, float b2, float eps, float c1, float c2, plat_stream st) {
    hipLaunchKernelGGL(k_adam, dim3((P + 255) / 256), dim3(256), 0, st, theta, m, v, grad, P, lr, b1, b2, eps, c1, c2);
}
inline void launch_total_loss(double* hist, int step, const float* out, int P, int K, const float* w_over_n, plat_stream st) {
    hipLaunchKernelGGL(k_total_loss, dim3(1), dim3(64), 0, st, hist, step, out, P, K, w_over_n);
}
// every redrawn term of a problem in ONE launch (sample_rules.hpp: ResampleTerm): one thread per point index over the largest set
__global__ void __launch_bounds__(256) k_resample(const ResampleTerm* samp, int nsamp, int step) {
    resample_point_sets(samp, nsamp, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x), step);
}
inline void launch_resample(const ResampleTerm* samp, int nsamp, int max_n, int step, plat_stream st) {
    hipLaunchKernelGGL(k_resample, dim3((max_n + 255) / 256), dim3(256), 0, st, samp, nsamp, step);
}
__global__ void k_adam_fused(const AdamFusedArgs a) { adam_fused_body((int)(blockIdx.x * blockDim.x + threadIdx.x), a); }
inline void launch_adam_fused(const AdamFusedArgs& a, plat_stream st) {
    hipLaunchKernelGGL(k_adam_fused, dim3((a.P + 255) / 256), dim3(256), 0, st, a);
}
#endif

}  // namespace aux
