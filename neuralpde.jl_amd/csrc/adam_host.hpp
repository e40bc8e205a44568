// adam_host.hpp — the two pieces of adam.cpp that are plain host arithmetic: no engine types, no device calls, so that a stand-alone program
// can drive them under the host sanitizers (tools/micro/adam_host_check.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace pe {

// Adam's bias correction of step t (1-based), 1 / (1 - beta^t), formed in double and narrowed once: what every update kernel takes as c1 / c2
inline float adam_bias(float beta, long long t) { return (float)(1.0 / (1.0 - std::pow((double)beta, (double)t))); }

// thread -> element map of the persistent training kernel (pinn_train.hpp: TrainArgs::own_r) for a launch of `blocks` workgroups of 256
// threads, blocks * 256 >= P + K.  row_theta / row_ptr / row_off: the launch group's CSR theta element -> slab offsets (Group).
// Theta element r sits at gid = its FIRST slab entry when those are distinct and leave room for the K sums at the end of the grid (lanes of
// a wave then read consecutive slab entries: coalesced; `coalesce` false: never), else at gid = r; the K sums take threads without an
// element, from the end of the grid; -1: the thread owns nothing.  *hist_gid: the last such thread (it writes the loss history), 0 if none.
inline std::vector<int> train_thread_map(const std::vector<int>& row_theta, const std::vector<int>& row_ptr, const std::vector<int>& row_off,
                                         int blocks, int P, int K, bool coalesce, int* hist_gid) {
    const int nthr = blocks * 256;
    std::vector<int> own((size_t)nthr, -1);
    bool by_entry = true;
    for (size_t i = 0; i < row_theta.size() && by_entry; ++i) {
        const int e0 = row_ptr[i] < row_ptr[i + 1] ? row_off[row_ptr[i]] : -1;
        if (e0 < 0 || e0 >= nthr - K || own[(size_t)e0] >= 0) by_entry = false;
        else own[(size_t)e0] = row_theta[i];
    }
    int placed = 0;
    for (int v : own) placed += v >= 0;
    if (!by_entry || placed != P || !coalesce) {
        std::fill(own.begin(), own.end(), -1);
        for (int r = 0; r < P; ++r) own[(size_t)r] = r;
    } else {
        // 64-entry groups dealt round-robin over the workgroups (group g -> workgroup g % blocks, wave g / blocks): the slab reads of an
        // update spread over every CU of the launch instead of the first ceil(PW / 256)
        int last = 0;
        for (int e = 0; e < nthr; ++e) if (own[(size_t)e] >= 0) last = e;
        const int ngroups = last / 64 + 1;
        if ((ngroups + blocks - 1) / blocks <= 4) {
            std::vector<int> dealt((size_t)nthr, -1);
            for (int g = 0; g < ngroups; ++g)
                for (int l = 0; l < 64; ++l) dealt[(size_t)((g % blocks) * 256 + (g / blocks) * 64 + l)] = own[(size_t)(g * 64 + l)];
            own.swap(dealt);
        }
    }
    for (int k = 0, gid = nthr - 1; k < K && gid >= 0; --gid)           // the K sums: threads without an element, from the end of the grid
        if (own[(size_t)gid] < 0) own[(size_t)gid] = P + k++;
    *hist_gid = 0;
    for (int gid = nthr - 1; gid >= 0; --gid) if (own[(size_t)gid] < 0) { *hist_gid = gid; break; }
    return own;
}

}  // namespace pe
