// adam_replica_kernels.hpp — replica-resident Adam (pinn_adam_replicas_*): nrep independent Adam trainings of ONE
// discretised problem in ONE launch, one workgroup each.
//
// The persistent training kernel (pinn_train.hpp) runs one training on at most 32 workgroups joined by a grid barrier; a 12..32-wide network
// on 100..1,000 points fills one or two waves of it.  Restarts from several initialisations, learning-rate sweeps and deep ensembles need
// nothing from one another, so here workgroup r (four waves, as every family-1 launch) OWNS replica r for the whole call and its optimiser
// state lives in LDS:
//
//     (once)       theta | m | v of the replica (3 P floats) HBM -> LDS, behind the evaluation's S::LDS_WG floats; lr[r] into a register
//     (per step)   barrier | wave_main<MODE_FUSED>: the four waves walk ALL tiles of ALL K terms (tile t = 4 it + w), weights register-resident
//                            from the replica's own image -> the replica's gradient slab and per-wave loss partials
//                  barrier | thread t owns elements t, t + 256, ... of theta: the fixed-order double sum of the element's slab entries (map order,
//                            the association of aux::reduce_direct_body for one workgroup), narrowed to float; ur::adam_update on the LDS
//                            state; the new value into the LDS theta and straight into the element's positions of the replica's weight image
//                            (and parameter row).  Thread 0: the four waves' loss partials per term in wave order -> hist[r][step], the loss
//                            at the iterate BEFORE the update, as pinn_adam_steps records it
//     (once)       LDS -> the replica's HBM rows; the last evaluation's K sums of squares
//
// Inside the step loop the HBM traffic is the evaluation's own (image, slab, loss partials, record scratch: slice r of each, as ChainArgs), the
// shared read-only maps and one history store.  Nothing one workgroup writes is read by another: no grid barrier, no atomics, no loop that
// waits on memory; every barrier is a workgroup barrier reached by all 256 threads under uniform control flow (the loop bounds are kernel
// arguments), so workgroups beyond the CU count simply queue.  The PINN_EMU build runs the same text: the four waves as host threads, a wave's
// 64 threads serially.
#pragma once
#include "pinn_kernels.hpp"
#include "update_rules.hpp"

namespace pk {

constexpr int REPLICA_MAX_P = 2048;          // theta elements per replica: the LDS state block is 3 x REPLICA_MAX_P floats (24 KB) behind S::LDS_WG
constexpr int REPLICA_MAX_REPLICAS = 1024;   // replicas per handle (each has its own image, slab, loss partials and record scratch)
constexpr int REPLICA_THREADS = 256;
constexpr int REPLICA_MAX_STEPS = 4096;      // steps per launch: no launch runs for seconds on a shared device

struct ReplicaArgs {
    float* state;                // [nrep][3 P]: theta | m | v rows of every replica
    float* packed;               // [nrep][Spec::PACKED] weight images
    float* params;               // [nrep][MAX_PARAMS] parameter rows of the residual tape
    double* sse;                 // [nrep][K] raw sums of squares of the last evaluation
    double* hist;                // [nrep][hist_stride] total weighted loss of every step's evaluation
    const float* lr;             // [nrep]
    const float* c12;            // [2 * nsteps]: 1 / (1 - b1^t), 1 / (1 - b2^t) of every step of this launch
    const float* w_over_n;       // [K]
    const float* defaults;       // [np] PDE parameters that are not estimated
    const int* row_ptr; const int* row_ent;      // theta element -> slab entries (the handle's reduce map)
    const int* inv_ptr; const int* inv_pos;      // theta element -> image positions (the handle's inverse pack map)
    int P, K, np, ne, p_off;     // PDE parameters, the first ne of them estimated: theta elements [p_off, p_off + ne)
    int nsteps, hist_stride;
    float b1, b2, eps;
};

// a wave's threads: the device runs the statement once per thread; the emulation, serially for the wave's 64
#ifdef PINN_EMU
#define REPLICA_THREADS_OF(t, w) for (int t = (w) * 64; t < (w) * 64 + 64; ++t)
#define REPLICA_FIRST(w) ((w) == 0)
#else
#define REPLICA_THREADS_OF(t, w) const int t = (int)threadIdx.x;
#define REPLICA_FIRST(w) (threadIdx.x == 0)
#endif

struct ReplicaView {             // replica r's slices
    float* th; float* m; float* v;               // LDS
    float* image; float* params;
    const float* slab; const double* lossp;
};

// value x of element i into the replica's weight image and parameter row: what k_pack / k_params make of theta[i]
DEV void replica_scatter(int i, const ReplicaArgs& ra, const ReplicaView& v, float x) {
    const int q1 = ra.inv_ptr[i + 1];
    for (int q = ra.inv_ptr[i]; q < q1; ++q) v.image[ra.inv_pos[q] & 0xFFFFFF] = x;
    if (i >= ra.p_off && i < ra.p_off + ra.ne) v.params[i - ra.p_off] = x;
}
// element i of the evaluation's gradient: its slab entries in map order, one double accumulator (lbfgs_replica_kernels.hpp sums likewise)
DEV double replica_slab_sum(int i, const ReplicaArgs& ra, const ReplicaView& v) {
    double s = 0.0;
    const int e1 = ra.row_ptr[i + 1];
    for (int e = ra.row_ptr[i]; e < e1; ++e) s += (double)v.slab[ra.row_ent[e]];
    return s;
}
// element i after an evaluation: the gradient narrowed; the Adam rule on the LDS state
DEV void replica_update(int i, const ReplicaArgs& ra, const ReplicaView& v, float lr, float c1, float c2) {
    float mi = v.m[i], vi = v.v[i];
    const float t = ur::adam_update(v.th[i], mi, vi, (float)replica_slab_sum(i, ra, v), lr, ra.b1, ra.b2, ra.eps, c1, c2);
    v.m[i] = mi;
    v.v[i] = vi;
    v.th[i] = t;
    replica_scatter(i, ra, v, t);
}
// raw sum of squares of term k: the four waves' partials in wave order (aux::reduce_direct_body)
DEV double replica_term_sum(int k, const ReplicaView& v, int nterms_total) {
    double s = 0.0;
    for (int j = 0; j < 4; ++j) s += v.lossp[(size_t)j * nterms_total + k];
    return s;
}

// the wave program: replica `rep`, wave `w` of its workgroup; lds = [S::LDS_WG evaluation | 3 x REPLICA_MAX_P state]
template <class S, int ACTK>
DEV void wave_adam_replicas(const GroupArgs& ga, const ReplicaArgs& ra, int rep, int w, float* lds) {
    const size_t P = (size_t)ra.P, r = (size_t)rep;
    float* row = ra.state + r * 3 * P;
    ReplicaView v;
    v.th = lds + S::LDS_WG; v.m = v.th + P; v.v = v.m + P;
    v.image = ra.packed + r * S::PACKED;
    v.params = ra.params + r * MAX_PARAMS;
    v.slab = ga.slabs + r * S::SLAB;
    v.lossp = ga.losspart + r * 4 * (size_t)ga.nterms_total;
    const float lr = ra.lr[rep];
    double* hist = ra.hist + r * (size_t)ra.hist_stride;
    // the replica's state into LDS; its image and parameter row from theta (the host zeroed the images' padding once)
    { REPLICA_THREADS_OF(t, w) {
        for (int i = t; i < ra.P; i += REPLICA_THREADS) {
            const float x = row[i];
            v.th[i] = x; v.m[i] = row[P + i]; v.v[i] = row[2 * P + i];
            replica_scatter(i, ra, v, x);
        }
        if (t >= ra.ne && t < ra.np) v.params[t] = ra.defaults[t];
    } }
    for (int s = 0; s < ra.nsteps; ++s) {
        wg_barrier();                                    // the image and the parameter row are written
        wave_main<S, MODE_FUSED, ACTK>(ga, 0, 1, w, lds, rep);
        wg_barrier();                                    // the slab and the loss partials are written
        const float c1 = ra.c12[2 * s], c2 = ra.c12[2 * s + 1];
        { REPLICA_THREADS_OF(t, w)
            for (int i = t; i < ra.P; i += REPLICA_THREADS) replica_update(i, ra, v, lr, c1, c2); }
        if (REPLICA_FIRST(w)) {                          // aux::total_loss_body on the narrowed sums
            double tot = 0.0;
            for (int k = 0; k < ra.K; ++k) tot += (double)(float)replica_term_sum(k, v, ga.nterms_total) * (double)ra.w_over_n[k];
            hist[s] = tot;
        }
    }
    // (no barrier: every thread writes back the elements it alone updated; the loss partials are those of the last evaluation)
    { REPLICA_THREADS_OF(t, w)
        for (int i = t; i < ra.P; i += REPLICA_THREADS) { row[i] = v.th[i]; row[P + i] = v.m[i]; row[2 * P + i] = v.v[i]; } }
    if (REPLICA_FIRST(w))
        for (int k = 0; k < ra.K; ++k) ra.sse[r * (size_t)ra.K + k] = replica_term_sum(k, v, ga.nterms_total);
}

}  // namespace pk
