// lbfgs_replica_kernels.hpp — replica-resident L-BFGS (pinn_lbfgs_replicas_*): the quasi-Newton finisher of nrep
// trainings of ONE discretised problem in ONE launch, one workgroup each.
//
// The resident finisher of section 4.8 pays, per slot, one 256-thread control launch plus the handle's multi-launch evaluation; the networks the
// replicas serve (12..32 wide, 100..1,000 points) fill one or two waves of either.  A replica needs nothing from any other, so here workgroup r
// (four waves, as every family-1 launch) OWNS replica r for the whole launch, and what the iteration touches most lives in LDS behind the
// evaluation's S::LDS_WG floats:
//
//     (once)       x | g | xn | d of the replica (4 P doubles) and its control block HBM -> LDS; the trial point narrowed into theta32 (LDS) and
//                  scattered into the replica's weight image and parameter row
//     (per slot)   barrier | when a trial point awaits its evaluation — wave_main<MODE_FUSED>: the four waves walk ALL tiles of ALL K terms,
//                            weights register-resident from the replica's own image -> the replica's gradient slab and per-wave loss partials
//                  barrier | thread t sums the slab entries of elements t, t + 256, ... (replica_slab_sum: map order, one double, narrowed) into
//                            ev (LDS); thread 0 forms the K term sums from the four waves' partials in wave order (replica_term_sum)
//                  barrier | lbfgs::step_body<float> over the workgroup (qn::DevCtx): JUDGE the evaluation, PROPOSE the next trial point — the
//                            text of the single-training finisher, its arguments pointing into LDS; the rings S, Y, rho stay in HBM, read at
//                            workgroup-uniform slots with affine, unconditional addresses
//                  barrier | a terminal status (CONVERGED / STALLED / MAXITER) ends the replica's loop: its workgroup retires.  Otherwise every
//                            thread scatters its elements of the new theta32 into the image and the parameter row
//     (once)       LDS -> the replica's HBM rows, its control block and the last evaluation's K sums
//
// A slot proposes at most one trial point, as section 4.8's; the first slot after _init (or after a call that ended on a terminal status) has no
// evaluation to judge and only proposes.  A launch that ends at its slot bound leaves a proposed, unevaluated point (pending = 1) in xn: the next
// launch evaluates it first, so a call may end inside a line search and resume there.  Every branch depends on the control block, the kernel's
// arguments and workgroup-uniform sums only, so every barrier is reached by all 256 threads; replicas run different numbers of slots and nothing
// one workgroup writes is read by another: no grid barrier, no atomics, no loop that waits on memory.
// The PINN_EMU build runs the same text: the four waves as host threads, a wave's 64 threads serially, step_body with qn::EmuCtx on wave 0.
#pragma once
#include "adam_replica_kernels.hpp"
#include "lbfgs_kernels.hpp"

namespace pk {

constexpr int LBFGS_REPLICA_MAX_SLOTS = 4096;        // slots per launch: no launch runs for seconds on a shared device
constexpr int LBFGS_REPLICA_MAX_TERMS = 16;          // term sums held in LDS (a launch group has at most MAX_GROUP_TERMS)
enum { LBFGS_REPLICA_SLOTS = 0, LBFGS_REPLICA_ADOPT = 1 };
// the scalars of a replica in LDS, in doubles: alpha | rho | the context's per-wave sums | the term sums | the control block
constexpr int LBFGS_REPLICA_SCALARS = 2 * lbfgs::MAX_HISTORY + 4 + LBFGS_REPLICA_MAX_TERMS + 8;
static_assert(sizeof(lbfgs::Ctl) <= 8 * sizeof(double), "the control block's room in LDS");
static_assert(MAX_GROUP_TERMS <= LBFGS_REPLICA_MAX_TERMS, "the term sums' room in LDS");
// floats of LDS of a workgroup: the evaluation's (padded to a double's alignment), 4 vectors of doubles, the scalars, theta32 | ev
constexpr int lbfgs_replica_lds(int eval_floats) {
    return ((eval_floats + 1) & ~1) + 2 * (4 * REPLICA_MAX_P + LBFGS_REPLICA_SCALARS) + 2 * REPLICA_MAX_P;
}

struct LbfgsReplicaArgs {
    ReplicaArgs r;               // packed, params, defaults, the four maps, P, K, np, ne, p_off (the Adam members are not read)
    double* state;               // [nrep][4 P]: x | g | xn | d rows of every replica
    double* rings;               // [nrep][2 m P + m]: S | Y | rho
    lbfgs::Ctl* ctl;             // [nrep]
    double* sums;                // [nrep][K] raw sums of squares of the last evaluation
    double* hist;                // [nrep][hist_stride] objective after iteration it0 + i of the running call
    const double* tab;           // [2 K]: term weights | n_norm
    const int* call;             // [nrep][3]: it0, it_end, slots of this launch
    int m, mode, hist_stride;    // history; LBFGS_REPLICA_SLOTS / _ADOPT
    double gtol;
};

// the wave program: replica `rep`, wave `w` of its workgroup; lds = [S::LDS_WG evaluation | x g xn d | scalars | theta32 ev]
template <class S, int ACTK>
DEV void wave_lbfgs_replicas(const GroupArgs& ga, const LbfgsReplicaArgs& la, int rep, int w, float* lds) {
    const ReplicaArgs& ra = la.r;
    const bool adopt = la.mode == LBFGS_REPLICA_ADOPT;
    const int P = ra.P, K = ra.K;
    const size_t r = (size_t)rep, m = (size_t)la.m;
    const int it0 = la.call[3 * rep], it_end = la.call[3 * rep + 1], nslots = adopt ? 1 : la.call[3 * rep + 2];
    if (nslots <= 0) return;                             // (a terminal replica, or no evaluations left: its rows stay as they are)
    double* dv = reinterpret_cast<double*>(lds + ((S::LDS_WG + 1) & ~1));
    double* al = dv + 4 * REPLICA_MAX_P;
    double* rh = al + lbfgs::MAX_HISTORY;
    double* sh = rh + lbfgs::MAX_HISTORY;
    double* sums = sh + 4;
    lbfgs::Ctl* ctl = reinterpret_cast<lbfgs::Ctl*>(sums + LBFGS_REPLICA_MAX_TERMS);
    float* th32 = reinterpret_cast<float*>(dv + 4 * REPLICA_MAX_P + LBFGS_REPLICA_SCALARS);
    float* ev = th32 + REPLICA_MAX_P;
    lbfgs::Args a{};
    a.P = P; a.K = K; a.f64form = 0; a.m = la.m;
    a.x = dv; a.g = dv + P; a.xn = dv + 2 * P; a.d = dv + 3 * P;
    a.w = la.tab; a.nrm = la.tab + K; a.sums = sums;
    a.loss_hist = la.hist + r * (size_t)la.hist_stride;
    a.th_eval64 = nullptr; a.th_eval32 = th32;
    a.S = la.rings + r * (2 * m * (size_t)P + m); a.Y = a.S + m * (size_t)P; a.rho = a.Y + m * (size_t)P;
    a.ctl = ctl;
    ReplicaView v{};
    v.image = ra.packed + r * S::PACKED;
    v.params = ra.params + r * MAX_PARAMS;
    v.slab = ga.slabs + r * S::SLAB;
    v.lossp = ga.losspart + r * 4 * (size_t)ga.nterms_total;
    double* row = la.state + r * 4 * (size_t)P;
    // the replica's vectors into LDS (thread t: the elements t, t + 256, ... of each, the ones it alone touches afterwards); its image and
    // parameter row from the point to evaluate: x at ADOPT, the trial point otherwise (the host zeroed the images' padding once)
    { REPLICA_THREADS_OF(t, w) {
        for (int i = t; i < P; i += REPLICA_THREADS) {
            for (int j = 0; j < 4; ++j) dv[j * P + i] = row[(size_t)j * P + i];
            const float x = (float)row[(adopt ? 0 : 2 * (size_t)P) + i];
            th32[i] = x;
            replica_scatter(i, ra, v, x);
        }
        if (t >= ra.ne && t < ra.np) v.params[t] = ra.defaults[t];
    } }
    if (REPLICA_FIRST(w)) {
        *ctl = la.ctl[rep];
        for (int k = 0; k < K; ++k) sums[k] = la.sums[r * (size_t)K + k];
    }
    for (int s = 0; s < nslots; ++s) {
        wg_barrier();                                    // the image, the parameter row and the control block are written
        if (adopt || ctl->pending) {
            wave_main<S, MODE_FUSED, ACTK>(ga, 0, 1, w, lds, rep);
            wg_barrier();                                // the slab and the loss partials are written
            { REPLICA_THREADS_OF(t, w)
                for (int i = t; i < P; i += REPLICA_THREADS) ev[i] = (float)replica_slab_sum(i, ra, v); }
            if (REPLICA_FIRST(w))
                for (int k = 0; k < K; ++k) sums[k] = replica_term_sum(k, v, ga.nterms_total);
        }
        wg_barrier();                                    // ev and the sums are written; every wave has read `pending`
        const int qmode = adopt ? lbfgs::MODE_ADOPT : lbfgs::MODE_SLOT;
#ifdef PINN_EMU
        if (w == 0) {
            qn::EmuCtx c;
            lbfgs::step_body<float>(c, al, rh, a, ev, qmode, it0, it_end, la.gtol);
        }
#else
        qn::DevCtx c{sh, (int)threadIdx.x};
        lbfgs::step_body<float>(c, al, rh, a, ev, qmode, it0, it_end, la.gtol);
#endif
        wg_barrier();                                    // the control block, the vectors and theta32 are written
        if (adopt || ctl->status >= qn::ST_CONVERGED) break;
        { REPLICA_THREADS_OF(t, w)
            for (int i = t; i < P; i += REPLICA_THREADS) replica_scatter(i, ra, v, th32[i]); }
    }
    // (behind the last slot's barrier: every thread writes back the elements it loaded)
    { REPLICA_THREADS_OF(t, w)
        for (int i = t; i < P; i += REPLICA_THREADS)
            for (int j = 0; j < 4; ++j) row[(size_t)j * P + i] = dv[j * P + i]; }
    if (REPLICA_FIRST(w)) {
        la.ctl[rep] = *ctl;
        for (int k = 0; k < K; ++k) la.sums[r * (size_t)K + k] = sums[k];
    }
}

}  // namespace pk
