// nuts_kernels.hpp — the device-resident No-U-Turn transition of a Bayesian PINN (pinn_nuts_draws): multinomial NUTS
// with the generalised U-turn criterion in iterative form, on the chain, metric, priors and generator of hmc_kernels.hpp.  The host queues SLOTS
// back to back and reads nothing but the control block between chunks of them:
//     one slot = ONE evaluation of the handle's resident path at the evaluation's copy of theta + ONE k_nuts_step<T> launch
// (T = the evaluation's element type: double in float64 mode, float otherwise).  k_nuts_step is ONE workgroup of 256 threads and a state machine
// on the control block; thread t owns the elements i = t (mod 256) of every vector, so the vector passes need no barrier:
//   JUDGE (an evaluated leaf is pending)   gradient of logp and the second half kick (hmc::leap_body), logp from the K sums
//       (hmc::logp_from_sums), kinetic energy, delta = H0 - H; accept statistic; divergence; progressive multinomial sampling of the subtree's
//       candidate; rho_sub += r; checkpoint (r, rho_sub) at slot popcount(n) when n is even; when n is odd the U-turn checks of the sub-trees
//       that end here, against the checkpoints; after the subtree's last leaf the merge (proposal, logW, rho, the edge) and the whole tree's check.
//       At the end of a transition: row `draw` of the samples, the per-draw statistics, current state <- the tree's proposal;
//       then the next draw's momentum r0 = z / sqrt(minv) and H0.
//   PROPOSE   first half kick and drift from the edge the new subtree grows from (n == 0) or from the moving end, into the evaluation's copy.
//   With every draw of the call done (status DONE) the launch does nothing.
// The arithmetic restates neuralpde.jl_amd/bpinn.py `_nuts_transition` operation by operation with floating-point contraction off (the pragma
// is repeated in every lambda that multiplies and adds).  Every dot product has hmc::k_hmc_energy's fixed order (the contexts of
// qn_kernels.hpp).  No atomics, workgroup barriers only; the control block and all scalars are ordinary stores of the lead thread.
// Vector state (HBM, double): current state, moving end (Args::th_prop, r, g_prop), both edges (theta, r, g), the subtree's and the tree's
// candidates (theta, g; logp in the control block), rho, rho_sub, and the checkpoints r_ck[D][P], rho_ck[D][P]: address base + slot * P + i
// with a workgroup-uniform slot, loads unconditional.
#pragma once
#include "hmc_kernels.hpp"
#include "qn_kernels.hpp"

namespace nuts {

using hmc::Args;

enum { ST_RUN = 0, ST_DONE = 1 };
constexpr int MAX_DEPTH = 10;
constexpr int BLOCK = qn::BLOCK;

struct Ctl {                             // all the host downloads between chunks
    double h0, log_w, logw_sub, sum_acc; // H at the draw's start; log of the tree's / the running subtree's weight; sum of min(1, exp delta)
    double lp_tc, lp_sc;                 // logp of the tree's proposal / of the subtree's candidate
    int status, draw;                    // ST_*; draws completed in this call
    int pending, fresh;                  // a leaf awaits its judgement; the call's first launch (starts draw 0)
    int depth, n, n_leaf, v;             // doublings completed; leaf index in the running subtree; leaves of this draw; its direction (+1 / -1)
};

struct Tree {                            // the sampler's NUTS buffers and a call's arguments
    Ctl* ctl;
    double* th_l; double* r_l; double* g_l;       // [P] left edge
    double* th_r; double* r_r; double* g_r;       // [P] right edge
    double* th_sc; double* g_sc;                  // [P] the running subtree's candidate
    double* th_tc; double* g_tc;                  // [P] the tree's proposal
    double* rho; double* rho_sub;                 // [P] momentum sums of the tree / the running subtree
    double* r_ck; double* rho_ck;                 // [MAX_DEPTH][P] checkpoints
    const double* normals; const double* uniforms;          // [ndraws][P], [ndraws][nu], or null: the generator
    double* samples; double* accept_stat; double* logp;     // [ndraws][P] (nullable), [ndraws], [ndraws]
    int* tree_depth; int* n_leapfrog; int* divergent;       // [ndraws]
    int ndraws, max_depth, nu;           // nu = 2 D + 2^D - 1 uniforms per draw: u_dir[D] | u_merge[D] | u_leaf[2^D - 1]
    double eps, delta_max;
    unsigned seed_lo, seed_hi, ctr0;     // the generator's seed; the draw counter at the call's start
};

HMC_DEV double logaddexp(double x, double y) {           // bpinn.py `_logaddexp`
    HMC_NO_CONTRACT
    const double m = x > y ? x : y;
    if (m == -INFINITY) return -INFINITY;
    return m + log1p(exp(-fabs(x - y)));
}
HMC_DEV double uniform(const Args& a, const Tree& q, int draw, unsigned key, int idx) {
    return q.uniforms ? q.uniforms[(size_t)draw * q.nu + idx] : hmc::rng_uniform(key, (unsigned)(a.P + idx));
}
// sum_i rho_i minv_i r_i <= 0 with rho_i = f(i)
template <class C, class F> HMC_DEV bool turning(C& c, const Args& a, F rho, const double* r) {
    const double d = c.sum(a.P, [&](int i) { HMC_NO_CONTRACT return rho(i) * a.minv[i] * r[i]; });
    return d <= 0.0;
}

template <class T, class C> HMC_DEV void step_body(C& c, const Args& a, const Tree& q, const T* ev, const double* sse) {
    HMC_NO_CONTRACT
    const int P = a.P, D = q.max_depth;
    Ctl k = *q.ctl;                                      // every thread reads the block before anyone writes it (the barrier below)
    c.sync();
    if (k.status != ST_RUN) return;
    bool start = k.fresh != 0, ended = false;
    k.fresh = 0;
    unsigned key = hmc::rng_key(q.seed_lo, q.seed_hi, q.ctr0 + (unsigned)k.draw);
    if (k.pending) {
        // ---- JUDGE the leaf at the moving end
        k.pending = 0;
        const int n = k.n;
        const double s = (double)k.v * q.eps, kick = 0.5 * s;
        c.each(P, [&](int i) { hmc::leap_body<T>(i, a, ev, kick, s, 0); });
        const double kin = c.sum(P, [&](int i) { HMC_NO_CONTRACT const double r = a.r[i]; return a.minv[i] * r * r; });
        const double pri = c.sum(a.nn, [&](int i) { HMC_NO_CONTRACT const double z = (a.th_prop[i] - a.nn_mu) / a.nn_sigma; return z * z; });
        const double lp = hmc::logp_from_sums(a, pri, sse);
        const double h = -lp + 0.5 * kin;
        double delta = k.h0 - h;
        if (!hmc::is_finite(delta)) delta = -INFINITY;
        k.sum_acc += exp(delta < 0.0 ? delta : 0.0);
        ++k.n_leaf;
        int divergent = 0;
        if (!(-delta <= q.delta_max)) { divergent = 1; ended = true; }
        else {
            k.logw_sub = logaddexp(n == 0 ? -INFINITY : k.logw_sub, delta);
            const double ul = uniform(a, q, k.draw, key, 2 * D + k.n_leaf - 1);
            if (n == 0 || ul < exp(delta - k.logw_sub)) {
                c.each(P, [&](int i) { q.th_sc[i] = a.th_prop[i]; q.g_sc[i] = a.g_prop[i]; });
                k.lp_sc = lp;
            }
            const int even = (n & 1) == 0;
            double* rc_w = q.r_ck + (size_t)__builtin_popcount((unsigned)n) * P;      // (n even and < 2^(D - 1): slot <= D - 2)
            double* pc_w = q.rho_ck + (size_t)__builtin_popcount((unsigned)n) * P;
            c.each(P, [&](int i) {
                const double r = a.r[i];
                const double rs = (n == 0 ? 0.0 : q.rho_sub[i]) + r;
                q.rho_sub[i] = rs;
                if (even) { rc_w[i] = r; pc_w[i] = rs; }
            });
            if (!even) {                                 // the sub-trees of 2, 4, ... 2^kk leaves that end at this leaf
                const int i_max = __builtin_popcount((unsigned)(n >> 1));
                int kk = 0;
                while ((n >> kk) & 1) ++kk;
                for (int j = i_max; j > i_max - kk && !ended; --j) {
                    const double* rc = q.r_ck + (size_t)j * P;
                    const double* pc = q.rho_ck + (size_t)j * P;
                    auto rho_s = [&](int i) { return q.rho_sub[i] - pc[i] + rc[i]; };
                    ended = turning(c, a, rho_s, rc) || turning(c, a, rho_s, a.r);
                }
            }
            if (!ended && n == (1 << k.depth) - 1) {
                // ---- the subtree is complete: merge
                const double um = uniform(a, q, k.draw, key, D + k.depth);
                if (um < exp(k.logw_sub - k.log_w)) {
                    c.each(P, [&](int i) { q.th_tc[i] = q.th_sc[i]; q.g_tc[i] = q.g_sc[i]; });
                    k.lp_tc = k.lp_sc;
                }
                k.log_w = logaddexp(k.log_w, k.logw_sub);
                double* th_e = k.v > 0 ? q.th_r : q.th_l;
                double* r_e = k.v > 0 ? q.r_r : q.r_l;
                double* g_e = k.v > 0 ? q.g_r : q.g_l;
                c.each(P, [&](int i) {
                    q.rho[i] = q.rho[i] + q.rho_sub[i];
                    th_e[i] = a.th_prop[i]; r_e[i] = a.r[i]; g_e[i] = a.g_prop[i];
                });
                ++k.depth;
                k.n = 0;
                auto rho_t = [&](int i) { return q.rho[i]; };
                ended = turning(c, a, rho_t, q.r_l) || turning(c, a, rho_t, q.r_r);
                if (k.depth >= D) ended = true;
            } else if (!ended) ++k.n;
        }
        if (ended) {
            // ---- the transition's result: the tree's proposal becomes the current state
            double* row = q.samples ? q.samples + (size_t)k.draw * P : nullptr;
            c.each(P, [&](int i) {
                const double x = q.th_tc[i];
                a.th_cur[i] = x;
                a.g_cur[i] = q.g_tc[i];
                if (row) row[i] = x;
            });
            if (c.lead()) {
                q.accept_stat[k.draw] = k.sum_acc / (double)k.n_leaf;
                q.logp[k.draw] = k.lp_tc;
                q.tree_depth[k.draw] = k.depth;
                q.n_leapfrog[k.draw] = k.n_leaf;
                q.divergent[k.draw] = divergent;
                a.sc[hmc::SC_LP_CUR] = k.lp_tc;          // (read only by a call's first launch, which judges nothing)
            }
            ++k.draw;
            if (k.draw < q.ndraws) start = true;
            else k.status = ST_DONE;
        }
    }
    if (start) {
        // ---- the next draw: momentum, H0, both edges and the proposal at the current state
        const double lp_cur = ended ? k.lp_tc : a.sc[hmc::SC_LP_CUR];
        key = hmc::rng_key(q.seed_lo, q.seed_hi, q.ctr0 + (unsigned)k.draw);
        const double* z = q.normals ? q.normals + (size_t)k.draw * P : nullptr;
        c.each(P, [&](int i) {
            const double r0 = (z ? z[i] : hmc::rng_normal(key, (unsigned)i)) / sqrt(a.minv[i]);
            const double x = a.th_cur[i], g = a.g_cur[i];
            q.th_l[i] = x; q.r_l[i] = r0; q.g_l[i] = g;
            q.th_r[i] = x; q.r_r[i] = r0; q.g_r[i] = g;
            q.th_tc[i] = x; q.g_tc[i] = g;
            q.rho[i] = r0;
        });
        const double kin0 = c.sum(P, [&](int i) { HMC_NO_CONTRACT const double r = q.r_l[i]; return a.minv[i] * r * r; });
        k.h0 = -lp_cur + 0.5 * kin0;
        k.lp_tc = lp_cur;
        k.log_w = 0.0; k.logw_sub = 0.0; k.sum_acc = 0.0;
        k.depth = 0; k.n = 0; k.n_leaf = 0;
    }
    if (k.status == ST_RUN) {
        // ---- PROPOSE the next leaf: half kick and drift from the edge (a new subtree) or the moving end
        if (k.n == 0) k.v = uniform(a, q, k.draw, key, k.depth) < 0.5 ? 1 : -1;
        const double* th_s = k.n > 0 ? a.th_prop : (k.v > 0 ? q.th_r : q.th_l);
        const double* r_s = k.n > 0 ? a.r : (k.v > 0 ? q.r_r : q.r_l);
        const double* g_s = k.n > 0 ? a.g_prop : (k.v > 0 ? q.g_r : q.g_l);
        const double s = (double)k.v * q.eps, kick = 0.5 * s;
        c.each(P, [&](int i) {
            HMC_NO_CONTRACT
            const double r = r_s[i] + kick * g_s[i];
            const double x = th_s[i] + s * a.minv[i] * r;
            a.r[i] = r;
            a.th_prop[i] = x;
            if (a.th_eval64) a.th_eval64[i] = x;
            if (a.th_eval32) a.th_eval32[i] = (float)x;
        });
        k.pending = 1;
    }
    if (c.lead()) *q.ctl = k;
}

#ifdef PINN_EMU
template <class T> inline void launch_step(const Args& a, const Tree& q, const T* ev, const double* sse, plat_stream) {
    qn::EmuCtx c;
    step_body<T>(c, a, q, ev, sse);
}
#else
template <class T> __global__ void __launch_bounds__(BLOCK) k_nuts_step(const Args a, const Tree q, const T* ev, const double* sse) {
    __shared__ double sh[BLOCK / qn::WAVE];
    qn::DevCtx c{sh, (int)threadIdx.x};
    step_body<T>(c, a, q, ev, sse);
}
template <class T> inline void launch_step(const Args& a, const Tree& q, const T* ev, const double* sse, plat_stream st) {
    hipLaunchKernelGGL(k_nuts_step<T>, dim3(1), dim3(BLOCK), 0, st, a, q, ev, sse);
}
#endif

}  // namespace nuts
