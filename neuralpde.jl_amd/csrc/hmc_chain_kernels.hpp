// hmc_chain_kernels.hpp — chain-resident HMC (pinn_hmc_chains_*): nchains BPINN chains in ONE launch, one workgroup each.
//
// The resident sampler of section 4.7 pays, per leapfrog step, the evaluation's launches plus one update launch: 17-28 us for the networks
// BPINNs are used with (1-6-1 .. 1-16-16-1 on 13 .. 100 points), whose arithmetic fills one or two waves.  A chain needs nothing from any other
// chain, so here workgroup c (four waves, as every family-1 launch) OWNS chain c for the whole call and runs whole trajectories between
// workgroup barriers only:
//
//     (per draw)   momentum -> H_old -> half kick + drift -> image
//     (per step)   barrier | wave_main<MODE_FUSED>: the four waves walk ALL tiles of ALL K terms (tile t = 4 it + w), weights register-resident
//                            from the chain's own image -> the chain's gradient slab and per-wave loss partials
//                  barrier | thread t owns elements t, t + 256, ... of theta: the fixed-order double sum of the element's slab entries (map order,
//                            the association of aux::reduce_direct_body for one workgroup), narrowed to float as the evaluation's output is;
//                            hmc::leap_body<float> — log-posterior gradient with the priors, kick, drift, in double; the narrowed new value
//                            stored straight into the element's positions of the chain's weight image (and parameter row)
//     (per draw)   H_new (hmc::energy_partial / energy_finish: strided sums, xor butterfly per wave, the four waves in order) -> accept
//
// Nothing one workgroup writes is read by another inside the launch: no grid barrier, no atomics, no loop that waits on memory.  Every chain
// has its slice of every buffer at an offset affine in the chain index — state (theta, momentum, gradients, energies: double), weight image
// (the layout aux::k_pack produces), parameter row, record scratch, gradient slab, loss partials; point sets, inverse metric, priors and the
// maps are shared and read-only.  The bodies are those of hmc_rules.hpp, so a chain's arithmetic is the resident sampler's operation by
// operation; what differs is the evaluation's tile -> wave assignment (one workgroup here), i.e. the fp32 association of the slab sums.
// The PINN_EMU build runs the same text: the four waves as host threads, a wave's 64 threads serially, the butterfly restated.
#pragma once
#include "pinn_kernels.hpp"
#include "hmc_rules.hpp"

namespace pk {

constexpr int CHAIN_MAX_ELEMS = 8;           // theta elements per thread the host admits: P <= 256 * CHAIN_MAX_ELEMS.  A stated bound, not a structural one: the
                                             // update's loops are strided and re-read their maps every step (no per-thread registers hold them), so nothing in the
                                             // kernel depends on it; it keeps the update phase small beside the evaluation of a network of at most 32 units
constexpr int CHAIN_MAX_CHAINS = 1024;       // chains per handle (each has its own record scratch: 4 x Spec::SCR floats)

struct ChainArgs {
    hmc::Args a;                 // shared tables and sizes; the per-chain pointers (th_cur .. g_prop, sc) are formed in the kernel
    double* state;               // [nchains][5 P + SC_COUNT]: th_cur | th_prop | r | g_cur | g_prop | scalars
    float* packed;               // [nchains][Spec::PACKED] weight images
    float* params;               // [nchains][MAX_PARAMS] parameter rows of the residual tape
    float* ev;                   // [nchains][P] the evaluation's gradient, narrowed to float
    double* sse;                 // [nchains][K] its sums of squares
    const float* defaults;       // [np] PDE parameters that are not estimated
    const int* row_ptr; const int* row_ent;      // theta element -> slab entries (the handle's reduce map)
    const int* inv_ptr; const int* inv_pos;      // theta element -> image positions (the handle's inverse pack map)
    int np, ne, p_off;           // PDE parameters, the first ne of them estimated: theta elements [p_off, p_off + ne)
    int init;                    // 1: logp and its gradient at th_cur (the image is packed first), no draws
    int ndraws, n_leapfrog;
    double eps;
    const double* momenta;       // [nchains][ndraws][P] or nullptr: the generator
    const double* uniforms;      // [nchains][ndraws] or nullptr
    double* samples;             // [nchains][ndraws][P]
    double* accept_prob; double* logp;           // [nchains][ndraws]
    unsigned seed_lo, seed_hi, ctr0;             // the generator's seed and the draw counter of this call's first draw
};

// the generator's key of (draw, chain): chain 0 is the stream of pinn_hmc_draws
DEV unsigned chain_key(unsigned seed_lo, unsigned seed_hi, unsigned ctr, unsigned chain) {
    const unsigned key = hmc::rng_key(seed_lo, seed_hi, ctr);
    return chain == 0u ? key : aux::mix32(key ^ aux::mix32(chain * 0xCC9E2D51U + 0x1B873593U));
}

// a wave's threads: the device runs the statement once per thread; the emulation, serially for the wave's 64
#ifdef PINN_EMU
#define CHAIN_THREADS(t, w) for (int t = (w) * 64; t < (w) * 64 + 64; ++t)
#define CHAIN_FIRST(w) ((w) == 0)
#else
#define CHAIN_THREADS(t, w) const int t = (int)threadIdx.x;
#define CHAIN_FIRST(w) (threadIdx.x == 0)
#endif

struct ChainView {               // chain c's slices
    hmc::Args a;
    float* image; float* params; float* ev;
    const float* slab; const double* lossp;
    double* sse;
    double* sh;                  // LDS: [2][4] per-wave energy sums
};

// the narrowed value of element i into the chain's weight image and parameter row: what k_pack / k_params make of th_eval32[i]
DEV void chain_scatter(int i, const ChainArgs& ca, const ChainView& v, double x) {
    const float xf = (float)x;
    const int q1 = ca.inv_ptr[i + 1];
    for (int q = ca.inv_ptr[i]; q < q1; ++q) v.image[ca.inv_pos[q] & 0xFFFFFF] = xf;
    if (i >= ca.p_off && i < ca.p_off + ca.ne) v.params[i - ca.p_off] = xf;
}
// element i of the evaluation's gradient: its slab entries in map order, one double accumulator, narrowed
DEV void chain_grad(int i, const ChainArgs& ca, const ChainView& v) {
    double s = 0.0;
    const int e1 = ca.row_ptr[i + 1];
    for (int e = ca.row_ptr[i]; e < e1; ++e) s += (double)v.slab[ca.row_ent[e]];
    v.ev[i] = (float)s;
}
// the update after an evaluation at the proposal
DEV void chain_step(const ChainArgs& ca, const ChainView& v, int w, double kick, double eps, int drift) {
    CHAIN_THREADS(t, w)
    for (int i = t; i < v.a.P; i += hmc::BLOCK) {
        chain_grad(i, ca, v);
        hmc::leap_body<float>(i, v.a, v.ev, kick, eps, drift);
        if (drift) chain_scatter(i, ca, v, v.a.th_prop[i]);
    }
}
// hmc::k_hmc_energy for the chain; ends behind a workgroup barrier with the scalars written by the first thread
DEV void chain_energy(const ChainArgs& ca, const ChainView& v, int w, int mode, int nterms_total) {
#ifdef PINN_EMU
    double q[2][64];
    for (int l = 0; l < 64; ++l) hmc::energy_partial(w * 64 + l, v.a, mode == 1, q[0][l], q[1][l]);
    for (int j = 0; j < 2; ++j) v.sh[j * 4 + w] = hmc::wave_butterfly(q[j]);
#else
    double kin, pri;
    hmc::energy_partial((int)threadIdx.x, v.a, mode == 1, kin, pri);
    for (int m = 32; m >= 1; m >>= 1) {
        kin += __shfl_xor(kin, m, 64);
        pri += __shfl_xor(pri, m, 64);
    }
    if ((threadIdx.x & 63) == 0) { v.sh[w] = kin; v.sh[4 + w] = pri; }
#endif
    wg_barrier();
    if (CHAIN_FIRST(w)) {
        double kin_ = v.sh[0], pri_ = v.sh[4];
        for (int j = 1; j < 4; ++j) { kin_ += v.sh[j]; pri_ += v.sh[4 + j]; }
        if (mode == 1)                                   // the K sums of squares: the four waves' partials in order (aux::reduce_direct_body)
            for (int k = 0; k < v.a.K; ++k) {
                double s = 0.0;
                for (int j = 0; j < 4; ++j) s += v.lossp[(size_t)j * nterms_total + k];
                v.sse[k] = s;
            }
        hmc::energy_finish(v.a, mode, kin_, pri_, v.sse);
    }
    wg_barrier();
}

// the wave program: chain `chain`, wave `w` of its workgroup
template <class S, int ACTK>
DEV void wave_hmc_chains(const GroupArgs& ga, const ChainArgs& ca, int chain, int w, float* lds) {
    ChainView v;
    v.a = ca.a;
    const size_t P = (size_t)ca.a.P, c = (size_t)chain;
    double* st = ca.state + c * (5 * P + hmc::SC_COUNT);
    v.a.th_cur = st; v.a.th_prop = st + P; v.a.r = st + 2 * P; v.a.g_cur = st + 3 * P; v.a.g_prop = st + 4 * P; v.a.sc = st + 5 * P;
    v.image = ca.packed + c * S::PACKED;
    v.params = ca.params + c * MAX_PARAMS;
    v.ev = ca.ev + c * P;
    v.slab = ga.slabs + c * S::SLAB;
    v.lossp = ga.losspart + c * 4 * (size_t)ga.nterms_total;
    v.sse = ca.sse + c * (size_t)ca.a.K;
    v.sh = reinterpret_cast<double*>(lds);
    const hmc::Args& a = v.a;
    auto eval = [&] {
        wg_barrier();                                    // the image and the parameter row are written
        wave_main<S, MODE_FUSED, ACTK>(ga, 0, 1, w, lds, chain);
        wg_barrier();                                    // the slab and the loss partials are written
    };
    if (ca.init) {
        { CHAIN_THREADS(t, w) {
            for (int i = t; i < a.P; i += hmc::BLOCK) {
                a.th_prop[i] = a.th_cur[i];
                chain_scatter(i, ca, v, a.th_cur[i]);
            }
            if (t >= ca.ne && t < ca.np) v.params[t] = ca.defaults[t];
        } }
        eval();
        chain_step(ca, v, w, 0.0, 0.0, 0);               // (gradient only)
        chain_energy(ca, v, w, 1, ga.nterms_total);
        { CHAIN_THREADS(t, w) {
            for (int i = t; i < a.P; i += hmc::BLOCK) a.g_cur[i] = a.g_prop[i];
            if (t == 0) a.sc[hmc::SC_LP_CUR] = a.sc[hmc::SC_LP_PROP];
        } }
        return;
    }
    const double eps = ca.eps;
    const double* uni = ca.uniforms ? ca.uniforms + c * (size_t)ca.ndraws : nullptr;
    double* smp = ca.samples + c * (size_t)ca.ndraws * P;
    double* acc = ca.accept_prob + c * (size_t)ca.ndraws;
    double* lp = ca.logp + c * (size_t)ca.ndraws;
    for (int d = 0; d < ca.ndraws; ++d) {
        const unsigned key = chain_key(ca.seed_lo, ca.seed_hi, ca.ctr0 + (unsigned)d, (unsigned)chain);
        const double* row = ca.momenta ? ca.momenta + (c * (size_t)ca.ndraws + (size_t)d) * P : nullptr;
        { CHAIN_THREADS(t, w)
            for (int i = t; i < a.P; i += hmc::BLOCK) hmc::momentum_body(i, a, nullptr, row, key); }
        chain_energy(ca, v, w, 0, ga.nterms_total);
        { CHAIN_THREADS(t, w)
            for (int i = t; i < a.P; i += hmc::BLOCK) {
                hmc::leap_body<float>(i, a, nullptr, 0.5 * eps, eps, 1);
                chain_scatter(i, ca, v, a.th_prop[i]);
            } }
        for (int s = 0; s < ca.n_leapfrog; ++s) {
            eval();
            const bool last = s == ca.n_leapfrog - 1;
            chain_step(ca, v, w, last ? 0.5 * eps : eps, eps, last ? 0 : 1);
        }
        chain_energy(ca, v, w, 1, ga.nterms_total);
        { CHAIN_THREADS(t, w)
            for (int i = t; i < a.P; i += hmc::BLOCK) hmc::accept_body(i, a, d, uni, key, smp, acc, lp); }
    }
}

}  // namespace pk
