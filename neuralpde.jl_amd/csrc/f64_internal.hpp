// f64_internal.hpp — what the units of the float64 evaluation mode share, and nobody else sees: f64.cpp (launch building, grouping, evaluation,
// the per-point closures, the device-entry adapters), f64_setup.cpp (state, kernel look-up, point sets and per-point data, the affine analysis),
// f64_stencil.cpp (the reference-semantics validation mode), f64_adam.cpp (the resident optimiser loop).  The interface of the mode to the rest
// of the library is the f64_* block of engine_types.hpp.
#pragma once
#include "resident.hpp"
#include "pinn_kernels6.hpp"

namespace pe {

// a term of the problem — or a PSEUDO-term built on the stack (a merged group, a network's trial function at caller-supplied points, a virtual
// network of a stencil): a pseudo-term BORROWS d_pts.  The type has no destructor and only f64_free releases the buffers of S.terms, so a
// borrowed pointer needs no clearing on the way out.
struct F64Term {
    const pk::F64Kernel* k = nullptr;
    const pk::F64MKernel* km = nullptr;  // the matrix-pipe kernels of the same jet set (family 4m), nullptr: one lane per point (family 4)
    std::vector<int> nets;               // networks the equation references, increasing
    std::vector<int> slot_net, slot_chan;      // per slot: index into `nets`, jet channel
    rp::Instr* d_prog = nullptr;
    double* d_imm = nullptr;
    int nops = 0, out_row = 0, nslots = 0;
    double* d_pts = nullptr;             // [n][d] double; converted from the float set unless pinn_set_points_f64 installed it
    int64_t cap = 0, n = 0;
    bool exact_pts = false;              // installed in double (not a conversion of the float set)
    int ndata = 0;                       // per-point DATA channels of the residual (OP_DATA), valid for the current point set only
    double* d_data = nullptr;            // [ndata][n]; converted from the float rows unless pinn_set_point_data_f64 installed them
    int64_t data_cap = 0, data_n = 0;
    // affine residual (r06, f64_affine): r = S(point) + sum_s a_s u_s — the matrix-pipe tile kernel then skips the tape interpreter (F64Sub::lin)
    bool lin = false;
    std::vector<double> lin_a;                           // [nslots]
    std::vector<std::pair<double, int>> lin_terms;       // S = lin_k + sum coef * (tape row that depends on coordinates / constants only)
    double lin_k = 0.0;
    double* d_lin = nullptr;             // [nslots | n]: coefficients, then S at the points of the current set
    int64_t lin_cap = 0, lin_n = 0;      // lin_n == n: S is valid for the installed set
};
// one (network, shift sequence) of a term's finite-difference stencils: the trial function of `net` at the term's points moved by the shifts in order
struct F64VNet { int net; std::vector<std::pair<int, double>> shifts; };
// the reference-semantics evaluation of one term (pinn_set_option(h, "derivative", "stencil"); pinn_kernels4.hpp: k_f64_stape)
struct F64Stencil {
    bool active = false;                 // the term has derivative slots (value-only terms evaluate as always: nothing to difference)
    std::vector<F64VNet> vnets;
    rp::Instr* d_prog = nullptr;         // stencil tape: the difference formulas, then the term's ops; rows [coordinates | params | vnets | ops]
    double* d_imm = nullptr;
    int nops = 0, out_row = 0;
};
struct F64State {
    std::vector<F64Term> terms;
    bool stencil = false;                // derivative slots by the reference's central differences instead of exact jets
    std::vector<F64Stencil> sten;
    double* d_uv = nullptr;              // [nv][n] values of the virtual networks
    double* d_seeds = nullptr;           // [nv][n][2 + ne]
    double* d_spts = nullptr;            // [nv][n][d] their shifted point sets
    size_t uv_cap = 0, seeds_cap = 0, spts_cap = 0;
    double* d_theta = nullptr;           // [P] parameters of the running EVALUATION (host-entry evaluations upload here; never the optimiser's iterate)
    double* d_opt_theta = nullptr;       // [P] the Adam loop's iterate (f64_adam_*): evaluations in between — adaptive reweighting, callbacks — leave it alone
    double* d_grad = nullptr;            // [P]
    double* d_sumsq = nullptr;           // [K]
    double* d_scratch = nullptr;
    size_t scratch_cap = 0;
    double* d_slab = nullptr;
    size_t slab_cap = 0;
    double* d_tpart = nullptr;           // matrix-pipe kernels: per-tile partial sums of the first / last layer entries (F64Args::tpart)
    size_t tpart_cap = 0;
    double* h_pin = nullptr;             // pinned host staging: [P] theta on its way in | [P + K] gradient and sums on their way out (one copy each way)
    double* d_m = nullptr;               // optimiser moments of the float64 Adam loop (f64_adam_*), allocated on first use
    double* d_v = nullptr;
    double* d_w_over_n = nullptr;        // [K] w_k / N_k of the running call
    double* d_hist = nullptr;
    size_t hist_cap = 0;
    bool opt_ready = false;              // d_opt_theta holds the optimiser's parameters
    double* d_aux_pts = nullptr;         // caller-supplied points of pinn_phi_f64 / pinn_derivative_f64 [n][d]
    double* d_aux_out = nullptr;         // per-point outputs (residuals, trial-function values / derivatives) [n]
    size_t aux_pts_cap = 0, aux_out_cap = 0;
    // MERGED launches of small problems (r06, f64_make_groups): terms that share networks, input binding and an instantiated jet set in ONE tile / dW /
    // reduction launch sequence; rebuilt when a term's point count changes or the merge switches flip
    struct Group { std::vector<int> terms, nets; std::map<int, std::vector<int>> inmap; const pk::F64Kernel* k = nullptr; const pk::F64MKernel* km = nullptr; std::vector<std::vector<int>> slot_chan; };
    std::vector<Group> groups;
    std::vector<int64_t> groups_sig;     // what the grouping was made for: the terms' point counts, then the merge switches (empty: not made yet)
    // what the last call launched, for pinn_get_option — kept here and nowhere else
    int path = 0;                        // kernels: bit 0 one lane per point (family 4), bit 1 matrix pipe (family 4m)                ("f64_path")
    int merged_launches = 0;             // merged launch sequences of the last EVALUATION                                            ("f64_merged")
    int max_chunks = 0;                  // the most launches one point set took (f64_buffers)                                        ("f64_chunks")
    void new_call() { path = 0; max_chunks = 0; }                             // a per-point closure (residuals, trial function)
    void new_evaluation() { new_call(); merged_launches = 0; }
    void ran(bool mfma) { path |= mfma ? 2 : 1; }
    void took(int64_t chunks) { max_chunks = std::max(max_chunks, (int)chunks); }
    void ran_merged() { ran(true); ++merged_launches; took(1); }
};
inline F64State& state(pinn_engine& E) { return *(F64State*)E.f64; }
inline const F64State& state(const pinn_engine& E) { return *(const F64State*)E.f64; }

// the A/B switches of the mode ($PINN_F64_*), read in ONE pass over the environment at every entry into the mode (f64_read_switches) and passed
// down: each takes effect at the next call on a live handle
struct F64Switches {
    bool no_mfma = false;                // one lane per point (family 4) where the matrix-pipe kernels would run
    bool no_sliced = false;              // kernel look-up passes over the channel-sliced matrix-pipe kernels (family 4s)
    bool no_merge = false;               // every term its own launch sequence
    bool no_lin = false;                 // affine residuals go through the tape interpreter
    bool no_short_blocks = false;        // 512-point blocks for the dW kernel of small launches too
    bool full_channels = false;          // every network carries the kernel's whole jet set (A/B, tests)
    double scratch_mb = 0.0;             // scratch budget of one launch in MB (>= 1); 0: the default of the kernel family
    int dwt_wgs = 512;                   // workgroups a short-block dW launch aims at (A/B knob)
};
F64Switches f64_read_switches();

// ---- one term (or pseudo-term) as the kernels see it ----
struct F64Launch {
    pk::F64Args a;
    int rows = 0;                        // scratch rows per point
    int acls = pk::ACLS_A;               // activation class of the term's networks (one per term: f64_enable)
    bool mfma = false;
    bool sliced = false;                 // family 4s: the tile kernel passes every layer through the scratch rows (needed in every mode)
    F64Switches sw;                      // the switches it was built under (f64_buffers, f64_short_blocks)
};

// the "first reduction writes or adds to the gradient" rule of an evaluation, and the only memset of the gradient.  The first reduction WRITES
// the gradient instead of adding to it when its term's entries cover all of theta (one network, or every network in the first equation);
// otherwise the gradient is zeroed once, in front of that reduction, and every reduction adds.  An evaluation whose launches all add (stencil
// mode: one seeded sequence per virtual network) zeroes up front.
struct GradStart {
    pinn_engine& E;
    double* grad;                        // nullptr: loss only
    bool started = false;
    void zero() {
        if (grad) plat_memset(grad, 0, sizeof(double) * E.ntheta, E.stream);
        started = true;
    }
    // called in front of a reduction over the entries of `nets`: 1 = that launch writes the gradient, 0 = it adds
    int first_reduction_writes(const std::vector<int>& nets) {
        if (!grad || started) return 0;
        int64_t covered = E.ne;
        for (int ni : nets) covered += E.nets[ni].nparams();
        if (covered == E.ntheta) { started = true; return 1; }
        zero();
        return 0;
    }
};

// ---- the one spelling of things several units need ----
inline bool f64_act_ok(int act) { return act == pk::ACT_TANH || act == pk::ACT_SIGMOID || act == pk::ACT_SIN || act == pk::ACT_MIXED || act == pk::ACT_SWISH; }
// a term's quadrature weights, when they belong to its current point set
inline const float* term_pw(const Term& T) { return (T.pw_n == T.n && T.pw_n > 0) ? T.d_pw : nullptr; }
// d (w_k L_k) / d (sum of squares) in double (engine.cpp's term_scale rounds the same expression to float: not shared)
inline double f64_term_scale(const Term& T, double w) { return 2.0 * w / (double)T.n_norm; }
// default values of the PDE parameters, zero-filled to MAX_PARAMS
inline void fill_pdef(const pinn_engine& E, double* pdef) {
    for (int j = 0; j < pk::MAX_PARAMS; ++j) pdef[j] = j < (int)E.p_defaults.size() ? E.p_defaults[j] : 0.0;
}
// which coordinate of a term feeds input i of `net`: the term's explicit map or the identity, padded to four entries; its length (the caller
// compares it with the network's input count where the map comes from outside)
inline int input_binding(const pinn_engine& E, int net, const std::map<int, std::vector<int>>* inmap, int* imap) {
    std::vector<int> m;
    if (inmap && inmap->count(net)) m = inmap->at(net);
    else for (int i = 0; i < E.nets[net].sizes[0]; ++i) m.push_back(i);
    for (int i = 0; i < 4; ++i) imap[i] = i < (int)m.size() ? m[i] : 0;
    return (int)m.size();
}
// the caller's float term weights (nullptr: ones) as the doubles the evaluation takes
inline std::vector<double> f64_widen_weights(const float* term_w, int K) {
    std::vector<double> w(K);
    for (int k = 0; k < K; ++k) w[k] = term_w ? (double)term_w[k] : 1.0;
    return w;
}

// f64_setup.cpp
const pk::F64Kernel* f64_find(int D, const std::vector<Slot>& slots, std::vector<int>& chan, std::string& why);
const pk::F64MKernel* f64_find_m(const pinn_engine& E, const pk::F64Kernel* k, const std::vector<int>& nets, const F64Switches& sw);
inline const double* f64_lin_ptr(const F64Term& F) { return (F.lin && F.lin_n == F.n && F.n > 0) ? F.d_lin : nullptr; }
// f64.cpp
int f64_build(pinn_engine& E, const F64Term& F, int dt, const std::map<int, std::vector<int>>* inmap, const F64Switches& sw, F64Launch& L);
int f64_buffers(pinn_engine& E, F64State& S, F64Launch& L, int64_t n, bool with_sums, int64_t& chunk_out);
void f64_launch_forward(const F64Term& F, F64Launch& L, plat_stream st);
void f64_launch_chunk(pinn_engine& E, F64State& S, const F64Term& F, F64Launch& L, double* grad, GradStart* gs, pk::F64ReduceArgs& r);
int f64_values(pinn_engine& E, F64State& S, const F64Term& F, F64Launch& L, int64_t n, double* d_out);
int f64_eval_device(pinn_engine& E, const double* theta, double* grad, double* sumsq, const double* term_w);
// f64_stencil.cpp
int f64_stencil_term(pinn_engine& E, const F64Switches& sw, int t, const double* theta, double* grad, double* sumsq_t, double w, int mode, double* d_resid);

// the launches of one point set of n points: buffers for a launch (f64_buffers picks the chunk), then launch() once per chunk with
// L.a.p0 / L.a.npts set.  Notes the kernel family and the chunk count for pinn_get_option
template <class Fn> int f64_for_chunks(pinn_engine& E, F64State& S, F64Launch& L, int64_t n, bool with_sums, Fn&& launch) {
    S.ran(L.mfma);
    int64_t chunk = 0;
    if (f64_buffers(E, S, L, n, with_sums, chunk)) return 1;
    S.took((n + chunk - 1) / chunk);
    for (int64_t p0 = 0; p0 < n; p0 += chunk) {
        L.a.p0 = (int)p0;
        L.a.npts = (int)std::min<int64_t>(chunk, n - p0);
        launch();
    }
    return 0;
}
// a reduction that sums into ONE term's sum of squares (r.sumsq[0]; a merged launch widens nsq / sq_off to its members); `init`: it writes
// the sums instead of adding to them
inline pk::F64ReduceArgs f64_reduce_into(double* sumsq_t, bool init) {
    pk::F64ReduceArgs r;
    std::memset(&r, 0, sizeof r);
    r.sumsq = sumsq_t; r.nsq = 1; r.sq_off[0] = 0; r.init_sumsq = init ? 1 : 0;
    return r;
}

}  // namespace pe
