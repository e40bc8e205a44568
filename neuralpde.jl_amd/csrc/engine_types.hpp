// engine_types.hpp — data model of the host side of the C ABI, shared by descriptor.cpp (parsing), program.cpp (residual-program
// passes), plan.cpp (kernel selection, buffers, reduction maps), engine.cpp (evaluation + the extern "C" entry points) and the resident
// solvers' units (adam.cpp, hmc.cpp, lbfgs.cpp, ensemble.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pinn_hip.h"
#include "aux_limits.hpp"
#include "int_limits.hpp"
#include "plat.hpp"
#include "spec_registry.hpp"

namespace pe {

constexpr int REDUCE_SPLIT = 32;     // stage-1 chunks of the fixed-order slab reduction

extern thread_local std::string g_err;      // message of the last failed call on this thread (pinn_last_error)
int fail(const std::string& m);             // records the message, returns 1

constexpr int MAX_DERIV_ORDER = 6;
struct Slot {
    int net;
    int order;
    int axes[MAX_DERIV_ORDER];       // sorted; order <= 2 may be mixed in the fixed channel categories, anything else rides a general set
    unsigned lap = 0;        // != 0: the sum of the pure second derivatives over these axes (one "forward Laplacian" jet channel)
};
struct Net {
    int act;                         // ACT_TANH / ACT_SIGMOID / ACT_SIN / ACT_SWISH on every hidden layer, or ACT_MIXED with
    int act_layers = 0;              //   the kind of hidden layer l (tanh / sigmoid) in bits 4l .. 4l+3
    int theta_off;
    std::vector<int> sizes;          // n0 .. nL (nL == 1); DGM: {d, modes, 1}
    int kind = 0;                    // 0: Chain of Dense layers; 1: the reference's DGM architecture (src/dgm.jl:97-115)
    int dgm_layers = 0;              // DGM: number of gated (LSTM-type) layers
    int act2 = 0;                    // DGM: activation of the H gate (activation2); `act` is activation1
    // periodic input embedding in front of the chain (Boltz.Layers.PeriodicEmbedding(idxs, periods), reference test
    // test/CUDA/nnpde_cuda__1d_pde_dirichlet_bc_cuda.jl:26,48): inputs emb_idx[k] (0-based) leave the input list and come back at its end
    // as sin(2 pi x / period) for all k, then cos(2 pi x / period) for all k; sizes[0] counts the FEATURES the first Dense layer takes
    std::vector<int> emb_idx;
    std::vector<double> emb_period;
    int n_inputs() const { return sizes[0] - (int)emb_idx.size(); }       // arguments of the dependent variable
    // the features [n][sizes[0]] the first Dense layer takes at n points of the arguments x [n][n_inputs()]: pass-through arguments, then sin,
    // then cos of the embedded ones — phases and sin / cos in double, narrowed to T only at the store
    template <class T> std::vector<T> features(const T* x, int64_t n) const {
        const int nin = n_inputs(), ne = (int)emb_idx.size(), F = sizes[0];
        std::vector<T> f((size_t)n * F);
        for (int64_t q = 0; q < n; ++q) {
            int pass = 0;
            for (int a = 0; a < nin; ++a) {
                const double xa = x[(size_t)q * nin + a];
                const auto it = std::find(emb_idx.begin(), emb_idx.end(), a);
                if (it == emb_idx.end()) { f[(size_t)q * F + pass++] = (T)xa; continue; }
                const int k = (int)(it - emb_idx.begin());
                const double ph = 6.283185307179586476925286766559 / emb_period[k] * xa;
                f[(size_t)q * F + nin - ne + k] = (T)std::sin(ph);
                f[(size_t)q * F + nin + k] = (T)std::cos(ph);
            }
        }
        return f;
    }
    int nparams() const {
        if (kind == 1) { const int d = sizes[0], M = sizes[1]; return M * d + M + dgm_layers * (4 * M * d + 4 * M * M + 4 * M) + M + 1; }
        int n = 0;
        for (size_t i = 0; i + 1 < sizes.size(); ++i) n += sizes[i + 1] * sizes[i] + sizes[i + 1];
        return n;
    }
    int maxhidden() const {
        int m = 0;
        for (size_t i = 1; i + 1 < sizes.size(); ++i) m = std::max(m, sizes[i]);
        return m;
    }
};
struct LinearForm { float k = 0.f; float a[pk::LIN_MAX_C] = {}; float b[pk::LIN_MAX_SRC] = {}; };
struct EmbCol { int src; double omega; int is_cos; };      // device coordinate row = sin / cos (omega x coordinate `src`)
// one integral node of a term (descriptor `integral` block): I(x) = int_lo^hi f(s) ds over coordinate `var`, f a tape of its own over
// rows [coordinates (row `var` = the quadrature node) | params | its slots | ops]; its slots are Term::slots[slot0, slot0 + nslots)
struct IntNode {
    int var = 0;
    int lo_row = -1, hi_row = -1;    // >= 0: the bound is that coordinate of the collocation point
    double lo = 0.0, hi = 0.0;       // otherwise the constant
    int slot0 = 0, nslots = 0;
    std::vector<rp::Instr> ops;
    int out_row = 0;
};
struct Term {
    // integral terms: rows [d+np+n_outer, d+np+n_outer+inodes.size()) of the tape are the integral nodes; `slots` holds
    // the outer slots first, then every node's.  The device point buffer d_pts is the term's SITE SET [sites()][n][d]: block 0 the
    // collocation points as installed, block 1 + k Q + q the points with node k's variable moved to quadrature node q
    // (aux::k_int_sites whenever the point set changes)
    std::vector<IntNode> inodes;
    int n_outer = 0;                 // outer slots (== slots.size() without integral nodes)
    int int_q = 0;                   // Gauss-Legendre nodes per integral node (handle option "integral_nodes")
    rp::Instr* d_int_prog = nullptr; // the nodes' tapes, node after node
    int sites() const { return 1 + (int)inodes.size() * int_q; }      // evaluations of the network(s) per collocation point
    int tape_row0(int np) const { return d + np + (inodes.empty() ? (int)slots.size() : n_outer + (int)inodes.size()); }      // first op row
    int d = 0;                       // coordinate rows of the device point set (embedded terms: d_user rows + emb_cols)
    int d_user = 0;                  // coordinates per point at the C ABI (pinn_set_points, samplers, pinn_get_points); == d without embeddings
    std::vector<EmbCol> emb_cols;    // rows d_user .. d-1, written by aux::k_embed whenever the point set changes (descriptor.cpp: apply_embeddings)
    float* d_upts = nullptr;         // embedded terms: the point set as installed, [n][d_user]; otherwise unused (d_pts is the set)
    EmbCol* d_emb_cols = nullptr;
    bool linear = false;             // the fused tape is affine in the jet channels / sources (plan.cpp: detect_linear)
    LinearForm lin;
    std::vector<Slot> slots;
    std::vector<rp::Instr> ops;      // descriptor row numbering
    std::vector<double> imm64;       // the ops' immediates as the descriptor spelled them (Instr::imm is a float): the float64 evaluation mode reads these
    int out_row = 0;
    // plan
    int net = -1;
    int group = -1;
    int slot_in_group = -1;
    int coupled = -1;                // >= 0: index into pinn_engine::coupled (equation couples several networks)
    std::vector<int> chan_of_slot;
    // per referenced network: which of the term's coordinates feed the network's inputs (descriptor `inmap` lines; default
    // identity) — dependent variables of one system may take different arguments (src/discretize.jl:111-131)
    std::map<int, std::vector<int>> inmap;
    // coordinate-only subexpressions hoisted out of the fused tape (analyse_static): evaluated by k_src per point set
    std::vector<rp::Instr> src_prog;     // compact numbering: rows [0,d) coordinates, row d+i = static op i
    std::vector<int> src_root;           // compact row of source j
    std::vector<int> src_of_op;          // per descriptor op: source index, or -1
    std::vector<int> tape_ops;           // descriptor ops that stay in the fused tape, in order
    rp::Instr* d_src_prog = nullptr;
    float* d_src = nullptr;              // [nsrc][n]
    int64_t src_cap = 0;
    // user-supplied per-point data channels (OP_DATA; pinn_set_point_data), valid for the current point set only
    int ndata = 0;
    float* d_data = nullptr;
    int64_t data_n = 0, data_cap = 0;
    // optional quadrature weights of the current point set, stored as sqrt(n_norm * w_i) (pinn_set_point_weights)
    float* d_pw = nullptr;
    int64_t pw_n = 0, pw_cap = 0;
    // data
    float* d_pts = nullptr;
    long long hint_n = 0;            // descriptor `hint`: points the caller expects to install (0: unknown)
    int64_t pts_cap = 0;             // points d_pts has room for (grows, never shrinks: resampled sets of varying size reuse it)
    int64_t n = 0, n_norm = 0;
    float* d_resid = nullptr;
    int64_t resid_cap = 0;
    // on-device sampler: kind 0 = fixed set, 1 = uniform (StochasticTraining), 2 = Latin hypercube (QuasiRandomTraining default),
    // redrawn before every training step
    int sampler = 0;
    float* d_lb = nullptr;
    float* d_ub = nullptr;
    unsigned seed = 0, draws = 0;
};
struct Group {
    int kind = 0;                    // 0: fused (single-network terms); 1: per-network FWD/GRADIN launches of coupled terms;
                                     // 2: TAIL network of a coupled term: forward + residual tape + reverse in one launch (Coupled::tail)
    int net = -1;
    const pk::SpecInfo* spec = nullptr;
    std::vector<int> terms;
    pk::GroupArgs ga;
    rp::Instr* d_prog = nullptr;
    std::vector<int> prog_off, prog_n, out_row;
    float* d_slabs = nullptr;
    double* d_losspart = nullptr;
    float* d_scratch = nullptr;
    size_t scratch_cap = 0;          // family 3: floats allocated (rows x padded points; grows with the point sets)
    float* d_rec = nullptr;          // kind 1, family 2: per-tile records of the forward launch, read back by the reverse launch
    size_t rec_slots = 0;            // (instead of running the forward pass twice; falls back to recomputation above REC_BUDGET)
    bool use_rec = false;
    double* d_tmp = nullptr;         // stage-1 partial sums [nsplit][nent + K]
    std::vector<int> row_theta, row_ptr, row_off;   // host CSR: theta element -> slab offsets of this group
    int* d_ent_theta = nullptr;      // inverse map slab entry -> theta element (-1: none) when every theta element this group feeds has exactly
                                     // one slab entry (families 2, 3): input of the one-kernel reduction (aux::k_reduce_one)
    bool ent_covers_theta = false;   // ... and the group feeds EVERY theta element (single-network problems)
    int nent = 0;
    int slab_floats = 0;             // floats per block of d_slabs
    int blocks = 0;
    int max_blocks = 0;
    bool active = false;
    int chain_to = -1;               // earlier launch group of the same network whose slab set this group may accumulate into
    int merged = -1;                 // >= 0: index into pinn_engine::merged — this group's tiles can ride in ONE launch with another group's
    int launched_blocks = 0;         // workgroups of the launch that carried this group's tiles in the current evaluation
    int launched_by = -1;            // launch group whose launch carried them (itself, or the head of a merged launch)
    plat_event ev_a, ev_b;
    bool timed = false;
};
// an equation that couples several networks (systems of PDEs, src/discretize.jl:58-80): forward launch per network ->
// k_expr (tape over all networks' jets) -> reverse launch per network
struct Coupled {
    int term = -1;
    std::vector<int> nets;           // networks referenced, increasing
    std::vector<int> groups;         // per network: the kind-1 group that runs it
    std::vector<int> slot_net;       // per slot: index into `nets`
    std::vector<float*> d_jets, d_ubar;   // per network: [C_n][N]
    // TAIL launch (r04): the network with the widest channel set of the equation (family 2) runs forward + tape + reverse in ONE launch
    // (kind-2 group, MODE_FUSED): the other networks' jets — written by their forward launches into ONE array, network after network —
    // are its tape's source rows, and it writes their seeds.  No k_expr launch, and the tail network's records never go through HBM.
    // -1: every network takes the forward / k_expr / reverse path (narrow nets, tapes beyond 32 rows, DATA channels, PINN_NO_TAIL_FUSE=1)
    int tail = -1;                   // index into `nets` / `groups`
    std::vector<int> src_off;        // per network: first source row of its kernel's channels (tail: -1)
    int nsrc = 0;                    // source rows = sum of the other kernels' channel counts
    float* d_jets_all = nullptr;     // [nsrc][cap]; d_jets[i] / d_ubar[i] of the other networks point into these (rows packed with stride n)
    float* d_ubar_all = nullptr;
    int64_t cap = 0;
    rp::Instr* d_prog = nullptr;
    double* d_losspart = nullptr;    // pseudo-group for the reduction: [blocks*4][K]
    float* d_pslab = nullptr;        // [blocks][16]
    double* d_tmp = nullptr;
    int blocks = 0, cap_blocks = 0;
    std::vector<int> row_theta, row_ptr, row_off;
};
// two fused launch groups of one network (same shape, slab layout and reduce rows; e.g. interior jet set + value-only boundary set) for
// which a merged kernel exists (pk::PairInfo): one persistent launch walks the head's tiles, then the tail's, with the weight-gradient
// accumulators in registers across both (plan.cpp: plan_merge_groups; engine.cpp: run_loss_grad)
struct MergedUnit {
    int head = -1, tail = -1;
    const pk::PairInfo* pair = nullptr;
    float* d_scratch = nullptr;      // record scratch of the merged launch: max_blocks x pair->SCR
    double* d_losspart = nullptr;    // per-wave loss partials of the merged launch [max_blocks * NW][K] (both groups' terms)
    int max_blocks = 0;
};
struct NetPlan {
    const pk::SpecInfo* spec = nullptr;   // any spec with the right (HP,NHH,D): packed layout is shared
    float* d_packed = nullptr;
    int* d_pack_idx = nullptr;
    const float* cur = nullptr;      // weights the kernels read in the current evaluation: d_packed (DGM kernels: theta + theta_off)
    std::vector<int> h_pack_idx;     // host copy (inverse map construction)
    int npacked = 0;
};
struct HmcState;                     // hmc.cpp
struct LbfgsState;                   // lbfgs.cpp
struct BfgsState;                    // bfgs.cpp
struct EnsState;                     // ensemble.cpp
struct CubState;                     // cubature.cpp

}  // namespace pe

using pe::Coupled; using pe::Group; using pe::MergedUnit; using pe::Net; using pe::NetPlan; using pe::Slot; using pe::Term;

struct pinn_engine {
    int64_t ntheta = 0;
    int np = 0, ne = 0, p_theta_off = 0;
    std::vector<double> p_defaults;  // values of the PDE parameters that are not estimated, as the descriptor states them (the float64 mode reads these)
    std::vector<float> p_defaults32; // the same decimals rounded to float: what d_defaults uploads for the fp32 kernels
    std::vector<Net> nets;
    std::vector<Term> terms;
    std::vector<Term> terms0;        // the terms as parsed, before the planner's rewrites (Laplacian fusion, source hoisting): what the float64 mode evaluates
    void* f64 = nullptr;             // pe::F64State: the float64 evaluation mode (pinn_set_option "precision"), nullptr = off
    std::vector<Group> groups;
    std::vector<Coupled> coupled;
    std::vector<MergedUnit> merged;
    std::vector<NetPlan> netplans;
    int ncu = 0;
    int gemm = pk::GEMM_SPLIT;       // GEMM arithmetic of the neuron-split kernels of this handle (pinn_set_option "gemm"; $PINN_GEMM at pinn_create)
    bool gemm_auto = false;          // pinn_set_option(h, "gemm", "auto"): the engine picks split / fp32 from the gradient-health figure below
    double grad_health = -1.0;       // rho = |grad sum_k w_k L_k|_2 / sqrt(sum_k w_k L_k) of the last evaluation that measured it (-1: none yet)
    double gemm_delta = -1.0;        // last measured |grad(split) - grad(fp32)|_2 / |grad(fp32)|_2 at one theta (-1: none yet)
    long long gemm_check_t = -1;     // optimiser step / evaluation count of the last such comparison
    long long eval_count = 0;        // host-entry evaluations with a gradient (the "clock" of the policy outside the resident loop)
    int device = 0;                  // the HIP device this handle lives on (pinn_create: the caller's current device; pinn_create_on)
    // engine-owned data-parallel collective (comm.cpp): communicator of this handle's rank, nullptr = single device
    void* comm = nullptr;
    int comm_size = 1, comm_rank = 0;
    bool comm_per_process = false;   // the other ranks live in other processes (pinn_comm_init_rank / _custom): this handle's own calls carry the collective
    pinn_allreduce_fn comm_fn = nullptr;     // caller-supplied transport (pinn_comm_init_custom) instead of RCCL
    void* comm_ctx = nullptr;
    plat_stream stream = nullptr;
    bool own_stream = true;
    float* d_theta = nullptr;
    float* d_params = nullptr;
    float* d_defaults = nullptr;
    double* d_lossraw = nullptr;
    int* d_gr_ptr = nullptr;         // global reduce CSR over theta: contributions (group, entry)
    int* d_gr_grp = nullptr;
    int* d_gr_ent = nullptr;
    int* d_red_perm = nullptr;       // [P + K] thread order of the one-stage reduction (aux::Reduce2Args::perm)
    float* d_out = nullptr;          // [P grad | K raw sums]
    // pinned host block of the host entry points: [P floats theta | P + K floats out | K doubles raw sums]
    float* hp_theta = nullptr;
    float* hp_out = nullptr;
    double* hp_raw = nullptr;
    plat_event ev0, ev1, ev2, ev3;
    plat_stream aux_stream[2] = {nullptr, nullptr};     // under-filled launch groups run concurrently (fork/join by events)
    plat_event ev_fork, ev_join[aux::MAX_GROUPS];
    float last_kernel_ms = 0.f, last_total_ms = 0.f;
    bool timing_valid = false;
    int timing_level = 0;        // 0 (default since r04): no events, 1: per-launch-group kernel events, 2: + phase events (pinn_last_timing)
    int timing_group = -1;       // level >= 1: which launch group gets events (-1: all)
    // resident fp32 Adam (adam.cpp; pinn_adam_*).  The optimiser state lives from pinn_adam_init to pinn_destroy and survives a re-plan; the
    // inverse pack map and the contribution counts belong to the kernel plan (plan.cpp builds them, free_plan releases the map); everything
    // from d_c12 down is the persistent training kernel's (pinn_train.hpp), allocated at its first launch and kept to pinn_destroy (free_plan
    // only marks the thread map stale: own_blocks = 0)
    float* d_opt_theta = nullptr;
    float* d_opt_m = nullptr;
    float* d_opt_v = nullptr;
    float* d_opt_out = nullptr;      // [P + K] the step's [gradient | raw sums]
    float* d_w_over_n = nullptr;     // [K] term weight / n_norm of the current call
    double* d_hist = nullptr;        // loss history of the current call
    size_t hist_cap = 0;
    long long opt_t = 0;             // steps taken since pinn_adam_init
    int adam_path = 0;               // what the last pinn_adam_steps call ran: 0 nothing yet, 1 the stand-alone loop, 2 the persistent kernel
    int* d_inv_ptr = nullptr;        // theta element -> positions (net << 24 | offset) in the packed weight images: the update kernels write
    int* d_inv_pos = nullptr;        // the new parameters straight into the images
    bool inv_ok = false;
    int max_contrib = 0, max_inv_pos = 0;      // most slab entries / image positions of one theta element (plan.cpp)
    bool persistent = true;          // pinn_set_option "persistent": small problems run pinn_adam_steps inside one launch
    float* d_c12 = nullptr;          // bias-correction table [2 x steps] of a persistent launch
    size_t c12_cap = 0;              // floats
    unsigned* d_bar = nullptr;       // grid-barrier words of the persistent training kernel (pinn_train.hpp)
    unsigned* h_flag = nullptr;      // host-mapped: a launch's barrier timed out
    unsigned bar_arrivals = 0;       // arrivals the barrier counter has seen so far (it is never reset between launches)
    float* d_sums2 = nullptr;        // its [2][K] per-step sums
    int* d_own_r = nullptr;          // its thread -> element map (pinn_train.hpp: TrainArgs::own_r), built for own_blocks workgroups
    int own_blocks = 0, hist_gid = 0;
    void* d_train_samp = nullptr;    // its table of redrawn terms (pk::TrainSampler[train_samp_cap])
    size_t train_samp_cap = 0;       // bytes
    float* d_opt_bak = nullptr;      // [3 P] snapshot of (theta, m, v) at the start of a persistent launch (restored when its barrier times out)
    int eval_path = 0;              // what the last host-entry loss + gradient evaluation ran: 1 the stand-alone kernels, 2 one launch (eval_fused)
    int int_q = 16;                  // pinn_set_option "integral_nodes": Gauss-Legendre nodes per integral node (2..64)
    double* d_int_xi = nullptr;      // [int_q] nodes on [-1, 1] (double) and
    float* d_int_w = nullptr;        // [int_q] weights of the rule, computed in double on the host
    // phi scratch
    float* d_phi_pts = nullptr;
    float* d_phi_out = nullptr;
    float* d_phi_scr = nullptr;      // family 3: scratch rows of a pinn_phi / pinn_derivative call
    size_t phi_scr_cap = 0;
    int64_t phi_cap = 0;
    int phi_chan = 0;                // jet channels d_phi_out holds per point
    pe::HmcState* hmc = nullptr;     // resident HMC sampler state (hmc.cpp; pinn_hmc_init), nullptr = none
    pe::LbfgsState* lbfgs = nullptr; // resident L-BFGS state (lbfgs.cpp; pinn_lbfgs_init), nullptr = none
    int lbfgs_history = 0;           // its history length (pinn_describe)
    int nuts_chunk = 8;              // option "nuts_chunk": slots pinn_nuts_draws queues between two downloads of its control block, 1..64
    int lbfgs_chunk = 8;             // option "lbfgs_chunk": slots pinn_lbfgs_steps / pinn_bfgs_steps queue between two downloads of the control block, 1..64
    pe::BfgsState* bfgs = nullptr;   // resident dense BFGS state (bfgs.cpp; pinn_bfgs_init), nullptr = none
    pe::EnsState* ens = nullptr;     // buffers of pinn_phi_ensemble (ensemble.cpp), nullptr = none yet
    pe::CubState* cub = nullptr;     // region lists of pinn_cubature_refine (cubature.cpp), nullptr = none yet
};

namespace pe {
// descriptor.cpp
int parse_descriptor(const char* text, pinn_engine& E);
int apply_embeddings(pinn_engine& E);
// sexpr.cpp: the symbolic front end ("pinnir 2"): lhs / rhs of an equation as prefix s-expressions -> jet slots + tape
struct SexprContext {
    std::vector<std::string> params;                         // PDE parameter names, in theta.p order
    std::vector<std::string> depvars;                        // dependent-variable name of net i
    std::vector<std::vector<std::string>> depvar_inputs;     // its argument names (dict_depvar_input)
};
int lower_sexpr_term(const SexprContext& C, const std::vector<std::string>& indvars, const std::string& lhs, const std::string& rhs,
                     int np, Term& T);
// program.cpp
void analyse_static(Term& T, int np);
bool fuse_laplacian(Term& T, int np);
// engine.cpp (shared with comm.cpp, adam.cpp and the resident solvers' units)
// One fp32 evaluation, as its caller asks for it: a call site fills the fields it means and leaves the rest at their defaults.
struct EvalRequest {
    const float* d_theta = nullptr;  // parameters in device memory (nullptr: E.d_theta)
    float* d_out = nullptr;          // [P gradient | K sums] in device-visible memory (loss_only: [0, P) is left untouched)
    const float* term_w = nullptr;   // host, K term weights (nullptr: all 1)
    int only_term = -1;              // >= 0: this term alone, the others with scale 0 (pinn_term_grads)
    bool timing = false;             // record the events the handle's timing level asks for
    double* lossraw = nullptr;       // K exact double sums (nullptr: E.d_lossraw)
    bool packed_fresh = false;       // the optimiser's update kernel has already written the fp32 weight images
    bool loss_only = false;          // MODE_LOSS launches, no reverse sweep, only the K sums are reduced
    float* d_sums = nullptr;         // the K float sums (nullptr: d_out + P)
    // parameters and results in device memory
    static EvalRequest device(const float* d_theta, float* d_out, const float* term_w) {
        EvalRequest rq;
        rq.d_theta = d_theta; rq.d_out = d_out; rq.term_w = term_w;
        return rq;
    }
    // a host entry point: the uploaded parameters, results straight into the handle's pinned block
    static EvalRequest host_entry(const pinn_engine& E, const float* term_w) {
        EvalRequest rq = device(E.d_theta, E.hp_out, term_w);
        rq.lossraw = E.hp_raw;
        return rq;
    }
};
int run_loss_grad(pinn_engine& E, const EvalRequest& rq);
int upload_theta(pinn_engine& E, const float* theta, int64_t p);
void sums_from_double(float* d_out_sums, const double* d_raw, int K, plat_stream st);      // (float)raw[k] -> out_sums[k], on the stream
int ensure_points(pinn_engine& E);              // every term has its point set (and per-point data) installed, or the reason in g_err
// the steps of pinn_set_points / pinn_set_point_weights / pinn_residual around their copies, for a unit whose kernels write a term's points and
// weight factors on the device (cubature.cpp): room for n points; the bookkeeping after n points were written (sources, tile tables; per-point
// data and weights of the previous set are dropped); room for n weight factors; the bookkeeping after they were written (n == 0: none); the
// term's residual at its installed set into Term::d_resid with the uploaded, packed parameters — queued, nothing downloaded
int points_reserve(pinn_engine& E, int term, int64_t n);
int points_written(pinn_engine& E, int term, int64_t n, int64_t n_norm);
int weights_reserve(pinn_engine& E, int term, int64_t n);
void weights_written(pinn_engine& E, int term, int64_t n);
int residual_device(pinn_engine& E, int term);
// loss + gradient for a host entry point that synchronises right after: small problems in ONE launch (eval_fused), everything else by
// run_loss_grad; results in d_out / lossraw either way.  Synchronises.
int eval_and_sync(pinn_engine& E, float* d_out, const float* term_w, double* lossraw, bool timing);
// switch the GEMM arithmetic of a live handle: the kernel plan is rebuilt for the other mode (packed weight images, gradient-slab maps and
// reduction tables differ), the installed point sets, samplers, per-point data / weights and the optimiser state stay
int replan_gemm(pinn_engine& E, int mode);
// the weights every network's kernels read in the next evaluation: the packed images rebuilt from d_theta (nullptr: E.d_theta) by k_pack;
// packed_fresh: the optimiser's update kernel has written the fp32 images already
void pack_all(pinn_engine& E, const float* d_theta = nullptr, bool packed_fresh = false);
// seed of a term's device sampler on this rank: ranks of a communicator draw different points (their shards of one global draw)
inline unsigned sampler_seed(const pinn_engine& E, const Term& T) {
    return E.comm_size > 1 ? T.seed + 0x85EBCA6BU * (unsigned)(E.comm_rank + 1) : T.seed;
}
// one redraw of a sampled term's float point set on the handle's stream: the draw with the rank's seed (the draw counter advances), the
// embedding rows, and with `sources` the term's coordinate-only source channels.  The float64 optimiser loop passes false: its kernels
// read the widened copy (f64_points_from_device) and not the float source rows
void redraw_term(pinn_engine& E, Term& T, bool sources);
// "gemm" = "auto" (engine.cpp): the gradient-health figure of a host copy of [gradient | raw sums], and the policy's check at d_theta
void measure_grad_health(pinn_engine& E, const float* grad_and_sums, const float* term_w);
int gemm_auto_check(pinn_engine& E, const float* d_theta, const float* term_w, long long now);
// adam.cpp: loss + gradient of a small problem in ONE launch of the persistent kernel (its eval_only form), synchronised.  0: done, results
// in d_out / lossraw; 1: failed (g_err); 2: the handle does not qualify, or the launch's grid barrier timed out — the caller takes the
// stand-alone kernels
int eval_one_launch(pinn_engine& E, float* d_out, const float* term_w, double* lossraw);
inline int check_theta(const pinn_engine& E, const char* who, int64_t p) {
    return p == E.ntheta ? 0 : fail(std::string(who) + ": theta length " + std::to_string(p) + " != ntheta " + std::to_string(E.ntheta));
}
// one caller array of n elements of type T, seen as element type V at the precision boundary of a float / double entry point: the caller's
// own array when T is V; otherwise a converted copy — of the caller's values for an input (T const), or one that put() converts back into
// the caller's array for an output.  A null array stays null.
template <class V, class T> class As {
    static constexpr bool same = std::is_same_v<V, std::remove_const_t<T>>;
    T* x_;
    std::vector<V> copy_;
public:
    As(T* x, size_t n) : x_(x) {
        if constexpr (!same) {
            if (x && std::is_const_v<T>) copy_.assign(x, x + n);      // an input: the caller's values, converted
            else if (x) copy_.resize(n);                               // an output: written by the evaluation, converted back by put()
        }
    }
    auto get() {
        if constexpr (same) return x_;
        else return x_ ? copy_.data() : nullptr;
    }
    int put() {                                          // (outputs; returns 0)
        if constexpr (!same) if (x_) std::copy(copy_.begin(), copy_.end(), x_);
        return 0;
    }
};
template <class V, class T> As<V, T> as(T* x, size_t n) { return As<V, T>(x, n); }
// hmc.cpp, lbfgs.cpp, bfgs.cpp, ensemble.cpp: release the handle's resident solver state / ensemble buffers (nothing to do when there is none)
void hmc_free(pinn_engine& E);
void lbfgs_free(pinn_engine& E);
void bfgs_free(pinn_engine& E);
int bfgs_params(const pinn_engine& E);          // P of the resident BFGS state (pinn_describe), 0 = none
void ens_free(pinn_engine& E);
void cub_free(pinn_engine& E);
const float* cub_phase_ms(const pinn_engine& E);      // cubature.cpp: [6] phase times of the last pinn_cubature_refine at timing level 2 (zeros otherwise)
// ensemble.cpp: of the last pinn_derivative_ensemble call — 0: jet passes, 1: point passes, 2: jet passes on the scratch storage (0 before any call)
int ens_counter(const pinn_engine& E, int which);
// comm.cpp: sum vec[i] ([P + K] floats) and raw[i] (K doubles) of the ndev handles' ranks over their communicator, in place, each on its
// handle's stream.  ndev == 1: a one-process-per-GPU communicator (RCCL or the caller's transport; no communicator: nothing to do);
// ndev > 1: the handles of one pinn_comm_init_all communicator, one grouped RCCL call
int comm_all_reduce(pinn_engine** es, int ndev, float** vec, double** raw);
int comm_all_reduce_f64(pinn_engine** es, int ndev, double** vec, int64_t count);       // `count` doubles per rank, in place (float64 mode)
// every entry point that touches the device first makes the handle's device current (single-process multi-GPU callers)
struct DeviceScope {
    int prev;
    explicit DeviceScope(int dev) : prev(plat_get_device()) { if (prev != dev) plat_set_device(dev); else prev = -1; }
    ~DeviceScope() { if (prev >= 0) plat_set_device(prev); }
};
// an entry point that evaluates on a caller's stream: the handle's work goes there for the duration (NULL is the legacy default stream —
// e.g. torch's current stream), the handle's own stream is back on every way out
struct StreamScope {
    pinn_engine& E;
    plat_stream saved;
    StreamScope(pinn_engine& E_, void* stream) : E(E_), saved(E_.stream) { E.stream = (plat_stream)stream; }
    ~StreamScope() { E.stream = saved; }
    StreamScope(const StreamScope&) = delete;
    StreamScope& operator=(const StreamScope&) = delete;
};
// f64.cpp (evaluation), f64_setup.cpp, f64_stencil.cpp, f64_adam.cpp: the float64 evaluation mode (pinn_kernels4.hpp); what those units share
// among themselves is f64_internal.hpp
int f64_enable(pinn_engine& E);
void f64_destroy(pinn_engine& E);
std::string f64_describe(const pinn_engine& E);
int f64_affine_terms(const pinn_engine& E);      // terms whose residual the matrix-pipe tile kernel evaluates in affine form, without the tape interpreter
int f64_chunks(const pinn_engine& E);            // the most launches (scratch-sized chunks) one point set took in the last float64 call: 1 = none chunked
int f64_merged(const pinn_engine& E);            // merged launch sequences of the last float64 evaluation (small problems: f64.cpp f64_make_groups)
const char* f64_path(const pinn_engine& E);      // kernels of the last float64 evaluation: "mfma" | "lanes" | "mfma+lanes" | "none" | "off"
int f64_points_changed(pinn_engine& E, int term);
int f64_set_points(pinn_engine& E, int term, const double* pts, int64_t n);
int f64_set_point_data(pinn_engine& E, int term, const double* data);      // nullptr: convert the float rows just installed
int f64_eval(pinn_engine& E, const double* theta, const double* term_w, double* term_losses, double* grad);
int f64_residual(pinn_engine& E, int term, const double* theta, double* r);      // host theta, host r[n_term]
// the same in pieces, for kernels that write a term's double point set on the device (cubature.cpp): the evaluation's parameters; room for n points
// (the buffer); the bookkeeping after n points were written; the residual at the installed set, queued, *d_r the device array it lands in
int f64_upload_theta(pinn_engine& E, const double* theta);
double* f64_points_reserve(pinn_engine& E, int term, int64_t n);
int f64_points_written(pinn_engine& E, int term, int64_t n);
int f64_residual_device(pinn_engine& E, int term, const double** d_r);
int f64_net_eval(pinn_engine& E, int net, const double* theta, const double* pts, int64_t n, int order, const int* axes, double* out);      // d^order phi_net / dx_axes at host points
int f64_adam_apply(pinn_engine& E, const double* grad_and_sums, double lr, double beta1, double beta2, double eps, const float* term_w, double* loss);
int f64_stencil_enable(pinn_engine& E, bool on);      // pinn_set_option "derivative" = "stencil" | "exact"
bool f64_stencil_on(const pinn_engine& E);
int f64_adam_init(pinn_engine& E, const double* theta);
int f64_adam_get(pinn_engine& E, double* theta);
int f64_adam_steps(pinn_engine& E, int nsteps, double lr, double beta1, double beta2, double eps, const float* term_w, double* loss_history);
int f64_points_from_device(pinn_engine& E, int term);
int f64_eval_from_device_f32(pinn_engine& E, const float* d_theta, const float* term_w, float* d_out, bool want_grad);
int f64_eval_from_device_f64(pinn_engine& E, const double* d_theta, const float* term_w, double* d_out);
double* f64_theta_buffer(pinn_engine& E);          // the device buffer [P, padded] every float64 evaluation of the handle reads its parameters from
int f64_eval_resident(pinn_engine& E, const double* term_w, double* d_out);      // evaluate at the parameters in that buffer: d_out = [gradient | raw sums] (P + K doubles, device)
int f64_eval_sharded_local(pinn_engine& E, const double* theta, const double* term_w, double** d_out);      // host theta -> this device's [gradient | sums] (P + K doubles, device)
int f64_adam_steps_comm(pinn_engine** es, int ndev, int nsteps, double lr, double beta1, double beta2, double eps, const float* term_w, double* loss_history);
// plan.cpp
// GEMM arithmetic the kernel look-ups of the calling thread select (family 2 kernels exist as split-operand and fp32 twins): set for the
// duration of an entry point that may look kernels up
int current_gemm();
int current_act_hint();             // activation kind of the network being planned (-1: none): which kernels a hiprtc-specialised member compiles first
struct GemmScope {
    int prev;
    explicit GemmScope(int mode);
    ~GemmScope();
};
int round_hp(int h);
const pk::SpecInfo* find_spec(int HP, int NHH, int D, unsigned need_first, const std::vector<std::pair<int, int>>& need_pairs,
                              unsigned need_hi, std::vector<int>* pair_index, int need_variant = 0, int need_family = 0);
int chan_of(const pk::SpecInfo& s, const Slot& sl);
// find_spec, or — for shapes / jet sets outside the ahead-of-time table — compile, cache and load the kernel (jit.cpp) and look again
const pk::SpecInfo* ensure_spec(const Net& N, unsigned need_first, const std::vector<std::pair<int, int>>& need_pairs, unsigned need_hi,
                                int need_family = 0);
// jit.cpp
int jit_round_hp(int h);
int jit_spec(int HP, int NHH, int D, unsigned D1MASK, unsigned long long PAIRS, int NPAIR, unsigned HI, int variant);
std::string jit_take_launch_error();          // message of a specialised kernel that could not be launched since the last call (empty: none); clears it
// general multi-index jet sets (mixed derivatives of order >= 3, orders 5-6): closed, ordered channel list of a set of requested
// multi-indices (nibble 0 = order, nibbles 1.. = sorted axes) and the kernel generated for it
std::vector<unsigned> gen_close(const std::vector<unsigned>& want);
int jit_spec_gen(int HP, int NHH, int D, const std::vector<unsigned>& channels, int variant);
int jit_spec_dgm(int MP, int L, int D, unsigned D1MASK, unsigned long long PAIRS, int NPAIR, unsigned HI, const std::vector<unsigned>* gen_channels, int act1, int act2);
// plan.cpp: process-wide table of requested general sets; a request travels through the (first, pairs, hi) needs as hi = GEN_FLAG | id
constexpr unsigned GEN_FLAG = 0x80000000u;
int gen_set_id(const std::vector<unsigned>& want);             // id of the (closed) set containing `want`
const std::vector<unsigned>& gen_set(int id);
unsigned slot_mi(const Slot& s);                               // multi-index of a slot
bool slot_is_general(const Slot& s);                           // not representable by the fixed channel categories      // jet channel of a slot in a kernel's channel set (-1: not carried)
// kernel-variant bit a network's activation needs beyond the tanh / sigmoid kernels every spec has (SpecInfo::has_sin)
inline int variant_of(int act) { return act == pk::ACT_SIN ? pk::VARIANT_SIN : (act == pk::ACT_MIXED ? pk::VARIANT_MIXED : (act == pk::ACT_SWISH ? pk::VARIANT_SWISH : 0)); }
std::string spec_name(const pk::SpecInfo& s);
int build_plan(pinn_engine& E);
void free_plan(pinn_engine& E);            // releases everything build_plan allocated (the terms keep their point sets)
void retile(pinn_engine& E, int gi);
}  // namespace pe
