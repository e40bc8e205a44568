// engine.cpp — host side of the C ABI: handles, point sets and samplers, options, and the evaluation (run_loss_grad and the entry points over
// it).  Parsing, program passes and the kernel plan are descriptor.cpp, program.cpp and plan.cpp; the communicator comm.cpp; the float64 mode
// f64.cpp and its f64_*.cpp units; the resident solvers adam.cpp, hmc.cpp, lbfgs.cpp and ensemble.cpp.  This unit alone sees aux_kernels.hpp.
//
// Mirrors what the reference does once per `discretize` call on the host
// (src/discretize.jl:413-767: build loss functions, merge with the strategy, build full_loss_function)
// and what it does per optimiser iteration (src/discretize.jl:567-598).
#include "resident.hpp"
#include "aux_kernels.hpp"
#include <unistd.h>      // environ

#ifdef PINN_EMU
namespace wv {
thread_local void (*emu_barrier_hook)(void*) = nullptr;
thread_local void* emu_barrier_ctx = nullptr;
thread_local void (*emu_grid_hook)(void*) = nullptr;
thread_local void* emu_grid_ctx = nullptr;
}  // namespace wv
#endif

namespace pk {
std::deque<SpecInfo>& registry() {
    static std::deque<SpecInfo> r;
    return r;
}
std::deque<PairInfo>& pair_registry() {
    static std::deque<PairInfo> r;
    return r;
}
}  // namespace pk

namespace pe {
thread_local std::string g_err;
int fail(const std::string& m) {
    g_err = m;
    return 1;
}
}  // namespace pe

using namespace pe;

namespace {

// (re-)evaluate a term's coordinate-only source channels for its current point set
// embedded terms (periodic input embedding): the installed point set lives in d_upts [n][d_user]; the device rows [n][d] = the
// coordinates followed by their sin / cos rows are rebuilt from it whenever it changes (set_points, every sampler draw)
inline float* user_pts(Term& T) { return T.emb_cols.empty() ? T.d_pts : T.d_upts; }
void expand_sites(pinn_engine& E, Term& T);
void embed_points(pinn_engine& E, Term& T) {
    expand_sites(E, T);                                  // (integral terms: the site set follows every change of the point set)
    if (T.emb_cols.empty() || !T.d_upts || T.n <= 0) return;
    aux::EmbedArgs a;
    std::memset(&a, 0, sizeof a);
    a.upts = T.d_upts; a.pts = T.d_pts; a.n = (int)T.n; a.du = T.d_user; a.dx = T.d;
    for (size_t k = 0; k < T.emb_cols.size() && k < 4; ++k) { a.src[k] = T.emb_cols[k].src; a.is_cos[k] = T.emb_cols[k].is_cos; a.omega[k] = T.emb_cols[k].omega; }
    aux::launch_embed(a, E.stream);
}
// integral terms: device form of node k (shared by the site expansion and the tail kernel)
aux::IntNodeDev int_node_dev(const Term& T, int k, int prog_off) {
    const IntNode& Nd = T.inodes[(size_t)k];
    aux::IntNodeDev d;
    std::memset(&d, 0, sizeof d);
    d.var = Nd.var; d.lo_row = Nd.lo_row; d.hi_row = Nd.hi_row; d.lo = (float)Nd.lo; d.hi = (float)Nd.hi; d.lo64 = Nd.lo; d.hi64 = Nd.hi;
    d.slot0 = Nd.slot0; d.nslots = Nd.nslots; d.prog_off = prog_off; d.nops = (int)Nd.ops.size(); d.out_row = Nd.out_row;
    return d;
}
// (re-)build blocks 1.. of an integral term's site set from block 0, the collocation points (set_points, every sampler draw)
void expand_sites(pinn_engine& E, Term& T) {
    if (T.inodes.empty() || !T.d_pts || T.n <= 0) return;
    aux::IntSitesArgs a;
    std::memset(&a, 0, sizeof a);
    a.sites = T.d_pts; a.N = (int)T.n; a.d = T.d; a.nnodes = (int)T.inodes.size(); a.Q = T.int_q; a.xi = E.d_int_xi;
    for (int k = 0; k < a.nnodes; ++k) a.node[k] = int_node_dev(T, k, 0);
    aux::launch_int_sites(a, E.stream);
}
void eval_sources(pinn_engine& E, Term& T) {
    if (T.src_root.empty() || T.coupled >= 0) return;
    aux::SrcArgs a;
    std::memset(&a, 0, sizeof a);
    a.pts = T.d_pts; a.N = (int)T.n; a.d = T.d; a.prog = T.d_src_prog; a.nops = (int)T.src_prog.size();
    a.nsrc = (int)T.src_root.size();
    for (int j = 0; j < a.nsrc; ++j) a.root[j] = T.src_root[j];
    a.out = T.d_src;
    a.data = T.d_data;
    if (T.ndata > 0 && T.data_n != T.n) return;          // data not installed yet for this point set (ensure_points reports it)
    aux::launch_src(a, E.stream);
}

}  // namespace

void pe::redraw_term(pinn_engine& E, Term& T, bool sources) {
    aux::launch_sample(T.sampler, user_pts(T), (int)(T.n * T.d_user), T.d_user, T.d_lb, T.d_ub, sampler_seed(E, T), T.draws++, E.stream);
    embed_points(E, T);                                  // (the float feature rows of an embedded term stay in step with the draw: a later switch back to fp32 reads them)
    if (sources) eval_sources(E, T);
}

int pe::ensure_points(pinn_engine& E) {
    for (size_t t = 0; t < E.terms.size(); ++t) {
        if (!E.terms[t].d_pts || E.terms[t].n <= 0)
            return fail("term " + std::to_string(t) + " has no collocation points (call pinn_set_points first)");
        if (E.terms[t].ndata > 0 && E.terms[t].data_n != E.terms[t].n)
            return fail("term " + std::to_string(t) + " uses per-point data channels but none are installed for its current point set (call pinn_set_point_data after pinn_set_points)");
    }
    return 0;
}

// the weights every network's kernels read in this evaluation: the packed image rebuilt by k_pack (DGM kernels read theta itself)
void pe::pack_all(pinn_engine& E, const float* d_theta, bool packed_fresh) {
    const float* th = d_theta ? d_theta : E.d_theta;
    for (size_t n = 0; n < E.nets.size(); ++n) {
        NetPlan& NP = E.netplans[n];
        if (!NP.spec) continue;
        if (NP.spec->family == 3) { NP.cur = th + E.nets[n].theta_off; continue; }          // DGM kernels read theta unpacked
        NP.cur = NP.d_packed;
        const bool gather = !packed_fresh;                         // (fresh: the optimiser's update kernel already wrote the fp32 image)
        if (gather && !NP.spec->BFX) aux::launch_pack(NP.d_packed, NP.d_pack_idx, th, NP.npacked, E.stream);
        if (NP.spec->BFX) {                                        // split-operand GEMMs: the three bf16 pieces of every hidden->hidden weight,
                                                                   // written by the same launch as the fp32 image
            const Net& N = E.nets[n];
            aux::PackBfArgs pa;
            std::memset(&pa, 0, sizeof pa);
            pa.theta = th; pa.out_fwd = (unsigned*)(NP.d_packed + NP.spec->OFF_WB); pa.out_tr = (unsigned*)(NP.d_packed + NP.spec->OFF_WTB);
            pa.nhh = NP.spec->NHH; pa.hp = NP.spec->HP;
            pa.packed = NP.d_packed; pa.idx = NP.d_pack_idx; pa.n_gather = gather ? NP.spec->OFF_WB : 0;      // (the fp32 part of the image ends where the bf16 pieces begin)
            if (pa.nhh > aux::PACK_BF_MAX_LAYERS) return;          // (build_plan refuses such nets)
            int o = N.theta_off;
            for (size_t j = 0; j + 1 < N.sizes.size(); ++j) {
                if (j >= 1 && j <= (size_t)pa.nhh) { pa.woff[j - 1] = o; pa.nin[j - 1] = N.sizes[j]; pa.nout[j - 1] = N.sizes[j + 1]; }
                o += N.sizes[j + 1] * N.sizes[j] + N.sizes[j + 1];
            }
            aux::launch_pack_bf16(pa, E.stream);
        }
    }
    for (auto& G : E.groups) G.ga.packed = E.netplans[G.net].cur;
    aux::launch_params(E.d_params, th, E.d_defaults, E.np, E.ne, E.p_theta_off, E.stream);
}

namespace {

// launch arguments of k_expr for one coupled equation
aux::ExprArgs expr_args(pinn_engine& E, Coupled& Cp, float scale, float* resid) {
    Term& T = E.terms[Cp.term];
    aux::ExprArgs a;
    std::memset(&a, 0, sizeof a);
    a.pts = T.d_pts; a.N = (int)T.n; a.d = T.d; a.nparams = E.np; a.nparams_estim = E.ne; a.params = E.d_params;
    a.nslots = (int)T.slots.size();
    std::vector<std::vector<char>> used(Cp.nets.size());
    for (size_t i = 0; i < Cp.nets.size(); ++i) used[i].assign(E.groups[Cp.groups[i]].spec->C, 0);
    for (int si = 0; si < a.nslots; ++si) {
        const int i = Cp.slot_net[si], ch = T.chan_of_slot[si];
        a.jets[si] = Cp.d_jets[i] + (size_t)ch * T.n;
        a.ubar[si] = Cp.d_ubar[i] + (size_t)ch * T.n;
        used[i][ch] = 1;
    }
    for (size_t i = 0; i < Cp.nets.size(); ++i)
        for (size_t ch = 0; ch < used[i].size(); ++ch)
            if (!used[i][ch] && a.nzero < aux::EXPR_MAX_SLOTS) a.zero[a.nzero++] = Cp.d_ubar[i] + ch * T.n;
    a.prog = Cp.d_prog; a.nops = (int)T.ops.size(); a.out_row = T.out_row; a.scale = scale;
    a.losspart = Cp.d_losspart; a.pslab = Cp.d_pslab; a.K = (int)E.terms.size(); a.term_id = Cp.term; a.resid = resid;
    a.data = T.d_data;
    a.pw = (T.pw_n == T.n && T.pw_n > 0) ? T.d_pw : nullptr;
    return a;
}

// launch arguments of k_int_expr for an integral term (one network: Cp.d_jets[0] / d_ubar[0] are [C][sites x N])
aux::IntExprArgs int_expr_args(pinn_engine& E, Coupled& Cp, float scale, float* resid) {
    Term& T = E.terms[Cp.term];
    aux::IntExprArgs a;
    std::memset(&a, 0, sizeof a);
    a.sites = T.d_pts; a.N = (int)T.n; a.d = T.d; a.nparams = E.np; a.nparams_estim = E.ne; a.params = E.d_params;
    a.jets = Cp.d_jets[0]; a.ubar = Cp.d_ubar[0]; a.C = E.groups[Cp.groups[0]].spec->C;
    a.n_outer = T.n_outer; a.nnodes = (int)T.inodes.size(); a.Q = T.int_q;
    for (size_t si = 0; si < T.slots.size(); ++si) a.chan[si] = T.chan_of_slot[si];
    for (int c = 0; c < aux::INT_MAX_C; ++c) {
        a.outer_slot_of_chan[c] = -1;
        for (int k = 0; k < aux::INT_MAX_NODES; ++k) a.node_slot_of_chan[k][c] = -1;
    }
    for (int si = 0; si < T.n_outer; ++si) a.outer_slot_of_chan[T.chan_of_slot[(size_t)si]] = si;
    int off = 0;
    for (int k = 0; k < a.nnodes; ++k) {
        a.node[k] = int_node_dev(T, k, off);
        off += (int)T.inodes[(size_t)k].ops.size();
        for (int si = a.node[k].slot0; si < a.node[k].slot0 + a.node[k].nslots; ++si) a.node_slot_of_chan[k][T.chan_of_slot[(size_t)si]] = si;
    }
    a.w = E.d_int_w;
    a.prog = Cp.d_prog; a.iprog = T.d_int_prog; a.nops = (int)T.ops.size(); a.out_row = T.out_row; a.scale = scale;
    a.losspart = Cp.d_losspart; a.pslab = Cp.d_pslab; a.K = (int)E.terms.size(); a.term_id = Cp.term; a.resid = resid;
    a.data = T.d_data;
    a.pw = (T.pw_n == T.n && T.pw_n > 0) ? T.d_pw : nullptr;
    return a;
}

// Gauss-Legendre rule of q nodes on [-1, 1] in double (Newton on P_q from the Chebyshev guess), nodes increasing: what
// numpy.polynomial.legendre.leggauss(q) returns to rounding.  Uploaded as the handle's rule for integral terms.
int upload_int_rule(pinn_engine& E, int q) {
    std::vector<double> xi((size_t)q), w((size_t)q);
    const double PI = 3.14159265358979323846264338327950288;
    for (int i = 0; i < q; ++i) {
        double x = -std::cos(PI * (i + 0.75) / (q + 0.5)), dp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p0 = 1.0, p1 = x;
            for (int n = 2; n <= q; ++n) { const double p2 = ((2.0 * n - 1.0) * x * p1 - (n - 1.0) * p0) / n; p0 = p1; p1 = p2; }
            dp = q * (x * p1 - p0) / (x * x - 1.0);
            const double dx = p1 / dp;
            x -= dx;
            if (std::fabs(dx) < 1e-16) break;
        }
        {
            double p0 = 1.0, p1 = x;
            for (int n = 2; n <= q; ++n) { const double p2 = ((2.0 * n - 1.0) * x * p1 - (n - 1.0) * p0) / n; p0 = p1; p1 = p2; }
            dp = q * (x * p1 - p0) / (x * x - 1.0);
        }
        xi[(size_t)i] = x;
        w[(size_t)i] = 2.0 / ((1.0 - x * x) * dp * dp);
    }
    std::vector<float> wf(w.begin(), w.end());
    if (!E.d_int_xi) {
        E.d_int_xi = (double*)plat_malloc(sizeof(double) * aux::INT_MAX_Q);
        E.d_int_w = (float*)plat_malloc(sizeof(float) * aux::INT_MAX_Q);
        if (!E.d_int_xi || !E.d_int_w) return fail("device allocation failed (quadrature rule)");
    }
    plat_h2d(E.d_int_xi, xi.data(), sizeof(double) * q, E.stream);
    plat_h2d(E.d_int_w, wf.data(), sizeof(float) * q, E.stream);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());      // (pageable temporaries)
    return 0;
}

// workgroups of a forward-only launch (MODE_FWD / FWDREC / LOSS / RESID) over ntiles tiles: as many as stay resident, at most one per tile
// (family 1: per four tiles, one per wave)
int fwd_blocks(const pinn_engine& E, const pk::SpecInfo* spec, int ntiles) {
    return std::max(1, std::min(E.ncu * spec->WG_FWD, spec->family == 1 ? (ntiles + 3) / 4 : ntiles));
}
// where a term sits in a group's term list (the last match; 0: not in it)
int slot_of_term(const Group& G, int term) {
    int j = 0;
    for (size_t q = 0; q < G.terms.size(); ++q) if (G.terms[q] == term) j = (int)q;
    return j;
}
// one = a group's launch arguments narrowed to its term j: that term's tiles alone, from tile 0
void narrow_to_term(pk::GroupArgs& one, const pk::GroupArgs& ga, int j) {
    one = ga;
    one.nterms = 1;
    one.terms[0] = ga.terms[j];
    one.terms[0].tile0 = 0;
    one.ntiles = one.terms[0].ntiles;
}

// ---- the evaluation (run_loss_grad) in phases ----

// the A/B switches of the launch structure, all read from the environment once per evaluation (the tests switch them on a live handle),
// and what they come to for this evaluation
struct EvalSwitches {
    bool no_merge, no_chain, no_reduce_one, no_reduce_perm;
    bool concurrent;                 // the fused groups run on auxiliary streams (fork / join by events)
    bool may_merge;                  // a merged pair of groups may go out as ONE launch
};
EvalSwitches read_switches(const pinn_engine& E, const EvalRequest& rq) {
    EvalSwitches sw = {};
    bool want_concurrent = false;
    // a switch is on when its variable is set, to anything (as with getenv); ONE pass over the environment finds all five — this runs in
    // every evaluation, and five getenv scans cost the host more than the three the evaluation used to make
    const struct { const char* name; bool* on; } vars[] = {{"NO_MERGE=", &sw.no_merge}, {"NO_CHAIN=", &sw.no_chain},
        {"NO_REDUCE_ONE=", &sw.no_reduce_one}, {"NO_REDUCE_PERM=", &sw.no_reduce_perm}, {"CONCURRENT_GROUPS=", &want_concurrent}};
    for (char** e = environ; e && *e; ++e) {
        if (std::strncmp(*e, "PINN_", 5) != 0) continue;
        for (const auto& v : vars)
            if (std::strncmp(*e + 5, v.name, std::strlen(v.name)) == 0) *v.on = true;
    }
    // opt-in: on this stack a cross-stream event wait costs 15-20 us, more than the overlap buys (profiles/r01 timeline).  Fused groups that
    // cannot fill the chip on their own (at most ~1.5 rounds of workgroups, e.g. one rank's share in an 8-GPU strong-scaling run) are then
    // launched concurrently on auxiliary streams; big groups run back to back.
    if (want_concurrent) {
        int nfused_active = 0;
        bool all_small = true;
        for (const Group& G : E.groups) {
            bool on = false;
            for (int ti : G.terms) on = on || (rq.only_term < 0 || rq.only_term == ti);
            if (G.kind != 0 || !on) continue;
            ++nfused_active;
            const int per_round = G.max_blocks * (G.spec->family == 2 ? 1 : 4);
            if (2 * G.ga.ntiles > 3 * per_round) all_small = false;
        }
        sw.concurrent = nfused_active >= 2 && all_small;
    }
    sw.may_merge = !sw.no_merge && !sw.no_chain && !sw.concurrent && rq.only_term < 0;
    return sw;
}

inline bool term_on(const EvalRequest& rq, int ti) { return rq.only_term < 0 || rq.only_term == ti; }
// d (w_k L_k) / d (sum of squares): the factor a term's seeds carry (0: the term is switched off in this evaluation)
float term_scale(const pinn_engine& E, const EvalRequest& rq, int ti) {
    const float w = rq.term_w ? rq.term_w[ti] : 1.0f;
    return term_on(rq, ti) ? (float)(2.0 * (double)w / (double)E.terms[ti].n_norm) : 0.f;
}

// kernel events around a launch group's launch when this evaluation times that group (timing level >= 1); Group::timed says whether it did
struct GroupTimer {
    Group& G;
    const plat_stream st;
    const bool on;
    GroupTimer(const pinn_engine& E, const EvalRequest& rq, size_t g, Group& G_, plat_stream st_)
        : G(G_), st(st_), on(rq.timing && E.timing_level >= 1 && (E.timing_group < 0 || E.timing_group == (int)g)) {
        if (on) plat_event_record(G.ev_a, st);
    }
    ~GroupTimer() {
        if (on) plat_event_record(G.ev_b, st);
        G.timed = on;
    }
};

// The reduction's arguments: one slot per launch group, then one per coupled equation (the pseudo-group of its k_expr / k_int_expr launch),
// filled while the launches go out; launch() then sums the slabs and loss partials of the active slots into the caller's arrays.
struct ReduceSlots {
    aux::Reduce1Args a1;
    aux::Reduce2Args a2;
    const int K;
    const bool loss_only;
    int max_n1 = 1, max_split = 1;
    int nslabsets = 0, slabset_group = -1;          // launch groups whose own slab set carries gradient sums in this evaluation
    bool coupled_active = false;

    ReduceSlots(int K_, bool loss_only_) : K(K_), loss_only(loss_only_) {
        std::memset(&a1, 0, sizeof a1);
        std::memset(&a2, 0, sizeof a2);
    }
    void slot(int g, double* tmp, float* slabs, double* losspart, int slab, int nblocks, int nsplit, int nent, int nwpb, bool active, bool ent_active) {
        a1.tmp[g] = tmp; a1.slabs[g] = slabs; a1.losspart[g] = losspart;
        a1.slab[g] = slab; a1.nblocks[g] = nblocks; a1.nsplit[g] = nsplit; a1.nent[g] = nent; a1.active[g] = active; a1.nwpb[g] = nwpb;
        a2.tmp[g] = tmp; a2.stride[g] = nent + K; a2.nsplit[g] = nsplit; a2.nent[g] = nent; a2.active[g] = active; a2.ent_active[g] = ent_active;
    }
    void count(int nsplit, int nent) {
        max_n1 = std::max(max_n1, nent / 4 + K);
        max_split = std::max(max_split, nsplit);
    }
    // a group with a launch of its own over `blocks` workgroups (inactive: switched off in this evaluation, nothing is launched); chained: its
    // gradient sums went onto the head group's slabs; losspart: where the launch writes its loss partials
    void launched(int g, const Group& G, int blocks, bool active, bool chained, double* losspart) {
        const int nent = (chained || loss_only) ? 0 : G.nent;
        // stage-1 chunks: the serial part of the two-stage sum is (blocks / chunks) loads in stage 1 plus (chunks x slab entries per theta
        // element: 4 per-wave copies in family 1, 1 in the others) in stage 2 — shortest for chunks ~ sqrt(blocks / entries)
        const int epe = G.spec->family == 1 ? 4 : 1;
        const int nsplit = std::max(1, std::min(REDUCE_SPLIT, (int)std::ceil(std::sqrt((double)blocks / epe))));
        const bool ent_active = active && !chained && !loss_only;
        slot(g, G.d_tmp, G.d_slabs, losspart, G.slab_floats, blocks, nsplit, nent, G.spec->NW, active, ent_active);
        if (!active) return;
        if (ent_active) { ++nslabsets; slabset_group = g; }
        count(nsplit, nent);
    }
    // a group whose tiles rode in another group's launch (the tail of a merged pair): its gradient and its loss partials are in the head's buffers
    void rode(int g, const Group& G) { slot(g, G.d_tmp, G.d_slabs, G.d_losspart, G.slab_floats, 0, 1, 0, G.spec->NW, false, false); }
    // the pseudo-group of a coupled equation.  active: its term is on and its k_expr / k_int_expr launch carries the term's sums (not the
    // equation's tail launch); launched: that launch goes out in this evaluation
    void coupled(int g, const Coupled& Cp, bool active, bool launched) {
        const int nsplit = std::min(REDUCE_SPLIT, Cp.blocks);
        const int nent = loss_only ? 0 : 16;
        slot(g, Cp.d_tmp, Cp.d_pslab, Cp.d_losspart, 16, Cp.blocks, nsplit, nent, 4, active, active && !loss_only);
        if (launched) count(nsplit, nent);
    }
    // a loss-only launch of group g ran `blocks` workgroups: the rows of loss partials it wrote
    void rows(int g, int blocks) { a1.nblocks[g] = blocks; }

    // one kernel when a single slab set carries the whole gradient (a single network whose launch groups are merged / chained) or only the
    // K sums are asked for; else reduce1 -> reduce2
    void launch(pinn_engine& E, const EvalRequest& rq, const EvalSwitches& sw) {
        float* d_sums = rq.d_sums ? rq.d_sums : rq.d_out + E.ntheta;      // the K sums follow the gradient unless the caller has a buffer of their own (loss-only)
        a1.K = K;
        a2.out = rq.d_out; a2.sums = d_sums; a2.lossraw = rq.lossraw ? rq.lossraw : E.d_lossraw;
        a2.row_ptr = E.d_gr_ptr; a2.row_grp = E.d_gr_grp; a2.row_ent = E.d_gr_ent;
        a2.ngroups = (int)(E.groups.size() + E.coupled.size()); a2.P = (int)E.ntheta; a2.K = K;
        a2.skip_grad = loss_only ? 1 : 0;
        a2.perm = sw.no_reduce_perm ? nullptr : E.d_red_perm;
        const Group* RG = (nslabsets == 1 && !coupled_active && !loss_only && !sw.no_reduce_one) ? &E.groups[slabset_group] : nullptr;
        const bool one_kernel = ((RG && RG->d_ent_theta && RG->ent_covers_theta) || (loss_only && !sw.no_reduce_one)) && !aux::reduce_is_small(a1, a2);
        if (!one_kernel) {
            aux::launch_reduce(a1, a2, max_n1, max_split, E.stream);
            return;
        }
        aux::ReduceOneArgs ro;
        std::memset(&ro, 0, sizeof ro);
        if (RG) { ro.slabs = RG->d_slabs; ro.slab = RG->slab_floats; ro.nblocks = a1.nblocks[slabset_group]; ro.nent = RG->nent; ro.ent_theta = RG->d_ent_theta; }
        ro.out = rq.d_out; ro.sums = d_sums; ro.lossraw = a2.lossraw; ro.P = (int)E.ntheta; ro.K = K;       // (loss-only: nent = 0, only the K loss blocks run)
        for (int g = 0; g < a2.ngroups; ++g)
            if (a1.active[g]) { ro.losspart[ro.nloss] = a1.losspart[g]; ro.nrows[ro.nloss] = a1.nblocks[g] * a1.nwpb[g]; ++ro.nloss; }
        aux::launch_reduce_one(ro, E.stream);
    }
};

// ga = ONE launch for the head group G's tiles and the tail group's of a merged pair: terms and tiles concatenated, the tail's after the
// head's.  Returns its workgroups.
int merged_args(pinn_engine& E, const EvalRequest& rq, const Group& G, const MergedUnit& mu, pk::GroupArgs& ga) {
    const Group& T2 = E.groups[mu.tail];
    ga = G.ga;
    for (size_t j = 0; j < T2.terms.size(); ++j) {
        pk::TermDev td = T2.ga.terms[j];
        td.tile0 += G.ga.ntiles;
        td.scale = term_scale(E, rq, T2.terms[j]);
        ga.terms[G.terms.size() + j] = td;
    }
    ga.nterms = (int)(G.terms.size() + T2.terms.size());
    ga.sub_terms0 = (int)G.terms.size();
    ga.sub_tiles0 = G.ga.ntiles;
    ga.ntiles = G.ga.ntiles + T2.ga.ntiles;
    ga.scratch = mu.d_scratch;
    ga.scr_stride = mu.pair->SCR;
    ga.losspart = mu.d_losspart;
    ga.chain = 0;
    return std::max(1, std::min(rq.loss_only ? E.ncu * mu.pair->WG_FWD : mu.max_blocks, ga.ntiles));
}

// every launch group in plan order: its terms' scales and its per-evaluation state (Group::active, launched_by, launched_blocks, ga.slabs,
// ga.chain), its slot of the reduction, and the launch itself — fused groups (merged with / chained onto an earlier group of their
// network where the plan and the switches allow) and the forward launches of coupled equations' networks
void launch_groups(pinn_engine& E, const EvalRequest& rq, const EvalSwitches& sw, ReduceSlots& R) {
    const bool loss_only = rq.loss_only;
    int nforked = 0;
    if (sw.concurrent) plat_event_record(E.ev_fork, E.stream);
    for (size_t g = 0; g < E.groups.size(); ++g) {
        Group& G = E.groups[g];
        bool any = false;
        for (size_t j = 0; j < G.terms.size(); ++j) {
            G.ga.terms[j].scale = term_scale(E, rq, G.terms[j]);
            any = any || term_on(rq, G.terms[j]);
        }
        G.active = any;
        G.timed = false;
        const MergedUnit* mu = (sw.may_merge && G.kind == 0 && G.merged >= 0) ? &E.merged[G.merged] : nullptr;
        if (mu && (int)g == mu->tail) {                  // this group's tiles ran in the head's merged launch
            G.launched_by = mu->head;
            G.launched_blocks = E.groups[mu->head].launched_blocks;
            R.rode((int)g, G);
            continue;
        }
        // chained launch groups: this group's workgroups add their sums onto the slabs the head group (same network, launched
        // earlier on the same stream in this evaluation) has just written, so the reduction reads one slab set, not two
        const bool chained = any && !loss_only && !sw.no_chain && !sw.concurrent && G.kind == 0 && G.chain_to >= 0 && E.groups[G.chain_to].active &&
                             G.blocks <= E.groups[G.chain_to].launched_blocks;
        G.ga.slabs = chained ? E.groups[G.chain_to].d_slabs : G.d_slabs;
        G.ga.chain = chained ? 1 : 0;
        pk::GroupArgs ga_one;
        const pk::GroupArgs* ga_launch = &G.ga;
        int blocks = G.blocks;
        // a single-term evaluation (pinn_term_grads) of a fused group launches ONLY that term's tiles: the K per-term gradients then cost
        // about one full evaluation in total instead of K
        if (any && rq.only_term >= 0 && G.kind == 0 && G.terms.size() > 1) {
            narrow_to_term(ga_one, G.ga, slot_of_term(G, rq.only_term));
            blocks = std::max(1, std::min(G.max_blocks, G.spec->family == 1 ? (ga_one.ntiles + 3) / 4 : ga_one.ntiles));
            ga_launch = &ga_one;
        }
        const bool merged_head = mu && (int)g == mu->head;
        if (merged_head) {
            blocks = merged_args(E, rq, G, *mu, ga_one);
            ga_launch = &ga_one;
        }
        G.launched_blocks = blocks;
        G.launched_by = (int)g;
        R.launched((int)g, G, blocks, any, chained, merged_head ? mu->d_losspart : G.d_losspart);
        if (!any) continue;
        if (G.kind == 1) {               // coupled: forward launch now, reverse launch after k_expr / the equation's tail launch
            G.spec->launch(G.ga, (G.use_rec && !loss_only) ? pk::MODE_FWDREC : pk::MODE_FWD, fwd_blocks(E, G.spec, G.ga.ntiles), E.stream);
            continue;
        }
        if (G.kind == 2) continue;       // tail launch of a coupled equation: after the other networks' forward launches (launch_coupled)
        plat_stream st = E.stream;
        const bool forked = sw.concurrent && nforked++ > 0;       // the first fused group stays on the caller's stream
        if (forked) {
            st = E.aux_stream[nforked % 2];
            plat_stream_wait_event(st, E.ev_fork);
        }
        {
            GroupTimer timer(E, rq, g, G, st);
            if (merged_head) mu->pair->launch(*ga_launch, loss_only ? pk::MODE_LOSS : pk::MODE_FUSED, blocks, st);
            else if (loss_only) {
                const int fb = fwd_blocks(E, G.spec, ga_launch->ntiles);
                R.rows((int)g, fb);
                G.launched_blocks = fb;
                G.spec->launch(*ga_launch, pk::MODE_LOSS, fb, st);
            } else G.spec->launch(*ga_launch, pk::MODE_FUSED, blocks, st);
        }
        if (forked) {
            plat_event_record(E.ev_join[g], st);
            plat_stream_wait_event(E.stream, E.ev_join[g]);
        }
    }
}

// every coupled equation whose networks ran forward above: its slot of the reduction, then its TAIL launch — forward pass of the widest
// network + the equation's tape (the other networks' jets as source rows) + its reverse sweep in one kernel; it writes the other networks'
// seeds and carries the term's loss partials and parameter gradients itself, so the pseudo-group stays out of the reduction — or
// k_expr / k_int_expr over all networks' jets
void launch_coupled(pinn_engine& E, const EvalRequest& rq, ReduceSlots& R) {
    const bool loss_only = rq.loss_only;
    for (size_t c = 0; c < E.coupled.size(); ++c) {
        Coupled& Cp = E.coupled[c];
        bool groups_active = false;
        for (int gi : Cp.groups) groups_active = groups_active || E.groups[gi].active;
        const bool by_tail = groups_active && Cp.tail >= 0;
        R.coupled((int)(E.groups.size() + c), Cp, term_on(rq, Cp.term) && !by_tail, groups_active && !by_tail);
        if (!groups_active) continue;
        R.coupled_active = true;
        if (by_tail) {
            const int gt = Cp.groups[Cp.tail];
            Group& G = E.groups[gt];
            GroupTimer timer(E, rq, (size_t)gt, G, E.stream);
            if (loss_only) {
                const int fb = fwd_blocks(E, G.spec, G.ga.ntiles);      // (the tail network's kernel is family 2: plan.cpp)
                R.rows(gt, fb);
                G.launched_blocks = fb;
                G.spec->launch(G.ga, pk::MODE_LOSS, fb, E.stream);
            } else G.spec->launch(G.ga, pk::MODE_FUSED, G.blocks, E.stream);
        } else if (!E.terms[Cp.term].inodes.empty()) {          // integral term: the tail kernel over the site set's jets
            aux::IntExprArgs ia = int_expr_args(E, Cp, term_scale(E, rq, Cp.term), nullptr);
            ia.loss_only = loss_only ? 1 : 0;
            aux::launch_int_expr(ia, Cp.blocks, E.stream);
        } else {
            aux::ExprArgs ea = expr_args(E, Cp, term_scale(E, rq, Cp.term), nullptr);    // scale 0 => zero seeds
            ea.loss_only = loss_only ? 1 : 0;
            aux::launch_expr(ea, Cp.blocks, E.stream);
        }
    }
}

// the reverse launches of coupled equations' networks, from the seeds k_expr / the tail launch wrote
void launch_coupled_reverse(pinn_engine& E, const EvalRequest& rq) {
    for (size_t g = 0; g < E.groups.size(); ++g) {
        Group& G = E.groups[g];
        if (G.kind != 1 || !G.active) continue;
        GroupTimer timer(E, rq, g, G, E.stream);
        G.spec->launch(G.ga, G.use_rec ? pk::MODE_GRADREC : pk::MODE_GRADIN, G.blocks, E.stream);
    }
}

}  // namespace

// The device section shared by all fp32 loss / gradient entry points: what rq (engine_types.hpp: EvalRequest) asks for, queued on E.stream.
// Launches per evaluation: pack (1 per net) -> fused residual kernel (1 per group, or 1 per MERGED pair of groups); coupled equations:
// forward launches, k_expr / k_int_expr / the tail launch, reverse launches -> reduction (one kernel when a single slab set carries the
// gradient, else reduce1 -> reduce2).  loss_only: MODE_LOSS launches (forward + tape + sums of squares; coupled equations: forward
// launches + k_expr without adjoints), only the K sums are reduced.  Each phase is one function above; what an evaluation leaves in a
// Group (active, timed, launched_blocks, launched_by, ga.slabs, ga.chain, the terms' scales) is read afterwards by pinn_group_timing,
// pinn_group_launched_by, eval_one_launch and the next evaluation's chaining decision.
int pe::run_loss_grad(pinn_engine& E, const EvalRequest& rq) {
    if (ensure_points(E)) return 1;
    const bool phase_ev = rq.timing && E.timing_level >= 2;
    if (phase_ev) plat_event_record(E.ev0, E.stream);
    pack_all(E, rq.d_theta, rq.packed_fresh);
    if (phase_ev) plat_event_record(E.ev1, E.stream);
    const EvalSwitches sw = read_switches(E, rq);        // (after the pack launches: the device is busy while the host looks)
    ReduceSlots R((int)E.terms.size(), rq.loss_only);
    launch_groups(E, rq, sw, R);
    launch_coupled(E, rq, R);
    if (!rq.loss_only) launch_coupled_reverse(E, rq);
    if (phase_ev) plat_event_record(E.ev2, E.stream);
    R.launch(E, rq, sw);
    if (phase_ev) plat_event_record(E.ev3, E.stream);
    // a run-time specialised kernel whose code object could not be produced / loaded at its first launch (jit.cpp: rtc_launch) was NOT launched
    { const std::string e = jit_take_launch_error(); if (!e.empty()) return fail(e); }
    return 0;
}

void pe::sums_from_double(float* d_out_sums, const double* d_raw, int K, plat_stream st) { aux::launch_sums_from_double(d_out_sums, d_raw, K, st); }

int pe::upload_theta(pinn_engine& E, const float* theta, int64_t p) {
    if (p != E.ntheta) return fail("theta length " + std::to_string(p) + " != ntheta " + std::to_string(E.ntheta));
    std::memcpy(E.hp_theta, theta, sizeof(float) * p);          // pinned staging: the copy below is a plain DMA, no pageable bounce
    if (plat_h2d(E.d_theta, E.hp_theta, sizeof(float) * p, E.stream)) return fail(std::string("H2D copy of theta failed: ") + plat_last_error());
    return 0;
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char* pinn_backend(void) { return plat_name(); }
int pinn_abi_version(void) { return 1; }
const char* pinn_last_error(void) { return g_err.c_str(); }

int pinn_create(const char* descriptor, pinn_handle* out) { return pinn_create_on(descriptor, -1, out); }

int pinn_create_on(const char* descriptor, int device, pinn_handle* out) {
    if (!descriptor || !out) return fail("pinn_create: null argument");
    *out = nullptr;
    std::string err;
    if (plat_init(err)) return fail(err);
    if (device >= plat_device_count()) return fail("pinn_create_on: device " + std::to_string(device) + " does not exist (" + std::to_string(plat_device_count()) + " visible)");
    const int dev = device < 0 ? plat_get_device() : device;
    DeviceScope scope(dev);
    std::unique_ptr<pinn_engine> E(new pinn_engine());
    E->device = dev;
    if (const char* gm = std::getenv("PINN_GEMM")) {             // default GEMM arithmetic of new handles (pinn_set_option switches a live one)
        if (std::string(gm) == "fp32") E->gemm = pk::GEMM_FP32;
        else if (std::string(gm) == "split") E->gemm = pk::GEMM_SPLIT;
        else return fail(std::string("PINN_GEMM must be \"split\" or \"fp32\", not \"") + gm + "\"");
    }
    if (parse_descriptor(descriptor, *E)) return 1;
    E->terms0 = E->terms;                              // (before the planner rewrites them: the float64 mode evaluates the terms as parsed)
    E->ncu = plat_num_cus();
#ifdef PINN_EMU
    // the emulated device has 2 CUs unless $PINN_EMU_CUS (1..64) says otherwise: launch decisions that weigh a group against the chip (the
    // concurrent path takes groups of at most 1.5 rounds of workgroups) are out of a small problem's reach on 2
    if (const char* cus = std::getenv("PINN_EMU_CUS")) E->ncu = std::max(1, std::min(64, std::atoi(cus)));
#endif
    E->stream = plat_stream_create();
    const int K = (int)E->terms.size();
    E->d_theta = (float*)plat_malloc(sizeof(float) * E->ntheta);
    E->d_params = (float*)plat_malloc(sizeof(float) * pk::MAX_PARAMS);
    E->d_defaults = (float*)plat_malloc(sizeof(float) * pk::MAX_PARAMS);
    E->d_lossraw = (double*)plat_malloc(sizeof(double) * K);
    E->d_out = (float*)plat_malloc(sizeof(float) * (E->ntheta + K));
    plat_event_create(E->ev0); plat_event_create(E->ev1); plat_event_create(E->ev2); plat_event_create(E->ev3);
    plat_event_create(E->ev_fork);
    for (auto& e : E->ev_join) plat_event_create(e);
    for (auto& st : E->aux_stream) st = plat_stream_create();
    if (!E->d_theta || !E->d_params || !E->d_defaults || !E->d_lossraw || !E->d_out) {
        pinn_destroy(E.release());                   // releases whatever was allocated
        return fail("device allocation failed");
    }
    plat_h2d(E->d_defaults, E->p_defaults32.data(), sizeof(float) * pk::MAX_PARAMS, E->stream);
    // one pinned block for the host entry points; the reduction writes its results straight into it
    E->hp_theta = (float*)plat_host_alloc(sizeof(float) * (2 * E->ntheta + K + 2) + sizeof(double) * K);
    if (!E->hp_theta) {
        pinn_destroy(E.release());
        return fail("pinned host allocation failed");
    }
    E->hp_out = E->hp_theta + E->ntheta;
    E->hp_raw = (double*)(E->hp_theta + ((2 * E->ntheta + K + 1) / 2) * 2);
    bool any_int = false;
    for (auto& T : E->terms) any_int = any_int || !T.inodes.empty();
    if ((any_int && upload_int_rule(*E, E->int_q)) || build_plan(*E)) {
        const std::string msg = g_err;               // pinn_destroy must not lose the reason
        pinn_destroy(E.release());
        g_err = msg;
        return 1;
    }
    *out = E.release();
    return 0;
}

int pinn_destroy(pinn_handle h) {
    if (!h) return 0;
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    pinn_comm_destroy(h);
    plat_sync(E.stream);
    hmc_free(E);
    lbfgs_free(E);
    bfgs_free(E);
    ens_free(E);
    cub_free(E);
    f64_destroy(E);
    free_plan(E);
    for (auto& T : E.terms) { plat_free(T.d_pts); plat_free(T.d_upts); plat_free(T.d_resid); plat_free(T.d_lb); plat_free(T.d_ub); plat_free(T.d_data); plat_free(T.d_pw); }
    plat_free(E.d_opt_theta); plat_free(E.d_opt_m); plat_free(E.d_opt_v); plat_free(E.d_opt_out); plat_free(E.d_w_over_n); plat_free(E.d_hist); plat_free(E.d_c12); plat_free(E.d_bar); plat_free(E.d_sums2); plat_free(E.d_own_r); plat_free(E.d_train_samp); plat_free(E.d_opt_bak); plat_host_free(E.h_flag);
    plat_free(E.d_theta); plat_free(E.d_params); plat_free(E.d_defaults); plat_free(E.d_lossraw);
    plat_free(E.d_int_xi); plat_free(E.d_int_w);
    plat_free(E.d_out); plat_free(E.d_phi_pts); plat_free(E.d_phi_out); plat_free(E.d_phi_scr);
    plat_host_free(E.hp_theta);
    plat_event_destroy(E.ev0); plat_event_destroy(E.ev1); plat_event_destroy(E.ev2); plat_event_destroy(E.ev3);
    plat_event_destroy(E.ev_fork);
    for (auto& e : E.ev_join) plat_event_destroy(e);
    for (auto& st : E.aux_stream) plat_stream_destroy(st);
    if (E.own_stream) plat_stream_destroy(E.stream);
    delete h;
    return 0;
}

int pinn_num_terms(pinn_handle h) { return h ? (int)h->terms.size() : -1; }
int64_t pinn_num_theta(pinn_handle h) { return h ? h->ntheta : -1; }

static int term_installed(pinn_engine& E, int term);
static int set_points_impl(pinn_handle h, int term, const float* pts, int64_t n, int64_t n_norm, bool device) {
    if (!h) return fail("null handle");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (term < 0 || term >= (int)E.terms.size()) return fail("pinn_set_points: term index out of range");
    if (!pts || n <= 0) return fail("pinn_set_points: empty point set (the reference's mean(abs2, .) over an empty set is NaN; refusing)");
    Term& T = E.terms[term];
    if (n * T.d >= (int64_t)1 << 31) return fail("pinn_set_points: point set too large for 32-bit indexing; shard it");
    const int64_t S = T.sites();                         // integral terms: d_pts is the site set, the installed points are its block 0
    if (S > 1 && n * S * std::max(T.d, aux::INT_MAX_C) >= (int64_t)1 << 31)
        return fail("pinn_set_points: the site set of integral term " + std::to_string(term) + " (" + std::to_string(n) + " points x (1 + " +
                    std::to_string(T.inodes.size()) + " integral node(s) x " + std::to_string(T.int_q) + " quadrature nodes) = " + std::to_string(n * S) +
                    " sites) exceeds what one launch group takes (32-bit indexing of its jet channels); shard the point set or lower integral_nodes");
    if (points_reserve(E, term, n)) return 1;
    int rc = device ? plat_d2d(user_pts(T), pts, sizeof(float) * n * T.d_user, E.stream) : plat_h2d(user_pts(T), pts, sizeof(float) * n * T.d_user, E.stream);
    if (rc) return fail(std::string("copy of points failed: ") + plat_last_error());
    if (points_written(E, term, n, n_norm)) return 1;
    return f64_points_changed(E, term);                  // (float64 mode: the double copy follows)
}
// room for n points in the term's point buffer (the contents do not survive a growth)
extern "C++" int pe::points_reserve(pinn_engine& E, int term, int64_t n) {
    Term& T = E.terms[term];
    const int64_t S = T.sites();
    if (n > T.pts_cap || !T.d_pts) {                     // grow only: a resampled set of another size reuses the buffer
        plat_sync(E.stream);                             // (an evaluation in flight may still read the old buffer)
        plat_free(T.d_pts);
        plat_free(T.d_upts);
        T.d_upts = nullptr;
        T.pts_cap = 0;
        T.d_pts = (float*)plat_malloc(sizeof(float) * n * S * T.d);
        if (!T.emb_cols.empty()) T.d_upts = (float*)plat_malloc(sizeof(float) * n * T.d_user);
        if (!T.d_pts || (!T.emb_cols.empty() && !T.d_upts)) return fail("device allocation failed (points)");
        T.pts_cap = n;
    }
    return 0;
}
// the term's point buffer holds a new set of n points (a copy, or a kernel's stores queued on the stream): the bookkeeping that follows.  The
// double copy of the float64 mode is the caller's
extern "C++" int pe::points_written(pinn_engine& E, int term, int64_t n, int64_t n_norm) {
    Term& T = E.terms[term];
    T.n = n;
    embed_points(E, T);
    plat_sync(E.stream);
    T.n_norm = n_norm > 0 ? n_norm : n;
    T.data_n = 0;                                        // per-point data and weights belong to the previous set
    T.pw_n = 0;
    return term_installed(E, term);
}

// what follows the installation of a term's point set (also after a re-plan, pinn_set_option): source channels, tile tables, the buffers of
// a coupled equation
static int term_installed(pinn_engine& E, int term) {
    Term& T = E.terms[term];
    int64_t n = T.n;
    if (T.coupled < 0) {
        if (!T.src_root.empty()) {
            if (T.src_cap < n) {
                plat_free(T.d_src);
                T.d_src = (float*)plat_malloc(sizeof(float) * T.src_root.size() * (size_t)n);
                if (!T.d_src) return fail("device allocation failed (source channels)");
                T.src_cap = n;
            }
            eval_sources(E, T);
            plat_sync(E.stream);
        }
        retile(E, T.group);
        return 0;
    }
    Coupled& Cp = E.coupled[T.coupled];
    const int K = (int)E.terms.size();
    const int64_t npts = n;
    n *= T.sites();                                      // (integral terms: the networks' jets / seeds cover the site set)
    if (Cp.cap < n) {
        for (size_t i = 0; i < Cp.d_jets.size(); ++i)
            if (Cp.tail < 0 || (int)i == Cp.tail) { plat_free(Cp.d_jets[i]); plat_free(Cp.d_ubar[i]); }
        plat_free(Cp.d_jets_all); plat_free(Cp.d_ubar_all);
        Cp.d_jets_all = Cp.d_ubar_all = nullptr;
        Cp.d_jets.assign(Cp.nets.size(), nullptr);
        Cp.d_ubar.assign(Cp.nets.size(), nullptr);
        Cp.cap = 0;
        if (Cp.tail >= 0 && Cp.nsrc > 0) {               // the other networks' channels in ONE array each way: the tail launch's source rows
            Cp.d_jets_all = (float*)plat_malloc(sizeof(float) * (size_t)Cp.nsrc * n);
            Cp.d_ubar_all = (float*)plat_malloc(sizeof(float) * (size_t)Cp.nsrc * n);
            if (!Cp.d_jets_all || !Cp.d_ubar_all) return fail("device allocation failed (coupled jets)");
        }
        for (size_t i = 0; i < Cp.nets.size(); ++i) {
            if (Cp.tail >= 0 && (int)i != Cp.tail) continue;
            const int C = E.groups[Cp.groups[i]].spec->C;
            Cp.d_jets[i] = (float*)plat_malloc(sizeof(float) * (size_t)C * n);
            Cp.d_ubar[i] = (float*)plat_malloc(sizeof(float) * (size_t)C * n);
            if (!Cp.d_jets[i] || !Cp.d_ubar[i]) return fail("device allocation failed (coupled jets)");
        }
        Cp.cap = n;
    }
    if (Cp.tail >= 0)                                    // rows packed with stride n (the kernels address channel c at c * N)
        for (size_t i = 0; i < Cp.nets.size(); ++i)
            if ((int)i != Cp.tail) { Cp.d_jets[i] = Cp.d_jets_all + (size_t)Cp.src_off[i] * n; Cp.d_ubar[i] = Cp.d_ubar_all + (size_t)Cp.src_off[i] * n; }
    Cp.blocks = (int)((npts + 255) / 256);
    if (Cp.cap_blocks < Cp.blocks) {
        plat_free(Cp.d_losspart); plat_free(Cp.d_pslab);
        Cp.d_losspart = (double*)plat_malloc(sizeof(double) * (size_t)Cp.blocks * 4 * K);
        Cp.d_pslab = (float*)plat_malloc(sizeof(float) * (size_t)Cp.blocks * 16);
        if (!Cp.d_losspart || !Cp.d_pslab) return fail("device allocation failed (coupled partials)");
        plat_memset(Cp.d_losspart, 0, sizeof(double) * (size_t)Cp.blocks * 4 * K, E.stream);
        plat_memset(Cp.d_pslab, 0, sizeof(float) * (size_t)Cp.blocks * 16, E.stream);
        plat_sync(E.stream);
        Cp.cap_blocks = Cp.blocks;
    }
    for (int gi : Cp.groups) retile(E, gi);
    return 0;
}
int pinn_set_points(pinn_handle h, int term, const float* pts, int64_t n, int64_t n_norm) { return set_points_impl(h, term, pts, n, n_norm, false); }
int pinn_set_points_device(pinn_handle h, int term, const float* d_pts, int64_t n, int64_t n_norm) { return set_points_impl(h, term, d_pts, n, n_norm, true); }
int pinn_set_points_f64(pinn_handle h, int term, const double* pts, int64_t n, int64_t n_norm) {
    if (!h || !pts || n <= 0) return fail("pinn_set_points_f64: null argument / empty point set");
    if (term < 0 || term >= (int)h->terms.size()) return fail("pinn_set_points_f64: term index out of range");
    auto p32 = as<float>(pts, (size_t)n * h->terms[term].d_user);
    if (set_points_impl(h, term, p32.get(), n, n_norm, false)) return 1;        // the fp32 kernels' copy (EltypeAdaptor, src/eltype_matching.jl:8-10)
    if (!h->f64) return 0;
    DeviceScope scope(h->device);
    return f64_set_points(*h, term, pts, n);                                    // the float64 mode reads the points as given
}

extern "C++" int pe::eval_and_sync(pinn_engine& E, float* d_out, const float* term_w, double* lossraw, bool timing) {
    E.eval_path = 1;
    if (ensure_points(E)) return 1;                  // (every path: the one-launch evaluation below does not go through run_loss_grad's check — ADVICE r04)
    const int one = eval_one_launch(E, d_out, term_w, lossraw);
    if (one == 1) return 1;
    if (one == 0) { E.eval_path = 2; return 0; }     // (2: not a small problem, or timed out — the stand-alone kernels run / repeat the evaluation)
    EvalRequest rq = EvalRequest::device(E.d_theta, d_out, term_w);
    rq.timing = timing;
    rq.lossraw = lossraw;
    if (run_loss_grad(E, rq)) return 1;
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

// the fp32 body of pinn_loss_grad[_f64]: theta goes through the pinned staging block and the results land in it (no per-call host allocation)
static int loss_grad_f32(pinn_engine& E, const float* theta, const float* term_w, double* term_losses, float* grad) {
    const int K = (int)E.terms.size();
    if (upload_theta(E, theta, E.ntheta)) return 1;
    // grad == NULL: loss-only evaluation (no records, no reverse sweep, no gradient reduction) — what a callback, an adaptive-weight
    // rule or a rejected line-search trial needs (the reference's per-term closures are value-only unless differentiated,
    // src/training_strategies.jl:215-221)
    if (grad) {
        if (eval_and_sync(E, E.hp_out, term_w, E.hp_raw, true)) return 1;                                            // results land in pinned host memory
    } else {
        EvalRequest rq = EvalRequest::host_entry(E, term_w);
        rq.timing = true;
        rq.loss_only = true;
        if (run_loss_grad(E, rq)) return 1;
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    }
    E.timing_valid = E.timing_level >= 2;
    if (term_losses)
        for (int k = 0; k < K; ++k) term_losses[k] = E.hp_raw[k] / (double)E.terms[k].n_norm;   // exact double sums
    if (grad) std::memcpy(grad, E.hp_out, sizeof(float) * E.ntheta);
    if (grad && E.gemm_auto) {                           // "gemm" = "auto": this evaluation's gradient health decides the NEXT evaluation's GEMM mode
        std::vector<float> gs((size_t)E.ntheta + K);
        std::memcpy(gs.data(), E.hp_out, sizeof(float) * E.ntheta);
        for (int k = 0; k < K; ++k) gs[(size_t)E.ntheta + k] = (float)E.hp_raw[k];
        measure_grad_health(E, gs.data(), term_w);
        if (gemm_auto_check(E, E.d_theta, term_w, ++E.eval_count)) return 1;
    }
    return 0;
}

// l = sum_k logpdf(MvNormal(r_k, sigma_k^2 I), 0) = sum_k [ -N_k/2 log(2 pi) - N_k log sigma_k - SSE_k / (2 sigma_k^2) ]
// (src/training_strategies.jl:113-127; "SSE not MSE", src/discretize.jl:681): an affine function of the per-term sums of squares,
// so grad_theta l = - grad_theta sum_k w_k L_k with w_k = N_k / (2 sigma_k^2): ONE weighted evaluation.  sse[k]: raw sums of squares.
static void loglik_from_sse(const pinn_engine& E, const double* stds, const double* sse, double* loglik, double* grad_std) {
    const int K = (int)E.terms.size();
    double ll = 0.0;
    for (int k = 0; k < K; ++k) {
        // sharded point sets (n < n_norm): every quantity returned here is THIS SHARD'S additive part — the constants count the shard's
        // own points — so that loglik, grad_theta and grad_std summed over the ranks are the global values
        const double N = (double)E.terms[k].n, sd = stds[k];
        ll += -0.5 * N * std::log(2.0 * 3.14159265358979323846) - N * std::log(sd) - sse[k] / (2.0 * sd * sd);
        if (grad_std) grad_std[k] = -N / sd + sse[k] / (sd * sd * sd);
    }
    *loglik = ll;
}
// the float64-mode evaluation behind both pinn_loglik_grad entry points: grad_theta in double
static int loglik_f64(pinn_engine& E, const double* theta, const double* stds, double* loglik, double* grad_theta, double* grad_std) {
    const int K = (int)E.terms.size();
    std::vector<double> w(K), L(K), g(grad_theta ? (size_t)E.ntheta : 0);
    for (int k = 0; k < K; ++k) w[k] = (double)E.terms[k].n_norm / (2.0 * stds[k] * stds[k]);
    if (f64_eval(E, theta, w.data(), L.data(), grad_theta ? g.data() : nullptr)) return 1;
    for (int k = 0; k < K; ++k) L[k] *= (double)E.terms[k].n_norm;           // mean -> SSE
    loglik_from_sse(E, stds, L.data(), loglik, grad_std);
    if (grad_theta) for (int64_t i = 0; i < E.ntheta; ++i) grad_theta[i] = -g[(size_t)i];
    return 0;
}

// ... and its fp32 counterpart
static int loglik_f32(pinn_engine& E, const float* theta, const double* stds, double* loglik, float* grad_theta, double* grad_std) {
    const int K = (int)E.terms.size();
    std::vector<float> w(K);
    for (int k = 0; k < K; ++k) w[k] = (float)((double)E.terms[k].n_norm / (2.0 * stds[k] * stds[k]));
    if (upload_theta(E, theta, E.ntheta)) return 1;
    if (run_loss_grad(E, EvalRequest::host_entry(E, w.data()))) return 1;
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    loglik_from_sse(E, stds, E.hp_raw, loglik, grad_std);
    if (grad_theta)
        for (int64_t i = 0; i < E.ntheta; ++i) grad_theta[i] = -E.hp_out[i];
    return 0;
}

// float64 mode: K evaluations with one-hot weights (the double kernels evaluate whole problems; per-term statistics are not their hot path);
// row k of term_grads (K x P doubles) = d term_losses[k] / d theta
static int term_grads_f64(pinn_engine& E, const double* theta, double* term_losses, double* term_grads) {
    const int K = (int)E.terms.size();
    const int64_t p = E.ntheta;
    std::vector<double> w(K), L(K);
    for (int k = 0; k < K; ++k) {
        for (int j = 0; j < K; ++j) w[j] = (j == k) ? 1.0 : 0.0;
        if (f64_eval(E, theta, w.data(), L.data(), term_grads + (size_t)k * p)) return 1;
        if (term_losses) term_losses[k] = L[k];
    }
    return 0;
}

// fp32: K evaluations of one term each; row k of term_grads (K x P floats)
static int term_grads_f32(pinn_engine& E, const float* theta, double* term_losses, float* term_grads) {
    const int K = (int)E.terms.size();
    const int64_t p = E.ntheta;
    if (upload_theta(E, theta, p)) return 1;
    for (int k = 0; k < K; ++k) {
        EvalRequest rq = EvalRequest::host_entry(E, nullptr);
        rq.only_term = k;
        if (run_loss_grad(E, rq)) return 1;
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        std::memcpy(term_grads + (size_t)k * p, E.hp_out, sizeof(float) * p);
        if (term_losses) term_losses[k] = E.hp_raw[k] / (double)E.terms[k].n_norm;
    }
    return 0;
}

int pinn_loss_grad_device(pinn_handle h, const float* d_theta, const float* term_w, float* d_out, void* stream) {
    if (!h || !d_theta || !d_out) return fail("pinn_loss_grad_device: null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    int rc;
    {
        StreamScope on_callers(E, stream);
        EvalRequest rq = EvalRequest::device(d_theta, d_out, term_w);
        rq.timing = true;
        // float64 mode (r05): the double kernels between a device-side widening of theta and narrowing of [gradient | sums]
        rc = E.f64 ? f64_eval_from_device_f32(E, d_theta, term_w, d_out, true) : run_loss_grad(E, rq);
    }
    if (rc && g_err.empty()) return fail("pinn_loss_grad_device failed");
    E.timing_valid = (rc == 0) && E.timing_level >= 2;
    return rc;
}

int pinn_loss_grad_device_f64(pinn_handle h, const double* d_theta, const float* term_w, double* d_out, void* stream) {
    if (!h || !d_theta || !d_out) return fail("pinn_loss_grad_device_f64: null argument");
    pinn_engine& E = *h;
    if (!E.f64) return fail("pinn_loss_grad_device_f64: the handle is not in the float64 evaluation mode (pinn_set_option(h, \"precision\", \"f64\"))");
    DeviceScope scope(E.device);
    int rc;
    {
        StreamScope on_callers(E, stream);
        rc = f64_eval_from_device_f64(E, d_theta, term_w, d_out);
    }
    if (rc && g_err.empty()) return fail("pinn_loss_grad_device_f64 failed");
    return rc;
}

int pinn_loss_device(pinn_handle h, const float* d_theta, float* d_sums, void* stream) {
    if (!h || !d_theta || !d_sums) return fail("pinn_loss_device: null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    int rc;
    {
        StreamScope on_callers(E, stream);
        EvalRequest rq;                                  // loss-only: no gradient vector at all
        rq.d_theta = d_theta;
        rq.loss_only = true;
        rq.d_sums = d_sums;
        rc = E.f64 ? f64_eval_from_device_f32(E, d_theta, nullptr, d_sums, false) : run_loss_grad(E, rq);
    }
    if (rc && g_err.empty()) return fail("pinn_loss_device failed");
    return rc;
}

int pinn_group_launched_by(pinn_handle h, int group) {
    if (!h || group < 0 || group >= (int)h->groups.size()) return -1;
    return h->groups[group].launched_by;
}

// fp32: residual_k(set_k, theta) at every point of the installed set (pinn_residual[_f64])
static int residual_f32(pinn_engine& E, int term, const float* theta, float* r) {
    Term& T = E.terms[term];
    if (!T.d_pts) return fail("pinn_residual: term has no points");
    if (upload_theta(E, theta, E.ntheta)) return 1;
    pack_all(E);
    jit_take_launch_error();                             // (a stale message of an earlier call must not fail this one)
    if (residual_device(E, term)) return 1;
    if (plat_d2h(r, T.d_resid, sizeof(float) * T.n, E.stream)) return fail("D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    // a run-time specialised kernel whose (mode, activation) member could not be compiled at this, its first, launch leaves r unwritten
    { const std::string le = jit_take_launch_error(); if (!le.empty()) return fail("pinn_residual: " + le); }
    return 0;
}
// its device part: the term's residual at every point of its installed set into T.d_resid, with the parameters the packed weight images hold; queued
// on the stream, nothing is downloaded
extern "C++" int pe::residual_device(pinn_engine& E, int term) {
    Term& T = E.terms[term];
    if (T.resid_cap < T.n) {
        plat_free(T.d_resid);
        T.d_resid = (float*)plat_malloc(sizeof(float) * T.n);
        T.resid_cap = T.n;
        if (!T.d_resid) return fail("device allocation failed (residual)");
    }
    if (T.coupled >= 0) {
        Coupled& Cp = E.coupled[T.coupled];
        for (int gi : Cp.groups) {
            Group& G = E.groups[gi];
            pk::GroupArgs ga;
            narrow_to_term(ga, G.ga, slot_of_term(G, term));
            G.spec->launch(ga, pk::MODE_FWD, fwd_blocks(E, G.spec, ga.ntiles), E.stream);
        }
        if (!T.inodes.empty()) aux::launch_int_expr(int_expr_args(E, Cp, 0.f, T.d_resid), Cp.blocks, E.stream);
        else aux::launch_expr(expr_args(E, Cp, 0.f, T.d_resid), Cp.blocks, E.stream);
        return 0;
    }
    Group& G = E.groups[T.group];
    pk::GroupArgs ga;
    narrow_to_term(ga, G.ga, T.slot_in_group);
    ga.terms[0].out = T.d_resid;
    G.spec->launch(ga, pk::MODE_RESID, fwd_blocks(E, G.spec, ga.ntiles), E.stream);
    return 0;
}

// forward-only launch of one network on caller-supplied points with kernel `sp`: the jet channels land in E.d_phi_out as [C][n]
static int forward_jets(pinn_engine& E, int net, const pk::SpecInfo* sp, const float* theta, const float* pts, int64_t n) {
    const Net& N = E.nets[net];
    if (!E.netplans[net].spec) return fail("network is not used by any term");
    if (sp->family != E.netplans[net].spec->family || sp->PACKED != E.netplans[net].spec->PACKED)
        return fail("internal: forward kernel and the network's packed weight image disagree");
    if (upload_theta(E, theta, E.ntheta)) return 1;
    pack_all(E);
    jit_take_launch_error();                             // (clear: the check behind the launch below reports THIS launch)
    if (E.phi_cap < n || E.phi_chan < sp->C) {
        plat_sync(E.stream);
        plat_free(E.d_phi_pts); plat_free(E.d_phi_out);
        E.phi_cap = std::max(E.phi_cap, n);
        E.phi_chan = std::max(E.phi_chan, sp->C);
        E.d_phi_pts = (float*)plat_malloc(sizeof(float) * E.phi_cap * 8);
        E.d_phi_out = (float*)plat_malloc(sizeof(float) * E.phi_cap * E.phi_chan);
        if (!E.d_phi_pts || !E.d_phi_out) { E.phi_cap = 0; E.phi_chan = 0; return fail("device allocation failed (phi)"); }
    }
    if (!N.emb_idx.empty()) {                                  // periodic embedding: [arguments] -> [features] on the host (this entry point takes host points)
        const std::vector<float> feats = N.features(pts, n);
        plat_h2d(E.d_phi_pts, feats.data(), sizeof(float) * feats.size(), E.stream);
        plat_sync(E.stream);                                   // (feats is a pageable temporary)
    } else
        plat_h2d(E.d_phi_pts, pts, sizeof(float) * n * N.sizes[0], E.stream);
    pk::GroupArgs ga;
    std::memset(&ga, 0, sizeof ga);
    ga.packed = E.netplans[net].cur;
    ga.params = E.d_params;
    ga.nterms = 1;
    ga.nterms_total = 1;
    ga.act = N.act;
    ga.act_layers = N.act_layers;
    ga.terms[0].pts = E.d_phi_pts;
    ga.terms[0].dt = N.sizes[0];
    for (int i = 0; i < 4; ++i) ga.terms[0].imap[i] = i;
    ga.terms[0].N = (int)n;
    ga.terms[0].tile0 = 0;
    ga.terms[0].ntiles = (int)((n + sp->TP - 1) / sp->TP);
    ga.terms[0].out = E.d_phi_out;
    ga.ntiles = ga.terms[0].ntiles;
    if (sp->family == 3) {               // DGM: unpacked weights + point-major scratch rows for these points
        const size_t need = (size_t)sp->dgm_rows * (size_t)ga.ntiles * 64;
        if (need > E.phi_scr_cap) {
            plat_sync(E.stream);
            plat_free(E.d_phi_scr);
            E.d_phi_scr = (float*)plat_malloc(sizeof(float) * need);
            E.phi_scr_cap = E.d_phi_scr ? need : 0;
            if (!E.d_phi_scr) return fail("device allocation failed (phi scratch)");
        }
        ga.scratch = E.d_phi_scr;
        ga.dgm_modes = N.sizes[1];
        ga.dgm_npad = ga.ntiles * 64;
        ga.dgm_nparams = N.nparams();
    }
    sp->launch(ga, pk::MODE_FWD, fwd_blocks(E, sp, ga.ntiles), E.stream);
    { const std::string le = jit_take_launch_error(); if (!le.empty()) return fail("forward kernel: " + le); }
    return 0;
}

// fp32: d^order phi_net / dx_axes (order 0: the trial function itself) at n caller-supplied argument points [n][n_inputs]
static int net_eval_f32(const char* who, pinn_engine& E, int net, const float* theta, const float* pts, int64_t n, int order, const int* axes, float* out) {
    GemmScope gs(E.gemm);
    const Net& N = E.nets[net];
    if (!E.netplans[net].spec) return fail(std::string(who) + ": network is not used by any term");
    Slot sl;
    sl.net = net; sl.order = order; sl.lap = 0;
    for (int a = 0; a < MAX_DERIV_ORDER; ++a) sl.axes[a] = a < order ? axes[a] : 0;
    std::sort(sl.axes, sl.axes + order);
    unsigned need_first = 0, need_hi = 0;
    std::vector<std::pair<int, int>> need_pairs;
    if (slot_is_general(sl)) need_hi = GEN_FLAG | (unsigned)gen_set_id({slot_mi(sl)});      // mixed of order >= 3, orders 5-6: generated jet set
    else {
        for (int a = 0; a < order; ++a) need_first |= 1u << sl.axes[a];
        if (order >= 2) need_pairs.push_back({sl.axes[0], sl.axes[1]});
        if (order >= 3) need_hi = (unsigned)order << (4 * sl.axes[0]);
    }
    const pk::SpecInfo* sp = ensure_spec(N, need_first, need_pairs, need_hi, E.netplans[net].spec->family);
    if (!sp) return fail(std::string(who) + (order == 0 ? ": no value-only kernel" : ": no kernel carries this derivative") + " for this network shape (" + g_err + ")");
    const int ch = chan_of(*sp, sl);
    if (ch < 0) return fail("internal: derivative has no channel");
    if (forward_jets(E, net, sp, theta, pts, n)) return 1;
    if (plat_d2h(out, E.d_phi_out + (size_t)ch * n, sizeof(float) * n, E.stream)) return fail("D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

int pinn_set_sampler(pinn_handle h, int term, int kind, const float* lb, const float* ub, int64_t n, uint64_t seed) {
    if (!h) return fail("null handle");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (term < 0 || term >= (int)E.terms.size()) return fail("pinn_set_sampler: term index out of range");
    Term& T = E.terms[term];
    if (kind < 0 || kind > 3) return fail("pinn_set_sampler: kind must be 0 (fixed set), 1 (uniform), 2 (Latin hypercube) or 3 (Sobol)");
    if (kind == 3 && T.d_user > 8) return fail("pinn_set_sampler: the Sobol sampler covers up to 8 axes");
    if (kind == 0) { T.sampler = 0; return 0; }
    if (!lb || !ub || n <= 0) return fail("pinn_set_sampler: bounds and a positive point count are required");
    if (!T.d_lb) { T.d_lb = (float*)plat_malloc(sizeof(float) * 8); T.d_ub = (float*)plat_malloc(sizeof(float) * 8); }
    if (!T.d_lb || !T.d_ub) return fail("device allocation failed (sampler)");
    plat_h2d(T.d_lb, lb, sizeof(float) * T.d_user, E.stream);
    plat_h2d(T.d_ub, ub, sizeof(float) * T.d_user, E.stream);
    T.seed = (unsigned)(seed ^ (seed >> 32)) + 0x9E3779B9U * (unsigned)(term + 1);
    if (kind == 3 && seed == 0) T.seed = 0;              // un-randomised Sobol: the same design on every draw
    T.draws = 0;
    // allocate / size the term's point buffer through the normal path with a first draw
    std::vector<float> tmp((size_t)n * T.d_user, 0.f);
    if (set_points_impl(h, term, tmp.data(), n, 0, false)) return 1;
    T.sampler = kind;                                    // only now: every check and allocation above has succeeded
    aux::launch_sample(kind, user_pts(T), (int)(n * T.d_user), T.d_user, T.d_lb, T.d_ub, T.seed, T.draws++, E.stream);
    embed_points(E, T);
    eval_sources(E, T);
    if (E.f64 && f64_points_from_device(E, term)) return 1;       // float64 mode: the double copy follows every draw (r05)
    plat_sync(E.stream);
    return 0;
}

int pinn_set_point_data(pinn_handle h, int term, const float* data, int ndata, int64_t n) {
    if (!h || !data) return fail("pinn_set_point_data: null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (term < 0 || term >= (int)E.terms.size()) return fail("pinn_set_point_data: term index out of range");
    Term& T = E.terms[term];
    if (T.ndata == 0) return fail("pinn_set_point_data: the term's residual has no DATA channels");
    if (ndata != T.ndata) return fail("pinn_set_point_data: the term's residual uses " + std::to_string(T.ndata) + " data channel(s)");
    if (!T.d_pts || n != T.n) return fail("pinn_set_point_data: the term holds " + std::to_string(T.n) + " points (install the point set first)");
    if (T.sampler != 0) return fail("pinn_set_point_data: per-point data cannot follow a resampled point set");
    plat_sync(E.stream);
    if (T.data_cap < n) {
        plat_free(T.d_data);
        T.d_data = (float*)plat_malloc(sizeof(float) * (size_t)T.ndata * n);
        if (!T.d_data) return fail("device allocation failed (point data)");
        T.data_cap = n;
    }
    if (plat_h2d(T.d_data, data, sizeof(float) * (size_t)T.ndata * n, E.stream)) return fail("H2D copy of point data failed");
    T.data_n = n;
    eval_sources(E, T);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return f64_set_point_data(E, term, nullptr);         // (float64 mode: the double rows follow)
}
int pinn_set_point_data_f64(pinn_handle h, int term, const double* data, int ndata, int64_t n) {
    if (!h || !data || ndata <= 0 || n <= 0) return fail("pinn_set_point_data_f64: null argument / empty data");
    auto d32 = as<float>(data, (size_t)ndata * (size_t)n);
    if (pinn_set_point_data(h, term, d32.get(), ndata, n)) return 1;            // the fp32 kernels' rows (and every check)
    if (!h->f64) return 0;
    DeviceScope scope(h->device);
    return f64_set_point_data(*h, term, data);                                  // the float64 mode reads the observations as given
}

int pinn_set_point_weights(pinn_handle h, int term, const float* w, int64_t n) {
    if (!h) return fail("pinn_set_point_weights: null handle");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (term < 0 || term >= (int)E.terms.size()) return fail("pinn_set_point_weights: term index out of range");
    Term& T = E.terms[term];
    plat_sync(E.stream);
    if (w) {
        if (!T.d_pts || n != T.n) return fail("pinn_set_point_weights: the term holds " + std::to_string(T.n) + " points (install the point set first)");
        if (T.sampler != 0) return fail("pinn_set_point_weights: weights cannot follow a resampled point set");
        std::vector<float> s((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            if (!(w[i] >= 0.f)) return fail("pinn_set_point_weights: weights must be non-negative");
            s[i] = (float)std::sqrt((double)w[i] * (double)T.n_norm);
        }
        if (weights_reserve(E, term, n)) return 1;
        if (plat_h2d(T.d_pw, s.data(), sizeof(float) * (size_t)n, E.stream)) return fail("H2D copy of point weights failed");
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    }
    weights_written(E, term, w ? n : 0);
    return 0;
}
extern "C++" int pe::weights_reserve(pinn_engine& E, int term, int64_t n) {
    Term& T = E.terms[term];
    if (T.pw_cap < n) {
        plat_free(T.d_pw);
        T.d_pw = (float*)plat_malloc(sizeof(float) * (size_t)n);
        if (!T.d_pw) { T.pw_cap = 0; return fail("device allocation failed (point weights)"); }
        T.pw_cap = n;
    }
    return 0;
}
// the term's weight buffer holds the factors of its current n points (n == 0: back to the plain mean)
extern "C++" void pe::weights_written(pinn_engine& E, int term, int64_t n) {
    Term& T = E.terms[term];
    T.pw_n = n;
    if (T.coupled < 0) retile(E, T.group);
    else for (int gi : E.coupled[T.coupled].groups) retile(E, gi);
}

int pinn_get_points(pinn_handle h, int term, float* pts, int64_t n) {
    if (!h || !pts) return fail("pinn_get_points: null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (term < 0 || term >= (int)E.terms.size()) return fail("pinn_get_points: term index out of range");
    Term& T = E.terms[term];
    if (!T.d_pts || n != T.n) return fail("pinn_get_points: the term holds " + std::to_string(T.n) + " points");
    if (plat_d2h(pts, user_pts(T), sizeof(float) * (size_t)n * T.d_user, E.stream)) return fail("D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

extern "C++" int pe::replan_gemm(pinn_engine& E, int mode) {
    if (mode == E.gemm) return 0;
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    const int prev = E.gemm;
    free_plan(E);
    E.gemm = mode;
    int rc = build_plan(E);
    if (rc) {                                            // e.g. the other mode's kernel of a run-time specialised shape failed to compile: go back
        const std::string why = g_err;
        free_plan(E);
        E.gemm = prev;
        if (build_plan(E)) return fail("pinn_set_option: the kernel plan could not be rebuilt (" + why + "); the handle is unusable");
        g_err = why;
    }
    for (size_t t = 0; t < E.terms.size(); ++t)
        if (E.terms[t].d_pts && E.terms[t].n > 0 && term_installed(E, (int)t)) return 1;
    for (size_t t = 0; t < E.terms.size(); ++t) {        // per-point data feeds the source channels: re-evaluate where installed
        Term& T = E.terms[t];
        if (T.ndata > 0 && T.data_n == T.n && T.n > 0) eval_sources(E, T);
    }
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return rc;
}

// ---- "gemm" = "auto": WHEN to leave the split-bf16 products ----
// The rule is a MEASUREMENT, not a heuristic: at the current parameters the gradient is evaluated with both GEMM arithmetics of the handle
// (the split-bf16 products and their fp32-MFMA twin: an fmaf chain per product) and compared,
//     delta = |grad(split) - grad(fp32)|_2 / |grad(fp32)|_2 ,
// which IS the split products' arithmetic error at this iterate up to the twin's own (2 - 7 x smaller, profiles/r05_theta_variants_ab.txt
// section F).  "split" is kept while delta <= 1e-5 (the north star's tolerance), "fp32" runs above; an fp32 handle goes back when delta has
// fallen under 3e-6.  At initialisation delta ~ 2e-7; on the trained fixtures (cfg2 after 2,000 / 6,000 Adam steps) 1e-5 / 4e-3: the policy leaves
// the fast products exactly where parity starts to depend on them.  Cost: two evaluations and at most two re-plans (milliseconds) per check; checks
// run at the end of a pinn_adam_steps call (loop path) and inside pinn_loss_grad with a gradient, at most once per GEMM_CHECK_EVERY optimiser
// steps / evaluations, never inside a resident loop.  Also reported: rho = |grad|_2 / sqrt(L) ("grad_health"): |grad| <= 2 sqrt(L) J_rms, so rho
// against its value at initialisation is the cancellation factor of the gradient sum — when it has fallen by ~1e3 no fp32 arithmetic holds 1e-3
// any more and "precision" = "f64" is the remedy (the glue's precision policy puts Float64 parameters there from the start).
constexpr double GEMM_DELTA_UP = 1e-5, GEMM_DELTA_DOWN = 3e-6;
constexpr long long GEMM_CHECK_EVERY = 1000;
extern "C++" void pe::measure_grad_health(pinn_engine& E, const float* grad_and_sums, const float* term_w) {
    const int K = (int)E.terms.size();
    const int64_t P = E.ntheta;
    double g2 = 0.0, L = 0.0;
    for (int64_t i = 0; i < P; ++i) g2 += (double)grad_and_sums[i] * (double)grad_and_sums[i];
    for (int k = 0; k < K; ++k) L += (term_w ? (double)term_w[k] : 1.0) * (double)grad_and_sums[P + k] / (double)E.terms[k].n_norm;
    E.grad_health = L > 0.0 ? std::sqrt(g2) / std::sqrt(L) : -1.0;
}
// the policy's check at the device-resident parameters d_theta (clock: `now` optimiser steps / evaluations)
extern "C++" int pe::gemm_auto_check(pinn_engine& E, const float* d_theta, const float* term_w, long long now) {
    if (!E.gemm_auto || E.f64 || E.comm) return 0;
    if (E.gemm_check_t >= 0 && now - E.gemm_check_t < GEMM_CHECK_EVERY && now >= E.gemm_check_t) return 0;
    bool has_twin = false;
    for (const NetPlan& NP : E.netplans) has_twin = has_twin || (NP.spec && NP.spec->family == 2 && NP.spec->twin);
    if (!has_twin) return 0;
    const int64_t P = E.ntheta;
    const int start = E.gemm;
    std::vector<float> ga((size_t)P), gb((size_t)P);
    if (run_loss_grad(E, EvalRequest::device(d_theta, E.d_out, term_w))) return 1;
    if (plat_d2h(ga.data(), E.d_out, sizeof(float) * P, E.stream) || plat_sync(E.stream)) return fail("D2H copy failed");
    if (replan_gemm(E, start == pk::GEMM_SPLIT ? pk::GEMM_FP32 : pk::GEMM_SPLIT)) return 1;
    if (E.gemm == start) return 0;                       // (the twin could not be built: the handle stays where it was)
    if (run_loss_grad(E, EvalRequest::device(d_theta, E.d_out, term_w))) return 1;
    if (plat_d2h(gb.data(), E.d_out, sizeof(float) * P, E.stream) || plat_sync(E.stream)) return fail("D2H copy failed");
    const std::vector<float>& gs = start == pk::GEMM_SPLIT ? ga : gb;      // split / fp32 gradients
    const std::vector<float>& gf = start == pk::GEMM_SPLIT ? gb : ga;
    double d2 = 0.0, n2 = 0.0;
    for (int64_t i = 0; i < P; ++i) { const double d = (double)gs[(size_t)i] - (double)gf[(size_t)i]; d2 += d * d; n2 += (double)gf[(size_t)i] * (double)gf[(size_t)i]; }
    E.gemm_delta = n2 > 0.0 ? std::sqrt(d2 / n2) : 0.0;
    E.gemm_check_t = now;
    const int want = (start == pk::GEMM_SPLIT) ? (E.gemm_delta > GEMM_DELTA_UP ? pk::GEMM_FP32 : pk::GEMM_SPLIT)
                                               : (E.gemm_delta < GEMM_DELTA_DOWN ? pk::GEMM_SPLIT : pk::GEMM_FP32);
    return replan_gemm(E, want);
}

int pinn_set_option(pinn_handle h, const char* name, const char* value) {
    if (!h || !name || !value) return fail("pinn_set_option: null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    const std::string k = name, v = value;
    if (k == "gemm") {
        if (v == "split") { E.gemm_auto = false; return replan_gemm(E, pk::GEMM_SPLIT); }
        if (v == "fp32") { E.gemm_auto = false; return replan_gemm(E, pk::GEMM_FP32); }
        if (v == "auto") { E.gemm_auto = true; E.gemm_check_t = -1; return 0; }
        return fail("pinn_set_option: gemm must be \"split\", \"fp32\" or \"auto\"");
    }
    if (k == "precision") {
        if (v == "f64") return f64_enable(E);
        if (v == "f32") { plat_sync(E.stream); f64_destroy(E); return 0; }
        return fail("pinn_set_option: precision must be \"f32\" or \"f64\"");
    }
    if (k == "persistent") {
        if (v == "on" || v == "1") { E.persistent = true; return 0; }
        if (v == "off" || v == "0") { E.persistent = false; return 0; }
        return fail("pinn_set_option: persistent must be \"on\" or \"off\"");
    }
    if (k == "integral_nodes") {
        // Gauss-Legendre nodes per integral node.  A live handle is RE-PLANNED: the installed point sets of its integral terms stay, their
        // site sets are rebuilt for the new rule (buffers grow as needed); optimiser state, samplers and weights stay
        char* end = nullptr;
        const long q = std::strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || q < 2 || q > aux::INT_MAX_Q) return fail("pinn_set_option: integral_nodes must be an integer in 2.." + std::to_string(aux::INT_MAX_Q) + ", not \"" + v + "\"");
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        for (auto& T : E.terms)
            if (!T.inodes.empty() && T.d_pts && T.n > 0 && T.n * (1 + (int64_t)T.inodes.size() * q) * std::max(T.d, aux::INT_MAX_C) >= (int64_t)1 << 31)
                return fail("pinn_set_option: integral_nodes = " + std::to_string(q) + " makes a site set of " + std::to_string(T.n * (1 + (int64_t)T.inodes.size() * q)) +
                            " sites, more than one launch group takes; the handle keeps " + std::to_string(E.int_q));
        bool any = false;
        for (auto& T : E.terms) any = any || !T.inodes.empty();
        if (!any) { E.int_q = (int)q; return 0; }
        // allocate first, commit after: a failed allocation of a site buffer leaves the handle exactly as it was
        std::vector<float*> nbuf(E.terms.size(), nullptr);
        for (size_t t = 0; t < E.terms.size(); ++t) {
            Term& T = E.terms[t];
            if (T.inodes.empty() || !T.d_pts || T.n <= 0) continue;
            const int64_t new_sites = 1 + (int64_t)T.inodes.size() * q;
            if (T.n * new_sites <= T.pts_cap * (int64_t)T.sites()) continue;      // the buffer (pts_cap points at the current rule) has room
            nbuf[t] = (float*)plat_malloc(sizeof(float) * (size_t)T.n * new_sites * T.d);
            if (!nbuf[t]) {
                for (float* b : nbuf) plat_free(b);
                return fail("pinn_set_option: device allocation failed (site set for integral_nodes = " + std::to_string(q) + "); the handle keeps " + std::to_string(E.int_q));
            }
        }
        if (upload_int_rule(E, (int)q)) {
            for (float* b : nbuf) plat_free(b);
            if (E.d_int_xi) upload_int_rule(E, E.int_q);
            return 1;
        }
        E.int_q = (int)q;
        for (size_t t = 0; t < E.terms.size(); ++t) {
            Term& T = E.terms[t];
            if (T.inodes.empty()) continue;
            const int64_t room = T.pts_cap * (int64_t)T.sites();          // sites the current buffer holds
            T.int_q = E.int_q;
            if (!T.d_pts || T.n <= 0) { T.pts_cap = 0; continue; }        // (no set installed: pinn_set_points sizes the buffer)
            if (nbuf[t]) {
                plat_d2d(nbuf[t], T.d_pts, sizeof(float) * (size_t)T.n * T.d, E.stream);      // block 0: the collocation points
                plat_sync(E.stream);
                plat_free(T.d_pts);
                T.d_pts = nbuf[t];
                T.pts_cap = T.n;
            } else T.pts_cap = room / T.sites();                          // points the kept buffer holds at the new rule (>= n)
            expand_sites(E, T);
            if (term_installed(E, (int)t)) return 1;
        }
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        return 0;
    }
    if (k == "derivative") {
        if (v == "stencil") return f64_stencil_enable(E, true);
        if (v == "exact") return E.f64 ? f64_stencil_enable(E, false) : 0;
        return fail("pinn_set_option: derivative must be \"exact\" or \"stencil\"");
    }
    if (k == "lbfgs_chunk") {
        char* end = nullptr;
        const long q = std::strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || q < 1 || q > 64) return fail("pinn_set_option: lbfgs_chunk must be an integer in 1..64, not \"" + v + "\"");
        E.lbfgs_chunk = (int)q;
        return 0;
    }
    if (k == "nuts_chunk") {
        char* end = nullptr;
        const long q = std::strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || q < 1 || q > 64) return fail("pinn_set_option: nuts_chunk must be an integer in 1..64, not \"" + v + "\"");
        E.nuts_chunk = (int)q;
        return 0;
    }
    return fail("pinn_set_option: unknown option \"" + k + "\" (known: gemm, precision, persistent, derivative, integral_nodes, lbfgs_chunk, nuts_chunk)");
}

int pinn_get_option(pinn_handle h, const char* name, char* buf, int64_t buflen) {
    if (!h || !name || !buf || buflen <= 0) return fail("pinn_get_option: bad argument");
    const std::string k = name;
    if (k == "gemm") { std::snprintf(buf, (size_t)buflen, h->gemm_auto ? "auto(%s)" : "%s", h->gemm == pk::GEMM_FP32 ? "fp32" : "split"); return 0; }
    if (k == "grad_health") { std::snprintf(buf, (size_t)buflen, "%.9g", h->grad_health); return 0; }
    if (k == "gemm_delta") { std::snprintf(buf, (size_t)buflen, "%.9g", h->gemm_delta); return 0; }
    if (k == "precision") { std::snprintf(buf, (size_t)buflen, "%s", h->f64 ? "f64" : "f32"); return 0; }
    if (k == "persistent") { std::snprintf(buf, (size_t)buflen, "%s", h->persistent ? "on" : "off"); return 0; }
    if (k == "integral_nodes") { std::snprintf(buf, (size_t)buflen, "%d", h->int_q); return 0; }
    if (k == "derivative") { std::snprintf(buf, (size_t)buflen, "%s", pe::f64_stencil_on(*h) ? "stencil" : "exact"); return 0; }
    if (k == "eval_path") { std::snprintf(buf, (size_t)buflen, "%s", h->eval_path == 2 ? "one launch" : (h->eval_path == 1 ? "stand-alone kernels" : "none")); return 0; }
    if (k == "f64_path") { std::snprintf(buf, (size_t)buflen, "%s", pe::f64_path(*h)); return 0; }
    if (k == "f64_affine") { std::snprintf(buf, (size_t)buflen, "%d", pe::f64_affine_terms(*h)); return 0; }       // terms on the affine-residual fast path
    if (k == "f64_merged") { std::snprintf(buf, (size_t)buflen, "%d", pe::f64_merged(*h)); return 0; }          // merged launches of the last float64 evaluation
    if (k == "f64_chunks") { std::snprintf(buf, (size_t)buflen, "%d", pe::f64_chunks(*h)); return 0; }          // chunks of the largest point set in the last float64 call
    if (k == "adam_path") { std::snprintf(buf, (size_t)buflen, "%s", h->adam_path == 2 ? "persistent" : (h->adam_path == 1 ? "loop" : "none")); return 0; }
    if (k == "lbfgs_chunk") { std::snprintf(buf, (size_t)buflen, "%d", h->lbfgs_chunk); return 0; }
    if (k == "nuts_chunk") { std::snprintf(buf, (size_t)buflen, "%d", h->nuts_chunk); return 0; }
    if (k == "ens_passes") { std::snprintf(buf, (size_t)buflen, "%d", pe::ens_counter(*h, 0)); return 0; }            // jet passes of the last pinn_derivative_ensemble call
    if (k == "ens_point_passes") { std::snprintf(buf, (size_t)buflen, "%d", pe::ens_counter(*h, 1)); return 0; }      // ... its point passes
    if (k == "ens_scratch_passes") { std::snprintf(buf, (size_t)buflen, "%d", pe::ens_counter(*h, 2)); return 0; }    // ... its jet passes with the images in device scratch
    if (k == "cub_ms") {     // phases of the last pinn_cubature_refine under pinn_set_timing level 2: nodes, evaluation, estimate, plan + read-back, split, emit (ms)
        const float* ms = pe::cub_phase_ms(*h);
        std::snprintf(buf, (size_t)buflen, "%.4f %.4f %.4f %.4f %.4f %.4f", ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
        return 0;
    }
    return fail("pinn_get_option: unknown option \"" + k + "\" (known: gemm, precision, persistent, derivative, integral_nodes, lbfgs_chunk, nuts_chunk, grad_health, gemm_delta, adam_path, eval_path, f64_path, f64_merged, f64_chunks, f64_affine, ens_passes, ens_point_passes, ens_scratch_passes, cub_ms)");
}

int pinn_set_timing(pinn_handle h, int level, int group) {
    if (!h) return fail("pinn_set_timing: null handle");
    if (level < 0 || level > 2) return fail("pinn_set_timing: level must be 0, 1 or 2");
    if (group < -1 || group >= (int)h->groups.size()) return fail("pinn_set_timing: group index out of range");
    h->timing_level = level; h->timing_group = group;
    h->timing_valid = false;
    for (auto& G : h->groups) G.timed = false;
    return 0;
}

int pinn_last_timing(pinn_handle h, float* kernel_ms, float* total_ms) {
    if (!h) return fail("null handle");
    if (!h->timing_valid) return fail("no timing available: switch the phase events on (pinn_set_timing(h, 2, -1)), then call pinn_loss_grad");
    plat_event_sync(h->ev3);
    if (kernel_ms) *kernel_ms = plat_event_ms(h->ev1, h->ev2);
    if (total_ms) *total_ms = plat_event_ms(h->ev0, h->ev3);
    return 0;
}

int pinn_num_groups(pinn_handle h) { return h ? (int)h->groups.size() : -1; }

#ifdef PINN_STAMP
// profiling build only: the four phase-tick sums of the last persistent training launch (pinn_train.hpp: TRAIN_STAMP)
int pinn_debug_train_stamps(pinn_handle h, unsigned long long* out4) {
    if (!h || !h->d_bar || !out4) return -1;
    plat_sync(h->stream);
    plat_d2h(out4, h->d_bar + 4, sizeof(unsigned long long) * 4, h->stream);
    plat_sync(h->stream);
    return 0;
}
// profiling build only (tools/stamp_profile.sh): raw read-back of one workgroup's gradient slab incl. the stamp tail
int pinn_debug_slab(pinn_handle h, int group, int blk, float* dst, int64_t n) {
    if (!h || group < 0 || group >= (int)h->groups.size()) return -1;
    Group& G = h->groups[group];
    if (blk < 0) return G.blocks;
    if (blk == (1 << 30)) return G.spec->SLAB;
    if (blk >= G.blocks || n > G.spec->SLAB) return -1;
    plat_sync(h->stream);
    plat_d2h(dst, G.d_slabs + (size_t)blk * G.spec->SLAB + (G.spec->SLAB - n), sizeof(float) * n, h->stream);
    plat_sync(h->stream);
    return 0;
}
#endif

int pinn_group_timing(pinn_handle h, int group, float* ms, int64_t* points, int* channels, int* tiles) {
    if (!h) return fail("null handle");
    if (group < 0 || group >= (int)h->groups.size()) return fail("pinn_group_timing: group index out of range");
    Group& G = h->groups[group];
    if (ms) *ms = -1.f;                   // not timed in the last evaluation (pinn_set_timing)
    if (G.timed) {
        plat_event_sync(G.ev_b);
        if (ms) *ms = plat_event_ms(G.ev_a, G.ev_b);
    }
    int64_t n = 0;
    for (int t : G.terms) n += h->terms[t].n;
    if (points) *points = n;
    if (channels) *channels = G.spec->C;
    if (tiles) *tiles = G.ga.ntiles;
    return 0;
}

int pinn_describe(pinn_handle h, char* buf, int64_t buflen) {
    if (!h || !buf || buflen <= 0) return fail("pinn_describe: bad argument");
    std::ostringstream os;
    os << "backend=" << plat_name() << " cus=" << h->ncu << " ntheta=" << h->ntheta << " terms=" << h->terms.size()
       << (h->f64 ? " precision=f64 (pinn_loss_grad*, pinn_lbfgs evaluate in double — matrix-pipe tile kernels where instantiated, one lane per point elsewhere; the plan below serves the fp32 entry points)" + pe::f64_describe(*h) : std::string())
       << (h->lbfgs ? " lbfgs=resident(history=" + std::to_string(h->lbfgs_history) + ",chunk=" + std::to_string(h->lbfgs_chunk) + ")" : std::string())
       << (h->bfgs ? " bfgs=resident(P=" + std::to_string(pe::bfgs_params(*h)) + ",chunk=" + std::to_string(h->lbfgs_chunk) + ")" : std::string()) << "\n";
    for (size_t n = 0; n < h->netplans.size(); ++n)
        if (h->netplans[n].spec && h->netplans[n].spec->family != 3)
            os << "net " << n << " weights=packed image (k_pack per evaluation)"
               << " gemm=" << (h->netplans[n].spec->BFX ? (h->netplans[n].spec->BFX_DW ? "split-bf16(fwd,dA,dW)" : "split-bf16(fwd,dA)") : "fp32") << "\n";
    for (size_t g = 0; g < h->groups.size(); ++g) {
        const Group& G = h->groups[g];
        os << "group " << g << (G.kind == 1 ? (G.use_rec ? " [coupled fwd/gradin, records in HBM]" : " [coupled fwd/gradin]") :
                                (G.kind == 2 ? " [coupled tail: forward + tape + reverse in one launch]" : "")) << " net=" << G.net << " kernel=" << spec_name(*G.spec) << (G.ga.act == pk::ACT_SWISH ? "+swish" : "") << " tiles=" << G.ga.ntiles << " blocks=" << G.blocks << " terms=";
        for (int t : G.terms) {
            os << t;
            if (!h->terms[t].inodes.empty()) os << "+integral(" << h->terms[t].int_q << ")";       // its tiles are the term's site set
            os << ",";
        }
        if (G.chain_to >= 0) os << " slabs=" << (G.blocks <= h->groups[G.chain_to].blocks ? "chained onto group " : "own (more workgroups than group ") << G.chain_to << (G.blocks <= h->groups[G.chain_to].blocks ? "" : ")");
        if (G.merged >= 0 && h->merged[G.merged].tail == (int)g) os << " launch=merged into group " << h->merged[G.merged].head << "'s (one persistent kernel walks both tile lists)";
        os << "\n";
    }
    for (size_t t = 0; t < h->terms.size(); ++t) {
        const Term& T = h->terms[t];
        if (T.coupled >= 0) continue;
        os << "term " << t << ": tape ops=" << T.tape_ops.size() << " of " << T.ops.size() << ", sources=" << T.src_root.size()
           << " (" << T.src_prog.size() << " coordinate-only ops evaluated per point set)" << (T.linear ? ", affine residual: no tape interpreter" : "") << "\n";
    }
    std::string s = os.str();
    std::snprintf(buf, (size_t)buflen, "%s", s.c_str());
    return 0;
}

}  // extern "C"

// =================================================================================================
// The float / double twins of the host entry points (pinn_X, pinn_X_f64).  One rule for all of them: T, the ABI's element type, is the
// caller's; the evaluation runs in the HANDLE'S precision — the fp32 kernels (the *_f32 bodies above) or, in float64 mode, the double
// kernels (f64.cpp).  One body per pair: the arguments are checked once (null pointers, index ranges, theta length) before the handle's
// device is made current; where T is not the handle's type, the arrays are converted at this boundary (As), their lengths taken from
// the engine.  The reference's closures compute in eltype(theta) (src/pinn_types.jl:88-90, 445-482; src/discretize.jl:432-449).
// =================================================================================================
namespace {

template <class T> int loss_grad_twin(const char* who, pinn_handle h, const T* theta, int64_t p, const T* term_w, double* term_losses, T* grad) {
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, K = E.terms.size();
    if (E.f64) {
        auto th = as<double>(theta, P); auto w = as<double>(term_w, K); auto g = as<double>(grad, P);
        return f64_eval(E, th.get(), w.get(), term_losses, g.get()) ? 1 : g.put();
    }
    auto th = as<float>(theta, P); auto w = as<float>(term_w, K); auto g = as<float>(grad, P);
    return loss_grad_f32(E, th.get(), w.get(), term_losses, g.get()) ? 1 : g.put();
}

template <class T> int loglik_twin(const char* who, pinn_handle h, const T* theta, int64_t p, const double* stds, double* loglik, T* grad_theta, double* grad_std) {
    if (!h || !theta || !stds || !loglik) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    for (size_t k = 0; k < E.terms.size(); ++k)
        if (!(stds[k] > 0.0)) return fail(std::string(who) + ": standard deviations must be positive");
    DeviceScope scope(E.device);
    if (E.f64) {
        auto th = as<double>(theta, (size_t)p); auto g = as<double>(grad_theta, (size_t)p);
        return loglik_f64(E, th.get(), stds, loglik, g.get(), grad_std) ? 1 : g.put();
    }
    auto th = as<float>(theta, (size_t)p); auto g = as<float>(grad_theta, (size_t)p);
    return loglik_f32(E, th.get(), stds, loglik, g.get(), grad_std) ? 1 : g.put();
}

template <class T> int term_grads_twin(const char* who, pinn_handle h, const T* theta, int64_t p, double* term_losses, T* term_grads) {
    if (!h || !theta || !term_grads) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, KP = E.terms.size() * P;
    if (E.f64) {
        auto th = as<double>(theta, P); auto g = as<double>(term_grads, KP);
        return term_grads_f64(E, th.get(), term_losses, g.get()) ? 1 : g.put();
    }
    auto th = as<float>(theta, P); auto g = as<float>(term_grads, KP);
    return term_grads_f32(E, th.get(), term_losses, g.get()) ? 1 : g.put();
}

template <class T> int residual_twin(const char* who, pinn_handle h, int term, const T* theta, int64_t p, T* r) {
    if (!h || !theta || !r) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (term < 0 || term >= (int)E.terms.size()) return fail(std::string(who) + ": term index out of range");
    if (check_theta(E, who, p)) return 1;
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, n = (size_t)E.terms[term].n;
    if (E.f64) {
        auto th = as<double>(theta, P); auto o = as<double>(r, n);
        return f64_residual(E, term, th.get(), o.get()) ? 1 : o.put();
    }
    auto th = as<float>(theta, P); auto o = as<float>(r, n);
    return residual_f32(E, term, th.get(), o.get()) ? 1 : o.put();
}

// phi (order 0) and its derivatives at n points of the dependent variable's arguments, pts [n][n_inputs]
template <class T> int net_eval_twin(const char* who, pinn_handle h, int net, const T* theta, int64_t p, const T* pts, int64_t n, int order, const int* axes, T* out) {
    if (!h || !theta || !pts || !out) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (net < 0 || net >= (int)E.nets.size()) return fail(std::string(who) + ": net index out of range");
    if (n <= 0) return fail(std::string(who) + ": n must be positive");
    if (order < 0 || order > MAX_DERIV_ORDER || (order > 0 && !axes)) return fail(std::string(who) + ": order must be 0..6 (with `order` axes)");
    const Net& N = E.nets[net];
    if (order > 0 && !N.emb_idx.empty())
        return fail(std::string(who) + ": not available for a network behind a periodic input embedding (use pinn_residual on a term that carries the derivative)");
    for (int a = 0; a < order; ++a)
        if (axes[a] < 0 || axes[a] >= N.n_inputs()) return fail(std::string(who) + ": axis out of range");
    if (check_theta(E, who, p)) return 1;
    DeviceScope scope(E.device);
    const size_t P = (size_t)p, X = (size_t)n * N.n_inputs();
    if (E.f64) {
        auto th = as<double>(theta, P); auto x = as<double>(pts, X); auto o = as<double>(out, (size_t)n);
        return f64_net_eval(E, net, th.get(), x.get(), n, order, axes, o.get()) ? 1 : o.put();
    }
    auto th = as<float>(theta, P); auto x = as<float>(pts, X); auto o = as<float>(out, (size_t)n);
    return net_eval_f32(who, E, net, th.get(), x.get(), n, order, axes, o.get()) ? 1 : o.put();
}

}  // namespace

extern "C" {

int pinn_loss_grad(pinn_handle h, const float* theta, int64_t p, const float* term_w, double* term_losses, float* grad) {
    return loss_grad_twin(__func__, h, theta, p, term_w, term_losses, grad);
}
int pinn_loss_grad_f64(pinn_handle h, const double* theta, int64_t p, const double* term_w, double* term_losses, double* grad) {
    return loss_grad_twin(__func__, h, theta, p, term_w, term_losses, grad);
}
int pinn_loglik_grad(pinn_handle h, const float* theta, int64_t p, const double* stds, double* loglik, float* grad_theta, double* grad_std) {
    return loglik_twin(__func__, h, theta, p, stds, loglik, grad_theta, grad_std);
}
int pinn_loglik_grad_f64(pinn_handle h, const double* theta, int64_t p, const double* stds, double* loglik, double* grad_theta, double* grad_std) {
    return loglik_twin(__func__, h, theta, p, stds, loglik, grad_theta, grad_std);
}
int pinn_term_grads(pinn_handle h, const float* theta, int64_t p, double* term_losses, float* term_grads) {
    return term_grads_twin(__func__, h, theta, p, term_losses, term_grads);
}
int pinn_term_grads_f64(pinn_handle h, const double* theta, int64_t p, double* term_losses, double* term_grads) {
    return term_grads_twin(__func__, h, theta, p, term_losses, term_grads);
}
int pinn_residual(pinn_handle h, int term, const float* theta, int64_t p, float* r) { return residual_twin(__func__, h, term, theta, p, r); }
int pinn_residual_f64(pinn_handle h, int term, const double* theta, int64_t p, double* r) { return residual_twin(__func__, h, term, theta, p, r); }
int pinn_phi(pinn_handle h, int net, const float* theta, int64_t p, const float* pts, int64_t n, float* out) {
    return net_eval_twin(__func__, h, net, theta, p, pts, n, 0, nullptr, out);
}
int pinn_phi_f64(pinn_handle h, int net, const double* theta, int64_t p, const double* pts, int64_t n, double* out) {
    return net_eval_twin(__func__, h, net, theta, p, pts, n, 0, nullptr, out);
}
int pinn_derivative(pinn_handle h, int net, const float* theta, int64_t p, const float* pts, int64_t n, int order, const int* axes, float* out) {
    return net_eval_twin(__func__, h, net, theta, p, pts, n, order, axes, out);
}
int pinn_derivative_f64(pinn_handle h, int net, const double* theta, int64_t p, const double* pts, int64_t n, int order, const int* axes, double* out) {
    return net_eval_twin(__func__, h, net, theta, p, pts, n, order, axes, out);
}

}  // extern "C"

#ifdef PINN_EMU
// test hook of the emulation build only (never part of libpinn_hip.so): the device Sobol' bit generator
extern "C" unsigned pinn_emu_sobol_bits(unsigned index, int axis) { return aux::sobol_bits(index, axis); }
#endif
