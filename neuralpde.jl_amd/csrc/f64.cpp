// f64.cpp — host side of the float64 evaluation mode (pinn_set_option(h, "precision", "f64"); kernels: pinn_kernels4.hpp).
//
// The reference evaluates in Float64 by default (src/discretize.jl:432-449: `init_params` are converted to Float64 unless the chain is
// given Float32 parameters; the EltypeAdaptor then fixes the points' eltype, src/eltype_matching.jl:8-10).  This mode is that arithmetic
// on the device, for callers that need more than fp32 can give at trained parameters: `pinn_loss_grad_f64`
// evaluates natively, `pinn_loss_grad` converts at the boundary, `pinn_lbfgs` iterates on the float64 objective.
// Scope: Dense chains with tanh / sigmoid / sin, equations of one or SEVERAL dependent variables (systems: up to 6 networks per equation, all
// with the same number of inputs), derivative orders <= 2 in 1-3 inputs (1-D: <= 4; 4-D: first and pure second derivatives), PDE parameters
// (param_estim), quadrature weights, per-point DATA channels, device samplers, periodic input embeddings (r06: feature rows in double); no DGM networks.  Anything else fails at pinn_set_option with a message — the fp32 plan of the handle stays usable.
//
// This unit is the EVALUATION: launch building, launch geometry, grouping, f64_eval_device and its phases, the per-point closures, the
// device-entry adapters.  State, kernel look-up and point sets: f64_setup.cpp; the stencil validation mode: f64_stencil.cpp; the resident
// optimiser loop: f64_adam.cpp; what they share: f64_internal.hpp.
#include "f64_internal.hpp"

namespace pe {

// everything of F64Args that does not depend on the evaluation (theta, weights, mode, chunk): networks, scratch row numbering, tape, slots
int f64_build(pinn_engine& E, const F64Term& F, int dt, const std::map<int, std::vector<int>>* inmap, const F64Switches& sw, F64Launch& L) {
    L.sw = sw;
    pk::F64Args& a = L.a;
    std::memset(&a, 0, sizeof a);
    a.data = F.ndata > 0 ? F.d_data : nullptr;
    a.lin = f64_lin_ptr(F);
    a.pts = F.d_pts;
    a.N = (int)F.n; a.dt = dt;
    a.nnets = (int)F.nets.size();
    a.C = F.k->C;
    for (int i = 0; i < 8; ++i) a.first_ch[i] = F.k->first_ch[i];
    int rows = 0, ent = 0;
    L.acls = pk::ACLS_A;
    L.mfma = F.km && !sw.no_mfma;
    L.sliced = L.mfma && F.km->sliced != 0;
    a.use_ceff = L.sliced ? 1 : 0;
    for (int ni = 0; ni < a.nnets; ++ni) {
        const Net& N = E.nets[F.nets[ni]];
        pk::F64Net& n = a.net[ni];
        n.d = N.sizes[0];
        if (input_binding(E, F.nets[ni], inmap, n.imap) != n.d) return fail("precision f64: inmap length differs from the network's input count");
        n.nl = (int)N.sizes.size() - 1;
        int o = N.theta_off;
        for (int l = 0; l < n.nl; ++l) {
            n.sizes[l] = N.sizes[l];
            n.woff[l] = o;
            n.boff[l] = o + N.sizes[l + 1] * N.sizes[l];
            o = n.boff[l] + N.sizes[l + 1];
        }
        n.sizes[n.nl] = N.sizes[n.nl];
        n.act = N.act;
        n.act_layers = N.act_layers;
        n.ceff = 1;
        for (int sl = 0; sl < F.nslots; ++sl) if (F.slot_net[sl] == ni) n.ceff = std::max(n.ceff, F.slot_chan[sl] + 1);
        if (sw.full_channels) n.ceff = a.C;              // (A/B, tests)
        if (pk::act_class(N.act) != pk::ACLS_A) L.acls = pk::act_class(N.act);
        n.theta0 = N.theta_off; n.nparams = N.nparams(); n.ent0 = ent;
        ent += n.nparams;
        n.tp0 = a.tp_p;                                       // (running column count of the tile partial sums)
        a.tp_p += (n.d + 1) * N.sizes[1] + N.sizes[n.nl - 1] + 1;
        // scratch rows: per hidden layer record / post-activation jets / dZ, then this network's seeds
        const int LH = n.nl - 1;
        for (int l = 0; l < LH; ++l) { n.r_rec[l] = rows; rows += N.sizes[l + 1] * a.C; }
        // value-only terms of tanh / sigmoid networks: the record of an element IS its post-activation value (act_record), so the
        // matrix-pipe kernels keep ONE copy (a third of the tile kernel's stores less; 4 of the bench workload's 5 terms)
        const bool post_is_rec = L.mfma && a.C == 1 && !pk::act_records_z(pk::act_class(N.act));
        a.post_alias = post_is_rec ? 1 : 0;
        for (int l = 0; l < LH; ++l) { if (post_is_rec) n.r_post[l] = n.r_rec[l]; else { n.r_post[l] = rows; rows += N.sizes[l + 1] * a.C; } }
        for (int l = 0; l < LH; ++l) { n.r_dz[l] = rows; rows += N.sizes[l + 1] * a.C; }
        n.r_ubar = rows; rows += a.C;
    }
    a.ent_p = ent;
    a.nent = ent + E.ne + 1;
    a.r_pbar = rows; rows += std::max(E.ne, 1);
    a.r_sq = rows; rows += 1;
    a.np = E.np; a.ne = E.ne; a.p_off = E.p_theta_off;
    fill_pdef(E, a.pdef);
    a.prog = F.d_prog; a.imm = F.d_imm; a.nops = F.nops; a.out_row = F.out_row; a.nslots = F.nslots;
    for (int s = 0; s < F.nslots; ++s) { a.slot_chan[s] = F.slot_chan[s]; a.slot_net[s] = F.slot_net[s]; }
    a.nrows = rows;
    L.rows = rows;
    if (L.mfma) {
        a.ntp = a.tp_p + E.ne + 1;
        a.tile_pts = 16 * F.km->PG;
    }
    return 0;
}
// points per launch and the buffers of one: scratch rows (below 256 MB with one lane per point / 4 GB with the matrix-pipe kernels — one wave per
// 16-32 points there, a chunk should hold several tiles per SIMD: the bench workload's 65,536-point terms are one chunk each; $PINN_F64_SCRATCH_MB
// overrides), per-block slabs, per-tile partial sums.  An allocation that fails is retried with half the chunk down to one block.
// with_sums == false (values-only launches, a.mode == 2): no slabs / tile sums
int f64_buffers(pinn_engine& E, F64State& S, F64Launch& L, int64_t n, bool with_sums, int64_t& chunk_out) {
    pk::F64Args& a = L.a;
    double mb = L.sw.scratch_mb > 0.0 ? L.sw.scratch_mb : (L.mfma ? 4096.0 : 256.0);
    const bool need_scratch = !(L.mfma && a.mode != 0) || L.sliced;              // (the tile kernels keep everything in registers unless a reverse sweep / dW launch follows)
    for (;; mb *= 0.5) {
        int64_t chunk = (int64_t)((mb * 1024 * 1024) / (8.0 * L.rows));
        chunk = std::max<int64_t>(pk::F64_BLOCK, (chunk / pk::F64_BLOCK) * pk::F64_BLOCK);
        chunk = std::min<int64_t>(chunk, ((n + pk::F64_BLOCK - 1) / pk::F64_BLOCK) * pk::F64_BLOCK);
        const bool last_try = chunk <= pk::F64_BLOCK;
        bool ok = true;
        if (need_scratch) ok = dev_grow(S.d_scratch, S.scratch_cap, (size_t)L.rows * (size_t)chunk + pk::F64S_PAD_SCRATCH, E.stream);
        if (ok && with_sums) ok = dev_grow(S.d_slab, S.slab_cap, (size_t)(chunk / pk::F64_BLOCK) * (size_t)a.nent, E.stream);
        if (ok && with_sums && L.mfma) ok = dev_grow(S.d_tpart, S.tpart_cap, (size_t)(chunk / a.tile_pts + 1) * (size_t)a.ntp, E.stream);
        if (ok) {
            a.scratch = S.d_scratch; a.npad = (int)chunk; a.slab = S.d_slab; a.tpart = S.d_tpart;
            chunk_out = chunk;
            return 0;
        }
        if (last_try) return fail("device allocation failed (float64 scratch / slabs, even for one 512-point block)");
    }
}

// Small launches of the register-resident matrix-pipe kernels: SHORT blocks for the dW kernel.  One 512-point block = one workgroup per layer, whose four
// waves walk the block's 16-point groups x channels one dependent load + MFMA step after the other: 15 us for 176 points x 5 channels.  With short
// blocks the same steps spread over many workgroups (the slab gets one row per block, the reduction adds a few more rows).  Returns the block count.
constexpr int F64_SMALL_BLOCK = 64;
static int f64_short_blocks(pinn_engine& E, F64State& S, F64Launch& L) {
    pk::F64Args& a = L.a;
    a.block_pts = 0;
    const int full = (a.npts + pk::F64_BLOCK - 1) / pk::F64_BLOCK;
    if (!L.mfma || L.sliced || a.tile_pts <= 0 || F64_SMALL_BLOCK % a.tile_pts != 0 || L.sw.no_short_blocks) return full;
    // the shortest power-of-two block (>= 64 points) that still gives the launch ~512 workgroups: blocks x (hidden-to-hidden layers + 1)
    int rows = 1;
    for (int ni = 0; ni < a.nnets; ++ni) rows += std::max(0, a.net[ni].nl - 2);
    int bp = pk::F64_BLOCK;
    while (bp > F64_SMALL_BLOCK && (int64_t)((a.npts + bp - 1) / bp) * rows < L.sw.dwt_wgs) bp >>= 1;
    if (bp == pk::F64_BLOCK) return full;
    const int nb = (a.npts + bp - 1) / bp;
    if (!dev_grow(S.d_slab, S.slab_cap, (size_t)nb * (size_t)a.nent, E.stream)) return full;
    a.slab = S.d_slab;
    a.block_pts = bp;
    return nb;
}

// the matrix-pipe tile kernel reads the per-term fields through F64Args::sub (pinn_kernels4.hpp: F64Sub): a plain launch mirrors its own fields into entry 0
static void f64_launch_tile(const pk::F64MKernel* km, pk::F64Args& a, plat_stream st) {
    if (a.nsub == 0) {
        pk::F64Sub& u = a.sub[0];
        u.pts = a.pts; u.pw = a.pw; u.data = a.data; u.prog = a.prog; u.imm = a.imm; u.lin = a.lin; u.scale = a.scale;
        u.N = a.N; u.nops = a.nops; u.out_row = a.out_row; u.nslots = a.nslots;
        for (int q = 0; q < pk::F64_MAX_SLOTS; ++q) { u.slot_net[q] = (unsigned char)a.slot_net[q]; u.slot_chan[q] = (unsigned char)a.slot_chan[q]; }
    }
    km->launch_tile(a, st);
}

// Which terms ride in one launch (see F64State::Group).  Small problems only: a merged launch evaluates every member on the UNION jet set (a value-only
// boundary term carries the interior term's derivative channels), which costs nothing while every tile of the problem is resident at once and the
// evaluation is bound by the latency of one tile per launch — and would multiply the boundary terms' work on a large problem.
constexpr int64_t F64_MERGE_MAX_POINTS = 8192;
static void f64_make_groups(pinn_engine& E, F64State& S, const F64Switches& sw) {
    const int K = (int)S.terms.size();
    const bool off = sw.no_merge || sw.no_mfma;
    std::vector<int64_t> sig(K + 1);
    for (int t = 0; t < K; ++t) sig[t] = S.terms[t].n;
    sig[K] = off ? 1 : 0;                                // (the switches are part of what the grouping was made for: flipping one on a live handle remakes it)
    if (sig == S.groups_sig) return;
    S.groups_sig = sig;
    S.groups.clear();
    if (off) return;
    std::vector<char> used(K, 0);
    for (int t = 0; t < K; ++t) {
        if (used[t]) continue;
        const Term& T0 = E.terms0[t];
        const F64Term& F = S.terms[t];
        if (!F.km || F.km->sliced || F.n <= 0) continue;
        F64State::Group G;
        std::vector<Slot> slots = T0.slots;
        int64_t pts = F.n;
        G.terms.push_back(t);
        G.nets = F.nets;
        G.inmap = T0.inmap;
        const int d = E.nets[F.nets[0]].sizes[0];
        bool free_merge = true;                          // every member so far runs its OWN kernel on its own networks
        for (int u = t + 1; u < K && (int)G.terms.size() < pk::F64_MAX_SUB; ++u) {
            const Term& U0 = E.terms0[u];
            const F64Term& Fu = S.terms[u];
            if (used[u] || !Fu.km || Fu.km->sliced || Fu.n <= 0) continue;
            if (U0.d != T0.d || E.nets[Fu.nets[0]].sizes[0] != d) continue;
            // the launch evaluates the UNION of the members' networks for every tile (a network a member does not read gets zero seeds from it):
            // systems of equations over different subsets of the dependent variables (the reference's Lorenz test) still ride in one sequence
            std::vector<int> nets = G.nets;
            for (int ni : Fu.nets) if (std::find(nets.begin(), nets.end(), ni) == nets.end()) nets.push_back(ni);
            std::sort(nets.begin(), nets.end());
            if ((int)nets.size() > pk::F64_MAX_NETS) continue;
            std::map<int, std::vector<int>> inmap = G.inmap;
            bool clash = false;
            for (int ni : nets) {                        // one input binding per network: explicit maps must agree, an identity binding must be one for both
                const bool a_has = G.inmap.count(ni) != 0, b_has = U0.inmap.count(ni) != 0;
                const bool a_uses = std::find(G.nets.begin(), G.nets.end(), ni) != G.nets.end(), b_uses = std::find(Fu.nets.begin(), Fu.nets.end(), ni) != Fu.nets.end();
                if (a_uses && b_uses && (a_has != b_has || (a_has && G.inmap.at(ni) != U0.inmap.at(ni)))) { clash = true; break; }
                if (b_uses && b_has) inmap[ni] = U0.inmap.at(ni);
            }
            if (clash) continue;
            std::vector<Slot> trial = slots;
            trial.insert(trial.end(), U0.slots.begin(), U0.slots.end());
            std::vector<int> ch;
            std::string why;
            const pk::F64Kernel* k = f64_find(d, trial, ch, why);
            const pk::F64MKernel* km = k ? f64_find_m(E, k, nets, sw) : nullptr;
            if (!km || km->sliced) continue;
            // beyond the small-problem size a member joins only where it costs nothing: the same kernel and the same networks as every other member
            // (the four boundary terms of a 2-D problem: one dW / reduction launch instead of four)
            const bool same = free_merge && k == F.k && k == Fu.k && nets == F.nets && nets == Fu.nets;
            if (pts + Fu.n > F64_MERGE_MAX_POINTS && !same) continue;
            free_merge = same;
            slots.swap(trial);
            pts += Fu.n;
            G.terms.push_back(u);
            G.nets.swap(nets);
            G.inmap.swap(inmap);
        }
        if (G.terms.size() < 2 || (pts > F64_MERGE_MAX_POINTS && !free_merge)) continue;
        std::vector<int> ch;
        std::string why;
        G.k = f64_find(d, slots, ch, why);
        G.km = G.k ? f64_find_m(E, G.k, G.nets, sw) : nullptr;
        if (!G.km || G.km->sliced) continue;
        size_t o = 0;
        for (int u : G.terms) {
            const size_t ns = E.terms0[u].slots.size();
            G.slot_chan.emplace_back(ch.begin() + o, ch.begin() + o + ns);
            o += ns;
            used[u] = 1;
        }
        S.groups.push_back(std::move(G));
    }
}

// ---- one chunk of one launch sequence ----
// the forward kernel of the term's family: the matrix-pipe tile kernel, or one lane per point
void f64_launch_forward(const F64Term& F, F64Launch& L, plat_stream st) {
    if (L.mfma) f64_launch_tile(F.km, L.a, st);
    else F.k->launch_point(L.a, L.acls, st);
}
// what every reduction's arguments take from the launch: slab rows and entries, the gradient and the networks' places in theta
static void f64_reduce_common(const pinn_engine& E, const F64State& S, const pk::F64Args& a, double* grad, int nblocks, pk::F64ReduceArgs& r) {
    r.slab = S.d_slab; r.nblocks = nblocks; r.nent = a.nent;
    r.grad = grad; r.ent_p = a.ent_p; r.p_off = E.p_theta_off; r.nnets = a.nnets;
    for (int ni = 0; ni < a.nnets; ++ni) { r.ent0[ni] = a.net[ni].ent0; r.theta0[ni] = a.net[ni].theta0; }
    r.with_grad = grad ? 1 : 0;
}
// loss (+ gradient) of the points [L.a.p0, + L.a.npts): the forward kernel, dW on the lane path (the matrix-pipe tile kernel produces those
// entries itself), dWt, and the reduction of the same family.  `r` arrives with its sums of squares set (f64_reduce_into, or a merged launch's
// own); `gs` decides whether this reduction writes the gradient (nullptr: it adds)
void f64_launch_chunk(pinn_engine& E, F64State& S, const F64Term& F, F64Launch& L, double* grad, GradStart* gs, pk::F64ReduceArgs& r) {
    pk::F64Args& a = L.a;
    const int nblocks = f64_short_blocks(E, S, L);
    f64_launch_forward(F, L, E.stream);
    if (!L.mfma) pk::launch_f64_dw(a, E.stream);
    if (L.mfma) F.km->launch_dwt(a, E.stream);
    else pk::launch_f64_dwt(a, E.stream);
    f64_reduce_common(E, S, a, grad, nblocks, r);
    r.init_grad = gs ? gs->first_reduction_writes(F.nets) : 0;
    if (L.mfma) pk::launch_f64m_reduce(r, E.stream);
    else pk::launch_f64_reduce(r, E.stream);
}

// ---- the evaluation (f64_eval_device) in phases ----
// one evaluation, as every launch path reads it
struct F64Eval {
    pinn_engine& E;
    F64State& S;
    const F64Switches sw;
    const double* theta;                 // device; the handle's padded copy where the caller's buffer has no margin (padded_theta)
    double* grad;                        // device [P]; nullptr: loss only
    double* sumsq;                       // device [K]
    const double* term_w;                // host [K]; nullptr: ones
    GradStart gs;
    double w(int t) const { return term_w ? term_w[t] : 1.0; }
    int mode() const { return grad ? 0 : 1; }
};
// a CALLER's device buffer (pinn_loss_grad_device_f64): the matrix-pipe kernels read up to F64S_PAD_THETA doubles past a narrow layer's matrix —
// evaluate from the handle's padded copy (P doubles device to device: microseconds)
static int padded_theta(pinn_engine& E, F64State& S, const double*& theta) {
    if (theta == S.d_theta || theta == S.d_opt_theta) return 0;
    bool reads_past = false;                             // (family 4s and, r06, family 4m: unclamped weight fragments)
    for (auto& F : S.terms) reads_past = reads_past || F.km != nullptr;
    if (!reads_past) return 0;
    if (plat_d2d(S.d_theta, theta, sizeof(double) * E.ntheta, E.stream)) return fail("device copy of theta failed");
    theta = S.d_theta;
    return 0;
}
// every term has its points, and its per-point data where it reads any, for the set that is installed
static int check_ready(const pinn_engine& E, const F64State& S) {
    const int K = (int)E.terms.size();
    for (int t = 0; t < K; ++t)
        if (S.terms[t].n <= 0 || S.terms[t].n != E.terms[t].n) return fail("term " + std::to_string(t) + " has no collocation points (call pinn_set_points first)");
    for (int t = 0; t < K; ++t)
        if (S.terms[t].ndata > 0 && S.terms[t].data_n != S.terms[t].n)
            return fail("term " + std::to_string(t) + " uses per-point data channels but none are installed for its current point set (call pinn_set_point_data after pinn_set_points)");
    return 0;
}
// a merged group as ONE tile / dWt / reduction sequence: a pseudo-term on the union jet set; its networks, rows and slab entries are the
// members' (same networks).  `launched` stays false where the group does not go out as one launch (the lane path is forced, or it does not fit
// the scratch budget): the members then go one by one
static int eval_group(F64Eval& ev, const F64State::Group& G, bool& launched) {
    pinn_engine& E = ev.E;
    F64State& S = ev.S;
    const int m = (int)G.terms.size();
    F64Term Fg;
    Fg.k = G.k; Fg.km = G.km; Fg.nets = G.nets;
    Fg.nops = 0; Fg.nslots = 0; Fg.out_row = 0; Fg.ndata = 0;
    F64Launch L;
    if (f64_build(E, Fg, E.terms0[G.terms[0]].d, &G.inmap, ev.sw, L)) return 1;
    if (!L.mfma || L.sliced) return 0;
    pk::F64Args& a = L.a;
    const int tp = a.tile_pts;
    int tiles = 0;
    a.nsub = m;
    for (int q = 0; q < m; ++q) {
        const int t = G.terms[q];
        const Term& T = E.terms[t];
        const F64Term& F = S.terms[t];
        pk::F64Sub& u = a.sub[q];
        a.sub_tile0[q] = tiles;
        tiles += (int)((F.n + tp - 1) / tp);
        u.pts = F.d_pts; u.pw = term_pw(T); u.data = F.ndata > 0 ? F.d_data : nullptr;
        u.prog = F.d_prog; u.imm = F.d_imm; u.lin = f64_lin_ptr(F);
        u.scale = f64_term_scale(T, ev.w(t));
        u.N = (int)F.n; u.nops = F.nops; u.out_row = F.out_row; u.nslots = F.nslots;
        for (int sl = 0; sl < F.nslots; ++sl) {          // (slot_net: position of the slot's network in the launch's — the union's — list)
            u.slot_net[sl] = (unsigned char)(std::find(G.nets.begin(), G.nets.end(), F.nets[F.slot_net[sl]]) - G.nets.begin());
            u.slot_chan[sl] = (unsigned char)G.slot_chan[q][sl];
        }
    }
    a.sub_tile0[m] = tiles;
    for (int q = m + 1; q <= pk::F64_MAX_SUB; ++q) a.sub_tile0[q] = tiles;
    a.nent += m - 1;                                     // (the slab row ends in one sum of squares per member)
    a.theta = ev.theta;
    a.mode = ev.mode();
    a.p0 = 0;
    a.npts = tiles * tp;
    int64_t chunk = 0;
    if (f64_buffers(E, S, L, a.npts, true, chunk)) return 1;
    if (chunk < a.npts) return 0;
    S.ran_merged();
    pk::F64ReduceArgs r = f64_reduce_into(ev.sumsq, true);
    r.nsq = m;                                           // (every member's own sum of squares, written)
    for (int q = 0; q < m; ++q) r.sq_off[q] = G.terms[q];
    f64_launch_chunk(E, S, Fg, L, ev.grad, &ev.gs, r);
    launched = true;
    return 0;
}
// a term on its own: one launch sequence per scratch-sized chunk of its point set; the first chunk writes the term's sum of squares
static int eval_term(F64Eval& ev, int t) {
    pinn_engine& E = ev.E;
    const Term& T = E.terms[t];
    const Term& T0 = E.terms0[t];
    const F64Term& F = ev.S.terms[t];
    F64Launch L;
    if (f64_build(E, F, T0.d, &T0.inmap, ev.sw, L)) return 1;
    pk::F64Args& a = L.a;
    a.theta = ev.theta;
    a.pw = term_pw(T);
    a.scale = f64_term_scale(T, ev.w(t));
    a.mode = ev.mode();
    return f64_for_chunks(E, ev.S, L, F.n, true, [&] {
        pk::F64ReduceArgs r = f64_reduce_into(ev.sumsq + t, a.p0 == 0);
        f64_launch_chunk(E, ev.S, F, L, ev.grad, &ev.gs, r);
    });
}
// a term with derivative slots in stencil mode: the reference's central differences (a validation mode, one lane per point)
static int eval_stencil_term(F64Eval& ev, int t) {
    ev.S.ran(false);
    return f64_stencil_term(ev.E, ev.sw, t, ev.theta, ev.grad, ev.sumsq + t, ev.w(t), ev.mode(), nullptr);
}

// loss sums (`sumsq`, K doubles) and gradient (`grad`, P doubles; nullptr: loss only) at the parameters `theta` — all three device pointers —
// everything on the device, nothing synchronised.  Merged groups first, then every term no group took, in term order
int f64_eval_device(pinn_engine& E, const double* theta, double* grad, double* sumsq, const double* term_w) {
    F64State& S = state(E);
    const int K = (int)E.terms.size();
    if (padded_theta(E, S, theta) || check_ready(E, S)) return 1;
    F64Eval ev{E, S, f64_read_switches(), theta, grad, sumsq, term_w, GradStart{E, grad}};      // (the switches after the copy: the device is busy while the host looks)
    if (S.stencil) ev.gs.zero();                         // (stencil mode's seeded launches all add)
    S.new_evaluation();
    std::vector<char> done(K, 0);
    if (!S.stencil) {
        f64_make_groups(E, S, ev.sw);
        for (const F64State::Group& G : S.groups) {
            bool launched = false;
            if (eval_group(ev, G, launched)) return 1;
            if (launched) for (int t : G.terms) done[t] = 1;
        }
    }
    for (int t = 0; t < K; ++t) {
        if (done[t]) continue;
        if ((S.stencil && S.sten[t].active) ? eval_stencil_term(ev, t) : eval_term(ev, t)) return 1;
    }
    return 0;
}

int f64_eval(pinn_engine& E, const double* theta, const double* term_w, double* term_losses, double* grad) {
    F64State& S = state(E);
    const int K = (int)E.terms.size();
    const int64_t P = E.ntheta;
    // (pinned staging both ways: a pageable source / destination makes every copy a synchronous, internally staged one — the host entry of a small problem
    // is mostly those copies; gradient and sums are one device vector, so one copy brings both)
    std::memcpy(S.h_pin, theta, sizeof(double) * P);
    if (plat_h2d(S.d_theta, S.h_pin, sizeof(double) * P, E.stream)) return fail("H2D copy of theta failed");
    if (f64_eval_device(E, S.d_theta, grad ? S.d_grad : nullptr, S.d_sumsq, term_w)) return 1;
    double* out = S.h_pin + P;
    if (grad ? plat_d2h(out, S.d_grad, sizeof(double) * (P + K), E.stream) : plat_d2h(out + P, S.d_sumsq, sizeof(double) * K, E.stream)) return fail("D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    if (term_losses)
        for (int k = 0; k < K; ++k) term_losses[k] = out[(size_t)P + k] / (double)E.terms[k].n_norm;
    if (grad) std::memcpy(grad, out, sizeof(double) * P);
    return 0;
}

// ---- the public closures that return PER-POINT values, in double (r06): the reference evaluates them in eltype(theta) = Float64 by default —
// datafree_pde_loss_functions[i](cord, theta) (src/pinn_types.jl:435-439, compared at rtol 1e-8 in test/Forward/forward__ode.jl:46-47),
// phi(x, theta) (src/pinn_types.jl:88-90), numeric_derivative (src/pinn_types.jl:445-482; atol 1e-8 in test/Forward/forward__derivatives.jl:29-30) ----
// values-only launches (F64Args::mode == 2) of `L` over n points: out[p] on the device
int f64_values(pinn_engine& E, F64State& S, const F64Term& F, F64Launch& L, int64_t n, double* d_out) {
    pk::F64Args& a = L.a;
    a.mode = 2;
    a.resid = d_out;
    a.scale = 0.0;
    return f64_for_chunks(E, S, L, n, false, [&] { f64_launch_forward(F, L, E.stream); });
}
// residual_k(set_k, theta) at every point of the installed set (pinn_residual_f64; pinn_residual in float64 mode)
int f64_residual(pinn_engine& E, int term, const double* theta, double* r) {
    const F64Term& F = state(E).terms[term];
    if (F.n <= 0 || F.n != E.terms[term].n) return fail("pinn_residual: term has no points");
    if (F.ndata > 0 && F.data_n != F.n) return fail("pinn_residual: the term uses per-point data channels but none are installed for its current point set");
    const double* d_r = nullptr;
    if (f64_upload_theta(E, theta) || f64_residual_device(E, term, &d_r)) return 1;
    if (plat_d2h(r, d_r, sizeof(double) * (size_t)F.n, E.stream) || plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}
int f64_upload_theta(pinn_engine& E, const double* theta) {
    return plat_h2d(state(E).d_theta, theta, sizeof(double) * E.ntheta, E.stream) ? fail("H2D copy of theta failed") : 0;
}
// its device part: the values-only launches over the term's double point set at the uploaded parameters, queued on the stream
int f64_residual_device(pinn_engine& E, int term, const double** d_r) {
    F64State& S = state(E);
    const F64Term& F = S.terms[term];
    if (!dev_grow(S.d_aux_out, S.aux_out_cap, (size_t)F.n, E.stream)) return fail("device allocation failed (float64 residuals)");
    const F64Switches sw = f64_read_switches();
    S.new_call();
    if (S.stencil && S.sten[term].active) {
        S.ran(false);
        if (f64_stencil_term(E, sw, term, S.d_theta, nullptr, nullptr, 1.0, 2, S.d_aux_out)) return 1;
    } else {
        F64Launch L;
        if (f64_build(E, F, E.terms0[term].d, &E.terms0[term].inmap, sw, L)) return 1;
        L.a.theta = S.d_theta;
        if (f64_values(E, S, F, L, F.n, S.d_aux_out)) return 1;
    }
    *d_r = S.d_aux_out;
    return 0;
}
// d^order phi_net / dx_axes (order 0: the trial function itself) at n caller-supplied points (pinn_phi[_f64], pinn_derivative[_f64] in float64 mode;
// engine.cpp has checked order, axes and the embedding): a pseudo-term of one slot and an empty tape on the jet set that carries the derivative
int f64_net_eval(pinn_engine& E, int net, const double* theta, const double* pts, int64_t n, int order, const int* axes, double* out) {
    F64State& S = state(E);
    const Net& N = E.nets[net];
    const std::string who = "float64 trial-function evaluation: ";
    if (N.kind != 0) return fail(who + "DGM networks are not covered by the float64 mode");
    if (!f64_act_ok(N.act)) return fail(who + "this activation is not covered by the float64 mode");
    if ((int)N.sizes.size() - 1 > pk::F64_MAX_LAYERS || N.sizes[0] > 4) return fail(who + "more than 16 Dense layers / more than 4 inputs");
    const int d = N.sizes[0];
    // a network behind a periodic input embedding (r06; value only): the caller's points are the dependent variable's ARGUMENTS [n][n_inputs]; the
    // Dense chain takes the features, formed here in double
    std::vector<double> feats;
    if (!N.emb_idx.empty()) {
        feats = N.features(pts, n);
        pts = feats.data();
    }
    Slot sl;
    sl.net = net; sl.order = order; sl.lap = 0;
    for (int q = 0; q < MAX_DERIV_ORDER; ++q) sl.axes[q] = q < order ? axes[q] : 0;
    std::sort(sl.axes, sl.axes + order);
    const F64Switches sw = f64_read_switches();
    F64Term F;
    std::string why;
    F.k = f64_find(d, std::vector<Slot>{sl}, F.slot_chan, why);
    if (!F.k) return fail(who + why);
    F.nets = {net};
    F.km = f64_find_m(E, F.k, F.nets, sw);
    F.slot_net = {0};
    F.nops = 0; F.nslots = 1; F.out_row = d + E.np;
    F.n = n;
    const bool okp = dev_grow(S.d_aux_pts, S.aux_pts_cap, (size_t)n * d, E.stream), oko = dev_grow(S.d_aux_out, S.aux_out_cap, (size_t)n, E.stream);
    if (!okp || !oko) return fail("device allocation failed (float64 trial-function points)");
    F.d_pts = S.d_aux_pts;                               // (borrowed)
    if (plat_h2d(S.d_theta, theta, sizeof(double) * E.ntheta, E.stream) || plat_h2d(S.d_aux_pts, pts, sizeof(double) * (size_t)n * d, E.stream)) return fail("H2D copy failed");
    F64Launch L;
    const int rc = f64_build(E, F, d, nullptr, sw, L);
    L.a.theta = S.d_theta;
    S.new_call();
    if (rc || f64_values(E, S, F, L, n, S.d_aux_out)) return 1;
    if (plat_d2h(out, S.d_aux_out, sizeof(double) * (size_t)n, E.stream) || plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

// this device's part of a single-process multi-device evaluation (pinn_loss_grad_sharded_f64): theta from the host, [gradient | sums] stay on the device
int f64_eval_sharded_local(pinn_engine& E, const double* theta, const double* term_w, double** d_out) {
    F64State& S = state(E);
    if (plat_h2d(S.d_theta, theta, sizeof(double) * E.ntheta, E.stream)) return fail("H2D copy of theta failed");
    if (f64_eval_device(E, S.d_theta, S.d_grad, S.d_sumsq, term_w)) return 1;
    *d_out = S.d_grad;
    return 0;
}
// float64 evaluation at DEVICE-resident float parameters (pinn_loss_grad_device / pinn_loss_device in float64 mode): theta converted on the
// device, [gradient | term sums] converted back into the caller's float vector — the kernels in between are the double ones
int f64_eval_from_device_f32(pinn_engine& E, const float* d_theta, const float* term_w, float* d_out, bool want_grad) {
    F64State& S = state(E);
    const int K = (int)E.terms.size();
    const int64_t P = E.ntheta;
    const std::vector<double> w = f64_widen_weights(term_w, K);
    pk::launch_f64_cvt(d_theta, S.d_theta, P, E.stream);
    if (f64_eval_device(E, S.d_theta, want_grad ? S.d_grad : nullptr, S.d_sumsq, w.data())) return 1;
    if (want_grad) pk::launch_f64_narrow(S.d_grad, d_out, P, E.stream);
    pk::launch_f64_narrow(S.d_sumsq, d_out + (want_grad ? P : 0), K, E.stream);
    return 0;
}

// theta and [gradient | raw sums] as DOUBLE device pointers: nothing crosses the boundary in fp32, nothing crosses PCIe; the kernels read the
// caller's theta and write the caller's [gradient | sums] directly: no copies
int f64_eval_from_device_f64(pinn_engine& E, const double* d_theta, const float* term_w, double* d_out) {
    const std::vector<double> w = f64_widen_weights(term_w, (int)E.terms.size());
    return f64_eval_device(E, d_theta, d_out, d_out + E.ntheta, w.data());
}

// the resident HMC loop (hmc.cpp: pinn_hmc_*) in float64 mode: its update kernel writes the proposal into the evaluation's own parameter buffer
// (padded as the matrix-pipe kernels need) and every leapfrog step evaluates there, [gradient | raw sums] into the sampler's own vector (P + K doubles)
double* f64_theta_buffer(pinn_engine& E) { return state(E).d_theta; }
int f64_eval_resident(pinn_engine& E, const double* term_w, double* d_out) {
    return f64_eval_device(E, state(E).d_theta, d_out, d_out + E.ntheta, term_w);
}

// " f64_channels=5,1,1,1,1 f64_kernels=mfma:HT4xPG1,mfma:HT4xPG4,..." for pinn_describe
std::string f64_describe(const pinn_engine& E) {
    if (!E.f64) return "";
    const F64State& S = state(E);
    std::string c = " f64_channels=", k = " f64_kernels=";
    for (size_t t = 0; t < S.terms.size(); ++t) {
        const F64Term& F = S.terms[t];
        c += (t ? "," : "") + std::to_string(F.k ? F.k->C : 0);
        k += (t ? "," : "") + (F.km ? std::string(F.km->sliced ? "mfma-sliced:HT" : "mfma:HT") + std::to_string(F.km->HT) + "xPG" + std::to_string(F.km->PG) : std::string("lanes"))
             + (!F.nets.empty() && E.nets[F.nets[0]].act == pk::ACT_SWISH ? "+swish" : "");
    }
    return c + k;
}

int f64_merged(const pinn_engine& E) { return E.f64 ? state(E).merged_launches : 0; }
int f64_chunks(const pinn_engine& E) { return E.f64 ? state(E).max_chunks : 0; }
int f64_affine_terms(const pinn_engine& E) {
    if (!E.f64) return 0;
    int n = 0;
    for (auto& F : state(E).terms) n += f64_lin_ptr(F) != nullptr && F.km != nullptr;
    return n;
}
const char* f64_path(const pinn_engine& E) {
    if (!E.f64) return "off";
    const int p = state(E).path;
    return p == 2 ? "mfma" : (p == 1 ? "lanes" : (p == 3 ? "mfma+lanes" : "none"));
}

}  // namespace pe
