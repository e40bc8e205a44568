// f64_setup.cpp — the float64 evaluation mode's state: kernel registries and look-up, enabling the mode (pinn_set_option(h, "precision", "f64")), the
// affine analysis of residuals, installation of point sets and per-point data in double, teardown.  The evaluation itself: f64.cpp.
#include <unistd.h>      // environ
#include "f64_internal.hpp"

namespace pk {
std::deque<F64Kernel>& f64_registry() {
    static std::deque<F64Kernel> r;
    return r;
}
std::deque<F64MKernel>& f64m_registry() {
    static std::deque<F64MKernel> r;
    return r;
}
}  // namespace pk

namespace pe {

static void f64_free(F64State* S) {
    if (!S) return;
    for (auto& T : S->terms) { plat_free(T.d_prog); plat_free(T.d_imm); plat_free(T.d_pts); plat_free(T.d_data); plat_free(T.d_lin); }
    for (auto& X : S->sten) { plat_free(X.d_prog); plat_free(X.d_imm); }
    plat_free(S->d_uv); plat_free(S->d_seeds); plat_free(S->d_spts);
    plat_free(S->d_theta); plat_free(S->d_opt_theta); plat_free(S->d_aux_pts); plat_free(S->d_aux_out); plat_free(S->d_grad); plat_free(S->d_scratch); plat_free(S->d_slab); plat_free(S->d_tpart);
    plat_free(S->d_m); plat_free(S->d_v); plat_free(S->d_w_over_n); plat_free(S->d_hist);
    plat_host_free(S->h_pin);
    delete S;
}
void f64_destroy(pinn_engine& E) {
    f64_free((F64State*)E.f64);
    E.f64 = nullptr;
}

// a switch is on when its variable is set, to anything (as with getenv); the two numbers are read as getenv's callers read them.  ONE pass over
// the environment finds all eight: this runs in every evaluation, where a getenv scan per switch is measurable on small problems
F64Switches f64_read_switches() {
    F64Switches sw;
    const struct { const char* name; bool* on; } flags[] = {{"NO_MFMA=", &sw.no_mfma}, {"NO_SLICED=", &sw.no_sliced}, {"NO_MERGE=", &sw.no_merge},
        {"NO_LIN=", &sw.no_lin}, {"NO_SHORT_BLOCKS=", &sw.no_short_blocks}, {"FULL_CHANNELS=", &sw.full_channels}};
    for (char** e = environ; e && *e; ++e) {
        if (std::strncmp(*e, "PINN_F64_", 9) != 0) continue;
        const char* v = *e + 9;
        for (const auto& f : flags)
            if (std::strncmp(v, f.name, std::strlen(f.name)) == 0) *f.on = true;
        if (std::strncmp(v, "SCRATCH_MB=", 11) == 0) sw.scratch_mb = std::max(1.0, std::atof(v + 11));
        if (std::strncmp(v, "DWT_WGS=", 8) == 0) sw.dwt_wgs = std::max(1, std::atoi(v + 8));
    }
    return sw;
}

// the smallest float64 kernel of `D` inputs that carries every derivative slot of the term
const pk::F64Kernel* f64_find(int D, const std::vector<Slot>& slots, std::vector<int>& chan, std::string& why) {
    const pk::F64Kernel* best = nullptr;
    for (const pk::F64Kernel& k : pk::f64_registry()) {
        if (k.D != D) continue;
        pk::SpecInfo s;
        std::memset(&s, 0, sizeof s);
        s.D = D; s.D1MASK = k.D1MASK; s.PAIRS = k.PAIRS; s.NPAIR = k.NPAIR; s.HI = k.HI; s.NFIRST = k.NFIRST; s.LAP = 0; s.ngen = 0;
        bool ok = true;
        std::vector<int> ch;
        for (auto& sl : slots) {
            if (sl.lap || slot_is_general(sl)) { ok = false; break; }
            if (sl.order == 1 && !((k.D1MASK >> sl.axes[0]) & 1)) { ok = false; break; }     // (chan_of ranks first derivatives inside the mask, it does not test membership)
            const int c = chan_of(s, sl);
            if (c < 0) { ok = false; break; }
            ch.push_back(c);
        }
        if (ok && (!best || k.C < best->C)) { best = &k; chan = ch; }
    }
    if (!best) why = "no float64 kernel carries this term's derivatives (orders <= 2 in 1-3 inputs; 1-D: <= 4; 4-D: first and pure second derivatives)";
    return best;
}

// family 4m (v_mfma_f64_16x16x4_f64) for the jet set of `k`: tanh / sigmoid networks with at least one hidden layer, none wider than an instantiated
// 16 * HT; nullptr: family 4 (one lane per point)
const pk::F64MKernel* f64_find_m(const pinn_engine& E, const pk::F64Kernel* k, const std::vector<int>& nets, const F64Switches& sw) {
    int maxh = 0;
    for (int net : nets) {
        const Net& N = E.nets[net];
        if (pk::act_records_z(pk::act_class(N.act)) || N.sizes.size() < 3) return nullptr;        // sin, swish: family 4
        for (size_t j = 1; j + 1 < N.sizes.size(); ++j) maxh = std::max(maxh, N.sizes[j]);
    }
    // a register-resident kernel (family 4m) before a channel-sliced one (family 4s: every layer through the scratch rows); the narrowest that covers the width
    const pk::F64MKernel* best = nullptr;
    for (const pk::F64MKernel& km : pk::f64m_registry()) {
        if (!(km.D == k->D && km.D1MASK == k->D1MASK && km.PAIRS == k->PAIRS && km.NPAIR == k->NPAIR && km.HI == k->HI && 16 * km.HT >= maxh)) continue;
        if (km.sliced && sw.no_sliced) continue;
        if (!best || (km.sliced < best->sliced) || (km.sliced == best->sliced && km.HT < best->HT)) best = &km;
    }
    return best;
}

// ---- affine residuals: r = S(point) + sum_s a_s u_s ----
// Symbolic pass over the term's tape (descriptor rows [coordinates | parameters | slots | ops]): every row is either a constant-coefficient affine
// form in the slots plus coordinate-only rows, or the term is not affine (nonlinear in u, point-dependent coefficients, estimated parameters, DATA
// rows) and keeps the interpreter.  Boundary conditions, linear PDEs with forcing terms (Poisson, heat, wave) qualify; Burgers does not.
static void f64_affine(const pinn_engine& E, const Term& T, const F64Switches& sw, F64Term& F) {
    F.lin = false;
    if (sw.no_lin || F.ndata > 0) return;
    struct Form { bool ok = true; std::vector<double> a; std::vector<std::pair<double, int>> t; double k = 0.0; };
    const int dt = T.d, np = E.np, ns = (int)T.slots.size(), R0 = dt + np + ns;
    std::vector<Form> row((size_t)R0 + T.ops.size());
    for (auto& f : row) f.a.assign((size_t)ns, 0.0);
    for (int i = 0; i < dt; ++i) row[i].t.push_back({1.0, i});
    for (int k = 0; k < np; ++k) { if (k < E.ne) row[dt + k].ok = false; else row[dt + k].k = k < (int)E.p_defaults.size() ? E.p_defaults[k] : 0.0; }
    for (int q = 0; q < ns; ++q) row[dt + np + q].a[q] = 1.0;
    auto has_u = [&](const Form& f) { for (double x : f.a) if (x != 0.0) return true; return false; };
    auto is_const = [&](const Form& f) { return f.ok && !has_u(f) && f.t.empty(); };
    auto scaled = [&](const Form& f, double c) { Form g = f; for (double& x : g.a) x *= c; for (auto& y : g.t) y.first *= c; g.k *= c; return g; };
    auto add = [&](const Form& x, const Form& y, double sy) {
        Form g = x;
        for (int q = 0; q < ns; ++q) g.a[q] += sy * y.a[q];
        for (auto& z : y.t) g.t.push_back({sy * z.first, z.second});
        g.k += sy * y.k;
        return g;
    };
    for (size_t o = 0; o < T.ops.size(); ++o) {
        const rp::Instr& I = T.ops[o];
        const double imm = o < T.imm64.size() ? T.imm64[o] : (double)I.imm;
        Form& f = row[(size_t)R0 + o];
        const Form* A = rp::is_nullary(I.code) ? nullptr : &row[(size_t)I.a];
        const Form* B = rp::is_binary(I.code) ? &row[(size_t)I.b] : nullptr;
        if ((A && !A->ok) || (B && !B->ok) || I.code == rp::OP_DATA) { f.ok = false; continue; }
        const bool u_dep = (A && has_u(*A)) || (B && has_u(*B));
        auto self = [&]() { Form g; g.a.assign((size_t)ns, 0.0); g.t.push_back({1.0, R0 + (int)o}); return g; };     // a coordinate-only row, evaluated by the source pass
        switch (I.code) {
            case rp::OP_CONST: f.k = imm; break;
            case rp::OP_ADD: f = add(*A, *B, 1.0); break;
            case rp::OP_SUB: f = add(*A, *B, -1.0); break;
            case rp::OP_NEG: f = scaled(*A, -1.0); break;
            case rp::OP_ADDC: f = *A; f.k += imm; break;
            case rp::OP_MULC: f = scaled(*A, imm); break;
            case rp::OP_MUL:
                if (is_const(*A)) f = scaled(*B, A->k);
                else if (is_const(*B)) f = scaled(*A, B->k);
                else if (!u_dep) f = self();
                else f.ok = false;
                break;
            case rp::OP_DIV:
                if (is_const(*B) && B->k != 0.0) f = scaled(*A, 1.0 / B->k);
                else if (!u_dep) f = self();
                else f.ok = false;
                break;
            default:
                if (!u_dep) f = self(); else f.ok = false;
                break;
        }
        if (f.ok && f.a.size() != (size_t)ns) f.a.assign((size_t)ns, 0.0);
    }
    const Form& out = row[(size_t)T.out_row];
    if (!out.ok) return;
    // (a MULC / DIV by a constant is not bit-identical to the tape's order of operations: the results agree to rounding, which is the mode's contract)
    std::vector<std::pair<double, int>> terms;
    for (auto& z : out.t) {
        bool merged = false;
        for (auto& y : terms) if (y.second == z.second) { y.first += z.first; merged = true; break; }
        if (!merged) terms.push_back(z);
    }
    if ((int)terms.size() > pk::F64_LIN_MAX_TERMS) return;
    F.lin = true; F.lin_a = out.a; F.lin_terms = terms; F.lin_k = out.k;
}
// S at the points of the installed set (device pass over F.d_pts), behind the coefficients in d_lin
static int f64_lin_install(pinn_engine& E, F64Term& F, const Term& T0) {
    F.lin_n = 0;
    if (!F.lin || F.n <= 0 || !F.d_pts) return 0;
    const int ns = F.nslots;
    if (F.lin_cap < F.n) {
        plat_sync(E.stream);
        plat_free(F.d_lin);
        F.d_lin = (double*)plat_malloc(sizeof(double) * ((size_t)ns + (size_t)F.n));
        F.lin_cap = F.d_lin ? F.n : 0;
        if (!F.d_lin) return fail("device allocation failed (float64 affine residual)");
    }
    if (ns > 0 && plat_h2d(F.d_lin, F.lin_a.data(), sizeof(double) * ns, E.stream)) return fail("H2D copy failed (float64 affine residual)");
    pk::F64LinSrcArgs a;
    std::memset(&a, 0, sizeof a);
    a.pts = F.d_pts; a.N = (int)F.n; a.dt = T0.d; a.np = E.np; a.nslots = ns; a.nops = F.nops;
    fill_pdef(E, a.pdef);
    a.prog = F.d_prog; a.imm = F.d_imm;
    a.nterms = (int)F.lin_terms.size();
    for (int j = 0; j < a.nterms; ++j) { a.coef[j] = F.lin_terms[j].first; a.row[j] = F.lin_terms[j].second; }
    a.k = F.lin_k;
    a.out = F.d_lin + ns;
    pk::launch_f64_lin_src(a, E.stream);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());      // (lin_a is a host vector; installs are rare)
    F.lin_n = F.n;
    return 0;
}

// feature rows of an embedded term, in double: row d_user + k = sin / cos (omega_k x coordinate src_k) of every point of the [n][T.d] host image
static void f64_embed_host(const Term& T, std::vector<double>& pts, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        for (size_t k = 0; k < T.emb_cols.size(); ++k) {
            const double ph = T.emb_cols[k].omega * pts[(size_t)i * T.d + T.emb_cols[k].src];
            pts[(size_t)i * T.d + T.d_user + k] = T.emb_cols[k].is_cos ? std::cos(ph) : std::sin(ph);
        }
}
// room for n points of d coordinates in the term's double buffer (grow-only; the stream drains before a buffer it may still read is freed — a
// no-op where it is idle already)
static int f64_grow_points(pinn_engine& E, F64Term& F, int64_t n, int d) {
    if (F.cap >= n) return 0;
    plat_sync(E.stream);
    plat_free(F.d_pts);
    F.d_pts = (double*)plat_malloc(sizeof(double) * (size_t)n * d);
    if (!F.d_pts) { F.cap = 0; return fail("device allocation failed (float64 points)"); }
    F.cap = n;
    return 0;
}
static int f64_convert_points(pinn_engine& E, F64Term& F, const Term& T) {
    // the float set as installed -> double (exact conversion of the fp32 values the fp32 kernels read)
    const int64_t n = T.n;
    F.data_n = 0;                                        // (per-point data belong to the previous set)
    if (n <= 0 || !T.d_pts) { F.n = 0; return 0; }
    std::vector<float> h((size_t)n * T.d);
    if (plat_d2h(h.data(), T.d_pts, sizeof(float) * h.size(), E.stream) || plat_sync(E.stream)) return fail("D2H copy of points failed");
    std::vector<double> hd(h.begin(), h.end());
    if (!T.emb_cols.empty()) f64_embed_host(T, hd, n);    // (the float rows hold float-rounded sin / cos: recomputed from the coordinates in double)
    if (f64_grow_points(E, F, n, T.d)) return 1;
    if (plat_h2d(F.d_pts, hd.data(), sizeof(double) * hd.size(), E.stream) || plat_sync(E.stream)) return fail("H2D copy of points failed");
    F.n = n;
    F.exact_pts = false;
    return f64_lin_install(E, F, T);
}

// the term's DATA rows in double: `src` given in double (pinn_set_point_data_f64), or the conversion of the float rows as installed
static int f64_install_data(pinn_engine& E, F64Term& F, const Term& T, const double* src) {
    const int64_t n = T.n;
    if (F.ndata == 0 || n <= 0) return 0;
    std::vector<double> hd;
    if (!src) {
        if (!T.d_data || T.data_n != n) { F.data_n = 0; return 0; }
        std::vector<float> h((size_t)F.ndata * n);
        if (plat_d2h(h.data(), T.d_data, sizeof(float) * h.size(), E.stream) || plat_sync(E.stream)) return fail("D2H copy of point data failed");
        hd.assign(h.begin(), h.end());
        src = hd.data();
    }
    if (F.data_cap < n) {
        plat_sync(E.stream);
        plat_free(F.d_data);
        F.d_data = (double*)plat_malloc(sizeof(double) * (size_t)F.ndata * n);
        if (!F.d_data) { F.data_cap = 0; return fail("device allocation failed (float64 point data)"); }
        F.data_cap = n;
    }
    if (plat_h2d(F.d_data, src, sizeof(double) * (size_t)F.ndata * n, E.stream) || plat_sync(E.stream)) return fail("H2D copy of point data failed");
    F.data_n = n;
    return 0;
}

int f64_enable(pinn_engine& E) {
    if (E.f64) return 0;
    if (E.terms0.size() != E.terms.size()) return fail("precision f64: internal (no pristine copy of the terms)");
    std::unique_ptr<F64State, void (*)(F64State*)> S(new F64State(), &f64_free);
    const F64Switches sw = f64_read_switches();
    S->terms.resize(E.terms0.size());
    for (size_t t = 0; t < E.terms0.size(); ++t) {
        const Term& T = E.terms0[t];
        F64Term& F = S->terms[t];
        const std::string who = "precision f64: term " + std::to_string(t) + ": ";
        if (!T.inodes.empty())
            return fail(who + "integral terms run on the fp32 kernels only (the float64 evaluation mode does not cover them): use precision = \"f32\"");
        std::vector<int> nets;
        for (auto& sl : T.slots) if (std::find(nets.begin(), nets.end(), sl.net) == nets.end()) nets.push_back(sl.net);
        std::sort(nets.begin(), nets.end());
        if (nets.empty()) return fail(who + "references no dependent variable");
        if ((int)nets.size() > pk::F64_MAX_NETS) return fail(who + "references more than 6 dependent variables");
        F.nets = nets;
        bool any_sin = false, all_sin = true, any_swish = false, all_swish = true;
        for (int net : nets) {
            const Net& N = E.nets[net];
            if (N.kind != 0) return fail(who + "DGM networks are not covered by the float64 mode");
            if (!f64_act_ok(N.act)) return fail(who + "this activation is not covered by the float64 mode");
            if (N.act == pk::ACT_MIXED && (int)N.sizes.size() - 2 > 8) return fail(who + "per-layer tanh / sigmoid mixes of more than 8 hidden layers are not covered by the float64 mode");
            if ((int)N.sizes.size() - 1 > pk::F64_MAX_LAYERS) return fail(who + "more than 16 Dense layers");
            if (N.sizes[0] != E.nets[nets[0]].sizes[0]) return fail(who + "its dependent variables take different numbers of arguments (one jet set serves all networks of an equation in the float64 mode)");
            any_sin = any_sin || N.act == pk::ACT_SIN;
            all_sin = all_sin && N.act == pk::ACT_SIN;
            any_swish = any_swish || N.act == pk::ACT_SWISH;
            all_swish = all_swish && N.act == pk::ACT_SWISH;
        }
        if (any_swish && !all_swish) return fail(who + "mixes swish networks with networks of another activation");
        if (any_sin && !all_sin) return fail(who + "mixes sin networks with tanh / sigmoid networks");
        // (periodic input embeddings, r06: the descriptor has rewritten the term already — sin / cos feature rows behind the user's coordinates, the
        // network mapped onto them, derivative slots as chain-rule combinations (descriptor.cpp: apply_embeddings); this mode fills the feature rows in DOUBLE)
        if (T.emb_cols.size() > 4) return fail(who + "more than 4 embedded feature rows");
        if (T.d > 4 || E.nets[nets[0]].sizes[0] > 4) return fail(who + "more than 4 coordinates");
        if ((int)T.slots.size() > pk::F64_MAX_SLOTS || T.d + E.np + (int)T.slots.size() + (int)T.ops.size() > pk::F64_MAX_ROWS)
            return fail(who + "residual expression too long for the float64 tape (96 rows)");
        F.ndata = E.terms[t].ndata;                      // (OP_DATA rows stay in this mode's tape: the float path hoists them into source channels)
        std::string why;
        F.k = f64_find(E.nets[nets[0]].sizes[0], T.slots, F.slot_chan, why);
        if (!F.k) return fail(who + why);
        F.km = f64_find_m(E, F.k, nets, sw);
        F.slot_net.clear();
        for (auto& sl : T.slots) F.slot_net.push_back((int)(std::find(nets.begin(), nets.end(), sl.net) - nets.begin()));
        F.nops = (int)T.ops.size(); F.out_row = T.out_row; F.nslots = (int)T.slots.size();
        std::vector<double> imm(T.ops.size());
        for (size_t q = 0; q < T.ops.size(); ++q) imm[q] = q < T.imm64.size() ? T.imm64[q] : (double)T.ops[q].imm;
        F.d_prog = (rp::Instr*)plat_malloc(sizeof(rp::Instr) * std::max<size_t>(T.ops.size(), 1));
        F.d_imm = (double*)plat_malloc(sizeof(double) * std::max<size_t>(T.ops.size(), 1));
        if (!F.d_prog || !F.d_imm) return fail("device allocation failed (float64 programs)");
        if (!T.ops.empty()) {
            plat_h2d(F.d_prog, T.ops.data(), sizeof(rp::Instr) * T.ops.size(), E.stream);
            plat_h2d(F.d_imm, imm.data(), sizeof(double) * imm.size(), E.stream);
            if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        }
        f64_affine(E, T, sw, F);
        if (f64_convert_points(E, F, E.terms[t])) return 1;
        if (f64_install_data(E, F, E.terms[t], nullptr)) return 1;
    }
    const int K = (int)E.terms.size();
    // (+ F64S_PAD_THETA zeroed doubles behind theta: the sliced matrix-pipe kernels read full 16 HT-wide fragments of a narrower layer's matrix)
    S->d_theta = (double*)plat_malloc(sizeof(double) * (E.ntheta + pk::F64S_PAD_THETA));
    if (S->d_theta) plat_memset(S->d_theta, 0, sizeof(double) * (E.ntheta + pk::F64S_PAD_THETA), E.stream);
    S->d_grad = (double*)plat_malloc(sizeof(double) * (E.ntheta + K));      // [gradient (P) | sums (K)] contiguous: one all-reduce over a communicator
    S->d_sumsq = S->d_grad ? S->d_grad + E.ntheta : nullptr;
    if (!S->d_theta || !S->d_grad) return fail("device allocation failed (float64 state)");
    S->h_pin = (double*)plat_host_alloc(sizeof(double) * (2 * (size_t)E.ntheta + K));
    if (!S->h_pin) return fail("pinned host allocation failed (float64 staging)");
    E.f64 = S.release();
    return 0;
}

// a float set was (re)installed through pinn_set_points while the mode is on: keep the double copy in step
int f64_points_changed(pinn_engine& E, int term) {
    if (!E.f64) return 0;
    return f64_convert_points(E, state(E).terms[term], E.terms[term]);
}

double* f64_points_reserve(pinn_engine& E, int term, int64_t n) {
    F64Term& F = state(E).terms[term];
    return f64_grow_points(E, F, n, E.terms[term].d) ? nullptr : F.d_pts;
}
// the term's double point buffer holds a new set of n points, as given in double
int f64_points_written(pinn_engine& E, int term, int64_t n) {
    F64Term& F = state(E).terms[term];
    F.n = n;
    F.exact_pts = true;
    return f64_lin_install(E, F, E.terms[term]);
}

int f64_set_points(pinn_engine& E, int term, const double* pts, int64_t n) {
    F64Term& F = state(E).terms[term];
    const Term& T = E.terms[term];
    if (!f64_points_reserve(E, term, n)) return 1;
    if (T.emb_cols.empty()) {
        if (plat_h2d(F.d_pts, pts, sizeof(double) * (size_t)n * T.d, E.stream) || plat_sync(E.stream)) return fail("H2D copy of points failed");
    } else {                                             // the caller's [n][d_user] coordinates + the feature rows
        std::vector<double> hd((size_t)n * T.d);
        for (int64_t i = 0; i < n; ++i)
            for (int j = 0; j < T.d_user; ++j) hd[(size_t)i * T.d + j] = pts[(size_t)i * T.d_user + j];
        f64_embed_host(T, hd, n);
        if (plat_h2d(F.d_pts, hd.data(), sizeof(double) * hd.size(), E.stream) || plat_sync(E.stream)) return fail("H2D copy of points failed");
    }
    return f64_points_written(E, term, n);
}

// pinn_set_point_data while the mode is on: the double rows follow (data == nullptr: converted from the float rows just installed)
int f64_set_point_data(pinn_engine& E, int term, const double* data) {
    if (!E.f64) return 0;
    return f64_install_data(E, state(E).terms[term], E.terms[term], data);
}

// a sampled term's float points (just redrawn on the device) -> the double copy the float64 kernels read
int f64_points_from_device(pinn_engine& E, int term) {
    F64Term& F = state(E).terms[term];
    const Term& T = E.terms[term];
    if (f64_grow_points(E, F, T.n, T.d)) return 1;
    if (T.emb_cols.empty()) pk::launch_f64_cvt(T.d_pts, F.d_pts, (int64_t)T.n * T.d, E.stream);
    else {                                               // the draw lives in d_upts [n][d_user] (the float feature rows are not refreshed by this loop): widened, features in double
        pk::F64EmbedArgs ea;
        ea.pts = F.d_pts; ea.upts = T.d_upts; ea.n = (int)T.n; ea.d = T.d; ea.du = T.d_user; ea.ncols = (int)T.emb_cols.size();
        for (int k = 0; k < ea.ncols; ++k) { ea.src[k] = T.emb_cols[k].src; ea.is_cos[k] = T.emb_cols[k].is_cos; ea.omega[k] = T.emb_cols[k].omega; }
        pk::launch_f64_embed(ea, E.stream);
    }
    F.n = T.n;
    F.exact_pts = false;
    F.lin_n = 0;                                         // (a redrawn set: the affine fast path's per-point part is not recomputed inside the loop — the tape runs)
    F.data_n = 0;                                        // (per-point data belong to the previous set: a sampled term with DATA channels fails its next evaluation with the message — ADVICE r05)
    return 0;
}

}  // namespace pe
