// f64_stencil.cpp — the reference-semantics ("stencil") validation mode of the float64 evaluation (pinn_set_option(h, "derivative", "stencil")):
// derivative slots by the reference's own central differences instead of exact jets.  Kernels: pinn_kernels4.hpp (k_f64_shift, k_f64_stape);
// the seeded launches go through f64.cpp's chunk launcher.
#include "f64_internal.hpp"

namespace pe {

// ---- the reference-semantics ("stencil") validation mode ----
// get_eps (src/symbolic_utilities.jl:98-103): eps(Float64)^(1 / (2 + order)), the TOTAL order of the derivative on every axis (:185)
static double stencil_eps(int order) { return std::pow(2.220446049250313e-16, 1.0 / (2.0 + (double)order)); }
namespace {
struct StOperand { int kind, idx; };     // 0: virtual network idx, 1: stencil op idx, 2: an original row below the slots (coordinate / parameter)
struct StBuilder {
    std::vector<F64VNet> vnets;
    struct Op { int code; StOperand a, b; double imm; };
    std::vector<Op> ops;
    int vnet(int net, const std::vector<std::pair<int, double>>& sh) {
        for (size_t i = 0; i < vnets.size(); ++i) if (vnets[i].net == net && vnets[i].shifts == sh) return (int)i;
        vnets.push_back({net, sh});
        return (int)vnets.size() - 1;
    }
    StOperand op(int code, StOperand a, StOperand b, double imm) { ops.push_back({code, a, b, imm}); return {1, (int)ops.size() - 1}; }
    StOperand mulc(StOperand a, double c) { return op(rp::OP_MULC, a, {2, 0}, c); }
    StOperand u(int net, std::vector<std::pair<int, double>> sh, int axis, double delta) {
        sh.push_back({axis, delta});
        return {0, vnet(net, sh)};
    }
    // numeric_derivative(phi, u, x, eps_s, order, theta) (src/pinn_types.jl:445-482) at the points shifted by `sh`: axes[0 .. k) = the derivative
    // variables, eps = the step (one magnitude for all axes: the total order's); the formulas in the reference's own order of operations
    StOperand deriv(int net, const int* axes, int k, double eps, const std::vector<std::pair<int, double>>& sh) {
        if (k == 0) return {0, vnet(net, sh)};
        const double inv = 1.0 / eps;                    // _epsilon = inv(first(eps[eps .!= 0]))
        const int ax = axes[k - 1];                      // eps = eps_s[order]
        bool same = true;
        for (int i = 1; i < k; ++i) same = same && axes[i] == axes[0];
        if (k > 4 || !same) {                            // :454-460
            auto up = sh, dn = sh;
            up.push_back({ax, eps}); dn.push_back({ax, -eps});
            const StOperand a = deriv(net, axes, k - 1, eps, up), b = deriv(net, axes, k - 1, eps, dn);
            return mulc(mulc(op(rp::OP_SUB, a, b, 0.0), inv), 0.5);
        }
        if (k == 4) {                                    // :461-468: (u(x+2e) - 4u(x+e) + 6u(x) - 4u(x-e) + u(x-2e)) * _epsilon^4
            StOperand t = op(rp::OP_SUB, u(net, sh, ax, 2.0 * eps), mulc(u(net, sh, ax, eps), 4.0), 0.0);
            t = op(rp::OP_ADD, t, mulc({0, vnet(net, sh)}, 6.0), 0.0);
            t = op(rp::OP_SUB, t, mulc(u(net, sh, ax, -eps), 4.0), 0.0);
            t = op(rp::OP_ADD, t, u(net, sh, ax, -2.0 * eps), 0.0);
            return mulc(t, (inv * inv) * (inv * inv));
        }
        if (k == 3) {                                    // :469-474: (u(x+2e) - 2u(x+e) + 2u(x-e) - u(x-2e)) * _epsilon^3 / 2
            StOperand t = op(rp::OP_SUB, u(net, sh, ax, 2.0 * eps), mulc(u(net, sh, ax, eps), 2.0), 0.0);
            t = op(rp::OP_ADD, t, mulc(u(net, sh, ax, -eps), 2.0), 0.0);
            t = op(rp::OP_SUB, t, u(net, sh, ax, -2.0 * eps), 0.0);
            return mulc(mulc(t, inv * inv * inv), 0.5);
        }
        if (k == 2) {                                    // :475-476: (u(x+e) + u(x-e) - 2u(x)) * _epsilon^2
            StOperand t = op(rp::OP_ADD, u(net, sh, ax, eps), u(net, sh, ax, -eps), 0.0);
            t = op(rp::OP_SUB, t, mulc({0, vnet(net, sh)}, 2.0), 0.0);
            return mulc(t, inv * inv);
        }
        return mulc(mulc(op(rp::OP_SUB, u(net, sh, ax, eps), u(net, sh, ax, -eps), 0.0), inv), 0.5);      // :477-478
    }
};
}  // namespace

// build every term's stencil tape (pinn_set_option(h, "derivative", "stencil"); the float64 mode must be on)
int f64_stencil_enable(pinn_engine& E, bool on) {
    if (!E.f64) return fail("pinn_set_option: \"derivative\" = \"stencil\" is a validation mode of the float64 evaluation (set \"precision\" to \"f64\" first)");
    F64State& S = state(E);
    if (!on) { S.stencil = false; return 0; }
    if (!S.sten.empty()) { S.stencil = true; return 0; }
    std::vector<F64Stencil> sten(E.terms0.size());
    struct Guard {                                       // (a failure below must not leak the tapes already uploaded)
        std::vector<F64Stencil>& v; bool armed = true;
        ~Guard() { if (armed) for (auto& X : v) { plat_free(X.d_prog); plat_free(X.d_imm); } }
    } guard{sten};
    for (size_t t = 0; t < E.terms0.size(); ++t) {
        const Term& T = E.terms0[t];
        F64Stencil& X = sten[t];
        const std::string who = "derivative = stencil: term " + std::to_string(t) + ": ";
        for (auto& sl : T.slots) X.active = X.active || sl.order > 0 || sl.lap != 0;
        if (!X.active) continue;
        if (!T.emb_cols.empty()) return fail(who + "the term reads a network behind a periodic input embedding: its derivative slots are derivatives with respect to the sin / cos FEATURES (descriptor rewrite), central differences of which are not the reference's differences in the coordinates");
        StBuilder B;
        std::vector<StOperand> slot_val;
        for (auto& sl : T.slots) {
            if (sl.lap) return fail(who + "internal (a fused Laplacian slot in the pristine term)");
            slot_val.push_back(B.deriv(sl.net, sl.axes, sl.order, stencil_eps(sl.order), {}));
        }
        const int dt = T.d, np = E.np, nv = (int)B.vnets.size(), nold = (int)T.slots.size(), npre = (int)B.ops.size();
        if (nv > pk::F64_MAX_SLOTS || dt + np + nv + npre + (int)T.ops.size() > pk::F64_MAX_ROWS)
            return fail(who + "the stencil tape needs " + std::to_string(dt + np + nv + npre + (int)T.ops.size()) + " rows / " + std::to_string(nv) + " shifted evaluations (limits: 96 / 24)");
        for (auto& vn : B.vnets)
            if (vn.shifts.size() > 8) return fail(who + "derivative order above 8");
        auto row = [&](StOperand o) { return o.kind == 0 ? dt + np + o.idx : (o.kind == 1 ? dt + np + nv + o.idx : o.idx); };
        std::vector<rp::Instr> prog;
        std::vector<double> imm;
        for (auto& o : B.ops) {
            rp::Instr I;
            std::memset(&I, 0, sizeof I);
            I.code = o.code; I.a = row(o.a); I.b = rp::is_binary(o.code) ? row(o.b) : 0; I.imm = (float)o.imm;
            rp::finalize(I);
            prog.push_back(I); imm.push_back(o.imm);
        }
        auto remap = [&](int r) {                        // a row of the term's own numbering [coordinates | params | slots | ops]
            if (r < dt + np) return r;
            if (r < dt + np + nold) return row(slot_val[r - dt - np]);
            return dt + np + nv + npre + (r - dt - np - nold);
        };
        for (size_t q = 0; q < T.ops.size(); ++q) {
            rp::Instr I = T.ops[q];
            if (!rp::is_nullary(I.code)) I.a = remap(I.a);
            if (rp::is_binary(I.code)) I.b = remap(I.b);
            prog.push_back(I);
            imm.push_back(q < T.imm64.size() ? T.imm64[q] : (double)T.ops[q].imm);
        }
        X.vnets = B.vnets;
        X.nops = (int)prog.size();
        X.out_row = remap(T.out_row);
        X.d_prog = (rp::Instr*)plat_malloc(sizeof(rp::Instr) * std::max<size_t>(prog.size(), 1));
        X.d_imm = (double*)plat_malloc(sizeof(double) * std::max<size_t>(prog.size(), 1));
        if (!X.d_prog || !X.d_imm) return fail("device allocation failed (stencil tape)");
        plat_h2d(X.d_prog, prog.data(), sizeof(rp::Instr) * prog.size(), E.stream);
        plat_h2d(X.d_imm, imm.data(), sizeof(double) * imm.size(), E.stream);
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    }
    guard.armed = false;
    S.sten.swap(sten);
    S.stencil = true;
    return 0;
}
bool f64_stencil_on(const pinn_engine& E) { return E.f64 && state(E).stencil; }

// the value-only pseudo-term of virtual network `vn` of term t on its shifted set
static int stencil_vnet_term(pinn_engine& E, const F64VNet& vn, double* d_pts, int64_t n, F64Term& F) {
    const Net& N = E.nets[vn.net];
    std::string why;
    Slot sl;
    sl.net = vn.net; sl.order = 0; sl.lap = 0;
    for (int q = 0; q < MAX_DERIV_ORDER; ++q) sl.axes[q] = 0;
    F.k = f64_find(N.sizes[0], std::vector<Slot>{sl}, F.slot_chan, why);
    if (!F.k) return fail("derivative = stencil: " + why);
    F.km = nullptr;                                      // (one lane per point: a validation mode)
    F.nets = {vn.net};
    F.slot_net = {0};
    F.nops = 0; F.nslots = 1; F.out_row = N.sizes[0] + E.np;
    F.n = n;
    F.d_pts = d_pts;
    return 0;
}
// one term in stencil mode.  mode 0: loss + gradient (accumulated into `grad`, which the caller has zeroed), 1: loss only, 2: residuals into d_resid
int f64_stencil_term(pinn_engine& E, const F64Switches& sw, int t, const double* theta, double* grad, double* sumsq_t, double w, int mode, double* d_resid) {
    F64State& S = state(E);
    const F64Stencil& X = S.sten[t];
    const F64Term& F0 = S.terms[t];
    const Term& T = E.terms[t];
    const Term& T0 = E.terms0[t];
    const int64_t n = F0.n;
    const int nv = (int)X.vnets.size(), stride = 2 + E.ne;
    int dmax = 1;
    for (auto& vn : X.vnets) dmax = std::max(dmax, E.nets[vn.net].sizes[0]);
    if (!dev_grow(S.d_uv, S.uv_cap, (size_t)nv * n, E.stream) || !dev_grow(S.d_seeds, S.seeds_cap, (size_t)nv * n * stride, E.stream) ||
        !dev_grow(S.d_spts, S.spts_cap, (size_t)nv * n * dmax, E.stream)) return fail("device allocation failed (stencil evaluation)");
    // 1. shifted sets and the virtual networks' values
    for (int v = 0; v < nv; ++v) {
        const F64VNet& vn = X.vnets[v];
        pk::F64ShiftArgs sa;
        std::memset(&sa, 0, sizeof sa);
        sa.pts = F0.d_pts; sa.dt = T0.d; sa.out = S.d_spts + (size_t)v * n * dmax; sa.d = E.nets[vn.net].sizes[0]; sa.n = (int)n;
        input_binding(E, vn.net, &T0.inmap, sa.imap);
        sa.nshift = (int)vn.shifts.size();
        for (int q = 0; q < sa.nshift; ++q) { sa.axis[q] = vn.shifts[q].first; sa.delta[q] = vn.shifts[q].second; }
        pk::launch_f64_shift(sa, E.stream);
        F64Term F;
        F64Launch L;
        if (stencil_vnet_term(E, vn, sa.out, n, F) || f64_build(E, F, sa.d, nullptr, sw, L)) return 1;
        L.a.theta = theta;
        if (f64_values(E, S, F, L, n, S.d_uv + (size_t)v * n)) return 1;
    }
    // 2. the stencil tape: residuals / squared residuals / seeds
    pk::F64StapeArgs ta;
    std::memset(&ta, 0, sizeof ta);
    ta.pts = F0.d_pts; ta.dt = T0.d; ta.n = (int)n; ta.theta = theta;
    ta.np = E.np; ta.ne = E.ne; ta.p_off = E.p_theta_off;
    fill_pdef(E, ta.pdef);
    ta.pw = term_pw(T);
    ta.data = F0.ndata > 0 ? F0.d_data : nullptr;
    ta.uv = S.d_uv; ta.nv = nv;
    ta.prog = X.d_prog; ta.imm = X.d_imm; ta.nops = X.nops; ta.out_row = X.out_row;
    ta.scale = f64_term_scale(T, w);
    ta.mode = mode; ta.resid = d_resid; ta.seeds = S.d_seeds; ta.seed_stride = stride;
    pk::launch_f64_stape(ta, E.stream);
    if (mode == 2) return 0;
    // 3. seeded launches: the squared residuals ride in virtual network 0's records; loss only: that launch alone
    for (int v = 0; v < (mode == 1 ? 1 : nv); ++v) {
        const F64VNet& vn = X.vnets[v];
        F64Term F;
        F64Launch L;
        if (stencil_vnet_term(E, vn, S.d_spts + (size_t)v * n * dmax, n, F) || f64_build(E, F, E.nets[vn.net].sizes[0], nullptr, sw, L)) return 1;
        pk::F64Args& a = L.a;
        a.theta = theta; a.mode = mode; a.scale = 0.0;
        a.seed = S.d_seeds + (size_t)v * n * stride; a.seed_stride = stride;
        const int rc = f64_for_chunks(E, S, L, n, true, [&] {
            pk::F64ReduceArgs r = f64_reduce_into(sumsq_t, v == 0 && a.p0 == 0);
            f64_launch_chunk(E, S, F, L, grad, nullptr, r);          // (no GradStart: every seeded launch adds to the zeroed gradient)
        });
        if (rc) return rc;
    }
    return 0;
}

}  // namespace pe
