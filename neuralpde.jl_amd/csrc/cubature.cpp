// cubature.cpp — h-adaptive cubature of a term's loss (1 / area) int r^2 dx, resident on the device: pinn_cubature_refine / _get (DESIGN.md section
// 4.13).  A ROUND = cub::k_cub_nodes (the Genz-Malik nodes of the pending boxes, written as the term's point set) + the term's own residual kernel
// over them (engine.cpp: residual_device / f64.cpp: f64_residual_device) + cub::k_cub_estimate + cub::k_cub_plan + one download of cub::Rec;
// cub::k_cub_split when the record says so.  After the last round cub::k_cub_emit writes a composite tensor Gauss-Legendre rule on the final mesh
// into the term's point and weight buffers, and the bookkeeping of pinn_set_points / pinn_set_point_weights follows: from there the set is an
// ordinary weighted point set.  While the rounds run, the term's point buffer is the scratch the nodes are evaluated from.
// The region lists have buffers of their own, one per refined term, and stay until pinn_destroy (pinn_cubature_get reads them).
#include "resident.hpp"
#include "cub_kernels.hpp"

using namespace pe;

namespace {

// Gauss-Legendre rules with 1..8 nodes on [-1, 1]: the nodes, and the weights halved (fractions of the mean), as doubles — the values
// numpy.polynomial.legendre.leggauss returns, so that a caller can restate the emitted set bit for bit
const double GL_X[cub::MAX_GAUSS][cub::MAX_GAUSS] = {
    {0.0},
    {-0.5773502691896257, 0.5773502691896257},
    {-0.7745966692414834, 0.0, 0.7745966692414834},
    {-0.8611363115940526, -0.33998104358485626, 0.33998104358485626, 0.8611363115940526},
    {-0.906179845938664, -0.5384693101056831, 0.0, 0.5384693101056831, 0.906179845938664},
    {-0.932469514203152, -0.6612093864662645, -0.23861918608319693, 0.23861918608319693, 0.6612093864662645, 0.932469514203152},
    {-0.9491079123427585, -0.7415311855993945, -0.4058451513773972, 0.0, 0.4058451513773972, 0.7415311855993945, 0.9491079123427585},
    {-0.9602898564975362, -0.7966664774136267, -0.525532409916329, -0.18343464249564978, 0.18343464249564978, 0.525532409916329, 0.7966664774136267, 0.9602898564975362},
};
const double GL_W[cub::MAX_GAUSS][cub::MAX_GAUSS] = {
    {1.0},
    {0.5, 0.5},
    {0.27777777777777785, 0.4444444444444444, 0.27777777777777785},
    {0.17392742256872684, 0.3260725774312731, 0.3260725774312731, 0.17392742256872684},
    {0.11846344252809471, 0.2393143352496831, 0.2844444444444445, 0.2393143352496831, 0.11846344252809471},
    {0.08566224618958487, 0.18038078652406947, 0.23395696728634569, 0.23395696728634569, 0.18038078652406947, 0.08566224618958487},
    {0.06474248308443532, 0.1398526957446383, 0.19091502525255916, 0.20897959183673448, 0.19091502525255916, 0.1398526957446383, 0.06474248308443532},
    {0.050614268145188344, 0.11119051722668717, 0.15685332293894352, 0.18134189168918088, 0.18134189168918088, 0.15685332293894352, 0.11119051722668717, 0.050614268145188344},
};

// the region list of one term and what the last refinement left in it
struct Mesh {
    double* d_c = nullptr; double* d_h = nullptr;        // [cap][MAX_FREE]
    double* d_share = nullptr; double* d_I7 = nullptr; double* d_err = nullptr;
    int* d_axis = nullptr; int* d_slot = nullptr; int* d_pend = nullptr;
    size_t cap = 0;                                      // boxes
    int nb = 0, nf = 0, d = 0;
    int free_ax[cub::MAX_FREE] = {};
    double fixed[cub::MAX_D] = {};
    void release() {
        plat_free(d_c); plat_free(d_h); plat_free(d_share); plat_free(d_I7); plat_free(d_err); plat_free(d_axis); plat_free(d_slot); plat_free(d_pend);
        *this = Mesh();
    }
    bool reserve(size_t n, plat_stream st) {
        if (cap >= n) return true;
        plat_sync(st);
        release();
        d_c = (double*)plat_malloc(sizeof(double) * n * cub::MAX_FREE);
        d_h = (double*)plat_malloc(sizeof(double) * n * cub::MAX_FREE);
        d_share = (double*)plat_malloc(sizeof(double) * n);
        d_I7 = (double*)plat_malloc(sizeof(double) * n);
        d_err = (double*)plat_malloc(sizeof(double) * n);
        d_axis = (int*)plat_malloc(sizeof(int) * n);
        d_slot = (int*)plat_malloc(sizeof(int) * n);
        d_pend = (int*)plat_malloc(sizeof(int) * n);
        if (!d_c || !d_h || !d_share || !d_I7 || !d_err || !d_axis || !d_slot || !d_pend) { release(); return false; }
        cap = n;
        return true;
    }
};

}  // namespace

enum { PH_NODES = 0, PH_EVAL, PH_ESTIMATE, PH_PLAN, PH_SPLIT, PH_EMIT, PH_COUNT };
struct pe::CubState {
    std::map<int, Mesh> mesh;            // per refined term
    cub::Rec* d_rec = nullptr;
    // pinn_set_timing level 2: events at the phase boundaries of a round, read after the round's one synchronisation
    plat_event ev[PH_COUNT + 3];         // [PH_COUNT + 1], [PH_COUNT + 2]: around k_cub_split, read after the NEXT round's synchronisation
    bool have_events = false;
    float phase_ms[PH_COUNT] = {};
};

void pe::cub_free(pinn_engine& E) {
    if (!E.cub) return;
    for (auto& m : E.cub->mesh) m.second.release();
    plat_free(E.cub->d_rec);
    if (E.cub->have_events) for (auto& e : E.cub->ev) plat_event_destroy(e);
    delete E.cub;
    E.cub = nullptr;
}
const float* pe::cub_phase_ms(const pinn_engine& E) {
    static const float none[PH_COUNT] = {};
    return E.cub ? E.cub->phase_ms : none;
}

namespace {

// the rule's weights per node class for n free axes (fractions of the mean)
void genz_malik_weights(int n, double* w7, double* w5) {
    const double dn = (double)n;
    w7[0] = (12824.0 - 9120.0 * dn + 400.0 * dn * dn) / 19683.0;
    w7[1] = 980.0 / 6561.0;
    w7[2] = (1820.0 - 400.0 * dn) / 19683.0;
    w7[3] = 200.0 / 19683.0;
    w7[4] = 6859.0 / 19683.0 / (double)(1 << n);
    w5[0] = (729.0 - 950.0 * dn + 50.0 * dn * dn) / 729.0;
    w5[1] = 245.0 / 486.0;
    w5[2] = (265.0 - 100.0 * dn) / 1458.0;
    w5[3] = 25.0 / 729.0;
    w5[4] = 0.0;
}

// nodes of the pending boxes -> the term's point set -> its residual there; returns the device array of the n = npend M values through r32 / r64
// (`mark`: the event between the two phases, at timing level 2)
int evaluate_pending(pinn_engine& E, int term, const cub::Args& a, const float** r32, const double** r64, plat_event* mark) {
    const int64_t n = (int64_t)a.npend * a.M;
    if (E.f64) {
        double* pts = f64_points_reserve(E, term, n);
        if (!pts) return 1;
        cub::launch_nodes<double>(a, pts, E.stream);
        if (f64_points_written(E, term, n)) return 1;
        if (mark) plat_event_record(*mark, E.stream);
        return f64_residual_device(E, term, r64);
    }
    if (points_reserve(E, term, n)) return 1;
    cub::launch_nodes<float>(a, E.terms[term].d_pts, E.stream);
    if (points_written(E, term, n, n)) return 1;
    if (mark) plat_event_record(*mark, E.stream);
    if (residual_device(E, term)) return 1;
    *r32 = E.terms[term].d_resid;
    return 0;
}

}  // namespace

extern "C" {

int pinn_cubature_refine(pinn_handle h, int term, const double* theta, int64_t p, const double* lb, const double* ub, int d, double reltol, double abstol,
                         int max_regions, int max_rounds, int nodes, double* integral, double* error, int64_t* nregions, int64_t* npoints, int* rounds,
                         int* status) {
    const std::string who = "pinn_cubature_refine: ";
    if (!h || !theta || !lb || !ub) return fail(who + "null argument");
    pinn_engine& E = *h;
    if (term < 0 || term >= (int)E.terms.size()) return fail(who + "term index out of range");
    if (check_theta(E, "pinn_cubature_refine", p)) return 1;
    const Term& T0 = E.terms[term];
    if (E.comm) return fail(who + "the handle belongs to a communicator; the refinement runs on a single device only");
    if (T0.sampler != 0) return fail(who + "the term redraws its points on the device (a device sampler); remove the sampler first");
    if (!T0.inodes.empty()) return fail(who + "integral terms are not covered");
    if (T0.ndata > 0) return fail(who + "terms with per-point data channels are not covered (the data belong to a fixed point set)");
    if (!T0.emb_cols.empty()) return fail(who + "terms behind a periodic input embedding are not covered");
    if (E.f64 && f64_stencil_on(E)) return fail(who + "the stencil derivative mode is not covered (use derivative = exact)");
    if (d != T0.d_user || d > cub::MAX_D) return fail(who + "d = " + std::to_string(d) + " != the term's " + std::to_string(T0.d_user) + " coordinates");
    if (nodes < 1 || nodes > cub::MAX_GAUSS) return fail(who + "nodes must be in 1..8");
    if (!(reltol >= 0.0) || !(abstol >= 0.0)) return fail(who + "negative tolerance");
    if (max_regions < 1) return fail(who + "max_regions must be at least 1");
    if (max_rounds < 0) return fail(who + "max_rounds must not be negative");
    cub::Args a;
    std::memset(&a, 0, sizeof a);
    a.d = d;
    for (int i = 0; i < d; ++i) {
        if (!(lb[i] <= ub[i])) return fail(who + "lb > ub on coordinate " + std::to_string(i));
        a.fixed[i] = lb[i];
        if (lb[i] < ub[i]) a.free_ax[a.nf++] = i;      // (d <= MAX_D <= MAX_FREE)
    }
    if (a.nf == 0) return fail(who + "zero free axes (lb == ub on every coordinate)");
    a.M = cub::node_count(a.nf);
    int64_t npl = 1;
    for (int k = 0; k < a.nf; ++k) npl *= nodes;
    if ((int64_t)max_regions * std::max<int64_t>(npl, a.M) * d >= (int64_t)1 << 31)
        return fail(who + "max_regions x points per region exceeds 32-bit indexing of a point set; lower max_regions or nodes");
    genz_malik_weights(a.nf, a.w7, a.w5);

    DeviceScope scope(E.device);
    if (!E.cub) E.cub = new CubState();
    CubState& S = *E.cub;
    if (!S.d_rec) S.d_rec = (cub::Rec*)plat_malloc(sizeof(cub::Rec));
    Mesh& Mh = S.mesh[term];
    if (!S.d_rec || !Mh.reserve((size_t)max_regions, E.stream)) return fail(who + "device allocation failed (region list)");
    a.c = Mh.d_c; a.h = Mh.d_h; a.share = Mh.d_share; a.I7 = Mh.d_I7; a.err = Mh.d_err; a.axis = Mh.d_axis; a.slot = Mh.d_slot; a.pend = Mh.d_pend;
    a.rec = S.d_rec;
    Mh.nb = 0; Mh.nf = a.nf; Mh.d = d;
    std::copy(a.free_ax, a.free_ax + cub::MAX_FREE, Mh.free_ax);
    std::copy(a.fixed, a.fixed + cub::MAX_D, Mh.fixed);

    // the parameters of every evaluation of this call, and the root box
    if (E.f64) {
        if (f64_upload_theta(E, theta)) return 1;
    } else {
        auto th = as<float>(theta, (size_t)p);
        if (upload_theta(E, th.get(), E.ntheta)) return 1;
        pack_all(E);
        jit_take_launch_error();
    }
    double root[2 * cub::MAX_FREE] = {};
    const double one = 1.0;
    const int zero = 0;
    for (int k = 0; k < a.nf; ++k) {
        root[k] = 0.5 * (lb[a.free_ax[k]] + ub[a.free_ax[k]]);
        root[cub::MAX_FREE + k] = 0.5 * (ub[a.free_ax[k]] - lb[a.free_ax[k]]);
    }
    if (plat_h2d(Mh.d_c, root, sizeof(double) * cub::MAX_FREE, E.stream) || plat_h2d(Mh.d_h, root + cub::MAX_FREE, sizeof(double) * cub::MAX_FREE, E.stream) ||
        plat_h2d(Mh.d_share, &one, sizeof(double), E.stream) || plat_h2d(Mh.d_pend, &zero, sizeof(int), E.stream) || plat_sync(E.stream))
        return fail(who + "H2D copy failed");

    const bool timed = E.timing_level >= 2;
    if (timed && !S.have_events) { for (auto& e : S.ev) plat_event_create(e); S.have_events = true; }
    std::fill(S.phase_ms, S.phase_ms + PH_COUNT, 0.f);
    auto mark = [&](int i) { if (timed) plat_event_record(S.ev[i], E.stream); };
    auto account = [&](int first, int last) { if (timed) for (int i = first; i < last; ++i) S.phase_ms[i] += plat_event_ms(S.ev[i], S.ev[i + 1]); };

    a.nb = 1; a.npend = 1;
    cub::Rec rec;
    int nrounds = 0;
    bool split_pending = false;
    for (;;) {
        mark(PH_NODES);
        const float* r32 = nullptr;
        const double* r64 = nullptr;
        if (evaluate_pending(E, term, a, &r32, &r64, timed ? &S.ev[PH_EVAL] : nullptr)) return 1;
        mark(PH_ESTIMATE);
        if (E.f64) cub::launch_estimate<double>(a, r64, E.stream);
        else cub::launch_estimate<float>(a, r32, E.stream);
        mark(PH_PLAN);
        cub::launch_plan(a, reltol, abstol, max_regions, nrounds < max_rounds ? 1 : 0, E.stream);
        if (plat_d2h(&rec, S.d_rec, sizeof(cub::Rec), E.stream)) return fail(who + "D2H copy failed");
        mark(PH_SPLIT);
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        account(PH_NODES, PH_SPLIT);
        if (split_pending) S.phase_ms[PH_SPLIT] += plat_event_ms(S.ev[PH_COUNT + 1], S.ev[PH_COUNT + 2]);
        if (!E.f64) { const std::string le = jit_take_launch_error(); if (!le.empty()) return fail(who + le); }
        if (rec.status != cub::ST_SPLIT) break;
        mark(PH_COUNT + 1);
        cub::launch_split(a, E.stream);
        mark(PH_COUNT + 2);
        split_pending = timed;
        a.nb = rec.nboxes; a.npend = rec.npending;
        ++nrounds;
    }
    Mh.nb = a.nb;

    // the composite Gauss-Legendre rule on the final mesh, straight into the term's buffers
    const int64_t n = (int64_t)a.nb * npl;
    cub::EmitArgs e;
    std::memset(&e, 0, sizeof e);
    e.G = nodes; e.npl = (int)npl; e.n_norm = (double)n;
    std::copy(GL_X[nodes - 1], GL_X[nodes - 1] + nodes, e.gx);
    std::copy(GL_W[nodes - 1], GL_W[nodes - 1] + nodes, e.gw);
    if (points_reserve(E, term, n) || weights_reserve(E, term, n)) return 1;
    mark(PH_EMIT);
    e.pw = E.terms[term].d_pw;
    if (E.f64) {
        double* pts = f64_points_reserve(E, term, n);
        if (!pts) return 1;
        e.pts32 = E.terms[term].d_pts;
        cub::launch_emit<double>(a, e, pts, E.stream);
    } else {
        cub::launch_emit<float>(a, e, E.terms[term].d_pts, E.stream);
    }
    if (points_written(E, term, n, n)) return 1;
    if (E.f64 && f64_points_written(E, term, n)) return 1;
    weights_written(E, term, n);
    mark(PH_COUNT);
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    account(PH_EMIT, PH_COUNT);

    if (integral) *integral = rec.I;
    if (error) *error = rec.E;
    if (nregions) *nregions = a.nb;
    if (npoints) *npoints = n;
    if (rounds) *rounds = nrounds;
    if (status) *status = rec.status;
    return 0;
}

int pinn_cubature_get(pinn_handle h, int term, double* boxes, double* est, int64_t nregions) {
    const std::string who = "pinn_cubature_get: ";
    if (!h) return fail(who + "null handle");
    pinn_engine& E = *h;
    if (!E.cub || !E.cub->mesh.count(term) || E.cub->mesh[term].nb == 0) return fail(who + "the term has no region list (call pinn_cubature_refine first)");
    const Mesh& Mh = E.cub->mesh[term];
    if (nregions != Mh.nb) return fail(who + "the region list holds " + std::to_string(Mh.nb) + " regions");
    DeviceScope scope(E.device);
    const size_t nb = (size_t)Mh.nb;
    std::vector<double> c(nb * cub::MAX_FREE), hw(nb * cub::MAX_FREE), i7(nb), er(nb);
    if (plat_d2h(c.data(), Mh.d_c, sizeof(double) * c.size(), E.stream) || plat_d2h(hw.data(), Mh.d_h, sizeof(double) * hw.size(), E.stream) ||
        plat_d2h(i7.data(), Mh.d_I7, sizeof(double) * nb, E.stream) || plat_d2h(er.data(), Mh.d_err, sizeof(double) * nb, E.stream) || plat_sync(E.stream))
        return fail(who + "D2H copy failed");
    for (size_t i = 0; i < nb; ++i) {
        if (boxes) {
            double* lo = boxes + i * 2 * Mh.d;
            double* hi = lo + Mh.d;
            for (int j = 0; j < Mh.d; ++j) lo[j] = hi[j] = Mh.fixed[j];
            for (int k = 0; k < Mh.nf; ++k) {
                lo[Mh.free_ax[k]] = c[i * cub::MAX_FREE + k] - hw[i * cub::MAX_FREE + k];
                hi[Mh.free_ax[k]] = c[i * cub::MAX_FREE + k] + hw[i * cub::MAX_FREE + k];
            }
        }
        if (est) { est[2 * i] = i7[i]; est[2 * i + 1] = er[i]; }
    }
    return 0;
}

}  // extern "C"
