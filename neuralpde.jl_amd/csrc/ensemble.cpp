// ensemble.cpp — ensemble prediction (pinn_phi_ensemble): phi of one network at S parameter vectors and n points + the mean / standard
// deviation over the S predictions (ens_kernels.hpp).  One upload of the parameter vectors, one of the points, the launches back to back on
// the handle's stream, one download.  The buffers belong to this entry point and grow on demand; nothing else of the handle is touched.
#include <array>
#include "resident.hpp"
#include "ens_kernels.hpp"

using namespace pe;

struct pe::EnsState {
    void* d_th = nullptr; void* d_pts = nullptr;         // [S][P] | [n][d] in the compute type
    double* d_preds = nullptr; double* d_stat = nullptr; // [requests][S][points of one pass] | [mean requests x n | std requests x n]  (pinn_phi_ensemble: one request)
    void* d_scr = nullptr;                               // pinn_derivative_ensemble: the image regions of the scratch storage
    size_t th_cap = 0, pts_cap = 0, scr_cap = 0;         // bytes
    size_t preds_cap = 0, stat_cap = 0;                  // doubles
    int jet_passes = 0, point_passes = 0, scratch_passes = 0;      // of the last pinn_derivative_ensemble call (pinn_get_option "ens_passes", ...)
};

// the device-memory budget in bytes ($PINN_ENS_GB, default 4; read per call)
static double ens_budget_bytes() {
    double gb = 4.0;
    if (const char* e = std::getenv("PINN_ENS_GB")) { const double v = std::atof(e); if (v > 0.0) gb = v; }
    return gb * 1073741824.0;
}

// Requests -> jet passes, so that no network forward runs more often than needed.  Request j is d^orders[j] / dx_axes[4j ..]; `d` = inputs of the
// network.  Every mixed second derivative (a, b) takes a two-axis pass (u, d_a u, d_b u, d_a d_b u) that also serves the first derivatives along
// a or b; what is left of the pure requests along one axis shares a line jet of the highest order left on that axis; the value rides in the
// first pass, or — with no derivative asked for — goes to the value kernel (value_dst).  Nonzero + `why` when the table is refused.
static int ens_plan_passes(int d, int nder, const int* orders, const int* axes, std::vector<ens::JetPass>& passes, int& value_dst, std::string& why) {
    passes.clear();
    value_dst = -1;
    std::vector<std::array<int, 3>> req((size_t)nder);   // (order, a, b) with a <= b: the canonical form of a request (pure: a == b; the value: -1, -1)
    for (int j = 0; j < nder; ++j) {
        const int o = orders[j];
        if (o < 0 || o > 4) { why = "request " + std::to_string(j) + ": order " + std::to_string(o) + " outside 0..4"; return 1; }
        int a = -1, b = -1;
        for (int k = 0; k < o; ++k) {
            const int x = axes[4 * j + k];
            if (x < 0 || x >= d) { why = "request " + std::to_string(j) + ": axis " + std::to_string(x) + " outside the network's " + std::to_string(d) + " inputs"; return 1; }
            a = k == 0 ? x : std::min(a, x);
            b = k == 0 ? x : std::max(b, x);
        }
        if (a != b && o >= 3) { why = "request " + std::to_string(j) + ": a mixed derivative of order " + std::to_string(o) + " (orders 3 and 4 run along one axis)"; return 1; }
        req[j] = {o, a, b};
        for (int i = 0; i < j; ++i)
            if (req[i] == req[j]) { why = "request " + std::to_string(j) + " repeats request " + std::to_string(i); return 1; }
    }
    auto fresh = [](int kind, int a, int b) { ens::JetPass p; p.kind = kind; p.axis[0] = a; p.axis[1] = b; for (int& x : p.dst) x = -1; return p; };
    std::vector<char> served((size_t)nder, 0);
    for (int j = 0; j < nder; ++j)
        if (req[j][0] == 2 && req[j][1] != req[j][2]) {
            passes.push_back(fresh(ens::JET_PAIR, req[j][1], req[j][2]));
            passes.back().dst[3] = j;
            served[j] = 1;
        }
    for (int j = 0; j < nder; ++j)
        for (size_t q = 0; q < passes.size() && req[j][0] == 1 && !served[j]; ++q)
            for (int k = 0; k < 2; ++k)
                if (passes[q].axis[k] == req[j][1]) { passes[q].dst[1 + k] = j; served[j] = 1; break; }
    for (int a = 0; a < d; ++a) {
        int K = 0;
        for (int j = 0; j < nder; ++j)
            if (!served[j] && req[j][0] >= 1 && req[j][1] == a) K = std::max(K, req[j][0]);
        if (K == 0) continue;
        passes.push_back(fresh(K, a, a));
        for (int j = 0; j < nder; ++j)
            if (!served[j] && req[j][0] >= 1 && req[j][1] == a) { passes.back().dst[req[j][0]] = j; served[j] = 1; }
    }
    for (int j = 0; j < nder; ++j)
        if (req[j][0] == 0) { if (passes.empty()) value_dst = j; else passes[0].dst[0] = j; }
    return 0;
}

namespace {

// points per pass: all of them unless the predictions [requests][S][n] exceed the budget ($PINN_ENS_GB, default 4) — then the largest multiple of
// the point block within it.  $PINN_ENS_CHUNK (points, rounded up to whole blocks) overrides the budget: the tests force several passes with it.
// Both are read per call.  Points are independent and the statistics never split over samples, so the passes change no bit.
int64_t ens_chunk_points(int64_t n, int64_t S, int ppb, int nder = 1) {
    int64_t c = (int64_t)(ens_budget_bytes() / (8.0 * (double)S * (double)nder));
    if (const char* e = std::getenv("PINN_ENS_CHUNK")) { const long long v = std::atoll(e); if (v > 0) c = (int64_t)v; }
    c = std::min(c, (int64_t)(1 << 30) / S * ppb);       // (the launch's workgroup count S x blocks stays below 2^30
    c = std::min(c, (int64_t)(1 << 30));                 //  and the points of one pass, an int in the kernels, too; 2^30 is a multiple of ppb)
    c = std::max<int64_t>((c + ppb - 1) / ppb, 1) * ppb;
    return std::min(c, n);
}

template <class T> int ens_run(const char* who, pinn_engine& E, EnsState& X, const ens::Net& net, int ppb, const double* thetas, int64_t S, const double* pts, int64_t n,
                               int ddof, double* mean, double* sd, double* preds) {
    const size_t P = (size_t)E.ntheta, d = (size_t)net.sizes[0], ns = (size_t)n;
    const int64_t chunk = ens_chunk_points(n, S, ppb);
    if (!dev_grow(X.d_th, X.th_cap, sizeof(T) * (size_t)S * P, E.stream) || !dev_grow(X.d_pts, X.pts_cap, sizeof(T) * ns * d, E.stream) ||
        !dev_grow(X.d_preds, X.preds_cap, (size_t)S * (size_t)chunk, E.stream) || !dev_grow(X.d_stat, X.stat_cap, 2 * ns, E.stream))
        return fail(std::string(who) + ": device allocation failed");
    double* d_preds = X.d_preds;
    double* d_stat = X.d_stat;
    auto th = as<T>(thetas, (size_t)S * P); auto x = as<T>(pts, ns * d);          // (float)theta, (float)x on an fp32 handle
    if (plat_h2d(X.d_th, th.get(), sizeof(T) * (size_t)S * P, E.stream) || plat_h2d(X.d_pts, x.get(), sizeof(T) * ns * d, E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    for (int64_t p0 = 0; p0 < n; p0 += chunk) {
        const int nc = (int)std::min(chunk, n - p0);
        if (ens::launch_forward<T>(net, (const T*)X.d_th, (int)S, P, (const T*)X.d_pts + (size_t)p0 * d, nc, d_preds, (size_t)nc, ppb, E.stream) ||
            ens::launch_stats(d_preds, (size_t)nc, (int)S, ddof, nc, d_stat + p0, d_stat + ns + p0, E.stream))
            return fail(std::string(who) + ": kernel launch failed (" + plat_last_error() + ")");
        for (int64_t s = 0; preds && s < (nc == n ? 1 : S); ++s)                  // (one pass: [S][n] is one contiguous block)
            if (plat_d2h(preds + (size_t)s * ns + p0, d_preds + (size_t)s * nc, sizeof(double) * (size_t)(nc == n ? S * n : nc), E.stream))
                return fail(std::string(who) + ": D2H copy failed");
    }
    std::vector<double> st(2 * ns);
    if (plat_d2h(st.data(), d_stat, sizeof(double) * 2 * ns, E.stream)) return fail(std::string(who) + ": D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    std::copy(st.begin(), st.begin() + ns, mean);
    std::copy(st.begin() + ns, st.end(), sd);
    return 0;
}

// pinn_derivative_ensemble: the jet passes of a request table (ens_plan_passes) with, per pass, its points per block and the bytes of scratch
// storage it takes (0: LDS)
constexpr int ENS_MAX_REQUESTS = 32;
constexpr int ENS_LDS_MIN_WGS = 4;                       // a jet pass keeps its images in LDS while that many workgroups fit a CU (40 KB each)
// workgroups of the scratch storage's bounded grid per CU (measured on the 4 x 64 network, DESIGN.md section 4.10: double levels off at 8, float still gains at 16)
constexpr int ens_scratch_wgs_per_cu(size_t elem) { return elem == sizeof(double) ? 8 : 16; }
struct EnsPlan {
    std::vector<ens::JetPass> passes;
    std::vector<int> ppb;
    std::vector<size_t> scr;
    int value_dst = -1, value_ppb = 0;                   // the value request when no jet pass carries it: the value kernel
    int ppb_min = 0, grid = 0;
    size_t scr_bytes = 0;
};

template <class T> int ens_run_der(const char* who, pinn_engine& E, EnsState& X, const ens::Net& net, const EnsPlan& plan, const double* thetas, int64_t S, const double* pts,
                                   int64_t n, int nder, int ddof, double* mean, double* sd, double* preds) {
    const size_t P = (size_t)E.ntheta, d = (size_t)net.sizes[0], ns = (size_t)n, R = (size_t)nder;
    const int64_t chunk = ens_chunk_points(n, S, plan.ppb_min, nder);
    if (!dev_grow(X.d_th, X.th_cap, sizeof(T) * (size_t)S * P, E.stream) || !dev_grow(X.d_pts, X.pts_cap, sizeof(T) * ns * d, E.stream) ||
        !dev_grow(X.d_preds, X.preds_cap, R * (size_t)S * (size_t)chunk, E.stream) || !dev_grow(X.d_stat, X.stat_cap, 2 * R * ns, E.stream) ||
        !dev_grow(X.d_scr, X.scr_cap, plan.scr_bytes, E.stream))
        return fail(std::string(who) + ": device allocation failed");
    double* d_preds = X.d_preds;
    double* d_stat = X.d_stat;
    auto th = as<T>(thetas, (size_t)S * P); auto x = as<T>(pts, ns * d);          // (float)theta, (float)x on an fp32 handle
    if (plat_h2d(X.d_th, th.get(), sizeof(T) * (size_t)S * P, E.stream) || plat_h2d(X.d_pts, x.get(), sizeof(T) * ns * d, E.stream))
        return fail(std::string(who) + ": H2D copy failed");
    int point_passes = 0, scratch_passes = 0;
    for (int64_t p0 = 0; p0 < n; p0 += chunk, ++point_passes) {
        const int nc = (int)std::min(chunk, n - p0);
        const size_t slab = (size_t)S * (size_t)nc;                               // request j: d_preds[j * slab ..], [S][nc]
        const T* xp = (const T*)X.d_pts + (size_t)p0 * d;
        int bad = 0;
        for (size_t q = 0; q < plan.passes.size() && !bad; ++q)
            bad = ens::launch_jet<T>(net, plan.passes[q], (const T*)X.d_th, (int)S, P, xp, nc, d_preds, (size_t)nc, plan.ppb[q], plan.scr[q] ? (T*)X.d_scr : nullptr, plan.grid, E.stream);
        if (!bad && plan.value_dst >= 0)
            bad = ens::launch_forward<T>(net, (const T*)X.d_th, (int)S, P, xp, nc, d_preds + (size_t)plan.value_dst * slab, (size_t)nc, plan.value_ppb, E.stream);
        for (size_t j = 0; j < R && !bad; ++j)
            bad = ens::launch_stats(d_preds + j * slab, (size_t)nc, (int)S, ddof, nc, d_stat + j * ns + p0, d_stat + (R + j) * ns + p0, E.stream);
        if (bad) return fail(std::string(who) + ": kernel launch failed (" + plat_last_error() + ")");
        if (preds && nc == n) {                                                   // (one pass: [requests][S][n] is one contiguous block)
            if (plat_d2h(preds, d_preds, sizeof(double) * R * slab, E.stream)) return fail(std::string(who) + ": D2H copy failed");
        } else if (preds) {
            for (size_t js = 0; js < R * (size_t)S; ++js)
                if (plat_d2h(preds + js * ns + p0, d_preds + js * nc, sizeof(double) * (size_t)nc, E.stream)) return fail(std::string(who) + ": D2H copy failed");
        }
    }
    for (size_t q = 0; q < plan.passes.size(); ++q) scratch_passes += plan.scr[q] != 0;
    std::vector<double> st(2 * R * ns);
    if (plat_d2h(st.data(), d_stat, sizeof(double) * 2 * R * ns, E.stream)) return fail(std::string(who) + ": D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    std::copy(st.begin(), st.begin() + R * ns, mean);
    std::copy(st.begin() + R * ns, st.end(), sd);
    X.jet_passes = (int)plan.passes.size(); X.point_passes = point_passes; X.scratch_passes = scratch_passes;
    return 0;
}

}  // namespace

void pe::ens_free(pinn_engine& E) {
    if (EnsState* X = E.ens) {
        plat_free(X->d_th); plat_free(X->d_pts); plat_free(X->d_preds); plat_free(X->d_stat); plat_free(X->d_scr);
        delete X;
    }
    E.ens = nullptr;
}

// what both entry points refuse, and the network as the kernels take it
static int ens_check(const char* who, pinn_handle h, int net, const double* thetas, int64_t nsamples, int64_t p, const double* pts, int64_t n, int ddof, const double* mean,
                     const double* std_, ens::Net& en) {
    if (!h || !thetas || !pts || !mean || !std_) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (net < 0 || net >= (int)E.nets.size()) return fail(std::string(who) + ": net index " + std::to_string(net) + " out of range (the handle has " + std::to_string(E.nets.size()) + " networks)");
    if (check_theta(E, who, p)) return 1;
    if (nsamples < 1) return fail(std::string(who) + ": nsamples must be at least 1");
    if (nsamples > (int64_t)(1 << 30)) return fail(std::string(who) + ": nsamples must be at most 2^30");
    if (ddof != 0 && ddof != 1) return fail(std::string(who) + ": ddof must be 0 or 1");
    if (nsamples - ddof < 1) return fail(std::string(who) + ": nsamples - ddof must be at least 1 (" + std::to_string(nsamples) + " samples, ddof " + std::to_string(ddof) + ")");
    if (n < 1) return fail(std::string(who) + ": n must be at least 1");
    const Net& N = E.nets[net];
    if (N.kind == 1) return fail(std::string(who) + ": not available for a DGM network (Dense chains only)");
    if (!N.emb_idx.empty()) return fail(std::string(who) + ": not available for a network behind a periodic input embedding");
    const int nl = (int)N.sizes.size() - 1;
    if (nl > ens::MAX_LAYERS) return fail(std::string(who) + ": more than " + std::to_string(ens::MAX_LAYERS) + " Dense layers");
    std::memset(&en, 0, sizeof en);
    en.nl = nl; en.act = N.act; en.act_layers = N.act_layers; en.theta0 = N.theta_off;
    for (int l = 0; l <= nl; ++l) { en.sizes[l] = N.sizes[l]; en.wmax = std::max(en.wmax, N.sizes[l]); }
    return 0;
}
static std::string ens_lds_refusal(const char* who, const ens::Net& en, size_t elem) {
    return std::string(who) + ": the widest layer (" + std::to_string(en.wmax) + " neurons) needs " + std::to_string(ens::lds_bytes(en, ens::MIN_PPB, elem)) +
           " bytes of LDS for two images of " + std::to_string(ens::MIN_PPB) + " points; the limit is " + std::to_string(ens::LDS_MAX);
}

int pe::ens_counter(const pinn_engine& E, int which) {
    if (!E.ens) return 0;
    return which == 0 ? E.ens->jet_passes : (which == 1 ? E.ens->point_passes : E.ens->scratch_passes);
}

extern "C" {

int pinn_phi_ensemble(pinn_handle h, int net, const double* thetas, int64_t nsamples, int64_t p, const double* pts, int64_t n, int ddof,
                      double* mean, double* std_, double* preds) {
    const char* who = "pinn_phi_ensemble";
    ens::Net en;
    if (ens_check(who, h, net, thetas, nsamples, p, pts, n, ddof, mean, std_, en)) return 1;
    pinn_engine& E = *h;
    const size_t elem = E.f64 ? sizeof(double) : sizeof(float);
    const int ppb = ens::pick_ppb(en, elem);
    if (ppb == 0) return fail(ens_lds_refusal(who, en, elem));
    DeviceScope scope(E.device);
    if (!E.ens) E.ens = new EnsState;
    EnsState& X = *E.ens;
    return E.f64 ? ens_run<double>(who, E, X, en, ppb, thetas, nsamples, pts, n, ddof, mean, std_, preds)
                 : ens_run<float>(who, E, X, en, ppb, thetas, nsamples, pts, n, ddof, mean, std_, preds);
}

int pinn_derivative_ensemble(pinn_handle h, int net, const double* thetas, int64_t nsamples, int64_t p, const double* pts, int64_t n, int nder, const int* orders,
                             const int* axes, int ddof, double* mean, double* std_, double* preds) {
    const char* who = "pinn_derivative_ensemble";
    ens::Net en;
    if (ens_check(who, h, net, thetas, nsamples, p, pts, n, ddof, mean, std_, en)) return 1;
    pinn_engine& E = *h;
    if (nder < 1 || nder > ENS_MAX_REQUESTS) return fail(std::string(who) + ": nder must be in 1.." + std::to_string(ENS_MAX_REQUESTS) + ", not " + std::to_string(nder));
    if (!orders || !axes) return fail(std::string(who) + ": null argument");
    EnsPlan plan;
    std::string why;
    if (ens_plan_passes(en.sizes[0], nder, orders, axes, plan.passes, plan.value_dst, why)) return fail(std::string(who) + ": " + why);
    const size_t elem = E.f64 ? sizeof(double) : sizeof(float);
    DeviceScope scope(E.device);
    // the storage of every pass.  LDS by pick_ppb's rule with the C factor while the images leave room for ENS_LDS_MIN_WGS workgroups per CU (one
    // workgroup of 64 points is ONE wave: a 96 KB image pair means one wave per CU, measured 2.3x - 5x slower than the scratch storage on the
    // 4 x 64 network); the scratch storage beyond that, and always when two images of 64 points exceed the CU's LDS.
    // $PINN_ENS_NO_LDS = 1 forces the scratch storage, = 0 the LDS wherever two images of 64 points fit (tests, A/B); same bits.
    const char* no_lds = std::getenv("PINN_ENS_NO_LDS");
    const int storage = no_lds && *no_lds ? (std::atoi(no_lds) == 1 ? 1 : 0) : -1;      // 1: scratch, 0: LDS, -1: the rule above
    int wgs = ens_scratch_wgs_per_cu(elem);
    if (const char* e = std::getenv("PINN_ENS_SCRATCH_WGS")) { const int v = std::atoi(e); if (v >= 1 && v <= 64) wgs = v; }
    const int64_t cap = (int64_t)wgs * plat_num_cus(), blocks = (n + ens::MIN_PPB - 1) / ens::MIN_PPB;
    plan.grid = (int)(blocks >= cap ? cap : std::min(cap, nsamples * blocks));           // (never more workgroups than (sample, block) pairs)
    plan.ppb_min = ens::MAX_PPB;
    if (plan.value_dst >= 0) {
        plan.value_ppb = ens::pick_ppb(en, elem);
        if (plan.value_ppb == 0) return fail(ens_lds_refusal(who, en, elem));
        plan.ppb_min = plan.value_ppb;
    }
    for (const ens::JetPass& ps : plan.passes) {
        const int C = ens::jet_channels(ps.kind);
        int ppb = storage == 1 ? 0 : ens::pick_ppb(en, elem, C);
        if (storage == -1 && ppb && ens::lds_bytes(en, ppb, elem, C) > ens::LDS_MAX / (size_t)ENS_LDS_MIN_WGS) ppb = 0;
        size_t scr = 0;
        if (ppb == 0) {
            ppb = ens::MIN_PPB;
            scr = (size_t)plan.grid * ens::jet_region(en, C, ppb) * elem;
            if ((double)scr > ens_budget_bytes())
                return fail(std::string(who) + ": the widest layer (" + std::to_string(en.wmax) + " neurons) with " + std::to_string(C) + " jet channels needs " +
                            std::to_string(ens::jet_region(en, C, ppb) * elem) + " bytes of image scratch per workgroup, " + std::to_string(scr) + " bytes for " +
                            std::to_string(plan.grid) + " workgroups; the memory budget ($PINN_ENS_GB) is " + std::to_string((long long)ens_budget_bytes()) + " bytes");
        }
        plan.ppb.push_back(ppb);
        plan.scr.push_back(scr);
        plan.scr_bytes = std::max(plan.scr_bytes, scr);
        plan.ppb_min = std::min(plan.ppb_min, ppb);
    }
    if (!E.ens) E.ens = new EnsState;
    EnsState& X = *E.ens;
    return E.f64 ? ens_run_der<double>(who, E, X, en, plan, thetas, nsamples, pts, n, nder, ddof, mean, std_, preds)
                 : ens_run_der<float>(who, E, X, en, plan, thetas, nsamples, pts, n, nder, ddof, mean, std_, preds);
}

}  // extern "C"
