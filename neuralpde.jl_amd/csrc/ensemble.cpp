// ensemble.cpp — ensemble prediction (pinn_phi_ensemble): phi of one network at S parameter vectors and n points + the mean / standard
// deviation over the S predictions (ens_kernels.hpp).  One upload of the parameter vectors, one of the points, the launches back to back on
// the handle's stream, one download.  The buffers belong to this entry point and grow on demand; nothing else of the handle is touched.
#include "resident.hpp"
#include "ens_kernels.hpp"

using namespace pe;

struct pe::EnsState {
    void* d_th = nullptr; void* d_pts = nullptr;         // [S][P] | [n][d] in the compute type
    double* d_preds = nullptr; double* d_stat = nullptr; // [S][points of one pass] | [mean n | std n]
    size_t th_cap = 0, pts_cap = 0;                      // bytes
    size_t preds_cap = 0, stat_cap = 0;                  // doubles
};

namespace {

// points per pass: all of them unless the predictions [S][n] exceed the budget ($PINN_ENS_GB, default 4) — then the largest multiple of the
// point block within it.  $PINN_ENS_CHUNK (points, rounded up to whole blocks) overrides the budget: the tests force several passes with it.
// Both are read per call.  Points are independent and the statistics never split over samples, so the passes change no bit.
int64_t ens_chunk_points(int64_t n, int64_t S, int ppb) {
    double gb = 4.0;
    if (const char* e = std::getenv("PINN_ENS_GB")) { const double v = std::atof(e); if (v > 0.0) gb = v; }
    int64_t c = (int64_t)(gb * 1073741824.0 / (8.0 * (double)S));
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

}  // namespace

void pe::ens_free(pinn_engine& E) {
    if (EnsState* X = E.ens) {
        plat_free(X->d_th); plat_free(X->d_pts); plat_free(X->d_preds); plat_free(X->d_stat);
        delete X;
    }
    E.ens = nullptr;
}

extern "C" {

int pinn_phi_ensemble(pinn_handle h, int net, const double* thetas, int64_t nsamples, int64_t p, const double* pts, int64_t n, int ddof,
                      double* mean, double* std_, double* preds) {
    const char* who = "pinn_phi_ensemble";
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
    ens::Net en;
    std::memset(&en, 0, sizeof en);
    en.nl = nl; en.act = N.act; en.act_layers = N.act_layers; en.theta0 = N.theta_off;
    for (int l = 0; l <= nl; ++l) { en.sizes[l] = N.sizes[l]; en.wmax = std::max(en.wmax, N.sizes[l]); }
    const size_t elem = E.f64 ? sizeof(double) : sizeof(float);
    const int ppb = ens::pick_ppb(en, elem);
    if (ppb == 0)
        return fail(std::string(who) + ": the widest layer (" + std::to_string(en.wmax) + " neurons) needs " + std::to_string(ens::lds_bytes(en, ens::MIN_PPB, elem)) +
                    " bytes of LDS for two images of " + std::to_string(ens::MIN_PPB) + " points; the limit is " + std::to_string(ens::LDS_MAX));
    DeviceScope scope(E.device);
    if (!E.ens) E.ens = new EnsState;
    EnsState& X = *E.ens;
    return E.f64 ? ens_run<double>(who, E, X, en, ppb, thetas, nsamples, pts, n, ddof, mean, std_, preds)
                 : ens_run<float>(who, E, X, en, ppb, thetas, nsamples, pts, n, ddof, mean, std_, preds);
}

}  // extern "C"
