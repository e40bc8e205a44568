// qn_emu_check.cpp — stand-alone check of the resident quasi-Newton kernels' bodies (csrc/qn_kernels.hpp, lbfgs_kernels.hpp, bfgs_kernels.hpp) in
// their serial emulation under the host sanitizers.  Nothing of the engine is linked: the "evaluation" is written by this program as
// [gradient | one raw sum] of the convex quadratic f = 1/2 x'Ax - b'x (A = tridiagonal(-1, 2 + i / P, -1), b = 1), and the slot loop of
// lbfgs.cpp / bfgs.cpp is restated around lbfgs::launch_step and bfgs::launch_ctl / _matvec / _update.  Cases: P = 5; P = 131 (odd, ld = 256:
// pad columns in use); L-BFGS with history 3 and more than 3 accepted iterations (the ring wraps); both element types.  Exit status 0 iff every
// run ends ST_CONVERGED with max |g| <= gtol.  A CPU program: from the repository root
//   g++ -std=c++17 -DPINN_EMU -g -fsanitize=address,undefined -Ineuralpde.jl_amd/csrc tools/micro/qn_emu_check.cpp -o /tmp/qn_emu_check && /tmp/qn_emu_check
#include "lbfgs_kernels.hpp"
#include "bfgs_kernels.hpp"
#include <cstdio>
#include <vector>

// the evaluation at the point the kernels wrote for it: ev = [A x - b | f], the one sum again in double
template <class T> static void evaluate(int P, const std::vector<T>& th, std::vector<T>& ev, double& sum) {
    double f = 0.0;
    for (int i = 0; i < P; ++i) {
        const double x = (double)th[i], lo = i > 0 ? (double)th[i - 1] : 0.0, hi = i + 1 < P ? (double)th[i + 1] : 0.0;
        const double Ax = (2.0 + (double)i / P) * x - lo - hi;
        ev[i] = (T)(Ax - 1.0);
        f += 0.5 * x * Ax - x;
    }
    ev[P] = (T)f;
    sum = f;
}

template <class T> static void point_at(qn::Args& a, std::vector<T>& th) {
    if constexpr (sizeof(T) == 8) a.th_eval64 = th.data();
    else a.th_eval32 = th.data();
}

// the common arguments over the vectors in `vec` (x | g | xn | d, `stride` apart), one term of weight 1 and n_norm 1
static void wire(qn::Args& a, int P, std::vector<double>& vec, size_t stride, double* tab, const double* sum, std::vector<double>& hist) {
    a.P = P; a.K = 1; a.f64form = 1;
    a.x = vec.data(); a.g = a.x + stride; a.xn = a.g + stride; a.d = a.xn + stride;
    tab[0] = 1.0; tab[1] = 1.0;
    a.w = tab; a.nrm = tab + 1;
    a.sums = sum;
    a.loss_hist = hist.data();
}

static int report(const char* what, int P, const qn::Ctl& k, const double* g, double gtol, int accepted_min) {
    double gmax = 0.0;
    for (int i = 0; i < P; ++i) gmax = std::fmax(gmax, std::fabs(g[i]));
    const bool ok = k.status == qn::ST_CONVERGED && gmax <= gtol && k.it >= accepted_min;
    std::printf("%-18s P=%3d  status %d  iterations %3d  evaluations %3d  f %.12e  max|g| %.3e  %s\n", what, P, k.status, k.it, k.evals, k.f, gmax, ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}

constexpr int MAX_ITERS = 400, MAX_SLOTS = 4000;

template <class T> static int run_lbfgs(int P, double gtol) {
    const int m = 3;
    std::vector<double> vec((size_t)(4 * P + 2 * m * P + m), 0.0), hist(MAX_ITERS);
    std::vector<T> th(P), ev(P + 1);
    double tab[2], sum = 0.0;
    lbfgs::Ctl ctl{};
    lbfgs::Args a{};
    wire(a, P, vec, (size_t)P, tab, &sum, hist);
    point_at(a, th);
    a.m = m; a.S = a.d + P; a.Y = a.S + (size_t)m * P; a.rho = a.Y + (size_t)m * P;
    a.ctl = &ctl;
    for (int i = 0; i < P; ++i) a.x[i] = 0.25 * ((i % 7) - 3);
    lbfgs::launch_step<T>(a, ev.data(), lbfgs::MODE_LOAD, 0, 0, 0.0, nullptr);
    evaluate(P, th, ev, sum);
    lbfgs::launch_step<T>(a, ev.data(), lbfgs::MODE_ADOPT, 0, 0, 0.0, nullptr);
    for (int s = 0; s < MAX_SLOTS && ctl.status < qn::ST_CONVERGED; ++s) {
        lbfgs::launch_step<T>(a, ev.data(), lbfgs::MODE_SLOT, 0, MAX_ITERS, gtol, nullptr);
        evaluate(P, th, ev, sum);
    }
    return report(sizeof(T) == 8 ? "lbfgs m=3 double" : "lbfgs m=3 float", P, ctl, a.g, gtol, m + 1);
}

template <class T> static int run_bfgs(int P, double gtol) {
    const size_t ld = (size_t)bfgs::padded_ld(P);
    std::vector<double> vec(7 * ld, 0.0), H((size_t)P * ld), hist(MAX_ITERS);
    std::vector<T> th(P), ev(P + 1);
    double tab[2], sum = 0.0;
    bfgs::Ctl ctl{};
    bfgs::Args a{};
    wire(a, P, vec, ld, tab, &sum, hist);
    point_at(a, th);
    a.ld = (int)ld; a.s = a.d + ld; a.y = a.s + ld; a.u = a.y + ld; a.H = H.data();
    a.ctl = &ctl;
    for (int i = 0; i < P; ++i) a.x[i] = 0.25 * ((i % 7) - 3);
    bfgs::launch_ctl<T>(a, ev.data(), bfgs::PH_LOAD, 0, 0, 0.0, nullptr);
    evaluate(P, th, ev, sum);
    bfgs::launch_ctl<T>(a, ev.data(), bfgs::PH_ADOPT, 0, 0, 0.0, nullptr);
    for (int s = 0; s < MAX_SLOTS && ctl.status < qn::ST_CONVERGED; ++s) {
        bfgs::launch_ctl<T>(a, ev.data(), bfgs::PH_JUDGE, 0, MAX_ITERS, gtol, nullptr);
        bfgs::launch_matvec(a, nullptr);
        bfgs::launch_ctl<T>(a, ev.data(), bfgs::PH_MID, 0, MAX_ITERS, gtol, nullptr);
        bfgs::launch_update(a, nullptr);
        bfgs::launch_ctl<T>(a, ev.data(), bfgs::PH_PROPOSE, 0, MAX_ITERS, gtol, nullptr);
        evaluate(P, th, ev, sum);
    }
    for (size_t i = (size_t)P; i < ld; ++i)              // the vectors' pads are never written
        for (int v = 0; v < 7; ++v)
            if (vec[(size_t)v * ld + i] != 0.0) { std::printf("bfgs: pad entry %zu of vector %d was written\n", i, v); return 1; }
    return report(sizeof(T) == 8 ? "bfgs double" : "bfgs float", P, ctl, a.g, gtol, 2);
}

int main() {
    int bad = 0;
    for (int P : {5, 131}) {
        // gtol from the objective's resolution, not from what the runs reach: Armijo needs a decrease of about |g|^2 / (2 |A|), |A| <= 5, that
        // the objective can show.  double: ulp(f) = 3e-14 at |f| = 234 (P = 131) -> |g| >~ 5e-7.  float: the evaluation sees float(x), |x| <~ 8,
        // so f moves by about |g| sqrt(P) 2^-24 |x| on its own -> |g| >~ 5e-5.  Two and twenty times those.
        bad += run_lbfgs<double>(P, 1e-6) + run_lbfgs<float>(P, 1e-3);
        bad += run_bfgs<double>(P, 1e-6) + run_bfgs<float>(P, 1e-3);
    }
    if (bad) { std::printf("qn_emu_check: %d run(s) FAILED\n", bad); return 1; }
    std::puts("qn_emu_check: ok");
    return 0;
}
