// resident.hpp — host plumbing the resident solvers share (hmc.cpp, lbfgs.cpp, bfgs.cpp; the grow-only buffers also adam.cpp, ensemble.cpp, the f64*.cpp units).
// Host-only: no kernel translation unit sees it.
#pragma once
#include "engine_types.hpp"

namespace pe {

// grow-only device buffer: true when p holds `need` (capacity `cap`) already, or after the stream has drained and a larger block has replaced
// it; a failed allocation leaves p null with capacity 0.  Capacities in bytes here, in elements of T below.
inline bool dev_grow(void*& p, size_t& cap, size_t need, plat_stream st) {
    if (cap >= need) return true;
    plat_sync(st);
    plat_free(p);
    p = plat_malloc(need);
    cap = p ? need : 0;
    return p != nullptr;
}
template <class T> bool dev_grow(T*& p, size_t& cap, size_t need, plat_stream st) {
    if (cap >= need) return true;
    void* v = p;
    size_t bytes = 0;
    dev_grow(v, bytes, sizeof(T) * need, st);
    p = (T*)v;
    cap = p ? need : 0;
    return p != nullptr;
}

// The evaluation lane of a resident solver: the handle's loss + gradient at parameters the solver's kernels wrote on the device, in the precision
// mode the solver was initialised in.  float64 mode: f64_eval_resident reads the mode's own parameter buffer (theta64) and writes [gradient | raw
// sums] to d_ev64.  fp32: run_loss_grad reads the narrowed copy d_th32 and writes [P + K] floats to d_ev32, the K sums again as doubles to d_raw.
struct ResidentEval {
    bool f64 = false;
    std::vector<double> w64;             // the term weights of every evaluation
    std::vector<float> w32;
    double* d_ev64 = nullptr;
    float* d_ev32 = nullptr;
    double* d_raw = nullptr;
    float* d_th32 = nullptr;

    int init(pinn_engine& E, const char* who, const double* w, int K) {
        const size_t P = (size_t)E.ntheta;
        f64 = E.f64 != nullptr;
        w64.assign(w, w + K);
        w32.resize(K);
        for (int k = 0; k < K; ++k) w32[k] = (float)w[k];
        if (f64) d_ev64 = (double*)plat_malloc(sizeof(double) * (P + K));
        else {
            d_ev32 = (float*)plat_malloc(sizeof(float) * (P + K));
            d_raw = (double*)plat_malloc(sizeof(double) * (size_t)K);
            d_th32 = (float*)plat_malloc(sizeof(float) * P);
        }
        if (f64 ? !d_ev64 : (!d_ev32 || !d_raw || !d_th32)) return fail(std::string(who) + ": device allocation failed");
        return 0;
    }
    void release() { plat_free(d_ev64); plat_free(d_ev32); plat_free(d_raw); plat_free(d_th32); }
    // the handle's precision mode is still the one of init_name's call (what every later call of the solver checks first)
    int ready(const pinn_engine& E, const char* who, const char* init_name) const {
        if (f64 != (E.f64 != nullptr))
            return fail(std::string(who) + ": the handle's precision changed since " + init_name + " (call " + init_name + " again)");
        return 0;
    }
    int eval(pinn_engine& E) {
        if (f64) return f64_eval_resident(E, w64.data(), d_ev64);
        EvalRequest rq = EvalRequest::device(d_th32, d_ev32, w32.data());
        rq.lossraw = d_raw;
        return run_loss_grad(E, rq);
    }
    template <class T> const T* out() const {            // [gradient | sums] of the last evaluation, T the mode's type
        if constexpr (std::is_same_v<T, double>) return d_ev64;
        else return d_ev32;
    }
    const double* sums(size_t P) const { return f64 ? d_ev64 + P : d_raw; }      // its K raw sums in double
    // where the solver's kernels write the parameters of the next evaluation (one of the two is null); the float64 buffer is asked for per call:
    // the mode may have been left and entered again since init
    double* theta64(pinn_engine& E) const { return f64 ? f64_theta_buffer(E) : nullptr; }
    float* theta32() const { return d_th32; }
};

// a resident solver runs on one device against fixed point sets; `one_device` and `fixed_what` are the solver's own words for the two refusals
inline int resident_refuse_target(const pinn_engine& E, const char* who, const char* one_device, const char* fixed_what) {
    if (E.comm) return fail(std::string(who) + ": the handle belongs to a communicator; " + one_device);
    for (auto& T : E.terms)
        if (T.sampler != 0) return fail(std::string(who) + ": a term redraws its points on the device; " + fixed_what + " (fixed point sets)");
    return 0;
}

// The noise-floor switch of the quasi-Newton routines (pinn_lbfgs, pinn_lbfgs_steps, pinn_bfgs_steps).  A line search that cannot decrease the objective along a descent
// direction has reached the evaluation's noise floor; the split-operand GEMMs' floor is 2-4 x that of the fp32 MFMA kernels:
// a handle in "split" mode is switched to them once per call and goes on from the same iterate.  The switch only changes arithmetic where a launch
// group runs a family-2 kernel that exists as a split / fp32 twin; $PINN_LBFGS_KEEP_GEMM disables it; every exit path hands the handle back in the
// mode it came in.
struct GemmFloorSwitch {
    pinn_engine& E;
    bool switched = false, armed = false, has_twin = false;
    explicit GemmFloorSwitch(pinn_engine& e) : E(e) {
        for (const NetPlan& NP : E.netplans) has_twin = has_twin || (NP.spec && NP.spec->family == 2 && NP.spec->twin);
    }
    ~GemmFloorSwitch() { if (armed && E.gemm != pk::GEMM_SPLIT) { const std::string keep = g_err; replan_gemm(E, pk::GEMM_SPLIT); if (!keep.empty()) g_err = keep; } }
    bool eligible() const { return !E.f64 && E.gemm == pk::GEMM_SPLIT && !switched && has_twin && std::getenv("PINN_LBFGS_KEEP_GEMM") == nullptr; }
    // 0: done, `switched` says whether the handle now runs the fp32 kernels; 1: error; 2: the switch failed (the fp32 twin of a run-time specialised
    // shape did not compile) and left the handle in split mode — replan_gemm restored the plan: the iterate reached so far is the answer, not an
    // error
    int engage() {
        if (replan_gemm(E, pk::GEMM_FP32)) { if (E.gemm != pk::GEMM_SPLIT || E.groups.empty()) return 1; g_err.clear(); return 2; }
        switched = E.gemm == pk::GEMM_FP32;
        armed = switched;
        return 0;
    }
    int finish() {                                       // the regular end of a call
        if (!switched) return 0;
        armed = false;
        return replan_gemm(E, pk::GEMM_SPLIT) ? 1 : 0;
    }
};

}  // namespace pe
