// adam.cpp — the resident fp32 Adam of the C ABI (pinn_adam_init / _steps / _steps_sharded / _apply / _get; the float64 loop: f64_adam.cpp) and
// the host side of the persistent training kernel (pinn_train.hpp): the stand-alone loop, K iterations of a small problem inside one launch,
// and that kernel's eval_only form behind pe::eval_and_sync.
#include "resident.hpp"
#include "adam_host.hpp"
#include "adam_kernels.hpp"

using namespace pe;

namespace {

// fp32 optimiser state (float64 mode: f64_adam.cpp keeps its own, in double)
int adam_init_f32(pinn_engine& E, const float* theta) {
    const int64_t p = E.ntheta;
    const int K = (int)E.terms.size();
    if (!E.d_opt_theta) {
        E.d_opt_theta = (float*)plat_malloc(sizeof(float) * p);
        E.d_opt_m = (float*)plat_malloc(sizeof(float) * p);
        E.d_opt_v = (float*)plat_malloc(sizeof(float) * p);
        E.d_opt_out = (float*)plat_malloc(sizeof(float) * (p + K));
        E.d_w_over_n = (float*)plat_malloc(sizeof(float) * K);
        if (!E.d_opt_theta || !E.d_opt_m || !E.d_opt_v || !E.d_opt_out || !E.d_w_over_n) return fail("device allocation failed (optimiser state)");
    }
    plat_h2d(E.d_opt_theta, theta, sizeof(float) * p, E.stream);
    plat_memset(E.d_opt_m, 0, sizeof(float) * p, E.stream);
    plat_memset(E.d_opt_v, 0, sizeof(float) * p, E.stream);
    plat_sync(E.stream);
    E.opt_t = 0;
    return 0;
}

int adam_get_f32(pinn_engine& E, float* theta) {
    if (!E.d_opt_theta) return fail("pinn_adam_get: no optimiser state (call pinn_adam_init first)");
    if (plat_d2h(theta, E.d_opt_theta, sizeof(float) * E.ntheta, E.stream)) return fail("D2H copy failed");
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return 0;
}

// the bias-correction table of steps opt_t + 1 .. opt_t + nsteps, [c1 | c2] per step: filled into c12 and queued for upload to
// E.d_c12 (grown on demand; false: the allocation failed).  c12 is pageable: the caller keeps it until its next synchronisation
bool upload_c12(pinn_engine& E, int nsteps, float beta1, float beta2, std::vector<float>& c12) {
    if (!dev_grow(E.d_c12, E.c12_cap, 2 * (size_t)nsteps, E.stream)) return false;
    c12.resize(2 * (size_t)nsteps);
    for (int s = 0; s < nsteps; ++s) {
        c12[2 * s] = adam_bias(beta1, E.opt_t + s + 1);
        c12[2 * s + 1] = adam_bias(beta2, E.opt_t + s + 1);
    }
    plat_h2d(E.d_c12, c12.data(), sizeof(float) * c12.size(), E.stream);
    return true;
}

// Device-side table of a handle's redrawn terms (aux::ResampleTerm), draw counters as they stand now.  Returns the number of terms in the
// table (0: no sampler), -1 when a redrawn term carries what the one-launch redraw does not cover (embeddings, per-point data / weights,
// coupled equations: the per-term kernels stay), -2 on a device error (g_err set).  max_n = the largest set.
int upload_resample_table(pinn_engine& E, int* max_n) {
    std::vector<pk::TrainSampler> samp;
    *max_n = 0;
    for (auto& T : E.terms) {
        if (T.sampler == 0) continue;
        if (!T.emb_cols.empty() || T.ndata > 0 || T.pw_n > 0 || T.coupled >= 0 || T.src_root.size() > (size_t)aux::SRC_MAX) return -1;
        pk::TrainSampler S;
        std::memset(&S, 0, sizeof S);
        S.pts = T.d_pts; S.n = (int)T.n; S.d = T.d; S.kind = T.sampler; S.lb = T.d_lb; S.ub = T.d_ub;
        S.seed = sampler_seed(E, T); S.draw0 = T.draws;
        S.has_src = T.src_root.empty() ? 0 : 1;
        if (S.has_src) {
            S.src.pts = T.d_pts; S.src.N = (int)T.n; S.src.d = T.d; S.src.prog = T.d_src_prog; S.src.nops = (int)T.src_prog.size();
            S.src.nsrc = (int)T.src_root.size();
            for (int j = 0; j < S.src.nsrc; ++j) S.src.root[j] = T.src_root[(size_t)j];
            S.src.out = T.d_src; S.src.data = nullptr;
        }
        *max_n = std::max(*max_n, S.n);
        samp.push_back(S);
    }
    if (samp.empty()) return 0;
    if (plat_sync(E.stream)) { fail(std::string("device error: ") + plat_last_error()); return -2; }      // (an earlier launch may still read the table)
    if (!dev_grow(E.d_train_samp, E.train_samp_cap, sizeof(pk::TrainSampler) * samp.size(), E.stream)) { fail("device allocation failed (table of redrawn terms)"); return -2; }
    plat_h2d(E.d_train_samp, samp.data(), sizeof(pk::TrainSampler) * samp.size(), E.stream);
    if (plat_sync(E.stream)) { fail(std::string("device error: ") + plat_last_error()); return -2; }      // (samp is a pageable temporary)
    return (int)samp.size();
}

// the resident loop over ndev handles: one handle (plain, or a rank of a one-process-per-GPU communicator), or the handles of one
// pinn_comm_init_all communicator (single process, several devices).  Per iteration and device: redraw the sampled sets -> evaluate the
// local shards; then ONE all-reduce of [gradient | sums] (+ the K double sums) over the communicator, each rank's call on its own stream;
// then the fused update (Adam + total loss + weight-image scatter) on every device.  No host synchronisation inside the loop: the step
// index, the bias corrections and the draw counters are kernel arguments.
int adam_loop(pinn_engine** es, int ndev, int nsteps, float lr, float beta1, float beta2, float eps, const float* term_w) {
    const int K = (int)es[0]->terms.size(), P = (int)es[0]->ntheta;
    const bool collective = ndev > 1 || (es[0]->comm != nullptr && es[0]->comm_per_process);
    std::vector<float*> vec(ndev);
    std::vector<double*> raw(ndev);
    for (int i = 0; i < ndev; ++i) { vec[i] = es[i]->d_opt_out; raw[i] = es[i]->d_lossraw; }
    // redrawn point sets: ONE launch per step redraws every such term and its source channels (aux::k_resample over a device-side table);
    // terms with embeddings / per-point data keep their own sampler / embed / source launches (PINN_NO_FUSED_RESAMPLE=1: always)
    std::vector<int> nsamp(ndev, -1), max_n(ndev, 0);
    for (int i = 0; i < ndev && std::getenv("PINN_NO_FUSED_RESAMPLE") == nullptr; ++i) {
        DeviceScope scope(es[i]->device);
        nsamp[i] = upload_resample_table(*es[i], &max_n[i]);
        if (nsamp[i] == -2) return 1;
    }
    for (int s = 0; s < nsteps; ++s) {
        for (int i = 0; i < ndev; ++i) {
            pinn_engine& E = *es[i];
            DeviceScope scope(E.device);
            if (nsamp[i] > 0) {
                aux::launch_resample((const pk::TrainSampler*)E.d_train_samp, nsamp[i], max_n[i], s, E.stream);
                for (auto& T : E.terms) if (T.sampler != 0) ++T.draws;
            }
            for (size_t t = 0; t < E.terms.size() && nsamp[i] < 0; ++t)              // resampling strategies: fresh points every evaluation, on device
                if (E.terms[t].sampler != 0) redraw_term(E, E.terms[t], true);
            // from the second step on the packed weight images are already those of the current theta: the update kernel below wrote them
            const bool fused = E.inv_ok && E.d_inv_ptr && std::getenv("PINN_NO_FUSED_ADAM") == nullptr;
            EvalRequest rq = EvalRequest::device(E.d_opt_theta, E.d_opt_out, term_w);
            rq.packed_fresh = fused && s > 0;
            if (run_loss_grad(E, rq)) return 1;
        }
        if (collective) {
            if (comm_all_reduce(es, ndev, vec.data(), raw.data())) return 1;
            for (int i = 0; i < ndev; ++i) {
                DeviceScope scope(es[i]->device);
                sums_from_double(es[i]->d_opt_out + P, es[i]->d_lossraw, K, es[i]->stream);      // the exact (double) sums replace the float-summed ones
            }
        }
        for (int i = 0; i < ndev; ++i) {
            pinn_engine& E = *es[i];
            DeviceScope scope(E.device);
            ++E.opt_t;
            const float c1 = adam_bias(beta1, E.opt_t), c2 = adam_bias(beta2, E.opt_t);
            // one update kernel per step: Adam + the evaluation's total loss + the new parameters scattered into the packed weight images
            // (PINN_NO_FUSED_ADAM=1: total_loss, adam and next step's pack as three launches)
            const bool fused = E.inv_ok && E.d_inv_ptr && std::getenv("PINN_NO_FUSED_ADAM") == nullptr;
            if (fused) {
                aux::AdamFusedArgs fa;
                std::memset(&fa, 0, sizeof fa);
                fa.theta = E.d_opt_theta; fa.m = E.d_opt_m; fa.v = E.d_opt_v; fa.out = E.d_opt_out; fa.P = P; fa.K = K;
                fa.lr = lr; fa.b1 = beta1; fa.b2 = beta2; fa.eps = eps; fa.c1 = c1; fa.c2 = c2;
                fa.inv_ptr = E.d_inv_ptr; fa.inv_pos = E.d_inv_pos;
                for (size_t n = 0; n < E.nets.size(); ++n) fa.packed[n] = E.netplans[n].d_packed;
                fa.hist = E.d_hist; fa.step = s; fa.w_over_n = E.d_w_over_n;
                aux::launch_adam_fused(fa, E.stream);
            } else {
                aux::launch_total_loss(E.d_hist, s, E.d_opt_out, P, K, E.d_w_over_n, E.stream);
                aux::launch_adam(E.d_opt_theta, E.d_opt_m, E.d_opt_v, E.d_opt_out, P, lr, beta1, beta2, eps, c1, c2, E.stream);
            }
        }
    }
    return 0;
}

// ---- persistent training kernel (pinn_train.hpp): the iterations of pinn_adam_steps, or one evaluation, inside ONE launch ----
// The launch shape both uses need: ONE fused family-1 launch group of ONE network whose spec carries the kernel (tanh / sigmoid), no
// communicator, float32, every workgroup resident (one per CU) and few enough for the one-stage reduction whose association the kernel repeats
// (aux::reduce_is_small) — i.e. the small problems of the reference's own test-suite.  PINN_PERSISTENT=0 (read per call) keeps the stand-alone
// kernels; results are bit-identical either way (tests/test_train_kernel.py).
bool train_shape_ok(const pinn_engine& E) {
    const char* e = std::getenv("PINN_PERSISTENT");
    if (!E.persistent || (e && std::atoi(e) == 0)) return false;
    if (E.comm || E.f64 || E.groups.size() != 1 || !E.coupled.empty() || E.nets.size() != 1) return false;
    const Group& G = E.groups[0];
    if (G.kind != 0 || !G.spec || G.spec->family != 1 || !G.spec->train) return false;
    if (G.ga.act != pk::ACT_TANH && G.ga.act != pk::ACT_SIGMOID) return false;
    const char* lim = std::getenv("PINN_REDUCE_DIRECT_MAX");
    const int direct_max = lim ? std::atoi(lim) : aux::REDUCE_DIRECT_MAX;
    return G.blocks <= direct_max && G.blocks <= 32 && G.blocks <= E.ncu;
}
// ... and of such a launch: every thread owns at most one element of [theta | K sums] with at most TRAIN_MAX_CONTRIB slab entries.  A launch
// with fewer threads than parameters (a handful of points under a comparatively large net) has nothing to win from the kernel
bool train_thread_per_element(const pinn_engine& E) {
    return E.groups[0].blocks * 256 >= (int)E.ntheta + (int)E.terms.size() && E.max_contrib <= pk::TRAIN_MAX_CONTRIB;
}
// K Adam iterations inside the launch: besides the shape, the optimiser's needs — the inverse pack map, no estimated PDE parameters, fixed or
// plainly redrawn point sets, and a thread per element that keeps its maps and optimiser state in registers (PINN_TRAIN_GENERAL=1: the kernel's
// general form, which re-reads them every step, runs the launches that miss this)
bool train_eligible(pinn_engine& E) {
    if (!train_shape_ok(E) || E.ne != 0 || !E.inv_ok || !E.d_inv_ptr) return false;
    for (auto& T : E.terms)          // redrawn point sets: drawn inside the kernel unless they carry embeddings or per-point data / weights
        if (T.sampler != 0 && (!T.emb_cols.empty() || T.ndata > 0 || T.pw_n > 0 || T.coupled >= 0 || T.src_root.size() > (size_t)aux::SRC_MAX)) return false;
    if (!train_thread_per_element(E) || E.max_inv_pos > pk::TRAIN_MAX_POS) return std::getenv("PINN_TRAIN_GENERAL") != nullptr;
    return true;
}
// one evaluation inside the launch: the shape without the optimiser's needs (estimated PDE parameters are fine here); callers that asked for
// HIP events around the kernels (pinn_set_timing) keep the stand-alone kernels those events bracket.  PINN_NO_FUSED_EVAL=1: never.
bool eval_eligible(pinn_engine& E) {
    return E.timing_level == 0 && !std::getenv("PINN_NO_FUSED_EVAL") && train_shape_ok(E) && train_thread_per_element(E);
}

// what a launch of the training kernel needs besides the optimiser: barrier words, the reduction inputs of the (single) launch group, the
// thread -> element map, the seeds of the reverse sweep.  Returns 0 / 1 (g_err set).
int train_common(pinn_engine& E, pk::TrainArgs& ta, const float* term_w) {
    const int K = (int)E.terms.size(), P = (int)E.ntheta;
    Group& G = E.groups[0];
    if (!E.d_bar) {
        E.d_bar = (unsigned*)plat_malloc(sizeof(unsigned) * 16);      // [0] arrivals, [1] time-out flag, [4..11] phase ticks of a PINN_STAMP build
        E.d_sums2 = (float*)plat_malloc(sizeof(float) * 2 * (size_t)std::max(K, 1));
        E.h_flag = (unsigned*)plat_host_alloc(sizeof(unsigned) * 4);
        if (!E.d_bar || !E.d_sums2 || !E.h_flag) return fail("device allocation failed (grid barrier words)");
        E.h_flag[0] = 0;
        E.bar_arrivals = 0;
        plat_memset(E.d_bar, 0, sizeof(unsigned) * 16, E.stream);     // (once: the arrival counter runs on from launch to launch)
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    }
    for (size_t j = 0; j < G.terms.size(); ++j) {
        const int ti = G.terms[j];
        G.ga.terms[j].scale = (float)(2.0 * (double)(term_w ? term_w[ti] : 1.0f) / (double)E.terms[ti].n_norm);
    }
    G.ga.slabs = G.d_slabs;
    G.ga.chain = 0;
    G.active = true;
    G.timed = false;
    G.launched_blocks = G.blocks;
    G.launched_by = 0;
    std::memset(&ta, 0, sizeof ta);
    ta.slabs = G.d_slabs; ta.losspart = G.d_losspart; ta.row_ptr = E.d_gr_ptr; ta.row_ent = E.d_gr_ent;
    ta.slab_floats = G.slab_floats; ta.nblocks = G.blocks;
    ta.P = P; ta.K = K;
    ta.sums2 = E.d_sums2;
    ta.bar = E.d_bar;
    ta.hflag = E.h_flag;
    ta.cached = (train_thread_per_element(E) && E.max_inv_pos <= pk::TRAIN_MAX_POS && std::getenv("PINN_TRAIN_NO_CACHE") == nullptr) ? 1 : 0;
    if (ta.cached && (!E.d_own_r || E.own_blocks != G.blocks)) {
        const std::vector<int> own = train_thread_map(G.row_theta, G.row_ptr, G.row_off, G.blocks, P, K,
                                                      std::getenv("PINN_TRAIN_NO_COALESCE") == nullptr, &E.hist_gid);
        plat_sync(E.stream);
        plat_free(E.d_own_r);
        E.d_own_r = (int*)plat_malloc(sizeof(int) * own.size());
        if (!E.d_own_r) return fail("device allocation failed (training kernel: thread map)");
        plat_h2d(E.d_own_r, own.data(), sizeof(int) * own.size(), E.stream);
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        E.own_blocks = G.blocks;
    }
    ta.own_r = E.d_own_r;
    ta.hist_gid = ta.cached ? E.hist_gid : 0;
    return 0;
}
// after a synchronisation: did a launch of the training kernel run into its barrier's time-out?  Then the barrier words start afresh and the
// handle keeps the stand-alone kernels from now on.
bool train_timed_out(pinn_engine& E) {
    if (E.h_flag[0] == 0 && std::getenv("PINN_TRAIN_FORCE_TIMEOUT") == nullptr) return false;
    E.h_flag[0] = 0;
    E.bar_arrivals = 0;
    plat_memset(E.d_bar, 0, sizeof(unsigned) * 16, E.stream);
    plat_sync(E.stream);
    E.persistent = false;
    std::fprintf(stderr, "[pinn] the persistent kernel's grid barrier timed out (its workgroups were not all resident: is the device shared?); "
                         "this handle continues with the stand-alone kernels\n");
    return true;
}

// ONE evaluation of a small problem in one launch (pinn_train.hpp, TrainArgs::eval_only): the residual kernel, a grid barrier and the
// fixed-order sums of aux::reduce_direct_body, thread per slab entry — instead of the residual kernel + the reduction kernel.  Only for
// callers that synchronise right after (the host entry points): a time-out is detected there and the evaluation repeated by the
// stand-alone kernels.  Same numbers bit for bit.  Returns 0 launched, 1 failure.
int eval_fused(pinn_engine& E, const float* d_theta, float* d_out, const float* term_w, double* lossraw) {
    Group& G = E.groups[0];
    pk::TrainArgs ta;
    if (train_common(E, ta, term_w)) return 1;
    pack_all(E, d_theta, false);
    ta.out = d_out; ta.lossraw = lossraw ? lossraw : E.d_lossraw;
    ta.eval_only = 1; ta.nsteps = 1;
    ta.arrivals0 = E.bar_arrivals;
    E.bar_arrivals += (unsigned)G.blocks;
    G.spec->train(G.ga, ta, G.blocks, E.stream);
    return 0;
}

// (theta, m, v) into the snapshot block E.d_opt_bak [3 P], or back from it
void opt_snapshot(pinn_engine& E, bool restore) {
    const size_t P = (size_t)E.ntheta;
    float* const state[3] = {E.d_opt_theta, E.d_opt_m, E.d_opt_v};
    for (size_t j = 0; j < 3; ++j) {
        float* const bak = E.d_opt_bak + j * P;
        plat_d2d(restore ? state[j] : bak, restore ? bak : state[j], sizeof(float) * P, E.stream);
    }
}

// returns 0 when all nsteps ran inside the kernel, 1 on failure (g_err set), 2 when the kernel's grid barrier timed out: the optimiser state
// and the draw counters are back where the call started and the caller runs the loop
int adam_steps_train(pinn_engine& E, int nsteps, float lr, float beta1, float beta2, float eps, const float* term_w) {
    const int P = (int)E.ntheta;
    Group& G = E.groups[0];
    pk::TrainArgs ta;
    if (train_common(E, ta, term_w)) return 1;
    std::vector<float> c12;
    if (!upload_c12(E, nsteps, beta1, beta2, c12)) return fail("device allocation failed (bias-correction table)");
    // snapshot of the optimiser state: a launch whose workgroups were not all resident (another process filling the device) ends by its
    // barrier time-out with wrong numbers — then the state is restored and the caller runs the stand-alone loop instead
    if (!E.d_opt_bak) {
        E.d_opt_bak = (float*)plat_malloc(sizeof(float) * 3 * (size_t)P);
        if (!E.d_opt_bak) return fail("device allocation failed (optimiser snapshot)");
    }
    opt_snapshot(E, false);
    std::vector<unsigned> draws0(E.terms.size());
    for (size_t t = 0; t < E.terms.size(); ++t) draws0[t] = E.terms[t].draws;
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());       // (c12 is a pageable temporary)
    pack_all(E, E.d_opt_theta, false);                        // the weight image of the current theta; the kernel keeps it current from here on
    ta.out = E.d_opt_out; ta.lossraw = E.d_lossraw;
    ta.theta = E.d_opt_theta; ta.m = E.d_opt_m; ta.v = E.d_opt_v;
    ta.lr = lr; ta.b1 = beta1; ta.b2 = beta2; ta.eps = eps;
    ta.inv_ptr = E.d_inv_ptr; ta.inv_pos = E.d_inv_pos; ta.packed = E.netplans[G.net].d_packed;
    ta.w_over_n = E.d_w_over_n;
    // redrawn point sets (device samplers): the host draws the set of a launch's FIRST step, exactly as the loop does before every step;
    // the kernel draws the sets of the following steps itself (pinn_train.hpp: train_resample)
    bool any_sampler = false;
    for (auto& T : E.terms) any_sampler = any_sampler || T.sampler != 0;
    ta.fenced = any_sampler ? 1 : 0;
    // launches of at most TRAIN_CHUNK iterations
    const char* chunk_env = std::getenv("PINN_TRAIN_CHUNK");                        // (tests: several launches per call)
    const int TRAIN_CHUNK = (chunk_env && std::atoi(chunk_env) > 0) ? std::atoi(chunk_env) : 4096;
    for (int s0 = 0; s0 < nsteps; s0 += TRAIN_CHUNK) {
        ta.nsteps = std::min(TRAIN_CHUNK, nsteps - s0);
        ta.c12 = E.d_c12 + 2 * (size_t)s0;
        ta.hist = E.d_hist + s0;
        if (any_sampler) {
            int max_n = 0;
            const int ns = upload_resample_table(E, &max_n);      // draw counters of this launch's first step
            if (ns < 0) return ns == -2 ? 1 : fail("pinn_adam_steps: a redrawn term of the persistent kernel carries embeddings or per-point data");
            aux::launch_resample((const pk::TrainSampler*)E.d_train_samp, ns, max_n, 0, E.stream);
            for (auto& T : E.terms) if (T.sampler != 0) T.draws += (unsigned)ta.nsteps;
            ta.nsamp = ns;
            ta.samp = (const pk::TrainSampler*)E.d_train_samp;
        }
        ta.arrivals0 = E.bar_arrivals;
        E.bar_arrivals += (unsigned)G.blocks * 2u * (unsigned)ta.nsteps;
        G.spec->train(G.ga, ta, G.blocks, E.stream);
    }
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    if (train_timed_out(E)) {
        opt_snapshot(E, true);                                // back to the state the call started from
        for (size_t t = 0; t < E.terms.size(); ++t) E.terms[t].draws = draws0[t];
        if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
        return 2;
    }
    E.opt_t += nsteps;
    return 0;
}

// checks and per-call device state shared by the Adam entry points
int adam_prepare(pinn_engine& E, int nsteps, const float* term_w, const char* who) {
    if (!E.d_opt_theta) return fail(std::string(who) + ": call pinn_adam_init first");
    if (nsteps <= 0) return fail(std::string(who) + ": nsteps must be positive");
    if (ensure_points(E)) return 1;
    const int K = (int)E.terms.size();
    for (auto& T : E.terms)
        if (T.sampler == 3 && T.seed == 0 && E.comm_size > 1)
            return fail(std::string(who) + ": an un-randomised Sobol design (seed 0) is the same on every rank and cannot be sharded; give the sampler a seed");
    if (!dev_grow(E.d_hist, E.hist_cap, (size_t)nsteps, E.stream)) return fail("device allocation failed (loss history)");
    std::vector<float> wn(K);
    for (int k = 0; k < K; ++k) wn[k] = (term_w ? term_w[k] : 1.0f) / (float)E.terms[k].n_norm;
    plat_h2d(E.d_w_over_n, wn.data(), sizeof(float) * K, E.stream);
    return plat_sync(E.stream) ? fail(std::string("device error: ") + plat_last_error()) : 0;      // (wn is a pageable temporary)
}

// the end of a call that ran nsteps on the ndev handles: the loss history (rank 0's), with last_out also the last step's [gradient | raw sums]
// of es[0] (sized by the caller), then every handle's stream drained
int adam_finish(pinn_engine** es, int ndev, int nsteps, double* loss_history, std::vector<float>* last_out = nullptr) {
    {
        pinn_engine& E = *es[0];
        DeviceScope scope(E.device);
        if (loss_history && plat_d2h(loss_history, E.d_hist, sizeof(double) * nsteps, E.stream)) return fail("D2H copy failed");
        if (last_out && plat_d2h(last_out->data(), E.d_opt_out, sizeof(float) * last_out->size(), E.stream)) return fail("D2H copy failed");
    }
    for (int i = 0; i < ndev; ++i) {
        DeviceScope scope(es[i]->device);
        if (plat_sync(es[i]->stream)) return fail(std::string("device error: ") + plat_last_error());
    }
    return 0;
}

}  // namespace

int pe::eval_one_launch(pinn_engine& E, float* d_out, const float* term_w, double* lossraw) {
    if (!eval_eligible(E)) return 2;
    if (eval_fused(E, E.d_theta, d_out, term_w, lossraw)) return 1;
    if (plat_sync(E.stream)) return fail(std::string("device error: ") + plat_last_error());
    return train_timed_out(E) ? 2 : 0;
}

extern "C" {

int pinn_adam_steps(pinn_handle h, int nsteps, float lr, float beta1, float beta2, float eps, const float* term_w, double* loss_history) {
    if (!h) return fail("null handle");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    if (E.comm && !E.comm_per_process && E.comm_size > 1)
        return fail("pinn_adam_steps: the handle belongs to a single-process communicator (pinn_comm_init_all): use pinn_adam_steps_sharded");
    if (E.f64) {                                         // float64 mode: redraw -> evaluate -> Adam, all in double on the device (f64_adam.cpp)
        if (nsteps <= 0) return fail("pinn_adam_steps: nsteps must be positive");
        E.adam_path = 1;
        return f64_adam_steps(E, nsteps, (double)lr, (double)beta1, (double)beta2, (double)eps, term_w, loss_history);
    }
    if (adam_prepare(E, nsteps, term_w, "pinn_adam_steps")) return 1;
    pinn_engine* es[1] = {&E};
    E.adam_path = 1;
    if (train_eligible(E)) {                     // small problems: every iteration inside one persistent launch (pinn_train.hpp)
        E.adam_path = 2;
        const int rc = adam_steps_train(E, nsteps, lr, beta1, beta2, eps, term_w);
        if (rc == 1) return 1;
        if (rc == 0) return adam_finish(es, 1, nsteps, loss_history);
        E.adam_path = 1;                         // (rc == 2: timed out and restored — the loop below runs the same steps)
    }
    if (adam_loop(es, 1, nsteps, lr, beta1, beta2, eps, term_w)) return 1;
    std::vector<float> gs;                               // "gemm" = "auto": the last step's [gradient | raw sums] (one small copy per CALL)
    if (E.gemm_auto && !E.comm) gs.resize((size_t)E.ntheta + E.terms.size());
    if (adam_finish(es, 1, nsteps, loss_history, gs.empty() ? nullptr : &gs)) return 1;
    if (!gs.empty()) {
        measure_grad_health(E, gs.data(), term_w);
        if (gemm_auto_check(E, E.d_opt_theta, term_w, E.opt_t)) return 1;      // (the optimiser state survives a re-plan: replan_gemm)
    }
    return 0;
}

int pinn_adam_steps_sharded(pinn_handle* hs, int ndev, int nsteps, float lr, float beta1, float beta2, float eps, const float* term_w,
                            double* loss_history) {
    if (!hs || ndev < 1) return fail("pinn_adam_steps_sharded: need at least one handle");
    for (int i = 0; i < ndev; ++i) {
        if (!hs[i] || !hs[i]->comm || hs[i]->comm_per_process || hs[i]->comm_size != ndev || hs[i]->comm_rank != i)
            return fail("pinn_adam_steps_sharded: pass the handles of one pinn_comm_init_all communicator, in rank order");
        if ((hs[i]->f64 != nullptr) != (hs[0]->f64 != nullptr)) return fail("pinn_adam_steps_sharded: the handles are in different precision modes");
        if (hs[i]->opt_t != hs[0]->opt_t) return fail("pinn_adam_steps_sharded: the handles' optimiser states are at different steps (pinn_adam_init every handle with the same theta)");
        if (hs[i]->f64) continue;
        DeviceScope scope(hs[i]->device);
        if (adam_prepare(*hs[i], nsteps, term_w, "pinn_adam_steps_sharded")) return 1;
    }
    if (hs[0]->f64) {                                    // float64 mode (r06): the double kernels, one all-reduce of [P + K] doubles per iteration
        if (nsteps <= 0) return fail("pinn_adam_steps_sharded: nsteps must be positive");
        return f64_adam_steps_comm(hs, ndev, nsteps, (double)lr, (double)beta1, (double)beta2, (double)eps, term_w, loss_history);
    }
    if (adam_loop(hs, ndev, nsteps, lr, beta1, beta2, eps, term_w)) return 1;
    return adam_finish(hs, ndev, nsteps, loss_history);
}

int pinn_adam_apply(pinn_handle h, const float* grad_and_sums, int64_t n, float lr, float beta1, float beta2, float eps, const float* term_w,
                    double* loss) {
    if (!h || !grad_and_sums) return fail("pinn_adam_apply: null argument");
    pinn_engine& E = *h;
    DeviceScope scope(E.device);
    const int K = (int)E.terms.size(), P = (int)E.ntheta;
    if (n != (int64_t)P + K) return fail("pinn_adam_apply: the vector must hold P + K floats ([gradient | raw per-term sums])");
    if (E.f64) {                                         // float64 mode: the optimiser state lives in double (f64_adam.cpp)
        std::vector<double> v(grad_and_sums, grad_and_sums + n);
        return f64_adam_apply(E, v.data(), (double)lr, (double)beta1, (double)beta2, (double)eps, term_w, loss);
    }
    if (adam_prepare(E, 1, term_w, "pinn_adam_apply")) return 1;
    if (plat_h2d(E.d_opt_out, grad_and_sums, sizeof(float) * (size_t)(P + K), E.stream)) return fail("H2D copy failed");
    ++E.opt_t;
    aux::launch_total_loss(E.d_hist, 0, E.d_opt_out, P, K, E.d_w_over_n, E.stream);
    aux::launch_adam(E.d_opt_theta, E.d_opt_m, E.d_opt_v, E.d_opt_out, P, lr, beta1, beta2, eps, adam_bias(beta1, E.opt_t), adam_bias(beta2, E.opt_t), E.stream);
    pinn_engine* es[1] = {&E};
    return adam_finish(es, 1, 1, loss);
}

}  // extern "C"

// the float / double twins (engine.cpp states the rule): the optimiser state lives in the HANDLE'S precision, T is the caller's
namespace {

template <class T> int adam_init_twin(const char* who, pinn_handle h, const T* theta, int64_t p) {
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    DeviceScope scope(E.device);
    if (E.f64) return f64_adam_init(E, as<double>(theta, (size_t)p).get());
    return adam_init_f32(E, as<float>(theta, (size_t)p).get());
}

template <class T> int adam_get_twin(const char* who, pinn_handle h, T* theta, int64_t p) {
    if (!h || !theta) return fail(std::string(who) + ": null argument");
    pinn_engine& E = *h;
    if (check_theta(E, who, p)) return 1;
    DeviceScope scope(E.device);
    if (E.f64) {
        auto th = as<double>(theta, (size_t)p);
        return f64_adam_get(E, th.get()) ? 1 : th.put();
    }
    auto th = as<float>(theta, (size_t)p);
    return adam_get_f32(E, th.get()) ? 1 : th.put();
}

}  // namespace

extern "C" {

int pinn_adam_init(pinn_handle h, const float* theta, int64_t p) { return adam_init_twin(__func__, h, theta, p); }
int pinn_adam_init_f64(pinn_handle h, const double* theta, int64_t p) { return adam_init_twin(__func__, h, theta, p); }
int pinn_adam_get(pinn_handle h, float* theta, int64_t p) { return adam_get_twin(__func__, h, theta, p); }
int pinn_adam_get_f64(pinn_handle h, double* theta, int64_t p) { return adam_get_twin(__func__, h, theta, p); }

}  // extern "C"
