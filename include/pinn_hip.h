/*
 * pinn_hip.h — C ABI of the MI355X-native PINN residual/loss engine (libpinn_hip.so).
 *
 * Drop-in boundary for NeuralPDE.jl's PhysicsInformedNN/discretize hot path.  The Julia glue
 *  `ccall`s these from the per-term loss closures that
 * `merge_strategy_with_loss_function` returns (reference: src/training_strategies.jl:131-160,
 * 247-269, 336-363) and from the `grad` of the OptimizationFunction built in
 * src/discretize.jl:776-780.  Plain pointers and sizes only; all matrices use the reference's
 * own memory layout (Julia column-major):
 *     points of a term      : d x N Float32, point-major (each point's d coordinates contiguous)
 *                             == the `cord` matrix of the generated loss function, src/discretize.jl:126-131
 *     theta / gradient      : flat vector in ComponentArrays order
 *                             [net(depvar 1): W1 (out x in, col-major) | b1 | W2 | b2 ... | net(depvar 2) ... | p]
 *                             == pinnrep.flat_init_params, src/discretize.jl:451-465
 * Every function returns 0 on success, non-zero on error; pinn_last_error() gives the message
 * (thread-local).  The engine computes with exact (Taylor-mode) derivatives, in fp32 on the device by default
 * (it reproduces the reference's Float64 finite-difference semantics to ~1e-7 relative at initialisation,
 * SURVEY.md §8c) or in float64 (pinn_set_option "precision"; every entry point has a double twin `_f64`).
 * There is NO CPU fallback: without a gfx950 device pinn_create fails.
 *
 * One handle = one caller thread at a time (the reference's loss closures are not re-entrant
 * either: `iteration[] += 1`, src/discretize.jl:574-576).
 */
#ifndef PINN_HIP_H
#define PINN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pinn_engine* pinn_handle;

/* ABI / build identification ("hip" for the product library). */
const char* pinn_backend(void);
int pinn_abi_version(void);
const char* pinn_last_error(void);

/*
 * Build an engine from a problem descriptor (text; "pinnir 1": residual tapes, or "pinnir 2": the equations as s-expressions, lowered
 * inside the library — grammar of both in DESIGN.md §2; optional trailing `hint <term> <points>` lines announce the sizes of the point
 * sets the caller is going to install, so that the planner can put small terms onto a launch their network already has).
 * The descriptor carries what symbolic_discretize extracts from the PDESystem:
 * chains (sizes, activation, offset in theta)   <- pinnrep.phi / flat_init_params   (src/discretize.jl:432-465)
 * per term: dimension, jet slots, residual tape <- symbolic_pde/bc_loss_functions   (src/discretize.jl:505-525)
 * Replaces: build_loss_function + RuntimeGeneratedFunction (src/discretize.jl:163-175).
 * Unsupported expressions / network shapes fail HERE (never a silent fallback).
 *
 * INTEGRAL TERMS ("pinnir 1" extension; the reference's `Integral(s in ClosedInterval(lo, hi))(f)`, src/discretize.jl:355-396).  A term whose
 * residual holds integral nodes I(x) = int_lo^hi f(s; x, u, du, p) ds carries them between its `term` line and its own `slot` lines:
 *     term <k> <d> <#slots> <#ops> <out row>
 *     integrals <NI>                                        1 <= NI <= 4
 *     integral <var> <lo> <hi> <#slots> <#ops> <out row>    NI blocks; <var>: coordinate index of the integration variable; <lo>, <hi>: a finite
 *     slot ... / op ...                                       number, or x<i> = coordinate i of the collocation point (x<var> gives the reference's 0..t)
 *     slot ... / op ...                                     the term's own slots and ops
 * Rows of the term's tape: [coordinates | parameters | slots | integral nodes | ops] — node j is row d + np + #slots + j, read like a jet slot.
 * Rows of a node's tape (the integrand): [coordinates, row <var> holding the quadrature abscissa | parameters | the node's slots | its ops]; its
 * slots are evaluated at the substituted point.  The node is evaluated as a Q-node Gauss-Legendre rule on [lo, hi],
 * (hi - lo)/2 * sum_q w_q f(lo + (hi - lo)(xi_q + 1)/2), Q = option "integral_nodes"; nodes and weights are computed in double by the library.
 * Refused at pinn_create with the limit named: bounds that are not a finite number or a coordinate, integrands without a dependent variable,
 * lap slots / DATA ops inside a node, integral terms that reference several networks, a DGM network or a periodically embedded network.
 * "pinnir 2": the node is the list `(integral <var> <lo> <hi> <body>)` inside lhs / rhs — <var> an independent variable of the term, <lo> / <hi> a
 * number or an independent variable, <body> any expression of the form's grammar holding a dependent variable — lowered to the same nodes;
 * nested integrals, a list in place of <var> (multi-variable), Inf bounds, bounds that are expressions and bodies without a dependent
 * variable are refused by name.  A term with integral nodes may list a slot only once per node and once among its own slots.
 */
int pinn_create(const char* descriptor, pinn_handle* out);          /* on the caller's current HIP device */
int pinn_create_on(const char* descriptor, int device, pinn_handle* out);   /* on HIP device `device` (single process, several GPUs) */
int pinn_destroy(pinn_handle h);

/* Number of loss terms K (pde terms first, then bcs: the order of src/discretize.jl:569-570) and length of theta. */
int pinn_num_terms(pinn_handle h);
int64_t pinn_num_theta(pinn_handle h);

/*
 * Install the collocation set of one term (host pointer; copied to HBM and kept resident).
 * Replaces the `train_set` captured by get_loss_function (src/training_strategies.jl:215-221) or the
 * per-call sample of StochasticTraining / QuasiRandomTraining (:271-282, :365-389).
 * n_norm: the N of mean(abs2, .) — the GLOBAL point count when the set is one shard of a
 * multi-GPU partition; pass 0 for n_norm == n.
 */
int pinn_set_points(pinn_handle h, int term, const float* pts, int64_t n, int64_t n_norm);
/* Same, `pts` already in device memory (adopted by copy). */
int pinn_set_points_device(pinn_handle h, int term, const float* d_pts, int64_t n, int64_t n_norm);

/*
 * One evaluation of full_loss_function and its reverse-mode gradient (src/discretize.jl:567-598, :778):
 *   term_losses[k] = mean(abs2, residual_k(set_k, theta))            (K doubles, unweighted)
 *   grad           = d/dtheta sum_k term_w[k] * term_losses[k]       (P floats, nullable)
 * theta: P floats (host).  term_w: K floats (adaptive-loss weights, src/adaptive_losses.jl; NULL = ones).
 * Deterministic: identical inputs give bit-identical outputs.
 * grad == NULL selects the LOSS-ONLY evaluation: forward pass + residual + sums of squares, no records, no reverse sweep, no
 * gradient reduction (about a third of the full evaluation) — the cost class of the reference's per-term closures when they are only
 * evaluated, not differentiated (src/training_strategies.jl:215-221: callbacks, MiniMax / SoftAdapt reweighting, rejected line-search
 * trials).  The per-point residuals are those of the full evaluation bit for bit and their squares are summed in double precision, so
 * the term losses agree with the full evaluation's to the order of those sums (1e-13 relative; identical as floats).
 */
int pinn_loss_grad(pinn_handle h, const float* theta, int64_t p, const float* term_w,
                   double* term_losses, float* grad);
/* Float64 convenience for the reference's default eltype (src/discretize.jl:432-449): converts at the boundary. */
int pinn_loss_grad_f64(pinn_handle h, const double* theta, int64_t p, const double* term_w,
                       double* term_losses, double* grad);
/*
 * Per-term gradients for GradientScaleAdaptiveLoss (src/adaptive_losses.jl:112-123):
 * term_grads is K x P (row k = d term_losses[k] / d theta), row-major.
 */
int pinn_term_grads(pinn_handle h, const float* theta, int64_t p, double* term_losses, float* term_grads);
/* The same with theta and the K x P gradients in double (r06): native on a handle in float64 mode, fp32 kernels + widening otherwise. */
int pinn_term_grads_f64(pinn_handle h, const double* theta, int64_t p, double* term_losses, double* term_grads);

/*
 * BPINN physics (+ data) log-likelihood and its gradients in one evaluation:
 *   loglik = sum_k logpdf(MvNormal(residual_k(set_k, theta), stds[k]^2 I), 0)
 *          = sum_k [ -N_k/2 log(2 pi) - N_k log stds[k] - SSE_k / (2 stds[k]^2) ]                     (SSE, not MSE)
 * i.e. the sum the reference's BayesianPINN builds from get_points_loss_functions (src/training_strategies.jl:113-127,
 * src/discretize.jl:678-754, ext/bpinn/PDE_BPINN.jl:16-26) over the pde and bc terms; a data-misfit term (descriptor op DATA) with
 * its own std is the L2LossData term (ext/bpinn/PDE_BPINN.jl:148-183).  grad_theta (P floats, nullable) = d loglik / d theta by the
 * engine's reverse sweep (the reference differentiates with ForwardDiff over all P parameters, ext/bpinn/PDE_BPINN.jl:519);
 * grad_std (K doubles, nullable) = d loglik / d stds[k] = -N_k / s + SSE_k / s^3 for samplers that treat the stds as parameters.
 * N_k is the number of points INSTALLED for term k (pinn_set_points' n), not its n_norm: with sharded point sets (n < n_norm) every
 * returned quantity is this shard's additive part — loglik, grad_theta and grad_std summed over the ranks are the global values; a caller
 * that passes n_norm != n for another reason (a re-normalised mean) gets the constants of n points here.
 */
int pinn_loglik_grad(pinn_handle h, const float* theta, int64_t p, const double* stds, double* loglik, float* grad_theta, double* grad_std);
/* theta and grad_theta in double (r06; the reference's BPINN samples Float64 parameters, ext/bpinn/PDE_BPINN.jl:519): native on a handle in
 * float64 mode, fp32 kernels + widening otherwise. */
int pinn_loglik_grad_f64(pinn_handle h, const double* theta, int64_t p, const double* stds, double* loglik, double* grad_theta, double* grad_std);
/*
 * Device-resident variant for multi-GPU data parallelism (one process per GPU; the caller
 * all-reduces d_out with RCCL): d_theta = P floats in HBM; d_out = P + K floats in HBM:
 *   d_out[0..P)   = this shard's gradient contribution (already scaled by term_w[k]/n_norm_k)
 *   d_out[P..P+K) = this shard's sum of squared residuals per term (divide by n_norm_k after the all-reduce)
 * Asynchronous on `stream` (a hipStream_t; NULL = the default stream, e.g. torch's current stream).
 * d_out may be any device-accessible address, including pinned device-mapped host memory (hipHostMalloc): the last
 * reduction kernel then delivers the result to the host without a copy command (what pinn_loss_grad does internally).
 */
int pinn_loss_grad_device(pinn_handle h, const float* d_theta, const float* term_w, float* d_out, void* stream);
/* The same for a handle in the float64 evaluation mode (pinn_set_option(h, "precision", "f64")) with DOUBLE device buffers: d_theta = P doubles,
 * d_out = P + K doubles — the Float64 caller's residual + gradient without a narrowing at the boundary and without PCIe (the device-array form
 * of src/discretize.jl:541-545 with Float64 parameters).  Fails on a handle that is not in the mode. */
int pinn_loss_grad_device_f64(pinn_handle h, const double* d_theta, const float* term_w, double* d_out, void* stream);
/* Loss-only counterpart: d_sums = K floats in device-accessible memory = this shard's sum of squared residuals per term
 * (divide by n_norm_k; the same numbers pinn_loss_grad_device writes to d_out[P..P+K)).  Asynchronous on `stream`. */
int pinn_loss_device(pinn_handle h, const float* d_theta, float* d_sums, void* stream);

/*
 * Engine-owned data parallelism over the GPUs of one node: every term's point set is split into contiguous column
 * blocks (install each block with pinn_set_points(..., n_norm = GLOBAL N)), theta is replicated, and ONE RCCL all-reduce (sum, fp32) of
 * the packed vector [gradient (P) | per-term sums of squares (K)] — 51 KB for 4x64 — completes the evaluation on the evaluation's own
 * stream.  The reference aggregates the K term losses on the host (src/discretize.jl:568-588); this is that aggregation across devices.
 *   one process per GPU : rank 0: pinn_comm_unique_id(id); distribute the PINN_COMM_ID_BYTES bytes; all ranks: pinn_comm_init_rank;
 *                         per evaluation pinn_loss_grad_sharded_device (as pinn_loss_grad_device, d_out all-reduced in place; d_out
 *                         must be device memory; divide the K sums by n_norm_k afterwards).
 *   one process, G GPUs : pinn_create_on(desc, g) for g = 0..G-1; pinn_comm_init_all(handles, G) (ncclCommInitAll); per evaluation
 *                         pinn_loss_grad_sharded(handles, G, theta, ...) = pinn_loss_grad over all shards (host pointers in and out).
 * RCCL is loaded on first use; single-GPU work never needs it.
 *   bring your own collective : pinn_comm_init_custom(h, nranks, rank, fn, ctx) makes `fn` the transport of this handle's communicator
 *                         (one process per GPU): the engine calls  fn(ctx, buf, count, dtype, stream)  to sum `count` elements of `buf`
 *                         (dtype 0: float, 1: double; device memory of this rank) over the ranks IN PLACE, ordered after the work already
 *                         queued on `stream` and before whatever the engine queues next (an MPI caller synchronises the stream and calls
 *                         MPI_Allreduce on the device pointers; a torch caller wraps them and calls dist.all_reduce).  Non-zero = failure.
 *
 * The RESIDENT training loop over a communicator (r04): pinn_adam_steps on a handle that belongs to a one-process-per-GPU communicator
 * (pinn_comm_init_rank / _custom), or pinn_adam_steps_sharded over the handles of a pinn_comm_init_all communicator, runs per iteration
 *     [redraw this rank's sampled sets] -> evaluate the local shards -> ONE in-stream all-reduce of [gradient | sums] (+ the K sums as
 *     doubles) -> fused Adam update + weight-image scatter on EVERY rank
 * with nothing crossing PCIe and no host synchronisation inside the loop: every rank applies the identical update to its identical copy
 * of theta (pinn_adam_init with the same theta on every rank).  This is `solve(prob, Adam(lr); maxiters)` over full_loss_function
 * (test/NNPDE1/nnpde__pde_ii_2d_poisson.jl:83-85, src/discretize.jl:567-598) with the K-term aggregation done across devices.
 * Device samplers draw rank-specific points (the rank is mixed into the seed); an un-randomised Sobol design (seed 0) cannot be sharded.
 */
#define PINN_COMM_ID_BYTES 128
typedef int (*pinn_allreduce_fn)(void* ctx, void* buf, int64_t count, int dtype, void* stream);
int pinn_comm_init_custom(pinn_handle h, int nranks, int rank, pinn_allreduce_fn fn, void* ctx);
int pinn_adam_steps_sharded(pinn_handle* hs, int ndev, int nsteps, float lr, float beta1, float beta2, float eps, const float* term_w,
                            double* loss_history);
/* One Adam update of the resident state from a caller-supplied vector [gradient (P) | raw per-term sums (K)] in host memory: the
 * host-optimiser form of the sharded loop (evaluate with pinn_loss_grad_sharded, apply here); *loss (nullable) = sum_k w_k sums_k / n_norm_k. */
int pinn_adam_apply(pinn_handle h, const float* grad_and_sums, int64_t n, float lr, float beta1, float beta2, float eps, const float* term_w,
                    double* loss);
int pinn_comm_unique_id(void* id, int64_t nbytes);
int pinn_comm_init_rank(pinn_handle h, int nranks, int rank, const void* id, int64_t nbytes);
int pinn_comm_init_all(pinn_handle* hs, int ndev);
int pinn_comm_size(pinn_handle h);
int pinn_comm_rank(pinn_handle h);
int pinn_comm_destroy(pinn_handle h);
int pinn_loss_grad_sharded_device(pinn_handle h, const float* d_theta, const float* term_w, float* d_out, void* stream);
int pinn_loss_grad_sharded(pinn_handle* hs, int ndev, const float* theta, int64_t p, const float* term_w,
                           double* term_losses, float* grad);
/* The same over handles / buffers in the FLOAT64 evaluation mode (r06): this rank's shards by the double kernels, ONE all-reduce of [P + K] doubles
 * (ncclDouble; a caller's transport is called with dtype 1).  pinn_adam_steps on a float64-mode handle with a one-process-per-GPU communicator and
 * pinn_adam_steps_sharded over float64-mode handles run the resident double loop with that all-reduce inside every iteration. */
int pinn_loss_grad_sharded_device_f64(pinn_handle h, const double* d_theta, const float* term_w, double* d_out, void* stream);
int pinn_loss_grad_sharded_f64(pinn_handle* hs, int ndev, const double* theta, int64_t p, const double* term_w,
                               double* term_losses, double* grad);

/* residual_k(set_k, theta): the datafree loss function of src/discretize.jl:174 on the installed set; r has n_k floats. */
int pinn_residual(pinn_handle h, int term, const float* theta, int64_t p, float* r);
/* Trial function phi(x, theta) of one net (src/pinn_types.jl:88-90): pts = d x n point-major, out = n floats. */
int pinn_phi(pinn_handle h, int net, const float* theta, int64_t p, const float* pts, int64_t n, float* out);
/*
 * derivative(phi, u, x, eps, order, theta) of one net at n points (numeric_derivative, src/pinn_types.jl:445-482; its epsilons come from
 * get_eps, src/symbolic_utilities.jl:98-103): the derivative of the trial function of order `order` (0..4) along `axes[0..order)`
 * (network-input axes, 0-based; order 2 may be mixed, orders 3-4 are along one axis).  The engine returns the EXACT derivative the
 * Taylor-jet kernels carry (the value the reference's central differences approximate to ~1e-8, test/Forward/forward__derivatives.jl:22-44).
 */
int pinn_derivative(pinn_handle h, int net, const float* theta, int64_t p, const float* pts, int64_t n, int order, const int* axes, float* out);
/*
 * The three per-point closures in DOUBLE (r06).  The reference evaluates them in eltype(theta), Float64 by default (src/discretize.jl:432-449,
 * src/eltype_matching.jl:8-10), and pins them at Float64 tolerances: datafree_pde_loss_functions[i](cord, theta) at rtol 1e-8
 * (src/pinn_types.jl:435-439, test/Forward/forward__ode.jl:46-47), numeric_derivative against automatic differentiation at atol 1e-8 / 4e-5
 * (src/pinn_types.jl:445-482, test/Forward/forward__derivatives.jl:29-44), phi(x, theta) (src/pinn_types.jl:88-90).  On a handle in float64
 * mode (pinn_set_option(h, "precision", "f64")) theta, points and results cross the boundary in double and the double kernels evaluate them
 * (matrix-pipe tile kernels where instantiated, one lane per point elsewhere): results equal a Float64 evaluation to rounding.  On an fp32
 * handle they narrow / widen at the boundary (the fp32 kernels run).  pinn_derivative_f64 covers the derivatives the float64 jet sets carry
 * (orders <= 2 in 1-3 inputs, pure orders 3-4, first + pure second in 4 inputs); anything else fails with a message.
 * pinn_residual_f64 reads the term's set as installed: pinn_set_points_f64 for Float64 coordinates.
 */
int pinn_residual_f64(pinn_handle h, int term, const double* theta, int64_t p, double* r);
int pinn_phi_f64(pinn_handle h, int net, const double* theta, int64_t p, const double* pts, int64_t n, double* out);
int pinn_derivative_f64(pinn_handle h, int net, const double* theta, int64_t p, const double* pts, int64_t n, int order, const int* axes, double* out);

/*
 * Resident-theta training loop: theta, the Adam moments and the collocation sets stay in HBM; no
 * per-iteration PCIe traffic.  Mirrors `solve(prob, Adam(lr); maxiters)` ([3P] OptimizationOptimisers, used by every
 * reference test, e.g. test/NNPDE1/nnpde__pde_ii_2d_poisson.jl:83) on the objective of pinn_loss_grad.
 *   pinn_set_sampler : kind 1 = redraw the term's points uniformly in [lb, ub] on the device before every step
 *                      (StochasticTraining, src/training_strategies.jl:242-245, 277-281); kind 2 = Latin-hypercube redraw
 *                      (QuasiRandomTraining with its default LatinHypercubeSample and resampling = true, :321, 375-381);
 *                      kind 3 = Sobol' design (QuasiRandomTraining with SobolSample: Gray-code sequence, Joe-Kuo direction numbers,
 *                      first element skipped as in Sobol.jl; seed 0 = the plain sequence on every draw, otherwise a fresh digital shift per draw);
 *                      kind 0 = keep the installed set.
 *   pinn_adam_init   : upload theta (P floats), zero the moments.
 *   pinn_adam_steps  : nsteps updates m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2, theta -= lr m^/(sqrt(v^) + eps);
 *                      loss_history (nullable) receives the weighted total loss of every step.
 *   pinn_adam_get    : download theta.
 */
int pinn_set_sampler(pinn_handle h, int term, int kind, const float* lb, const float* ub, int64_t n, uint64_t seed);
/*
 * Per-point data of a term whose residual contains DATA channels (descriptor op `DATA j`): ndata x N floats, channel-major, for the
 * point set installed last (observations d_i of a data-misfit term  u(x_i) - d_i, the usual content of the reference's
 * `additional_loss`, e.g. docs/src/tutorials/param_estim.md:79-95, evaluated inside the fused loss + gradient instead of on the host).
 */
int pinn_set_point_data(pinn_handle h, int term, const float* data, int ndata, int64_t n);
/* the same with the observations in double: the float64 evaluation mode reads them as given, the fp32 kernels their float conversion */
int pinn_set_point_data_f64(pinn_handle h, int term, const double* data, int ndata, int64_t n);
/*
 * Quadrature weights for the term's current point set: the term's loss becomes  sum_i w[i] * r_i^2  (with sum_i w[i] = 1: a weighted mean,
 * e.g. a tensor Gauss-Legendre rule — (1/area) * integral of r^2, the objective of the reference's QuadratureTraining,
 * src/training_strategies.jl:451-481) instead of mean(abs2, r).  NULL restores the plain mean.  Sharded sets: pass the shard's
 * weights of the GLOBAL rule (n_norm of pinn_set_points is then only a scale that cancels).
 */
int pinn_set_point_weights(pinn_handle h, int term, const float* w, int64_t n);
/* Copy the term's current collocation set (d x N, point-major, as installed or as last drawn by the device sampler) to the host. */
int pinn_get_points(pinn_handle h, int term, float* pts, int64_t n);
int pinn_adam_init(pinn_handle h, const float* theta, int64_t p);
int pinn_adam_steps(pinn_handle h, int nsteps, float lr, float beta1, float beta2, float eps, const float* term_w, double* loss_history);
int pinn_adam_get(pinn_handle h, float* theta, int64_t p);
/* The same in double (r05).  On a handle in float64 mode (pinn_set_option(h, "precision", "f64")) the WHOLE loop runs in double on the
 * device — parameters, moments, the redrawn point sets (the fp32 samplers' points widened on the device: StochasticTraining /
 * QuasiRandomTraining(resampling = true) with the reference's default Float64 parameters, src/discretize.jl:432-449,
 * src/training_strategies.jl:271-282, 365-389), residual + gradient kernels, Adam — and pinn_adam_init / pinn_adam_get convert at the
 * boundary; in float32 mode these two narrow / widen at the boundary.
 * Each precision mode keeps an optimiser state of its own: pinn_adam_steps continues the state of the mode the handle is in.  The double state goes
 * with the mode ("precision" = "f32" frees it: after a return to "f64" pinn_adam_steps / pinn_adam_get are refused until pinn_adam_init is called
 * again), the fp32 state survives a visit to "f64".  Evaluations, pinn_phi / pinn_derivative / pinn_phi_ensemble, pinn_lbfgs, the resident L-BFGS and
 * HMC, pinn_set_timing, "persistent" on / off and an option or a point set taken to another value and back between two pinn_adam_steps calls leave
 * the iterate, the moments and the step counter alone: k1 + k2 steps in two calls are bit-equal to k1 + k2 in one (tests/test_handle_history.py). */
int pinn_adam_init_f64(pinn_handle h, const double* theta, int64_t p);
int pinn_adam_get_f64(pinn_handle h, double* theta, int64_t p);
/*
 * L-BFGS on the weighted objective sum_k w_k L_k over FIXED point sets (the quasi-Newton finisher of the reference's scripts,
 * `solve(prob, BFGS() / LBFGS(); maxiters)`, e.g. test/NNPDE1/nnpde__pde_ii_2d_poisson.jl:86 — there [3P] OptimizationOptimJL on the
 * host; here inside the library so that C / Julia / Python callers share it).  theta (double, in/out) is iterated in double precision
 * on the host; every objective / gradient evaluation is one fused device evaluation in fp32.  Two-loop recursion with `history` pairs,
 * backtracking line search (Armijo), stops after `maxiters` iterations, when the gradient's max-norm falls below `gtol`, or when the line
 * search cannot decrease the objective any more (the noise floor of the evaluation; a handle in "split" GEMM mode first switches itself to
 * "fp32" there and goes on — the split products' floor is 2-4 x higher — and is switched back before the call returns;
 * $PINN_LBFGS_KEEP_GEMM=1 disables that).  loss_history (nullable): objective after every iteration,
 * `maxiters` entries; *iters_done: iterations performed.  Terms with device samplers are refused (the objective must not change).
 */
int pinn_lbfgs(pinn_handle h, double* theta, int64_t p, int maxiters, int history, double gtol, const float* term_w, double* loss_history,
               int* iters_done);

/*
 * RESIDENT HMC: the transition loop of the BPINN sampler (`ahmc_bayesian_pinn_pde` with Kernel = HMC(eps, n_leapfrog),
 * ext/bpinn/PDE_BPINN.jl:371-640) on the device.  theta, momentum, the diagonal inverse metric, the log-posterior gradient and the energies stay in
 * HBM in double; pinn_hmc_draws runs `ndraws` complete transitions — momentum draw, n_leapfrog leapfrog steps, Metropolis accept / reject — without
 * a host synchronisation and downloads everything once at its end.  A leapfrog step is the handle's own resident evaluation (the double kernels in
 * float64 mode; the fp32 kernels at (float)theta otherwise, their K sums of squares in double) plus one fused update launch.  Opt-in: nothing else in
 * the library uses it.  The state has buffers of its own — evaluations and pinn_adam_* between two calls leave the chain alone and vice versa.
 *   log-posterior  logp(theta) = loglik(theta)                                         exactly pinn_loglik_grad's number for stds[0..k)
 *                               + sum_{i < P - n_prior} logpdf(Normal(nn_mu, nn_sigma), theta_i)          the network weights
 *                               + sum_{j < n_prior} logpdf(prior_j, theta_{P - n_prior + j})             the trailing PDE parameters;
 *                  prior_kind[j] = 0: Normal(prior_mu[j], prior_sigma[j]); 1: LogNormal(prior_mu[j], prior_sigma[j]) — its log-density at x <= 0 is
 *                  -inf (gradient 0), so a proposal that carries the parameter there is rejected.
 *   transition     r = z / sqrt(minv), z ~ N(0, I);  H = -logp + 1/2 sum_i minv_i r_i^2;
 *                  r += eps/2 grad logp;  then n_leapfrog times { theta += eps minv r;  evaluate;  r += eps grad logp (eps/2 the last time) };
 *                  a = exp(min(0, H_old - H_new)), a = 0 when H_new is not finite;  accept iff u < a, u ~ U[0, 1).
 *   pinn_hmc_init        uploads theta (p doubles), checks and stores stds (k == pinn_num_terms) and the priors, evaluates logp and its gradient
 *                        at theta once, sets the unit metric and the draw counter 0.  A second call replaces the state.
 *   pinn_hmc_set_metric  p positive entries of the diagonal inverse mass matrix; NULL: ones.
 *   pinn_hmc_draws       momenta: ndraws x p doubles, row i = the momentum r of draw i (used as given), or NULL; uniforms: ndraws doubles or NULL;
 *                        samples (nullable): ndraws x p, row i = the state AFTER draw i; accept_prob[i] = a of draw i; logp[i] = logp of that state.
 *   pinn_hmc_get         the current state: theta (p doubles), *logp (nullable), grad = d logp / d theta (p doubles, nullable).
 * GENERATOR (momenta / uniforms == NULL), counter-based, all arithmetic in uint32 (wrapping) and double:
 *     mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16                  (csrc/sample_rules.hpp)
 *     key     = mix32( mix32(seed_lo + 0x9E3779B9 * seed_hi) ^ (c * 0x85EBCA6B + 0xC2B2AE35) )              c = draw counter, seed = seed_hi : seed_lo
 *     word(e, j) = mix32( key ^ mix32((2 e + j) * 0x9E3779B9 + 0x165667B1) )
 *     z_e     = sqrt(-2 ln((word(e, 0) + 1) / 2^32)) * cos(6.283185307179586 * (word(e, 1) / 2^32))         Box-Muller, element e of theta
 *     u       = word(P, 0) / 2^32
 *   The draw counter lives in the handle, starts at 0 in pinn_hmc_init and advances by one per completed draw (also when momenta and uniforms are
 *   supplied): 2 + 3 draws in two calls are bit-equal to 5 draws in one.
 * The precision mode taken to the other value AND BACK between two calls is not a change: the chain continues, and its evaluations read the point
 * sets as the mode holds them after the return (double copies converted from the float buffers).
 * Refused, with the handle left as it was: any call before pinn_hmc_init; a handle whose precision mode changed since (init again); a term with a
 * device sampler (the target must be fixed, as for pinn_lbfgs); a handle on a communicator; p != ntheta, k != the number of terms; stds, prior
 * sigmas or metric entries that are not positive; eps <= 0, n_leapfrog < 1, ndraws < 1.
 */
int pinn_hmc_init(pinn_handle h, const double* theta, int64_t p, const double* stds, int k, double nn_mu, double nn_sigma,
                  int n_prior, const int* prior_kind, const double* prior_mu, const double* prior_sigma);
int pinn_hmc_set_metric(pinn_handle h, const double* inv_metric, int64_t p);
int pinn_hmc_draws(pinn_handle h, int ndraws, int n_leapfrog, double eps, uint64_t seed, const double* momenta, const double* uniforms,
                   double* samples, int64_t p, double* accept_prob, double* logp);
int pinn_hmc_get(pinn_handle h, double* theta, int64_t p, double* logp, double* grad);

/*
 * RESIDENT HMC WARM-UP: the other half of the sampler — AdvancedHMC's find_good_stepsize and StanHMCAdaptor with a
 * DiagEuclideanMetric as neuralpde.jl_amd/bpinn.py `_hmc_device` restates them — with the chain of pinn_hmc_init resident.  Opt-in; pinn_hmc_draws
 * and every other path are unchanged.  All adaptation arithmetic is double with floating-point contraction off, in `_hmc_device`'s order.
 *   pinn_hmc_find_stepsize  the initial search.  normals: p standard normals z, or NULL: the generator above with the FIXED counter 2^32 - 1 (the
 *                        search neither reads nor advances the draw counter).  r0 = z / sqrt(minv) under the handle's current metric,
 *                        h0 = -logp(current) + 1/2 sum minv r0^2; a trial at eps is one leapfrog step from the current state with r0 and the stored
 *                        gradient, d = h0 - H(eps), a non-finite d counts as -inf.  The first trial runs at eps0 and fixes the direction (up iff
 *                        d > log 0.8); eps is then doubled / halved for at most 40 further trials until d crosses log 0.8 (up: d <= log 0.8;
 *                        down: d > log 0.8).  *eps = the last eps tried, *ntrials (nullable) = trials run, 1..41.  One double pair is read back
 *                        per trial (the loop is data-dependent).  The chain is left exactly where it was: theta, gradient, logp, metric, counter.
 *   pinn_hmc_warmup      n_adapts transitions as in pinn_hmc_draws, each followed ON THE DEVICE by the adaptation; no host synchronisation inside
 *                        the call, one download at its end.
 *       normals    n_adapts x p STANDARD NORMALS z (row i for draw i), or NULL.  The device forms r = z / sqrt(minv) with the metric in force at
 *                  that draw — unlike the `momenta` of pinn_hmc_draws, which are used as given: the metric changes inside this call, so a caller
 *                  cannot pre-divide.  uniforms: n_adapts doubles or NULL.  NULL: the generator above, same key, same counter as pinn_hmc_draws.
 *                  The draw counter advances by one per completed draw.
 *       outputs    samples (nullable, n_adapts x p), accept_prob, logp (n_adapts each): as in pinn_hmc_draws.  step_sizes (nullable, n_adapts):
 *                  step_sizes[i] = the eps draw i ran with, step_sizes[0] == eps0.  *eps_final: the step size to sample with afterwards.
 *                  inv_metric (nullable, p): the metric in force after the call.
 *       step size  t0 = 10, gamma = 0.05, kappa = 0.75, mu = log(10 eps0), hbar = log_eps_bar = 0, m = 0; after a draw with acceptance a:
 *                  m += 1;  hbar = (1 - 1/(m + t0)) hbar + (target - a)/(m + t0);  log_eps = mu - sqrt(m)/gamma hbar;  eta = pow(m, -kappa);
 *                  log_eps_bar = eta log_eps + (1 - eta) log_eps_bar;  eps = exp(log_eps).
 *       metric     w0 = (int)(0.15 n_adapts), w1 = (int)(0.9 n_adapts) (double arithmetic).  After draw w1 - 1, if w1 - w0 >= 8 and n_adapts >= 100:
 *                  minv_i = (k/(k + 5)) var_i + 1e-3 (5/(k + 5)), var_i the population variance (mean first, then squared deviations, rows in
 *                  order) of element i over the k = w1 - w0 states after draws [w0, w1); then mu = log(10 eps) with the eps just updated and
 *                  hbar = log_eps_bar = m = 0.  Shorter warm-ups keep the metric they started with.
 *       the end    after the last draw eps = exp(log_eps_bar) if m > 0: *eps_final.
 *       afterwards the chain sits at the last draw and the handle holds the adapted metric as if pinn_hmc_set_metric had been called:
 *                  pinn_hmc_draws(..., *eps_final, ...) continues the run.  The warm-up starts from the metric the handle holds (ones after
 *                  pinn_hmc_init).  A warm-up is one call: its dual-averaging state does not carry over to a second one.
 * Refused, with the handle and the chain left as they were: everything pinn_hmc_draws refuses; n_adapts < 1; n_leapfrog < 1; eps0 not positive
 * and finite; target outside (0, 1); NULL accept_prob, logp or eps_final; for the search NULL eps.  An evaluation that fails in mid-call leaves the
 * chain at its last completed draw, the counter advanced by the completed draws, and the metric the one in force at that draw: the adapted one if
 * draw w1 - 1 had completed, the initial one otherwise.
 */
int pinn_hmc_find_stepsize(pinn_handle h, double eps0, uint64_t seed, const double* normals, int64_t p, double* eps, int* ntrials);
int pinn_hmc_warmup(pinn_handle h, int n_adapts, int n_leapfrog, double eps0, double target, uint64_t seed, const double* normals,
                    const double* uniforms, double* samples, int64_t p, double* accept_prob, double* logp, double* step_sizes, double* eps_final,
                    double* inv_metric);

/*
 * RESIDENT NUTS: the second kernel of the BPINN sampler (`ahmc_bayesian_pinn_pde` with Kernel = NUTS(delta)) — No-U-Turn
 * transitions of the chain of pinn_hmc_init, under the metric of pinn_hmc_set_metric; pinn_hmc_get reads the state afterwards.  Opt-in: pinn_hmc_*
 * and every other path are unchanged.  Multinomial NUTS with the generalised U-turn criterion in iterative form, as neuralpde.jl_amd/bpinn.py
 * `_nuts_transition` states it (the specification; Stan's additional cross-subtree checks at a merge are not part of it), D = max_depth:
 *   start       r0 = z / sqrt(minv), H0 = -logp + 1/2 sum minv r0^2; both edges and the proposal = the current state; rho = r0, logW = 0, depth = 0.
 *   doubling    while depth < D: v = +1 if u_dir[depth] < 0.5 else -1; 2^depth leaves outward from the right (v = +1) or the left edge, a leaf =
 *               one leapfrog step of signed size v eps from the moving end (r += v eps/2 g; theta += v eps minv r; evaluate; r += v eps/2 g).
 *   per leaf n  delta = H0 - H (-inf when not finite); sum_acc += min(1, exp delta); n_leaf += 1; not -delta <= delta_max: DIVERGENT, the
 *               transition ends and the subtree is discarded; logw_sub = logaddexp(logw_sub, delta); the leaf becomes the subtree's candidate if
 *               n == 0 or u_leaf[n_leaf - 1] < exp(delta - logw_sub); rho_sub += r; n even: checkpoint (r, rho_sub) at index popcount(n); n odd: for
 *               every sub-tree of 2, 4, ... leaves that ends here, rho_s = rho_sub - rho_ck + r_ck of its first leaf; turning if
 *               sum rho_s minv r_ck <= 0 or sum rho_s minv r <= 0: the transition ends and the subtree is discarded.
 *   merge       after leaf 2^depth - 1: proposal <- candidate if u_merge[depth] < exp(logw_sub - logW); logW = logaddexp(logW, logw_sub);
 *               rho += rho_sub; the edge on the subtree's side = its last leaf; depth += 1; the transition ends if
 *               sum rho minv r_left <= 0 or sum rho minv r_right <= 0, or at depth == D.
 *   result      the proposal becomes the current state.  samples (nullable): ndraws x p, row i = the state after draw i; logp[i] its logp;
 *               accept_stat[i] = sum_acc / n_leaf; tree_depth[i] = depth; n_leapfrog[i] = n_leaf; divergent[i] = 0 / 1.
 *   normals     ndraws x p STANDARD normals z (the device divides by sqrt(minv), as in pinn_hmc_warmup), or NULL;
 *   uniforms    ndraws rows of 2 D + 2^D - 1 doubles [u_dir[0..D) | u_merge[0..D) | u_leaf[0 .. 2^D - 1)], or NULL.
 *               NULL: the generator of pinn_hmc_draws with the same key: normal i = z_i, uniform k = word(P + k, 0) / 2^32.  The draw counter is the one
 *               pinn_hmc_draws advances, by one per completed draw: interleaved HMC and NUTS calls form one stream, and 2 + 3 draws equal 5.
 * The host queues SLOTS — one evaluation of the handle's resident path plus one state-machine launch (judge the leaf just evaluated, propose the
 * next) — in chunks of "nuts_chunk" (pinn_set_option, 1..64, default 8) and reads the control block, nothing else, after each chunk; slots queued
 * behind the last draw do nothing (at most nuts_chunk - 1 evaluations are spent on them).  One download at the end.  All sums have the fixed order
 * of pinn_hmc_draws' energies: a call is bit-reproducible and independent of "nuts_chunk".
 * Refused, with the handle and the chain left as they were: everything pinn_hmc_draws refuses; max_depth outside 1..10; eps or delta_max not
 * positive and finite; NULL accept_stat, logp, tree_depth, n_leapfrog or divergent.  An evaluation that fails in mid-call leaves the chain at its
 * last completed draw and the counter advanced by the completed draws.
 */
int pinn_nuts_draws(pinn_handle h, int ndraws, int max_depth, double eps, double delta_max, uint64_t seed, const double* normals,
                    const double* uniforms, double* samples, int64_t p, double* accept_stat, double* logp, int* tree_depth, int* n_leapfrog,
                    int* divergent);

/*
 * RESIDENT L-BFGS: pinn_lbfgs's iteration with the iterate x, its gradient, the trial point, the direction, the curvature
 * pairs (rings of `history` vectors) and the line search's bookkeeping in HBM in double.  Opt-in: pinn_lbfgs is unchanged.  The host queues SLOTS —
 * one state-machine launch (judge the evaluation just finished: Armijo test, accept with the curvature-pair update or halve the step; propose the
 * next point: two-loop recursion and first step, or the next trial of the running line search) followed by one full evaluation of the handle's resident
 * path (the double kernels in float64 mode; the fp32 kernels at (float)x otherwise, their K sums in double) — in chunks of "lbfgs_chunk" slots
 * (pinn_set_option, 1..64, default 8; 1 = one synchronisation per evaluation) and reads the control block, nothing else, after each chunk.
 * Same algorithm and constants as pinn_lbfgs (Armijo c1 = 1e-4, halving, 30 trials, pair kept iff s.y > 1e-10 |s| |y|, gamma = s.y / y.y, restart
 * from -g when g.d >= 0, first step min(1, 1 / |g|_2)), same order of operations; dot products are summed in a fixed parallel order, so the
 * iterates agree with pinn_lbfgs's to rounding and are bit-reproducible from run to run.  ONE difference: a rejected trial costs a full evaluation
 * here (pinn_lbfgs evaluates rejected trials loss-only and the accepted point once more with its gradient); an accepted trial is never re-evaluated.
 *   pinn_lbfgs_init   uploads theta (p doubles), fixes the term weights (NULL: ones — they cannot change later: the curvature pairs belong to one
 *                     objective), evaluates f and g once, clears the rings and the counters.  A second call replaces the state.
 *   pinn_lbfgs_steps  continues from the stored state for at most `maxiters` further iterations and at most `max_evals` further trial evaluations
 *                     (2 iterations followed by 3 are bit-equal to 5 in one call; a call that ends inside a line search is resumed there).
 *                     loss_history (nullable): objective after every iteration of this call, `maxiters` entries, padded with the last objective;
 *                     *iters_done / *evals_done: iterations / trial evaluations of this call; *status: 0 RUN or 1 RETRY (max_evals ended the call
 *                     between / inside line searches), 2 CONVERGED (max |g_i| <= gtol), 3 STALLED (30 trials without decrease: the evaluation's
 *                     noise floor), 4 MAXITER.  A terminal status ends the call, not the optimisation: the next call tests again.  Slots queued behind
 *                     a terminal one do nothing (at most lbfgs_chunk - 1 evaluations are spent on them).  At STALLED a handle in "split" GEMM mode
 *                     switches itself to "fp32" once per call, re-evaluates at x, clears the rings and goes on, and is switched back before the
 *                     call returns, as in pinn_lbfgs ($PINN_LBFGS_KEEP_GEMM=1 disables that).
 *   pinn_lbfgs_get    the current iterate: theta (p doubles), *f (nullable), grad (p doubles, nullable).
 * The state has buffers of its own: evaluations, pinn_adam_* and pinn_hmc_* between two calls leave it alone and vice versa.
 * The precision mode taken to the other value AND BACK between two calls is not a change: the iteration continues, on the point sets as the mode
 * holds them after the return (double copies converted from the float buffers).
 * Refused, with the handle left as it was: pinn_lbfgs_steps / _get before pinn_lbfgs_init; a handle whose precision mode changed since (init again);
 * a term with a device sampler; a handle on a communicator; p != ntheta; history outside 1..64; maxiters < 1; max_evals < 1.
 */
int pinn_lbfgs_init(pinn_handle h, const double* theta, int64_t p, int history, const float* term_w);
int pinn_lbfgs_steps(pinn_handle h, int maxiters, int max_evals, double gtol, double* loss_history, int* iters_done, int* evals_done, int* status);
int pinn_lbfgs_get(pinn_handle h, double* theta, int64_t p, double* f, double* grad);

/*
 * RESIDENT BFGS: the dense quasi-Newton finisher — `solve(prob, BFGS(); maxiters)` of the reference's scripts — with the
 * iterate, the P x P inverse-Hessian approximation H (double, full symmetric storage) and the line search in HBM.  Opt-in; the L-BFGS routines are
 * unchanged.  Same line search, constants, slots, chunks ("lbfgs_chunk") and statuses as the resident L-BFGS above; in place of the two-loop
 * recursion, per accepted iteration, u = H y (one read pass over H by many workgroups, one wave per row) and the rank-two update
 *     H[i][j] <- (H[i][j] - rho (s_i u_j + u_i s_j)) + c (s_i s_j),  rho = 1 / s.y,  c = rho (1 + rho y.u),
 * fused with the next direction d = -H g (one read + write pass); every product is rounded on its own, so H stays bit-symmetric.  The update is
 * skipped unless s.y > 1e-10 |s| |y|.  H starts as the identity (first step min(1, 1 / |g|_2)), is scaled to (s.y / y.y) I when the first update
 * arrives, and returns to the identity when g.d >= 0 (restart); the identity costs no pass over the matrix.  Bit-reproducible from run to run and
 * independent of "lbfgs_chunk".  A rejected trial costs a full evaluation; an accepted trial is never re-evaluated.
 *   pinn_bfgs_init    uploads theta (p doubles), fixes the term weights (NULL: ones), evaluates f and g once, H = I.  A second call replaces the state.
 *   pinn_bfgs_steps   as pinn_lbfgs_steps, argument by argument: at most `maxiters` further iterations and `max_evals` further trial evaluations from
 *                     the stored state; loss_history padded with the last objective; *status 0 RUN, 1 RETRY, 2 CONVERGED, 3 STALLED, 4 MAXITER.  A
 *                     terminal status ends the call, not the optimisation.  At STALLED a handle in "split" GEMM mode switches itself to "fp32" once
 *                     per call, re-evaluates at x, resets H to the identity and goes on, and is switched back before the call returns
 *                     ($PINN_LBFGS_KEEP_GEMM=1 disables that).
 *   pinn_bfgs_get     the current iterate: theta (p doubles), *f (nullable), grad (p doubles, nullable), hinv (p x p doubles row-major, nullable):
 *                     the inverse-Hessian approximation as it stands — at an optimum the covariance of a Laplace approximation.
 * The state has buffers of its own: evaluations, pinn_adam_*, pinn_lbfgs_* and pinn_hmc_* between two calls leave it alone and vice versa.
 * Refused, with the handle left as it was: pinn_bfgs_steps / _get before pinn_bfgs_init; a handle whose precision mode changed since (init again);
 * a term with a device sampler; a handle on a communicator; p != ntheta; maxiters < 1; max_evals < 1; p above 32768 (the matrix is 8 p^2 bytes:
 * 8 GiB there; $PINN_BFGS_MAX_P lowers the cap) or a matrix the device cannot allocate — the message names P and the bytes.
 */
int pinn_bfgs_init(pinn_handle h, const double* theta, int64_t p, const float* term_w);
int pinn_bfgs_steps(pinn_handle h, int maxiters, int max_evals, double gtol, double* loss_history, int* iters_done, int* evals_done, int* status);
int pinn_bfgs_get(pinn_handle h, double* theta, int64_t p, double* f, double* grad, double* hinv);

/*
 * ADAPTIVE CUBATURE: the reference's QuadratureTraining contract — a term's loss is (1 / area) int r^2 dx, integrated
 * adaptively to reltol / abstol (src/training_strategies.jl:396-481) — as an h-adaptive refinement resident on the device.  Opt-in; nothing else
 * changes.  At the given theta (p doubles; narrowed to float on an fp32 handle) the box [lb, ub] (d doubles each; a coordinate with lb == ub is
 * held fixed at that value, 1..4 coordinates are free) is covered by a list of axis-aligned boxes.  Every new box is evaluated with the
 * Genz-Malik degree-7 rule and its embedded degree-5 rule through the term's own residual kernel (7 / 17 / 33 / 57 nodes for 1..4 free axes):
 * I7 and I5 as fractions of the mean, err = |I7 - I5|.  Per round I = sum I7, E = sum err, tau = max(abstol, reltol |I|); the refinement ends when
 * E <= tau, otherwise every box with err > tau vol(box) / vol(domain) is bisected along its axis of largest fourth difference, all in one batch.
 *   *status  0 converged; 1 the next split would exceed max_regions (the mesh before that split is kept); 2 max_rounds splits were made; 3 I or E is not finite
 *            (a NaN / Inf residual at this theta: the mesh as it stands is emitted, nothing was compared).
 *   *integral, *error  I and E of the last round; *nregions the boxes; *rounds the splits made; every output pointer is nullable.
 * In every case the call then installs, as the term's point set, the tensor Gauss-Legendre rule with `nodes` (1..8) nodes per free axis on every
 * box of the final mesh (*npoints = nregions x nodes^free points, box after box, the first free axis fastest) with per-point weights
 * w = vol(box) / vol(domain) x the rule's weights (they sum to 1): exactly the state pinn_set_points[_f64](n_norm = npoints) followed by
 * pinn_set_point_weights(float(w)) leaves.  Every evaluation, optimiser and pinn_term_grads then works on that set unchanged; its gradient is that of
 * the emitted quadrature value on the mesh frozen at this theta.  Region list, nodes, estimates, decisions and the emitted set stay on the device;
 * the host reads one 40-byte record per round.  While the call runs the term's point buffer holds the rule's nodes: after a call that fails
 * half-way (a device allocation) install a point set before the next evaluation.
 * With pinn_set_timing level 2, pinn_get_option(h, "cub_ms") = six times in ms of the last call, from HIP events at the phase boundaries, summed
 * over its rounds: node generation (+ the installed node set's bookkeeping), evaluation, estimate, plan + read-back, split, emit.
 *   pinn_cubature_get  the final mesh of the term's last refinement: boxes [nregions][2][d] (lo, then hi; fixed coordinates repeat their value) and
 *                      est [nregions][2] (I7, err of each box); either may be NULL.  The list stays until the next refinement of the term.
 * Refused, with the handle left as it was: a term with a device sampler; integral terms; terms with per-point data channels; terms behind a periodic
 * embedding; the stencil derivative mode; a handle on a communicator; lb > ub; d != the term's coordinates; zero free axes (more than 4 cannot occur: a term has at most 4 coordinates); nodes
 * outside 1..8; a negative tolerance; max_regions < 1; max_rounds < 0; max_regions x points per box beyond 32-bit indexing; p != ntheta;
 * pinn_cubature_get before a refinement of the term, or with another nregions.
 */
int pinn_cubature_refine(pinn_handle h, int term, const double* theta, int64_t p, const double* lb, const double* ub, int d, double reltol, double abstol,
                         int max_regions, int max_rounds, int nodes, double* integral, double* error, int64_t* nregions, int64_t* npoints, int* rounds,
                         int* status);
int pinn_cubature_get(pinn_handle h, int term, double* boxes, double* est, int64_t nregions);

/*
 * ENSEMBLE PREDICTION: the trial function of network `net` at `nsamples` parameter vectors and n points, and the mean and
 * standard deviation over the samples at every point, in one call — the prediction stage of a Bayesian PINN (ext/bpinn/PDE_BPINN.jl:254-302),
 * deep-ensemble or checkpoint prediction.  Opt-in: pinn_phi / pinn_phi_f64 are unchanged.
 *   thetas  [nsamples][p] FULL parameter vectors (p == ntheta; the engine takes the network's own slice, as pinn_phi does)
 *   pts     [n][d] point-major, d = the network's inputs (as pinn_phi_f64)
 *   mean[i] = (sum_s phi(x_i; theta_s)) / nsamples,  std[i] = sqrt(sum_s (phi(x_i; theta_s) - mean[i])^2 / (nsamples - ddof)),  ddof = 0 | 1:
 *           both sums in double in the fixed order s = 0 .. nsamples-1 (numpy.mean / numpy.std(ddof)); bit-reproducible
 *   preds   nullable: [nsamples][n], every prediction
 * The compute type follows the handle: double on a handle in float64 mode; otherwise the float kernel at (float)theta, (float)x, its
 * predictions widened — the statistics are in double either way.  One upload of thetas, one of pts, one launch per (samples x point blocks)
 * + one for the statistics with no synchronisation in between, one download.  Predictions beyond a device-memory budget ($PINN_ENS_GB,
 * default 4; $PINN_ENS_CHUNK = points per pass overrides it) are produced in passes over POINTS; the results do not depend on the passes.
 * Refused, with the handle left as it was: net out of range; p != ntheta; nsamples < 1; ddof not 0 or 1; nsamples - ddof < 1; n < 1; a DGM
 * network; a network behind a periodic input embedding; more than 16 Dense layers; a layer so wide that two activation images of 64 points
 * exceed the 160 KB of LDS (wider than 160 neurons in float64 mode, 320 otherwise) — the message names the sizes.
 */
int pinn_phi_ensemble(pinn_handle h, int net, const double* thetas, int64_t nsamples, int64_t p, const double* pts, int64_t n, int ddof,
                      double* mean, double* std, double* preds);

/*
 * ENSEMBLE DERIVATIVES: posterior mean and standard deviation of derivatives of the trial function — a flux -k du/dx, a
 * velocity from a stream function, the u_xx of a residual — over the same samples and points, in one call instead of one pinn_derivative[_f64]
 * call per sample.  thetas, p, pts, n, ddof: exactly as pinn_phi_ensemble, which is unchanged.
 *   orders  [nder], axes [nder][4]: request j is the derivative of order orders[j] (0 .. 4) along axes[4j .. 4j + orders[j]) — the multi-index
 *           grammar of pinn_derivative.  Order 0 is phi itself, order 2 may be mixed, orders 3 and 4 run along one axis.  1 <= nder <= 32.
 *   mean, std  [nder][n]: the statistics of pinn_phi_ensemble per request (double sums in the fixed order s = 0 .. nsamples-1)
 *   preds   nullable: [nder][nsamples][n]
 * The requests are grouped into jet passes so that no network forward runs more often than needed: every mixed (a, b) takes a two-axis pass
 * (u, d_a u, d_b u, d_a d_b u) that also serves the first derivatives along a or b; the remaining pure requests along one axis share a line
 * jet u, d_a u, .., d_a^K u, K the highest order left on that axis; the value rides in the first pass (a table of order 0 alone takes
 * pinn_phi_ensemble's kernel).  One result does not depend on what else is in the table (bit for bit), and the order-0 request equals
 * pinn_phi_ensemble bit for bit.  pinn_get_option(h, "ens_passes") = the jet passes of the last call ("ens_point_passes": its passes over
 * points; "ens_scratch_passes": its jet passes whose images lived in device scratch).
 * The compute type follows the handle as in pinn_phi_ensemble.  One upload of thetas, one of pts (the request table travels in the launch
 * arguments), the launches back to back on the handle's stream, one download of mean | std and one of preds when asked for.  The budget
 * $PINN_ENS_GB counts nder prediction slabs; $PINN_ENS_CHUNK as in pinn_phi_ensemble.  A jet multiplies the activation images by its channel
 * count (2 .. 5): a pass keeps them in LDS while four workgroups fit a CU (40 KB each); beyond that — and always where two images of 64
 * points exceed the 160 KB of LDS — they live in a device scratch buffer of 8 (double) / 16 (float) workgroups per CU instead: same
 * arithmetic, same bits.  $PINN_ENS_NO_LDS (read per call) = 1 forces that storage, = 0 the LDS wherever two images of 64 points fit;
 * $PINN_ENS_SCRATCH_WGS = workgroups per CU of the scratch storage (1 .. 64; A/B).
 * Refused, with the handle left as it was: everything pinn_phi_ensemble refuses (its LDS limit only for a table of order 0 alone); nder outside
 * 1..32; an order outside 0..4; an axis outside the network's inputs; a mixed request of order >= 3; a table that repeats a request (the axes of
 * a mixed request in either order are one request); a scratch buffer beyond $PINN_ENS_GB — the message names the sizes.
 */
int pinn_derivative_ensemble(pinn_handle h, int net, const double* thetas, int64_t nsamples, int64_t p, const double* pts, int64_t n,
                             int nder, const int* orders, const int* axes, int ddof, double* mean, double* std, double* preds);

/*
 * Run-time options of a handle. "gemm" = arithmetic of the hidden-layer GEMMs of the 64- / 128-wide (neuron-split) kernels:
 *   "split" (default) — every fp32 product rebuilt from three bf16 pieces per operand on the bf16 matrix pipe (6 MFMAs, fp32 accumulation):
 *                       2-4 x the rounding error of an fp32 fmaf chain, ~1.35 x faster (error budget: DESIGN.md section 6);
 *   "fp32"            — v_mfma_f32_16x16x4_f32: bit-for-bit an fmaf chain per product, for callers that need the last bit (a quasi-Newton
 *                       finisher at its noise floor: the reference's `solve(prob, BFGS())` stage, test/NNPDE1/nnpde__pde_iii_3rd_order_ode.jl:89-93,
 *                       runs on Float64 CPU arithmetic there).
 *   "auto" (r06)      — the engine chooses between the two by MEASUREMENT: at the current parameters the gradient is evaluated with both arithmetics,
 *                       delta = |grad(split) - grad(fp32)|_2 / |grad(fp32)|_2  (the split products' arithmetic error at this iterate); "split" runs
 *                       while delta <= 1e-5 (the north star's tolerance), "fp32" above, back under 3e-6.  ~2e-7 at initialisation, 1e-5 / 4e-3 at the
 *                       trained fixtures (cfg2 after 2,000 / 6,000 Adam steps).  Checked at the end of a pinn_adam_steps call (loop path) and inside
 *                       pinn_loss_grad with a gradient, at most once per 1,000 optimiser steps / evaluations (two evaluations + at most two re-plans
 *                       per check), never inside a resident loop.  pinn_get_option(h, "gemm") reports "auto(split)" / "auto(fp32)",
 *                       "gemm_delta" the last delta, "grad_health" rho = |grad|_2 / sqrt(sum_k w_k L_k) of the last measured evaluation: rho against
 *                       its value at initialisation is the cancellation factor of the gradient sum — once it has fallen by ~1e3 no fp32 evaluation holds
 *                       1e-3 any more and "precision" = "f64" is the remedy (the glue's precision policy puts Float64 parameters there from the start).
 * Both kernel sets are in the library; switching rebuilds the handle's kernel plan in place (milliseconds) and keeps point sets, samplers,
 * per-point data / weights and the optimiser state.  Narrower nets (one-wave-per-tile kernels) and DGM nets compute on fp32 MFMAs / the
 * VALU in either mode.  $PINN_GEMM = split | fp32 sets the mode new handles start in.  pinn_get_option writes the current value.
 * "precision" = "f32" (default) | "f64": the FLOAT64 evaluation mode — the reference's default eltype (src/discretize.jl:432-449).  With
 *   "f64", pinn_loss_grad_f64 evaluates natively in double (pinn_loss_grad converts at the boundary) and pinn_lbfgs iterates on the double
 *   objective: what a quasi-Newton stage needs to take an objective below ~1e-7 (test/NNPDE1/nnpde__pde_iii_3rd_order_ode.jl:89-93) and
 *   what parity at TRAINED parameters needs (fp32 cannot hold 1e-5 there).  Kernels: wave-private tiles on
 *   v_mfma_f64_16x16x4_f64 (csrc/pinn_kernels5.hpp) for tanh / sigmoid nets with hidden layers up to 64 wide and the instantiated jet sets,
 *   one lane per point on the fp64 VALU (csrc/pinn_kernels4.hpp) for everything else the mode covers; pinn_get_option(h, "f64_path") reports
 *   what the last evaluation ran ("mfma" | "lanes" | "mfma+lanes").  7-8x the time of the fp32 kernels on the matrix pipe.
 *   Covers equations of up to 6 dependent variables (same argument count), Dense chains with tanh / sigmoid / sin / swish (sin, swish: one lane per point), derivative orders <= 2
 *   in 1-3 inputs (1-D, and mixed / pure in 2-D and 3-D where instantiated: <= 4; 4-D: first and pure second), PDE parameters, quadrature
 *   weights, per-point DATA channels, device samplers, periodic input embeddings (r06); anything else (DGM) fails HERE with a message and leaves the fp32
 *   plan usable.  In this mode EVERY evaluating entry point runs the double kernels (r06): pinn_loss_grad / pinn_loss_grad_device /
 *   pinn_loss_device / pinn_term_grads / pinn_loglik_grad / pinn_residual / pinn_phi / pinn_derivative convert at the boundary, their _f64
 *   twins hand everything over in double; pinn_adam_init / _steps / _get / _apply keep theta and the moments in double on the device, in
 *   a buffer of their own (evaluations between two pinn_adam_steps calls — adaptive reweighting, callbacks — leave the iterate alone);
 *   samplers redraw in float and the double copy follows.  pinn_set_points_f64 / pinn_set_point_data_f64 install a point set / its
 *   observations in double (the fp32 kernels get the float conversion).  Communicators (r06): pinn_loss_grad_sharded_device_f64 /
 *   pinn_loss_grad_sharded_f64 and the resident loops (pinn_adam_steps over a one-process-per-GPU communicator, pinn_adam_steps_sharded) all-reduce
 *   [P + K] DOUBLES; the float entry points pinn_loss_grad_sharded(_device) run the fp32 kernels whatever the mode.
 *   Small problems (r06: the reference's own regime, a few hundred points per term): row-tile counts of 1 / 2 for 16- / 32-wide nets, and the terms
 *   that share an input binding and an instantiated jet set are evaluated by ONE launch sequence (<= 6 members, <= 8,192 points together) —
 *   same results to rounding; pinn_get_option(h, "f64_merged") = the number of such sequences in the last evaluation, $PINN_F64_NO_MERGE=1
 *   switches them off (A/B, tests).  Terms whose residual is affine in the trial function(s) with constant coefficients (boundary conditions, linear
 *   PDEs with forcing terms) skip the tape interpreter in the tile kernel: the coordinate-only part is evaluated once per point set
 *   (pinn_get_option(h, "f64_affine") = the number of such terms; $PINN_F64_NO_LIN=1: off).  The weight-gradient kernel of a small launch works on
 *   short point blocks (64 ... 256 instead of 512 points per workgroup row, chosen so that the launch has ~512 workgroups; $PINN_F64_NO_SHORT_BLOCKS=1: off).
 *   PRECISION POLICY of the glue (Julia: HIPStrategy / hip_discretize `precision = :auto`; Python mirror: PhysicsInformedNN(precision = "auto")):
 *   the reference's contract compute dtype = eltype(theta) (src/eltype_matching.jl:8-10) — Float64 parameters select "f64", Float32
 *   parameters "f32"; "f32" on Float64 parameters is the explicit fast opt-in.
 * "derivative" = "exact" (default) | "stencil" (r06; float64 mode only): a VALIDATION mode, not a performance path.  "stencil" evaluates every
 *   derivative slot as the reference's central differences — numeric_derivative (src/pinn_types.jl:445-482: the order-1..4 formulas, the
 *   recursion for mixed derivatives and orders > 4) with the steps of get_eps (src/symbolic_utilities.jl:98-103: eps(Float64)^(1/(2+order)),
 *   the TOTAL order's step on every axis, :185), in the reference's order of operations — as value-only forward passes at shifted copies of the
 *   point set, the difference formulas as tape ops, and a reverse sweep through the same combination (one seeded launch per shifted set;
 *   csrc/f64_stencil.cpp: f64_stencil_term).  pinn_loss_grad*, pinn_term_grads*, pinn_loglik_grad*, pinn_residual* then return the reference's
 *   finite-difference numbers instead of exact derivatives: for digit-by-digit comparisons with the reference's generated loss functions
 *   (julia: NeuralPDEHIP.selftest) and with the stencil oracle.  How close two correct implementations of these formulas can be is bounded by the
 *   formulas themselves: u(x +- eps) carries ~1e-16 relative rounding and 1 / eps^2 ~ 7e7 multiplies it — 1e-8 at initialisation, 1e-5 ... 1e-4
 *   of the gradient at trained parameters (tests/test_f64_mode.py measures it as the stencil oracle against itself with permuted neurons).
 * "integral_nodes" = "2" ... "64" (default "16"): Gauss-Legendre nodes per integral node of the handle's integral terms (fp32 kernels only:
 *   "precision" = "f64" is refused on a handle with integral terms, and the refusal names "f32").  Setting it on a live handle RE-PLANS the
 *   integral terms: their installed point sets, samplers and the optimiser state stay, the site sets (every point plus Q abscissae per
 *   integral node) are rebuilt for the new rule; site buffers that have room are kept, larger ones are allocated BEFORE anything changes.  A value
 *   outside the range, one whose site set exceeds 32-bit indexing, or a failed site-buffer allocation is refused and the handle stays as it was
 *   (a failure later, in the per-term jet buffers, reports the error and leaves the handle to be destroyed).  pinn_describe marks the launch groups of such terms `+integral(Q)`.
 * "persistent" = "on" (default) | "off": pinn_adam_steps runs a SMALL problem — one network of the one-wave-per-tile kernel family, at most
 *   32 workgroups (~2,000 points of a 3 x 32 net), fixed or device-redrawn point sets (pinn_set_sampler), no estimated PDE parameters, no communicator — as ONE persistent launch
 *   per call (csrc/pinn_train.hpp: evaluation, fixed-order reduction, Adam and the weight-image update of every iteration inside the kernel,
 *   two grid barriers per iteration) instead of three launches per iteration: the reference's own test regime,
 *   solve(prob, Adam; maxiters = 4000) on 100-1,000 points (test/NNPDE1/nnpde__pde_ii_2d_poisson.jl:83-85).  Bit-identical to the loop.
 *   A launch whose workgroups are not all resident (a device shared with another process) ends by its barrier's time-out: the call then
 *   restores the optimiser state, runs the loop instead and keeps the loop for the handle.  $PINN_PERSISTENT=0 switches it off for every handle.  pinn_get_option(h, "adam_path") reports what the last pinn_adam_steps call ran:
 *   "persistent" | "loop" | "none".  The host-entry evaluations of such a problem (pinn_loss_grad with a gradient, the objective calls of
 *   pinn_lbfgs) take the same kernel in its evaluation-only form — residual kernel, grid barrier and fixed-order sums in ONE launch instead of
 *   two, same numbers — unless HIP events were requested (pinn_set_timing); pinn_get_option(h, "eval_path"): "one launch" | "stand-alone kernels".
 */
int pinn_set_points_f64(pinn_handle h, int term, const double* pts, int64_t n, int64_t n_norm);
int pinn_set_option(pinn_handle h, const char* name, const char* value);
int pinn_get_option(pinn_handle h, const char* name, char* buf, int64_t buflen);

/* Timing of the last pinn_loss_grad*: HIP-event milliseconds of the fused residual kernels / of the whole device section. */
int pinn_last_timing(pinn_handle h, float* kernel_ms, float* total_ms);
/* How many HIP events an evaluation records: level 0 (default) none, 1 a start/stop pair around launch group `group` (-1: every
 * group), 2 additionally the phase events behind pinn_last_timing.  Every recorded event costs a few us of dispatch gap between
 * kernels — 25 us per pinn_loss_grad call at level 2, measured on the reference's 1-D Poisson test (profiles/r04_train_kernel.txt) —
 * so events are opt-in (the default changed from level 2 to level 0 in r04: callers of pinn_last_timing must call pinn_set_timing(h, 2, -1)
 * first): with the events off pinn_last_timing FAILS (non-zero return, pinn_last_error says how to switch them on) and
 * pinn_group_timing reports ms = -1. */
int pinn_set_timing(pinn_handle h, int level, int group);
/* Kernel plan: number of launch groups (terms that share one fused kernel) and the HIP-event duration of group g's
 * fused residual kernel in the last evaluation (-1 if that group was not timed, see pinn_set_timing), with the
 * points / jet channels / wave tiles it processed. */
int pinn_num_groups(pinn_handle h);
int pinn_group_timing(pinn_handle h, int group, float* ms, int64_t* points, int* channels, int* tiles);
/* Launch group whose launch carried group g's tiles in the last evaluation: g itself, or the head group of a MERGED launch (two
 * kernel-family members of one network — e.g. the interior jet set and the value-only boundary set — walked by one persistent
 * kernel; the head's pinn_group_timing then covers both).  -1: not launched yet / bad index. */
int pinn_group_launched_by(pinn_handle h, int group);
/* Introspection used by tests and bench: writes a short human-readable description of the kernel plan. */
int pinn_describe(pinn_handle h, char* buf, int64_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* PINN_HIP_H */
