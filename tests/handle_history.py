"""Seeded generator and runner of OPERATION SEQUENCES on one long-lived engine handle, for tests/test_handle_history.py: the handle's
grow-only buffers, validity counters, packed weight images, float64 state, re-plans and resident optimiser / sampler states (csrc/engine_types.hpp)
are driven through histories nobody wrote by hand, and what the reused handle then computes is read next to a FRESH handle brought straight to the
same state.  Deterministic in (problem, seed) through numpy.random.default_rng; this module generates and runs, it asserts nothing.

    run(npde, problem_name, seed) -> Record(problem, seed, ops, checkpoints, resumed, final, sizes, paths)
        ops          every generated operation: kind, detail, and for an expected refusal the message wanted and what came
        checkpoints  one inside the sequence and one at its end: the observables of the reused and of a fresh handle (observe())
        resumed      a resumable state continued: what the reused handle returned and what k1 + k2 in one go on a fresh handle returned
        final        the model state at the end (drawn sets read back) and the reused handle's observables, for the oracle
        sizes        per term, every point-set size it went through; paths: what eval_path / adam_path / f64_path reported

Problems (the smallest shape of each code path):
    poisson16  2 x 16 tanh Poisson                      family 1, boundary terms riding, one-launch evaluation, persistent Adam kernel
    poisson64  2 x 64 tanh Poisson                      family 2, merged launch, both GEMM arithmetics
    system16   the nonlinear two-network system of test_coupled_system_of_pdes, 2 x 16, nu estimated     forward / k_expr / reverse launches
    system64   the same at 2 x 64                                                                        fused tail launch
    inverse    heat equation with an estimated diffusivity and a data-misfit term (OP_DATA, set_point_data)
    heat       the periodic-embedding heat problem (d_upts)
    integral   the integro-differential equation of test_integral_terms ("ide"), 2 x 16               site sets, integral_nodes re-plans
    dgm        Burgers through the Deep Galerkin family
Point-set sizes come from LADDER: the edges of a wave, of the 16-point float64 tile, of the "more than 64 boundary points" rule and of the
256-point coupled block.

OPERATION CLASSES
    state        the model of the handle's state changes; the fresh handle gets only the final value
                 points (set_points / set_points_f64, n_norm), data (set_point_data[_f64]), pweights (set_point_weights), option (precision /
                 gemm / persistent / derivative / integral_nodes), sampler (set_sampler kind 1-3, and kind 0, which keeps the drawn set)
    traceless    must leave nothing behind
                 eval (loss_grad with / without gradient, term_grads, loglik_grad, residual, the _f64 twins, at another theta), net (phi /
                 derivative / phi_ensemble at ladder sizes), adam (init + steps), lbfgs (pinn_lbfgs), rlbfgs (lbfgs_init + lbfgs_steps), hmc
                 (hmc_init + hmc_draws), sampler_detour (set_sampler, Adam steps, kind 0, reinstall), timing (set_timing 2 / 1, an evaluation,
                 back to 0), option_detour (A -> B -> A with an evaluation in between), points_detour (other ladder sizes and back)
    resumable    begin_adam / begin_rlbfgs / begin_hmc put a resident state and run k1 steps; resume_* runs k2 more after whatever came in between

CONTRACT TABLE (include/pinn_hip.h; "continue" = k1 + k2 on the reused handle is bit-equal to k1 + k2 in one call on a fresh handle)
    in between                      adam (pinn_adam_steps)                      rlbfgs (pinn_lbfgs_steps)         hmc (pinn_hmc_draws)
    traceless operations            continue                                    continue                          continue
    precision f32 -> f64            refused: "call pinn_adam_init first"        refused: "precision changed"      refused: "precision changed"
    precision f64 -> f32            (not generated: the fp32 state is separate) refused: "precision changed"      refused: "precision changed"
    precision there and back        fp32 state: continue; f64 state: refused    continue (fp32) / see DESIGN 6.5  continue (fp32) / see DESIGN 6.5
                                    ("call pinn_adam_init first": the double
                                    state went with the mode)
    a device sampler installed      accepted, on the redrawn sets (k2 finite     refused: "redraws its points"     refused: "redraws its points"
                                    losses; another objective: not compared)
    points / data / weights change, gemm / derivative / integral_nodes set to another value
                                    (not generated: another objective or arithmetic; the generator drops the state)
    persistent on / off             continue (the persistent kernel and the loop are bit-identical)
Not cells of their own: "the fp32 Adam state survives a visit to f64" is met only where an option_detour of the precision falls between begin_adam
and resume_adam on an fp32 handle (a traceless operation of the first row); Adam begun in f64 and resumed in f32 is not generated — which fp32 state
exists then depends on earlier runs — and the generator runs a plain evaluation (logged "eval") in its place.
Other refusals the generator provokes on purpose, each with the handle left as it was: precision f64 on a handle with integral terms or a
DGM network, derivative = stencil outside the float64 mode or behind a periodic embedding, pinn_lbfgs / lbfgs_init / hmc_init with a device
sampler installed, per-point data or weights for a sampled term, an evaluation of a data term whose set was replaced without its data,
phi_ensemble on a DGM or periodically embedded network."""
import copy
from collections import namedtuple

import numpy as np
import sympy as sp
import torch

import helpers
import pinn_oracle as po

LADDER = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 700)
LADDER_W = np.array([3, 2, 2, 2, 2, 3, 3, 1.5, 1.5, 1.5, 0.6])
LADDER_W2 = np.array([3, 2, 2, 2, 2, 3, 3, 0.3, 0.3, 0.3, 0.1])          # 64-wide networks: the emulation's cost is in the large sets
PROBLEMS = ("poisson16", "poisson64", "system16", "system64", "inverse", "heat", "integral", "dgm")
FAMILIES = {"family 1": ("poisson16", "system16", "inverse", "heat", "integral"), "family 2": ("poisson64", "system64"), "family 3": ("dgm",)}      # kernel families
WALKS = ((257, 1, 256), (1, 65, 64, 257))       # point-set detours: both 64 / 256 edges in both directions, n = 1, a set larger than any before after a shrink
N_MASTER = 700
N_PROBE = 33
SEQ_LEN = 10                    # generated operations per sequence (the installation of the first sets not counted)

STATE_KINDS = ("points", "data", "pweights", "option", "sampler")
TRACELESS_KINDS = ("eval", "net", "adam", "lbfgs", "rlbfgs", "hmc", "sampler_detour", "timing", "option_detour", "points_detour")
RESUMABLE_KINDS = ("begin_adam", "begin_rlbfgs", "begin_hmc", "resume_adam", "resume_rlbfgs", "resume_hmc")

Record = namedtuple("Record", "problem seed ops checkpoints resumed final sizes paths")
Problem = namedtuple("Problem", "name index descriptor K P theta dims master ndata net_d resid lb ub f64_ok stencil_ok ens_ok integral embedded ne family2")

_PROBLEMS = {}


# ------------------------------------------------------------------------------------------------------------------------------------------
# problems
# ------------------------------------------------------------------------------------------------------------------------------------------
def _system(npde, width):
    x, y = npde.parameters("x y")
    u1, u2 = npde.variables("u1 u2")
    (nu,) = npde.parameters("nu")
    Dx, Dy = npde.Differential(x), npde.Differential(y)
    Dxx, Dyy = Dx ** 2, Dy ** 2
    eqs = [npde.Eq(u1(x, y) * Dx(u1(x, y)) + u2(x, y) * Dy(u1(x, y)), nu * (Dxx(u1(x, y)) + Dyy(u1(x, y)))),
           npde.Eq(Dx(u1(x, y)) + Dy(u2(x, y)), sp.sin(sp.pi * x) * u2(x, y))]
    bcs = [npde.Eq(u1(x, 1), 1.0), npde.Eq(u2(0, y), 0.0), npde.Eq(u1(0, y), 0.0)]
    dom = [npde.In(x, npde.Interval(0.0, 1.0)), npde.In(y, npde.Interval(0.0, 1.0))]
    sysm = npde.PDESystem(eqs, bcs, dom, [x, y], [u1(x, y), u2(x, y)], ps=[nu], defaults={nu: 0.05})
    chains = [npde.Chain(npde.Dense(2, width, "tanh"), npde.Dense(width, width, "tanh"), npde.Dense(width, 1)) for _ in range(2)]
    return sysm, chains


def _inverse(npde):
    t, x = npde.parameters("t x")
    (u,) = npde.variables("u")
    (k,) = npde.parameters("k")
    Dt, Dxx = npde.Differential(t), npde.Differential(x) ** 2
    eq = npde.Eq(Dt(u(t, x)), k * Dxx(u(t, x)))
    bcs = [npde.Eq(u(0, x), sp.sin(sp.pi * x)), npde.Eq(u(t, 0), 0.0), npde.Eq(u(t, 1), 0.0)]
    dom = [npde.In(t, npde.Interval(0.0, 1.0)), npde.In(x, npde.Interval(0.0, 1.0))]
    sysm = npde.PDESystem([eq], bcs, dom, [t, x], [u(t, x)], ps=[k], defaults={k: 0.7})
    chain = npde.Chain(npde.Dense(2, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    return sysm, [chain]


def _data_values(pts, variant):
    """observations of the data-misfit term on a point set (any smooth function plus seeded noise; variant: another draw of the noise)"""
    rng = np.random.default_rng([5, int(variant), pts.shape[1]])
    return (np.exp(-pts[0]) * np.sin(np.pi * pts[1]) + 0.01 * rng.standard_normal(pts.shape[1])).reshape(1, -1)


def _theta(chains, index):
    return np.concatenate([po.glorot_theta(po.Chain(tuple(c.sizes), c.act), np.random.default_rng([17, index, i])) for i, c in enumerate(chains)])


def problem(npde, name):
    """the problem `name` on the current default library: descriptor, parameters, master point sets and the float64 residuals of its terms"""
    key = (npde._lib.default_library().backend, name)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    import test_emu_parity as tp
    index = PROBLEMS.index(name)
    param_estim, data_loss, Q, case = False, [], None, None
    if name in ("poisson16", "poisson64"):
        sysm, chain = tp.poisson2d(npde, "tanh", 16 if name == "poisson16" else 64, 2)
        chains = [chain]
    elif name in ("system16", "system64"):
        sysm, chains = _system(npde, 16 if name == "system16" else 64)
        param_estim = True
    elif name == "inverse":
        sysm, chains = _inverse(npde)
        param_estim = True
        xd = np.random.default_rng(9).uniform(0.05, 0.95, size=(2, 24))
        data_loss = [npde.DataLoss(sysm.dvs[0], xd, _data_values(xd, 0).reshape(-1))]
    elif name == "heat":
        sysm, chain = tp.periodic_heat(npde)
        chains = [chain]
    elif name == "integral":
        import test_integral_terms as ti
        case = ti.CASES["ide"](npde)
        sysm, chains, Q = case.sysm, [ti.make_chain(npde, case.d, "w16")], 16
    elif name == "dgm":
        import test_dgm as td
        sysm, chains = td._burgers(npde), [npde.DGM(2, 1, 8, 2, "tanh", "tanh", "identity")]
    else:
        raise ValueError(name)
    theta = _theta(chains, index)
    strat = npde.QuasiRandomTraining(37, bcs_points=19, sampling_alg=npde.SobolSample(seed=3), resampling=False, minibatch=1)
    kw = dict(integral_nodes=Q) if Q else {}
    disc = npde.PhysicsInformedNN(chains if len(chains) > 1 else chains[0], strat, init_params=theta, param_estim=param_estim, precision="f32",
                                  data_loss=data_loss, **kw)
    rep = npde.symbolic_discretize(sysm, disc)
    eng = rep.engine
    small = list(rep.pde_train_sets) + list(rep.bcs_train_sets) + [np.asarray(dl.points, dtype=np.float64) for dl in data_loss]
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    rng = np.random.default_rng([3, index])
    master, lb, ub = [], [], []
    for s in small:                                               # constant rows (the face of a boundary term) stay; the others are redrawn
        lo, hi = s.min(axis=1), s.max(axis=1)
        m = lo[:, None] + (hi - lo)[:, None] * rng.uniform(size=(s.shape[0], N_MASTER))
        master.append(np.ascontiguousarray(m.astype(np.float32).astype(np.float64)))       # float32 numbers: every entry point holds them exactly
        lb.append(lo.astype(np.float32))
        ub.append(np.where(hi > lo, hi, lo + 1e-3).astype(np.float32))
    ochains = [po.Chain(tuple(c.sizes), c.act, tuple(getattr(c, "embed", ()))) for c in chains]
    resid = []
    if case is not None:
        nnet = ochains[0].nparams
        for fn in case.resid:
            resid.append(lambda cord, t_, data, q, fn=fn: fn(ochains[0], t_[:nnet], torch.tensor(case.p0, dtype=po.DT), cord, q).reshape(-1))
    else:
        prob = helpers.oracle_problem(npde, sysm, chains, param_estim=param_estim)
        for term in list(prob.pde_terms) + list(prob.bc_terms):
            fn = po.build_residual(prob, term, mode="exact")
            resid.append(lambda cord, t_, data, q, fn=fn: fn(cord, t_).reshape(-1))
        for _ in data_loss:
            nnet = ochains[0].nparams
            resid.append(lambda cord, t_, data, q: ochains[0](cord, t_[:nnet])[0].reshape(-1) - data.reshape(-1))
    K = eng.K
    assert len(resid) == K == len(master)
    ndata = [0] * (K - len(data_loss)) + [1] * len(data_loss)
    dgm, emb = name == "dgm", name == "heat"
    P = Problem(name=name, index=index, descriptor=eng.descriptor, K=K, P=eng.P, theta=th, dims=[m.shape[0] for m in master], master=master, ndata=ndata,
                net_d=[c.n_inputs if hasattr(c, "n_inputs") else c.sizes[0] for c in chains], resid=resid, lb=lb, ub=ub,
                f64_ok=not (dgm or case is not None), stencil_ok=not (dgm or case is not None or emb), ens_ok=not (dgm or emb),
                integral=case is not None, embedded=emb, ne=int(eng.P - sum(oc.nparams for oc in ochains)), family2=name in ("poisson64", "system64"))
    _PROBLEMS[key] = P
    return P


def oracle(P, S, theta, weights):
    """float64, exact derivatives: the K term losses, the gradient of sum_k w_k loss_k and every term's residuals, of the state S (the sets, n_norm,
    observations, quadrature weights and rule it holds)"""
    th = torch.tensor(np.asarray(theta, dtype=np.float64), dtype=po.DT, requires_grad=True)
    losses, rs = [], []
    for k, t in enumerate(S["terms"]):
        cord = torch.tensor(np.asarray(t["pts"], dtype=np.float64), dtype=po.DT)
        data = torch.tensor(np.asarray(t["data"], dtype=np.float64), dtype=po.DT) if t["data"] is not None else None
        with torch.enable_grad():
            r = P.resid[k](cord, th, data, S["Q"])
        if t["pw"] is not None:
            q = np.sqrt(np.asarray(t["pw"], dtype=np.float32).astype(np.float64) * t["n_norm"]).astype(np.float32).astype(np.float64)
            losses.append(torch.sum(torch.tensor(q * q / t["n_norm"], dtype=po.DT) * r * r))       # (what pinn_set_point_weights stores: float sqrt(n_norm w_i))
        else:
            losses.append(torch.sum(r * r) / float(t["n_norm"]))
        rs.append(r.detach().numpy().reshape(-1))
    total = sum(float(w) * l for w, l in zip(weights, losses))
    (g,) = torch.autograd.grad(total, th)
    return po.Evaluation(np.array([float(l.detach()) for l in losses]), float(total.detach()), g.numpy()), rs


# ------------------------------------------------------------------------------------------------------------------------------------------
# the model of a handle's state, and a handle brought straight to it
# ------------------------------------------------------------------------------------------------------------------------------------------
def _subset(P, k, n, variant):
    perm = np.random.default_rng([23, P.index, k, int(variant)]).permutation(N_MASTER)
    return np.ascontiguousarray(P.master[k][:, perm[:n]])


def _pw(n, variant):
    w = np.random.default_rng([29, int(variant), n]).uniform(0.5, 1.5, size=n)
    return (w / w.sum()).astype(np.float32)


def _install(eng, S, k):
    """term k of the model on a handle: sampler, set, observations, quadrature weights — through the entry points the model remembers"""
    t = S["terms"][k]
    f64 = S["prec"] == "f64"
    if t["sampler"] is not None:
        kind, seed, n = t["sampler"]
        eng.set_sampler(k, S["lb"][k], S["ub"][k], n, seed=seed, kind=kind)
        if t["drawn"]:
            return
    (eng.set_points_f64 if f64 and t["entry"] == "f64" else eng.set_points)(k, t["pts"], t["n_norm"])
    if t["data"] is not None:
        (eng.set_point_data_f64 if f64 and t["data_entry"] == "f64" else eng.set_point_data)(k, t["data"])
    if t["pw"] is not None:
        eng.set_point_weights(k, t["pw"])


def fresh(npde, P, S):
    eng = npde._lib.Engine(P.descriptor)
    if eng.get_option("gemm") != S["gemm"]:
        eng.set_option("gemm", S["gemm"])
    if S["persistent"] != "on":
        eng.set_option("persistent", S["persistent"])
    if P.integral and S["Q"] != 16:
        eng.set_option("integral_nodes", str(S["Q"]))
    if S["prec"] == "f64":
        eng.set_option("precision", "f64")
    for k in range(P.K):
        _install(eng, S, k)
    if S["deriv"] == "stencil":
        eng.set_option("derivative", "stencil")
    return eng


def _probe(P, net):
    d = P.net_d[net]
    k = next(i for i, dk in enumerate(P.dims) if dk == d)
    return _subset(P, k, N_PROBE, 991)


def observe(eng, P, S, theta, weights):
    """everything a checkpoint reads, as a dict of arrays; drawn sets are read back into the model by the caller"""
    out = {}
    ns = [t["n"] for t in S["terms"]]
    out["loss"], out["grad"] = eng.loss_grad(theta, weights)
    out["loss_only"], _ = eng.loss_grad(theta, weights, want_grad=False)
    out["tl"], out["tg"] = eng.term_grads(theta)
    for k in range(P.K):
        out["res%d" % k] = eng.residual(k, theta, ns[k])
        out["pts%d" % k] = eng.get_points(k, P.dims[k], ns[k])
    pr = _probe(P, 0)
    out["phi"] = eng.phi(0, theta, pr)
    if not P.embedded:                                            # (pinn_derivative is refused behind a periodic embedding)
        out["d2"] = eng.derivative(0, theta, pr, [0, 0])
    if S["prec"] == "f64":
        out["loss64"], out["grad64"] = eng.loss_grad_f64(theta, weights)
        out["loss_only64"], _ = eng.loss_grad_f64(theta, weights, want_grad=False)
        out["tl64"], out["tg64"] = eng.term_grads_f64(theta)
        for k in range(P.K):
            out["res64_%d" % k] = eng.residual_f64(k, theta, ns[k])
        out["phi64"] = eng.phi_f64(0, theta, pr)
        if not P.embedded:
            out["d2_64"] = eng.derivative_f64(0, theta, pr, [0, 0])
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# the runner
# ------------------------------------------------------------------------------------------------------------------------------------------
class _Run:
    def __init__(self, npde, P, seed):
        self.npde, self.P, self.seed = npde, P, seed
        self.rng = np.random.default_rng([41, P.index, int(seed)])
        self.EngineError = npde._lib.EngineError
        self.eng = npde._lib.Engine(P.descriptor)
        self.S = dict(prec="f32", gemm=self.eng.get_option("gemm"), persistent="on", deriv="exact", Q=16, lb=P.lb, ub=P.ub,
                      terms=[dict(n=0, pts=None, n_norm=0, entry="f32", data=None, data_entry="f32", pw=None, sampler=None, drawn=False) for _ in range(P.K)])
        self.ops, self.checkpoints, self.resumed = [], [], []
        self.sizes = [[] for _ in range(P.K)]
        self.paths = dict(eval_path=set(), adam_path=set(), f64_path=set())
        self.pending = None                     # the resumable state: dict(kind, prec, k1, first, ...)
        self.w = np.linspace(1.0, 2.0, P.K)
        self.stds = np.linspace(0.5, 1.5, P.K)

    # ---- bookkeeping -------------------------------------------------------------------------------------------------------------------
    def pick(self, seq, p=None):
        return seq[int(self.rng.choice(len(seq), p=p))]

    def size(self):
        w = LADDER_W2 if self.P.family2 else LADDER_W
        return int(self.pick(LADDER, w / w.sum()))

    def other_theta(self):
        return self.P.theta + 0.05 * self.rng.standard_normal(self.P.P)

    def log(self, kind, detail, refused=None):
        self.ops.append(dict(kind=kind, detail=detail, refused=refused))

    def expect_refusal(self, kind, detail, match, fn):
        """fn must be refused with `match` in the message; what came instead is recorded for the test to assert on"""
        try:
            fn()
            got = "ran"
        except self.EngineError as e:
            got = str(e)
        self.ops.append(dict(kind=kind, detail=detail, refused=dict(want=match, got=got)))

    def note_paths(self):
        for name in self.paths:
            self.paths[name].add(self.eng.get_option(name))

    def sampled(self):
        return any(t["sampler"] is not None for t in self.S["terms"])

    def fixed_terms(self):
        return [k for k, t in enumerate(self.S["terms"]) if t["sampler"] is None]

    # ---- state operations --------------------------------------------------------------------------------------------------------------
    def set_points(self, k, n=None, variant=None, log=True, same_n=False):
        S, P, t = self.S, self.P, self.S["terms"][k]
        n = self.size() if n is None else n
        if same_n:                              # a set of the size the term holds: stale per-point weights would still fit it
            n = t["n"]
        variant = int(self.rng.integers(1000)) if variant is None else variant
        entry = "f64" if self.rng.integers(2) else "f32"
        n_norm = 2 * n if self.rng.integers(5) == 0 else n
        pts = _subset(P, k, n, variant)
        (self.eng.set_points_f64 if entry == "f64" else self.eng.set_points)(k, pts, n_norm)
        t.update(n=n, pts=pts, n_norm=n_norm, entry=entry if S["prec"] == "f64" else "f32", data=None, pw=None, drawn=False)
        self.sizes[k].append(n)
        if log:
            self.log("points", (k, n, entry, n_norm))
        if P.ndata[k]:
            if log and self.rng.integers(3) == 0:
                self.expect_refusal("eval_without_data", k, "data", lambda: self.eng.loss_grad(P.theta))
            self.set_data(k, log=False)

    def set_data(self, k, log=True):
        t = self.S["terms"][k]
        entry = "f64" if self.rng.integers(2) else "f32"
        data = _data_values(t["pts"], int(self.rng.integers(1000)))
        (self.eng.set_point_data_f64 if entry == "f64" else self.eng.set_point_data)(k, data)
        t.update(data=data if entry == "f64" and self.S["prec"] == "f64" else data.astype(np.float32).astype(np.float64),
                 data_entry=entry if self.S["prec"] == "f64" else "f32")
        if log:
            self.log("data", (k, entry))

    def set_pweights(self):
        k = self.pick(range(self.P.K))
        t = self.S["terms"][k]
        if t["sampler"] is not None:
            return self.expect_refusal("pweights", k, "resampled", lambda: self.eng.set_point_weights(k, _pw(t["n"], 0)))
        if t["pw"] is not None and self.rng.integers(2):
            self.eng.set_point_weights(k, None)
            t["pw"] = None
        else:
            t["pw"] = _pw(t["n"], int(self.rng.integers(1000)))
            self.eng.set_point_weights(k, t["pw"])
        self.log("pweights", (k, t["pw"] is not None))

    def set_precision(self, v):
        S = self.S
        if v == "f64" and not self.P.f64_ok:
            return self.expect_refusal("option", ("precision", v), "f32" if self.P.integral else "DGM", lambda: self.eng.set_option("precision", "f64"))
        self.eng.set_option("precision", v)
        if self.pending is not None and self.pending["prec"] == "f64" and S["prec"] == "f64" and v == "f32":
            self.pending["left_f64"] = True     # the double copies are converted from the float buffers from here on: another objective where they differ
            if any((t["entry"] == "f64" and self.P.embedded) or (t["data"] is not None and t["data_entry"] == "f64") for t in S["terms"]):
                self.pending = None
        if v != S["prec"]:
            S["deriv"] = "exact"                # the stencil tapes belong to the float64 state
            for t in S["terms"]:                # the double copies went with the mode / are converted from the float buffers
                t["entry"], t["data_entry"] = "f32", "f32"
                if t["pts"] is not None:
                    t["pts"] = t["pts"].astype(np.float32).astype(np.float64)
                if t["data"] is not None:
                    t["data"] = t["data"].astype(np.float32).astype(np.float64)
        S["prec"] = v
        self.log("option", ("precision", v))

    def set_option(self):
        S, P = self.S, self.P
        name = self.pick((("precision", "precision") if P.f64_ok else ("persistent", "gemm")) + ("precision", "gemm", "persistent", "derivative")
                         + (("integral_nodes",) * 2 if P.integral else ()))
        if name == "precision":
            return self.set_precision("f32" if S["prec"] == "f64" else "f64")
        if name != "persistent":
            self.pending = None                 # another arithmetic / another objective: a resumable state is dropped
        if name == "gemm":
            S["gemm"] = "fp32" if S["gemm"] == "split" else "split"
            self.eng.set_option("gemm", S["gemm"])
            return self.log("option", ("gemm", S["gemm"]))
        if name == "persistent":
            S["persistent"] = "off" if S["persistent"] == "on" else "on"
            self.eng.set_option("persistent", S["persistent"])
            return self.log("option", ("persistent", S["persistent"]))
        if name == "derivative":
            v = "exact" if S["deriv"] == "stencil" else "stencil"
            if v == "stencil" and S["prec"] != "f64":
                return self.expect_refusal("option", ("derivative", v), "precision", lambda: self.eng.set_option("derivative", "stencil"))
            if v == "stencil" and not P.stencil_ok:
                return self.expect_refusal("option", ("derivative", v), "embedding", lambda: self.eng.set_option("derivative", "stencil"))
            self.eng.set_option("derivative", v)
            S["deriv"] = v
            return self.log("option", ("derivative", v))
        q = int(self.pick((4, 9, 16, 24)))
        self.eng.set_option("integral_nodes", str(q))
        S["Q"] = q
        self.log("option", ("integral_nodes", q))

    def set_sampler(self):
        S, P = self.S, self.P
        on = [k for k, t in enumerate(S["terms"]) if t["sampler"] is not None]
        if on and self.rng.integers(2):
            k = self.pick(on)                   # kind 0: the drawn set stays, as a fixed set
            t = S["terms"][k]
            self.eng.set_sampler(k, P.lb[k], P.ub[k], t["n"], kind=0)
            if t["drawn"]:
                t.update(pts=self.eng.get_points(k, P.dims[k], t["n"]).astype(np.float64), entry="f32")
            t.update(sampler=None, drawn=False)
            return self.log("sampler", (k, 0))
        k = self.pick(range(P.K))
        kind, seed, n = int(self.rng.integers(1, 4)), int(self.rng.integers(1, 1000)), self.size()
        t = S["terms"][k]
        if P.ndata[k]:
            data = _data_values(t["pts"], 1)
            self.eng.set_sampler(k, P.lb[k], P.ub[k], t["n"], seed=seed, kind=kind)      # (a sampled data term is refused where it is used:)
            self.expect_refusal("data_on_sampled_term", k, "resampled", lambda: self.eng.set_point_data(k, data))
            self.eng.set_sampler(k, P.lb[k], P.ub[k], t["n"], kind=0)
            return self.set_points(k, t["n"], log=False)
        self.eng.set_sampler(k, P.lb[k], P.ub[k], n, seed=seed, kind=kind)
        t.update(n=n, pts=None, n_norm=n, entry="f32", data=None, pw=None, sampler=(kind, seed, n), drawn=True)
        self.sizes[k].append(n)
        self.log("sampler", (k, kind, n))

    # ---- traceless operations ----------------------------------------------------------------------------------------------------------
    def evaluate(self, log=True):
        eng, P, th = self.eng, self.P, self.other_theta()
        f64 = bool(self.rng.integers(2))
        what = self.pick(("loss_grad", "loss_only", "term_grads", "loglik", "residual"))
        if what == "loss_grad":
            (eng.loss_grad_f64 if f64 else eng.loss_grad)(th, self.w if self.rng.integers(2) else None)
        elif what == "loss_only":
            (eng.loss_grad_f64 if f64 else eng.loss_grad)(th, None, want_grad=False)
        elif what == "term_grads":
            (eng.term_grads_f64 if f64 else eng.term_grads)(th)
        elif what == "loglik":
            (eng.loglik_grad_f64 if f64 else eng.loglik_grad)(th, self.stds)
        else:
            k = self.pick(range(P.K))
            (eng.residual_f64 if f64 else eng.residual)(k, th, self.S["terms"][k]["n"])
        self.note_paths()
        if log:
            self.log("eval", (what, f64))

    def net_eval(self):
        eng, P, th = self.eng, self.P, self.other_theta()
        net = int(self.rng.integers(len(P.net_d)))
        k = next(i for i, dk in enumerate(P.dims) if dk == P.net_d[net])
        pts = _subset(P, k, self.size(), int(self.rng.integers(1000)))
        f64 = bool(self.rng.integers(2))
        what = self.pick(("phi", "derivative", "ensemble") if P.ens_ok else ("phi", "derivative", "phi", "phi", "ensemble"))
        if what == "phi":
            (eng.phi_f64 if f64 else eng.phi)(net, th, pts)
        elif what == "derivative":
            axes = [0, 0] if self.rng.integers(2) else [0]
            if P.embedded:
                return self.expect_refusal("net", ("derivative",), "embedding", lambda: eng.derivative(net, th, pts, axes))
            (eng.derivative_f64 if f64 else eng.derivative)(net, th, pts, axes)
        else:
            ths = np.stack([self.other_theta() for _ in range(3)])
            if not P.ens_ok:
                return self.expect_refusal("net", ("ensemble",), "DGM" if P.name == "dgm" else "embedding", lambda: eng.phi_ensemble(net, ths, pts))
            eng.phi_ensemble(net, ths, pts, ddof=1)
        self.log("net", (what, f64, pts.shape[1]))

    def adam(self):
        if self.sampled():                      # (a sampled term's draw counter is part of the state: only the detour runs Adam on one)
            return self.evaluate()
        th0 = self.other_theta()
        n = int(self.rng.integers(2, 5))
        (self.eng.adam_f64 if self.rng.integers(2) else self.eng.adam)(th0, n, 1e-3, self.w if self.rng.integers(2) else None)
        self.note_paths()
        self.log("adam", n)

    def lbfgs(self):
        th0 = self.other_theta()
        if self.sampled():
            return self.expect_refusal("lbfgs", "sampled", "redraws", lambda: self.eng.lbfgs(th0, 2))
        self.eng.lbfgs(th0, 2, self.w if self.rng.integers(2) else None, history=3)
        self.note_paths()
        self.log("lbfgs", 2)

    def rlbfgs(self):
        th0 = self.other_theta()
        if self.sampled():
            return self.expect_refusal("rlbfgs", "sampled", "redraws", lambda: self.eng.lbfgs_init(th0, None, 3))
        self.eng.lbfgs_init(th0, self.w if self.rng.integers(2) else None, history=3)
        self.eng.lbfgs_steps(2)
        self.eng.lbfgs_get()
        self.log("rlbfgs", 2)

    def priors(self):
        return [("normal", 0.5, 1.0)] * self.P.ne

    def hmc(self):
        th0 = self.other_theta()
        if self.sampled():
            return self.expect_refusal("hmc", "sampled", "redraws", lambda: self.eng.hmc_init(th0, self.stds, param_priors=self.priors()))
        self.eng.hmc_init(th0, self.stds, param_priors=self.priors())
        self.eng.hmc_draws(2, 2, 1e-3, seed=int(self.rng.integers(1, 1000)))
        self.log("hmc", 2)

    def sampler_detour(self):
        S, P = self.S, self.P
        cand = [k for k in self.fixed_terms() if not P.ndata[k]]
        if not cand or self.sampled():
            return self.evaluate()
        k = self.pick(cand)
        t = S["terms"][k]
        kind, n = int(self.rng.integers(1, 4)), self.size()
        self.eng.set_sampler(k, P.lb[k], P.ub[k], n, seed=int(self.rng.integers(1, 1000)), kind=kind)
        self.sizes[k].append(n)
        (self.eng.adam_f64 if S["prec"] == "f64" and self.rng.integers(2) else self.eng.adam)(self.other_theta(), 3, 1e-3)
        self.note_paths()
        self.eng.set_sampler(k, P.lb[k], P.ub[k], n, kind=0)
        self.reinstall(k)
        self.log("sampler_detour", (k, kind, n))

    def reinstall(self, k):
        """the model's term k once more, as it is held"""
        t = self.S["terms"][k]
        self.sizes[k].append(t["n"])
        _install(self.eng, self.S, k)

    def timing(self):
        level = int(self.rng.integers(1, 3))
        self.eng.set_timing(level, -1)
        self.evaluate(log=False)
        if level == 2 and self.S["prec"] == "f32":          # (the phase events bracket the fp32 evaluation)
            self.eng.loss_grad(self.other_theta(), self.w)
            self.eng.last_timing()
        self.note_paths()
        self.eng.set_timing(0, -1)
        self.log("timing", level)

    def option_detour(self):
        S, P = self.S, self.P
        name = self.pick(("gemm", "persistent") + (("precision", "derivative") if P.f64_ok else ()) + (("integral_nodes",) * 2 if P.integral else ()))
        if name == "gemm":
            other = "fp32" if S["gemm"] == "split" else "split"
            self.eng.set_option("gemm", other); self.evaluate(log=False); self.eng.set_option("gemm", S["gemm"])
        elif name == "persistent":
            other = "off" if S["persistent"] == "on" else "on"
            self.eng.set_option("persistent", other); self.evaluate(log=False); self.eng.set_option("persistent", S["persistent"])
        elif name == "integral_nodes":
            self.eng.set_option("integral_nodes", str(self.pick((5, 33)))); self.evaluate(log=False); self.eng.set_option("integral_nodes", str(S["Q"]))
        elif name == "derivative":
            if S["prec"] != "f64" or not P.stencil_ok:
                return self.evaluate()
            other = "exact" if S["deriv"] == "stencil" else "stencil"
            self.eng.set_option("derivative", other); self.evaluate(log=False); self.eng.set_option("derivative", S["deriv"])
        else:
            # the mode there and back: what the float64 state held in double is held as float afterwards — the model follows
            if not P.f64_ok:
                return self.evaluate()
            back = S["prec"]
            self.set_precision("f64" if back == "f32" else "f32"); self.ops.pop()
            self.evaluate(log=False)
            self.set_precision(back); self.ops.pop()
        self.log("option_detour", name)

    def points_detour(self):
        cand = self.fixed_terms()
        if not cand:
            return self.evaluate()
        k = self.pick(cand)
        keep = copy.deepcopy(self.S["terms"][k])
        path = list(WALKS[int(self.seed) % len(WALKS)]) + [self.size()]
        for n in path:
            self.set_points(k, n, log=False)
            if self.rng.integers(2):
                self.evaluate(log=False)
        self.S["terms"][k] = keep
        self.reinstall(k)
        self.log("points_detour", (k, tuple(path)))

    # ---- resumable states --------------------------------------------------------------------------------------------------------------
    def freeze_samplers(self):
        """kind 0 on every sampled term: the sets drawn last stay, as fixed sets, and the model reads them back"""
        S, P = self.S, self.P
        for k, t in enumerate(S["terms"]):
            if t["sampler"] is not None:
                self.eng.set_sampler(k, P.lb[k], P.ub[k], t["n"], kind=0)
                if t["drawn"]:
                    t.update(pts=self.eng.get_points(k, P.dims[k], t["n"]).astype(np.float64), entry="f32")
                t.update(sampler=None, drawn=False)
                self.log("sampler", (k, 0))

    def begin(self, kind):
        S, P = self.S, self.P
        self.freeze_samplers()                  # a fixed objective first
        th0, k1 = self.other_theta(), int(self.rng.integers(1, 4))
        w = self.w if self.rng.integers(2) else None
        pend = dict(kind=kind, prec=S["prec"], th0=th0, k1=k1, w=w, left_f64=False, seed=int(self.rng.integers(1, 1000)))
        if kind == "adam":
            pend["first"] = (self.eng.adam_f64 if S["prec"] == "f64" else self.eng.adam)(th0, k1, 1e-3, w)
            self.note_paths()
        elif kind == "rlbfgs":
            self.eng.lbfgs_init(th0, w, history=3)
            pend["first"] = self.eng.lbfgs_steps(k1)
        else:
            self.eng.hmc_init(th0, self.stds, param_priors=self.priors())
            pend["first"] = self.eng.hmc_draws(k1, 2, 1e-3, seed=pend["seed"])
        self.pending = pend
        self.log("begin_" + kind, k1)

    def resume(self):
        S, p, eng = self.S, self.pending, self.eng
        self.pending = None
        kind, k2 = p["kind"], int(self.rng.integers(1, 4))
        step = {"adam": lambda e: (e.adam_f64 if S["prec"] == "f64" else e.adam)(None, k2, 1e-3, p["w"], init=False),
                "rlbfgs": lambda e: e.lbfgs_steps(k2) + e.lbfgs_get(),
                "hmc": lambda e: e.hmc_draws(k2, 2, 1e-3, seed=p["seed"]) + e.hmc_get()}[kind]
        if kind == "adam" and p["prec"] == "f64" and S["prec"] == "f32":
            return self.evaluate()              # (the fp32 optimiser state is another state, begun or not by an earlier run: nothing to compare with)
        if S["prec"] != p["prec"] or (p["prec"] == "f64" and p["left_f64"] and kind == "adam"):
            match = "pinn_adam_init" if kind == "adam" else "precision changed"
            return self.expect_refusal("resume_" + kind, "precision", match, lambda: step(eng))
        if kind == "adam" and self.sampled():
            # accepted, on the redrawn sets: another objective, so no fresh handle to compare with — the call runs its k2 steps and returns k2 finite
            # losses; the sets drawn last then stay as fixed sets, so that the model knows what the handle holds
            th, hist = step(eng)
            self.resumed.append(dict(kind="adam_on_sampler", got=(np.array(hist.size), np.array(bool(np.isfinite(hist).all() and np.isfinite(th).all()))),
                                     want=(np.array(k2), np.array(True)), at=len(self.ops)))
            self.log("resume_adam", ("sampled", k2))
            self.note_paths()
            return self.freeze_samplers()
        if self.sampled():
            return self.expect_refusal("resume_" + kind, "sampled", "redraws", lambda: step(eng))
        got = step(eng)
        # the same k1 + k2 in one go on a fresh handle
        f = fresh(self.npde, self.P, S)
        if kind == "adam":
            th, hist = (f.adam_f64 if S["prec"] == "f64" else f.adam)(p["th0"], p["k1"] + k2, 1e-3, p["w"])
            want, got = (th, hist), (got[0], np.concatenate([p["first"][1], got[1]]))
        elif kind == "rlbfgs":
            f.lbfgs_init(p["th0"], p["w"], history=3)
            h, ev, st = f.lbfgs_steps(p["k1"] + k2)
            want = (h,) + f.lbfgs_get()
            got = (np.concatenate([p["first"][0], got[0]]),) + tuple(got[3:])
        else:
            f.hmc_init(p["th0"], self.stds, param_priors=self.priors())
            smp, acc, lp = f.hmc_draws(p["k1"] + k2, 2, 1e-3, seed=p["seed"])
            want = (smp, acc, lp) + f.hmc_get()
            got = tuple(np.concatenate([a, b]) for a, b in zip(p["first"], got[:3])) + tuple(got[3:])
        f.close()
        self.resumed.append(dict(kind=kind, got=got, want=want, at=len(self.ops)))
        self.log("resume_" + kind, k2)

    # ---- checkpoints -------------------------------------------------------------------------------------------------------------------
    def checkpoint(self, final):
        S, P = self.S, self.P
        if final and S["deriv"] == "stencil":   # the two handles are compared under stencil first; the oracle bars are those of exact derivatives
            self.checkpoint(False)
            self.eng.set_option("derivative", "exact")
            S["deriv"] = "exact"
        a = observe(self.eng, P, S, P.theta, self.w)
        self.note_paths()
        f = fresh(self.npde, P, S)
        b = observe(f, P, S, P.theta, self.w)
        f.close()
        self.checkpoints.append(dict(at=len(self.ops), final=final, reused=a, fresh=b, prec=S["prec"]))
        if not final:
            return None
        Sx = copy.deepcopy(S)
        for k, t in enumerate(Sx["terms"]):
            if t["pts"] is None:
                t["pts"] = a["pts%d" % k].astype(np.float64)
        return dict(state=Sx, obs=a)

    # ---- one sequence ------------------------------------------------------------------------------------------------------------------
    def state_op(self, kind):
        P = self.P
        if kind in ("points", "data", "pweights"):
            self.pending = None                 # another objective: a resumable state is dropped
        if kind == "points":
            k = self.pick(self.fixed_terms() or list(range(P.K)))
            self.set_points(k, same_n=self.S["terms"][k]["pw"] is not None)
        elif kind == "data":
            self.set_data(P.ndata.index(1))
        else:
            getattr(self, "set_" + kind)()

    def run(self):
        """SEQ_LEN slots: one resumable state (its kind by the seed) begun in the first half and resumed two to four slots later, with only
        traceless operations in between on three seeds of four and a device sampler or the other precision mode right behind the begin on the
        fourth (the refusal / acceptance cells of the contract table); the other slots take state operations (three in ten) and traceless ones from
        decks that rotate with the seed, so that a few seeds reach every kind"""
        P, seed = self.P, int(self.seed)
        if P.f64_ok and seed % 4 == 2:          # a quarter of the sequences start in the float64 mode
            self.set_precision("f64")
        for k in range(P.K):
            self.set_points(k, log=False)
        begin_at = int(self.rng.integers(0, 5))
        resume_at = begin_at + int(self.rng.integers(2, 5))
        kind3 = ("adam", "rlbfgs", "hmc")[seed % 3]
        if P.family2:                           # (half the seeds: one sequence per resumable kind over the two 64-wide problems)
            quiet = not (seed >= 3 and (seed + P.index // 2) % 2 == 0)
        else:
            quiet = (seed // 3) % 4 != 3
        # the other sequences put a contract cell right behind the begin: a device sampler or the other precision mode
        forced = None if quiet else ("sampler" if (kind3 == "adam" and P.family2) or (seed + P.index) % 2 == 0 else "precision")
        states = ("pweights", "points", "option", "sampler", "pweights", "option", "points")
        if any(P.ndata):
            states = ("data",) + states + ("data",)
        sdeck = [states[(seed * 3 + i) % len(states)] for i in range(SEQ_LEN)]
        tdeck = [TRACELESS_KINDS[(seed * 3 + i) % len(TRACELESS_KINDS)] for i in range(2 * SEQ_LEN)]
        mid = int(self.rng.integers(2, SEQ_LEN - 1))
        for i in range(SEQ_LEN):
            if i == mid:
                self.checkpoint(False)
            between = begin_at < i < resume_at
            if i == begin_at:
                self.begin(kind3)
            elif i == begin_at + 1 and forced == "sampler":
                self.set_sampler()
            elif i == begin_at + 1 and forced == "precision":
                self.set_precision("f32" if self.S["prec"] == "f64" else "f64")
            elif i == resume_at and self.pending is not None:
                self.resume()
            elif self.rng.uniform() < 0.3 and not (between and quiet):
                self.state_op(sdeck.pop(0))
            else:
                busy = self.pending["kind"] if self.pending else None
                kind = tdeck.pop(0)
                while (busy == "adam" and kind in ("adam", "sampler_detour")) or (busy == kind):
                    kind = tdeck.pop(0)
                getattr(self, {"eval": "evaluate", "net": "net_eval"}.get(kind, kind))()
        final = self.checkpoint(True)
        self.eng.close()
        return Record(P.name, self.seed, self.ops, self.checkpoints, self.resumed, final, self.sizes, self.paths)


def run(npde, name, seed):
    return _Run(npde, problem(npde, name), seed).run()
