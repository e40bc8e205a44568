"""Chain-resident HMC (`pinn_hmc_chains_*`): nchains BPINN chains in one launch, one workgroup each.

Reference: the leapfrog / energy / accept recurrence in numpy double with the log-posterior gradient from `oracle/pinn_oracle.py`
`loss_and_grad` (float64, exact mode) plus the priors — never the code under test.  Computed once per (problem, n_leapfrog) for three chains and
shared; an nchains = 1 call is compared with its chain 0.

Problems (the smallest at which the kernel can go wrong): (a) 1-6-1 tanh on GridTraining(0.1): 11 + 1 + 1 points, one partly filled tile per term,
K = 3, three of the four waves idle in some phase, P = 19; (b) 2-16-16-1 sigmoid on 70 interior + 2 x 20 boundary Sobol' points: two tiles, one
masked, one estimated PDE parameter with a LogNormal prior, P = 338 (no multiple of 256).

THE BAR of test 1 is, per problem, 4 x the worst error of the existing fp32 `sampler="device"` lane (`pinn_hmc_draws`) against the same reference
on the same cases, measured on MI355X with tools/hmc_chains_error.py (profiles/hmc_chains.txt): DEVICE_LANE_ERR below.  Errors are max-norm
relative per output array (samples, logp, accept_prob).  Every test runs twice (fixture `lib`): on the g++ emulation (`use_emu`) and, marked
`gpu`, on the product library (`hip_lib`).  The communicator refusal needs a second device and is not exercised here."""
import functools
import os
import sys

import numpy as np
import pytest
import sympy as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import helpers
import pinn_oracle as po

DEVICE_LANE_ERR = {"a": 6.255e-05, "b": 3.544e-06}        # worst case of the fp32 device lane per problem on an MI355X (profiles/hmc_chains.txt)
NN_PRIOR = (0.0, 2.0)
NCH, NDRAWS = 3, 3
EPS = {1: 2.0e-2, 5: 1.0e-2}


def problem(npde, case):
    """-> rep, oracle problem, point sets, theta0 [NCH x P], stds, nn, priors"""
    from neuralpde_jl_amd import bpinn
    if case == "a":
        (x,) = npde.parameters("x")
        (u,) = npde.variables("u")
        eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.pi ** 2 * sp.sin(sp.pi * x), 0)
        sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
        chain = npde.Chain(npde.Dense(1, 6, "tanh"), npde.Dense(6, 1))
        disc = lambda th: npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=th, precision="f32")
        priors, stds = [], np.array([0.5, 0.3, 0.3])
    else:
        x, y = npde.parameters("x y")
        (p,) = npde.parameters("p")
        (u,) = npde.variables("u")
        Dx, Dy = npde.Differential(x), npde.Differential(y)
        eq = npde.Eq(Dx(Dx(u(x, y))) + Dy(Dy(u(x, y))) + p * sp.sin(sp.pi * x) * sp.sin(sp.pi * y), 0)
        sysm = npde.PDESystem([eq], [npde.Eq(u(0.0, y), 0.0), npde.Eq(u(x, 1.0), 0.0)],
                              [npde.In(x, npde.Interval(0.0, 1.0)), npde.In(y, npde.Interval(0.0, 1.0))], [x, y], [u(x, y)], ps=[p], defaults={p: 4.0})
        chain = npde.Chain(npde.Dense(2, 16, "sigmoid"), npde.Dense(16, 16, "sigmoid"), npde.Dense(16, 1))
        strat = npde.QuasiRandomTraining(70, bcs_points=20, sampling_alg=npde.SobolSample(seed=31), resampling=False, minibatch=1)
        disc = lambda th: npde.PhysicsInformedNN(chain, strat, init_params=th, param_estim=True, precision="f32")
        priors, stds = [bpinn.LogNormal(2.0, 0.5)], np.array([0.5, 0.3, 0.3])
    rep = npde.symbolic_discretize(sysm, disc(npde.initialparameters(np.random.default_rng(7), chain)))
    eng = rep.engine
    nn = eng.P - len(priors)
    th = np.tile(np.asarray(rep.flat_init_params, dtype=np.float64), (NCH, 1))
    th[1:, :nn] += 0.05 * np.random.default_rng(8).standard_normal((NCH - 1, nn))
    for j, pr in enumerate(priors):
        th[:, nn + j] = pr.params()[0] * (1.0 + 0.1 * np.arange(NCH))
    sets = [np.asarray(s, dtype=np.float64) for s in rep.pde_train_sets + rep.bcs_train_sets]
    return rep, helpers.oracle_problem(npde, sysm, [chain], param_estim=bool(priors)), sets, th, stds, nn, priors


def kinds_of(priors):
    from neuralpde_jl_amd import bpinn
    return [(1 if isinstance(q, bpinn.LogNormal) else 0,) + tuple(q.params()) for q in priors]


def inputs(P, case, n_leapfrog):
    rng = np.random.default_rng(100 * n_leapfrog + ord(case))
    minv = 0.5 + rng.random(P)
    return minv, rng.standard_normal((NCH, NDRAWS, P)) / np.sqrt(minv), rng.random((NCH, NDRAWS))


def reference(prob, sets, th0, stds, nn, priors, minv, mom, uni, n_leapfrog, eps):
    """one chain in numpy double -> samples, logp, accept_prob, final (theta, logp, grad)"""
    n = np.array([s.shape[1] for s in sets], dtype=np.float64)
    w = n / (2.0 * stds ** 2)
    mu0, sd0 = NN_PRIOR

    def logp_grad(th):
        ev = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
        lp = float(np.sum(-0.5 * n * np.log(2.0 * np.pi) - n * np.log(stds) - w * ev.term_losses))
        g = -np.asarray(ev.grad, dtype=np.float64)
        lp += -0.5 * np.sum(((th[:nn] - mu0) / sd0) ** 2) - nn * (np.log(sd0) + 0.5 * np.log(2 * np.pi))
        g[:nn] -= (th[:nn] - mu0) / sd0 ** 2
        for j, pr in enumerate(priors):
            l, d = pr.logpdf_grad(float(th[nn + j]))
            lp += l
            g[nn + j] += d
        return lp, g
    th = th0.copy()
    lp, g = logp_grad(th)
    S, L, A = [], [], []
    for r, u in zip(mom, uni):
        h_old = -lp + 0.5 * np.sum(minv * r * r)
        tn, rn = th, r + 0.5 * eps * g
        for s in range(n_leapfrog):
            tn = tn + eps * minv * rn
            lpn, gn = logp_grad(tn)
            rn = rn + (eps if s < n_leapfrog - 1 else 0.5 * eps) * gn
        h_new = -lpn + 0.5 * np.sum(minv * rn * rn)
        a = float(np.exp(min(0.0, h_old - h_new))) if np.isfinite(h_new) else 0.0
        if u < a:
            th, lp, g = tn, lpn, gn
        S.append(th.copy()); L.append(lp); A.append(a)
    return np.asarray(S), np.asarray(L), np.asarray(A), (th, lp, g)


@functools.lru_cache(maxsize=None)
def shared_reference(npde, case, n_leapfrog):
    """the NCH reference chains of a (problem, n_leapfrog) pair, computed once (read-only afterwards)"""
    rep, prob, sets, th0, stds, nn, priors = problem(npde, case)
    minv, mom, uni = inputs(rep.engine.P, case, n_leapfrog)
    return [reference(prob, sets, th0[c], stds, nn, priors, minv, mom[c], uni[c], n_leapfrog, EPS[n_leapfrog]) for c in range(NCH)]


def relerr(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(x - ref))) / float(np.max(np.abs(ref)))


def run(eng, th0, stds, priors, minv, mom, uni, n_leapfrog, chains=slice(None), splits=(NDRAWS,)):
    """chains `chains` through pinn_hmc_chains_*, the draws in calls of `splits` draws -> samples, accept_prob, logp"""
    eng.hmc_chains_init(th0[chains], EPS[n_leapfrog], stds, NN_PRIOR, kinds_of(priors), n_leapfrog, minv)
    out, d0 = [], 0
    for nd in splits:
        out.append(eng.hmc_chains_draws(nd, mom[chains, d0:d0 + nd], uni[chains, d0:d0 + nd]))
        d0 += nd
    return [np.concatenate([o[j] for o in out], axis=1) for j in range(3)]


@pytest.fixture(params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("use_emu" if request.param == "emu" else "hip_lib")


# ---- test 1: against the plain double reference ----
@pytest.mark.parametrize("case,nchains,n_leapfrog", [(c, n, L) for c in "ab" for n in (1, NCH) for L in (1, 5)])
def test_reference(npde, lib, case, nchains, n_leapfrog):
    rep, _, _, th0, stds, nn, priors = problem(npde, case)
    minv, mom, uni = inputs(rep.engine.P, case, n_leapfrog)
    ref = shared_reference(npde, case, n_leapfrog)
    smp, acc, lp = run(rep.engine, th0, stds, priors, minv, mom, uni, n_leapfrog, slice(0, nchains))
    err = max(max(relerr(smp[c], ref[c][0]), relerr(lp[c], ref[c][1]), relerr(acc[c], ref[c][2])) for c in range(nchains))
    bar = 4.0 * DEVICE_LANE_ERR[case]
    print(f"hmc chains vs reference [{case} nchains={nchains} L={n_leapfrog}]: err {err:.3e}  bar {bar:.3e}  a = {np.round([r[2] for r in ref[:nchains]], 4).tolist()}")
    assert all(0.0 < r[2].min() for r in ref)
    assert err <= bar


# ---- test 2: chain independence, exact; the generator's chain keying ----
@pytest.mark.parametrize("case,n_leapfrog", [("a", 1), ("a", 5), ("b", 1), ("b", 5)])
def test_independence(npde, lib, case, n_leapfrog):
    rep, _, _, th0, stds, nn, priors = problem(npde, case)
    minv, mom, uni = inputs(rep.engine.P, case, n_leapfrog)
    three = run(rep.engine, th0, stds, priors, minv, mom, uni, n_leapfrog)
    for c in range(NCH):
        one = run(rep.engine, th0, stds, priors, minv, mom, uni, n_leapfrog, slice(c, c + 1))
        assert all(np.array_equal(one[j][0], three[j][c]) for j in range(3)), f"chain {c} depends on its neighbours"
    split = run(rep.engine, th0, stds, priors, minv, mom, uni, n_leapfrog, splits=(2, 1))
    assert all(np.array_equal(split[j], three[j]) for j in range(3))


def test_generator(npde, lib):
    """momenta and uniforms from the generator: chain 0 is the stream of pinn_hmc_draws (problem (a): one workgroup in both lanes, so the same
    bits), the other chains draw differently from the same start, and the counter runs on over calls"""
    rep, _, _, th0, stds, nn, priors = problem(npde, "a")
    eng = rep.engine
    eng.hmc_init(th0[0], stds, NN_PRIOR, [])
    want = eng.hmc_draws(NDRAWS, 5, EPS[5], 9)
    eng.hmc_chains_init(np.tile(th0[0], (NCH, 1)), EPS[5], stds, NN_PRIOR, [], 5, None, 9)
    got = [np.concatenate(x, axis=1) for x in zip(eng.hmc_chains_draws(2), eng.hmc_chains_draws(1))]
    assert all(np.array_equal(g[0], w) for g, w in zip(got, want))
    assert not np.array_equal(got[0][1], got[0][0]) and not np.array_equal(got[0][2], got[0][0]) and not np.array_equal(got[0][2], got[0][1])


# ---- test 3: both branches of the accept step ----
@pytest.mark.parametrize("case", ["a", "b"])
def test_accept_branches(npde, lib, case):
    rep, prob, sets, th0, stds, nn, priors = problem(npde, case)
    eng = rep.engine
    eps, seed = {"a": (0.05, 0), "b": (0.04, 0)}[case]       # picked with the reference alone: a > 0 for the first draw, a < 1 for the second, every chain
    rng = np.random.default_rng(seed)
    minv = 0.5 + rng.random(eng.P)
    mom = rng.standard_normal((NCH, 2, eng.P)) / np.sqrt(minv)
    uni = np.tile([0.0, 1.0], (NCH, 1))
    for c in range(NCH):
        a = reference(prob, sets, th0[c], stds, nn, priors, minv, mom[c], uni[c], 1, eps)[2]
        assert a[0] > 0.0 and a[1] < 1.0
    init = lambda: eng.hmc_chains_init(th0, eps, stds, NN_PRIOR, kinds_of(priors), 1, minv)
    init()
    eng.hmc_chains_draws(1, mom[:, :1], uni[:, :1])
    state1 = eng.hmc_chains_get()
    init()
    smp, acc, lp = eng.hmc_chains_draws(2, mom, uni)
    assert np.all(smp[:, 0] != th0) and np.all(acc[:, 0] > 0.0) and np.all(acc[:, 1] < 1.0)
    assert np.array_equal(smp[:, 1], smp[:, 0]) and np.array_equal(lp[:, 1], lp[:, 0])
    for got, want in zip(eng.hmc_chains_get(), state1):       # theta, logp and the gradient are those of the accepted draw
        assert np.array_equal(got, want)


# ---- test 4: API ----
def poisson1d(npde, chain):
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.pi ** 2 * sp.sin(sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    return sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=npde.initialparameters(np.random.default_rng(7), chain), precision="f32")


# set-ups outside the kernel's evaluation -> the words of their refusal; the named ones are tests/handle_history.py's problems
SETUPS = [("sampler", "redraws its points"), ("integral", "integral terms"), ("heat", "embedded coordinates"), ("system16", "several networks"),
          ("dgm", "DGM networks"), ("sin", "sin, swish and per-layer"), ("swish", "sin, swish and per-layer"), ("mixed", "sin, swish and per-layer"),
          ("poisson64", "no chain kernel"), ("wide", "2209 parameters")]


@pytest.mark.parametrize("setup,words", SETUPS)
def test_refused_setups(npde, lib, setup, words):
    """every set-up the kernel's evaluation does not cover is refused by name, and the handle evaluates afterwards what it evaluated before"""
    import handle_history as hh
    import test_emu_parity as tp
    if setup in hh.PROBLEMS:
        P = hh.problem(npde, setup)
        eng, th = npde._lib.Engine(P.descriptor), P.theta
        for k in range(P.K):
            eng.set_points(k, P.master[k][:, :24])
    else:
        if setup in ("sin", "swish"):
            sysm, chain = tp.poisson2d(npde, setup, 16, 2)       # (a shape whose sin / swish kernels are compiled ahead of time)
            disc = npde.PhysicsInformedNN(chain, npde.GridTraining(0.25), init_params=npde.initialparameters(np.random.default_rng(7), chain), precision="f32")
        else:
            sizes = {"sampler": (6,), "mixed": (8, 8), "wide": (32, 32, 32)}[setup]
            acts = ("tanh", "sigmoid", "tanh") if setup == "mixed" else ("tanh",) * 3
            dims = (1,) + sizes
            sysm, disc = poisson1d(npde, npde.Chain(*[npde.Dense(dims[i], dims[i + 1], acts[i]) for i in range(len(sizes))], npde.Dense(sizes[-1], 1)))
        rep = npde.symbolic_discretize(sysm, disc)
        eng, th = rep.engine, np.asarray(rep.flat_init_params, dtype=np.float64)
        if setup == "sampler":
            eng.set_sampler(0, np.zeros(1, dtype=np.float32), np.ones(1, dtype=np.float32), 11, seed=3, kind=1)
    before = eng.loss_grad(th)
    with pytest.raises(npde.EngineError, match=words):
        eng.hmc_chains_init(th[None], 0.01, np.ones(eng.K))
    with pytest.raises(npde.EngineError, match="pinn_hmc_chains_init first"):
        eng.hmc_chains_draws(1, np.zeros((1, 1, eng.P)))
    if setup != "sampler":       # (a redrawn set differs from evaluation to evaluation)
        after = eng.loss_grad(th)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_api(npde, lib):
    from neuralpde_jl_amd import bpinn
    rep, _, _, th0, stds, nn, priors = problem(npde, "a")
    eng = rep.engine
    before = eng.loss_grad(th0[0])

    def refused(what, *a, **kw):
        with pytest.raises(npde.EngineError, match=what):
            eng.hmc_chains_init(*a, **kw)
    refused("nchains", np.zeros((0, eng.P)), 0.01, stds)
    refused("nchains", np.tile(th0[0], (1025, 1)), 0.01, stds)
    refused("eps", th0, 0.0, stds)
    refused("inverse metric", th0, 0.01, stds, inv_metric=np.zeros(eng.P))
    refused("standard deviations", th0, 0.01, -stds)
    refused("n_leapfrog", th0, 0.01, stds, n_leapfrog=0)
    eng.hmc_chains_init(th0, 0.01, stds)
    with pytest.raises(npde.EngineError, match="ndraws"):
        eng.hmc_chains_draws(0)
    eng.set_option("precision", "f64")
    refused("float64", th0, 0.01, stds)
    eng.set_option("precision", "f32")
    after = eng.loss_grad(th0[0])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    sysm, disc = poisson1d(npde, npde.Chain(npde.Dense(1, 6, "tanh"), npde.Dense(6, 1)))
    kw = dict(draw_samples=40, n_leapfrog=3, bcstd=(0.3,), phystd=(0.5,), seed=3)
    with pytest.raises(ValueError, match="chains"):
        bpinn.ahmc_bayesian_pinn_pde(npde, sysm, disc, nchains=2, sampler="device", **kw)
    with pytest.raises(ValueError, match="nuts"):
        bpinn.ahmc_bayesian_pinn_pde(npde, sysm, disc, nchains=2, sampler="chains", kernel="nuts", **kw)
    with pytest.raises(ValueError, match="\"host\" or \"device\""):
        bpinn.ahmc_bayesian_pinn_pde(npde, sysm, disc, sampler="gpu", **kw)
    sol = bpinn.ahmc_bayesian_pinn_pde(npde, sysm, disc, nchains=3, sampler="chains", **kw)
    assert sol.chain_samples.shape == (3, 36, 19) and sol.samples.shape == (108, 19) and sol.stats["acceptance"].shape == (3, 36)
    assert np.all(np.isfinite(sol.ensemblesol[0])) and np.all(np.isfinite(sol.ensemblestd[0])) and np.all(np.isfinite(sol.samples))
