"""Resident HMC (`pinn_hmc_*`): the transition loop of `bpinn._hmc` / `logp_grad` with the chain on the device.

The reference throughout is `restate` below: a numpy restatement of the inner loop of `bpinn._hmc` and of `logp_grad` in
`ahmc_bayesian_pinn_pde`, driven by the SAME handle's `loglik_grad_f64` (one host round trip per leapfrog step) — never the code under test.

Every body is written once as a function of `npde` and exposed twice: on the CPU through the g++ emulation (`use_emu`) and, marked `gpu`,
on the product library (`hip_lib`).

Problems (the smallest that cross the kernels' boundaries): the 1-D Poisson problem u'' = -pi^2 sin(pi x), u(0) = u(1) = 0 on GridTraining(0.1)
(11 + 1 + 1 points), Dense 1 -> 16 -> 16 -> 1 tanh: P = 321 = one 256-thread block + a second that ends on a partial wave; the inverse problem
u'' = -p sin(pi x) with one estimated parameter and one DataLoss term (P = 322, K = 4).

THE BAR.  Device and restatement differ in the order of the energy sums (kinetic energy, prior sum of squares) and in the last place of
library log / exp / cos; the elementwise update arithmetic is restated operation by operation.  The restatement's own sensitivity to that is
measured by running it twice, its energy sums in forward and in reversed order: s = the largest max-norm relative difference over samples,
logp and accept_prob of the two runs.  That measurement is quantised: a = exp(H_old - H_new) with |H| ~ 1.5e3 here, so reordering a sum
either leaves H bit-equal (s = 0, most runs) or moves it by one unit in its last place, which moves a by ulp(H) = 2^-52 |H| relative
(s = 1.9e-13, some runs; both were seen on the CPU).  The bar therefore floors s at its own resolution q = 2^-52 max|H| (|H| from the
restatement):  bar = min(1e-9, 100 * max(s, q)),  3.4e-11 for these problems.  All errors are max-norm relative per output array (an
array's entries share one scale: the a's of a chain, the logp's, a sample row's weights).  Measured figures: profiles/resident_hmc.txt."""
import ctypes as C

import numpy as np
import pytest
import sympy as sp

EPS64 = 2.0 ** -52
PRECISIONS = ("f64", "f32")


# ------------------------------------------------------------------------------------------------------------------------------------
# problems
# ------------------------------------------------------------------------------------------------------------------------------------
def chain16(npde):
    return npde.Chain(npde.Dense(1, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))


def forward_problem(npde, precision, seed=7):
    """-> (engine, theta0, stds, nn, priors); the handle is kept alive by the returned representation"""
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.pi ** 2 * sp.sin(sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = chain16(npde)
    theta0 = npde.initialparameters(np.random.default_rng(seed), chain)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta0, precision=precision))
    th = np.asarray(rep.flat_init_params, dtype=np.float64).copy()
    assert rep.engine.P == 321 and rep.engine.K == 3
    return rep, th, np.array([0.5, 0.3, 0.3]), 321, []


def inverse_problem(npde, precision, prior, seed=7):
    from neuralpde_jl_amd import bpinn
    (x,) = npde.parameters("x")
    (p,) = npde.parameters("p")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + p * sp.sin(sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)], ps=[p], defaults={p: 4.0})
    chain = chain16(npde)
    theta0 = npde.initialparameters(np.random.default_rng(seed), chain)
    xs = np.linspace(0.05, 0.95, 7)
    disc = npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta0, param_estim=True,
                                  data_loss=[npde.DataLoss(u(x), xs[None, :], np.sin(np.pi * xs))], precision=precision)
    rep = npde.symbolic_discretize(sysm, disc)
    assert rep.engine.P == 322 and rep.engine.K == 4
    pr = bpinn.LogNormal(2.0, 0.5) if prior == "lognormal" else bpinn.Normal(9.0, 2.0)
    th = np.asarray(rep.flat_init_params, dtype=np.float64).copy()
    th[321] = pr.params()[0]
    return rep, th, np.array([0.5, 0.3, 0.3, 0.2]), 321, [pr]


NN_PRIOR = (0.0, 2.0)


def kinds_of(priors):
    from neuralpde_jl_amd import bpinn
    return [(1 if isinstance(q, bpinn.LogNormal) else 0,) + tuple(q.params()) for q in priors]


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement (bpinn.py: logp_grad of ahmc_bayesian_pinn_pde, the draw loop of _hmc); `rev`: energy sums in reversed order
# ------------------------------------------------------------------------------------------------------------------------------------
def make_logp(eng, stds, nn, priors, rev=False):
    mu0, sd0 = NN_PRIOR
    sm = (lambda v: np.sum(v[::-1])) if rev else np.sum

    def logp_grad(th):
        ll, g, _ = eng.loglik_grad_f64(th, stds)
        g = g.astype(np.float64)
        w = th[:nn]
        lp = ll - 0.5 * sm(((w - mu0) / sd0) ** 2) - nn * (np.log(sd0) + 0.5 * np.log(2 * np.pi))
        g[:nn] -= (w - mu0) / sd0 ** 2
        for j, pr in enumerate(priors):
            l, d = pr.logpdf_grad(float(th[nn + j]))
            lp += l
            g[nn + j] += d
        return lp, g
    return logp_grad, sm


def restate(eng, stds, nn, priors, th0, minv, momenta, uniforms, n_leapfrog, eps, rev=False, state=None):
    """-> samples, logp, accept_prob, h_new per draw, final state (th, lp, g)"""
    logp_grad, sm = make_logp(eng, stds, nn, priors, rev)
    if state is None:
        th = th0.astype(np.float64).copy()
        lp, g = logp_grad(th)
    else:
        th, lp, g = state
    S, L, A, HN = [], [], [], []
    with np.errstate(all="ignore"):
        for r, u in zip(momenta, uniforms):
            h_old = -lp + 0.5 * sm(minv * r * r)
            tn, rn, gn = th, r + 0.5 * eps * g, g
            for s in range(n_leapfrog):
                tn = tn + eps * minv * rn
                lpn, gn = logp_grad(tn)
                rn = rn + (eps if s < n_leapfrog - 1 else 0.5 * eps) * gn
            h_new = -lpn + 0.5 * sm(minv * rn * rn)
            a = float(np.exp(min(0.0, h_old - h_new))) if np.isfinite(h_new) else 0.0
            if u < a:
                th, lp, g = tn, lpn, gn
            S.append(th.copy()); L.append(lp); A.append(a); HN.append(h_new)
    return np.asarray(S), np.asarray(L), np.asarray(A), np.asarray(HN), (th, lp, g)


def relerr(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.max(np.abs(ref)))
    return float(np.max(np.abs(x - ref))) / scale if scale > 0 else float(np.max(np.abs(x)))


def compare(got, ref):
    """largest max-norm relative error over (samples, logp, accept_prob)"""
    return max(relerr(g, r) for g, r in zip(got[:3], ref[:3]))


def bar_of(eng, stds, nn, priors, th0, minv, mom, uni, n_leapfrog, eps):
    fwd = restate(eng, stds, nn, priors, th0, minv, mom, uni, n_leapfrog, eps)
    bwd = restate(eng, stds, nn, priors, th0, minv, mom, uni, n_leapfrog, eps, rev=True)
    sens = compare(bwd, fwd)
    h = np.concatenate([fwd[3][np.isfinite(fwd[3])], fwd[1][np.isfinite(fwd[1])]])
    return fwd, sens, min(1e-9, 100.0 * max(sens, EPS64 * float(np.max(np.abs(h)))))


def inputs(P, ndraws, minv, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ndraws, P)) / np.sqrt(minv), rng.random(ndraws)


def metric(P, kind):
    return np.ones(P) if kind == "unit" else 0.25 + 1.5 * np.random.default_rng(5).random(P)


EPS_STEP = 2.0e-2          # steps at which the a's of these chains are neither all 0 nor all 1 (looked at on the CPU): 1 and 2 leapfrog steps,
EPS_LONG = 1.0e-2          # 5 leapfrog steps


def draws(eng, *args):
    """Engine.hmc_draws in the restatement's order: (samples, logp, accept_prob)"""
    smp, acc, lp = eng.hmc_draws(*args)
    return smp, lp, acc


# ------------------------------------------------------------------------------------------------------------------------------------
# bodies
# ------------------------------------------------------------------------------------------------------------------------------------
def body_trajectory_parity(npde, precision, metric_kind, n_leapfrog):
    """cases 1 (float64 mode) and 5 (fp32 mode): supplied momenta and uniforms, samples / logp / accept_prob against the restatement"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    minv = metric(eng.P, metric_kind)
    mom, uni = inputs(eng.P, 5, minv, 11 + n_leapfrog)
    eps = EPS_LONG if n_leapfrog == 5 else EPS_STEP
    ref, sens, bar = bar_of(eng, stds, nn, priors, th0, minv, mom, uni, n_leapfrog, eps)
    eng.hmc_init(th0, stds, NN_PRIOR, kinds_of(priors))
    eng.hmc_set_metric(None if metric_kind == "unit" else minv)
    got = draws(eng, 5, n_leapfrog, eps, 0, mom, uni)
    err = compare(got, ref)
    print(f"resident hmc parity [{precision} {metric_kind} L={n_leapfrog}]: err {err:.3e}  sensitivity {sens:.3e}  bar {bar:.3e}  a = {np.round(ref[2], 4)}")
    assert 0.0 < ref[2].min() and ref[2].max() <= 1.0
    assert err <= bar
    th, lp, g = eng.hmc_get()
    assert relerr(th, ref[4][0]) <= bar and relerr(lp, ref[4][1]) <= bar and relerr(g, ref[4][2]) <= bar


def body_metropolis_branches(npde, precision):
    """case 2: u = 0 accepts every finite proposal, u = 1 rejects every proposal"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    minv = np.ones(eng.P)
    mom, _ = inputs(eng.P, 4, minv, 21)
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    _, lp0, _ = eng.hmc_get()
    smp, acc, lp = eng.hmc_draws(4, 2, EPS_STEP, 0, mom, np.ones(4))
    assert np.all(acc <= 1.0) and np.all(smp == th0[None, :]) and np.all(lp == lp0)
    th, lpg, _ = eng.hmc_get()
    assert np.array_equal(th, th0) and lpg == lp0
    ref = restate(eng, stds, nn, priors, th0, minv, mom, np.zeros(4), 2, EPS_STEP)
    smp, acc, lp = eng.hmc_draws(4, 2, EPS_STEP, 0, mom, np.zeros(4))
    assert np.all(acc > 0.0) and np.all(np.isfinite(lp))
    assert all(not np.array_equal(smp[i], smp[i - 1] if i else th0) for i in range(4))          # every proposal was taken
    assert compare((smp, lp, acc), ref) <= 1e-9 and np.array_equal(ref[0][-1], ref[4][0])


EPS_DIVERGENT = 50.0       # one leapfrog step of this size: the restatement's H_new is +inf or a underflows to 0 (checked on the CPU)


def body_divergent(npde, precision):
    """case 3: a divergent proposal is rejected with a == 0, leaves every output finite and the state untouched; the next draw is normal"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    minv = np.ones(eng.P)
    mom, uni = inputs(eng.P, 3, minv, 31)
    bad = restate(eng, stds, nn, priors, th0, minv, mom[:1], uni[:1], 3, EPS_DIVERGENT)
    assert bad[2][0] == 0.0, (bad[2], bad[3])
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    _, lp0, g0 = eng.hmc_get()
    smp, acc, lp = eng.hmc_draws(1, 3, EPS_DIVERGENT, 0, mom[:1], uni[:1])
    assert acc[0] == 0.0 and np.array_equal(smp[0], th0) and lp[0] == lp0
    th, lpg, g = eng.hmc_get()
    assert np.array_equal(th, th0) and lpg == lp0 and np.array_equal(g, g0) and np.all(np.isfinite(g))
    ref, sens, bar = bar_of(eng, stds, nn, priors, th0, minv, mom[1:], uni[1:], 2, EPS_STEP)
    got = draws(eng, 2, 2, EPS_STEP, 0, mom[1:], uni[1:])
    assert all(np.all(np.isfinite(q)) for q in got)
    assert compare(got, ref) <= bar


def body_priors(npde, precision, prior):
    """case 4: the inverse problem under a Normal / LogNormal parameter prior; draw 1's momentum carries the parameter below zero"""
    rep, th0, stds, nn, priors = inverse_problem(npde, precision, prior)
    eng = rep.engine
    minv = np.ones(eng.P)
    mom, uni = inputs(eng.P, 4, minv, 41)
    mom[1, nn] = -(abs(th0[nn]) + 25.0) / EPS_STEP
    uni[1] = 0.0                                          # (accepted whenever a > 0: only a == 0 rejects it)
    ref, sens, bar = bar_of(eng, stds, nn, priors, th0, minv, mom, uni, 1, EPS_STEP)
    eng.hmc_init(th0, stds, NN_PRIOR, kinds_of(priors))
    got = draws(eng, 4, 1, EPS_STEP, 0, mom, uni)
    err = compare(got, ref)
    print(f"resident hmc priors [{precision} {prior}]: err {err:.3e}  sensitivity {sens:.3e}  bar {bar:.3e}  a = {ref[2]}")
    if prior == "lognormal":
        assert ref[2][1] == 0.0 and ref[3][1] == np.inf and got[2][1] == 0.0 and np.array_equal(got[0][1], got[0][0])
    assert np.all(got[0][:, nn] > 0.0) or prior == "normal"
    assert err <= bar


# ---- the generator of include/pinn_hip.h, restated ----
M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def gen_draw(seed, counter, P):
    """-> (z [P], u) of draw `counter`"""
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    base = mix32((lo + np.uint64(0x9E3779B9) * hi) & M32)
    key = mix32(base ^ ((np.uint64(counter) * np.uint64(0x85EBCA6B) + np.uint64(0xC2B2AE35)) & M32))
    e = np.arange(P + 1, dtype=np.uint64)
    word = lambda j: mix32(key ^ mix32(((np.uint64(2) * e + np.uint64(j)) * np.uint64(0x9E3779B9) + np.uint64(0x165667B1)) & M32))
    w0, w1 = word(0).astype(np.float64), word(1).astype(np.float64)
    z = np.sqrt(-2.0 * np.log((w0[:P] + 1.0) / 4294967296.0)) * np.cos(6.283185307179586 * (w1[:P] / 4294967296.0))
    return z, float(w0[P] / 4294967296.0)


GEN_SEED = (2 ** 40) + 12345


def body_generator(npde, precision):
    """case 6: the chain drawn on the device from `seed` against the restatement fed with the restated generator's momenta / uniforms"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    minv = metric(eng.P, "nonunit")
    zs, us = zip(*[gen_draw(GEN_SEED, c, eng.P) for c in range(5)])
    mom, uni = np.asarray(zs) / np.sqrt(minv), np.asarray(us)
    assert abs(mom.mean()) < 0.2 and 0.7 < (mom * np.sqrt(minv)).std() < 1.3 and np.all((uni >= 0) & (uni < 1))
    ref, sens, bar = bar_of(eng, stds, nn, priors, th0, minv, mom, uni, 2, EPS_STEP)
    assert np.all(np.abs(ref[2] - uni) > 1e-6), (ref[2], uni)          # no accept decision on the edge for this seed
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.hmc_set_metric(minv)
    got = draws(eng, 5, 2, EPS_STEP, GEN_SEED)
    err = compare(got, ref)
    print(f"resident hmc generator [{precision}]: err {err:.3e}  sensitivity {sens:.3e}  bar {bar:.3e}  a = {np.round(ref[2], 4)} u = {np.round(uni, 4)}")
    assert err <= bar
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.hmc_set_metric(minv)
    other = draws(eng, 5, 2, EPS_STEP, GEN_SEED + 1)
    assert not np.array_equal(other[0], got[0]) and not np.array_equal(other[2], got[2])


def body_chunking(npde, precision):
    """case 7: 2 + 3 draws == 5 draws, and two fresh handles agree, bit for bit"""
    outs = []
    for split in ((5,), (2, 3), (5,)):
        rep, th0, stds, nn, priors = forward_problem(npde, precision)
        eng = rep.engine
        eng.hmc_init(th0, stds, NN_PRIOR, [])
        parts = [eng.hmc_draws(n, 2, EPS_STEP, 99) for n in split]
        outs.append([np.concatenate([q[i] for q in parts]) for i in range(3)] + list(eng.hmc_get()))
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    assert len(set(map(float, outs[0][2]))) > 1


def body_isolation(npde, precision):
    """case 8: an evaluation and an Adam run between two hmc_draws calls leave the chain alone, and the draws leave the Adam iterate alone"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    whole = eng.hmc_draws(5, 2, EPS_STEP, 5)
    rep2, _, _, _, _ = forward_problem(npde, precision)
    e2 = rep2.engine
    e2.hmc_init(th0, stds, NN_PRIOR, [])
    first = e2.hmc_draws(2, 2, EPS_STEP, 5)
    other = th0 + 0.1
    e2.loss_grad_f64(other)
    adam = e2.adam_f64 if precision == "f64" else e2.adam
    get = e2.adam_get_f64 if precision == "f64" else e2.adam_get
    it0, _ = adam(other, 3, 1e-3)
    second = e2.hmc_draws(3, 2, EPS_STEP, 5)
    assert np.array_equal(get(), it0)
    for i in range(3):
        assert np.array_equal(np.concatenate([first[i], second[i]]), whole[i])


def small_problem(npde):
    """the smallest tanh problem: Dense 1 -> 2 -> 1, the value-only equation u(x) ~ 2 x + 1 on 11 points and u(0) ~ 1 (P = 7)"""
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    sysm = npde.PDESystem([npde.Eq(u(x), 2 * x + 1)], [npde.Eq(u(0.0), 1.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 2, "tanh"), npde.Dense(2, 1))
    theta0 = npde.initialparameters(np.random.default_rng(2), chain)
    return sysm, chain, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta0, precision="f64")


def body_known_target(npde):
    """case 9.  The engine does not plan a chain of ONE Dense layer (`Chain`: "the HIP engine needs at least one hidden layer"; confirmed
    below), so the closed-form Gaussian target is not available and the issue's alternative applies: the device sampler against the host
    `_hmc` on the smallest tanh problem, 2,000 draws x 5 steps each through ahmc_bayesian_pinn_pde.  The weights' posterior is multimodal
    (hidden-unit symmetries), so the compared quantity is the posterior of the PREDICTION u(x) at x = 0, 0.5, 1, which is not: mean within
    0.25 sd and sd within 25 % of the other sampler's (the bars of tests/test_host_logic.py::test_hmc_sampler_on_a_gaussian), acceptance
    in (0.6, 1].  Both chains are seeded: the outcome is deterministic.  Weight prior N(0, 1): under N(0, 2) this posterior mixes so slowly
    that 2,000-draw chains of the HOST sampler differ from one another by more than these bars (u(1) = 2.75 ... 2.91 over three seeds,
    sd 0.33), which would test the seed; under N(0, 1) three host and three device seeds agree to 0.05 (looked at on the CPU)."""
    with pytest.raises(ValueError, match="hidden layer"):
        npde.Chain(npde.Dense(1, 1))
    sysm, chain, disc = small_problem(npde)
    kw = dict(draw_samples=2000, n_leapfrog=5, phystd=[0.5], bcstd=[0.5], priorsNNw=(0.0, 1.0))
    dev = npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", seed=3, **kw)
    host = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(4), **kw)
    assert dev.stats["sampler"] == "device" and dev.samples.shape == (2000, 7) and dev.stats["n_adapts"] == 200
    xs = np.array([0.0, 0.5, 1.0])

    def predict(sol):
        S = sol.samples[500:]
        W1, b1, W2, b2 = S[:, 0:2], S[:, 2:4], S[:, 4:6], S[:, 6]
        return np.stack([np.sum(W2 * np.tanh(W1 * x + b1), axis=1) + b2 for x in xs], axis=1)

    pd_, ph = predict(dev), predict(host)
    acc = dev.stats["acceptance"][200:].mean()
    print(f"resident hmc known target: u(0, .5, 1) device mean {pd_.mean(axis=0)} sd {pd_.std(axis=0)}; host mean {ph.mean(axis=0)} sd {ph.std(axis=0)}; "
          f"acceptance device {acc:.3f} host {host.stats['acceptance'][200:].mean():.3f}")
    assert np.all(np.abs(pd_.mean(axis=0) - ph.mean(axis=0)) < 0.25 * np.minimum(pd_.std(axis=0), ph.std(axis=0)))
    assert np.all(np.abs(pd_.std(axis=0) / ph.std(axis=0) - 1.0) < 0.25)
    assert 0.6 < acc <= 1.0


def body_refusals(npde, precision):
    """case 10: every refusal is named and leaves the handle evaluating as before"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    L, dp = eng.L, C.POINTER(C.c_double)
    ev0 = eng.loglik_grad_f64(th0, stds)
    acc, lp, smp = np.zeros(4), np.zeros(4), np.zeros((4, eng.P))
    ptr = lambda a: a.ctypes.data_as(dp)

    def refused(rc, *words):
        assert rc != 0
        msg = L.last_error()
        assert all(w in msg for w in words), msg
        ev = eng.loglik_grad_f64(th0, stds)
        assert ev[0] == ev0[0] and np.array_equal(ev[1], ev0[1])

    draws = lambda nd, nl, eps, p=eng.P: L.lib.pinn_hmc_draws(eng.h, nd, nl, eps, 0, None, None, ptr(smp), p, ptr(acc), ptr(lp))
    init = lambda p, sd, nn_sd=2.0: L.lib.pinn_hmc_init(eng.h, ptr(th0), p, ptr(sd), sd.size, 0.0, nn_sd, 0, None, None, None)
    refused(draws(1, 1, 0.1), "pinn_hmc_draws", "pinn_hmc_init first")
    refused(L.lib.pinn_hmc_set_metric(eng.h, None, eng.P), "pinn_hmc_set_metric", "pinn_hmc_init first")
    refused(L.lib.pinn_hmc_get(eng.h, ptr(smp), eng.P, None, None), "pinn_hmc_get", "pinn_hmc_init first")
    refused(init(eng.P - 1, stds), "pinn_hmc_init", "ntheta")
    refused(init(eng.P, stds[:2].copy()), "pinn_hmc_init", "standard deviations for 3 loss terms")
    refused(init(eng.P, np.array([0.5, 0.0, 0.3])), "pinn_hmc_init", "must be positive")
    refused(init(eng.P, stds, 0.0), "pinn_hmc_init", "weight prior")
    eng.comm_init_custom(1, 0, lambda buf, count, dtype, stream: 0)
    refused(init(eng.P, stds), "pinn_hmc_init", "communicator")
    eng.comm_destroy()
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    ref = eng.hmc_get()
    refused(draws(0, 1, 0.1), "ndraws")
    refused(draws(1, 0, 0.1), "n_leapfrog")
    refused(draws(1, 1, 0.0), "eps")
    refused(draws(1, 1, -1.0), "eps")
    refused(draws(1, 1, 0.1, eng.P + 1), "ntheta")
    refused(L.lib.pinn_hmc_set_metric(eng.h, ptr(np.zeros(eng.P)), eng.P), "inverse metric")
    eng.comm_init_custom(1, 0, lambda buf, count, dtype, stream: 0)
    refused(draws(1, 1, 0.1), "communicator")
    eng.comm_destroy()
    eng.set_sampler(0, [0.0], [1.0], 11, seed=1)
    ev0 = eng.loglik_grad_f64(th0, stds)
    refused(draws(1, 1, 0.1), "pinn_hmc_draws", "fixed")
    refused(init(eng.P, stds), "pinn_hmc_init", "fixed")
    now = eng.hmc_get()
    assert all(np.array_equal(a, b) for a, b in zip(now, ref))          # the chain itself is where it was


def body_mirror(npde):
    """case 11: sampler="host" is the default path; an unknown sampler is a ValueError"""
    sysm, chain, disc = small_problem(npde)
    kw = dict(draw_samples=20, n_leapfrog=3, phystd=[0.5], bcstd=[0.5])
    a = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), **kw)
    b = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), sampler="host", **kw)
    assert np.array_equal(a.samples, b.samples) and b.stats["sampler"] == "host"
    assert set(a.stats) >= {"acceptance", "step_size", "inv_metric", "n_adapts", "sampler"}
    with pytest.raises(ValueError):
        npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="gpu", **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# the two faces of every body
# ------------------------------------------------------------------------------------------------------------------------------------
PARITY = [(p, m, n) for p in PRECISIONS for m in ("unit", "nonunit") for n in (1, 2, 5)]


@pytest.mark.parametrize("precision,metric_kind,n_leapfrog", PARITY)
def test_trajectory_parity(npde, use_emu, precision, metric_kind, n_leapfrog):
    body_trajectory_parity(npde, precision, metric_kind, n_leapfrog)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,metric_kind,n_leapfrog", PARITY)
def test_trajectory_parity_gpu(npde, hip_lib, precision, metric_kind, n_leapfrog):
    body_trajectory_parity(npde, precision, metric_kind, n_leapfrog)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_metropolis_branches(npde, use_emu, precision):
    body_metropolis_branches(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_metropolis_branches_gpu(npde, hip_lib, precision):
    body_metropolis_branches(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_divergent_proposal(npde, use_emu, precision):
    body_divergent(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_divergent_proposal_gpu(npde, hip_lib, precision):
    body_divergent(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("prior", ("normal", "lognormal"))
def test_parameter_priors(npde, use_emu, precision, prior):
    body_priors(npde, precision, prior)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("prior", ("normal", "lognormal"))
def test_parameter_priors_gpu(npde, hip_lib, precision, prior):
    body_priors(npde, precision, prior)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_generator(npde, use_emu, precision):
    body_generator(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_generator_gpu(npde, hip_lib, precision):
    body_generator(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_and_reproducibility(npde, use_emu, precision):
    body_chunking(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_and_reproducibility_gpu(npde, hip_lib, precision):
    body_chunking(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_isolation(npde, use_emu, precision):
    body_isolation(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_isolation_gpu(npde, hip_lib, precision):
    body_isolation(npde, precision)


def test_known_target(npde, use_emu):
    body_known_target(npde)


@pytest.mark.gpu
def test_known_target_gpu(npde, hip_lib):
    body_known_target(npde)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(npde, use_emu, precision):
    body_refusals(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_gpu(npde, hip_lib, precision):
    body_refusals(npde, precision)


def test_mirror(npde, use_emu):
    body_mirror(npde)


@pytest.mark.gpu
def test_mirror_gpu(npde, hip_lib):
    body_mirror(npde)
