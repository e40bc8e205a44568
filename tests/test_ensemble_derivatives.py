"""Device ensemble derivatives (`pinn_derivative_ensemble`): derivatives of one network's trial function at S parameter vectors
and n points, and the mean and standard deviation over the S predictions per request, in one call.

The reference throughout is the float64 oracle's `po.exact_derivative` (nested autograd) per sample on the SAME `thetas` and `pts`, then
`mean(axis=0)` and `std(axis=0, ddof=ddof)` — never the engine's own `preds`.  The error measure per request, over `preds`, `mean` and `std`, is
max|got - ref| / max(1, max|ref|) (the measure of tests/test_ensemble_prediction.py).  Bars: 1e-11 on a handle in float64 mode; 1e-5 on an fp32
handle for orders <= 2; for orders 3 and 4 on an fp32 handle max(1e-5, 4 x the error of the existing per-sample `pinn_derivative` on the same
handle, thetas and points against the same oracle) — the factor 4 allows for a different but equally long summation order.  Both numbers are
printed.  (That per-sample reference is the one slow step of this file: for a shape outside the ahead-of-time table — the sigmoid 2-40-40-40-1,
the tanh/sigmoid mix and 3-64-64-1 on an fp32 handle — the first `pinn_derivative` of order 3 / 4 specialises a kernel at run time, tens of
seconds with an empty kernel cache and nothing after; `pinn_derivative_ensemble` itself needs no specialisation for any shape.)

Every body is written once as a function of `npde` and exposed twice: on the CPU through the g++ emulation (`use_emu`) and, marked `gpu`, on
the product library (`hip_lib`).  Handles and references are built once per (chain, precision) and shared by the cases."""
import ctypes as C
import os
from contextlib import contextmanager

import numpy as np
import pytest
import sympy as sp
import torch

import pinn_oracle as po

PRECISIONS = ("f64", "f32")
BAR = {"f64": 1e-11, "f32": 1e-5}
N_POINTS = (1, 63, 64, 65, 130)            # one lane, a ragged wave, one full block, a second block, a ragged last block
SAMPLE_CASES = ((1, 0), (2, 0), (5, 1))    # (S, ddof)

# name -> (sizes, activation per hidden layer)
CHAINS = {
    "1-6-1": ((1, 6, 1), "tanh"),
    "2-16-16-1": ((2, 16, 16, 1), "tanh"),
    "2-40x3-1": ((2, 40, 40, 40, 1), "sigmoid"),
    "sin": ((2, 16, 16, 1), "sin"),
    "swish": ((2, 16, 16, 1), "swish"),
    "mix": ((2, 16, 16, 1), ("tanh", "sigmoid")),
    "3-64-64-1": ((3, 64, 64, 1), "tanh"),       # float64 mode, C >= 3: two images of 64 points exceed the LDS -> the scratch storage by itself
    "1-16-16-1": ((1, 16, 16, 1), "tanh"),       # (the storage / point-pass comparisons)
}
PARITY = ("1-6-1", "2-16-16-1", "2-40x3-1", "sin", "swish", "mix", "3-64-64-1")


@pytest.fixture(autouse=True)
def _oracle_knows_swish(monkeypatch):
    """the oracle looks activations up in pinn_oracle.ACTS at call time and has no swish: registered for the duration of a test (as tests/test_swish.py)"""
    monkeypatch.setitem(po.ACTS, "swish", lambda z: z * torch.sigmoid(z))


def requests_for(d):
    """orders 0..4 along axis 0, orders 1 and 2 along the last axis, the mixed (0, 1) where d >= 2"""
    r = [(k, (0,) * k) for k in range(5)]
    if d >= 2:
        r += [(1, (d - 1,)), (2, (d - 1, d - 1)), (2, (0, 1))]
    return r


def acts_of(name):
    sizes, act = CHAINS[name]
    return [act] * (len(sizes) - 2) if isinstance(act, str) else list(act)


def make_chain(npde, name):
    sizes, _ = CHAINS[name]
    kinds = acts_of(name) + ["identity"]
    return npde.Chain(*[npde.Dense(sizes[l], sizes[l + 1], kinds[l]) if kinds[l] != "identity" else npde.Dense(sizes[l], sizes[l + 1]) for l in range(len(sizes) - 1)])


def theta_for(sizes, seed):
    return po.glorot_theta(po.Chain(tuple(sizes), "tanh"), np.random.default_rng(seed)).astype(np.float64)


_U = lambda cord, th, phi: phi(cord, th)


def oracle_derivative(sizes, kinds, theta, pts, axes):
    """float64 oracle: d^k phi / dx_axes at the columns of pts (d x N) -> (N,)"""
    chain = po.Chain(tuple(sizes), ",".join(kinds))
    th = torch.tensor(np.asarray(theta[:chain.nparams], dtype=np.float64), dtype=po.DT)
    return po.exact_derivative(chain, _U, torch.tensor(np.asarray(pts, dtype=np.float64), dtype=po.DT), list(axes), th).detach().numpy().reshape(-1)


def err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref))) / max(1.0, float(np.max(np.abs(ref))))


def value_problem(npde, chains, precision, ps=False):
    """a handle whose networks are `chains` (all of d inputs): one value-only equation per network (u_k(x..) ~ x_0 [* p]), one boundary value"""
    d = chains[0].sizes[0]
    xs = npde.parameters(" ".join("xyz"[:d]))
    us = npde.variables(" ".join(f"u{k}" for k in range(len(chains))))
    kw = {}
    rhs = xs[0]
    if ps:
        (p,) = npde.parameters("p")
        rhs, kw = p * xs[0], dict(ps=[p], defaults={p: 2.0})
    eqs = [npde.Eq(u(*xs), rhs) for u in us]
    zero = [0.0] * d
    bcs = [npde.Eq(u(*zero), 0.0) for u in us]
    sysm = npde.PDESystem(eqs, bcs, [npde.In(x, npde.Interval(0.0, 1.0)) for x in xs], list(xs), [u(*xs) for u in us], **kw)
    rng = np.random.default_rng(5)
    init = [npde.initialparameters(rng, c) for c in chains]
    disc = npde.PhysicsInformedNN(chains if len(chains) > 1 else chains[0], npde.GridTraining(0.5), init_params=init if len(chains) > 1 else init[0],
                                  param_estim=ps, precision=precision)
    return npde.symbolic_discretize(sysm, disc)


_CACHE = {}
_REF = {}


def reference(name):
    """-> (thetas (5 x P), pts (d x 130), requests, ref (R x 5 x 130)); the oracle once per chain, shared by both precisions and libraries"""
    if name not in _REF:
        sizes = CHAINS[name][0]
        rng = np.random.default_rng(11)
        P = len(theta_for(sizes, 0))
        thetas = np.stack([theta_for(sizes, 100 + s) * (1.0 + 0.1 * rng.standard_normal(P)) for s in range(5)])
        pts = rng.uniform(-1.0, 1.0, size=(sizes[0], max(N_POINTS)))
        reqs = requests_for(sizes[0])
        ref = np.stack([np.stack([oracle_derivative(sizes, acts_of(name), th, pts, ax) for th in thetas]) for _, ax in reqs])
        ref.setflags(write=False)
        _REF[name] = (thetas, pts, reqs, ref)
    return _REF[name]


def problem(npde, name, precision):
    key = (id(npde._lib.default_library()), name, precision)
    if key not in _CACHE:
        _CACHE[key] = value_problem(npde, [make_chain(npde, name)], precision)
        assert _CACHE[key].engine.P == reference(name)[0].shape[1]
    return (_CACHE[key],) + reference(name)


@contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. parity grid
# ------------------------------------------------------------------------------------------------------------------------------------
def body_parity(npde, name, precision):
    rep, thetas, pts, reqs, ref = problem(npde, name, precision)
    eng = rep.engine
    bars = [BAR[precision]] * len(reqs)
    if precision == "f32":                               # orders 3 and 4: the bar follows the existing per-sample closure's own error
        for j, (o, ax) in enumerate(reqs):
            if o >= 3:
                single = err(np.stack([eng.derivative(0, th, pts, ax) for th in thetas]), ref[j])
                bars[j] = max(1e-5, 4.0 * single)
                print(f"ensemble derivatives {name} f32 order {o}: per-sample pinn_derivative error {single:.2e} -> bar {bars[j]:.2e}")
    worst = [0.0] * len(reqs)
    for n in N_POINTS:
        for S, ddof in SAMPLE_CASES:
            mean, std, preds = eng.derivative_ensemble(0, thetas[:S], pts[:, :n], reqs, ddof=ddof, return_preds=True)
            assert preds.shape == (len(reqs), S, n) and mean.shape == std.shape == (len(reqs), n)
            for j, (o, ax) in enumerate(reqs):
                r = ref[j, :S, :n]
                e = (err(preds[j], r), err(mean[j], r.mean(axis=0)), err(std[j], r.std(axis=0, ddof=ddof)))
                worst[j] = max(worst[j], *e)
                print(f"ensemble derivatives {name} {precision} n={n} S={S} ddof={ddof} order {o} axes {ax}: preds {e[0]:.2e} mean {e[1]:.2e} std {e[2]:.2e} (bar {bars[j]:.2e})")
                assert max(e) <= bars[j]
            if S == 1:
                assert np.all(std == 0.0)
            if n == 65:
                m2, s2 = eng.derivative_ensemble(0, thetas[:S], pts[:, :n], reqs, ddof=ddof)    # without preds: the same statistics
                assert np.array_equal(m2, mean) and np.array_equal(s2, std)
    for j, (o, ax) in enumerate(reqs):
        print(f"ensemble derivatives {name} {precision} order {o} axes {ax}: worst {worst[j]:.2e} (bar {bars[j]:.2e})")
    if name == "3-64-64-1":                              # 64 neurons x C >= 3 channels: every pass lands on the scratch storage by itself
        assert int(eng.get_option("ens_scratch_passes")) == int(eng.get_option("ens_passes")) == 3
    if name == "1-6-1":                                  # ... and a 6-wide network's C = 5 jet stays in LDS
        assert int(eng.get_option("ens_scratch_passes")) == 0


def body_system(npde, precision):
    """a two-network system evaluated for the SECOND network (theta_off != 0), one estimated PDE parameter trailing theta"""
    chains = [npde.Chain(npde.Dense(1, 6, "tanh"), npde.Dense(6, 1)), npde.Chain(npde.Dense(1, 16, "sigmoid"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))]
    rep = value_problem(npde, chains, precision, ps=True)
    eng = rep.engine
    s0, s1 = (1, 6, 1), (1, 16, 16, 1)
    n0, n1 = len(theta_for(s0, 0)), len(theta_for(s1, 0))
    assert eng.P == n0 + n1 + 1
    rng = np.random.default_rng(3)
    thetas = np.stack([np.concatenate([theta_for(s0, 10 + s), theta_for(s1, 20 + s), [2.0]]) * (1.0 + 0.1 * rng.standard_normal(eng.P)) for s in range(5)])
    pts = rng.uniform(-1.0, 1.0, size=(1, 65))
    reqs = [(0, ()), (1, (0,)), (2, (0, 0))]
    for net, sizes, kinds, off in ((1, s1, ["sigmoid", "tanh"], n0), (0, s0, ["tanh"], 0)):
        mean, std, preds = eng.derivative_ensemble(net, thetas, pts, reqs, ddof=1, return_preds=True)
        for j, (o, ax) in enumerate(reqs):
            ref = np.stack([oracle_derivative(sizes, kinds, th[off:], pts, ax) for th in thetas])
            e = (err(preds[j], ref), err(mean[j], ref.mean(axis=0)), err(std[j], ref.std(axis=0, ddof=1)))
            print(f"ensemble derivatives system {precision} net {net} order {o}: preds {e[0]:.2e} mean {e[1]:.2e} std {e[2]:.2e}")
            assert max(e) <= BAR[precision]


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. internal consistency: all bit-exact
# ------------------------------------------------------------------------------------------------------------------------------------
def body_consistency(npde, name, precision):
    rep, thetas, pts, reqs, _ = problem(npde, name, precision)
    eng = rep.engine
    mean, std, preds = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)
    again = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)
    assert same((mean, std, preds), again)                                   # two identical calls
    m0, s0, p0 = eng.phi_ensemble(0, thetas, pts, ddof=1, return_preds=True)
    assert reqs[0] == (0, ())
    assert np.array_equal(mean[0], m0) and np.array_equal(std[0], s0) and np.array_equal(preds[0], p0)      # channel 0 of a jet pass == the value kernel
    for j, r in enumerate(reqs):                                             # pass sharing changes nothing
        m1, s1, p1 = eng.derivative_ensemble(0, thetas, pts, [r], ddof=1, return_preds=True)
        assert np.array_equal(m1[0], mean[j]) and np.array_equal(s1[0], std[j]) and np.array_equal(p1[0], preds[j]), r
    m1, s1 = eng.derivative_ensemble(0, thetas[:1], pts, reqs)                # S = 1: std = 0 exactly
    assert np.all(s1 == 0.0) and np.array_equal(m1, preds[:, 0, :])
    one, col = eng.derivative_ensemble(0, thetas, pts[:, 0], reqs), eng.derivative_ensemble(0, thetas, pts[:, :1], reqs)      # a single point as (d,)
    assert one[0].shape == (len(reqs), 1) and same(one, col)


def body_storage(npde, name, precision):
    """the images in LDS and in the device scratch buffer ($PINN_ENS_NO_LDS=1): the same bits"""
    rep, thetas, pts, reqs, _ = problem(npde, name, precision)
    eng = rep.engine
    width, d = max(CHAINS[name][0]), CHAINS[name][0][0]
    elem = 8 if precision == "f64" else 4
    image_pair = lambda C: 2 * width * C * 64 * elem                         # bytes of two images of 64 points
    chans = (4, 5, 3) if d == 2 else (5,)                                    # the passes of requests_for(d): two-axis, line K = 4 along axis 0, line K = 2 along axis 1
    with env(PINN_ENS_NO_LDS="0"):                                           # LDS wherever two images of 64 points fit the CU's 160 KB
        a = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)
        npass = int(eng.get_option("ens_passes"))
        # (only the C = 5 line jet of 2-40-40-40-1 in float64 mode exceeds it: 200 KB; its C = 4 pass takes exactly 160 KB)
        assert npass == len(chans) and int(eng.get_option("ens_scratch_passes")) == sum(image_pair(C) > 160 * 1024 for C in chans) < npass
    with env(PINN_ENS_NO_LDS="1"):
        b = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)
        assert int(eng.get_option("ens_scratch_passes")) == npass
        with env(PINN_ENS_CHUNK="1"):                                        # ... and in several point passes
            c = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)
    assert same(a, b) and same(a, c)
    dflt = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)      # (the variable is read per call)
    # by itself a pass stays in LDS while its images leave room for 4 workgroups per CU (40 KB)
    assert int(eng.get_option("ens_scratch_passes")) == sum(image_pair(C) > 40 * 1024 for C in chans)
    assert same(a, dflt)


def body_chunks(npde, name, precision):
    """1, 2 and 3 passes over the 130 points (64 points per block with the C = 5 line jet in the table)"""
    rep, thetas, pts, reqs, _ = problem(npde, name, precision)
    eng = rep.engine
    a = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)
    assert int(eng.get_option("ens_point_passes")) == 1
    for chunk, passes in (("1", 3), ("65", 2)):
        with env(PINN_ENS_CHUNK=chunk):
            c = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)
            assert int(eng.get_option("ens_point_passes")) == passes, chunk
        assert same(a, c), chunk


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. pass grouping
# ------------------------------------------------------------------------------------------------------------------------------------
V, D0, D00, D1, D11, D01 = (0, ()), (1, (0,)), (2, (0, 0)), (1, (1,)), (2, (1, 1)), (2, (0, 1))
GROUPING = {
    "1-6-1": [([V], 0), ([D0], 1), (requests_for(1), 1), ([V, (4, (0, 0, 0, 0))], 1)],
    "2-16-16-1": [([V], 0), ([V, D0], 1), ([D0, D1], 2), ([V, D0, D00, D1, D01], 2),      # the two-axis pass serves d01, d1, d0 and the value; the K = 2 line jet d00
                  ([D01], 1), ([D01, D0, D1, V], 1), ([(2, (1, 0))], 1), (requests_for(2), 3), ([D00, D11], 2)],
    "3-64-64-1": [(requests_for(3), 3), ([D01, (2, (0, 2)), (2, (1, 2))], 3), ([D01, (1, (2,))], 2)],
}


def body_grouping(npde, name, precision):
    rep, thetas, pts, _, _ = problem(npde, name, precision)
    eng = rep.engine
    for table, passes in GROUPING[name]:
        eng.derivative_ensemble(0, thetas[:2], pts[:, :3], table)
        assert int(eng.get_option("ens_passes")) == passes, (table, eng.get_option("ens_passes"))


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. mirror
# ------------------------------------------------------------------------------------------------------------------------------------
def body_mirror(npde, precision):
    """the 13-point 1-D Poisson BPINN of tests/test_ensemble_prediction.py (1-16-16-1 tanh), 30 draws, 10 retained"""
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.pi ** 2 * sp.sin(sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    theta0 = npde.initialparameters(np.random.default_rng(7), chain)
    disc = npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta0, precision=precision)
    kw = dict(draw_samples=30, n_leapfrog=3, step_size=0.002, phystd=[0.5], bcstd=[0.3], seed=4)
    want = [("u", 1, [0]), ("u", 2, [0, 0])]
    keys = [("u", 1, (0,)), ("u", 2, (0, 0))]
    host = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), ensemble="host", ensemble_derivatives=want, **kw)
    dev = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), ensemble="device", ensemble_derivatives=want, **kw)
    assert np.array_equal(host.samples, dev.samples)
    assert sorted(host.ensemble_derivs) == sorted(dev.ensemble_derivs) == sorted(host.ensemble_derivs_std) == sorted(dev.ensemble_derivs_std) == sorted(keys)
    for k in keys:
        e = (err(dev.ensemble_derivs[k], host.ensemble_derivs[k]), err(dev.ensemble_derivs_std[k], host.ensemble_derivs_std[k]))
        print(f"ensemble derivatives mirror {precision} {k}: mean {e[0]:.2e} std {e[1]:.2e}")
        assert dev.ensemble_derivs[k].shape == host.ensemble_derivs[k].shape == (11,) and max(e) <= BAR[precision]
        assert float(np.max(host.ensemble_derivs_std[k])) > 0.0
    # the oracle on the retained draws: the host curves are what they claim to be
    ens_draws = host.samples[-11:][:10]
    for k in keys:
        ref = np.stack([oracle_derivative((1, 16, 16, 1), ["tanh", "tanh"], th, host.timepoints[0], k[2]) for th in ens_draws])
        assert err(host.ensemble_derivs[k], ref.mean(axis=0)) <= BAR[precision] and err(host.ensemble_derivs_std[k], ref.std(axis=0)) <= BAR[precision]
    # the default () changes nothing
    for mode, with_d in (("host", host), ("device", dev)):
        plain = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), ensemble=mode, **kw)
        empty = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), ensemble=mode, ensemble_derivatives=(), **kw)
        for sol in (plain, empty):
            assert not getattr(sol, "ensemble_derivs", None) and not getattr(sol, "ensemble_derivs_std", None)
            assert set(vars(sol)) == {"samples", "ensemblesol", "ensemblestd", "timepoints", "stats", "estimated_de_params"}
            assert np.array_equal(sol.samples, with_d.samples) and np.array_equal(sol.ensemblesol[0], with_d.ensemblesol[0])
            assert np.array_equal(sol.ensemblestd[0], with_d.ensemblestd[0]) and np.array_equal(sol.timepoints[0], with_d.timepoints[0])
    with pytest.raises(ValueError, match="no dependent variable"):
        npde.ahmc_bayesian_pinn_pde(sysm, disc, ensemble_derivatives=[("w", 1, [0])], **kw)
    with pytest.raises(ValueError, match="axes"):
        npde.ahmc_bayesian_pinn_pde(sysm, disc, ensemble_derivatives=[("u", 2, [0])], **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def body_refusals(npde, precision):
    rep, thetas, pts, reqs, _ = problem(npde, "2-16-16-1", precision)
    eng = rep.engine
    L, dp, ip = eng.L, C.POINTER(C.c_double), C.POINTER(C.c_int)
    ptr = lambda a: a.ctypes.data_as(dp)
    before = eng.phi_ensemble(0, thetas, pts, ddof=1, return_preds=True)
    before_d = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)
    th0 = np.asarray(rep.flat_init_params, dtype=np.float64)
    loss0 = eng.loss_grad_f64(th0)
    flat = np.ascontiguousarray(pts.T).reshape(-1)
    mean, std = np.zeros((40, pts.shape[1])), np.zeros((40, pts.shape[1]))

    def call(net=0, S=5, p=eng.P, n=pts.shape[1], ddof=0, table=(D0,), nder=None):
        orders = np.zeros(40, dtype=np.int32)
        axes = np.zeros(160, dtype=np.int32)
        for j, (o, ax) in enumerate(table):
            orders[j] = o
            axes[4 * j:4 * j + len(ax)] = ax
        return L.lib.pinn_derivative_ensemble(eng.h, net, ptr(thetas), S, p, ptr(flat), n, len(table) if nder is None else nder, orders.ctypes.data_as(ip),
                                              axes.ctypes.data_as(ip), ddof, ptr(mean), ptr(std), None)

    def refused(rc, *words):
        assert rc != 0
        msg = L.last_error()
        assert "pinn_derivative_ensemble" in msg and all(w in msg for w in words), msg

    assert call() == 0
    # what pinn_phi_ensemble refuses
    refused(call(net=1), "net index 1 out of range")
    refused(call(net=-1), "out of range")
    refused(call(p=eng.P - 1), "ntheta")
    refused(call(S=0), "nsamples must be at least 1")
    refused(call(ddof=2), "ddof must be 0 or 1")
    refused(call(ddof=-1), "ddof must be 0 or 1")
    refused(call(S=1, ddof=1), "nsamples - ddof must be at least 1")
    refused(call(n=0), "n must be at least 1")
    # the request table
    refused(call(nder=0), "nder must be in 1..32")
    refused(call(nder=-1), "nder must be in 1..32")
    refused(call(table=[D0] * 33), "nder must be in 1..32", "33")
    refused(call(table=[V, (5, (0, 0, 0, 0))]), "request 1", "order 5 outside 0..4")
    refused(call(table=[(-1, ())]), "order -1 outside 0..4")
    refused(call(table=[D0, (1, (2,))]), "request 1", "axis 2 outside the network's 2 inputs")
    refused(call(table=[(2, (0, -1))]), "axis -1 outside")
    refused(call(table=[(3, (0, 0, 1))]), "mixed derivative of order 3")
    refused(call(table=[(4, (0, 1, 1, 1))]), "mixed derivative of order 4")
    refused(call(table=[V, D0, D01, D0]), "request 3 repeats request 1")
    refused(call(table=[D01, (2, (1, 0))]), "request 1 repeats request 0")
    refused(call(table=[V, V]), "repeats")
    with env(PINN_ENS_NO_LDS="1", PINN_ENS_GB="1e-7"):                       # a scratch region beyond the memory budget: the message names the sizes
        refused(call(), "bytes of image scratch per workgroup", "memory budget", str(2 * 16 * 2 * 64 * (8 if precision == "f64" else 4)))
    with pytest.raises(ValueError, match="order 2 takes 2 axes"):
        eng.derivative_ensemble(0, thetas, pts, [(2, (0,))])
    after = eng.phi_ensemble(0, thetas, pts, ddof=1, return_preds=True)
    after_d = eng.derivative_ensemble(0, thetas, pts, reqs, ddof=1, return_preds=True)
    assert same(before, after) and same(before_d, after_d)
    loss1 = eng.loss_grad_f64(th0)
    assert np.array_equal(np.asarray(loss0[0]), np.asarray(loss1[0])) and np.array_equal(loss0[1], loss1[1])


def body_refused_networks(npde, precision):
    """a DGM network, a network behind a periodic embedding: refused as by pinn_phi_ensemble, the handle left as it was"""
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    sysm = npde.PDESystem([npde.Eq(u(x), x)], [npde.Eq(u(0.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    pts = np.linspace(0.0, 1.0, 7)[None, :]

    def refused(chain, *words):
        theta0 = npde.initialparameters(np.random.default_rng(1), chain)
        rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.5), init_params=theta0, precision=precision))
        th = np.asarray(rep.flat_init_params, dtype=np.float64)
        own = rep.phi(pts, th)
        with pytest.raises(Exception) as ei:
            rep.engine.derivative_ensemble(0, np.stack([th, th]), pts, [D0])
        assert "pinn_derivative_ensemble" in str(ei.value) and all(w in str(ei.value) for w in words), str(ei.value)
        assert np.array_equal(rep.phi(pts, th), own)

    if precision == "f32":                               # (the float64 mode does not cover DGM networks: no such handle exists)
        refused(npde.DGM(1, 1, 8, 1), "DGM")
    refused(npde.Chain(npde.PeriodicEmbedding([1], [1.0]), npde.Dense(2, 16, "tanh"), npde.Dense(16, 1)), "periodic input embedding")


# ------------------------------------------------------------------------------------------------------------------------------------
# the two faces of every body
# ------------------------------------------------------------------------------------------------------------------------------------
GRID = [(n, p) for n in PARITY for p in PRECISIONS]
CONSISTENCY = [(n, p) for n in ("1-6-1", "2-16-16-1", "mix", "3-64-64-1") for p in PRECISIONS]
STORAGE = [(n, p) for n in ("1-16-16-1", "2-40x3-1") for p in PRECISIONS]
CHUNKS = [(n, p) for n in ("1-16-16-1", "2-16-16-1") for p in PRECISIONS]
GROUPS = [(n, p) for n in GROUPING for p in PRECISIONS]


@pytest.mark.parametrize("name,precision", GRID)
def test_parity(npde, use_emu, name, precision):
    body_parity(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", GRID)
def test_parity_gpu(npde, hip_lib, name, precision):
    body_parity(npde, name, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_system_second_network(npde, use_emu, precision):
    body_system(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_system_second_network_gpu(npde, hip_lib, precision):
    body_system(npde, precision)


@pytest.mark.parametrize("name,precision", CONSISTENCY)
def test_internal_consistency(npde, use_emu, name, precision):
    body_consistency(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", CONSISTENCY)
def test_internal_consistency_gpu(npde, hip_lib, name, precision):
    body_consistency(npde, name, precision)


@pytest.mark.parametrize("name,precision", STORAGE)
def test_lds_and_scratch_storage_agree(npde, use_emu, name, precision):
    body_storage(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", STORAGE)
def test_lds_and_scratch_storage_agree_gpu(npde, hip_lib, name, precision):
    body_storage(npde, name, precision)


@pytest.mark.parametrize("name,precision", CHUNKS)
def test_point_passes(npde, use_emu, name, precision):
    body_chunks(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", CHUNKS)
def test_point_passes_gpu(npde, hip_lib, name, precision):
    body_chunks(npde, name, precision)


@pytest.mark.parametrize("name,precision", GROUPS)
def test_pass_grouping(npde, use_emu, name, precision):
    body_grouping(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", GROUPS)
def test_pass_grouping_gpu(npde, hip_lib, name, precision):
    body_grouping(npde, name, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror(npde, use_emu, precision):
    body_mirror(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror_gpu(npde, hip_lib, precision):
    body_mirror(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(npde, use_emu, precision):
    body_refusals(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_gpu(npde, hip_lib, precision):
    body_refusals(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refused_networks(npde, use_emu, precision):
    body_refused_networks(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refused_networks_gpu(npde, hip_lib, precision):
    body_refused_networks(npde, precision)
