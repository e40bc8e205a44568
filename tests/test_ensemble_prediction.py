"""Device ensemble prediction (`pinn_phi_ensemble`): phi of one network at S parameter vectors and n points, and the mean and
standard deviation over the S predictions, in one call.

The reference throughout is `mlp_forward` below: a float64 numpy restatement of a Dense chain, evaluated per sample on the SAME `thetas` and
`pts`, then `mean(axis=0)` and `std(axis=0, ddof=ddof)` — never the engine's own `preds`.  The error measure for `preds`, `mean` and `std` is
max|got - ref| / max(1, max|ref|); the bars are the project's existing ones: 1e-11 on a handle in float64 mode (tests/test_f64_mode.py,
DESIGN §6.2), 1e-5 on an fp32 handle (§6.1).

Every body is written once as a function of `npde` and exposed twice: on the CPU through the g++ emulation (`use_emu`) and, marked `gpu`, on
the product library (`hip_lib`).  Handles and references are built once per (chain, precision) and shared by the cases.

The issue's grid lists a single `Dense(2, 1)`; `Chain` refuses a chain without a hidden layer ("the HIP engine needs at least one hidden
layer", pinned by tests/test_resident_hmc.py), so no handle of that shape exists: the parity grid cannot reach it, and the case is
`test_no_hidden_layer_chain_is_refused`, which confirms the refusal."""
import ctypes as C
import os

import numpy as np
import pytest
import sympy as sp

import pinn_oracle as po

PRECISIONS = ("f64", "f32")
BAR = {"f64": 1e-11, "f32": 1e-5}
N_POINTS = (1, 63, 64, 65, 130)            # one lane, a ragged wave, one full block, a second block, a ragged last block
SAMPLE_CASES = ((1, 0), (2, 0), (5, 0), (5, 1))      # (S, ddof)

# name -> (sizes, activation per hidden layer)
CHAINS = {
    "1-6-1": ((1, 6, 1), "tanh"),
    "1-16-16-1": ((1, 16, 16, 1), "tanh"),
    "2-40x3-1": ((2, 40, 40, 40, 1), "tanh"),
    "2-64x4-1": ((2, 64, 64, 64, 64, 1), "tanh"),
    "3-128-128-1": ((3, 128, 128, 1), "tanh"),
    "sigmoid": ((1, 16, 16, 1), "sigmoid"),
    "sin": ((2, 16, 16, 1), "sin"),            # (2-16-16-1: the shape whose sin / swish kernels are in the ahead-of-time table)
    "swish": ((2, 16, 16, 1), "swish"),
    "mix": ((1, 16, 16, 1), ("tanh", "sigmoid")),
}
ACT = {"tanh": np.tanh, "sigmoid": lambda z: 1.0 / (1.0 + np.exp(-z)), "sin": np.sin, "swish": lambda z: z / (1.0 + np.exp(-z))}


def acts_of(name):
    sizes, act = CHAINS[name]
    return [act] * (len(sizes) - 2) if isinstance(act, str) else list(act)


def make_chain(npde, name):
    sizes, _ = CHAINS[name]
    kinds = acts_of(name) + ["identity"]
    return npde.Chain(*[npde.Dense(sizes[l], sizes[l + 1], kinds[l]) if kinds[l] != "identity" else npde.Dense(sizes[l], sizes[l + 1]) for l in range(len(sizes) - 1)])


def theta_for(sizes, seed):
    return po.glorot_theta(po.Chain(tuple(sizes), "tanh"), np.random.default_rng(seed)).astype(np.float64)


def mlp_forward(sizes, kinds, theta, pts):
    """float64 restatement: theta in ComponentArrays order (per layer W, n_out x n_in column-major, then b); pts (d x N) -> (N,)"""
    a, o = np.asarray(pts, dtype=np.float64), 0
    for l in range(len(sizes) - 1):
        n_in, n_out = sizes[l], sizes[l + 1]
        W = theta[o:o + n_out * n_in].reshape(n_in, n_out).T
        b = theta[o + n_out * n_in:o + n_out * n_in + n_out]
        o += n_out * n_in + n_out
        a = W @ a + b[:, None]
        if l < len(sizes) - 2:
            a = ACT[kinds[l]](a)
    return a[0]


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


def problem(npde, name, precision):
    """-> (rep, thetas (5 x P), pts (d x 130), reference preds (5 x 130)); built once per (library, chain, precision)"""
    key = (id(npde._lib.default_library()), name, precision)
    if key not in _CACHE:
        sizes = CHAINS[name][0]
        rep = value_problem(npde, [make_chain(npde, name)], precision)
        assert rep.engine.P == len(theta_for(sizes, 0))
        rng = np.random.default_rng(11)
        thetas = np.stack([theta_for(sizes, 100 + s) * (1.0 + 0.1 * rng.standard_normal(rep.engine.P)) for s in range(5)])
        pts = rng.uniform(-1.0, 1.0, size=(sizes[0], max(N_POINTS)))
        ref = np.stack([mlp_forward(sizes, acts_of(name), th, pts) for th in thetas])
        _CACHE[key] = (rep, thetas, pts, ref)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. parity grid
# ------------------------------------------------------------------------------------------------------------------------------------
def body_parity(npde, name, precision):
    rep, thetas, pts, ref = problem(npde, name, precision)
    eng, bar, worst = rep.engine, BAR[precision], 0.0
    for n in N_POINTS:
        for S, ddof in SAMPLE_CASES:
            mean, std, preds = eng.phi_ensemble(0, thetas[:S], pts[:, :n], ddof=ddof, return_preds=True)
            r = ref[:S, :n]
            e = (err(preds, r), err(mean, r.mean(axis=0)), err(std, r.std(axis=0, ddof=ddof)))
            worst = max(worst, *e)
            print(f"ensemble parity {name} {precision} n={n} S={S} ddof={ddof}: preds {e[0]:.2e} mean {e[1]:.2e} std {e[2]:.2e} (bar {bar:g})")
            assert preds.shape == (S, n) and mean.shape == (n,) and std.shape == (n,)
            assert max(e) <= bar
            if S == 1:
                assert np.all(std == 0.0)
            m2, s2 = eng.phi_ensemble(0, thetas[:S], pts[:, :n], ddof=ddof)        # without preds: the same statistics
            assert np.array_equal(m2, mean) and np.array_equal(s2, std)
    print(f"ensemble parity {name} {precision}: worst {worst:.2e}")


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
    for net, sizes, kinds, off in ((1, s1, ["sigmoid", "tanh"], n0), (0, s0, ["tanh"], 0)):
        ref = np.stack([mlp_forward(sizes, kinds, th[off:], pts) for th in thetas])
        mean, std, preds = eng.phi_ensemble(net, thetas, pts, ddof=1, return_preds=True)
        e = (err(preds, ref), err(mean, ref.mean(axis=0)), err(std, ref.std(axis=0, ddof=1)))
        print(f"ensemble system {precision} net {net}: preds {e[0]:.2e} mean {e[1]:.2e} std {e[2]:.2e}")
        assert max(e) <= BAR[precision]


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. preds against the product's own closure
# ------------------------------------------------------------------------------------------------------------------------------------
def body_closure(npde, name, precision):
    rep, thetas, pts, _ = problem(npde, name, precision)
    eng = rep.engine
    preds = eng.phi_ensemble(0, thetas, pts, return_preds=True)[2]
    for s, th in enumerate(thetas):
        own = eng.phi_f64(0, th, pts) if precision == "f64" else eng.phi(0, th, pts).astype(np.float64)
        e = err(preds[s], own)
        print(f"ensemble closure {name} {precision} sample {s}: {e:.2e}")
        assert e <= BAR[precision]
    one, col = eng.phi_ensemble(0, thetas, pts[:, 0]), eng.phi_ensemble(0, thetas, pts[:, :1])      # a single point as (d,), as Phi takes it
    assert one[0].shape == (1,) and np.array_equal(one[0], col[0]) and np.array_equal(one[1], col[1])


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. determinism, independence of the point passes
# ------------------------------------------------------------------------------------------------------------------------------------
def body_chunks(npde, name, precision):
    rep, thetas, pts, _ = problem(npde, name, precision)
    eng = rep.engine
    a = eng.phi_ensemble(0, thetas, pts, ddof=1, return_preds=True)
    b = eng.phi_ensemble(0, thetas, pts, ddof=1, return_preds=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    old = os.environ.get("PINN_ENS_CHUNK")
    try:
        for chunk in ("1", "100"):                       # one point block per pass (3 passes of 130 points at 64 per block; 1 at 256) | two blocks
            os.environ["PINN_ENS_CHUNK"] = chunk
            c = eng.phi_ensemble(0, thetas, pts, ddof=1, return_preds=True)
            assert all(np.array_equal(x, y) for x, y in zip(a, c)), chunk
    finally:
        if old is None:
            os.environ.pop("PINN_ENS_CHUNK", None)
        else:
            os.environ["PINN_ENS_CHUNK"] = old


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. mirror
# ------------------------------------------------------------------------------------------------------------------------------------
def body_mirror(npde, precision):
    """the 1-D Poisson problem of tests/test_resident_hmc.py (11 + 1 + 1 points, 1-16-16-1 tanh), a few draws"""
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.pi ** 2 * sp.sin(sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    theta0 = npde.initialparameters(np.random.default_rng(7), chain)
    disc = npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta0, precision=precision)
    kw = dict(draw_samples=30, n_leapfrog=3, step_size=0.002, phystd=[0.5], bcstd=[0.3], seed=4)
    host = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), ensemble="host", **kw)
    dev = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), ensemble="device", **kw)
    default = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), **kw)
    assert host.stats["ensemble"] == "host" and dev.stats["ensemble"] == "device" and default.stats["ensemble"] == "host"
    assert np.array_equal(host.samples, dev.samples) and host.estimated_de_params == dev.estimated_de_params
    assert len(host.timepoints) == len(dev.timepoints) == 1 and np.array_equal(host.timepoints[0], dev.timepoints[0])
    assert np.array_equal(default.ensemblesol[0], host.ensemblesol[0]) and np.array_equal(default.ensemblestd[0], host.ensemblestd[0])
    e = (err(dev.ensemblesol[0], host.ensemblesol[0]), err(dev.ensemblestd[0], host.ensemblestd[0]))
    print(f"ensemble mirror {precision}: ensemblesol {e[0]:.2e} ensemblestd {e[1]:.2e}")
    assert dev.ensemblesol[0].shape == host.ensemblesol[0].shape == (11,) and max(e) <= BAR[precision]
    assert float(np.max(host.ensemblestd[0])) > 0.0
    with pytest.raises(ValueError, match="host.*device"):
        npde.ahmc_bayesian_pinn_pde(sysm, disc, ensemble="gpu", **kw)
    dev2 = npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", ensemble="device", **kw)      # independent of the sampler
    assert dev2.stats["sampler"] == "device" and dev2.stats["ensemble"] == "device" and dev2.ensemblesol[0].shape == (11,)


def body_mirror_system(npde, precision):
    """two dependent variables with networks of different shapes (u' = w, w' = -u): the device branch passes the full sample vectors and each
    variable's network index where the host loop slices the variable's parameters out of every draw"""
    (x,) = npde.parameters("x")
    u, w = npde.variables("u w")
    Dx = npde.Differential(x)
    sysm = npde.PDESystem([npde.Eq(Dx(u(x)), w(x)), npde.Eq(Dx(w(x)), -u(x))], [npde.Eq(u(0.0), 0.0), npde.Eq(w(0.0), 1.0)],
                          [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x), w(x)])
    chains = [npde.Chain(npde.Dense(1, 6, "tanh"), npde.Dense(6, 1)), npde.Chain(npde.Dense(1, 8, "sigmoid"), npde.Dense(8, 8, "tanh"), npde.Dense(8, 1))]
    rng = np.random.default_rng(9)
    init = [npde.initialparameters(rng, c) for c in chains]
    disc = npde.PhysicsInformedNN(chains, npde.GridTraining(0.1), init_params=init, precision=precision)
    kw = dict(draw_samples=30, n_leapfrog=3, step_size=0.0001, phystd=[0.5], bcstd=[0.3], seed=6)
    host = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(2), ensemble="host", **kw)
    dev = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(2), ensemble="device", **kw)
    assert host.stats["ensemble"] == "host" and dev.stats["ensemble"] == "device"
    assert np.array_equal(host.samples, dev.samples) and host.estimated_de_params == dev.estimated_de_params
    assert len(host.ensemblesol) == len(dev.ensemblesol) == 2 and len(dev.timepoints) == 2
    for i in range(2):
        assert np.array_equal(host.timepoints[i], dev.timepoints[i])
        e = (err(dev.ensemblesol[i], host.ensemblesol[i]), err(dev.ensemblestd[i], host.ensemblestd[i]))
        print(f"ensemble mirror system {precision} variable {i}: ensemblesol {e[0]:.2e} ensemblestd {e[1]:.2e}")
        assert dev.ensemblesol[i].shape == host.ensemblesol[i].shape == (11,) and max(e) <= BAR[precision]
        assert float(np.max(host.ensemblestd[i])) > 0.0
    assert not np.array_equal(dev.ensemblesol[0], dev.ensemblesol[1])          # (each variable from its own network)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def body_refusals(npde, precision):
    rep, thetas, pts, _ = problem(npde, "1-16-16-1", precision)
    eng = rep.engine
    L, dp = eng.L, C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)
    before = eng.phi_ensemble(0, thetas, pts, ddof=1, return_preds=True)
    th0 = np.asarray(rep.flat_init_params, dtype=np.float64)
    loss0 = eng.loss_grad_f64(th0) if hasattr(eng, "loss_grad_f64") else None
    flat = np.ascontiguousarray(pts.T).reshape(-1)
    mean, std = np.zeros(pts.shape[1]), np.zeros(pts.shape[1])

    def call(net=0, S=5, p=eng.P, n=pts.shape[1], ddof=0):
        return L.lib.pinn_phi_ensemble(eng.h, net, ptr(thetas), S, p, ptr(flat), n, ddof, ptr(mean), ptr(std), None)

    def refused(rc, *words):
        assert rc != 0
        msg = L.last_error()
        assert "pinn_phi_ensemble" in msg and all(w in msg for w in words), msg

    refused(call(net=1), "net index 1 out of range")
    refused(call(net=-1), "out of range")
    refused(call(p=eng.P - 1), "ntheta")
    refused(call(S=0), "nsamples must be at least 1")
    refused(call(ddof=2), "ddof must be 0 or 1")
    refused(call(ddof=-1), "ddof must be 0 or 1")
    refused(call(S=1, ddof=1), "nsamples - ddof must be at least 1")
    refused(call(n=0), "n must be at least 1")
    after = eng.phi_ensemble(0, thetas, pts, ddof=1, return_preds=True)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    if loss0 is not None:
        loss1 = eng.loss_grad_f64(th0)
        assert np.array_equal(np.asarray(loss0[0]), np.asarray(loss1[0])) and np.array_equal(loss0[1], loss1[1])


def body_refused_networks(npde, precision):
    """a DGM network, a network behind a periodic embedding, a layer wider than the LDS allows.  The widths are the smallest the fp32 planner,
    which every handle passes first, takes beyond the limit (160 neurons in float64 mode: 256; 320 on an fp32 handle: 384).  On the device the
    planner's own 384-wide fp32 kernel does not fit the CU's LDS and `pinn_create` fails before any handle exists: there the fp32 limit cannot
    be reached and the case confirms that; the emulation has no LDS limit of its own and reaches the refusal."""
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    sysm = npde.PDESystem([npde.Eq(u(x), x)], [npde.Eq(u(0.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    pts = np.linspace(0.0, 1.0, 7)[None, :]

    def refused(chain, *words, planner_limit=None):
        theta0 = npde.initialparameters(np.random.default_rng(1), chain)
        try:
            rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.5), init_params=theta0, precision=precision))
        except Exception as e:
            assert planner_limit is not None and npde._lib.default_library().path.endswith("libpinn_hip.so") and planner_limit in str(e), str(e)
            return
        th = np.asarray(rep.flat_init_params, dtype=np.float64)
        own = rep.phi(pts, th)
        with pytest.raises(Exception) as ei:
            rep.engine.phi_ensemble(0, np.stack([th, th]), pts)
        assert "pinn_phi_ensemble" in str(ei.value) and all(w in str(ei.value) for w in words), str(ei.value)
        assert np.array_equal(rep.phi(pts, th), own)

    if precision == "f32":                               # (the float64 mode does not cover DGM networks: no such handle exists)
        refused(npde.DGM(1, 1, 8, 1), "DGM")
    refused(npde.Chain(npde.PeriodicEmbedding([1], [1.0]), npde.Dense(2, 16, "tanh"), npde.Dense(16, 1)), "periodic input embedding")
    wide = 256 if precision == "f64" else 384                # (the fp32 planner, which every handle passes, takes multiples of 64 here)
    refused(npde.Chain(npde.Dense(1, wide, "tanh"), npde.Dense(wide, wide, "tanh"), npde.Dense(wide, 1)), f"({wide} neurons)", "bytes of LDS", "163840",
            planner_limit="exceeds limit (163840)" if precision == "f32" else None)


# ------------------------------------------------------------------------------------------------------------------------------------
# the two faces of every body
# ------------------------------------------------------------------------------------------------------------------------------------
GRID = [(n, p) for n in CHAINS for p in PRECISIONS]
CLOSURE = [(n, p) for n in ("1-16-16-1", "2-40x3-1", "mix") for p in PRECISIONS]
CHUNKS = [(n, p) for n in ("1-16-16-1", "3-128-128-1") for p in PRECISIONS]      # 256 and 64 points per block


def test_no_hidden_layer_chain_is_refused(npde, use_emu):
    """the issue's single `Dense(2, 1)`: no handle of that shape can exist, so `phi_ensemble` can never see one (holds before this feature too)"""
    with pytest.raises(ValueError, match="hidden layer"):
        npde.Chain(npde.Dense(2, 1))


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


@pytest.mark.parametrize("name,precision", CLOSURE)
def test_preds_equal_the_closure(npde, use_emu, name, precision):
    body_closure(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", CLOSURE)
def test_preds_equal_the_closure_gpu(npde, hip_lib, name, precision):
    body_closure(npde, name, precision)


@pytest.mark.parametrize("name,precision", CHUNKS)
def test_determinism_and_point_passes(npde, use_emu, name, precision):
    body_chunks(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", CHUNKS)
def test_determinism_and_point_passes_gpu(npde, hip_lib, name, precision):
    body_chunks(npde, name, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror(npde, use_emu, precision):
    body_mirror(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror_gpu(npde, hip_lib, precision):
    body_mirror(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror_two_variables(npde, use_emu, precision):
    body_mirror_system(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror_two_variables_gpu(npde, hip_lib, precision):
    body_mirror_system(npde, precision)


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
