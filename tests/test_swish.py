"""The swish activation (Lux.swish, f(z) = z sigma(z)) on Dense chains: fp32 families 1 and 2 (both GEMM modes, every evaluation mode),
run-time specialised shapes, and the float64 lane-per-point family.  The layer records keep the pre-activation z (as for sin) and the
derivatives are f^(k) = z s^(k) + k s^(k-1) on the logistic polynomials of the sigmoid rules (csrc/pinn_kernels.hpp: act_derivs_n).

Every body is written once as a function of `npde` and exposed twice: on the CPU through the g++ lock-step emulation (`use_emu`) and,
marked `gpu`, on the product library (as tests/test_gpu_mirror.py does for the older suites).  The oracle looks activations up in
pinn_oracle.ACTS at call time; the fixture below registers swish there for the duration of a test.

Tolerances are the project's: fp32 against the float64 oracle at test_emu_parity.TOL = 1e-5 (exact derivatives and the reference's
stencils); pointwise derivatives of order 0..6 at the bound the existing pointwise-derivative tests use for orders >= 3
(2e-5 * max(1, max |exact|): tests/test_emu_parity.py::test_forward_derivatives_mirror, tests/test_jit.py); float64 at 1e-11 relative
for losses / gradients (tests/test_f64_mode.py: EXACT) and 1e-13 * max(1, max |exact|) for pointwise derivatives (its line 438);
resident Adam against a host Adam as tests/test_emu_parity.py (fp32: rtol 2e-5 / 5e-5) and tests/test_f64_mode.py (1e-13) compare them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import sympy as sp

import helpers
import pinn_oracle as po
import test_dgm as td
import test_emu_parity as tp
import test_f64_mode as tf

EXACT = tf.EXACT


@pytest.fixture(autouse=True)
def _oracle_knows_swish(monkeypatch):
    import torch
    monkeypatch.setitem(po.ACTS, "swish", lambda z: z * torch.sigmoid(z))


def _chain(npde, d, width, hidden):
    return npde.Chain(npde.Dense(d, width, "swish"), *[npde.Dense(width, width, "swish") for _ in range(hidden - 1)], npde.Dense(width, 1))


def _kernels(rep):
    return [l.split("kernel=")[1].split()[0] for l in rep.engine.describe().splitlines() if "kernel=" in l]


def _assert_swish_ran(rep, family=None):
    ks = _kernels(rep)
    assert ks and all(k.endswith("+swish") for k in ks), rep.engine.describe()
    if family is not None:
        assert all(k.startswith("F%d_" % family) for k in ks), ks


def _sobol(npde, n, nb, seed):
    return npde.QuasiRandomTraining(n, bcs_points=nb, sampling_alg=npde.SobolSample(seed=seed), resampling=False, minibatch=1)


def _sixth_order_ode(npde):
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    D = npde.Differential(x)
    eq = npde.Eq((D ** 6)(u(x)) + u(x) * D(u(x)), sp.cos(x))
    return npde.PDESystem([eq], [npde.Eq(u(0.0), 1.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. fp32 parity against the float64 oracle, exact derivatives and the reference's stencils, at TOL
# ------------------------------------------------------------------------------------------------------------------------------------
def body_parity_width16_family1(npde):
    sysm, _ = tp.poisson2d(npde)
    chain = _chain(npde, 2, 16, 2)
    for mode, seed in (("exact", 81), ("stencil", 82)):
        rep, *_ = tp.check(npde, sysm, [chain], _sobol(npde, 50, 21, 6), tp.theta_for(chain, seed), weights=[1.0, 2.0, 0.5, 1.5, 1.0], mode=mode)
        _assert_swish_ran(rep, family=1)


def body_parity_width64_family2(npde, gemm):
    sysm, _ = tp.poisson2d(npde)
    chain = _chain(npde, 2, 64, 4)
    for mode, seed in (("exact", 83), ("stencil", 84)):
        theta = tp.theta_for(chain, seed)
        # (tp.check with the GEMM mode chosen on the discretisation's engine: same statements)
        disc = npde.PhysicsInformedNN(chain, _sobol(npde, 50, 70, 6), init_params=theta, precision="f32")
        rep = npde.symbolic_discretize(sysm, disc)
        assert rep.engine.L.backend == tp.EXPECTED_BACKEND
        rep.engine.set_option("gemm", gemm)
        assert rep.engine.get_option("gemm") == gemm
        sets = rep.pde_train_sets + rep.bcs_train_sets
        th = rep.flat_init_params
        losses, grad = rep.engine.loss_grad(th)
        prob = helpers.oracle_problem(npde, sysm, [chain])
        ref = po.loss_and_grad(prob, th, sets, mode=mode)
        le, g2, gi = helpers.rel_errors(losses, grad, ref)
        print("swish 4x64 gemm=%s mode=%s: loss rel %.3e grad L2 %.3e Linf %.3e" % (gemm, mode, le.max(), g2, gi))
        assert le.max() < tp.TOL and g2 < tp.TOL and gi < tp.TOL, (gemm, mode, le, g2, gi)
        l2, g2_ = rep.engine.loss_grad(th)
        assert np.array_equal(l2, losses) and np.array_equal(g2_, grad)
        _assert_swish_ran(rep, family=2)
        assert ("split-bf16" in rep.engine.describe()) == (gemm == "split")


def body_parity_runtime_specialised_40x5(npde):
    sysm, _ = helpers.shape_problem(npde, 40, 5, 2)                  # mixed second derivatives; five hidden layers of 40: outside the table
    chain = _chain(npde, 2, 40, 5)
    for mode, seed in (("exact", 31), ("stencil", 32)):
        rep, *_ = tp.check(npde, sysm, [chain], _sobol(npde, 20, 8, 5), tp.theta_for(chain, seed), mode=mode)
        _assert_swish_ran(rep)
        assert any("HP64_NHH4" in k for k in _kernels(rep))


def body_parity_burgers(npde):
    sysm = td._burgers(npde)
    chain = _chain(npde, 2, 16, 2)
    for mode, seed in (("exact", 101), ("stencil", 102)):
        rep, *_ = tp.check(npde, sysm, [chain], _sobol(npde, 70, 20, 3), tp.theta_for(chain, seed), weights=[1.0, 2.0, 0.5, 3.0], mode=mode)
        _assert_swish_ran(rep)


def body_parity_third_order_ode(npde):
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq((npde.Differential(x) ** 3)(u(x)) + u(x) * npde.Differential(x)(u(x)), sp.cos(sp.pi * x))
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 1.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = _chain(npde, 1, 24, 2)
    rep, prob, sets, th = tp.check(npde, sysm, [chain], npde.GridTraining(0.05), tp.theta_for(chain, 33), mode="exact")
    _assert_swish_ran(rep)
    # the reference's own order-3 stencil (eps^(1/5)) agrees with the exact derivative to ~1e-5 only: the bound the sigmoid test uses
    ref_fd = po.loss_and_grad(prob, th, sets, mode="stencil")
    losses, grad = rep.engine.loss_grad(th)
    le, g2, gi = helpers.rel_errors(losses, grad, ref_fd)
    assert le.max() < 2e-4 and g2 < 2e-4, (le, g2)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the activation rules order by order: d[1] .. d[6] in the forward sweep, d[7] in the adjoint of an order-6 term
# ------------------------------------------------------------------------------------------------------------------------------------
def body_rules_order_by_order_f32(npde):
    import torch
    sysm = _sixth_order_ode(npde)
    chain = _chain(npde, 1, 12, 2)
    ochain = po.Chain((1, 12, 12, 1), "swish")
    # the gradient of a term whose residual holds u^(6): the reverse sweep reads f^(7)
    rep, prob, sets, th = tp.check(npde, sysm, [chain], npde.GridTraining(0.1), tp.theta_for(chain, 42), mode="exact")
    _assert_swish_ran(rep)
    uu = lambda cord, t_, phi: phi(cord, t_).sum(dim=0, keepdim=True)
    pts = np.random.default_rng(2).uniform(0.05, 0.95, size=(1, 40))
    tht = torch.tensor(th, dtype=po.DT)
    for k in range(7):
        got = rep.engine.derivative(0, th, pts, [0] * k)
        ex = po.exact_derivative(ochain, uu, torch.tensor(pts, dtype=po.DT), [0] * k, tht).detach().numpy().reshape(-1) if k else \
            po.phi_values(ochain, th, pts).reshape(-1)
        err, bound = np.max(np.abs(got - ex)), 2e-5 * max(1.0, np.max(np.abs(ex)))
        print("swish fp32 derivative order %d: max |err| %.3e (bound %.3e, max |exact| %.3e)" % (k, err, bound, np.max(np.abs(ex))))
        assert err < bound, (k, err, bound)
    with pytest.raises(Exception, match="order must be 0..6"):
        rep.engine.derivative(0, th, pts, [0] * 7)


def body_rules_order_by_order_f64(npde):
    import torch
    # a 1-D residual with u'''' binds the network to the float64 jet set carrying orders 0..4 (the float64 kernels: 1-D up to order 4)
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    D4 = npde.Differential(x) ** 4
    sysm = npde.PDESystem([npde.Eq(D4(u(x)) + u(x), sp.sin(x))], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.5)],
                          [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = _chain(npde, 1, 12, 2)
    ochain = po.Chain((1, 12, 12, 1), "swish")
    theta = tp.theta_for(chain, 5)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.05), init_params=theta, precision="f64"))
    eng = rep.engine
    assert eng.get_option("precision") == "f64"
    sets = rep.pde_train_sets + rep.bcs_train_sets
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    prob = helpers.oracle_problem(npde, sysm, [chain])
    ref = po.loss_and_grad(prob, th, sets, mode="exact")                # the reverse sweep of the order-4 term reads f^(5)
    l64, g64 = eng.loss_grad_f64(th)
    le, g2, gi = helpers.rel_errors(l64, g64, ref)
    assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)
    assert eng.get_option("f64_path") == "lanes"
    uu = lambda cord, t_, phi: phi(cord, t_).sum(dim=0, keepdim=True)
    pts = np.random.default_rng(5).uniform(0, 1, size=(1, 700))         # several chunks of the lanes kernels' blocks, ragged
    tht = torch.tensor(th, dtype=po.DT)
    for k in range(5):
        got = eng.derivative_f64(0, th, pts, [0] * k)
        ex = po.exact_derivative(ochain, uu, torch.tensor(pts, dtype=po.DT), [0] * k, tht).detach().numpy().reshape(-1) if k else \
            po.phi_values(ochain, th, pts).reshape(-1)
        assert np.max(np.abs(got - ex)) < 1e-13 * max(1.0, np.max(np.abs(ex))), k


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. float64 mode
# ------------------------------------------------------------------------------------------------------------------------------------
def body_f64_mode(npde):
    sysm, _ = helpers.shape_problem(npde, 16, 2, 2)                      # u_x, u_xx, u_xy, u_yy, u u_x
    chain = _chain(npde, 2, 16, 2)
    strat = _sobol(npde, 700, 150, 3)                                    # several ragged chunks / blocks of the lanes kernels
    prob = helpers.oracle_problem(npde, sysm, [chain])
    th0 = np.asarray(tp.theta_for(chain, 11), dtype=np.float64)
    for prec in ("f64", "auto"):
        rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=th0, precision=prec))
        eng = rep.engine
        assert eng.get_option("precision") == "f64" and "precision=f64" in eng.describe()
        assert rep.flat_init_params.dtype == np.float64
        sets = rep.pde_train_sets + rep.bcs_train_sets
        th = rep.flat_init_params
        w = np.linspace(1.0, 2.0, eng.K)
        ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
        l64, g64 = eng.loss_grad_f64(th, w)
        le, g2, gi = helpers.rel_errors(l64, g64, ref)
        print("swish f64 (%s): loss rel %.3e grad L2 %.3e Linf %.3e" % (prec, le.max(), g2, gi))
        assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)
        l2, g2_ = eng.loss_grad_f64(th, w)
        assert np.array_equal(l2, l64) and np.array_equal(g2_, g64)
        # swish runs the lane-per-point family, and the handle says so
        assert eng.get_option("f64_path") == "lanes" and "lanes+swish" in eng.describe() and "mfma" not in eng.describe().split("f64_kernels=")[1].split()[0]
    # loss-only evaluation in double
    lo, go = eng.loss_grad_f64(th, w, want_grad=False)
    assert go is None
    np.testing.assert_allclose(lo, l64, rtol=1e-13, atol=0)
    # phi, the datafree residual closures and the per-term gradients in double
    x = sets[0][:, :300]
    assert np.max(np.abs(rep.phi(x, th) - po.phi_values(prob.chains[0], th, x).reshape(1, -1))) < 1e-14
    for k in range(eng.K):
        r = eng.residual_f64(k, th, sets[k].shape[1])
        rr = po.residual_values(prob, th, k, sets[k], mode="exact")
        assert np.max(np.abs(r - rr)) < 1e-12 * max(1.0, np.max(np.abs(rr))), k
    r = rep.loss_functions.datafree_pde_loss_functions[0](sets[0], th)
    rr = po.residual_values(prob, th, 0, sets[0], mode="exact")
    assert r.dtype == np.float64 and np.max(np.abs(np.asarray(r).reshape(-1) - rr.reshape(-1))) < 1e-12 * max(1.0, np.max(np.abs(rr)))
    L, tg = eng.term_grads_f64(th)
    assert tg.dtype == np.float64 and tg.shape == (eng.K, eng.P)
    for k in range(eng.K):
        wk = np.zeros(eng.K)
        wk[k] = 1.0
        refk = po.loss_and_grad(prob, th, sets, weights=wk, mode="exact")
        assert abs(L[k] - refk.term_losses[k]) < EXACT * abs(refk.term_losses[k])
        assert np.linalg.norm(tg[k] - refk.grad) < EXACT * np.linalg.norm(refk.grad), k
    # an fp32 handle switched on the fly
    rep32 = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=th0, precision="f32"))
    rep32.engine.set_option("precision", "f64")
    for k, s_ in enumerate(sets):
        rep32.engine.set_points_f64(k, s_)
    l3, g3 = rep32.engine.loss_grad_f64(th, w)
    assert np.array_equal(l3, l64) and np.array_equal(g3, g64)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. every evaluation mode: loss only = the fused evaluation's losses; per-term gradients, residual / value / derivative entry points
# ------------------------------------------------------------------------------------------------------------------------------------
def body_evaluation_modes(npde, width, hidden, gemm):
    import torch
    sysm, _ = helpers.shape_problem(npde, width, hidden, 2)
    chain = _chain(npde, 2, width, hidden)
    rep, prob, sets, th = tp.check(npde, sysm, [chain], _sobol(npde, 33, 70 if width >= 64 else 20, 4), tp.theta_for(chain, 7))
    eng = rep.engine
    if gemm:
        eng.set_option("gemm", gemm)
    _assert_swish_ran(rep, family=2 if width >= 64 else 1)
    w = [1.0, 2.0, 0.5]
    losses, grad = eng.loss_grad(th, w)
    l_only, g_only = eng.loss_grad(th, w, want_grad=False)
    assert g_only is None
    np.testing.assert_allclose(l_only, losses, rtol=1e-13, atol=0)
    l_again, _ = eng.loss_grad(th, w, want_grad=False)
    assert np.array_equal(l_again, l_only)
    l2, g2 = eng.loss_grad(th, w)
    assert np.array_equal(l2, losses) and np.array_equal(g2, grad)
    # per-term gradients
    tl, tg = eng.term_grads(th)
    ref = po.loss_and_grad(prob, th, sets, mode="stencil", per_term_grads=True)
    assert np.max(np.abs(tg - ref.term_grads)) / np.max(np.abs(ref.term_grads)) < tp.TOL
    np.testing.assert_allclose(tl, ref.term_losses, rtol=tp.TOL)
    # value / residual / derivative entry points
    pts = sets[0][:, :33]
    assert np.max(np.abs(rep.phi(pts, th)[0] - po.phi_values(prob.chains[0], th, pts)[0])) < 1e-5
    r = eng.residual(0, th, sets[0].shape[1])
    r_ref = po.residual_values(prob, th, 0, sets[0], mode="exact")[0]
    assert np.max(np.abs(r - r_ref)) < 2e-5 * max(1.0, np.max(np.abs(r_ref)))
    uu = lambda cord, t_, phi: phi(cord, t_).sum(dim=0, keepdim=True)
    for axes in ([0], [1, 1], [0, 1]):
        ex = po.exact_derivative(prob.chains[0], uu, torch.tensor(pts, dtype=po.DT), axes, torch.tensor(th, dtype=po.DT)).detach().numpy().reshape(-1)
        assert np.max(np.abs(eng.derivative(0, th, pts, axes) - ex)) < 2e-5 * max(1.0, np.max(np.abs(ex))), axes


def body_large_preactivations_stay_finite(npde):
    """exp overflow at the ends: sigma saturates to exactly 0 or 1, swish to 0 or z and every derivative to 0 or 1 — never NaN"""
    sysm, _ = tp.poisson2d(npde)
    chain = _chain(npde, 2, 16, 2)
    th = np.asarray(tp.theta_for(chain, 3), dtype=np.float32) * np.float32(400.0)       # pre-activations of +-1e2 .. 1e4 and beyond
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, _sobol(npde, 50, 21, 6), init_params=th, precision="f32"))
    losses, grad = rep.engine.loss_grad(rep.flat_init_params)
    assert np.all(np.isfinite(losses)) and np.all(np.isfinite(grad))
    rep.engine.set_option("precision", "f64")
    for k, s_ in enumerate(rep.pde_train_sets + rep.bcs_train_sets):
        rep.engine.set_points_f64(k, s_)
    l64, g64 = rep.engine.loss_grad_f64(np.asarray(rep.flat_init_params, dtype=np.float64))
    assert np.all(np.isfinite(l64)) and np.all(np.isfinite(g64))


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. training
# ------------------------------------------------------------------------------------------------------------------------------------
def body_training_f32(npde):
    sysm, _ = tp.poisson2d(npde)
    chain = _chain(npde, 2, 16, 2)
    th0 = tp.theta_for(chain, 51)
    disc = npde.PhysicsInformedNN(chain, npde.GridTraining(0.25), init_params=th0,
                                  adaptive_loss=npde.NonAdaptiveLoss(pde_loss_weights=1.0, bc_loss_weights=[2.0, 1.0, 3.0, 1.0]), precision="f32")
    prob = npde.discretize(sysm, disc)
    res = npde.solve(prob, npde.Adam(0.01), maxiters=25)
    # the persistent training kernel keeps its tanh / sigmoid gate: a swish problem runs the stand-alone resident loop
    assert prob.pinnrep.engine.get_option("adam_path") == "loop"
    th, m_, v_, hist = prob.u0.astype(np.float32).copy(), 0.0, 0.0, []
    for it in range(1, 26):
        val, g = prob.f.value_and_grad(th)
        hist.append(val)
        g = g.astype(np.float32)
        m_ = np.float32(0.9) * m_ + np.float32(0.1) * g
        v_ = np.float32(0.999) * v_ + np.float32(0.001) * g * g
        th = (th - np.float32(0.01) * (m_ / np.float32(1 - 0.9 ** it)) / (np.sqrt(v_ / np.float32(1 - 0.999 ** it)) + np.float32(1e-8))).astype(np.float32)
    np.testing.assert_allclose(res.losses, hist, rtol=2e-5)
    assert np.max(np.abs(res.u - th)) < 5e-5
    assert res.losses[-1] < res.losses[0]
    _assert_swish_ran(prob.pinnrep)
    # L-BFGS inside the library
    disc = npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=th0, precision="f32")
    prob = npde.discretize(sysm, disc)
    rep = prob.pinnrep
    f0 = float(prob.f.value_and_grad(th0)[0])
    theta, hist = rep.engine.lbfgs(th0, 60, rep._weights_now())
    assert len(hist) >= 10 and np.all(np.diff(hist) <= 1e-12) and hist[-1] < 0.5 * f0
    f1 = float(prob.f.value_and_grad(theta)[0])
    assert abs(f1 - hist[-1]) <= 1e-5 * abs(f1) + 1e-12
    res = npde.solve(prob, npde.LBFGS(), maxiters=60)
    np.testing.assert_allclose(res.losses[-1], hist[-1], rtol=1e-12)


def body_training_f64(npde):
    sysm, _ = tp.poisson2d(npde)
    chain = _chain(npde, 2, 16, 2)
    th0 = np.asarray(tp.theta_for(chain, 52), dtype=np.float64)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, _sobol(npde, 96, 32, 2), init_params=th0, precision="f64"))
    eng = rep.engine
    assert eng.get_option("precision") == "f64"
    w = np.linspace(1.0, 2.0, eng.K)
    th_dev, hist = eng.adam_f64(th0, 12, 3e-3, w)
    assert eng.get_option("f64_path") == "lanes" and eng.get_option("adam_path") == "loop"
    th_host = tf._host_adam(th0, [lambda th: eng.loss_grad_f64(th, w)[1]] * 12, 3e-3)
    np.testing.assert_allclose(th_dev, th_host, rtol=0, atol=1e-13 * np.abs(th_host).max())
    l0, _ = eng.loss_grad_f64(th0, w)
    assert abs(hist[0] - float(np.dot(w, l0))) < 1e-13 * abs(hist[0])
    assert hist[-1] < hist[0]
    # the mirror's solve(...) in double, Adam then L-BFGS
    prob = npde.discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=th0, precision="f64"))
    res = npde.solve(prob, npde.Adam(0.01), maxiters=30)
    assert res.u.dtype == np.float64 and res.losses[-1] < res.losses[0]
    res2 = npde.solve(npde.remake(prob, u0=res.u), npde.LBFGS(), maxiters=40)
    assert res2.u.dtype == np.float64 and np.all(np.isfinite(res2.losses)) and res2.losses[-1] < res.losses[-1]


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. refusals stay loud
# ------------------------------------------------------------------------------------------------------------------------------------
def body_refusals(npde):
    sysm, _ = tp.poisson2d(npde)
    with pytest.raises(ValueError, match="mixes only tanh and sigmoid"):
        npde.Chain(npde.Dense(2, 16, "swish"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    with pytest.raises(ValueError, match="unsupported DGM activations"):
        npde.DGM(2, 1, 8, 1, "swish", "tanh")
    with pytest.raises(ValueError, match="unsupported DGM activations"):
        npde.DGM(2, 1, 8, 1, "tanh", "swish")
    for bad in ("relu", "gelu"):
        chain = npde.Chain(npde.Dense(2, 16, bad), npde.Dense(16, 16, bad), npde.Dense(16, 1))
        with pytest.raises(npde.EngineError, match="unsupported activation"):
            npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.25), precision="f32"))
    # the descriptor itself refuses the mixes the Python front end never writes
    head = "pinnir 1\nntheta 337\nparams 0 0 337\ndefaults \nnets 1\n"
    for net, msg in (("net 0 swish,tanh 0 4 2 16 16 1\n", "swish cannot be mixed with other activations inside one chain"),
                     ("net 0 dgm,swish,tanh,1 0 3 2 8 1\n", "unsupported DGM activations")):
        with pytest.raises(npde.EngineError, match=msg):
            npde.Engine(head + net + "terms 0\n")
    # PINN_NO_JIT: a swish shape outside the ahead-of-time table fails at create time with the table line to add, naming the variant
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import pinn_import; m = pinn_import.load(); m._lib.set_library(m.Library(%r))\n"
            "import test_emu_parity as tp\n"
            "sysm, _ = tp.poisson2d(m)\n"
            "odd = m.Chain(m.Dense(2, 200, 'swish'), m.Dense(200, 200, 'swish'), m.Dense(200, 1))\n"
            "try:\n    m.symbolic_discretize(sysm, m.PhysicsInformedNN(odd, m.GridTraining(0.5), precision='f32'))\nexcept m.EngineError as e:\n    print('ENGINEERROR', e)\n"
            % (root, os.path.join(root, "tests"), os.path.join(root, "oracle"), npde._lib.default_library().path))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PINN_NO_JIT="1"), capture_output=True, text=True, timeout=300)
    assert "ENGINEERROR" in r.stdout and "no compiled kernel" in r.stdout and "swish activation (PINN_INSTANTIATE*_SWISH)" in r.stdout \
        and "add a PINN_INSTANTIATE line" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------------------------
# the two expositions of every body
# ------------------------------------------------------------------------------------------------------------------------------------
BODIES = [
    ("parity_width16_family1", body_parity_width16_family1, {}),
    ("parity_width64_family2_split", body_parity_width64_family2, {"gemm": "split"}),
    ("parity_width64_family2_fp32", body_parity_width64_family2, {"gemm": "fp32"}),
    ("parity_runtime_specialised_40x5", body_parity_runtime_specialised_40x5, {}),
    ("parity_burgers", body_parity_burgers, {}),
    ("parity_third_order_ode", body_parity_third_order_ode, {}),
    ("rules_order_by_order_f32", body_rules_order_by_order_f32, {}),
    ("rules_order_by_order_f64", body_rules_order_by_order_f64, {}),
    ("f64_mode", body_f64_mode, {}),
    ("evaluation_modes_family1", body_evaluation_modes, {"width": 16, "hidden": 2, "gemm": None}),
    ("evaluation_modes_family2_split", body_evaluation_modes, {"width": 64, "hidden": 4, "gemm": "split"}),
    ("evaluation_modes_family2_fp32", body_evaluation_modes, {"width": 64, "hidden": 4, "gemm": "fp32"}),
    ("large_preactivations_stay_finite", body_large_preactivations_stay_finite, {}),
    ("training_f32", body_training_f32, {}),
    ("training_f64", body_training_f64, {}),
    ("refusals", body_refusals, {}),
]
_PARAMS = [pytest.param(fn, kw, id=name) for name, fn, kw in BODIES]


@pytest.mark.parametrize("fn,kw", _PARAMS)
def test_swish(npde, use_emu, fn, kw):
    fn(npde, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("fn,kw", _PARAMS)
def test_swish_on_hardware(npde, hip_lib, monkeypatch, fn, kw):
    monkeypatch.setattr(tp, "EXPECTED_BACKEND", "hip")
    assert npde._lib.default_library().backend == "hip", "the hardware twin must run on the product library"
    fn(npde, **kw)
