"""The FLOAT64 evaluation mode (pinn_set_option(h, "precision", "f64"); csrc/pinn_kernels4.hpp, csrc/f64*.cpp): the reference's default
eltype (src/discretize.jl:432-449) on the device.  Same mathematics as the fp32 kernels — exact Taylor jets, residual tape, hand-derived
reverse sweep — in IEEE double, one lane per point.  Against the float64 oracle's exact-derivative mode the results agree to ROUNDING
(1e-12 and better): the engine's algorithm and the oracle's autograd are the same function.  That is also the strongest statement this
repository can make about the fp32 kernels' mathematics: they instantiate the same jet / adjoint rules with V = float.
(CPU: the g++ emulation; tests/test_gpu_mirror.py re-runs this module on the hardware.)"""
import numpy as np
import pytest
import sympy as sp

import helpers
import pinn_oracle as po
import test_emu_parity as tp

EXACT = 1e-11


def _engine_f64(npde, wl, param_estim=False):
    rep = npde.symbolic_discretize(wl.pde_system, wl.discretization())
    eng = rep.engine
    sets = rep.pde_train_sets + rep.bcs_train_sets
    eng.set_option("precision", "f64")
    assert eng.get_option("precision") == "f64" and "precision=f64" in eng.describe()
    for k, s in enumerate(sets):
        eng.set_points_f64(k, s)
    prob = helpers.oracle_problem(npde, wl.pde_system, wl.chains, param_estim=wl.param_estim)
    return rep, eng, sets, prob


def _workloads():
    from neuralpde_jl_amd import workloads
    return {"cfg1": lambda: workloads.cfg1_poisson1d(64),
            "cfg2": lambda: workloads.cfg2_poisson2d(points=96, bcs_points=32),
            "cfg3": lambda: workloads.cfg3_burgers(points=1100, bcs_points=32),     # (three blocks of the weight-gradient kernels, the last one ragged)
            "cfg4": lambda: workloads.cfg4_cavity(points=48, bcs_points=16, width=16, hidden=2),
            "cfg5": lambda: workloads.cfg5_heat_inverse(points=64, bcs_points=32, width=16, hidden=2)}


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4", "cfg5"])
def test_f64_mode_equals_the_float64_oracle(npde, use_emu, name):
    """all five BASELINE problem types (1-D / 2-D Poisson, Burgers, the three-network cavity system, the 4-D inverse heat problem with an
    estimated parameter): losses and gradient of the float64 mode against the oracle's exact-derivative mode — equal to rounding; the same
    handle's fp32 evaluation stays available and is 1e-7-accurate"""
    wl = _workloads()[name]()
    rep, eng, sets, prob = _engine_f64(npde, wl)
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = np.linspace(1.0, 2.0, eng.K)
    ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
    l64, g64 = eng.loss_grad_f64(th, w)
    le, g2, gi = helpers.rel_errors(l64, g64, ref)
    assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)
    l2, g2_ = eng.loss_grad_f64(th, w)
    assert np.array_equal(l2, l64) and np.array_equal(g2_, g64)              # deterministic
    # r05: which kernels ran — the matrix-pipe family (csrc/pinn_kernels5.hpp, v_mfma_f64_16x16x4_f64) wherever a (jet set, width) pair is
    # instantiated, one lane per point elsewhere (4-D nets); both families agree to rounding
    # (r06: the 4-D jet set as well — channel-sliced kernels, csrc/pinn_kernels6.hpp)
    assert eng.get_option("f64_path") == "mfma"
    if True:
        import os
        os.environ["PINN_F64_NO_MFMA"] = "1"
        try:
            ll, gl = eng.loss_grad_f64(th, w)
        finally:
            del os.environ["PINN_F64_NO_MFMA"]
        assert eng.get_option("f64_path") == "lanes"
        np.testing.assert_allclose(ll, l64, rtol=1e-12)
        np.testing.assert_allclose(gl, g64, rtol=0, atol=1e-12 * np.abs(g64).max())
    lf, gf = eng.loss_grad(th, w)                                            # float entry point in f64 mode: converted at the boundary
    np.testing.assert_allclose(gf, g64.astype(np.float32), rtol=0, atol=1e-7 * np.abs(g64).max())
    eng.set_option("precision", "f32")
    assert eng.get_option("precision") == "f32"
    l32, g32 = eng.loss_grad_f64(th, w)
    le, g2, gi = helpers.rel_errors(l32, g32, ref)
    assert 1e-9 < g2 < 1e-5 and le.max() < 1e-5                              # (back on the fp32 kernels)


def test_f64_mode_at_trained_parameters_and_lbfgs(npde, use_emu):
    """the regime fp32 cannot follow: parameters after 6,000 float64 Adam steps (committed fixture) — the float64 mode
    still equals the oracle to rounding where the fp32 kernels are off by 1e-4 ... 1e-2; and pinn_lbfgs iterates on the double objective,
    far below the fp32 noise floor"""
    import os
    from neuralpde_jl_amd import workloads
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg2_variants.npz"))
    wl = workloads.cfg2_poisson2d(points=256, bcs_points=64)
    rep, eng, sets, prob = _engine_f64(npde, wl)
    w = g["weights"]
    th = g["theta_adam6000"]
    ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
    l64, g64 = eng.loss_grad_f64(th, w)
    le, g2, gi = helpers.rel_errors(l64, g64, ref)
    assert le.max() < 1e-9 and g2 < 1e-9 and gi < 1e-9, (le, g2, gi)
    eng.set_option("precision", "f32")
    l32, g32 = eng.loss_grad_f64(th, w)
    assert helpers.rel_errors(l32, g32, ref)[1] > 1e-5                       # the fp32 evaluation of the same point: not 1e-5-accurate
    eng.set_option("precision", "f64")
    for k, s in enumerate(sets):
        eng.set_points_f64(k, s)
    # a small quasi-Newton run on a 1-D problem: the objective falls through the fp32 floor
    wl1 = workloads.cfg1_poisson1d(32)
    rep1, eng1, sets1, prob1 = _engine_f64(npde, wl1)
    th0 = np.asarray(rep1.flat_init_params, dtype=np.float64)
    th1, hist = eng1.lbfgs(th0, 3000, history=20, gtol=1e-14)
    assert hist[-1] < 1e-8 and hist[-1] < 1e-9 * hist[0], (hist[0], hist[-1])     # measured 4.2e-10 (from 44.6)
    rep32 = npde.symbolic_discretize(wl1.pde_system, wl1.discretization())
    _, hist32 = rep32.engine.lbfgs(th0, 600, history=20, gtol=1e-14)
    assert hist32[-1] > 50.0 * hist[-1], (hist32[-1], hist[-1])                   # the fp32 objective stalls at its noise floor (2.6e-6 measured)
    ref1 = po.loss_and_grad(prob1, th1, sets1, mode="exact")
    l1, g1 = eng1.loss_grad_f64(th1)
    np.testing.assert_allclose(l1, ref1.term_losses, rtol=1e-5)      # (boundary residuals of 1e-8: eps / 1e-8 is the rounding floor)


def test_f64_mode_derivative_orders_activations_weights(npde, use_emu):
    """third derivative (the reference's 3rd-order ODE, sigma network), a KS-type fourth derivative in 1-D, sin activation, quadrature
    weights; and what the mode does not cover fails at pinn_set_option with a message while the fp32 plan keeps working"""
    from neuralpde_jl_amd import workloads
    def run(sysm, chain, strat, seed, weights=None):
        theta = tp.theta_for(chain, seed)
        disc = npde.PhysicsInformedNN(chain, strat, init_params=theta, precision="f32")
        rep = npde.symbolic_discretize(sysm, disc)
        eng = rep.engine
        sets = rep.pde_train_sets + rep.bcs_train_sets
        eng.set_option("precision", "f64")
        for k, s in enumerate(sets):
            eng.set_points_f64(k, s)
        prob = helpers.oracle_problem(npde, sysm, [chain])
        th = np.asarray(rep.flat_init_params, dtype=np.float64)
        ref = po.loss_and_grad(prob, th, sets, weights=weights, mode="exact")
        l64, g64 = eng.loss_grad_f64(th, weights)
        le, g2, gi = helpers.rel_errors(l64, g64, ref)
        assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)
        return rep, eng, sets
    run(tp._third_order_ode(npde), npde.Chain(npde.Dense(1, 8, "sigmoid"), npde.Dense(8, 1)), npde.GridTraining(0.05), 31)
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    D4 = npde.Differential(x) ** 4
    sys4 = npde.PDESystem([npde.Eq(D4(u(x)) + u(x), sp.sin(x))], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.5)],
                          [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    run(sys4, npde.Chain(npde.Dense(1, 12, "tanh"), npde.Dense(12, 12, "tanh"), npde.Dense(12, 1)), npde.GridTraining(0.05), 5)
    # r05: orders 3 and 4 and a mixed second derivative in TWO dimensions (csrc/inst_f64.hip: f64_d2_h4), and a 3-D case
    x, y = npde.parameters("x y")
    (u,) = npde.variables("u")
    Dx, Dy = npde.Differential(x), npde.Differential(y)
    sys2 = npde.PDESystem([npde.Eq((Dx ** 4)(u(x, y)) + (Dy ** 3)(u(x, y)) + 0.5 * Dx(Dy(u(x, y))) - u(x, y) * Dx(u(x, y)), sp.sin(x) * sp.cos(y))],
                          [npde.Eq(u(0.0, y), 0.0), npde.Eq(u(x, 1.0), x)],
                          [npde.In(x, npde.Interval(0.0, 1.0)), npde.In(y, npde.Interval(0.0, 1.0))], [x, y], [u(x, y)])
    strat2 = npde.QuasiRandomTraining(48, bcs_points=12, sampling_alg=npde.SobolSample(seed=2), resampling=False, minibatch=1)
    rep_h, eng_h, _ = run(sys2, npde.Chain(npde.Dense(2, 12, "tanh"), npde.Dense(12, 12, "tanh"), npde.Dense(12, 1)), strat2, 9)
    assert "f64_channels=10" in eng_h.describe()
    t, x3, y3 = npde.parameters("t x y")
    U3 = u(t, x3, y3)
    Dt, Dx3, Dy3 = npde.Differential(t), npde.Differential(x3), npde.Differential(y3)
    sys3 = npde.PDESystem([npde.Eq(Dt(U3) + (Dx3 ** 4)(U3), (Dy3 ** 2)(U3) + 0.3 * Dx3(Dy3(U3)) + (Dy3 ** 3)(U3))],
                          [npde.Eq(u(0.0, x3, y3), sp.sin(sp.pi * x3) * sp.sin(sp.pi * y3)), npde.Eq(u(t, 0.0, y3), 0.0)],
                          [npde.In(v_, npde.Interval(0.0, 1.0)) for v_ in (t, x3, y3)], [t, x3, y3], [U3])
    strat3 = npde.QuasiRandomTraining(40, bcs_points=12, sampling_alg=npde.SobolSample(seed=4), resampling=False, minibatch=1)
    run(sys3, npde.Chain(npde.Dense(3, 10, "sigmoid"), npde.Dense(10, 10, "sigmoid"), npde.Dense(10, 1)), strat3, 13)
    sysm, chain = tp.poisson2d(npde, act="sin", width=16, hidden=2)
    strat = npde.QuasiRandomTraining(60, bcs_points=20, sampling_alg=npde.SobolSample(seed=3), resampling=False, minibatch=1)
    rep, eng, sets = run(sysm, chain, strat, 11, weights=[1.0, 2.0, 0.5, 1.5, 3.0])
    # quadrature weights on the interior term
    wq = np.random.default_rng(0).random(sets[0].shape[1]).astype(np.float32)
    wq /= wq.sum()
    eng.set_point_weights(0, wq)
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    l64, _ = eng.loss_grad_f64(th)
    prob = helpers.oracle_problem(npde, sysm, [chain])
    r = po.residual_values(prob, th, 0, sets[0], mode="exact").reshape(-1)
    np.testing.assert_allclose(l64[0], float(np.sum(wq.astype(np.float64) * r * r)), rtol=1e-6)      # (the weights are stored as float sqrt(N w))
    # device samplers (r05: covered — the double copy follows every draw; test_f64_mode_resident_adam_samplers_and_device_entry_points): a
    # handle that already redraws a term switches to float64 and evaluates the drawn set in double
    wl = workloads.cfg2_poisson2d(points=64, bcs_points=16)
    rep2 = npde.symbolic_discretize(wl.pde_system, wl.discretization())
    rep2.engine.set_sampler(0, np.zeros(2, np.float32), np.ones(2, np.float32), 64, seed=3, kind=1)
    l32, g32 = rep2.engine.loss_grad_f64(np.asarray(rep2.flat_init_params, dtype=np.float64))
    rep2.engine.set_option("precision", "f64")
    assert rep2.engine.get_option("precision") == "f64"
    l64s, g64s = rep2.engine.loss_grad_f64(np.asarray(rep2.flat_init_params, dtype=np.float64))
    assert 1e-10 < np.linalg.norm(g64s - g32) / np.linalg.norm(g64s) < 1e-5
    # still outside the mode: DGM networks — the switch fails with a message and the fp32 plan stays usable (periodic embeddings: covered since r06,
    # test_f64_periodic_embedding)


def test_reference_pde_iii_system_meets_its_float64_criterion(npde, use_emu):
    """test/NNPDE1/nnpde__pde_iii_3rd_order_ode.jl:58-137 with the reference's OWN criteria: u''' = cos(pi x) as a first-order system of five
    dependent variables (u, Dxu, Dxxu and two slack networks; equations that reference three networks at once), Sobol design of 100 points,
    BFGS until the objective is below 1e-9, then `u_predict ≈ u_real atol = 1e-4`.  The fp32 evaluation stops at 1.9e-7 / 1.6e-4
    (tests/test_gpu_reference_acceptance.py::test_pde_iii_third_order_ode_system_fp32_limit); `PhysicsInformedNN(..., precision = "f64")`
    — what a Float64 init_params selects in the reference — meets both (measured: 9.97e-10 after 2,629 iterations, 2.6e-5)."""
    import math
    (x,) = npde.parameters("x")
    u, Dxu, Dxxu, O1, O2 = npde.variables("u Dxu Dxxu O1 O2")
    Dx = npde.Differential(x)
    eq = npde.Eq(Dx(Dxxu(x)), sp.cos(sp.pi * x))
    ep = (np.finfo(np.float64).eps ** (1 / 3)) ** 2 / 6
    bcs = [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), math.cos(math.pi)), npde.Eq(Dxu(1.0), 1.0),
           npde.Eq(Dxu(x), Dx(u(x)) + ep * O1(x)), npde.Eq(Dxxu(x), Dx(Dxu(x)) + ep * O2(x))]
    dom = [npde.In(x, npde.Interval(0.0, 1.0))]
    wide = lambda: npde.Chain(npde.Dense(1, 12, "tanh"), npde.Dense(12, 12, "tanh"), npde.Dense(12, 1))
    slack = lambda: npde.Chain(npde.Dense(1, 4, "tanh"), npde.Dense(4, 1))
    chains = [wide(), wide(), wide(), slack(), slack()]
    rng = np.random.default_rng(100)
    theta0 = np.concatenate([npde.initialparameters(rng, c) for c in chains])
    strat = npde.QuasiRandomTraining(100, sampling_alg=npde.SobolSample(seed=1), resampling=False, minibatch=1)
    prob = npde.discretize(npde.PDESystem([eq], bcs, dom, [x], [u(x), Dxu(x), Dxxu(x), O1(x), O2(x)]),
                           npde.PhysicsInformedNN(chains, strat, init_params=theta0, precision="f64"))
    assert prob.pinnrep.engine.get_option("precision") == "f64"
    res = npde.solve(prob, npde.BFGS(), maxiters=5000, callback=lambda st, l: l < 1e-9)
    xs = np.arange(0.0, 1.0 + 0.005, 0.01)[None, :]
    real = (np.pi * xs[0] * (-xs[0] + (np.pi ** 2) * (2 * xs[0] - 3) + 1) - np.sin(np.pi * xs[0])) / (np.pi ** 3)
    rep = prob.pinnrep
    err = np.linalg.norm(rep.phi[0](xs, npde.depvar_params(rep, res.u, "u"))[0] - real)
    print(f"pde_iii in float64: objective {res.objective:.3e} (reference: < 1e-9), ||u_predict - u_real||_2 = {err:.2e} (reference atol 1e-4)")
    assert res.objective < 1e-9 and err < 1e-4


def _host_adam(theta, grads, lr, b1=0.9, b2=0.999, eps=1e-8):
    """float64 Adam over a list of gradient callbacks (one per step): the reference's `solve(prob, Adam(lr))` arithmetic"""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))       # (the C ABI takes the hyper-parameters as floats)
    th, m, v = theta.copy(), np.zeros_like(theta), np.zeros_like(theta)
    for t, gfun in enumerate(grads, start=1):
        g = gfun(th)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        th = th - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
    return th


def test_f64_mode_resident_adam_samplers_and_device_entry_points(npde, use_emu):
    """r05: the float64 mode covers the optimiser loop and the device samplers — StochasticTraining /
    QuasiRandomTraining(resampling = true) with the reference's default Float64 parameters (src/discretize.jl:432-449,
    src/training_strategies.jl:271-282, 365-389) no longer falls back to fp32.  (a) pinn_adam_* on fixed sets = a float64 host Adam over the
    mode's own gradients, to rounding; (b) with device samplers: every step's redrawn set read back, the same iterates from a second handle
    evaluated on exactly those points; (c) pinn_loss_grad_device / pinn_loss_device / pinn_term_grads evaluate in double in this mode."""
    from neuralpde_jl_amd import workloads
    wl = workloads.cfg2_poisson2d(points=96, bcs_points=32, width=16, hidden=2)
    rep, eng, sets, prob = _engine_f64(npde, wl)
    th0 = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = np.linspace(1.0, 2.0, eng.K)
    # (a) fixed sets
    th_dev, hist = eng.adam_f64(th0, 12, 3e-3, w)
    assert eng.get_option("f64_path") == "mfma"
    th_host = _host_adam(th0, [lambda th: eng.loss_grad_f64(th, w)[1]] * 12, 3e-3)
    np.testing.assert_allclose(th_dev, th_host, rtol=0, atol=1e-13 * np.abs(th_host).max())
    l0, _ = eng.loss_grad_f64(th0, w)
    assert abs(hist[0] - float(np.dot(w, l0))) < 1e-13 * abs(hist[0])
    th_f32 = eng.adam(th0, 3, 3e-3, w)[0]                                     # the float entry points of the same loop: converted at the boundary
    np.testing.assert_allclose(th_f32, _host_adam(th0, [lambda th: eng.loss_grad_f64(th, w)[1]] * 3, 3e-3).astype(np.float32), rtol=0, atol=2e-7)
    # (b) device samplers in float64 mode: every step's redrawn sets read back, the update reproduced from a second handle's gradient on them
    d = sets[0].shape[0]
    lb, ub = [0.0] * d, [1.0] * d
    eng.set_sampler(0, lb, ub, 80, seed=5, kind=1)
    eng.set_sampler(1, [0.0, 0.0], [0.0, 1.0], 24, seed=6, kind=2)
    rep2, eng2, _, _ = _engine_f64(npde, wl)
    for k, s_ in enumerate(sets):                                              # (a second discretisation draws its own boundary sets: same sets on both handles)
        eng2.set_points_f64(k, s_)
    th_prev, m, v = th0.copy(), np.zeros_like(th0), np.zeros_like(th0)
    seen = []
    for t in range(1, 5):
        th_dev, _ = eng.adam_f64(th0 if t == 1 else None, 1, 3e-3, w, init=(t == 1))
        assert eng.get_option("f64_path") == "mfma"
        for k, n in ((0, 80), (1, 24)):
            pts = eng.get_points(k, d, n).astype(np.float64)
            eng2.set_points_f64(k, pts)
            if k == 0:
                seen.append(pts.copy())
        g = eng2.loss_grad_f64(th_prev, w)[1]
        lr, b1, b2, eps = (float(np.float32(x)) for x in (3e-3, 0.9, 0.999, 1e-8))
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        th_host = th_prev - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
        np.testing.assert_allclose(th_dev, th_host, rtol=0, atol=1e-13 * np.abs(th_host).max())
        th_prev = th_dev
    assert not np.array_equal(seen[0], seen[1]) and seen[0].min() >= 0.0 and seen[0].max() <= 1.0      # (fresh points every step)
    # (c) device-pointer entry points and per-term gradients in float64 mode (emulation: "device" pointers are host pointers)
    rep3, eng3, sets3, _ = _engine_f64(npde, wl)
    l64, g64 = eng3.loss_grad_f64(th0, w)
    th32 = th0.astype(np.float32)
    l64b, g64b = eng3.loss_grad_f64(th32.astype(np.float64), w)
    n_norm = np.array([s.shape[1] for s in sets], dtype=np.float64)
    if eng3.L.backend == "hip":                                                # (the mirror of this test on the hardware: real device memory)
        import torch
        d_th = torch.tensor(th32, device="cuda")
        d_out = torch.zeros(eng3.P + eng3.K, dtype=torch.float32, device="cuda")
        d_sums = torch.zeros(eng3.K, dtype=torch.float32, device="cuda")
        eng3.loss_grad_device(d_th.data_ptr(), d_out.data_ptr(), w)
        eng3.loss_device(d_th.data_ptr(), d_sums.data_ptr())
        torch.cuda.synchronize()
        out, sums = d_out.cpu().numpy(), d_sums.cpu().numpy()
    else:
        out = np.zeros(eng3.P + eng3.K, dtype=np.float32)
        sums = np.zeros(eng3.K, dtype=np.float32)
        eng3.loss_grad_device(th32.ctypes.data, out.ctypes.data, w)
        eng3.loss_device(th32.ctypes.data, sums.ctypes.data)
    # the double device-pointer entry (pinn_loss_grad_device_f64): the host entry's numbers bit for bit, nothing narrowed
    if eng3.L.backend == "hip":
        d_th64 = torch.tensor(th0, dtype=torch.float64, device="cuda")
        d_out64 = torch.zeros(eng3.P + eng3.K, dtype=torch.float64, device="cuda")
        eng3.loss_grad_device_f64(d_th64.data_ptr(), d_out64.data_ptr(), w)
        torch.cuda.synchronize()
        out64 = d_out64.cpu().numpy()
    else:
        out64 = np.zeros(eng3.P + eng3.K, dtype=np.float64)
        eng3.loss_grad_device_f64(th0.ctypes.data, out64.ctypes.data, w)
    assert np.array_equal(out64[:eng3.P], g64) and np.array_equal(out64[eng3.P:] / n_norm, l64)
    eng3.set_option("precision", "f32")
    with pytest.raises(RuntimeError, match="float64 evaluation mode"):
        eng3.loss_grad_device_f64(th0.ctypes.data, out64.ctypes.data, w)
    eng3.set_option("precision", "f64")
    for k, s_ in enumerate(sets3):
        eng3.set_points_f64(k, s_)
    np.testing.assert_allclose(out[:eng3.P], g64b.astype(np.float32), rtol=0, atol=1e-7 * np.abs(g64b).max())
    np.testing.assert_allclose(out[eng3.P:] / n_norm, l64b, rtol=2e-7)
    np.testing.assert_allclose(sums / n_norm, l64b, rtol=2e-7)
    tl, tg = eng3.term_grads(th32)
    np.testing.assert_allclose(tl, l64b, rtol=1e-12)
    np.testing.assert_allclose((tg * w[:, None]).sum(0), g64b, rtol=0, atol=2e-7 * np.abs(g64b).max())


def test_mirror_solve_adam_keeps_theta_in_double(npde, use_emu):
    """`solve(prob, Adam(lr))` of the Python mirror on a `precision = "f64"` discretisation goes through pinn_adam_init_f64 /
    pinn_adam_get_f64: a run cut into chunks by a callback (50 steps per chunk, neuralpde.jl_amd/pinn.py::solve) ends at the same
    parameters as one uninterrupted run to the last bit kept by the device state, and the result is not a float32 value."""
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    Dx = npde.Differential(x)
    eq = npde.Eq(Dx(Dx(u(x))), -sp.sin(x))
    bcs = [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), float(np.sin(1.0)))]
    dom = [npde.In(x, npde.Interval(0.0, 1.0))]
    chain = npde.Chain(npde.Dense(1, 8, "tanh"), npde.Dense(8, 8, "tanh"), npde.Dense(8, 1))
    theta0 = npde.initialparameters(np.random.default_rng(3), chain)

    def run(callback):
        prob = npde.discretize(npde.PDESystem([eq], bcs, dom, [x], [u(x)]),
                               npde.PhysicsInformedNN(chain, npde.GridTraining(0.05), init_params=theta0, precision="f64"))
        assert prob.pinnrep.engine.get_option("precision") == "f64"
        return npde.solve(prob, npde.Adam(0.01), maxiters=120, callback=callback)

    whole, chunks = run(None), run(lambda st, l: False)
    assert whole.u.dtype == np.float64 and np.any(whole.u != whole.u.astype(np.float32))
    assert np.array_equal(whole.u, chunks.u) and np.array_equal(whole.losses, chunks.losses)
    assert whole.losses[-1] < whole.losses[0]


def test_f64_mode_data_misfit_term_and_estimated_parameter(npde, use_emu):
    """A Float64 inverse problem (test/NNPDE2/additional_loss__lorenz_system.jl:66-77 / docs/src/tutorials/param_estim.md:79-95 in the
    reference's default eltype): PDE parameter in theta, observations as per-point DATA channels of a device-side misfit term
    (pinn_set_point_data_f64).  Against (a) the oracle's network values at the observation points, (b) the same objective with the misfit
    as a host-side float64 `additional_loss` (torch autograd) — value and gradient to 1e-11, where the fp32 mode's bar is 1e-5
    (tests/test_reference_examples.py::test_data_misfit_terms_on_device)."""
    import torch
    import pinn_oracle as po
    t, x = npde.parameters("t x")
    (u,) = npde.variables("u")
    (k,) = npde.parameters("k")
    Dt, Dxx = npde.Differential(t), npde.Differential(x) ** 2
    eq = npde.Eq(Dt(u(t, x)), k * Dxx(u(t, x)))
    bcs = [npde.Eq(u(0, x), sp.sin(sp.pi * x)), npde.Eq(u(t, 0), 0.0)]
    dom = [npde.In(t, npde.Interval(0.0, 1.0)), npde.In(x, npde.Interval(0.0, 1.0))]
    chain = npde.Chain(npde.Dense(2, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    th = npde.initialparameters(np.random.default_rng(171), chain)
    mk = lambda: npde.QuasiRandomTraining(40, bcs_points=16, sampling_alg=npde.SobolSample(seed=8), resampling=False, minibatch=1)
    pts = np.random.default_rng(3).uniform(size=(2, 37))
    vals = np.exp(-0.3 * np.pi ** 2 * pts[0]) * np.sin(np.pi * pts[1])
    sysm = npde.PDESystem([eq], bcs, dom, [t, x], [u(t, x)], ps=[k], defaults={k: 0.7})
    weights = npde.NonAdaptiveLoss(pde_loss_weights=1.0, bc_loss_weights=2.0, additional_loss_weights=0.5)
    prob = npde.discretize(sysm, npde.PhysicsInformedNN(chain, mk(), init_params=th, param_estim=True, precision="f64", adaptive_loss=weights,
                                                        data_loss=[npde.DataLoss(u(t, x), pts, vals, weight=3.0)]))
    rep = prob.pinnrep
    assert rep.engine.get_option("precision") == "f64"
    theta = rep.flat_init_params
    oc = po.Chain(tuple(chain.sizes), chain.act)
    u_at = po.phi_values(oc, theta[:chain.nparams], pts).reshape(-1)
    dl = rep.loss_functions.data_loss_functions[0](theta)
    assert abs(dl - np.mean((u_at - vals) ** 2)) < 1e-12 * dl

    def additional(phi, th_net, p):
        tt = torch.tensor(np.asarray(th_net), dtype=torch.float64, requires_grad=True)
        out = oc(torch.tensor(pts, dtype=torch.float64), tt).reshape(-1)
        val = 3.0 * torch.mean((out - torch.tensor(vals, dtype=torch.float64)) ** 2)
        (gr,) = torch.autograd.grad(val, tt)
        return float(val.detach()), np.concatenate([gr.numpy(), np.zeros(1)])
    prob_h = npde.discretize(sysm, npde.PhysicsInformedNN(chain, mk(), init_params=th, param_estim=True, precision="f64", adaptive_loss=weights,
                                                          additional_loss=additional))
    v_d, g_d = prob.f.value_and_grad(theta)
    v_h, g_h = prob_h.f.value_and_grad(theta)
    print(f"float64 inverse problem: objective {v_d:.12e} (host misfit {v_h:.12e}), gradient rel L2 {np.linalg.norm(g_d - g_h) / np.linalg.norm(g_h):.2e}")
    assert abs(v_d - v_h) < 1e-11 * abs(v_h)
    assert np.linalg.norm(g_d - g_h) < 1e-11 * np.linalg.norm(g_h)
    assert g_d[-1] != 0.0                                   # (the estimated parameter's slot)
    # points re-installed without their observations: refused, as in the fp32 mode
    rep.engine.set_points_f64(3, pts)
    with pytest.raises(RuntimeError, match="per-point data"):
        rep.engine.loss_grad_f64(theta)
    rep.engine.set_point_data_f64(3, vals[None, :])
    assert abs(rep.engine.loss_grad_f64(theta, want_grad=False)[0][3] - dl) < 1e-13 * dl
    res = npde.solve(prob, npde.Adam(0.01), maxiters=30)
    assert res.u.dtype == np.float64 and res.losses[-1] < res.losses[0]


# ---- r06: float64 through the WHOLE boundary — every public closure of the reference in eltype(theta) = Float64 ----
def test_forward_derivatives_pin_at_the_reference_tolerances_f64(npde, use_emu):
    """test/Forward/forward__derivatives.jl:7-44 through the C ABI in float64 mode AT THE REFERENCE'S OWN TOLERANCES: a 2 -> 16 -> 16 -> 1
    sigmoid chain at [1, 2]; pinn_derivative_f64 (the engine's numeric_derivative: exact Taylor jets) against Zygote's role (the oracle's
    exact derivatives) and against the reference's central differences with its get_eps steps — first order atol 1e-8, second order
    (xx, xy, yy) atol 4e-5 (:29-30, :40-43).  (tests/test_emu_parity.py::test_forward_derivatives_mirror is the fp32 path's version: 2e-6.)"""
    import torch
    sysm, _ = helpers.shape_problem(npde, 16, 2, 2)
    chain = npde.Chain(npde.Dense(2, 16, "sigmoid"), npde.Dense(16, 16, "sigmoid"), npde.Dense(16, 1))
    ochain = po.Chain((2, 16, 16, 1), "sigmoid")
    u = lambda cord, th, phi: phi(cord, th).sum(dim=0, keepdim=True)      # u_ of the reference test
    x = np.array([[1.0], [2.0]])
    xt = torch.tensor(x, dtype=po.DT)
    for seed in range(3):
        theta = po.glorot_theta(ochain, np.random.default_rng(seed), bias_amp=0.0)
        rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.25), init_params=theta, precision="f64"))
        eng = rep.engine
        assert eng.get_option("precision") == "f64"
        tht = torch.tensor(theta, dtype=po.DT)
        assert abs(eng.phi_f64(0, theta, x)[0] - float(ochain(xt, tht))) < 1e-14                       # phi([1, 2], theta)
        for ax in (0, 1):
            got = float(eng.derivative_f64(0, theta, x, [ax])[0])
            fd = float(po.numeric_derivative(ochain, u, xt, [po.get_eps(2, ax + 1, np.float64, 1)], 1, tht))
            ex = float(po.exact_derivative(ochain, u, xt, [ax], tht))
            assert abs(got - ex) < 1e-14 and abs(got - fd) < 1e-8, (ax, got, ex, fd)                   # forward__derivatives.jl:29-30: atol 1e-8
        ex_, ey_ = po.get_eps(2, 1, np.float64, 2), po.get_eps(2, 2, np.float64, 2)
        for epss, axes in [([ex_, ex_], [0, 0]), ([ex_, ey_], [0, 1]), ([ey_, ey_], [1, 1])]:
            got = float(eng.derivative_f64(0, theta, x, axes)[0])
            fd = float(po.numeric_derivative(ochain, u, xt, epss, 2, tht))
            ex = float(po.exact_derivative(ochain, u, xt, axes, tht))
            assert abs(got - ex) < 1e-13 and abs(got - fd) < 4e-5, (axes, got, ex, fd)                 # :40-43: atol 4e-5
        # the float entry points of a handle in float64 mode run the same double kernels and narrow at the boundary
        assert abs(float(eng.derivative(0, theta, x, [0])[0]) - float(eng.derivative_f64(0, theta, x, [0])[0])) < 1e-7
        assert abs(float(eng.phi(0, theta, x)[0]) - float(eng.phi_f64(0, theta, x)[0])) < 1e-7
    pts = np.random.default_rng(5).uniform(0, 1, size=(2, 700))      # two chunks of the lanes kernels' blocks, ragged
    for axes in ([], [0], [1], [0, 0], [0, 1], [1, 1]):
        got = eng.derivative_f64(0, theta, pts, axes)
        ex = po.exact_derivative(ochain, u, torch.tensor(pts, dtype=po.DT), axes, tht).detach().numpy().reshape(-1)
        assert np.max(np.abs(got - ex)) < 1e-13 * max(1.0, np.max(np.abs(ex))), axes
    with pytest.raises(Exception, match="no float64 kernel carries"):
        eng.derivative_f64(0, theta, pts, [0, 0, 1])                 # mixed third derivative: fp32 generated jet sets only
    with pytest.raises(Exception, match="axis out of range"):
        eng.derivative_f64(0, theta, pts, [2])
    # an fp32 handle: the double entry points narrow / widen at the boundary (fp32 kernels)
    eng.set_option("precision", "f32")
    got = eng.derivative_f64(0, theta, pts, [0, 0])
    ex = po.exact_derivative(ochain, u, torch.tensor(pts, dtype=po.DT), [0, 0], tht).detach().numpy().reshape(-1)
    assert 1e-10 < np.max(np.abs(got - ex)) < 1e-5


def test_forward_ode_pin_at_the_reference_tolerance_f64(npde, use_emu):
    """test/Forward/forward__ode.jl:10-47 in float64 mode: chain x -> x.^2 is not expressible as Dense layers, so the same statement on a
    network: the datafree residual closure of `Dx(u(x)) ~ 0` on the GridTraining(0.1) set (BC argument 0.0 removed: 0.1 ... 1.0) equals
    du/dx at rtol 1e-8 (:46-47) — through pinn_residual_f64, and through the mirror's datafree_pde_loss_functions under precision = "f64"."""
    import torch
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    U = u(x)
    sysm = npde.PDESystem([npde.Eq(npde.Differential(x)(U), 0.0)], [npde.Eq(u(0.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [U])
    chain = npde.Chain(npde.Dense(1, 12, "tanh"), npde.Dense(12, 12, "tanh"), npde.Dense(12, 1))
    ochain = po.Chain((1, 12, 12, 1), "tanh")
    theta = po.glorot_theta(ochain, np.random.default_rng(3))
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta, precision="f64"))
    train = rep.pde_train_sets[0]
    assert train.shape[0] == 1 and train.shape[1] >= 10                             # (0.1 ... 1.0, with or without the BC's own 0.0: strategies.py keeps the v6.2.2 `dif` quirk)
    uf = lambda cord, th, phi: phi(cord, th)
    tht = torch.tensor(theta, dtype=po.DT)
    exact = po.exact_derivative(ochain, uf, torch.tensor(train, dtype=po.DT), [0], tht).detach().numpy().reshape(-1)
    r = rep.engine.residual_f64(0, theta, train.shape[1])
    np.testing.assert_allclose(r, exact, rtol=1e-12)
    r2 = rep.loss_functions.datafree_pde_loss_functions[0](train, theta)            # the reference's public closure (pinn_types.jl:435-439)
    assert r2.dtype == np.float64 and r2.shape == (1, train.shape[1])
    np.testing.assert_allclose(r2.reshape(-1), exact, rtol=1e-8)                    # forward__ode.jl:46-47
    fd = po.numeric_derivative(ochain, uf, torch.tensor(train, dtype=po.DT), [po.get_eps(1, 1, np.float64, 1)], 1, tht).detach().numpy().reshape(-1)
    np.testing.assert_allclose(r2.reshape(-1), fd, rtol=1e-8, atol=1e-9)            # = the reference's own stencil value to its pin


@pytest.mark.parametrize("name", ["cfg2", "cfg4", "cfg5"])
def test_f64_per_point_and_per_term_entry_points(npde, use_emu, name):
    """pinn_residual_f64 / pinn_term_grads_f64 / pinn_loglik_grad_f64 on a handle in float64 mode against the float64 oracle: a single-network
    problem on the matrix-pipe kernels, the three-network system, the 4-D inverse problem (lanes kernels, estimated parameter)"""
    wl = _workloads()[name]()
    rep, eng, sets, prob = _engine_f64(npde, wl)
    th = np.asarray(rep.flat_init_params, dtype=np.float64) * 1.0
    for k in range(eng.K):
        r = eng.residual_f64(k, th, sets[k].shape[1])
        ref = po.residual_values(prob, th, k, sets[k], mode="exact")
        assert np.max(np.abs(r - ref)) < 1e-12 * max(1.0, np.max(np.abs(ref))), k
        rf = eng.residual(k, th, sets[k].shape[1])                                   # float entry point: same kernels, narrowed
        assert rf.dtype == np.float32 and np.max(np.abs(rf - ref)) < 2e-7 * max(1.0, np.max(np.abs(ref)))
    L, tg = eng.term_grads_f64(th)
    assert tg.dtype == np.float64 and tg.shape == (eng.K, eng.P)
    for k in range(eng.K):
        w = np.zeros(eng.K)
        w[k] = 1.0
        ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
        assert abs(L[k] - ref.term_losses[k]) < EXACT * abs(ref.term_losses[k])
        assert np.linalg.norm(tg[k] - ref.grad) < EXACT * np.linalg.norm(ref.grad), k
    # BPINN log-likelihood: ll = sum_k [-N/2 log 2pi - N log s - SSE/(2 s^2)], d/dtheta, d/ds
    stds = np.linspace(0.05, 0.2, eng.K)
    ll, g, gs = eng.loglik_grad_f64(th, stds)
    N = np.array([s.shape[1] for s in sets], dtype=np.float64)
    w = N / (2.0 * stds ** 2)
    ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
    sse = ref.term_losses * N
    ll_ref = float(np.sum(-0.5 * N * np.log(2 * np.pi) - N * np.log(stds) - sse / (2 * stds ** 2)))
    assert abs(ll - ll_ref) < 1e-12 * abs(ll_ref)
    assert np.linalg.norm(g + ref.grad) < EXACT * np.linalg.norm(ref.grad)
    np.testing.assert_allclose(gs, -N / stds + sse / stds ** 3, rtol=1e-11)
    ll32, g32, _ = eng.loglik_grad(th, stds)                                         # float entry point in float64 mode: evaluated in double
    assert abs(ll32 - ll) < 1e-6 * abs(ll) and np.linalg.norm(g32 - g) < 1e-5 * np.linalg.norm(g)      # (theta itself is narrowed to float at that boundary)


@pytest.mark.parametrize("name", ["cfg2", "cfg4"])
def test_float_and_double_twins_follow_one_precision_rule(npde, use_emu, name):
    """every float / double pair of host entry points evaluates in the HANDLE'S precision and converts at the ABI boundary: on a handle in
    float64 mode the float entry point returns the narrowed double result, on an fp32 handle the double entry point returns the widened
    float result — bit for bit, since every double input below is a float and both kernel paths are deterministic"""
    from neuralpde_jl_amd import workloads
    wl = {"cfg2": lambda: workloads.cfg2_poisson2d(points=40, bcs_points=12, width=16, hidden=2),
          "cfg4": lambda: workloads.cfg4_cavity(points=40, bcs_points=12, width=16, hidden=2)}[name]()
    rep64, e64, sets, _ = _engine_f64(npde, wl)
    e32 = npde.symbolic_discretize(wl.pde_system, wl.discretization()).engine
    e32.set_option("precision", "f32")
    for k, s in enumerate(sets):
        e32.set_points_f64(k, s)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    th = f32(rep64.flat_init_params).astype(np.float64)
    w = f32(np.linspace(1.0, 2.0, e64.K)).astype(np.float64)
    stds = f32(np.linspace(0.05, 0.2, e64.K)).astype(np.float64)
    pts = f32(np.random.default_rng(3).uniform(0, 1, size=(2, 37))).astype(np.float64)
    for eng in (e64, e32):
        # narrow: the float entry point's output as the narrowing of the double one (f64 handle), or the double one's as the widening (fp32)
        if eng is e64:
            same = lambda lo, hi: np.array_equal(lo, f32(hi)) and lo.dtype == np.float32
        else:
            same = lambda lo, hi: np.array_equal(hi, np.asarray(lo, dtype=np.float64)) and lo.dtype == np.float32
        for want_grad in (True, False):
            lf, gf = eng.loss_grad(f32(th), f32(w), want_grad=want_grad)
            ld, gd = eng.loss_grad_f64(th, w, want_grad=want_grad)
            assert np.array_equal(lf, ld) and (gf is None and gd is None or same(gf, gd)), (eng is e64, want_grad)
        llf, gf, gsf = eng.loglik_grad(f32(th), stds)
        lld, gd, gsd = eng.loglik_grad_f64(th, stds)
        assert llf == lld and np.array_equal(gsf, gsd) and same(gf, gd)
        Lf, tgf = eng.term_grads(f32(th))
        Ld, tgd = eng.term_grads_f64(th)
        assert np.array_equal(Lf, Ld) and same(tgf, tgd)
        for k in range(eng.K):
            assert same(eng.residual(k, f32(th), sets[k].shape[1]), eng.residual_f64(k, th, sets[k].shape[1])), k
        for net in range(len(wl.chains)):
            assert same(eng.phi(net, f32(th), f32(pts)), eng.phi_f64(net, th, pts)), net
            for axes in ([0], [0, 1]):
                assert same(eng.derivative(net, f32(th), f32(pts), axes), eng.derivative_f64(net, th, pts, axes)), (net, axes)
        tf, hf = eng.adam(f32(th), 2, 1e-3)
        td, hd = eng.adam_f64(th, 2, 1e-3)
        assert np.array_equal(hf, hd) and same(tf, td)
        assert same(eng.adam_get(), eng.adam_get_f64())


def test_f64_adam_iterate_survives_evaluations_between_chunks(npde, use_emu):
    """in float64 mode the Adam iterate lived in the evaluation buffer — any evaluation between two pinn_adam_steps calls
    (adaptive reweighting, a callback that evaluates the loss) destroyed it.  The iterate has its own buffer now: a chunked run with
    evaluations in between equals the unchunked run bit for bit, and solve() with GradientScaleAdaptiveLoss / a loss-evaluating callback runs."""
    from neuralpde_jl_amd import workloads
    wl = workloads.cfg1_poisson1d(48)
    rep, eng, sets, prob = _engine_f64(npde, wl)
    th0 = np.asarray(rep.flat_init_params, dtype=np.float64)
    ref_th, ref_hist = eng.adam_f64(th0, 12, 1e-3)
    th, h1 = eng.adam_f64(th0, 5, 1e-3)
    eng.loss_grad_f64(th0 * 0.5)                           # an evaluation at OTHER parameters between the chunks
    eng.term_grads_f64(th0 * 0.25)
    eng.residual_f64(0, th0 * 2.0, sets[0].shape[1])
    th, h2 = eng.adam_f64(None, 7, 1e-3, init=False)
    assert np.array_equal(np.concatenate([h1, h2]), ref_hist) and np.array_equal(th, ref_th)
    # pinn_adam_apply on the float64 state: one host-driven update equals the resident loop's first step
    l0, g0 = eng.loss_grad_f64(th0)
    eng.adam_f64(th0, 1, 1e-3)                             # reference: theta after one resident step
    one = eng.adam_f64(th0, 1, 1e-3)[0]
    eng.L.check(eng.L.lib.pinn_adam_init_f64(eng.h, th0.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_double)), th0.size), "init")
    raw = l0 * np.array([s.shape[1] for s in sets], dtype=np.float64)
    eng.adam_apply(np.concatenate([g0, raw]), 1e-3)
    got = np.zeros(eng.P)
    import ctypes as C
    eng.L.check(eng.L.lib.pinn_adam_get_f64(eng.h, got.ctypes.data_as(C.POINTER(C.c_double)), got.size), "get")
    np.testing.assert_allclose(got, one, rtol=0, atol=2e-10)                         # (the gradient crosses pinn_adam_apply's float boundary)
    # the mirror's solve(): adaptive reweighting between chunks + a callback that evaluates the loss
    disc = npde.PhysicsInformedNN(wl.chains[0], wl.strategy, init_params=th0, precision="f64",
                                  adaptive_loss=npde.GradientScaleAdaptiveLoss(4))
    prob2 = npde.discretize(wl.pde_system, disc)
    seen = []
    def cb(state, loss):
        seen.append(prob2.f(state["u"]))
        return False
    res = npde.solve(prob2, npde.Adam(1e-3), maxiters=12, callback=cb)
    assert len(seen) >= 3 and np.all(np.isfinite(seen)) and np.isfinite(res.objective) and res.u.dtype == np.float64


def test_precision_policy_follows_eltype_of_theta(npde, use_emu):
    """the glue's precision policy = the reference's contract, compute dtype = eltype(theta) (src/eltype_matching.jl:8-10,
    src/discretize.jl:432-449): PhysicsInformedNN(...) [precision = "auto"] runs the float64 kernels for Float64 parameters (incl. the default
    init_params = None) and the fp32 kernels for Float32 init_params; "f32" on Float64 parameters is the explicit fast opt-in; a problem the
    float64 kernels do not cover fails at discretize time under "auto" — with the reason and the opt-in spelled out, never a silent narrowing"""
    from neuralpde_jl_amd import workloads
    wl = workloads.cfg2_poisson2d(points=64, bcs_points=16)
    chain, strat = wl.chains[0], wl.strategy
    prob = helpers.oracle_problem(npde, wl.pde_system, wl.chains)
    for init, want in ((None, "f64"), (wl.theta.astype(np.float64), "f64"), (wl.theta.astype(np.float32), "f32")):
        rep = npde.symbolic_discretize(wl.pde_system, npde.PhysicsInformedNN(chain, strat, init_params=init))
        assert rep.engine.get_option("precision") == want, (None if init is None else init.dtype, want)
        assert rep.flat_init_params.dtype == (np.float32 if want == "f32" else np.float64)
        th = rep.flat_init_params
        val, g = rep._value_and_grad(th)
        assert g.dtype == th.dtype
        ref = po.loss_and_grad(prob, np.asarray(th, dtype=np.float64), rep.pde_train_sets + rep.bcs_train_sets, mode="exact")
        g2 = np.linalg.norm(g - ref.grad) / np.linalg.norm(ref.grad)
        assert (g2 < 1e-11) if want == "f64" else (1e-9 < g2 < 1e-5), (want, g2)
        # phi and the datafree residual closures compute in the same dtype
        x = np.array([[0.3, 0.6], [0.2, 0.9]])
        ph = rep.phi(x, th)
        exact = po.phi_values(prob.chains[0], np.asarray(th, dtype=np.float64), x).reshape(1, -1)
        err = np.max(np.abs(ph - exact))
        assert (err < 1e-14) if want == "f64" else (1e-10 < err < 1e-5)
    rep = npde.symbolic_discretize(wl.pde_system, npde.PhysicsInformedNN(chain, strat, init_params=wl.theta, precision="f32"))
    assert rep.engine.get_option("precision") == "f32"                               # the explicit fast opt-in on Float64 parameters
    assert wl.discretization().precision == "f32" and wl.discretization("auto").precision == "auto"      # (the benchmark workloads opt in explicitly)
    # DGM networks have fp32 kernels only: "auto" + Float64 parameters refuses, naming the opt-in
    t, x = npde.parameters("t x")
    (u,) = npde.variables("u")
    sysd = npde.PDESystem([npde.Eq(npde.Differential(t)(u(t, x)) + npde.Differential(x)(u(t, x)), 0)], [npde.Eq(u(0, x), sp.sin(x))],
                          [npde.In(t, npde.Interval(0.0, 1.0)), npde.In(x, npde.Interval(0.0, 1.0))], [t, x], [u(t, x)])
    with pytest.raises(npde.EngineError, match='DGM networks are not covered by the float64 mode(.|\n)*precision = "f32"'):
        npde.discretize(sysd, npde.DeepGalerkin(2, 1, 8, 1, "tanh", "tanh", "identity", npde.GridTraining(0.25)))
    npde.discretize(sysd, npde.DeepGalerkin(2, 1, 8, 1, "tanh", "tanh", "identity", npde.GridTraining(0.25), precision="f32"))
    with pytest.raises(ValueError, match="precision must be"):
        npde.PhysicsInformedNN(chain, strat, precision="f16")


# ---- r06: the reference-semantics validation mode, pinn_set_option(h, "derivative", "stencil") ----
def _permutation(chain, nparams_total, rng):
    """index vector `idx` of the same network with the neurons of every hidden layer permuted: theta[idx] parametrises the identical function
    (another summation order in every layer), and its gradient is grad[idx]"""
    ix = np.arange(nparams_total)
    sizes, out, o, perm_in = chain.sizes, [], 0, None
    for l in range(len(sizes) - 1):
        n_in, n_out = sizes[l], sizes[l + 1]
        W = ix[o:o + n_in * n_out].reshape(n_in, n_out).T.copy()       # (out x in) from the column-major flat block
        b = ix[o + n_in * n_out:o + n_in * n_out + n_out].copy()
        o += n_in * n_out + n_out
        if perm_in is not None:
            W = W[:, perm_in]
        perm_out = rng.permutation(n_out) if l < len(sizes) - 2 else np.arange(n_out)
        W, b = W[perm_out], b[perm_out]
        out += [W.T.reshape(-1), b]
        perm_in = perm_out
    return np.concatenate(out + [ix[o:]])


def _stencil_noise(prob, th, sets, w, st, seeds=(11, 12)):
    """the stencil oracle against ITSELF on the same function with permuted hidden neurons (first network): the reproducibility of the
    reference's finite-difference numbers across summation orders, as (loss rel, grad rel L2, grad rel Linf) maxima over the seeds"""
    worst = np.zeros(3)
    for seed in seeds:
        idx = _permutation(prob.chains[0], len(th), np.random.default_rng(seed))
        stp = po.loss_and_grad(prob, th[idx], sets, weights=w, mode="stencil")
        gp = st.grad[idx]
        worst = np.maximum(worst, [np.max(np.abs(stp.term_losses - st.term_losses) / np.abs(st.term_losses)),
                                   np.linalg.norm(stp.grad - gp) / np.linalg.norm(gp), np.max(np.abs(stp.grad - gp)) / np.max(np.abs(gp))])
    return worst


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg4", "cfg5"])
def test_stencil_mode_reproduces_the_reference_finite_differences(npde, use_emu, name):
    """derivative = "stencil": every derivative slot evaluated as the reference's central differences (numeric_derivative,
    src/pinn_types.jl:445-482, steps get_eps = eps(Float64)^(1/(2+order)), src/symbolic_utilities.jl:98-103, in the reference's order of
    operations) — losses, gradient and the datafree residuals against the STENCIL oracle.  The yardstick is the stencil's own noise floor:
    u(x +- eps) carries ~1e-16 relative rounding error and the difference formulas multiply it by 1 / eps^2 ~ 7e7, so ANY two correct
    implementations differ by ~1e-8 in a second derivative — measured here as the stencil oracle against ITSELF on the same network with its
    hidden neurons permuted (the identical function, another summation order: `_stencil_noise`).  The engine must sit within 4 x that."""
    wl = _workloads()[name]()
    rep, eng, sets, prob = _engine_f64(npde, wl)
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = np.linspace(1.0, 2.0, eng.K)
    st = po.loss_and_grad(prob, th, sets, weights=w, mode="stencil")
    noise = _stencil_noise(prob, th, sets, w, st)          # the stencil oracle's own reproducibility (systems: the first network's neurons permuted)
    eng.set_option("derivative", "stencil")
    assert eng.get_option("derivative") == "stencil"
    l, g = eng.loss_grad_f64(th, w)
    le, g2, gi = helpers.rel_errors(l, g, st)
    ex = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
    fd = helpers.rel_errors(st.term_losses, st.grad, ex)
    print(f"\n{name}: engine(stencil) vs stencil oracle: loss {le.max():.1e} grad L2 {g2:.1e} Linf {gi:.1e}; the oracle against its permuted self: loss {noise[0]:.1e} "
          f"grad L2 {noise[1]:.1e} Linf {noise[2]:.1e}; stencil vs exact oracle: loss {fd[0].max():.1e} grad {fd[1]:.1e}")
    assert le.max() < 4 * max(noise[0], 2e-9) and g2 < 4 * max(noise[1], 2e-9) and gi < 4 * max(noise[2], 2e-9), (le, g2, gi, noise)
    lo, _ = eng.loss_grad_f64(th, w, want_grad=False)
    assert np.array_equal(lo, l)                                               # loss-only evaluation: the same sums
    l2, g2_ = eng.loss_grad_f64(th, w)
    assert np.array_equal(l2, l) and np.array_equal(g2_, g)                    # deterministic
    for k in range(eng.K):
        r = eng.residual_f64(k, th, sets[k].shape[1])
        rr = po.residual_values(prob, th, k, sets[k], mode="stencil")
        assert np.max(np.abs(r - rr)) < 2e-6 * max(1.0, np.max(np.abs(rr))), k   # (per-point noise: ~1e-16 |u| / eps^2)
    eng.set_option("derivative", "exact")
    l3, g3 = eng.loss_grad_f64(th, w)
    assert max(helpers.rel_errors(l3, g3, ex)[1:]) < EXACT


def test_stencil_mode_at_trained_parameters_and_higher_orders(npde, use_emu):
    """at TRAINED parameters the reference's finite differences and exact derivatives give gradients ~1e-3 apart (cfg2 after 6,000 Adam steps:
    8e-4 at full size) — the stencil mode is held to the reproducibility of the reference's own numbers there; third / fourth order formulas
    and a mixed derivative (the recursion of :454-460) against the stencil oracle; the mode needs the float64 evaluation and says so"""
    import os
    from neuralpde_jl_amd import workloads
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg2_variants.npz"))
    wl = workloads.cfg2_poisson2d(points=768, bcs_points=64)
    rep, eng, sets, prob = _engine_f64(npde, wl)
    th, w = g["theta_adam6000"], g["weights"]
    st = po.loss_and_grad(prob, th, sets, weights=w, mode="stencil")
    ex = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
    fd = helpers.rel_errors(st.term_losses, st.grad, ex)
    l, gr = eng.loss_grad_f64(th, w)
    e_exact = helpers.rel_errors(l, gr, st)                                    # the exact-derivative kernels against the REFERENCE's semantics
    eng.set_option("derivative", "stencil")
    l, gr = eng.loss_grad_f64(th, w)
    e_sten = helpers.rel_errors(l, gr, st)
    noise = _stencil_noise(prob, th, sets, w, st, seeds=(1, 2, 3))
    print(f"\ncfg2 adam6000 (768 + 4 x 64 points): stencil vs exact oracle grad L2 {fd[1]:.1e}; engine exact mode vs stencil oracle {e_exact[1]:.1e}; engine stencil mode vs "
          f"stencil oracle: loss {e_sten[0].max():.1e} grad L2 {e_sten[1]:.1e} Linf {e_sten[2]:.1e}; the stencil oracle against its permuted self: loss {noise[0]:.1e} grad L2 {noise[1]:.1e} Linf {noise[2]:.1e}")
    # FINDING (r06): at trained parameters the reference's finite-difference gradient is itself reproducible only to ~1e-4 relative — the
    # oracle against the SAME function with permuted neurons moves by as much as the engine's stencil mode differs from it; most of the
    # "8e-4 finite-difference error" of such a point is this rounding noise (1e-16 |u| / eps^2 per point against a gradient that is a small
    # difference of large terms), not truncation error.  The engine's stencil mode is held to that floor (x 4); the losses — sums of squares,
    # where the per-point noise averages out — agree to ~1e-6
    assert e_sten[0].max() < 4 * max(noise[0], 1e-8) and e_sten[1] < 4 * noise[1] and e_sten[2] < 4 * noise[2], (e_sten, noise)
    # orders 3 and 4 in 1-D (test/NNPDE1/nnpde__pde_iii_3rd_order_ode.jl; a KS-type fourth derivative), a mixed second derivative in 2-D
    def run(sysm, chain, strat, seed):
        theta = tp.theta_for(chain, seed)
        rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=theta, precision="f64"))
        e = rep.engine
        e.set_option("derivative", "stencil")
        sets_ = rep.pde_train_sets + rep.bcs_train_sets
        pr = helpers.oracle_problem(npde, sysm, [chain])
        th_ = np.asarray(rep.flat_init_params, dtype=np.float64)
        ref = po.loss_and_grad(pr, th_, sets_, mode="stencil")
        l_, g_ = e.loss_grad_f64(th_)
        le, g2, gi = helpers.rel_errors(l_, g_, ref)
        exr = po.loss_and_grad(pr, th_, sets_, mode="exact")
        return le.max(), g2, helpers.rel_errors(ref.term_losses, ref.grad, exr)[1]
    le, g2, fd3 = run(tp._third_order_ode(npde), npde.Chain(npde.Dense(1, 8, "sigmoid"), npde.Dense(8, 1)), npde.GridTraining(0.05), 31)
    assert le < 1e-4 * max(1.0, fd3 / 1e-6) and g2 < 1e-3, (le, g2, fd3)       # (order 3: eps = 7.4e-4, noise 1e-16 / eps^3 ~ 2.5e-7 per point)
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    D4 = npde.Differential(x) ** 4
    sys4 = npde.PDESystem([npde.Eq(D4(u(x)) + u(x), sp.sin(x))], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.5)],
                          [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    le, g2, fd4 = run(sys4, npde.Chain(npde.Dense(1, 10, "tanh"), npde.Dense(10, 10, "tanh"), npde.Dense(10, 1)), npde.GridTraining(0.05), 32)
    assert le < 1e-3 and g2 < 1e-3, (le, g2, fd4)                              # (order 4: eps = 2.5e-3, noise 1e-16 / eps^4 ~ 2.7e-6 per point)
    sysm, chain = helpers.shape_problem(npde, 16, 2, 2)                        # u_xx + u_yy + 0.5 u_xy - u u_x: the mixed derivative takes the recursion
    le, g2, fdm = run(sysm, chain, npde.GridTraining(0.25), 33)
    assert le < 1e-6 and g2 < 1e-6, (le, g2, fdm)
    # an fp32 handle refuses the option with the reason
    rep32 = npde.symbolic_discretize(wl.pde_system, wl.discretization("f32"))
    with pytest.raises(npde.EngineError, match="validation mode of the float64 evaluation"):
        rep32.engine.set_option("derivative", "stencil")
    assert rep32.engine.get_option("derivative") == "exact"


# ---- r06: family 4s — the channel-sliced matrix-pipe kernels (csrc/pinn_kernels6.hpp) for 128-wide nets and the 3-D / 4-D jet sets ----
@pytest.mark.parametrize("name", ["cfg4_128", "cfg4_100", "cfg5_128", "cfg5_64", "hess3d_64", "poisson1d_128", "poisson2d_128"])
def test_sliced_matrix_pipe_kernels_equal_the_oracle(npde, use_emu, name):
    """BASELINE configs 4 and 5 at their true width (three 128-wide nets; the 4-D set {u, u_t, u_x, u_y, u_z, u_xx, u_yy, u_zz} on a 128-wide
    net), a width that is not a multiple of 16, the 3-D Hessian set, 1-D and 2-D 128-wide nets: losses, gradient, loss-only evaluation and the
    datafree residuals of the float64 mode on the sliced v_mfma_f64 kernels against the float64 oracle — to rounding — and against the
    lane-per-point family on the same handle; point counts that leave ragged tiles and (hess3d) several 512-point blocks"""
    import dataclasses
    import os
    from neuralpde_jl_amd import workloads
    if name.startswith("cfg4"):
        wl = workloads.cfg4_cavity(points=40, bcs_points=20, width=int(name.split("_")[1]), hidden=3 if name.endswith("128") else 2)
    elif name.startswith("cfg5"):
        wl = workloads.cfg5_heat_inverse(points=50, bcs_points=24, width=int(name.split("_")[1]), hidden=2 if name.endswith("128") else 3)
    elif name == "hess3d_64":
        sysm, chain = helpers.shape_problem(npde, 64, 2, 3)
        strat = npde.QuasiRandomTraining(1100, bcs_points=40, sampling_alg=npde.SobolSample(seed=3), resampling=False, minibatch=1)
        wl = workloads.Workload("hess3d", sysm, [chain], strat, tp.theta_for(chain, 77))
    elif name == "poisson1d_128":
        wl = workloads.cfg1_poisson1d(70)
        ch = workloads.mlp(1, 128, 2)
        wl = dataclasses.replace(wl, chains=[ch], theta=workloads.synthetic_theta([ch], 5))
    else:
        wl = workloads.cfg2_poisson2d(points=90, bcs_points=20)
        ch = workloads.mlp(2, 128, 2)
        wl = dataclasses.replace(wl, chains=[ch], theta=workloads.synthetic_theta([ch], 6))
    rep, eng, sets, prob = _engine_f64(npde, wl)
    assert "mfma-sliced" in eng.describe()
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = np.linspace(1.0, 2.0, eng.K)
    ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
    l64, g64 = eng.loss_grad_f64(th, w)
    assert eng.get_option("f64_path") == "mfma"
    le, g2, gi = helpers.rel_errors(l64, g64, ref)
    assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)
    l2, g2_ = eng.loss_grad_f64(th, w)
    assert np.array_equal(l2, l64) and np.array_equal(g2_, g64)              # deterministic
    lo, _ = eng.loss_grad_f64(th, w, want_grad=False)
    np.testing.assert_allclose(lo, l64, rtol=1e-13)
    for k in (0, eng.K - 1):
        r = eng.residual_f64(k, th, sets[k].shape[1])
        rr = po.residual_values(prob, th, k, sets[k], mode="exact")
        assert np.max(np.abs(r - rr)) < 1e-12 * max(1.0, np.max(np.abs(rr)))
    os.environ["PINN_F64_NO_SLICED"] = "1"                                   # the same handle's terms on the lane-per-point family
    try:
        eng.set_option("precision", "f32")
        eng.set_option("precision", "f64")
        for k, s in enumerate(sets):
            eng.set_points_f64(k, s)
        assert "mfma-sliced" not in eng.describe()
        ll, gl = eng.loss_grad_f64(th, w)
    finally:
        del os.environ["PINN_F64_NO_SLICED"]
    np.testing.assert_allclose(ll, l64, rtol=1e-12)
    np.testing.assert_allclose(gl, g64, rtol=0, atol=1e-12 * np.abs(g64).max())


def test_f64_per_layer_activation_mixes(npde, use_emu):
    """tanh and sigmoid mixed inside one chain (the reference's Lorenz chains, test/NNPDE2/additional_loss__lorenz_system.jl:46-50) in float64 mode
    (r06): the activation kind is a run-time value per hidden layer in every float64 kernel family — losses, gradient, trial function against the
    float64 oracle to rounding, on the matrix-pipe kernels and on the lane-per-point family"""
    import os
    for d, width, acts, seed in ((2, 12, ("tanh", "sigmoid"), 71), (2, 16, ("sigmoid", "tanh", "sigmoid"), 72), (1, 10, ("sigmoid", "sigmoid", "tanh"), 74)):
        sysm, _ = helpers.shape_problem(npde, width, len(acts), d)
        layers = [npde.Dense(d, width, acts[0])] + [npde.Dense(width, width, a) for a in acts[1:]] + [npde.Dense(width, 1)]
        chain = npde.Chain(*layers)
        strat = npde.QuasiRandomTraining(50, bcs_points=30, sampling_alg=npde.SobolSample(seed=seed), resampling=False, minibatch=1)
        theta = tp.theta_for(chain, seed)
        rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=theta))          # Float64 parameters: float64 kernels by default
        eng = rep.engine
        assert eng.get_option("precision") == "f64"
        sets = rep.pde_train_sets + rep.bcs_train_sets
        prob = helpers.oracle_problem(npde, sysm, [chain])
        th = np.asarray(rep.flat_init_params, dtype=np.float64)
        ref = po.loss_and_grad(prob, th, sets, mode="exact")
        for nomfma in (False, True):
            if nomfma:
                os.environ["PINN_F64_NO_MFMA"] = "1"
            try:
                l64, g64 = eng.loss_grad_f64(th)
            finally:
                os.environ.pop("PINN_F64_NO_MFMA", None)
            le, g2, gi = helpers.rel_errors(l64, g64, ref)
            assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (acts, nomfma, le, g2, gi)
        pts = np.array([[0.3, 0.7], [0.6, 0.2]])[:d]
        np.testing.assert_allclose(rep.phi(pts, th)[0], po.phi_values(prob.chains[0], th, pts)[0], rtol=1e-13, atol=1e-14)


def test_f64_periodic_embedding(npde, use_emu):
    """r06: a network behind a periodic input embedding (test/CUDA/nnpde_cuda__1d_pde_dirichlet_bc_cuda.jl:26-48) in the float64 mode — what a
    Float64 init_params selects by default.  The term is the descriptor's rewrite over the features (t, sin x, cos x); the feature rows of the
    double point sets are formed in DOUBLE (host sets, pinn_set_points_f64, redrawn sets).  Losses, gradient, residuals and the trial function
    against the float64 oracle (which embeds inside the chain and differentiates in (t, x)) to rounding; on the matrix pipe and lane per point."""
    import os
    sysm, chain = tp.periodic_heat(npde)
    strat = npde.QuasiRandomTraining(60, bcs_points=23, sampling_alg=npde.SobolSample(seed=5), resampling=False, minibatch=1)
    theta = tp.theta_for(chain, 11)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=theta))
    eng = rep.engine
    assert eng.get_option("precision") == "f64"
    sets = rep.pde_train_sets + rep.bcs_train_sets
    prob = helpers.oracle_problem(npde, sysm, [chain])
    th = np.asarray(rep.flat_init_params, dtype=np.float64) + 1e-9
    w = [1.0, 2.0, 0.5, 1.5]
    ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
    for nomfma in (False, True):
        if nomfma:
            os.environ["PINN_F64_NO_MFMA"] = "1"
        try:
            l64, g64 = eng.loss_grad_f64(th, w)
            path = eng.get_option("f64_path")
        finally:
            os.environ.pop("PINN_F64_NO_MFMA", None)
        assert path == ("lanes" if nomfma else "mfma")
        le, g2, gi = helpers.rel_errors(l64, g64, ref)
        assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (nomfma, le, g2, gi)
    r = eng.residual_f64(0, th, sets[0].shape[1])
    np.testing.assert_allclose(r, po.residual_values(prob, th, 0, sets[0], mode="exact").reshape(-1), rtol=0, atol=1e-11)
    pts = np.array([[0.3, 0.7], [0.4, 5.0]])
    np.testing.assert_allclose(eng.phi_f64(0, th, pts), po.phi_values(prob.chains[0], th, pts).reshape(-1), rtol=0, atol=1e-13)
    np.testing.assert_allclose(eng.phi_f64(0, th, pts), eng.phi_f64(0, th, pts + np.array([[0.0], [2 * np.pi]])), rtol=0, atol=1e-13)
    with pytest.raises(Exception, match="periodic input embedding"):
        eng.derivative_f64(0, th, pts, [1])
    # the float trial function of the same handle reads the caller's ARGUMENTS (2 per point, not the 3 features): enough points that the
    # argument buffer is a heap block of its own
    many = np.random.default_rng(8).uniform([[0.0], [0.0]], [[1.0], [2 * np.pi]], size=(2, 1200))
    got = eng.phi(0, th, many)
    ex = po.phi_values(prob.chains[0], th, many).reshape(-1)
    assert got.dtype == np.float32 and np.max(np.abs(got - ex)) < 1e-6 * max(1.0, np.max(np.abs(ex)))
    # the float entry point of the same handle: converted at the boundary
    l32, g32 = eng.loss_grad(th.astype(np.float32), np.asarray(w, dtype=np.float32))
    assert np.linalg.norm(g32 - ref.grad) / np.linalg.norm(ref.grad) < 1e-5
    # a set installed in float is converted and its feature rows recomputed in double
    eng.set_points(0, sets[0].astype(np.float32))
    s32 = sets[0].astype(np.float32).astype(np.float64)
    ref32 = po.loss_and_grad(prob, th, [s32] + sets[1:], weights=w, mode="exact")
    l, g = eng.loss_grad_f64(th, w)
    le, g2, gi = helpers.rel_errors(l, g, ref32)
    assert le.max() < EXACT and g2 < EXACT, (le, g2)
    # device samplers: drawn in the caller's coordinates (float), feature rows in double on the device
    eng.set_sampler(0, [0.0, 0.0], [1.0, 2 * np.pi], 50, seed=7, kind=1)
    th1, hist = eng.adam_f64(th, 1, 1e-3, w)
    drawn = eng.get_points(0, 2, 50).astype(np.float64)
    refd = po.loss_and_grad(prob, th, [drawn] + sets[1:], weights=w, mode="exact")
    assert abs(hist[0] - float(np.dot(w, refd.term_losses))) < 1e-11 * abs(hist[0])
    # the reference-semantics validation mode differentiates in the coordinates: refused for an embedded term, the exact mode stays
    with pytest.raises(Exception, match="periodic input embedding"):
        eng.set_option("derivative", "stencil")
    assert eng.get_option("derivative") == "exact"


def _lorenz(npde):
    """the reference's Lorenz test (test/NNPDE2/additional_loss__lorenz_system.jl): three equations over different subsets of three networks,
    three initial conditions, three estimated parameters -> (system, chains, initial parameters)"""
    (tt,) = npde.parameters("t")
    sg, rho, beta = npde.parameters("sigma_ rho beta")
    xv, yv, zv = npde.variables("x y z")
    D = npde.Differential(tt)
    eqs = [npde.Eq(D(xv(tt)), sg * (yv(tt) - xv(tt))), npde.Eq(D(yv(tt)), xv(tt) * (rho - zv(tt)) - yv(tt)), npde.Eq(D(zv(tt)), xv(tt) * yv(tt) - beta * zv(tt))]
    ics = [npde.Eq(xv(0), 1.0), npde.Eq(yv(0), 0.0), npde.Eq(zv(0), 0.0)]
    lsys = npde.PDESystem(eqs, ics, [npde.In(tt, npde.Interval(0.0, 1.0))], [tt], [xv(tt), yv(tt), zv(tt)], ps=[sg, rho, beta], defaults={sg: 1.0, rho: 1.0, beta: 1.0})
    chains = [npde.Chain(npde.Dense(1, 12, "tanh"), npde.Dense(12, 12, "sigmoid"), npde.Dense(12, 1)) for _ in range(3)]
    th0 = np.concatenate([tp.theta_for(c, 40 + i) for i, c in enumerate(chains)])
    return lsys, chains, th0


def test_f64_merged_launches_of_small_problems(npde, use_emu):
    """r06: small problems (the reference's own regime) are bound by one tile's latency per launch, so the terms that share networks, input binding and
    an instantiated jet set ride in ONE tile / dW / reduction launch sequence on the union jet set (csrc/f64.cpp: f64_make_groups; F64Sub in
    pinn_kernels4.hpp).  Merged = term by term (PINN_F64_NO_MERGE=1) = the float64 oracle to rounding: per-term losses, weighted gradient, loss-only
    evaluations, quadrature weights, more members than one launch takes, the resident Adam loop."""
    import os

    def both(sysm, chains, strat, seed, weights, expect_merged):
        th0 = np.concatenate([tp.theta_for(c, seed + i) for i, c in enumerate(chains)])
        out = []
        for merge in (True, False):
            if not merge:
                os.environ["PINN_F64_NO_MERGE"] = "1"
            try:
                rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chains if len(chains) > 1 else chains[0], strat(), init_params=th0))      # (a fresh strategy: same design)
                eng = rep.engine
                th = np.asarray(rep.flat_init_params, dtype=np.float64) + 1e-9
                l, g = eng.loss_grad_f64(th, weights)
                nm = int(eng.get_option("f64_merged"))
                l1, _ = eng.loss_grad_f64(th, weights, want_grad=False)
                tha, hist = eng.adam_f64(th, 3, 1e-3, weights)
            finally:
                os.environ.pop("PINN_F64_NO_MERGE", None)
            assert eng.get_option("f64_path") == "mfma"
            assert nm == (expect_merged if merge else 0), (merge, nm)
            np.testing.assert_array_equal(l1, l)
            out.append((l, g, tha, hist))
        sets = rep.pde_train_sets + rep.bcs_train_sets
        prob = helpers.oracle_problem(npde, sysm, chains)
        ref = po.loss_and_grad(prob, th, sets, weights=weights, mode="exact")
        for l, g, _, _ in out:
            le, g2, gi = helpers.rel_errors(l, g, ref)
            assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)
        np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-14)
        assert np.linalg.norm(out[0][1] - out[1][1]) / np.linalg.norm(out[1][1]) < 1e-14
        np.testing.assert_allclose(out[0][2], out[1][2], rtol=0, atol=1e-12)
        np.testing.assert_allclose(out[0][3], out[1][3], rtol=1e-12)
        return rep

    # 2-D Poisson, 16-wide (HT = 1 kernels) and 40-wide (HT = 4): interior + four boundary terms -> one launch sequence
    for width, hidden in ((16, 2), (40, 2)):
        sysm, chain = tp.poisson2d(npde, "tanh", width=width, hidden=hidden)
        both(sysm, [chain], lambda: npde.GridTraining(0.1), 5, [1.0, 2.0, 0.5, 1.5, 3.0], 1)
    # a quasi-random design on a sigmoid network
    sysm, chain = tp.poisson2d(npde, "sigmoid", width=12, hidden=2)
    both(sysm, [chain], lambda: npde.QuasiRandomTraining(70, bcs_points=9, sampling_alg=npde.SobolSample(seed=4), resampling=False, minibatch=1), 9, None, 1)
    # 3-D heat equation: one interior + five boundary / initial terms = six members; a seventh term would start a second sequence
    t, x, y = npde.parameters("t x y")
    (u,) = npde.variables("u")
    Dt, Dxx, Dyy = npde.Differential(t), npde.Differential(x) ** 2, npde.Differential(y) ** 2
    eq = npde.Eq(Dt(u(t, x, y)), Dxx(u(t, x, y)) + Dyy(u(t, x, y)))
    bcs = [npde.Eq(u(0.0, x, y), sp.sin(x) * sp.cos(y)), npde.Eq(u(t, 0.0, y), 0.0), npde.Eq(u(t, 1.0, y), sp.exp(-2 * t) * sp.sin(1.0) * sp.cos(y)),
           npde.Eq(u(t, x, 0.0), sp.exp(-2 * t) * sp.sin(x)), npde.Eq(u(t, x, 1.0), sp.exp(-2 * t) * sp.sin(x) * sp.cos(1.0)), npde.Eq(u(1.0, x, y), sp.exp(-2.0) * sp.sin(x) * sp.cos(y))]
    dom = [npde.In(v, npde.Interval(0.0, 1.0)) for v in (t, x, y)]
    chain = npde.Chain(npde.Dense(3, 20, "tanh"), npde.Dense(20, 20, "tanh"), npde.Dense(20, 1))
    both(npde.PDESystem([eq], bcs, dom, [t, x, y], [u(t, x, y)]), [chain], lambda: npde.GridTraining(0.25), 21, [1.0, 0.5, 2.0, 1.5, 1.0, 3.0, 0.7], 1)
    # a system whose equations read different subsets of the dependent variables (the reference's Lorenz test, test/NNPDE2/additional_loss__lorenz_system.jl:
    # three networks, estimated parameters): the launch evaluates the union of the members' networks, six terms in one sequence
    lsys, chains, th0 = _lorenz(npde)
    res = []
    for merge in (True, False):
        if not merge:
            os.environ["PINN_F64_NO_MERGE"] = "1"
        try:
            rep = npde.symbolic_discretize(lsys, npde.PhysicsInformedNN(chains, npde.GridTraining(0.05), init_params=th0, param_estim=True))
            th = np.asarray(rep.flat_init_params, dtype=np.float64) + 1e-9
            w = [1.0, 2.0, 0.5, 1.5, 3.0, 0.7]
            l, g = rep.engine.loss_grad_f64(th, w)
            res.append((l, g, int(rep.engine.get_option("f64_merged"))))
        finally:
            os.environ.pop("PINN_F64_NO_MERGE", None)
    assert res[0][2] == 1 and res[1][2] == 0
    prob = helpers.oracle_problem(npde, lsys, chains, param_estim=True)
    ref = po.loss_and_grad(prob, th, rep.pde_train_sets + rep.bcs_train_sets, weights=w, mode="exact")
    for l, g, _ in res:
        le, g2, gi = helpers.rel_errors(l, g, ref)
        assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)
    # a large set is not merged (the union jet set would multiply the boundary terms' work)
    sysm, chain = tp.poisson2d(npde, "tanh", width=16, hidden=2)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.QuasiRandomTraining(9000, bcs_points=64, sampling_alg=npde.SobolSample(seed=1), resampling=False, minibatch=1),
                                                              init_params=tp.theta_for(chain, 3)))
    rep.engine.loss_grad_f64(np.asarray(rep.flat_init_params, dtype=np.float64))
    assert int(rep.engine.get_option("f64_merged")) == 1        # the four boundary terms together; the 9,000-point interior term on its own


def test_f64_merge_switch_on_a_live_handle(npde, use_emu):
    """PINN_F64_NO_MERGE takes effect at the next call on a LIVE handle, like every other switch of the mode (csrc/f64_setup.cpp:
    f64_read_switches; the switch is part of what f64.cpp: f64_make_groups keys the grouping on) — no point set is touched in between.  The
    smallest case of test_f64_merged_launches_of_small_problems (the Lorenz system: six terms, a few dozen points): merged -> term by term -> merged
    again on one handle; first and third results bit-equal, the second bit-equal to a fresh handle created with the variable set, all = the oracle."""
    import os

    lsys, chains, th0 = _lorenz(npde)
    w = [1.0, 2.0, 0.5, 1.5, 3.0, 0.7]

    def handle():
        return npde.symbolic_discretize(lsys, npde.PhysicsInformedNN(chains, npde.GridTraining(0.05), init_params=th0, param_estim=True))

    def run(eng, th):
        l, g = eng.loss_grad_f64(th, w)
        return l, g, int(eng.get_option("f64_merged"))

    assert "PINN_F64_NO_MERGE" not in os.environ
    rep = handle()
    th = np.asarray(rep.flat_init_params, dtype=np.float64) + 1e-9
    first = run(rep.engine, th)
    os.environ["PINN_F64_NO_MERGE"] = "1"
    try:
        second = run(rep.engine, th)
        fresh = run(handle().engine, th)
    finally:
        os.environ.pop("PINN_F64_NO_MERGE", None)
    third = run(rep.engine, th)
    assert first[2] >= 1 and second[2] == 0 and fresh[2] == 0 and third[2] == first[2], (first[2], second[2], fresh[2], third[2])
    for a, b in ((first, third), (second, fresh)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    prob = helpers.oracle_problem(npde, lsys, chains, param_estim=True)
    ref = po.loss_and_grad(prob, th, rep.pde_train_sets + rep.bcs_train_sets, weights=w, mode="exact")
    for l, g, _ in (first, second, fresh, third):
        le, g2, gi = helpers.rel_errors(l, g, ref)
        assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)


def test_f64_affine_residual_fast_path(npde, use_emu):
    """r06: residuals that are affine in the trial functions with constant coefficients (boundary conditions, Poisson / heat with forcing terms) skip the
    tape interpreter in the matrix-pipe tile kernel — r = S(point) + sum a_s u_s, S evaluated once per point set on the device (csrc/f64_setup.cpp:
    f64_affine).  Same numbers as the tape (PINN_F64_NO_LIN=1) to rounding, = the oracle; nonlinear terms, estimated parameters and redrawn sets
    keep the interpreter."""
    import os
    from neuralpde_jl_amd import workloads

    def run(make, expect):
        res = []
        for lin in (True, False):
            if not lin:
                os.environ["PINN_F64_NO_LIN"] = "1"
            try:
                rep, w = make()
                eng = rep.engine
                th = np.asarray(rep.flat_init_params, dtype=np.float64) + 1e-9
                l, g = eng.loss_grad_f64(th, w)
                n_aff = int(eng.get_option("f64_affine"))
                r0 = eng.residual_f64(0, th, rep.pde_train_sets[0].shape[1])
            finally:
                os.environ.pop("PINN_F64_NO_LIN", None)
            assert n_aff == (expect if lin else 0), (lin, n_aff)
            res.append((l, g, r0))
        np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-13)
        assert np.linalg.norm(res[0][1] - res[1][1]) / np.linalg.norm(res[1][1]) < 1e-13
        np.testing.assert_allclose(res[0][2], res[1][2], rtol=0, atol=1e-13 * max(1.0, np.abs(res[1][2]).max()))
        return rep, th, w, res[0]

    def poisson():
        sysm, chain = tp.poisson2d(npde, "tanh", width=16, hidden=2)
        return npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=tp.theta_for(chain, 5))), [1.0, 2.0, 0.5, 1.5, 3.0]
    rep, th, w, (l, g, _) = run(poisson, 5)                      # -sin(pi x) sin(pi y) forcing: coordinate-only; all five terms affine
    sysm, chain = tp.poisson2d(npde, "tanh", width=16, hidden=2)
    ref = po.loss_and_grad(helpers.oracle_problem(npde, sysm, [chain]), th, rep.pde_train_sets + rep.bcs_train_sets, weights=w, mode="exact")
    le, g2, gi = helpers.rel_errors(l, g, ref)
    assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)

    def burgers():
        wl = workloads.cfg3_burgers(points=200, bcs_points=40)
        return npde.symbolic_discretize(wl.pde_system, wl.discretization(precision="f64")), None
    rep, th, w, (l, g, _) = run(burgers, 3)                      # u_t + u u_x - nu u_xx is nonlinear: tape; the three initial / boundary terms: affine
    # a redrawn set falls back to the tape (the per-point part is not recomputed inside the loop)
    rep, _ = poisson()
    eng = rep.engine
    assert int(eng.get_option("f64_affine")) == 5
    eng.set_sampler(0, [0.0, 0.0], [1.0, 1.0], 64, seed=3, kind=1)
    eng.adam_f64(np.asarray(rep.flat_init_params, dtype=np.float64), 2, 1e-3)
    assert int(eng.get_option("f64_affine")) == 4


@pytest.mark.parametrize("toggles", ["", "PINN_F64_NO_LIN", "PINN_F64_NO_MFMA", "PINN_F64_NO_MERGE", "PINN_F64_NO_LIN,PINN_F64_NO_MFMA,PINN_F64_NO_MERGE"])
def test_f64_mode_reads_fixed_parameters_in_double(npde, use_emu, toggles):
    """PDE parameters that are not estimated keep their descriptor value in double: a = 0.7 and b = -1.3 (neither is a float32 number, so a
    float copy would show at 1e-8) in a nonlinear interior term (the tape interpreter) and in an affine Robin term (coefficient and data of the
    affine fast path) — losses, gradient, residuals, per-term gradients, the BPINN log-likelihood and one resident Adam step against the
    exact-mode oracle, on the matrix-pipe and lane-per-point kernels, with and without the affine path and merged launches"""
    import os
    x, y = npde.parameters("x y")
    a, b = npde.parameters("a b")
    (u,) = npde.variables("u")
    U = u(x, y)
    Dx, Dy = npde.Differential(x), npde.Differential(y)
    eqs = [npde.Eq(a * ((Dx ** 2)(U) + (Dy ** 2)(U)) + b * U * Dx(U) + Dy(U), sp.sin(sp.pi * x) * y)]
    bcs = [npde.Eq(u(0, y) + b * Dx(u(0, y)), a * sp.cos(y)), npde.Eq(u(x, 1), a * x)]
    dom = [npde.In(x, npde.Interval(0.0, 1.0)), npde.In(y, npde.Interval(0.0, 1.0))]
    sysm = npde.PDESystem(eqs, bcs, dom, [x, y], [U], ps=[a, b], defaults={a: 0.7, b: -1.3})
    chain = npde.Chain(npde.Dense(2, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    strat = npde.QuasiRandomTraining(37, bcs_points=19, sampling_alg=npde.SobolSample(seed=3), resampling=False, minibatch=1)
    prob = helpers.oracle_problem(npde, sysm, [chain])
    names = [t for t in toggles.split(",") if t]
    for t in names:
        os.environ[t] = "1"
    try:
        rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=tp.theta_for(chain, 23), precision="f64"))
        eng = rep.engine
        sets = rep.pde_train_sets + rep.bcs_train_sets
        th = np.asarray(rep.flat_init_params, dtype=np.float64)
        assert th.size == chain.nparams                                              # (nothing estimated)
        w = np.linspace(1.0, 2.0, eng.K)
        l, g = eng.loss_grad_f64(th, w)
        assert eng.get_option("f64_path") == ("lanes" if "PINN_F64_NO_MFMA" in names else "mfma")
        assert int(eng.get_option("f64_affine")) == (0 if "PINN_F64_NO_LIN" in names else 2)
        res = [eng.residual_f64(k, th, s.shape[1]) for k, s in enumerate(sets)]
        L, tg = eng.term_grads_f64(th)
        stds = np.linspace(0.05, 0.2, eng.K)
        ll, gl, gs = eng.loglik_grad_f64(th, stds)
        th1, hist = eng.adam_f64(th, 1, 3e-3, w, eps=1.0)
    finally:
        for t in names:
            os.environ.pop(t, None)
    ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact", per_term_grads=True)
    le, g2, gi = helpers.rel_errors(l, g, ref)
    print("fixed parameters in float64 mode:", toggles, le.max(), g2, gi)
    assert le.max() < EXACT and g2 < EXACT and gi < EXACT, (le, g2, gi)
    for k, s in enumerate(sets):
        rr = po.residual_values(prob, th, k, s, mode="exact").reshape(-1)
        assert np.max(np.abs(res[k] - rr)) < 1e-12 * max(1.0, np.max(np.abs(rr))), k
        assert abs(L[k] - ref.term_losses[k]) < EXACT * abs(ref.term_losses[k])
        assert np.linalg.norm(tg[k] - ref.term_grads[k]) < EXACT * np.linalg.norm(ref.term_grads[k]), k
    N = np.array([s.shape[1] for s in sets], dtype=np.float64)
    refl = po.loss_and_grad(prob, th, sets, weights=N / (2.0 * stds ** 2), mode="exact")
    sse = refl.term_losses * N
    ll_ref = float(np.sum(-0.5 * N * np.log(2 * np.pi) - N * np.log(stds) - sse / (2 * stds ** 2)))
    assert abs(ll - ll_ref) < EXACT * abs(ll_ref)
    assert np.linalg.norm(gl + refl.grad) < EXACT * np.linalg.norm(refl.grad)
    np.testing.assert_allclose(gs, -N / stds + sse / stds ** 3, rtol=EXACT)
    # one resident Adam step with eps = 1 (the first step of Adam with a small eps is lr * sign(g): blind to a gradient that is a little off)
    th_host = _host_adam(th, [lambda t_: ref.grad], 3e-3, eps=1.0)
    assert abs(hist[0] - ref.loss) < EXACT * abs(ref.loss)
    assert np.linalg.norm(th1 - th_host) < EXACT * np.linalg.norm(th_host - th)
