"""Host-side mirror of the reference API: symbolic lowering, point sets, descriptor, error behaviour (CPU only)."""
import numpy as np
import pytest
import sympy as sp


def _poisson(npde):
    x, y = npde.parameters("x y")
    (u,) = npde.variables("u")
    Dxx, Dyy = npde.Differential(x) ** 2, npde.Differential(y) ** 2
    eq = npde.Eq(Dxx(u(x, y)) + Dyy(u(x, y)), -sp.sin(sp.pi * x) * sp.sin(sp.pi * y))
    bcs = [npde.Eq(u(0, y), 0.0), npde.Eq(u(1, y), 0.0), npde.Eq(u(x, 0), 0.0), npde.Eq(u(x, 1), 0.0)]
    dom = [npde.In(x, npde.Interval(0.0, 1.0)), npde.In(y, npde.Interval(0.0, 1.0))]
    return npde.PDESystem([eq], bcs, dom, [x, y], [u(x, y)]), (x, y, u)


def test_lowering_poisson_slots_and_ops(npde):
    sysm, (x, y, u) = _poisson(npde)
    vi = npde.get_vars(sysm.ivs, sysm.dvs)
    t = npde.lower_equation(sysm.eqs[0], vi, (), "pde")
    assert t.dim == 2 and t.indvars == ("x", "y")
    assert sorted(s.axes for s in t.slots) == [(0, 0), (1, 1)]          # u_xx, u_yy; the value u itself is not needed
    assert [q.op for q in t.ops].count("SINPI") == 2                     # sin(pi x) sin(pi y) -> sinpi
    # boundary condition: call arguments are dropped (symbolic_utilities.jl:145-160) -> plain value slot
    b = npde.lower_equation(sysm.bcs[0], vi, (), "bc")
    assert [s.axes for s in b.slots] == [()] and b.indvars == ("x", "y")


def test_get_argument_variables_and_bounds(npde):
    sysm, _ = _poisson(npde)
    vi = npde.get_vars(sysm.ivs, sysm.dvs)
    args = npde.get_argument(sysm.bcs, vi)
    assert args[0][0] == 0.0 and str(args[0][1]) == "y" and str(args[2][0]) == "x" and args[2][1] == 0.0
    assert [[str(a) for a in v] for v in npde.get_variables(sysm.bcs, vi)] == [["y"], ["y"], ["x"], ["x"]]
    # docs/src/developer/debugging.md: 100 stochastic points on [0,1] -> bounds [0.01, 0.99]; numeric bc args -> [c, c]
    pb, bb = npde.get_bounds(sysm.domain, sysm.eqs, sysm.bcs, np.float64, vi, 100)
    np.testing.assert_allclose(pb[0][0], [0.01, 0.01]); np.testing.assert_allclose(pb[0][1], [0.99, 0.99])
    np.testing.assert_allclose(bb[1][0], [1.0, 0.01]); np.testing.assert_allclose(bb[1][1], [1.0, 0.99])


def test_grid_training_sets(npde):
    sysm, _ = _poisson(npde)
    vi = npde.get_vars(sysm.ivs, sysm.dvs)
    pde, bcs = npde.generate_training_sets(sysm.domain, 0.25, sysm.eqs, sysm.bcs, np.float64, vi)
    # full 5x5 grid (reference v6.2.2: `dif` stays empty, discretize.jl:202-214), first variable fastest
    assert pde[0].shape == (2, 25)
    np.testing.assert_allclose(pde[0][:, :6].T, [[0, 0], [0.25, 0], [0.5, 0], [0.75, 0], [1, 0], [0, 0.25]])
    assert bcs[0].shape == (2, 5) and np.all(bcs[0][0] == 0.0) and np.all(bcs[3][1] == 1.0)


def test_stochastic_and_quasirandom_sets_inside_bounds(npde):
    sysm, _ = _poisson(npde)
    vi = npde.get_vars(sysm.ivs, sysm.dvs)
    for strat in (npde.StochasticTraining(64, bcs_points=16, rng=np.random.default_rng(0)),
                  npde.QuasiRandomTraining(64, bcs_points=16, sampling_alg=npde.SobolSample(seed=1)),
                  npde.QuasiRandomTraining(64, bcs_points=16, sampling_alg=npde.LatinHypercubeSample(seed=1), resampling=False, minibatch=3)):
        pde, bc, resample = strat.point_sets(sysm, vi, np.float64)
        assert pde[0].shape == (2, 64) and bc[0].shape == (2, 16)
        d = 1.0 / 64
        assert pde[0].min() >= d - 1e-12 and pde[0].max() <= 1 - d + 1e-12
        assert np.all(bc[0][0] == 0.0) and np.all(bc[1][0] == 1.0)
        if resample is not None:
            p2, _ = resample()
            assert p2[0].shape == (2, 64)


def test_burgers_and_params_lowering(npde):
    t, x = npde.parameters("t x")
    (u,) = npde.variables("u")
    (nu,) = npde.parameters("nu")
    Dt, Dx, Dxx = npde.Differential(t), npde.Differential(x), npde.Differential(x) ** 2
    eq = npde.Eq(Dt(u(t, x)) + u(t, x) * Dx(u(t, x)) - nu * Dxx(u(t, x)), 0)
    vi = npde.get_vars([t, x], [u(t, x)])
    term = npde.lower_equation(eq, vi, (nu,), "pde")
    assert sorted(s.axes for s in term.slots) == [(), (0,), (1,), (1, 1)]
    d, NP = 2, 1
    assert any(q.op == "MUL" and (q.a == d or q.b == d) for q in term.ops)        # the parameter row d is used
    desc = npde.ProblemIR(ntheta=10, nets=[npde.NetIR((2, 4, 1), "tanh", 0)], terms=[term], nparams=1, nparams_estim=1,
                          p_theta_off=9, p_defaults=[0.5]).to_descriptor()
    assert desc.startswith("pinnir 1\n") and "params 1 1 9" in desc and "slot 0 2 1 1" in desc


def test_lowering_errors(npde):
    x, y = npde.parameters("x y")
    (u,) = npde.variables("u")
    vi = npde.get_vars([x, y], [u(x, y)])
    with pytest.raises(npde.LoweringError):
        npde.lower_equation(npde.Eq((npde.Differential(x) ** 7)(u(x, y)), 0), vi, (), "pde")      # order 7 (orders up to 6 are carried)
    t5 = npde.lower_equation(npde.Eq((npde.Differential(x) ** 2)(npde.Differential(y)(u(x, y))), 0), vi, (), "pde")   # mixed order 3: one slot
    assert [s.axes for s in t5.slots] == [(0, 0, 1)]
    t3 = npde.lower_equation(npde.Eq((npde.Differential(x) ** 3)(u(x, y)), 0), vi, (), "pde")     # pure third derivative: supported
    assert [s.axes for s in t3.slots] == [(0, 0, 0)]
    with pytest.raises(npde.LoweringError):
        npde.lower_equation(npde.Eq(sp.gamma(u(x, y)), 0), vi, (), "pde")                        # outside the op set
    with pytest.raises(npde.LoweringError):
        npde.lower_equation(npde.Eq(x + y, 0), vi, (), "pde")                                     # no dependent variable


def test_discretizer_errors(npde, use_emu):
    sysm, (x, y, u) = _poisson(npde)
    chain = npde.Chain(npde.Dense(2, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    with pytest.raises(TypeError):                # no boundary conditions (reference: MethodError in the solve phase)
        npde.symbolic_discretize(npde.PDESystem(sysm.eqs, [], sysm.domain, sysm.ivs, sysm.dvs),
                                 npde.PhysicsInformedNN(chain, npde.GridTraining(0.5), precision="f32"))
    with pytest.raises(ValueError):               # trivial bc 0 ~ 0 (reference: ArgumentError at discretize)
        npde.symbolic_discretize(npde.PDESystem(sysm.eqs, [npde.Eq(0.0, 0.0)], sysm.domain, sysm.ivs, sysm.dvs),
                                 npde.PhysicsInformedNN(chain, npde.GridTraining(0.5), precision="f32"))
    with pytest.raises(ValueError):               # chain count != dependent variable count
        npde.symbolic_discretize(sysm, npde.PhysicsInformedNN([chain, chain], npde.GridTraining(0.5), precision="f32"))
    # shapes outside the kernel table are specialised at create time (tests/test_jit.py); what cannot be built fails loudly, never a fallback
    odd = npde.Chain(npde.Dense(2, 200, "relu"), npde.Dense(200, 200, "relu"), npde.Dense(200, 1))
    with pytest.raises(npde.EngineError, match="unsupported activation"):
        npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(odd, npde.GridTraining(0.5), precision="f32"))
    with pytest.raises(npde.EngineError):
        npde.Engine("pinnir 2\n")


def test_chain_and_init_params(npde):
    chain = npde.Chain(npde.Dense(2, 12, "σ"), npde.Dense(12, 12, "σ"), npde.Dense(12, 1))
    assert chain.act == "sigmoid" and chain.sizes == (2, 12, 12, 1) and chain.nparams == 2 * 12 + 12 + 144 + 12 + 12 + 1
    th = npde.initialparameters(np.random.default_rng(0), chain)
    assert th.dtype == np.float64 and th.size == chain.nparams          # Float64 default (src/discretize.jl:432-449)
    with pytest.raises(ValueError):
        npde.Chain(npde.Dense(2, 8, "tanh"), npde.Dense(9, 1))


def test_engine_error_paths(npde, use_emu):
    """C-ABI error behaviour: every misuse returns a status + message (rethrown as EngineError), never a crash or a silent default."""
    x, y = npde.parameters("x y")
    (u,) = npde.variables("u")
    vi = npde.get_vars([x, y], [u(x, y)])
    term = npde.lower_equation(npde.Eq((npde.Differential(x) ** 2)(u(x, y)), 0), vi, (), "pde")
    ir = npde.ProblemIR(ntheta=16 * 2 + 16 + 16 * 16 + 16 + 16 + 1, nets=[npde.NetIR((2, 16, 16, 1), "tanh", 0)], terms=[term])
    eng = npde.Engine(ir.to_descriptor())
    th = np.zeros(eng.P)
    with pytest.raises(npde.EngineError, match="no collocation points"):
        eng.loss_grad(th)
    with pytest.raises(npde.EngineError, match="out of range"):
        eng.set_points(3, np.zeros((2, 4)))
    with pytest.raises(npde.EngineError, match="empty point set"):
        eng.set_points(0, np.zeros((2, 0)))
    eng.set_points(0, np.random.default_rng(0).uniform(size=(2, 7)))
    with pytest.raises(npde.EngineError, match="theta length"):
        eng.loss_grad(np.zeros(eng.P + 1))
    losses, grad = eng.loss_grad(th)
    assert losses.shape == (1,) and grad.shape == (eng.P,) and np.all(np.isfinite(grad))
    with pytest.raises(npde.EngineError, match="holds 7 points"):
        eng.get_points(0, 2, 8)
    # descriptor errors name the problem
    for bad, msg in (("pinnir 1\nntheta 5\nparams 0 0 5\ndefaults \nnets 1\nnet 0 relu 0 3 2 16 1\nterms 0\n", "unsupported activation"),
                     (ir.to_descriptor().replace("op ADDC", "op FOO"), "unknown op"),
                     (ir.to_descriptor().replace("slot 0 2 0 0", "slot 0 2 0 5"), "axis out of range"),
                     (ir.to_descriptor().replace("slot 0 2 0 0", "slot 0 7 0 0 0 0 0 0 0"), "order > 6"),
                     (ir.to_descriptor() + "garbage 1 2\n", "trailing text after the last term"),
                     (ir.to_descriptor() + "hint 9 4\n", "trailing text after the last term")):          # (no term 9)
        with pytest.raises(npde.EngineError, match=msg):
            npde.Engine(bad)


def test_strategy_plugin_contract(npde, use_emu):
    """the reference's strategy plug-in points by name (test/Interface/interface__abstract_contracts.jl:15-22, 53-64): a custom
    AbstractTrainingStrategy subtype works through discretize, and merge_strategy_with_loss_function / get_loss_function give the
    per-term closures  theta -> mean(abs2, residual(set, theta))."""
    sysm, (x, y, u) = _poisson(npde)

    class TwoRowsOfPoints(npde.AbstractTrainingStrategy):
        def point_sets(self, pde_system, vi, dtype):
            g = np.linspace(0.1, 0.9, 9)
            pde = [np.stack([np.tile(g, 2), np.repeat([0.3, 0.7], 9)]).astype(dtype)]
            bc = [np.stack([np.zeros(5), np.linspace(0, 1, 5)]), np.stack([np.ones(5), np.linspace(0, 1, 5)]),
                  np.stack([np.linspace(0, 1, 5), np.zeros(5)]), np.stack([np.linspace(0, 1, 5), np.ones(5)])]
            return pde, [b.astype(dtype) for b in bc], None

    chain = npde.Chain(npde.Dense(2, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    th = npde.initialparameters(np.random.default_rng(5), chain)
    strat = TwoRowsOfPoints()
    prob = npde.discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=th, precision="f32"))
    rep = prob.pinnrep
    assert rep.pde_train_sets[0].shape == (2, 18)
    lf = rep.loss_functions
    pde_l, bc_l = npde.merge_strategy_with_loss_function(rep, strat, lf.datafree_pde_loss_functions, lf.datafree_bc_loss_functions)
    assert len(pde_l) == 1 and len(bc_l) == 4
    np.testing.assert_allclose([f(th) for f in pde_l + bc_l], [f(th) for f in lf.pde_loss_functions + lf.bc_loss_functions], rtol=2e-5)
    one = npde.get_loss_function(th, lf.datafree_bc_loss_functions[2], rep.bcs_train_sets[2], np.float64, strat)
    assert abs(one(th) - lf.bc_loss_functions[2](th)) < 2e-5 * max(1.0, abs(one(th)))
    assert abs(prob.f(th) - sum(f(th) for f in pde_l + bc_l)) < 1e-4 * abs(prob.f(th))       # low_level.md:52-67: sum of the term closures


def test_dropped_call_arguments_quirk(npde, use_emu):
    """The generated loss drops the actual arguments of dependent-variable calls (src/symbolic_utilities.jl:145-160): the `periodic` bc
    `u(t,-1) ~ u(t,1)` of docs/src/tutorials/low_level.md:33 evaluates both sides on the SAME point set (the first call's arguments,
    get_argument) and is identically zero.  Reproduced, not fixed."""
    t, x = npde.parameters("t x")
    (u,) = npde.variables("u")
    Dt, Dx, Dxx = npde.Differential(t), npde.Differential(x), npde.Differential(x) ** 2
    eq = npde.Eq(Dt(u(t, x)) + u(t, x) * Dx(u(t, x)) - (0.01 / sp.pi) * Dxx(u(t, x)), 0)
    bcs = [npde.Eq(u(0, x), -sp.sin(sp.pi * x)), npde.Eq(u(t, -1), 0.0), npde.Eq(u(t, 1), 0.0), npde.Eq(u(t, -1), u(t, 1))]
    dom = [npde.In(t, npde.Interval(0.0, 1.0)), npde.In(x, npde.Interval(-1.0, 1.0))]
    sysm = npde.PDESystem([eq], bcs, dom, [t, x], [u(t, x)])
    chain = npde.Chain(npde.Dense(2, 16, "sigmoid"), npde.Dense(16, 16, "sigmoid"), npde.Dense(16, 1))
    th = npde.initialparameters(np.random.default_rng(2), chain)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.25), init_params=th, precision="f32"))
    assert np.all(rep.bcs_train_sets[3][1] == -1.0)                      # the first call's arguments define the set
    assert rep.loss_functions.bc_loss_functions[3](th) == 0.0
    assert rep.loss_functions.bc_loss_functions[1](th) > 0.0


def test_hmc_sampler_on_a_gaussian(npde):
    """the host-side HMC of the BPINN mirror (bpinn._hmc: dual-averaging step size, windowed diagonal metric) on a known target:
    N(mu, diag(s^2)) in 5 dimensions — sample mean and standard deviation within Monte-Carlo error, acceptance near the target."""
    from neuralpde_jl_amd import bpinn
    mu, sd = np.array([1.0, -2.0, 0.5, 3.0, 0.0]), np.array([0.5, 2.0, 1.0, 0.1, 5.0])
    logp = lambda th: (float(-0.5 * np.sum(((th - mu) / sd) ** 2)), -(th - mu) / sd ** 2)
    samples, stats = bpinn._hmc(logp, np.zeros(5), 4000, 10, 0.1, 0.8, np.random.default_rng(0))
    s = samples[1000:]
    assert np.all(np.abs(s.mean(axis=0) - mu) < 0.25 * sd + 0.02)
    assert np.all(np.abs(s.std(axis=0) / sd - 1.0) < 0.25)
    assert 0.6 < stats["acceptance"][400:].mean() <= 1.0 and stats["n_adapts"] == 400


@pytest.mark.parametrize("n", (100, 107, 20))
def test_warmup_loop_meets_the_device_restatement(npde, n):
    """the one warm-up loop of the BPINN mirror (bpinn._adapt_and_draw) against the restatement the resident warm-up is held to
    (tests/test_resident_hmc_warmup.py: `recurrence`, `window_metric`, its bar), driven by a scripted transition that returns prescribed
    acceptances and sample rows: the step size handed to every transition and the final one, the metric at the window's event, and the hook
    that tells the device about it — once when the event fires (n = 100, 107), never otherwise (n = 20)."""
    from neuralpde_jl_amd import bpinn
    from test_resident_hmc_warmup import EPS0, EPS64, TARGET, check_recurrence, relmax, supplied, window, window_metric
    P = 5
    rows, acc = supplied(P, n)
    w0, w1, event = window(n)
    steps, metrics, hooked = [], [], []

    def transition(nd, eps, metric):
        assert nd == 1 and len(steps) < n
        steps.append(eps)
        metrics.append(metric.minv)
        return [(rows[len(steps) - 1], acc[len(steps) - 1])]
    out, eps_final, metric = bpinn._adapt_and_draw(transition, bpinn._DiagMetric(np.ones(P)), EPS0, TARGET, n, n, hooked.append)
    assert len(out) == n and all(np.array_equal(o[0], r) for o, r in zip(out, rows))
    check_recurrence(f"mirror n={n}", acc, np.asarray(steps), eps_final)
    assert len(hooked) == (1 if event else 0)
    if event:
        m64, mld = window_metric(rows[w0:w1], np.float64), window_metric(rows[w0:w1], np.longdouble)
        bar = 100.0 * max(relmax(m64, mld), EPS64)
        assert relmax(hooked[0], m64) <= bar
        assert all(np.array_equal(m, np.ones(P)) for m in metrics[:w1]) and all(m is hooked[0] for m in metrics[w1:])
    else:
        assert all(np.array_equal(m, np.ones(P)) for m in metrics)
    assert metric.minv is metrics[-1]
