"""Integral terms in residuals (`npde.Integral`, the reference's integro-differential equations, src/discretize.jl:355-396): the fp32
engine evaluates I(x) = int_lo^hi f(s; x, u, du, p) ds with a fixed Q-node Gauss-Legendre rule on the device (site expansion kernel ->
forward launches over the site set -> integral tail kernel -> seeded reverse launches).

oracle/pinn_oracle.py has no integral, so this file carries its own float64 reference: sites from numpy's `leggauss(Q)`, the oracle's
`po.Chain` / `po.exact_derivative` through torch in float64, each residual written out by hand, gradients by torch autograd.

Every body is written once as a function of `npde` and exposed twice: on the CPU through the g++ lock-step emulation (`use_emu`) and,
marked `gpu`, on the product library (the pattern of tests/test_swish.py).

Bars: fp32 against the float64 reference at the project's 1e-5 relative (test_emu_parity.TOL): per-term loss, gradient L2 and Linf (norms,
never entry-wise: the output bias of a value-free term is structurally zero); pointwise residuals at 1e-5 * max(1, max |r_ref|); resident
Adam against a host Adam at the tolerance tests/test_emu_parity.py::test_resident_adam_matches_host_adam_and_sampler uses (rtol 2e-5).
Measured: loss <= 1.2e-6, gradient <= 1.0e-6 on the emulation; loss <= 2.2e-6, gradient <= 1.0e-6 on an MI355X (profiles/integral_terms.txt)."""
import os

import numpy as np
import pytest
import sympy as sp
import torch
from numpy.polynomial.legendre import leggauss

import pinn_oracle as po
import test_emu_parity as tp

TOL = tp.TOL
QS = (4, 16, 33)
UU = lambda cord, th, phi: phi(cord, th)


# ------------------------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ------------------------------------------------------------------------------------------------------------------------------------
def gl_integral(f, lo, hi, Q):
    """(hi - lo)/2 * sum_q w_q f(lo + (hi - lo)(xi_q + 1)/2); lo / hi: floats or (1 x N) tensors; f: (1 x N) abscissae -> (1 x N)."""
    xi, w = leggauss(Q)
    acc = 0.0
    for q in range(Q):
        acc = acc + float(w[q]) * f(lo + (hi - lo) * (0.5 * (float(xi[q]) + 1.0)))
    return 0.5 * (hi - lo) * acc


class Case:
    """A problem: the PDESystem for the engine and, per term, the residual written out by hand for the reference."""

    def __init__(self, sysm, d, resid, param_estim=False, p0=()):
        self.sysm, self.d, self.resid, self.param_estim, self.p0 = sysm, d, resid, param_estim, tuple(p0)


def ide(npde):
    """The reference's IntegroDiff example: Dt(i) + 2 i + 5 int_0^t i = 1, i(0) = 0 on [0, 2]; solution 1/2 exp(-t) sin(2 t)."""
    (t,) = npde.parameters("t")
    (i,) = npde.variables("i")
    Ii = npde.Integral(npde.In(t, npde.Interval(0.0, t)))
    eq = npde.Eq(npde.Differential(t)(i(t)) + 2 * i(t) + 5 * Ii(i(t)), 1)
    sysm = npde.PDESystem([eq], [npde.Eq(i(0.0), 0.0)], [npde.In(t, npde.Interval(0.0, 2.0))], [t], [i(t)])

    def r_pde(ch, th, p, x, Q):
        return po.exact_derivative(ch, UU, x, [0], th) + 2 * ch(x, th) + 5 * gl_integral(lambda s: ch(s, th), 0.0, x, Q) - 1

    return Case(sysm, 1, [r_pde, lambda ch, th, p, x, Q: ch(x, th)])


def volterra(npde):
    """int_0^x u(s) cos(s) ds = x^3 / 3."""
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Integral(npde.In(x, npde.Interval(0.0, x)))(u(x) * sp.cos(x)), x ** 3 / 3)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.5))], [x], [u(x)])

    def r_pde(ch, th, p, xx, Q):
        return gl_integral(lambda s: ch(s, th) * torch.cos(s), 0.0, xx, Q) - xx ** 3 / 3

    return Case(sysm, 1, [r_pde, lambda ch, th, p, xx, Q: ch(xx, th)])


def strip2d(npde):
    """2-D: the integral runs over y with x held fixed, a derivative slot inside the integrand and constant bounds; one boundary
    condition carries an integral node too."""
    x, y = npde.parameters("x y")
    (u,) = npde.variables("u")
    Dx, Dy = npde.Differential(x), npde.Differential(y)
    Iy = npde.Integral(npde.In(y, npde.Interval(0.0, 1.0)))
    eq = npde.Eq(Dy(u(x, y)) + Iy(Dx(u(x, y))) * u(x, y), x * y)
    bcs = [npde.Eq(u(x, 0.0), sp.sin(x)), npde.Eq(Iy(u(0.0, y)) + u(0.0, y), 0.5)]
    dom = [npde.In(x, npde.Interval(0.0, 1.0)), npde.In(y, npde.Interval(0.0, 1.0))]
    sysm = npde.PDESystem([eq], bcs, dom, [x, y], [u(x, y)])

    def at_y(pts, s):
        return torch.cat([pts[0:1], s + torch.zeros_like(pts[1:2])], dim=0)      # (constant bounds: the abscissa is a number)

    def r_pde(ch, th, p, pts, Q):
        I = gl_integral(lambda s: po.exact_derivative(ch, UU, at_y(pts, s), [0], th), 0.0, 1.0, Q)
        return po.exact_derivative(ch, UU, pts, [1], th) + I * ch(pts, th) - pts[0:1] * pts[1:2]

    def r_bc0(ch, th, p, pts, Q):
        return ch(pts, th) - torch.sin(pts[0:1])

    def r_bc1(ch, th, p, pts, Q):
        return gl_integral(lambda s: ch(at_y(pts, s), th), 0.0, 1.0, Q) + ch(pts, th) - 0.5

    return Case(sysm, 2, [r_pde, r_bc0, r_bc1])


def ide_param(npde):
    """param_estim with the PDE parameter inside the integrand: Dt(i) + 2 i + int_0^t a i(s) (1 + b s) ds = 1."""
    (t,) = npde.parameters("t")
    a, b = npde.parameters("a b")
    (i,) = npde.variables("i")
    Ii = npde.Integral(npde.In(t, npde.Interval(0.0, t)))
    eq = npde.Eq(npde.Differential(t)(i(t)) + 2 * i(t) + Ii(a * i(t) * (1 + b * t)), 1)
    sysm = npde.PDESystem([eq], [npde.Eq(i(0.0), 0.0)], [npde.In(t, npde.Interval(0.0, 2.0))], [t], [i(t)], ps=[a, b], defaults={a: 5.0, b: 0.25})

    def r_pde(ch, th, p, x, Q):
        I = gl_integral(lambda s: p[0] * ch(s, th) * (1 + p[1] * s), 0.0, x, Q)
        return po.exact_derivative(ch, UU, x, [0], th) + 2 * ch(x, th) + I - 1

    return Case(sysm, 1, [r_pde, lambda ch, th, p, x, Q: ch(x, th)], param_estim=True, p0=(5.0, 0.25))


CASES = {"ide": ide, "volterra": volterra, "strip2d": strip2d, "ide_param": ide_param}


def make_chain(npde, d, kind):
    width, hidden = {"w16": (16, 2), "w64": (64, 4), "odd": (40, 3)}[kind]      # family 1; family 2; outside the ahead-of-time table
    return npde.Chain(npde.Dense(d, width, "tanh"), *[npde.Dense(width, width, "tanh") for _ in range(hidden - 1)], npde.Dense(width, 1))


def reference(case, chain, theta, sets, Q, weights=None):
    """float64: per-term losses mean(r^2), gradient of sum_k w_k loss_k, and the residual vectors."""
    ochain = po.Chain(tuple(chain.sizes), chain.act)
    th = torch.tensor(np.asarray(theta, dtype=np.float64), dtype=po.DT, requires_grad=True)
    nnet = ochain.nparams
    net, p = th[:nnet], (th[nnet:] if case.param_estim else torch.tensor(case.p0, dtype=po.DT))
    rs = [fn(ochain, net, p, torch.tensor(np.asarray(s, dtype=np.float64), dtype=po.DT), Q) for fn, s in zip(case.resid, sets)]
    losses = [torch.mean(r ** 2) for r in rs]
    w = np.ones(len(rs)) if weights is None else np.asarray(weights, dtype=np.float64)
    total = sum(float(wk) * l for wk, l in zip(w, losses))
    (g,) = torch.autograd.grad(total, th)
    return np.array([float(l.detach()) for l in losses]), g.numpy(), [r.detach().numpy().reshape(-1) for r in rs]


def discretise(npde, case, chain, Q, theta, strategy=None, gemm=None):
    strategy = strategy or npde.QuasiRandomTraining(40, bcs_points=12, sampling_alg=npde.SobolSample(seed=3), resampling=False, minibatch=1)
    disc = npde.PhysicsInformedNN(chain, strategy, init_params=theta, param_estim=case.param_estim, precision="f32", integral_nodes=Q)
    rep = npde.symbolic_discretize(case.sysm, disc)
    assert rep.engine.L.backend == tp.EXPECTED_BACKEND
    if gemm is not None:
        rep.engine.set_option("gemm", gemm)
        assert rep.engine.get_option("gemm") == gemm
    assert rep.engine.get_option("integral_nodes") == str(Q)
    assert "+integral(%d)" % Q in rep.engine.describe(), rep.engine.describe()
    sets = [np.asarray(s, dtype=np.float32).astype(np.float64) for s in rep.pde_train_sets + rep.bcs_train_sets]      # what the engine holds
    return rep, sets


def errors(losses, grad, ref_losses, ref_grad):
    le = np.max(np.abs(np.asarray(losses) - ref_losses) / np.abs(ref_losses))
    g = np.asarray(grad, dtype=np.float64)
    return le, np.linalg.norm(g - ref_grad) / np.linalg.norm(ref_grad), np.max(np.abs(g - ref_grad)) / np.max(np.abs(ref_grad))


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. parity: loss, gradient, residuals, per-term gradients, loss-only, reproducibility
# ------------------------------------------------------------------------------------------------------------------------------------
def body_parity(npde, case, kind, gemm=None):
    c = CASES[case](npde)
    chain = make_chain(npde, c.d, kind)
    for Q in QS:
        rep, sets = discretise(npde, c, chain, Q, tp.theta_for(chain, 300 + Q).astype(np.float32), gemm=gemm)
        th = rep.flat_init_params
        K = len(sets)
        w = list(np.linspace(1.0, 2.0, K))
        losses, grad = rep.engine.loss_grad(th, w)
        ref_l, ref_g, ref_r = reference(c, chain, th, sets, Q, w)
        le, g2, gi = errors(losses, grad, ref_l, ref_g)
        print("integral %s %s gemm=%s Q=%d: loss rel %.3e grad L2 %.3e Linf %.3e   (losses %s)" % (case, kind, gemm, Q, le, g2, gi, ref_l))
        assert le < TOL and g2 < TOL and gi < TOL, (case, kind, gemm, Q, le, g2, gi)
        # two evaluations are bit-identical
        l2, g2_ = rep.engine.loss_grad(th, w)
        assert np.array_equal(l2, losses) and np.array_equal(g2_, grad)
        # residuals, pointwise
        for k in range(K):
            r = rep.engine.residual(k, th, sets[k].shape[1])
            err, bound = np.max(np.abs(r - ref_r[k])), TOL * max(1.0, np.max(np.abs(ref_r[k])))
            print("   residual of term %d: max abs err %.3e (bound %.3e)" % (k, err, bound))
            assert err < bound, (case, kind, Q, k, err, bound)
        # per-term gradients sum to the whole (unit weights)
        l1, g1 = rep.engine.loss_grad(th)
        tl, tg = rep.engine.term_grads(th)
        assert np.allclose(tl, l1, rtol=1e-6, atol=0)
        assert np.linalg.norm(tg.sum(axis=0) - g1) <= 2e-6 * np.linalg.norm(g1)
        # loss-only evaluation = the losses of the full evaluation
        lo, none = rep.engine.loss_grad(th, w, want_grad=False)
        assert none is None and np.array_equal(lo, losses)
        if kind == "w16":
            assert "kernel=F1_" in rep.engine.describe()
        if kind == "w64":
            assert "kernel=F2_" in rep.engine.describe() and ("split-bf16" in rep.engine.describe()) == (gemm == "split")


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the rule itself (float64 reference only): the error against Q = 64 does not grow with Q
# ------------------------------------------------------------------------------------------------------------------------------------
def body_rule_sanity(npde):
    c = ide(npde)
    chain = make_chain(npde, 1, "w16")
    ochain = po.Chain(tuple(chain.sizes), chain.act)
    th = torch.tensor(tp.theta_for(chain, 7), dtype=po.DT)
    x = torch.linspace(0.05, 2.0, 23, dtype=po.DT)[None, :]
    val = lambda Q: gl_integral(lambda s: ochain(s, th), 0.0, x, Q).numpy()
    ref = val(64)
    errs = [np.max(np.abs(val(Q) - ref)) for Q in (8, 16, 32)]
    print("Gauss-Legendre rule against Q = 64: Q = 8 / 16 / 32 -> %.3e / %.3e / %.3e" % tuple(errs))
    assert errs[1] <= errs[0] + 1e-15 and errs[2] <= errs[1] + 1e-15, errs
    # and the engine's option follows PhysicsInformedNN(..., integral_nodes = Q): Q = 32 is closer to the Q = 64 loss than Q = 4
    theta = tp.theta_for(chain, 7).astype(np.float32)
    ls = {}
    for Q in (4, 32, 64):
        rep, _ = discretise(npde, c, chain, Q, theta)
        ls[Q] = rep.engine.loss_grad(rep.flat_init_params)[0][0]
    assert abs(ls[32] - ls[64]) <= abs(ls[4] - ls[64])


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. resampling: the site set follows every device redraw
# ------------------------------------------------------------------------------------------------------------------------------------
def body_resampling(npde, kind_name):
    c = ide(npde)
    chain = make_chain(npde, 1, "w16")
    theta = tp.theta_for(chain, 11).astype(np.float32)
    kind = {"uniform": 1, "lhs": 2, "sobol": 3}[kind_name]
    n, steps, lr = 48, 6, 0.01
    lb, ub = [0.0], [2.0]
    rep_a, _ = discretise(npde, c, chain, 16, theta)
    rep_a.engine.set_sampler(0, lb, ub, n, seed=5, kind=kind)
    _, hist_a = rep_a.engine.adam(theta, steps, lr)
    assert rep_a.engine.get_option("adam_path") == "loop"
    # the same draws, read back before every step and installed into a second handle through pinn_set_points
    rep_b, _ = discretise(npde, c, chain, 16, theta)
    rep_c, _ = discretise(npde, c, chain, 16, theta)
    rep_b.engine.set_sampler(0, lb, ub, n, seed=5, kind=kind)
    hist_c, th, seen = [], theta, []
    for s in range(steps):
        # one resident step on B redraws, evaluates and updates; its point set after the step is the draw the step used
        th_b, hb = rep_b.engine.adam(th, 1, lr, init=(s == 0))
        pts = rep_b.engine.get_points(0, 1, n)
        seen.append(pts.copy())
        rep_c.engine.set_points(0, pts)
        _, hc = rep_c.engine.adam(th, 1, lr, init=True) if s == 0 else rep_c.engine.adam(None, 1, lr, init=False)
        hist_c.append(hc[0])
        assert hb[0] == hist_a[s]
    assert np.array_equal(np.asarray(hist_c), hist_a), (hist_c, hist_a)
    assert len({p.tobytes() for p in seen}) == steps          # (the sets did change from step to step)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. training
# ------------------------------------------------------------------------------------------------------------------------------------
def body_training(npde):
    c = ide(npde)
    chain = make_chain(npde, 1, "w16")
    th0 = tp.theta_for(chain, 21).astype(np.float32)
    Q, K, lr = 16, 25, 0.01
    rep, sets = discretise(npde, c, chain, Q, th0, strategy=npde.GridTraining(0.05))
    w = [1.0, 10.0]
    th_dev, hist = rep.engine.adam(th0, K, lr, w)
    assert rep.engine.get_option("adam_path") == "loop"
    # host loop, the same Adam rule, on the float64 reference's gradients
    th, m_, v_, ref_hist = th0.astype(np.float64), 0.0, 0.0, []
    for it in range(1, K + 1):
        l, g, _ = reference(c, chain, th, sets, Q, w)
        ref_hist.append(float(np.dot(w, l)))
        m_ = 0.9 * m_ + 0.1 * g
        v_ = 0.999 * v_ + 0.001 * g * g
        th = th - lr * (m_ / (1 - 0.9 ** it)) / (np.sqrt(v_ / (1 - 0.999 ** it)) + 1e-8)
    print("resident Adam vs float64 host Adam, max rel loss difference over %d steps: %.3e" % (K, np.max(np.abs(hist - ref_hist) / np.abs(ref_hist))))
    np.testing.assert_allclose(hist, ref_hist, rtol=2e-5)
    assert hist[-1] < hist[0]
    # accuracy against the analytic solution after a longer run of both loops
    K2 = 300
    th_dev, hist2 = rep.engine.adam(th0, K2, lr, w)
    th, m_, v_ = th0.astype(np.float64), 0.0, 0.0
    for it in range(1, K2 + 1):
        _, g, _ = reference(c, chain, th, sets, Q, w)
        m_ = 0.9 * m_ + 0.1 * g
        v_ = 0.999 * v_ + 0.001 * g * g
        th = th - lr * (m_ / (1 - 0.9 ** it)) / (np.sqrt(v_ / (1 - 0.999 ** it)) + 1e-8)
    grid = np.linspace(0.0, 2.0, 201)[None, :]
    exact = 0.5 * np.exp(-grid) * np.sin(2 * grid)
    ochain = po.Chain(tuple(chain.sizes), chain.act)
    mse = lambda t_: float(np.mean((po.phi_values(ochain, np.asarray(t_, dtype=np.float64), grid).reshape(1, -1) - exact) ** 2))
    mse_dev, mse_ref = mse(th_dev), mse(th)
    line = "IDE after %d Adam steps (lr %g, Q %d, 16-wide chain): MSE against 1/2 exp(-t) sin(2t): engine %.6e, float64 host loop %.6e [%s]" % (
        K2, lr, Q, mse_dev, mse_ref, rep.engine.L.backend)
    print(line)
    out = os.environ.get("PINN_INTEGRAL_PROFILE")          # (a measuring run appends the two figures to this file)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    assert mse_dev <= 2.0 * mse_ref, (mse_dev, mse_ref)
    # L-BFGS inside the library on the fixed set lowers the loss further and stays finite
    f_adam = float(np.dot(w, rep.engine.loss_grad(th_dev, w, want_grad=False)[0]))
    theta, lh = rep.engine.lbfgs(th_dev, 40, w)
    assert len(lh) >= 1 and np.all(np.isfinite(lh)) and np.all(np.isfinite(theta)) and lh[-1] < f_adam, (lh, f_adam)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. integral_nodes on a live handle: the handle is re-planned, installed point sets stay
# ------------------------------------------------------------------------------------------------------------------------------------
def body_option_replans(npde):
    c = ide(npde)
    chain = make_chain(npde, 1, "w16")
    theta = tp.theta_for(chain, 31).astype(np.float32)
    rep, sets = discretise(npde, c, chain, 4, theta)
    l4, g4 = rep.engine.loss_grad(theta)
    rep.engine.set_option("integral_nodes", "33")           # grows the site set of the installed points
    assert rep.engine.get_option("integral_nodes") == "33" and "+integral(33)" in rep.engine.describe()
    rep33, _ = discretise(npde, c, chain, 33, theta)
    l33, g33 = rep.engine.loss_grad(theta)
    l33b, g33b = rep33.engine.loss_grad(theta)
    assert np.array_equal(l33, l33b) and np.array_equal(g33, g33b) and not np.array_equal(l33, l4)
    rep.engine.set_option("integral_nodes", "4")            # and back
    l4b, g4b = rep.engine.loss_grad(theta)
    assert np.array_equal(l4, l4b) and np.array_equal(g4, g4b)
    for bad in ("1", "65", "0", "-3", "sixteen", "4.5"):
        with pytest.raises(npde.EngineError, match="integral_nodes must be an integer in 2..64"):
            rep.engine.set_option("integral_nodes", bad)
    l4c, _ = rep.engine.loss_grad(theta)
    assert np.array_equal(l4, l4c)                          # a refused value leaves the handle as it was


def body_replan_buffer_reuse(npde):
    """The re-plan keeps a site buffer that has room and replaces one that has not: a smaller set after a larger one, shrink, grow."""
    c = ide(npde)
    chain = make_chain(npde, 1, "w16")
    theta = tp.theta_for(chain, 32).astype(np.float32)
    rep, sets = discretise(npde, c, chain, 33, theta)           # 40 points at Q = 33
    small = np.ascontiguousarray(sets[0][:, :10])

    def fresh(Q):
        r, _ = discretise(npde, c, chain, Q, theta)
        r.engine.set_points(0, small)
        return r.engine.loss_grad(theta)

    rep.engine.set_points(0, small)                              # 10 points in the buffer of 40
    for Q in (33, 4, 64, 2, 16):                                 # shrink (kept), grow within the room (kept), ...
        rep.engine.set_option("integral_nodes", str(Q))
        l, g = rep.engine.loss_grad(theta)
        lf, gf = fresh(Q)
        assert np.array_equal(l, lf) and np.array_equal(g, gf), Q
        assert np.array_equal(rep.engine.get_points(0, 1, 10), small.astype(np.float32))
    rep.engine.set_points(0, sets[0])                            # and the larger set again
    l, g = rep.engine.loss_grad(theta)
    r16, _ = discretise(npde, c, chain, 16, theta)
    lf, gf = r16.engine.loss_grad(theta)
    assert np.array_equal(l, lf) and np.array_equal(g, gf)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5b. the symbolic front end ("pinnir 2"): (integral <var> <lo> <hi> <body>) lowers to the same engine as the pinnir-1 lines
# ------------------------------------------------------------------------------------------------------------------------------------
def _with_descriptor2(fn):
    old = os.environ.get("PINN_DESCRIPTOR")
    os.environ["PINN_DESCRIPTOR"] = "2"
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["PINN_DESCRIPTOR"]
        else:
            os.environ["PINN_DESCRIPTOR"] = old


def body_pinnir2(npde):
    for case in ("ide", "strip2d", "ide_param"):
        c = CASES[case](npde)
        chain = make_chain(npde, c.d, "w16")
        theta = tp.theta_for(chain, 61).astype(np.float32)
        rep1, sets = discretise(npde, c, chain, 16, theta)
        rep2, _ = _with_descriptor2(lambda: discretise(npde, c, chain, 16, theta))
        assert rep1.engine.descriptor.startswith("pinnir 1") and rep2.engine.descriptor.startswith("pinnir 2")
        assert "(integral " in rep2.engine.descriptor and "integrals" not in rep2.engine.descriptor, rep2.engine.descriptor
        th = rep1.flat_init_params
        l1, g1 = rep1.engine.loss_grad(th)
        l2, g2 = rep2.engine.loss_grad(th)
        assert np.array_equal(l1, l2) and np.array_equal(g1, g2), (case, l1, l2)
        for k in range(len(sets)):
            assert np.array_equal(rep1.engine.residual(k, th, sets[k].shape[1]), rep2.engine.residual(k, th, sets[k].shape[1]))
    # the named refusals of the form
    head = ("pinnir 2\nntheta 321\nparams 0 0 321\ndefaults \npnames \nnets 1\nnet 0 tanh 0 4 1 16 16 1\nnetvar 0 i 1 t\n"
            "terms 1\nsterm 0 1 t\nlhs %s\nrhs 1\n")
    for lhs, msg in (("(integral t 0 t (integral t 0 t (i t)))", "nested integrals"),
                     ("(integral s 0 t (i t))", "integration variable s is not an independent variable"),
                     ("(integral (t s) 0 t (i t))", "multi-variable integrals"),
                     ("(integral t 0 Inf (i t))", "infinite upper bound"),
                     ("(integral t -Inf 0 (i t))", "infinite lower bound"),
                     ("(integral t 0 (^ t 2) (i t))", "general expression"),
                     ("(integral t 0 t (* t t))", "does not contain a dependent variable"),
                     ("(integral t 0 t)", "malformed .integral"),
                     ("(D t 1 (integral t 0 t (i t)))", "Differential must act on a dependent variable")):
        with pytest.raises(npde.EngineError, match=msg):
            npde.Engine(head % lhs)
    e = npde.Engine(head % "(+ (D t 1 (i t)) (* 5 (integral t 0 t (i t))))")          # and the well-formed line is taken
    assert "+integral(16)" in e.describe()


# ------------------------------------------------------------------------------------------------------------------------------------
# 5c. point weights and per-point data around an integral term; site sets beyond one launch group
# ------------------------------------------------------------------------------------------------------------------------------------
def body_point_weights(npde):
    c = ide(npde)
    chain = make_chain(npde, 1, "w16")
    theta = tp.theta_for(chain, 71).astype(np.float32)
    rep, sets = discretise(npde, c, chain, 16, theta)
    n = sets[0].shape[1]
    wq = np.random.default_rng(4).uniform(0.2, 2.0, size=n) / n          # quadrature-style weights: loss = sum_i w_i r_i^2
    rep.engine.set_point_weights(0, wq)
    tw = [1.5, 0.5]
    losses, grad = rep.engine.loss_grad(theta, tw)
    ochain = po.Chain(tuple(chain.sizes), chain.act)
    th = torch.tensor(theta.astype(np.float64), dtype=po.DT, requires_grad=True)
    rs = [fn(ochain, th, None, torch.tensor(s_, dtype=po.DT), 16) for fn, s_ in zip(c.resid, sets)]
    ref_l = [torch.sum(torch.tensor(wq.astype(np.float32).astype(np.float64))[None, :] * rs[0] ** 2), torch.mean(rs[1] ** 2)]
    (ref_g,) = torch.autograd.grad(tw[0] * ref_l[0] + tw[1] * ref_l[1], th)
    le, g2, gi = errors(losses, grad, np.array([float(l.detach()) for l in ref_l]), ref_g.numpy())
    print("integral term with point weights: loss rel %.3e grad L2 %.3e Linf %.3e" % (le, g2, gi))
    assert le < TOL and g2 < TOL and gi < TOL, (le, g2, gi)
    lo, _ = rep.engine.loss_grad(theta, tw, want_grad=False)
    assert np.array_equal(lo, losses)
    rep.engine.set_point_weights(0, None)                                 # back to the plain mean
    l0, _ = rep.engine.loss_grad(theta, tw)
    ref0, _, _ = reference(c, chain, theta, sets, 16, tw)
    assert np.max(np.abs(l0 - ref0) / ref0) < TOL


def body_point_data(npde):
    """A DATA channel in the outer tape of an integral term: residual = (the IDE's residual) - d_i."""
    from neuralpde_jl_amd.ir import Instr
    c = ide(npde)
    chain = make_chain(npde, 1, "w16")
    theta = tp.theta_for(chain, 72).astype(np.float32)
    rep, sets = discretise(npde, c, chain, 16, theta)
    ir = rep.ir
    t0 = ir.terms[0]
    base = t0.dim + ir.nparams + len(t0.slots) + len(t0.integrals)
    t0.ops = list(t0.ops) + [Instr("DATA", 0, 0, 0.0), Instr("SUB", t0.out_row, base + len(t0.ops), 0.0)]
    t0.out_row = base + len(t0.ops) - 1
    eng = npde.Engine(ir.to_descriptor())
    eng.set_option("integral_nodes", "16")
    for k, s_ in enumerate(sets):
        eng.set_points(k, s_)
    n = sets[0].shape[1]
    data = np.random.default_rng(5).uniform(-1.0, 1.0, size=(1, n)).astype(np.float32)
    eng.set_point_data(0, data)
    losses, grad = eng.loss_grad(theta)
    ochain = po.Chain(tuple(chain.sizes), chain.act)
    th = torch.tensor(theta.astype(np.float64), dtype=po.DT, requires_grad=True)
    r0 = c.resid[0](ochain, th, None, torch.tensor(sets[0], dtype=po.DT), 16) - torch.tensor(data.astype(np.float64), dtype=po.DT)
    r1 = c.resid[1](ochain, th, None, torch.tensor(sets[1], dtype=po.DT), 16)
    ref_l = [torch.mean(r0 ** 2), torch.mean(r1 ** 2)]
    (ref_g,) = torch.autograd.grad(ref_l[0] + ref_l[1], th)
    le, g2, gi = errors(losses, grad, np.array([float(l.detach()) for l in ref_l]), ref_g.numpy())
    print("integral term with a DATA channel: loss rel %.3e grad L2 %.3e Linf %.3e" % (le, g2, gi))
    assert le < TOL and g2 < TOL and gi < TOL, (le, g2, gi)
    r = eng.residual(0, theta, n)
    assert np.max(np.abs(r - r0.detach().numpy().reshape(-1))) < TOL * max(1.0, float(r0.detach().abs().max()))


def body_site_set_too_large(npde):
    c = ide(npde)
    chain = make_chain(npde, 1, "w16")
    theta = tp.theta_for(chain, 73).astype(np.float32)
    rep, sets = discretise(npde, c, chain, 64, theta)
    n = 1_400_000                                                         # x (1 + 64) sites x 24 channel rows >= 2^31
    big = np.linspace(0.0, 2.0, n, dtype=np.float32)[None, :]
    with pytest.raises(npde.EngineError, match=r"1400000 points x \(1 \+ 1 integral node\(s\) x 64 quadrature nodes\) = 91000000 sites\) exceeds"):
        rep.engine.set_points(0, big)
    l0, g0 = rep.engine.loss_grad(theta)                                  # the installed set is still there
    rep2, _ = discretise(npde, c, chain, 64, theta)
    l1, g1 = rep2.engine.loss_grad(theta)
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1)
    rep.engine.set_option("integral_nodes", "2")
    rep.engine.set_points(0, big)                                         # 4,200,000 sites: fine
    with pytest.raises(npde.EngineError, match=r"integral_nodes = 64 makes a site set of 91000000 sites(.|\n)*keeps 2"):
        rep.engine.set_option("integral_nodes", "64")
    assert rep.engine.get_option("integral_nodes") == "2" and "+integral(2)" in rep.engine.describe()


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def body_refusals(npde):
    (t,) = npde.parameters("t")
    x, y = npde.parameters("x y")
    (i,) = npde.variables("i")
    (u,) = npde.variables("u")
    chain1 = make_chain(npde, 1, "w16")
    dom1 = [npde.In(t, npde.Interval(0.0, 2.0))]
    strat = npde.GridTraining(0.25)

    def disc1(eq, chain=chain1, **kw):
        kw.setdefault("precision", "f32")
        sysm = npde.PDESystem([eq], [npde.Eq(i(0.0), 0.0)], dom1, [t], [i(t)])
        return npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, **kw))

    Ii = npde.Integral(npde.In(t, npde.Interval(0.0, t)))
    good = npde.Eq(npde.Differential(t)(i(t)) + 5 * Ii(i(t)), 1)
    # nested integrals
    with pytest.raises(npde.LoweringError, match="nested integrals"):
        disc1(npde.Eq(Ii(Ii(i(t))), 1))
    # multi-variable integrals
    with pytest.raises(npde.LoweringError, match="multi-variable integrals"):
        npde.Integral(npde.In((x, y), npde.ProductDomain(npde.Interval(0.0, 1.0), npde.Interval(0.0, 1.0))))
    # infinite bounds
    with pytest.raises(npde.LoweringError, match="infinite"):
        disc1(npde.Eq(npde.Integral(npde.In(t, npde.Interval(0.0, sp.oo)))(i(t)), 1))
    # a bound that is a general expression
    with pytest.raises(npde.LoweringError, match="general expression"):
        disc1(npde.Eq(npde.Integral(npde.In(t, npde.Interval(0.0, t ** 2)))(i(t)), 1))
    # an integrand over a DGM network
    with pytest.raises(npde.EngineError, match="integral terms over a DGM network"):
        disc1(good, chain=npde.DGM(1, 1, 8, 1, "tanh", "tanh"))
    # ... or a periodically embedded coordinate
    emb = npde.Chain(npde.PeriodicEmbedding([1], [2.0]), npde.Dense(2, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    with pytest.raises(npde.EngineError, match="periodic input embedding"):
        disc1(good, chain=emb)
    # several dependent variables in one integral equation
    (v,) = npde.variables("v")
    sys2 = npde.PDESystem([npde.Eq(Ii(i(t)) + v(t), 1), npde.Eq(npde.Differential(t)(v(t)), i(t))], [npde.Eq(i(0.0), 0.0), npde.Eq(v(0.0), 0.0)],
                          dom1, [t], [i(t), v(t)])
    with pytest.raises(npde.EngineError, match="one dependent variable"):
        npde.symbolic_discretize(sys2, npde.PhysicsInformedNN([chain1, make_chain(npde, 1, "w16")], strat, precision="f32"))
    # the float64 evaluation mode: Float64 parameters under precision = "auto" fail at discretize time, naming the opt-in
    th64 = tp.theta_for(chain1, 3)
    with pytest.raises(npde.EngineError, match=r'integral terms run on the fp32 kernels(.|\n)*precision = "f32"'):
        disc1(good, init_params=th64, precision="auto")
    with pytest.raises(npde.EngineError, match=r'integral terms run on the fp32 kernels(.|\n)*precision = "f32"'):
        disc1(good, init_params=th64, precision="f64")
    # a refused switch on a live fp32 handle leaves its plan usable
    rep = disc1(good, init_params=th64.astype(np.float32))
    l0, g0 = rep.engine.loss_grad(rep.flat_init_params)
    with pytest.raises(npde.EngineError, match=r'precision = "f32"'):
        rep.engine.set_option("precision", "f64")
    assert rep.engine.get_option("precision") == "f32"
    l1, g1 = rep.engine.loss_grad(rep.flat_init_params)
    assert np.array_equal(l0, l1) and np.array_equal(g0, g1)
    # integral_nodes outside 2..64
    for bad in (1, 65, 2.5):
        with pytest.raises(ValueError, match="integral_nodes must be an integer in 2..64"):
            npde.PhysicsInformedNN(chain1, strat, integral_nodes=bad)
    # malformed descriptor lines fail with named messages
    head = "pinnir 1\nntheta 321\nparams 0 0 321\ndefaults \nnets 1\nnet 0 tanh 0 4 1 16 16 1\nterms 1\nterm 0 1 0 1 1\n"
    for block, msg in (("integrals 9\n", "integrals line"),
                       ("integrals 1\nintegral 3 0.0 x0 1 1 2\n", "integral variable is not a coordinate"),
                       ("integrals 1\nintegral 0 0.0 x4 1 1 2\n", "integral bound names a coordinate"),
                       ("integrals 1\nintegral 0 0.0 inf 1 1 2\n", "infinite integral bounds"),
                       ("integrals 1\nintegral 0 0.0 t*t 1 1 2\n", "general expression"),
                       ("integrals 1\nintegral 0 0.0 x0 0 1 2\n", "must contain a dependent variable"),
                       ("integrals 1\nintegral 0 0.0 x0 1 1 9\nslot 0 0 \nop ADDC 1 0 0.0\n", "integral out row out of range"),
                       ("integrals 1\nintegral 0 0.0 x0 2 1 3\nslot 0 0 \nslot 0 0 \nop ADD 1 2 0.0\n", "an integral node lists the same slot twice")):
        with pytest.raises(npde.EngineError, match=msg):
            npde.Engine(head + block + "op ADDC 1 0 0.0\n")


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. point shards over a communicator: sites are local to a point
# ------------------------------------------------------------------------------------------------------------------------------------
def test_integral_terms_sharded_over_two_emulated_devices(npde, use_emu):
    """Each rank expands the sites of its own points; two emulated devices = the single handle (as tests/test_engine_comm.py compares them)."""
    c = ide(npde)
    chain = make_chain(npde, 1, "w16")
    theta = tp.theta_for(chain, 41).astype(np.float32)
    rep, sets = discretise(npde, c, chain, 16, theta)
    w = np.array([1.0, 2.0], dtype=np.float32)
    L0, G0 = rep.engine.loss_grad(theta, w)
    engs = [npde.Engine(rep.engine.descriptor, device=g) for g in range(2)]
    for g, e in enumerate(engs):
        e.set_option("integral_nodes", "16")
        for k, s_ in enumerate(sets):
            n = s_.shape[1]
            lo, hi = (n * g) // 2, (n * (g + 1)) // 2
            if hi == lo:                                     # (a one-point boundary set: both ranks hold it, normalised to 2 N)
                e.set_points(k, s_, n_norm=2 * n)
            else:
                e.set_points(k, s_[:, lo:hi], n_norm=n)
    npde.comm_init_all(engs)
    L, G = npde.loss_grad_sharded(engs, theta, w)
    np.testing.assert_allclose(L, L0, rtol=1e-6)
    assert np.linalg.norm(G - G0) / np.linalg.norm(G0) < TOL
    for e in engs:
        e.comm_destroy()


# ------------------------------------------------------------------------------------------------------------------------------------
# the two expositions of every body
# ------------------------------------------------------------------------------------------------------------------------------------
BODIES = [("parity_%s_%s%s" % (case, kind, "_" + gemm if gemm else ""), body_parity, {"case": case, "kind": kind, "gemm": gemm})
          for case in CASES for kind, gemm in (("w16", None), ("w64", "split"), ("w64", "fp32"), ("odd", None))
          if kind != "odd" or case == "ide"]
BODIES += [
    ("rule_sanity", body_rule_sanity, {}),
    ("resampling_uniform", body_resampling, {"kind_name": "uniform"}),
    ("resampling_lhs", body_resampling, {"kind_name": "lhs"}),
    ("resampling_sobol", body_resampling, {"kind_name": "sobol"}),
    ("training", body_training, {}),
    ("option_replans", body_option_replans, {}),
    ("replan_buffer_reuse", body_replan_buffer_reuse, {}),
    ("pinnir2", body_pinnir2, {}),
    ("point_weights", body_point_weights, {}),
    ("point_data", body_point_data, {}),
    ("site_set_too_large", body_site_set_too_large, {}),
    ("refusals", body_refusals, {}),
]
_PARAMS = [pytest.param(fn, kw, id=name) for name, fn, kw in BODIES]


@pytest.mark.parametrize("fn,kw", _PARAMS)
def test_integral_terms(npde, use_emu, fn, kw):
    fn(npde, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("fn,kw", _PARAMS)
def test_integral_terms_on_hardware(npde, hip_lib, monkeypatch, fn, kw):
    monkeypatch.setattr(tp, "EXPECTED_BACKEND", "hip")
    assert npde._lib.default_library().backend == "hip", "the hardware twin must run on the product library"
    fn(npde, **kw)
