"""Pins the oracle (oracle/pinn_oracle.py) against every numeric pin the reference's own tests/docs hold for this path
(SURVEY.md §8c).  Beyond these the reference has no golden loss/gradient vectors: parity is otherwise unpinned."""
import numpy as np
import torch

import pinn_oracle as po


def test_get_eps_float32_order1_matches_debugging_doc():
    # docs/src/developer/debugging.md:64-65 prints 0.0049215667 for the Float32 first-order epsilon
    e = po.get_eps(2, 1, np.float32, 1)
    assert e.dtype == np.float32 and e[1] == 0
    assert abs(float(e[0]) - 0.0049215667) < 1e-9


def test_get_eps_float64_values():
    # eps(Float64)^(1/(2+order)), src/symbolic_utilities.jl:98-103
    for order, val in [(1, 6.0554544523933395e-06), (2, 1.220703125e-04), (3, 7.4009597974140505e-04), (4, 2.4607833005707410e-03)]:
        assert abs(po.get_eps(3, 2, np.float64, order)[1] - val) < 1e-15 * max(1.0, val / 1e-16) * 1e-3 + 1e-18


def test_forward_derivatives_fd_vs_exact():
    # restates test/Forward/forward__derivatives.jl:7-44: 2->16->16->1 sigmoid chain at [1, 2];
    # first order atol 1e-8, second order (xx, xy, yy) atol 4e-5
    chain = po.Chain((2, 16, 16, 1), "sigmoid")
    u = lambda cord, th, phi: phi(cord, th).sum(dim=0, keepdim=True)
    x = torch.tensor([[1.0], [2.0]], dtype=po.DT)
    for seed in range(5):
        theta = torch.tensor(po.glorot_theta(chain, np.random.default_rng(seed), bias_amp=0.0), dtype=po.DT)
        for ax in (0, 1):
            fd = po.numeric_derivative(chain, u, x, [po.get_eps(2, ax + 1, np.float64, 1)], 1, theta)
            ex = po.exact_derivative(chain, u, x, [ax], theta)
            assert abs(float(fd) - float(ex)) < 1e-8
        ex_, ey_ = po.get_eps(2, 1, np.float64, 2), po.get_eps(2, 2, np.float64, 2)
        for epss, axes in [([ex_, ex_], [0, 0]), ([ex_, ey_], [0, 1]), ([ey_, ey_], [1, 1])]:
            fd = po.numeric_derivative(chain, u, x, epss, 2, theta)
            ex = po.exact_derivative(chain, u, x, axes, theta)
            assert abs(float(fd) - float(ex)) < 4e-5


def test_forward_ode_golden(npde):
    # restates test/Forward/forward__ode.jl:10-47: parameter-free chain x -> x.^2, Dx(u(x)) ~ 0, GridTraining(0.1) on
    # [0, 1]: the datafree pde loss function returns 2x on the training set, rtol 1e-8
    import sympy as sp
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(u(x)), 0.0)
    bcs = [npde.Eq(u(0.0), u(0.0))]
    sysm = npde.PDESystem([eq], bcs, [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    vi = npde.get_vars(sysm.ivs, sysm.dvs)
    pde_sets, bc_sets = npde.generate_training_sets(sysm.domain, 0.1, sysm.eqs, sysm.bcs, np.float64, vi)
    train = pde_sets[0]
    assert train.shape[0] == 1 and train.shape[1] >= 10
    phi = lambda cord, th: cord ** 2
    cord = torch.tensor(train, dtype=po.DT)
    r = po.numeric_derivative(phi, po.get_u(), cord, [po.get_eps(1, 1, np.float64, 1)], 1, None) - 0.0
    np.testing.assert_allclose(r.numpy(), 2 * train, rtol=1e-8)


def test_numeric_derivative_orders_3_4_and_mixed_formulas():
    # src/pinn_types.jl:454-474 on an analytic function: u = sin(x) * exp(y)
    phi = lambda cord, th: torch.sin(cord[0:1]) * torch.exp(cord[1:2])
    x = torch.tensor([[0.3, 1.1], [0.2, -0.4]], dtype=po.DT)
    u = po.get_u()
    e3 = po.get_eps(2, 1, np.float64, 3)
    d3 = po.numeric_derivative(phi, u, x, [e3, e3, e3], 3, None)
    np.testing.assert_allclose(d3.numpy(), (-torch.cos(x[0:1]) * torch.exp(x[1:2])).numpy(), rtol=1e-5)
    e4 = po.get_eps(2, 1, np.float64, 4)
    d4 = po.numeric_derivative(phi, u, x, [e4] * 4, 4, None)
    np.testing.assert_allclose(d4.numpy(), (torch.sin(x[0:1]) * torch.exp(x[1:2])).numpy(), rtol=1e-4)
    ex_, ey_ = po.get_eps(2, 1, np.float64, 2), po.get_eps(2, 2, np.float64, 2)
    dxy = po.numeric_derivative(phi, u, x, [ex_, ey_], 2, None)
    np.testing.assert_allclose(dxy.numpy(), (torch.cos(x[0:1]) * torch.exp(x[1:2])).numpy(), rtol=1e-6)


def test_lux_dense_layout_and_phi():
    # [3P] Lux Dense / ComponentArrays flat layout: [W (out x in, column-major) | b | ...]
    chain = po.Chain((2, 3, 1), "tanh")
    theta = np.arange(1, chain.nparams + 1, dtype=np.float64) / 10
    W1 = theta[:6].reshape(2, 3).T
    b1 = theta[6:9]
    W2 = theta[9:12].reshape(3, 1).T
    b2 = theta[12:13]
    x = np.array([[0.5], [-1.0]])
    ref = W2 @ np.tanh(W1 @ x + b1[:, None]) + b2[:, None]
    np.testing.assert_allclose(po.phi_values(chain, theta, x), ref, rtol=1e-14)


def test_max_min_nodes_value_and_selected_branch_gradient():
    """sp.Max / sp.Min in build_residual.ev (n-ary, both modes) against a numpy evaluation written out by hand on fixed inputs; the gradient
    is the selected operand's gradient.  No point of this test sits on a tie (there torch splits the gradient in half, the engine gives
    it to one operand: DESIGN §6)."""
    import sympy as sp
    x, y = sp.symbols("x y")
    u = sp.Function("u")
    chain = po.Chain((2, 3, 1), "tanh")
    theta = np.linspace(-0.9, 1.1, chain.nparams)
    pts = np.array([[0.1, 0.35, 0.6, 0.85, 0.5], [0.9, 0.2, 0.7, 0.4, 0.05]])
    W1, b1, W2, b2 = theta[:6].reshape(2, 3).T, theta[6:9], theta[9:12].reshape(3, 1).T, theta[12:13]
    h = np.tanh(W1 @ pts + b1[:, None])
    U = (W2 @ h + b2[:, None])[0]
    ux = ((W2 * W1[:, 0]) @ (1 - h * h))[0]
    X, Y = pts
    cases = [(sp.Max(u(x, y), 0.2 + x), np.maximum(U, 0.2 + X), [U, 0.2 + X], np.argmax),
             (sp.Min(u(x, y), 0.2 + x), np.minimum(U, 0.2 + X), [U, 0.2 + X], np.argmin),
             (sp.Max(u(x, y), x * y, 0.5 - y), np.maximum(np.maximum(U, X * Y), 0.5 - Y), [U, X * Y, 0.5 - Y], np.argmax),
             (sp.Min(sp.Derivative(u(x, y), x) + 1.2, y - 0.5, 2 * x - 1.2), np.minimum(np.minimum(ux + 1.2, Y - 0.5), 2 * X - 1.2), [ux + 1.2, Y - 0.5, 2 * X - 1.2], np.argmin)]
    for mode in ("exact", "stencil"):
        for e, want, operands, pick in cases:
            prob = po.Problem(chains=[chain], depvars=[u], net_indvars=[(x, y)], pde_terms=[po.TermSpec(e, sp.Integer(0), (x, y))], bc_terms=[])
            got = po.residual_values(prob, theta, 0, pts, mode=mode)[0]
            ops = np.stack(operands)
            assert np.min(np.abs(np.diff(np.sort(ops, axis=0), axis=0))) > 1e-3                 # no tie, not nearly
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-14 if mode == "exact" or operands[0] is U else 1e-8)
            # d loss / d theta = that of the residual with every point's selected operand alone (the network operand where it is selected,
            # a coordinate function, whose gradient is zero, elsewhere)
            sel = pick(ops, axis=0)
            assert 0 < np.count_nonzero(sel == 0) < pts.shape[1]                                # both kinds of point occur
            g = po.loss_and_grad(prob, theta, [pts], mode=mode).grad
            net = po.TermSpec(e.args[[a.has(u) for a in e.args].index(True)], sp.Integer(0), (x, y))
            res_net = po.build_residual(po.Problem(chains=[chain], depvars=[u], net_indvars=[(x, y)], pde_terms=[net], bc_terms=[]), net, mode=mode)
            th = torch.tensor(theta, dtype=po.DT, requires_grad=True)
            r = res_net(torch.tensor(pts, dtype=po.DT), th)[0]
            mask = torch.tensor((sel == 0).astype(np.float64))
            (g_sel,) = torch.autograd.grad(torch.mean((r * mask + torch.tensor(want) * (1 - mask)) ** 2), th)
            np.testing.assert_allclose(g, g_sel.numpy(), rtol=1e-12, atol=1e-15)


# The stencil mode differentiates by finite differences, which turns the last bits of every float64 GEMM into ~1e-10 of a loss: the
# math library's code path (CPU model, thread count) then decides whether a 1e-12 pin holds.  The pinned stencil values of the fixtures
# below are therefore computed, and re-checked, in one child process with a fixed code path: MKL's conditional numerical
# reproducibility mode COMPATIBLE on one thread.
_FIXED_MODE_CHILD = r"""
import sys
import numpy as np
import torch
root, out = sys.argv[1], sys.argv[2]
sys.path[:0] = [root, root + "/oracle", root + "/tests"]
torch.set_num_threads(1)
import pinn_import, pinn_oracle as po, helpers, make_golden as mg
npde = pinn_import.load()
from neuralpde_jl_amd import workloads
makers = {"cfg1_poisson1d_1024": lambda: workloads.cfg1_poisson1d(1024),
          "cfg2_poisson2d_512": lambda: workloads.cfg2_poisson2d(points=512, bcs_points=128),
          "cfg3_burgers_512": lambda: workloads.cfg3_burgers(points=512, bcs_points=128)}
res = {}
for name in sys.argv[3:]:
    g = np.load(root + "/tests/golden/" + name + ".npz")
    if name in makers:
        wl = makers[name]()
        sets = [g["set%d" % k] for k in range(int(g["nsets"]))]
        prob = helpers.oracle_problem(npde, wl.pde_system, wl.chains)
        ev = po.loss_and_grad(prob, g["theta"], sets, weights=g["weights"], mode="stencil")
        res[name + "/losses"], res[name + "/grad"] = ev.term_losses, ev.grad
    else:
        wl = mg.FULL_CASES[name][0]()
        sets = mg.point_sets(wl)
        prob = helpers.oracle_problem(npde, wl.pde_system, wl.chains)
        res[name + "/losses"], res[name + "/grad"] = mg.chunked_loss_and_grad(prob, g["theta"], sets, g["weights"], chunk=int(g["chunk"]))
np.savez(out, **res)
"""


def _stencil_in_fixed_mode(tmp_path, names):
    """{name: (term losses, gradient)} of the stencil-mode oracle on the fixtures' own inputs, evaluated in a fresh process whose math
    library runs the fixed code path (MKL_CBWR has to be set before the library's first call, hence the child)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "fixed_mode.npz")
    env = dict(os.environ, MKL_CBWR="COMPATIBLE", OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-s", "-c", _FIXED_MODE_CHILD, root, out, *names], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    d = np.load(out)
    return {n: (d[n + "/losses"], d[n + "/grad"]) for n in names}


def test_golden_fixtures_reproduce(npde, tmp_path):
    """The committed fixtures (oracle/make_golden.py) are what the oracle computes today."""
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    names = ["cfg1_poisson1d_1024", "cfg2_poisson2d_512", "cfg3_burgers_512"]
    got = _stencil_in_fixed_mode(tmp_path, names)
    for name in names:
        g = np.load(os.path.join(root, name + ".npz"))
        losses, grad = got[name]
        np.testing.assert_allclose(losses, g["losses_stencil"], rtol=1e-12)
        np.testing.assert_allclose(grad, g["grad_stencil"], rtol=1e-9, atol=1e-14)
        # the two oracle modes (reference FD semantics vs exact derivatives) agree far inside the 1e-5 parity bar
        assert np.linalg.norm(g["grad_stencil"] - g["grad_exact"]) / np.linalg.norm(g["grad_exact"]) < 1e-6
        assert np.max(np.abs(g["losses_stencil"] - g["losses_exact"]) / g["losses_exact"]) < 1e-6


def test_full_size_fixtures_reproduce(npde, tmp_path):
    """The full-size fixtures (`python oracle/make_golden.py full`): the regenerated point sets have the pinned SHA-256 digests, and
    the benchmarked configuration's fixture (cfg2_full: 65,536 + 4 x 65,536 points) is what the oracle computes today."""
    import os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "oracle"))
    import make_golden as mg
    for name in ("cfg2_full", "cfg3_full"):
        g = np.load(os.path.join(root, "tests", "golden", name + ".npz"))
        wl = mg.FULL_CASES[name][0]()
        sets = mg.point_sets(wl)
        assert [mg.set_digest(s) for s in sets] == list(g["set_sha256"])
    g = np.load(os.path.join(root, "tests", "golden", "cfg2_full.npz"))
    losses, grad = _stencil_in_fixed_mode(tmp_path, ["cfg2_full"])["cfg2_full"]
    np.testing.assert_allclose(losses, g["losses_stencil"], rtol=1e-12)
    np.testing.assert_allclose(grad, g["grad_stencil"], rtol=1e-9, atol=1e-13)
