"""Shape table and references of tests/test_layer_shapes.py: Dense chains whose hidden layers differ in width (tapering, widening, hourglass,
narrow first layer), one row of shapes per kernel site, and what the engine's numbers are compared with — oracle/pinn_oracle.py in its
exact-derivative mode and a plain numpy MLP.  Nothing here evaluates the engine.

Every reference is computed once per process (per case: shape, activations, problem, seed) and shared by the fp32 and the float64 cases and
by the emulation and the hardware expositions: the parameters are float32-representable (glorot_theta rounded to float, kept as doubles), so
an fp32 handle and a float64 handle are given the same numbers."""
import numpy as np
import torch

import helpers
import pinn_oracle as po
import test_emu_parity as tp

# ---- the shape table: (sizes, activation per hidden layer or one name) ---------------------------------------------------------------
HP16 = [((2, 16, 8, 1), "tanh"), ((2, 7, 12, 5, 1), "sigmoid"), ((2, 16, 1, 16, 1), "tanh"), ((1, 1, 1, 1), "sigmoid"),
        ((2, 12, 5, 1), ("tanh", "sigmoid"))]
HP32 = [((2, 16, 32, 1), "tanh"), ((2, 32, 9, 1), "sigmoid"), ((1, 20, 3, 1), "tanh"), ((3, 10, 24, 1), "sigmoid")]
HP64 = [((2, 64, 40, 64, 1), "tanh"), ((2, 40, 64, 33, 1), "tanh"), ((2, 64, 1, 1), "sigmoid"), ((2, 1, 64, 1), "tanh")]
HP128 = [((2, 128, 70, 100, 1), "tanh"), ((2, 65, 128, 90, 1), "tanh")]
SLICED_MORE = [((2, 65, 128, 1), "tanh"), ((2, 128, 70, 1), "sigmoid")]
LANES = [((2, 7, 12, 5, 1), "sigmoid"), ((2, 64, 40, 64, 1), "tanh")]
WEIGHTS = (1.0, 2.0, 0.5, 1.5, 3.0)            # unequal term weights (the first K of them)
BALANCE = 1e-2                                 # every parameter block's reference gradient norm >= BALANCE x the largest block's


def shape_id(sizes, acts):
    return "-".join(str(s) for s in sizes) + "-" + (acts if isinstance(acts, str) else "+".join(acts))


def act_list(sizes, acts):
    return [acts] * (len(sizes) - 2) if isinstance(acts, str) else list(acts)


def make_chain(npde, sizes, acts, embed=None):
    kinds = act_list(sizes, acts)
    layers = [npde.Dense(sizes[l], sizes[l + 1], kinds[l]) for l in range(len(sizes) - 2)] + [npde.Dense(sizes[-2], sizes[-1])]
    return npde.Chain(*(([embed] if embed is not None else []) + layers))


def uneven(sizes):
    """the table's rule: at least two adjacent hidden layers of different width"""
    hidden = sizes[1:-1]
    return any(a != b for a, b in zip(hidden[:-1], hidden[1:]))


def sobol(npde, seed, n=40, nb=20):
    return npde.QuasiRandomTraining(n, bcs_points=nb, sampling_alg=npde.SobolSample(seed=seed), resampling=False, minibatch=1)


def theta32(ochain, seed):
    """po.glorot_theta, rounded to float32 and kept in double"""
    return po.glorot_theta(ochain, np.random.default_rng(seed)).astype(np.float32).astype(np.float64)


def system_for(npde, sizes, problem):
    """"shape": the residuals of helpers.shape_problem for d = sizes[0] (mixed second derivatives; its own chain is not used);
    "poisson": tests/test_emu_parity.py: poisson2d's equation; "periodic": periodic_heat's problem"""
    if problem == "poisson":
        return tp.poisson2d(npde)[0]
    if problem == "periodic":
        return tp.periodic_heat(npde)[0]
    return helpers.shape_problem(npde, 16, 2, sizes[0])[0]


# ---- parameter blocks ------------------------------------------------------------------------------------------------------------------
def blocks(sizes, offset=0):
    """[(name, slice)] of W and b of every layer in the flat parameter vector (per layer W, n_out x n_in column-major, then b)"""
    out, o = [], offset
    for l in range(len(sizes) - 1):
        nw = sizes[l] * sizes[l + 1]
        out.append(("W%d" % l, slice(o, o + nw)))
        out.append(("b%d" % l, slice(o + nw, o + nw + sizes[l + 1])))
        o += nw + sizes[l + 1]
    return out


def block_norms(ref_grad, blks):
    return np.array([np.linalg.norm(ref_grad[s]) for _, s in blks])


def block_errors(grad, ref_grad, blks):
    """|| g_b - r_b || / || r_b || per parameter block"""
    g = np.asarray(grad, dtype=np.float64)
    return np.array([np.linalg.norm(g[s] - ref_grad[s]) / np.linalg.norm(ref_grad[s]) for _, s in blks])


# ---- the numpy MLP ---------------------------------------------------------------------------------------------------------------------
ACT = {"tanh": np.tanh, "sigmoid": lambda z: 1.0 / (1.0 + np.exp(-z)), "sin": np.sin, "swish": lambda z: z / (1.0 + np.exp(-z))}


def mlp(sizes, kinds, theta, pts):
    """theta: per layer W (n_out x n_in, column-major), then b; pts (d x N) -> (N,)"""
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


_U = lambda cord, th, phi: phi(cord, th)


def exact_derivative(ochain, theta, pts, axes):
    th = torch.tensor(np.asarray(theta[:ochain.nparams], dtype=np.float64), dtype=po.DT)
    return po.exact_derivative(ochain, _U, torch.tensor(np.asarray(pts, dtype=np.float64), dtype=po.DT), list(axes), th).detach().numpy().reshape(-1)


def derivative_axes(d):
    """orders 1 and 2, one of them mixed where the net has two inputs"""
    return [[0], [d - 1, d - 1], [0, d - 1]] if d > 1 else [[0], [0, 0]]


# ---- references, once per case ---------------------------------------------------------------------------------------------------------
_REF = {}


class Reference:
    """the oracle's view of one case: problem, point sets, parameters, weights, loss / gradient / per-term gradients in exact mode, host
    points with phi (numpy MLP) and the exact derivatives"""


def reference(npde, rep, sysm, chains, key, seed, weights=None):
    """-> Reference for `key`; the first caller's handle supplies the (deterministic) point sets, later callers are checked against them"""
    sets = rep.pde_train_sets + rep.bcs_train_sets
    if key not in _REF:
        R = Reference()
        R.prob = helpers.oracle_problem(npde, sysm, chains)
        R.sets = [np.array(s, dtype=np.float64) for s in sets]
        R.theta = np.concatenate([theta32(oc, seed + i) for i, oc in enumerate(R.prob.chains)])
        R.w = np.asarray(WEIGHTS[:len(sets)] if weights is None else weights, dtype=np.float64)
        ev = po.loss_and_grad(R.prob, R.theta, R.sets, weights=R.w, mode="exact", per_term_grads=True)
        R.term_losses, R.grad, R.term_grads = ev.term_losses, ev.grad, ev.term_grads
        R.ev = ev
        R.blocks, o = [], 0
        for i, oc in enumerate(R.prob.chains):
            R.blocks += [("net%d.%s" % (i, n), s) for n, s in blocks(oc.sizes, o)]
            o += oc.nparams
        for a in (R.theta, R.w, R.term_losses, R.grad, R.term_grads, *R.sets):
            a.setflags(write=False)
        R.points = {}
        _REF[key] = R
    R = _REF[key]
    assert len(sets) == len(R.sets) and all(np.array_equal(a, b) for a, b in zip(sets, R.sets)), "the case's point sets changed"
    return R


def host_points(R, net=0):
    """70 host points in the unit cube with phi from the numpy MLP and the oracle's exact derivatives of orders 1 and 2"""
    if net not in R.points:
        oc = R.prob.chains[net]
        off = sum(c.nparams for c in R.prob.chains[:net])
        th = R.theta[off:off + oc.nparams]
        d = oc.sizes[0]
        pts = np.random.default_rng(70 + d).uniform(0.0, 1.0, size=(d, 70))
        kinds = act_list(oc.sizes, oc.act if "," not in oc.act else tuple(oc.act.split(",")))
        phi = mlp(oc.sizes, kinds, th, pts)
        ders = {tuple(ax): exact_derivative(oc, th, pts, ax) for ax in derivative_axes(d)}
        for a in (pts, phi, *ders.values()):
            a.setflags(write=False)
        R.points[net] = (pts, phi, ders)
    return R.points[net]
