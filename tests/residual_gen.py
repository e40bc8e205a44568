"""Seeded generator of random residual programs for tests/test_random_residuals.py: equations assembled from the atoms, coefficients and
term shapes the planner's rewrites act on (program.cpp: analyse_static, fuse_laplacian; plan.cpp: detect_linear, riding boundary terms,
coupled / tail / two-launch paths; f64_setup.cpp: f64_affine; sexpr.cpp), so that sign patterns and shared subexpressions nobody wrote by hand
reach them.  Deterministic in (family, seed) through numpy.random.default_rng; plain Python + sympy.

    case(npde, family, seed) -> Case(sysm, chains, theta, param_estim, symbolic, record)

Families (the smallest shapes at which the code paths differ; all kernels are in the ahead-of-time table):
    single  one network, d in {1, 2, 3}, 2 x 16, tanh (a third of the seeds: sigmoid)       family 1 kernels
    wide    one network, d = 2, 4 x 64 tanh                                                  family 2 register tape
    system  2 or 3 networks, d = 2, 2 x 16 tanh                                              forward / k_expr / reverse launches
            (a quarter of the seeds: 2 x 64, family 2 — only those kernels run the fused tail launch)
    params  as single (d = 2) and system (2 networks) with PDE parameters a = 0.7, b = -1.3  half the seeds estimated, half fixed
    long    one network, d = 2, 2 x 16: more than 32 tape rows after hoisting                the two-launch path of one network
Odd seeds go through the symbolic front end ("pinnir 2"), even seeds through the tape form."""
from collections import namedtuple

import numpy as np
import sympy as sp

import pinn_oracle as po

FAMILIES = ("single", "wide", "system", "params", "long")
CONSTS = (1, -1, 2, 0.5, -0.3, 3, 1.5)
N_INTERIOR, N_BOUNDARY = 37, 19
PARAM_DEFAULTS = (0.7, -1.3)            # neither is a float32 number: a float copy of a fixed parameter shows at 1e-8 in the float64 mode
N_BLOCKS = 6

Case = namedtuple("Case", "sysm chains theta param_estim symbolic record")


def _stream(family, seed):
    return np.random.default_rng([FAMILIES.index(family), int(seed)])


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _coord_fn(rng, ivs):
    v, w = _pick(rng, ivs), _pick(rng, ivs)
    return _pick(rng, (sp.exp(-v), 1 + v * w, sp.sin(sp.pi * v), sp.cos(v) + 2, v, sp.sqrt(1 + w)))


class _Net:
    """one dependent variable on the interior point: its atoms"""

    def __init__(self, npde, fn, ivs):
        self.fn, self.ivs = fn, ivs
        self.U = fn(*ivs)
        self.D = [npde.Differential(v) for v in ivs]
        self.first = [D(self.U) for D in self.D]
        self.pure = [(D ** 2)(self.U) for D in self.D]
        self.mixed = [self.D[i](self.D[j](self.U)) for i in range(len(ivs)) for j in range(i + 1, len(ivs))]

    def atom(self, rng, second=True):
        pool = ([self.U] * 2 + self.first) * 2 + ((self.pure + self.mixed) if second else [])
        return _pick(rng, pool)


def _laplacian_block(rng, net, ivs, coef, pattern):
    """the terms of one equation's second-derivative block (the sign / coefficient patterns fuse_laplacian has to tell apart)"""
    d = len(ivs)
    c = coef()
    if pattern == 0:                                       # c u_aa for all axes
        return [c * p for p in net.pure]
    if pattern == 1:                                       # all axes but one with another coefficient
        c2 = coef()
        odd = int(rng.integers(d))
        return [(c2 if a == odd and d > 1 else c) * p for a, p in enumerate(net.pure)]
    if pattern == 2:                                       # c (sum u_aa): one term
        return [c * sp.Add(*net.pure)]
    if pattern == 3:                                       # c u_xx - c u_yy
        return [c * net.pure[0]] + [-c * p for p in net.pure[1:2]] + [c * p for p in net.pure[2:]]
    if pattern == 4:                                       # f(x) (sum u_aa)
        return [_coord_fn(rng, ivs) * sp.Add(*net.pure)]
    return [c * p for p in net.pure] + [_pick(rng, net.pure) * net.U]      # all axes, and one second derivative used twice


def _shaped_term(rng, nets, ivs, coef, linear):
    a = _pick(rng, nets).atom(rng)
    if linear:
        return coef() * a
    b = _pick(rng, nets).atom(rng, second=False)
    u = _pick(rng, nets).U
    shape = int(rng.integers(8))
    return (coef() * a, _coord_fn(rng, ivs) * a, a * b, sp.sin(a), sp.tanh(a), sp.exp(-u ** 2), a ** 2, a / (2 + sp.cos(ivs[0])))[shape]


def _long_terms(rng, net):
    """the forced terms of the long family: the residual of test_long_residual_takes_the_two_launch_path, each with a drawn coefficient"""
    U, (ux, uy), (uxx, uyy), uxy = net.U, net.first, net.pure, net.mixed[0]
    forced = [uxx * sp.exp(U), uyy * sp.cos(U), U ** 3 * ux, sp.tanh(U) * uy, sp.sin(U) * sp.cos(U) / (1 + U ** 2), sp.exp(-U ** 2) * ux ** 2,
              sp.log(1 + U ** 2) * uy ** 2, sp.sqrt(1 + U ** 2), sp.sinh(U) * sp.cosh(U) * 1e-2, uxy * U, (U + 0.5) ** 4 * 0.01]
    return [_pick(rng, CONSTS) * t for t in forced]


def _boundary_term(npde, rng, fn, ivs):
    """Dirichlet (constant or coordinate data), Robin, or a condition with a derivative on the right-hand side, on one face of the unit box"""
    d = len(ivs)
    axis, side = int(rng.integers(d)), int(rng.integers(2))
    args = [sp.Integer(side) if a == axis else v for a, v in enumerate(ivs)]
    ub = fn(*args)
    free = [v for a, v in enumerate(ivs) if a != axis]
    data = _coord_fn(rng, free) if free and rng.integers(2) else sp.Float(_pick(rng, CONSTS)) * 0.5
    Dn = npde.Differential(ivs[axis])
    kind = int(rng.integers(4))
    if kind <= 1:
        return npde.Eq(ub, data if kind else 0.25 * float(_pick(rng, CONSTS)))
    if kind == 2:
        return npde.Eq(ub + _pick(rng, CONSTS) * Dn(ub), data)
    Dt = npde.Differential(_pick(rng, ivs))
    return npde.Eq(ub, _pick(rng, CONSTS) * Dt(ub) + data)


def case(npde, family, seed):
    rng = _stream(family, seed)
    symbolic = bool(seed % 2)
    nparam = 0
    estim = False
    act = "tanh"
    width, hidden = 16, 2
    if family == "single":
        d, nnet = 1 + int(rng.integers(3)), 1
        act = "sigmoid" if seed % 3 == 2 else "tanh"
    elif family == "wide":
        d, nnet, width, hidden = 2, 1, 64, 4
    elif family == "system":
        d, nnet = 2, 2 + (seed // 2) % 2
        if seed % 4 == 1:
            width = 64                  # 2 x 64 (family 2): the shape at which a coupled equation's widest network runs the fused tail launch
    elif family == "params":
        d, nnet, nparam = 2, 1 + (seed // 4) % 2, 2
        estim = bool((seed // 2) % 2)
    elif family == "long":
        d, nnet = 2, 1
    else:
        raise ValueError(family)
    ivs = list(npde.parameters(" ".join("xyz"[:d])))
    fns = list(npde.variables(" ".join(f"u{i + 1}" for i in range(nnet)) if nnet > 1 else "u"))
    nets = [_Net(npde, f, ivs) for f in fns]
    ps = list(npde.parameters("a b")) if nparam else []
    reads = set()

    def coef():
        if ps and rng.integers(2):
            p = _pick(rng, ps)
            reads.add(str(p))
            return p
        return _pick(rng, CONSTS)

    linear = family in ("single", "params") and seed % 5 == 0            # constant coefficients, no products: the affine shortcuts' domain
    eqs, blocks = [], []
    for e in range(nnet):
        pattern = int(rng.integers(N_BLOCKS))
        if linear and pattern in (4, 5):
            pattern -= 4
        blocks.append(pattern)
        terms = _laplacian_block(rng, nets[e], ivs, coef, pattern)
        if family == "long":
            terms += _long_terms(rng, nets[e])
        for _ in range(1 + int(rng.integers(3))):
            terms.append(_shaped_term(rng, nets, ivs, coef, linear))
        if ps and e == 0:                                               # every params case reads a parameter in a linear and a nonlinear place
            terms.append(ps[0] * nets[0].first[0])
            terms.append(ps[1] * (nets[0].U if linear else nets[0].U ** 2))
            reads.update(str(p) for p in ps)
        if rng.integers(3):
            terms.append(_coord_fn(rng, ivs) * _pick(rng, CONSTS))      # forcing
        order = rng.permutation(len(terms))
        cut = 1 + int(rng.integers(len(terms)))
        eqs.append(npde.Eq(sp.Add(*[terms[i] for i in order[:cut]]), sp.Add(*[terms[i] for i in order[cut:]])))
    bcs = [_boundary_term(npde, rng, _pick(rng, fns), ivs) for _ in range(1 + int(rng.integers(3)))]
    dom = [npde.In(v, npde.Interval(0.0, 1.0)) for v in ivs]
    kw = dict(ps=ps, defaults=dict(zip(ps, PARAM_DEFAULTS))) if ps else {}
    sysm = npde.PDESystem(eqs, bcs, dom, ivs, [n.U for n in nets], **kw)
    layers = lambda: [npde.Dense(d, width, act)] + [npde.Dense(width, width, act) for _ in range(hidden - 1)] + [npde.Dense(width, 1)]
    chains = [npde.Chain(*layers()) for _ in range(nnet)]
    theta = np.concatenate([po.glorot_theta(po.Chain(tuple(c.sizes), c.act), np.random.default_rng([7, FAMILIES.index(family), int(seed), i]))
                            for i, c in enumerate(chains)])
    record = dict(family=family, seed=seed, d=d, nnet=nnet, act=act, width=width, blocks=blocks, linear=linear, symbolic=symbolic,
                  estimated=estim and bool(ps), fixed_params_read=sorted(reads) if ps and not estim else [])
    return Case(sysm, chains, theta, estim, symbolic, record)


def strategy(npde, seed):
    return npde.QuasiRandomTraining(N_INTERIOR, bcs_points=N_BOUNDARY, sampling_alg=npde.SobolSample(seed=1 + seed % 50), resampling=False, minibatch=1)
