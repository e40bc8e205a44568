"""The op x interpreter matrix of tests/test_op_matrix.py: a table of op cases (one expression per tape op, written so that the op gets a
network-dependent operand in every operand position that has an adjoint) and a table of interpreter sites (the smallest handle that makes
the planner run the residual tape in one particular interpreter).  Plain Python + sympy; deterministic.

    problem(npde, case, site) -> Problem(sysm, chains, theta, symbolic, expr, atoms)
    conditions(expr) -> the subexpressions whose values decide whether a case is well-conditioned (bases, denominators, branch deciders)

The atoms of a case: U (the network), V (a second network at the two-network sites; u_y elsewhere), u_x, u_y, u_xx and the coordinates x, y.
The equation of every case:  u_xx + 0.5 u_yy + 1.5 expr = sin(pi x) y  with two Dirichlet terms (two-network sites: + 0.25 V on the left, a
second equation v_xx + v_yy + U V = x y, and one Dirichlet term per network)."""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import sympy as sp

import pinn_oracle as po

N_INTERIOR, N_BOUNDARY = 37, 19
INT_Q = 4                       # Gauss-Legendre nodes of the integral site (the smallest count tests/test_integral_terms.py uses)

Case = namedtuple("Case", "name ops expr kind")        # kind: "adj" (the op has a network operand), "src" (coordinate-only argument: k_src)
Site = namedtuple("Site", "name nnet width hidden arch precision pad seed")
Problem = namedtuple("Problem", "sysm chains theta symbolic expr atoms")


def _c(name, ops, expr, kind="adj"):
    return Case(name, tuple(ops.split()), expr, kind)


# op codes are those of csrc/rprog.hpp / ir.OPS.  A constant in a case keeps it inside the conditions of test_op_matrix (bases and
# denominators > 0.5, branch deciders away from zero with both branches taken): change it there, never a bar.
CASES = [
    _c("tan", "TAN", lambda A: sp.tan(0.5 * A.U)),
    _c("sech", "SECH", lambda A: sp.sech(A.U)),
    _c("powc_1.5", "POWC", lambda A: (2 + A.U) ** 1.5),
    _c("powc_-0.7", "POWC", lambda A: (2 + A.U) ** (-0.7)),
    _c("pow_net_net", "POW", lambda A: (2 + A.U) ** (1 + 0.5 * A.ux)),                   # both adjoints
    _c("pow_net_src", "POW", lambda A: (2 + A.U) ** (1 + A.x)),                          # the exponent is a hoisted source: the base adjoint only
    _c("powi_-2", "POWI", lambda A: (2 + A.U) ** (-2)),
    _c("powi_2", "POWI", lambda A: (A.U + A.ux) ** 2),
    _c("powi_3", "POWI", lambda A: (A.U + 0.5 * A.V) ** 3),
    _c("powi_4", "POWI", lambda A: (0.5 + A.U) ** 4),
    _c("div", "DIV", lambda A: A.uxx / (2 + A.U ** 2)),
    _c("div_net_net", "DIV", lambda A: (A.U * A.ux) / (2 + sp.cos(A.V))),
    _c("max_net_net", "MAX", lambda A: sp.Max(A.U + A.x, A.V + 1 - A.x)),
    _c("min_net_net", "MIN", lambda A: sp.Min(A.U + A.x, A.V + 1 - A.x)),
    _c("max_net_src", "MAX", lambda A: sp.Max(A.U + A.x, 1.2 * A.y)),                    # the other side is a source channel
    _c("min_net_src", "MIN", lambda A: sp.Min(A.U + A.x, 1.2 * A.y)),
    _c("max_3", "MAX", lambda A: sp.Max(0.3 * A.U + A.x, 0.3 * A.V + 1 - A.x, 0.25 + A.y)),
    _c("min_3", "MIN", lambda A: sp.Min(0.3 * A.U + A.x, 0.3 * A.V + 1 - A.x, 0.25 + A.y)),
    _c("sinpi", "SINPI", lambda A: sp.sin(sp.pi * A.U)),
    _c("cospi", "COSPI", lambda A: sp.cos(sp.pi * (0.5 * A.ux))),
    _c("abs", "ABS", lambda A: sp.Abs(A.ux + 3 * (A.x - 0.6))),
    _c("log", "LOG", lambda A: sp.log(2 + A.U)),
    _c("sqrt", "SQRT", lambda A: sp.sqrt(2 + A.U)),
    _c("sinh", "SINH", lambda A: sp.sinh(A.U)),
    _c("cosh", "COSH", lambda A: sp.cosh(A.ux)),
    _c("sin", "SIN", lambda A: sp.sin(A.U + A.ux)),
    _c("cos", "COS", lambda A: sp.cos(2 * A.U)),
    _c("exp", "EXP", lambda A: sp.exp(-A.U)),
    _c("tanh", "TANH", lambda A: sp.tanh(A.ux)),
    # the bilinear ops with a network operand on each side (the product keeps the residual out of the affine shortcuts)
    _c("bilinear", "ADD SUB MUL NEG ADDC MULC", lambda A: (A.U + A.ux) * (A.uy - A.U) - (0.3 + A.U) * A.V + (-A.U - A.ux) * A.uxx),
    # every unary (and binary) op once more on a coordinate-only argument: evaluated by k_src per point set, no adjoint
    _c("src_a", "TAN SECH POWC POW POWI ABS DIV", lambda A: A.U * (sp.tan(0.5 * A.x) + sp.sech(A.y) + (1 + A.x) ** 1.5 + (1 + A.x) ** (0.5 + A.y)
                                                           + (1 + A.y) ** (-2) + sp.Abs(A.x - 0.45) + A.x / (1 + A.y)), "src"),
    _c("src_b", "LOG SQRT SINH COSH SIN COS", lambda A: A.U * (sp.log(1 + A.x) + sp.sqrt(1 + A.y) + sp.sinh(A.x) + sp.cosh(A.y) + sp.sin(A.x * A.y)
                                                          + sp.cos(A.x - A.y)), "src"),
    _c("src_c", "EXP TANH SINPI COSPI MAX MIN", lambda A: A.U * (sp.exp(-A.x) + sp.tanh(A.y) + sp.sin(sp.pi * A.x * 0.5) + sp.cos(sp.pi * A.y)
                                                            + sp.Max(A.x, 0.9 - A.y) + sp.Min(A.x, A.y ** 2)), "src"),
]
CASE = {c.name: c for c in CASES}
ADJ = [c.name for c in CASES if c.kind == "adj"]
SRC = [c.name for c in CASES if c.kind == "src"]
STENCIL = ["tan", "pow_net_net", "div", "max_net_net", "sqrt"]          # derivative = stencil changes the slots, not the tape: a handful of ops

# 33 rows on the 2 x 16 kernel that serves {u, u_x, u_y, u_xx, u_yy} (the 6-channel Hessian kernel of the ahead-of-time table) and 32 with the
# 5 channels the residual reads: the planner has to count the kernel's channels when it chooses between the fused tape and the two-launch path
ROWS_33 = Case("rows_33", ("ADD", "SUB", "MUL", "NEG", "ADDC", "MULC"),
               lambda A: (A.U + A.ux) * (A.uy - A.U) - (0.3 + A.U) * A.ux + 0.7 * (A.U * A.uy) - A.ux * A.uy + 0.1 * (-A.U - A.ux) * A.uxx, "adj")

# padding of the "long" site: cheap nonlinear terms that push the residual past the 32 LDS tape rows of a fused launch (plan.cpp: two_launch)
_PAD = lambda A: 0.01 * (A.uxx * sp.exp(A.U) + A.U ** 3 * A.ux + sp.tanh(A.U) * A.uy + sp.sin(A.U) * sp.cos(A.U) / (1 + A.U ** 2)
                         + sp.exp(-A.U ** 2) * A.ux ** 2 + sp.log(1 + A.U ** 2) * A.uy ** 2 + sp.sqrt(1 + A.U ** 2) + (A.U + 0.5) ** 4)

# name: networks, width, hidden layers, architecture, precision of the checks, padded, parameter seed
SITES = [
    Site("f1", 1, 16, 2, "dense", "f32", False, 3),               # family 1: LDS tape (pinn_kernels.hpp)
    Site("f2", 1, 64, 4, "dense", "f32", False, 4),               # family 2: register tape (pinn_kernels2.hpp)
    Site("sys16", 2, 16, 2, "dense", "f32", False, 5),            # forward / k_expr / reverse launches (aux_kernels.hpp)
    Site("sys64", 2, 64, 2, "dense", "f32", False, 6),            # the fused tail launch
    Site("long", 1, 16, 2, "dense", "f32", True, 7),              # the two-launch path of one network
    Site("dgm", 1, 8, 1, "dgm", "f32", False, 8),                 # family 3: one lane per point (pinn_kernels3.hpp)
    Site("int", 1, 16, 2, "integral", "f32", False, 10),          # the integrand of an integral term (aux_kernels.hpp: k_int_expr), fp32 only
    Site("f64_4m", 1, 16, 2, "dense", "f64", False, 7),           # float64 tiles (pinn_kernels5.hpp); the same handle under PINN_F64_NO_MFMA: lanes
    Site("f64_4s", 1, 65, 2, "dense", "f64", False, 9),           # float64 sliced tiles (pinn_kernels6.hpp): the narrowest 2-D width past family 4m
]
SITE = {s.name: s for s in SITES}


def atoms(npde, nnet):
    x, y = npde.parameters("x y")
    fns = list(npde.variables("u v")) if nnet == 2 else list(npde.variables("u"))
    Dx, Dy = npde.Differential(x), npde.Differential(y)
    U = fns[0](x, y)
    A = SimpleNamespace(x=x, y=y, fns=fns, U=U, ux=Dx(U), uy=Dy(U), uxx=(Dx ** 2)(U), uyy=(Dy ** 2)(U), Dx=Dx, Dy=Dy)
    A.V = fns[1](x, y) if nnet == 2 else A.uy
    return A


def chain_of(npde, site):
    if site.arch == "dgm":
        return npde.DGM(2, 1, site.width, site.hidden, "tanh", "tanh", "identity")
    return npde.Chain(npde.Dense(2, site.width, "tanh"), *[npde.Dense(site.width, site.width, "tanh") for _ in range(site.hidden - 1)],
                      npde.Dense(site.width, 1))


def problem(npde, case, site, symbolic):
    A = atoms(npde, site.nnet)
    expr = case.expr(A)
    body = 1.5 * expr + (_PAD(A) if site.pad else 0)
    eqs = [npde.Eq(A.uxx + 0.5 * A.uyy + body + (0.25 * A.V if site.nnet == 2 else 0), sp.sin(sp.pi * A.x) * A.y)]
    if site.arch == "integral":         # u_y + u + int_0^1 1.5 expr(x, s) ds = sin(pi x) y, as tests/test_integral_terms.py (strip2d) builds it
        Iy = npde.Integral(npde.In(A.y, npde.Interval(0.0, 1.0)))
        eqs = [npde.Eq(A.uy + A.U + Iy(body), sp.sin(sp.pi * A.x) * A.y)]
    u = A.fns[0]
    bcs = [npde.Eq(u(0, A.y), 0.25 * A.y)]
    if site.nnet == 2:
        v = A.fns[1]
        eqs.append(npde.Eq((A.Dx ** 2)(A.V) + (A.Dy ** 2)(A.V) + A.U * A.V, A.x * A.y))
        bcs.append(npde.Eq(v(A.x, 1), sp.sin(A.x)))
    else:
        bcs.append(npde.Eq(u(A.x, 1), sp.sin(A.x)))
    dom = [npde.In(A.x, npde.Interval(0.0, 1.0)), npde.In(A.y, npde.Interval(0.0, 1.0))]
    sysm = npde.PDESystem(eqs, bcs, dom, [A.x, A.y], [f(A.x, A.y) for f in A.fns])
    chains = [chain_of(npde, site) for _ in range(site.nnet)]
    theta = np.concatenate([po.glorot_theta(po.Chain(tuple(c.sizes), c.act), np.random.default_rng([13, site.seed, i])) for i, c in enumerate(chains)])
    return Problem(sysm, chains, theta, symbolic, expr, A)


# op-rich problems for the persistent training kernel (tests/test_train_kernel.py): name -> (width, expression).  The kernel exists for
# family-1 launch groups only (adam.cpp: train_eligible) and the ahead-of-time table has no family-1 kernel for 2 x 64 (a 64-wide net runs
# family 2 and keeps the stand-alone loop), so the widest two-layer shape the kernel takes, 2 x 32, stands where a 2 x 64 problem would
TRAIN = {
    "ops_2x16": (16, lambda A: sp.sech(A.U) + sp.log(2 + A.U) * sp.sqrt(2 + A.U) + sp.sinh(A.U) * sp.cosh(A.ux) + sp.sin(sp.pi * A.U) + A.U ** 3),
    "ops_2x32": (32, lambda A: (2 + A.U) ** 1.5 + sp.Abs(A.ux) + sp.exp(-A.U) * sp.tanh(A.ux) + sp.Min(A.U + A.x, 1.2 * A.y)),
    "ops_max_pow_tan_div_2x16": (16, lambda A: sp.Max(A.U, A.uy + 0.2) + (2 + A.U) ** (1 + 0.5 * A.ux) + sp.tan(0.5 * A.U) + A.uxx / (2 + A.U ** 2)),
}


def train_problem(npde, name):
    """(PDESystem, chain, strategy, theta) of one op-rich problem: the equation of the matrix on 2 x width tanh, 37 + 2 x 19 fixed points"""
    width, expr = TRAIN[name]
    site = Site(name, 1, width, 2, "dense", "f32", False, 21 + len(name))
    P = problem(npde, Case(name, (), expr, "adj"), site, False)
    return P.sysm, P.chains[0], strategy(npde, site), P.theta


def strategy(npde, site):
    return npde.QuasiRandomTraining(N_INTERIOR, bcs_points=N_BOUNDARY, sampling_alg=npde.SobolSample(seed=1 + site.seed), resampling=False, minibatch=1)


def conditions(expr, is_dep):
    """[(kind, subexpression, network-dependent)] for every node of `expr` whose operand values decide the conditioning of the case:
    "base" (LOG, SQRT, POW, POWC: > 0.5), "den" (DIV, negative integer powers: magnitude > 0.5), "decide" (MAX / MIN fold steps a - b in the
    order the front ends fold them; ABS: a — magnitude > 1e-4 and, where the node is network-dependent, both signs on >= 5 points)."""
    out = []
    for e in sp.preorder_traversal(expr):
        dep = is_dep(e)
        if e.is_Pow:
            b, p = e.args
            if p.is_Integer:
                if p < 0:
                    out.append(("den", b, dep))
            else:
                out.append(("base", b, dep))
        elif isinstance(e, sp.log):
            out.append(("base", e.args[0], dep))
        elif isinstance(e, sp.Abs):
            out.append(("decide", e.args[0], dep))
        elif isinstance(e, (sp.Max, sp.Min)):
            acc = e.args[0]
            for a in e.args[1:]:
                out.append(("decide", acc - a, dep))
                acc = type(e)(acc, a, evaluate=False)
    return out
