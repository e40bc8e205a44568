"""Adaptive cubature on the device (`pinn_cubature_refine / _get`) and `QuadratureTraining(adaptive=True)`.

The reference of the refinement is `restate` below: a numpy restatement of the algorithm of csrc/cub_kernels.hpp whose integrand values come from
the SAME handle's `set_points[_f64]` + `residual[_f64]` at the restatement's own nodes (or from an analytic g) — never from the cubature entry
points.  The reference of the integral's VALUE is a dense tensor Gauss-Legendre rule over the oracle's float64 residuals.

Making the integrand exact: a term `u(x..) ~ g(x..)` at theta = 0 has the residual -g, so the integrand r^2 = g^2 is any tape function of the
coordinates.  Dense(d, 4, tanh) -> Dense(4, 1) chains on unit cubes, float64 mode unless stated.

EDGE DISTANCE (a condition on the inputs, asserted on the restatement alone): device and restatement differ in the order of the 7..57-term sums
only, so they take the same decisions when every comparison the restatement makes is clear of its threshold by 1e3 u sum_j (|w7_j| + |w5_j|) v_j
share (err_i vs tau share_i, E vs tau: summed over the boxes) resp. 1e3 u max_j v_j (largest vs second largest fourth difference of a box that is
split); u = 2^-52 in float64 mode, 2^-24 on fp32 handles.

Every body is written once as a function of `npde` and exposed twice: on the CPU through the g++ emulation (`use_emu`) and, marked `gpu`, on the
product library (`hip_lib`).  Measured figures: profiles/adaptive_cubature.txt."""
import itertools

import numpy as np
import pytest
from numpy.polynomial.legendre import leggauss

import helpers
import pinn_oracle as po

U = {"f64": 2.0 ** -52, "f32": 2.0 ** -24}
L2, L3, L5 = np.sqrt(9.0 / 70.0), np.sqrt(9.0 / 10.0), np.sqrt(9.0 / 19.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# the rule and the restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def gm_rule(n):
    """-> nodes [M, n] on [-1, 1]^n in the kernels' lane order, w7 [M], w5 [M] (fractions of the mean)"""
    nodes, w7, w5 = [np.zeros(n)], [(12824.0 - 9120.0 * n + 400.0 * n * n) / 19683.0], [(729.0 - 950.0 * n + 50.0 * n * n) / 729.0]
    for lam, a7, a5 in ((L2, 980.0 / 6561.0, 245.0 / 486.0), (L3, (1820.0 - 400.0 * n) / 19683.0, (265.0 - 100.0 * n) / 1458.0)):
        for i in range(n):
            for s in (1.0, -1.0):
                e = np.zeros(n); e[i] = s * lam
                nodes.append(e); w7.append(a7); w5.append(a5)
    for i, j in itertools.combinations(range(n), 2):
        for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            e = np.zeros(n); e[i] = si * L3; e[j] = sj * L3
            nodes.append(e); w7.append(200.0 / 19683.0); w5.append(25.0 / 729.0)
    for signs in itertools.product((1.0, -1.0), repeat=n):
        nodes.append(L5 * np.array(signs)); w7.append(6859.0 / 19683.0 / 2 ** n); w5.append(0.0)
    return np.array(nodes), np.array(w7), np.array(w5)


def test_rule_constants():
    """the constants of DESIGN §4.13, pure numpy: 7 / 17 / 33 / 57 nodes; w7 exact to degree 7, w5 to degree 5 and off at degree 6.  (It checks the
    restatement's own table, not the library: it is the one test of this file that does not need the new entry points.)"""
    for n in (1, 2, 3, 4):
        x, w7, w5 = gm_rule(n)
        assert len(x) == (7, 17, 33, 57)[n - 1] and abs(w7.sum() - 1) < 1e-15 and abs(w5.sum() - 1) < 1e-15
        worst6 = 0.0
        for powers in itertools.product(range(8), repeat=n):
            deg = sum(powers)
            if deg > 7:
                continue
            exact = np.prod([0.0 if q % 2 else 1.0 / (q + 1) for q in powers])      # mean of the monomial over [-1, 1]^n
            mono = np.prod(x ** np.array(powers), axis=1)
            assert abs(np.dot(w7, mono) - exact) < 1e-15
            if deg <= 5:
                assert abs(np.dot(w5, mono) - exact) < 1e-15
            if deg == 6:
                worst6 = max(worst6, abs(np.dot(w5, mono) - exact))
        assert 1e-2 < worst6 < 1e-1


def restate(resid, lb, ub, reltol, abstol, max_regions=4096, max_rounds=32, u=U["f64"], check=True):
    """resid: points [n, d] (float64) -> residuals [n].  -> dict(c, h, share, I7, err: per box in the device's order; lo, hi [nb, d]; I, E, tau,
    status, rounds, depth [nb]; w7v, wv [nb]: share sum_j |w7_j| v_j and share sum_j (|w7_j| + |w5_j|) v_j of each box); asserts the edge distance of every comparison it makes (check = False: a timing run that compares nothing)"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    free = [i for i in range(lb.size) if ub[i] > lb[i]]
    nf = len(free)
    x, w7, w5 = gm_rule(nf)
    M = len(x)
    c, h = [0.5 * (lb[free] + ub[free])], [0.5 * (ub[free] - lb[free])]
    share, I7, err, axis, depth = [1.0], [0.0], [0.0], [0], [0]
    w7v, wv, gap, vmax = [0.0], [0.0], [np.inf], [0.0]      # per box: share sum |w7| v; share sum (|w7| + |w5|) v; D_(1) - D_(2); max v
    pending, rounds = [0], 0
    while True:
        pts = np.repeat(lb[None, :], len(pending) * M, axis=0)
        for p, b in enumerate(pending):
            pts[p * M:(p + 1) * M][:, free] = c[b][None, :] + h[b][None, :] * x
        v = np.asarray(resid(pts), dtype=np.float64).reshape(len(pending), M) ** 2
        for p, b in enumerate(pending):
            vb = v[p]
            i7, i5 = share[b] * np.dot(w7, vb), share[b] * np.dot(w5, vb)
            I7[b], err[b] = i7, abs(i7 - i5)
            w7v[b], wv[b], vmax[b] = share[b] * np.dot(np.abs(w7), vb), share[b] * np.dot(np.abs(w7) + np.abs(w5), vb), vb.max()
            D = np.array([abs((vb[1 + 2 * k] + vb[2 + 2 * k] - 2.0 * vb[0]) - (vb[1 + 2 * nf + 2 * k] + vb[2 + 2 * nf + 2 * k] - 2.0 * vb[0]) / 7.0)
                          for k in range(nf)])
            axis[b] = int(np.argmax(D))
            Ds = np.sort(D)
            gap[b] = (Ds[-1] - Ds[-2]) if nf > 1 else np.inf
        I, E = float(np.sum(I7)), float(np.sum(err))
        tau = max(abstol, reltol * abs(I))
        assert not check or abs(E - tau) >= 1e3 * u * sum(wv), f"E = {E} sits on the edge of tau = {tau}"
        nb = len(c)
        flags = [err[b] > tau * share[b] for b in range(nb)]
        for b in range(nb):
            assert not check or abs(err[b] - tau * share[b]) >= 1e3 * u * wv[b], f"box {b}: err = {err[b]} sits on the edge of its share of tau"
        nsplit = sum(flags)
        if E <= tau or nsplit == 0:
            status = 0
        elif nb + nsplit > max_regions:
            status = 1
        elif rounds >= max_rounds:
            status = 2
        else:
            status = -1
        if status >= 0:
            break
        s, pending = 0, []
        for b in range(nb):
            if not flags[b]:
                continue
            assert not check or gap[b] >= 1e3 * u * vmax[b], f"box {b}: its two largest fourth differences tie to rounding"
            a = axis[b]
            hh = 0.5 * h[b][a]
            cb, hb = c[b].copy(), h[b].copy()
            cb[a] += hh; hb[a] = hh
            c[b] = c[b].copy(); h[b] = h[b].copy()
            c[b][a] -= hh; h[b][a] = hh
            share[b] *= 0.5
            depth[b] += 1
            c.append(cb); h.append(hb); share.append(share[b]); I7.append(0.0); err.append(0.0); axis.append(0); depth.append(depth[b])
            w7v.append(0.0); wv.append(0.0); gap.append(np.inf); vmax.append(0.0)
            pending += [b, nb + s]
            s += 1
        rounds += 1
    c, h = np.array(c), np.array(h)
    lo, hi = np.repeat(lb[None, :], len(c), axis=0), np.repeat(ub[None, :], len(c), axis=0)
    lo[:, free], hi[:, free] = c - h, c + h
    return dict(c=c, h=h, share=np.array(share), I7=np.array(I7), err=np.array(err), lo=lo, hi=hi, I=I, E=E, tau=tau, status=status, rounds=rounds,
                depth=np.array(depth), free=free, w7v=np.array(w7v), wv=np.array(wv))


def emitted(boxes, lb, ub, G):
    """the composite Gauss-Legendre rule on `boxes` [nb, 2, d] as DESIGN §4.13 states it -> points [n, d] float64, weights [n] float64"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    free = [i for i in range(lb.size) if ub[i] > lb[i]]
    gx, gw = leggauss(G)
    gw = gw / 2.0
    nb, npl = len(boxes), G ** len(free)
    pts = np.repeat(lb[None, :], nb * npl, axis=0)
    w = np.zeros(nb * npl)
    for b in range(nb):
        lo, hi = boxes[b, 0, free], boxes[b, 1, free]
        c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
        sh = float(np.prod(h / (0.5 * (ub[free] - lb[free]))))
        q = np.arange(npl)
        wq = np.full(npl, sh)
        for k in range(len(free)):
            ik = (q // G ** k) % G
            pts[b * npl:(b + 1) * npl, free[k]] = c[k] + h[k] * gx[ik]
            wq = wq * gw[ik]
        w[b * npl:(b + 1) * npl] = wq
    return pts, w


def sort_rows(a):
    a = np.asarray(a).reshape(len(a), -1)
    return a[np.lexsort(a.T[::-1])]


# ------------------------------------------------------------------------------------------------------------------------------------
# problems
# ------------------------------------------------------------------------------------------------------------------------------------
def value_problem(npde, d, g, precision="f64"):
    """u(x0..) ~ g(x0..) on the unit cube with the boundary term u(0, x1..) ~ 0; theta = 0: the residual of term 0 is -g exactly"""
    xs = npde.parameters(" ".join(f"x{i}" for i in range(d)))
    (u,) = npde.variables("u")
    sysm = npde.PDESystem([npde.Eq(u(*xs), g(*xs))], [npde.Eq(u(0.0, *xs[1:]), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0)) for x in xs], list(xs), [u(*xs)])
    chain = npde.Chain(npde.Dense(d, 4, "tanh"), npde.Dense(4, 1))
    th = np.zeros(chain.nparams, dtype=np.float64)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.5), init_params=th, precision=precision))
    return rep, th, sysm, chain


def burgers_problem(npde, precision, seed=6):
    """(seed 6: of the seeds 1..12 the one whose restatement keeps the edge distance in both precisions — at 2^-24 the distance is a third of tau —
    and still refines unevenly: 7 boxes in float64 at reltol 1e-4, 5 on the fp32 kernels at 1e-3, depths 1..3)"""
    t, x = npde.parameters("t x")
    (u,) = npde.variables("u")
    Dt, Dx = npde.Differential(t), npde.Differential(x)
    eq = npde.Eq(Dt(u(t, x)) + u(t, x) * Dx(u(t, x)) - 0.05 * Dx(Dx(u(t, x))), 0)
    import sympy as sp
    bcs = [npde.Eq(u(0.0, x), -sp.sin(sp.pi * x)), npde.Eq(u(t, -1.0), 0.0), npde.Eq(u(t, 1.0), 0.0)]
    sysm = npde.PDESystem([eq], bcs, [npde.In(t, npde.Interval(0.0, 1.0)), npde.In(x, npde.Interval(-1.0, 1.0))], [t, x], [u(t, x)])
    chain = npde.Chain(npde.Dense(2, 8, "tanh"), npde.Dense(8, 8, "tanh"), npde.Dense(8, 1))
    th = npde.initialparameters(np.random.default_rng(seed), chain)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.25), init_params=th, precision=precision))
    return rep, np.asarray(th, dtype=np.float64), sysm, chain


def handle_resid(eng, term, theta, precision):
    def f(pts):
        if precision == "f64":
            eng.set_points_f64(term, pts.T)
            return eng.residual_f64(term, theta, len(pts))
        eng.set_points(term, pts.T.astype(np.float32))
        return eng.residual(term, theta.astype(np.float32), len(pts)).astype(np.float64)
    return f


def sp_():
    import sympy as sp
    return sp


INPUTS = {     # name -> (d, g, reltol, centre of the feature)
    "tanh1": (1, lambda x: sp_().tanh(20 * (x - 0.3)), 1e-6, (0.3,)),
    "bump1": (1, lambda x: sp_().exp(-((x - 0.3) / 0.05) ** 2), 1e-6, (0.3,)),
    "bump2": (2, lambda x, y: sp_().exp(-((x - 0.3) ** 2 + (y - 0.6) ** 2) / 0.1 ** 2), 1e-4, (0.3, 0.6)),
    "bump3": (3, lambda x, y, z: sp_().exp(-((x - 0.3) ** 2 + (y - 0.6) ** 2 + (z - 0.5) ** 2) / 0.2 ** 2), 1e-3, (0.3, 0.6, 0.5)),
    "bump4": (4, lambda x, y, z, s: sp_().exp(-(((x - 0.3) / 0.25) ** 2 + ((y - 0.6) / 0.35) ** 2 + ((z - 0.5) / 0.45) ** 2 + ((s - 0.4) / 0.6) ** 2)), 1e-2,
              (0.3, 0.6, 0.5, 0.4)),
}
ABSTOL = 1e-12


def check_parity(eng, term, out, ref, d, u):
    """the device's mesh and figures against the restatement's: boxes equal; integral to 64 u sum |w7| v, error to 64 u sum (|w7| + |w5|) v, over the boxes"""
    assert (out["status"], out["rounds"], out["nregions"]) == (ref["status"], ref["rounds"], len(ref["lo"]))
    boxes, est = eng.cubature_get(term, out["nregions"], d)
    assert np.array_equal(sort_rows(boxes), sort_rows(np.stack([ref["lo"], ref["hi"]], axis=1)))
    assert np.array_equal(boxes[:, 0], ref["lo"]) and np.array_equal(boxes[:, 1], ref["hi"])      # (the device's order is part of the statement)
    bar7, bar = 64 * u * ref["w7v"].sum(), 64 * u * ref["wv"].sum()      # only w7 enters the integral; both rules enter the error
    print(f"parity: integral {out['integral']!r} vs {ref['I']!r}, bar {bar7:.3e}; error {out['error']!r} vs {ref['E']!r}, bar {bar:.3e}")
    assert abs(out["integral"] - ref["I"]) <= bar7 and abs(out["error"] - ref["E"]) <= bar
    assert np.all(np.abs(est[:, 0] - ref["I7"]) <= 64 * u * ref["w7v"]) and np.all(np.abs(est[:, 1] - ref["err"]) <= 64 * u * ref["wv"])      # box by box
    return boxes


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. rule exactness
# ------------------------------------------------------------------------------------------------------------------------------------
POLYS = ("x0x1", "x0^3", "affine")


def body_rule(npde, n, poly):
    if poly == "x0x1" and n < 2:
        return
    g = {"x0x1": lambda *x: x[0] * x[1], "x0^3": lambda *x: x[0] ** 3, "affine": lambda *x: 1 + x[0] - 2 * x[n - 1]}[poly]
    exact = {"x0x1": 1.0 / 9.0, "x0^3": 1.0 / 7.0, "affine": (1.0 / 3.0 if n == 1 else 1.0 / 4.0 + 1.0 / 12.0 + 4.0 / 12.0)}[poly]      # mean of g^2 over the unit cube
    rep, th, _, _ = value_problem(npde, n, g)
    eng = rep.engine
    lb, ub = np.zeros(n), np.ones(n)
    # max_rounds = 0: one box.  (The restatement's own edge assertions are moot for a rule that is exact: err ~ 0 vs tau; they are skipped by
    # a tolerance no estimate can meet or miss: abstol = 1 for the exact rules; x0^3 (v of degree 6) has err > 0 and keeps abstol = 1e-12.)
    abstol = 1e-12 if poly == "x0^3" else 1.0
    ref = restate(handle_resid(eng, 0, th, "f64"), lb, ub, 1e-6, abstol, max_rounds=0)
    out = eng.cubature_refine(0, th, lb, ub, reltol=1e-6, abstol=abstol, max_rounds=0)
    bar = 64 * 2.0 ** -52 * ref["w7v"][0]                # 64 2^-52 sum |w7_j| v_j
    bar_err = 64 * 2.0 ** -52 * ref["wv"][0]             # (both rules enter the error)
    print(f"rule n={n} {poly}: integral {out['integral']!r} restatement {ref['I']!r} closed form {exact!r} bar {bar:.3e}; error {out['error']!r} vs {ref['E']!r}")
    assert out["nregions"] == 1 and out["rounds"] == 0
    assert abs(out["integral"] - ref["I"]) <= bar
    assert abs(ref["I"] - exact) <= bar
    if poly == "x0^3":
        assert out["status"] == 2 and out["error"] > 0 and abs(out["error"] - ref["E"]) <= bar_err
    else:
        assert out["status"] == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. tree parity, 3. accuracy against the oracle
# ------------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def oracle_integral(npde, name, tau):
    """dense tensor Gauss-Legendre over the oracle's float64 residuals (exact mode), the node count doubled until the value moves by < 1e-3 tau"""
    if name in _REF:
        return _REF[name]
    d, g = INPUTS[name][:2]
    _, th, sysm, chain = _problem_cache(npde, name)
    prob = helpers.oracle_problem(npde, sysm, [chain])
    m, prev = {1: 64, 2: 32, 3: 16, 4: 12}[d], None
    while True:
        x, w = leggauss(m)
        x, w = 0.5 * (x + 1.0), 0.5 * w
        grids = np.meshgrid(*([x] * d), indexing="ij")
        wts = np.meshgrid(*([w] * d), indexing="ij")
        pts = np.stack([q.reshape(-1) for q in grids])
        W = np.prod(np.stack([q.reshape(-1) for q in wts]), axis=0)
        val = float(np.dot(W, po.residual_values(prob, th, 0, pts, mode="exact").reshape(-1) ** 2))
        if prev is not None and abs(val - prev) < 1e-3 * tau:
            break
        prev, m = val, 2 * m
        assert m <= 2048
    _REF[name] = val
    return val


_PROB = {}


def _problem_cache(npde, name):
    """(the symbolic system of an input is built once for the oracle; every test makes its own handle)"""
    d, g = INPUTS[name][:2]
    if name not in _PROB:
        _PROB[name] = (None,) + value_problem(npde, d, g)[1:]      # (theta, system, chain: the handle is not kept)
    return _PROB[name]


def body_tree(npde, name):
    d, g, reltol, centre = INPUTS[name]
    rep, th, _, _ = value_problem(npde, d, g)
    eng = rep.engine
    lb, ub = np.zeros(d), np.ones(d)
    ref = restate(handle_resid(eng, 0, th, "f64"), lb, ub, reltol, ABSTOL)
    out = eng.cubature_refine(0, th, lb, ub, reltol=reltol, abstol=ABSTOL)
    print(f"{name}: {out}")
    check_parity(eng, 0, out, ref, d, U["f64"])
    assert out["status"] == 0
    # the mesh is local: the deepest leaf contains the feature's centre
    deepest = np.flatnonzero(ref["depth"] == ref["depth"].max())
    assert ref["depth"].min() < ref["depth"].max()
    assert any(np.all(ref["lo"][b] <= np.array(centre)) and np.all(np.array(centre) <= ref["hi"][b]) for b in deepest)
    # 3. accuracy: the returned integral and the installed loss against the independent reference
    tau = max(ABSTOL, reltol * out["integral"])
    I_ref = oracle_integral(npde, name, tau)
    tol = max(ABSTOL, reltol * I_ref)
    installed = eng.loss_grad_f64(th, want_grad=False)[0][0]
    print(f"{name}: I_ref {I_ref!r}; |integral - I_ref| = {abs(out['integral'] - I_ref):.3e}, |installed - I_ref| = {abs(installed - I_ref):.3e}, tolerance {tol:.3e}; "
          f"{out['nregions']} leaves, {out['npoints']} points, {out['rounds']} rounds, error estimate {out['error']:.3e}")
    assert abs(out["integral"] - I_ref) <= tol
    assert abs(installed - I_ref) <= tol


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the installed set is an ordinary set (Burgers, both precisions)
# ------------------------------------------------------------------------------------------------------------------------------------
BURGERS_LB, BURGERS_UB = np.array([0.0, -1.0]), np.array([1.0, 1.0])


def body_installed(npde, precision):
    f64 = precision == "f64"
    reltol = 1e-4 if f64 else 1e-3
    rep, th, _, _ = burgers_problem(npde, precision)
    eng = rep.engine
    ref = restate(handle_resid(eng, 0, th, precision), BURGERS_LB, BURGERS_UB, reltol, ABSTOL, u=U[precision])
    out = eng.cubature_refine(0, th, BURGERS_LB, BURGERS_UB, reltol=reltol, abstol=ABSTOL)
    print(f"burgers {precision}: {out}")
    boxes = check_parity(eng, 0, out, ref, 2, U[precision])
    pts, w = emitted(boxes, BURGERS_LB, BURGERS_UB, 4)
    n = out["npoints"]
    assert n == len(pts) == 16 * out["nregions"]
    assert np.array_equal(eng.get_points(0, 2, n), pts.T.astype(np.float32))
    assert abs(float(np.sum(w.astype(np.float32).astype(np.float64))) - 1.0) <= n * 2.0 ** -24
    fresh, _, _, _ = burgers_problem(npde, precision)
    if f64:
        fresh.engine.set_points_f64(0, pts.T, n)
    else:
        fresh.engine.set_points(0, pts.T.astype(np.float32), n)
    fresh.engine.set_point_weights(0, w.astype(np.float32))
    thx = th if f64 else th.astype(np.float32)
    for fn in ("loss_grad_f64", "term_grads_f64") if f64 else ("loss_grad", "term_grads"):
        a, b = getattr(eng, fn)(thx), getattr(fresh.engine, fn)(thx)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), fn


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. fixed coordinates
# ------------------------------------------------------------------------------------------------------------------------------------
def body_fixed(npde, precision):
    """u(t, -1) ~ 0 (x fixed, t free) and u(0, x) ~ -sin(pi x) (t fixed, x free: the free axis is not coordinate 0)"""
    rep, th, _, _ = burgers_problem(npde, precision)
    eng = rep.engine
    reltol = 1e-6 if precision == "f64" else 1e-3
    for term, lb, ub, fixed_row, value in ((2, np.array([0.0, -1.0]), np.array([1.0, -1.0]), 1, -1.0), (1, np.array([0.0, -1.0]), np.array([0.0, 1.0]), 0, 0.0)):
        ref = restate(handle_resid(eng, term, th, precision), lb, ub, reltol, ABSTOL, u=U[precision])
        out = eng.cubature_refine(term, th, lb, ub, reltol=reltol, abstol=ABSTOL)
        print(f"fixed {precision} term {term}: {out}")
        boxes = check_parity(eng, term, out, ref, 2, U[precision])
        assert out["npoints"] == 4 * out["nregions"]
        if term == 1 and precision == "f64":
            assert out["nregions"] > 1
        got = eng.get_points(term, 2, out["npoints"])
        assert np.all(got[fixed_row] == value) and np.all((got[1 - fixed_row] > lb[1 - fixed_row]) & (got[1 - fixed_row] < ub[1 - fixed_row]))
        pts, w = emitted(boxes, lb, ub, 4)
        assert np.array_equal(got, pts.T.astype(np.float32))
        assert abs(float(np.sum(w.astype(np.float32).astype(np.float64))) - 1.0) <= out["npoints"] * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. sizes that cross the kernels' strides
# ------------------------------------------------------------------------------------------------------------------------------------
def body_sizes(npde, max_regions, nodes):
    d, g = INPUTS["bump2"][:2]
    rep, th, _, _ = value_problem(npde, d, g)
    eng = rep.engine
    lb, ub = np.zeros(2), np.ones(2)
    ref = restate(handle_resid(eng, 0, th, "f64"), lb, ub, 1e-7, ABSTOL, max_regions=max_regions)
    out = eng.cubature_refine(0, th, lb, ub, reltol=1e-7, abstol=ABSTOL, max_regions=max_regions, nodes=nodes)
    print(f"sizes max_regions={max_regions}: {out}")
    boxes = check_parity(eng, 0, out, ref, 2, U["f64"])
    assert out["status"] == 1 and out["nregions"] <= max_regions
    if max_regions == 300:
        assert out["nregions"] > 256                     # k_cub_plan's second stride
    assert float(np.sum(np.prod(boxes[:, 1] - boxes[:, 0], axis=1))) == 1.0
    pts, w = emitted(boxes, lb, ub, nodes)
    assert out["npoints"] == nodes ** 2 * out["nregions"]
    assert np.array_equal(eng.get_points(0, 2, out["npoints"]), pts.T.astype(np.float32))
    assert abs(float(np.sum(w.astype(np.float32).astype(np.float64))) - 1.0) <= out["npoints"] * 2.0 ** -24


def body_leaf_81(npde):
    """nodes = 3 on 4 free axes: 81 points per leaf, not a multiple of a wave"""
    d, g, reltol, _ = INPUTS["bump4"]
    rep, th, _, _ = value_problem(npde, d, g)
    eng = rep.engine
    lb, ub = np.zeros(4), np.ones(4)
    out = eng.cubature_refine(0, th, lb, ub, reltol=reltol, abstol=ABSTOL, nodes=3)
    boxes, _ = eng.cubature_get(0, out["nregions"], 4)
    pts, w = emitted(boxes, lb, ub, 3)
    assert out["npoints"] == 81 * out["nregions"] and out["nregions"] > 1
    assert np.array_equal(eng.get_points(0, 4, out["npoints"]), pts.T.astype(np.float32))
    fresh, _, _, _ = value_problem(npde, d, g)
    fresh.engine.set_points_f64(0, pts.T, len(pts))
    fresh.engine.set_point_weights(0, w.astype(np.float32))
    a, b = eng.loss_grad_f64(th), fresh.engine.loss_grad_f64(th)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. history, 8. refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def body_history(npde, precision):
    f64 = precision == "f64"
    ev = (lambda e, t: e.loss_grad_f64(t)) if f64 else (lambda e, t: e.loss_grad(t.astype(np.float32)))
    rep, th, _, _ = burgers_problem(npde, precision)
    th2 = np.asarray(npde.initialparameters(np.random.default_rng(11), npde.Chain(npde.Dense(2, 8, "tanh"), npde.Dense(8, 8, "tanh"), npde.Dense(8, 1))), dtype=np.float64)
    kw = dict(reltol=1e-3, abstol=ABSTOL)
    eng = rep.engine
    o1 = eng.cubature_refine(0, th, BURGERS_LB, BURGERS_UB, **kw)
    ev(eng, th)
    o2 = eng.cubature_refine(0, th2, BURGERS_LB, BURGERS_UB, **kw)
    a = ev(eng, th2)
    fresh, _, _, _ = burgers_problem(npde, precision)
    o3 = fresh.engine.cubature_refine(0, th2, BURGERS_LB, BURGERS_UB, **kw)
    b = ev(fresh.engine, th2)
    assert o2 == o3 and (o1["nregions"], o1["integral"]) != (o2["nregions"], o2["integral"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # refine -> set_points of a plain grid -> evaluate == a handle that never refined
    grid = rep.pde_train_sets[0]
    (eng.set_points_f64 if f64 else eng.set_points)(0, grid)
    never, _, _, _ = burgers_problem(npde, precision)
    a, b = ev(eng, th), ev(never.engine, th)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def refused(npde, eng, ev, msg, **args):
    """the call is refused by message and the handle evaluates as before"""
    before = ev()
    with pytest.raises(npde.EngineError, match=msg):
        eng.cubature_refine(**args)
    after = ev()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), msg


def evaluator(eng, th, precision):
    return (lambda: eng.loss_grad_f64(th)) if precision == "f64" else (lambda: eng.loss_grad(th.astype(np.float32)))


def body_refusals(npde, precision):
    rep, th, _, _ = burgers_problem(npde, precision)
    eng = rep.engine
    ev = evaluator(eng, th, precision)
    lb, ub = BURGERS_LB, BURGERS_UB
    cases = [
        (dict(lb=ub, ub=lb), "lb > ub"),
        (dict(lb=lb[:1], ub=ub[:1]), "coordinates"),
        (dict(lb=lb, ub=lb), "zero free axes"),
        (dict(nodes=0), "nodes"), (dict(nodes=9), "nodes"),
        (dict(reltol=-1.0), "negative tolerance"), (dict(abstol=-1.0), "negative tolerance"),
        (dict(max_regions=0), "max_regions"),
        (dict(term=7), "term index"),
        (dict(theta=th[:-1]), "theta length"),
    ]
    for kw, msg in cases:
        args = dict(term=0, theta=th, lb=lb, ub=ub)
        args.update(kw)
        refused(npde, eng, ev, msg, **args)
    with pytest.raises(npde.EngineError, match="no region list"):
        eng.cubature_get(0, 1, 2)
    # a handle in a communicator
    eng.comm_init_custom(1, 0, lambda buf, count, dtype, stream: 0)
    refused(npde, eng, ev, "communicator", term=0, theta=th, lb=lb, ub=ub)
    eng.comm_destroy()
    assert eng.cubature_refine(0, th, lb, ub, reltol=1e-3, abstol=ABSTOL)["status"] == 0      # (the same call is taken once the communicator is gone)
    if precision == "f32":                               # a term with a device sampler (fp32 handles have them)
        eng.set_sampler(0, lb, ub, 64, seed=1, kind=1)
        refused(npde, eng, ev, "sampler", term=0, theta=th, lb=lb, ub=ub)


def body_refusal_kinds(npde):
    """terms and shapes the refinement does not cover: per-point data channels, integral terms; why more than 4 free axes cannot be asked for"""
    sp = sp_()
    # a DataLoss term: per-point data channels
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    sysm = npde.PDESystem([npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.sin(sp.pi * x), 0)], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)],
                          [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 8, "tanh"), npde.Dense(8, 1))
    th = np.asarray(npde.initialparameters(np.random.default_rng(2), chain), dtype=np.float64)
    xs = np.linspace(0.05, 0.95, 7)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=th, precision="f32",
                                                                  data_loss=[npde.DataLoss(u(x), xs[None, :], np.sin(np.pi * xs))]))
    eng = rep.engine
    refused(npde, eng, evaluator(eng, th, "f32"), "per-point data", term=eng.K - 1, theta=th, lb=[0.0], ub=[1.0])
    # an integral term (the reference's integro-differential example; fp32: the float64 mode has no integral terms)
    (t,) = npde.parameters("t")
    (i,) = npde.variables("i")
    Ii = npde.Integral(npde.In(t, npde.Interval(0.0, t)))
    sysm = npde.PDESystem([npde.Eq(npde.Differential(t)(i(t)) + 2 * i(t) + 5 * Ii(i(t)), 1)], [npde.Eq(i(0.0), 0.0)], [npde.In(t, npde.Interval(0.0, 2.0))], [t], [i(t)])
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.25), init_params=th, precision="f32"))
    eng = rep.engine
    refused(npde, eng, evaluator(eng, th, "f32"), "integral terms", term=0, theta=th, lb=[0.0], ub=[2.0])
    # more than 4 free axes cannot be stated: the engine takes no term with more than 4 coordinates (its own refusal, at pinn_create), and d must
    # equal the term's coordinates; all 4 free and 3 of 4 free are cases 1 / 2 and below
    with pytest.raises(npde.EngineError, match="more than 4 coordinates"):
        value_problem(npde, 5, lambda *x: x[0] + x[4], "f32")
    rep, th4, _, _ = value_problem(npde, 4, lambda *x: x[0] + x[3], "f32")
    eng = rep.engine
    refused(npde, eng, evaluator(eng, th4, "f32"), "coordinates", term=0, theta=th4, lb=np.zeros(5), ub=np.ones(5))
    out = eng.cubature_refine(0, th4, np.zeros(4), np.array([1.0, 1.0, 0.0, 1.0]), reltol=1e-3, abstol=ABSTOL, max_rounds=0)
    assert out["nregions"] == 1 and out["npoints"] == 64 and np.all(eng.get_points(0, 4, 64)[2] == 0.0)


def body_nonfinite(npde, precision):
    """a theta at which the residual is not finite (an infinite output bias; term 1 is u(0, x) + sin(pi x)): status 3, not 'converged' with a NaN
    estimate; a complete partition is still installed, and the next call at a sane theta is unaffected"""
    rep, th, _, _ = burgers_problem(npde, precision)
    lb, ub = np.array([0.0, -1.0]), np.array([0.0, 1.0])
    bad = th.copy()
    bad[-1] = np.inf
    out = rep.engine.cubature_refine(1, bad, lb, ub, reltol=1e-3, abstol=ABSTOL)
    print(f"nonfinite {precision}: {out}")
    assert out["status"] == 3 and not np.isfinite(out["integral"]) and (out["nregions"], out["npoints"], out["rounds"]) == (1, 4, 0)
    assert rep.engine.cubature_refine(1, th, lb, ub, reltol=1e-3, abstol=ABSTOL)["status"] == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 9. the mirror
# ------------------------------------------------------------------------------------------------------------------------------------
def poisson_bump(npde, strategy, seed=5):
    sp = sp_()
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))), sp.exp(-((x - 0.3) / 0.05) ** 2))
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 8, "tanh"), npde.Dense(8, 1))
    th = npde.initialparameters(np.random.default_rng(seed), chain)
    disc = npde.PhysicsInformedNN(chain, strategy, init_params=th, precision="f64")
    return sysm, chain, disc, np.asarray(th, dtype=np.float64)


# QuadratureTraining() / QuadratureTraining(nodes = 6) on poisson_bump, float64 mode, as the parent commit computes them:
# (points of term 0, first and last point, first weight, loss of term 0 at the initial parameters)
PINNED = {None: (32, 0.001368069075259215, 0.9986319309247408, 0.003509305004734649, 0.050978382844777126),
          6: (6, 0.033765242898423975, 0.966234757101576, 0.08566224618958487, 0.00792145343893958)}


# the fixed rule's whole sets and weights of term 0 (32 and 6 values each), as the parent commit produces them
PINNED_POINTS_DEFAULT = np.array([
    0.001368069075259215, 0.007194244227365809, 0.017618872206246805, 0.03254696203113017, 0.0518394221169739, 0.07531619313371501,
    0.10275810201602881, 0.13390894062985514, 0.16847786653489238, 0.20614212137961885, 0.24655004553388532, 0.28932436193468236,
    0.33406569885893617, 0.38035631887393145, 0.42776401920860174, 0.4758461671561308, 0.5241538328438692, 0.5722359807913983,
    0.6196436811260685, 0.6659343011410639, 0.7106756380653176, 0.7534499544661146, 0.7938578786203812, 0.8315221334651076,
    0.8660910593701449, 0.8972418979839711, 0.924683806866285, 0.9481605778830261, 0.9674530379688698, 0.9823811277937532,
    0.9928057557726342, 0.9986319309247408,
])
PINNED_WEIGHTS_DEFAULT = np.array([
    0.003509305004734649, 0.008137197365452983, 0.012696032654631213, 0.017136931456510813, 0.021417949011113213, 0.025499029631188122,
    0.029342046739267852, 0.032911111388180876, 0.036172897054424225, 0.039096947893535156, 0.04165596211347342, 0.043826046502201954,
    0.04558693934788193, 0.04692219954040228, 0.04781936003963742, 0.048270044257363906, 0.048270044257363906, 0.04781936003963742,
    0.04692219954040228, 0.04558693934788193, 0.043826046502201954, 0.04165596211347342, 0.039096947893535156, 0.036172897054424225,
    0.032911111388180876, 0.029342046739267852, 0.025499029631188122, 0.021417949011113213, 0.017136931456510813, 0.012696032654631213,
    0.008137197365452983, 0.003509305004734649,
])
PINNED_POINTS_NODES6 = np.array([
    0.033765242898423975, 0.16939530676686776, 0.3806904069584015, 0.6193095930415985, 0.8306046932331322, 0.966234757101576,
])
PINNED_WEIGHTS_NODES6 = np.array([
    0.08566224618958487, 0.18038078652406947, 0.23395696728634569, 0.23395696728634569, 0.18038078652406947, 0.08566224618958487,
])


def body_mirror_fixed(npde, nodes):
    strat = npde.QuadratureTraining() if nodes is None else npde.QuadratureTraining(nodes=nodes)
    sysm, chain, disc, th = poisson_bump(npde, strat)
    rep = npde.symbolic_discretize(sysm, disc)
    s, w = rep.pde_train_sets[0], strat.point_weights()[0]
    loss = rep.engine.loss_grad_f64(th, want_grad=False)[0][0]
    print(f"mirror fixed nodes={nodes}: ({s.shape[1]}, {s[0, 0]!r}, {s[0, -1]!r}, {w[0]!r}, {loss!r})")
    n, p0, p1, w0, l0 = PINNED[nodes]
    assert s.shape == (1, n) and s[0, 0] == p0 and s[0, -1] == p1 and w[0] == w0
    assert np.array_equal(s[0], PINNED_POINTS_DEFAULT if nodes is None else PINNED_POINTS_NODES6)
    assert np.array_equal(w, PINNED_WEIGHTS_DEFAULT if nodes is None else PINNED_WEIGHTS_NODES6)
    for k in (1, 2):                                     # the two point conditions: one point, weight 1
        assert rep.bcs_train_sets[k - 1].shape == (1, 1) and np.array_equal(strat.point_weights()[k], [1.0])
    assert abs(loss - l0) <= 1e-11 * l0                  # (the float64 mode's agreement between builds: to rounding)
    assert rep.cubature == {} and rep._refine is None


def body_mirror_adaptive(npde):
    strat = npde.QuadratureTraining(adaptive=True, reltol=1e-4, abstol=ABSTOL, refresh=25)
    sysm, chain, disc, th = poisson_bump(npde, strat)
    prob = npde.discretize(sysm, disc)
    rep = prob.pinnrep
    assert rep._state["refines"] == 1 and set(rep.cubature) == {0}      # (the two point conditions have no free axis)
    res = npde.solve(prob, npde.Adam(0.01), maxiters=100)
    assert rep._state["refines"] == 1 + 4
    # "decreasing" is asked of the run as a whole: the objective changes at every re-mesh (steps 25, 50, 75), where the history may step up
    assert np.all(np.isfinite(res.losses)) and res.losses[-1] < res.losses[0]
    last = rep.cubature[0]
    print(f"mirror adaptive: {last}; losses {res.losses[0]!r} -> {res.losses[-1]!r}")
    assert last["status"] in (0, 1, 2) and last["npoints"] == 4 * last["nregions"]
    # at the final theta: the installed loss against the dense oracle reference
    theta = np.asarray(res.u, dtype=np.float64)
    oprob = helpers.oracle_problem(npde, sysm, [chain])
    m, prev = 128, None
    while True:
        x, w = leggauss(m)
        val = float(np.dot(0.5 * w, po.residual_values(oprob, theta, 0, (0.5 * (x + 1.0))[None, :], mode="exact").reshape(-1) ** 2))
        if prev is not None and abs(val - prev) < 1e-3 * max(ABSTOL, 1e-4 * val):
            break
        prev, m = val, 2 * m
    installed = rep.engine.loss_grad_f64(theta, want_grad=False)[0][0]
    tol = max(ABSTOL, 1e-4 * val)
    print(f"mirror adaptive: installed {installed!r} reference {val!r} tolerance {tol:.3e} status {last['status']}")
    assert last["status"] == 0 and abs(installed - val) <= tol


# ------------------------------------------------------------------------------------------------------------------------------------
# the two expositions
# ------------------------------------------------------------------------------------------------------------------------------------
RULE = [(n, p) for n in (1, 2, 3, 4) for p in POLYS if not (p == "x0x1" and n < 2)]
PRECISIONS = ("f64", "f32")
SIZES = [(300, 4), (64, 8), (65, 4)]


@pytest.mark.parametrize("n,poly", RULE)
def test_rule(npde, use_emu, n, poly):
    body_rule(npde, n, poly)


@pytest.mark.gpu
@pytest.mark.parametrize("n,poly", RULE)
def test_rule_gpu(npde, hip_lib, n, poly):
    body_rule(npde, n, poly)


@pytest.mark.parametrize("name", list(INPUTS))
def test_tree_and_accuracy(npde, use_emu, name):
    body_tree(npde, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(INPUTS))
def test_tree_and_accuracy_gpu(npde, hip_lib, name):
    body_tree(npde, name)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_installed_set(npde, use_emu, precision):
    body_installed(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_installed_set_gpu(npde, hip_lib, precision):
    body_installed(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fixed_coordinate(npde, use_emu, precision):
    body_fixed(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_fixed_coordinate_gpu(npde, hip_lib, precision):
    body_fixed(npde, precision)


@pytest.mark.parametrize("max_regions,nodes", SIZES)
def test_sizes(npde, use_emu, max_regions, nodes):
    body_sizes(npde, max_regions, nodes)


@pytest.mark.gpu
@pytest.mark.parametrize("max_regions,nodes", SIZES)
def test_sizes_gpu(npde, hip_lib, max_regions, nodes):
    body_sizes(npde, max_regions, nodes)


def test_leaf_81(npde, use_emu):
    body_leaf_81(npde)


@pytest.mark.gpu
def test_leaf_81_gpu(npde, hip_lib):
    body_leaf_81(npde)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_history(npde, use_emu, precision):
    body_history(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_history_gpu(npde, hip_lib, precision):
    body_history(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(npde, use_emu, precision):
    body_refusals(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_gpu(npde, hip_lib, precision):
    body_refusals(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_nonfinite(npde, use_emu, precision):
    body_nonfinite(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nonfinite_gpu(npde, hip_lib, precision):
    body_nonfinite(npde, precision)


def test_refusal_kinds(npde, use_emu):
    body_refusal_kinds(npde)


@pytest.mark.gpu
def test_refusal_kinds_gpu(npde, hip_lib):
    body_refusal_kinds(npde)


@pytest.mark.parametrize("nodes", (None, 6))
def test_mirror_fixed(npde, use_emu, nodes):
    body_mirror_fixed(npde, nodes)


@pytest.mark.gpu
@pytest.mark.parametrize("nodes", (None, 6))
def test_mirror_fixed_gpu(npde, hip_lib, nodes):
    body_mirror_fixed(npde, nodes)


def test_mirror_adaptive(npde, use_emu):
    body_mirror_adaptive(npde)


@pytest.mark.gpu
def test_mirror_adaptive_gpu(npde, hip_lib):
    body_mirror_adaptive(npde)
