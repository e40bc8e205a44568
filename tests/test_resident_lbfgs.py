"""Resident L-BFGS (`pinn_lbfgs_init / _steps / _get`): pinn_lbfgs's iteration with the iterate, the curvature rings and the
line search on the device.

The reference throughout is `restate` below: a numpy restatement of the slot algorithm of csrc/lbfgs_kernels.hpp (full evaluations only),
driven by the SAME handle's `loss_grad_f64` in float64 mode and by `loss_grad` at float32(x) otherwise — never the code under test, and not
`pinn_lbfgs`.

Every body is written once as a function of `npde` and exposed twice: on the CPU through the g++ emulation (`use_emu`) and, marked `gpu`,
on the product library (`hip_lib`).

Problems (those of tests/test_resident_hmc.py, the smallest that cross the kernel's boundaries), both on GridTraining(0.1) with Dense
1 -> 16 -> 16 -> 1 tanh: the 1-D Poisson problem, P = 321 = one 256-stride pass of the workgroup plus a partial one; the inverse problem with
one estimated parameter and one DataLoss term, P = 322, K = 4.  Both precisions.

THE BAR.  Device and restatement differ only in the order of the dot-product sums; L-BFGS amplifies such differences from one iteration to
the next.  The restatement's own sensitivity is measured by running it twice, its dots in forward and in reversed order: s = the largest
max-norm relative difference over the iterates, loss_history and the final gradient.  bar = min(1e-6, 100 * max(s, q)) with the resolution
floor q = 2^-52 * (number of iterations); the margin of 100 is §4.7's.  The two restatement runs must take the same sequence of accept /
reject / push / skip / restart decisions (asserted).  Measured figures: profiles/resident_lbfgs.txt.

The gradient-sign restart branch (not g.d < 0 -> steepest descent with cleared rings) needs curvature pairs that pass the s.y > 0 test and
still give an ascent direction, which exact arithmetic excludes (the two-loop matrix of pairs with s.y > 0 is positive definite).  Through the
public interface it is reached only with a non-finite g.d (the second weight set of the non-finite case); no back door was added."""
import ctypes as C

import numpy as np
import pytest

from test_resident_hmc import forward_problem, inverse_problem, relerr, NN_PRIOR

EPS64 = 2.0 ** -52
PRECISIONS = ("f64", "f32")
PROBLEMS = ("poisson", "inverse")


def problem(npde, name, precision):
    """-> (representation, theta0)"""
    rep, th0 = (forward_problem(npde, precision) if name == "poisson" else inverse_problem(npde, precision, "normal"))[:2]
    return rep, th0


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement; `rev`: dot products in reversed order
# ------------------------------------------------------------------------------------------------------------------------------------
def restate(eng, precision, th0, w, history, maxiters, gtol=1e-8, rev=False):
    """-> dict(xs = iterate after every iteration, hist, x, f, g, evals, status, log = (rejected trials, pushed, restarted) per iteration,
    nonfinite = trials whose objective was not finite)"""
    dot = (lambda a, b: float(np.sum((a * b)[::-1]))) if rev else (lambda a, b: float(np.sum(a * b)))
    wd = np.ones(eng.K) if w is None else np.asarray(w, dtype=np.float32).astype(np.float64)

    def ev(x):
        if precision == "f64":
            L, g = eng.loss_grad_f64(x, w)
        else:
            L, g = eng.loss_grad(x.astype(np.float32), w)
        f = 0.0
        for k in range(eng.K):
            f += wd[k] * L[k]
        return f, g.astype(np.float64)

    x = np.asarray(th0, dtype=np.float64).copy()
    with np.errstate(all="ignore"):
        f, g = ev(x)
        S, Y, RHO, xs, hist, log = [], [], [], [], [], []
        evals, nonfinite, status = 0, 0, "MAXITER"
        for it in range(maxiters):
            if not (np.fmax.reduce(np.abs(g), initial=0.0) > gtol):          # (fmax: a NaN entry is skipped, as std::max skips it)
                status = "CONVERGED"
                break
            q = g.copy()
            alpha = [0.0] * len(S)
            for i in reversed(range(len(S))):
                alpha[i] = RHO[i] * dot(S[i], q)
                q = q - alpha[i] * Y[i]
            gamma = dot(S[-1], Y[-1]) / dot(Y[-1], Y[-1]) if S else 1.0
            q = q * gamma
            for i in range(len(S)):
                beta = RHO[i] * dot(Y[i], q)
                q = q + (alpha[i] - beta) * S[i]
            d = -q
            gd = dot(g, d)
            restart = False
            if not (gd < 0.0):
                S, Y, RHO, restart = [], [], [], True
                d = -g
                gd = dot(g, d)
            t = 1.0
            if not S:
                r = 1.0 / np.sqrt(dot(g, g))
                t = r if r < 1.0 else 1.0
            ok, rejects = False, 0
            for ls in range(30):
                xn = x + t * d
                fn, gn = ev(xn)
                evals += 1
                nonfinite += not np.isfinite(fn)
                if np.isfinite(fn) and fn <= f + 1e-4 * t * gd:
                    ok = True
                    break
                t *= 0.5
                rejects += 1
            if not ok:
                status = "STALLED"
                log.append((rejects, False, restart))
                break
            s, y = xn - x, gn - g
            sy = dot(s, y)
            push = bool(sy > 1e-10 * np.sqrt(dot(s, s) * dot(y, y)))
            if push:
                S.append(s); Y.append(y); RHO.append(1.0 / sy)
                if len(S) > history:
                    S.pop(0); Y.pop(0); RHO.pop(0)
            x, g, f = xn, gn, fn
            hist.append(f); xs.append(x.copy()); log.append((rejects, push, restart))
    return dict(xs=np.asarray(xs), hist=np.asarray(hist), x=x, f=f, g=g, evals=evals, status=status, log=log, nonfinite=nonfinite)


def compare(got, ref):
    """largest max-norm relative error over every iterate, loss_history and the final gradient"""
    assert got["xs"].shape == ref["xs"].shape and got["hist"].shape == ref["hist"].shape, (got["xs"].shape, ref["xs"].shape)
    errs = [relerr(a, b) for a, b in zip(got["xs"], ref["xs"])] + [relerr(got["g"], ref["g"])]
    if len(ref["hist"]):
        errs.append(relerr(got["hist"], ref["hist"]))
    return max(errs)


def bar_of(eng, precision, th0, w, history, maxiters, gtol=1e-8):
    fwd = restate(eng, precision, th0, w, history, maxiters, gtol)
    bwd = restate(eng, precision, th0, w, history, maxiters, gtol, rev=True)
    assert fwd["log"] == bwd["log"] and fwd["status"] == bwd["status"], (fwd["log"], bwd["log"])     # the same decisions, or the case is on an edge
    sens = compare(bwd, fwd)
    return fwd, sens, min(1e-6, 100.0 * max(sens, EPS64 * max(len(fwd["hist"]), 1)))


def device_run(eng, th0, w, history, maxiters, gtol=1e-8, per_iteration=True):
    """the resident loop: one call of `maxiters` iterations and (per_iteration) the same again one iteration per call for the iterates, which
    must end on the same bits"""
    eng.lbfgs_init(th0, w, history=history)
    hist, evals, status = eng.lbfgs_steps(maxiters, gtol=gtol)
    x, f, g = eng.lbfgs_get()
    out = dict(hist=hist, evals=evals, status=status, x=x, f=f, g=g, xs=None)
    if per_iteration:
        eng.lbfgs_init(th0, w, history=history)
        xs = []
        for _ in range(len(hist)):
            h1, _, _ = eng.lbfgs_steps(1, gtol=gtol)
            assert len(h1) == 1
            xs.append(eng.lbfgs_get()[0])
        out["xs"] = np.asarray(xs).reshape(len(hist), eng.P)
        assert len(hist) == 0 or np.array_equal(out["xs"][-1], x)
    return out


# start / weights of the backtracking case (looked at on the CPU emulation: the restatement rejects trials in at least two iterations)
BACKTRACK = dict(scale=1.0, weights=[10.0, 1.0, 1.0])       # rejected trials per iteration there: 0, 0, 1, 9, 0, 1, 0, 0


def backtrack_setup(npde, precision):
    rep, th0 = problem(npde, "poisson", precision)
    return rep, BACKTRACK["scale"] * th0, BACKTRACK["weights"]


# ------------------------------------------------------------------------------------------------------------------------------------
# bodies
# ------------------------------------------------------------------------------------------------------------------------------------
def body_parity(npde, name, precision, history):
    """case 1: history = 2 over 6 iterations (the ring wraps and evicts), history = 10 (it never fills)"""
    rep, th0 = problem(npde, name, precision)
    eng = rep.engine
    ref, sens, bar = bar_of(eng, precision, th0, None, history, 6)
    got = device_run(eng, th0, None, history, 6)
    err = compare(got, ref)
    print(f"resident lbfgs parity [{name} {precision} m={history}]: err {err:.3e}  sensitivity {sens:.3e}  bar {bar:.3e}  log {ref['log']}")
    assert len(ref["hist"]) == 6 and sum(p for _, p, _ in ref["log"]) > history or history == 10
    assert got["status"] == ref["status"] == "MAXITER" and got["evals"] == ref["evals"]
    assert err <= bar
    assert relerr(got["f"], ref["f"]) <= bar and "lbfgs=resident(history=%d" % history in eng.describe()


def body_backtracking(npde, precision):
    """case 2: a start from which the restatement rejects at least one trial in at least two different iterations"""
    rep, th0, w = backtrack_setup(npde, precision)
    eng = rep.engine
    ref, sens, bar = bar_of(eng, precision, th0, w, 5, 8)
    print(f"resident lbfgs backtracking [{precision}]: sensitivity {sens:.3e}  bar {bar:.3e}  log {ref['log']}")
    assert sum(r > 0 for r, _, _ in ref["log"]) >= 2, ref["log"]
    got = device_run(eng, th0, w, 5, 8)
    err = compare(got, ref)
    print(f"resident lbfgs backtracking [{precision}]: err {err:.3e}  evals {got['evals']}")
    assert got["evals"] == ref["evals"] and got["status"] == ref["status"]
    assert err <= bar


def state_of(eng):
    return list(eng.lbfgs_get())


def body_chunking(npde, precision):
    """case 3: lbfgs_chunk = 1, 3, 8; steps(2) + steps(3) against steps(5); a chunk boundary on a RETRY slot (backtracking case, chunk 1)"""
    outs = []
    for chunk, split in ((8, (5,)), (1, (5,)), (3, (5,)), (8, (2, 3)), (3, (2, 3))):
        rep, th0 = problem(npde, "poisson", precision)
        eng = rep.engine
        eng.set_option("lbfgs_chunk", str(chunk))
        assert eng.get_option("lbfgs_chunk") == str(chunk)
        eng.lbfgs_init(th0, None, history=2)
        parts = [eng.lbfgs_steps(n) for n in split]
        outs.append([np.concatenate([q[0] for q in parts]), sum(q[1] for q in parts)] + state_of(eng))
    assert len(outs[0][0]) == 5
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    outs = []
    for chunk in (8, 1):
        rep, th0, w = backtrack_setup(npde, precision)
        eng = rep.engine
        eng.set_option("lbfgs_chunk", str(chunk))
        eng.lbfgs_init(th0, w, history=5)
        hist, evals, status = eng.lbfgs_steps(8)
        outs.append([hist, evals] + state_of(eng))
    assert outs[0][1] > 8                                   # (there were rejected trials: with chunk 1 every RETRY slot ended a chunk)
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))


def body_termination(npde, precision):
    """case 4: gtol above the initial gmax; max_evals smaller than needed, then continued; maxiters reached exactly with a padded history"""
    rep, th0, w = backtrack_setup(npde, precision)
    eng = rep.engine
    L, dp, ip = eng.L, C.POINTER(C.c_double), C.POINTER(C.c_int)
    eng.lbfgs_init(th0, w, history=5)
    x0, f0, g0 = eng.lbfgs_get()
    assert np.array_equal(x0, th0)
    hist, evals, status = eng.lbfgs_steps(4, gtol=2.0 * float(np.max(np.abs(g0))))
    x, f, g = eng.lbfgs_get()
    assert status == "CONVERGED" and len(hist) == 0 and evals == 0 and np.array_equal(x, th0) and f == f0 and np.array_equal(g, g0)
    # the whole run for comparison
    whole_hist, whole_evals, whole_status = eng.lbfgs_steps(8)
    whole = state_of(eng)
    assert whole_status == "MAXITER" and len(whole_hist) == 8 and whole_evals > 8
    # in pieces of 3 evaluations
    eng.lbfgs_init(th0, w, history=5)
    hs, ev_total, calls = [], 0, 0
    while sum(map(len, hs)) < 8:
        left = 8 - sum(map(len, hs))
        h, e, st = eng.lbfgs_steps(left, max_evals=3)
        assert e <= 3 and (st in ("RUN", "RETRY") or sum(map(len, hs)) + len(h) == 8)
        hs.append(h); ev_total += e; calls += 1
        assert calls < 40
    assert calls >= 3 and ev_total == whole_evals
    assert np.array_equal(np.concatenate(hs), whole_hist) and all(np.array_equal(a, b) for a, b in zip(state_of(eng), whole))
    # padding: 3 iterations asked of a state that converges by gtol after fewer — and the raw ABI's padded history
    eng.lbfgs_init(th0, w, history=5)
    buf = np.full(6, -1.0)
    it, ev, st = C.c_int(), C.c_int(), C.c_int()
    L.check(L.lib.pinn_lbfgs_steps(eng.h, 2, 1000, 1e-8, buf.ctypes.data_as(dp), C.byref(it), C.byref(ev), C.byref(st)), "pinn_lbfgs_steps")
    assert it.value == 2 and st.value == 4 and np.array_equal(buf[:2], whole_hist[:2]) and np.all(buf[2:] == -1.0)
    gnow = float(np.max(np.abs(eng.lbfgs_get()[2])))
    L.check(L.lib.pinn_lbfgs_steps(eng.h, 6, 1000, 2.0 * gnow, buf.ctypes.data_as(dp), C.byref(it), C.byref(ev), C.byref(st)), "pinn_lbfgs_steps")
    assert it.value == 0 and st.value == 2 and np.all(buf == whole_hist[1])          # padded with the objective at the iterate, as pinn_lbfgs pads


# term weights (floats) under which the fp32 adjoint seeds 2 w r / N sit just under the overflow: objective and gradient are finite at the
# start, a later gradient overflows, the direction and with it every trial point and trial objective are not finite (looked at on the CPU
# emulation).  The second set reaches the restart branch too: g.d is NaN there, which is not < 0.
HUGE_WEIGHTS = ([1.0e38, 1.0e38, 1.0e38], [5.0e37, 1.0, 1.0])


def body_nonfinite(npde, weights):
    """case 5 (fp32 mode): trials whose objective is not finite are rejected, not propagated; the iterate stays finite.  In float64 mode no
    start was found whose objective is finite while a trial's is not: the first step has norm <= 1 and the term weights are floats, so the
    double evaluation does not overflow between the two; is_finite(fn) is the same code for both element types."""
    rep, th0 = problem(npde, "poisson", "f32")
    eng = rep.engine
    ref = restate(eng, "f32", th0, weights, 5, 3)
    print(f"resident lbfgs non-finite {weights}: restatement status {ref['status']} non-finite trials {ref['nonfinite']} log {ref['log']}")
    assert ref["nonfinite"] >= 1 and ref["status"] == "STALLED"
    got = device_run(eng, th0, weights, 5, 3, per_iteration=False)
    assert got["status"] == ref["status"] and got["evals"] == ref["evals"] and len(got["hist"]) == len(ref["hist"])
    assert np.all(np.isfinite(got["x"])) and np.isfinite(got["f"]) and np.all(np.isfinite(got["hist"]))
    assert relerr(got["x"], ref["x"]) <= 1e-9 and relerr(got["f"], ref["f"]) <= 1e-9


def body_isolation(npde, precision):
    """case 6: evaluations, an Adam run and HMC draws between two lbfgs_steps calls leave the iterates alone, and the reverse"""
    rep, th0 = problem(npde, "poisson", precision)
    eng = rep.engine
    eng.lbfgs_init(th0, None, history=3)
    whole = list(eng.lbfgs_steps(5)) + state_of(eng)
    rep2, _ = problem(npde, "poisson", precision)
    e2 = rep2.engine
    stds = np.array([0.5, 0.3, 0.3])
    adam = e2.adam_f64 if precision == "f64" else e2.adam
    get = e2.adam_get_f64 if precision == "f64" else e2.adam_get
    other = th0 + 0.1
    it0, _ = adam(other, 3, 1e-3)
    e2.hmc_init(other, stds, NN_PRIOR, [])
    hmc0 = e2.hmc_get()
    e2.lbfgs_init(th0, None, history=3)
    first = e2.lbfgs_steps(2)
    assert np.array_equal(get(), it0) and all(np.array_equal(a, b) for a, b in zip(e2.hmc_get(), hmc0))
    e2.loss_grad_f64(other)
    e2.loss_grad(other)
    adam(other, 2, 1e-3)
    e2.hmc_draws(2, 2, 2.0e-2, 5)
    second = e2.lbfgs_steps(3)
    assert np.array_equal(np.concatenate([first[0], second[0]]), whole[0]) and first[1] + second[1] == whole[1]
    assert all(np.array_equal(a, b) for a, b in zip(state_of(e2), whole[3:]))


def body_refusals(npde, precision):
    """case 7: every refusal is named and leaves the handle evaluating as before"""
    rep, th0 = problem(npde, "poisson", precision)
    eng = rep.engine
    L, dp, ip = eng.L, C.POINTER(C.c_double), C.POINTER(C.c_int)
    ev0 = eng.loss_grad_f64(th0)
    hist, out = np.zeros(8), np.zeros(eng.P + 1)
    ptr = lambda a: a.ctypes.data_as(dp)
    n = [C.c_int(), C.c_int(), C.c_int()]

    def refused(rc, *words):
        assert rc != 0
        msg = L.last_error()
        assert all(w in msg for w in words), msg
        ev = eng.loss_grad_f64(th0)
        assert np.array_equal(ev[0], ev0[0]) and np.array_equal(ev[1], ev0[1])

    steps = lambda mi, me: L.lib.pinn_lbfgs_steps(eng.h, mi, me, 1e-8, ptr(hist), C.byref(n[0]), C.byref(n[1]), C.byref(n[2]))
    init = lambda p, m: L.lib.pinn_lbfgs_init(eng.h, ptr(th0), p, m, None)
    refused(steps(1, 10), "pinn_lbfgs_steps", "pinn_lbfgs_init first")
    refused(L.lib.pinn_lbfgs_get(eng.h, ptr(out), eng.P, None, None), "pinn_lbfgs_get", "pinn_lbfgs_init first")
    refused(init(eng.P - 1, 5), "pinn_lbfgs_init", "ntheta")
    refused(init(eng.P, 0), "pinn_lbfgs_init", "history")
    refused(init(eng.P, 65), "pinn_lbfgs_init", "history")
    eng.comm_init_custom(1, 0, lambda buf, count, dtype, stream: 0)
    refused(init(eng.P, 5), "pinn_lbfgs_init", "communicator")
    eng.comm_destroy()
    assert "lbfgs=resident" not in eng.describe()
    eng.lbfgs_init(th0, None, history=5)
    eng.lbfgs_steps(2)
    ref = state_of(eng)
    refused(steps(0, 10), "pinn_lbfgs_steps", "maxiters")
    refused(steps(1, 0), "pinn_lbfgs_steps", "max_evals")
    refused(L.lib.pinn_lbfgs_get(eng.h, ptr(out), eng.P + 1, None, None), "pinn_lbfgs_get", "ntheta")
    with pytest.raises(Exception, match="lbfgs_chunk"):
        eng.set_option("lbfgs_chunk", "65")
    with pytest.raises(Exception, match="lbfgs_chunk"):
        eng.set_option("lbfgs_chunk", "0")
    eng.comm_init_custom(1, 0, lambda buf, count, dtype, stream: 0)
    refused(steps(1, 10), "pinn_lbfgs_steps", "communicator")
    eng.comm_destroy()
    # a precision-mode change since init
    other = "f32" if precision == "f64" else "f64"
    eng.set_option("precision", other)
    ev0 = eng.loss_grad_f64(th0)
    refused(steps(1, 10), "pinn_lbfgs_steps", "precision changed")
    refused(L.lib.pinn_lbfgs_get(eng.h, ptr(out), eng.P, None, None), "pinn_lbfgs_get", "precision changed")
    eng.set_option("precision", precision)
    if precision == "f64":
        for k, s_ in enumerate(rep.pde_train_sets + rep.bcs_train_sets):
            eng.set_points_f64(k, s_)
    ev0 = eng.loss_grad_f64(th0)
    assert all(np.array_equal(a, b) for a, b in zip(state_of(eng), ref))          # the state itself is where it was
    eng.set_sampler(0, [0.0], [1.0], 11, seed=1)
    ev0 = eng.loss_grad_f64(th0)
    refused(steps(1, 10), "pinn_lbfgs_steps", "fixed")
    refused(init(eng.P, 5), "pinn_lbfgs_init", "fixed")
    assert all(np.array_equal(a, b) for a, b in zip(state_of(eng), ref))


def mirror_problem(npde, precision):
    import sympy as sp
    from test_resident_hmc import chain16
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.pi ** 2 * sp.sin(sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = chain16(npde)
    theta0 = npde.initialparameters(np.random.default_rng(7), chain)
    return npde.discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta0, precision=precision))


def body_mirror(npde, precision):
    """case 8: solve(prob, LBFGS(resident=True), maxiters=6) against the restatement; LBFGS() is still the host routine, bit for bit"""
    prob = mirror_problem(npde, precision)
    rep = prob.pinnrep
    eng = rep.engine
    th0 = np.asarray(prob.u0, dtype=np.float64)
    w = rep._weights_now()
    ref, sens, bar = bar_of(eng, precision, th0, w, 10, 6)
    it_before = rep.iteration[0]
    res = npde.solve(prob, npde.LBFGS(resident=True), maxiters=6)
    assert rep.iteration[0] == it_before + 6 and res.u.dtype == prob.u0.dtype
    e_u = relerr(res.u, ref["x"].astype(prob.u0.dtype))
    e_h = relerr(res.losses, ref["hist"])
    print(f"resident lbfgs mirror [{precision}]: theta err {e_u:.3e}  history err {e_h:.3e}  bar {bar:.3e}")
    assert e_h <= bar and abs(res.objective - ref["hist"][-1]) <= bar * abs(ref["hist"][-1])
    assert e_u <= max(bar, 2.0 ** -24 if prob.u0.dtype == np.float32 else 0.0)       # (a float32 u0 narrows the answer)
    assert npde.LBFGS().resident is False
    host = npde.solve(prob, npde.LBFGS(), maxiters=6)
    theta, hist = eng.lbfgs(prob.u0, 6, w, history=10, gtol=1e-8)
    assert np.array_equal(host.u, theta.astype(prob.u0.dtype)) and np.array_equal(host.losses, hist)


# ------------------------------------------------------------------------------------------------------------------------------------
# the two faces of every body
# ------------------------------------------------------------------------------------------------------------------------------------
PARITY = [(n, p, m) for n in PROBLEMS for p in PRECISIONS for m in (2, 10)]


@pytest.mark.parametrize("name,precision,history", PARITY)
def test_parity(npde, use_emu, name, precision, history):
    body_parity(npde, name, precision, history)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision,history", PARITY)
def test_parity_gpu(npde, hip_lib, name, precision, history):
    body_parity(npde, name, precision, history)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_backtracking(npde, use_emu, precision):
    body_backtracking(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_backtracking_gpu(npde, hip_lib, precision):
    body_backtracking(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking(npde, use_emu, precision):
    body_chunking(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_gpu(npde, hip_lib, precision):
    body_chunking(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_termination(npde, use_emu, precision):
    body_termination(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_termination_gpu(npde, hip_lib, precision):
    body_termination(npde, precision)


@pytest.mark.parametrize("weights", HUGE_WEIGHTS)
def test_nonfinite_trial(npde, use_emu, weights):
    body_nonfinite(npde, weights)


@pytest.mark.gpu
@pytest.mark.parametrize("weights", HUGE_WEIGHTS)
def test_nonfinite_trial_gpu(npde, hip_lib, weights):
    body_nonfinite(npde, weights)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_isolation(npde, use_emu, precision):
    body_isolation(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_isolation_gpu(npde, hip_lib, precision):
    body_isolation(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(npde, use_emu, precision):
    body_refusals(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_gpu(npde, hip_lib, precision):
    body_refusals(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror(npde, use_emu, precision):
    body_mirror(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror_gpu(npde, hip_lib, precision):
    body_mirror(npde, precision)
