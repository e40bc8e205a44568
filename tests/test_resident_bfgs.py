"""Resident BFGS (`pinn_bfgs_init / _steps / _get`): the library's dense quasi-Newton finisher with the iterate, the inverse-Hessian
approximation H and the line search on the device.

The reference throughout is `restate` below: a numpy restatement of the algorithm of csrc/bfgs_kernels.hpp, driven by the SAME handle's
`loss_grad_f64` in float64 mode and by `loss_grad` at float32(x) otherwise — never the code under test, and never scipy.  Its `rev` switch runs
every dot product and every row sum of H v in reversed order.

Every body is written once as a function of `npde` and exposed twice: on the CPU through the g++ emulation (`use_emu`) and, marked `gpu`, on
the product library (`hip_lib`).

Problems (the smallest that cross the kernels' boundaries), all on GridTraining(0.1), both precisions:
  poisson   1-D Poisson, Dense 1 -> 16 -> 16 -> 1 tanh, P = 321: odd (rows are 16-byte aligned only through the padded leading dimension);
            five full 64-column strides plus one column; 80 workgroups of four rows plus one that owns a single row
  inverse   the inverse problem with one estimated parameter and one DataLoss term, P = 322 (even), K = 4
  tiny      Dense 1 -> 4 -> 1 on the Poisson problem, P = 13: fewer columns than a wave has lanes (one stride, mostly padding); three workgroups
            of four rows and one that owns a single row

THE BAR.  Device and restatement differ only in the order of the sums (dot products, row sums of H v); BFGS amplifies such differences from one
iteration to the next exactly as L-BFGS does.  The restatement's own sensitivity is measured by running it twice, its sums in forward and in
reversed order: s = the largest max-norm relative difference over the iterates, loss_history, the final gradient and the final H.
bar = min(1e-6, 100 * max(s, 2^-52 * iterations)); the margin of 100 is §4.7's / §4.8's.  The two restatement runs must take the same sequence
of accept / reject / update / skip / restart decisions (asserted): otherwise the case sits on an edge.  Measured figures:
profiles/resident_bfgs.txt."""
import ctypes as C

import numpy as np
import pytest

from test_resident_hmc import forward_problem, inverse_problem, relerr, NN_PRIOR
from test_resident_lbfgs import BACKTRACK, HUGE_WEIGHTS

EPS64 = 2.0 ** -52
PRECISIONS = ("f64", "f32")
PROBLEMS = ("poisson", "inverse", "tiny")


def tiny_problem(npde, precision, seed=7):
    import sympy as sp
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.pi ** 2 * sp.sin(sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 4, "tanh"), npde.Dense(4, 1))
    theta0 = npde.initialparameters(np.random.default_rng(seed), chain)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta0, precision=precision))
    assert rep.engine.P == 13 and rep.engine.K == 3
    return rep, np.asarray(rep.flat_init_params, dtype=np.float64).copy()


def problem(npde, name, precision):
    """-> (representation, theta0); the handle is kept alive by the representation"""
    if name == "tiny":
        return tiny_problem(npde, precision)
    return (forward_problem(npde, precision) if name == "poisson" else inverse_problem(npde, precision, "normal"))[:2]


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement; `rev`: dot products and row sums in reversed order
# ------------------------------------------------------------------------------------------------------------------------------------
def restate(eng, precision, th0, w, maxiters, gtol=1e-8, rev=False):
    """-> dict(xs = iterate after every iteration, hist, x, f, g, H = the materialised matrix, evals, status,
    log = (rejected trials, 'update' | 'skip', restarted) per iteration, nonfinite = trials whose objective was not finite,
    pair = the last accepted (s, y), ident)"""
    if rev:
        dot = lambda a, b: float(np.sum((a * b)[::-1]))
        matvec = lambda H, v: np.sum((H * v[None, :])[:, ::-1], axis=1)
    else:
        dot = lambda a, b: float(np.sum(a * b))
        matvec = lambda H, v: np.sum(H * v[None, :], axis=1)
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
    P = x.size
    with np.errstate(all="ignore"):
        f, g = ev(x)
        ident, gamma, H = True, 1.0, None
        xs, hist, log, pair = [], [], [], None
        evals, nonfinite, status = 0, 0, "MAXITER"
        for it in range(maxiters):
            if not (np.fmax.reduce(np.abs(g), initial=0.0) > gtol):          # (fmax: a NaN entry is skipped)
                status = "CONVERGED"
                break
            d = -(gamma * g) if ident else -matvec(H, g)
            gd = dot(g, d)
            restart = False
            if not (gd < 0.0):
                ident, gamma, restart = True, 1.0, True
                d = -g
                gd = dot(g, d)
            t = 1.0
            if ident and gamma == 1.0:
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
                log.append((rejects, "stall", restart))
                break
            s, y = xn - x, gn - g
            sy = dot(s, y)
            update = bool(sy > 1e-10 * np.sqrt(dot(s, s) * dot(y, y)))
            if update:
                if ident:
                    gamma = sy / dot(y, y)
                    H = gamma * np.eye(P)
                    ident = False
                u = matvec(H, y)
                rho = 1.0 / sy
                c = rho * (1.0 + rho * dot(y, u))
                H = (H - rho * (np.outer(s, u) + np.outer(u, s))) + c * np.outer(s, s)
            pair = (s, y)
            x, g, f = xn, gn, fn
            hist.append(f); xs.append(x.copy()); log.append((rejects, "update" if update else "skip", restart))
    Hm = gamma * np.eye(P) if ident else H
    return dict(xs=np.asarray(xs), hist=np.asarray(hist), x=x, f=f, g=g, H=Hm, evals=evals, status=status, log=log, nonfinite=nonfinite,
                pair=pair, ident=ident)


def compare(got, ref):
    """largest max-norm relative error over every iterate, loss_history, the final gradient and the final H"""
    assert got["xs"].shape == ref["xs"].shape and got["hist"].shape == ref["hist"].shape, (got["xs"].shape, ref["xs"].shape)
    errs = [relerr(a, b) for a, b in zip(got["xs"], ref["xs"])] + [relerr(got["g"], ref["g"]), relerr(got["H"], ref["H"])]
    if len(ref["hist"]):
        errs.append(relerr(got["hist"], ref["hist"]))
    return max(errs)


def bar_of(eng, precision, th0, w, maxiters, gtol=1e-8):
    fwd = restate(eng, precision, th0, w, maxiters, gtol)
    bwd = restate(eng, precision, th0, w, maxiters, gtol, rev=True)
    assert fwd["log"] == bwd["log"] and fwd["status"] == bwd["status"], (fwd["log"], bwd["log"])     # the same decisions, or the case is on an edge
    sens = compare(bwd, fwd)
    return fwd, sens, min(1e-6, 100.0 * max(sens, EPS64 * max(len(fwd["hist"]), 1)))


def state_of(eng):
    return list(eng.bfgs_get(want_hinv=True))


def device_run(eng, th0, w, maxiters, gtol=1e-8, per_iteration=True):
    """the resident loop: one call of `maxiters` iterations and (per_iteration) the same again one iteration per call for the iterates, which
    must end on the same bits"""
    eng.bfgs_init(th0, w)
    hist, evals, status = eng.bfgs_steps(maxiters, gtol=gtol)
    x, f, g, H = eng.bfgs_get(want_hinv=True)
    out = dict(hist=hist, evals=evals, status=status, x=x, f=f, g=g, H=H, xs=None, gs=None)
    if per_iteration:
        eng.bfgs_init(th0, w)
        xs, gs = [], []
        for _ in range(len(hist)):
            h1, _, _ = eng.bfgs_steps(1, gtol=gtol)
            assert len(h1) == 1
            xi, _, gi, _ = eng.bfgs_get()
            xs.append(xi); gs.append(gi)
        out["xs"] = np.asarray(xs).reshape(len(hist), eng.P)
        out["gs"] = np.asarray(gs).reshape(len(hist), eng.P)
        assert len(hist) == 0 or (np.array_equal(out["xs"][-1], x) and np.array_equal(eng.bfgs_get(want_hinv=True)[3], H))
    return out


def backtrack_setup(npde, precision):
    rep, th0 = problem(npde, "poisson", precision)
    return rep, BACKTRACK["scale"] * th0, BACKTRACK["weights"]


# ------------------------------------------------------------------------------------------------------------------------------------
# bodies
# ------------------------------------------------------------------------------------------------------------------------------------
def body_parity(npde, name, precision):
    """case 1: six iterations; iterates after every iteration, loss_hist, f, g, hinv within the bar; evals and status equal.
    On the Poisson problem the second accepted step fails the curvature test s.y > 1e-10 |s| |y| while H is a matrix (Armijo alone does not
    enforce s.y > 0 on a non-convex objective): the update is SKIPPED and d = -H g comes from k_bfgs_matvec (case 5; looked at on the CPU
    emulation, asserted on the restatement)."""
    rep, th0 = problem(npde, name, precision)
    eng = rep.engine
    ref, sens, bar = bar_of(eng, precision, th0, None, 6)
    got = device_run(eng, th0, None, 6)
    err = compare(got, ref)
    print(f"resident bfgs parity [{name} {precision}]: err {err:.3e}  sensitivity {sens:.3e}  bar {bar:.3e}  log {ref['log']}")
    kinds = [k for _, k, _ in ref["log"]]
    assert len(ref["hist"]) == 6 and kinds.count("update") >= 3
    assert name != "poisson" or ("skip" in kinds and "update" in kinds[:kinds.index("skip")]), ref["log"]
    assert got["status"] == ref["status"] == "MAXITER" and got["evals"] == ref["evals"]
    assert err <= bar
    assert relerr(got["f"], ref["f"]) <= bar and "bfgs=resident(P=%d" % eng.P in eng.describe()


def body_backtracking(npde, precision):
    """case 2: a start from which the restatement rejects at least one trial in at least two different iterations"""
    rep, th0, w = backtrack_setup(npde, precision)
    eng = rep.engine
    ref, sens, bar = bar_of(eng, precision, th0, w, 8)
    print(f"resident bfgs backtracking [{precision}]: sensitivity {sens:.3e}  bar {bar:.3e}  log {ref['log']}")
    assert sum(r > 0 for r, _, _ in ref["log"]) >= 2, ref["log"]
    got = device_run(eng, th0, w, 8)
    err = compare(got, ref)
    print(f"resident bfgs backtracking [{precision}]: err {err:.3e}  evals {got['evals']}")
    assert got["evals"] == ref["evals"] and got["status"] == ref["status"]
    assert err <= bar


def body_chunking(npde, precision):
    """case 3: lbfgs_chunk = 1, 3, 8; steps(2) + steps(3) against steps(5); a chunk boundary on a RETRY slot (backtracking case, chunk 1);
    a max_evals that ends a call inside a line search"""
    outs = []
    for chunk, split in ((8, (5,)), (1, (5,)), (3, (5,)), (8, (2, 3)), (3, (2, 3))):
        rep, th0 = problem(npde, "poisson", precision)
        eng = rep.engine
        eng.set_option("lbfgs_chunk", str(chunk))
        eng.bfgs_init(th0, None)
        parts = [eng.bfgs_steps(n) for n in split]
        outs.append([np.concatenate([q[0] for q in parts]), sum(q[1] for q in parts)] + state_of(eng))
    assert len(outs[0][0]) == 5
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    outs = []
    for chunk in (8, 1):
        rep, th0, w = backtrack_setup(npde, precision)
        eng = rep.engine
        eng.set_option("lbfgs_chunk", str(chunk))
        eng.bfgs_init(th0, w)
        hist, evals, status = eng.bfgs_steps(8)
        outs.append([hist, evals] + state_of(eng))
    assert outs[0][1] > 8                                   # (there were rejected trials: with chunk 1 every RETRY slot ended a chunk)
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
    whole_hist, whole_evals, whole = outs[0][0], outs[0][1], outs[0][2:]
    # in pieces of 3 evaluations: some call ends inside a line search (status RETRY) and the next one resumes there
    eng.bfgs_init(th0, w)
    hs, ev_total, calls, statuses = [], 0, 0, []
    while sum(map(len, hs)) < 8:
        left = 8 - sum(map(len, hs))
        h, e, st = eng.bfgs_steps(left, max_evals=3)
        assert e <= 3 and (st in ("RUN", "RETRY") or sum(map(len, hs)) + len(h) == 8)
        hs.append(h); ev_total += e; calls += 1; statuses.append(st)
        assert calls < 40
    assert "RETRY" in statuses and ev_total == whole_evals
    assert np.array_equal(np.concatenate(hs), whole_hist) and all(np.array_equal(a, b) for a, b in zip(state_of(eng), whole))


def body_matrix(npde, name, precision):
    """case 4: hinv is exactly I before any update, bit-symmetric after; the secant equation hinv y = s of the last accepted pair holds as
    well as it does for the restatement; positive definite.
    The bound on the secant residual: 100 x the larger of the restatement's own residual and the resolution floor 2^-52 P max|hinv| max|y| of
    one row sum (the restatement's residual may fall below the floor by luck)."""
    rep, th0 = problem(npde, name, precision)
    eng = rep.engine
    eng.bfgs_init(th0, None)
    assert np.array_equal(eng.bfgs_get(want_hinv=True)[3], np.eye(eng.P))
    ref = restate(eng, precision, th0, None, 6)
    assert ref["log"][-1][1] == "update" and len(ref["hist"]) == 6
    got = device_run(eng, th0, None, 6)
    H = got["H"]
    assert np.array_equal(H, H.T) and not np.array_equal(H, np.eye(eng.P))
    s = got["xs"][-1] - got["xs"][-2]
    y = got["gs"][-1] - got["gs"][-2]
    res = float(np.max(np.abs(H @ y - s)))
    rs, ry = ref["pair"]
    ref_res = float(np.max(np.abs(ref["H"] @ ry - rs)))
    floor = EPS64 * eng.P * float(np.max(np.abs(H))) * float(np.max(np.abs(y)))
    lam = float(np.linalg.eigvalsh(H).min())
    print(f"resident bfgs matrix [{name} {precision}]: secant residual {res:.3e}  restatement's {ref_res:.3e}  floor {floor:.3e}  min eigenvalue {lam:.3e}")
    assert res <= 100.0 * max(ref_res, floor)
    if name != "inverse":
        assert lam > 0.0


def body_nonfinite(npde, weights):
    """case 5 (fp32 mode; the skipped update is in case 1): trials whose objective is not finite are rejected and counted, not propagated; with the second weight set g.d is
    not finite, which is not < 0: the restart branch, H back to the identity.  The decisions match the restatement's."""
    rep, th0 = problem(npde, "poisson", "f32")
    eng = rep.engine
    ref = restate(eng, "f32", th0, weights, 3)
    print(f"resident bfgs non-finite {weights}: restatement status {ref['status']} non-finite trials {ref['nonfinite']} log {ref['log']}")
    assert ref["nonfinite"] >= 1 and ref["status"] == "STALLED"
    if weights is HUGE_WEIGHTS[1]:
        assert ref["log"][-1][2] and ref["ident"]             # the restart was taken
    got = device_run(eng, th0, weights, 3, per_iteration=False)
    assert got["status"] == ref["status"] and got["evals"] == ref["evals"] and len(got["hist"]) == len(ref["hist"])
    assert np.all(np.isfinite(got["x"])) and np.isfinite(got["f"]) and np.all(np.isfinite(got["hist"]))
    assert relerr(got["x"], ref["x"]) <= 1e-9 and relerr(got["f"], ref["f"]) <= 1e-9
    if ref["ident"]:
        assert np.array_equal(got["H"], np.eye(eng.P))


def body_stall_switch(npde, monkeypatch):
    """case 5, the noise-floor switch: a handle in "split" GEMM mode whose kernels have fp32 twins (two 64-wide hidden layers, P = 4,353: the
    smallest such network) that reaches STALLED is switched to "fp32" once, re-adopted at x with H = I, runs 30 more trials and is handed
    back in "split" mode; $PINN_LBFGS_KEEP_GEMM keeps it where it is.  The stall is that of the first non-finite weight set."""
    import sympy as sp
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.pi ** 2 * sp.sin(sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 64, "tanh"), npde.Dense(64, 64, "tanh"), npde.Dense(64, 1))
    theta0 = npde.initialparameters(np.random.default_rng(7), chain)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta0, precision="f32"))
    eng = rep.engine
    th0 = np.asarray(rep.flat_init_params, dtype=np.float64)
    assert eng.P == 4353 and eng.get_option("gemm") == "split"
    ref = restate(eng, "f32", th0, HUGE_WEIGHTS[0], 3)
    assert ref["status"] == "STALLED" and ref["ident"] and ref["nonfinite"] == 30, ref["log"]
    monkeypatch.setenv("PINN_LBFGS_KEEP_GEMM", "1")
    eng.bfgs_init(th0, HUGE_WEIGHTS[0])
    hist, evals, status = eng.bfgs_steps(3)
    assert status == "STALLED" and evals == ref["evals"] and len(hist) == len(ref["hist"]) and eng.get_option("gemm") == "split"
    monkeypatch.delenv("PINN_LBFGS_KEEP_GEMM")
    eng.bfgs_init(th0, HUGE_WEIGHTS[0])
    hist, evals, status = eng.bfgs_steps(3)
    x1, f1, _, _ = eng.bfgs_get()
    print(f"resident bfgs stall switch: evals {evals} (restatement without the switch: {ref['evals']})  status {status}")
    assert status == "STALLED" and evals == ref["evals"] + 30 and len(hist) == len(ref["hist"])
    assert eng.get_option("gemm") == "split" and np.all(np.isfinite(x1)) and np.isfinite(f1)
    assert relerr(x1, ref["x"]) <= 1e-9


def body_independence(npde, name, precision):
    """case 6: evaluations, an Adam step, an L-BFGS run and (the forward problem) HMC draws between two bfgs_steps calls leave the iteration
    alone, and each returns the bits it returns on a fresh handle"""
    rep, th0 = problem(npde, name, precision)
    eng = rep.engine
    eng.bfgs_init(th0, None)
    whole = list(eng.bfgs_steps(5)) + state_of(eng)
    other = th0 + 0.1
    stds = np.array([0.5, 0.3, 0.3])

    def others(e):
        adam = e.adam_f64 if precision == "f64" else e.adam
        out = [e.loss_grad_f64(other) if precision == "f64" else e.loss_grad(other.astype(np.float32))]
        out.append(adam(other, 1, 1e-3))
        e.lbfgs_init(other, None, history=3)
        out.append(e.lbfgs_steps(2)[0])
        out.append(e.lbfgs_get())
        if name == "poisson":
            e.hmc_init(other, stds, NN_PRIOR, [])
            out.append(e.hmc_draws(2, 2, 2.0e-2, 5))
        flat = []
        for o in out:
            flat += [np.asarray(q) for q in o if q is not None]
        return flat
    fresh = others(problem(npde, name, precision)[0].engine)
    rep2, _ = problem(npde, name, precision)
    e2 = rep2.engine
    e2.bfgs_init(th0, None)
    first = e2.bfgs_steps(2)
    between = others(e2)
    assert len(between) == len(fresh) and all(np.array_equal(a, b) for a, b in zip(between, fresh))
    second = e2.bfgs_steps(3)
    assert np.array_equal(np.concatenate([first[0], second[0]]), whole[0]) and first[1] + second[1] == whole[1]
    assert all(np.array_equal(a, b) for a, b in zip(state_of(e2), whole[3:]))


def body_reproducible(npde, precision):
    """case 7: two fresh handles give bit-equal histories, iterates and hinv"""
    runs = []
    for _ in range(2):
        rep, th0, w = backtrack_setup(npde, precision)
        got = device_run(rep.engine, th0, w, 6)
        runs.append([got["hist"], got["xs"], got["x"], got["g"], got["H"], np.float64(got["f"])])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


def body_refusals(npde, precision, monkeypatch):
    """case 8: every refusal is named and leaves the handle evaluating as before"""
    rep, th0 = problem(npde, "poisson", precision)
    eng = rep.engine
    L, dp = eng.L, C.POINTER(C.c_double)
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

    steps = lambda mi, me: L.lib.pinn_bfgs_steps(eng.h, mi, me, 1e-8, ptr(hist), C.byref(n[0]), C.byref(n[1]), C.byref(n[2]))
    init = lambda p: L.lib.pinn_bfgs_init(eng.h, ptr(th0), p, None)
    get = lambda p: L.lib.pinn_bfgs_get(eng.h, ptr(out), p, None, None, None)
    refused(steps(1, 10), "pinn_bfgs_steps", "pinn_bfgs_init first")
    refused(get(eng.P), "pinn_bfgs_get", "pinn_bfgs_init first")
    refused(init(eng.P - 1), "pinn_bfgs_init", "ntheta")
    eng.comm_init_custom(1, 0, lambda buf, count, dtype, stream: 0)
    refused(init(eng.P), "pinn_bfgs_init", "communicator")
    eng.comm_destroy()
    monkeypatch.setenv("PINN_BFGS_MAX_P", "100")             # a matrix that is not to be allocated: the message names P and the bytes
    refused(init(eng.P), "pinn_bfgs_init", "P = 321", "%d bytes" % (8 * 321 * 384))
    monkeypatch.delenv("PINN_BFGS_MAX_P")
    assert "bfgs=resident" not in eng.describe()
    eng.bfgs_init(th0, None)
    eng.bfgs_steps(2)
    ref = state_of(eng)
    refused(steps(0, 10), "pinn_bfgs_steps", "maxiters")
    refused(steps(1, 0), "pinn_bfgs_steps", "max_evals")
    refused(get(eng.P + 1), "pinn_bfgs_get", "ntheta")
    eng.comm_init_custom(1, 0, lambda buf, count, dtype, stream: 0)
    refused(steps(1, 10), "pinn_bfgs_steps", "communicator")
    eng.comm_destroy()
    # a precision-mode change since init
    other = "f32" if precision == "f64" else "f64"
    eng.set_option("precision", other)
    ev0 = eng.loss_grad_f64(th0)
    refused(steps(1, 10), "pinn_bfgs_steps", "precision changed")
    refused(get(eng.P), "pinn_bfgs_get", "precision changed")
    eng.set_option("precision", precision)
    if precision == "f64":
        for k, s_ in enumerate(rep.pde_train_sets + rep.bcs_train_sets):
            eng.set_points_f64(k, s_)
    ev0 = eng.loss_grad_f64(th0)
    assert all(np.array_equal(a, b) for a, b in zip(state_of(eng), ref))          # the state itself is where it was
    eng.set_sampler(0, [0.0], [1.0], 11, seed=1)
    ev0 = eng.loss_grad_f64(th0)
    refused(steps(1, 10), "pinn_bfgs_steps", "fixed")
    refused(init(eng.P), "pinn_bfgs_init", "fixed")
    assert all(np.array_equal(a, b) for a, b in zip(state_of(eng), ref))


def body_mirror(npde, precision):
    """case 9: solve(prob, BFGS(resident=True), maxiters=40) against the restatement; BFGS() is still scipy on the host"""
    from test_resident_lbfgs import mirror_problem
    prob = mirror_problem(npde, precision)
    rep = prob.pinnrep
    eng = rep.engine
    th0 = np.asarray(prob.u0, dtype=np.float64)
    w = rep._weights_now()
    ref, sens, bar = bar_of(eng, precision, th0, w, 40)
    res = npde.solve(prob, npde.BFGS(resident=True), maxiters=40)
    print(f"resident bfgs mirror [{precision}]: objective {res.objective:.6e}  restatement's {ref['f']:.6e}  bar {bar:.3e}  iterations {len(res.losses)}")
    assert np.all(np.isfinite(res.losses)) and np.all(np.diff(res.losses) <= 0.0) and res.losses[-1] < res.losses[0]
    assert len(res.losses) == len(ref["hist"]) and abs(res.objective - ref["f"]) <= bar * abs(ref["f"])
    assert "bfgs=resident(P=321" in eng.describe()
    with pytest.raises(ValueError, match="callback"):
        npde.solve(prob, npde.BFGS(resident=True), maxiters=2, callback=lambda state, loss: False)
    assert npde.BFGS().resident is False
    prob2 = mirror_problem(npde, precision)
    host = npde.solve(prob2, npde.BFGS(), maxiters=3)
    assert np.isfinite(host.objective) and "bfgs=resident" not in prob2.pinnrep.engine.describe()


# ------------------------------------------------------------------------------------------------------------------------------------
# the two faces of every body
# ------------------------------------------------------------------------------------------------------------------------------------
PARITY = [(n, p) for n in PROBLEMS for p in PRECISIONS]
MATRIX = [(n, p) for n in PROBLEMS for p in PRECISIONS]
INDEP = [(n, p) for n in ("poisson", "inverse") for p in PRECISIONS]


@pytest.mark.parametrize("name,precision", PARITY)
def test_parity(npde, use_emu, name, precision):
    body_parity(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", PARITY)
def test_parity_gpu(npde, hip_lib, name, precision):
    body_parity(npde, name, precision)


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


@pytest.mark.parametrize("name,precision", MATRIX)
def test_matrix(npde, use_emu, name, precision):
    body_matrix(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", MATRIX)
def test_matrix_gpu(npde, hip_lib, name, precision):
    body_matrix(npde, name, precision)


@pytest.mark.parametrize("weights", HUGE_WEIGHTS)
def test_nonfinite_trial_and_restart(npde, use_emu, weights):
    body_nonfinite(npde, weights)


@pytest.mark.gpu
@pytest.mark.parametrize("weights", HUGE_WEIGHTS)
def test_nonfinite_trial_and_restart_gpu(npde, hip_lib, weights):
    body_nonfinite(npde, weights)


def test_stall_switches_gemm(npde, use_emu, monkeypatch):
    body_stall_switch(npde, monkeypatch)


@pytest.mark.gpu
def test_stall_switches_gemm_gpu(npde, hip_lib, monkeypatch):
    body_stall_switch(npde, monkeypatch)


@pytest.mark.parametrize("name,precision", INDEP)
def test_independence(npde, use_emu, name, precision):
    body_independence(npde, name, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", INDEP)
def test_independence_gpu(npde, hip_lib, name, precision):
    body_independence(npde, name, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_reproducible(npde, use_emu, precision):
    body_reproducible(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_reproducible_gpu(npde, hip_lib, precision):
    body_reproducible(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(npde, use_emu, precision, monkeypatch):
    body_refusals(npde, precision, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_gpu(npde, hip_lib, precision, monkeypatch):
    body_refusals(npde, precision, monkeypatch)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror(npde, use_emu, precision):
    body_mirror(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirror_gpu(npde, hip_lib, precision):
    body_mirror(npde, precision)
