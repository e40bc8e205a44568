"""Replica-resident L-BFGS (`pinn_lbfgs_replicas_*`): the quasi-Newton finisher of nrep trainings in one launch, one workgroup each.

Reference: `restate` of tests/test_resident_lbfgs.py (the slot algorithm in numpy double), driven by `oracle/pinn_oracle.py` `loss_and_grad` (float64,
exact mode) at float32(x) with the same term weights — never the code under test.  Computed once per (problem, history, maxiters) for three
replicas and shared; an nrep = 1 call is compared with replica 0.

Problems and start points: the two of tests/test_adam_replicas.py, imported with their seeds (init + 0.05 N(0, 1)) — (a) 1-6-1 tanh, P = 19 < 256,
idle waves; (b) 2-16-16-1 sigmoid, P = 338, one estimated parameter, a masked tile, term_w = [1, 10, 0.5].  These seeds were looked at on the CPU
with the oracle alone (and twelve others beside them): the reference's decision log (rejected trials, pushed, restarted per iteration) is the same
with its dot products forward and reversed (sensitivity of the iterates <= 7e-15) and the same when the emulation's `loss_grad` drives it instead of
the oracle (iterates then differ by <= 4.2e-5, the fp32 evaluation's noise, so no Armijo or curvature decision sits within that of its edge).
history = 2 over six iterations: every replica of (a) rejects trials in a later iteration (1 + 1, 2, 6 of them) and skips a curvature pair, every
replica of (b) rejects 3-4 trials in its first line search; all push more than two pairs, so the ring wraps and evicts.  test_reference asserts
all of this on the reference before it compares.

Compared, max-norm relative per replica (`compare`): every iterate's DISPLACEMENT x_k - x_0, the loss history, the final gradient; iterations,
evaluations and status must equal the reference's.  THE BAR is, per problem, 4 x the worst error of the existing `pinn_lbfgs_init / _steps` fp32
lane against the same reference on the same cases, measured on MI355X with tools/lbfgs_replicas_error.py (profiles/lbfgs_replicas.txt):
DEVICE_LANE_ERR below.  Every test runs twice (fixture `lib`): on the g++ emulation and, marked `gpu`, on the product library."""
import functools

import numpy as np
import pytest

import pinn_oracle as po
import test_adam_replicas as ar
from test_resident_lbfgs import restate, compare, relerr

DEVICE_LANE_ERR = {"a": 7.917e-06, "b": 5.362e-05}       # worst case of the pinn_lbfgs_steps fp32 lane per problem on an MI355X (profiles/lbfgs_replicas.txt)
CASES = [(10, 1), (2, 6)]                    # (history, maxiters): the ring never fills; it wraps and evicts
NREP = ar.NREP
TERM_W = ar.TERM_W


class OracleEval:
    """what `restate` asks of an engine, answered by the oracle"""
    def __init__(self, prob, sets):
        self.prob, self.sets, self.K = prob, sets, len(sets)

    def loss_grad(self, x32, w):
        ev = po.loss_and_grad(self.prob, np.asarray(x32, dtype=np.float64), self.sets, weights=w, mode="exact")
        return ev.term_losses, ev.grad


def problem(npde, case):
    """-> rep, oracle problem, point sets, theta0 [NREP x P] double (float32 values)"""
    rep, prob, sets, th0 = ar.problem(npde, case)
    return rep, prob, sets, th0.astype(np.float64)


@functools.lru_cache(maxsize=None)
def shared_reference(npde, case, history, maxiters):
    """per replica the restatement's result (read-only afterwards); its decisions must not depend on the order of its dot products"""
    _, prob, sets, th0 = problem(npde, case)
    out = []
    for r in range(NREP):
        fwd, bwd = (restate(OracleEval(prob, sets), "f32", th0[r], TERM_W[case], history, maxiters, rev=rev) for rev in (False, True))
        assert fwd["log"] == bwd["log"] and fwd["status"] == bwd["status"], (fwd["log"], bwd["log"])
        out.append(fwd)
    return out


def run(eng, th0, case, history, calls, **kw):
    """the rows of th0 through pinn_lbfgs_replicas_*, one _steps call per entry of `calls` -> per replica: history of the performed iterations,
    iterations, evaluations, status, x, f, g"""
    eng.lbfgs_replicas_init(th0, TERM_W[case], history=history)
    hists, its, evs = [[] for _ in th0], 0, 0
    for n in calls:
        h, it, ev, st = eng.lbfgs_replicas_steps(n, **kw)
        for r in range(len(th0)):
            hists[r].append(h[r, :it[r]])
            assert np.array_equal(h[r, it[r]:], np.full(n - it[r], eng.lbfgs_replicas_get()[1][r]), equal_nan=True)     # padded with the last objective
        its, evs = its + it, evs + ev
    x, f, g = eng.lbfgs_replicas_get()
    return dict(hist=[np.concatenate(h) for h in hists], its=its, evals=evs, status=st, x=x, f=f, g=g)


def same(p, i, q, j):
    """replica i of run p and replica j of run q hold the same bits"""
    return all(np.array_equal(p[k][i], q[k][j], equal_nan=True) for k in ("hist", "its", "evals", "status", "x", "f", "g"))


@pytest.fixture(params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def lib(request):
    return request.getfixturevalue("use_emu" if request.param == "emu" else "hip_lib")


def errors(npde, eng, case, nrep, history, maxiters, lane):
    """`lane(th0 rows) -> (per replica dict(xs, hist, g, evals, status name))` against the shared reference -> worst `compare` over the replicas"""
    th0 = problem(npde, case)[3]
    refs = shared_reference(npde, case, history, maxiters)
    for r in range(nrep):                                # the same decisions under the fp32 evaluation's noise, or the case is on an edge
        assert restate(eng, "f32", th0[r], TERM_W[case], history, maxiters)["log"] == refs[r]["log"]
    got, err = lane(th0[:nrep]), 0.0
    for r in range(nrep):
        assert (got[r]["status"], got[r]["evals"], len(got[r]["hist"])) == (refs[r]["status"], refs[r]["evals"], len(refs[r]["hist"]))
        err = max(err, compare(dict(got[r], xs=got[r]["xs"] - th0[r]), dict(refs[r], xs=refs[r]["xs"] - th0[r])))
    return err


def replica_lane(eng, case, history, maxiters):
    """one call of `maxiters` iterations, and the same again one iteration per call for the iterates, which must end on the same bits"""
    def lane(th0):
        whole = run(eng, th0, case, history, (maxiters,))
        eng.lbfgs_replicas_init(th0, TERM_W[case], history=history)
        xs = []
        for _ in range(maxiters):
            eng.lbfgs_replicas_steps(1)
            xs.append(eng.lbfgs_replicas_get()[0])
        xs = np.asarray(xs)
        assert np.array_equal(xs[-1], whole["x"])
        return [dict(xs=xs[:whole["its"][r], r], hist=whole["hist"][r], g=whole["g"][r], evals=whole["evals"][r],
                     status=eng.LBFGS_STATUS[whole["status"][r]]) for r in range(len(th0))]
    return lane


# ---- test 1: against the plain double reference ----
@pytest.mark.parametrize("case,nrep,history,maxiters", [(c, n, m, k) for c in "ab" for n in (1, NREP) for m, k in CASES])
def test_reference(npde, lib, case, nrep, history, maxiters):
    refs = shared_reference(npde, case, history, maxiters)
    if history == 2:                                     # what the case is for: rejected trials, a wrapped ring
        assert any(rej > 0 for q in refs for rej, _, _ in q["log"]) and all(sum(p for _, p, _ in q["log"]) > history for q in refs)
    eng = problem(npde, case)[0].engine
    err = errors(npde, eng, case, nrep, history, maxiters, replica_lane(eng, case, history, maxiters))
    bar = 4.0 * DEVICE_LANE_ERR[case]
    print(f"lbfgs replicas vs reference [{case} nrep={nrep} m={history} maxiters={maxiters}]: err {err:.3e}  bar {bar:.3e}")
    assert err <= bar


# ---- test 2: replica independence and continuation, exact ----
@pytest.mark.parametrize("case", ["a", "b"])
def test_independence(npde, lib, case):
    rep, _, _, th0 = problem(npde, case)
    eng = rep.engine
    three = run(eng, th0, case, 2, (6,))
    assert len(set(three["evals"])) > 1 or case == "b"   # (a): the workgroups run different numbers of slots
    for c in range(NREP):
        assert same(run(eng, th0[c:c + 1], case, 2, (6,)), 0, three, c), f"replica {c} alone differs"
        th1 = np.roll(th0, 1, axis=0) + 0.1              # its neighbours elsewhere; one of them not finite: it is terminal after its first slot
        th1[c], th1[(c + 1) % NREP] = th0[c], np.nan
        other = run(eng, th1, case, 2, (6,))
        assert other["status"][(c + 1) % NREP] == 2 and other["evals"][(c + 1) % NREP] == 0
        assert same(other, c, three, c), f"replica {c} depends on its neighbours"
    split = run(eng, th0, case, 2, (2, 4))
    assert all(same(split, c, three, c) for c in range(NREP))
    # one evaluation per call: every call but the first ends and resumes inside a line search or between two iterations
    c = int(np.argmax(three["evals"]))
    eng.lbfgs_replicas_init(th0[c:c + 1], TERM_W[case], history=2)
    hist, evals, calls = [], 0, 0
    while len(hist) < 6 and calls < 40:
        h, it, ev, st = eng.lbfgs_replicas_steps(6 - len(hist), max_evals=1)
        assert ev[0] <= 1
        hist += list(h[0, :it[0]]); evals += ev[0]; calls += 1
    x, f, g = eng.lbfgs_replicas_get()
    assert calls == three["evals"][c] + 1 and evals == three["evals"][c] and st[0] == three["status"][c] == 4
    assert np.array_equal(hist, three["hist"][c]) and np.array_equal(x[0], three["x"][c]) and f[0] == three["f"][c] and np.array_equal(g[0], three["g"][c])


# ---- test 3: refusals by name, the handle untouched ----
SETUPS = [(s, w.replace("no replica", "no lbfgs replica")) for s, w in ar.SETUPS if s not in ("lr", "noinit")] + [
    ("history0", "history must be in"), ("history65", "history must be in"), ("maxiters0", "maxiters must be"),
    ("noinit", "pinn_lbfgs_replicas_init first")]


@pytest.mark.parametrize("setup,words", SETUPS)
def test_refused_setups(npde, lib, setup, words):
    import handle_history as hh
    import test_emu_parity as tp
    if setup in hh.PROBLEMS:
        P = hh.problem(npde, setup)
        eng, th = npde._lib.Engine(P.descriptor), np.asarray(P.theta, dtype=np.float32)
        for k in range(P.K):
            eng.set_points(k, P.master[k][:, :24])
    else:
        if setup == "sin":
            sysm, chain = tp.poisson2d(npde, "sin", 16, 2)
            disc = npde.PhysicsInformedNN(chain, npde.GridTraining(0.25), init_params=npde.initialparameters(np.random.default_rng(7), chain), precision="f32")
        else:
            sysm, disc = ar.hc.poisson1d(npde, npde.Chain(npde.Dense(1, 6, "tanh"), npde.Dense(6, 1)))
        rep = npde.symbolic_discretize(sysm, disc)
        eng, th = rep.engine, np.asarray(rep.flat_init_params, dtype=np.float32)
        if setup == "sampler":
            eng.set_sampler(0, np.zeros(1, dtype=np.float32), np.ones(1, dtype=np.float32), 11, seed=3, kind=1)
    before = eng.loss_grad(th)
    if setup == "f64":
        eng.set_option("precision", "f64")
    with pytest.raises(npde.EngineError, match=words):
        if setup == "maxiters0":
            eng.lbfgs_replicas_init(np.stack([th, th]))
            eng.lbfgs_replicas_steps(0)
        elif setup == "noinit":
            eng.lbfgs_replicas_steps(1)
        else:
            eng.lbfgs_replicas_init(np.tile(th, ({"nrep0": 0, "nrep1025": 1025}.get(setup, 1), 1)), history={"history0": 0, "history65": 65}.get(setup, 10))
    if setup == "f64":
        eng.set_option("precision", "f32")
    if setup != "sampler":       # (a redrawn set differs from evaluation to evaluation)
        after = eng.loss_grad(th)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ---- test 4: API ----
def test_api(npde, lib):
    chain = npde.Chain(npde.Dense(1, 6, "tanh"), npde.Dense(6, 1))
    sysm, disc = ar.hc.poisson1d(npde, chain)
    prob = npde.discretize(sysm, disc)
    th0 = problem(npde, "a")[3]
    sol = npde.solve_replicas(prob, npde.LBFGS(m=4), th0, maxiters=3)
    eng = prob.pinnrep.engine
    eng.lbfgs_replicas_init(th0, prob.pinnrep._weights_now(), history=4)
    hist, it, ev, st = eng.lbfgs_replicas_steps(3)
    x, f, g = eng.lbfgs_replicas_get()
    assert np.array_equal(sol.u, x.astype(sol.u.dtype)) and np.array_equal(sol.losses, hist) and np.array_equal(sol.objective, f)
    assert sol.u.shape == (NREP, 19) and sol.losses.shape == (NREP, 3) and sol.best == int(np.argmin(f)) and np.array_equal(sol.status, st)
    with pytest.raises(ValueError, match="etas"):
        npde.solve_replicas(prob, npde.LBFGS(), th0, maxiters=2, etas=ar.LRS)
    with pytest.raises(ValueError, match="Adam or finished by LBFGS"):
        npde.solve_replicas(prob, npde.BFGS(), th0, maxiters=2)
    adam = npde.solve_replicas(prob, npde.Adam(0.01), th0.astype(np.float32), maxiters=4, etas=ar.LRS)      # the Adam call of test_adam_replicas
    th, _, _, h = ar.run(eng, th0.astype(np.float32), ar.LRS, "a", (4,))
    assert np.array_equal(adam.u, th.astype(adam.u.dtype)) and np.array_equal(adam.losses, h) and adam.status is None
