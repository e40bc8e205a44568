"""Resident HMC warm-up (`pinn_hmc_find_stepsize`, `pinn_hmc_warmup`): the initial step-size search, the dual averaging of the
step size and the windowed diagonal metric of `bpinn._hmc_device` with the chain on the device.

Problems, restatement (`restate`), bar (`bar_of`) and generator (`gen_draw`) are those of tests/test_resident_hmc.py, imported unchanged.  Every
body is written once and exposed twice: on the CPU emulation (`use_emu`) and, marked `gpu`, on the product library (`hip_lib`).

WHY PIECEWISE.  An adaptive chain amplifies last-place differences (the restated warm-up against itself with its energy sums reversed, 100 draws x 2
steps: 3e-9 ... 3e-8 in float64 mode, O(1) in fp32 mode), so a warm-up is never compared end to end.  It is checked in well-conditioned pieces:
  1. every transition  draw j alone, restated from samples[j - 1] with step_sizes[j], Z[j] / sqrt(metric in force), U[j]: the bar of `bar_of`
  2. the recurrence    step_sizes and eps_final recomputed in numpy from the returned accept_prob alone
  3. the metric        recomputed from the returned sample rows [w0, w1); the handle holds it (one further draw meets the restatement with it)
BARS of 2 and 3: 100 x the largest elementwise relative difference between the numpy recomputation in float64 and in numpy.longdouble, measured
in the test, floored at 100 x 2^-52 (no double result resolves its own last place).  Measured figures: profiles/resident_hmc_warmup.txt."""
import ctypes as C

import numpy as np
import pytest

from test_resident_hmc import (EPS64, EPS_STEP, GEN_SEED, NN_PRIOR, PRECISIONS, bar_of, compare, forward_problem, gen_draw, inverse_problem, kinds_of,
                               make_logp, small_problem)

EPS0, TARGET = 0.02, 0.8
RUNS = ((100, 2), (107, 1))
SHORT = (1, 20)
EDGE = 1e-6                # |u - a| of every reference draw: no accept decision on the edge (body_generator's threshold)


def window(n):
    w0, w1 = int(0.15 * n), int(0.9 * n)
    return w0, w1, (w1 - w0 >= 8 and n >= 100)


def supplied(P, n):
    rng = np.random.default_rng(11)
    Z = rng.standard_normal((n, P))
    return Z, rng.random(n)


def relmax(x, ref):
    """largest elementwise relative difference"""
    x, ref = np.asarray(x, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(x - ref) / np.abs(ref)))


# ------------------------------------------------------------------------------------------------------------------------------------
# numpy restatements of the adaptation (bpinn.py: _hmc_device), in the float type `ft`
# ------------------------------------------------------------------------------------------------------------------------------------
def recurrence(acc, eps0, target, ft):
    """-> (step_sizes [n], eps_final) from the acceptance probabilities alone"""
    n = len(acc)
    _, w1, event = window(n)
    f = ft
    t0, gamma, kappa = f(10.0), f(0.05), f(0.75)
    eps = f(eps0)
    mu, hbar, leb, m = np.log(f(10) * eps), f(0.0), f(0.0), 0
    steps = []
    for it in range(n):
        steps.append(eps)
        a = f(acc[it])
        m += 1
        hbar = (f(1) - f(1) / (f(m) + t0)) * hbar + (f(target) - a) / (f(m) + t0)
        log_eps = mu - np.sqrt(f(m)) / gamma * hbar
        eta = np.power(f(m), -kappa)
        leb = eta * log_eps + (f(1) - eta) * leb
        eps = np.exp(log_eps)
        if event and it == w1 - 1:
            mu, hbar, leb, m = np.log(f(10) * eps), f(0.0), f(0.0), 0
        if it == n - 1 and m > 0:
            eps = np.exp(leb)
    return np.asarray(steps, dtype=ft), eps


def window_metric(rows, ft):
    rows = np.asarray(rows, dtype=ft)
    k = ft(rows.shape[0])
    return (k / (k + ft(5.0))) * np.var(rows, axis=0) + ft(1e-3) * (ft(5.0) / (k + ft(5.0)))


def search(eng, stds, nn, priors, th0, minv, z, eps0):
    """bpinn.py `_hmc_device` lines 140-158 -> (eps, trials, smallest |d - log 0.8|, largest |H|)"""
    logp_grad, _ = make_logp(eng, stds, nn, priors)
    th = th0.astype(np.float64).copy()
    lp, g = logp_grad(th)

    def one_step(r, eps):
        r = r + 0.5 * eps * g
        t1 = th + eps * minv * r
        lp1, g1 = logp_grad(t1)
        r = r + 0.5 * eps * g1
        return -lp1 + 0.5 * np.sum(minv * r * r)
    eps = eps0
    r0 = z / np.sqrt(minv)
    h0 = -lp + 0.5 * np.sum(minv * r0 * r0)
    with np.errstate(all="ignore"):
        d = h0 - one_step(r0, eps)
        margins, trials = [abs(d - np.log(0.8))], 1
        direction = 1.0 if (np.isfinite(d) and d > np.log(0.8)) else -1.0
        for _ in range(40):
            eps *= 2.0 ** direction
            d = h0 - one_step(r0, eps)
            trials += 1
            if not np.isfinite(d):
                d = -np.inf
            margins.append(abs(d - np.log(0.8)))
            if (direction > 0) == (d <= np.log(0.8)):
                break
    return eps, trials, min(margins), abs(h0)


# ------------------------------------------------------------------------------------------------------------------------------------
# one warm-up per (face, precision, n_adapts, n_leapfrog), shared by the cases that look at it; nothing below changes it
# ------------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


class Run:
    pass


def warmup_run(npde, face, precision, n, L):
    key = (face, precision, n, L)
    if key not in _CACHE:
        w = Run()
        w.rep, w.th0, w.stds, w.nn, w.priors = forward_problem(npde, precision)
        w.eng = w.rep.engine
        w.n, w.L = n, L
        w.Z, w.U = supplied(w.eng.P, n)
        w.eng.hmc_init(w.th0, w.stds, NN_PRIOR, [])
        w.smp, w.acc, w.lp, w.steps, w.eps_final, w.minv = w.eng.hmc_warmup(n, L, EPS0, TARGET, 0, w.Z, w.U)
        w.state = w.eng.hmc_get()
        _CACHE[key] = w
    return _CACHE[key]


def check_transitions(tag, eng, stds, nn, priors, start, out, Z, U, L):
    """case 1: every draw of a warm-up `out` against its own one-draw restatement"""
    smp, acc, lp, steps, eps_final, minv_end = out
    n = len(acc)
    _, w1, event = window(n)
    ones = np.ones(eng.P)
    worst, worst_bar, edge, accepted = 0.0, 0.0, np.inf, 0
    for j in range(n):
        minv = minv_end if (event and j > w1 - 1) else ones
        prev = start if j == 0 else smp[j - 1]
        ref, sens, bar = bar_of(eng, stds, nn, priors, prev, minv, (Z[j] / np.sqrt(minv))[None, :], U[j:j + 1], L, float(steps[j]))
        edge = min(edge, abs(ref[2][0] - U[j]))
        accepted += bool(U[j] < ref[2][0])
        err = compare((smp[j:j + 1], lp[j:j + 1], acc[j:j + 1]), ref)
        if worst_bar == 0.0 or err / bar > worst / worst_bar:
            worst, worst_bar = err, bar
        assert err <= bar, (tag, j, err, bar, sens)
    print(f"resident warm-up transitions [{tag}]: worst err {worst:.3e} at bar {worst_bar:.3e}; accepted {accepted}/{n}; a == 0: {int(np.sum(acc == 0))}, "
          f"a == 1: {int(np.sum(acc == 1))}; eps {steps.min():.4g} ... {steps.max():.4g}; min |u - a| {edge:.1e}")
    assert edge > EDGE                                   # no accept decision of the reference sits on the edge
    assert 0 < accepted


def check_recurrence(tag, acc, steps, eps_final):
    """case 2"""
    s64, e64 = recurrence(acc, EPS0, TARGET, np.float64)
    sld, eld = recurrence(acc, EPS0, TARGET, np.longdouble)
    own = max(relmax(s64, sld), relmax(e64, eld))
    bar = 100.0 * max(own, EPS64)
    err = max(relmax(steps, s64), relmax(eps_final, e64))
    print(f"resident warm-up recurrence [{tag}]: err {err:.3e}  float64 vs longdouble {own:.3e}  bar {bar:.3e}  eps_final {eps_final:.6g}")
    assert steps[0] == EPS0
    assert err <= bar


def body_every_transition(npde, face, precision, n, L):
    w = warmup_run(npde, face, precision, n, L)
    check_transitions(f"{precision} n={n} L={L}", w.eng, w.stds, w.nn, w.priors, w.th0, (w.smp, w.acc, w.lp, w.steps, w.eps_final, w.minv), w.Z, w.U, L)


def body_recurrence(npde, face, precision, n, L):
    w = warmup_run(npde, face, precision, n, L)
    check_recurrence(f"{precision} n={n} L={L}", w.acc, w.steps, w.eps_final)


def body_metric(npde, face, precision, n, L):
    """case 3: the metric from the returned rows; the chain sits at the last draw; the handle holds the metric"""
    w = warmup_run(npde, face, precision, n, L)
    w0, w1, event = window(n)
    assert event
    m64, mld = window_metric(w.smp[w0:w1], np.float64), window_metric(w.smp[w0:w1], np.longdouble)
    own = relmax(m64, mld)
    bar = 100.0 * max(own, EPS64)
    err = relmax(w.minv, m64)
    print(f"resident warm-up metric [{precision} n={n} L={L}]: err {err:.3e}  float64 vs longdouble {own:.3e}  bar {bar:.3e}  "
          f"minv {w.minv.min():.3e} ... {w.minv.max():.3e}")
    assert err <= bar
    assert np.array_equal(w.state[0], w.smp[-1]) and w.state[1] == w.lp[-1]
    # one further draw with the returned metric (the other cases read the run's outputs and evaluate on its handle; none reads its chain)
    rng = np.random.default_rng(12)
    mom, uni = (rng.standard_normal(w.eng.P) / np.sqrt(w.minv))[None, :], rng.random(1)
    ref, sens, tbar = bar_of(w.eng, w.stds, w.nn, w.priors, w.smp[-1], w.minv, mom, uni, L, w.eps_final)
    assert abs(ref[2][0] - uni[0]) > EDGE
    th_now = w.eng.hmc_get()[0]
    assert np.array_equal(th_now, w.smp[-1])
    s, a, lp = w.eng.hmc_draws(1, L, w.eps_final, 0, mom, uni)
    err = compare((s, lp, a), ref)
    print(f"resident warm-up metric held [{precision} n={n} L={L}]: next draw err {err:.3e}  bar {tbar:.3e}  a {ref[2][0]:.4f}")
    assert err <= tbar


def body_no_metric_event(npde, precision, n):
    """case 4: short warm-ups keep the unit metric; n = 1 ends on the m > 0 average at once"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    Z, U = supplied(eng.P, n)
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    out = eng.hmc_warmup(n, 2, EPS0, TARGET, 0, Z, U)
    assert np.array_equal(out[5], np.ones(eng.P))
    check_transitions(f"{precision} n={n} L=2", eng, stds, nn, priors, th0, out, Z, U, 2)
    check_recurrence(f"{precision} n={n} L=2", out[1], out[3], out[4])
    assert np.array_equal(eng.hmc_get()[0], out[0][-1])


def body_generator(npde, precision):
    """case 5: NULL inputs draw from the generator of pinn_hmc_draws at the handle's counter, which the warm-up advances"""
    n, L = 100, 2
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.hmc_draws(2, L, EPS_STEP, GEN_SEED)              # counter 0, 1
    start = eng.hmc_get()[0]
    out = eng.hmc_warmup(n, L, EPS0, TARGET, GEN_SEED)
    zs, us = zip(*[gen_draw(GEN_SEED, 2 + j, eng.P) for j in range(n)])
    check_transitions(f"{precision} generator n={n} L={L}", eng, stds, nn, priors, start, out, np.asarray(zs), np.asarray(us), L)
    z, u = gen_draw(GEN_SEED, 2 + n, eng.P)
    ref, sens, bar = bar_of(eng, stds, nn, priors, out[0][-1], out[5], (z / np.sqrt(out[5]))[None, :], np.array([u]), L, out[4])
    assert abs(ref[2][0] - u) > EDGE
    s, a, lp = eng.hmc_draws(1, L, out[4], GEN_SEED)
    err = compare((s, lp, a), ref)
    print(f"resident warm-up generator [{precision}]: draw at counter {2 + n} err {err:.3e}  bar {bar:.3e}")
    assert err <= bar


def body_reproducibility(npde, precision):
    """case 6: fresh handles agree bit for bit; a used and re-initialised handle equals a fresh one; the Adam iterate is left alone"""
    n, L = 100, 2
    outs = []
    for used in (False, False, True):
        rep, th0, stds, nn, priors = forward_problem(npde, precision)
        eng = rep.engine
        Z, U = supplied(eng.P, n)
        if used:
            eng.loss_grad_f64(th0 + 0.1)
            eng.loglik_grad_f64(th0 - 0.1, stds)
            adam = eng.adam_f64 if precision == "f64" else eng.adam
            adam(th0 + 0.1, 3, 1e-3)
            eng.hmc_init(th0 + 0.05, stds, NN_PRIOR, [])
            eng.hmc_warmup(n, 1, 0.05, 0.7, 9)
            eng.hmc_find_stepsize(0.1, 3)
        eng.hmc_init(th0, stds, NN_PRIOR, [])
        out = eng.hmc_warmup(n, L, EPS0, TARGET, 0, Z, U)
        outs.append(list(out[:4]) + [np.float64(out[4]), out[5]] + list(eng.hmc_get()))
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    assert len(set(map(float, outs[0][1]))) > 1 and not np.array_equal(outs[0][5], np.ones(outs[0][5].size))
    # isolation (body_isolation's): an Adam run before a warm-up, its iterate after it
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    adam = eng.adam_f64 if precision == "f64" else eng.adam
    get = eng.adam_get_f64 if precision == "f64" else eng.adam_get
    it0, _ = adam(th0 + 0.1, 3, 1e-3)
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.hmc_find_stepsize(EPS0, 0, Z[0])
    eng.hmc_warmup(20, L, EPS0, TARGET, 0, Z[:20], U[:20])
    assert np.array_equal(get(), it0)


SEARCHES = (0.02, 0.1, 1e-4)


def body_search(npde, precision, eps0):
    """case 7: the search equals its numpy restatement exactly (trial values are eps0 times powers of two; the decisions have margin)"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    z = np.random.default_rng(21).standard_normal(eng.P)
    want_eps, want_trials, margin, hmax = search(eng, stds, nn, priors, th0, np.ones(eng.P), z, eps0)
    print(f"resident search [{precision} eps0={eps0}]: eps {want_eps:.6g} after {want_trials} trials; smallest |d - log 0.8| {margin:.3g}; |h0| {hmax:.4g}")
    assert margin >= 0.1                                 # against a disagreement of the two energy sums of at most 100 ulp(H) = 100 * 2^-52 * 1.6e3 = 4e-11
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    before = eng.hmc_get()
    eps, trials = eng.hmc_find_stepsize(eps0, 0, z)
    assert eps == want_eps and trials == want_trials
    after = eng.hmc_get()
    assert all(np.array_equal(a, b) for a, b in zip(after, before))
    gen = eng.hmc_find_stepsize(eps0, GEN_SEED)          # the generator's momentum: a fixed counter, so the same answer twice
    assert gen == eng.hmc_find_stepsize(eps0, GEN_SEED) and gen[0] > 0 and 1 <= gen[1] <= 41
    mine = eng.hmc_draws(3, 2, EPS_STEP, 5)
    rep2, _, _, _, _ = forward_problem(npde, precision)
    e2 = rep2.engine
    e2.hmc_init(th0, stds, NN_PRIOR, [])
    other = e2.hmc_draws(3, 2, EPS_STEP, 5)
    assert all(np.array_equal(a, b) for a, b in zip(mine + eng.hmc_get(), other + e2.hmc_get()))


def body_search_nonunit_metric(npde, precision):
    """the search under a metric that is not ones (r0 = z / sqrt(minv), the drift and the kinetic energy use it), and on the inverse problem"""
    rep, th0, stds, nn, priors = inverse_problem(npde, precision, "lognormal")
    eng = rep.engine
    z = np.random.default_rng(21).standard_normal(eng.P)
    minv = 0.25 + 1.5 * np.random.default_rng(5).random(eng.P)
    want_eps, want_trials, margin, _ = search(eng, stds, nn, priors, th0, minv, z, 0.02)
    print(f"resident search [{precision} inverse, metric]: eps {want_eps:.6g} after {want_trials} trials; smallest |d - log 0.8| {margin:.3g}")
    assert margin >= 1e-6
    eng.hmc_init(th0, stds, NN_PRIOR, kinds_of(priors))
    eng.hmc_set_metric(minv)
    assert eng.hmc_find_stepsize(0.02, 0, z) == (want_eps, want_trials)


MIRROR_KW = dict(n_leapfrog=3, phystd=[0.5], bcstd=[0.5])


def body_mirror(npde):
    """case 8, first half: adaptation="device" through ahmc_bayesian_pinn_pde"""
    sysm, chain, disc = small_problem(npde)
    kw = dict(draw_samples=1000, **MIRROR_KW)
    dev = npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", adaptation="device", seed=3, **kw)
    host = npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", adaptation="host", seed=3, **kw)
    dflt = npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", seed=3, **kw)
    assert set(dev.stats) == set(host.stats) and "adaptation" in dev.stats
    assert dev.stats["adaptation"] == "device" and host.stats["adaptation"] == "host" and dflt.stats["adaptation"] == "host"
    assert dev.samples.shape == (1000, 7) and dev.stats["n_adapts"] == 100 and dev.stats["acceptance"].shape == (1000,)
    assert np.array_equal(dev.samples[0], host.samples[0]) and dev.stats["acceptance"][0] == host.stats["acceptance"][0]
    assert dflt.samples.tobytes() == host.samples.tobytes() and dflt.stats["acceptance"].tobytes() == host.stats["acceptance"].tobytes()
    assert dflt.stats["step_size"] == host.stats["step_size"] and dflt.stats["inv_metric"].tobytes() == host.stats["inv_metric"].tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(dflt.ensemblesol + dflt.ensemblestd, host.ensemblesol + host.ensemblestd))
    assert not np.array_equal(dev.stats["inv_metric"], np.ones(7)) and dev.stats["step_size"] > 0
    with pytest.raises(ValueError, match="adaptation"):
        npde.ahmc_bayesian_pinn_pde(sysm, disc, adaptation="device", **kw)                       # the host sampler
    with pytest.raises(ValueError, match="adaptation"):
        npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", adaptation="gpu", **kw)


def body_known_target_device_adaptation(npde):
    """case 8, second half: body_known_target's comparison (tests/test_resident_hmc.py, its settings and bars) with adaptation="device"""
    sysm, chain, disc = small_problem(npde)
    kw = dict(draw_samples=2000, n_leapfrog=5, phystd=[0.5], bcstd=[0.5], priorsNNw=(0.0, 1.0))
    dev = npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", adaptation="device", seed=3, **kw)
    host = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(4), **kw)
    assert dev.stats["adaptation"] == "device" and dev.samples.shape == (2000, 7) and dev.stats["n_adapts"] == 200
    xs = np.array([0.0, 0.5, 1.0])

    def predict(sol):
        S = sol.samples[500:]
        W1, b1, W2, b2 = S[:, 0:2], S[:, 2:4], S[:, 4:6], S[:, 6]
        return np.stack([np.sum(W2 * np.tanh(W1 * x + b1), axis=1) + b2 for x in xs], axis=1)

    pd_, ph = predict(dev), predict(host)
    acc = dev.stats["acceptance"][200:].mean()
    print(f"resident warm-up known target: u(0, .5, 1) device mean {pd_.mean(axis=0)} sd {pd_.std(axis=0)}; host mean {ph.mean(axis=0)} sd {ph.std(axis=0)}; "
          f"acceptance device {acc:.3f} host {host.stats['acceptance'][200:].mean():.3f}; step size {dev.stats['step_size']:.4g} / {host.stats['step_size']:.4g}")
    assert np.all(np.abs(pd_.mean(axis=0) - ph.mean(axis=0)) < 0.25 * np.minimum(pd_.std(axis=0), ph.std(axis=0)))
    assert np.all(np.abs(pd_.std(axis=0) / ph.std(axis=0) - 1.0) < 0.25)
    assert 0.6 < acc <= 1.0


def body_refusals(npde, precision):
    """case 9: every refusal is named and leaves the handle evaluating, and the chain sitting, as before"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    L, dp = eng.L, C.POINTER(C.c_double)
    ev0 = eng.loglik_grad_f64(th0, stds)
    n = 4
    acc, lp, smp, steps, minv = np.zeros(n), np.zeros(n), np.zeros((n, eng.P)), np.zeros(n), np.zeros(eng.P)
    epsf, eps, nt = C.c_double(), C.c_double(), C.c_int()
    ptr = lambda a: a.ctypes.data_as(dp)

    def refused(rc, *words):
        assert rc != 0
        msg = L.last_error()
        assert all(w in msg for w in words), msg
        ev = eng.loglik_grad_f64(th0, stds)
        assert ev[0] == ev0[0] and np.array_equal(ev[1], ev0[1])

    def warm(na=n, nl=1, e0=0.1, tg=0.8, p=eng.P, a=ptr(acc), l=ptr(lp), ef=C.byref(epsf)):
        return L.lib.pinn_hmc_warmup(eng.h, na, nl, e0, tg, 0, None, None, ptr(smp), p, a, l, ptr(steps), ef, ptr(minv))

    def find(e0=0.1, p=eng.P, out=C.byref(eps)):
        return L.lib.pinn_hmc_find_stepsize(eng.h, e0, 0, None, p, out, C.byref(nt))

    refused(warm(), "pinn_hmc_warmup", "pinn_hmc_init first")
    refused(find(), "pinn_hmc_find_stepsize", "pinn_hmc_init first")
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    ref = eng.hmc_get()
    refused(warm(na=0), "pinn_hmc_warmup", "n_adapts")
    refused(warm(nl=0), "pinn_hmc_warmup", "n_leapfrog")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(warm(e0=bad), "pinn_hmc_warmup", "eps0")
        refused(find(e0=bad), "pinn_hmc_find_stepsize", "eps0")
    for bad in (0.0, 1.0, -0.2, 1.5, float("nan")):
        refused(warm(tg=bad), "pinn_hmc_warmup", "target")
    refused(warm(p=eng.P + 1), "pinn_hmc_warmup", "ntheta")
    refused(find(p=eng.P - 1), "pinn_hmc_find_stepsize", "ntheta")
    refused(warm(a=None), "pinn_hmc_warmup", "null argument")
    refused(warm(l=None), "pinn_hmc_warmup", "null argument")
    refused(warm(ef=None), "pinn_hmc_warmup", "null argument")
    refused(find(out=None), "pinn_hmc_find_stepsize", "null argument")
    eng.comm_init_custom(1, 0, lambda buf, count, dtype, stream: 0)
    refused(warm(), "pinn_hmc_warmup", "communicator")
    refused(find(), "pinn_hmc_find_stepsize", "communicator")
    eng.comm_destroy()
    now = eng.hmc_get()
    assert all(np.array_equal(a, b) for a, b in zip(now, ref))
    # nothing moved the draw counter or the metric either: the draws that follow are those of a handle that was never refused
    mine = eng.hmc_draws(2, 1, EPS_STEP, 7)
    rep2, _, _, _, _ = forward_problem(npde, precision)
    e2 = rep2.engine
    e2.hmc_init(th0, stds, NN_PRIOR, [])
    assert all(np.array_equal(a, b) for a, b in zip(mine, e2.hmc_draws(2, 1, EPS_STEP, 7)))
    eng.set_sampler(0, [0.0], [1.0], 11, seed=1)
    ev0 = eng.loglik_grad_f64(th0, stds)
    refused(warm(), "pinn_hmc_warmup", "fixed")
    refused(find(), "pinn_hmc_find_stepsize", "fixed")


# ------------------------------------------------------------------------------------------------------------------------------------
# the two faces of every body
# ------------------------------------------------------------------------------------------------------------------------------------
WARMUPS = [(p, n, L) for p in PRECISIONS for (n, L) in RUNS]


@pytest.mark.parametrize("precision,n,L", WARMUPS)
def test_every_transition(npde, use_emu, precision, n, L):
    body_every_transition(npde, "emu", precision, n, L)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,n,L", WARMUPS)
def test_every_transition_gpu(npde, hip_lib, precision, n, L):
    body_every_transition(npde, "hip", precision, n, L)


@pytest.mark.parametrize("precision,n,L", WARMUPS)
def test_recurrence(npde, use_emu, precision, n, L):
    body_recurrence(npde, "emu", precision, n, L)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,n,L", WARMUPS)
def test_recurrence_gpu(npde, hip_lib, precision, n, L):
    body_recurrence(npde, "hip", precision, n, L)


@pytest.mark.parametrize("precision,n,L", WARMUPS)
def test_metric(npde, use_emu, precision, n, L):
    body_metric(npde, "emu", precision, n, L)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,n,L", WARMUPS)
def test_metric_gpu(npde, hip_lib, precision, n, L):
    body_metric(npde, "hip", precision, n, L)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", SHORT)
def test_no_metric_event(npde, use_emu, precision, n):
    body_no_metric_event(npde, precision, n)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", SHORT)
def test_no_metric_event_gpu(npde, hip_lib, precision, n):
    body_no_metric_event(npde, precision, n)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_generator(npde, use_emu, precision):
    body_generator(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_generator_gpu(npde, hip_lib, precision):
    body_generator(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_reproducibility_and_isolation(npde, use_emu, precision):
    body_reproducibility(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_reproducibility_and_isolation_gpu(npde, hip_lib, precision):
    body_reproducibility(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("eps0", SEARCHES)
def test_search(npde, use_emu, precision, eps0):
    body_search(npde, precision, eps0)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("eps0", SEARCHES)
def test_search_gpu(npde, hip_lib, precision, eps0):
    body_search(npde, precision, eps0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_search_nonunit_metric(npde, use_emu, precision):
    body_search_nonunit_metric(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_search_nonunit_metric_gpu(npde, hip_lib, precision):
    body_search_nonunit_metric(npde, precision)


def test_mirror(npde, use_emu):
    body_mirror(npde)


@pytest.mark.gpu
def test_mirror_gpu(npde, hip_lib):
    body_mirror(npde)


def test_known_target_device_adaptation(npde, use_emu):
    body_known_target_device_adaptation(npde)


@pytest.mark.gpu
def test_known_target_device_adaptation_gpu(npde, hip_lib):
    body_known_target_device_adaptation(npde)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(npde, use_emu, precision):
    body_refusals(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_gpu(npde, hip_lib, precision):
    body_refusals(npde, precision)
