"""Dense Euclidean metric of the resident HMC sampler (`pinn_hmc_set_metric_dense`): r = L^-T z, theta += eps M^-1 r,
kinetic energy 1/2 r.(M^-1 r), and the warm-up's windowed covariance with its on-device Cholesky factorisation.

Problems, `make_logp`, `relerr`, the generator and the bar's rule are those of tests/test_resident_hmc.py; the warm-up is checked piecewise by the
method of tests/test_resident_hmc_warmup.py (its `window`, `supplied`, `check_recurrence`).  The reference is `restate` below: test_resident_hmc's
draw loop with `minv * r` replaced by `Minv @ r`, numpy's own Cholesky factor and triangular solve, driven by the same handle's `loglik_grad_f64`.
Every body is written once and exposed twice: on the CPU emulation (`use_emu`) and, marked `gpu`, on the product library (`hip_lib`).

THE BAR (cases 1, 2, 4) is test_resident_hmc.bar_of's: min(1e-9, 100 max(s, q)), q = 2^-52 max|H|, s = the restatement against itself with its sums
(energy sums and every row of Minv @ r) in reversed order.  For generated momenta s also includes the restatement run with a second lower factor
L2 of the same matrix computed along another route: the Cholesky factor of M^-1 in reversed row and column order, permuted back (an UPPER factor
U, M^-1 = U U^T), brought to lower form by the QR factorisation of U^T.  (U itself is a different square root: U^-T z is another momentum, not a
perturbed one.)  Case 3's L L^T bar is numpy's own residual x 100, floored at 2^-52 P.  Measured figures: profiles/resident_hmc_dense.txt."""
import numpy as np
import pytest

from test_resident_hmc import (EPS64, EPS_LONG, EPS_STEP, GEN_SEED, NN_PRIOR, PRECISIONS, compare, forward_problem, gen_draw, inverse_problem, kinds_of,
                               make_logp, relerr, small_problem)
from test_resident_hmc_warmup import EDGE, EPS0, TARGET, check_recurrence, supplied, window


def dense_metric(P, seed=3):
    """B B^T / P + D, B standard normal, D diagonal in [0.5, 1.5]; condition number below 50 (asserted)"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((P, P))
    M = B @ B.T / P + np.diag(0.5 + rng.random(P))
    M = 0.5 * (M + M.T)
    assert np.linalg.cond(M) < 50.0
    return M


def second_factor(M):
    U = np.linalg.cholesky(M[::-1, ::-1])[::-1, ::-1]
    R = np.linalg.qr(U.T)[1]
    return (R * np.sign(np.diag(R))[:, None]).T


def restate(eng, stds, nn, priors, th0, Minv, momenta, uniforms, n_leapfrog, eps, rev=False, state=None):
    """test_resident_hmc.restate under a dense metric -> samples, logp, accept_prob, h_new per draw, final state (th, lp, g)"""
    logp_grad, sm = make_logp(eng, stds, nn, priors, rev)
    mv = (lambda r: Minv[:, ::-1] @ r[::-1]) if rev else (lambda r: Minv @ r)
    th, lp, g = state if state is not None else (th0.astype(np.float64).copy(),) + logp_grad(th0.astype(np.float64))
    S, L, A, HN = [], [], [], []
    with np.errstate(all="ignore"):
        for r, u in zip(momenta, uniforms):
            h_old = -lp + 0.5 * sm(r * mv(r))
            tn, rn, gn = th, r + 0.5 * eps * g, g
            for s in range(n_leapfrog):
                tn = tn + eps * mv(rn)
                lpn, gn = logp_grad(tn)
                rn = rn + (eps if s < n_leapfrog - 1 else 0.5 * eps) * gn
            h_new = -lpn + 0.5 * sm(rn * mv(rn))
            a = float(np.exp(min(0.0, h_old - h_new))) if np.isfinite(h_new) else 0.0
            if u < a:
                th, lp, g = tn, lpn, gn
            S.append(th.copy()); L.append(lp); A.append(a); HN.append(h_new)
    return np.asarray(S), np.asarray(L), np.asarray(A), np.asarray(HN), (th, lp, g)


def bar_of(eng, stds, nn, priors, th0, Minv, mom, uni, n_leapfrog, eps, normals=None, state=None):
    """-> reference, s, q, bar.  normals: the momenta are L^-T z of these; the second factor's run then enters s"""
    args = (eng, stds, nn, priors, th0, Minv)
    fwd = restate(*args, mom, uni, n_leapfrog, eps, state=state)
    sens = compare(restate(*args, mom, uni, n_leapfrog, eps, rev=True, state=state), fwd)
    if normals is not None:
        sens = max(sens, compare(restate(*args, np.linalg.solve(second_factor(Minv).T, normals.T).T, uni, n_leapfrog, eps, state=state), fwd))
    h = np.concatenate([fwd[3][np.isfinite(fwd[3])], fwd[1][np.isfinite(fwd[1])]])
    q = EPS64 * float(np.max(np.abs(h)))
    return fwd, sens, q, min(1e-9, 100.0 * max(sens, q))


def problem(npde, kind, precision):
    return forward_problem(npde, precision) if kind == "forward" else inverse_problem(npde, precision, "lognormal")


def draws(eng, *args):
    smp, acc, lp = eng.hmc_draws(*args)
    return smp, lp, acc


def body_transitions(npde, precision, kind, n_leapfrog):
    """case 1: 4 draws with supplied momenta and uniforms, then 4 from the device generator, and the final state"""
    rep, th0, stds, nn, priors = problem(npde, kind, precision)
    eng = rep.engine
    P = eng.P
    Minv = dense_metric(P)
    Lnp = np.linalg.cholesky(Minv)
    eps = EPS_LONG if n_leapfrog == 5 else EPS_STEP
    rng = np.random.default_rng(11 + n_leapfrog)
    mom, uni = np.linalg.solve(Lnp.T, rng.standard_normal((4, P)).T).T, rng.random(4)
    ref, sens, q, bar = bar_of(eng, stds, nn, priors, th0, Minv, mom, uni, n_leapfrog, eps)
    eng.hmc_init(th0, stds, NN_PRIOR, kinds_of(priors))
    eng.hmc_set_metric_dense(Minv)
    err = compare(draws(eng, 4, n_leapfrog, eps, 0, mom, uni), ref)
    print(f"dense hmc supplied [{precision} {kind} L={n_leapfrog}]: err {err:.3e}  s {sens:.3e}  q {q:.3e}  bar {bar:.3e}  a = {np.round(ref[2], 4)}")
    assert 0.0 < ref[2].max() <= 1.0
    assert err <= bar, f"error {err:.3e} is {err / bar:.2f} x the bar {bar:.3e}"
    th, lp, g = eng.hmc_get()
    assert relerr(th, ref[4][0]) <= bar and relerr(lp, ref[4][1]) <= bar and relerr(g, ref[4][2]) <= bar
    # the generator: counters 4..7 (supplied draws advance it too), from the restatement's own state after the first call
    zs, us = zip(*[gen_draw(GEN_SEED, 4 + c, P) for c in range(4)])
    zs, us = np.asarray(zs), np.asarray(us)
    gref, gs, _, gbar = bar_of(eng, stds, nn, priors, th0, Minv, np.linalg.solve(Lnp.T, zs.T).T, us, n_leapfrog, eps, normals=zs, state=ref[4])
    assert np.all(np.abs(gref[2] - us) > EDGE), (gref[2], us)
    gerr = compare(draws(eng, 4, n_leapfrog, eps, GEN_SEED), gref)
    print(f"dense hmc generator [{precision} {kind} L={n_leapfrog}]: err {gerr:.3e}  s {gs:.3e}  bar {gbar:.3e}  a = {np.round(gref[2], 4)}")
    assert gerr <= gbar, f"error {gerr:.3e} is {gerr / gbar:.2f} x the bar {gbar:.3e}"


def body_diagonal_agreement(npde, precision):
    """case 2: set_metric_dense(diag(m)) against set_metric(m)"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    m = 0.25 + 1.5 * np.random.default_rng(5).random(eng.P)
    rng = np.random.default_rng(17)
    mom, uni = rng.standard_normal((4, eng.P)) / np.sqrt(m), rng.random(4)
    ref, sens, q, bar = bar_of(eng, stds, nn, priors, th0, np.diag(m), mom, uni, 2, EPS_STEP)
    out = []
    for dense in (False, True):
        eng.hmc_init(th0, stds, NN_PRIOR, [])
        eng.hmc_set_metric_dense(np.diag(m)) if dense else eng.hmc_set_metric(m)
        out.append(draws(eng, 4, 2, EPS_STEP, 0, mom, uni))
    err = max(compare(out[1], out[0]), compare(out[1], ref))
    print(f"dense hmc diagonal agreement [{precision}]: err {err:.3e}  bar {bar:.3e}")
    assert err <= bar


def body_factor_and_refusals(npde, precision):
    """case 3"""
    from neuralpde_jl_amd._lib import EngineError
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    P = eng.P
    Minv = dense_metric(P)
    Lnp = np.linalg.cholesky(Minv)
    with pytest.raises(EngineError, match="pinn_hmc_init first"):
        eng.hmc_set_metric_dense(Minv)
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    fresh = eng.hmc_draws(2, 2, EPS_STEP, 7)
    with pytest.raises(EngineError, match="diagonal metric"):
        eng.hmc_get_metric_dense()
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.hmc_set_metric_dense(Minv)
    M, L = eng.hmc_get_metric_dense()
    scale = float(np.max(np.abs(Minv)))
    bar = max(100.0 * float(np.max(np.abs(Lnp @ Lnp.T - Minv))) / scale, EPS64 * P)
    err = float(np.max(np.abs(L @ L.T - Minv))) / scale
    print(f"dense hmc factor [{precision}]: |L L^T - M^-1| / |M^-1| {err:.3e}  bar {bar:.3e}  |L - L_numpy| {relerr(L, Lnp):.3e}")
    assert np.array_equal(M, Minv) and np.all(np.triu(L, 1) == 0.0) and np.all(np.diag(L) > 0.0)
    assert err <= bar
    w, V = np.linalg.eigh(Minv)
    w[P // 2] = -w[P // 2]
    indefinite = (V * w) @ V.T
    asym = Minv.copy()
    asym[3, 200] += 1e-6
    bad = [(0.5 * (indefinite + indefinite.T), "pivot"), (asym, "symmetric"), (Minv[:-1, :-1], "ntheta"), (np.where(np.eye(P) > 0, np.nan, Minv), "non-finite")]
    for mat, word in bad:
        with pytest.raises(EngineError, match=word):
            eng.hmc_set_metric_dense(mat)
    with pytest.raises(EngineError, match="dense metric"):
        eng.nuts_draws(1, 2, EPS_STEP)
    with pytest.raises(EngineError, match="dense metric"):
        eng.hmc_chains_init(th0[None, :], EPS_STEP, stds)
    M2, L2 = eng.hmc_get_metric_dense()
    assert np.array_equal(M2, M) and np.array_equal(L2, L)
    mine = eng.hmc_draws(2, 2, EPS_STEP, 7)
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.hmc_set_metric_dense(Minv)
    assert all(np.array_equal(a, b) for a, b in zip(mine, eng.hmc_draws(2, 2, EPS_STEP, 7)))      # the refusals left metric and chain alone
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.hmc_set_metric_dense(Minv)
    eng.hmc_set_metric(None)                             # back to today's diagonal behaviour
    assert all(np.array_equal(a, b) for a, b in zip(fresh, eng.hmc_draws(2, 2, EPS_STEP, 7)))


def body_cap_and_keywords(npde):
    """case 3, the rest: P above the cap is refused at the call; the Python keyword's refusals"""
    from neuralpde_jl_amd._lib import EngineError
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    sysm = npde.PDESystem([npde.Eq(u(x), 2 * x + 1)], [npde.Eq(u(0.0), 1.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 64, "tanh"), npde.Dense(64, 64, "tanh"), npde.Dense(64, 1))      # P = 4353 > 4096
    theta0 = npde.initialparameters(np.random.default_rng(2), chain)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=theta0, precision="f32"))
    eng = rep.engine
    assert eng.P > 4096
    eng.hmc_init(np.asarray(rep.flat_init_params, dtype=np.float64), np.array([0.5, 0.5]), NN_PRIOR, [])
    with pytest.raises(EngineError, match="4096"):
        eng.hmc_set_metric_dense(None)                   # (NULL: nothing of size P x P exists on either side)
    sysm, chain, disc = small_problem(npde)
    kw = dict(draw_samples=20, n_leapfrog=3, phystd=[0.5], bcstd=[0.5], metric="dense")
    for extra in (dict(kernel="nuts"), dict(sampler="chains"), dict(metric="full")):
        with pytest.raises(ValueError, match="metric"):
            npde.ahmc_bayesian_pinn_pde(sysm, disc, **{**kw, **extra})


def body_warmup(npde, precision):
    """case 4: n_adapts = 100 (window 15..90: 75 draws, fewer than P, no multiple of 4), n_leapfrog = 3, piecewise as test_resident_hmc_warmup"""
    n, L = 100, 3
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    P = eng.P
    Z, U = supplied(P, n)
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.hmc_set_metric_dense(None)
    smp, acc, lp, steps, eps_final, diag = eng.hmc_warmup(n, L, EPS0, TARGET, 0, Z, U)
    assert not eng.metric_kept
    M, Lf = eng.hmc_get_metric_dense()
    w0, w1, event = window(n)
    assert event and w1 - w0 == 75
    # the metric from the returned rows: float64 against longdouble fixes the bar (max norm: a covariance entry near zero has no scale of its own)
    Wl = smp[w0:w1].astype(np.longdouble)
    mld = (75 / np.longdouble(80)) * ((Wl - Wl.mean(axis=0)).T @ (Wl - Wl.mean(axis=0)) / 75) + np.longdouble(1e-3) * (5 / np.longdouble(80)) * np.eye(P)
    m64 = (75 / 80.0) * np.cov(smp[w0:w1].T, bias=True) + 1e-3 * (5.0 / 80.0) * np.eye(P)
    own = relerr(m64, mld)
    mbar = 100.0 * max(own, EPS64)
    merr = relerr(M, m64)
    print(f"dense warm-up metric [{precision}]: err {merr:.3e}  float64 vs longdouble {own:.3e}  bar {mbar:.3e}  cond {np.linalg.cond(M):.3g}")
    assert merr <= mbar and np.array_equal(M, M.T) and np.array_equal(diag, np.diag(M))
    assert float(np.max(np.abs(Lf @ Lf.T - M))) / float(np.max(np.abs(M))) <= max(100.0 * relerr(np.linalg.cholesky(M) @ np.linalg.cholesky(M).T, M), EPS64 * P)
    check_recurrence(f"dense {precision}", acc, steps, eps_final)
    worst, edge = 0.0, np.inf
    for j in range(n):                                   # every draw alone, from the state before it, under the metric in force
        Minv = M if j > w1 - 1 else np.eye(P)
        mom = np.linalg.solve(np.linalg.cholesky(Minv).T, Z[j])[None, :]
        ref, sens, q, bar = bar_of(eng, stds, nn, priors, th0 if j == 0 else smp[j - 1], Minv, mom, U[j:j + 1], L, float(steps[j]), normals=Z[j:j + 1])
        err = compare((smp[j:j + 1], lp[j:j + 1], acc[j:j + 1]), ref)
        worst, edge = max(worst, err / bar), min(edge, abs(ref[2][0] - U[j]))
        assert err <= bar, (j, err, bar, sens)
    print(f"dense warm-up transitions [{precision}]: worst err / bar {worst:.3f}; min |u - a| {edge:.1e}; eps {steps.min():.4g} ... {steps.max():.4g}")
    assert edge > EDGE and np.array_equal(eng.hmc_get()[0], smp[-1])


def body_mirror(npde):
    """case 5: the keyword through ahmc_bayesian_pinn_pde; the existing mirror tests feed no common stream to host and device samplers, so
    adaptation="host" against adaptation="device" on the device sampler (test_resident_hmc_warmup.body_mirror's comparison)"""
    sysm, chain, disc = small_problem(npde)
    kw = dict(draw_samples=1000, n_leapfrog=3, phystd=[0.5], bcstd=[0.5], metric="dense")
    dev = npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", adaptation="device", seed=3, **kw)
    hst = npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", adaptation="host", seed=3, **kw)
    cpu = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), **{**kw, "draw_samples": 200})
    for sol in (dev, hst, cpu):
        M = sol.stats["inv_metric"]
        assert sol.stats["metric"] == "dense" and M.shape == (7, 7) and np.allclose(M, M.T) and np.all(np.linalg.eigvalsh(M) > 0)
    assert cpu.stats["inv_metric"].shape == (7, 7) and not np.array_equal(dev.stats["inv_metric"], np.eye(7))
    assert np.array_equal(dev.samples[0], hst.samples[0]) and dev.stats["acceptance"][0] == hst.stats["acceptance"][0]
    assert dev.samples.shape == (1000, 7) and 0.3 < dev.stats["acceptance"][100:].mean() <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------
# the two faces of every body: the CPU emulation, and (marked gpu) the product library
# ------------------------------------------------------------------------------------------------------------------------------------
FACES = pytest.mark.parametrize("face", ["use_emu", pytest.param("hip_lib", marks=pytest.mark.gpu)])
TRANSITIONS = [(p, k, n) for p in PRECISIONS for k in ("forward", "inverse") for n in (1, 5)]


@FACES
@pytest.mark.parametrize("precision,kind,n_leapfrog", TRANSITIONS)
def test_transitions(npde, request, face, precision, kind, n_leapfrog):
    request.getfixturevalue(face)
    body_transitions(npde, precision, kind, n_leapfrog)


@FACES
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("body", [body_diagonal_agreement, body_factor_and_refusals, body_warmup])
def test_per_precision(npde, request, face, body, precision):
    request.getfixturevalue(face)
    body(npde, precision)


@FACES
@pytest.mark.parametrize("body", [body_cap_and_keywords, body_mirror])
def test_interface(npde, request, face, body):
    request.getfixturevalue(face)
    body(npde)
