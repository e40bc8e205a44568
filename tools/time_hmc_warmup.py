"""BPINN warm-up, microseconds per adaptation draw: the loop of `bpinn._hmc_device` with adaptation="host" (one `hmc_draws(1)` round trip per draw,
dual averaging and the windowed metric in numpy, `hmc_set_metric` at the metric event) against ONE `hmc_warmup` call (pinn_hmc_warmup, DESIGN.md
section 4.11), both from the same start with the same generator seed; and the initial step-size search on the host evaluation path against
`hmc_find_stepsize`.  Both paths run in the same process, alternating; --warm untimed runs of each, then the median of --reps.  Times are host
clock around work that ends in a synchronise (every path ends in a download).
  python tools/time_hmc_warmup.py [--reps 21] [--warm 3] [--adapts 150] [--only poisson|bpinn1d]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import sympy as sp
import pinn_import
npde = pinn_import.load()

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--adapts", type=int, default=150)
ap.add_argument("--only", default="")
args = ap.parse_args()

NN_PRIOR = (0.0, 1.0)


def poisson(prec):
    """forward Poisson, GridTraining(0.1) = 13 points, 1-16-16-1 (profiles/resident_hmc.txt section 3)"""
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(npde.Differential(x)(u(x))) + sp.pi ** 2 * sp.sin(sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0), npde.Eq(u(1.0), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    th = npde.initialparameters(np.random.default_rng(7), chain)
    return npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=th, precision=prec)), np.array([0.5, 0.3, 0.3])


def bpinn1d(prec):
    """reference 1-D BPINN, u' = cos(2 pi t) on [0, 2], GridTraining(0.01) = 202 points, 1-6-1"""
    (t,) = npde.parameters("t")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(t)(u(t)) - sp.cos(2 * sp.pi * t), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0)], [npde.In(t, npde.Interval(0.0, 2.0))], [t], [u(t)])
    chain = npde.Chain(npde.Dense(1, 6, "tanh"), npde.Dense(6, 1))
    th = npde.initialparameters(np.random.default_rng(100), chain)
    return npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.01), init_params=th, precision=prec)), np.array([0.01, 0.01])


def host_warmup(eng, n_adapts, n_leapfrog, eps, target, seed):
    """bpinn.py `_hmc_device`, its adaptation loop as it stands with adaptation="host" """
    mu, hbar, log_eps_bar, t0, gamma, kappa = np.log(10 * eps), 0.0, 0.0, 10.0, 0.05, 0.75
    w0, w1 = int(0.15 * n_adapts), int(0.9 * n_adapts)
    win, m_count = [], 0
    for it in range(n_adapts):
        smp, acc, _ = eng.hmc_draws(1, n_leapfrog, eps, seed)
        th, a = smp[0], float(acc[0])
        m_count += 1
        hbar = (1 - 1 / (m_count + t0)) * hbar + (target - a) / (m_count + t0)
        log_eps = mu - np.sqrt(m_count) / gamma * hbar
        eta = m_count ** (-kappa)
        log_eps_bar = eta * log_eps + (1 - eta) * log_eps_bar
        eps = float(np.exp(log_eps))
        if w0 <= it < w1:
            win.append(th)
        if it == w1 - 1 and len(win) >= 8 and n_adapts >= 100:
            k = len(win)
            eng.hmc_set_metric((k / (k + 5.0)) * np.var(np.asarray(win), axis=0) + 1e-3 * (5.0 / (k + 5.0)))
            mu, hbar, log_eps_bar, m_count = np.log(10 * eps), 0.0, 0.0, 0
        if it == n_adapts - 1:
            eps = float(np.exp(log_eps_bar)) if m_count > 0 else eps
    return eps


def host_search(eng, stds, th, z, eps):
    """bpinn.py `_hmc_device`, its initial search on the host evaluation path (unit metric, Normal weight prior) -> (eps, trials)"""
    mu0, sd0 = NN_PRIOR

    def logp_grad(t):
        ll, g, _ = eng.loglik_grad_f64(t, stds)
        g = g.astype(np.float64)
        return ll - 0.5 * np.sum(((t - mu0) / sd0) ** 2) - t.size * (np.log(sd0) + 0.5 * np.log(2 * np.pi)), g - (t - mu0) / sd0 ** 2
    lp, g = logp_grad(th)

    def one_step(r, e):
        r = r + 0.5 * e * g
        lp1, g1 = logp_grad(th + e * r)
        r = r + 0.5 * e * g1
        return -lp1 + 0.5 * np.sum(r * r)
    h0 = -lp + 0.5 * np.sum(z * z)
    with np.errstate(all="ignore"):
        d = h0 - one_step(z, eps)
        direction, trials = (1.0 if (np.isfinite(d) and d > np.log(0.8)) else -1.0), 1
        for _ in range(40):
            eps *= 2.0 ** direction
            d = h0 - one_step(z, eps)
            trials += 1
            if not np.isfinite(d):
                d = -np.inf
            if (direction > 0) == (d <= np.log(0.8)):
                break
    return eps, trials


def alternate(fa, fb, prepare):
    """medians (seconds) of fa and fb, alternating, each after an untimed prepare()"""
    ta, tb = [], []
    for i in range(args.warm + args.reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            prepare()
            t0 = time.perf_counter()
            fn()
            if i >= args.warm:
                ts.append(time.perf_counter() - t0)
    return float(np.median(ta)), float(np.median(tb))


for name, make in (("poisson", poisson), ("bpinn1d", bpinn1d)):
    if args.only and args.only != name:
        continue
    for prec in ("f64", "f32"):
        rep, stds = make(prec)
        eng = rep.engine
        th0 = np.asarray(rep.flat_init_params, dtype=np.float64).copy()
        prepare = lambda: eng.hmc_init(th0, stds, NN_PRIOR, [])
        z = np.random.default_rng(21).standard_normal(eng.P)
        prepare()
        eps_h, tr_h = host_search(eng, stds, th0, z, 0.1)
        eps_d, tr_d = eng.hmc_find_stepsize(0.1, 0, z)
        t_h, t_d = alternate(lambda: host_search(eng, stds, th0, z, 0.1), lambda: eng.hmc_find_stepsize(0.1, 0, z), prepare)
        print(f"{name:8s} {prec} P={eng.P:4d} search from 0.1: host eps {eps_h:.6g} in {tr_h} trials {1e6 * t_h:9.1f} us   device eps {eps_d:.6g} in {tr_d} trials "
              f"{1e6 * t_d:9.1f} us   x{t_h / t_d:5.2f}", flush=True)
        for steps in (5, 30):
            n = args.adapts
            t_h, t_d = alternate(lambda: host_warmup(eng, n, steps, eps_d, 0.8, 1), lambda: eng.hmc_warmup(n, steps, eps_d, 0.8, 1), prepare)
            prepare(); e_h = host_warmup(eng, n, steps, eps_d, 0.8, 1)
            prepare(); e_d = eng.hmc_warmup(n, steps, eps_d, 0.8, 1)[4]
            print(f"{name:8s} {prec} P={eng.P:4d} n_adapts={n} steps={steps:2d}: host adaptation {1e6 * t_h / n:8.1f} us/draw   hmc_warmup {1e6 * t_d / n:8.1f} us/draw   "
                  f"x{t_h / t_d:5.2f}   final eps host {e_h:.4g} device {e_d:.4g}", flush=True)
