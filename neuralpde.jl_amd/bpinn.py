"""Physics log-likelihood of a Bayesian PINN on top of the engine's per-term sums.

The reference's BPINN (ext/bpinn/PDE_BPINN.jl:425) sums, over the PDE and boundary terms, the closures that
`get_points_loss_functions` builds for `GridTraining` (src/training_strategies.jl:113-127):

    l_k(theta, sigma_k) = logpdf(MvNormal(r_k(X_k; theta), sigma_k^2 I), 0)
                        = -N_k/2 log(2 pi) - N_k log(sigma_k) - SSE_k / (2 sigma_k^2),      SSE_k = sum_i r_k(x_i; theta)^2

i.e. an affine function of the per-term sums of squares the engine already returns (L_k = SSE_k / N_k), and

    grad_theta sum_k l_k = - grad_theta sum_k w_k L_k        with  w_k = N_k / (2 sigma_k^2),

which is one `pinn_loss_grad` call with those term weights (reverse mode over all P parameters, where the reference
uses forward-mode ForwardDiff over every parameter of the network).  By default the priors and the HMC sampler itself stay on the
host as in the reference (`sampler="host"`: one device evaluation and one host round trip per leapfrog step).  `sampler="device"` runs the
transitions on the device (`pinn_hmc_*`): theta, momentum, metric, gradient and energies stay resident, a call
makes many draws and downloads once; the step-size search, dual averaging and the windowed metric stay here in Python unless
`adaptation="device"` runs the whole warm-up in ONE resident call (`pinn_hmc_warmup`).  Every sampler here shares
one copy of each: `_find_stepsize` is the search, `_adapt_and_draw` the dual-averaging recurrence, the window and the chunked draws around a
sampler's `transition`, `_DiagMetric` / `_DenseMetric` (`_dense_window_metric`) the metric's arithmetic and its window rule.
`kernel="nuts"` replaces the fixed-length trajectory by No-U-Turn transitions (`_nuts_transition`, the specification; on the device
`pinn_nuts_draws`).
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np


def physics_loglikelihood(engine, theta, stds: Sequence[float], term_sizes: Sequence[int], want_grad: bool = True
                          ) -> Tuple[float, np.ndarray]:
    """sum_k logpdf(MvNormal(r_k, sigma_k^2 I), 0) and its gradient w.r.t. theta.
    stds: sigma_k per term (PDE terms first, then boundary terms: `allstd[1:2]` of the reference, flattened);
    term_sizes: N_k, the number of points of every term's (fixed) set."""
    sig = np.asarray(stds, dtype=np.float64)
    n = np.asarray(term_sizes, dtype=np.float64)
    if sig.shape != (engine.K,) or n.shape != (engine.K,):
        raise ValueError(f"need one std and one set size per loss term ({engine.K})")
    if np.any(sig <= 0):
        raise ValueError("standard deviations must be positive")
    w = n / (2.0 * sig ** 2)
    losses, grad = engine.loss_grad_f64(theta, w) if want_grad else (engine.loss_grad(theta, w, want_grad=False)[0], None)
    ll = float(np.sum(-0.5 * n * math.log(2.0 * math.pi) - n * np.log(sig) - w * np.asarray(losses, dtype=np.float64)))
    return ll, (None if grad is None else -np.asarray(grad, dtype=np.float64))


def loglikelihood(engine, theta, stds: Sequence[float], want_grad: bool = True):
    """The same log-likelihood through the engine's own entry point `pinn_loglik_grad`: returns (loglik, d/dtheta, d/dstds) — the stds
    as trailing sampler parameters (`allstd` of ext/bpinn/PDE_BPINN.jl:16-26 when they are not fixed).  Terms may include DataLoss
    terms: with their own std they are the L2LossData term (ext/bpinn/PDE_BPINN.jl:148-183), evaluated in the same fused call."""
    ll, g, gs = engine.loglik_grad_f64(theta, stds, want_grad=want_grad)      # (double at the ABI: native on a handle in float64 mode, fp32 kernels + widening otherwise)
    return ll, (None if g is None else g.astype(np.float64)), gs


# ------------------------------------------------------------------------------------------------
# host-side sampler: the mirror of `ahmc_bayesian_pinn_pde` (ext/bpinn/PDE_BPINN.jl:371-640)
# ------------------------------------------------------------------------------------------------
class BPINNsolution:
    """ext/bpinn/PDE_BPINN.jl `BPINNsolution`: samples, per-dependent-variable ensemble prediction (mean, std over the last `numensemble`
    draws) on the `saveats` grid, and that grid."""

    def __init__(self, samples, ensemblesol, ensemblestd, timepoints, stats):
        self.samples, self.ensemblesol, self.ensemblestd, self.timepoints, self.stats = samples, ensemblesol, ensemblestd, timepoints, stats


def _dense_window_metric(win):
    """the dense twin of the windowed variance rule: (k/(k+5)) cov + 1e-3 (5/(k+5)) I over the k window rows, and its lower Cholesky factor;
    None when the matrix is not positive definite (the metric in force stays)"""
    W = np.asarray(win)
    k = W.shape[0]
    Minv = (k / (k + 5.0)) * np.cov(W.T, bias=True) + 1e-3 * (5.0 / (k + 5.0)) * np.eye(W.shape[1])
    try:
        return Minv, np.linalg.cholesky(Minv)
    except np.linalg.LinAlgError:
        return None


class _DiagMetric:
    """diagonal Euclidean metric (DiagEuclideanMetric), `minv` the inverse mass vector: what a trajectory needs of a metric — the momentum of
    standard normals z, the position step M^-1 r, the kinetic energy — and the metric an adaptation window gives"""

    def __init__(self, minv):
        self.minv = minv

    def momentum(self, z):
        return z / np.sqrt(self.minv)

    def velocity(self, r):
        return self.minv * r

    def kinetic(self, r):
        return 0.5 * np.sum(self.minv * r * r)

    def from_window(self, win):
        """the windowed variance rule: (k/(k+5)) var + 1e-3 (5/(k+5)) over the k window rows"""
        var = np.var(np.asarray(win), axis=0)
        k = len(win)
        return _DiagMetric((k / (k + 5.0)) * var + 1e-3 * (5.0 / (k + 5.0)))


class _DenseMetric:
    """dense Euclidean metric (DenseEuclideanMetric), M^-1 = `minv` = L L^T with L = `chol`: r = L^-T z, theta += eps M^-1 r, kinetic energy
    1/2 r.(M^-1 r)"""

    def __init__(self, minv, chol):
        self.minv, self.chol = minv, chol

    def momentum(self, z):
        return np.linalg.solve(self.chol.T, z)

    def velocity(self, r):
        return self.minv @ r

    def kinetic(self, r):
        return 0.5 * (r @ (self.minv @ r))

    def from_window(self, win):
        """`_dense_window_metric`, or None (the metric in force stays)"""
        new = _dense_window_metric(win)
        return None if new is None else _DenseMetric(*new)


def _find_stepsize(logp_grad, th, lp, g, metric, eps, z):
    """the initial step-size search of every sampler here (AdvancedHMC.find_good_stepsize) from (th, lp, g), with the momentum `metric` makes of
    the standard normals z: double or halve eps until the acceptance of ONE leapfrog step crosses 0.8, at most 40 trials after the first"""
    r0 = metric.momentum(z)

    def one_step(e):
        r = r0 + 0.5 * e * g
        lp1, g1 = logp_grad(th + e * metric.velocity(r))
        r = r + 0.5 * e * g1
        return -lp1 + metric.kinetic(r)

    h0 = -lp + metric.kinetic(r0)
    d = h0 - one_step(eps)
    direction = 1.0 if (np.isfinite(d) and d > np.log(0.8)) else -1.0
    for _ in range(40):
        eps *= 2.0 ** direction
        d = h0 - one_step(eps)
        if not np.isfinite(d):
            d = -np.inf
        if (direction > 0) == (d <= np.log(0.8)):
            break
    return eps


def _chunks(n, chunk=256):
    """the sizes of the calls that make n draws after the adaptation: `chunk` draws each, the last one the rest"""
    while n > 0:
        nd = min(int(chunk), n)
        yield nd
        n -= nd


def _adapt_and_draw(transition, metric, eps, target, draw_samples, n_adapts, set_metric=None, chunk=256):
    """The warm-up and the draws of every sampler here, from the step size of `_find_stepsize`.  transition(n, eps, metric) runs n draws of the
    chain and returns one row (th, acceptance, ...) per draw, th the chain's state after accept/reject.  The first n_adapts draws, one per call,
    adapt Stan-style (StanHMCAdaptor): dual averaging of the step size towards `target` acceptance after every draw and, at the end of the window
    [0.15 n_adapts, 0.9 n_adapts), a metric from the window's rows (`metric.from_window`), which set_metric(minv) tells the device about; the dual
    averaging restarts on it, and the last adaptation draw fixes the step size at the averaged one.  The remaining draws come in calls of `chunk`.
    -> rows, step size, metric."""
    mu, hbar, log_eps_bar, t0, gamma, kappa = np.log(10 * eps), 0.0, 0.0, 10.0, 0.05, 0.75
    w0, w1 = int(0.15 * n_adapts), int(0.9 * n_adapts)            # variance window of the metric adaptation
    win, rows = [], []
    m_count = 0
    for it in range(min(n_adapts, draw_samples)):
        row = transition(1, eps, metric)[0]
        rows.append(row)
        a = float(row[1])
        m_count += 1
        hbar = (1 - 1 / (m_count + t0)) * hbar + (target - a) / (m_count + t0)
        log_eps = mu - np.sqrt(m_count) / gamma * hbar
        eta = m_count ** (-kappa)
        log_eps_bar = eta * log_eps + (1 - eta) * log_eps_bar
        eps = float(np.exp(log_eps))
        if w0 <= it < w1:
            win.append(row[0])
        if it == w1 - 1 and len(win) >= 8 and n_adapts >= 100:       # (a metric from fewer draws is noise; short runs keep the unit metric)
            new = metric.from_window(win)
            if new is not None:
                metric = new
                if set_metric is not None:
                    set_metric(metric.minv)
            mu, hbar, log_eps_bar, m_count = np.log(10 * eps), 0.0, 0.0, 0          # restart the step-size search on the new metric
        if it == n_adapts - 1:
            eps = float(np.exp(log_eps_bar)) if m_count > 0 else eps
    for nd in _chunks(draw_samples - len(rows), chunk):
        rows.extend(transition(nd, eps, metric))
    return rows, eps, metric


def _stats(rows, eps, minv, n_adapts):
    """-> samples, stats: the columns every sampler has"""
    col = lambda j: np.asarray([r[j] for r in rows], dtype=np.float64)
    return col(0), {"acceptance": col(1), "step_size": eps, "inv_metric": minv, "n_adapts": n_adapts}


def _hmc(logp_grad, theta0, draw_samples, n_leapfrog, eps0, target, rng, n_adapts=None, metric="diag"):
    """HMC with `n_leapfrog` leapfrog steps per draw ([3P] AdvancedHMC.HMC(eps, n_leapfrog)), Stan-style adaptation during the first
    n_adapts = min(draw_samples / 10, 1000) draws (AdvancedHMC's default, `_adapt_and_draw`): dual averaging of the step size towards `target`
    acceptance and a diagonal metric from the windowed sample variance (StanHMCAdaptor + DiagEuclideanMetric).  metric="dense": a full inverse
    metric M^-1 = L L^T from the windowed covariance (`_DenseMetric`)."""
    n = theta0.size
    n_adapts = min(draw_samples // 10, 1000) if n_adapts is None else n_adapts
    th = theta0.astype(np.float64).copy()
    lp, g = logp_grad(th)
    met = _DenseMetric(np.eye(n), np.eye(n)) if metric == "dense" else _DiagMetric(np.ones(n))
    eps = _find_stepsize(logp_grad, th, lp, g, met, eps0, rng.standard_normal(n))

    def leap(th, r, g, eps, steps, met):
        r = r + 0.5 * eps * g
        for s in range(steps):
            th = th + eps * met.velocity(r)
            lp, g = logp_grad(th)
            r = r + (eps if s < steps - 1 else 0.5 * eps) * g
        return th, r, lp, g

    def transition(nd, eps, met):
        nonlocal th, lp, g
        out = []
        for _ in range(nd):
            r = met.momentum(rng.standard_normal(n))
            h_old = -lp + met.kinetic(r)
            tn, rn, lpn, gn = leap(th, r, g, eps, n_leapfrog, met)
            h_new = -lpn + met.kinetic(rn)
            a = float(np.exp(min(0.0, h_old - h_new))) if np.isfinite(h_new) else 0.0
            if rng.random() < a:
                th, lp, g = tn, lpn, gn
            out.append((th.copy(), a))
        return out
    rows, eps, met = _adapt_and_draw(transition, met, eps, target, draw_samples, n_adapts)
    return _stats(rows, eps, met.minv, n_adapts)


def _hmc_device(eng, logp_grad, theta0, init_chain, draw_samples, n_leapfrog, eps0, target, rng, seed, n_adapts=None, chunk=256, adaptation="host",
                metric="diag"):
    """`_hmc` with the transitions on the device (Engine.hmc_*): the same initial step-size search on the host evaluation path (`_find_stepsize`,
    at most 42 evaluations), the same dual averaging and windowed metric (`_adapt_and_draw`) around `hmc_draws(1, ...)` during adaptation (a new
    metric goes down through `hmc_set_metric`), then the remaining draws in chunks of `chunk`.  Momenta and uniforms come from the device generator (`seed`).
    adaptation="device": the adaptation draws are ONE `hmc_warmup` call — the same recurrence and window on the device — after the same host
    search, so both settings start from the same step size.  metric="dense": the chain starts under the dense identity
    (`hmc_set_metric_dense`); the host adaptation sends the windowed covariance down through it, the device adaptation forms and factorises it
    in the `hmc_warmup` call; stats["inv_metric"] is then P x P."""
    n = theta0.size
    n_adapts = min(draw_samples // 10, 1000) if n_adapts is None else n_adapts
    th = theta0.astype(np.float64).copy()
    lp, g = logp_grad(th)
    met = _DiagMetric(np.ones(n))
    dense = metric == "dense"
    eps = _find_stepsize(logp_grad, th, lp, g, met, eps0, rng.standard_normal(n))
    init_chain(th)
    if dense:                                        # (the search above ran under the unit metric, which the dense identity is)
        eng.hmc_set_metric_dense(None)
        met = _DenseMetric(np.eye(n), np.eye(n))

    def transition(nd, eps, met):
        smp, acc, _ = eng.hmc_draws(nd, n_leapfrog, eps, seed)
        return list(zip(smp, acc))
    if adaptation == "device" and min(n_adapts, draw_samples) >= 1:
        if n_adapts > draw_samples:
            raise ValueError("adaptation=\"device\": the warm-up is one call of n_adapts draws; draw_samples must be at least n_adapts")
        smp, acc, _, _, eps, minv = eng.hmc_warmup(n_adapts, n_leapfrog, eps, target, seed)
        if dense:
            minv = eng.hmc_get_metric_dense()[0]
        rows = list(zip(smp, acc))
        for nd in _chunks(draw_samples - n_adapts, chunk):
            rows.extend(transition(nd, eps, None))
        return _stats(rows, eps, minv, n_adapts)
    rows, eps, met = _adapt_and_draw(transition, met, eps, target, draw_samples, n_adapts, eng.hmc_set_metric_dense if dense else eng.hmc_set_metric, chunk)
    return _stats(rows, eps, met.minv, n_adapts)


# ------------------------------------------------------------------------------------------------
# NUTS: multinomial No-U-Turn transitions with the generalised U-turn criterion, iterative form
# ------------------------------------------------------------------------------------------------
def _logaddexp(a, b):
    m = a if a > b else b
    if m == -math.inf:
        return -math.inf
    return m + math.log1p(math.exp(-abs(a - b)))


def _exp(x):
    return math.exp(x) if x < 709.0 else math.inf       # (a weight ratio may overflow: the comparison u < inf is what matters)


def nuts_uniforms(max_depth):
    """length of a draw's row of uniforms: [u_dir[0..D) | u_merge[0..D) | u_leaf[0 .. 2^D - 1)]"""
    return 2 * int(max_depth) + (1 << int(max_depth)) - 1


def _nuts_transition(logp_grad, state, minv, eps, z, u, max_depth, delta_max=1000.0, *, sum_fn=np.sum, trace=None):
    """ONE No-U-Turn transition from state = (th, lp, g), g = grad logp, under the diagonal inverse metric `minv`, with all its randomness
    supplied: z = P standard normals, u = `nuts_uniforms(max_depth)` uniforms.  -> (th, lp, g), stats.  This function is the specification:
    the host sampler's transition, the tests' restatement, and the text csrc/nuts_kernels.hpp restates operation by operation.
    Conventions are `_hmc`'s: H = -logp + 1/2 sum minv r^2; a leapfrog of signed step s = v eps is r += s/2 g; th += s minv r; evaluate;
    r += s/2 g.  A doubling at depth d builds 2^d leaves outward from the right (v = +1, u_dir[d] < 0.5) or the left edge; per leaf:
    delta = H0 - H (-inf if not finite), sum_acc += exp(min(0, delta)), divergence if not -delta <= delta_max, progressive multinomial
    sampling of the subtree's candidate, the momentum sum, a checkpoint (r, rho_sub) at index popcount(n) when n is even and the U-turn
    checks of every sub-tree that ends at an odd n against the checkpoints.  A subtree that diverges or turns is discarded and ends the
    transition; a completed one is merged (proposal <- candidate with probability min(1, w_sub / W)) and the whole tree is checked.
    O(max_depth) saved vectors, no recursion.  sum_fn: the sum every dot product uses (the tests reverse it); trace: a list that receives
    (kind, lhs, rhs, scale, outcome) of every comparison made — kind "direction", "divergence", "leaf", "merge", "uturn" (scale: what
    |lhs - rhs| is relative to) — and ("energy", H, H0, 0, None) per leaf, ("end", reason, depth, leaves of the turning sub-tree, None)."""
    th, lp, g = state
    D = int(max_depth)
    u = np.asarray(u, dtype=np.float64)
    u_dir, u_merge, u_leaf = u[:D], u[D:2 * D], u[2 * D:]
    note = (lambda *a: trace.append(a)) if trace is not None else (lambda *a: None)

    def turning(rho, r):
        t = rho * minv * r
        d = float(sum_fn(t))
        note("uturn", d, 0.0, float(np.sum(np.abs(t))), d <= 0.0)
        return d <= 0.0

    r0 = z / np.sqrt(minv)
    h0 = -lp + 0.5 * float(sum_fn(minv * r0 * r0))
    left, right = (th, r0, g), (th, r0, g)
    prop = (th, lp, g)
    rho = r0.copy()
    log_w, depth, n_leaf, sum_acc, divergent = 0.0, 0, 0, 0.0, 0
    r_ck, rho_ck = [None] * max(D, 1), [None] * max(D, 1)
    with np.errstate(all="ignore"):
        while depth < D:
            v = 1.0 if u_dir[depth] < 0.5 else -1.0
            note("direction", float(u_dir[depth]), 0.5, 1.0, v > 0)
            th_m, r_m, g_m = right if v > 0 else left
            s = v * eps
            rho_sub, logw_sub, cand, ended = np.zeros_like(r0), -math.inf, None, False
            for n in range(1 << depth):
                r_m = r_m + 0.5 * s * g_m
                th_m = th_m + s * minv * r_m
                lp_m, g_m = logp_grad(th_m)
                r_m = r_m + 0.5 * s * g_m
                h = -lp_m + 0.5 * float(sum_fn(minv * r_m * r_m))
                note("energy", h, h0, 0.0, None)
                delta = h0 - h
                if not math.isfinite(delta):
                    delta = -math.inf
                sum_acc += math.exp(min(0.0, delta))
                n_leaf += 1
                note("divergence", -delta, delta_max, max(abs(delta), delta_max), not (-delta <= delta_max))
                if not (-delta <= delta_max):
                    divergent, ended = 1, True
                    note("end", "divergent", depth, n, None)
                    break
                logw_sub = _logaddexp(logw_sub, delta)
                if n > 0:
                    p = _exp(delta - logw_sub)
                    note("leaf", float(u_leaf[n_leaf - 1]), p, max(float(u_leaf[n_leaf - 1]), p), bool(u_leaf[n_leaf - 1] < p))
                if n == 0 or u_leaf[n_leaf - 1] < _exp(delta - logw_sub):
                    cand = (th_m, lp_m, g_m)
                rho_sub = rho_sub + r_m
                if n % 2 == 0:
                    i = bin(n).count("1")
                    r_ck[i], rho_ck[i] = r_m, rho_sub
                else:
                    i_max = bin(n >> 1).count("1")
                    k = 0
                    while (n >> k) & 1:
                        k += 1
                    for i in range(i_max, i_max - k, -1):
                        rho_s = rho_sub - rho_ck[i] + r_ck[i]
                        if turning(rho_s, r_ck[i]) or turning(rho_s, r_m):
                            ended = True
                            note("end", "subtree", depth, 1 << (i_max - i + 1), None)
                            break
                    if ended:
                        break
            if ended:
                break
            p = _exp(logw_sub - log_w)
            note("merge", float(u_merge[depth]), p, max(float(u_merge[depth]), p), bool(u_merge[depth] < p))
            if u_merge[depth] < p:
                prop = cand
            log_w = _logaddexp(log_w, logw_sub)
            rho = rho + rho_sub
            if v > 0:
                right = (th_m, r_m, g_m)
            else:
                left = (th_m, r_m, g_m)
            depth += 1
            if turning(rho, left[1]) or turning(rho, right[1]):
                note("end", "uturn", depth, 0, None)
                break
            if depth == D:
                note("end", "max_depth", depth, 0, None)
    return prop, {"tree_depth": depth, "n_leapfrog": n_leaf, "accept_stat": sum_acc / n_leaf, "divergent": divergent}


def _nuts(logp_grad, theta0, draw_samples, max_depth, eps0, target, rng, n_adapts=None, transition=None, set_metric=None, init_chain=None, chunk=256):
    """NUTS ([3P] AdvancedHMC.NUTS(delta)) with `_hmc`'s step-size search, dual averaging — on the tree's accept_stat — and windowed diagonal
    metric during the first n_adapts draws (`_find_stepsize`, `_adapt_and_draw`).  transition(n, eps, metric) -> lists of per-draw (th,
    accept_stat, tree_depth, n_leapfrog, divergent) runs n draws of the chain: by default `_nuts_transition` on the host with z and u from
    `rng`; `_nuts_device` passes the resident one (and set_metric / init_chain, which tell the device about a new metric / the start)."""
    n = theta0.size
    n_adapts = min(draw_samples // 10, 1000) if n_adapts is None else n_adapts
    th = theta0.astype(np.float64).copy()
    lp, g = logp_grad(th)
    met = _DiagMetric(np.ones(n))
    eps = _find_stepsize(logp_grad, th, lp, g, met, eps0, rng.standard_normal(n))
    if init_chain is not None:
        init_chain(th)
    host_state = [(th, lp, g)]

    def host_transition(nd, eps, met):
        out = []
        for _ in range(nd):
            z, u = rng.standard_normal(n), rng.random(nuts_uniforms(max_depth))
            host_state[0], st = _nuts_transition(logp_grad, host_state[0], met.minv, eps, z, u, max_depth)
            out.append((host_state[0][0].copy(), st["accept_stat"], st["tree_depth"], st["n_leapfrog"], st["divergent"]))
        return out
    rows, eps, met = _adapt_and_draw(host_transition if transition is None else transition, met, eps, target, draw_samples, n_adapts, set_metric, chunk)
    samples, stats = _stats(rows, eps, met.minv, n_adapts)
    for j, key in ((2, "tree_depth"), (3, "n_leapfrog"), (4, "divergent")):
        stats[key] = np.asarray([r[j] for r in rows], dtype=np.int64)
    return samples, stats


def _nuts_device(eng, logp_grad, theta0, init_chain, draw_samples, max_depth, eps0, target, rng, seed, n_adapts=None, chunk=256):
    """`_nuts` with the transitions on the device (Engine.nuts_draws): `_hmc_device`'s structure — `nuts_draws(1, ...)` during adaptation (a
    new metric goes down through `hmc_set_metric`), then chunks of `chunk`; normals and uniforms from the device generator (`seed`)."""
    def transition(nd, eps, met):
        smp, acc, _, depth, nleap, div = eng.nuts_draws(nd, max_depth, eps, seed)
        return [(smp[i], float(acc[i]), int(depth[i]), int(nleap[i]), int(div[i])) for i in range(nd)]
    return _nuts(logp_grad, theta0, draw_samples, max_depth, eps0, target, rng, n_adapts, transition, eng.hmc_set_metric, init_chain, chunk)


class LogNormal:
    """[3P] Distributions.LogNormal(mu, sigma) as a parameter prior (`param = [LogNormal(6.0, 0.5)]`, test/PDEBPINN/bpinn_pde__bpinn_pde_inv_i_*.jl:58)."""

    def __init__(self, mu, sigma):
        self.mu, self.sigma = float(mu), float(sigma)

    def params(self):
        return (self.mu, self.sigma)

    def logpdf_grad(self, x):
        if not x > 0.0:
            return -np.inf, 0.0
        z = (np.log(x) - self.mu) / self.sigma
        return float(-np.log(x * self.sigma * np.sqrt(2 * np.pi)) - 0.5 * z * z), float(-1.0 / x - z / (self.sigma * x))


class Normal:
    """[3P] Distributions.Normal(mu, sigma) as a parameter prior."""

    def __init__(self, mu, sigma):
        self.mu, self.sigma = float(mu), float(sigma)

    def params(self):
        return (self.mu, self.sigma)

    def logpdf_grad(self, x):
        z = (x - self.mu) / self.sigma
        return float(-np.log(self.sigma * np.sqrt(2 * np.pi)) - 0.5 * z * z), float(-z / self.sigma)


def ahmc_bayesian_pinn_pde(npde, pde_system, discretization, draw_samples=1000, bcstd=(0.01,), l2std=(0.05,), phystd=(0.05,), priorsNNw=(0.0, 2.0),
                           param=(), n_leapfrog=30, step_size=0.1, targetacceptancerate=0.8, saveats=(0.1,), numensemble=None, rng=None,
                           sampler="host", seed=0, ensemble="host", ensemble_derivatives=(), adaptation="host", kernel="hmc", max_depth=10, nchains=1,
                           metric="diag"):
    """`ahmc_bayesian_pinn_pde(pde_system, discretization; draw_samples, bcstd, phystd, priorsNNw, Kernel = HMC(0.1, 30), saveats,
    numensemble)` — the forward-problem form of ext/bpinn/PDE_BPINN.jl:371-640: the posterior over the network parameters is
    prior N(priorsNNw[1], priorsNNw[2]^2 I) x physics likelihood (`pinn_loglik_grad`: every leapfrog step is ONE fused device evaluation,
    reverse mode over all parameters where the reference differentiates forward over each of them); the HMC sampler, its adaptation and
    the ensemble statistics run on the host, as in the reference.  `discretization`: a PhysicsInformedNN with fixed point sets (the
    reference's BayesianPINN takes GridTraining).  Inverse problems: `param = [prior of every PDE parameter]` (the chain starts at the
    priors' first parameter, as in the reference), the discretization built with `param_estim = True` and the observations as `data_loss`
    terms (the reference's `dataset`), whose standard deviations are `l2std` — the L2 data term then sits in the same fused device call.
    `sampler = "device"` runs the transitions resident on the device (`pinn_hmc_*`; momenta and uniforms from its counter-based generator
    keyed by `seed`, the host `rng` — default_rng(seed) unless given — only feeds the initial step-size search); `stats["sampler"]` says which ran.
    `ensemble = "device"` (independent of `sampler`) forms the ensemble curves in ONE `pinn_phi_ensemble` call per dependent variable — every
    retained draw's prediction and the mean / std over them on the device — instead of one trial-function call per draw; `stats["ensemble"]`.
    `ensemble_derivatives = [(depvar name, order, axes), ...]` adds the posterior mean / std of derivatives of the trial functions on the same
    grid (a flux, a velocity, the u_xx of a residual): `sol.ensemble_derivs` / `sol.ensemble_derivs_std`, dicts keyed by (name, order, axes
    as a tuple).  `ensemble = "device"` forms them in ONE `pinn_derivative_ensemble` call per dependent variable, `"host"` with one
    `pinn_derivative[_f64]` call per draw and numpy.  The default `()` adds nothing.
    `adaptation = "device"` (needs `sampler = "device"`) runs the adaptation draws — dual averaging of the step size, the windowed diagonal
    metric — in ONE `pinn_hmc_warmup` call instead of one `pinn_hmc_draws(1)` round trip per draw; the initial step-size search stays on the
    host, so both settings start from the same step size; `stats["adaptation"]` says which ran.  The default `"host"` changes nothing.
    `kernel = "nuts"` (the reference's `Kernel = NUTS(delta)`, delta = targetacceptancerate) replaces the fixed-length trajectory by
    No-U-Turn transitions of at most 2^max_depth - 1 leapfrog steps (`_nuts_transition`; `n_leapfrog` is then unused): on the host with
    `sampler = "host"`, resident on the device (`pinn_nuts_draws`) with `sampler = "device"`; the warm-up adapts on
    the tree's accept_stat and stays on the host (`adaptation = "device"` is refused).  `stats` gains "kernel" and, for NUTS, "tree_depth",
    "n_leapfrog" and "divergent" per draw.  The default `"hmc"` changes nothing.
    `sampler = "chains"` with `nchains` (the reference's `nchains`, ext/bpinn/PDE_BPINN.jl:548) runs `nchains` chains side by side, one workgroup
    each, whole trajectories inside one launch (`pinn_hmc_chains_*`).  The warm-up — step size and metric — runs ONCE
    on the `sampler = "device"` path (`adaptation` as given) from the first start point; the chains share its step size and metric, chain 0
    starts where the warm-up ended and chain c > 0 at a draw of the weight prior (PDE parameters at their priors' first parameter), and each
    makes `draw_samples - n_adapts` draws.  `sol.chain_samples` (set by this sampler only) is [nchains x draws x P]; `sol.samples` and the ensemble statistics pool the
    chains (draw-major, so the last rows hold every chain's last draws).  `numensemble` counts pooled rows and is not scaled by `nchains`: the default
    `draw_samples // 3` takes about `numensemble / nchains` final draws of every chain.  The chain kernel runs the fp32 kernels: the discretization needs
    `precision = "f32"` (the float64 mode is refused by name).  `kernel = "nuts"` is refused; `nchains > 1` needs `sampler = "chains"`.
    `metric = "dense"` (the reference's `Metric = DenseEuclideanMetric`) adapts a full inverse mass matrix from the windowed sample covariance
    instead of its diagonal: in numpy with `sampler = "host"`, resident on the device (`pinn_hmc_set_metric_dense`) with
    `sampler = "device"` under either `adaptation`; `stats["inv_metric"]` is then P x P and `stats["metric"]` says which ran.  `kernel = "nuts"`
    and `sampler = "chains"` are refused with it.  The default `"diag"` changes nothing."""
    reqs = []
    for r in ensemble_derivatives:
        name, order, axes = r
        reqs.append((str(name), int(order), tuple(int(a) for a in axes)))
        if len(reqs[-1][2]) != reqs[-1][1]:
            raise ValueError(f"ensemble_derivatives: order {order} takes {order} axes, not {list(axes)}")
    if sampler not in ("host", "device", "chains"):
        raise ValueError(f"sampler must be \"host\" or \"device\" (or \"chains\"), not {sampler!r}")
    nchains = int(nchains)
    if nchains < 1:
        raise ValueError("nchains must be at least 1")
    if nchains > 1 and sampler != "chains":
        raise ValueError("nchains > 1 needs sampler=\"chains\": the host and device samplers run one chain")
    if sampler == "chains" and kernel == "nuts":
        raise ValueError("sampler=\"chains\" runs fixed-length HMC trajectories; kernel=\"nuts\" needs sampler=\"host\" or \"device\"")
    if ensemble not in ("host", "device"):
        raise ValueError(f"ensemble must be \"host\" or \"device\", not {ensemble!r}")
    if adaptation not in ("host", "device"):
        raise ValueError(f"adaptation must be \"host\" or \"device\", not {adaptation!r}")
    if adaptation == "device" and sampler not in ("device", "chains"):
        raise ValueError("adaptation=\"device\" needs sampler=\"device\" or \"chains\": the host sampler adapts on the host")
    if kernel not in ("hmc", "nuts"):
        raise ValueError(f"kernel must be \"hmc\" or \"nuts\", not {kernel!r}")
    if kernel == "nuts" and adaptation == "device":
        raise ValueError("kernel=\"nuts\" with adaptation=\"device\": the resident warm-up runs fixed-length HMC transitions only; NUTS adapts on the host")
    if metric not in ("diag", "dense"):
        raise ValueError(f"metric must be \"diag\" or \"dense\", not {metric!r}")
    if metric == "dense" and (kernel == "nuts" or sampler == "chains"):
        raise ValueError("metric=\"dense\" runs fixed-length HMC on one chain: kernel=\"nuts\" and sampler=\"chains\" keep the diagonal metric")
    if kernel == "nuts" and not 1 <= int(max_depth) <= 10:
        raise ValueError("max_depth must be in 1..10")
    if rng is None:
        rng = np.random.default_rng() if sampler == "host" else np.random.default_rng(seed)
    rep = npde.symbolic_discretize(pde_system, discretization)
    eng = rep.engine
    n_pde, n_bc = len(rep.eqs), len(rep.bcs)
    bro = lambda s, n: list(np.broadcast_to(np.asarray(s, dtype=np.float64).reshape(-1), (n,))) if np.size(s) in (1, n) else None
    ps, bs = bro(phystd, n_pde), bro(bcstd, n_bc)
    if ps is None or bs is None:
        raise ValueError("phystd / bcstd: one standard deviation per equation / boundary condition (or one for all)")
    n_data = eng.K - n_pde - n_bc
    ls = bro(l2std, n_data) if n_data else []
    if ls is None:
        raise ValueError("l2std: one standard deviation per data term (or one for all)")
    stds = np.asarray(ps + bs + ls, dtype=np.float64)
    mu0, sd0 = float(priorsNNw[0]), float(priorsNNw[1])
    ninv = len(param)
    if ninv and (not discretization.param_estim or ninv != int(eng.P - sum(c.nparams for c in discretization.chain))):
        raise ValueError("param: one prior per estimated PDE parameter, and the discretization needs param_estim = True")
    nn = eng.P - ninv

    def logp_grad(th):
        ll, g, _ = eng.loglik_grad_f64(th, stds)
        g = g.astype(np.float64)
        w = th[:nn]
        lp = ll - 0.5 * np.sum(((w - mu0) / sd0) ** 2) - nn * (np.log(sd0) + 0.5 * np.log(2 * np.pi))
        g[:nn] -= (w - mu0) / sd0 ** 2
        for j, pr in enumerate(param):
            l, d = pr.logpdf_grad(float(th[nn + j]))
            lp += l
            g[nn + j] += d
        return lp, g
    theta0 = np.asarray(rep.flat_init_params, dtype=np.float64).copy()
    for j, pr in enumerate(param):
        theta0[nn + j] = pr.params()[0]
    chain_samples = None
    if sampler in ("device", "chains"):
        kinds = []
        for pr in param:
            if not isinstance(pr, (Normal, LogNormal)):
                raise ValueError("sampler=\"device\": parameter priors must be Normal or LogNormal")
            kinds.append((1 if isinstance(pr, LogNormal) else 0,) + tuple(pr.params()))
        if sampler == "chains":
            # the shared warm-up on the resident single-chain path, then every chain's draws in launches of `chunk` draws
            n_adapts = min(int(draw_samples) // 10, 1000)
            _, stats = _hmc_device(eng, logp_grad, theta0, lambda th: eng.hmc_init(th, stds, (mu0, sd0), kinds), n_adapts, int(n_leapfrog),
                                      float(step_size), float(targetacceptancerate), rng, int(seed), n_adapts=n_adapts, adaptation=adaptation)
            starts = np.tile(eng.hmc_get(want_grad=False)[0] if n_adapts else theta0, (nchains, 1))
            starts[1:, :nn] = mu0 + sd0 * rng.standard_normal((nchains - 1, nn))
            eng.hmc_chains_init(starts, stats["step_size"], stds, (mu0, sd0), kinds, int(n_leapfrog), stats["inv_metric"], int(seed))
            parts, accs = [], []
            for nd in _chunks(int(draw_samples) - n_adapts):
                smp, acc, _ = eng.hmc_chains_draws(nd)
                parts.append(smp); accs.append(acc)
            chain_samples = np.concatenate(parts, axis=1) if parts else np.zeros((nchains, 0, eng.P))
            samples = chain_samples.transpose(1, 0, 2).reshape(-1, eng.P)          # pooled, draw-major
            stats["acceptance"] = np.concatenate(accs, axis=1) if accs else np.zeros((nchains, 0))
            stats["nchains"] = nchains
        elif kernel == "nuts":
            samples, stats = _nuts_device(eng, logp_grad, theta0, lambda th: eng.hmc_init(th, stds, (mu0, sd0), kinds), int(draw_samples), int(max_depth),
                                          float(step_size), float(targetacceptancerate), rng, int(seed))
        else:
            samples, stats = _hmc_device(eng, logp_grad, theta0, lambda th: eng.hmc_init(th, stds, (mu0, sd0), kinds), int(draw_samples), int(n_leapfrog),
                                         float(step_size), float(targetacceptancerate), rng, int(seed), adaptation=adaptation, metric=metric)
    elif kernel == "nuts":
        samples, stats = _nuts(logp_grad, theta0, int(draw_samples), int(max_depth), float(step_size), float(targetacceptancerate), rng)
    else:
        samples, stats = _hmc(logp_grad, theta0, int(draw_samples), int(n_leapfrog), float(step_size), float(targetacceptancerate), rng, metric=metric)
    stats["sampler"] = sampler
    stats["ensemble"] = ensemble
    stats["adaptation"] = adaptation
    stats["kernel"] = kernel
    stats["metric"] = metric
    numensemble = int(draw_samples // 3) if numensemble is None else int(numensemble)
    # inference: the last `numensemble` draws on the saveats grid (one spacing per independent variable), per dependent variable
    doms = {str(d.variable): (float(d.domain.lo), float(d.domain.hi)) for d in pde_system.domain}
    # the reference slices samples[(end - numensemble):end] — numensemble + 1 draws (ext/bpinn/PDE_BPINN.jl:254) — estimates the PDE
    # parameters over all of them (:264-269) and builds the ensemble curves from the first numensemble of the slice (:302); restated as is
    ens_samples = samples[-(numensemble + 1):]
    ens, ens_std, tps = [], [], []
    ens_d, ens_d_std = {}, {}
    for r in reqs:
        if r[0] not in [str(v) for v in rep.depvars]:
            raise ValueError(f"ensemble_derivatives: no dependent variable {r[0]!r} (known: {[str(v) for v in rep.depvars]})")
    f64_mode = bool(reqs) and eng.get_option("precision") == "f64"
    for i, name in enumerate(rep.depvars):
        ins = list(rep.dict_depvar_input[name])
        if len(saveats) not in (1, len(pde_system.ivs)):
            raise ValueError("saveats: one grid spacing per independent variable")
        axes = []
        for v in ins:
            k = [str(q) for q in pde_system.ivs].index(str(v))
            lo, hi = doms[str(v)]
            step = float(saveats[k if len(saveats) > 1 else 0])
            axes.append(np.arange(lo, hi + 0.5 * step, step))
        mesh = np.meshgrid(*axes, indexing="ij")
        pts = np.stack([m.ravel() for m in mesh])
        net = (rep.phi[i] if isinstance(rep.phi, (list, tuple)) else rep.phi).net
        mine = [r for r in reqs if r[0] == str(name)]
        if mine and ensemble == "device":        # every derivative of this variable in one call
            dmean, dstd = eng.derivative_ensemble(net, ens_samples[:numensemble], pts, [(o, ax) for _, o, ax in mine])
            for j, r in enumerate(mine):
                ens_d[r], ens_d_std[r] = dmean[j], dstd[j]
        elif mine:                               # the comparison path: one derivative call per draw and request (the full vectors: the engine slices)
            for r in mine:
                der = (lambda th: eng.derivative_f64(net, th, pts, r[2])) if f64_mode else (lambda th: eng.derivative(net, th, pts, r[2]).astype(np.float64))
                dpreds = np.stack([der(th) for th in ens_samples[:numensemble]])
                ens_d[r], ens_d_std[r] = dpreds.mean(axis=0), dpreds.std(axis=0)
        if ensemble == "device":                 # the full sample vectors and the variable's network index: the engine slices
            mean, std = eng.phi_ensemble(net, ens_samples[:numensemble], pts)
            ens.append(mean); ens_std.append(std); tps.append(pts)
            continue
        preds = np.stack([rep.phi[i](pts, npde.depvar_params(rep, th, name))[0] if isinstance(rep.phi, (list, tuple)) else rep.phi(pts, th)[0]
                          for th in ens_samples[:numensemble]])     # the reference predicts with the FIRST numensemble of its slice (:302)
        ens.append(preds.mean(axis=0)); ens_std.append(preds.std(axis=0)); tps.append(pts)
    sol = BPINNsolution(samples, ens, ens_std, tps, stats)
    if chain_samples is not None:        # sampler="chains": every chain's own draws, [nchains x draws x P]
        sol.chain_samples = chain_samples
    if reqs:
        sol.ensemble_derivs, sol.ensemble_derivs_std = ens_d, ens_d_std
    sol.estimated_de_params = [float(ens_samples[:, nn + j].mean()) for j in range(ninv)]
    return sol
