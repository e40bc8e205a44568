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
`adaptation="device"` runs the whole warm-up in ONE resident call (`pinn_hmc_warmup`).
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


def _hmc(logp_grad, theta0, draw_samples, n_leapfrog, eps0, target, rng, n_adapts=None):
    """HMC with `n_leapfrog` leapfrog steps per draw ([3P] AdvancedHMC.HMC(eps, n_leapfrog)), Stan-style adaptation during the first
    n_adapts = min(draw_samples / 10, 1000) draws (AdvancedHMC's default): dual averaging of the step size towards `target` acceptance
    and a diagonal metric from the windowed sample variance (StanHMCAdaptor + DiagEuclideanMetric)."""
    n = theta0.size
    n_adapts = min(draw_samples // 10, 1000) if n_adapts is None else n_adapts
    th = theta0.astype(np.float64).copy()
    lp, g = logp_grad(th)
    minv = np.ones(n)                                # inverse mass (diagonal metric)

    def leap(th, r, g, eps, steps):
        r = r + 0.5 * eps * g
        for s in range(steps):
            th = th + eps * minv * r
            lp, g = logp_grad(th)
            r = r + (eps if s < steps - 1 else 0.5 * eps) * g
        return th, r, lp, g

    # find_good_stepsize: double / halve until the one-step acceptance crosses 0.8 (AdvancedHMC.find_good_stepsize)
    eps = eps0
    r0 = rng.standard_normal(n) / np.sqrt(minv)
    h0 = -lp + 0.5 * np.sum(minv * r0 * r0)
    t1, r1, lp1, _ = leap(th, r0, g, eps, 1)
    d = h0 - (-lp1 + 0.5 * np.sum(minv * r1 * r1))
    direction = 1.0 if (np.isfinite(d) and d > np.log(0.8)) else -1.0
    for _ in range(40):
        eps *= 2.0 ** direction
        t1, r1, lp1, _ = leap(th, r0, g, eps, 1)
        d = h0 - (-lp1 + 0.5 * np.sum(minv * r1 * r1))
        if not np.isfinite(d):
            d = -np.inf
        if (direction > 0) == (d <= np.log(0.8)):
            break
    mu, hbar, log_eps_bar, t0, gamma, kappa = np.log(10 * eps), 0.0, 0.0, 10.0, 0.05, 0.75
    w0, w1 = int(0.15 * n_adapts), int(0.9 * n_adapts)            # variance window of the metric adaptation
    win = []
    samples, accs = [], []
    m_count = 0
    for it in range(draw_samples):
        r = rng.standard_normal(n) / np.sqrt(minv)
        h_old = -lp + 0.5 * np.sum(minv * r * r)
        tn, rn, lpn, gn = leap(th, r, g, eps, n_leapfrog)
        h_new = -lpn + 0.5 * np.sum(minv * rn * rn)
        a = float(np.exp(min(0.0, h_old - h_new))) if np.isfinite(h_new) else 0.0
        if rng.random() < a:
            th, lp, g = tn, lpn, gn
        samples.append(th.copy())
        accs.append(a)
        if it < n_adapts:
            m_count += 1
            hbar = (1 - 1 / (m_count + t0)) * hbar + (target - a) / (m_count + t0)
            log_eps = mu - np.sqrt(m_count) / gamma * hbar
            eta = m_count ** (-kappa)
            log_eps_bar = eta * log_eps + (1 - eta) * log_eps_bar
            eps = float(np.exp(log_eps))
            if w0 <= it < w1:
                win.append(th.copy())
            if it == w1 - 1 and len(win) >= 8 and n_adapts >= 100:       # (a metric from fewer draws is noise; short runs keep the unit metric)
                var = np.var(np.asarray(win), axis=0)
                k = len(win)
                minv = (k / (k + 5.0)) * var + 1e-3 * (5.0 / (k + 5.0))
                mu, hbar, log_eps_bar, m_count = np.log(10 * eps), 0.0, 0.0, 0          # restart the step-size search on the new metric
            if it == n_adapts - 1:
                eps = float(np.exp(log_eps_bar)) if m_count > 0 else eps
    return np.asarray(samples), {"acceptance": np.asarray(accs), "step_size": eps, "inv_metric": minv, "n_adapts": n_adapts}


def _hmc_device(eng, logp_grad, theta0, init_chain, draw_samples, n_leapfrog, eps0, target, rng, seed, n_adapts=None, chunk=256, adaptation="host"):
    """`_hmc` with the transitions on the device (Engine.hmc_*): the same initial step-size search on the host evaluation path (at most 42
    evaluations), the same dual averaging and windowed metric in Python around `hmc_draws(1, ...)` during adaptation (a new metric goes down
    through `hmc_set_metric`), then the remaining draws in chunks of `chunk`.  Momenta and uniforms come from the device generator (`seed`).
    adaptation="device": the adaptation draws are ONE `hmc_warmup` call — the same recurrence and window on the device — after the same host
    search, so both settings start from the same step size."""
    n = theta0.size
    n_adapts = min(draw_samples // 10, 1000) if n_adapts is None else n_adapts
    th = theta0.astype(np.float64).copy()
    lp, g = logp_grad(th)
    minv = np.ones(n)

    def one_step(r, eps):
        r = r + 0.5 * eps * g
        t1 = th + eps * minv * r
        lp1, g1 = logp_grad(t1)
        r = r + 0.5 * eps * g1
        return -lp1 + 0.5 * np.sum(minv * r * r)

    eps = eps0
    r0 = rng.standard_normal(n) / np.sqrt(minv)
    h0 = -lp + 0.5 * np.sum(minv * r0 * r0)
    d = h0 - one_step(r0, eps)
    direction = 1.0 if (np.isfinite(d) and d > np.log(0.8)) else -1.0
    for _ in range(40):
        eps *= 2.0 ** direction
        d = h0 - one_step(r0, eps)
        if not np.isfinite(d):
            d = -np.inf
        if (direction > 0) == (d <= np.log(0.8)):
            break
    init_chain(th)
    mu, hbar, log_eps_bar, t0, gamma, kappa = np.log(10 * eps), 0.0, 0.0, 10.0, 0.05, 0.75
    w0, w1 = int(0.15 * n_adapts), int(0.9 * n_adapts)
    win, samples, accs = [], [], []
    m_count = 0
    host_adapts = min(n_adapts, draw_samples)
    if adaptation == "device" and host_adapts >= 1:
        if n_adapts > draw_samples:
            raise ValueError("adaptation=\"device\": the warm-up is one call of n_adapts draws; draw_samples must be at least n_adapts")
        smp, acc, _, _, eps, minv = eng.hmc_warmup(n_adapts, n_leapfrog, eps, target, seed)
        samples.extend(smp)
        accs.extend(acc)
        host_adapts = 0
    for it in range(host_adapts):
        smp, acc, _ = eng.hmc_draws(1, n_leapfrog, eps, seed)
        th, a = smp[0], float(acc[0])
        samples.append(th)
        accs.append(a)
        m_count += 1
        hbar = (1 - 1 / (m_count + t0)) * hbar + (target - a) / (m_count + t0)
        log_eps = mu - np.sqrt(m_count) / gamma * hbar
        eta = m_count ** (-kappa)
        log_eps_bar = eta * log_eps + (1 - eta) * log_eps_bar
        eps = float(np.exp(log_eps))
        if w0 <= it < w1:
            win.append(th)
        if it == w1 - 1 and len(win) >= 8 and n_adapts >= 100:
            var = np.var(np.asarray(win), axis=0)
            k = len(win)
            minv = (k / (k + 5.0)) * var + 1e-3 * (5.0 / (k + 5.0))
            eng.hmc_set_metric(minv)
            mu, hbar, log_eps_bar, m_count = np.log(10 * eps), 0.0, 0.0, 0
        if it == n_adapts - 1:
            eps = float(np.exp(log_eps_bar)) if m_count > 0 else eps
    done = len(samples)
    while done < draw_samples:
        nd = min(int(chunk), draw_samples - done)
        smp, acc, _ = eng.hmc_draws(nd, n_leapfrog, eps, seed)
        samples.extend(smp)
        accs.extend(acc)
        done += nd
    return np.asarray(samples), {"acceptance": np.asarray(accs), "step_size": eps, "inv_metric": minv, "n_adapts": n_adapts}


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


def _find_stepsize(logp_grad, th, lp, g, minv, eps, r0):
    """the initial step-size search of `_hmc` (AdvancedHMC.find_good_stepsize) from (th, lp, g) with the momentum r0"""
    def one_step(e):
        r = r0 + 0.5 * e * g
        lp1, g1 = logp_grad(th + e * minv * r)
        r = r + 0.5 * e * g1
        return -lp1 + 0.5 * np.sum(minv * r * r)

    h0 = -lp + 0.5 * np.sum(minv * r0 * r0)
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


def _nuts(logp_grad, theta0, draw_samples, max_depth, eps0, target, rng, n_adapts=None, transition=None, set_metric=None, init_chain=None, chunk=256):
    """NUTS ([3P] AdvancedHMC.NUTS(delta)) with `_hmc`'s step-size search, dual averaging — on the tree's accept_stat — and windowed diagonal
    metric during the first n_adapts draws.  transition(n, eps, minv) -> lists of per-draw (th, accept_stat, tree_depth, n_leapfrog,
    divergent) runs n draws of the chain: by default `_nuts_transition` on the host with z and u from `rng`; `_nuts_device` passes the
    resident one (and set_metric / init_chain, which tell the device about a new metric / the start)."""
    n = theta0.size
    n_adapts = min(draw_samples // 10, 1000) if n_adapts is None else n_adapts
    th = theta0.astype(np.float64).copy()
    lp, g = logp_grad(th)
    minv = np.ones(n)
    eps = _find_stepsize(logp_grad, th, lp, g, minv, eps0, rng.standard_normal(n) / np.sqrt(minv))
    if init_chain is not None:
        init_chain(th)
    host_state = [(th, lp, g)]

    def host_transition(nd, eps, minv):
        out = []
        for _ in range(nd):
            z, u = rng.standard_normal(n), rng.random(nuts_uniforms(max_depth))
            host_state[0], st = _nuts_transition(logp_grad, host_state[0], minv, eps, z, u, max_depth)
            out.append((host_state[0][0].copy(), st["accept_stat"], st["tree_depth"], st["n_leapfrog"], st["divergent"]))
        return out
    transition = host_transition if transition is None else transition
    mu, hbar, log_eps_bar, t0, gamma, kappa = np.log(10 * eps), 0.0, 0.0, 10.0, 0.05, 0.75
    w0, w1 = int(0.15 * n_adapts), int(0.9 * n_adapts)
    win, rows = [], []
    m_count = 0
    for it in range(min(n_adapts, draw_samples)):
        row = transition(1, eps, minv)[0]
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
        if it == w1 - 1 and len(win) >= 8 and n_adapts >= 100:
            var = np.var(np.asarray(win), axis=0)
            k = len(win)
            minv = (k / (k + 5.0)) * var + 1e-3 * (5.0 / (k + 5.0))
            if set_metric is not None:
                set_metric(minv)
            mu, hbar, log_eps_bar, m_count = np.log(10 * eps), 0.0, 0.0, 0
        if it == n_adapts - 1:
            eps = float(np.exp(log_eps_bar)) if m_count > 0 else eps
    while len(rows) < draw_samples:
        rows.extend(transition(min(int(chunk), draw_samples - len(rows)), eps, minv))
    col = lambda j, dt: np.asarray([r[j] for r in rows], dtype=dt)
    return col(0, np.float64), {"acceptance": col(1, np.float64), "step_size": eps, "inv_metric": minv, "n_adapts": n_adapts,
                                "tree_depth": col(2, np.int64), "n_leapfrog": col(3, np.int64), "divergent": col(4, np.int64)}


def _nuts_device(eng, logp_grad, theta0, init_chain, draw_samples, max_depth, eps0, target, rng, seed, n_adapts=None, chunk=256):
    """`_nuts` with the transitions on the device (Engine.nuts_draws): `_hmc_device`'s structure — `nuts_draws(1, ...)` during adaptation (a
    new metric goes down through `hmc_set_metric`), then chunks of `chunk`; normals and uniforms from the device generator (`seed`)."""
    def transition(nd, eps, minv):
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
                           sampler="host", seed=0, ensemble="host", ensemble_derivatives=(), adaptation="host", kernel="hmc", max_depth=10):
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
    "n_leapfrog" and "divergent" per draw.  The default `"hmc"` changes nothing."""
    reqs = []
    for r in ensemble_derivatives:
        name, order, axes = r
        reqs.append((str(name), int(order), tuple(int(a) for a in axes)))
        if len(reqs[-1][2]) != reqs[-1][1]:
            raise ValueError(f"ensemble_derivatives: order {order} takes {order} axes, not {list(axes)}")
    if sampler not in ("host", "device"):
        raise ValueError(f"sampler must be \"host\" or \"device\", not {sampler!r}")
    if ensemble not in ("host", "device"):
        raise ValueError(f"ensemble must be \"host\" or \"device\", not {ensemble!r}")
    if adaptation not in ("host", "device"):
        raise ValueError(f"adaptation must be \"host\" or \"device\", not {adaptation!r}")
    if adaptation == "device" and sampler != "device":
        raise ValueError("adaptation=\"device\" needs sampler=\"device\": the host sampler adapts on the host")
    if kernel not in ("hmc", "nuts"):
        raise ValueError(f"kernel must be \"hmc\" or \"nuts\", not {kernel!r}")
    if kernel == "nuts" and adaptation == "device":
        raise ValueError("kernel=\"nuts\" with adaptation=\"device\": the resident warm-up runs fixed-length HMC transitions only; NUTS adapts on the host")
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
    if sampler == "device":
        kinds = []
        for pr in param:
            if not isinstance(pr, (Normal, LogNormal)):
                raise ValueError("sampler=\"device\": parameter priors must be Normal or LogNormal")
            kinds.append((1 if isinstance(pr, LogNormal) else 0,) + tuple(pr.params()))
        if kernel == "nuts":
            samples, stats = _nuts_device(eng, logp_grad, theta0, lambda th: eng.hmc_init(th, stds, (mu0, sd0), kinds), int(draw_samples), int(max_depth),
                                          float(step_size), float(targetacceptancerate), rng, int(seed))
        else:
            samples, stats = _hmc_device(eng, logp_grad, theta0, lambda th: eng.hmc_init(th, stds, (mu0, sd0), kinds), int(draw_samples), int(n_leapfrog),
                                         float(step_size), float(targetacceptancerate), rng, int(seed), adaptation=adaptation)
    elif kernel == "nuts":
        samples, stats = _nuts(logp_grad, theta0, int(draw_samples), int(max_depth), float(step_size), float(targetacceptancerate), rng)
    else:
        samples, stats = _hmc(logp_grad, theta0, int(draw_samples), int(n_leapfrog), float(step_size), float(targetacceptancerate), rng)
    stats["sampler"] = sampler
    stats["ensemble"] = ensemble
    stats["adaptation"] = adaptation
    stats["kernel"] = kernel
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
    if reqs:
        sol.ensemble_derivs, sol.ensemble_derivs_std = ens_d, ens_d_std
    sol.estimated_de_params = [float(ens_samples[:, nn + j].mean()) for j in range(ninv)]
    return sol
