"""Resident NUTS (`pinn_nuts_draws`): No-U-Turn transitions of the BPINN chain on the device.

The reference throughout is `bpinn._nuts_transition` — the specification — driven by the SAME handle's `loglik_grad_f64` through
`test_resident_hmc.make_logp` (one host round trip per leapfrog step), never the code under test.  Every device draw is compared with ONE
call of it that starts from the device's own previous state (`hmc_get`): errors do not compound through the chain (§4.11's lesson).

Every body is written once as a function of `npde` and exposed twice: on the CPU through the g++ emulation (`use_emu`) and, marked `gpu`,
on the product library (`hip_lib`).  Problems: §4.7's (test_resident_hmc.forward_problem / inverse_problem, P = 321 / 322).

THE BAR (test_resident_hmc's, per draw).  Device and restatement differ in the order of the dot products and in the last place of library
exp / log / log1p / cos; the elementwise arithmetic is restated operation by operation.  s = the restatement's own sensitivity to the order
of its sums (run again with every sum reversed): the largest max-norm relative difference over (theta, logp, accept_stat).
bar = min(1e-9, 100 max(s, 2^-52 max|H|)), |H| over the leaves of the restatement.  tree_depth, n_leapfrog and divergent must be equal.
CONDITION ON THE INPUTS (asserted, not skipped): for the seeds below the forward and the reversed restatement take identical decisions, and
every comparison the restatement makes (u < p, dot product <= 0, -delta <= delta_max) has a relative margin >= 1e-6 — relative to
max(u, p), to sum |terms| of the dot product, to max(|delta|, delta_max).  The smallest margin seen over all parity, coverage and
generator cases, on the CPU emulation and on an MI355X alike: 1.26e-3 (parity, fp32, non-unit metric, max_depth 3); per case in
profiles/resident_nuts.txt."""
import ctypes as C

import numpy as np
import pytest

from test_resident_hmc import (EPS64, GEN_SEED, NN_PRIOR, PRECISIONS, chain16, forward_problem, gen_draw, inverse_problem, kinds_of, make_logp, metric,  # noqa: F401
                               mix32, relerr, small_problem)

MARGIN = 1e-6               # (the smallest margin the chosen inputs leave is 1.26e-3)
DECISIONS = ("direction", "divergence", "leaf", "merge", "uturn")


def nuts_mod():
    from neuralpde_jl_amd import bpinn
    return bpinn


def nuts_inputs(P, ndraws, max_depth, seed):
    """-> standard normals [ndraws, P], uniforms [ndraws, 2 D + 2^D - 1]"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ndraws, P)), rng.random((ndraws, nuts_mod().nuts_uniforms(max_depth)))


def margin_of(entry):
    kind, lhs, rhs, scale, _ = entry
    if not (np.isfinite(lhs) and np.isfinite(rhs)):
        return np.inf                                     # (delta = -inf, a weight ratio of inf: decided by any arithmetic)
    return abs(lhs - rhs) / scale if scale > 0 else np.inf


def restate_draw(eng, stds, nn, priors, state, minv, eps, z, u, max_depth, delta_max=1000.0):
    """ONE transition of the specification from `state`, forward and with every sum reversed.
    -> (state', stats), sensitivity s, bar, smallest margin, trace of the forward run.  Asserts the condition on the inputs."""
    bp = nuts_mod()
    out = []
    for rev in (False, True):
        logp_grad, sm = make_logp(eng, stds, nn, priors, rev)
        tr = []
        new, st = bp._nuts_transition(logp_grad, state, minv, eps, z, u, max_depth, delta_max, sum_fn=sm, trace=tr)
        out.append((new, st, tr))
    (new, st, tr), (new_b, st_b, tr_b) = out
    dec = lambda t: [(e[0], e[4]) for e in t if e[0] in DECISIONS] + [e[:4] for e in t if e[0] == "end"]
    assert dec(tr) == dec(tr_b), "the forward and the reversed restatement decide differently: choose other inputs"
    assert all(st[q] == st_b[q] for q in ("tree_depth", "n_leapfrog", "divergent"))
    mg = min(margin_of(e) for t in (tr, tr_b) for e in t if e[0] in DECISIONS)
    assert mg >= MARGIN, f"a comparison of the restatement has relative margin {mg:.3e} < {MARGIN}: choose other inputs"
    sens = max(relerr(new_b[0], new[0]), relerr(new_b[1], new[1]), relerr(st_b["accept_stat"], st["accept_stat"]))
    hs = [abs(e[1]) for e in tr if e[0] == "energy" and np.isfinite(e[1])] + [abs(e[2]) for e in tr if e[0] == "energy"]
    bar = min(1e-9, 100.0 * max(sens, EPS64 * max(hs)))
    return (new, st), sens, bar, mg, tr


def ends_of(tr):
    return [e[1:4] for e in tr if e[0] == "end"]


def run_against_restatement(eng, stds, nn, priors, minv, eps, z, u, max_depth, label, delta_max=1000.0):
    """every row of (z, u) as one device draw against one restated transition from the device's previous state -> list of traces"""
    traces, worst, low = [], 0.0, np.inf
    for d in range(len(z)):
        prev = eng.hmc_get()
        (new, st), sens, bar, mg, tr = restate_draw(eng, stds, nn, priors, prev, minv, eps, z[d], u[d], max_depth, delta_max)
        smp, acc, lp, depth, nleap, div = eng.nuts_draws(1, max_depth, eps, 0, z[d:d + 1], u[d:d + 1], delta_max)
        err = max(relerr(smp[0], new[0]), relerr(lp[0], new[1]), relerr(acc[0], st["accept_stat"]))
        print(f"resident nuts {label} draw {d}: depth {depth[0]} leaves {nleap[0]} divergent {div[0]} accept_stat {acc[0]:.4f} ends {ends_of(tr)}  "
              f"err {err:.3e}  sensitivity {sens:.3e}  bar {bar:.3e}  margin {mg:.3e}")
        assert (int(depth[0]), int(nleap[0]), int(div[0])) == (st["tree_depth"], st["n_leapfrog"], st["divergent"])
        assert err <= bar
        th, lpg, g = eng.hmc_get()
        assert np.array_equal(th, smp[0]) and lpg == lp[0] and relerr(g, new[2]) <= bar
        traces.append(tr)
        worst, low = max(worst, err / bar), min(low, mg)
    print(f"resident nuts {label}: worst err / bar {worst:.3f}, smallest margin {low:.3e}")
    return traces


# (max_depth -> step size, seed of the inputs): looked for on the CPU emulation so that the condition on the inputs holds
PARITY_INPUTS = {3: (1.0e-2, 3), 5: (1.0e-2, 5)}
ND = 4


def body_transition_parity(npde, precision, metric_kind, max_depth):
    """case 1: supplied normals and uniforms; every draw against the specification"""
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    minv = metric(eng.P, metric_kind)
    eps, seed = PARITY_INPUTS[max_depth]
    z, u = nuts_inputs(eng.P, ND, max_depth, seed)
    eng.hmc_init(th0, stds, NN_PRIOR, kinds_of(priors))
    eng.hmc_set_metric(None if metric_kind == "unit" else minv)
    run_against_restatement(eng, stds, nn, priors, minv, eps, z, u, max_depth, f"parity [{precision} {metric_kind} D={max_depth}]")


# Under the likelihood of the parity cases a trajectory of <= 31 steps never turns: the stable step size is set by the few stiff directions
# of the likelihood, the turn by the ~320 directions the prior N(0, 2^2) governs (half a period = 2 pi time units).  The coverage runs
# therefore weaken the likelihood (every std x 20: inputs of pinn_hmc_init like any other), which lets steps of 0.2 - 0.4 run.
# (step size, max_depth, seed, draws), looked for on the CPU emulation
COVERAGE_STD_SCALE = 20.0
COVERAGE = ((0.2, 5, 0, 6), (0.4, 5, 0, 1))
EPS_DIVERGENT = 50.0


def body_branch_coverage(npde, precision):
    """case 2: between them the inputs end draws by the top-level U-turn, by a checkpoint check of a sub-tree of >= 4 leaves, by max_depth
    and by divergence, go in both directions, take a merge and decline one — asserted on the restatement, and the device agrees on each"""
    rep, th0, stds, nn, priors = inverse_problem(npde, precision, "lognormal")
    stds = stds * COVERAGE_STD_SCALE
    eng = rep.engine
    minv = np.ones(eng.P)
    traces = []
    for eps, D, seed, nd in COVERAGE:
        eng.hmc_init(th0, stds, NN_PRIOR, kinds_of(priors))
        z, u = nuts_inputs(eng.P, nd, D, seed)
        traces += run_against_restatement(eng, stds, nn, priors, minv, eps, z, u, D, f"coverage [{precision} eps={eps} D={D}]")
    z, u = nuts_inputs(eng.P, 1, 2, 77)
    before = eng.hmc_get()
    div = run_against_restatement(eng, stds, nn, priors, minv, EPS_DIVERGENT, z, u, 2, f"coverage [{precision} divergent]")
    after = eng.hmc_get()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))          # a divergent first leaf: the chain stays where it was
    traces += div
    ends = [e for t in traces for e in ends_of(t)]
    reasons = {e[0] for e in ends}
    assert reasons >= {"uturn", "subtree", "max_depth", "divergent"}, reasons
    assert any(e[0] == "subtree" and e[2] >= 4 for e in ends), ends
    flat = [e for t in traces for e in t]
    assert {e[4] for e in flat if e[0] == "direction"} == {True, False}
    assert {e[4] for e in flat if e[0] == "merge"} == {True, False}
    assert {e[4] for e in flat if e[0] == "leaf"} == {True, False}


def gen_nuts(seed, counter, P, max_depth):
    """the generator of include/pinn_hip.h for a NUTS draw: normal i = element i's Box-Muller value, uniform k = word(P + k, 0) / 2^32"""
    nu = nuts_mod().nuts_uniforms(max_depth)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    M32 = np.uint64(0xFFFFFFFF)
    base = mix32((lo + np.uint64(0x9E3779B9) * hi) & M32)
    key = mix32(base ^ ((np.uint64(counter) * np.uint64(0x85EBCA6B) + np.uint64(0xC2B2AE35)) & M32))
    e = np.arange(P, P + nu, dtype=np.uint64)
    w0 = mix32(key ^ mix32(((np.uint64(2) * e) * np.uint64(0x9E3779B9) + np.uint64(0x165667B1)) & M32)).astype(np.float64)
    return gen_draw(seed, counter, P)[0], w0 / 4294967296.0


def body_generator(npde, precision):
    """case 3: NULL normals / uniforms against runs supplied with the restated generator's values.  The uniforms are exact arithmetic
    (a 32-bit word / 2^32): a run supplied with them is BIT-equal.  The normals are not: sqrt(-2 log u1) cos(2 pi u2) goes through the
    library's log and cos, and numpy's differ from the C library's in the last place (1 of the 321 normals of draw 0 on the CPU; the
    device's own library differs again), so `gen_draw`'s normals cannot reproduce a run bit for bit anywhere.  For them each draw is
    compared, from the same state (a fresh handle brought there by generator draws), within the bar of the parity case — as
    test_resident_hmc's generator case compares."""
    D, eps, nd = 3, 1.0e-2, 4

    def fresh():
        rep, th0, stds, nn, priors = forward_problem(npde, precision)
        rep.engine.hmc_init(th0, stds, NN_PRIOR, [])
        rep.engine.hmc_set_metric(minv)
        return rep, stds, nn, priors

    minv = metric(321, "nonunit")
    rep, stds, nn, priors = fresh()
    own = rep.engine.nuts_draws(nd, D, eps, GEN_SEED) + rep.engine.hmc_get()
    zs, us = map(np.asarray, zip(*[gen_nuts(GEN_SEED, c, 321, D) for c in range(nd)]))
    assert us[0, 0] == gen_draw(GEN_SEED, 0, 321)[1]                         # uniform 0 is the u of pinn_hmc_draws
    assert np.all((us >= 0) & (us < 1)) and 0.7 < zs.std() < 1.3 and len(np.unique(us)) == us.size
    rep, stds, nn, priors = fresh()
    uni = rep.engine.nuts_draws(nd, D, eps, GEN_SEED, None, us) + rep.engine.hmc_get()
    assert all(np.array_equal(a, b) for a, b in zip(own, uni))
    for c in range(nd):
        rep, stds, nn, priors = fresh()
        eng = rep.engine
        if c:
            eng.nuts_draws(c, D, eps, GEN_SEED)
        prev = eng.hmc_get()
        assert np.array_equal(prev[0], own[0][c - 1]) or c == 0
        (new, st), sens, bar, mg, tr = restate_draw(eng, stds, nn, priors, prev, minv, eps, zs[c], us[c], D)
        sup = eng.nuts_draws(1, D, eps, GEN_SEED, zs[c:c + 1])                # supplied normals, the generator's uniforms of counter c
        err = max(relerr(sup[0][0], own[0][c]), relerr(sup[2][0], own[2][c]), relerr(sup[1][0], own[1][c]))
        print(f"resident nuts generator [{precision}] draw {c}: err {err:.3e}  bar {bar:.3e}  margin {mg:.3e}")
        assert (sup[3][0], sup[4][0], sup[5][0]) == (own[3][c], own[4][c], own[5][c]) == (st["tree_depth"], st["n_leapfrog"], st["divergent"])
        assert err <= bar
        assert max(relerr(own[0][c], new[0]), relerr(own[2][c], new[1]), relerr(own[1][c], st["accept_stat"])) <= bar
    rep, stds, nn, priors = fresh()
    other = rep.engine.nuts_draws(nd, D, eps, GEN_SEED + 1)
    assert not np.array_equal(other[0], own[0])


def body_chunking(npde, precision):
    """case 4: 2 + 3 draws == 5 draws; "nuts_chunk" 1, 8 and 64; a fresh handle; hmc_draws(2) then nuts_draws(2) consume counters 0 - 3"""
    D, eps = 3, 2.0e-2
    outs = []
    for split, chunk in (((5,), None), ((2, 3), None), ((5,), 1), ((5,), 64), ((5,), 8)):
        rep, th0, stds, nn, priors = forward_problem(npde, precision)
        eng = rep.engine
        if chunk is None:
            assert eng.get_option("nuts_chunk") == "8"
        else:
            eng.set_option("nuts_chunk", str(chunk))
            assert eng.get_option("nuts_chunk") == str(chunk)
        eng.hmc_init(th0, stds, NN_PRIOR, [])
        parts = [eng.nuts_draws(n, D, eps, 99) for n in split]
        outs.append([np.concatenate([q[i] for q in parts]) for i in range(6)] + list(eng.hmc_get()))
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))
    assert len(set(map(int, outs[0][4]))) > 1 or len(set(map(float, outs[0][1]))) > 1
    for bad in ("0", "65", "x"):
        with pytest.raises(Exception, match="nuts_chunk"):
            eng.set_option("nuts_chunk", bad)
    # one stream of counters: the NUTS draws after two HMC draws are those of counters 2 and 3
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.hmc_draws(2, 2, eps, 99)
    mid = eng.hmc_get()
    mixed = eng.nuts_draws(2, D, eps, 99)
    rep2, _, _, _, _ = forward_problem(npde, precision)
    e2 = rep2.engine
    e2.hmc_init(th0, stds, NN_PRIOR, [])
    e2.hmc_draws(2, 2, eps, 99)
    assert all(np.array_equal(a, b) for a, b in zip(e2.hmc_get(), mid))
    zs, us = map(np.asarray, zip(*[gen_nuts(99, c, e2.P, D) for c in (2, 3)]))
    # the uniforms (exact arithmetic) bit for bit; the normals of counter 2 to the bar of one restated draw (body_generator says why)
    assert all(np.array_equal(a, b) for a, b in zip(mixed, e2.nuts_draws(2, D, eps, 99, None, us)))
    rep3, _, _, _, _ = forward_problem(npde, precision)
    e3 = rep3.engine
    e3.hmc_init(th0, stds, NN_PRIOR, [])
    e3.hmc_draws(2, 2, eps, 99)
    (new, st), sens, bar, mg, tr = restate_draw(e3, stds, nn, priors, mid, np.ones(e3.P), eps, zs[0], us[0], D)
    one = e3.nuts_draws(1, D, eps, 0, zs[:1], us[:1])
    assert (one[3][0], one[4][0], one[5][0]) == (mixed[3][0], mixed[4][0], mixed[5][0])
    assert max(relerr(one[0][0], mixed[0][0]), relerr(one[2][0], mixed[2][0]), relerr(one[1][0], mixed[1][0])) <= bar
    z0, u0 = gen_nuts(99, 0, e3.P, D)
    assert not np.array_equal(z0, zs[0]) and not np.array_equal(u0, us[0])


def body_isolation(npde, precision):
    """case 5: evaluations and an Adam run between two calls leave the chain alone and vice versa; a precision change since init is refused"""
    D, eps = 3, 2.0e-2
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    whole = eng.nuts_draws(5, D, eps, 5)
    rep2, _, _, _, _ = forward_problem(npde, precision)
    e2 = rep2.engine
    e2.hmc_init(th0, stds, NN_PRIOR, [])
    first = e2.nuts_draws(2, D, eps, 5)
    other = th0 + 0.1
    e2.loss_grad_f64(other)
    adam = e2.adam_f64 if precision == "f64" else e2.adam
    get = e2.adam_get_f64 if precision == "f64" else e2.adam_get
    it0, _ = adam(other, 3, 1e-3)
    second = e2.nuts_draws(3, D, eps, 5)
    assert np.array_equal(get(), it0)
    for i in range(6):
        assert np.array_equal(np.concatenate([first[i], second[i]]), whole[i])
    state = e2.hmc_get()
    e2.set_option("precision", "f32" if precision == "f64" else "f64")
    with pytest.raises(Exception, match="precision changed since pinn_hmc_init"):
        e2.nuts_draws(1, D, eps, 5)
    e2.set_option("precision", precision)
    assert all(np.array_equal(a, b) for a, b in zip(e2.hmc_get(), state))


def body_known_target(npde):
    """case 6: the problem and the bars of test_resident_hmc.body_known_target with NUTS on the device against the host `_hmc`"""
    sysm, chain, disc = small_problem(npde)
    kw = dict(draw_samples=2000, phystd=[0.5], bcstd=[0.5], priorsNNw=(0.0, 1.0))
    dev = npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", kernel="nuts", max_depth=5, seed=3, **kw)
    host = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(4), n_leapfrog=5, **kw)
    assert dev.stats["sampler"] == "device" and dev.stats["kernel"] == "nuts" and dev.samples.shape == (2000, 7) and dev.stats["n_adapts"] == 200
    xs = np.array([0.0, 0.5, 1.0])

    def predict(sol):
        S = sol.samples[500:]
        W1, b1, W2, b2 = S[:, 0:2], S[:, 2:4], S[:, 4:6], S[:, 6]
        return np.stack([np.sum(W2 * np.tanh(W1 * x + b1), axis=1) + b2 for x in xs], axis=1)

    pd_, ph = predict(dev), predict(host)
    acc = dev.stats["acceptance"][200:].mean()
    print(f"resident nuts known target: u(0, .5, 1) device mean {pd_.mean(axis=0)} sd {pd_.std(axis=0)}; host hmc mean {ph.mean(axis=0)} sd {ph.std(axis=0)}; "
          f"accept_stat {acc:.3f} mean leaves {dev.stats['n_leapfrog'][200:].mean():.2f} divergent {int(dev.stats['divergent'].sum())}")
    assert np.all(np.abs(pd_.mean(axis=0) - ph.mean(axis=0)) < 0.25 * np.minimum(pd_.std(axis=0), ph.std(axis=0)))
    assert np.all(np.abs(pd_.std(axis=0) / ph.std(axis=0) - 1.0) < 0.25)
    assert 0.6 < acc <= 1.0


def body_refusals(npde, precision):
    """case 7: every refusal is named and leaves the chain where it was: a following draw is bit-equal to that of an untouched handle"""
    D, eps = 3, 2.0e-2
    rep, th0, stds, nn, priors = forward_problem(npde, precision)
    eng = rep.engine
    L, dp, ip = eng.L, C.POINTER(C.c_double), C.POINTER(C.c_int)
    acc, lp, smp = np.zeros(4), np.zeros(4), np.zeros((4, eng.P))
    dep, nl, dv = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(dp)
    iptr = lambda a: None if a is None else a.ctypes.data_as(ip)

    def call(nd=1, depth=D, e=eps, dmax=1000.0, p=None, a=acc, l=lp, t=dep, n=nl, d=dv):
        return L.lib.pinn_nuts_draws(eng.h, nd, depth, e, dmax, 7, None, None, ptr(smp), eng.P if p is None else p,
                                     None if a is None else ptr(a), None if l is None else ptr(l), iptr(t), iptr(n), iptr(d))

    def refused(rc, *words):
        assert rc != 0
        msg = L.last_error()
        assert all(w in msg for w in words), msg

    refused(call(), "pinn_nuts_draws", "pinn_hmc_init first")
    eng.hmc_init(th0, stds, NN_PRIOR, [])
    eng.nuts_draws(1, D, eps, 7)
    ref = eng.hmc_get()
    refused(call(nd=0), "pinn_nuts_draws", "ndraws")
    refused(call(depth=0), "max_depth")
    refused(call(depth=11), "max_depth")
    refused(call(e=0.0), "eps")
    refused(call(e=float("inf")), "eps")
    refused(call(dmax=0.0), "delta_max")
    refused(call(dmax=float("nan")), "delta_max")
    refused(call(p=eng.P + 1), "ntheta")
    for kw in (dict(a=None), dict(l=None), dict(t=None), dict(n=None), dict(d=None)):
        refused(call(**kw), "pinn_nuts_draws", "null argument")
    eng.comm_init_custom(1, 0, lambda buf, count, dtype, stream: 0)
    refused(call(), "communicator")
    eng.comm_destroy()
    assert all(np.array_equal(a, b) for a, b in zip(eng.hmc_get(), ref))
    nxt = eng.nuts_draws(2, D, eps, 7)
    rep2, _, _, _, _ = forward_problem(npde, precision)
    e2 = rep2.engine
    e2.hmc_init(th0, stds, NN_PRIOR, [])
    e2.nuts_draws(1, D, eps, 7)
    assert all(np.array_equal(a, b) for a, b in zip(nxt, e2.nuts_draws(2, D, eps, 7)))
    eng.set_sampler(0, [0.0], [1.0], 11, seed=1)
    refused(call(), "pinn_nuts_draws", "fixed")


def body_mirror(npde):
    """case 8: kernel="nuts" with sampler="host" and "device" on the small problem; refusals; the defaults are untouched"""
    sysm, chain, disc = small_problem(npde)
    kw = dict(draw_samples=30, phystd=[0.5], bcstd=[0.5])
    for sampler in ("host", "device"):
        sol = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), seed=2, sampler=sampler, kernel="nuts", max_depth=4, **kw)
        st = sol.stats
        assert st["kernel"] == "nuts" and st["sampler"] == sampler and sol.samples.shape == (30, 7)
        assert set(st) >= {"acceptance", "step_size", "inv_metric", "n_adapts", "sampler", "kernel", "tree_depth", "n_leapfrog", "divergent"}
        assert all(len(st[q]) == 30 for q in ("acceptance", "tree_depth", "n_leapfrog", "divergent"))
        assert np.all((st["tree_depth"] >= 0) & (st["tree_depth"] <= 4)) and np.all((st["n_leapfrog"] >= 1) & (st["n_leapfrog"] <= 15))
        assert np.all(np.isfinite(sol.samples)) and all(np.all(np.isfinite(e)) for e in sol.ensemblesol + sol.ensemblestd)
    with pytest.raises(ValueError, match="adaptation"):
        npde.ahmc_bayesian_pinn_pde(sysm, disc, sampler="device", kernel="nuts", adaptation="device", **kw)
    with pytest.raises(ValueError, match="kernel"):
        npde.ahmc_bayesian_pinn_pde(sysm, disc, kernel="slice", **kw)
    a = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), n_leapfrog=3, **kw)
    b = npde.ahmc_bayesian_pinn_pde(sysm, disc, rng=np.random.default_rng(1), n_leapfrog=3, kernel="hmc", **kw)
    assert np.array_equal(a.samples, b.samples) and a.stats["kernel"] == "hmc" and "tree_depth" not in a.stats


# ------------------------------------------------------------------------------------------------------------------------------------
# the two faces of every body
# ------------------------------------------------------------------------------------------------------------------------------------
PARITY = [(p, m, d) for p in PRECISIONS for m in ("unit", "nonunit") for d in (3, 5)]


@pytest.mark.parametrize("precision,metric_kind,max_depth", PARITY)
def test_transition_parity(npde, use_emu, precision, metric_kind, max_depth):
    body_transition_parity(npde, precision, metric_kind, max_depth)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,metric_kind,max_depth", PARITY)
def test_transition_parity_gpu(npde, hip_lib, precision, metric_kind, max_depth):
    body_transition_parity(npde, precision, metric_kind, max_depth)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_branch_coverage(npde, use_emu, precision):
    body_branch_coverage(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_branch_coverage_gpu(npde, hip_lib, precision):
    body_branch_coverage(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_generator(npde, use_emu, precision):
    body_generator(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_generator_gpu(npde, hip_lib, precision):
    body_generator(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_and_reproducibility(npde, use_emu, precision):
    body_chunking(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_and_reproducibility_gpu(npde, hip_lib, precision):
    body_chunking(npde, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_isolation(npde, use_emu, precision):
    body_isolation(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_isolation_gpu(npde, hip_lib, precision):
    body_isolation(npde, precision)


def test_known_target(npde, use_emu):
    body_known_target(npde)


@pytest.mark.gpu
def test_known_target_gpu(npde, hip_lib):
    body_known_target(npde)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(npde, use_emu, precision):
    body_refusals(npde, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_gpu(npde, hip_lib, precision):
    body_refusals(npde, precision)


def test_mirror(npde, use_emu):
    body_mirror(npde)


@pytest.mark.gpu
def test_mirror_gpu(npde, hip_lib):
    body_mirror(npde)
