"""Launch geometry of the kernels: the host code that cuts a problem into launches (csrc/f64.cpp: f64_buffers, f64_short_blocks,
f64_make_groups; the fp32 plan's tiles) against the float64 oracle at the point counts where those cuts change — chunked float64 launches
(a forced scratch budget, $PINN_F64_SCRATCH_MB), the merged-group fallback, the short-dW-block ladder, the merge limit and every family's
tile edges (n = 1, 2, tile - 1, tile, tile + 1, 2 tile + 1).  Each case also agrees with the same handle's unchunked / unmerged / long-block
run to 1e-13, so a wrong chunk offset, a sum initialised twice or a padded lane counted twice fails here even where the oracle bar is wide.
(CPU: the g++ emulation; tests/test_gpu_mirror.py re-runs this module on the hardware.)"""
import contextlib
import os
import re

import numpy as np
import pytest
import sympy as sp
import torch

import helpers
import pinn_oracle as po
import test_emu_parity as tp
from test_f64_mode import EXACT, _engine_f64, _stencil_noise

SAME = 1e-13            # chunked against unchunked (merged against unmerged, short against long blocks) on one handle: rounding only
FP32 = 1e-5             # the suite's fp32 bar (tests/test_emu_parity.py: TOL)


@contextlib.contextmanager
def _env(**kv):
    """set (value str) or unset (None) environment toggles of the float64 host code for the block; restore them afterwards"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _chunked():
    return _env(PINN_F64_SCRATCH_MB="1")        # the smallest budget: 512-point chunks for every net of this module (f64.cpp: f64_buffers)


def _close(a, b, tol=SAME):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b)) <= tol * max(np.max(np.abs(b)), 1e-300)


def _at_oracle(l, g, ref, bar=EXACT, loss_floor=0.0):
    """loss_floor: per-term loss errors relative to max(|loss_k|, loss_floor * max_k |loss_k|) (a 1-point fp32 term whose residual is a
    small difference of O(1) network outputs carries the absolute, not the relative, fp32 error)"""
    le, g2, gi = helpers.rel_errors(l, g, ref)
    if loss_floor:
        lr = np.abs(ref.term_losses)
        le = np.abs(np.asarray(l) - ref.term_losses) / np.maximum(lr, loss_floor * lr.max())
    assert le.max() < bar and g2 < bar and gi < bar, (le, g2, gi)


def _u(cord, th, phi):
    return phi(cord, th)


def _derivative_ref(chain, th, pts, axes):
    tht = torch.tensor(np.asarray(th[:chain.nparams], dtype=np.float64), dtype=po.DT)
    x = torch.tensor(pts, dtype=po.DT)
    return po.exact_derivative(chain, _u, x, axes, tht).detach().numpy().reshape(-1)


# ---- A1 / A2: chunked float64 evaluation ----
def _chunk_workloads():
    from neuralpde_jl_amd import workloads
    return {"cfg2": (lambda: workloads.cfg2_poisson2d(points=1500, bcs_points=600), [0, 0]),       # 3 chunks (the last 476 points), 2 per wall
            "cfg3": (lambda: workloads.cfg3_burgers(points=1300, bcs_points=40), [1, 1]),
            "cfg5": (lambda: workloads.cfg5_heat_inverse(points=1200, bcs_points=24, width=16, hidden=2), [1, 1])}    # estimated parameter


def _chunk_parity(npde, rep, eng, sets, prob, th, w, deriv_axes, nomfma, ref=None):
    """every float64 entry point of `eng` with forced 512-point chunks: = the oracle (`ref` replaces the loss / gradient oracle where the
    module builds it itself) and = the same handle unchunked"""
    lanes = "1" if nomfma else None
    K = eng.K
    pts = np.random.default_rng(17).uniform(0.0, 1.0, size=(sets[0].shape[0], 2600))
    ks = (0, K - 1)

    def run():
        l, g = eng.loss_grad_f64(th, w)
        nch = int(eng.get_option("f64_chunks"))
        path = eng.get_option("f64_path")
        lo, _ = eng.loss_grad_f64(th, w, want_grad=False)
        res = {k: eng.residual_f64(k, th, sets[k].shape[1]) for k in ks}
        phi = eng.phi_f64(0, th, pts)
        nch_v = int(eng.get_option("f64_chunks"))
        der = eng.derivative_f64(0, th, pts, deriv_axes)
        nch_v = min(nch_v, int(eng.get_option("f64_chunks")))
        return l, g, lo, res, phi, der, nch, nch_v, path

    with _env(PINN_F64_NO_MFMA=lanes, PINN_F64_SCRATCH_MB=None):
        base = run()
    with _env(PINN_F64_NO_MFMA=lanes, PINN_F64_SCRATCH_MB="1"):
        got = run()
        # the float entry points of the same handle: the double evaluation narrowed at the boundary
        f32 = lambda a: np.asarray(a, dtype=np.float32)
        th32, w32 = f32(th).astype(np.float64), f32(w).astype(np.float64)
        lf, gf = eng.loss_grad(f32(th), f32(w))
        ld, gd = eng.loss_grad_f64(th32, w32)
        assert np.array_equal(lf, ld) and np.array_equal(gf, f32(gd))
        assert np.array_equal(eng.residual(K - 1, f32(th), sets[K - 1].shape[1]), f32(eng.residual_f64(K - 1, th32, sets[K - 1].shape[1])))
        assert np.array_equal(eng.phi(0, f32(th), f32(pts)), f32(eng.phi_f64(0, th32, f32(pts).astype(np.float64))))
    l, g, lo, res, phi, der, nch, nch_v, path = got
    assert path == ("lanes" if nomfma else "mfma")
    # the default budget holds each set in one launch; 1 MB does not (value-only launches keep fewer rows per point: larger chunks)
    assert base[6] == 1 and base[7] == 1 and nch >= 3 and nch_v >= 2, (base[6], base[7], nch, nch_v)
    ref = ref if ref is not None else po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
    _at_oracle(l, g, ref)
    assert _close(l, base[0]) and _close(g, base[1]) and _close(lo, base[2]) and _close(lo, l)
    for k in ks:
        rr = po.residual_values(prob, th, k, sets[k], mode="exact").reshape(-1)
        assert np.max(np.abs(res[k] - rr)) < 1e-12 * max(1.0, np.max(np.abs(rr))), k
        assert _close(res[k], base[3][k]), k
    ph = po.phi_values(prob.chains[0], th[:prob.chains[0].nparams], pts).reshape(-1)
    assert np.max(np.abs(phi - ph)) < 1e-13 * max(1.0, np.max(np.abs(ph)))
    dr = _derivative_ref(prob.chains[0], th, pts, deriv_axes)
    assert np.max(np.abs(der - dr)) < 1e-12 * max(1.0, np.max(np.abs(dr)))
    assert _close(phi, base[4]) and _close(der, base[5])
    return nch


@pytest.mark.parametrize("name,nomfma", [(c, f) for c in ("cfg2", "cfg3", "cfg5") for f in (False, True)])      # (one mark: the hardware mirror)
def test_chunked_f64_evaluation(npde, use_emu, name, nomfma):
    """A1: a 1 MB scratch budget cuts every set into 512-point chunks (>= 3 on the interior term, the last one ragged): losses, gradient,
    loss-only sums, residuals of the first and last term, trial function and a derivative at 2,600 host points, the float entry points —
    on the matrix-pipe and on the lane-per-point family"""
    make, axes = _chunk_workloads()[name]
    rep, eng, sets, prob = _engine_f64(npde, make())
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = np.linspace(0.5, 3.0, eng.K)[::-1].copy()
    _chunk_parity(npde, rep, eng, sets, prob, th, w, axes, nomfma)


def _weighted_ref(prob, th, sets, w, k_pw, q):
    """losses / weighted gradient when term k_pw carries the stored quadrature factors q (loss_k = sum (q r)^2 / N)"""
    tt = torch.tensor(th, dtype=po.DT, requires_grad=True)
    terms = list(prob.pde_terms) + list(prob.bc_terms)
    total, losses = 0.0, []
    for k, s in enumerate(sets):
        r = po.build_residual(prob, terms[k], mode="exact")(torch.tensor(s, dtype=po.DT), tt).reshape(-1)
        if k == k_pw:
            r = r * torch.tensor(q, dtype=po.DT)
        lk = torch.mean(r * r)
        losses.append(float(lk.detach()))
        total = total + w[k] * lk
    (g,) = torch.autograd.grad(total, tt)
    return po.Evaluation(np.array(losses), float(total.detach()), g.numpy(), None)


@pytest.mark.parametrize("nomfma", [False, True])
def test_chunked_f64_quadrature_weights_and_data_rows(npde, use_emu, nomfma):
    """A2: inputs indexed by the GLOBAL point (quadrature weights, per-point DATA rows) under forced chunks — a chunk that read its own
    first rows instead of rows p0 .. p0 + n fails here first"""
    from neuralpde_jl_amd import workloads
    wl = workloads.cfg2_poisson2d(points=1300, bcs_points=40, width=16, hidden=2)
    rep, eng, sets, prob = _engine_f64(npde, wl)
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = np.array([1.5, 2.0, 0.5, 1.0, 3.0])
    n = sets[0].shape[1]
    wq = (np.random.default_rng(5).uniform(0.2, 2.0, n) / n).astype(np.float32)
    eng.set_point_weights(0, wq)
    q = np.sqrt(wq.astype(np.float64) * n).astype(np.float32).astype(np.float64)      # what pinn_set_point_weights stores
    ref = _weighted_ref(prob, th, sets, w, 0, q)
    _chunk_parity(npde, rep, eng, sets, prob, th, w, [0, 0], nomfma, ref=ref)
    # per-point DATA rows: the misfit term of test_f64_mode_data_misfit_term_and_estimated_parameter at 3,000 observations
    t, x = npde.parameters("t x")
    (u,) = npde.variables("u")
    (k,) = npde.parameters("k")
    Dt, Dxx = npde.Differential(t), npde.Differential(x) ** 2
    sysm = npde.PDESystem([npde.Eq(Dt(u(t, x)), k * Dxx(u(t, x)))], [npde.Eq(u(0, x), sp.sin(sp.pi * x)), npde.Eq(u(t, 0), 0.0)],
                          [npde.In(t, npde.Interval(0.0, 1.0)), npde.In(x, npde.Interval(0.0, 1.0))], [t, x], [u(t, x)], ps=[k], defaults={k: 0.7})
    chain = npde.Chain(npde.Dense(2, 16, "tanh"), npde.Dense(16, 16, "tanh"), npde.Dense(16, 1))
    th0 = npde.initialparameters(np.random.default_rng(171), chain)
    strat = npde.QuasiRandomTraining(40, bcs_points=16, sampling_alg=npde.SobolSample(seed=8), resampling=False, minibatch=1)
    pts = np.random.default_rng(3).uniform(size=(2, 3000))
    vals = np.exp(-0.3 * np.pi ** 2 * pts[0]) * np.sin(np.pi * pts[1]) + 0.01 * np.cos(7 * pts[0])
    weights = npde.NonAdaptiveLoss(pde_loss_weights=1.0, bc_loss_weights=2.0, additional_loss_weights=0.5)
    dprob = npde.discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=th0, param_estim=True, precision="f64", adaptive_loss=weights,
                                                         data_loss=[npde.DataLoss(u(t, x), pts, vals, weight=3.0)]))
    eng = dprob.pinnrep.engine
    theta = np.asarray(dprob.pinnrep.flat_init_params, dtype=np.float64)
    oc = po.Chain(tuple(chain.sizes), chain.act)
    u_at = po.phi_values(oc, theta[:chain.nparams], pts).reshape(-1)
    kd = eng.K - 1
    with _env(PINN_F64_NO_MFMA="1" if nomfma else None):
        base = eng.loss_grad_f64(theta)
        r0 = eng.residual_f64(kd, theta, pts.shape[1])
        with _chunked():
            l, g = eng.loss_grad_f64(theta)
            assert int(eng.get_option("f64_chunks")) >= 2
            r = eng.residual_f64(kd, theta, pts.shape[1])
    tt = torch.tensor(theta[:chain.nparams], dtype=po.DT, requires_grad=True)
    mis = torch.mean((oc(torch.tensor(pts, dtype=po.DT), tt).reshape(-1) - torch.tensor(vals, dtype=po.DT)) ** 2)
    (gm,) = torch.autograd.grad(mis, tt)
    assert abs(l[kd] - float(mis)) < EXACT * float(mis)
    np.testing.assert_allclose(r, u_at - vals, rtol=0, atol=1e-13)
    assert _close(l, base[0]) and _close(g, base[1]) and _close(r, r0)
    # the misfit's share of the gradient: the full gradient minus the physics terms' (the same handle with the misfit weighted 0)
    wts = np.ones(eng.K)
    wts[kd] = 0.0
    with _chunked(), _env(PINN_F64_NO_MFMA="1" if nomfma else None):
        l1, g1 = eng.loss_grad_f64(theta, np.where(np.arange(eng.K) == kd, 1.0, 0.0))
    assert np.linalg.norm(g1[:chain.nparams] - gm.numpy()) < EXACT * np.linalg.norm(gm.numpy())


# ---- A3: chunked stencil mode ----
@pytest.mark.parametrize("name", ["cfg2", "mixed"])
def test_chunked_stencil_mode(npde, use_emu, name):
    """A3: derivative = "stencil" with forced chunks (shifted-set value launches, seeded dW launches, the first chunk of the first virtual
    network initialising the sums): against the stencil oracle at its noise floor, and = the unchunked run"""
    from neuralpde_jl_amd import workloads
    if name == "cfg2":
        wl = workloads.cfg2_poisson2d(points=1100, bcs_points=24, width=16, hidden=2)
    else:
        sysm, chain = helpers.shape_problem(npde, 16, 2, 2)
        strat = npde.QuasiRandomTraining(1100, bcs_points=24, sampling_alg=npde.SobolSample(seed=6), resampling=False, minibatch=1)
        wl = workloads.Workload("mixed", sysm, [chain], strat, tp.theta_for(chain, 61))
    rep, eng, sets, prob = _engine_f64(npde, wl)
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = np.linspace(2.0, 1.0, eng.K)
    eng.set_option("derivative", "stencil")
    l0, g0 = eng.loss_grad_f64(th, w)
    r0 = eng.residual_f64(0, th, sets[0].shape[1])
    with _chunked():
        l, g = eng.loss_grad_f64(th, w)
        assert int(eng.get_option("f64_chunks")) >= 2             # (value launches of the shifted sets keep few rows per point: larger chunks)
        lo, _ = eng.loss_grad_f64(th, w, want_grad=False)
        r = eng.residual_f64(0, th, sets[0].shape[1])
    st = po.loss_and_grad(prob, th, sets, weights=w, mode="stencil")
    noise = _stencil_noise(prob, th, sets, w, st)
    # per point the chunked launches compute the same numbers (residuals bit-equal, losses to rounding); the gradient sums seeds of size
    # r / eps^2 that cancel between the shifted evaluations, in another order per chunk — its rounding is the stencil's own noise floor
    assert np.array_equal(r, r0) and _close(l, l0) and _close(lo, l0)
    assert np.linalg.norm(g - g0) / np.linalg.norm(g0) < max(noise[1], 2e-9), (np.linalg.norm(g - g0) / np.linalg.norm(g0), noise)
    le, g2, gi = helpers.rel_errors(l, g, st)
    assert le.max() < 4 * max(noise[0], 2e-9) and g2 < 4 * max(noise[1], 2e-9) and gi < 4 * max(noise[2], 2e-9), (le, g2, gi, noise)
    rr = po.residual_values(prob, th, 0, sets[0], mode="stencil")
    assert np.max(np.abs(r - rr)) < 2e-6 * max(1.0, np.max(np.abs(rr)))


# ---- A4: a merged group larger than one chunk ----
def test_merged_group_larger_than_a_chunk_falls_back(npde, use_emu):
    """A4: a small multi-term problem merges into one launch sequence by default; with a chunk below the group's tiled point total (> 512)
    the members go one by one (f64.cpp: `chunk < a.npts`), the interior term itself chunked — same numbers as the merged launch, = the oracle"""
    sysm, chain = tp.poisson2d(npde, "tanh", width=16, hidden=2)
    strat = npde.QuasiRandomTraining(600, bcs_points=40, sampling_alg=npde.SobolSample(seed=4), resampling=False, minibatch=1)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=tp.theta_for(chain, 44), precision="f64"))
    eng = rep.engine
    sets = rep.pde_train_sets + rep.bcs_train_sets
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = [1.0, 2.0, 0.5, 1.5, 3.0]
    l0, g0 = eng.loss_grad_f64(th, w)
    assert int(eng.get_option("f64_merged")) == 1 and int(eng.get_option("f64_chunks")) == 1
    with _chunked():
        l, g = eng.loss_grad_f64(th, w)
        assert int(eng.get_option("f64_merged")) == 0 and int(eng.get_option("f64_chunks")) == 2
        lo, _ = eng.loss_grad_f64(th, w, want_grad=False)
        assert int(eng.get_option("f64_merged")) == 0
    l1, g1 = eng.loss_grad_f64(th, w)
    assert int(eng.get_option("f64_merged")) == 1 and np.array_equal(l1, l0) and np.array_equal(g1, g0)
    ref = po.loss_and_grad(helpers.oracle_problem(npde, sysm, [chain]), th, sets, weights=w, mode="exact")
    _at_oracle(l, g, ref)
    _at_oracle(l0, g0, ref)
    assert _close(l, l0) and _close(g, g0) and _close(lo, l)


# ---- A5: the short-dW-block ladder ----
def _short_block(npts, rows, tile_pts):
    """f64.cpp: f64_short_blocks — block points of one matrix-pipe launch of npts points (512 = no short blocks)"""
    bp = 512
    if 64 % tile_pts != 0:
        return bp
    while bp > 64 and -(-npts // bp) * rows < 512:
        bp >>= 1
    return bp


def _ladder_counts(rows, tile_pts):
    """the point counts around each switch of the ladder (512 -> 256 -> 128 -> 64) and one that leaves a partial last 64-point block"""
    out = set()
    for lo_bp in (256, 128, 64):
        last = max(n for n in range(1, 512 * 512) if _short_block(n, rows, tile_pts) <= lo_bp)      # the largest count with blocks <= lo_bp
        assert _short_block(last + 1, rows, tile_pts) == 2 * lo_bp
        out |= {last - 1, last, last + 1}
    out.add(64 * 5 + 37)
    return sorted(out)


@pytest.mark.parametrize("width", [16])
def test_short_block_ladder(npde, use_emu, width):
    """A5: interior point counts at every switch point of the short-block ladder and +- 1 (the rows of the formula from the net's depth,
    the switch points from the formula), each = the oracle and = long blocks (PINN_F64_NO_SHORT_BLOCKS) on the same handle.  A deep net puts
    the switch points within the emulation's reach: rows = 1 + hidden-to-hidden layers (a deep 64-wide 1-D net runs on the channel-sliced
    family, which takes no short blocks)."""
    hidden = 12 if width == 64 else 15
    sysm, chain = helpers.shape_problem(npde, width, hidden, 1)
    rows = 1 + (hidden - 1)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.01), init_params=tp.theta_for(chain, 90 + width), precision="f64"))
    eng = rep.engine
    m = re.search(r"mfma:HT\d+xPG(\d+)", eng.describe())        # (term 0: family 4m, the ladder's precondition)
    assert m, eng.describe()
    tile = 16 * int(m.group(1))
    counts = _ladder_counts(rows, tile)
    assert max(counts) < 20000, counts
    prob = helpers.oracle_problem(npde, sysm, [chain])
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    grid = np.linspace(0.0, 1.0, max(counts))[None, :]
    bsets = [s[:, :1] for s in rep.bcs_train_sets]
    w = [1.0, 2.0, 0.5]
    with _env(PINN_F64_NO_MERGE="1"):          # (each term its own launch: the interior launch has exactly n points)
        for n in counts:
            sets = [grid[:, np.linspace(0, grid.shape[1] - 1, n).astype(int)]] + bsets
            for k, s in enumerate(sets):
                eng.set_points_f64(k, s)
            l, g = eng.loss_grad_f64(th, w)
            assert eng.get_option("f64_path") == "mfma" and int(eng.get_option("f64_merged")) == 0
            with _env(PINN_F64_NO_SHORT_BLOCKS="1"):
                ll, gl = eng.loss_grad_f64(th, w)
            assert _close(l, ll) and _close(g, gl), n
            ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
            _at_oracle(l, g, ref)


# ---- A6: merge limits ----
def test_merge_limits(npde, use_emu):
    """A6: total point counts 8191 / 8192 / 8193 over terms that do not share a kernel (a second-derivative interior term and value-only
    boundary terms), a 1-point boundary term next to a 5,000-point interior term, the Lorenz-style union of networks — merged (where the
    limit allows) = term by term (PINN_F64_NO_MERGE, set before the handle's first evaluation) = the oracle"""
    sysm, chain = tp.poisson2d(npde, "tanh", width=16, hidden=2)
    prob = helpers.oracle_problem(npde, sysm, [chain])
    theta = tp.theta_for(chain, 66)
    rng = np.random.default_rng(9)
    w = [1.0, 2.0, 0.5, 1.5, 3.0]

    def sets_for(n_int, n_bc):
        s = [rng.uniform(0.0, 1.0, size=(2, n_int))]
        for k, n in enumerate(n_bc):
            b = rng.uniform(0.0, 1.0, size=(2, n))
            b[k // 2] = float(k % 2)
            s.append(b)
        return s

    def both(sets, expect):
        out = []
        for merge in (True, False):
            with _env(PINN_F64_NO_MERGE=None if merge else "1"):
                rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.25), init_params=theta, precision="f64"))
                eng = rep.engine
                for k, s in enumerate(sets):
                    eng.set_points_f64(k, s)
                th = np.asarray(rep.flat_init_params, dtype=np.float64)
                l, g = eng.loss_grad_f64(th, w)
                out.append((l, g, int(eng.get_option("f64_merged"))))
        assert out[0][2] == expect and out[1][2] == 0, (sum(s.shape[1] for s in sets), out[0][2])
        assert _close(out[0][0], out[1][0]) and _close(out[0][1], out[1][1])
        _at_oracle(out[0][0], out[0][1], po.loss_and_grad(prob, th, sets, weights=w, mode="exact"))

    both(sets_for(8191 - 4, [1, 1, 1, 1]), 1)                  # 8191 points: one launch sequence
    both(sets_for(8192 - 4, [1, 1, 1, 1]), 1)                  # 8192: at the limit, still one
    both(sets_for(8193 - 4, [1, 1, 1, 1]), 1)                  # 8193: the interior term alone, the four boundary terms (same kernel) together
    both(sets_for(8193 - 40, [10, 10, 10, 10]), 1)
    both(sets_for(5000, [1, 37, 1, 200]), 1)                   # 1-point boundary terms next to a 5,000-point interior term
    # the Lorenz-style system: three networks, equations over different subsets of them, estimated parameters; ragged sets of 1 .. 300 points
    (tt,) = npde.parameters("t")
    sg, rho, beta = npde.parameters("sigma_ rho beta")
    xv, yv, zv = npde.variables("x y z")
    D = npde.Differential(tt)
    eqs = [npde.Eq(D(xv(tt)), sg * (yv(tt) - xv(tt))), npde.Eq(D(yv(tt)), xv(tt) * (rho - zv(tt)) - yv(tt)), npde.Eq(D(zv(tt)), xv(tt) * yv(tt) - beta * zv(tt))]
    ics = [npde.Eq(xv(0), 1.0), npde.Eq(yv(0), 0.0), npde.Eq(zv(0), 0.0)]
    lsys = npde.PDESystem(eqs, ics, [npde.In(tt, npde.Interval(0.0, 1.0))], [tt], [xv(tt), yv(tt), zv(tt)], ps=[sg, rho, beta],
                          defaults={sg: 1.0, rho: 1.0, beta: 1.0})
    chains = [npde.Chain(npde.Dense(1, 12, "tanh"), npde.Dense(12, 12, "sigmoid"), npde.Dense(12, 1)) for _ in range(3)]
    th0 = np.concatenate([tp.theta_for(c, 40 + i) for i, c in enumerate(chains)])
    lsets = [rng.uniform(0.0, 1.0, size=(1, n)) for n in (300, 1, 17)] + [np.zeros((1, 1))] * 3
    lw = [1.0, 2.0, 0.5, 1.5, 3.0, 0.7]
    res = []
    for merge in (True, False):
        with _env(PINN_F64_NO_MERGE=None if merge else "1"):
            rep = npde.symbolic_discretize(lsys, npde.PhysicsInformedNN(chains, npde.GridTraining(0.05), init_params=th0, param_estim=True))
            for k, s in enumerate(lsets):
                rep.engine.set_points_f64(k, s)
            th = np.asarray(rep.flat_init_params, dtype=np.float64) + 1e-9
            l, g = rep.engine.loss_grad_f64(th, lw)
            res.append((l, g, int(rep.engine.get_option("f64_merged"))))
    assert res[0][2] == 1 and res[1][2] == 0
    assert _close(res[0][0], res[1][0]) and _close(res[0][1], res[1][1])
    ref = po.loss_and_grad(helpers.oracle_problem(npde, lsys, chains, param_estim=True), th, lsets, weights=lw, mode="exact")
    _at_oracle(res[0][0], res[0][1], ref)


# ---- A7: the point-count ladder of every kernel family ----
def _ladder(tile):
    return sorted({1, 2, tile - 1, tile, tile + 1, 2 * tile + 1})


def _fp32_tile(eng, n_probe, nbc):
    """the tile of the fp32 kernel that serves term 0, from the plan's own tile count for an n_probe-point interior set and 1-point
    boundary sets (group lines of pinn_describe: tiles = sum over the group's terms of ceil(n / TP))"""
    for line in eng.describe().splitlines():
        m = re.search(r" tiles=(\d+) .*terms=([\d,]+)", line)
        if m and "0" in m.group(2).split(","):
            tiles = int(m.group(1))
            others = len([t for t in m.group(2).split(",") if t and t != "0"])
            cands = [tp_ for tp_ in (16, 32, 64, 128) if -(-n_probe // tp_) + others == tiles]
            assert len(cands) == 1, (line, cands)
            return cands[0]
    raise AssertionError(eng.describe())


def _fp32_family(npde, name):
    if name.startswith("wave"):
        width = int(name[4:])
        sysm, chain = tp.poisson2d(npde, "tanh", width=width, hidden=2)
    elif name.startswith("split"):
        width = int(name.split("_")[0][5:])
        sysm, chain = tp.poisson2d(npde, "tanh", width=width, hidden=4 if width == 64 else 2)
    else:
        from test_dgm import _burgers
        sysm, chain = _burgers(npde), npde.DGM(2, 1, 12, 2, "tanh", "tanh", "identity")
    return sysm, chain


@pytest.mark.parametrize("name", ["wave8", "wave16", "wave32", "split64_split", "split64_fp32", "split128_split", "split128_fp32", "dgm"])
def test_point_count_ladder_fp32(npde, use_emu, name):
    """A7, fp32 families (one-wave kernels 8 / 16 / 32 wide, neuron-split kernels 64 / 128 wide in both GEMM modes, the DGM family): interior
    sets of 1, 2, tile - 1, tile, tile + 1, 2 tile + 1 points next to 1-point boundary terms, = the oracle at 1e-5"""
    sysm, chain = _fp32_family(npde, name)
    theta = tp.theta_for(chain, 300 + len(name))
    probe = 1000
    strat = npde.QuasiRandomTraining(probe, bcs_points=1, sampling_alg=npde.SobolSample(seed=2), resampling=False, minibatch=1)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=theta, precision="f32"))
    eng = rep.engine
    if name.endswith("_fp32"):
        eng.set_option("gemm", "fp32")
    sets0 = rep.pde_train_sets + rep.bcs_train_sets
    assert sets0[0].shape[1] == probe and all(s.shape[1] == 1 for s in sets0[1:])
    tile = _fp32_tile(eng, probe, len(sets0) - 1)
    prob = helpers.oracle_problem(npde, sysm, [chain])
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = list(np.linspace(1.0, 2.5, eng.K))
    for n in _ladder(tile):
        sets = [sets0[0][:, :n]] + sets0[1:]
        eng.set_points(0, sets[0])
        l, g = eng.loss_grad(th, w)
        _at_oracle(l, g, po.loss_and_grad(prob, th, sets, weights=w, mode="exact"), bar=FP32, loss_floor=0.1)


@pytest.mark.parametrize("family", ["4m", "4s", "lanes"])
def test_point_count_ladder_f64(npde, use_emu, family):
    """A7, float64 families (matrix-pipe tiles of 16 PG points, channel-sliced tiles, one lane per point in 64-lane waves): the same ladder
    on the interior term next to 1-point boundary terms, = the oracle to rounding"""
    sysm, chain = tp.poisson2d(npde, "tanh", width=128 if family == "4s" else 16, hidden=2)
    theta = tp.theta_for(chain, 500 + len(family))
    strat = npde.QuasiRandomTraining(300, bcs_points=1, sampling_alg=npde.SobolSample(seed=3), resampling=False, minibatch=1)
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, strat, init_params=theta, precision="f64"))
    eng = rep.engine
    kinds = re.findall(r"(mfma-sliced|mfma|lanes)(?::HT\d+xPG(\d+))?", eng.describe().split("f64_kernels=", 1)[1].split()[0])
    assert kinds, eng.describe()
    if family == "lanes":
        tile = 64
    else:
        assert kinds[0][0] == ("mfma-sliced" if family == "4s" else "mfma"), kinds
        tile = 16 * int(kinds[0][1])
    sets0 = rep.pde_train_sets + rep.bcs_train_sets
    prob = helpers.oracle_problem(npde, sysm, [chain])
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = list(np.linspace(1.0, 2.5, eng.K))
    with _env(PINN_F64_NO_MFMA="1" if family == "lanes" else None):
        for n in _ladder(tile):
            sets = [sets0[0][:, :n]] + sets0[1:]
            eng.set_points_f64(0, sets[0])
            l, g = eng.loss_grad_f64(th, w)
            assert eng.get_option("f64_path") == ("lanes" if family == "lanes" else "mfma")
            _at_oracle(l, g, po.loss_and_grad(prob, th, sets, weights=w, mode="exact"))
            r = eng.residual_f64(0, th, n)
            rr = po.residual_values(prob, th, 0, sets[0], mode="exact").reshape(-1)
            assert np.max(np.abs(r - rr)) < 1e-12 * max(1.0, np.max(np.abs(rr))), n
