"""Random residual programs (tests/residual_gen.py) against the float64 oracle in exact mode: the planner's graph rewrites — coordinate-only
subexpressions hoisted into source channels, second derivatives fused into one Laplacian channel, the fp32 and the float64 affine shortcuts,
boundary terms riding on the interior launch, coupled / tail / two-launch paths, both front ends — on equations nobody wrote by hand.
Per case: fp32 losses and gradient (the suite's 1e-5 with the loss floor of test_launch_geometry._at_oracle), the pointwise residual of
every term, the float64 mode of the same handle at 1e-11 / 1e-12, repeatability, and for a quarter of the seeds the same again on
reinstalled (permuted, shrunk) point sets.  The reference's own sensitivity to float32 inputs (q) bounds how ill-conditioned a committed seed
may be; the coverage conditions keep the generator on the rewrites.  Each case prints its figures before it asserts (`pytest -s`).
(CPU: the g++ emulation; tests/test_gpu_mirror.py re-runs this module on the hardware.)"""
import os
import re

import numpy as np
import pytest

import helpers
import pinn_oracle as po
import residual_gen as rg
from test_f64_mode import EXACT
from test_launch_geometry import FP32, _at_oracle

Q_MAX = 2e-6                    # the oracle at float32(theta, points) against the oracle at the double inputs: conditioning of a committed seed
LOSS_FLOOR = 0.1
# committed seeds per family and seeds per test (about 0.15 s per 2 x 16 case and 1.3 s per 4 x 64 case on the emulation).
# params 35 is replaced by 51 (the same kind of case: one network, estimated parameters, symbolic front end): its reference alone moves by
# q = 2.09e-6 under float32 inputs, past Q_MAX
SEEDS = {"single": (list(range(144)), 12), "wide": (list(range(24)), 4), "system": (list(range(60)), 12),
         "params": ([s for s in range(48) if s != 35] + [51], 12), "long": (list(range(16)), 8)}
assert all(len(seeds) % per == 0 for seeds, per in SEEDS.values())
BATCHES = [(f, b) for f, (seeds, per) in SEEDS.items() for b in range(len(seeds) // per)]

REJECTED = {}                   # (backend, family) -> seeds whose draw was rejected for a structural reason (never for an error size)
_PLANS = {}                     # (backend, family, seed) -> what the planner made of the case (describe(), f64_affine) + the generator's record


def _backend(npde):
    return npde._lib.default_library().backend


def _build(npde, monkeypatch, family, seed):
    """the case of (family, seed) on a fresh fp32 handle; a draw whose equation simplifies to one without a dependent variable (the mirror's
    LoweringError) is replaced by the next seed of its replacement stream, seed + 1000"""
    s = seed
    while True:
        c = rg.case(npde, family, s)
        if c.symbolic:
            monkeypatch.setenv("PINN_DESCRIPTOR", "2")
        else:
            monkeypatch.delenv("PINN_DESCRIPTOR", raising=False)
        disc = npde.PhysicsInformedNN(c.chains if len(c.chains) > 1 else c.chains[0], rg.strategy(npde, s), init_params=c.theta,
                                      param_estim=c.param_estim, precision="f32")
        try:
            rep = npde.symbolic_discretize(c.sysm, disc)
        except npde.LoweringError as e:
            if "does not contain a dependent variable" not in str(e):
                raise
            REJECTED.setdefault((_backend(npde), family), set()).add(s)
            s += 1000
            assert s < seed + 4000, (family, seed)
            continue
        finally:
            monkeypatch.delenv("PINN_DESCRIPTOR", raising=False)
        return c, rep


def _plan(npde, monkeypatch, family, seed, built=None):
    key = (_backend(npde), family, seed)
    if key in _PLANS and "K" in _PLANS[key]:
        return _PLANS[key]
    c, rep = built if built is not None else _build(npde, monkeypatch, family, seed)
    eng = rep.engine
    n_pde = len(c.sysm.eqs)
    rec = dict(c.record, lap=False, affine32=0, tape32=0, hoisted=0, riding=False, two_launch=False, tail=False)
    for line in eng.describe().splitlines():
        m = re.match(r"group \d+( \[[^\]]*\])? net=\d+ kernel=(\S+) .*terms=([\d,]+)", line)
        if m:
            terms = [int(t) for t in m.group(3).split(",") if t]
            how = m.group(1) or ""
            if any(t < n_pde for t in terms):
                tag = re.search(r"_L(\d+)_", m.group(2))
                rec["lap"] = rec["lap"] or bool(tag and int(tag.group(1)))
            rec["riding"] = rec["riding"] or len(terms) > 1
            rec["tail"] = rec["tail"] or "coupled tail" in how
            rec["two_launch"] = rec["two_launch"] or ("coupled" in how and len(c.chains) == 1)
        m = re.match(r"term (\d+): tape ops=\d+ of \d+, sources=(\d+) .*?(, affine residual)?", line)
        if m and int(m.group(1)) < n_pde:
            affine = "affine residual" in line
            rec["affine32"] += affine
            rec["tape32"] += not affine
            rec["hoisted"] += int(m.group(2)) > 0
    if built is None:                                          # (a checked case reads the count after its float64 evaluation)
        eng.set_option("precision", "f64")
        for k, s in enumerate(rep.pde_train_sets + rep.bcs_train_sets):
            eng.set_points_f64(k, s)
        eng.loss_grad_f64(np.asarray(rep.flat_init_params, dtype=np.float64))
        rec["f64_affine"], rec["K"] = int(eng.get_option("f64_affine")), eng.K
    _PLANS[key] = rec
    return rec


def _measures(l, g, ref, floor):
    """the three relative measures of _at_oracle"""
    le, g2, gi = helpers.rel_errors(l, g, ref)
    if floor:
        lr = np.abs(ref.term_losses)
        le = np.abs(np.asarray(l) - ref.term_losses) / np.maximum(lr, floor * lr.max())
    return float(le.max()), float(g2), float(gi)


def _pointwise(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)) / max(1.0, np.max(np.abs(ref))))


def _check_sets(eng, prob, th, w, sets, f64, tag, reference=None):
    """checks 1 - 4 of one precision on installed sets; returns the reference evaluation.  `reference(th, sets, w) -> (Evaluation, residual
    vectors)` replaces the oracle's exact mode where the oracle lacks a node (integral terms: tests/test_op_matrix.py)"""
    if reference is None:
        ref = po.loss_and_grad(prob, th, sets, weights=w, mode="exact")
        refs = [po.residual_values(prob, th, k, s, mode="exact").reshape(-1) for k, s in enumerate(sets)]
    else:
        ref, refs = reference(th, sets, w)
    if f64:
        l, g = eng.loss_grad_f64(th, w)
        res = [eng.residual_f64(k, th, s.shape[1]) for k, s in enumerate(sets)]
        l2, g2_ = eng.loss_grad_f64(th, w)
    else:
        l, g = eng.loss_grad(th, w)
        res = [eng.residual(k, th, s.shape[1]) for k, s in enumerate(sets)]
        l2, g2_ = eng.loss_grad(th, w)
    floor = 0.0 if f64 else LOSS_FLOOR
    fig = _measures(l, g, ref, floor) + (max(_pointwise(r, rr) for r, rr in zip(res, refs)),)
    print("RR", *tag, "f64" if f64 else "fp32", *("%.3e" % v for v in fig))
    _at_oracle(l, g, ref, bar=EXACT if f64 else FP32, loss_floor=floor)
    for k, (r, rr) in enumerate(zip(res, refs)):
        assert r.shape == rr.shape and np.max(np.abs(r - rr)) < (1e-12 if f64 else 2e-5) * max(1.0, np.max(np.abs(rr))), (tag, k)
    assert np.array_equal(l2, l) and np.array_equal(g2_, g), tag          # a second evaluation is bit-equal
    return ref


def _check_conditioning(prob, th, w, sets, ref, tag, reference=None):
    """q < Q_MAX: the oracle at float32-rounded inputs against the oracle at the double inputs (`ref`)"""
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    if reference is None:
        lo = po.loss_and_grad(prob, f32(th), [f32(s) for s in sets], weights=w, mode="exact")
    else:
        lo = reference(f32(th), [f32(s) for s in sets], w)[0]
    q = max(_measures(lo.term_losses, lo.grad, ref, LOSS_FLOOR))
    print("RR", *tag, "q", "%.3e" % q)
    assert q < Q_MAX, (tag, q)
    return q


def _check_case(npde, monkeypatch, family, seed):
    c, rep = _build(npde, monkeypatch, family, seed)
    eng = rep.engine
    tag = (_backend(npde), family, seed)
    prob = helpers.oracle_problem(npde, c.sysm, c.chains, param_estim=c.param_estim)
    sets = rep.pde_train_sets + rep.bcs_train_sets
    assert sets[0].shape[1] == rg.N_INTERIOR
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = np.linspace(1.0, 2.0, eng.K)
    # the conditioning of the case, on the reference alone
    ref = _check_sets(eng, prob, th, w, sets, False, tag)
    _check_conditioning(prob, th, w, sets, ref, tag)
    rec = _plan(npde, monkeypatch, family, seed, built=(c, rep))
    eng.set_option("precision", "f64")
    for k, s in enumerate(sets):
        eng.set_points_f64(k, s)
    _check_sets(eng, prob, th, w, sets, True, tag)
    rec["f64_affine"], rec["K"] = int(eng.get_option("f64_affine")), eng.K
    if seed % 8 in (0, 3):
        # reinstalled point sets, permuted and shrunk: the source channels and the float64 affine part are evaluated again
        rng = np.random.default_rng([11, seed])
        new = []
        for s in sets:
            n = s.shape[1]
            new.append(np.ascontiguousarray(s[:, rng.permutation(n)[: max(1, n - 1 - n // 4)]]))
        for k, s in enumerate(new):
            eng.set_points_f64(k, s)
        _check_sets(eng, prob, th, w, new, True, tag + ("reinstalled",))
        eng.set_option("precision", "f32")
        for k, s in enumerate(new):
            eng.set_points(k, s)
        _check_sets(eng, prob, th, w, new, False, tag + ("reinstalled",))


@pytest.mark.parametrize("family,batch", BATCHES)
def test_random_residuals_meet_the_oracle(npde, use_emu, monkeypatch, tmp_path, family, batch):
    seeds, per = SEEDS[family]
    monkeypatch.setenv("PINN_JIT_DIR", str(tmp_path / "jit"))
    for seed in seeds[batch * per: (batch + 1) * per]:
        _check_case(npde, monkeypatch, family, seed)
    # the generator stays inside the ahead-of-time kernel table: a case that specialises a kernel at run time is a generator error
    assert not os.path.exists(tmp_path / "jit"), sorted(p.name for p in (tmp_path / "jit").rglob("*"))


def test_generator_reaches_the_rewrites(npde, use_emu, monkeypatch, tmp_path):
    """coverage conditions over the whole seed list, from describe(), get_option("f64_affine") and the generator's record — so that the
    generator cannot drift away from the rewrites unnoticed — and the share of rejected draws"""
    monkeypatch.setenv("PINN_JIT_DIR", str(tmp_path / "jit"))
    recs = [_plan(npde, monkeypatch, f, s) for f, (seeds, _) in SEEDS.items() for s in seeds]
    count = lambda pred: sum(1 for r in recs if pred(r))
    one_net = lambda r: r["nnet"] == 1 and r["family"] != "long"
    got = {
        "fused Laplacian channel": count(lambda r: one_net(r) and r["lap"]),
        "no fused Laplacian channel": count(lambda r: one_net(r) and not r["lap"]),
        "fp32 affine shortcut": count(lambda r: r["affine32"] > 0),
        "fp32 tape": count(lambda r: r["tape32"] > 0),
        "hoisted sources": count(lambda r: r["hoisted"] > 0),
        "riding boundary terms": count(lambda r: r["riding"]),
        "float64 affine terms": sum(r["f64_affine"] for r in recs),
        "float64 interpreter terms": sum(r["K"] - r["f64_affine"] for r in recs),
        "two-launch path of one network": count(lambda r: r["two_launch"]),
        "fixed parameters read": count(lambda r: bool(r["fixed_params_read"])),
        "every Laplacian block": min(count(lambda r, p=p: p in r["blocks"]) for p in range(rg.N_BLOCKS)),
    }
    at_least_10 = {"fused tail launch": count(lambda r: r["tail"]), "estimated parameters": count(lambda r: r["estimated"])}
    print("RR coverage", _backend(npde), got, at_least_10)
    assert all(v >= 15 for v in got.values()) and all(v >= 10 for v in at_least_10.values()), (got, at_least_10)
    symbolic = count(lambda r: r["symbolic"])
    assert 0.4 * len(recs) <= symbolic <= 0.6 * len(recs)
    for f, (seeds, _) in SEEDS.items():
        assert len(REJECTED.get((_backend(npde), f), ())) <= 0.05 * len(seeds), (f, REJECTED)
    assert not os.path.exists(tmp_path / "jit")
