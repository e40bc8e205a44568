"""History independence of a handle (tests/handle_history.py): after any generated sequence of state changes, evaluations at other parameters,
complete optimiser / sampler runs, option and point-set detours, a reused handle computes, BIT FOR BIT, what a fresh handle brought straight to
the same state computes — loss and gradient, the loss-only evaluation, per-term gradients, every term's residuals, phi and a second derivative on
a 33-point probe set, the installed sets, and the float64 twins of all of these where the sequence ends in float64 mode.  Derived, not measured:
same kernels, same launch geometry, fixed-order reductions; a difference is a stale buffer, a missing invalidation or a counter that was not
restored.  No observable is exempt.  Resumable states (resident Adam, resident L-BFGS, resident HMC) continued after operations in between are
k1 + k2 steps of a fresh handle bit for bit, or the refusal the header names (the contract table is in tests/handle_history.py).  At the final
checkpoint the reused handle also meets the float64 oracle in exact mode at the bars of tests/test_random_residuals.py (fp32: 1e-5 with its
LOSS_FLOOR, residuals 2e-5; float64: 1e-11 / 1e-12), on seeds whose reference alone moves by less than its Q_MAX under float32 inputs.
Each sequence prints its figures before it asserts (`pytest -s`).  (CPU: the g++ emulation; tests/test_gpu_mirror.py re-runs this module on
the hardware, where the asynchronous hazards — a free under an evaluation in flight, the shared pinned staging block, the aux-stream fork / join,
the persistent kernel's backup — can show.)"""
import numpy as np
import pytest

import handle_history as hh
from test_f64_mode import EXACT
from test_launch_geometry import FP32, _at_oracle
from test_random_residuals import LOSS_FLOOR, Q_MAX, _backend, _measures, _pointwise

# committed seeds per problem and seeds per test (the emulation takes about 0.5 s per sequence of a 16-wide problem and 5 s of a 64-wide one)
SEEDS = {name: ((list(range(6)), 1) if name in ("poisson64", "system64") else (list(range(12)), 4)) for name in hh.PROBLEMS}
assert all(len(seeds) % per == 0 for seeds, per in SEEDS.values())
BATCHES = [(p, b) for p, (seeds, per) in SEEDS.items() for b in range(len(seeds) // per)]

# what get_option reports over a problem's sequences: every value the problem can reach.  f64_path names what the LAST float64 launch sequence
# ran, whatever the entry point: "lanes" / "mfma+lanes" appear where a stencil evaluation or a value-only phi / derivative launch of a shape without
# a tile kernel came last before the option was read, which depends on the order of operations, not on the problem — so "mfma" is required of every
# float64-capable problem and the other two are allowed, not required
PATHS = {
    "eval_path": lambda P: {"one launch", "stand-alone kernels"} if P.name in ("poisson16", "inverse", "heat") else {"stand-alone kernels"},
    "adam_path": lambda P: {"persistent", "loop"} if P.name in ("poisson16", "heat") else {"loop"},
    "f64_path": lambda P: {"mfma"} if P.f64_ok else set(),          # (+ "lanes" / "mfma+lanes" where a stencil or value-only launch ran last: allowed, not required)
}

_RECORDS = {}                   # (backend, problem, seed) -> Record


def _record(npde, name, seed):
    key = (_backend(npde), name, seed)
    if key not in _RECORDS:
        _RECORDS[key] = hh.run(npde, name, seed)
    return _RECORDS[key]


def _check_sequence(npde, name, seed):
    r = _record(npde, name, seed)
    tag = (_backend(npde), name, seed)
    P = hh.problem(npde, name)
    print("HH", *tag, "ops", [o["kind"] + ("(refused)" if o["refused"] else "") for o in r.ops])
    # 1. every refusal is the named one
    for o in r.ops:
        if o["refused"]:
            assert o["refused"]["want"] in o["refused"]["got"], (tag, o)
    # 2. reused against fresh, bit for bit, at both checkpoints
    for c in r.checkpoints:
        assert set(c["reused"]) == set(c["fresh"])
        diff = {k: float(np.max(np.abs(np.asarray(c["reused"][k], dtype=np.float64) - np.asarray(c["fresh"][k], dtype=np.float64))))
                for k in c["reused"] if not np.array_equal(c["reused"][k], c["fresh"][k])}
        assert not diff, (tag, "checkpoint after operation %d" % c["at"], [o["kind"] for o in r.ops[:c["at"]]], diff)
    # 3. resumable states
    for x in r.resumed:
        for i, (a, b) in enumerate(zip(x["got"], x["want"])):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (tag, "resume_" + x["kind"], i, [o["kind"] for o in r.ops[:x["at"]]])
    # 4. the oracle at the final checkpoint
    S, obs = r.final["state"], r.final["obs"]
    f64 = S["prec"] == "f64"
    w = np.linspace(1.0, 2.0, P.K)
    ref, refs = hh.oracle(P, S, P.theta, w)
    if not f64:
        # the conditioning of the final state, on the reference alone
        f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
        S32 = dict(S, terms=[dict(t, pts=f32(t["pts"])) for t in S["terms"]])
        lo, _ = hh.oracle(P, S32, f32(P.theta), w)
        q = max(_measures(lo.term_losses, lo.grad, ref, LOSS_FLOOR))
        print("HH", *tag, "q", "%.3e" % q)
        assert q < Q_MAX, (tag, q)
    l, g = (obs["loss64"], obs["grad64"]) if f64 else (obs["loss"], obs["grad"])
    res = [obs[("res64_%d" if f64 else "res%d") % k] for k in range(P.K)]
    floor = 0.0 if f64 else LOSS_FLOOR
    fig = _measures(l, g, ref, floor) + (max(_pointwise(a, b) for a, b in zip(res, refs)),)
    print("HH", *tag, "f64" if f64 else "fp32", *("%.3e" % v for v in fig))
    _at_oracle(l, g, ref, bar=EXACT if f64 else FP32, loss_floor=floor)
    for k, (a, b) in enumerate(zip(res, refs)):
        assert a.shape == b.shape and np.max(np.abs(a - b)) < (1e-12 if f64 else 2e-5) * max(1.0, np.max(np.abs(b))), (tag, k)


@pytest.mark.parametrize("problem,batch", BATCHES)
def test_reused_handle_equals_fresh_handle(npde, use_emu, problem, batch):
    seeds, per = SEEDS[problem]
    for seed in seeds[batch * per: (batch + 1) * per]:
        _check_sequence(npde, problem, seed)


def _crossed(sizes, edge):
    up = any(a <= edge < b for a, b in zip(sizes, sizes[1:]))
    down = any(b <= edge < a for a, b in zip(sizes, sizes[1:]))
    return up and down


def _grew_after_shrinking(sizes):
    """a shrink, then a set larger than anything the buffer has held (grow-only capacity = the running maximum)"""
    cap, shrunk = 0, False
    for a, b in zip([0] + sizes, sizes):
        if shrunk and b > cap:
            return True
        shrunk = shrunk or b < a
        cap = max(cap, b)
    return False


def test_generator_reaches_the_state(npde, use_emu):
    """coverage conditions over the committed seeds, so that the generator cannot drift away from the state it is there to exercise"""
    total = refused = 0
    for family, names in hh.FAMILIES.items():
        ran, kinds = {}, set(hh.STATE_KINDS + hh.TRACELESS_KINDS + hh.RESUMABLE_KINDS)
        for name in names:
            P = hh.problem(npde, name)
            recs = [_record(npde, name, s) for s in SEEDS[name][0]]
            for r in recs:
                for o in r.ops:
                    total += 1
                    refused += bool(o["refused"])
                    if not o["refused"]:
                        ran[o["kind"]] = ran.get(o["kind"], 0) + 1
            seqs = [s for r in recs for s in r.sizes]               # the sizes every term of every sequence went through
            assert any(_grew_after_shrinking(s) for s in seqs), name
            assert any(1 in s[1:] for s in seqs), name
            assert any(_crossed(s, 64) for s in seqs) and any(_crossed(s, 256) for s in seqs), name
            for opt, reach in PATHS.items():
                seen = set().union(*[r.paths[opt] for r in recs]) - {"none", "off"}
                print("HH paths", _backend(npde), name, opt, sorted(seen))
                if opt == "f64_path":
                    seen -= {"lanes", "mfma+lanes"}
                assert seen == reach(P), (name, opt, seen)
        if not any(any(hh.problem(npde, name).ndata) for name in names):
            kinds.discard("data")
        few = {k: ran.get(k, 0) for k in kinds if ran.get(k, 0) < 3}
        print("HH coverage", _backend(npde), family, ran)
        assert not few, (family, few)
    print("HH refusals", refused, "of", total)
    assert refused <= 0.25 * total
