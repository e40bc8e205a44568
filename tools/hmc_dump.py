"""Every output of a fixed series of resident-sampler calls (pinn_hmc_*, pinn_nuts_draws, pinn_hmc_chains_*) in one .npz, for comparing two trees
byte for byte: a change that promises unchanged arithmetic must reproduce the file.  Public Python API only, so the same script runs against
any tree that has these calls: --root names the tree whose package, library and test helpers are used (default: the tree this file is in).
Problems: tests/test_resident_hmc.py's forward Poisson problem (13 points, 1-16-16-1, P = 321: a second 256-thread block, two elements per
thread in the strided sums, ld = 384 under the dense metric) and its inverse problem under a Normal and a LogNormal parameter prior; float64
and fp32; a non-unit diagonal metric and tests/test_hmc_dense_metric.py's dense_metric(P).
  python tools/hmc_dump.py --out FILE.npz [--root DIR] [--emu]        (--emu: the CPU emulation library of the tree's tests)
  python tools/hmc_dump.py --compare A.npz B.npz                      (exit status 1 unless every array is byte-identical)"""
import argparse, os, sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--emu", action="store_true")
ap.add_argument("--out", default="")
ap.add_argument("--compare", nargs=2, metavar="NPZ")
args = ap.parse_args()

if not args.compare and not args.out:
    ap.error("--out FILE.npz is required unless --compare is given")
if args.compare:
    a, b = (np.load(f) for f in args.compare)
    bad = sorted(set(a.files) ^ set(b.files))
    bad += [k for k in a.files if k in b.files and (a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes())]
    print(f"hmc_dump: {len(a.files)} arrays, {len(bad)} differ" + "".join(f"\n  {k}" for k in bad))
    sys.exit(1 if bad or not a.files else 0)

root = os.path.abspath(args.root)
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import pinn_import
npde = pinn_import.load()
import test_resident_hmc as th
import test_hmc_dense_metric as td
if args.emu:
    npde._lib.set_library(npde.Library(os.path.join(root, "tests", "emu", "libpinn_emu.so")))

out = {}
EPS, SEED = th.EPS_STEP, 11


def put(tag, names, values):
    for n, v in zip(names, values):
        out[f"{tag}/{n}"] = np.asarray(v)


def state(eng, tag):
    put(tag, ("theta", "logp_cur", "grad"), eng.hmc_get())


def series(name, make, precision, dense):
    rep, th0, stds, nn, priors = make(precision)
    eng, tag = rep.engine, f"{name}/{precision}/{'dense' if dense else 'diag'}"
    P, rng = eng.P, np.random.default_rng(23)
    eng.hmc_init(th0, stds, th.NN_PRIOR, th.kinds_of(priors))
    state(eng, tag + "/init")
    if dense:
        eng.hmc_set_metric_dense(td.dense_metric(P))
    else:
        eng.hmc_set_metric(th.metric(P, "random"))
    for L in (1, 3):
        put(f"{tag}/draws_L{L}", ("samples", "accept_prob", "logp"), eng.hmc_draws(3, L, EPS, SEED))
        state(eng, f"{tag}/draws_L{L}")
    put(tag + "/draws_supplied", ("samples", "accept_prob", "logp"), eng.hmc_draws(3, 3, EPS, SEED, rng.standard_normal((3, P)), rng.random(3)))
    state(eng, tag + "/draws_supplied")
    put(tag + "/find_stepsize", ("eps", "ntrials"), eng.hmc_find_stepsize(EPS, SEED))
    state(eng, tag + "/find_stepsize")
    if not dense:
        put(tag + "/nuts", ("samples", "accept_stat", "logp", "tree_depth", "n_leapfrog", "divergent"), eng.nuts_draws(3, 3, EPS, SEED))
        state(eng, tag + "/nuts")
    put(tag + "/warmup", ("samples", "accept_prob", "logp", "step_sizes", "eps_final", "inv_metric"), eng.hmc_warmup(100, 1, EPS, 0.8, SEED))
    state(eng, tag + "/warmup")
    if dense:
        put(tag + "/warmup", ("metric", "factor"), eng.hmc_get_metric_dense())
    print(f"hmc_dump: {tag}", flush=True)


problems = {"forward": lambda p: th.forward_problem(npde, p),
            "normal": lambda p: th.inverse_problem(npde, p, "normal"),
            "lognormal": lambda p: th.inverse_problem(npde, p, "lognormal")}
for name, make in problems.items():
    for precision in th.PRECISIONS:
        for dense in (False, True):
            series(name, make, precision, dense)

# two chains of the forward problem (fp32, tanh), the second from a shifted start; the generator's draws, then supplied ones
rep, th0, stds, nn, priors = th.forward_problem(npde, "f32")
eng, rng = rep.engine, np.random.default_rng(29)
eng.hmc_chains_init(np.stack([th0, th0 + 0.01]), EPS, stds, th.NN_PRIOR, [], 3, th.metric(eng.P, "random"), SEED)
put("chains/init", ("theta", "logp_cur", "grad"), eng.hmc_chains_get())
put("chains/draws", ("samples", "accept_prob", "logp"), eng.hmc_chains_draws(3))
put("chains/draws", ("theta", "logp_cur", "grad"), eng.hmc_chains_get())
put("chains/draws_supplied", ("samples", "accept_prob", "logp"), eng.hmc_chains_draws(3, rng.standard_normal((2, 3, eng.P)), rng.random((2, 3))))
put("chains/draws_supplied", ("theta", "logp_cur", "grad"), eng.hmc_chains_get())

np.savez(args.out, **out)
print(f"hmc_dump: {len(out)} arrays -> {args.out}")
