"""Chain-resident HMC (pinn_hmc_chains_*), microseconds per leapfrog step for nchains = 1, 8, 64, 256 against the
resident single-chain sampler (pinn_hmc_draws, fp32) on the same handle, in one process.  The two problems of section 4.7: the forward Poisson
problem (13 points, 1-16-16-1) and the reference's 1-D BPINN set-up (GridTraining(0.01), 1-6-1); 30 leapfrog steps per draw; medians of --reps
calls of --draws draws after one warm-up call each.  A call's time includes its upload and its single download.
The forward problem's set-up is tests/test_resident_hmc.py's, imported as tools/time_resident_nuts.py imports it.  Section 2 of
profiles/hmc_chains.txt is this tool's output.
  python tools/time_hmc_chains.py [--reps 21] [--draws 8] [--out FILE]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import sympy as sp
import pinn_import
npde = pinn_import.load()
import test_resident_hmc as th

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--draws", type=int, default=8)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--eps", type=float, default=1.0e-3)
ap.add_argument("--out", default="")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bpinn_1d():
    (x,) = npde.parameters("x")
    (u,) = npde.variables("u")
    eq = npde.Eq(npde.Differential(x)(u(x)) - sp.cos(2 * sp.pi * x), 0)
    sysm = npde.PDESystem([eq], [npde.Eq(u(0.0), 0.0)], [npde.In(x, npde.Interval(0.0, 2.0))], [x], [u(x)])
    chain = npde.Chain(npde.Dense(1, 6, "tanh"), npde.Dense(6, 1))
    rep = npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.01), init_params=npde.initialparameters(np.random.default_rng(7), chain), precision="f32"))
    return rep, np.asarray(rep.flat_init_params, dtype=np.float64), np.array([0.05, 0.01])


def median_of(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


say(f"# us per leapfrog step and chain-steps per second, medians of {args.reps} calls of {args.draws} draws x {args.steps} steps, eps {args.eps}, fp32")
for name in ("forward Poisson 13 points 1-16-16-1", "1-D BPINN GridTraining(0.01) 1-6-1"):
    if name.startswith("forward"):
        rep, th0, stds, _, _ = th.forward_problem(npde, "f32")
    else:
        rep, th0, stds = bpinn_1d()
    eng = rep.engine
    steps = args.draws * args.steps
    eng.hmc_init(th0, stds, th.NN_PRIOR, [])
    t = median_of(lambda: eng.hmc_draws(args.draws, args.steps, args.eps, 11), args.reps)
    say(f"{name}: P={eng.P} | pinn_hmc_draws {1e6 * t / steps:7.2f} us/step")
    for nc in (1, 8, 64, 256):
        eng.hmc_chains_init(np.tile(th0, (nc, 1)), args.eps, stds, th.NN_PRIOR, [], args.steps, None, 11)
        t = median_of(lambda: eng.hmc_chains_draws(args.draws), args.reps)
        say(f"{name}: nchains {nc:3d} | {1e6 * t / steps:7.2f} us/step per launch | {nc * steps / t:12.0f} chain-steps/s")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
