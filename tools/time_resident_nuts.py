"""BPINN NUTS, microseconds per leapfrog step: the resident transitions (pinn_nuts_draws) at nuts_chunk = 1, 8 and 64,
against the host loop around `bpinn._nuts_transition` on the same handle (one `loglik_grad_f64` round trip per leapfrog step) and against the
resident fixed-length HMC step (pinn_hmc_draws).  The two problems of section 4.7 (test_resident_hmc.forward_problem / inverse_problem) in both
precisions; medians of --reps calls after one warm-up call each; every call starts from the same chain state and the same counter, so all
NUTS variants build the same trees (the leapfrog count of a call is the sum of its n_leapfrog).
  python tools/time_resident_nuts.py [--reps 21] [--draws 4] [--depth 5] [--out profiles/resident_nuts_timing.txt]
  python tools/time_resident_nuts.py --kernels     # one short resident run per problem and nothing else: the workload to put under a kernel
                                                   # trace (rocprofv3 --kernel-trace --stats -- python ...) for k_nuts_step's own time beside
                                                   # the evaluation's kernels"""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import pinn_import
npde = pinn_import.load()
from neuralpde_jl_amd import bpinn
import test_resident_hmc as th

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--draws", type=int, default=4)
ap.add_argument("--depth", type=int, default=5)
ap.add_argument("--eps", type=float, default=1.0e-2)
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
SEED = 11
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_us(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts))


say(f"# us per leapfrog step, medians of {args.reps} calls of {args.draws} draws, max_depth {args.depth}, eps {args.eps}")
for which in ("forward", "inverse"):
    for prec in th.PRECISIONS:
        rep, th0, stds, nn, priors = th.forward_problem(npde, prec) if which == "forward" else th.inverse_problem(npde, prec, "lognormal")
        eng = rep.engine
        kinds = th.kinds_of(priors)
        init = lambda: eng.hmc_init(th0, stds, th.NN_PRIOR, kinds)
        init()
        leaps = int(eng.nuts_draws(args.draws, args.depth, args.eps, SEED)[4].sum())
        if args.kernels:
            init()
            eng.nuts_draws(args.draws, args.depth, args.eps, SEED)
            eng.hmc_draws(args.draws, max(leaps // args.draws, 1), args.eps, SEED)
            say(f"{which} {prec}: P={eng.P} one resident NUTS call of {leaps} leapfrog steps and one HMC call of {args.draws * max(leaps // args.draws, 1)}")
            continue
        line = f"{which:8s} {prec} P={eng.P} leapfrog steps per call {leaps:4d}"
        for chunk in (1, 8, 64):
            eng.set_option("nuts_chunk", str(chunk))

            def run():
                init()
                t0 = time.perf_counter()
                eng.nuts_draws(args.draws, args.depth, args.eps, SEED)
                run.t.append(time.perf_counter() - t0)
            run.t = []
            for _ in range(args.reps + 1):
                run()
            line += f" | nuts chunk {chunk:2d}: {1e6 * float(np.median(run.t[1:])) / leaps:8.1f}"
        eng.set_option("nuts_chunk", "8")
        # the host loop: the specification around the same handle's evaluations, randomness from the restated generator
        logp_grad, _ = th.make_logp(eng, stds, nn, priors)
        minv = np.ones(eng.P)
        rng = np.random.default_rng(SEED)
        zs, us = rng.standard_normal((args.draws, eng.P)), rng.random((args.draws, bpinn.nuts_uniforms(args.depth)))
        st0 = (th0,) + tuple(logp_grad(th0))
        count = [0]

        def host():
            st, n = st0, 0
            for d in range(args.draws):
                st, stats = bpinn._nuts_transition(logp_grad, st, minv, args.eps, zs[d], us[d], args.depth)
                n += stats["n_leapfrog"]
            count[0] = n
        t_host = median_us(host, max(args.reps // 3, 3))
        line += f" | host _nuts: {t_host / count[0]:8.1f} ({count[0]} steps)"
        nl = max(leaps // args.draws, 1)

        def hmc():
            init()
            t0 = time.perf_counter()
            eng.hmc_draws(args.draws, nl, args.eps, SEED)
            hmc.t.append(time.perf_counter() - t0)
        hmc.t = []
        for _ in range(args.reps + 1):
            hmc()
        line += f" | hmc_draws: {1e6 * float(np.median(hmc.t[1:])) / (args.draws * nl):8.1f}"
        say(line)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
