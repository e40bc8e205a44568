"""Replica-resident Adam (pinn_adam_replicas_*), microseconds per Adam step of a launch for nrep = 1, 8, 64, 256 against
the resident single-training loop (pinn_adam_steps) on the same handle, in one process.  The two problems of tests/test_adam_replicas.py (imported,
as tools/time_hmc_chains.py imports its test's): (a) 1-6-1 tanh on 13 points, (b) 2-16-16-1 sigmoid on 110 points with an estimated parameter.
Medians of --reps calls of --steps steps after one warm-up call each.  A call's time includes its uploads and its single download (the loss
history); the replicas' state is not re-initialised between calls.  Section 3 of profiles/adam_replicas.txt is this tool's output.
  python tools/time_adam_replicas.py [--reps 21] [--steps 200] [--out FILE]"""
import argparse, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pinn_import
npde = pinn_import.load()
import test_adam_replicas as t

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--lr", type=float, default=1.0e-3)
ap.add_argument("--out", default="")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_of(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


say(f"# us per Adam step of a launch and replica-steps per second, medians of {args.reps} calls of {args.steps} steps, lr {args.lr}, fp32")
for case, name in (("a", "(a) 1-6-1 tanh, 13 points"), ("b", "(b) 2-16-16-1 sigmoid, 110 points, 1 estimated parameter")):
    rep, _, _, th0 = t.problem(npde, case)
    eng, w = rep.engine, t.TERM_W[case]
    eng.adam(th0[0], 1, args.lr, w)
    tm = median_of(lambda: eng.adam(None, args.steps, args.lr, w, init=False), args.reps)
    say(f"{name}: P={eng.P} | pinn_adam_steps ({eng.get_option('adam_path')}) {1e6 * tm / args.steps:7.2f} us/step")
    for nr in (1, 8, 64, 256):
        eng.adam_replicas_init(np.tile(th0[0], (nr, 1)))
        tm = median_of(lambda: eng.adam_replicas_steps(args.steps, args.lr, w), args.reps)
        say(f"{name}: nrep {nr:3d} | {1e6 * tm / args.steps:7.2f} us/step per launch | {nr * args.steps / tm:12.0f} replica-steps/s")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
