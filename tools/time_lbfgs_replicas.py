"""Replica-resident L-BFGS (pinn_lbfgs_replicas_*), microseconds per slot (one trial evaluation and its judgement) of a
launch for nrep = 1, 8, 64, 256 against the resident single-training loop (pinn_lbfgs_steps) on the same handle, in one process.  The two problems
of tests/test_lbfgs_replicas.py (imported): (a) 1-6-1 tanh on 13 points, (b) 2-16-16-1 sigmoid on 110 points with an estimated parameter; every
replica starts at the first start point, so all run the same slots.  Medians of --reps _steps calls of --iters iterations at history 10, each from
a fresh _init (not timed), after one warm-up; a call's time includes its uploads and the downloads of the control blocks and the history, and is
divided by the trial evaluations the call made.  Section 2 of profiles/lbfgs_replicas.txt is this tool's output.
  python tools/time_lbfgs_replicas.py [--reps 21] [--iters 40] [--out FILE]"""
import argparse, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pinn_import
npde = pinn_import.load()
import test_lbfgs_replicas as t

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--out", default="")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_of(init, steps, reps):
    """median seconds of steps() after init(), and the evaluations steps() reports"""
    ts = []
    for i in range(reps + 1):
        init()
        t0 = time.perf_counter()
        ev = steps()
        if i:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), int(ev)


say(f"# us per slot, medians of {args.reps} _steps calls of {args.iters} iterations, history 10, fp32")
for case, name in (("a", "(a) 1-6-1 tanh, 13 points"), ("b", "(b) 2-16-16-1 sigmoid, 110 points, 1 estimated parameter")):
    rep, _, _, th0 = t.problem(npde, case)
    eng, w = rep.engine, t.TERM_W[case]
    tm, ev = median_of(lambda: eng.lbfgs_init(th0[0], w, history=10), lambda: eng.lbfgs_steps(args.iters)[1], args.reps)
    say(f"{name}: P={eng.P} | pinn_lbfgs_steps (lbfgs_chunk {eng.get_option('lbfgs_chunk')}) {1e6 * tm / ev:7.2f} us/slot ({ev} evaluations)")
    for nr in (1, 8, 64, 256):
        rows = np.tile(th0[0], (nr, 1))
        tm, ev = median_of(lambda: eng.lbfgs_replicas_init(rows, w, history=10), lambda: eng.lbfgs_replicas_steps(args.iters)[2].max(), args.reps)
        say(f"{name}: nrep {nr:3d} | {1e6 * tm / ev:7.2f} us/slot per launch ({ev} evaluations per replica) | {nr * ev / tm:12.0f} replica-slots/s")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
