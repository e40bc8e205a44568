"""L-BFGS finisher, microseconds per objective evaluation: the host routine (pinn_lbfgs: one host round trip per line-search trial) against
the device-resident loop (pinn_lbfgs_init / pinn_lbfgs_steps) at lbfgs_chunk = 1 and 8.  Medians of --reps runs of
--iters iterations from the same start, after one warm-up run each.  Evaluations: the resident loop reports its own count (every trial is a
full evaluation); the host routine takes the same decisions, so its count is derived from the resident run's per-iteration counts — 1 initial
+ per iteration (trials, + 1 when a trial was rejected: the accepted point is re-evaluated with its gradient; rejected trials are loss-only).
  python tools/time_resident_lbfgs.py [--only small|cfg2] [--reps 21] [--iters 40]
Also prints, for the float64 Poisson problem, the final theta of the resident run against pinn_lbfgs at equal maxiters."""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import numpy as np
import pinn_import
npde = pinn_import.load()
from neuralpde_jl_amd import workloads
import test_emu_parity as tp

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--iters", type=int, default=40)
args = ap.parse_args()


def problems():
    if args.only in ("", "small"):
        for prec in ("f64", "f32"):
            sysm, chain = tp.poisson2d(npde, "tanh", width=16, hidden=2)
            yield f"poisson2d 2x16 165 pts {prec}", sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=tp.theta_for(chain, 5), precision=prec), prec
    if args.only in ("", "cfg2"):
        wl = workloads.cfg2_poisson2d(points=4096, bcs_points=512)
        yield "cfg2-shaped 4x64 4,096 + 4 x 512 pts f32", wl.pde_system, wl.discretization(), "f32"


def median_us(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts))


for name, sysm, disc, prec in problems():
    rep = npde.symbolic_discretize(sysm, disc)
    eng = rep.engine
    if prec == "f64" and eng.get_option("precision") != "f64":
        eng.set_option("precision", "f64")
    th0 = np.asarray(rep.flat_init_params, dtype=np.float64)
    N = args.iters
    # per-iteration evaluation counts of the resident run
    eng.lbfgs_init(th0, None, history=10)
    per_it = []
    for _ in range(N):
        h, e, st = eng.lbfgs_steps(1)
        if len(h) == 0:
            break
        per_it.append(e)
    n_it = len(per_it)
    host_evals = 1 + sum(e + (e > 1) for e in per_it)
    res_evals = sum(per_it)
    t_host = median_us(lambda: eng.lbfgs(th0, n_it, None, history=10), args.reps)
    line = f"{name:44s} P={eng.P:6d} iterations {n_it:3d}  host: {host_evals:3d} evals {t_host / host_evals:8.1f} us/eval {t_host / n_it:8.1f} us/iter"
    for chunk in (1, 8):
        eng.set_option("lbfgs_chunk", str(chunk))

        def run():
            eng.lbfgs_init(th0, None, history=10)
            t0 = time.perf_counter()
            eng.lbfgs_steps(n_it)
            run.t.append(time.perf_counter() - t0)
        run.t = []
        for _ in range(args.reps + 1):
            run()
        t = 1e6 * float(np.median(run.t[1:]))
        line += f" | chunk {chunk}: {res_evals:3d} evals {t / res_evals:8.1f} us/eval {t / n_it:8.1f} us/iter"
    print(line, flush=True)
    if prec == "f64":
        eng.set_option("lbfgs_chunk", "8")
        eng.lbfgs_init(th0, None, history=10)
        eng.lbfgs_steps(n_it)
        xr = eng.lbfgs_get()[0]
        xh, _ = eng.lbfgs(th0, n_it, None, history=10)
        print(f"    final theta, resident against pinn_lbfgs after {n_it} iterations: max-norm relative difference {np.max(np.abs(xr - xh)) / np.max(np.abs(xh)):.3e}", flush=True)
