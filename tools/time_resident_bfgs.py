"""BFGS finisher, microseconds per iteration: the host path (`solve(prob, BFGS())`: scipy.optimize.minimize over the handle's fused evaluation,
one host round trip per objective call and a dense P x P update in numpy per iteration) against the device-resident loop (pinn_bfgs_init /
pinn_bfgs_steps) at lbfgs_chunk = 1 and 8.  One warm-up call each, then the median of --reps runs of --iters iterations
from the same start (the P = 12,737 problem: --iters-large iterations; its host path is timed --reps-large times, scipy's update is two dense
P x P x P products per iteration).
  python tools/time_resident_bfgs.py [--only small|cfg2] [--reps 11] [--iters 40] [--no-host] [--out profiles/resident_bfgs.txt]
  python tools/time_resident_bfgs.py --profile-run            # only the resident loop at P = 12,737: the command to put under
                                                              #   rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/time_resident_bfgs.py --profile-run
  python tools/time_resident_bfgs.py --kernel-db DIR          # k_bfgs_matvec / k_bfgs_update times of that run and the bytes they move per second
Lines are printed and, with --out, appended to that file."""
import argparse, glob, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--iters-large", type=int, default=10)
ap.add_argument("--reps-large", type=int, default=1)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--profile-run", action="store_true")
ap.add_argument("--kernel-db", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()

COPY_TBS = 6.29          # measured device-to-device copy rate of an MI355X, TB/s (read + written bytes)


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if args.kernel_db:
    import sqlite3
    dbs = sorted(glob.glob(os.path.join(args.kernel_db, "**", "*_results.db"), recursive=True))
    assert dbs, "no results database under " + args.kernel_db
    c = sqlite3.connect(dbs[0])
    P, ld = 12737, 12800
    emit(f"kernel times at P = {P} (leading dimension {ld}), rocprofv3 --kernel-trace --stats, no counters in that run; a launch that found nothing to do"
         " (rejected trial, terminal state, H = gamma I) is counted apart: shorter than 50 us")
    for kern, nbytes, what in (("k_bfgs_matvec", 8 * P * ld, "8 P ld read"), ("k_bfgs_update", 16 * P * ld, "16 P ld read + written")):
        d = [r[0] for r in c.execute("select duration from kernels where name like ? order by start", ("%" + kern + "%",))]
        work = sorted(q for q in d if q >= 50e3)
        idle = sorted(q for q in d if q < 50e3)
        if not work:
            emit(f"  {kern}: {len(d)} launches, none did a pass over H")
            continue
        med = work[len(work) // 2]
        tbs = nbytes / med / 1e3
        emit(f"  {kern}: {len(work)} passes over H, median {med / 1e3:8.1f} us (min {work[0] / 1e3:.1f}, max {work[-1] / 1e3:.1f}); {nbytes / 1e9:.3f} GB ({what})"
             f" -> {tbs:.2f} TB/s = {100.0 * tbs / COPY_TBS:.0f} % of the {COPY_TBS} TB/s copy rate; {len(idle)} early exits, median"
             f" {(idle[len(idle) // 2] / 1e3 if idle else 0.0):.1f} us")
    for kern in ("k_bfgs_ctl",):
        d = sorted(r[0] for r in c.execute("select duration from kernels where name like ?", ("%" + kern + "%",)))
        if d:
            emit(f"  {kern}: {len(d)} launches, median {d[len(d) // 2] / 1e3:.1f} us, max {d[-1] / 1e3:.1f} us")
    sys.exit(0)

import pinn_import
npde = pinn_import.load()
from neuralpde_jl_amd import workloads
import test_emu_parity as tp


def problems():
    if args.only in ("", "small") and not args.profile_run:
        for prec in ("f64", "f32"):
            sysm, chain = tp.poisson2d(npde, "tanh", width=16, hidden=2)
            yield f"poisson2d 2x16 165 pts {prec}", sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.1), init_params=tp.theta_for(chain, 5), precision=prec), prec, args.iters, args.reps
    if args.only in ("", "cfg2") or args.profile_run:
        wl = workloads.cfg2_poisson2d(points=4096, bcs_points=512)
        yield "cfg2-shaped 4x64 4,096 + 4 x 512 pts f32", wl.pde_system, wl.discretization(), "f32", args.iters_large, args.reps_large


for name, sysm, disc, prec, N, host_reps in problems():
    prob = npde.discretize(sysm, disc)
    rep = prob.pinnrep
    eng = rep.engine
    if prec == "f64" and eng.get_option("precision") != "f64":
        eng.set_option("precision", "f64")
    th0 = np.asarray(prob.u0, dtype=np.float64)
    w = rep._weights_now()
    if args.profile_run:
        eng.bfgs_init(th0, w)
        hist, evals, status = eng.bfgs_steps(N)
        emit(f"profile run: {name} P={eng.P} iterations {len(hist)} evaluations {evals} status {status} objective {hist[-1]:.6e}")
        continue
    line = f"{name:42s} P={eng.P:6d}"
    if not args.no_host:
        # the warm-up call counts scipy's iterations through a callback (which costs one more evaluation each); the timed calls have none
        seen = []

        def count(state, loss):
            seen.append(state["iter"])
            if eng.P > 4096:
                print(f"    (host warm-up: iteration {state['iter']})", flush=True)
            return False
        npde.solve(prob, npde.BFGS(), maxiters=N, callback=count)
        n_host = max(len(seen), 1)
        print(f"    ({name}: host warm-up done, {n_host} iterations)", flush=True)
        ts = []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            npde.solve(prob, npde.BFGS(), maxiters=N)
            ts.append(time.perf_counter() - t0)
            print(f"    (host run: {ts[-1]:.3f} s)", flush=True)
        t_host = 1e6 * float(np.median(ts))
        line += f"  host (scipy): {n_host:3d} iterations {t_host / n_host:12.1f} us/iter"
    for chunk in (1, 8):
        eng.set_option("lbfgs_chunk", str(chunk))
        out = {}

        def run():
            eng.bfgs_init(th0, w)
            t0 = time.perf_counter()
            out["r"] = eng.bfgs_steps(N)
            run.t.append(time.perf_counter() - t0)
        run.t = []
        reps = args.reps if N == args.iters else max(args.reps_large, 5)
        for _ in range(reps + 1):
            run()
        t = 1e6 * float(np.median(run.t[1:]))
        hist, evals, status = out["r"]
        n_it = max(len(hist), 1)
        line += f" | resident chunk {chunk}: {n_it:3d} iterations {evals:3d} evals {t / n_it:10.1f} us/iter ({status})"
    emit(line)
