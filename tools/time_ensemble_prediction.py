"""BPINN prediction stage, milliseconds per dependent variable: the host loop of `ahmc_bayesian_pinn_pde` (one `phi` call per retained draw,
mean / std in numpy) against one `phi_ensemble` call (pinn_phi_ensemble) on the same samples and points.  Medians
of --reps runs after one warm-up run each, both paths in the same process.  Also prints the largest difference of the two paths' curves.
  python tools/time_ensemble_prediction.py [--only small|mid|big] [--reps 21] [--samples 333] [--once device] [--derivatives]
--once device: one warm-up and one device call per problem, nothing else (the run a kernel trace is taken from).
--derivatives: the same comparison for u_x and u_xx on "mid" and "big": the host loop of one `derivative[_f64]` call per
retained draw and request, mean / std in numpy, against ONE `derivative_ensemble` call (pinn_derivative_ensemble) for both requests."""
import argparse, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import pinn_import
npde = pinn_import.load()

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="")
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--samples", type=int, default=333)
ap.add_argument("--once", default="")
ap.add_argument("--derivatives", action="store_true")
args = ap.parse_args()

PROBLEMS = {            # name -> (layer sizes, points per axis)
    "small": ((1, 6, 1), 101),
    "mid": ((1, 16, 16, 1), 101),
    "big": ((2, 64, 64, 64, 64, 1), 101),
}


def handle(sizes, prec):
    d = sizes[0]
    xs = npde.parameters(" ".join("xy"[:d]))
    (u,) = npde.variables("u")
    sysm = npde.PDESystem([npde.Eq(u(*xs), xs[0])], [npde.Eq(u(*([0.0] * d)), 0.0)], [npde.In(x, npde.Interval(0.0, 1.0)) for x in xs], list(xs), [u(*xs)])
    chain = npde.Chain(*[npde.Dense(sizes[l], sizes[l + 1], "tanh") for l in range(len(sizes) - 2)], npde.Dense(sizes[-2], 1))
    th = npde.initialparameters(np.random.default_rng(1), chain)
    return npde.symbolic_discretize(sysm, npde.PhysicsInformedNN(chain, npde.GridTraining(0.5), init_params=th, precision=prec)), th


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


for name, (sizes, per_axis) in PROBLEMS.items():
    if args.only and args.only != name:
        continue
    for prec in ("f64", "f32"):
        rep, th = handle(sizes, prec)
        rng = np.random.default_rng(2)
        thetas = np.asarray(th, dtype=np.float64)[None, :] * (1.0 + 0.1 * rng.standard_normal((args.samples, rep.engine.P)))
        axes = [np.linspace(0.0, 1.0, per_axis)] * sizes[0]
        pts = np.stack([m.ravel() for m in np.meshgrid(*axes, indexing="ij")])

        def host():
            preds = np.stack([rep.phi(pts, t)[0] for t in thetas])       # (bpinn.py: the ensemble="host" loop)
            return preds.mean(axis=0), preds.std(axis=0)

        def device():
            return rep.engine.phi_ensemble(0, thetas, pts)

        if args.derivatives:
            if name == "small":
                continue
            eng, reqs = rep.engine, [(1, (0,)), (2, (0, 0))]
            der = (lambda t, ax: eng.derivative_f64(0, t, pts, ax)) if prec == "f64" else (lambda t, ax: eng.derivative(0, t, pts, ax).astype(np.float64))

            def host():                                                  # (bpinn.py: the ensemble="host" loop over ensemble_derivatives)
                preds = np.stack([np.stack([der(t, ax) for t in thetas]) for _, ax in reqs])
                return preds.mean(axis=1), preds.std(axis=1)

            def device():
                return eng.derivative_ensemble(0, thetas, pts, reqs)

        if args.once == "device":
            device(); device()
            continue
        (mh, sh), (md, sd) = host(), device()
        diff = max(np.max(np.abs(mh - md)), np.max(np.abs(sh - sd))) / max(1.0, np.max(np.abs(mh)))
        t_host, t_dev = median_ms(host, args.reps), median_ms(device, args.reps)
        what = "derivative_ensemble (u_x, u_xx)" if args.derivatives else "phi_ensemble"
        print(f"{'-'.join(map(str, sizes)):18s} {prec} n={pts.shape[1]:6d} S={args.samples:4d}  host loop {t_host:9.3f} ms  {what} {t_dev:8.3f} ms  "
              f"x{t_host / t_dev:7.1f}  curves differ by {diff:.2e}", flush=True)
