"""Timings of the resident HMC sampler under the dense metric (profiles/resident_hmc_dense.txt): medians of 21 timed calls after 3
warm-up calls, wall clock around the synchronous ABI call, forward Poisson problem of tests/test_resident_hmc.py (13 points, 1-16-16-1, P = 321).
  python tools/hmc_dense_timing.py            # one table on stdout
  python tools/hmc_dense_timing.py --trace    # ONE pinn_hmc_draws(2 draws x 3 steps) under the dense metric, for a kernel trace's launch list"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pinn_import  # noqa: E402
from test_resident_hmc import EPS_STEP, NN_PRIOR, forward_problem  # noqa: E402
from test_hmc_dense_metric import dense_metric  # noqa: E402


def median_us(f, reps=21, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def main():
    npde = pinn_import.load()
    nd, L = 20, 10
    for precision in ("f64", "f32"):
        rep, th0, stds, nn, priors = forward_problem(npde, precision)
        eng = rep.engine
        Minv = dense_metric(eng.P)
        eng.hmc_init(th0, stds, NN_PRIOR, [])
        if "--trace" in sys.argv:
            eng.hmc_set_metric_dense(Minv)
            eng.hmc_draws(2, 3, EPS_STEP, 1)
            continue
        diag = median_us(lambda: eng.hmc_draws(nd, L, EPS_STEP, 1, want_samples=False)) / (nd * L)
        setm = median_us(lambda: eng.hmc_set_metric_dense(Minv))
        dense = median_us(lambda: eng.hmc_draws(nd, L, EPS_STEP, 1, want_samples=False)) / (nd * L)

        def warm(n):
            eng.hmc_init(th0, stds, NN_PRIOR, [])
            eng.hmc_set_metric_dense(None)
            t0 = time.perf_counter()
            eng.hmc_warmup(n, 1, 0.02, 0.8, 1)
            return (time.perf_counter() - t0) * 1e6
        for _ in range(3):
            warm(100)
        with_event = statistics.median(warm(100) for _ in range(21))
        without = statistics.median(warm(99) for _ in range(21))
        print(f"{precision}  P = {eng.P}:  diagonal {diag:.1f} us / leapfrog step   dense {dense:.1f} us / leapfrog step   set_metric_dense {setm:.0f} us   "
              f"warm-up metric update {with_event - without * 100.0 / 99.0:.0f} us (warm-up of 100 x 1 steps: {with_event:.0f} us, of 99: {without:.0f} us)")


if __name__ == "__main__":
    main()
