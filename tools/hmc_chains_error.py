"""Chain-resident HMC: max-norm relative error over (samples, logp, accept_prob) of the existing fp32 sampler="device" lane
(pinn_hmc_draws) and of the chain kernel (pinn_hmc_chains_*) against the numpy-double reference of tests/test_hmc_chains.py, on that file's
cases — its problems, inputs and reference are imported, as tools/time_resident_nuts.py imports its test's.  The device lane's worst figure per
problem fixes the tests' bar (DEVICE_LANE_ERR); section 1 of profiles/hmc_chains.txt is this tool's output on an MI355X.
  python tools/hmc_chains_error.py [emu] [--out FILE]      # emu: the g++ emulation library instead of the product library"""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pinn_import
npde = pinn_import.load()
if "emu" in sys.argv[1:]:
    npde._lib.set_library(npde.Library(os.path.join(ROOT, "tests", "emu", "libpinn_emu.so")))
import test_hmc_chains as t

out = []
worst = {}
for case in "ab":
    for L in (1, 5):
        rep, _, _, th0, stds, nn, priors = t.problem(npde, case)
        eng = rep.engine
        minv, mom, uni = t.inputs(eng.P, case, L)
        ref = t.shared_reference(npde, case, L)
        smp, acc, lp = t.run(eng, th0, stds, priors, minv, mom, uni, L)
        for c in range(t.NCH):
            eng.hmc_init(th0[c], stds, t.NN_PRIOR, t.kinds_of(priors))
            eng.hmc_set_metric(minv)
            s1, a1, l1 = eng.hmc_draws(t.NDRAWS, L, t.EPS[L], 0, mom[c], uni[c])
            e_dev = max(t.relerr(s1, ref[c][0]), t.relerr(l1, ref[c][1]), t.relerr(a1, ref[c][2]))
            e_ch = max(t.relerr(smp[c], ref[c][0]), t.relerr(lp[c], ref[c][1]), t.relerr(acc[c], ref[c][2]))
            worst[case] = tuple(max(p, q) for p, q in zip(worst.get(case, (0.0, 0.0)), (e_dev, e_ch)))
            out.append(f"case {case} L={L} chain {c}: device lane {e_dev:.3e}  chain kernel {e_ch:.3e}  a = {np.round(ref[c][2], 4).tolist()}  equal bits: {np.array_equal(s1, smp[c])}")
            print(out[-1], flush=True)
for case, (e_dev, e_ch) in worst.items():
    out.append(f"worst of case {case}: device lane {e_dev:.3e}  chain kernel {e_ch:.3e}")
    print(out[-1])
if "--out" in sys.argv:
    open(sys.argv[sys.argv.index("--out") + 1], "w").write("\n".join(out) + "\n")
