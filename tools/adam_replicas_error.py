"""Replica-resident Adam: max-norm relative error over (displacement theta_k - theta_0, loss history) of the existing
resident lane (pinn_adam_steps) and of the replica kernel (pinn_adam_replicas_*) against the numpy-double reference of tests/test_adam_replicas.py,
on that file's cases — its problems, seeds and reference are imported, as tools/hmc_chains_error.py imports its test's.  The pinn_adam_steps
lane's worst figure per problem fixes the tests' bar (DEVICE_LANE_ERR); section 1 of profiles/adam_replicas.txt is this tool's output on an MI355X.
  python tools/adam_replicas_error.py [emu] [--out FILE]      # emu: the g++ emulation library instead of the product library"""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pinn_import
npde = pinn_import.load()
if "emu" in sys.argv[1:]:
    npde._lib.set_library(npde.Library(os.path.join(ROOT, "tests", "emu", "libpinn_emu.so")))
import test_adam_replicas as t

out = []
worst = {}
for case in "ab":
    rep, _, _, th0 = t.problem(npde, case)
    eng = rep.engine
    ref = t.shared_reference(npde, case)
    for n in (1, t.NSTEPS):
        th, _, _, hist = t.run(eng, th0, t.LRS, case, (n,))
        for r in range(t.NREP):
            th1, h1 = eng.adam(th0[r], n, t.LRS[r], t.TERM_W[case], t.B1, t.B2, t.EPS)
            disp, href = ref[r][0][n] - ref[r][0][0], ref[r][1][:n]
            e_dev = max(t.hc.relerr(th1.astype(np.float64) - th0[r], disp), t.hc.relerr(h1, href))
            e_rep = max(t.hc.relerr(th[r].astype(np.float64) - th0[r], disp), t.hc.relerr(hist[r], href))
            worst[case] = tuple(max(p, q) for p, q in zip(worst.get(case, (0.0, 0.0)), (e_dev, e_rep)))
            out.append(f"case {case} nsteps={n} replica {r} lr={t.LRS[r]:.0e}: pinn_adam_steps {e_dev:.3e} (path {eng.get_option('adam_path')})  replica kernel {e_rep:.3e}  "
                       f"equal bits: {np.array_equal(th1, th[r]) and np.array_equal(h1, hist[r])}")
            print(out[-1], flush=True)
for case, (e_dev, e_rep) in worst.items():
    out.append(f"worst of case {case}: pinn_adam_steps {e_dev:.3e}  replica kernel {e_rep:.3e}")
    print(out[-1])
if "--out" in sys.argv:
    open(sys.argv[sys.argv.index("--out") + 1], "w").write("\n".join(out) + "\n")
