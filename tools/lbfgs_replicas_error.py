"""Replica-resident L-BFGS: max-norm relative error over (every iterate's displacement x_k - x_0, loss history, final
gradient) of the existing resident lane (pinn_lbfgs_init / _steps, fp32) and of the replica kernel (pinn_lbfgs_replicas_*) against the numpy-double
reference of tests/test_lbfgs_replicas.py, on that file's cases — its problems, start points and reference are imported.  The pinn_lbfgs_steps
lane's worst figure per problem fixes the tests' bar (DEVICE_LANE_ERR); section 1 of profiles/lbfgs_replicas.txt is this tool's output on an MI355X.
  python tools/lbfgs_replicas_error.py [emu] [--out FILE]      # emu: the g++ emulation library instead of the product library"""
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
import test_lbfgs_replicas as t
import test_resident_lbfgs as rl

out = []
worst = {}
for case in "ab":
    eng = t.problem(npde, case)[0].engine
    for history, maxiters in t.CASES:
        def single(th0):                                 # the loop users have today: one resident training after the other
            return [rl.device_run(eng, x0, t.TERM_W[case], history, maxiters) for x0 in th0]
        e_dev = t.errors(npde, eng, case, t.NREP, history, maxiters, single)
        e_rep = t.errors(npde, eng, case, t.NREP, history, maxiters, t.replica_lane(eng, case, history, maxiters))
        worst[case] = tuple(max(p, q) for p, q in zip(worst.get(case, (0.0, 0.0)), (e_dev, e_rep)))
        out.append(f"case {case} history={history} maxiters={maxiters} ({t.NREP} replicas): pinn_lbfgs_steps {e_dev:.3e}  replica kernel {e_rep:.3e}")
        print(out[-1], flush=True)
for case, (e_dev, e_rep) in worst.items():
    out.append(f"worst of case {case}: pinn_lbfgs_steps {e_dev:.3e}  replica kernel {e_rep:.3e}")
    print(out[-1])
if "--out" in sys.argv:
    open(sys.argv[sys.argv.index("--out") + 1], "w").write("\n".join(out) + "\n")
