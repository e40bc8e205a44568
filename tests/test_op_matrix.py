"""Every op of the residual tape (csrc/rprog.hpp: apply, adjoint, apply_bilinear, powi), value and adjoint, in every interpreter that
instantiates it, against the float64 oracle in exact mode.  tests/op_matrix.py holds the op cases and the interpreter sites; per (case, site)
the checks are those of tests/test_random_residuals.py (`_check_sets`, `_check_conditioning`): losses and gradient at the project's fp32 bar
(1e-5, loss floor 0.1) or float64 bar (1e-11), every term's pointwise residual (2e-5 / 1e-12), a bit-equal repeat, and the reference's own
sensitivity to float32 inputs q < Q_MAX.  The conditions on a case (bases and denominators > 0.5, branch deciders of MAX / MIN / ABS away from
zero by 1e-4 with each branch on >= 5 of the 37 interior points) are asserted on the reference alone.  Each case prints its figures before it
asserts (`pytest -s`); profiles/op_matrix.txt holds them for both backends.

Sites (op_matrix.SITES) and what puts the tape there:
    f1       2 x 16 tanh                       family-1 LDS tape (pinn_kernels.hpp); every case through BOTH front ends here; k_src cases
    f2       4 x 64 tanh                       family-2 register tape (pinn_kernels2.hpp)
    sys16    two 2 x 16 networks, V in the op  forward / k_expr / reverse launches (aux_kernels.hpp)
    sys64    two 2 x 64 networks               the fused tail launch
    long     2 x 16, > 32 tape rows            the two-launch path of one network (k_expr)
    dgm      DGM(2, 1, 8, 1)                   family 3, one lane per point (pinn_kernels3.hpp).  DGM kernels have no ahead-of-time table:
                                               this site alone specialises its kernel at run time (once per machine, as tests/test_dgm.py)
    int      2 x 16, u_y + u + int_0^1 1.5 expr ds   the integrand of an integral term (aux_kernels.hpp: k_int_expr), 4 Gauss-Legendre nodes; the
                                               oracle has no integral node, so the reference sums the oracle's integrand over the same nodes
    f64_4m   2 x 16, float64                   float64 tiles (pinn_kernels5.hpp); the same handle under PINN_F64_NO_MFMA: the lanes kernels
                                               (pinn_kernels4.hpp); five cases with derivative = stencil against the stencil oracle
    f64_4s   2 x 65, float64                   float64 sliced tiles (pinn_kernels6.hpp): 65 is the narrowest 2-D width family 4m does not cover
Away from f1 the front end alternates with site + case index.  The tape-form op codes come from symbolic.lower_equation; the library has no
entry point that returns the tape sexpr.cpp lowered, so for that front end the table reads the heads of the s-expression it was given.

Cells of the op x site table that cannot be reached, and why:
    POWI exponents 0 and 1                     sympy folds x**0 and x**1 before either front end sees them: no front end emits them
    "src" cases away from f1 / f64_4m          a coordinate-only argument is hoisted into a source channel and evaluated once per point set by
                                               k_src (sample_rules.hpp) or the float64 source pass, whatever kernel runs the tape: one fp32 and
                                               one float64 site cover it
    float64 at sys16 / sys64 / long / dgm / int   the float64 mode has no coupled launches (one lane or tile kernel takes all networks of a
                                               term), refuses DGM networks and has no integral terms: its interpreters are the three f64 sites
    stencil at all but five cases              derivative = stencil changes how the slots are filled, not the tape: op_matrix.STENCIL
(CPU: the g++ emulation; tests/test_gpu_mirror.py re-runs this module on the hardware.)"""
import os
import re

import numpy as np
import pytest
import sympy as sp

import helpers
import op_matrix as om
import pinn_oracle as po
import test_launch_geometry as tl
import test_random_residuals as tq
from test_f64_mode import _stencil_noise

PER_BATCH = {"int": 10, "f1": 11, "f2": 3, "sys16": 10, "sys64": 5, "long": 10, "dgm": 10, "f64_4m": 11, "f64_4s": 3}
CASES_OF = {s.name: om.ADJ + (om.SRC if s.name in ("f1", "f64_4m") else []) for s in om.SITES}
BATCHES = [(s, b) for s, names in CASES_OF.items() for b in range((len(names) + PER_BATCH[s] - 1) // PER_BATCH[s])]

_CELLS = {}         # (backend, site, case, symbolic) -> what the planner made of it


def _symbolic(site, case):
    """the front end of a (site, case) away from f1 (which takes both): alternating"""
    return bool(([s.name for s in om.SITES].index(site) + [c.name for c in om.CASES].index(case)) % 2)


def _build(npde, monkeypatch, site, case, symbolic):
    S, C = om.SITE[site], om.CASE[case]
    P = om.problem(npde, C, S, symbolic)
    if symbolic:
        monkeypatch.setenv("PINN_DESCRIPTOR", "2")
    else:
        monkeypatch.delenv("PINN_DESCRIPTOR", raising=False)
    try:
        kw = dict(integral_nodes=om.INT_Q) if S.arch == "integral" else {}
        disc = npde.PhysicsInformedNN(P.chains if len(P.chains) > 1 else P.chains[0], om.strategy(npde, S), init_params=P.theta, precision="f32", **kw)
        rep = npde.symbolic_discretize(P.sysm, disc)
    finally:
        monkeypatch.delenv("PINN_DESCRIPTOR", raising=False)
    return P, rep


def _to_f64(eng, sets):
    eng.set_option("precision", "f64")
    for k, s in enumerate(sets):
        eng.set_points_f64(k, s)


def _f64_kernel(eng, term=0):
    return re.search(r"f64_kernels=(\S+)", eng.describe()).group(1).split(",")[term]


def _cell(npde, monkeypatch, site, case, symbolic, built=None):
    """the record of one cell: which kernel holds term 0, how much of its tape the interpreter runs, the op codes of the lowered term"""
    key = (tq._backend(npde), site, case, symbolic)
    if key in _CELLS:
        return _CELLS[key]
    P, rep = built if built is not None else _build(npde, monkeypatch, site, case, symbolic)
    eng = rep.engine
    from neuralpde_jl_amd import sexpr, symbolic as sym
    vi = npde.get_vars(P.sysm.ivs, P.sysm.dvs)
    term = sym.lower_equation(P.sysm.eqs[0], vi, [], "pde")
    d, ns, ops = term.dim, len(term.slots), term.ops
    if term.integrals:                  # the integral site: the codes of the integrand's tape, rows [coordinates | its slots | ops]
        ns, ops = len(term.integrals[0].slots), term.integrals[0].ops
    # op -> does any instruction of that code read a row that is neither a coordinate nor a coordinate-only op (tape form)
    rows = [False] * d + [True] * ns
    codes = {}
    from neuralpde_jl_amd.ir import BINARY, NULLARY
    for q in ops:
        a = rows[q.a] if q.op not in NULLARY else False
        b = rows[q.b] if q.op in BINARY else False
        rows.append(a or b)
        cur = codes.setdefault(q.op, [False, False])
        cur[0], cur[1] = cur[0] or a, cur[1] or b
    rec = dict(K=eng.K, codes=codes, sexpr=sexpr.sexpr(P.sysm.eqs[0].lhs), kernels=[], how=[], tape=None, of=None, sources=None, affine=False,
               f64_kernel=None, f64_path=None, f64_affine=None, lanes_kernel=None, lanes_path=None)
    for line in eng.describe().splitlines():
        m = re.match(r"group \d+( \[[^\]]*\])? net=\d+ kernel=(\S+) .*terms=([\d,+a-z()]+)", line)
        if m and "0" in re.findall(r"\d+", re.sub(r"\(\d+\)", "", m.group(3))):
            rec["kernels"].append(m.group(2))
            rec["how"].append(m.group(1) or "")
        m = re.match(r"term 0: tape ops=(\d+) of (\d+), sources=(\d+)", line)
        if m:
            rec["tape"], rec["of"], rec["sources"] = (int(v) for v in m.groups())
            rec["affine"] = "affine residual" in line
    if om.SITE[site].precision == "f64":
        sets = rep.pde_train_sets + rep.bcs_train_sets
        th = np.asarray(rep.flat_init_params, dtype=np.float64)
        if eng.get_option("precision") != "f64":
            _to_f64(eng, sets)
        eng.loss_grad_f64(th)
        rec["f64_kernel"], rec["f64_path"], rec["f64_affine"] = _f64_kernel(eng), eng.get_option("f64_path"), int(eng.get_option("f64_affine"))
        if site == "f64_4m":
            with tl._env(PINN_F64_NO_MFMA="1"):
                eng.loss_grad_f64(th)
                rec["lanes_path"] = eng.get_option("f64_path")
    _CELLS[key] = rec
    return rec


def _values(prob0, A, sub, th, pts):
    """a subexpression of the case on the interior points, by the oracle"""
    prob = po.Problem(chains=prob0.chains, depvars=prob0.depvars, net_indvars=prob0.net_indvars, pde_terms=[po.TermSpec(sub, sp.Integer(0), (A.x, A.y))], bc_terms=[])
    return po.residual_values(prob, th, 0, pts, mode="exact").reshape(-1)


def _check_conditions(P, prob, th, pts, tag):
    """the conditions on the inputs, on the reference alone"""
    is_dep = lambda e: bool(e.atoms(sp.core.function.AppliedUndef))
    for kind, sub, dep in om.conditions(P.expr, is_dep):
        v = _values(prob, P.atoms, sub, th, pts)
        if kind == "base":
            assert v.min() > 0.5, (tag, kind, sub, v.min())
        elif kind == "den":
            assert np.abs(v).min() > 0.5, (tag, kind, sub, np.abs(v).min())
        else:
            assert np.abs(v).min() > 1e-4, (tag, kind, sub, np.abs(v).min())
            if dep:
                pos = int(np.count_nonzero(v > 0))
                assert 5 <= pos <= v.size - 5, (tag, kind, sub, pos, v.size)


def _integral_reference(P, prob):
    """the float64 reference of the integral site (the oracle has no integral node): the Q-node Gauss-Legendre sum of the integrand — the
    oracle's own evaluation of 1.5 expr at (x, s_q) — plus the rest of the equation; gradients by torch autograd.  The rule is part of the
    method (tests/test_integral_terms.py); returns (Evaluation, residual vectors) like the oracle's exact mode"""
    import torch
    from numpy.polynomial.legendre import leggauss
    A = P.atoms
    xi, wq = leggauss(om.INT_Q)
    inner = po.build_residual(prob, po.TermSpec(1.5 * P.expr, sp.Integer(0), (A.x, A.y)), mode="exact")
    outer = po.build_residual(prob, po.TermSpec(A.uy + A.U, sp.sin(sp.pi * A.x) * A.y, (A.x, A.y)), mode="exact")
    bcs = [po.build_residual(prob, t, mode="exact") for t in prob.bc_terms]

    def reference(th, sets, w):
        tht = torch.tensor(np.asarray(th, dtype=np.float64), dtype=po.DT, requires_grad=True)
        cs = [torch.tensor(np.asarray(s, dtype=np.float64), dtype=po.DT) for s in sets]
        r = outer(cs[0], tht)
        for q in range(om.INT_Q):
            at = torch.cat([cs[0][0:1], torch.full_like(cs[0][1:2], 0.5 * (float(xi[q]) + 1.0))], dim=0)
            r = r + 0.5 * float(wq[q]) * inner(at, tht)
        rs = [r] + [f(c, tht) for f, c in zip(bcs, cs[1:])]
        losses = [torch.mean(v * v) for v in rs]
        total = sum(float(wk) * L for wk, L in zip(w, losses))
        (g,) = torch.autograd.grad(total, tht)
        return (po.Evaluation(np.array([float(L.detach()) for L in losses]), float(total.detach()), g.numpy()),
                [v.detach().numpy().reshape(-1) for v in rs])

    return reference


def _check_cell(npde, monkeypatch, site, case, symbolic):
    S = om.SITE[site]
    P, rep = _build(npde, monkeypatch, site, case, symbolic)
    eng = rep.engine
    tag = (tq._backend(npde), "op", site, case, "sexpr" if symbolic else "tape")
    prob = helpers.oracle_problem(npde, P.sysm, P.chains)
    sets = rep.pde_train_sets + rep.bcs_train_sets
    assert sets[0].shape[1] == om.N_INTERIOR and all(s.shape[1] == om.N_BOUNDARY for s in sets[len(P.sysm.eqs):])
    th = np.asarray(rep.flat_init_params, dtype=np.float64)
    w = np.linspace(1.0, 2.0, eng.K)
    reference, pts = None, sets[0]
    if S.arch == "integral":            # the conditions hold on the site set (x_i, s_q), where the integrand is evaluated
        from numpy.polynomial.legendre import leggauss
        assert "+integral(%d)" % om.INT_Q in eng.describe(), tag
        reference = _integral_reference(P, prob)
        pts = np.concatenate([np.stack([sets[0][0], np.full(sets[0].shape[1], 0.5 * (xq + 1.0))]) for xq in leggauss(om.INT_Q)[0]], axis=1)
    _check_conditions(P, prob, th, pts, tag)
    if S.precision == "f32":
        ref = tq._check_sets(eng, prob, th, w, sets, False, tag, reference=reference)
        tq._check_conditioning(prob, th, w, sets, ref, tag, reference=reference)
        _cell(npde, monkeypatch, site, case, symbolic, built=(P, rep))
        return
    _to_f64(eng, sets)
    ref = tq._check_sets(eng, prob, th, w, sets, True, tag)
    kernel = _f64_kernel(eng)
    assert eng.get_option("f64_path") == "mfma" and kernel.startswith("mfma-sliced:" if site == "f64_4s" else "mfma:HT"), (tag, kernel)
    tq._check_conditioning(prob, th, w, sets, ref, tag)
    if site == "f64_4m":
        with tl._env(PINN_F64_NO_MFMA="1"):                                  # the same handle on the lanes kernels
            tq._check_sets(eng, prob, th, w, sets, True, tag + ("lanes",))
            assert eng.get_option("f64_path") == "lanes", tag
        if case in om.STENCIL:
            # derivative = stencil: the slots by the reference's central differences, the same tape; against the stencil-mode oracle at the
            # bar of test_f64_mode.test_stencil_mode_reproduces_the_reference_finite_differences (4 x the stencil oracle's own noise floor)
            st = po.loss_and_grad(prob, th, sets, weights=w, mode="stencil")
            noise = _stencil_noise(prob, th, sets, w, st)
            eng.set_option("derivative", "stencil")
            l, g = eng.loss_grad_f64(th, w)
            le, g2, gi = helpers.rel_errors(l, g, st)
            print("RR", *tag, "stencil", *("%.3e" % v for v in (le.max(), g2, gi)), "noise", *("%.3e" % v for v in noise))
            assert le.max() < 4 * max(noise[0], 2e-9) and g2 < 4 * max(noise[1], 2e-9) and gi < 4 * max(noise[2], 2e-9), (tag, le, g2, gi, noise)
            for k in range(eng.K):
                r = eng.residual_f64(k, th, sets[k].shape[1])
                rr = po.residual_values(prob, th, k, sets[k], mode="stencil")
                assert np.max(np.abs(r - rr)) < 2e-6 * max(1.0, np.max(np.abs(rr))), (tag, k)
            eng.set_option("derivative", "exact")
    _cell(npde, monkeypatch, site, case, symbolic, built=(P, rep))


@pytest.mark.parametrize("site,batch", BATCHES)
def test_op_cases_meet_the_oracle(npde, use_emu, monkeypatch, tmp_path, site, batch):
    if site != "dgm":                   # (family 3 has no ahead-of-time table: a DGM kernel is always specialised, once per machine)
        monkeypatch.setenv("PINN_JIT_DIR", str(tmp_path / "jit"))
    names = CASES_OF[site]
    for case in names[batch * PER_BATCH[site]: (batch + 1) * PER_BATCH[site]]:
        for symbolic in ((False, True) if site == "f1" else (_symbolic(site, case),)):
            _check_cell(npde, monkeypatch, site, case, symbolic)
    # the cases stay inside the ahead-of-time kernel table: none specialises a kernel at run time
    assert not os.path.exists(tmp_path / "jit"), sorted(p.name for p in (tmp_path / "jit").rglob("*"))


def test_residual_one_row_past_the_fused_tape_takes_the_two_launch_path(npde, use_emu, monkeypatch, tmp_path):
    """Regression: the planner chose between the fused 32-row tape and the two-launch path by the channels the residual READS, then counted
    the channels of the kernel that RUNS it.  For {u, u_x, u_y, u_xx, u_yy} on a small net that is the 6-channel Hessian kernel of the
    ahead-of-time table: a residual of 32 rows by the first count and 33 by the second was refused ("residual expression too long for the
    fused kernel tape (33 rows > 32)") instead of planned.  Both front ends; the checks of every other cell."""
    monkeypatch.setenv("PINN_JIT_DIR", str(tmp_path / "jit"))
    monkeypatch.setitem(om.CASE, om.ROWS_33.name, om.ROWS_33)
    for symbolic in (False, True):
        _check_cell(npde, monkeypatch, "f1", om.ROWS_33.name, symbolic)
        rec = _cell(npde, monkeypatch, "f1", om.ROWS_33.name, symbolic)
        assert len(rec["kernels"]) == 1 and "(C=6)" in rec["kernels"][0] and "coupled fwd/gradin" in rec["how"][0], rec
    assert not os.path.exists(tmp_path / "jit")


# what a site must show in describe() for term 0: (kernel name pattern, launch marker)
EXPECT = {"f1": (r"^F1_", ""), "f2": (r"^F2_HP64_", ""), "sys16": (r"^F1_", "coupled fwd/gradin"), "sys64": (r"^F2_HP64_", "coupled tail"),
          "long": (r"^F1_", "coupled fwd/gradin"), "dgm": (r"^F3_", ""), "int": (r"^F1_", "coupled fwd/gradin"), "f64_4m": (r"", ""), "f64_4s": (r"", "")}
SEXPR_HEAD = {"TAN": "(tan ", "SECH": "(sech ", "POWC": "(^ ", "POW": "(^ ", "POWI": "(^ ", "DIV": "(/ ", "MAX": "(max ", "MIN": "(min ", "SINPI": "(sin (* ",
              "COSPI": "(cos (* ", "ABS": "(abs ", "LOG": "(log ", "SQRT": "(^ ", "SINH": "(sinh ", "COSH": "(cosh ", "SIN": "(sin ", "COS": "(cos ",
              "EXP": "(exp ", "TANH": "(tanh ", "ADD": "(+ ", "SUB": "(+ ", "MUL": "(* ", "NEG": "(* -1 ", "ADDC": "(+ ", "MULC": "(* "}
BINARY_ADJ = {"POW": ("pow_net_net",), "DIV": ("div_net_net",), "MAX": ("max_net_net", "max_3"), "MIN": ("min_net_net", "min_3"),
              "ADD": ("bilinear",), "SUB": ("bilinear",), "MUL": ("bilinear",)}


def test_op_x_site_table_is_full(npde, use_emu, monkeypatch, tmp_path):
    """op x site, from what was actually planned: describe() (kernel name, tape op count, sources=, coupled / coupled tail markers),
    get_option("f64_path"), the float64 kernel string and the instruction codes of the lowered term.  Every op with an adjoint has run with a
    non-source operand — binary ops in both operand positions — at every fp32 and float64 site; no affine shortcut swallowed a case; every op
    went through both front ends.

    What a cell holds.  The op codes and the network-operand flags come from symbolic.lower_equation for BOTH front ends; for the sexpr front
    end the evidence that the op was handed over is the head of the s-expression alone ("(^ " stands for SQRT, POWC and POWI alike, "(+ " for
    ADD, SUB and ADDC): the table records what the library was given, not what sexpr.cpp emitted or what the planner kept on the tape after
    hoisting.  At the coupled sites (sys16, sys64, long, int) describe() prints no "term 0: tape ops" line, so the tape count and the
    "affine residual" marker are not read there: those residuals are nonlinear by construction (the op case itself), and the
    "coupled" marker of the group shows that k_expr ran them.
    The cells are those the batch tests above recorded in this process; run alone (-k, or another worker) this test builds every cell
    itself, about 330 handles, which takes minutes on the emulation."""
    table = {}                      # op -> site -> cases that ran it with a network operand
    front = {}                      # op -> front ends
    for s in om.SITES:
        if s.name != "dgm":             # (as in the batch test: family 3 alone specialises its kernel, once per machine)
            monkeypatch.setenv("PINN_JIT_DIR", str(tmp_path / "jit"))
        else:
            monkeypatch.delenv("PINN_JIT_DIR", raising=False)
        for case in CASES_OF[s.name]:
            C = om.CASE[case]
            for symbolic in ((False, True) if s.name == "f1" else (_symbolic(s.name, case),)):
                rec = _cell(npde, monkeypatch, s.name, case, symbolic)
                tag = (s.name, case, symbolic, rec)
                pat, how = EXPECT[s.name]
                assert rec["kernels"] and all(re.search(pat, k) for k in rec["kernels"]) and any(how in h for h in rec["how"]), tag
                if not how:
                    assert not any("coupled" in h for h in rec["how"]), tag
                    assert rec["tape"] > 0 and not rec["affine"], tag             # the interpreter ran this term's tape
                    assert C.kind != "src" or rec["sources"] > 0, tag             # ... and k_src the coordinate-only ops
                if s.precision == "f64":
                    want = "mfma-sliced:HT" if s.name == "f64_4s" else "mfma:HT"
                    assert rec["f64_path"] == "mfma" and rec["f64_kernel"].startswith(want) and rec["f64_affine"] == rec["K"] - 1, tag      # (the two Dirichlet terms are affine; term 0 is not)
                    assert s.name != "f64_4m" or rec["lanes_path"] == "lanes", tag
                for op in C.ops:
                    assert op in rec["codes"], (tag, op)
                    assert SEXPR_HEAD[op] in rec["sexpr"], (tag, op)
                    if C.kind == "adj":
                        a, b = rec["codes"][op]
                        assert a or b, (tag, op)
                        if op in BINARY_ADJ and case in BINARY_ADJ[op]:
                            assert a and b, (tag, op)
                        table.setdefault(op, {}).setdefault(s.name, []).append(case)
                        if s.name == "f64_4m":
                            table[op].setdefault("f64_lanes", []).append(case)
                    else:
                        table.setdefault(op + " (k_src)", {}).setdefault(s.name, []).append(case)
                    front.setdefault(op, set()).add("sexpr" if symbolic else "tape")
    sites = [s.name for s in om.SITES] + ["f64_lanes"]
    from neuralpde_jl_amd.ir import OPS
    with_adjoint = [op for op in OPS if op not in ("CONST", "DATA")]
    print("OPM table", tq._backend(npde), "sites", *sites)
    for op in with_adjoint + [op + " (k_src)" for op in with_adjoint if op + " (k_src)" in table]:
        row = table.get(op, {})
        print("OPM", "%-14s" % op, *("%s=%d" % (s, len(row.get(s, []))) for s in sites))
    for op in with_adjoint:
        assert all(table.get(op, {}).get(s) for s in sites), (op, table.get(op))           # no empty reachable cell
        assert front[op] == {"tape", "sexpr"}, (op, front[op])
        for bop, cases in BINARY_ADJ.items():                                             # both operand positions at every site
            assert all(any(c in table[bop][s] for c in cases) for s in sites), bop
    for op in with_adjoint:
        if op not in ("ADD", "SUB", "MUL", "NEG", "ADDC", "MULC"):
            assert table.get(op + " (k_src)", {}).get("f1") and table[op + " (k_src)"].get("f64_4m"), op
    assert not os.path.exists(tmp_path / "jit")
