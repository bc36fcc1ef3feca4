"""The single-launch small-problem kernels of k_small.hip in every geometry band, both types: K = 20 iterations with a check every 10 at ϵ = 0, ρ = 0.1 and a
non-zero warm start, against the structured fp64 reference -- x, z, y and the two residuals of the last check.  tests/small_band_cases.py holds the
case table, the route every case reaches with the dispatch lines that send it there, the bounds and the figures measured on an MI355X;
tests/test_small_bands_cpu.py checks on the CPU that the table covers every reachable form and that every case would fail a kernel that dropped its
last column block or its last row.  Every figure is printed before its assertion (run with -s)."""
import json
import os
import subprocess
import sys
import textwrap
import time

import numpy as np
import pytest

import loop_param_cases as C
import small_band_cases as S
import width_band_cases as W

pytestmark = pytest.mark.gpu


def _hold(tag, name, got, ref, bound, t0):
    """Print every figure against its bound, then assert them."""
    fig = S.errors(got, ref, S.ADMM_KEYS)
    print(f"{tag} {name}: " + " ".join(f"{k} {v:.2e}/{bound[k]:.1e}" for k, v in fig.items()) + f" wall {time.perf_counter() - t0:.2f} s")
    for k, v in fig.items():
        assert v <= bound[k], (name, tag, k, v, bound[k])              # (a NaN fails here too)
    return fig


def _solve(h, f, **extra):
    x, info = f.x0.copy(), {}
    h.solve(x, info=info, **C.api_kw(S.solve_params(**extra)))
    z, y = h.dual()
    return dict(x=x, z=z, y=y, resPrim=info["resPrim"], resDual=info["resDual"]), info


def _handle(gpu, case, f):
    return gpu.QuadraticProgram(f.dense_P(), f.q, f.A, f.l, f.u, dtype=case.dtype)


def _adaptive(h, case, f, t0, tag):
    ra = S.reference(case, adpt=True)
    got, info = _solve(h, f, adptRho=True, fctrRho=S.ADMM_FCTR)
    _hold(tag + " adaptive", S.case_id(case), got, ra, S.bounds(case, adpt=True), t0)
    assert info["iterations"] == S.K and info["sweepVariant"] == 4, info
    print(f"{tag} adaptive {S.case_id(case)}: numRefactor {info['numRefactor']}/{ra['numRefactor']} rhoFinal {info['rhoFinal']:.12g}/{ra['rhoFinal']:.12g}")
    if case.dtype == "f64":                                            # one refactor after the first check, a relaunch from it_begin = 10
        assert info["numRefactor"] == ra["numRefactor"] == 1 and info["rhoFinal"] == pytest.approx(ra["rhoFinal"], rel=1e-9)


@pytest.mark.parametrize("case", S.SINGLE_CASES, ids=S.case_id)
def test_single_launch_iterates_match_the_structured_reference(gpu, case):
    t0 = time.perf_counter()
    f, ref, bound = S.member(case), S.reference(case), S.bounds(case)
    key = (case.dtype, case.n, case.m)
    with _handle(gpu, case, f) as h:
        got, info = _solve(h, f)
        _hold(case.route[0], S.case_id(case), got, ref, bound, t0)
        assert info["iterations"] == S.K and info["convFlag"] == 1 and info["sweepVariant"] == 4, info
        if key in S.REPEAT_SINGLE:                                     # stale LDS or scratch state across launches would show here
            again, info2 = _solve(h, f)
            same = all(np.array_equal(again[k], got[k]) for k in ("x", "z", "y")) and again["resPrim"] == got["resPrim"] and again["resDual"] == got["resDual"]
            print(f"repeat {S.case_id(case)}: bit for bit {same}")
            assert same and info2["iterations"] == S.K and info2["sweepVariant"] == 4
    if key in S.ADAPTIVE_SINGLE:                                       # a fresh handle, as every run
        with _handle(gpu, case, f) as h:
            _adaptive(h, case, f, t0, case.route[0])


@pytest.mark.parametrize("case", S.OUTSIDE_CASES, ids=S.case_id)
def test_shapes_just_outside_the_domain_take_the_multi_launch_loop(gpu, case):
    t0 = time.perf_counter()
    f = S.member(case)
    with _handle(gpu, case, f) as h:
        got, info = _solve(h, f)
    _hold("outside", S.case_id(case), got, S.reference(case), S.bounds(case), t0)
    assert info["iterations"] == S.K and info["sweepVariant"] != 4, info


def _batch(gpu, case, t0, tag, adpt=False):
    members = [S.member(case, k) for k in range(S.COUNT)]
    extra = dict(adptRho=True, fctrRho=S.ADMM_FCTR) if adpt else {}
    with gpu.QuadraticProgramBatch([(f.dense_P(), f.q, f.A, f.l, f.u) for f in members], dtype=case.dtype) as h:
        X, flags, infos = h.solve(np.stack([f.x0 for f in members]), **C.api_kw(S.solve_params(**extra)))
        Z, Y = h.dual()
    for k in range(S.COUNT):                                           # every QP against its own reference run
        ref = S.reference(case, k, adpt)
        got = dict(x=X[k], z=Z[k], y=Y[k], resPrim=infos[k]["resPrim"], resDual=infos[k]["resDual"])
        _hold(tag, S.emu_key(case, k), got, ref, S.bounds(case, k), t0)
        # (the batch report's sweepVariant names the sweep of its factor, chol_sweep_variant, also on the single-launch path: it never reads 4)
        assert infos[k]["iterations"] == S.K and int(flags[k]) == 1 and infos[k]["sweepVariant"] == W.sweep_variant(case.dtype, case.NP) == 3, infos[k]
        if adpt:
            print(f"{tag} {S.emu_key(case, k)}: numRefactor {infos[k]['numRefactor']}/{ref['numRefactor']} rhoFinal {infos[k]['rhoFinal']:.12g}/{ref['rhoFinal']:.12g}")
            assert infos[k]["numRefactor"] == ref["numRefactor"] and infos[k]["rhoFinal"] == pytest.approx(ref["rhoFinal"], rel=1e-9)


@pytest.mark.parametrize("case", S.BATCH_CASES, ids=S.case_id)
def test_batch_register_kernel_matches_the_reference_of_every_member(gpu, case):
    t0 = time.perf_counter()
    _batch(gpu, case, t0, "batch")
    if (case.dtype, case.n, case.m) == S.ADAPTIVE_BATCH:               # one member refactors after the first check, the others run on
        _batch(gpu, case, t0, "batch adaptive", adpt=True)


CHILD = textwrap.dedent('''
    import sys, json
    sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
    import quadraticprogramsolver_amd as q
    import loop_param_cases as C
    import small_band_cases as S
    out = {}
    for dtype, n, m in json.loads(sys.argv[3]):
        case = S.find(S.SINGLE_CASES, dtype, n, m)
        f = S.member(case)
        with q.QuadraticProgram(f.dense_P(), f.q, f.A, f.l, f.u, dtype=dtype) as h:
            x, info = f.x0.copy(), {}
            h.solve(x, info=info, **C.api_kw(S.solve_params()))
            z, y = h.dual()
        out[S.case_id(case)] = dict(x=x.tolist(), z=z.tolist(), y=y.tolist(), resPrim=info["resPrim"], resDual=info["resDual"],
                                    iterations=info["iterations"], sweepVariant=info["sweepVariant"])
    print(json.dumps(out))
''')


def test_forms_reached_only_through_knobs(gpu, tmp_path):
    """QPS_SMALL_REG, QPS_SMALL_LDSMAT and QPS_SMALL_THREADS are read once per process: one child per knob set, one after the other, each held to the
    references and bounds of the table.  A child that fails ends the test: no further child is started."""
    tests = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "small_band_child.py"
    script.write_text(CHILD)
    for env_extra, runs in S.KNOB_RUNS:
        t0 = time.perf_counter()
        env = {k: v for k, v in os.environ.items() if not k.startswith("QPS_")}
        env.update(env_extra)
        shapes = json.dumps([r[:3] for r in runs])
        r = subprocess.run([sys.executable, str(script), os.path.dirname(tests), tests, shapes], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120)
        assert r.returncode == 0, (env_extra, r.returncode, r.stderr[-2000:])
        out = json.loads(r.stdout.strip().splitlines()[-1])
        tag = ",".join(f"{a}={b}" for a, b in env_extra.items())
        for dtype, n, m, _ in runs:
            case = S.find(S.SINGLE_CASES, dtype, n, m)
            o = out[S.case_id(case)]
            got = dict(x=np.array(o["x"]), z=np.array(o["z"]), y=np.array(o["y"]), resPrim=o["resPrim"], resDual=o["resDual"])
            _hold(tag, S.case_id(case), got, S.reference(case), S.bounds(case), t0)
            assert o["iterations"] == S.K and o["sweepVariant"] == 4, (tag, o["iterations"], o["sweepVariant"])
