"""Whitened two-launch iteration of a dense fp64 handle that solves on its cached factor (QPS_WHITEN=1; k_pass_w.hip): every figure is
printed before its assertion (run with -s).  Cases and references: tests/whitened_cases.py; the recurrences alone are held to the numpy oracle by
tests/test_whitened_cpu.py.  The route is read off the profiler: a whitened solve times the category "apass(fused A-pass; whitened, ...", a classic
one "apass(fused A-pass)".

Measured on an MI355X against c_oracle.solve, bounds 1e-9 (x, z, residuals) and 1e-8 (y), reused (whitened) solve at fixed K = 60, x / z / y / resPrim /
resDual: (200, 330) 1.1e-15 / 2.8e-15 / 1.8e-15 / 3.7e-15 / 1.6e-14; (1100, 2130) 1.1e-15 / 5.2e-15 / 4.1e-15 / 1.8e-15 / 2.0e-13; (2100, 300) 4.0e-15 / 5.5e-14 /
2.1e-14 / 1.2e-14 / 1.1e-13; (4100, 70) 5.1e-13 / 1.8e-12 / 2.9e-13 / 3.5e-13 / 3.6e-12.  Off-default (α, σ) and x0 != 0: within 8.6e-15 on x / z / y, 1.7e-13 on the
residuals.  To ϵ = 1e-6 at ρ = 0.1: flag 3 at iteration 2350 on both sides, x 1.9e-15, residuals within 3.0e-14.  Stall stop:
flag 2 at iteration 500 on both sides, x 4.0e-14, residuals within 3.6e-13.  QPS_WHITEN unset: whitened at n padded 2112 only, the figures of the forced runs.
QPS_PASS_WGS = 512 / 1024: the reused solve shows the figures of the default (z 5.15e-15, resDual 2.03e-13).  The whole file runs in 7 s."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import whitened_cases as W
from loop_param_cases import TOL, api_kw

pytestmark = pytest.mark.gpu
BOUND = TOL["f64"]


@pytest.fixture(autouse=True)
def whiten_on(monkeypatch):
    monkeypatch.setenv("QPS_WHITEN", "1")          # read when a handle is created


def run(h, shape, x0=None, reuse=False, **params):
    """One solve with every launch timed; ``whitened``: which of the two pass categories it ran."""
    x = np.zeros(shape[0]) if x0 is None else np.array(x0)
    info = {}
    h.set_profiling(2)
    flag = h.solve(x, info=info, reuseFactor=reuse, **api_kw(params))
    names = [k["name"] for k in h.kernel_times()]
    h.set_profiling(0)
    z, y = h.dual()
    assert int(flag) == info["convFlag"]
    whitened = any(n.startswith("apass(fused A-pass; whitened") for n in names)
    assert whitened != any(n == "apass(fused A-pass)" for n in names), names
    return dict(x=x, z=z, y=y, resPrim=info["resPrim"], resDual=info["resDual"], convFlag=info["convFlag"], iterations=info["iterations"],
                whitened=whitened, tSetup=info["tSetup"])


def hold(tag, got, want):
    for f in W.FIELDS:
        d = W.rel(got[f], want[f])
        print(f"{tag}: {f} {d:.2e} (bound {BOUND[f]:.0e})")
        assert d <= BOUND[f], (tag, f, d)


def same(a, b):
    return all(np.array_equal(np.asarray(a[f]), np.asarray(b[f])) for f in W.FIELDS) and a["iterations"] == b["iterations"]


@pytest.mark.parametrize("shape", W.SHAPES, ids=W.IDS)
def test_fresh_then_reused_match_oracle(gpu, c_oracle, shape):
    """A fresh solve (factorises: classic loop), then two reused ones (whitened): each within the iterate bounds of the oracle, the two reused ones
    bitwise equal."""
    p = W.fixed_k()
    want = W.reference(c_oracle, shape, **p)
    with gpu.QuadraticProgram(*W.problem(shape), dtype="f64") as h:
        fresh = run(h, shape, **p)
        assert not fresh["whitened"] and fresh["iterations"] == W.K
        hold(f"{shape} fresh", fresh, want)
        first = run(h, shape, reuse=True, **p)
        assert first["whitened"] and first["iterations"] == W.K and first["convFlag"] == 1
        hold(f"{shape} reused", first, want)
        again = run(h, shape, reuse=True, **p)
        print(f"{shape}: B and G built in {1e3 * (first['tSetup'] - again['tSetup']):.2f} ms")
        assert again["whitened"] and same(first, again)


@pytest.mark.parametrize("alpha,sigma", W.OFF_DEFAULT)
@pytest.mark.parametrize("shape", W.SHAPES[:2], ids=W.IDS[:2])
def test_off_default_alpha_sigma_and_start(gpu, c_oracle, shape, alpha, sigma):
    p = W.fixed_k(alpha=alpha, sigma=sigma)
    x0 = W.start(shape)
    with gpu.QuadraticProgram(*W.problem(shape), dtype="f64") as h:
        run(h, shape, **p)
        got = run(h, shape, reuse=True, **p)
        assert got["whitened"]
        hold(f"{shape} alpha={alpha} sigma={sigma}", got, W.reference(c_oracle, shape, **p))
        got = run(h, shape, x0, reuse=True, **p)
        assert got["whitened"]
        hold(f"{shape} alpha={alpha} sigma={sigma} x0 != 0", got, W.reference(c_oracle, shape, x0, **p))


def test_stop_by_tolerance_at_the_oracles_iteration(gpu, c_oracle):
    """Feasible case to ϵ = 1e-6 at a fixed ρ: the oracle's flag and stopping iteration (tests/test_whitened_cpu.py shows the margin of that stop)."""
    shape = W.SHAPES[0]
    want = W.reference(c_oracle, shape, **W.TO_EPS)
    with gpu.QuadraticProgram(*W.problem(shape), dtype="f64") as h:
        run(h, shape, **dict(W.TO_EPS, numIterations=25))
        got = run(h, shape, reuse=True, **W.TO_EPS)
    print(f"{shape} to eps: oracle flag {want['convFlag']} at {want['iterations']}, whitened flag {got['convFlag']} at {got['iterations']}")
    assert got["whitened"] and (got["convFlag"], got["iterations"]) == (want["convFlag"], want["iterations"]) and want["convFlag"] == 3
    hold(f"{shape} to eps", got, want)


def test_stall_stop_is_decided_by_the_step_norm(gpu, c_oracle):
    """Equality rows nothing satisfies (whitened_cases.STALL): |z - zp| = 0 and the residuals stay O(1), so the run ends by convAdmm at the first check at
    which max|L (p - pp)| -- slot 7, filled by the L pass alone -- is at most ϵAdmm.  A step norm that read 0 would stop at the first check (25); the
    oracle stops at 500 (tests/test_whitened_cpu.py shows the margin on both sides)."""
    shape = W.SHAPES[0]
    want = W.reference(c_oracle, shape, stall=True, **W.STALL)
    with gpu.QuadraticProgram(*W.problem(shape, stall=True), dtype="f64") as h:
        run(h, shape, **dict(W.STALL, numIterations=25))
        got = run(h, shape, reuse=True, **W.STALL)
    print(f"{shape} stall: oracle flag {want['convFlag']} at {want['iterations']}, whitened flag {got['convFlag']} at {got['iterations']}")
    assert got["whitened"] and (got["convFlag"], got["iterations"]) == (want["convFlag"], want["iterations"]) and want["convFlag"] == 2
    assert W.STALL["numItrConv"] < want["iterations"] < W.STALL["numIterations"]
    hold(f"{shape} stall", got, want)


@pytest.mark.parametrize("shape,expect", [(W.SHAPES[1], False), (W.SHAPES[2], True), (W.SHAPES[3], False)], ids=["NP1152_below", "NP2112_inside", "NP4160_above"])
def test_default_band_without_the_variable(gpu, c_oracle, monkeypatch, shape, expect):
    """QPS_WHITEN unset: a reused solve is whitened for 2048 < n padded <= 4096 and classic on either side of the band."""
    monkeypatch.delenv("QPS_WHITEN")
    p = W.fixed_k()
    with gpu.QuadraticProgram(*W.problem(shape), dtype="f64") as h:
        assert not run(h, shape, **p)["whitened"]
        got = run(h, shape, reuse=True, **p)
    assert got["whitened"] == expect, (shape, got["whitened"])
    hold(f"{shape} QPS_WHITEN unset, reused ({'whitened' if expect else 'classic'})", got, W.reference(c_oracle, shape, **p))


def test_another_rho_rebuilds(gpu, c_oracle):
    """A reused solve at another ρ factorises (classic loop); the next one is whitened on matrices rebuilt for that factor."""
    shape = W.SHAPES[1]
    p1, p2 = W.fixed_k(), W.fixed_k(rho=W.OTHER_RHO)
    with gpu.QuadraticProgram(*W.problem(shape), dtype="f64") as h:
        run(h, shape, **p1)
        assert run(h, shape, reuse=True, **p1)["whitened"]
        assert not run(h, shape, reuse=True, **p2)["whitened"]
        got = run(h, shape, reuse=True, **p2)
        assert got["whitened"]
        hold(f"{shape} rho={W.OTHER_RHO} after rho=1", got, W.reference(c_oracle, shape, **p2))
        back = run(h, shape, reuse=True, **p1)
        assert not back["whitened"]
        hold(f"{shape} back at rho=1", run(h, shape, reuse=True, **p1), W.reference(c_oracle, shape, **p1))


CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import quadraticprogramsolver_amd as qps
import whitened_cases as W
from loop_param_cases import api_kw
shape = tuple(json.loads(sys.argv[3]))
out = []
with qps.QuadraticProgram(*W.problem(shape), dtype="f64") as h:
    for reuse in (False, True):
        x = np.zeros(shape[0]); info = {}
        h.set_profiling(2)
        h.solve(x, info=info, reuseFactor=reuse, **api_kw(W.fixed_k()))
        names = [k["name"] for k in h.kernel_times()]
        z, y = h.dual()
        out.append(dict(x=x.tolist(), z=z.tolist(), y=y.tolist(), resPrim=info["resPrim"], resDual=info["resDual"], names=names))
print(json.dumps(out))
"""


def child(tmp_path, shape, **env_extra):
    """A fresh and a reused solve of ``shape`` in one child process with the given QPS_ variables (and no others): [fresh, reused]."""
    tests = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "whitened_child.py"
    script.write_text(CHILD)
    env = {k: v for k, v in os.environ.items() if not k.startswith("QPS_")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, str(script), os.path.dirname(tests), tests, json.dumps(shape)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_switched_off_a_reused_solve_is_the_fresh_one(gpu, tmp_path):
    """QPS_WHITEN=0, one child process: the reused solve runs the classic loop and equals the fresh one bit for bit."""
    fresh, reused = child(tmp_path, W.SHAPES[1], QPS_WHITEN="0")
    assert not any(n.startswith("apass(fused A-pass; whitened") for n in fresh["names"] + reused["names"])
    assert all(fresh[f] == reused[f] for f in W.FIELDS)


@pytest.mark.parametrize("wgs", ["512", "1024"])
def test_pass_workgroup_knob_does_not_reach_the_whitened_pass(gpu, c_oracle, tmp_path, wgs):
    """QPS_PASS_WGS (read once per process: one child per value) sizes the launch of the classic pass.  The whitened pass always launches 256 workgroups
    and splits the rows of B over those: at (1100, 2130), MP = 2176, a split taken from the knob would cover 2048 (512) or 1024 (1024) rows only."""
    shape = W.SHAPES[1]
    fresh, reused = child(tmp_path, shape, QPS_WHITEN="1", QPS_PASS_WGS=wgs)
    assert any(n.startswith("apass(fused A-pass; whitened") for n in reused["names"]) and "apass(fused A-pass)" in fresh["names"]
    want = W.reference(c_oracle, shape, **W.fixed_k())
    hold(f"{shape} QPS_PASS_WGS={wgs} fresh", {f: np.asarray(fresh[f]) for f in W.FIELDS}, want)
    hold(f"{shape} QPS_PASS_WGS={wgs} reused", {f: np.asarray(reused[f]) for f in W.FIELDS}, want)


def test_close_returns_the_device_memory(gpu):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]

    def free_bytes():
        assert hip.hipDeviceSynchronize() == 0
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    shape = W.SHAPES[1]
    p = W.fixed_k(numIterations=10)
    n, m = shape
    NP, MP = -(-n // 64) * 64, -(-m // 64) * 64
    own = 8 * (MP * NP + NP * NP)                                        # B and G at least
    with gpu.QuadraticProgram(*W.problem(shape), dtype="f64") as h:      # (warm-up: runtime pools)
        run(h, shape, **p)
        run(h, shape, reuse=True, **p)
    before = free_bytes()
    with gpu.QuadraticProgram(*W.problem(shape), dtype="f64") as h:
        run(h, shape, **p)
        classic = before - free_bytes()
        assert run(h, shape, reuse=True, **p)["whitened"]
        held = before - free_bytes()
        print(f"{shape}: handle holds {classic / 2**20:.1f} MiB, {held / 2**20:.1f} MiB once whitened (B and G: {own / 2**20:.1f} MiB)")
        assert held - classic >= own
    after = free_bytes()
    print(f"{shape}: free before {before / 2**20:.1f} MiB, after close {after / 2**20:.1f} MiB")
    assert after >= before - (1 << 20)
