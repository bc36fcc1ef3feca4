"""TEST INFRASTRUCTURE: the checks of tests/value_update_checks.py with torch device tensors as input (QPS_MEM_DEVICE), in a process of its own that imports
torch BEFORE the library -- torch bundles a HIP runtime, and device memory of one runtime is nothing the other knows about (one runtime per
process).  tests/test_gpu_value_update.py starts it once; one JSON line per check on stdout: {"check": name, "ok": bool, "detail": text}."""
import io
import json
import os
import sys
import traceback
from contextlib import redirect_stdout

import torch  # noqa: E402  (first: see above)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import matrix_update_cases as mc  # noqa: E402
import value_update_cases as vc  # noqa: E402
import value_update_checks as ck  # noqa: E402


def to_device(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to("cuda:0")


def value_errors(gpu, wrap):
    """What the Python layer refuses before the library is called: the handle stays what it was."""
    key = mc.CG_BANDED
    vP, vA = vc.values(key, 1)
    with ck.make(gpu, key) as h:
        before = ck.run(h, **mc.solve_kw(key))
        strided = wrap(np.repeat(vP, 2))[::2]
        assert not strided.is_contiguous() and strided.numel() == len(vP)
        for what, bad in (("float32", wrap(vP).to(torch.float32)), ("cpu", torch.from_numpy(vP)), ("non-contiguous", strided)):
            try:
                h.update_values(bad)
            except ValueError as e:
                print(what, e)
            else:
                raise AssertionError(f"{what}: no ValueError")
        try:
            h.update_values(wrap(vP), vA)                                  # a tensor beside a host array
        except ValueError as e:
            print("mixed", e)
        else:
            raise AssertionError("mixed: no ValueError")
        assert ck.same(ck.run(h, reuseFactor=True, **mc.solve_kw(key)), before)


def main():
    import quadraticprogramsolver_amd as gpu
    checks = dict(ck.CHECKS)
    checks["value-errors"] = (value_errors, ())
    names = sys.argv[1:] or list(checks)
    for name in names:
        fn, args = checks[name]
        log = io.StringIO()
        try:
            with redirect_stdout(log):
                fn(gpu, to_device, *args)
            ok, detail = True, log.getvalue()[-2000:]
        except Exception:
            ok, detail = False, log.getvalue()[-2000:] + traceback.format_exc()
        print(json.dumps({"check": name, "ok": ok, "detail": detail}), flush=True)
        if not ok and "QPS_ERR_HIP" in detail:                             # a device error: nothing more is started on that device
            break


if __name__ == "__main__":
    main()
