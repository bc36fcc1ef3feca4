"""The boundary's gates that need a handle, on tiny handles: every qps_*_shared_* entry point on a handle that is no shared-matrix batch, every refused
argument of a shared handle (after which the handle solves bitwise as before), and the entry points that want another kind of handle.  Status and text are
those of tests/golden/capi_errors.json ("gates", recorded on the MI355X before the boundary was refactored); the cases live in tests/capi_error_cases.py."""
import pytest

import capi_error_cases as cc

pytestmark = pytest.mark.gpu
NOT_SHARED = ("dense", "csc", "fused_batch", "fallback_batch", "proxqp")


@pytest.fixture(scope="module")
def gates(gpu):
    from quadraticprogramsolver_amd import _lib
    unchanged = []
    return cc.run_gates(_lib.lib(), unchanged), unchanged, cc.load_fixture()["gates"]


def test_every_gate_answers_as_recorded(gates):
    got, _, want = gates
    for name in sorted(set(got) | set(want)):
        print(name, got.get(name))
    assert got == want


def test_shared_entry_points_refuse_every_other_handle(gates):
    """QPS_ERR_UNSUPPORTED with the entry point's own "only shared-matrix batch handles (...)" text; qps_update_shared_vectors answers BAD_ARGUMENT."""
    got, _, _ = gates
    hits = {k: v for k, v in got.items() if k.split("@")[-1] in NOT_SHARED and "shared" in k.split("@")[0]}
    assert len(hits) == 11 * len(NOT_SHARED)
    for k, v in hits.items():
        fn = k.split("@")[0]
        if fn == "qps_update_shared_vectors":
            assert v == {"status": 1, "message": "not a shared-matrix batch handle"}, k
        else:
            assert v["status"] == 8 and v["message"].startswith(fn + ": only shared-matrix batch handles (qps_create_dense_shared_batch, qps_create_csc_shared_batch) "), (k, v)


def test_a_refused_argument_leaves_the_shared_handle_as_it_was(gates):
    got, unchanged, _ = gates
    assert len(unchanged) == 15 and all(same for _, same in unchanged), unchanged
    for name, _ in unchanged:
        assert got[name + "@shared"]["status"] in (1, 3), (name, got[name + "@shared"])


def test_handles_of_the_wrong_kind(gates):
    got, _, _ = gates
    assert got["qps_solve@fused_batch"] == got["qps_solve@fallback_batch"] == got["qps_solve@proxqp"] == {"status": 1, "message": "invalid handle"}
    assert got["qps_solve_batch@dense"] == got["qps_solve_batch@csc"] == {"status": 1, "message": "not a batch handle"}
    assert got["qps_proxqp_solve@dense"] == got["qps_proxqp_solve@shared"] == {"status": 1, "message": "not a ProxQP handle"}
    assert got["qps_operator_apply@fused_batch"]["status"] == 1 and "invalid handle" in got["qps_operator_apply@fused_batch"]["message"]
    assert got["qps_create_csc:too_large_to_densify"] == {"status": 2, "message": "problem too large to densify"}
