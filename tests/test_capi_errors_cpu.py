"""The refusals of the C boundary (csrc/qps_capi.hip), pinned: status and full qps_last_error text of every case of tests/capi_error_cases.py against
tests/golden/capi_errors.json, which was recorded from the library before the boundary was split into shape checks, a creator tail and a shared-family
gate.  No entry point may change its status, its wording, or the order in which it finds faults.  No device needed."""
import pytest

import capi_error_cases as cc


@pytest.fixture(scope="module")
def fixture():
    return cc.load_fixture()


@pytest.fixture(scope="module")
def L(qps):
    from quadraticprogramsolver_amd import _lib
    return _lib.lib()


def test_the_table_and_the_fixture_hold_the_same_cases(fixture):
    assert sorted(fixture["cpu"]) == sorted(c.name for c in cc.CASES)
    assert sorted(fixture["with_device"]) == sorted(cc.DEVICE_CASES)


def test_the_device_flag_cannot_swallow_the_table():
    """Only a well-formed call of each creator, and the finiteness cases of qps_proxqp_create_dense (which asks for the device first), may depend on
    whether a GPU is visible."""
    assert len(cc.DEVICE_CASES) <= len(cc.CREATORS) + len(cc.PROXQP_FINITENESS)
    assert sorted(cc.DEVICE_CASES) == sorted([f"{fn}:well_formed" for fn in cc.CREATORS] + [f"qps_proxqp_create_dense:{k}" for k in cc.PROXQP_FINITENESS])


def test_every_pair_is_recorded_with_the_answer_of_its_first_fault(fixture):
    """What makes the pairs pin the order: the recording itself answers a pair as it answers the earlier fault alone."""
    pairs = [c for c in cc.CASES if c.first]
    assert len(pairs) >= 100
    for c in pairs:
        assert fixture["cpu"][c.name] == fixture["cpu"][c.first], c.name


def test_without_a_device_the_device_cases_were_recorded_as_no_device(fixture):
    for name in cc.DEVICE_CASES:
        assert fixture["cpu"][name] == {"status": 7, "message": "no HIP device visible: libqps_hip has no CPU fallback"}, name
        assert fixture["with_device"][name]["status"] == (3 if name.split(":")[1] in cc.PROXQP_FINITENESS else 0), name


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_boundary_answers_as_recorded(L, fixture, case):
    section = "with_device" if case.device and L.qps_device_count() > 0 else "cpu"
    got = cc.run_case(L, case)
    print(case.name, got)
    assert got == fixture[section][case.name]
