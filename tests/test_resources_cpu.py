"""Ownership of device resources (csrc/bf_resources.h), the part that needs no device: a create that fails gives back what it took and its handle, and the types
that take nothing from the device come and go without a trace in the counters of bf_debug_live_resources."""
import ctypes as C

import pytest

from tests import resource_cases as rc


def _live(capi):
    return capi.debug_live_resources()


@pytest.fixture()
def ctx(built, tmp_path):
    from bundlefusion_amd.capi import lib
    c = {"tmp": tmp_path, "sens": rc.write_sens(tmp_path / "small.sens")}
    # without a device there is no image manager and no pipeline to build on: a bundler's create reads the manager's sensor description before anything can fail, so
    # it gets a zeroed block of the struct's size at least; a player or recorder only asks whether the pipeline is null (null: host buffers, which need no device)
    c["_block"] = C.create_string_buffer(1 << 16)
    c["im"] = C.cast(c["_block"], C.c_void_p)
    c["pipeline"] = C.cast(c["_block"], C.c_void_p)
    sd = C.c_void_p()
    assert lib.bf_sensor_data_open(str(c["sens"]).encode(), C.byref(sd)) == 0
    c["sd"] = sd
    yield c
    lib.bf_sensor_data_close(sd)


@pytest.mark.parametrize("case", rc.DEVICE_CASES, ids=[c[0] for c in rc.DEVICE_CASES])
def test_a_create_that_fails_without_a_device_keeps_nothing(built, ctx, case):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_resources_gpu.py fails every acquisition of every create instead")
    from bundlefusion_amd import capi
    name, _, create = case
    before = _live(capi)
    status, handle, _ = create(ctx)
    assert status != 0 and not handle.value, name
    assert capi.lib.bf_last_error(), name
    after = _live(capi)
    assert after[:4] == before[:4], (name, before, after)          # owners (== handles), device allocations, device bytes, pinned + events + streams
    assert after[5] == 0


@pytest.mark.parametrize("case", rc.HOST_CASES, ids=[c[0] for c in rc.HOST_CASES])
def test_types_that_need_no_device_come_and_go(built, ctx, case):
    from bundlefusion_amd import capi
    name, _, create = case
    before = _live(capi)
    status, handle, destroy = create(ctx)
    assert status == 0 and handle.value, (name, capi.lib.bf_last_error())
    assert _live(capi)[1:4] == before[1:4], name                    # nothing taken from the device
    assert destroy() == 0
    after = _live(capi)
    assert after[:4] == before[:4], (name, before, after)
    assert after[5] == 0


def test_an_armed_failure_is_switched_off_by_zero(built):
    from bundlefusion_amd import capi
    capi.debug_fail_acquire(3)
    capi.debug_fail_acquire(0)
    h = C.c_void_p()
    assert capi.lib.bf_trajectory_manager_create(4, 30, C.c_float(0.0), C.byref(h)) == 0
    assert capi.lib.bf_trajectory_manager_destroy(h) == 0
