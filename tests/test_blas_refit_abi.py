"""BLAS refit without a device: the calls that must fail before they touch one, and the numpy reference of
tests/blas_refit_cases.py against data the GPU never made - the refit identity refit(build(x), x) == build(x) on all
eight golden BLAS fixtures."""
import ctypes as C

import numpy as np
import pytest

from blas_refit_cases import FIXTURES, key, mesh_bounds_reference, refit_reference, unkey
from conftest import fields_equal, golden
from voidin_amd import abi


def test_null_arguments_are_errors_not_crashes():
    lib = abi.load()
    item = (abi.BvhRefitItem * 1)()
    out = C.c_void_p(0x1234)
    assert lib.vd_bvh_refit_plan_dev(None, C.addressof(item), 1, C.byref(out)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_refit_plan_dev(None, None, 0, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_refit_planned_dev(None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_refit_plan_release(None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_refit(None, None, 0, None, 0, None, 0) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_trace_accel_update_geometry_dev(None, None) == abi.VD_ERR_INVALID_ARG


def test_refit_item_layout_is_the_headers():
    assert C.sizeof(abi.BvhRefitItem) == 48
    assert abi.BvhRefitItem.mesh_info.offset == 24 and abi.BvhRefitItem.n_vert.offset == 32 and abi.BvhRefitItem.status.offset == 44


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_sweep_reproduces_every_fixture(name):
    g = golden(name)
    scrambled = np.array(g["nodes"], copy=True)
    scrambled["min"] = 7.0; scrambled["max"] = -7.0              # nothing of the stored boxes may survive into the result ...
    if len(scrambled) > 1:
        scrambled[1] = g["nodes"][1]                             # ... except the reserved slot, which a refit never touches
    assert fields_equal(refit_reference(g["vertices"], g["indices_out"], scrambled), g["nodes"])


def test_key_order_and_nan_rules():
    f = np.array([-np.inf, -1e30, -1.0, -0.0, 0.0, 1e-45, 1.0, 3e30, np.inf], dtype=np.float32)
    k = key(f)
    assert (np.diff(k) > 0).all() and unkey(k).tobytes() == f.tobytes()
    v = np.array([[np.nan, 1.0, -0.0], [2.0, np.nan, 0.0]], dtype=np.float32)
    lo, hi = mesh_bounds_reference(v)
    assert lo.tobytes() == np.array([2.0, 1.0, -0.0], dtype=np.float32).tobytes()
    assert hi.tobytes() == np.array([2.0, 1.0, 0.0], dtype=np.float32).tobytes()
    lo, hi = mesh_bounds_reference(np.full((2, 3), np.nan, dtype=np.float32))
    assert (lo == np.inf).all() and (hi == -np.inf).all()
