"""Asynchronous step of box-delivery / area-clearing: the C ABI surface and the Python surface, without a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("bp_bd_step_async", "bp_bd_async_drain", "bp_bd_async_open")


def _library():
    from benchpush_amd import _lib
    from benchpush_amd.build import build_hip
    build_hip()  # hipcc cross-compiles gfx950 without a GPU
    return _lib, _lib.load()


def test_header_declares_the_three_calls_with_their_arguments():
    header = open(os.path.join(ROOT, "include", "benchpush_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert ("int bp_bd_step_async(bp_handle *h, const double *actions, int32_t budget, uint8_t *obs, double *reward, uint8_t *terminated, "
            "uint8_t *truncated, double *info, uint8_t *ready, int32_t *slices, void *stream);") in flat
    assert ("int bp_bd_async_drain(bp_handle *h, uint8_t *obs, double *reward, uint8_t *terminated, uint8_t *truncated, double *info, "
            "uint8_t *ready, int32_t *slices, void *stream);") in flat
    assert "int32_t bp_bd_async_open(bp_handle *h);" in flat


def test_library_exports_them_and_exports_lists_them():
    _lib, L = _library()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)


def test_abi_version_is_still_11():
    _, L = _library()
    assert L.bp_abi_version() == 11


def test_null_handle_is_einval():
    _, L = _library()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert L.bp_bd_step_async(None, p, 100, p, p, p, p, p, p, p, None) == -1
    assert L.bp_bd_async_drain(None, p, p, p, p, p, p, p, None) == -1
    assert L.bp_bd_async_open(None) == 0


def test_both_batched_classes_have_the_calls():
    from benchpush_amd.envs.area_clearing import BatchedAreaClearingEnv
    from benchpush_amd.envs.box_delivery import BatchedBoxDeliveryEnv
    from benchpush_amd.envs.ship_ice import BatchedShipIceEnv
    for cls in (BatchedBoxDeliveryEnv, BatchedAreaClearingEnv):
        for name in ("step_async", "drain"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
        for name in ("async_open", "slices"):
            assert isinstance(getattr(cls, name), property), (cls.__name__, name)
    # the steps of ship-ice and maze have a fixed length: nothing to slice
    assert not hasattr(BatchedShipIceEnv, "step_async") and not hasattr(BatchedShipIceEnv, "drain")
