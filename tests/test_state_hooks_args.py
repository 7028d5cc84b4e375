"""CPU: the argument checks and trivial returns of the two scratch-poisoning hooks
(orbfe_debug_fill_extractor, orbfe_debug_fill_matcher) come before any device call, so they answer on a
machine without a GPU. What the hooks fill is tested on the device (tests/test_gpu_state_extractor.py,
tests/test_gpu_state_matcher.py)."""
import ctypes
import threading

from orb_slam3_ros_amd import _lib

OK, E_ARG, E_DEVICE = _lib.ORBFE_OK, _lib.ORBFE_E_ARG, _lib.ORBFE_E_DEVICE


def test_null_handle(orbfe_lib):
    n = ctypes.c_int64(-9)
    assert orbfe_lib.orbfe_debug_fill_extractor(None, 1, ctypes.byref(n)) == E_ARG
    assert n.value == 0
    assert orbfe_lib.orbfe_debug_fill_extractor(None, 1, None) == E_ARG
    assert orbfe_lib.orbfe_debug_fill_matcher(1, None) == E_ARG


def test_unused_extractor_fills_nothing(orbfe_lib):
    """A handle that has never extracted owns no buffer: ORBFE_OK, 0 bytes. Creating a handle needs a
    device (its streams); without one the create call itself says so and there is no handle to ask."""
    h = ctypes.c_void_p()
    rc = orbfe_lib.orbfe_extractor_create(500, 1.2, 8, 20, 7, ctypes.byref(h))
    if rc != OK:
        assert rc == E_DEVICE and h.value is None
        return
    try:
        for word in (0, 1):
            n = ctypes.c_int64(-9)
            assert orbfe_lib.orbfe_debug_fill_extractor(h, word, ctypes.byref(n)) == OK
            assert n.value == 0
        assert orbfe_lib.orbfe_debug_fill_extractor(h, 1, None) == OK
    finally:
        orbfe_lib.orbfe_extractor_destroy(h)


def test_thread_without_scratch_fills_nothing(orbfe_lib):
    """The matcher scratch is per thread: a thread that has made no matcher call has none."""
    got = {}

    def fresh_thread():
        out = (ctypes.c_int64 * 3)(-9, -9, -9)
        got["rc"] = orbfe_lib.orbfe_debug_fill_matcher(1, out)
        got["bytes"] = list(out)

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert got == {"rc": OK, "bytes": [0, 0, 0]}
