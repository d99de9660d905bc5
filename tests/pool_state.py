"""The context's pool accounting as the tests read it (csrc/testhooks.hip pgp_test_pool_state)."""
import ctypes as C


def pool_state(lib, handle=None):
    from pygps_amd import _lib
    out = (C.c_int64 * 9)()        # [7], [8]: scratch-pool bytes / buffers that are out (taken, not yet given back)
    assert lib.pgp_test_pool_state(_lib.ctx(), handle, out) == 0
    return list(out)
