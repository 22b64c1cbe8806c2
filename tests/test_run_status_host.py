"""The run-status ABI without a GPU (include/macx.h: macx_run_status, macx_run_status_reset, macx_handoff_selftest): symbols and
their ctypes signatures, the error code and its text, argument checks that return before any HIP call, the exception class, and
where the status words sit in `saved` -- outside the 576 counter words macx_cell_begin zeroes, which stay the buffer's tail."""
import ctypes as C

import pytest


def _opts_shapes(macx, B=5, S=5, N=49, d=512, p=4):
    cfg = macx.configs.flag_file_config("args", netLength=p, memDim=d, ctrlDim=d, attDim=d)
    return macx.freeze(cfg), macx._lib.MacxShapes(B=B, S=S, N=N, d=d, p=p, b0=0, d_logical=0)


def test_symbols_and_signatures(macx):
    L = macx._lib.lib()
    P = C.POINTER
    lib = macx._lib
    assert {"macx_run_status", "macx_run_status_reset", "macx_handoff_selftest"} <= set(lib.EXPORTS)
    assert L.macx_run_status.argtypes == [P(lib.MacxOpts), P(lib.MacxShapes), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                          P(C.c_uint32), P(C.c_int32)]
    assert L.macx_run_status_reset.argtypes == [P(lib.MacxOpts), P(lib.MacxShapes), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.macx_handoff_selftest.argtypes == [C.c_void_p, P(C.c_uint32)]
    for f in (L.macx_run_status, L.macx_run_status_reset, L.macx_handoff_selftest):
        assert f.restype is C.c_int
    assert L.macx_abi_version() == 5           # additive: the version stays


def test_ewait_has_a_text_of_its_own(macx):
    lib = macx._lib
    L = lib.lib()
    assert lib.MACX_EWAIT == -5
    text = L.macx_strerror(lib.MACX_EWAIT)
    assert text and text != L.macx_strerror(-99)
    others = [L.macx_strerror(c) for c in (lib.MACX_OK, lib.MACX_EINVAL, lib.MACX_EUNSUPPORTED, lib.MACX_EREJECTED, lib.MACX_ESMALL)]
    assert text not in others


def test_bad_arguments_are_refused_before_any_launch(macx):
    lib = macx._lib
    L = lib.lib()
    o, s = _opts_shapes(macx)
    bits, first = C.c_uint32(7), C.c_int32(7)
    n = L.macx_saved_floats(C.byref(o), C.byref(s), 1)
    assert n > 0
    assert L.macx_run_status(C.byref(o), C.byref(s), 1, None, n, None, C.byref(bits), C.byref(first)) == lib.MACX_EINVAL
    assert L.macx_run_status_reset(C.byref(o), C.byref(s), 1, None, n, None) == lib.MACX_EINVAL
    assert L.macx_run_status(None, C.byref(s), 1, None, n, None, None, None) == lib.MACX_EINVAL
    assert L.macx_handoff_selftest(None, None) == lib.MACX_EINVAL
    # a buffer smaller than the layout (never dereferenced: the size check comes first)
    fake = C.c_void_p(1 << 20)
    assert L.macx_run_status(C.byref(o), C.byref(s), 1, fake, n - 1, None, C.byref(bits), C.byref(first)) == lib.MACX_ESMALL
    assert L.macx_run_status_reset(C.byref(o), C.byref(s), 1, fake, n - 1, None) == lib.MACX_ESMALL
    assert (bits.value, first.value) == (7, 7)          # nothing was written


def test_handoff_timeout_is_a_runtime_error(macx):
    assert issubclass(macx.HandoffTimeout, RuntimeError)
    e = macx.HandoffTimeout(3, 5)
    assert (e.bits, e.first_step) == (3, 5)
    assert "step 5" in str(e) and "0x3" in str(e) and "tile" in str(e) and "filler" in str(e)
    assert "tile" in str(macx.HandoffTimeout(1, 0)) and "filler" not in str(macx.HandoffTimeout(1, 0))


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("B,S,N,d,p", [(5, 5, 49, 512, 4), (8, 7, 196, 512, 3), (4, 9, 196, 128, 2)])
def test_status_words_sit_in_front_of_the_counters(macx, B, S, N, d, p, keep):
    lib = macx._lib
    L = lib.lib()
    o, s = _opts_shapes(macx, B, S, N, d, p)
    total = L.macx_saved_floats(C.byref(o), C.byref(s), keep)
    off, cnt = C.c_size_t(0), C.c_size_t(0)
    assert L.macx_saved_segment(C.byref(o), C.byref(s), keep, lib.SEG["status"], C.byref(off), C.byref(cnt)) == 0
    assert cnt.value == lib.STATUS_WORDS == 16
    # outside the last 576 words (the counters macx_cell_begin zeroes; word 63 of them is indexed from the end) and directly in front
    assert off.value + cnt.value == total - 576
    # ... and behind every viewable segment
    for name, seg in lib.SEG.items():
        if name == "status":
            continue
        o2, c2 = C.c_size_t(0), C.c_size_t(0)
        assert L.macx_saved_segment(C.byref(o), C.byref(s), keep, seg, C.byref(o2), C.byref(c2)) == 0
        assert o2.value + c2.value <= off.value
