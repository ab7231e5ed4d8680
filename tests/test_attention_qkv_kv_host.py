"""One-pass sparse attention on fp8, MXFP8 and MXFP4 keys and values without a GPU (include/bsmr_hip.h): the
three entry points are declared, exported and bound, and the argument checks that need no device answer as their siblings
do - a NULL handle or a non-finite scale first, then K and Kv, then compute_mode and fp8_format - before the handle is
looked into.  As in tests/test_fp4_mx_host.py the K and mode cases hand the calls a block of zeroed host memory as handle."""
import ctypes as C

import pytest

from test_fp8_host import MODES

NAMES = ("bsmr_sparse_attention_qkv_kv8", "bsmr_sparse_attention_qkv_kv8_mx", "bsmr_sparse_attention_qkv_kv4_mx")


def _calls(hip):
    """(name, call(handle, K, Kv, scale, nb, mode, fmt)) with every pointer 16; the fp4 entry takes no fmt"""
    p = 16
    return (("kv8", lambda h, K, Kv, sc, nb, mode, fmt:
             hip.bsmr_sparse_attention_qkv_kv8(h, K, Kv, sc, p, p, p, p, p, p, nb, mode, fmt, None)),
            ("kv8_mx", lambda h, K, Kv, sc, nb, mode, fmt:
             hip.bsmr_sparse_attention_qkv_kv8_mx(h, K, Kv, sc, p, p, 1, p, 1, p, p, p, nb, mode, fmt, None)),
            ("kv4_mx", lambda h, K, Kv, sc, nb, mode, fmt:
             hip.bsmr_sparse_attention_qkv_kv4_mx(h, K, Kv, sc, p, p, 1, p, 1, p, p, p, nb, mode, None)))


def test_symbols_are_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    decl, exp = declared_functions(INCLUDE / "bsmr_hip.h"), exported(LIB / "libbsmr_hip.so")
    for name in NAMES:
        assert name in decl and name in engine.HIP_SYMBOLS and name in exp, name
        assert callable(getattr(engine, name[len("bsmr_"):])), name
    assert "One-pass sparse attention on fp8, MXFP8 and MXFP4 keys and values" in (INCLUDE / "bsmr_hip.h").read_text()
    assert engine.hip().bsmr_abi_revision() == 5   # three functions added, no layout changed


@pytest.mark.parametrize("nb", (1, 0))
def test_null_handle_is_refused_without_a_device(engine, nb):
    for name, call in _calls(engine.hip()):
        for K, Kv in ((32, 32), (48, 32), (32, 544)):   # the handle is looked at first: a bad K is still INVALID_ARG
            assert call(None, K, Kv, 1.0, nb, 0, 0) == engine.ERR_INVALID_ARG, (name, K, Kv)


def test_dims_modes_and_formats_are_judged_before_the_handle_is_read(engine):
    blank = C.create_string_buffer(1 << 16)   # zeroed host memory, never a real handle
    h = C.addressof(blank)
    for name, call in _calls(engine.hip()):
        for bad in (0, 16, 48, 544, 1024):
            for mode in MODES:   # K and Kv come before the mode
                assert call(h, bad, 64, 1.0, 1, mode, 0) == engine.ERR_UNSUPPORTED_K, (name, bad, mode)
                assert call(h, 64, bad, 1.0, 1, mode, 0) == engine.ERR_UNSUPPORTED_K, (name, bad, mode)
        for mode in MODES[2:]:
            assert call(h, 64, 512, 1.0, 1, mode, 0) == engine.ERR_INVALID_ARG, (name, mode)
        if name != "kv4_mx":
            for fmt in (2, -1, 7):
                assert call(h, 64, 64, 1.0, 1, 0, fmt) == engine.ERR_INVALID_ARG, (name, fmt)
        for scale in (float("nan"), float("inf")):   # with the handle, before K
            assert call(h, 48, 64, scale, 1, 0, 0) == engine.ERR_INVALID_ARG, (name, scale)
        for mode in (0, 1):   # a batch count of 0 is a no-op behind the checks
            assert call(h, 512, 32, 1.0, 0, mode, 1) == engine.OK, (name, mode)
            assert call(h, 512, 32, 1.0, 65536, mode, 1) == engine.ERR_INVALID_ARG, (name, mode)
    assert bytes(blank) == bytes(1 << 16)
