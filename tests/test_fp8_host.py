"""bsmr_widen_fp8 / bsmr_sddmm_b8 / bsmr_spmm_x8 / bsmr_sparse_attention_x8 without a GPU (include/bsmr_hip.h "fp8 keys and
values"): the four entry points are declared, exported and bound, the ABI revision did not move, the headers are still
C99, and the argument checks that need no device answer as documented - a NULL plan / handle first, then K, then
compute_mode and fp8_format - before the plan or handle is looked into.

As in tests/test_io16_host.py, the K and mode cases hand the calls a block of zeroed host memory as "handle": those checks
come before the handle is read, and a call that did read it would find an all-zero object, not a wild pointer."""
import ctypes as C

import numpy as np

NAMES = ("bsmr_widen_fp8", "bsmr_sddmm_b8", "bsmr_spmm_x8", "bsmr_sparse_attention_x8")
MODES = (0, 1, 2, 3, -1, 7)          # F16, BF16, then everything the fp8 calls refuse (F32 among them)
FORMATS = (0, 1, 2, -1)


def test_symbols_are_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    decl = declared_functions(INCLUDE / "bsmr_hip.h")
    exp = exported(LIB / "libbsmr_hip.so")
    for name in NAMES:
        assert name in decl and name in engine.HIP_SYMBOLS and name in exp, name
    for name in ("widen_fp8", "sddmm_b8", "spmm_x8", "sparse_attention_x8"):
        assert callable(getattr(engine, name)), name
    assert (engine.FP8_E4M3, engine.FP8_E5M2) == (0, 1)
    header = (INCLUDE / "bsmr_hip.h").read_text()
    assert "#define BSMR_FP8_E4M3 0" in header and "#define BSMR_FP8_E5M2 1" in header
    assert engine.hip().bsmr_abi_revision() == 5   # four functions added, no layout changed


def test_headers_still_compile_as_c(tmp_path):
    from test_capi import test_headers_compile_as_c

    test_headers_compile_as_c(tmp_path)


def test_null_handle_is_refused_without_a_device(engine):
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    for mode in MODES:
        for fmt in FORMATS:
            for nb in (1, 0):                                                # num_batches 0 is no excuse
                assert hip.bsmr_sddmm_b8(None, 32, 16, 16, 16, nb, mode, fmt, None) == bad
                assert hip.bsmr_spmm_x8(None, 32, 0, 16, 16, 16, nb, mode, fmt, None) == bad
                assert hip.bsmr_sparse_attention_x8(None, 32, 1.0, 16, 16, 16, 16, 16, nb, mode, fmt, None) == bad
    # the handle is looked at first: a bad K on a NULL handle is still INVALID_ARG
    assert hip.bsmr_sddmm_b8(None, 48, 16, 16, 16, 1, 0, 0, None) == bad
    assert hip.bsmr_spmm_x8(None, 48, 0, 16, 16, 16, 1, 0, 0, None) == bad
    assert hip.bsmr_sparse_attention_x8(None, 48, 1.0, 16, 16, 16, 16, 16, 1, 0, 0, None) == bad


def test_k_and_modes_are_judged_before_the_handle_is_read(engine):
    hip = engine.hip()
    blank = C.create_string_buffer(1 << 16)                                  # zeroed host memory, never a real handle
    h = C.addressof(blank)
    for K in (48, 0, 16, 33):
        for mode in MODES:
            for fmt in FORMATS:                                              # K comes before both modes
                assert hip.bsmr_sddmm_b8(h, K, 16, 16, 16, 1, mode, fmt, None) == engine.ERR_UNSUPPORTED_K
                assert hip.bsmr_spmm_x8(h, K, 0, 16, 16, 16, 1, mode, fmt, None) == engine.ERR_UNSUPPORTED_K
                assert hip.bsmr_sparse_attention_x8(h, K, 1.0, 16, 16, 16, 16, 16, 1, mode, fmt, None) == engine.ERR_UNSUPPORTED_K
    for mode in MODES:
        for fmt in FORMATS:
            if mode in (0, 1) and fmt in (0, 1):
                continue
            assert hip.bsmr_sddmm_b8(h, 32, 16, 16, 16, 1, mode, fmt, None) == engine.ERR_INVALID_ARG
            assert hip.bsmr_spmm_x8(h, 32, 0, 16, 16, 16, 1, mode, fmt, None) == engine.ERR_INVALID_ARG
            assert hip.bsmr_sparse_attention_x8(h, 32, 1.0, 16, 16, 16, 16, 16, 1, mode, fmt, None) == engine.ERR_INVALID_ARG
    for scale in (float("nan"), float("inf")):                               # with the handle, before K
        assert hip.bsmr_sparse_attention_x8(h, 48, scale, 16, 16, 16, 16, 16, 1, 0, 0, None) == engine.ERR_INVALID_ARG
    assert bytes(blank) == bytes(1 << 16)


def test_widen_follows_the_rule_of_memcpy(engine):
    """count 0 is a no-op whatever the pointers; count > 0 needs both, 16-byte aligned; the modes come first"""
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    assert hip.bsmr_memcpy_h2d(None, None, 0) == engine.OK and hip.bsmr_memcpy_h2d(None, None, 8) == bad
    for mode in (0, 1):
        for fmt in (0, 1):
            assert hip.bsmr_widen_fp8(None, None, 0, mode, fmt, None) == engine.OK
            assert hip.bsmr_widen_fp8(8, 2, 0, mode, fmt, None) == engine.OK
            for src, dst in ((None, None), (None, 4096), (4096, None), (4096 + 8, 4096), (4096, 4096 + 8)):
                assert hip.bsmr_widen_fp8(src, dst, 256, mode, fmt, None) == bad
    for mode in MODES:
        for fmt in FORMATS:
            if not (mode in (0, 1) and fmt in (0, 1)):
                assert hip.bsmr_widen_fp8(None, None, 0, mode, fmt, None) == bad


def test_python_wrappers_raise(engine):
    for call in (lambda: engine.widen_fp8(None, None, 16),
                 lambda: engine.widen_fp8(None, None, 0, mode=engine.COMPUTE_F32),
                 lambda: engine.sddmm_b8(None, 32, 16, 16, 16, 1, engine.COMPUTE_F16, engine.FP8_E4M3),
                 lambda: engine.spmm_x8(None, 32, False, 16, 16, 16, mode=engine.COMPUTE_BF16, fmt=engine.FP8_E5M2),
                 lambda: engine.sparse_attention_x8(None, 32, 1.0, 16, 16, 16, 16, 16, mode=engine.COMPUTE_F16)):
        with np.testing.assert_raises(engine.BsmrError):
            call()
    engine.widen_fp8(None, None, 0)                                          # the no-op does not raise
