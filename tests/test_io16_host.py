"""bsmr_sddmm_16 / bsmr_spmm_16 / bsmr_sddmm_backward_16 without a GPU: the three entry points are declared, exported and
bound, the ABI revision did not move, and the argument checks that need no device answer in the documented order - a NULL
plan / handle, then K, then compute_mode - before the plan or handle is looked into.

No plan or handle can be created without a device, so the K and compute_mode cases hand the calls a block of zeroed host
memory as "handle": the header promises that these checks come before the handle is read, and a call that did read it
would find an all-zero object (nnz = 0, no delegate), not a wild pointer."""
import ctypes as C

import numpy as np

NAMES = ("bsmr_sddmm_16", "bsmr_spmm_16", "bsmr_sddmm_backward_16")


def test_symbols_are_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    decl = declared_functions(INCLUDE / "bsmr_hip.h")
    exp = exported(LIB / "libbsmr_hip.so")
    for name in NAMES:
        assert name in decl and name in engine.HIP_SYMBOLS and name in exp, name
    for name in ("sddmm_16", "spmm_16", "sddmm_backward_16"):
        assert callable(getattr(engine, name)), name
    assert engine.hip().bsmr_abi_revision() == 5   # three functions added, no layout changed


def test_null_handle_is_refused_without_a_device(engine):
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    for mode in (engine.COMPUTE_F16, engine.COMPUTE_BF16, engine.COMPUTE_F32, 7):
        for nb in (1, 0):                                                    # num_batches 0 is no excuse
            assert hip.bsmr_sddmm_16(None, 32, 16, 16, 16, nb, mode, None) == bad
            assert hip.bsmr_spmm_16(None, 32, 0, 16, 16, 16, nb, mode, None) == bad
            assert hip.bsmr_sddmm_backward_16(None, 32, 16, 16, 16, 16, 16, nb, mode, None) == bad
    # the handle is looked at first: a bad K on a NULL handle is still INVALID_ARG, as for bsmr_spmm
    assert hip.bsmr_sddmm_16(None, 48, 16, 16, 16, 1, 0, None) == bad
    assert hip.bsmr_spmm_16(None, 48, 0, 16, 16, 16, 1, 0, None) == bad
    assert hip.bsmr_sddmm_backward_16(None, 48, 16, 16, 16, 16, 16, 1, 0, None) == bad
    for call in (lambda: engine.sddmm_16(None, 32, 16, 16, 16, 1, engine.COMPUTE_F16),
                 lambda: engine.spmm_16(None, 32, False, 16, 16, 16, mode=engine.COMPUTE_BF16),
                 lambda: engine.sddmm_backward_16(None, 32, 16, 16, 16, 16, 16, mode=engine.COMPUTE_F16)):
        with np.testing.assert_raises(engine.BsmrError):
            call()


def test_k_and_mode_are_judged_before_the_handle_is_read(engine):
    hip = engine.hip()
    blank = C.create_string_buffer(1 << 16)                                  # zeroed host memory, never a real handle
    h = C.addressof(blank)
    for K in (48, 0, 16, 33):
        for mode in (0, 1, 2):
            assert hip.bsmr_sddmm_16(h, K, 16, 16, 16, 1, mode, None) == engine.ERR_UNSUPPORTED_K
            assert hip.bsmr_spmm_16(h, K, 0, 16, 16, 16, 1, mode, None) == engine.ERR_UNSUPPORTED_K
            assert hip.bsmr_sddmm_backward_16(h, K, 16, 16, 16, 16, 16, 1, mode, None) == engine.ERR_UNSUPPORTED_K
    for mode in (engine.COMPUTE_F32, -1, 3):                                 # compute_mode = 2: the fp32 calls exist already
        assert hip.bsmr_sddmm_16(h, 32, 16, 16, 16, 1, mode, None) == engine.ERR_INVALID_ARG
        assert hip.bsmr_spmm_16(h, 32, 0, 16, 16, 16, 1, mode, None) == engine.ERR_INVALID_ARG
        assert hip.bsmr_sddmm_backward_16(h, 32, 16, 16, 16, 16, 16, 1, mode, None) == engine.ERR_INVALID_ARG
    assert bytes(blank) == bytes(1 << 16)


def test_headers_still_compile_as_c(tmp_path):
    from test_capi import test_headers_compile_as_c

    test_headers_compile_as_c(tmp_path)
