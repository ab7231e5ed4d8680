"""The fp16 / bf16 gather modes without a GPU: the four entry points are declared, exported and bound, the ABI revision
did not move (functions were added, no struct changed), and a NULL handle is refused before any device call."""
import numpy as np

NAMES = ("bsmr_spmm_mode", "bsmr_sddmm_backward_mode", "bsmr_spmm_lowp", "bsmr_backward_reserve_mode")


def test_symbols_are_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    decl = declared_functions(INCLUDE / "bsmr_hip.h")
    exp = exported(LIB / "libbsmr_hip.so")
    for name in NAMES:
        assert name in decl and name in engine.HIP_SYMBOLS and name in exp, name
    assert engine.hip().bsmr_abi_revision() == 5   # four functions added, no layout changed


def test_null_handle_is_refused_without_a_device(engine):
    hip, bad = engine.hip(), engine.ERR_INVALID_ARG
    for mode in (engine.COMPUTE_F16, engine.COMPUTE_BF16, engine.COMPUTE_F32, 7):
        assert hip.bsmr_spmm_mode(None, 32, 0, 16, 16, 16, 1, mode, None) == bad
        assert hip.bsmr_spmm_mode(None, 32, 0, 16, 16, 16, 0, mode, None) == bad       # num_batches 0 is no excuse
        assert hip.bsmr_sddmm_backward_mode(None, 32, 16, 16, 16, 16, 16, 1, mode, None) == bad
        assert hip.bsmr_spmm_lowp(None, 32, 1, 16, 16, 16, 1, mode, None) == bad
        assert hip.bsmr_backward_reserve_mode(None, 32, 1, mode) == bad
    # the handle is looked at first: a bad K on a NULL handle is still INVALID_ARG, as for bsmr_spmm
    assert hip.bsmr_spmm(None, 48, 0, 16, 16, 16, 1, None) == bad
    assert hip.bsmr_spmm_mode(None, 48, 0, 16, 16, 16, 1, 0, None) == bad
    for call in (lambda: engine.spmm(None, 32, False, 16, 16, 16, mode=engine.COMPUTE_F16),
                 lambda: engine.spmm_lowp(None, 32, False, 16, 16, 16, mode=engine.COMPUTE_BF16),
                 lambda: engine.sddmm_backward(None, 32, 16, 16, 16, 16, 16, mode=engine.COMPUTE_BF16),
                 lambda: engine.backward_reserve(None, 32, 1, mode=engine.COMPUTE_F16)):
        with np.testing.assert_raises(engine.BsmrError):
            call()


def test_headers_still_compile_as_c(tmp_path):
    from test_capi import test_headers_compile_as_c

    test_headers_compile_as_c(tmp_path)
