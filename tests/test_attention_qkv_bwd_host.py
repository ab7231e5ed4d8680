"""One-pass backward of sparse attention without a GPU (include/bsmr_hip.h "One-pass backward of sparse attention",
DESIGN.md 21): the two entry points are declared, exported and bound, and a NULL handle is refused before anything else is
looked at."""
import pytest

NAMES = ("bsmr_sparse_attention_qkv_backward_16", "bsmr_sparse_attention_qkv_backward_reserve")


def test_symbols_are_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    decl, exp = declared_functions(INCLUDE / "bsmr_hip.h"), exported(LIB / "libbsmr_hip.so")
    for name in NAMES:
        assert name in decl and name in engine.HIP_SYMBOLS and name in exp, name
        assert callable(getattr(engine, name[len("bsmr_"):])), name
    assert engine.hip().bsmr_abi_revision() == 5   # two functions added, no layout changed


@pytest.mark.parametrize("K,Kv", ((32, 32), (48, 32), (32, 288), (256, 256)))
@pytest.mark.parametrize("nb", (1, 0))
def test_null_handle_is_refused_without_a_device(engine, nb, K, Kv):
    hip, p = engine.hip(), 16
    assert hip.bsmr_sparse_attention_qkv_backward_16(None, K, Kv, 1.0, *[p] * 10, nb, 0, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_sparse_attention_qkv_backward_reserve(None, K, Kv, nb) == engine.ERR_INVALID_ARG
