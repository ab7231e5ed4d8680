"""One-pass grouped-head sparse attention on the MFMA without a GPU (include/bsmr_hip.h "One-pass grouped-head sparse
attention on the MFMA"): the entry point is declared, exported and bound, and a NULL handle is refused before
anything else is looked at."""
import pytest

NAME = "bsmr_sparse_attention_qkv_gqa_mfma_16"


def test_symbol_is_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    assert NAME in declared_functions(INCLUDE / "bsmr_hip.h") and NAME in exported(LIB / "libbsmr_hip.so")
    assert NAME in engine.HIP_SYMBOLS and callable(engine.sparse_attention_qkv_gqa_mfma_16)
    assert engine.hip().bsmr_abi_revision() == 5   # a function added, no layout changed


@pytest.mark.parametrize("K,Kv,nb,g", ((32, 32, 8, 4), (48, 32, 8, 0), (512, 512, 0, 2), (256, 256, 6, 1)))
def test_null_handle_is_refused_without_a_device(engine, K, Kv, nb, g):
    f = engine.hip().bsmr_sparse_attention_qkv_gqa_mfma_16
    assert f(None, K, Kv, 1.0, *[16] * 6, nb, g, 0, None) == engine.ERR_INVALID_ARG
