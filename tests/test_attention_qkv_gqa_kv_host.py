"""One-pass grouped-head sparse attention on a quantised KV cache without a GPU (include/bsmr_hip.h "One-pass grouped-head
sparse attention on fp8, MXFP8 and MXFP4 keys and values"): the three entry points are declared, exported and
bound, and a NULL handle is refused before anything else is looked at."""
import pytest

# name -> the arguments behind (bw, K, Kv, scale): pointers, then num_batches, kv_group, compute_mode[, fp8_format], stream
CALLS = {
    "bsmr_sparse_attention_qkv_gqa_kv8": ([16] * 6, (8, 4, 0, 0, None)),
    "bsmr_sparse_attention_qkv_gqa_kv8_mx": ([16] * 8, (8, 0, 0, 0, None)),
    "bsmr_sparse_attention_qkv_gqa_kv4_mx": ([16] * 8, (0, 2, 0, None)),
}


def test_symbols_are_declared_and_bound(engine):
    from test_capi import INCLUDE, LIB, declared_functions, exported

    decl, exp = declared_functions(INCLUDE / "bsmr_hip.h"), exported(LIB / "libbsmr_hip.so")
    for name in CALLS:
        assert name in decl and name in engine.HIP_SYMBOLS and name in exp, name
        assert callable(getattr(engine, name[len("bsmr_"):])), name
    assert engine.hip().bsmr_abi_revision() == 5   # functions added, no layout changed


@pytest.mark.parametrize("name", CALLS)
def test_null_handle_is_refused_without_a_device(engine, name):
    pointers, tail = CALLS[name]
    assert getattr(engine.hip(), name)(None, 512, 32, 1.0, *pointers, *tail) == engine.ERR_INVALID_ARG
