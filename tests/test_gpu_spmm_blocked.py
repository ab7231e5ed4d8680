"""The blocked SpMM on the device (include/bsmr_hip.h "Blocked SpMM"): bsmr_spmm_blocked[_16] bit for
bit against tests/blocked_twin.py - the block chains of the fp32 MFMA, the residue gather and their one addition - on the
pattern whose properties tests/test_spmm_blocked_host.py asserts (panels with 0 - 5 blocks, empty cells, a padding column,
a residue row of three chunks, empty rows, a ragged last panel), and through bsmr_torch.SparseOperator(blocked=True)."""
import ctypes as C

import numpy as np
import pytest

import blocked_twin as bt
from gather_twin import assert_twin, col_lists, gather, row_lists
from guarded import OPERAND, VALUES, Guarded, check_all

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = (32, 96, 256, 512)      # below one 64-feature group, not a multiple of 64, several groups
FORMS = ("fp32", "fp16", "bf16")
U16 = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}


def _dev():
    return torch.device("cuda:0")


def _dtype(form):
    return {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[form]


def _mode(engine, form):
    return {"fp32": engine.COMPUTE_F32, "fp16": engine.COMPUTE_F16, "bf16": engine.COMPUTE_BF16}[form]


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _round(a, form):
    """fp32 numpy -> the values of `form`, widened back to fp32 (round to nearest even, the casts of the kernels)"""
    if form == "fp32":
        return np.ascontiguousarray(a, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dtype(form)).float().numpy()


class Case:
    def __init__(self, engine, oracle, M, N, ro, ci, delta=0.3):
        self.engine, self.M, self.N, self.ro, self.ci, self.nnz = engine, M, N, ro, ci, int(ci.size)
        csr = engine.CSR.from_arrays(M, N, ro, ci)
        self.arrays = engine.Pipeline(csr, alpha=0.3, delta=delta, device=-1).arrays()
        self.bw = engine.backward_create(M, N, ro, ci, row_order=self.arrays["reorderedRows"], device=0)
        engine.backward_attach_blocks(self.bw, M, N, self.nnz, self.arrays)
        self.twin = bt.BlockedTwin(oracle, M, N, ro, ci, self.arrays)

    def close(self):
        self.engine.backward_destroy(self.bw)

    def run(self, K, v, X, form="fp32", nb=1, stream=None):
        """the device result widened to fp32 numpy; v (nb, nnz) or (nnz,), X values already representable in `form`"""
        lead = (nb,) if nb > 1 else ()
        tv = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(_dev())
        tX = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(_dev()).to(_dtype(form))
        tY = torch.full(lead + (self.M, K), float("nan"), dtype=_dtype(form), device=_dev())   # every element is written
        torch.cuda.synchronize()
        self.engine.spmm_blocked(self.bw, K, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), nb,
                                 _stream() if stream is None else stream, mode=_mode(self.engine, form))
        torch.cuda.synchronize()
        return tY.float().cpu().numpy()

    def gather(self, K, v, X):
        """bsmr_spmm (the plain gather) on the same handle"""
        tv = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(_dev())
        tX = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(_dev())
        tY = torch.full((self.M, K), float("nan"), dtype=torch.float32, device=_dev())
        self.engine.spmm(self.bw, K, False, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), 1, _stream())
        torch.cuda.synchronize()
        return tY.cpu().numpy()


@pytest.fixture(scope="module")
def case(engine, oracle):
    c = Case(engine, oracle, *bt.blocked_pattern())
    s = engine.backward_blocked_stats(c.bw)
    # the properties the cases below rely on (tests/test_spmm_blocked_host.py asserts them in full)
    assert s["panels_with_blocks"] < s["panels"] and s["max_blocks_per_panel"] >= 4 and s["padding_columns"] > 0
    assert s["split_residue_rows"] >= 1 and c.arrays["reorderedRows"].size < c.M and c.arrays["reorderedRows"].size % 16
    assert s["device_index_bytes"] > 1024 * s["blocks"]
    yield c
    c.close()


@pytest.fixture(scope="module")
def no_blocks(engine, oracle):
    c = Case(engine, oracle, *bt.blocked_pattern(), delta=1.0)
    assert engine.backward_blocked_stats(c.bw)["blocks"] == 0
    yield c
    c.close()


def _normal(seed, nnz, N, K, form="fp32"):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(nnz).astype(np.float32), _round(rng.standard_normal((N, K)), form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", KS)
def test_bit_for_bit_against_the_twin(case, K, form):
    v, X = _normal(K, case.nnz, case.N, K, form)
    got = case.run(K, v, X, form)
    assert_twin(got, _round(case.twin.twin(v, X), form), f"K={K} {form}")


def test_twin_differs_from_the_plain_gather(case, oracle):
    """what makes the test above a test of the blocked path: on normal data the two contracts disagree in many elements"""
    v, X = _normal(1, case.nnz, case.N, 64)
    a, b = case.twin.twin(v, X), gather(oracle, row_lists(case.ro, case.ci), v, X)
    assert (a.view(np.uint32) != b.view(np.uint32)).mean() > 0.2


@pytest.mark.parametrize("K", (32, 96))
def test_exact_integers_equal_the_gather(case, K):
    rng = np.random.default_rng(7)
    v = rng.integers(-7, 8, case.nnz).astype(np.float32)
    X = rng.integers(-15, 16, (case.N, K)).astype(np.float32)
    got, want = case.run(K, v, X), case.gather(K, v, X)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(got, case.twin.fp64(v, X)[0].astype(np.float32))


@pytest.mark.parametrize("form", FORMS)
def test_non_finite_operands(case, form):
    """+inf and NaN in rows of X that are block columns: the rows that store them behave as in the gather, the rows of the
    same panel with an EMPTY cell there get NaN (0 * inf), every other row keeps the bits of the clean run"""
    K = 96
    v, X = _normal(11, case.nnz, case.N, K, form)
    clean = case.run(K, v, X, form)
    dc = case.arrays["denseCols"].reshape(-1, 16)
    bv = case.arrays["blockValues"].reshape(-1, 16, 16)
    bo = case.arrays["blockOffsets"].astype(np.int64)
    rr = case.arrays["reorderedRows"]
    # two block columns of different panels, each with an empty cell in a row that exists
    picks = []
    for p in range(bo.size - 1):
        rows_here = min(16, rr.size - 16 * p)
        for b in range(bo[p], bo[p + 1]):
            js = [j for j in range(16) if dc[b, j] != case.N and (bv[b, :rows_here, j] == bt.NULL).any()
                  and (bv[b, :rows_here, j] != bt.NULL).any()]
            if js:
                picks.append((p, int(dc[b, js[0]])))
                break
    assert len(picks) >= 2
    (p1, c1), (p2, c2) = picks[0], picks[-1]
    assert p1 != p2
    Xb = X.copy()
    Xb[c1, 5], Xb[c2, 70] = np.inf, np.nan
    got = case.run(K, v, Xb, form)
    want = _round(case.twin.twin(v, Xb), form)
    assert_twin(got, want, form)
    row_of = np.repeat(np.arange(case.M), np.diff(case.ro.astype(np.int64)))
    for p, c, k in ((p1, c1, 5), (p2, c2, 70)):
        panel_rows = rr[16 * p:16 * p + 16]
        storing = np.unique(row_of[case.ci == c])
        empty_cell_rows = np.setdiff1d(panel_rows, storing)
        assert empty_cell_rows.size and np.isnan(got[empty_cell_rows, k]).all()          # the semantic difference
        holders = [q for q in range(bo.size - 1) if (dc[bo[q]:bo[q + 1]] == c).any()]
        touched = np.union1d(storing, np.concatenate([rr[16 * q:16 * q + 16] for q in holders]))
        others = np.setdiff1d(np.arange(case.M), touched)
        assert others.size and got[others, k].tobytes() == clean[others, k].tobytes()
    k_clean = np.setdiff1d(np.arange(K), [5, 70])
    assert got[:, k_clean].tobytes() == clean[:, k_clean].tobytes()


def test_zeros(case):
    K = 32
    v, X = _normal(13, case.nnz, case.N, K)
    v[::3] = -0.0
    X[::5, ::2] = -0.0
    assert_twin(case.run(K, v, X), case.twin.twin(v, X), "-0 operands")
    got = case.run(K, np.zeros(case.nnz, np.float32), -np.abs(X))
    assert not got.view(np.uint32).any()                                                # +0 everywhere, never -0


@pytest.mark.parametrize("form", ("fp32", "bf16"))
def test_batches_equal_single_calls(case, form):
    K, nb = 96, 3
    rng = np.random.default_rng(17)
    v = rng.standard_normal((nb, case.nnz)).astype(np.float32)
    X = _round(rng.standard_normal((nb, case.N, K)), form)
    got = case.run(K, v, X, form, nb=nb)
    for b in range(nb):
        assert got[b].tobytes() == case.run(K, v[b], X[b], form).tobytes(), b
    assert_twin(got[2], _round(case.twin.twin(v[2], X[2]), form), "batch 2")


def test_reproducible_call_to_call_and_stream_to_stream(case):
    K = 256
    v, X = _normal(19, case.nnz, case.N, K)
    first = case.run(K, v, X)
    assert case.run(K, v, X).tobytes() == first.tobytes()
    side = torch.cuda.Stream(device=_dev())
    assert case.run(K, v, X, stream=side.cuda_stream).tobytes() == first.tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_handle_without_blocks_gives_the_gather_bits(no_blocks, engine, form):
    K = 96
    c = no_blocks
    v, X = _normal(23, c.nnz, c.N, K, form)
    got = c.run(K, v, X, form)
    if form == "fp32":
        want = c.gather(K, v, X)
    else:
        tv = torch.from_numpy(v).to(_dev())
        tX = torch.from_numpy(X).to(_dev()).to(_dtype(form))
        tY = torch.empty((c.M, K), dtype=_dtype(form), device=_dev())
        engine.spmm_16(c.bw, K, False, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), 1, _stream(), mode=_mode(engine, form))
        torch.cuda.synchronize()
        want = tY.float().cpu().numpy()
    assert got.tobytes() == want.tobytes()


def test_edge_handles(engine, case):
    K = 64
    hip = engine.hip()
    # nnz = 0: zeros, NULL inputs allowed
    M, N = 40, 50
    ro = np.zeros(M + 1, dtype=np.uint32)
    empty = np.zeros(0, dtype=np.uint32)
    arrays = {k: empty for k in ("reorderedRows", "denseCols", "blockValues", "sparseValues", "sparseRelativeRows",
                                 "sparseColIndices")}
    arrays["blockOffsets"] = arrays["sparseValueOffsets"] = np.zeros(1, dtype=np.uint32)
    bw = engine.backward_create(M, N, ro, empty, device=0)
    try:
        tY = torch.full((M, K), float("nan"), device=_dev())
        # not attached yet
        assert hip.bsmr_spmm_blocked(bw, K, None, None, tY.data_ptr(), 1, None) == engine.ERR_BAD_PLAN
        assert hip.bsmr_spmm_blocked_16(bw, K, None, None, tY.data_ptr(), 1, engine.COMPUTE_F16, None) == engine.ERR_BAD_PLAN
        s = engine.BlockedStats()
        assert hip.bsmr_backward_get_blocked_stats(bw, C.byref(s), C.sizeof(s)) == engine.ERR_BAD_PLAN
        engine.backward_attach_blocks(bw, M, N, 0, arrays)
        assert engine.backward_attach_blocks_status(bw, M, N, 0, arrays) == engine.ERR_INVALID_ARG   # a second attach
        engine.spmm_blocked(bw, K, 0, 0, tY.data_ptr(), 1, _stream())
        t16 = torch.full((M, K), float("nan"), dtype=torch.float16, device=_dev())
        engine.spmm_blocked(bw, K, 0, 0, t16.data_ptr(), 1, _stream(), mode=engine.COMPUTE_F16)
        torch.cuda.synchronize()
        assert not tY.cpu().numpy().view(np.uint32).any() and not t16.cpu().numpy().view(np.uint16).any()
    finally:
        engine.backward_destroy(bw)
    # the argument rules of bsmr_spmm on a real handle
    bw = case.bw
    tv = torch.zeros(case.nnz, device=_dev())
    tX = torch.zeros(case.N, K, device=_dev())
    tY = torch.zeros(case.M, K, device=_dev())
    v, X, Y = tv.data_ptr(), tX.data_ptr(), tY.data_ptr()
    assert hip.bsmr_spmm_blocked(bw, 48, v, X, Y, 1, None) == engine.ERR_UNSUPPORTED_K
    assert hip.bsmr_spmm_blocked(bw, 0, v, X, Y, 1, None) == engine.ERR_UNSUPPORTED_K
    assert hip.bsmr_spmm_blocked_16(bw, 48, v, X, Y, 1, engine.COMPUTE_F16, None) == engine.ERR_UNSUPPORTED_K
    assert hip.bsmr_spmm_blocked(bw, K, v, X, Y, 65536, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_spmm_blocked(bw, K, v, X, Y, 0, None) == engine.OK
    assert hip.bsmr_spmm_blocked_16(bw, K, v, X, Y, 1, engine.COMPUTE_F32, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_spmm_blocked(bw, K, None, X, Y, 1, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_spmm_blocked(bw, K, v, None, Y, 1, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_spmm_blocked(bw, K, v, X, None, 1, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_spmm_blocked(bw, K, v + 2, X, Y, 1, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_spmm_blocked(bw, K, v, X + 8, Y, 1, None) == engine.ERR_INVALID_ARG
    assert hip.bsmr_spmm_blocked(bw, K, v, X, Y + 8, 1, None) == engine.ERR_INVALID_ARG
    # a desc that is not a partition is refused by attach as by the check, and leaves the handle unattached
    bad = bt.copy_arrays(case.arrays)
    bad["sparseColIndices"][0] = (bad["sparseColIndices"][0] + 1) % case.N
    bw2 = engine.backward_create(case.M, case.N, case.ro, case.ci, device=0)
    try:
        assert engine.backward_attach_blocks_status(bw2, case.M, case.N, case.nnz, bad) == engine.ERR_BAD_PLAN
        assert hip.bsmr_spmm_blocked(bw2, K, v, X, Y, 1, None) == engine.ERR_BAD_PLAN
    finally:
        engine.backward_destroy(bw2)


@pytest.mark.parametrize("form", FORMS)
def test_guarded_buffers(case, form):
    """the weakest alignment the header allows: 16 bytes for X and Y, 4 for v; nothing written outside Y (every element of
    it written), nothing read outside v and X (a guard value read into a sum would make it NaN)"""
    K, nb = 96, 2
    rng = np.random.default_rng(29)
    v = rng.standard_normal((nb, case.nnz)).astype(np.float32)
    X = _round(rng.standard_normal((nb, case.N, K)), form)
    gv = Guarded.input("v", v, VALUES, K, _dev())
    if form == "fp32":
        gX = Guarded.input("X", X, OPERAND, K, _dev())
        gY = Guarded.output("Y", nb * case.M * K, OPERAND, K, _dev())
    else:
        bits = torch.from_numpy(X).to(_dtype(form)).view(torch.int16).numpy().view(np.uint16)
        gX = Guarded.input("X16", bits, OPERAND, K, _dev(), dtype=np.uint16)
        gY = Guarded.output("Y16", nb * case.M * K, OPERAND, K, _dev(), dtype=np.uint16)
    case.engine.spmm_blocked(case.bw, K, gv.ptr, gX.ptr, gY.ptr, nb, _stream(), mode=_mode(case.engine, form))
    torch.cuda.synchronize()
    check_all(gv, gX, gY)
    if form == "fp32":
        got = gY.numpy().reshape(nb, case.M, K)
    else:
        got = torch.from_numpy(gY.numpy().view(np.int16).copy()).view(_dtype(form)).float().numpy().reshape(nb, case.M, K)
    for b in range(nb):
        assert_twin(got[b], _round(case.twin.twin(v[b], X[b]), form), f"guarded {form} batch {b}")


@pytest.mark.parametrize("form", FORMS)
def test_reserve_covers_the_calls(engine, oracle, form):
    K, nb = 128, 3
    c = Case(engine, oracle, *bt.blocked_pattern())
    try:
        engine.backward_reserve(c.bw, K, nb)
        before = engine.backward_stats(c.bw)["workspace_bytes"]
        assert before > 0
        rng = np.random.default_rng(31)
        v = rng.standard_normal((nb, c.nnz)).astype(np.float32)
        X = _round(rng.standard_normal((nb, c.N, K)), form)
        got = c.run(K, v, X, form, nb=nb)
        assert engine.backward_stats(c.bw)["workspace_bytes"] == before
        assert_twin(got[1], _round(c.twin.twin(v[1], X[1]), form), "after reserve")
    finally:
        c.close()


def test_error_against_fp64(case):
    worst = 0.0
    for K in (32, 256):
        v, X = _normal(37 + K, case.nnz, case.N, K)
        got = case.run(K, v, X).astype(np.float64)
        Y64, bound = case.twin.fp64(v, X)
        ratio = float((np.abs(got - Y64) / np.where(bound > 0, bound, 1.0)).max())
        worst = max(worst, ratio)
        assert (np.abs(got - Y64) <= bound).all(), ratio
    print(f"blocked SpMM: worst |Y - Y64| / bound = {worst:.3f}")


# ---- torch: SparseOperator(blocked=True) -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops(engine, oracle):
    import bsmr_torch
    M, N, ro, ci = bt.blocked_pattern()
    csr = engine.CSR.from_arrays(M, N, ro, ci)
    blocked = bsmr_torch.SparseOperator(csr, mode=engine.COMPUTE_F32, device=0, blocked=True)
    plain = bsmr_torch.SparseOperator(csr, mode=engine.COMPUTE_F32, device=0)
    off = bsmr_torch.SparseOperator(csr, mode=engine.COMPUTE_F32, device=0, blocked=False)
    twin = bt.BlockedTwin(oracle, M, N, ro, ci, blocked.pipeline.arrays())
    return {"blocked": blocked, "plain": plain, "off": off, "twin": twin, "ro": ro, "ci": ci,
            "cl": col_lists(M, N, ro, ci), "rl": row_lists(ro, ci)}


def _leaf(shape, seed, form):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).to(_dev()).to(_dtype(form)).requires_grad_(True)


def _np(t):
    return t.detach().float().cpu().numpy()


@pytest.mark.parametrize("form", ("fp32", "bf16"))
def test_torch_spmm_forward_and_gradients(engine, oracle, ops, form):
    K = 96
    op, tw = ops["blocked"], ops["twin"]
    v = _leaf((op.nnz,), 41, "fp32")
    X = _leaf((op.N, K), 42, form)
    H = _leaf((op.M, K), 43, form).detach()
    Y = op.spmm(v, X)
    raw = torch.empty_like(Y)
    engine.spmm_blocked(op._bw, K, v.data_ptr(), X.data_ptr(), raw.data_ptr(), 1, _stream(), mode=_mode(engine, form))
    torch.cuda.synchronize()
    assert _np(Y).tobytes() == _np(raw).tobytes()
    assert_twin(_np(Y), _round(tw.twin(_np(v), _np(X)), form), "spmm forward")
    (Y.float() * H.float()).sum().backward()
    # dX = S_v^T dY: the column direction, still the gather
    assert_twin(_np(X.grad), _round(gather(oracle, ops["cl"], _np(v), _np(H)), form), "dX")
    # d values = sddmm(dY, X), the forward's kernels: the bits of an operator without blocks
    v2, X2 = v.detach().clone().requires_grad_(True), X.detach().clone().requires_grad_(True)
    (ops["plain"].spmm(v2, X2).float() * H.float()).sum().backward()
    assert _np(v.grad).tobytes() == _np(v2.grad).tobytes()
    assert _np(X.grad).tobytes() == _np(X2.grad).tobytes()


@pytest.mark.parametrize("form", ("fp32", "bf16"))
@pytest.mark.parametrize("batch", (None, 2))
def test_torch_sddmm_gradients(oracle, ops, form, batch):
    K = 64
    op, tw = ops["blocked"], ops["twin"]
    lead = () if batch is None else (batch,)
    A = _leaf(lead + (op.M, K), 51, form)
    B = _leaf(lead + (op.N, K), 52, form)
    G = _leaf(lead + (op.nnz,), 53, "fp32").detach()
    (op.sddmm(A, B) * G).sum().backward()
    for b in range(batch or 1):
        sel = (lambda t: _np(t)) if batch is None else (lambda t, b=b: _np(t)[b])
        assert_twin(sel(A.grad), _round(tw.twin(sel(G), sel(B)), form), f"dA batch {b}")
        assert_twin(sel(B.grad), _round(gather(oracle, ops["cl"], sel(G), sel(A)), form), f"dB batch {b}")
    # only dA wanted: the blocked call alone; only dB wanted: the gather alone
    A2, B2 = A.detach().clone().requires_grad_(True), B.detach().clone()
    (op.sddmm(A2, B2) * G).sum().backward()
    assert B2.grad is None and _np(A2.grad).tobytes() == _np(A.grad).tobytes()
    A3, B3 = A.detach().clone(), B.detach().clone().requires_grad_(True)
    (op.sddmm(A3, B3) * G).sum().backward()
    assert A3.grad is None and _np(B3.grad).tobytes() == _np(B.grad).tobytes()


@pytest.mark.parametrize("form", ("fp32", "bf16"))
def test_torch_attention_agrees_with_the_gather(ops, form):
    """the two operators share the SDDMM and the softmax bit for bit; the last spmm differs by at most the two error
    bounds added: (max(16 nb, n_r) + 4) u S for the blocked form and (n + 2) u S for the gather, S = sum|w||x|; a 16-bit
    output adds one rounding of each result, u16 (|Y_blocked| + |Y_gather|)"""
    K = 64
    op, plain, tw = ops["blocked"], ops["plain"], ops["twin"]
    Q, Kt, V = _leaf((op.M, K), 61, form), _leaf((op.N, K), 62, form), _leaf((op.N, K), 63, form)
    with torch.no_grad():
        W = op.softmax(op.sddmm(Q, Kt), K ** -0.5)
        assert _np(W).tobytes() == _np(plain.softmax(plain.sddmm(Q, Kt), K ** -0.5)).tobytes()
        Yb, Yg = _np(op.attention(Q, Kt, V)).astype(np.float64), _np(plain.attention(Q, Kt, V)).astype(np.float64)
    _, bound_b = tw.fp64(_np(W), _np(V))
    n = np.diff(ops["ro"].astype(np.int64))[:, None]
    row_of = np.repeat(np.arange(op.M), n[:, 0])
    S = np.zeros((op.M, K))
    np.add.at(S, row_of, np.abs(_np(W).astype(np.float64))[:, None] * np.abs(_np(V).astype(np.float64))[ops["ci"]])
    bound = bound_b + (n + 2) * bt.U * S
    if form != "fp32":
        bound = bound + U16[form] * (np.abs(Yb) + np.abs(Yg))
    assert (np.abs(Yb - Yg) <= bound).all(), float((np.abs(Yb - Yg) - bound).max())


def test_torch_blocked_false_is_the_default(engine, ops):
    K = 96
    plain, off = ops["plain"], ops["off"]
    assert plain.blocked is False and off.blocked is False
    outs = []
    for op in (plain, off):
        v, X = _leaf((op.nnz,), 71, "fp32"), _leaf((op.N, K), 72, "fp32")
        A, B = _leaf((op.M, K), 73, "fp32"), _leaf((op.N, K), 74, "fp32")
        Y = op.spmm(v, X)
        O = op.attention(A, B, X)
        (Y.sum() + (O * O).sum()).backward()
        outs.append([_np(t).tobytes() for t in (Y, O, v.grad, X.grad, A.grad, B.grad)])
    assert outs[0] == outs[1]
    # and the default operator's spmm is the plain gather
    v, X = _leaf((plain.nnz,), 75, "fp32").detach(), _leaf((plain.N, K), 76, "fp32").detach()
    raw = torch.empty(plain.M, K, device=_dev())
    engine.spmm(plain._bw, K, False, v.data_ptr(), X.data_ptr(), raw.data_ptr(), 1, _stream())
    assert _np(plain.spmm(v, X)).tobytes() == _np(raw).tobytes()


def test_torch_blocked_needs_the_fp32_gather_mode(engine):
    import bsmr_torch
    M, N, ro, ci = bt.blocked_pattern()
    csr = engine.CSR.from_arrays(M, N, ro, ci)
    for gm in (engine.COMPUTE_F16, engine.COMPUTE_BF16):
        with pytest.raises(ValueError):
            bsmr_torch.SparseOperator(csr, device=0, gather_mode=gm, blocked=True)
