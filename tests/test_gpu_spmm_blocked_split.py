"""The blocked SpMM with split panels on the device (include/bsmr_hip.h "Blocked SpMM", segment_blocks; DESIGN section
14): bsmr_spmm_blocked[_16] on handles attached with bsmr_backward_attach_blocks_split, bit for bit against
tests/blocked_split_twin.py on the pattern of tests/blocked_twin.py (panels of 0, 2, 5, 5, 5, 5, 5, 3 blocks, the last one
ragged; a padding column, empty cells, a residue row of three chunks), and through
bsmr_torch.SparseOperator(blocked=True, segment_blocks=2).  tests/test_spmm_blocked_split_host.py shows that on normal
data splitting changes the bits of more than a fifth of the elements in rows of split panels."""
import ctypes as C

import numpy as np
import pytest

import blocked_split_twin as st
import blocked_twin as bt
from gather_twin import assert_twin, col_lists, gather
from guarded import OPERAND, VALUES, Guarded, check_all

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = (32, 96, 256)           # below one 64-feature group, not a multiple of 64, several groups
SPLIT = (1, 2, 4)            # every panel with blocks split; the two-block panel whole; the three-block panel whole too
WHOLE = (0, 5, 2 ** 32 - 1)  # no panel split
FORMS = ("fp32", "fp16", "bf16")


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


def _normal(seed, nnz, N, K, form="fp32"):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(nnz).astype(np.float32), _round(rng.standard_normal((N, K)), form)


class Case:
    """the pattern, its RPHM and its twin once; one handle per segment_blocks (key None: attached with
    bsmr_backward_attach_blocks itself)"""

    def __init__(self, engine, oracle):
        self.engine = engine
        self.M, self.N, self.ro, self.ci = bt.blocked_pattern()
        self.nnz = int(self.ci.size)
        csr = engine.CSR.from_arrays(self.M, self.N, self.ro, self.ci)
        self.arrays = engine.Pipeline(csr, alpha=0.3, delta=0.3, device=-1).arrays()
        self.twin = st.SplitTwin(oracle, self.M, self.N, self.ro, self.ci, self.arrays)
        self.handles = {}

    def create(self, S):
        e = self.engine
        bw = e.backward_create(self.M, self.N, self.ro, self.ci, row_order=self.arrays["reorderedRows"], device=0)
        if S is None:
            d, keep = e.rphm_desc(self.M, self.N, self.nnz, self.arrays)
            e._check(e.hip().bsmr_backward_attach_blocks(bw, C.byref(d)), "bsmr_backward_attach_blocks")
        else:
            e.backward_attach_blocks(bw, self.M, self.N, self.nnz, self.arrays, segment_blocks=S)
        return bw

    def bw(self, S):
        if S not in self.handles:
            self.handles[S] = self.create(S)
        return self.handles[S]

    def close(self):
        for bw in self.handles.values():
            self.engine.backward_destroy(bw)

    def run(self, S, K, v, X, form="fp32", nb=1, stream=None, bw=None):
        """the device result widened to fp32 numpy; v (nb, nnz) or (nnz,), X values already representable in `form`"""
        lead = (nb,) if nb > 1 else ()
        tv = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(_dev())
        tX = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(_dev()).to(_dtype(form))
        tY = torch.full(lead + (self.M, K), float("nan"), dtype=_dtype(form), device=_dev())   # every element is written
        torch.cuda.synchronize()
        self.engine.spmm_blocked(self.bw(S) if bw is None else bw, K, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), nb,
                                 _stream() if stream is None else stream, mode=_mode(self.engine, form))
        torch.cuda.synchronize()
        return tY.float().cpu().numpy()

    def gather(self, K, v, X):
        """bsmr_spmm (the plain gather)"""
        tv = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(_dev())
        tX = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(_dev())
        tY = torch.full((self.M, K), float("nan"), dtype=torch.float32, device=_dev())
        self.engine.spmm(self.bw(None), K, False, tv.data_ptr(), tX.data_ptr(), tY.data_ptr(), 1, _stream())
        torch.cuda.synchronize()
        return tY.cpu().numpy()


@pytest.fixture(scope="module")
def case(engine, oracle):
    c = Case(engine, oracle)
    yield c
    c.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("S", SPLIT)
def test_bit_for_bit_against_the_twin(case, S, K, form):
    v, X = _normal(K + S, case.nnz, case.N, K, form)
    got = case.run(S, K, v, X, form)
    assert_twin(got, _round(case.twin.twin(v, X, S), form), f"S={S} K={K} {form}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("S", WHOLE)
def test_without_a_split_panel_the_bytes_of_the_plain_attach(case, S, form):
    K = 96
    v, X = _normal(3, case.nnz, case.N, K, form)
    assert case.run(S, K, v, X, form).tobytes() == case.run(None, K, v, X, form).tobytes()


@pytest.mark.parametrize("S", SPLIT)
def test_exact_integers_equal_the_gather(case, S):
    K = 96
    rng = np.random.default_rng(7)
    v = rng.integers(-7, 8, case.nnz).astype(np.float32)
    X = rng.integers(-15, 16, (case.N, K)).astype(np.float32)
    got, want = case.run(S, K, v, X), case.gather(K, v, X)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(got, case.twin.fp64(v, X, S)[0].astype(np.float32))


@pytest.mark.parametrize("form", ("fp32", "bf16"))
@pytest.mark.parametrize("S", (1, 4))
def test_batches_equal_single_calls(case, S, form):
    """distinct v and X per batch: a wrong batch stride of the partials or of the staging rows mixes them"""
    K, nb = 96, 3
    rng = np.random.default_rng(17)
    v = rng.standard_normal((nb, case.nnz)).astype(np.float32)
    X = _round(rng.standard_normal((nb, case.N, K)), form)
    got = case.run(S, K, v, X, form, nb=nb)
    for b in range(nb):
        assert got[b].tobytes() == case.run(S, K, v[b], X[b], form).tobytes(), b
    assert_twin(got[2], _round(case.twin.twin(v[2], X[2], S), form), "batch 2")


def test_reproducible_call_to_call_and_stream_to_stream(case):
    K, S = 256, 2
    v, X = _normal(19, case.nnz, case.N, K)
    first = case.run(S, K, v, X)
    assert case.run(S, K, v, X).tobytes() == first.tobytes()
    side = torch.cuda.Stream(device=_dev())
    assert case.run(S, K, v, X, stream=side.cuda_stream).tobytes() == first.tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_non_finite_operands(case, form):
    """S = 2, +inf and NaN in rows of X that are block columns of split panels: the rows that store them behave as in the
    gather, the rows of the same panel with an EMPTY cell there get NaN (0 * inf) - through the partial of that segment -
    and every other row keeps the bits of the clean run"""
    K, S = 96, 2
    v, X = _normal(11, case.nnz, case.N, K, form)
    clean = case.run(S, K, v, X, form)
    dc = case.arrays["denseCols"].reshape(-1, 16)
    bv = case.arrays["blockValues"].reshape(-1, 16, 16)
    bo = case.arrays["blockOffsets"].astype(np.int64)
    rr = case.arrays["reorderedRows"]
    # two block columns of different split panels, each with an empty cell in a row that exists; the second pick lies
    # past the panel's first segment
    picks = []
    for p in range(bo.size - 1):
        if bo[p + 1] - bo[p] <= S:
            continue
        rows_here = min(16, rr.size - 16 * p)
        first = bo[p] + (S if picks else 0)
        for b in range(first, bo[p + 1]):
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
    got = case.run(S, K, v, Xb, form)
    assert_twin(got, _round(case.twin.twin(v, Xb, S), form), form)
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


@pytest.mark.parametrize("form", FORMS)
def test_guarded_buffers(case, form):
    """S = 1 and the weakest alignment the header allows: 16 bytes for X and Y, 4 for v; nothing written outside Y (every
    element of it written), nothing read outside v and X (a guard value read into a sum would make it NaN)"""
    K, nb, S = 96, 2, 1
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
    case.engine.spmm_blocked(case.bw(S), K, gv.ptr, gX.ptr, gY.ptr, nb, _stream(), mode=_mode(case.engine, form))
    torch.cuda.synchronize()
    check_all(gv, gX, gY)
    if form == "fp32":
        got = gY.numpy().reshape(nb, case.M, K)
    else:
        got = torch.from_numpy(gY.numpy().view(np.int16).copy()).view(_dtype(form)).float().numpy().reshape(nb, case.M, K)
    for b in range(nb):
        assert_twin(got[b], _round(case.twin.twin(v[b], X[b], S), form), f"guarded {form} batch {b}")


@pytest.mark.parametrize("form", ("fp32", "fp16"))
def test_reserve_covers_the_calls(case, form):
    """after bsmr_backward_reserve the workspace - residue partials, staging rows, segment partials - does not grow"""
    K, nb, S = 128, 3, 1
    engine = case.engine
    bw = case.create(S)
    try:
        engine.backward_reserve(bw, K, nb)
        before = engine.backward_stats(bw)["workspace_bytes"]
        s = engine.backward_blocked_stats(bw)
        split_segments = s["segments"] - (s["panels_with_blocks"] - s["split_panels"])
        assert before >= 4 * K * nb * 16 * (s["panels_with_blocks"] + split_segments)
        rng = np.random.default_rng(31)
        v = rng.standard_normal((nb, case.nnz)).astype(np.float32)
        X = _round(rng.standard_normal((nb, case.N, K)), form)
        for _ in range(2):
            got = case.run(S, K, v, X, form, nb=nb, bw=bw)
            assert engine.backward_stats(bw)["workspace_bytes"] == before
        assert_twin(got[1], _round(case.twin.twin(v[1], X[1], S), form), "after reserve")
    finally:
        engine.backward_destroy(bw)


@pytest.mark.parametrize("S", SPLIT)
def test_error_against_fp64(case, S):
    worst = 0.0
    for K in (32, 256):
        v, X = _normal(37 + K, case.nnz, case.N, K)
        got = case.run(S, K, v, X).astype(np.float64)
        Y64, bound = case.twin.fp64(v, X, S)
        ratio = float((np.abs(got - Y64) / np.where(bound > 0, bound, 1.0)).max())
        worst = max(worst, ratio)
        assert (np.abs(got - Y64) <= bound).all(), ratio
    print(f"blocked SpMM, segment_blocks = {S}: worst |Y - Y64| / bound = {worst:.3f}")


def test_device_statistics(case):
    engine = case.engine
    plain = engine.backward_blocked_stats(case.bw(None))
    assert plain == engine.backward_blocked_stats(case.bw(0))
    for S in SPLIT + WHOLE:
        dev = engine.backward_blocked_stats(case.bw(S))
        status, host = engine.blocked_check_status(case.M, case.N, case.ro, case.ci, case.arrays, segment_blocks=S)
        assert status == engine.OK
        assert {k: dev[k] for k in host if k != "device_index_bytes"} == {k: host[k] for k in host if k != "device_index_bytes"}
        assert {k: dev[k] for k in st.split_stats(case.arrays, S)} == st.split_stats(case.arrays, S)
        if S:   # the segment records (and the list of split panels) on top of the unsplit format
            assert dev["device_index_bytes"] > plain["device_index_bytes"]
    assert engine.backward_blocked_stats(case.bw(1))["device_index_bytes"] > engine.backward_blocked_stats(case.bw(5))["device_index_bytes"]


def test_second_attach_and_bad_plans(case):
    engine = case.engine
    assert engine.backward_attach_blocks_status(case.bw(2), case.M, case.N, case.nnz, case.arrays, segment_blocks=2) == \
        engine.ERR_INVALID_ARG
    assert engine.backward_attach_blocks_status(case.bw(None), case.M, case.N, case.nnz, case.arrays, segment_blocks=2) == \
        engine.ERR_INVALID_ARG
    bad = bt.copy_arrays(case.arrays)
    bad["sparseColIndices"][0] = (bad["sparseColIndices"][0] + 1) % case.N
    bw = engine.backward_create(case.M, case.N, case.ro, case.ci, device=0)
    try:
        assert engine.backward_attach_blocks_status(bw, case.M, case.N, case.nnz, bad, segment_blocks=2) == engine.ERR_BAD_PLAN
        assert engine.hip().bsmr_spmm_blocked(bw, 64, None, None, None, 1, None) == engine.ERR_BAD_PLAN   # still unattached
    finally:
        engine.backward_destroy(bw)


# ---- torch: SparseOperator(blocked=True, segment_blocks=S) -----------------------------------------------------------
@pytest.fixture(scope="module")
def ops(engine, oracle):
    import bsmr_torch
    M, N, ro, ci = bt.blocked_pattern()
    csr = engine.CSR.from_arrays(M, N, ro, ci)
    make = lambda **kw: bsmr_torch.SparseOperator(csr, mode=engine.COMPUTE_F32, device=0, **kw)
    split = make(blocked=True, segment_blocks=2)
    return {"split": split, "zero": make(blocked=True, segment_blocks=0), "blocked": make(blocked=True), "csr": csr,
            "twin": st.SplitTwin(oracle, M, N, ro, ci, split.pipeline.arrays()), "cl": col_lists(M, N, ro, ci)}


def _leaf(shape, seed, form):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).to(_dev()).to(_dtype(form)).requires_grad_(True)


def _np(t):
    return t.detach().float().cpu().numpy()


@pytest.mark.parametrize("form", ("fp32", "bf16"))
def test_torch_spmm_and_dA_against_the_twin(oracle, ops, form):
    K = 96
    op, tw = ops["split"], ops["twin"]
    assert op.blocked is True and op.segment_blocks == 2
    v = _leaf((op.nnz,), 41, "fp32").detach()
    X = _leaf((op.N, K), 42, form).detach()
    assert_twin(_np(op.spmm(v, X)), _round(tw.twin(_np(v), _np(X), 2), form), "spmm")
    A, B = _leaf((op.M, K), 51, form), _leaf((op.N, K), 52, form)
    G = _leaf((op.nnz,), 53, "fp32").detach()
    (op.sddmm(A, B) * G).sum().backward()
    assert_twin(_np(A.grad), _round(tw.twin(_np(G), _np(B), 2), form), "dA")
    assert_twin(_np(B.grad), _round(gather(oracle, ops["cl"], _np(G), _np(A)), form), "dB")   # the gather, untouched


def test_torch_segment_blocks_zero_is_blocked_true(ops):
    K = 96
    outs = []
    for op in (ops["zero"], ops["blocked"]):
        assert op.segment_blocks == 0
        v, X = _leaf((op.nnz,), 71, "fp32"), _leaf((op.N, K), 72, "fp32")
        A, B = _leaf((op.M, K), 73, "fp32"), _leaf((op.N, K), 74, "fp32")
        Y = op.spmm(v, X)
        (Y.sum() + (op.sddmm(A, B) * v.detach()).sum()).backward()
        outs.append([_np(t).tobytes() for t in (Y, v.grad, X.grad, A.grad, B.grad)])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("kwargs", [{"segment_blocks": 2}, {"blocked": False, "segment_blocks": 1},
                                    {"blocked": True, "segment_blocks": -1}, {"blocked": True, "segment_blocks": 2.0},
                                    {"blocked": True, "segment_blocks": None}])
def test_torch_value_errors(ops, kwargs):
    import bsmr_torch
    with pytest.raises(ValueError):
        bsmr_torch.SparseOperator(ops["csr"], device=0, **kwargs)
