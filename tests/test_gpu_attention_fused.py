"""The fused sparse attention on the device, through the C ABI (include/bsmr_hip.h "Fused sparse attention"):
  1. exact-weight inputs (one constant per row mixed with -inf): O, m and s bit for bit against the twin;
  2. random scores (|scale p| <= 8) and |V| <= 1 inside the header's bound, NaN exactly where fp64 has it;
  3. special values: NaN, +inf, an all -inf row, a single-entry row, an isolated -inf;
  4. reproducibility: natural / clustered / reversed row_order, batch against single calls, call against call;
  5. the 16-bit calls: O16 is the fp32 call on the widened V, rounded once; m and s are its bits;
  6. the backward: W inside the softmax bound, D and dP bit for bit against their twins, in place, 16-bit;
  7. the memory contract on guarded buffers at the weakest alignment;
  8. no allocation after bsmr_sparse_attention_reserve; the empty pattern with NULL inputs.
Patterns: a 16 x 1536 ladder with rows of 0, 1, 63, 64, 65, 511, 512, 513 and 1025 entries (unsplit rows, a 2-chunk row,
a 3-chunk row) and synth.random_pattern(256, 384, 12000, seed=5, empty_rows=19); Kv covers every slice width."""
import zlib

import numpy as np
import pytest

import synth
from attention_twin import check_forward, exact_forward, exact_scores, forward_f64, row_dot, values_backward
from gather_twin import assert_twin
from guarded import OPERAND, VALUES, Guarded, check_all
from softmax_twin import U, row_of, z_of
from softmax_twin import check_forward as check_weights

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KVS = (32, 64, 96, 128, 256, 512)
LADDER = (0, 1, 63, 64, 65, 511, 512, 513, 1025, 2, 7, 0, 3, 130, 600, 1)
DT = {0: torch.float16, 1: torch.bfloat16}


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=_dev())   # poisoned: every element must be written


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(" ".join(map(str, key)).encode()))


def to16(mode, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[mode])


def words(t16):
    return t16.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def ladder_pattern():
    rng = np.random.default_rng(11)
    cols = 1536
    per_row = [np.sort(rng.choice(cols, n, replace=False)) for n in LADDER]
    ro = np.concatenate([[0], np.cumsum(LADDER)]).astype(np.uint32)
    return len(LADDER), cols, ro, np.concatenate(per_row).astype(np.uint32)


PATTERNS = {"ladder": ladder_pattern,
            "random": lambda: synth.random_pattern(256, 384, 12000, seed=5, empty_rows=19)}


class Pat:
    def __init__(self, engine, rows, cols, ro, ci):
        self.engine, self.rows, self.cols = engine, rows, cols
        self.ro = np.ascontiguousarray(ro, dtype=np.uint32)
        self.ci = np.ascontiguousarray(ci, dtype=np.uint32)
        self.nnz = int(self.ci.size)
        self.lens = np.diff(self.ro.astype(np.int64))
        self.bw = engine.backward_create(rows, cols, self.ro, self.ci, device=0)

    def forward(self, p, V, scale, nb=1, bw=None, mode=None):
        """(O, m, s) as numpy; mode None: fp32 V [nb, N, Kv]; 0 / 1: V a CPU tensor of that 16-bit dtype, O its words"""
        Kv = V.shape[-1]
        tp = _t(p)
        tV = _t(V) if mode is None else V.to(_dev())
        tO = _nan(nb * self.rows, Kv, dtype=torch.float32 if mode is None else DT[mode])
        tm, ts = _nan(nb * self.rows), _nan(nb * self.rows)
        self.engine.sparse_attention(bw or self.bw, Kv, scale, tp.data_ptr(), tV.data_ptr(), tO.data_ptr(), tm.data_ptr(),
                                     ts.data_ptr(), nb, _stream(), mode=self.engine.COMPUTE_F32 if mode is None else mode)
        torch.cuda.synchronize()
        O = (tO.cpu().numpy() if mode is None else words(tO)).reshape(nb, self.rows, Kv)
        return O, tm.cpu().numpy().reshape(nb, self.rows), ts.cpu().numpy().reshape(nb, self.rows)

    def backward(self, p, m, s, dW, O, dO, scale, nb=1, in_place=False, mode=None):
        """(dP, W) as numpy; O / dO fp32 arrays, or CPU 16-bit tensors with mode 0 / 1"""
        Kv = O.shape[-1]
        tp, tm, ts, tdW = _t(p), _t(m), _t(s), _t(dW)
        tO, tdO = (_t(O), _t(dO)) if mode is None else (O.to(_dev()), dO.to(_dev()))
        tdP = tdW if in_place else _nan(nb * self.nnz)
        tW = _nan(nb * self.nnz)
        self.engine.sparse_attention_backward(self.bw, Kv, scale, tp.data_ptr(), tm.data_ptr(), ts.data_ptr(), tdW.data_ptr(),
                                              tO.data_ptr(), tdO.data_ptr(), tdP.data_ptr(), tW.data_ptr(), nb, _stream(),
                                              mode=self.engine.COMPUTE_F32 if mode is None else mode)
        torch.cuda.synchronize()
        return tdP.cpu().numpy().reshape(nb, self.nnz), tW.cpu().numpy().reshape(nb, self.nnz)

    def row_max(self, p, scale):
        """m of the contract for NaN-free scores: the fp32 maximum of fl(scale p), -inf for an empty row"""
        z = z_of(p, scale)
        m = np.full(self.rows, -np.inf, np.float32)
        live = np.nonzero(self.lens)[0]
        m[live] = np.maximum.reduceat(z, self.ro[live].astype(np.int64))
        return m


@pytest.fixture(scope="module")
def pats(engine):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Pat(engine, *PATTERNS[name]())
        return made[name]

    yield get
    for p in made.values():
        engine.backward_destroy(p.bw)


def test_patterns_have_their_rows(engine, pats):
    p = pats("ladder")
    st = engine.backward_stats(p.bw)
    assert (p.rows, p.cols) == (16, 1536) and st["chunk"] == 512
    assert st["split_rows"] == 3 and st["row_items"] == 13 + 2 + 3 + 2           # 513 and 600: 2 chunks, 1025: 3
    r = pats("random")
    assert (r.lens == 0).sum() >= 19 and r.nnz == 12000 and engine.backward_stats(r.bw)["split_rows"] == 0


# ---- 1. exact weights: bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", (1, 3))
@pytest.mark.parametrize("Kv", KVS)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_exact_weights_equal_the_twin(engine, oracle, pats, name, Kv, nb):
    p = pats(name)
    rng = _rng("exact", name, Kv, nb)
    dead = np.nonzero(p.lens > 1)[0][[1, -1]]                    # two rows whose entries are all -inf
    scores, es = zip(*(exact_scores(p.ro, rng, dead) for _ in range(nb)))
    V = rng.standard_normal((nb, p.cols, Kv)).astype(np.float32)
    scale = 0.5
    O, m, s = p.forward(np.stack(scores), V, scale, nb)
    for b in range(nb):
        want_O, want_s = exact_forward(oracle, p.ro, p.ci, es[b], V[b])
        assert want_s.max() > 16 and (want_s[dead] == 0).all()
        assert_twin(O[b], want_O, f"{name} Kv={Kv} batch {b}: O")
        assert np.array_equal(_bits(s[b]), _bits(want_s)), (name, Kv, b, "s")
        assert np.array_equal(_bits(m[b]), _bits(p.row_max(scores[b], scale))), (name, Kv, b, "m")
        assert (_bits(O[b][dead]) == 0).all() and (_bits(O[b][p.lens == 0]) == 0).all()      # exact +0 rows


# ---- 2. random scores under the bound ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Kv", KVS)
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_random_scores_stay_inside_the_bound(engine, pats, name, Kv):
    p = pats(name)
    rng = _rng("bound", name, Kv)
    scale = 0.37
    scores = (rng.uniform(-8, 8, p.nnz) / scale).astype(np.float32)
    V = rng.uniform(-1, 1, (p.cols, Kv)).astype(np.float32)
    O, m, s = p.forward(scores, V, scale)
    worst = check_forward(p.ro, p.ci, scores, scale, V, O[0], f"{name} Kv={Kv}")
    print(f"{name} Kv={Kv}: worst error / bound = {worst:.3f}")
    assert np.array_equal(_bits(m[0]), _bits(p.row_max(scores, scale)))
    _, _, m64, s64 = forward_f64(p.ro, p.ci, scores, scale, V)
    zr = np.array([np.abs(z_of(scores[a:b], scale) - m[0][i]).max() if b > a else 0.0
                   for i, (a, b) in enumerate(zip(p.ro[:-1], p.ro[1:]))])
    assert (np.abs(s[0] - s64) <= (p.lens + 3 + zr) * U * s64).all()            # the error of s


# ---- 3. special values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kv", (64, 256))
def test_special_values(engine, pats, Kv):
    p = pats("ladder")
    rng = _rng("special", Kv)
    scale = 0.7
    scores = (rng.standard_normal(p.nnz) * 4).astype(np.float32)
    V = rng.uniform(-1, 1, (p.cols, Kv)).astype(np.float32)
    clean, m0, s0 = p.forward(scores, V, scale)
    row = {n: LADDER.index(n) for n in (1, 63, 65, 511, 513, 1025, 600)}
    x = scores.copy()
    x[p.ro[row[63]] + 31] = np.nan                               # a NaN in a short row
    x[p.ro[row[1025]] + 700] = np.nan                            # ... and in the second chunk of a split one
    x[p.ro[row[65]] + 64] = np.inf                               # a +inf
    x[p.ro[row[513]]] = np.inf
    x[p.ro[row[511]]:p.ro[row[511] + 1]] = -np.inf               # all -inf rows, short and split
    x[p.ro[row[600]]:p.ro[row[600] + 1]] = -np.inf
    lone = LADDER.index(130)
    x[p.ro[lone] + 5] = -np.inf                                  # an isolated -inf
    O, m, s = p.forward(x, V, scale)
    O, m, s = O[0], m[0], s[0]
    for n in (63, 1025, 65, 513):
        assert np.isnan(O[row[n]]).all(), n
    assert np.isnan(m[row[63]]) and np.isnan(m[row[1025]]) and m[row[65]] == np.inf and np.isnan(s[row[513]])
    for n in (511, 600):
        assert (_bits(O[row[n]]) == 0).all() and m[row[n]] == -np.inf and _bits(s[row[n]]) == 0
    single = row[1]
    assert np.array_equal(_bits(O[single]), _bits(V[p.ci[p.ro[single]]]))       # e = 1, s = 1: the row of V itself
    assert s[single] == 1.0 and m[single] == z_of(scores[p.ro[single]], scale)
    touched = [row[n] for n in (63, 1025, 65, 513, 511, 600)] + [lone]
    rest = np.setdiff1d(np.arange(p.rows), touched)
    assert np.array_equal(_bits(O[rest]), _bits(clean[0][rest])) and np.array_equal(_bits(s[rest]), _bits(s0[0][rest]))
    check_forward(p.ro, p.ci, x, scale, V, O, f"special Kv={Kv}")                # the -inf entry weighs nothing; NaN rows
    assert not np.array_equal(_bits(O[lone]), _bits(clean[0][lone]))


# ---- 4. reproducibility -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,Kv", [("ladder", 128), ("random", 32), ("random", 512)])
def test_bits_do_not_depend_on_order_batch_or_call(engine, pats, name, Kv):
    p = pats(name)
    rng = _rng("repro", name, Kv)
    nb, scale = 3, 1.3
    scores = (rng.standard_normal((nb, p.nnz)) * 3).astype(np.float32)
    V = rng.standard_normal((nb, p.cols, Kv)).astype(np.float32)
    csr = engine.CSR.from_arrays(p.rows, p.cols, p.ro, p.ci)
    clustered = engine.Pipeline(csr, alpha=0.3, delta=0.3, device=-1).array("reorderedRows")
    others = [engine.backward_create(p.rows, p.cols, p.ro, p.ci, row_order=o, device=0)
              for o in (clustered, np.arange(p.rows, dtype=np.uint32)[::-1].copy())]
    try:
        first = p.forward(scores, V, scale, nb)
        same = lambda got, where: [np.testing.assert_array_equal(_bits(g), _bits(f), err_msg=where) for g, f in zip(got, first)]
        same(p.forward(scores, V, scale, nb), "second call")
        for i, bw in enumerate(others):
            same(p.forward(scores, V, scale, nb, bw=bw), f"row_order {i}")
        for b in range(nb):
            one = p.forward(scores[b], V[b], scale)
            for g, f in zip(one, first):
                assert np.array_equal(_bits(g[0]), _bits(f[b])), ("batch", b)
    finally:
        for bw in others:
            engine.backward_destroy(bw)


# ---- 5. the 16-bit forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name,Kv", [("ladder", k) for k in KVS] + [("random", 64), ("random", 256)])
def test_16_bit_forward_is_the_fp32_call_rounded_once(engine, pats, name, Kv, mode):
    p = pats(name)
    rng = _rng("io16", name, Kv, mode)
    nb, scale = 2, 0.6
    scores = (rng.standard_normal((nb, p.nnz)) * 3).astype(np.float32)
    scores[0, p.ro[3]:p.ro[4]] = -np.inf                         # a dead row in 16 bits too
    V16 = to16(mode, rng.standard_normal((nb, p.cols, Kv)))
    O16, m16, s16 = p.forward(scores, V16, scale, nb, mode=mode)
    O, m, s = p.forward(scores, V16.float().numpy(), scale, nb)
    assert np.array_equal(O16, words(to16(mode, O))), (name, Kv, mode)
    assert np.array_equal(_bits(m16), _bits(m)) and np.array_equal(_bits(s16), _bits(s))


# ---- 6. the backward ---------------------------------------------------------------------------------------------------
def _first_entry_scores(p, rng):
    """scores whose row has one finite entry, the first: w = (1, 0, 0, ...), so dP at that entry is (0 - D) for dW = 0"""
    x = np.full(p.nnz, -np.inf, np.float32)
    first = p.ro[:-1][p.lens > 0]
    x[first] = rng.integers(-4, 5, first.size).astype(np.float32)
    return x


@pytest.mark.parametrize("mode", (None, 0, 1))
@pytest.mark.parametrize("name,Kv", [("ladder", k) for k in KVS] + [("random", 32), ("random", 128)])
def test_backward_equals_its_twins(engine, oracle, pats, name, Kv, mode):
    p = pats(name)
    rng = _rng("backward", name, Kv, mode)
    nb, scale = 2, 0.45
    scores = (rng.standard_normal((nb, p.nnz)) * 5).astype(np.float32)
    V = rng.standard_normal((nb, p.cols, Kv)).astype(np.float32)
    dO = rng.standard_normal((nb, p.rows, Kv)).astype(np.float32)
    dW = rng.standard_normal((nb, p.nnz)).astype(np.float32)
    if mode is None:
        O, m, s = p.forward(scores, V, scale, nb)
        O_in, dO_in, O_wide, dO_wide = O, dO, O, dO
    else:
        V16, dO_in = to16(mode, V), to16(mode, dO)
        O, m, s = p.forward(scores, V16, scale, nb, mode=mode)
        O_in = torch.from_numpy(O.view(np.int16)).view(DT[mode])
        O_wide, dO_wide = O_in.float().numpy(), dO_in.float().numpy()          # D is taken on the saved, rounded O
    dP, W = p.backward(scores, m, s, dW, O_in, dO_in, scale, nb, mode=mode)
    where = f"{name} Kv={Kv} mode={mode}"
    for b in range(nb):
        check_weights(p.ro, scores[b], scale, W[b], f"{where} batch {b}: W")   # the bound of y in "Sparse row softmax"
        D = row_dot(oracle, dO_wide[b], O_wide[b])
        assert_twin(dP[b], values_backward(p.ro, W[b], dW[b], D, scale), f"{where} batch {b}: dP")
    dP2, W2 = p.backward(scores, m, s, dW, O_in, dO_in, scale, nb, in_place=True, mode=mode)
    assert np.array_equal(_bits(dP2), _bits(dP)) and np.array_equal(_bits(W2), _bits(W)), where + " in place"
    # D itself: with w = (1, 0, ...), dW = 0 and scale = 1 the first entry of a row holds 0 - D
    x = _first_entry_scores(p, rng)
    zero = np.zeros(p.nnz, np.float32)
    dPx, Wx = p.backward(x, p.row_max(x, 1.0), (p.lens > 0).astype(np.float32), zero, O_in[0], dO_in[0], 1.0, mode=mode)
    D = row_dot(oracle, dO_wide[0], O_wide[0])
    assert np.array_equal(Wx[0], np.isfinite(x).astype(np.float32))
    assert_twin(dPx[0], values_backward(p.ro, Wx[0], zero, D, 1.0), where + ": D")
    live = p.lens > 0
    assert np.array_equal(_bits(dPx[0][p.ro[:-1][live]]), _bits(np.float32(0) - D[live]))


def test_backward_of_dead_and_nan_rows(engine, pats):
    p = pats("ladder")
    rng = _rng("backward special")
    Kv, scale = 64, 0.8
    scores = (rng.standard_normal(p.nnz) * 3).astype(np.float32)
    dead, nan_row = LADDER.index(513), LADDER.index(65)
    scores[p.ro[dead]:p.ro[dead + 1]] = -np.inf
    scores[p.ro[nan_row] + 3] = np.nan
    V = rng.standard_normal((p.cols, Kv)).astype(np.float32)
    O, m, s = p.forward(scores, V, scale)
    dO = rng.standard_normal((p.rows, Kv)).astype(np.float32)
    dW = rng.standard_normal(p.nnz).astype(np.float32)
    dP, W = p.backward(scores, m, s, dW, O[0], dO, scale)
    r = row_of(p.ro)
    assert (_bits(W[0][r == dead]) == 0).all() and (dP[0][r == dead] == 0).all()
    assert np.isnan(W[0][r == nan_row]).all() and np.isnan(dP[0][r == nan_row]).all()
    rest = ~np.isin(r, (dead, nan_row))
    assert np.isfinite(W[0][rest]).all() and np.isfinite(dP[0][rest]).all()


# ---- 7. the memory contract ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (None, 0, 1))
@pytest.mark.parametrize("Kv", (32, 128, 512))
def test_calls_stay_inside_the_buffers(engine, pats, Kv, mode):
    """every array at the weakest alignment the header accepts, between NaN guards: guards and inputs intact, every word
    of O, m, s, dP and W written, and the bits of the same call on ordinary tensors"""
    p = pats("ladder")
    rng = _rng("guards", Kv, mode)
    nb, scale = 2, 0.9
    dev = _dev()
    f32, K = engine.COMPUTE_F32, Kv
    scores = (rng.standard_normal((nb, p.nnz)) * 3).astype(np.float32)
    V = rng.standard_normal((nb, p.cols, Kv)).astype(np.float32)
    dO = rng.standard_normal((nb, p.rows, Kv)).astype(np.float32)
    dW = rng.standard_normal((nb, p.nnz)).astype(np.float32)
    rows16 = np.float32 if mode is None else np.uint16
    as_rows = (lambda a: a) if mode is None else (lambda a: words(to16(mode, a)))
    gP = Guarded.input("P", scores, VALUES, K, dev)
    gV = Guarded.input("V", as_rows(V), OPERAND, K, dev, dtype=rows16)
    gO = Guarded.output("O", nb * p.rows * Kv, OPERAND, K, dev, dtype=rows16)
    gm, gs = (Guarded.output(n, nb * p.rows, VALUES, K, dev) for n in ("m", "s"))
    engine.sparse_attention(p.bw, Kv, scale, gP.ptr, gV.ptr, gO.ptr, gm.ptr, gs.ptr, nb, _stream(), mode=f32 if mode is None else mode)
    torch.cuda.synchronize()
    check_all(gP, gV, gO, gm, gs)
    Vin = V if mode is None else to16(mode, V)
    O, m, s = p.forward(scores, Vin, scale, nb, mode=mode)
    assert np.array_equal(_bits(gO.numpy()), _bits(O.ravel()))
    assert np.array_equal(_bits(gm.numpy()), _bits(m.ravel())) and np.array_equal(_bits(gs.numpy()), _bits(s.ravel()))
    for g in (gO, gm, gs):
        g.freeze()
    gdW = Guarded.input("dW", dW, VALUES, K, dev)
    gdO = Guarded.input("dO", as_rows(dO), OPERAND, K, dev, dtype=rows16)
    gdP, gW = (Guarded.output(n, nb * p.nnz, VALUES, K, dev) for n in ("dP", "W"))
    engine.sparse_attention_backward(p.bw, Kv, scale, gP.ptr, gm.ptr, gs.ptr, gdW.ptr, gO.ptr, gdO.ptr, gdP.ptr, gW.ptr, nb,
                                     _stream(), mode=f32 if mode is None else mode)
    torch.cuda.synchronize()
    check_all(gP, gm, gs, gdW, gO, gdO, gdP, gW)
    O_in = O if mode is None else torch.from_numpy(O.view(np.int16)).view(DT[mode])
    dP, W = p.backward(scores, m, s, dW, O_in, dO if mode is None else to16(mode, dO), scale, nb, mode=mode)
    assert np.array_equal(_bits(gdP.numpy()), _bits(dP.ravel())) and np.array_equal(_bits(gW.numpy()), _bits(W.ravel()))
    gD = Guarded.inplace("dW=dP", dW, VALUES, K, dev)                            # in place
    gW2 = Guarded.output("W", nb * p.nnz, VALUES, K, dev)
    engine.sparse_attention_backward(p.bw, Kv, scale, gP.ptr, gm.ptr, gs.ptr, gD.ptr, gO.ptr, gdO.ptr, gD.ptr, gW2.ptr, nb,
                                     _stream(), mode=f32 if mode is None else mode)
    torch.cuda.synchronize()
    check_all(gP, gm, gs, gO, gdO, gD, gW2)
    assert np.array_equal(_bits(gD.numpy()), _bits(dP.ravel()))


# ---- 8. workspace, empty pattern ---------------------------------------------------------------------------------------
def test_calls_after_reserve_allocate_nothing(engine):
    p = Pat(engine, *ladder_pattern())
    try:
        Kv, nb = 256, 3
        assert engine.backward_stats(p.bw)["workspace_bytes"] == 0
        engine.sparse_attention_reserve(p.bw, Kv, nb)
        before = engine.backward_stats(p.bw)["workspace_bytes"]
        slots = 2 + 2 + 3
        assert before >= 4 * nb * (slots * Kv + slots + p.rows)                  # the partial rows, partial sums and D
        rng = _rng("reserve")
        scores = rng.standard_normal((nb, p.nnz)).astype(np.float32)
        V = rng.standard_normal((nb, p.cols, Kv)).astype(np.float32)
        O, m, s = p.forward(scores, V, 1.0, nb)
        assert engine.backward_stats(p.bw)["workspace_bytes"] == before
        p.backward(scores, m, s, scores, O, O, 1.0, nb)
        p.forward(scores[0], to16(0, V[0]), 1.0, mode=0)
        tW, tdO, tY = _t(scores), _t(O), _nan(nb, p.cols, Kv)                    # the step's transposed SpMM fits too
        engine.spmm(p.bw, Kv, True, tW.data_ptr(), tdO.data_ptr(), tY.data_ptr(), nb, _stream())
        torch.cuda.synchronize()
        assert engine.backward_stats(p.bw)["workspace_bytes"] == before
    finally:
        engine.backward_destroy(p.bw)


@pytest.mark.parametrize("nb", (1, 2))
def test_empty_pattern_with_null_inputs(engine, nb):
    rows, Kv = 5, 64
    bw = engine.backward_create(rows, 7, np.zeros(rows + 1, np.uint32), np.zeros(0, np.uint32), device=0)
    hip = engine.hip()
    try:
        for mode in (None, 0, 1):
            tO = _nan(nb * rows, Kv, dtype=torch.float32 if mode is None else DT[mode])
            tm, ts = _nan(nb * rows), _nan(nb * rows)
            if mode is None:
                st = hip.bsmr_sparse_attention(bw, Kv, 1.0, None, None, tO.data_ptr(), tm.data_ptr(), ts.data_ptr(), nb, _stream())
                stb = hip.bsmr_sparse_attention_backward(bw, Kv, 1.0, None, None, None, None, None, None, None, None, nb, _stream())
            else:
                st = hip.bsmr_sparse_attention_16(bw, Kv, 1.0, None, None, tO.data_ptr(), tm.data_ptr(), ts.data_ptr(), nb, mode,
                                                  _stream())
                stb = hip.bsmr_sparse_attention_backward_16(bw, Kv, 1.0, None, None, None, None, None, None, None, None, nb,
                                                            mode, _stream())
            torch.cuda.synchronize()
            assert st == engine.OK and stb == engine.OK
            assert (tO.view(torch.int16 if mode is not None else torch.int32) == 0).all()
            assert (tm == float("-inf")).all() and (ts.view(torch.int32) == 0).all()
    finally:
        engine.backward_destroy(bw)
