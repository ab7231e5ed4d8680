"""torch entry point of the engine: one sparsity pattern S, its SDDMM and SpMM as differentiable operators.

    op = SparseOperator(csr)                 # pipeline (clustered rows), SDDMM plan, backward handle
    P = op.sddmm(A, B)                       # P[t] = A[row(t)] . B[col(t)]           (nnz,) or (b, nnz)
    W = op.softmax(P, scale)                 # W = softmax of scale * P over each row of S   (nnz,) or (b, nnz)
    Y = op.spmm(values, X)                   # Y = S_values X     (transpose=True: S_values^T X)
    O = op.attention(Q, Kt, V)               # spmm(softmax(sddmm(Q, Kt), K**-0.5), V)
    O = op.softmax_spmm(P, V, scale)         # softmax and spmm in one gather: the weights are never stored
    O = op.attention(Q, Kt, V, fused=True)   # softmax_spmm(sddmm(Q, Kt), V, K**-0.5)

All are torch.autograd.Functions whose backward runs on the engine (bsmr_sddmm_backward, bsmr_spmm, bsmr_sddmm,
bsmr_sparse_softmax_backward, bsmr_sparse_attention_backward), attention by composing the others:
    sddmm:    dA = S_dP B,  dB = S_dP^T A    (exact fp32 products of the given operands in every mode: the forward's
                                              operand rounding is treated as straight-through)
              with gather_mode = F16 / BF16:  dA = S_dP round(B),  dB = S_dP^T round(A) - the straight-through
                                              gradients of the product of the ROUNDED operands, which is what the
                                              forward computes when `mode` is the same format
    softmax:  dX = (W * (dW - rowsum(W * dW))) * scale   (bsmr_sparse_softmax_backward: bitwise reproducible)
    spmm:     d values = sddmm(dY, X)  (transposed: sddmm(X, dY)),  dX = spmm(values, dY, not transpose)
    softmax_spmm:  forward bsmr_sparse_attention, which also returns the row maxima m and row sums s; it saves
              (values, X, m, s, O).  Backward: dW = sddmm(dO, X);  bsmr_sparse_attention_backward recomputes the weights W
              from (values, m, s) and gives d values = (W * (dW - rowdot(dO, O))) * scale;  dX = spmm(W, dO, transposed).
              Its sums run in another order than softmax followed by spmm, so the two paths agree to rounding, not in
              bits (include/bsmr_hip.h "Fused sparse attention"); each is bitwise reproducible.  X follows spmm's dtype
              rule: 16-bit X gives 16-bit O and dX, and D = rowdot(dO, O) is taken on the saved, rounded O.
so SDDMM -> softmax -> SpMM, the usual sparse-attention layer, trains on the engine end to end.  attention(fused=True)
takes the fused path; the default (fused=False) is the composition, unchanged.

blocked (default False: every result bit for bit as without the argument): with blocked=True the operator attaches the
pipeline's RPHM to its backward handle (bsmr_backward_attach_blocks) and the row direction - spmm(transpose=False), hence
attention's last step, and the dA of sddmm's backward - runs bsmr_spmm_blocked[_16]: the entries in the RPHM's dense 16 x 16
blocks on the fp32 MFMA, one read of a row of X per block instead of one per entry, the rest on the gather.  Same
function, another summation order (include/bsmr_hip.h "Blocked SpMM": the result depends on the reordering; an empty block
cell meets a non-finite X as 0 * x).  The transposed spmm, dB, softmax, softmax_spmm and every SDDMM are untouched.
blocked=True needs gather_mode=COMPUTE_F32 (ValueError otherwise).
segment_blocks (default 0: the bits of blocked=True as without the argument) = S >= 1 attaches with
bsmr_backward_attach_blocks_split: a panel's block list is cut into segments of S blocks, one wave each, whose fp32 sums
are added in segment order, so a panel with many blocks is no longer one serial loop.  Panels with more than S blocks get
another summation order (the header's "Blocked SpMM", Segment chain).  It must be an int >= 0, and a non-zero value needs
blocked=True (ValueError otherwise).

gather_mode (default COMPUTE_F32: every result bit for bit as without the argument) is the format in which the gathers
read their operand rows: with COMPUTE_F16 / COMPUTE_BF16 spmm's X, the dY of its dX, and the B / A of sddmm's dA / dB are
rounded once per call and gathered as 16-bit rows (half the bytes); values, sums and results stay fp32.  spmm then
returns S_values round(X), and its dX is S_values^T round(dY): the gradients of the rounded-operand products.  The
SDDMM calls (the forward, d values of spmm) follow `mode`, not gather_mode.  Both arguments concern fp32 tensors only.

Operand tensors (A / B, Q / Kt, X, V) may also be torch.float16 or torch.bfloat16, as a model under autocast holds them.
The operands of one call share a dtype (a mix raises ValueError); attention's Q / Kt and V may differ, fp32 weights sit
between them.  The format then follows the dtype, whatever `mode` and `gather_mode` say, and nothing is cast or copied:
    sddmm:  P (fp32) = bsmr_sddmm_16(A, B), the fp32-accumulated products of the 16-bit values as they are;
            dA, dB in the operands' dtype = bsmr_sddmm_backward_16: round(S_dP B), round(S_dP^T A)
    spmm:   Y in X's dtype = bsmr_spmm_16: round(S_values X);  dX likewise from the transposed direction on dY (taken
            in that dtype, not widened);  d values (fp32) = bsmr_sddmm_16(dY, X)
Sums run in fp32 on the exactly widened rows and each output element is rounded once (round to nearest even).  The
value tensors - `values`, P, the input and output of softmax - are fp32 only: scores and weights are never 16-bit.
fp32 operands take the fp32 calls, bit for bit as before.

fp8 keys and values.  The column-side operand - B / Kt of sddmm, X / V of spmm, softmax_spmm and attention - may be
torch.float8_e4m3fn or torch.float8_e5m2, as an fp8 KV cache holds it (include/bsmr_hip.h "fp8 keys and values").  Both
formats embed exactly in fp16 and in bf16, so every such call is, bit for bit, the 16-bit call on the exactly widened
tensor - and nothing is cast or copied by the operator:
    sddmm(A, B8):  A fp16 / bf16 -> P (fp32) = bsmr_sddmm_b8 (B8 is widened into the plan's workspace, A read in place);
                   dA in A's dtype = bsmr_spmm_x8(dP, B8)
    spmm(values, X8, out_dtype=torch.float16 | torch.bfloat16):  Y in out_dtype = bsmr_spmm_x8, the gather reading the
                   bytes;  d values = bsmr_sddmm_b8(dY, X8).  transpose=True is refused (an fp8 row-side operand)
    softmax_spmm(values, X8, scale, out_dtype=...):  bsmr_sparse_attention_x8, saving (values, X8, m, s, O);
                   dW = bsmr_sddmm_b8(dO, X8), then bsmr_sparse_attention_backward_16 on (O, dO)
    attention(Q, Kt, V):  Kt and V may each be fp8, independently; out_dtype (default Q.dtype) is used when V is fp8
No gradient flows into an fp8 tensor: one that requires grad raises ValueError at the call.  out_dtype belongs to fp8 X
alone (ValueError with any other X, and when it is missing or not a 16-bit dtype with an fp8 X).  On a blocked=True
operator an fp8 X takes the gather: the blocked SpMM has no fp8 form, as it has none for the transposed direction.
Out of scope: per-row fp32 scales (a per-tensor scale of K folds into `scale` and one of V into the output, a per-row
one into values or P, by the caller), fp8 on the MFMA of the dense engine, fp8 outputs, an fp8 row-side operand.

MX block scales (MXFP8).  Every fp8 operand above takes a keyword - B_scale, X_scale, Kt_scale, V_scale - with the block
scales of the OCP Microscaling format: torch.float8_e8m0fnu or torch.uint8, shape (rows, K/32) or (b, rows, K/32) with
the operand's batch, contiguous, on the operator's device; one E8M0 code per 32 consecutive elements of a row, code e =
2^(e-127), 255 = NaN.  The operand is then dq = widen(code) * scale, one fp32 multiplication (include/bsmr_hip.h "MX block
scales"), and the calls above become bsmr_sddmm_b8_mx, bsmr_spmm_x8_mx and bsmr_sparse_attention_x8_mx in the forward and
in the backward alike; no gradient goes into codes or scales.  None (the default) is the unscaled call, the code that ran
before.  A scale beside an operand that is not fp8, of another dtype, shape, batch or device, or one that requires grad
raises ValueError.  bf16 is the format to put beside an MXFP8 Kt: the 16-bit copy sddmm dequantises into is exact in
bf16 for every scale code >= 3 (e4m3) / >= 10 (e5m2), in fp16 only for shifts in [-15, 7] / [-8, 0].
mx_quantize / mx_dequantize (plain torch, not a hot path) make and read such tensors.

MXFP4 keys and values.  B / Kt, X and V may also be torch.float4_e2m1fn_x2 (where torch has the dtype): OCP e2m1 codes, two
per byte, element 2i the low nibble of byte i; shape (rows, K/2) or (b, rows, K/2) with K = 2 * shape[-1] a positive multiple
of 32 (include/bsmr_hip.h "MXFP4 keys and values").  The matching scale keyword is then required (ValueError without it):
the same E8M0 tensor as above, (rows, K/32) or (b, rows, K/32).  dq = widen(code) * scale is exact in fp32 for every scale
code up to 254, and the calls are bsmr_sddmm_b4_mx, bsmr_spmm_x4_mx and bsmr_sparse_attention_x4_mx, forward and backward,
through autograd functions of their own in front of the dispatch above (a call without an fp4 tensor runs the code it ran
before):
    sddmm(A, B4, B_scale=Bs):  dA = bsmr_spmm_x4_mx(dP, B4, Bs)
    spmm(values, X4, out_dtype=..., X_scale=Xs):  d values = bsmr_sddmm_b4_mx(dY, X4, Xs);  transpose=True is refused
    softmax_spmm(values, X4, scale, out_dtype=..., X_scale=Xs):  dW = bsmr_sddmm_b4_mx(dO, X4, Xs), then
                   bsmr_sparse_attention_backward_16 on (O, dO)
    attention(Q, Kt, V):  Kt and V independently fp4, fp8 or 16-bit; out_dtype as for fp8
No gradient goes into codes or scales (ValueError if either requires grad); a blocked=True operator sends an fp4 X to the
gather.  Each call equals, bit for bit, the MXFP8 call on the e4m3 re-encoding of the codes with the same scales.  The
16-bit copy sddmm dequantises into is exact in bf16 for all 256 scale codes, in fp16 only for shifts in [-23, 13]: put
bf16 beside an MXFP4 Kt.  mx_quantize(x, torch.float4_e2m1fn_x2) / mx_dequantize work on the uint8 view (torch has no CPU
cast for the dtype): round to nearest, ties to the even code, saturating at +-6; NaN has no code (ValueError).
Out of scope: MXFP6, NVFP4 (fp8 scales per 16 elements), fp4 on the scaled MFMA of the dense engine, fp4 outputs or
row-side operands, any change to defaults or the tuner.

Every call runs on torch.cuda.current_stream(device).  Operands are contiguous, on the operator's device, with
K a positive multiple of 32; anything else raises ValueError.  Double backward is not supported.  Calls on one operator
share its workspaces: issue them from one thread (the current stream orders them).
"""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

import bsmr_amd as eng


_MODE16 = {torch.float16: eng.COMPUTE_F16, torch.bfloat16: eng.COMPUTE_BF16}   # the format follows the dtype
_MODE8 = {torch.float8_e4m3fn: eng.FP8_E4M3, torch.float8_e5m2: eng.FP8_E5M2}
_EMAX8 = {torch.float8_e4m3fn: 8, torch.float8_e5m2: 15}   # exponent of the largest normal: 448 = 1.75 2^8, 57344 = 1.75 2^15
_SCALE_DTYPES = (torch.uint8,) + ((torch.float8_e8m0fnu,) if hasattr(torch, "float8_e8m0fnu") else ())
MX_BLOCK = 32
_FP4 = getattr(torch, "float4_e2m1fn_x2", None)   # two e2m1 codes per byte, element 2i in the low nibble
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)   # the magnitude of code 0 .. 7; bit 3 is the sign
_E2M1_TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)   # the midpoint between codes i and i + 1


def _is8(t) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype in _MODE8


def _is4(t) -> bool:
    return _FP4 is not None and isinstance(t, torch.Tensor) and t.dtype == _FP4


def _k_of(t: torch.Tensor) -> int:
    """elements per row of a column-side operand: an fp4 tensor packs two per byte"""
    return 2 * t.shape[-1] if _is4(t) else t.shape[-1]


def _widen4(codes: torch.Tensor) -> torch.Tensor:
    """(..., K/2) packed e2m1 -> (..., K) fp32 by the table, low nibble first; -0 keeps its sign"""
    b = codes.view(torch.uint8).to(torch.int64)
    table = torch.tensor(_E2M1 + tuple(-x for x in _E2M1), dtype=torch.float32, device=codes.device)
    return torch.stack((table[b & 15], table[b >> 4]), dim=-1).reshape(tuple(codes.shape[:-1]) + (2 * codes.shape[-1],))


def _mx_scale_f32(scales: torch.Tensor) -> torch.Tensor:
    """E8M0 codes (uint8 or float8_e8m0fnu) as fp32: 2^(e-127) built from bits, code 0 the subnormal 2^-127, 255 NaN"""
    if scales.dtype not in _SCALE_DTYPES:
        raise ValueError(f"scales: dtype {scales.dtype}, expected torch.uint8 or torch.float8_e8m0fnu")
    e = scales.view(torch.uint8).to(torch.int32)
    bits = torch.where(e == 0, torch.full_like(e, 0x00400000), torch.where(e == 255, torch.full_like(e, 0x7FC00000), e << 23))
    return bits.view(torch.float32)


def mx_dequantize(codes: torch.Tensor, scales: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """widen(codes) * 2^(scales - 127) per block of 32 along the last dimension, one fp32 multiplication per element (the
    dq of include/bsmr_hip.h "MX block scales"), then cast to dtype.  codes (..., K) fp8, scales (..., K/32)."""
    if not (_is8(codes) or _is4(codes)):
        raise ValueError(f"codes: dtype {getattr(codes, 'dtype', None)}, expected torch.float8_e4m3fn, torch.float8_e5m2 or "
                         "torch.float4_e2m1fn_x2")
    K = _k_of(codes)   # fp4: (..., K/2) bytes
    if K % MX_BLOCK or tuple(scales.shape) != tuple(codes.shape[:-1]) + (K // MX_BLOCK,):
        raise ValueError(f"scales: shape {tuple(scales.shape)} beside codes {tuple(codes.shape)}, expected one per 32 elements")
    sc = _mx_scale_f32(scales).repeat_interleave(MX_BLOCK, dim=-1)
    return ((_widen4(codes) if _is4(codes) else codes.to(torch.float32)) * sc).to(dtype)


def mx_quantize(x: torch.Tensor, fp8_dtype=torch.float8_e4m3fn):
    """(codes, scales) of x (..., K), K a multiple of 32, in the OCP Microscaling way: per block of 32 the shared exponent
    e = floor(log2 amax) - emax_elem + 127 clamped to [0, 254] (amax the block's largest finite magnitude; an all-zero
    block gets 0), then x / 2^(e-127) cast with round to nearest even, saturating at the format's largest finite value
    (+-inf saturate too, NaN stays NaN).  codes in fp8_dtype, scales torch.uint8 (..., K/32).  A finite x never dequantises
    to a non-finite value.  A block whose amax has a mantissa above 1.75 saturates its largest e4m3 elements (the known
    clipping of the floor rule); e5m2 mantissas end at 1.75.
    fp8_dtype torch.float4_e2m1fn_x2: MXFP4, emax_elem = 2 (6 = 1.5 2^2); codes (..., K/2) packed low nibble first, rounded
    to nearest with ties to the even code, saturating at +-6 (a block whose amax has a mantissa above 1.5 saturates or
    rounds its largest elements to 6); NaN has no e2m1 code and raises ValueError."""
    if _FP4 is not None and fp8_dtype == _FP4:
        return _mx_quantize4(x)
    if fp8_dtype not in _MODE8:
        raise ValueError(f"fp8_dtype: {fp8_dtype!r}, expected torch.float8_e4m3fn, torch.float8_e5m2 or torch.float4_e2m1fn_x2")
    K = x.shape[-1]
    if K == 0 or K % MX_BLOCK:
        raise ValueError(f"x: K = {K}, expected a positive multiple of 32")
    blocks = x.to(torch.float64).reshape(tuple(x.shape[:-1]) + (K // MX_BLOCK, MX_BLOCK))
    mag = blocks.abs()
    amax = torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag)).amax(dim=-1)
    _, exp = torch.frexp(amax)                       # amax = f 2^exp, f in [0.5, 1): floor(log2 amax) = exp - 1
    e = (exp.to(torch.int64) - 1 - _EMAX8[fp8_dtype] + 127).clamp(0, 254)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    scaled = blocks * torch.exp2((127 - e).to(torch.float64)).unsqueeze(-1)   # exact: a power of two in fp64
    top = float(torch.finfo(fp8_dtype).max)
    codes = scaled.clamp(-top, top).to(torch.float32).to(fp8_dtype).reshape(x.shape)   # clamp keeps NaN
    return codes, e.to(torch.uint8)


def _mx_quantize4(x: torch.Tensor):
    K = x.shape[-1]
    if K == 0 or K % MX_BLOCK:
        raise ValueError(f"x: K = {K}, expected a positive multiple of 32")
    if torch.isnan(x).any():
        raise ValueError("x: NaN has no e2m1 code")
    blocks = x.to(torch.float64).reshape(tuple(x.shape[:-1]) + (K // MX_BLOCK, MX_BLOCK))
    mag = blocks.abs()
    amax = torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag)).amax(dim=-1)
    _, exp = torch.frexp(amax)                       # floor(log2 amax) = exp - 1
    e = (exp.to(torch.int64) - 1 - 2 + 127).clamp(0, 254)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    a = mag * torch.exp2((127 - e).to(torch.float64)).unsqueeze(-1)   # exact: a power of two in fp64
    code = torch.zeros_like(a, dtype=torch.int64)
    for i, mid in enumerate(_E2M1_TIES):             # nearest; a tie goes up only to an even code; beyond 5: code 7 = 6
        code += (a > mid) | ((a == mid) & bool((i + 1) % 2 == 0))
    code |= torch.signbit(blocks).to(torch.int64) << 3
    code = code.reshape(tuple(x.shape[:-1]) + (K // 2, 2))
    packed = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)    # element 2i in the low nibble
    return packed.view(_FP4), e.to(torch.uint8)


class SparseOperator:
    def __init__(self, csr: "eng.CSR", alpha=0.3, delta=0.3, mode=eng.COMPUTE_F16, device=0, gather_mode=eng.COMPUTE_F32,
                 blocked=False, segment_blocks=0):
        if gather_mode not in (eng.COMPUTE_F16, eng.COMPUTE_BF16, eng.COMPUTE_F32):
            raise ValueError(f"gather_mode: {gather_mode!r} is not one of COMPUTE_F16, COMPUTE_BF16, COMPUTE_F32")
        if blocked and gather_mode != eng.COMPUTE_F32:
            raise ValueError("blocked=True needs gather_mode=COMPUTE_F32: the blocked SpMM has no rounding-pass form")
        if not isinstance(segment_blocks, int) or isinstance(segment_blocks, bool) or not 0 <= segment_blocks < 2 ** 32:
            raise ValueError(f"segment_blocks: {segment_blocks!r} is not an int in [0, 2^32)")
        if segment_blocks and not blocked:
            raise ValueError("segment_blocks needs blocked=True: it splits the panels of the blocked SpMM")
        self.blocked = bool(blocked)
        self.segment_blocks = segment_blocks
        self.csr = csr
        self.M, self.N, self.nnz = csr.rows, csr.cols, csr.nnz
        self.mode = mode
        self.gather_mode = gather_mode
        self.device = torch.device("cuda", device)
        self._plan = self._bw = None
        self.pipeline = eng.Pipeline(csr, alpha=alpha, delta=delta, device=-1)   # host arrays (RPHM) only
        st, plan = eng.plan_from_arrays(self.M, self.N, self.nnz, self.pipeline.arrays(), device=device)
        eng._check(st, "bsmr_plan_create")
        self._plan = plan
        self._bw = eng.backward_create(self.M, self.N, csr.row_offsets, csr.col_indices,
                                       row_order=self.pipeline.array("reorderedRows"), device=device)
        if self.blocked:
            eng.backward_attach_blocks(self._bw, self.M, self.N, self.nnz, self.pipeline.arrays(), segment_blocks)

    def __del__(self):
        if getattr(self, "_bw", None):
            eng.backward_destroy(self._bw)
            self._bw = None
        if getattr(self, "_plan", None):
            eng.plan_destroy(self._plan)
            self._plan = None

    # --- public operators ---
    def sddmm(self, A: torch.Tensor, B: torch.Tensor, B_scale=None) -> torch.Tensor:
        """P = (A B^T) at S's stored positions: A (M,K) / B (N,K), or (b,M,K) / (b,N,K); P (nnz,) or (b,nnz).
        B may be fp8 (e4m3fn / e5m2) beside an fp16 / bf16 A: no gradient reaches it.  B_scale: its MX block scales."""
        if _is4(B):
            self._no_grad8(B, "B")
            return _SDDMM4.apply(self, A, B, self._check_scale(B_scale, "B_scale", B))
        if _is8(B):
            self._no_grad8(B, "B")
            return _SDDMM8.apply(self, A, B, None if B_scale is None else self._check_scale(B_scale, "B_scale", B))
        self._no_scale(B_scale, "B_scale", "B")
        return _SDDMM.apply(self, A, B)

    def spmm(self, values: torch.Tensor, X: torch.Tensor, transpose: bool = False, out_dtype=None,
             X_scale=None) -> torch.Tensor:
        """Y = S_values X (X (N,K) -> Y (M,K)) or, transposed, S_values^T X (X (M,K) -> Y (N,K)); batched with a
        leading b on values (b,nnz) and X.  fp8 X: out_dtype (torch.float16 or torch.bfloat16) is Y's dtype and
        transpose must be False; on a blocked=True operator it takes the gather (the blocked SpMM has no fp8 form).
        X_scale: the MX block scales of an fp8 X."""
        if _is4(X):
            self._fp4_call(X, transpose, out_dtype)
            return _SpMM4.apply(self, values, X, out_dtype, self._check_scale(X_scale, "X_scale", X))
        if self._fp8_call(X, transpose, out_dtype):
            return _SpMM8.apply(self, values, X, out_dtype,
                                None if X_scale is None else self._check_scale(X_scale, "X_scale", X))
        self._no_scale(X_scale, "X_scale", "X")
        return _SpMM.apply(self, values, X, bool(transpose))

    def softmax(self, values: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
        """the softmax of scale * values over each row of S (values (nnz,) or (b, nnz) in S's CSR order): a row whose
        entries are all -inf gives zeros, a NaN or +inf makes its row NaN, rows without entries hold nothing"""
        return _Softmax.apply(self, values, scale)

    def softmax_spmm(self, values: torch.Tensor, X: torch.Tensor, scale: float = 1.0, out_dtype=None,
                     X_scale=None) -> torch.Tensor:
        """spmm(softmax(values, scale), X) in one gather (bsmr_sparse_attention): values (nnz,) or (b, nnz) fp32, X (N, K)
        or (b, N, K) in fp32, fp16 or bf16 -> Y (M, K) in X's dtype.  A row of S without entries, or whose entries are
        all -inf, gives a zero row; a NaN or +inf makes its row NaN.  fp8 X: Y in out_dtype and X_scale, the rules of spmm."""
        if _is4(X):
            self._fp4_call(X, False, out_dtype)
            return _SoftmaxSpMM4.apply(self, values, X, scale, out_dtype, self._check_scale(X_scale, "X_scale", X))
        if self._fp8_call(X, False, out_dtype):
            return _SoftmaxSpMM8.apply(self, values, X, scale, out_dtype,
                                       None if X_scale is None else self._check_scale(X_scale, "X_scale", X))
        self._no_scale(X_scale, "X_scale", "X")
        return _SoftmaxSpMM.apply(self, values, X, scale)

    def attention(self, Q: torch.Tensor, Kt: torch.Tensor, V: torch.Tensor, scale=None, fused: bool = False,
                  out_dtype=None, Kt_scale=None, V_scale=None) -> torch.Tensor:
        """spmm(softmax(sddmm(Q, Kt), scale), V): Q (M, K), Kt (N, K), V (N, Kv), or all with a leading b; K and Kv
        positive multiples of 32; scale defaults to K**-0.5.  A row of S without entries gives a zero row.
        fused=True: softmax_spmm(sddmm(Q, Kt), V, scale) - the same function in another summation order.
        Kt and V may each be fp8 or fp4; out_dtype (default Q.dtype) is the result's dtype when V is, unused otherwise.
        Kt_scale / V_scale: the MX block scales of an fp8 Kt / V, independently of each other."""
        self._no_scale(None if _is8(Kt) or _is4(Kt) else Kt_scale, "Kt_scale", "Kt")   # both refused before any device work
        self._no_scale(None if _is8(V) or _is4(V) else V_scale, "V_scale", "V")
        if _is4(V):
            self._check_scale(V_scale, "V_scale", V)   # mandatory: refused here, not behind the SDDMM
        P = self.sddmm(Q, Kt, B_scale=Kt_scale)
        if scale is None:
            scale = Q.shape[-1] ** -0.5
        out_dtype = (Q.dtype if out_dtype is None else out_dtype) if _is8(V) or _is4(V) else None
        if fused:
            return self.softmax_spmm(P, V, scale, out_dtype=out_dtype, X_scale=V_scale)
        return self.spmm(self.softmax(P, scale), V, out_dtype=out_dtype, X_scale=V_scale)

    def stats(self) -> dict:
        return eng.backward_stats(self._bw)

    # --- checks and raw calls (no autograd) ---
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    @staticmethod
    def _no_grad8(t: torch.Tensor, name: str):
        if t.requires_grad:
            raise ValueError(f"{name}: an fp8 tensor that requires grad - no gradient is computed into fp8 operands")

    @staticmethod
    def _no_scale(scale, name: str, operand: str):
        if scale is not None:
            raise ValueError(f"{name}: MX block scales belong to an fp8 {operand}, this one is not fp8")

    def _check_scale(self, sc, name: str, t8: torch.Tensor) -> torch.Tensor:
        """the MX block scales of the fp8 or fp4 operand t8 as a uint8 tensor; t8 itself is checked by the call"""
        if sc is None:
            raise ValueError(f"{name}: missing - an fp4 operand always carries MX block scales")
        if not isinstance(sc, torch.Tensor):
            raise ValueError(f"{name}: expected a torch.Tensor")
        if sc.dtype not in _SCALE_DTYPES:
            raise ValueError(f"{name}: dtype {sc.dtype}, expected torch.float8_e8m0fnu or torch.uint8")
        if sc.requires_grad:
            raise ValueError(f"{name}: a scale tensor that requires grad - no gradient is computed into scales")
        if sc.device != self.device:
            raise ValueError(f"{name}: on {sc.device}, the operator lives on {self.device}")
        want = tuple(t8.shape[:-1]) + (_k_of(t8) // MX_BLOCK,) if isinstance(t8, torch.Tensor) and t8.dim() in (2, 3) else None
        if want is None or tuple(sc.shape) != want:
            raise ValueError(f"{name}: shape {tuple(sc.shape)}, expected {want}: the operand's batch and rows, K/32 blocks")
        if not sc.is_contiguous():
            raise ValueError(f"{name}: not contiguous")
        return sc.view(torch.uint8)

    def _fp8_call(self, X, transpose, out_dtype) -> bool:
        """whether a call with X and out_dtype is the fp8 form; raises on the combinations neither form accepts"""
        if not _is8(X):
            if out_dtype is not None:
                raise ValueError("out_dtype: only an fp8 X takes it, every other X gives its own dtype")
            return False
        if out_dtype not in _MODE16:
            raise ValueError(f"out_dtype: {out_dtype!r}, an fp8 X needs torch.float16 or torch.bfloat16")
        if transpose:
            raise ValueError("transpose=True with an fp8 X: the row-side operand is never fp8")
        self._no_grad8(X, "X")
        return True

    def _fp4_call(self, X, transpose, out_dtype):
        """the rules of _fp8_call for an fp4 X"""
        if out_dtype not in _MODE16:
            raise ValueError(f"out_dtype: {out_dtype!r}, an fp4 X needs torch.float16 or torch.bfloat16")
        if transpose:
            raise ValueError("transpose=True with an fp4 X: the row-side operand is never fp4")
        self._no_grad8(X, "X")

    def _check4(self, t: torch.Tensor, name: str, rows: int, batch):
        """_check for an fp4 tensor (rows, K/2) or (b, rows, K/2): returns (b or None, K) with K in elements"""
        if not _is4(t):
            raise ValueError(f"{name}: dtype {getattr(t, 'dtype', None)}, expected torch.float4_e2m1fn_x2")
        if t.device != self.device:
            raise ValueError(f"{name}: on {t.device}, the operator lives on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: not contiguous")
        if t.dim() not in (2, 3) or t.shape[-2] != rows:
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected ({rows}, K/2) or (b, {rows}, K/2)")
        b = t.shape[0] if t.dim() == 3 else None
        if batch is not None and b != batch[0]:
            raise ValueError(f"{name}: shape {tuple(t.shape)} does not match the batch of the other operand")
        K = 2 * t.shape[-1]
        if K == 0 or K % 32:
            raise ValueError(f"{name}: K = {K} ({t.shape[-1]} bytes per row), expected a positive multiple of 32")
        if b == 0:
            raise ValueError(f"{name}: empty batch")
        if t.data_ptr() % 16:
            raise ValueError(f"{name}: data not 16-byte aligned")
        return b, K

    def _check(self, t: torch.Tensor, name: str, rows: int, batch, fp8: bool = False):
        """batch None: either (rows, K) or (b, rows, K); returns (b or None, K).  fp8: the tensor must be fp8"""
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a torch.Tensor")
        if fp8:
            if t.dtype not in _MODE8:
                raise ValueError(f"{name}: dtype {t.dtype}, expected torch.float8_e4m3fn or torch.float8_e5m2")
        elif t.dtype != torch.float32 and t.dtype not in _MODE16:
            raise ValueError(f"{name}: dtype {t.dtype}, expected torch.float32, torch.float16 or torch.bfloat16")
        if t.device != self.device:
            raise ValueError(f"{name}: on {t.device}, the operator lives on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: not contiguous")
        if t.dim() not in (2, 3) or t.shape[-2] != rows:
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected ({rows}, K) or (b, {rows}, K)")
        b = t.shape[0] if t.dim() == 3 else None
        if batch is not None and b != batch[0]:
            raise ValueError(f"{name}: shape {tuple(t.shape)} does not match the batch of the other operand")
        K = t.shape[-1]
        if K == 0 or K % 32:
            raise ValueError(f"{name}: K = {K}, expected a positive multiple of 32")
        if b == 0:
            raise ValueError(f"{name}: empty batch")
        if t.data_ptr() % 16:
            raise ValueError(f"{name}: data not 16-byte aligned")
        return b, K

    @staticmethod
    def _mode16(a: torch.Tensor, b: torch.Tensor, names: str):
        """the compute mode of a call on 16-bit operands, None for fp32 ones; the two must share a dtype"""
        if a.dtype != b.dtype:
            raise ValueError(f"{names}: dtypes {a.dtype} and {b.dtype}, the operands of one call share a dtype")
        return _MODE16.get(a.dtype)

    def _check_values(self, v: torch.Tensor, b):
        if not isinstance(v, torch.Tensor):
            raise ValueError("values: expected a torch.Tensor")
        want = (self.nnz,) if b is None else (b, self.nnz)
        if v.dtype != torch.float32 or v.device != self.device or not v.is_contiguous() or tuple(v.shape) != want:
            raise ValueError(f"values: expected a contiguous float32 tensor of shape {want} on {self.device}, got "
                             f"{v.dtype} {tuple(v.shape)} on {v.device}")

    def _sddmm(self, A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
        b, K = self._check(A, "A", self.M, None)
        _, K2 = self._check(B, "B", self.N, (b,))
        if K2 != K:
            raise ValueError(f"A and B disagree on K ({K} vs {K2})")
        mode16 = self._mode16(A, B, "A and B")
        shape = (self.nnz,) if b is None else (b, self.nnz)
        P = torch.empty(shape, dtype=torch.float32, device=self.device)
        if self.nnz == 0:
            return P
        if mode16 is not None:
            eng.sddmm_16(self._plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), b or 1, mode16, self._stream())
            return P
        if b is None:
            eng.sddmm(self._plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), self.mode, self._stream())
        else:
            eng.sddmm_batch(self._plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), b, self.mode, self._stream())
        return P

    def _spmm(self, v: torch.Tensor, X: torch.Tensor, transpose: bool) -> torch.Tensor:
        rows_x, rows_y = (self.M, self.N) if transpose else (self.N, self.M)
        b, K = self._check(X, "X", rows_x, None)
        self._check_values(v, b)
        Y = torch.empty((rows_y, K) if b is None else (b, rows_y, K), dtype=X.dtype, device=self.device)
        if self.blocked and not transpose:
            eng.spmm_blocked(self._bw, K, v.data_ptr(), X.data_ptr(), Y.data_ptr(), b or 1, self._stream(),
                             mode=_MODE16.get(X.dtype, eng.COMPUTE_F32))
            return Y
        if X.dtype in _MODE16:
            eng.spmm_16(self._bw, K, transpose, v.data_ptr(), X.data_ptr(), Y.data_ptr(), b or 1, self._stream(),
                        mode=_MODE16[X.dtype])
            return Y
        eng.spmm(self._bw, K, transpose, v.data_ptr(), X.data_ptr(), Y.data_ptr(), b or 1, self._stream(),
                 mode=self.gather_mode)
        return Y

    # --- fp8 column-side operand: the 16-bit calls on the exactly widened tensor, nothing cast or copied ---
    def _sddmm_b8(self, A: torch.Tensor, B8: torch.Tensor, Bs=None) -> torch.Tensor:
        b, K = self._check(A, "A", self.M, None)
        _, K2 = self._check(B8, "B", self.N, (b,), fp8=True)
        if A.dtype not in _MODE16:
            raise ValueError(f"A: dtype {A.dtype} beside an fp8 B, expected torch.float16 or torch.bfloat16")
        if K2 != K:
            raise ValueError(f"A and B disagree on K ({K} vs {K2})")
        P = torch.empty((self.nnz,) if b is None else (b, self.nnz), dtype=torch.float32, device=self.device)
        if self.nnz and Bs is not None:
            eng.sddmm_b8_mx(self._plan, K, A.data_ptr(), B8.data_ptr(), Bs.data_ptr(), P.data_ptr(), b or 1, _MODE16[A.dtype],
                            _MODE8[B8.dtype], self._stream())
        elif self.nnz:
            eng.sddmm_b8(self._plan, K, A.data_ptr(), B8.data_ptr(), P.data_ptr(), b or 1, _MODE16[A.dtype],
                         _MODE8[B8.dtype], self._stream())
        return P

    def _spmm_x8(self, v: torch.Tensor, X8: torch.Tensor, out_dtype, Xs=None) -> torch.Tensor:
        """Y (M, K) in out_dtype; the gather also on a blocked operator"""
        b, K = self._check(X8, "X", self.N, None, fp8=True)
        self._check_values(v, b)
        Y = torch.empty((self.M, K) if b is None else (b, self.M, K), dtype=out_dtype, device=self.device)
        if Xs is not None:
            eng.spmm_x8_mx(self._bw, K, False, v.data_ptr(), X8.data_ptr(), Xs.data_ptr(), Y.data_ptr(), b or 1,
                           self._stream(), mode=_MODE16[out_dtype], fmt=_MODE8[X8.dtype])
            return Y
        eng.spmm_x8(self._bw, K, False, v.data_ptr(), X8.data_ptr(), Y.data_ptr(), b or 1, self._stream(),
                    mode=_MODE16[out_dtype], fmt=_MODE8[X8.dtype])
        return Y

    def _attention_x8(self, v: torch.Tensor, X8: torch.Tensor, scale, out_dtype, Xs=None):
        """_attention on fp8 rows: O in out_dtype"""
        b, K = self._check(X8, "X", self.N, None, fp8=True)
        _, scale = self._softmax_args(v, scale)
        self._check_values(v, b)
        O = torch.empty((self.M, K) if b is None else (b, self.M, K), dtype=out_dtype, device=self.device)
        m = torch.empty((self.M,) if b is None else (b, self.M), dtype=torch.float32, device=self.device)
        s = torch.empty_like(m)
        if Xs is not None:
            eng.sparse_attention_x8_mx(self._bw, K, scale, v.data_ptr(), X8.data_ptr(), Xs.data_ptr(), O.data_ptr(),
                                       m.data_ptr(), s.data_ptr(), b or 1, self._stream(), mode=_MODE16[out_dtype],
                                       fmt=_MODE8[X8.dtype])
            return O, m, s
        eng.sparse_attention_x8(self._bw, K, scale, v.data_ptr(), X8.data_ptr(), O.data_ptr(), m.data_ptr(), s.data_ptr(),
                                b or 1, self._stream(), mode=_MODE16[out_dtype], fmt=_MODE8[X8.dtype])
        return O, m, s

    # --- MXFP4 column-side operand: the calls above on e2m1 codes, the scales mandatory ---
    def _sddmm_b4(self, A: torch.Tensor, B4: torch.Tensor, Bs: torch.Tensor) -> torch.Tensor:
        b, K = self._check(A, "A", self.M, None)
        _, K2 = self._check4(B4, "B", self.N, (b,))
        if A.dtype not in _MODE16:
            raise ValueError(f"A: dtype {A.dtype} beside an fp4 B, expected torch.float16 or torch.bfloat16")
        if K2 != K:
            raise ValueError(f"A and B disagree on K ({K} vs {K2})")
        P = torch.empty((self.nnz,) if b is None else (b, self.nnz), dtype=torch.float32, device=self.device)
        if self.nnz:
            eng.sddmm_b4_mx(self._plan, K, A.data_ptr(), B4.data_ptr(), Bs.data_ptr(), P.data_ptr(), b or 1, _MODE16[A.dtype],
                            self._stream())
        return P

    def _spmm_x4(self, v: torch.Tensor, X4: torch.Tensor, out_dtype, Xs: torch.Tensor) -> torch.Tensor:
        """Y (M, K) in out_dtype; the gather also on a blocked operator"""
        b, K = self._check4(X4, "X", self.N, None)
        self._check_values(v, b)
        Y = torch.empty((self.M, K) if b is None else (b, self.M, K), dtype=out_dtype, device=self.device)
        eng.spmm_x4_mx(self._bw, K, False, v.data_ptr(), X4.data_ptr(), Xs.data_ptr(), Y.data_ptr(), b or 1, self._stream(),
                       mode=_MODE16[out_dtype])
        return Y

    def _attention_x4(self, v: torch.Tensor, X4: torch.Tensor, scale, out_dtype, Xs: torch.Tensor):
        """_attention on fp4 rows: O in out_dtype"""
        b, K = self._check4(X4, "X", self.N, None)
        _, scale = self._softmax_args(v, scale)
        self._check_values(v, b)
        O = torch.empty((self.M, K) if b is None else (b, self.M, K), dtype=out_dtype, device=self.device)
        m = torch.empty((self.M,) if b is None else (b, self.M), dtype=torch.float32, device=self.device)
        s = torch.empty_like(m)
        eng.sparse_attention_x4_mx(self._bw, K, scale, v.data_ptr(), X4.data_ptr(), Xs.data_ptr(), O.data_ptr(), m.data_ptr(),
                                   s.data_ptr(), b or 1, self._stream(), mode=_MODE16[out_dtype])
        return O, m, s

    def _softmax_args(self, v: torch.Tensor, scale):
        if not isinstance(v, torch.Tensor):
            raise ValueError("values: expected a torch.Tensor")
        b = v.shape[0] if v.dim() == 2 else None
        self._check_values(v, b)
        if b == 0:
            raise ValueError("values: empty batch")
        try:
            scale = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"scale: {scale!r} is not a number") from None
        if not math.isfinite(scale):
            raise ValueError(f"scale: {scale} is not finite")
        return b, scale

    def _softmax(self, v: torch.Tensor, scale: float) -> torch.Tensor:
        b, scale = self._softmax_args(v, scale)
        Y = torch.empty_like(v)
        eng.sparse_softmax(self._bw, scale, v.data_ptr(), Y.data_ptr(), b or 1, self._stream())
        return Y

    def _softmax_backward(self, Y: torch.Tensor, dY: torch.Tensor, scale: float) -> torch.Tensor:
        b, scale = self._softmax_args(Y, scale)
        self._check_values(dY, b)
        dX = torch.empty_like(dY)
        eng.sparse_softmax_backward(self._bw, scale, Y.data_ptr(), dY.data_ptr(), dX.data_ptr(), b or 1, self._stream())
        return dX

    def _attention(self, v: torch.Tensor, X: torch.Tensor, scale):
        """(O, m, s) of the fused forward; O (M, K) or (b, M, K) in X's dtype, m and s (M,) or (b, M) fp32"""
        b, K = self._check(X, "X", self.N, None)
        _, scale = self._softmax_args(v, scale)
        self._check_values(v, b)
        O = torch.empty((self.M, K) if b is None else (b, self.M, K), dtype=X.dtype, device=self.device)
        m = torch.empty((self.M,) if b is None else (b, self.M), dtype=torch.float32, device=self.device)
        s = torch.empty_like(m)
        eng.sparse_attention(self._bw, K, scale, v.data_ptr(), X.data_ptr(), O.data_ptr(), m.data_ptr(), s.data_ptr(), b or 1,
                             self._stream(), mode=_MODE16.get(X.dtype, eng.COMPUTE_F32))
        return O, m, s

    def _attention_backward(self, v, m, s, dW, O, dO, scale):
        """(dP, W) of the fused backward; dP is written over dW (the same tensor is returned)"""
        b, K = self._check(O, "O", self.M, None)
        self._check(dO, "dO", self.M, (b,))
        if dO.shape != O.shape or dO.dtype != O.dtype:
            raise ValueError(f"dO: {dO.dtype} {tuple(dO.shape)}, expected O's {O.dtype} {tuple(O.shape)}")
        _, scale = self._softmax_args(v, scale)
        self._check_values(v, b)
        self._check_values(dW, b)
        want = (self.M,) if b is None else (b, self.M)
        for t, name in ((m, "m"), (s, "s")):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device
                    or not t.is_contiguous() or tuple(t.shape) != want):
                raise ValueError(f"{name}: expected a contiguous float32 tensor of shape {want} on {self.device}")
        W = torch.empty_like(v)
        eng.sparse_attention_backward(self._bw, K, scale, v.data_ptr(), m.data_ptr(), s.data_ptr(), dW.data_ptr(),
                                      O.data_ptr(), dO.data_ptr(), dW.data_ptr(), W.data_ptr(), b or 1, self._stream(),
                                      mode=_MODE16.get(O.dtype, eng.COMPUTE_F32))
        return dW, W

    def _sddmm_backward(self, dP, A, B, need_a: bool, need_b: bool):
        b, K = self._check(A, "A", self.M, None)
        self._check(B, "B", self.N, (b,))
        self._check_values(dP, b)
        mode16 = self._mode16(A, B, "A and B")
        dA = torch.empty_like(A) if need_a else None
        dB = torch.empty_like(B) if need_b else None
        if self.blocked and need_a:   # dA = S_dP B over the blocks; dB (the column direction) stays on the gather
            eng.spmm_blocked(self._bw, K, dP.data_ptr(), B.data_ptr(), dA.data_ptr(), b or 1, self._stream(),
                             mode=eng.COMPUTE_F32 if mode16 is None else mode16)
            need_a = False
            if not need_b:
                return dA, dB
        if mode16 is not None:
            eng.sddmm_backward_16(self._bw, K, dP.data_ptr(), A.data_ptr(), B.data_ptr(), dA.data_ptr() if need_a else None,
                                  dB.data_ptr() if need_b else None, b or 1, self._stream(), mode=mode16)
            return dA, dB
        eng.sddmm_backward(self._bw, K, dP.data_ptr(), A.data_ptr(), B.data_ptr(), dA.data_ptr() if need_a else None,
                           dB.data_ptr() if need_b else None, b or 1, self._stream(), mode=self.gather_mode)
        return dA, dB


def _grad(t: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """an incoming gradient, contiguous in `dtype` (a 16-bit gradient of a 16-bit output stays as it is: no widening)"""
    return t.to(dtype).contiguous()


class _SDDMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op: SparseOperator, A, B):
        ctx.op = op
        ctx.save_for_backward(A, B)
        return op._sddmm(A, B)

    @staticmethod
    @once_differentiable
    def backward(ctx, dP):
        op = ctx.op
        A, B = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_a or need_b):
            return None, None, None
        dA, dB = op._sddmm_backward(_grad(dP), A, B, need_a, need_b)
        return None, dA, dB


class _SDDMM8(torch.autograd.Function):
    """sddmm with an fp8 B: dA = S_dP widen(B8) in A's dtype, nothing into B; Bs: B's MX block scales, dq for widen"""
    @staticmethod
    def forward(ctx, op: SparseOperator, A, B8, Bs):
        ctx.op, ctx.Bs = op, Bs
        ctx.save_for_backward(A, B8)
        return op._sddmm_b8(A, B8, Bs)

    @staticmethod
    @once_differentiable
    def backward(ctx, dP):
        A, B8 = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        return None, ctx.op._spmm_x8(_grad(dP), B8, A.dtype, ctx.Bs), None, None


class _SDDMM4(torch.autograd.Function):
    """sddmm with an fp4 B under the block scales Bs: dA = S_dP dq(B4, Bs) in A's dtype, nothing into B or Bs"""
    @staticmethod
    def forward(ctx, op: SparseOperator, A, B4, Bs):
        ctx.op, ctx.Bs = op, Bs
        ctx.save_for_backward(A, B4)
        return op._sddmm_b4(A, B4, Bs)

    @staticmethod
    @once_differentiable
    def backward(ctx, dP):
        A, B4 = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        return None, ctx.op._spmm_x4(_grad(dP), B4, A.dtype, ctx.Bs), None, None


class _SpMM4(torch.autograd.Function):
    """spmm with an fp4 X under the block scales Xs: d values = sddmm(dY, dq(X4, Xs)), nothing into X or Xs"""
    @staticmethod
    def forward(ctx, op: SparseOperator, values, X4, out_dtype, Xs):
        ctx.op, ctx.out_dtype, ctx.Xs = op, out_dtype, Xs
        ctx.save_for_backward(X4)
        return op._spmm_x4(values, X4, out_dtype, Xs)

    @staticmethod
    @once_differentiable
    def backward(ctx, dY):
        (X4,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        return None, ctx.op._sddmm_b4(_grad(dY, ctx.out_dtype), X4, ctx.Xs), None, None, None


class _SoftmaxSpMM4(torch.autograd.Function):
    """softmax_spmm with an fp4 X under the block scales Xs: the backward of _SoftmaxSpMM without dX"""
    @staticmethod
    def forward(ctx, op: SparseOperator, values, X4, scale, out_dtype, Xs):
        O, m, s = op._attention_x4(values, X4, scale, out_dtype, Xs)
        ctx.op, ctx.scale, ctx.Xs = op, float(scale), Xs
        ctx.save_for_backward(values, X4, m, s, O)
        return O

    @staticmethod
    @once_differentiable
    def backward(ctx, dO):
        op = ctx.op
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        values, X4, m, s, O = ctx.saved_tensors
        dO = _grad(dO, O.dtype)
        dP, _ = op._attention_backward(values, m, s, op._sddmm_b4(dO, X4, ctx.Xs), O, dO, ctx.scale)
        return None, dP, None, None, None, None


class _SpMM8(torch.autograd.Function):
    """spmm with an fp8 X: d values = sddmm(dY, widen(X8)), nothing into X; Xs: X's MX block scales, dq for widen"""
    @staticmethod
    def forward(ctx, op: SparseOperator, values, X8, out_dtype, Xs):
        ctx.op, ctx.out_dtype, ctx.Xs = op, out_dtype, Xs
        ctx.save_for_backward(X8)
        return op._spmm_x8(values, X8, out_dtype, Xs)

    @staticmethod
    @once_differentiable
    def backward(ctx, dY):
        (X8,) = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        return None, ctx.op._sddmm_b8(_grad(dY, ctx.out_dtype), X8, ctx.Xs), None, None, None


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op: SparseOperator, values, X, transpose: bool):
        ctx.op, ctx.transpose = op, transpose
        ctx.save_for_backward(values, X)
        return op._spmm(values, X, transpose)

    @staticmethod
    @once_differentiable
    def backward(ctx, dY):
        op, transpose = ctx.op, ctx.transpose
        values, X = ctx.saved_tensors
        dY = _grad(dY, X.dtype)
        dv = dX = None
        if ctx.needs_input_grad[1]:
            dv = op._sddmm(X, dY) if transpose else op._sddmm(dY, X)
        if ctx.needs_input_grad[2]:
            dX = op._spmm(values, dY, not transpose)
        return None, dv, dX, None


class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op: SparseOperator, values, scale):
        Y = op._softmax(values, scale)
        ctx.op, ctx.scale = op, float(scale)
        ctx.save_for_backward(Y)
        return Y

    @staticmethod
    @once_differentiable
    def backward(ctx, dY):
        if not ctx.needs_input_grad[1]:
            return None, None, None
        (Y,) = ctx.saved_tensors
        return None, ctx.op._softmax_backward(Y, _grad(dY), ctx.scale), None


class _SoftmaxSpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op: SparseOperator, values, X, scale):
        O, m, s = op._attention(values, X, scale)
        ctx.op, ctx.scale = op, float(scale)
        ctx.save_for_backward(values, X, m, s, O)
        return O

    @staticmethod
    @once_differentiable
    def backward(ctx, dO):
        op = ctx.op
        need_v, need_x = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_v or need_x):
            return None, None, None, None
        values, X, m, s, O = ctx.saved_tensors
        dO = _grad(dO, X.dtype)
        dP, W = op._attention_backward(values, m, s, op._sddmm(dO, X), O, dO, ctx.scale)
        dX = op._spmm(W, dO, True) if need_x else None
        return None, dP if need_v else None, dX, None


class _SoftmaxSpMM8(torch.autograd.Function):
    """softmax_spmm with an fp8 X: the backward of _SoftmaxSpMM without dX; Xs: X's MX block scales"""
    @staticmethod
    def forward(ctx, op: SparseOperator, values, X8, scale, out_dtype, Xs):
        O, m, s = op._attention_x8(values, X8, scale, out_dtype, Xs)
        ctx.op, ctx.scale, ctx.Xs = op, float(scale), Xs
        ctx.save_for_backward(values, X8, m, s, O)
        return O

    @staticmethod
    @once_differentiable
    def backward(ctx, dO):
        op = ctx.op
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        values, X8, m, s, O = ctx.saved_tensors
        dO = _grad(dO, O.dtype)
        dP, _ = op._attention_backward(values, m, s, op._sddmm_b8(dO, X8, ctx.Xs), O, dO, ctx.scale)
        return None, dP, None, None, None, None


__all__ = ["SparseOperator", "mx_quantize", "mx_dequantize"]
