#!/usr/bin/env python3
"""On an MI355X: the attention step of bsmr_torch.SparseOperator through its composed path (sddmm -> softmax -> spmm),
its fused path (sddmm -> softmax_spmm, bsmr_sparse_attention) and, for 16-bit operands, its one-pass path
(bsmr_sparse_attention_qkv_16), on the four shapes of tools/backward_lab.py, b = 1 and 8, fp32, fp16 and bf16 operands.
Per (shape, b, dtype):
  fwd     the part in which composed and fused differ, on given scores P: softmax + spmm (raw calls) against the fused call;
  fwdqkv  (16-bit) the whole forward from Q, Kt, V: sddmm + softmax + spmm, sddmm + fused call, the one-pass call;
  step    the whole step, forward + backward through autograd: attention(Q, Kt, V, fused= / one_pass=), and for 16-bit
          operands the one-pass step with one_pass_backward=True (bsmr_sparse_attention_qkv_backward_16) beside them;
  peak    torch.cuda.max_memory_allocated over one step of each path minus what was allocated before it, in bytes.
p_bytes is the size of the score array per batch (4 nnz): the one-pass forward neither writes nor reads it.
Microseconds per call, event timing: 3 windows of 20 calls after 5 warm-up calls; every figure is [best, worst] of its
three windows, so that a difference can be read against the windows' own spread.  The composed path runs first, both in
the same process.  `agree` is max |O_fused - O_composed| / max |O|.
--kv {fp8,mxfp8,mxfp4}: instead of the above, the forward on a quantised KV cache at K = Kv = 128, fp16 and bf16 Q: the
fused path (quantised sddmm, which first writes a 16-bit copy of Kt and then P, + the quantised fused call) against the
one-pass call on the same codes (bsmr_sparse_attention_qkv_kv8 / _kv8_mx / _kv4_mx), the fused path first.  kt16_bytes and
p_bytes are what the one-pass forward neither allocates nor moves, per batch: the 16-bit copy of Kt and the scores.
--blocks S: instead of the above, the 16-bit forward from Q, Kt, V on blocked=True operators built from the pipeline's RPHM,
attached whole (segment_blocks 0) and in segments of S blocks: the fused path, the one-pass call and the blocked one-pass
call (bsmr_sparse_attention_qkv_blocked_16) side by side in one job, K = Kv = 128, b = 1 and 8, fp16 and bf16.  coverage
is the blocks' entries / nnz: what the blocked kernel serves; the rest is the residue on the one-pass gather.
--steps: only the 16-bit step and peak columns of the first form (fused, one-pass, one-pass with its own backward).
--kv-group G [--features K]: instead of the above, the 16-bit forward with G query heads per key/value head, 1 and 2 KV
heads (b = G and 2 G), K = Kv = 128 or --features: the repeat_interleave of Kt and V on its own, the fused path and the
one-pass call on the repeated operands, and the grouped call (bsmr_sparse_attention_qkv_gqa_16) on the operands as they are
with its MFMA form (bsmr_sparse_attention_qkv_gqa_mfma_16, fwd_grouped_mfma; agree_mfma is max |O_mfma - O_grouped| / max |O|;
--mfma-only times just these two, the grouped call before and after the MFMA form);
then the backward on the forward's (O, m, s): repeat_interleave + bsmr_sparse_attention_qkv_backward_16 on b heads + the fp32
fold of dKt and dV (bwd_repeated) against bsmr_sparse_attention_qkv_gqa_backward_16 (bwd_grouped).
--kv-group G --kv FORMAT: the forward on a quantised KV cache with G query heads per key/value head, 1 and 2 KV heads, K = Kv
= 128: the repeat_interleave of codes and scales on its own, the ungrouped quantised one-pass call on the repeated codes and
scales, and the grouped call (bsmr_sparse_attention_qkv_gqa_kv8 / _kv8_mx / _kv4_mx) on the cache as it is; same_bits compares
the two.
Usage: python tools/attention_lab.py [--steps | --kv FORMAT | --blocks S | --kv-group G [--kv FORMAT]] [--out FILE] [shape ...]
(one JSON line per shape)"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "bsmr-sddmm_amd" / "python"))
sys.path.insert(0, str(REPO / "tools"))
import hostinfo  # noqa: E402

hostinfo.limit_openmp_threads()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bsmr_amd as eng  # noqa: E402
import bsmr_torch  # noqa: E402
import synth  # noqa: E402
from backward_lab import SHAPES  # noqa: E402

dev = torch.device("cuda:0")


def windows(fn, warmup=5, iters=20, count=3):
    """[best, worst] microseconds per call over `count` windows of `iters` calls"""
    s = torch.cuda.current_stream(dev)
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(iters):
            fn()
        e1.record(s)
        e1.synchronize()
        us.append(round(e0.elapsed_time(e1) * 1e3 / iters, 2))
    return [min(us), max(us)]


def peak_bytes(fn):
    """what one call of fn allocates at its peak, over what is allocated when it starts"""
    fn()
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - before


def main(names, out, steps_only=False):
    for name in names:
        gen, kwargs, K = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        lens = np.diff(ro.astype(np.int64))
        Kw = min(K, 128)
        line = {"shape": name, "M": rows, "N": cols, "nnz": int(ci.size), "K": Kw, "max_row": int(lens.max()),
                "rows_over_chunk": int((lens > 512).sum()), "p_bytes": 4 * int(ci.size)}
        op = bsmr_torch.SparseOperator(eng.CSR.from_arrays(rows, cols, ro, ci), device=0)   # the default modes
        scale = Kw ** -0.5
        us = {}
        for b in (1, 8):
            eng.sparse_attention_reserve(op._bw, Kw, b)
            for dtype, tag in ((torch.float32, "f32"), (torch.float16, "f16"), (torch.bfloat16, "bf16")):
                if steps_only and dtype == torch.float32:
                    continue
                g = torch.Generator(device=dev).manual_seed(7)
                leaf = lambda n: torch.randn(b, n, Kw, device=dev, generator=g).to(dtype).requires_grad_(True)
                Q, Kt, V = leaf(rows), leaf(cols), leaf(cols)
                H = torch.randn(b, rows, Kw, device=dev, generator=g).to(dtype)
                P = op._sddmm(Q.detach(), Kt.detach())
                Vd = V.detach()

                def step(fused, one_pass=False, one_pass_backward=False):
                    op.attention(Q, Kt, V, fused=fused, one_pass=one_pass, one_pass_backward=one_pass_backward).backward(H)
                    Q.grad = Kt.grad = V.grad = None

                key = f"b{b}_{tag}"
                if dtype != torch.float32:
                    eng.sparse_attention_qkv_backward_reserve(op._bw, Kw, Kw, b)
                    us[f"step_fused_{key}"] = windows(lambda: step(True))
                    us[f"step_one_pass_{key}"] = windows(lambda: step(False, True))
                    us[f"step_one_pass_bwd_{key}"] = windows(lambda: step(False, True, True))
                    for path, args in (("fused", (True,)), ("one_pass", (False, True)), ("one_pass_bwd", (False, True, True))):
                        line[f"peak_{path}_{key}"] = peak_bytes(lambda: step(*args))
                if steps_only:
                    del Q, Kt, V, H, P, Vd
                    continue
                us[f"fwd_composed_{key}"] = windows(lambda: op._spmm(op._softmax(P, scale), Vd, False))
                us[f"fwd_fused_{key}"] = windows(lambda: op._attention(P, Vd, scale))
                us[f"step_composed_{key}"] = windows(lambda: step(False))
                if dtype == torch.float32:
                    us[f"step_fused_{key}"] = windows(lambda: step(True))
                Oc = op._spmm(op._softmax(P, scale), Vd, False).float()
                Of = op._attention(P, Vd, scale)[0].float()
                line[f"agree_{key}"] = float((Of - Oc).abs().max() / Oc.abs().max())
                if dtype != torch.float32:   # the one-pass path beside the other two, from Q, Kt, V
                    Qd, Ktd = Q.detach(), Kt.detach()
                    us[f"fwdqkv_composed_{key}"] = windows(lambda: op._spmm(op._softmax(op._sddmm(Qd, Ktd), scale), Vd, False))
                    us[f"fwdqkv_fused_{key}"] = windows(lambda: op._attention(op._sddmm(Qd, Ktd), Vd, scale))
                    us[f"fwdqkv_one_pass_{key}"] = windows(lambda: op._attention_qkv(Qd, Ktd, Vd, scale))
                    O1 = op._attention_qkv(Qd, Ktd, Vd, scale)[0].float()
                    line[f"agree_one_pass_{key}"] = float((O1 - Oc).abs().max() / Oc.abs().max())
                    del Qd, Ktd, O1
                del Q, Kt, V, H, P, Vd, Oc, Of
        line["us"] = us
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
        del op
        torch.cuda.empty_cache()


def main_kv(names, out, kv):
    fmt = getattr(torch, "float4_e2m1fn_x2", None) if kv == "mxfp4" else torch.float8_e4m3fn
    for name in names:
        gen, kwargs, _ = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        Kw = 128
        line = {"shape": name, "kv": kv, "M": rows, "N": cols, "nnz": int(ci.size), "K": Kw, "p_bytes": 4 * int(ci.size),
                "kt16_bytes": 2 * cols * Kw, "kt_bytes": cols * Kw // (2 if kv == "mxfp4" else 1)}
        op = bsmr_torch.SparseOperator(eng.CSR.from_arrays(rows, cols, ro, ci), device=0)
        us = {}
        for b in (1, 8):
            g = torch.Generator(device=dev).manual_seed(7)
            rand = lambda n: torch.randn(b, n, Kw, device=dev, generator=g)
            quant = lambda: bsmr_torch.mx_quantize(rand(cols), fmt) if kv != "fp8" else (rand(cols).to(fmt),)
            Kt, Kts = (quant() + (None,))[:2]
            V, Vs = (quant() + (None,))[:2]
            for dtype, tag in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
                Q = rand(rows).to(dtype)
                key = f"b{b}_{tag}"
                fused = lambda: op.attention(Q, Kt, V, fused=True, Kt_scale=Kts, V_scale=Vs)
                one = lambda: op.attention(Q, Kt, V, one_pass=True, Kt_scale=Kts, V_scale=Vs)
                us[f"fwd_fused_{key}"] = windows(fused)
                us[f"fwd_one_pass_{key}"] = windows(one)
                Of = fused().float()
                line[f"agree_one_pass_{key}"] = float((one().float() - Of).abs().max() / Of.abs().max())
                del Q, Of
            del Kt, Kts, V, Vs
        line["us"] = us
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
        del op
        torch.cuda.empty_cache()


def main_blocks(names, out, S):
    for name in names:
        gen, kwargs, _ = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        Kw = 128
        scale = Kw ** -0.5
        csr = eng.CSR.from_arrays(rows, cols, ro, ci)
        ops = {seg: bsmr_torch.SparseOperator(csr, device=0, blocked=True, segment_blocks=seg) for seg in (0, S)}
        st = eng.backward_blocked_stats(ops[S]._bw)
        line = {"shape": name, "M": rows, "N": cols, "nnz": int(ci.size), "K": Kw, "blocks": st["blocks"],
                "coverage": round(st["block_entries"] / max(int(ci.size), 1), 4), "panels_with_blocks": st["panels_with_blocks"],
                "max_blocks_per_panel": st["max_blocks_per_panel"], "segments": st["segments"]}
        us = {}
        for b in (1, 8):
            for seg, op in ops.items():
                eng.sparse_attention_reserve(op._bw, Kw, b)
                eng.sparse_attention_qkv_blocked_reserve(op._bw, Kw, Kw, b)
            for dtype, tag in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
                g = torch.Generator(device=dev).manual_seed(7)
                Q, Kt, V = (torch.randn(b, n, Kw, device=dev, generator=g).to(dtype) for n in (rows, cols, cols))
                key = f"b{b}_{tag}"
                op = ops[0]
                us[f"fwd_fused_{key}"] = windows(lambda: op._attention(op._sddmm(Q, Kt), V, scale))
                us[f"fwd_one_pass_{key}"] = windows(lambda: op._attention_qkv(Q, Kt, V, scale))
                Of = op._attention(op._sddmm(Q, Kt), V, scale)[0].float()
                for seg, o in ops.items():
                    us[f"fwd_blocks_S{seg}_{key}"] = windows(lambda: o._attention_qkv(Q, Kt, V, scale, blocks=True))
                    Ob = o._attention_qkv(Q, Kt, V, scale, blocks=True)[0].float()
                    line[f"agree_blocks_S{seg}_{key}"] = float((Ob - Of).abs().max() / Of.abs().max())
                del Q, Kt, V, Of, Ob
        line["us"] = us
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
        del ops, op, o
        torch.cuda.empty_cache()


def main_gqa(names, out, g, Kw, mfma_only=False):
    for name in names:
        gen, kwargs, _ = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        scale = Kw ** -0.5
        op = bsmr_torch.SparseOperator(eng.CSR.from_arrays(rows, cols, ro, ci), device=0)
        line = {"shape": name, "M": rows, "N": cols, "nnz": int(ci.size), "K": Kw, "kv_group": g}
        us = {}
        for bk in (1, 2):
            b = bk * g
            eng.sparse_attention_reserve(op._bw, Kw, b)
            eng.sparse_attention_qkv_reserve(op._bw, Kw, Kw, b)
            for dtype, tag in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
                gen_ = torch.Generator(device=dev).manual_seed(7)
                Q, Kt, V = (torch.randn(h, n, Kw, device=dev, generator=gen_).to(dtype) for h, n in ((b, rows), (bk, cols), (bk, cols)))
                key = f"kv{bk}_{tag}"
                if mfma_only:   # the two grouped forwards alone, alternating: grouped, MFMA, grouped again
                    us[f"fwd_grouped_{key}"] = windows(lambda: op._attention_qkv_gqa(Q, Kt, V, scale, g))
                    us[f"fwd_grouped_mfma_{key}"] = windows(lambda: op._attention_qkv_gqa(Q, Kt, V, scale, g, mfma=True))
                    us[f"fwd_grouped_again_{key}"] = windows(lambda: op._attention_qkv_gqa(Q, Kt, V, scale, g))
                    Og, Om = (op._attention_qkv_gqa(Q, Kt, V, scale, g, mfma=f)[0].float() for f in (False, True))
                    line[f"agree_mfma_{key}"] = float((Om - Og).abs().max() / Og.abs().max())
                    del Q, Kt, V, Og, Om
                    continue
                us[f"repeat_{key}"] = windows(lambda: (Kt.repeat_interleave(g, 0), V.repeat_interleave(g, 0)))
                Kr, Vr = Kt.repeat_interleave(g, 0), V.repeat_interleave(g, 0)
                us[f"fwd_fused_{key}"] = windows(lambda: op._attention(op._sddmm(Q, Kr), Vr, scale))
                us[f"fwd_one_pass_{key}"] = windows(lambda: op._attention_qkv(Q, Kr, Vr, scale))
                us[f"fwd_grouped_{key}"] = windows(lambda: op._attention_qkv_gqa(Q, Kt, V, scale, g))
                us[f"fwd_grouped_mfma_{key}"] = windows(lambda: op._attention_qkv_gqa(Q, Kt, V, scale, g, mfma=True))
                same = all(torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int16),
                                       y.view(torch.int32 if y.dtype == torch.float32 else torch.int16))
                           for x, y in zip(op._attention_qkv_gqa(Q, Kt, V, scale, g), op._attention_qkv(Q, Kr, Vr, scale)))
                line[f"same_bits_{key}"] = same
                Og, Om = (op._attention_qkv_gqa(Q, Kt, V, scale, g, mfma=f)[0].float() for f in (False, True))
                line[f"agree_mfma_{key}"] = float((Om - Og).abs().max() / Og.abs().max())
                del Og, Om
                # the backward: what _AttentionOnePassGqa.backward ran before the grouped kernel (repeat, the one-pass backward
                # on b heads, the fold) against the grouped call on the operands as they are
                eng.sparse_attention_qkv_backward_reserve(op._bw, Kw, Kw, b)
                O, m, s = op._attention_qkv_gqa(Q, Kt, V, scale, g)
                H = torch.randn(b, rows, Kw, device=dev, generator=gen_).to(dtype)
                fold = lambda d, t: d.view((-1, g) + d.shape[1:]).sum(1, dtype=torch.float32).to(t.dtype)

                def repeated():
                    dQ, dKr, dVr = op._attention_qkv_backward(Q, Kt.repeat_interleave(g, 0), V.repeat_interleave(g, 0), O, H, m, s, scale)
                    return dQ, fold(dKr, Kt), fold(dVr, V)

                grouped = lambda: op._attention_qkv_backward(Q, Kt, V, O, H, m, s, scale, group=g)
                us[f"bwd_repeated_{key}"] = windows(repeated)
                us[f"bwd_grouped_{key}"] = windows(grouped)
                line[f"bwd_same_dq_bits_{key}"] = torch.equal(grouped()[0].view(torch.int16), repeated()[0].view(torch.int16))
                del Q, Kt, V, Kr, Vr, O, m, s, H
        line["us"] = us
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
        del op
        torch.cuda.empty_cache()


def main_gqa_kv(names, out, g, kv):
    fmt = getattr(torch, "float4_e2m1fn_x2", None) if kv == "mxfp4" else torch.float8_e4m3fn
    Kw = 128
    scale = Kw ** -0.5
    rep = lambda t: None if t is None else t.view(torch.uint8).repeat_interleave(g, 0).view(t.dtype)
    raw = lambda x: x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)
    for name in names:
        gen, kwargs, _ = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        op = bsmr_torch.SparseOperator(eng.CSR.from_arrays(rows, cols, ro, ci), device=0)
        line = {"shape": name, "kv": kv, "M": rows, "N": cols, "nnz": int(ci.size), "K": Kw, "kv_group": g}
        us = {}
        for bk in (1, 2):
            b = bk * g
            eng.sparse_attention_qkv_reserve(op._bw, Kw, Kw, b)
            gen_ = torch.Generator(device=dev).manual_seed(7)
            rand = lambda h, n: torch.randn(h, n, Kw, device=dev, generator=gen_)
            quant = lambda: bsmr_torch.mx_quantize(rand(bk, cols), fmt) if kv != "fp8" else (rand(bk, cols).to(fmt), None)
            (Kt, Kts), (V, Vs) = quant(), quant()
            for dtype, tag in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
                Q = rand(b, rows).to(dtype)
                key = f"kv{bk}_{tag}"
                us[f"repeat_{key}"] = windows(lambda: [rep(t) for t in (Kt, Kts, V, Vs)])
                Kr, Ksr, Vr, Vsr = (rep(t) for t in (Kt, Kts, V, Vs))
                repeated = lambda: op._attention_qkv_kv(Q, Kr, Vr, scale, Ksr, Vsr)
                grouped = lambda: op._attention_qkv_kv(Q, Kt, V, scale, Kts, Vs, group=g)
                us[f"fwd_one_pass_{key}"] = windows(repeated)
                us[f"fwd_grouped_{key}"] = windows(grouped)
                line[f"same_bits_{key}"] = all(torch.equal(raw(x), raw(y)) for x, y in zip(grouped(), repeated()))
                del Q, Kr, Ksr, Vr, Vsr
            del Kt, Kts, V, Vs
        line["us"] = us
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
        del op
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv-group", type=int, default=None, metavar="G",
                    help="time the grouped one-pass forward (G query heads per KV head) beside one-pass and fused on repeated Kt / V")
    ap.add_argument("--mfma-only", action="store_true", help="with --kv-group: only the grouped call and its MFMA form")
    ap.add_argument("--features", type=int, default=128, metavar="K", help="K = Kv of --kv-group (default 128)")
    ap.add_argument("--kv", choices=("fp8", "mxfp8", "mxfp4"), default=None,
                    help="time the forward on a quantised KV cache: fused path against one-pass")
    ap.add_argument("--blocks", type=int, default=None, metavar="S",
                    help="time the 16-bit forward over the RPHM's blocks (segment_blocks 0 and S) beside fused and one-pass")
    ap.add_argument("--steps", action="store_true", help="only the 16-bit step and peak columns of the default form")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("shapes", nargs="*", help=f"any of {', '.join(SHAPES)} (default: all)")
    args = ap.parse_args()
    unknown = [n for n in args.shapes if n not in SHAPES]
    if unknown:
        ap.error(f"unknown shape(s) {unknown}")
    if args.kv_group is not None:
        if args.blocks is not None or args.kv_group < 2 or args.features % 32 or not 32 <= args.features <= 256:
            ap.error("--kv-group takes G >= 2, K = Kv a multiple of 32 up to 256, and excludes --blocks")
        if args.kv:
            main_gqa_kv(args.shapes or list(SHAPES), args.out, args.kv_group, args.kv)
        else:
            main_gqa(args.shapes or list(SHAPES), args.out, args.kv_group, args.features, args.mfma_only)
    elif args.blocks is not None:
        if args.kv or args.blocks < 1:
            ap.error("--blocks takes S >= 1 and excludes --kv")
        main_blocks(args.shapes or list(SHAPES), args.out, args.blocks)
    elif args.kv:
        main_kv(args.shapes or list(SHAPES), args.out, args.kv)
    else:
        main(args.shapes or list(SHAPES), args.out, args.steps)
