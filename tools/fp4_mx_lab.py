#!/usr/bin/env python3
"""On an MI355X: the calls a holder of an MXFP4 KV cache makes (bsmr_spmm_x4_mx, bsmr_sparse_attention_x4_mx,
bsmr_sddmm_b4_mx) beside the MXFP8 calls on the e4m3 re-encoding of the same codes under the same scales, and beside the
16-bit calls on a dequantised copy the caller already holds, on the shapes and under the protocol of tools/fp8_mx_lab.py
(DESIGN section 17): the nips-like matrix and one row shard of the reddit-like graph at K = 128 and 256; microseconds per
call, best and worst of 3 windows of 20 event-timed back-to-back calls after 5 warm-up calls, the sides of a comparison
alternating window by window.
  spmm       bsmr_spmm_x4_mx              against  bsmr_spmm_x8_mx              and  bsmr_spmm_16 on the dequantised copy
  attention  bsmr_sparse_attention_x4_mx  against  bsmr_sparse_attention_x8_mx  and  bsmr_sparse_attention_16 on that copy
  sddmm      bsmr_sddmm_b4_mx             against  bsmr_sddmm_b8_mx             and  bsmr_sddmm_16 on that copy
The tensor is made by bsmr_torch.mx_quantize(x, torch.float4_e2m1fn_x2); the default mode is bf16, in which the 16-bit copy
of the dequantised tensor is exact, so that every pair the contract says agrees is compared bit for bit in the same run:
_x4_mx against _16 on the copy (`*_x4_same_bits_as_16`) and against _x8_mx on the re-encoding (`*_x4_same_bits_as_x8`).
No profiler runs here: these are the un-profiled numbers.
Usage: python tools/fp4_mx_lab.py [--out FILE] [--mode f16|bf16] [shape ...]   (one JSON line per shape and K)"""
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
from fp8_lab import KS, MODES, SHAPES, dev, timed_pair  # noqa: E402


def main(names, out, mode_name):
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    hip = eng.hip()
    p = lambda t: t.data_ptr()
    mode, dt = MODES[mode_name]
    fmt = eng.FP8_E4M3
    same = lambda a, b: bool(torch.equal(a.view(torch.int16) if a.dtype == dt else a.view(torch.int32),
                                         b.view(torch.int16) if b.dtype == dt else b.view(torch.int32)))
    for name in names:
        gen, kwargs = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        nnz = int(ci.size)
        pipe = eng.Pipeline(eng.CSR.from_arrays(rows, cols, ro, ci), alpha=0.3, delta=0.3, device=0)
        bw = eng.backward_create(rows, cols, ro, ci, pipe.array("reorderedRows"), device=0)
        try:
            for K in KS:
                v = torch.from_numpy(eng.make_data(nnz, 7)).to(dev)                      # U[0, 2): weights and scores
                A16 = (torch.from_numpy(eng.make_data(rows * K, 8)).view(rows, K) - 1).to(dt).to(dev)
                # rows of very different magnitude, as a cache holds them: 2^-6 .. 2^6 from block to block
                X = torch.from_numpy(eng.make_data(cols * K, 9)).view(cols, K) - 1
                X = X * torch.exp2(torch.randint(-6, 7, (cols, K // 32), generator=torch.Generator().manual_seed(K))
                                   .float()).repeat_interleave(32, dim=1)
                X4, E8 = bsmr_torch.mx_quantize(X, torch.float4_e2m1fn_x2)               # on the CPU
                dq = bsmr_torch.mx_dequantize(X4, E8)
                X8 = bsmr_torch.mx_dequantize(X4, torch.full_like(E8, 127)).to(torch.float8_e4m3fn)   # the same values in e4m3
                X16 = dq.to(dt)
                copy_exact = bool(torch.equal(X16.float(), dq))
                X4, X8, E8, X16 = X4.to(dev), X8.to(dev), E8.to(dev), X16.to(dev)
                Y4, Y8, Y16 = (torch.empty(rows, K, dtype=dt, device=dev) for _ in range(3))
                m4, s4, m8, s8, m16, s16 = (torch.empty(rows, device=dev) for _ in range(6))
                P4, P8, P16 = (torch.empty_like(v) for _ in range(3))
                line = {"shape": name, "M": rows, "N": cols, "nnz": nnz, "K": K, "mode": mode_name,
                        "copy_exact": copy_exact, "scale_codes": int(E8.unique().numel())}
                us = {}
                eng.sparse_attention_reserve(bw, K, 1)
                triples = {
                    "spmm": (lambda: hip.bsmr_spmm_x4_mx(bw, K, 0, p(v), p(X4), p(E8), p(Y4), 1, mode, stream()),
                             lambda: hip.bsmr_spmm_x8_mx(bw, K, 0, p(v), p(X8), p(E8), p(Y8), 1, mode, fmt, stream()),
                             lambda: hip.bsmr_spmm_16(bw, K, 0, p(v), p(X16), p(Y16), 1, mode, stream())),
                    "attention": (lambda: hip.bsmr_sparse_attention_x4_mx(bw, K, 0.5, p(v), p(X4), p(E8), p(Y4), p(m4), p(s4), 1,
                                                                          mode, stream()),
                                  lambda: hip.bsmr_sparse_attention_x8_mx(bw, K, 0.5, p(v), p(X8), p(E8), p(Y8), p(m8), p(s8), 1,
                                                                          mode, fmt, stream()),
                                  lambda: hip.bsmr_sparse_attention_16(bw, K, 0.5, p(v), p(X16), p(Y16), p(m16), p(s16), 1,
                                                                       mode, stream())),
                    "sddmm": (lambda: hip.bsmr_sddmm_b4_mx(pipe.plan, K, p(A16), p(X4), p(E8), p(P4), 1, mode, stream()),
                              lambda: hip.bsmr_sddmm_b8_mx(pipe.plan, K, p(A16), p(X8), p(E8), p(P8), 1, mode, fmt, stream()),
                              lambda: hip.bsmr_sddmm_16(pipe.plan, K, p(A16), p(X16), p(P16), 1, mode, stream())),
                }
                for key, calls in triples.items():
                    for tag, (b, w) in zip(("_x4", "_x8", "_16"), timed_pair(list(calls))):
                        us[key + tag], us[key + tag + "_worst_window"] = b, w
                    torch.cuda.synchronize()
                    if key == "sddmm":
                        line[key + "_x4_same_bits_as_16"] = same(P4, P16)
                        line[key + "_x4_same_bits_as_x8"] = same(P4, P8)
                    else:
                        extra = key == "attention"
                        line[key + "_x4_same_bits_as_16"] = same(Y4, Y16) and (not extra or (same(m4, m16) and same(s4, s16)))
                        line[key + "_x4_same_bits_as_x8"] = same(Y4, Y8) and (not extra or (same(m4, m8) and same(s4, s8)))
                line["us"] = us
                text = json.dumps(line)
                print(text, flush=True)
                if out:
                    with open(out, "a") as f:
                        f.write(text + "\n")
        finally:
            eng.backward_destroy(bw)
        del pipe


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--mode", default="bf16", choices=sorted(MODES))
    ap.add_argument("shapes", nargs="*", help=f"any of {', '.join(SHAPES)} (default: all)")
    args = ap.parse_args()
    unknown = [n for n in args.shapes if n not in SHAPES]
    if unknown:
        ap.error(f"unknown shape(s) {unknown}")
    main(args.shapes or list(SHAPES), args.out, args.mode)
