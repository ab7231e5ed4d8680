#!/usr/bin/env python3
"""On an MI355X: the calls a holder of an fp8 KV cache makes (bsmr_spmm_x8, bsmr_sparse_attention_x8, bsmr_sddmm_b8)
beside the 16-bit calls they replace, on the nips-like matrix and one row shard of the reddit-like graph (the shapes of
tools/backward_lab.py) at K = 128 and 256, rows scheduled in the plan's clustered order.
Microseconds per call: best and worst of 3 windows of 20 event-timed back-to-back calls after 5 warm-up calls; the two
sides of a comparison alternate window by window, so that what else runs on the machine meets both.
  spmm       bsmr_spmm_x8 (fp8 X, the gather widens in registers)     against  bsmr_spmm_16 on the widened copy
  attention  bsmr_sparse_attention_x8                                  against  bsmr_sparse_attention_16 on that copy
  sddmm      bsmr_sddmm_b8 (widening pass into the plan's workspace)   against  bsmr_sddmm_16 on a 16-bit B held beforehand,
             and against bsmr_widen_fp8 into a buffer of the caller's + bsmr_sddmm_16: the copy a caller makes today
Every pair is also compared bit for bit (`*_same_bits`).  No profiler runs here: these are the un-profiled numbers.
Usage: python tools/fp8_lab.py [--out FILE] [--mode f16|bf16] [--format e4m3|e5m2] [shape ...]   (one JSON line per shape and K)"""
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
import synth  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = {"nips": ("nips_like", {}), "reddit_shard": ("reddit_shard_like", {})}   # name: (generator, kwargs)
KS = (128, 256)
MODES = {"f16": (eng.COMPUTE_F16, torch.float16), "bf16": (eng.COMPUTE_BF16, torch.bfloat16)}
FORMATS = {"e4m3": (eng.FP8_E4M3, torch.float8_e4m3fn), "e5m2": (eng.FP8_E5M2, torch.float8_e5m2)}


def timed_pair(fns, warmup=5, iters=20, windows=3):
    """[(best, worst)] per function, microseconds per call; the functions take turns window by window"""
    s = torch.cuda.current_stream(dev)
    for fn in fns:
        for _ in range(warmup):
            assert fn() == eng.OK
    got = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(iters):
                fn()
            e1.record(s)
            e1.synchronize()
            got[i].append(round(e0.elapsed_time(e1) * 1e3 / iters, 2))
    return [(min(g), max(g)) for g in got]


def main(names, out, mode_name, fmt_name):
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    hip = eng.hip()
    p = lambda t: t.data_ptr()
    mode, dt = MODES[mode_name]
    fmt, f8 = FORMATS[fmt_name]
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
                X8 = (torch.from_numpy(eng.make_data(cols * K, 9)).view(cols, K) - 1).to(f8)   # cast on the CPU
                X16 = X8.to(torch.float32).to(dt).to(dev)                                # the exactly widened copy
                X8 = X8.to(dev)
                Y8, Y16 = (torch.empty(rows, K, dtype=dt, device=dev) for _ in range(2))
                m8, s8, m16, s16 = (torch.empty(rows, device=dev) for _ in range(4))
                P8, P16 = torch.empty_like(v), torch.empty_like(v)
                W16 = torch.empty_like(X16)                                              # the caller's own copy
                line = {"shape": name, "M": rows, "N": cols, "nnz": nnz, "K": K, "mode": mode_name, "format": fmt_name}
                us = {}
                eng.sparse_attention_reserve(bw, K, 1)
                pairs = {
                    "spmm": (lambda: hip.bsmr_spmm_x8(bw, K, 0, p(v), p(X8), p(Y8), 1, mode, fmt, stream()),
                             lambda: hip.bsmr_spmm_16(bw, K, 0, p(v), p(X16), p(Y16), 1, mode, stream())),
                    "attention": (lambda: hip.bsmr_sparse_attention_x8(bw, K, 0.5, p(v), p(X8), p(Y8), p(m8), p(s8), 1, mode, fmt, stream()),
                                  lambda: hip.bsmr_sparse_attention_16(bw, K, 0.5, p(v), p(X16), p(Y16), p(m16), p(s16), 1, mode, stream())),
                }
                for key, (f8call, f16call) in pairs.items():
                    (b8, w8), (b16, w16) = timed_pair([f8call, f16call])
                    us[key + "_x8"], us[key + "_x8_worst_window"] = b8, w8
                    us[key + "_16"], us[key + "_16_worst_window"] = b16, w16
                    torch.cuda.synchronize()
                    line[key + "_same_bits"] = same(Y8, Y16) and (key == "spmm" or (same(m8, m16) and same(s8, s16)))

                def copy_then_16():
                    st = hip.bsmr_widen_fp8(p(X8), p(W16), cols * K, mode, fmt, stream())
                    return st or hip.bsmr_sddmm_16(pipe.plan, K, p(A16), p(W16), p(P16), 1, mode, stream())

                got = timed_pair([lambda: hip.bsmr_sddmm_b8(pipe.plan, K, p(A16), p(X8), p(P8), 1, mode, fmt, stream()),
                                  lambda: hip.bsmr_sddmm_16(pipe.plan, K, p(A16), p(X16), p(P16), 1, mode, stream()),
                                  copy_then_16])
                for key, (b, w) in zip(("sddmm_b8", "sddmm_16", "sddmm_copy_then_16"), got):
                    us[key], us[key + "_worst_window"] = b, w
                torch.cuda.synchronize()
                line["sddmm_same_bits"] = same(P8, P16) and same(W16, X16)
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
    ap.add_argument("--mode", default="f16", choices=sorted(MODES))
    ap.add_argument("--format", default="e4m3", choices=sorted(FORMATS))
    ap.add_argument("shapes", nargs="*", help=f"any of {', '.join(SHAPES)} (default: all)")
    args = ap.parse_args()
    unknown = [n for n in args.shapes if n not in SHAPES]
    if unknown:
        ap.error(f"unknown shape(s) {unknown}")
    main(args.shapes or list(SHAPES), args.out, args.mode, args.format)
