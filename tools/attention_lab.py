#!/usr/bin/env python3
"""On an MI355X: the attention step of bsmr_torch.SparseOperator through its composed path (sddmm -> softmax -> spmm) and
its fused path (sddmm -> softmax_spmm, bsmr_sparse_attention), on the four shapes of tools/backward_lab.py, b = 1 and 8,
fp32 and fp16 operands.  Per (shape, b, dtype):
  fwd   the part that differs, on given scores P: softmax + spmm (raw calls) against the fused call;
  step  the whole step, forward + backward through autograd: attention(Q, Kt, V, fused=False / True).
Microseconds per call, event timing: 3 windows of 20 calls after 5 warm-up calls; every figure is [best, worst] of its
three windows, so that a difference can be read against the windows' own spread.  The composed path runs first, both in
the same process.  `agree` is max |O_fused - O_composed| / max |O|.
Usage: python tools/attention_lab.py [--out FILE] [shape ...]   (one JSON line per shape)"""
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


def main(names, out):
    for name in names:
        gen, kwargs, K = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        lens = np.diff(ro.astype(np.int64))
        Kw = min(K, 128)
        line = {"shape": name, "M": rows, "N": cols, "nnz": int(ci.size), "K": Kw, "max_row": int(lens.max()),
                "rows_over_chunk": int((lens > 512).sum())}
        op = bsmr_torch.SparseOperator(eng.CSR.from_arrays(rows, cols, ro, ci), device=0)   # the default modes
        scale = Kw ** -0.5
        us = {}
        for b in (1, 8):
            eng.sparse_attention_reserve(op._bw, Kw, b)
            for dtype, tag in ((torch.float32, "f32"), (torch.float16, "f16")):
                g = torch.Generator(device=dev).manual_seed(7)
                leaf = lambda n: torch.randn(b, n, Kw, device=dev, generator=g).to(dtype).requires_grad_(True)
                Q, Kt, V = leaf(rows), leaf(cols), leaf(cols)
                H = torch.randn(b, rows, Kw, device=dev, generator=g).to(dtype)
                P = op._sddmm(Q.detach(), Kt.detach())
                Vd = V.detach()

                def step(fused):
                    op.attention(Q, Kt, V, fused=fused).backward(H)
                    Q.grad = Kt.grad = V.grad = None

                key = f"b{b}_{tag}"
                us[f"fwd_composed_{key}"] = windows(lambda: op._spmm(op._softmax(P, scale), Vd, False))
                us[f"fwd_fused_{key}"] = windows(lambda: op._attention(P, Vd, scale))
                us[f"step_composed_{key}"] = windows(lambda: step(False))
                us[f"step_fused_{key}"] = windows(lambda: step(True))
                Oc = op._spmm(op._softmax(P, scale), Vd, False).float()
                Of = op._attention(P, Vd, scale)[0].float()
                line[f"agree_{key}"] = float((Of - Oc).abs().max() / Oc.abs().max())
                del Q, Kt, V, H, P, Vd, Oc, Of
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
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("shapes", nargs="*", help=f"any of {', '.join(SHAPES)} (default: all)")
    args = ap.parse_args()
    unknown = [n for n in args.shapes if n not in SHAPES]
    if unknown:
        ap.error(f"unknown shape(s) {unknown}")
    main(args.shapes or list(SHAPES), args.out)
