#!/usr/bin/env python3
"""On an MI355X: Y = S_v X through the gather (bsmr_spmm / bsmr_spmm_16) and through the blocked form
(bsmr_spmm_blocked / _16: the RPHM's dense 16 x 16 blocks on the fp32 MFMA + the gather over the residue), and dA of the
SDDMM backward both ways (bsmr_sddmm_backward[_16] with dB = NULL against the blocked call on (dP, B)), on the four shapes
of tools/backward_lab.py at K = 128, b = 1 and 8, fp32 and fp16 rows.
Microseconds per call, event timing: 3 windows of 20 calls after 5 warm-up calls; every figure is [best, worst] of its
three windows, so that a difference can be read against the windows' own spread.  The gather runs first, both on one
handle in one process: the baseline is the gather of the same build.  Per shape also what decides the outcome: the block
fill, the share of entries that lie in blocks, max_blocks_per_panel and the bytes of the blocked device format.
`agree` is max |Y_blocked - Y_gather| / max |Y_gather|.
Usage: python tools/spmm_lab.py [--out FILE] [shape ...]   (one JSON line per shape)"""
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
from attention_lab import windows  # noqa: E402
from backward_lab import SHAPES  # noqa: E402

dev = torch.device("cuda:0")
K = 128


def main(names, out):
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    for name in names:
        gen, kwargs, _ = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        nnz = int(ci.size)
        arrays = eng.Pipeline(eng.CSR.from_arrays(rows, cols, ro, ci), alpha=0.3, delta=0.3, device=-1).arrays()
        bw = eng.backward_create(rows, cols, ro, ci, arrays["reorderedRows"], device=0)
        try:
            eng.backward_attach_blocks(bw, rows, cols, nnz, arrays)
            st = eng.backward_blocked_stats(bw)
            line = {"shape": name, "M": rows, "N": cols, "nnz": nnz, "K": K, "blocks": st["blocks"],
                    "fill": round(st["block_entries"] / (256 * st["blocks"]), 4) if st["blocks"] else None,
                    "share_in_blocks": round(st["block_entries"] / max(nnz, 1), 4),
                    "max_blocks_per_panel": st["max_blocks_per_panel"], "panels_with_blocks": st["panels_with_blocks"],
                    "panels": st["panels"], "max_residue_row": st["max_residue_row"],
                    "blocked_index_MB": round(st["device_index_bytes"] / 1e6, 2)}
            us = {}
            for b in (1, 8):
                eng.backward_reserve(bw, K, b)
                for dtype, tag, mode in ((torch.float32, "f32", eng.COMPUTE_F32), (torch.float16, "f16", eng.COMPUTE_F16)):
                    g = torch.Generator(device=dev).manual_seed(7)
                    v = torch.randn(b, nnz, device=dev, generator=g)
                    X = torch.randn(b, cols, K, device=dev, generator=g).to(dtype)
                    A = torch.randn(b, rows, K, device=dev, generator=g).to(dtype)
                    Yg, Yb = torch.empty(b, rows, K, device=dev, dtype=dtype), torch.empty(b, rows, K, device=dev, dtype=dtype)
                    p = lambda t: t.data_ptr()
                    if mode == eng.COMPUTE_F32:
                        gather = lambda: eng.spmm(bw, K, False, p(v), p(X), p(Yg), b, stream())
                        dA_gather = lambda: eng.sddmm_backward(bw, K, p(v), p(A), p(X), p(Yg), None, b, stream())
                    else:
                        gather = lambda: eng.spmm_16(bw, K, False, p(v), p(X), p(Yg), b, stream(), mode=mode)
                        dA_gather = lambda: eng.sddmm_backward_16(bw, K, p(v), p(A), p(X), p(Yg), None, b, stream(), mode=mode)
                    blocked = lambda: eng.spmm_blocked(bw, K, p(v), p(X), p(Yb), b, stream(), mode=mode)
                    key = f"b{b}_{tag}"
                    us[f"spmm_gather_{key}"] = windows(gather)
                    us[f"spmm_blocked_{key}"] = windows(blocked)
                    us[f"dA_gather_{key}"] = windows(dA_gather)
                    us[f"dA_blocked_{key}"] = windows(blocked)
                    torch.cuda.synchronize()
                    line[f"agree_{key}"] = float((Yb.float() - Yg.float()).abs().max() / Yg.float().abs().max())
                    del v, X, A, Yg, Yb
            line["us"] = us
            line["blocked_faster"] = sorted(k[len("spmm_gather_"):] for k in us if k.startswith("spmm_gather_")
                                            and us["spmm_blocked_" + k[len("spmm_gather_"):]][1] < us[k][0])
        finally:
            eng.backward_destroy(bw)
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
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
