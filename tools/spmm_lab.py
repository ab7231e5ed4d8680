#!/usr/bin/env python3
"""On an MI355X: Y = S_v X through the gather (bsmr_spmm / bsmr_spmm_16) and through the blocked form
(bsmr_spmm_blocked / _16: the RPHM's dense 16 x 16 blocks on the fp32 MFMA + the gather over the residue) at several
segment_blocks = S (bsmr_backward_attach_blocks_split; 0 = no panel splitting), and dA of the SDDMM backward through the
gather (bsmr_sddmm_backward[_16] with dB = NULL; its blocked form is the very call timed as `spmm_blocked`, on (dP, B)),
on the four shapes of tools/backward_lab.py at K = 128, b = 1 and 8, fp32 and fp16 rows.
Microseconds per call, event timing: 3 windows of 20 calls after 5 warm-up calls; every figure is [best, worst] of its
three windows, so that a difference can be read against the windows' own spread.  One handle per S, all in one process; the
gather runs first, then the values of S interleaved window by window (window 1 of every S, then window 2, ...), so that a
drift of the machine does not favour one of them: the baseline is the gather of the same build.  Per shape also what
decides the outcome: the block fill, the share of entries that lie in blocks, max_blocks_per_panel, the bytes of the
blocked device format, and per S the work units (`segments`), the longest serial loop (`max_blocks_per_segment`) and the
bytes of the segment partials per batch at this K.
`agree` is max |Y_blocked - Y_gather| / max |Y_gather|.
Usage: python tools/spmm_lab.py [--out FILE] [--segment-blocks S ...] [shape ...]   (one JSON line per shape)"""
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
SEGMENT_BLOCKS = (0, 4, 8, 16, 32, 64)


def interleaved(fns, warmup=5, iters=20, count=3):
    """attention_lab.windows for several calls at once: {key: [best, worst]} microseconds per call, window w of every call
    before window w + 1 of any"""
    s = torch.cuda.current_stream(dev)
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    us = {k: [] for k in fns}
    for _ in range(count):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(iters):
                fn()
            e1.record(s)
            e1.synchronize()
            us[k].append(round(e0.elapsed_time(e1) * 1e3 / iters, 2))
    return {k: [min(u), max(u)] for k, u in us.items()}


def main(names, out, segment_blocks):
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    for name in names:
        gen, kwargs, _ = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        nnz = int(ci.size)
        arrays = eng.Pipeline(eng.CSR.from_arrays(rows, cols, ro, ci), alpha=0.3, delta=0.3, device=-1).arrays()
        handles = {}
        try:
            for S in segment_blocks:
                handles[S] = eng.backward_create(rows, cols, ro, ci, arrays["reorderedRows"], device=0)
                eng.backward_attach_blocks(handles[S], rows, cols, nnz, arrays, segment_blocks=S)
            bw = handles[segment_blocks[0]]          # the gather's handle: attached blocks leave it untouched
            st = eng.backward_blocked_stats(bw)
            line = {"shape": name, "M": rows, "N": cols, "nnz": nnz, "K": K, "blocks": st["blocks"],
                    "fill": round(st["block_entries"] / (256 * st["blocks"]), 4) if st["blocks"] else None,
                    "share_in_blocks": round(st["block_entries"] / max(nnz, 1), 4),
                    "max_blocks_per_panel": st["max_blocks_per_panel"], "panels_with_blocks": st["panels_with_blocks"],
                    "panels": st["panels"], "max_residue_row": st["max_residue_row"], "per_S": {}}
            for S, h in handles.items():
                s = eng.backward_blocked_stats(h)
                split_segments = s["segments"] - (s["panels_with_blocks"] - s["split_panels"])
                line["per_S"][str(S)] = {"segments": s["segments"], "split_panels": s["split_panels"],
                                         "max_blocks_per_segment": s["max_blocks_per_segment"],
                                         "partial_bytes_per_batch": 16 * split_segments * K * 4,
                                         "blocked_index_MB": round(s["device_index_bytes"] / 1e6, 2)}
            us = {}
            for b in (1, 8):
                for h in handles.values():
                    eng.backward_reserve(h, K, b)
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
                    blocked = {S: (lambda h=h: eng.spmm_blocked(h, K, p(v), p(X), p(Yb), b, stream(), mode=mode))
                               for S, h in handles.items()}
                    key = f"b{b}_{tag}"
                    us[f"dA_gather_{key}"] = windows(dA_gather)
                    us[f"spmm_gather_{key}"] = windows(gather)       # last: Yg holds Y for `agree`
                    for S, w in interleaved(blocked).items():
                        us[f"spmm_blocked_S{S}_{key}"] = w
                    scale = Yg.float().abs().max()
                    for S, fn in blocked.items():
                        fn()
                        torch.cuda.synchronize()
                        line["per_S"][str(S)][f"agree_{key}"] = float((Yb.float() - Yg.float()).abs().max() / scale)
                    del v, X, A, Yg, Yb
            line["us"] = us
            # the rule of DESIGN 13 / 14: faster only where the worst window lies below the gather's best
            line["blocked_faster"] = {
                k[len("spmm_gather_"):]: [S for S in handles if us[f"spmm_blocked_S{S}_" + k[len("spmm_gather_"):]][1] < us[k][0]]
                for k in us if k.startswith("spmm_gather_")}
            line["best_S"] = {
                k[len("spmm_gather_"):]: min(handles, key=lambda S: us[f"spmm_blocked_S{S}_" + k[len("spmm_gather_"):]][1])
                for k in us if k.startswith("spmm_gather_")}
        finally:
            for h in handles.values():
                eng.backward_destroy(h)
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--segment-blocks", type=int, nargs="+", default=list(SEGMENT_BLOCKS), metavar="S",
                    help="the segment_blocks values to attach, one handle each (0: no panel splitting)")
    ap.add_argument("shapes", nargs="*", help=f"any of {', '.join(SHAPES)} (default: all)")
    args = ap.parse_args()
    unknown = [n for n in args.shapes if n not in SHAPES]
    if unknown:
        ap.error(f"unknown shape(s) {unknown}")
    if any(S < 0 for S in args.segment_blocks) or len(set(args.segment_blocks)) != len(args.segment_blocks):
        ap.error("--segment-blocks: distinct values >= 0")
    main(args.shapes or list(SHAPES), args.out, args.segment_blocks)
