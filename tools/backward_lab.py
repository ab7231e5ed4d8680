#!/usr/bin/env python3
"""On an MI355X: the SDDMM backward (bsmr_sddmm_backward) on four shapes - dA = S_dP B with the rows scheduled in natural
order and in the plan's clustered order (reordered_rows), dB = S_dP^T A with dP permuted into CSC order first (the
default) and read in place through csc_to_csr (BSMR_BACKWARD_PERMUTE=0) - against hipSPARSE on the same products
(torch.sparse_csr_tensor(...) @ X) and the forward SDDMM of the same plan.  Microseconds per call (best of 3 windows of
event-timed repetitions) and effective GB/s: (gathered rows nnz*K*4 + written rows * K*4) / time.
Usage: python tools/backward_lab.py [--out FILE] [shape ...]   (one JSON line per shape on stdout; --out appends them to
FILE as well)"""
import argparse
import json
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "bsmr-sddmm_amd" / "python"))
import hostinfo  # noqa: E402

hostinfo.limit_openmp_threads()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bsmr_amd as eng  # noqa: E402
import synth  # noqa: E402

SHAPES = {   # name: (generator, kwargs, K)
    "nips_k128": ("nips_like", {}, 128),                          # the headline shape
    "dlmc4096_k512": ("bernoulli", {}, 512),                      # BASELINE configs[4]-like: 4096^2 at 10 %
    "reddit_shard_k256": ("reddit_shard_like", {}, 256),          # one of 8 row shards of the reddit-like graph
    "mycielskian15_k128": ("mycielskian_pattern", {"k": 15}, 128),
}
dev = torch.device("cuda:0")


def timed(fn, warmup=5, iters=20, windows=3):
    s = torch.cuda.current_stream(dev)
    for _ in range(warmup):
        fn()
    best = float("inf")
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(iters):
            fn()
        e1.record(s)
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return round(best, 2)


def main(names, out):
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    for name in names:
        gen, kwargs, K = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        nnz = int(ci.size)
        csr = eng.CSR.from_arrays(rows, cols, ro, ci)
        pipe = eng.Pipeline(csr, alpha=0.3, delta=0.3, device=0)
        order = pipe.array("reorderedRows")
        dP = torch.from_numpy(eng.make_data(nnz, 7)).to(dev)
        A = torch.from_numpy(eng.make_data(rows * K, 8)).to(dev).view(rows, K)
        B = torch.from_numpy(eng.make_data(cols * K, 9)).to(dev).view(cols, K)
        dA = torch.empty_like(A)
        dB = torch.empty_like(B)
        line = {"shape": name, "M": rows, "N": cols, "nnz": nnz, "K": K}
        line["gather_MB"] = round(nnz * K * 4 / 1e6, 1)
        line["dA_source_rows_MB"] = round(np.unique(ci).size * K * 4 / 1e6, 2)   # rows of B that dA reads
        line["dB_source_rows_MB"] = round(int((np.diff(ro) > 0).sum()) * K * 4 / 1e6, 2)
        handles = {}
        try:
            handles["natural"] = eng.backward_create(rows, cols, ro, ci, None, device=0)
            handles["clustered"] = eng.backward_create(rows, cols, ro, ci, order, device=0)
            os.environ["BSMR_BACKWARD_PERMUTE"] = "0"
            handles["in_place"] = eng.backward_create(rows, cols, ro, ci, order, device=0)
            os.environ.pop("BSMR_BACKWARD_PERMUTE")
            st = eng.backward_stats(handles["clustered"])
            line["stats"] = {k: st[k] for k in ("split_rows", "split_cols", "max_row_length", "max_col_length", "permute_values")}
            for h in handles.values():
                eng.backward_reserve(h, K, 1)
            bwd = lambda h, a, b: (lambda: eng.sddmm_backward(h, K, dP.data_ptr(), A.data_ptr(), B.data_ptr(),
                                                              a and dA.data_ptr(), b and dB.data_ptr(), 1, stream()))
            us = {
                "dA_natural": timed(bwd(handles["natural"], True, False)),
                "dA_clustered": timed(bwd(handles["clustered"], True, False)),
                "dB_permuted": timed(bwd(handles["clustered"], False, True)),
                "dB_in_place": timed(bwd(handles["in_place"], False, True)),
                "both_clustered": timed(bwd(handles["clustered"], True, True)),
            }
            ref = (dA.clone(), dB.clone())
            bwd(handles["natural"], True, True)()
            torch.cuda.synchronize()
            line["bitwise_natural_vs_clustered"] = bool(torch.equal(ref[0], dA) and torch.equal(ref[1], dB))
        finally:
            for h in handles.values():
                eng.backward_destroy(h)
        # hipSPARSE through torch on the same products (S and S^T as CSR, int32 indices)
        co, csc_rows, csc_to_csr = eng.csr_transpose(rows, cols, ro, ci)
        i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
        try:
            S = torch.sparse_csr_tensor(i32(ro), i32(ci), dP, size=(rows, cols))
            ST = torch.sparse_csr_tensor(i32(co), i32(csc_rows), dP[torch.from_numpy(csc_to_csr.astype(np.int64)).to(dev)],
                                         size=(cols, rows))
            us["hipsparse_dA"] = timed(lambda: S @ B)
            us["hipsparse_dB"] = timed(lambda: ST @ A)
            line["hipsparse_max_abs_diff"] = [float((S @ B - ref[0]).abs().max()), float((ST @ A - ref[1]).abs().max())]
        except Exception as e:   # a comparison only: record why it is missing
            line["hipsparse_error"] = f"{type(e).__name__}: {e}"[:200]
        P = torch.empty(nnz, dtype=torch.float32, device=dev)
        us["forward_sddmm_f16"] = timed(lambda: eng.sddmm(pipe.plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(),
                                                          eng.COMPUTE_F16, stream()))
        line["us"] = us
        written = {"dA": rows * K * 4, "dB": cols * K * 4}
        gbs = lambda key, w: round((nnz * K * 4 + w) / (us[key] * 1e3), 1) if key in us else None
        line["GBs"] = {"dA_natural": gbs("dA_natural", written["dA"]), "dA_clustered": gbs("dA_clustered", written["dA"]),
                       "dB_in_place": gbs("dB_in_place", written["dB"]), "dB_permuted": gbs("dB_permuted", written["dB"]),
                       "hipsparse_dA": gbs("hipsparse_dA", written["dA"]), "hipsparse_dB": gbs("hipsparse_dB", written["dB"])}
        line["clustered_over_natural"] = round(us["dA_clustered"] / us["dA_natural"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
        del pipe


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("shapes", nargs="*", help=f"any of {', '.join(SHAPES)} (default: all)")
    args = ap.parse_args()
    unknown = [n for n in args.shapes if n not in SHAPES]
    if unknown:
        ap.error(f"unknown shape(s) {unknown}")
    main(args.shapes or list(SHAPES), args.out)
