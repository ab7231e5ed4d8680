#!/usr/bin/env python3
"""On an MI355X: the sparse row softmax (bsmr_sparse_softmax / _backward) on the four shapes of tools/backward_lab.py,
against the torch composition it replaces (scatter_reduce amax, exp, index_add, divide; its autograd backward) and
torch.sparse.softmax on a sparse COO tensor where this torch build runs it on the device; then one attention step
(SparseOperator: sddmm -> softmax -> spmm, forward + backward) with either softmax.  Microseconds per call (event
timing, best of 3 windows after warm-up) and effective GB/s over the least bytes each call must move: forward
2 * nnz * 4 * b (read x, write y), backward 3 * nnz * 4 * b (read y and dY, write dX).
Usage: python tools/softmax_lab.py [--out FILE] [--hbm-gbs 8000] [shape ...]   (one JSON line per shape)"""
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
from backward_lab import SHAPES, timed  # noqa: E402

dev = torch.device("cuda:0")


def torch_softmax(rows_t, M, P):
    """the composition callers wrote by hand before bsmr_sparse_softmax (one batch)"""
    m = torch.full((M,), float("-inf"), device=P.device).scatter_reduce(0, rows_t, P.detach(), "amax")
    e = torch.exp(P - m[rows_t])
    s = torch.zeros(M, device=P.device, dtype=P.dtype).index_add(0, rows_t, e)
    return e / s[rows_t]


def main(names, out, hbm):
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    for name in names:
        gen, kwargs, K = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        nnz = int(ci.size)
        lens = np.diff(ro.astype(np.int64))
        line = {"shape": name, "M": rows, "N": cols, "nnz": nnz, "K": K, "max_row": int(lens.max()),
                "mean_row": round(float(lens[lens > 0].mean()), 1), "rows_over_chunk": int((lens > 512).sum()),
                "hbm_GBs": hbm}
        csr = eng.CSR.from_arrays(rows, cols, ro, ci)
        op = bsmr_torch.SparseOperator(csr, mode=eng.COMPUTE_F32, device=0)
        bw = op._bw
        us, gbs, roof = {}, {}, {}
        for b in (1, 8):
            X = torch.randn(b, nnz, device=dev) * 3
            Y, dY, dX = torch.empty_like(X), torch.randn_like(X), torch.empty_like(X)
            us[f"engine_fwd_b{b}"] = timed(lambda: eng.sparse_softmax(bw, 0.5, X.data_ptr(), Y.data_ptr(), b, stream()))
            us[f"engine_bwd_b{b}"] = timed(lambda: eng.sparse_softmax_backward(bw, 0.5, Y.data_ptr(), dY.data_ptr(),
                                                                               dX.data_ptr(), b, stream()))
            for kind, nbytes in (("fwd", 2 * nnz * 4 * b), ("bwd", 3 * nnz * 4 * b)):
                key = f"engine_{kind}_b{b}"
                gbs[key] = round(nbytes / (us[key] * 1e3), 1)
                roof[key] = round(nbytes / (hbm * 1e3), 2)   # us at the HBM roofline
            del X, Y, dY, dX
        rows_t = torch.from_numpy(np.repeat(np.arange(rows), lens)).to(dev)
        x = (torch.randn(nnz, device=dev) * 3).requires_grad_(True)
        g = torch.randn(nnz, device=dev)
        us["torch_fwd"] = timed(lambda: torch_softmax(rows_t, rows, x.detach() * 0.5))
        yt = torch_softmax(rows_t, rows, x * 0.5)
        us["torch_bwd"] = timed(lambda: torch.autograd.grad(yt, x, g, retain_graph=True))
        ye = op.softmax(x, 0.5)
        line["max_abs_diff_engine_vs_torch"] = float((ye - yt).abs().max())
        try:
            idx = torch.stack([rows_t, torch.from_numpy(ci.astype(np.int64)).to(dev)])
            S = torch.sparse_coo_tensor(idx, x.detach() * 0.5, (rows, cols)).coalesce()
            us["torch_sparse_softmax_fwd"] = timed(lambda: torch.sparse.softmax(S, 1))
        except Exception as e:   # a comparison only: record why it is missing
            line["torch_sparse_softmax_error"] = f"{type(e).__name__}: {e}"[:200]
        # one attention step, forward + backward, with either softmax
        Kw = min(K, 128)
        Q = torch.randn(rows, Kw, device=dev, requires_grad=True)
        Kt = torch.randn(cols, Kw, device=dev, requires_grad=True)
        V = torch.randn(cols, Kw, device=dev, requires_grad=True)
        H = torch.randn(rows, Kw, device=dev)

        def step(engine_softmax):
            P = op.sddmm(Q, Kt)
            W = op.softmax(P, Kw ** -0.5) if engine_softmax else torch_softmax(rows_t, rows, P * Kw ** -0.5)
            (op.spmm(W, V) * H).sum().backward()

        line["attention_K"] = Kw
        us["attention_step_engine"] = timed(lambda: step(True), warmup=2, iters=5)
        us["attention_step_torch"] = timed(lambda: step(False), warmup=2, iters=5)
        line["us"], line["GBs"], line["roofline_us"] = us, gbs, roof
        line["engine_over_torch_fwd"] = round(us["engine_fwd_b1"] / us["torch_fwd"], 3)
        line["engine_over_torch_bwd"] = round(us["engine_bwd_b1"] / us["torch_bwd"], 3)
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
        del op


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth for the roofline column (GB/s)")
    ap.add_argument("shapes", nargs="*", help=f"any of {', '.join(SHAPES)} (default: all)")
    args = ap.parse_args()
    unknown = [n for n in args.shapes if n not in SHAPES]
    if unknown:
        ap.error(f"unknown shape(s) {unknown}")
    main(args.shapes or list(SHAPES), args.out, args.hbm_gbs)
