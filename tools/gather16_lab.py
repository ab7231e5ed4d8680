#!/usr/bin/env python3
"""On an MI355X: the fp16 / bf16 gather modes of the SDDMM backward against the fp32 calls, on the four shapes of
tools/backward_lab.py, rows scheduled in the plan's clustered order.  Products: dA = S_dP B and
dB = S_dP^T A (bsmr_sddmm_backward[_mode], one output each) and Y = S_v X (bsmr_spmm[_mode], transpose 0).  Per product,
microseconds per call, best of 3 windows of 20 event-timed calls after 5 warm-up calls:
  fp32          bsmr_sddmm_backward / bsmr_spmm, with the worst of the three windows beside the best (their spread).
                --fp32-only --lib-dir DIR --label fp32_parent: only these columns, from the libraries of another build
                (the parent commit's lib/ directory) - run first, in the same session, for the fp32-did-not-move check
  f16 / bf16    the *_mode calls, conversion pass included, with 8 and with 4 elements per lane (BSMR_GATHER16_LANES)
  lowp          bsmr_spmm_lowp on rows converted beforehand (no pass), same two lane layouts
  pass          the conversion pass alone: (with pass) - (without), same layout
Usage: python tools/gather16_lab.py [--fp32-only] [--lib-dir DIR] [--label NAME] [--out FILE] [shape ...]
(one JSON line per shape)"""
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
from backward_lab import SHAPES  # noqa: E402

dev = torch.device("cuda:0")
MODES = {"f16": eng.COMPUTE_F16, "bf16": eng.COMPUTE_BF16}


def timed(fn, warmup=5, iters=20, windows=3):
    """(best, worst) window, microseconds per call"""
    s = torch.cuda.current_stream(dev)
    for _ in range(warmup):
        fn()
    got = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(iters):
            fn()
        e1.record(s)
        e1.synchronize()
        got.append(round(e0.elapsed_time(e1) * 1e3 / iters, 2))
    return min(got), max(got)


def main(names, out, fp32_only, label):
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
        dA, dB = torch.empty_like(A), torch.empty_like(B)
        line = {"shape": name, "M": rows, "N": cols, "nnz": nnz, "K": K, "gather_MB_fp32": round(nnz * K * 4 / 1e6, 1)}
        us = {}

        def products(lib, h, mode=None):
            """the three products through `lib` on handle h; mode None: the fp32 entry points"""
            tail = (1, stream()) if mode is None else (1, mode, stream())
            bwd = lib.bsmr_sddmm_backward if mode is None else lib.bsmr_sddmm_backward_mode
            spmm = lib.bsmr_spmm if mode is None else lib.bsmr_spmm_mode
            p = lambda t: t.data_ptr()
            return {"dA": lambda: bwd(h, K, p(dP), p(A), p(B), p(dA), None, *tail),
                    "dB": lambda: bwd(h, K, p(dP), p(A), p(B), None, p(dB), *tail),
                    "spmm": lambda: spmm(h, K, 0, p(dP), p(B), p(dA), *tail)}

        handles = {}
        try:
            for lanes in (8,) if fp32_only else (8, 4):
                os.environ["BSMR_GATHER16_LANES"] = str(lanes)
                handles[lanes] = eng.backward_create(rows, cols, ro, ci, order, device=0)
            os.environ.pop("BSMR_GATHER16_LANES")
            for h in handles.values():
                eng.backward_reserve(h, K, 1, **({} if fp32_only else {"mode": eng.COMPUTE_F16}))
            for key, fn in products(eng.hip(), handles[8]).items():
                assert fn() == eng.OK
                us[f"{label}_{key}"], us[f"{label}_{key}_worst_window"] = timed(fn)
            torch.cuda.synchronize()
            line["fp32_dA_crc"] = int(dA.view(torch.int32).sum(dtype=torch.int64))   # equal across builds: same bits
            for mname, mode in ({} if fp32_only else MODES).items():
                A16 = torch.empty(rows * K, dtype=torch.int16, device=dev)
                B16 = torch.empty(cols * K, dtype=torch.int16, device=dev)
                eng.convert_operands(pipe.plan, K, A.data_ptr(), B.data_ptr(), A16.data_ptr(), B16.data_ptr(), mode, stream())
                bits = {}
                for lanes, h in handles.items():
                    tag = f"{mname}_lanes{lanes}_"
                    for key, fn in products(eng.hip(), h, mode).items():
                        assert fn() == eng.OK
                        us[tag + key] = timed(fn)[0]
                    lowp = eng.hip().bsmr_spmm_lowp
                    calls = {"dA": lambda: lowp(h, K, 0, dP.data_ptr(), B16.data_ptr(), dA.data_ptr(), 1, mode, stream()),
                             "dB": lambda: lowp(h, K, 1, dP.data_ptr(), A16.data_ptr(), dB.data_ptr(), 1, mode, stream())}
                    for key, fn in calls.items():
                        assert fn() == eng.OK
                        us[tag + "lowp_" + key] = timed(fn)[0]
                        us[tag + "pass_" + key] = round(us[tag + key] - us[tag + "lowp_" + key], 2)
                    torch.cuda.synchronize()
                    bits[lanes] = (dA.clone(), dB.clone())
                line[mname + "_bits_equal_across_layouts"] = bool(torch.equal(bits[8][0], bits[4][0]) and
                                                                  torch.equal(bits[8][1], bits[4][1]))
        finally:
            for h in handles.values():
                eng.backward_destroy(h)
        line["us"] = us
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
        del pipe


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--fp32-only", action="store_true", help="only the fp32 columns (works with builds that lack the modes)")
    ap.add_argument("--lib-dir", default=None, help="load libbsmr_hip.so / libbsmr_host.so from this directory instead")
    ap.add_argument("--label", default="fp32", help="name of the fp32 columns (fp32_parent for another build)")
    ap.add_argument("shapes", nargs="*", help=f"any of {', '.join(SHAPES)} (default: all)")
    args = ap.parse_args()
    unknown = [n for n in args.shapes if n not in SHAPES]
    if unknown:
        ap.error(f"unknown shape(s) {unknown}")
    if args.lib_dir:
        eng.LIB_DIR = Path(args.lib_dir).resolve()
    if args.fp32_only:   # a build from before the modes lacks their symbols: bind only what it has
        for n in ("bsmr_spmm_mode", "bsmr_sddmm_backward_mode", "bsmr_spmm_lowp", "bsmr_backward_reserve_mode"):
            eng.HIP_SYMBOLS.pop(n)
    main(args.shapes or list(SHAPES), args.out, args.fp32_only, args.label)
