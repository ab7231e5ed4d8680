#!/usr/bin/env python3
"""On an MI355X: the calls a holder of fp16 / bf16 tensors makes (bsmr_spmm_16, bsmr_sddmm_backward_16, bsmr_sddmm_16)
beside what they replace, on the four shapes of tools/backward_lab.py (DESIGN sections 9 and 11), rows scheduled in the
plan's clustered order.  Products: dA = S_dP B, dB = S_dP^T A (one output each) and the forward P.  Microseconds per
call, best of 3 windows of 20 event-timed calls after 5 warm-up calls; for every `lowp` column also the worst window
(that call's own spread: a `16` column above it by more than that is a finding).
  fp32          bsmr_sddmm_backward / bsmr_sddmm on fp32 operands, best and worst window
  f16 / bf16    per format:
    mode        bsmr_sddmm_backward_mode / bsmr_sddmm: fp32 in, the engine rounds (pass included), fp32 out - what a
                16-bit caller pays today, minus its torch casts
    lowp        bsmr_spmm_lowp / bsmr_sddmm_lowp on 16-bit copies made beforehand: the same gather, fp32 output, no pass
    16          bsmr_spmm_16 (through bsmr_sddmm_backward_16) / bsmr_sddmm_16: 16-bit in, 16-bit dA / dB out
--parent --lib-dir DIR: the fp32, mode and lowp columns only, from the libraries of another build (the parent commit's
lib/ directory), under the prefix parent_ - run first, in the same session, for the nothing-moved check.
Usage: python tools/io16_lab.py [--parent] [--lib-dir DIR] [--out FILE] [shape ...]   (one JSON line per shape)"""
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
from backward_lab import SHAPES  # noqa: E402
from gather16_lab import timed  # noqa: E402

dev = torch.device("cuda:0")
MODES = {"f16": eng.COMPUTE_F16, "bf16": eng.COMPUTE_BF16}
NEW = ("bsmr_sddmm_16", "bsmr_spmm_16", "bsmr_sddmm_backward_16")


def main(names, out, parent):
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream
    hip = eng.hip()
    pre = "parent_" if parent else ""
    p = lambda t: t.data_ptr()
    for name in names:
        gen, kwargs, K = SHAPES[name]
        rows, cols, ro, ci = getattr(synth, gen)(**kwargs)
        ro = np.ascontiguousarray(ro, dtype=np.uint32)
        ci = np.ascontiguousarray(ci, dtype=np.uint32)
        nnz = int(ci.size)
        pipe = eng.Pipeline(eng.CSR.from_arrays(rows, cols, ro, ci), alpha=0.3, delta=0.3, device=0)
        bw = eng.backward_create(rows, cols, ro, ci, pipe.array("reorderedRows"), device=0)
        dP = torch.from_numpy(eng.make_data(nnz, 7)).to(dev)
        A = torch.from_numpy(eng.make_data(rows * K, 8)).to(dev).view(rows, K)
        B = torch.from_numpy(eng.make_data(cols * K, 9)).to(dev).view(cols, K)
        dA, dB, P = torch.empty_like(A), torch.empty_like(B), torch.empty_like(dP)
        line = {"shape": name, "M": rows, "N": cols, "nnz": nnz, "K": K}
        us = {}

        def record(key, fn, spread=False):
            assert fn() == eng.OK, key
            best, worst = timed(fn)
            us[pre + key] = best
            if spread:
                us[pre + key + "_worst_window"] = worst

        try:
            eng.backward_reserve(bw, K, 1, mode=eng.COMPUTE_F16)
            assert hip.bsmr_plan_reserve(pipe.plan, K) == eng.OK
            record("fp32_dA", lambda: hip.bsmr_sddmm_backward(bw, K, p(dP), p(A), p(B), p(dA), None, 1, stream()), True)
            record("fp32_dB", lambda: hip.bsmr_sddmm_backward(bw, K, p(dP), p(A), p(B), None, p(dB), 1, stream()), True)
            record("fp32_P", lambda: hip.bsmr_sddmm(pipe.plan, K, p(A), p(B), p(P), eng.COMPUTE_F32, stream()), True)
            torch.cuda.synchronize()
            line[pre + "fp32_dA_crc"] = int(dA.view(torch.int32).sum(dtype=torch.int64))   # equal across builds: same bits
            for m, mode in MODES.items():
                dt = torch.float16 if mode == eng.COMPUTE_F16 else torch.bfloat16
                A16, B16 = torch.empty(rows, K, dtype=dt, device=dev), torch.empty(cols, K, dtype=dt, device=dev)
                eng.convert_operands(pipe.plan, K, p(A), p(B), p(A16), p(B16), mode, stream())
                record(m + "_mode_dA", lambda: hip.bsmr_sddmm_backward_mode(bw, K, p(dP), p(A), p(B), p(dA), None, 1, mode, stream()))
                record(m + "_mode_dB", lambda: hip.bsmr_sddmm_backward_mode(bw, K, p(dP), p(A), p(B), None, p(dB), 1, mode, stream()))
                record(m + "_mode_P", lambda: hip.bsmr_sddmm(pipe.plan, K, p(A), p(B), p(P), mode, stream()))
                record(m + "_lowp_dA", lambda: hip.bsmr_spmm_lowp(bw, K, 0, p(dP), p(B16), p(dA), 1, mode, stream()), True)
                record(m + "_lowp_dB", lambda: hip.bsmr_spmm_lowp(bw, K, 1, p(dP), p(A16), p(dB), 1, mode, stream()), True)
                record(m + "_lowp_P", lambda: hip.bsmr_sddmm_lowp(pipe.plan, K, p(A16), p(B16), p(A), p(B), p(P), mode, stream()), True)
                torch.cuda.synchronize()
                line[pre + m + "_lowp_dA_crc"] = int(dA.view(torch.int32).sum(dtype=torch.int64))
                if parent:
                    continue
                dA16, dB16 = torch.empty_like(A16), torch.empty_like(B16)
                record(m + "_16_dA", lambda: hip.bsmr_sddmm_backward_16(bw, K, p(dP), p(A16), p(B16), p(dA16), None, 1, mode, stream()))
                record(m + "_16_dB", lambda: hip.bsmr_sddmm_backward_16(bw, K, p(dP), p(A16), p(B16), None, p(dB16), 1, mode, stream()))
                record(m + "_16_P", lambda: hip.bsmr_sddmm_16(pipe.plan, K, p(A16), p(B16), p(P), 1, mode, stream()))
                torch.cuda.synchronize()
                # the 16-bit outputs are the fp32 outputs of the lowp calls (still in dA / dB), cast once
                line[m + "_16_is_rounded_lowp"] = bool(torch.equal(dA16, dA.to(dt)) and torch.equal(dB16, dB.to(dt)))
        finally:
            eng.backward_destroy(bw)
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
    ap.add_argument("--parent", action="store_true", help="a build from before the 16-bit entry points: fp32, mode and lowp columns only")
    ap.add_argument("--lib-dir", default=None, help="load libbsmr_hip.so / libbsmr_host.so from this directory instead")
    ap.add_argument("shapes", nargs="*", help=f"any of {', '.join(SHAPES)} (default: all)")
    args = ap.parse_args()
    unknown = [n for n in args.shapes if n not in SHAPES]
    if unknown:
        ap.error(f"unknown shape(s) {unknown}")
    if args.lib_dir:
        eng.LIB_DIR = Path(args.lib_dir).resolve()
    if args.parent:   # that build lacks the new symbols: bind only what it has
        for n in NEW:
            eng.HIP_SYMBOLS.pop(n)
    main(args.shapes or list(SHAPES), args.out, args.parent)
