"""The streaming engine's kernel families on every destination encoding and group size its dispatch can reach
(csrc/bsmr_capi.hip: launchDense16, launchDenseCvt, launchDense32), where the rest of the suite reaches them by data and
by luck: denseStream (H = 1, and H = 2 in its one-wave form), denseGroups (H = 1 / 2 / 4, also with the windows staged
in LDS), denseGroupsAnyK (K = 96), denseStreamCvt / denseGroupsCvt (fp32 operands rounded in the kernel) and
denseGroupsF32 (mode 2) - on the mask form, 8-bit windows, 16-bit and 32-bit direct offsets, with 1, 3 and the default
number of blocks per work item.

Machinery of tests/test_gpu_numerics.py and tests/test_gpu_memory_contract.py: operands are signed integers in
[-127, 127] (every product and partial sum exact in fp32, exact in fp16 and bf16), the expectation is the fp64 oracle, P
lies in a guarded buffer prefilled with NaN, the comparison is ==.  No tolerance anywhere.

Every case asserts the path it meant to take as far as the C ABI shows it: bsmr_plan_dense_choice for H, the conversion
pass (Plan.converts) for pass + 16-bit kernel against in-kernel conversion, bsmr_plan_format_digest for mask form and
window / direct form, and plancheck_stream on the same arrays and options for 16- against 32-bit offsets.  The C ABI does
not say which kernel of the dispatch ran.  `runs` below PREDICTS it from the options, as a transcription of that dispatch
made when this file was written: it keeps the case tables honest (a case listed under one family whose options lead to
another fails) and labels the printed counts, but only its conversion-pass half is checked against the library; if the
dispatch changes, `runs` has to follow."""
import zlib
from collections import Counter

import numpy as np
import pytest

import synth
from rphm_desc import DIRECT16, DIRECT32, MASK, WIN8, desc_from_arrays, format_digest, stream_check
from test_gpu_memory_contract import guarded_forward
from test_gpu_numerics import Pattern, Plan, _rand_pattern, assert_exact, exact_ints, model

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EMPTY = 0xcbf29ce484222325          # FNV-1a of nothing: the array is not part of the format

# plan options of each encoding, and what plancheck_stream must report for it
ENCODINGS = {
    "mask": (dict(mask_tiles=1, output_mode=1), MASK),
    "win8": (dict(mask_tiles=0, output_mode=1), WIN8),
    "win8-lds": (dict(output_mode=2), WIN8),           # 8-bit windows assembled in LDS (denseGroups<..., LDS_STAGE>)
    "off16": (dict(output_mode=0), DIRECT16),
    "off32": (dict(force_tile32=1), DIRECT32),
}
WINDOWED = ("mask", "win8", "win8-lds")


@pytest.fixture(scope="module")
def pats(engine):
    """rand-hybrid and its all-dense twin: 9 panels (a ragged last group at H = 2 and 4), 220 = 13 * 16 + 12 columns.  The
    mask form needs an all-dense plan; with H > 1 it also needs every column shared by the panels of its group (columns
    of one panel alone are dealt round-robin behind the shared ones, out of column order): shared-dense, 72 x 100 half
    full, 4.5 panels."""
    rand = _rand_pattern()
    return {"rand-hybrid": Pattern(engine, "rand-hybrid", *rand, 0.1),
            "rand-dense": Pattern(engine, "rand-dense", *rand, 0.0),
            "shared-dense": Pattern(engine, "shared-dense", *synth.random_pattern(72, 100, 3600, seed=5), 0.0),
            "window-239": Pattern(engine, "window-239", *synth.window_pattern(239), 0.3),
            "window-240": Pattern(engine, "window-240", *synth.window_pattern(240), 0.3),
            "long-row": Pattern(engine, "long-row", *synth.long_row_pattern(65536), 0.0),
            "file-order": Pattern(engine, "file-order", *synth.file_order_rows(False), 0.1),
            "outlier-row": Pattern(engine, "outlier-row", *synth.outlier_row_pattern(), 0.3)}


@pytest.fixture(scope="module")
def refs(oracle):
    """operands and the exact result per (pattern, K), computed once: integers in [-127, 127] are fp16 and bf16 values,
    so the result is the same whether a path rounds its operands or not (asserted where it is built)"""
    made = {}

    def get(pat, K):
        key = (pat.name, K)
        if key not in made:
            rng = np.random.default_rng(zlib.crc32(f"{pat.name} {K}".encode()))
            A, B = exact_ints(rng, pat.rows, K), exact_ints(rng, pat.cols, K)
            none = np.zeros(pat.nnz, dtype=bool)
            want = model(oracle, pat, K, A, B, 2, none)
            for mode in (0, 1):
                assert np.array_equal(model(oracle, pat, K, A, B, mode, ~none), want)
            want.setflags(write=False)
            made[key] = (A, B, want)
        return made[key]
    return get


def host_report(engine, pat, opts, H, bpi):
    """plancheck_stream on the plan's arrays with the PackOptions bsmr_plan_create derives from `opts`.  (Blocks per item
    left to the plan: 2 for an ungrouped plan of fewer than 3 000 blocks, 32 for a grouped one.)"""
    d, keep = desc_from_arrays(engine, pat.rows, pat.cols, pat.nnz, pat.arrays)
    mode = opts.get("output_mode", 1)
    rc, r = stream_check(d, pat.ro, pat.ci, group=H, blocks_per_item=bpi or (2 if H == 1 else 32), wide=opts.get("force_tile32", 0),
                         staged=int(mode != 0), mask_tiles=int(mode == 1 and opts.get("mask_tiles", -1) > 0),
                         item_order=opts.get("item_order", 0), item_span=opts.get("item_span", 0), order_window=opts.get("order_window", 8192))
    assert rc == 0, (pat.name, opts, rc, r)
    return r


def runs(opts, pat, enc, H, max_blocks, K, mode):
    """The kernel a call is PREDICTED to land on - a transcription of launchDense32 / cvtInKernel / launchDenseCvt /
    launchDense16 of csrc/bsmr_capi.hip for a plan of the streaming engine with one dense format, not an observation.
    Returns (kernel, conversion pass); the second is what Plan.converts confirms."""
    if mode == 2:
        return "denseGroupsF32", False
    stream = opts.get("dense_stream", 1) != 0
    one_wave = opts.get("stream_waves", 1) != 4 and max_blocks <= 8
    cvt_serves = K in (32, 64, 128) and H == 1 and max_blocks <= 8 and enc in ("mask", "win8")
    # in-kernel conversion: asked for, or an all-dense plan with a small gather at K <= 64 that the streaming form serves
    if opts.get("convert_in_kernel", 0) == 1 or (K <= 64 and pat.delta == 0.0 and stream and cvt_serves):
        return ("denseStreamCvt" if cvt_serves and stream else "denseGroupsCvt"), False
    if K not in (32, 64, 128, 256, 512):
        return "denseGroupsAnyK", True
    if (H == 1 or (H == 2 and one_wave)) and max_blocks <= 32 and enc != "win8-lds" and stream:
        return "denseStream", True
    return "denseGroups", True


def check_case(engine, refs, pat, family, enc, H, bpi, Ks, modes, extra, counts):
    enc_opts, host_encoding = ENCODINGS[enc]
    opts = dict(fold_dense_below=0, promote_average=0, evict_wide_rows=0, dense_group=H, **enc_opts, **extra)
    if bpi:
        opts["dense_blocks_per_item"] = bpi
    where = f"{family} {enc} H={H} blocks/item={bpi or 'default'} {pat.name}"
    host = host_report(engine, pat, opts, H, bpi)
    assert host["encoding"] == host_encoding, (where, host)
    plan = Plan(engine, pat, opts)
    try:
        st = plan.plan_stats()
        assert st["num_dense_entries"] == host["dense"] > 0 and st["num_sparse_entries"] == host["residue"], (where, st, host)
        assert st["dense_work_items"] == host["items"] and st["group_size"] == H, (where, st, host)
        digest = format_digest(engine, plan.plan)
        assert digest["maskForm"] == (enc == "mask"), where
        assert (digest["winLen"] != EMPTY) == (enc in WINDOWED), where
        for K in Ks:
            A, B, want = refs(pat, K)
            for mode in modes:
                kernel, converts = runs(opts, pat, enc, H, host["max_item_blocks"], K, mode)
                assert kernel in family.split("/"), f"{where} K={K} mode={mode}: the dispatch takes {kernel}"
                got = guarded_forward(engine, plan, K, [(A, B)], mode)[0]
                assert plan.dense_group(K) == H, where
                if mode != 2:
                    assert plan.converts(K, mode) == converts, f"{where} K={K} mode={mode}: conversion pass"
                assert_exact(got, want, f"{where} K={K} mode={mode}")
                counts[(kernel + ("+lds" if enc == "win8-lds" and kernel == "denseGroups" else ""), enc, H)] += 1
    finally:
        plan.close()


def mask_pattern(pats, enc, H):
    if enc != "mask":
        return pats["rand-hybrid"]
    return pats["rand-dense"] if H == 1 else pats["shared-dense"]


def _cases(family):
    """(encoding, H, blocks per item, Ks, modes, plan options) of a family"""
    out = []
    if family == "denseStream":
        o = dict(dense_stream=1, convert_in_kernel=0, stream_waves=1)
        for enc in ("mask", "win8", "off16", "off32"):
            for bpi in (1, 3, None):
                # (an all-dense ungrouped plan with windows rounds in the kernel at K <= 64 while its items hold <= 8
                # blocks: the mask form meets denseStream at K = 32 in items of 12 blocks, the four-wave form)
                out.append((enc, 1, bpi, (512,) if enc == "mask" else (32, 512), (0, 1), o))
            for bpi in (1, 3):
                out.append((enc, 2, bpi, (32, 512), (0, 1), o))
        out.append(("mask", 1, 12, (32, 512), (0, 1), o))
        out.append(("win8", 1, 12, (32,), (0, 1), o))
        out.append(("off16", 1, 12, (32,), (0, 1), dict(o, stream_waves=4)))
    elif family == "denseGroups":
        o = dict(dense_stream=0, convert_in_kernel=0)
        for enc in ENCODINGS:
            for H in (1, 2, 4):
                for bpi in (1, 3, None):
                    out.append((enc, H, bpi, (32, 512) if bpi is None else (32,), (0, 1), o))
        # the LDS-staged form is what output_mode = 2 runs whatever dense_stream says; H = 2 in items of more than 8 blocks
        out.append(("win8-lds", 1, None, (32, 512), (0, 1), dict(convert_in_kernel=0)))
        out.append(("win8", 2, None, (32, 512), (0, 1), dict(convert_in_kernel=0)))
    elif family == "denseGroupsAnyK":
        o = dict(convert_in_kernel=0)
        for enc in ENCODINGS:
            for H in (1, 2, 4):
                for bpi in (1, 3, None):
                    out.append((enc, H, bpi, (96,), (0, 1), o))
    elif family == "denseStreamCvt/denseGroupsCvt":
        o = dict(convert_in_kernel=1)
        for enc in ENCODINGS:
            for H in (1, 2, 4):
                for bpi in (1, 3, None):
                    out.append((enc, H, bpi, (32, 128) if bpi is None or H == 1 else (32,), (0, 1), o))
        out.append(("win8", 1, 12, (32, 128), (0, 1), o))                  # items of more than 8 blocks: denseGroupsCvt
        out.append(("mask", 1, None, (32, 128), (0, 1), dict(o, dense_stream=0)))
        out.append(("mask", 1, 3, (32,), (0, 1), dict(convert_in_kernel=0)))   # the all-dense rule at K <= 64, not asked for
    elif family == "denseGroupsF32":
        for enc in ENCODINGS:
            for H in (1, 2, 4):
                for bpi in (1, 3, None):
                    out.append((enc, H, bpi, (32, 512) if bpi is None else (32,), (2,), dict()))
    return out


FAMILIES = ("denseStream", "denseGroups", "denseGroupsAnyK", "denseStreamCvt/denseGroupsCvt", "denseGroupsF32")


@pytest.mark.parametrize("family", FAMILIES)
def test_family_on_every_encoding_and_group(engine, refs, pats, family):
    counts = Counter()
    for enc, H, bpi, Ks, modes, extra in _cases(family):
        check_case(engine, refs, mask_pattern(pats, enc, H), family, enc, H, bpi, Ks, modes, extra, counts)
    for key in sorted(counts):
        print(f"predicted kernel {key[0]:<16} {key[1]:<9} H={key[2]}: {counts[key]} calls, all exact")
    kernels = {k for k, _, _ in counts}
    assert {k.split("+")[0] for k in kernels} == set(family.split("/")), kernels
    # every encoding at every group size the family has
    groups = (1, 2) if family == "denseStream" else (1, 2, 4)
    encs = [e for e in ENCODINGS if not (family == "denseStream" and e == "win8-lds")]
    for enc in encs:
        for H in groups:
            assert any(e == enc and h == H for _, e, h in counts), (family, enc, H)
    if family == "denseStreamCvt/denseGroupsCvt":
        for enc in ("mask", "win8"):                                     # the streaming form: ungrouped window tiles
            assert counts[("denseStreamCvt", enc, 1)] > 0
        for enc in ENCODINGS:                                            # the one-wave-per-item form: everything else
            assert counts[("denseGroupsCvt", enc, 4)] > 0 and (enc in ("mask", "win8") or counts[("denseGroupsCvt", enc, 1)] > 0)


@pytest.mark.parametrize("H", [1, 4])
def test_window_width_boundary_on_the_device(engine, refs, pats, H):
    """A (block, row) of 254 positions - the widest window, offset 253 the largest 8-bit offset but one - stays in window
    tiles; 255 positions fall back to 16-bit offsets, or to windows again once the outlier entries are evicted."""
    counts = Counter()
    for enc in ("win8", "win8-lds"):      # (no mask form: row 0's residue lies between its dense entries)
        for extra in (dict(dense_stream=1, convert_in_kernel=0), dict(dense_stream=0, convert_in_kernel=0), dict(convert_in_kernel=1)):
            family = "denseStreamCvt/denseGroupsCvt" if extra["convert_in_kernel"] else "denseStream/denseGroups"
            check_case(engine, refs, pats["window-239"], family + "/denseGroupsF32", enc, H, None, (32,), (0, 1, 2), extra, counts)
    pat = pats["window-240"]
    for extra in (dict(dense_stream=1, convert_in_kernel=0), dict(dense_stream=0, convert_in_kernel=0), dict(convert_in_kernel=1)):
        opts = dict(fold_dense_below=0, promote_average=0, evict_wide_rows=0, dense_group=H, **extra)
        host = host_report(engine, pat, opts, H, None)
        assert host["too_wide"] == 1 and host["encoding"] == DIRECT16, host
        plan = Plan(engine, pat, opts)
        try:
            assert format_digest(engine, plan.plan)["winLen"] == EMPTY
            A, B, want = refs(pat, 32)
            for mode in (0, 1, 2):
                assert_exact(guarded_forward(engine, plan, 32, [(A, B)], mode)[0], want, f"window-240 H={H} {extra} mode={mode}")
                assert plan.dense_group(32) == H
        finally:
            plan.close()
    if H == 1:          # (eviction serves ungrouped plans)
        plan = Plan(engine, pat, dict(fold_dense_below=0, promote_average=0, evict_wide_rows=1, dense_group=1, mask_tiles=0))
        try:
            st = plan.plan_stats()
            assert format_digest(engine, plan.plan)["winLen"] != EMPTY and 0 < st["num_dense_entries"] < 256, st
            A, B, want = refs(pat, 32)
            for mode in (0, 1, 2):
                assert_exact(guarded_forward(engine, plan, 32, [(A, B)], mode)[0], want, f"window-240 evicted mode={mode}")
        finally:
            plan.close()


def test_packer_chooses_32_bit_offsets_for_a_long_row(engine, refs, pats):
    """A row of 65 536 entries in file order: offset 65 535 from the row's first dense entry is the null value of a 16-bit
    tile, so the packer itself takes 32-bit tiles (nothing forced).  denseStream, denseGroups and denseGroupsF32 on them."""
    pat = pats["long-row"]
    for extra in (dict(dense_stream=1), dict(dense_stream=0)):
        opts = dict(fold_dense_below=0, promote_average=0, evict_wide_rows=0, dense_group=1, convert_in_kernel=0, **extra)
        host = host_report(engine, pat, opts, 1, None)
        assert host["encoding"] == DIRECT32 and host["too_wide"] == 1 and host["dense"] == pat.nnz, host
        plan = Plan(engine, pat, opts)
        try:
            digest = format_digest(engine, plan.plan)
            assert digest["winLen"] == EMPTY and digest["maskForm"] == 0
            A, B, want = refs(pat, 32)
            for mode in (0, 2):
                got = guarded_forward(engine, plan, 32, [(A, B)], mode)[0]
                assert mode == 2 or plan.converts(32, mode)
                assert_exact(got, want, f"long row {extra} mode={mode}")
        finally:
            plan.close()


@pytest.mark.parametrize("knob", ["item-order-1", "item-order-2", "item-span-64"])
def test_item_order_and_span_knobs(engine, refs, pats, monkeypatch, knob):
    """BSMR_ITEM_ORDER, BSMR_ORDER_WINDOW and BSMR_ITEM_SPAN (read by bsmr_plan_create_ex beside its options): other launch
    orders and cuts of the dense items, the per-item window arrays permuted along.  Same results; the item list is the
    one plancheck_stream accepts for the same options."""
    pat = pats["rand-hybrid"]
    opts = dict(fold_dense_below=0, promote_average=0, dense_group=1, dense_blocks_per_item=3, mask_tiles=0, convert_in_kernel=0)
    plain = Plan(engine, pat, opts)
    try:
        before = format_digest(engine, plain.plan)
    finally:
        plain.close()
    env = {"item-order-1": dict(BSMR_ITEM_ORDER="1"), "item-order-2": dict(BSMR_ITEM_ORDER="2", BSMR_ORDER_WINDOW="64"),
           "item-span-64": dict(BSMR_ITEM_SPAN="64")}[knob]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    host_opts = dict(opts, item_order=int(env.get("BSMR_ITEM_ORDER", 0)), item_span=int(env.get("BSMR_ITEM_SPAN", 0)),
                     order_window=int(env.get("BSMR_ORDER_WINDOW", 8192)))
    host = host_report(engine, pat, host_opts, 1, 3)
    plan = Plan(engine, pat, opts)
    try:
        digest = format_digest(engine, plan.plan)
        assert digest["numItems"] == host["items"] and digest["numBlocks"] == before["numBlocks"], (digest, host)
        assert digest["items"] != before["items"], "the knob must change the item list"
        assert digest["blockCols"] == before["blockCols"]
        if knob == "item-span-64":
            assert digest["numItems"] > before["numItems"]
        else:       # the same items in another order: their tiles stay, their window arrays move along
            assert digest["numItems"] == before["numItems"] and digest["tiles"] == before["tiles"]
            assert digest["rowBase"] != before["rowBase"] and digest["winLen"] != before["winLen"]
        for K in (32, 512):
            A, B, want = refs(pat, K)
            for mode in (0, 1, 2):
                assert_exact(guarded_forward(engine, plan, K, [(A, B)], mode)[0], want, f"{knob} K={K} mode={mode}")
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["window-239", "outlier-row", "window-240", "file-order"])
def test_device_packer_on_the_boundary_patterns(engine, refs, pats, name):
    """pack_on_device = 1 against 0.  The widest window and the plan the outlier pattern ends with after eviction are the
    device packer's own work: equal format digests.  A (block, row) one position wider and unsorted rows it leaves to the
    host: the plan is the host-packed one.  Either way the plan computes exactly."""
    pat = pats[name]
    accepted = name in ("window-239", "outlier-row")
    opts = dict(fold_dense_below=0, promote_average=0, dense_group=1, evict_wide_rows=1 if name == "outlier-row" else 0)
    plans = {where: Plan(engine, pat, dict(opts, pack_on_device=flag)) for where, flag in (("host", 0), ("device", 1))}
    try:
        host, device = format_digest(engine, plans["host"].plan), format_digest(engine, plans["device"].plan)
        assert host["numBlocks"] > 0 and device == host
        assert (host["winLen"] != EMPTY) == accepted
        assert plans["host"].plan_stats() == plans["device"].plan_stats()
        A, B, want = refs(pat, 32)
        for where, plan in plans.items():
            for mode in (0, 2):
                assert_exact(guarded_forward(engine, plan, 32, [(A, B)], mode)[0], want, f"{name} packed on the {where} mode={mode}")
    finally:
        for plan in plans.values():
            plan.close()
