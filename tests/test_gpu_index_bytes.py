"""device_index_bytes of bsmr_plan_get_stats, bsmr_backward_get_stats and bsmr_backward_get_blocked_stats: what a handle
reports for the arrays it keeps on the device.  Every array is counted where it is uploaded and taken off again where a
format is rebuilt, so the figure is pinned here for every road that counts: the streaming format from the host packer and
from the device packer (with and without the mask form of the tiles), the formats the tiles, sweep and GEMM engines build on
their first call, a tiles format rebuilt with another item length, a backward handle and its attached blocks.

One 256 x 256 Bernoulli(0.3) pattern, rows in natural order (no clustering: the RPHM does not depend on the host's
threads), delta = 0.3: 137 dense blocks and a residue of 6 193 entries.  The mask form of the tiles exists only where every
tile row's destinations are consecutive, so its cases use the same pattern at delta = 0 (256 blocks, no residue).  No
tuner runs, so every figure is a function of the pattern."""
import ctypes as C

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M = N = 256

# device_index_bytes as the library reported them at commit c976e39 ("Blocked SpMM: split long panels into segments
# across waves"), the parent of the commit that moved every device array into DevArray - recorded by running measure()
# below on a build of that commit.
RECORDED = {
    "stream": 147826,
    "stream_after_call": 147826,
    "host_packed": 244608,
    "host_packed_mask": 138112,
    "device_packed": 244608,
    "device_packed_mask": 138112,
    "tiles_before_call": 147826,
    "tiles": 221730,
    "sweep_before_call": 147826,
    "sweep": 245058,
    "gemm_before_call": 147826,
    "gemm": 211194,
    "tiles_rebuilt_2_to_4": 219170,
    "tiles_fresh_4": 219170,
    "backward": 246520,
    "blocked_0": 203864,
    "blocked_2": 205224,
    "dense_blocks": 137,
}


class Case:
    def __init__(self, engine):
        self.engine = engine
        rows, cols, self.ro, self.ci = synth.bernoulli(rows=M, cols=N, density=0.3, seed=11)
        csr = engine.CSR.from_arrays(rows, cols, self.ro, self.ci)
        self.nnz = csr.nnz
        self.arrays = engine.Pipeline(csr, alpha=0.3, delta=0.3, row_mode=engine.ROWS_IDENTITY, device=-1).arrays()
        self.all_dense = engine.Pipeline(csr, alpha=0.3, delta=0.0, row_mode=engine.ROWS_IDENTITY, device=-1).arrays()
        self.dev = torch.device("cuda:0")
        self.operands = {}

    def plan(self, arrays=None, **options):
        e = self.engine
        base = dict(fold_dense_below=0, promote_average=0, pack_on_device=0, mask_tiles=0, evict_wide_rows=0, convert_in_kernel=0)
        base.update(options)
        st, plan = e.plan_from_arrays(M, N, self.nnz, arrays or self.arrays, device=0, options=e.plan_options(**base))
        assert st == e.OK, st
        return plan

    def stats(self, plan):
        s = self.engine.PlanStats()
        assert self.engine.hip().bsmr_plan_get_stats(plan, C.byref(s)) == self.engine.OK
        return s

    def bytes(self, plan):
        return int(self.stats(plan).device_index_bytes)

    def format(self, plan):
        """(tiles the plan keeps: those of its streaming format and of the grouped second format this all-dense pattern
        gets; 1 when the streaming format holds them in the mask form)"""
        digest = (C.c_uint64 * 13)()
        assert self.engine.hip().bsmr_plan_format_digest(plan, digest) == self.engine.OK
        s = self.stats(plan)
        return int(s.num_dense_tiles + s.grouped_dense_tiles), int(digest[12])

    def call(self, plan, K):
        if K not in self.operands:
            rng = np.random.default_rng(K)
            self.operands[K] = (torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).to(self.dev),
                                torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32)).to(self.dev),
                                torch.zeros(self.nnz, dtype=torch.float32, device=self.dev))
        A, B, P = self.operands[K]
        self.engine.sddmm(plan, K, A.data_ptr(), B.data_ptr(), P.data_ptr(), self.engine.COMPUTE_F16,
                          torch.cuda.current_stream(self.dev).cuda_stream)
        torch.cuda.synchronize()

    def tiles_choice(self, blocks_per_item):
        return {"engine": self.engine.ENGINE_TILES, "group": 1, "blocks_per_item": blocks_per_item, "format": -1, "b_only": -1,
                "overlap": -1, "cvt_in_kernel": -1, "waves": 0}


def measure(engine):
    """every figure of RECORDED, from the library that `engine` loaded"""
    e, c, out = engine, Case(engine), {}
    plan = c.plan(dense_engine=e.ENGINE_STREAM)
    out["dense_blocks"] = int(c.stats(plan).num_dense_blocks)
    out["stream"] = c.bytes(plan)
    c.call(plan, 64)
    out["stream_after_call"] = c.bytes(plan)
    e.plan_destroy(plan)
    # the streaming format from the host packer and from the device packer, tiles of 256 bytes and in the 48-byte mask form
    for name, on_device, mask in (("host_packed", 0, 0), ("host_packed_mask", 0, 1), ("device_packed", 1, 0), ("device_packed_mask", 1, 1)):
        plan = c.plan(c.all_dense, dense_engine=e.ENGINE_STREAM, pack_on_device=on_device, mask_tiles=mask)
        c.call(plan, 64)
        out[name] = c.bytes(plan)
        out[name + "_tiles"], out[name + "_form"] = c.format(plan)
        e.plan_destroy(plan)
    for name, eng, K in (("tiles", e.ENGINE_TILES, 32), ("sweep", e.ENGINE_SWEEP, 64), ("gemm", e.ENGINE_GEMM, 64)):
        plan = c.plan(dense_engine=eng)
        out[name + "_before_call"] = c.bytes(plan)
        c.call(plan, K)
        out[name] = c.bytes(plan)
        c.call(plan, K)
        out[name + "_second_call"] = c.bytes(plan)
        e.plan_destroy(plan)
    # a tiles format rebuilt with another item length (bsmr_plan_set_tuned needs a plan built with BSMR_ENGINE_TUNED)
    plan = c.plan(dense_engine=e.ENGINE_TUNED)
    e.plan_set_tuned(plan, 32, c.tiles_choice(2))
    c.call(plan, 32)
    out["tiles_built_2"] = c.bytes(plan)
    e.plan_set_tuned(plan, 32, c.tiles_choice(4))
    c.call(plan, 32)
    out["tiles_rebuilt_2_to_4"] = c.bytes(plan)
    e.plan_destroy(plan)
    plan = c.plan(dense_engine=e.ENGINE_TUNED)
    e.plan_set_tuned(plan, 32, c.tiles_choice(4))
    c.call(plan, 32)
    out["tiles_fresh_4"] = c.bytes(plan)
    e.plan_destroy(plan)
    # the backward handle and its attached blocks
    for S in (0, 2):
        bw = e.backward_create(M, N, c.ro, c.ci, row_order=c.arrays["reorderedRows"], device=0)
        out["backward"] = int(e.backward_stats(bw)["device_index_bytes"])
        e.backward_attach_blocks(bw, M, N, c.nnz, c.arrays, segment_blocks=S)
        out[f"blocked_{S}"] = int(e.backward_blocked_stats(bw)["device_index_bytes"])
        assert int(e.backward_stats(bw)["device_index_bytes"]) == out["backward"]   # (the blocks are counted on their own)
        e.backward_destroy(bw)
    return out


@pytest.fixture(scope="module")
def measured(engine):
    return measure(engine)


def test_a_rebuilt_tiles_format_is_counted_like_a_fresh_one(measured):
    """bsmr_plan_set_tuned moves a plan's tiles format from 2 to 4 blocks per item: ensureTiles drops the old arrays and
    their bytes and counts the new ones - the plan then reports what a fresh plan given 4 blocks per item reports."""
    assert measured["dense_blocks"] >= 64
    assert measured["tiles_built_2"] != measured["tiles_fresh_4"]      # (the two item lengths give different formats)
    assert measured["tiles_rebuilt_2_to_4"] == measured["tiles_fresh_4"]


def test_lazily_built_formats_are_counted_once(measured):
    for name in ("tiles", "sweep", "gemm"):
        assert measured[name] > measured[name + "_before_call"], name       # the engine's format was built by the call
        assert measured[name + "_second_call"] == measured[name], name      # ... and is not counted again
    assert measured["stream_after_call"] == measured["stream"]


def test_the_mask_form_is_counted_at_48_bytes_a_block(measured):
    for road in ("host_packed", "device_packed"):
        assert (measured[road + "_form"], measured[road + "_mask_form"]) == (0, 1), road
        print(road, measured[road + "_tiles"], measured[road + "_mask_tiles"])
        assert measured[road + "_tiles"] == measured[road + "_mask_tiles"] >= 256, road
        assert measured[road] - measured[road + "_mask"] == (256 - 48) * measured[road + "_tiles"], road


def test_device_index_bytes_are_what_they_were(measured):
    for name, want in RECORDED.items():
        print(name, measured[name], want)
    assert {name: measured[name] for name in RECORDED} == RECORDED
