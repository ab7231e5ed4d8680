"""The layering of the device sources: helper headers define no kernel, no unit renames the namespace, and the
one-pass attention units reach helpers only - never a header that defines kernels of another unit."""
import re
from pathlib import Path

PKG = Path(__file__).resolve().parent.parent / "bsmr-sddmm_amd"
CSRC = PKG / "csrc"
HELPERS = ["lowp_device.hpp", "backward_lists.hpp", "softmax_device.hpp", "quant_device.hpp", "blocked_format.hpp",
           "attention_qkv_dispatch.hpp", "attention_qkv_launch.hpp"]
KERNEL_HEADERS = {"attention_kernels.hpp", "softmax_kernels.hpp", "spmm_kernels.hpp", "sddmm_kernels.hpp", "fp8_kernels.hpp",
                  "fp4_kernels.hpp", "spmm_blocked_kernels.hpp"}


def closure(path):
    """The files `path` includes with quotes, transitively, among csrc/ and include/."""
    seen, todo = set(), [path]
    while todo:
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', todo.pop().read_text(), re.M):
            for root in (CSRC, PKG / "include", PKG.parent / "include"):
                if (root / name).is_file() and root / name not in seen:
                    seen.add(root / name)
                    todo.append(root / name)
    return seen


def test_helper_headers_define_no_kernel():
    for name in HELPERS:
        assert "__global__" not in (CSRC / name).read_text(), name


def test_no_unit_renames_the_namespace():
    for f in CSRC.iterdir():
        assert not re.search(r"#\s*define\s+bsmr\b", f.read_text()), f.name


def test_one_pass_units_include_helpers_only():
    units = sorted(CSRC.glob("attention_qkv*.hip"))
    assert len(units) >= 4
    for unit in units:
        reached = {p.name for p in closure(unit)}
        assert not reached & KERNEL_HEADERS, (unit.name, sorted(reached & KERNEL_HEADERS))
