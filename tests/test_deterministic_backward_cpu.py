"""Host side of the deterministic backward (no GPU): the entry points are declared with their contract, bound and exported, the
``ops`` wrappers take ``deterministic``, and the workspace size is the documented function of the shapes."""
import ctypes
import inspect
import os
import re

from conftest import REPO

NEW = ["vfa_gather_backward_det_workspace_bytes", "vfa_project_gather_backward_det_f32", "vfa_column_sum_f32"]


def _header():
    return open(os.path.join(REPO, "include", "vfa_hip.h")).read()


def test_det_entry_points_are_declared_with_their_contract_bound_and_exported():
    from vfa_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(?:int|size_t)\s+(vfa_\w+)\s*\(", code))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    text = " ".join(_header().split())
    for phrase in ("function of the inputs and shapes only", "VFA_FLAG_RESERVED_CUS(n)", "exactly one fp32 add per element",
                   "masked boxes pass nothing", "VFA_ERR_BAD_ARGUMENT, nothing written", "no device-to-host read"):
        assert phrase in text, phrase
    assert "#define VFA_ABI_VERSION 9" in _header()


def test_ops_wrappers_take_deterministic():
    from vfa_amd import ops
    for fn in (ops.project_gather_backward, ops.relu_mask_backward, ops.collapse_gemm_relu_backward):
        p = inspect.signature(fn).parameters
        assert "deterministic" in p and p["deterministic"].default is None, fn.__name__
    assert list(inspect.signature(ops.column_sum).parameters)[:3] == ["x", "out", "accumulate"]


def _documented_bytes(n, nl, cells, C, Hf, Wf):
    """The layout the header documents: per record (16 per box) two 8-byte sort words and a 4-byte coefficient; 256 digit counts
    per 1024 records; one scan sum per 4096 counts; two gradient rows per run of 256 sorted positions; 256-byte aligned regions."""
    a = lambda x: (x + 255) // 256 * 256  # noqa: E731
    rec = 16 * n * nl * cells
    blocks = -(-rec // 1024)
    pieces = -(-rec // 256)
    return (2 * a(rec * 8) + a(rec * 4) + a(256 * blocks * 4) + a(-(-256 * blocks // 4096) * 4) + 2 * a(pieces * C * 4))


def test_det_workspace_size_is_the_documented_function_of_the_shapes():
    from vfa_amd import build
    lib = ctypes.CDLL(build.build())
    fn = lib.vfa_gather_backward_det_workspace_bytes
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.c_int] * 6
    for shape in [(7, 1, 40000, 256, 135, 240), (2, 5, 1003, 256, 68, 120), (3, 8, 77, 8, 34, 60), (1, 1, 1, 8, 5, 5)]:
        assert fn(*shape) == _documented_bytes(*shape), shape
    assert fn(0, 1, 100, 256, 10, 10) == 0 and fn(2, 1, 0, 256, 10, 10) == 0
    assert fn(7, 1, 40000, 256, 135, 240) < 1024 * 7 * 40000  # less than the 1 KiB of d vox per box at C = 256
    assert fn(1 << 12, 8, 1 << 20, 256, 10, 10) == 0  # beyond 2^31 records: refused (the callers chunk the cells)
