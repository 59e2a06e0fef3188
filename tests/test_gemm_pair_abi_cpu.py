"""C boundary of the paired GEMM launch, no GPU needed.  The pair goes through the EXISTING entry
``pgca_gemm_bf16_grouped`` (no new export, no struct change): header prototype <-> export <-> ctypes signature of that
entry and of ``pgca_set_option``, the option the pair adds, and the argument checks that run before any launch."""
import ctypes
import os

import pytest
import torch  # noqa: F401  (loads libamdhip64 first, as the product does)

from pgca_amd import REPO_ROOT, abi, hip


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        from pgca_amd import build
        build.build()
    return hip.load()


def prototype(name):
    assert abi.PROTOTYPES[name].ret == "int", f"{name} has no status-returning prototype in pgca_hip.h"
    return [f"{t} {n}" for t, n in abi.PROTOTYPES[name].params]


def test_grouped_entry_prototype_export_and_ctypes_agree(lib):
    params = prototype("pgca_gemm_bf16_grouped")
    assert params == ["const pgca_gemm_args* args", "int32_t count", "void* stream"]
    assert hasattr(lib, "pgca_gemm_bf16_grouped") and "pgca_gemm_bf16_grouped" in hip.EXPORTS
    sig = hip._SIGS["pgca_gemm_bf16_grouped"]
    assert sig == [ctypes.POINTER(hip.GemmArgs), ctypes.c_int32, ctypes.c_void_p]
    assert lib.pgca_gemm_bf16_grouped.argtypes == sig and lib.pgca_gemm_bf16_grouped.restype is ctypes.c_int
    # an array of two problems is contiguous with the C stride
    assert ctypes.sizeof(hip.GemmArgs * 2) == 2 * lib.pgca_sizeof_gemm_args()


def test_set_option_prototype_and_pair_options(lib):
    assert prototype("pgca_set_option") == ["const char* name", "int32_t value"]
    assert hip._SIGS["pgca_set_option"] == [ctypes.c_char_p, ctypes.c_int32]
    for value in (1, 0):
        assert lib.pgca_set_option(b"gemm_pair_order", value) == 0
    assert lib.pgca_set_option(b"gemm_pair_order", 2) == -1 and b"gemm_pair_order" in lib.pgca_last_error()
    for value in (0, 1):
        assert lib.pgca_set_option(b"gemm_group", value) == 0
    header = open(os.path.join(REPO_ROOT, "include", "pgca_hip.h")).read()
    assert '"gemm_pair_order"' in header and '"gemm_group"' in header


def _qualifying_pair():
    """Two NN problems that qualify for the paired launch but have no output buffer (fake, aligned operand addresses:
    validation reads no memory)."""
    arr = (hip.GemmArgs * 2)()
    for a in arr:
        a.A, a.B = 0x1000, 0x2000
        a.M, a.N, a.K, a.lda, a.ldb = 256, 256, 64, 64, 256
        a.layout, a.alpha = hip.NN, 1.0
    return arr


def test_pair_arguments_are_checked_before_any_launch(lib):
    assert lib.pgca_set_option(b"gemm_tile", 256) == 0
    try:
        arr = _qualifying_pair()
        assert lib.pgca_gemm_plan(ctypes.byref(arr[0])) == 6025601
        assert lib.pgca_gemm_bf16_grouped(arr, 2, None) == -1 and b"no output buffer" in lib.pgca_last_error()
        arr[1].lda = 60       # the SECOND problem is checked too
        arr[0].out_f32 = arr[1].out_f32 = 0x3000
        assert lib.pgca_gemm_bf16_grouped(arr, 2, None) == -1 and b"lda" in lib.pgca_last_error()
    finally:
        assert lib.pgca_set_option(b"gemm_tile", 0) == 0
    assert lib.pgca_gemm_bf16_grouped(None, 2, None) == -1
    assert lib.pgca_gemm_bf16_grouped((hip.GemmArgs * 2)(), 2, None) == -1 and b"null operand" in lib.pgca_last_error()
