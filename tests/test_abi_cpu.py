"""C-ABI surface checks that need no GPU: the library builds/loads and exports exactly the
entry points include/pgca_hip.h declares; the ctypes struct mirrors the C struct."""
import ctypes
import os
import re
import subprocess

import pytest
import torch  # noqa: F401  (loads libamdhip64 first, as the product does)

from pgca_amd import REPO_ROOT, hip


def header_functions():
    src = open(os.path.join(REPO_ROOT, "include", "pgca_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pgca_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        from pgca_amd import build
        build.build()
    return hip.load()


def test_every_declared_symbol_is_exported(lib):
    declared = header_functions()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in pgca_hip.h but not exported"
    assert sorted(hip.EXPORTS) == declared, set(hip.EXPORTS) ^ set(declared)


def test_version_and_error_string(lib):
    assert lib.pgca_version() >= 100
    assert isinstance(lib.pgca_last_error(), bytes)


def test_gemm_args_layout_matches_c_struct(tmp_path):
    """Compile a tiny C program against the header and compare sizeof/offsetof with ctypes."""
    fields = [f[0] for f in hip.GemmArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "pgca_hip.h"\nint main(){printf("%zu", sizeof(pgca_gemm_args));'
    for f in fields:
        prog += f'printf(" %zu", offsetof(pgca_gemm_args, {f}));'
    prog += "return 0;}\n"
    c = tmp_path / "o.c"
    c.write_text(prog)
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-I", os.path.join(REPO_ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(hip.GemmArgs)
    assert nums[1:] == [getattr(hip.GemmArgs, f).offset for f in fields]


def test_skinny_args_layout_matches_c_struct(tmp_path):
    fields = [f[0] for f in hip.SkinnyArgs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "pgca_hip.h"\nint main(){printf("%zu", sizeof(pgca_skinny_args));'
    for f in fields:
        prog += f'printf(" %zu", offsetof(pgca_skinny_args, {f}));'
    prog += "return 0;}\n"
    c = tmp_path / "s.c"
    c.write_text(prog)
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(REPO_ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(hip.SkinnyArgs)
    assert nums[1:] == [getattr(hip.SkinnyArgs, f).offset for f in fields]


def test_host_side_argument_validation_needs_no_gpu(lib):
    """Validation happens before any launch, so it is observable on a CPU-only box."""
    a = hip.GemmArgs()
    assert lib.pgca_gemm_bf16(ctypes.byref(a), None) == -1
    assert b"null operand" in lib.pgca_last_error()
    assert lib.pgca_attention_fwd(None, None, 1, 128, 1, 1, None, None, 0, 0, 1.0, None, None) == -1
    sk = hip.SkinnyArgs()
    assert lib.pgca_gemm_skinny(ctypes.byref(sk), None) == -1 and b"pgca_gemm_skinny" in lib.pgca_last_error()
    assert lib.pgca_gemm_skinny_workspace(1, 3072, 1024) > 0 and lib.pgca_gemm_skinny_workspace(0, 8, 8) == 0
    assert lib.pgca_seq_pack_prepare(None, 1, 16, 64, None, None, None, None, None, None, None) == -1
    assert lib.pgca_sqnorm_blocks(1) == 1 and lib.pgca_sqnorm_blocks(16384 * 3 + 1) == 4


@pytest.mark.parametrize("layout", [hip.TN, hip.NT, hip.NN], ids=["TN", "NT", "NN"])
def test_grouped_launch_rejects_empty_shapes_before_planning(lib, layout):
    """Two problems in the weight-gradient form (plain epilogue, accumulate into f32: the split-K candidates) with no
    output tiles are an argument error, found before the planner divides by the tile count."""
    X, G = torch.zeros(64, 64, dtype=torch.bfloat16), torch.zeros(64, 64)
    for M, N in ((0, 0), (0, 64), (64, 0), (-256, 64)):
        arr = (hip.GemmArgs * 2)()
        for a in arr:
            hip._gemm_args(X, X, M, N, 64, layout, lda=64, ldb=64, out_f32=G, ld_out_f32=64, accumulate=True, into=a)
        assert lib.pgca_gemm_bf16_grouped(arr, 2, None) == -1, (M, N)
        assert b"empty shape" in lib.pgca_last_error()


def test_wgrad_group_args_are_the_hand_filled_struct():
    """``gemm_wgrad_group`` fills its array through ``_gemm_args``: every field of every problem equals the struct it
    used to fill by hand (TN, alpha 1, accumulate into the f32 gradient, every leading dimension N, the rest zero)."""
    problems = []
    for M, N, K in ((512, 256, 2048), (256, 768, 200), (264, 520, 64)):
        problems.append((torch.zeros(K, M, dtype=torch.bfloat16), torch.zeros(K, N, dtype=torch.bfloat16), M, N, K,
                         torch.zeros(M, N)))
    arr = hip._wgrad_group_args(problems)
    assert len(arr) == len(problems)
    for got, (X, dY, M, N, K, gout) in zip(arr, problems):
        a = hip.GemmArgs()
        a.A, a.B = X.data_ptr(), dY.data_ptr()
        a.M, a.N, a.K = M, N, K
        a.lda, a.ldb = M, N
        a.layout, a.epilogue, a.alpha = hip.TN, hip.EPI_NONE, 1.0
        a.out_f32, a.ld_out_f32 = gout.data_ptr(), N
        a.ld_out_bf16 = a.ld_res = a.ld_aux = N
        a.accumulate = 1
        for name, _ in hip.GemmArgs._fields_:
            assert getattr(got, name) == getattr(a, name), name
        assert bytes(got) == bytes(a)
