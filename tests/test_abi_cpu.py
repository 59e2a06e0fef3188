"""C-ABI surface checks that need no GPU: the library builds/loads and exports exactly the entry points
include/pgca_hip.h declares; what the binding derives from the header (``pgca_amd.abi``: prototypes, structs, the
scalar mapping) is what a C++ compiler reads in it."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch  # noqa: F401  (loads libamdhip64 first, as the product does)

from pgca_amd import REPO_ROOT, abi, hip

INCLUDE = os.path.join(REPO_ROOT, "include")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        from pgca_amd import build
        build.build()
    return hip.load()


def test_every_declared_symbol_is_exported(lib):
    """Header and library name the same entry points, in both directions."""
    declared = sorted(abi.PROTOTYPES)
    assert len(declared) >= 30 and declared == sorted(hip.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in pgca_hip.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in nm.splitlines() if ln.split()[-1].startswith("pgca_"))
    assert exported == declared, set(exported) ^ set(declared)


def test_version_and_error_string(lib):
    assert lib.pgca_version() >= 100
    assert isinstance(lib.pgca_last_error(), bytes)


def abi_check_source(prototypes):
    """A C++ translation unit that compiles exactly when the header says what the reader's tables say: one assertion on
    the function type of every entry, offset and size of every struct field against the ctypes structure, and size,
    signedness and float/integer kind of every mapped scalar type.  Returns (source, entries, structs)."""
    out = ["#include <cstddef>", "#include <type_traits>", '#include "pgca_hip.h"']
    for name, p in prototypes.items():
        fn = f"{p.ret} (*)({', '.join(t for t, _ in p.params)})"
        out.append(f'static_assert(std::is_same_v<decltype(&{name}), {fn}>, "{name}");')
    for name, st in abi.STRUCTS.items():
        out.append(f'static_assert(sizeof({name}) == {ctypes.sizeof(st)}, "sizeof {name}");')
        for field, ctype in st._fields_:
            out.append(f"static_assert(offsetof({name}, {field}) == {getattr(st, field).offset} && "
                       f'sizeof({name}::{field}) == {ctypes.sizeof(ctype)}, "{name}.{field}");')
    for c, ctype in abi.SCALARS.items():
        is_float, is_signed = isinstance(ctype(0).value, float), ctype(-1).value < 0
        out.append(f"static_assert(sizeof({c}) == {ctypes.sizeof(ctype)} && std::is_floating_point_v<{c}> == "
                   f'{str(is_float).lower()} && std::is_signed_v<{c}> == {str(is_signed).lower()}, "{c}");')
    out.append(f'static_assert(sizeof(void*) == {ctypes.sizeof(ctypes.c_void_p)} && sizeof(const char*) == '
               f'{ctypes.sizeof(ctypes.c_char_p)}, "pointers");')
    return "\n".join(out) + "\n", len(prototypes), len(abi.STRUCTS)


def test_the_compiler_reads_the_header_as_the_binding_does(tmp_path):
    cxx = shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"

    def compiles(source, stem):
        f = tmp_path / (stem + ".cpp")
        f.write_text(source)
        return subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", INCLUDE, str(f)], capture_output=True, text=True)

    source, entries, structs = abi_check_source(abi.PROTOTYPES)
    assert entries >= 58 and structs >= 3 and source.count("decltype(&pgca_") == entries
    assert sum(len(st._fields_) for st in abi.STRUCTS.values()) >= 35 + 21 + 3
    ok = compiles(source, "abi")
    assert ok.returncode == 0, ok.stderr
    # one parameter type of one entry altered (each a mistake that would load, run and corrupt silently): refused
    for entry, index, wrong in (("pgca_adamw", 7, "int32_t"), ("pgca_attention_fwd", 8, "int32_t"),
                                ("pgca_sqnorm", 1, "int32_t"), ("pgca_dpo_loss", 0, "const void*")):
        p = abi.PROTOTYPES[entry]
        assert p.params[index][0] != wrong
        params = list(p.params)
        params[index] = (wrong, params[index][1])
        bad = compiles(abi_check_source({**abi.PROTOTYPES, entry: p._replace(params=params)})[0], "bad_" + entry)
        assert bad.returncode != 0 and entry in bad.stderr, (entry, bad.stderr)


@pytest.mark.parametrize("name", sorted(abi.STRUCTS))
def test_struct_layout_matches_c_struct(tmp_path, lib, name):
    """Compile a tiny C program against the header and compare sizeof/offsetof with ctypes and with the library."""
    st = abi.STRUCTS[name]
    assert st in (hip.GemmArgs, hip.SkinnyArgs, hip.SelectOpts)
    fields = [f[0] for f in st._fields_]
    prog = f'#include <stdio.h>\n#include <stddef.h>\n#include "pgca_hip.h"\nint main(){{printf("%zu", sizeof({name}));'
    for f in fields:
        prog += f'printf(" %zu", offsetof({name}, {f}));'
    prog += "return 0;}\n"
    c = tmp_path / "o.c"
    c.write_text(prog)
    exe = tmp_path / "o"
    subprocess.run(["gcc", "-I", INCLUDE, str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(st) == getattr(lib, name.replace("pgca_", "pgca_sizeof_"))()
    assert nums[1:] == [getattr(st, f).offset for f in fields]
    assert lib.pgca_version() == hip.ABI_VERSION == 306


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
