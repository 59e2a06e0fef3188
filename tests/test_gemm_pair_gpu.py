"""Paired launch of two NT / NN GEMMs (``hip.gemm_pair`` -> ``pgca_gemm_bf16_grouped`` with two problems): one grid of
2 x ntm x ntn workgroups of the phase-staggered 256^2 kernel, each workgroup running ITS problem's arguments.

A tile of the paired launch runs the same main loop over the same k order and the same epilogue code as the tile of a
separate launch, so every output must be BITWISE equal to two ``hip.gemm`` calls - compared over the whole buffers,
padding rows and columns included (poisoned before the launch: a tile that strays into the other problem's rows, or
past the edge, shows).

Shapes: M, N in {256, 320} (one full tile; a full tile plus a 64-wide partial one - two workgroups per problem along
that dimension), K in {64, 192} (two 32-deep steps: the prologue holds everything and the ring never refills; six: the
steady state with its counted waits), NN and NT.  The 256^2 tile is forced, as these shapes would take the 128^2 one.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = -12345.0
PAD_ROWS, PAD_COLS = 2, 8


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def tile256():
    from pgca_amd import hip
    hip.set_option("gemm_tile", 256)
    yield
    hip.set_option("gemm_tile", 0)
    hip.set_option("gemm_group", 1)
    hip.set_option("gemm_pair_order", 0)


def _out(M, N, dtype):
    return torch.full((M + PAD_ROWS, N + PAD_COLS), POISON, dtype=dtype, device=dev())


def problem(kind, layout, M, N, K, seed, accumulate=False):
    """(args, kwargs) of one ``hip.gemm`` call on seeded inputs and FRESH poisoned outputs, and the output tensors."""
    from pgca_amd import hip
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(K, M, generator=g) if layout == hip.TN else torch.randn(M, K, generator=g)).to(dev(), torch.bfloat16)
    B = (torch.randn(K, N, generator=g) if layout != hip.NT else torch.randn(N, K, generator=g)).to(dev(), torch.bfloat16)
    bias = torch.randn(N, generator=g).to(dev())
    stream = torch.randn(M + PAD_ROWS, N + PAD_COLS, generator=g).to(dev())     # the f32 residual stream
    rows = torch.randperm(4 * M, generator=g)[:M].to(dev(), torch.int32)          # padded position of every packed row
    ld = N + PAD_COLS
    kw = dict(bias=bias)
    if kind == "resid_drop_new":     # the policy's projection: dropout, residual added into a NEW buffer
        o = _out(M, N, torch.float32)
        kw.update(residual=stream, ld_res=ld, out_f32=o, ld_out_f32=ld, drop=hip.drop_args(seed * 7 + 1, 0.25),
                  drop_rows=rows)
        outs = [o, stream]
    elif kind == "resid_inplace":    # the reference's: the residual stream updated in place
        kw.update(residual=stream, ld_res=ld, out_f32=stream, ld_out_f32=ld)
        outs = [stream]
    elif kind == "gelu_d":           # the policy's c_fc: activation + its derivative for the backward
        o, aux = _out(M, N, torch.bfloat16), _out(M, N, torch.bfloat16)
        kw.update(epilogue=hip.EPI_GELU_NEW_D, out_bf16=o, ld_out_bf16=ld, aux_out=aux, ld_aux=ld)
        outs = [o, aux]
    elif kind == "gelu":
        o = _out(M, N, torch.bfloat16)
        kw.update(epilogue=hip.EPI_GELU_NEW, out_bf16=o, ld_out_bf16=ld)
        outs = [o]
    elif kind == "plain":
        o = _out(M, N, torch.bfloat16)
        kw.update(out_bf16=o, ld_out_bf16=ld)
        outs = [o]
    elif kind == "accumulate":       # a splittable problem: f32 accumulation onto zeros, nothing else
        o = _out(M, N, torch.float32)
        o[:M, :N] = 0
        kw = dict(out_f32=o, ld_out_f32=ld, accumulate=True)
        outs = [o]
    else:
        raise KeyError(kind)
    return ((A, B, M, N, K, layout), kw), outs, (A, B, bias)


def run_both(p0, p1):
    """p = (kind, layout, M, N, K, seed): the pair through ``gemm_pair`` and as two ``gemm`` calls, on separate buffers."""
    from pgca_amd import hip
    g0, o0, _ = problem(*p0)
    g1, o1, _ = problem(*p1)
    hip.gemm_pair(g0, g1)
    s0, r0, _ = problem(*p0)
    s1, r1, _ = problem(*p1)
    hip.gemm(*s0[0], **s0[1])
    hip.gemm(*s1[0], **s1[1])
    torch.cuda.synchronize()
    return o0 + o1, r0 + r1


def assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{what}: output {i} differs in {int((a != b).sum())} of {a.numel()} elements"
        assert bool((a[:-PAD_ROWS, :-PAD_COLS] != POISON).any()), f"{what}: output {i} was never written"


PAIRS = {
    "residual": ("resid_drop_new", "resid_inplace"),
    "residual_swapped": ("resid_inplace", "resid_drop_new"),
    "gelu": ("gelu_d", "gelu"),
    "gelu_swapped": ("gelu", "gelu_d"),
    "plain": ("plain", "plain"),
}


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("N", [256, 320])
@pytest.mark.parametrize("M", [256, 320])
@pytest.mark.parametrize("layout", ["NN", "NT"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_pair_equals_separate_launches(pair, layout, M, N, K):
    from pgca_amd import hip
    lay = getattr(hip, layout)
    k0, k1 = PAIRS[pair]
    for order in (0, 1):             # both tile orders of the paired grid
        hip.set_option("gemm_pair_order", order)
        got, want = run_both((k0, lay, M, N, K, 11), (k1, lay, M, N, K, 12))
        assert_same(got, want, f"{pair} {layout} {M}x{N}x{K} order {order}")
    hip.set_option("gemm_pair_order", 0)


def test_pair_is_one_launch_of_the_pair_plan():
    """The shapes above qualify: both problems plan the phase-staggered 256^2 tile without a K split (schedule 6)."""
    import ctypes
    from pgca_amd import hip
    (args, kw), _, _ = problem("plain", hip.NN, 320, 320, 192, 1)
    a = hip._gemm_args(*args, **kw)
    assert hip.load().pgca_gemm_plan(ctypes.byref(a)) == 6025601


def test_plain_pair_against_float_matmul():
    """Guard against two equal but wrong results.  Bound: twice the bf16 output rounding (2^-9 relative) on top of bf16 x bf16
    products accumulated in f32 (exact products, 2^-24 relative per add: negligible at K = 192)."""
    from pgca_amd import hip
    M, N, K = 320, 320, 192
    g0, o0, (A0, B0, b0) = problem("plain", hip.NN, M, N, K, 21)
    g1, o1, (A1, B1, b1) = problem("plain", hip.NN, M, N, K, 22)
    hip.gemm_pair(g0, g1)
    torch.cuda.synchronize()
    for o, A, B, b in ((o0[0], A0, B0, b0), (o1[0], A1, B1, b1)):
        ref = A.double() @ B.double() + b.double()
        err = (o[:M, :N].double() - ref).abs()
        assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-5).all()), float(err.max())


@pytest.mark.parametrize("case", ["different_M", "split_k", "group_off", "tn_mixed_in"])
def test_fallback_equals_separate_launches(case):
    from pgca_amd import hip
    if case == "different_M":
        got, want = run_both(("plain", hip.NN, 256, 320, 192, 31), ("plain", hip.NN, 320, 320, 192, 32))
    elif case == "split_k":          # 16 K tiles, one output tile: the plan splits K in two (atomics onto zeros)
        import ctypes
        (args, kw), _, _ = problem("accumulate", hip.NN, 256, 256, 1024, 33)
        assert hip.load().pgca_gemm_plan(ctypes.byref(hip._gemm_args(*args, **kw))) % 100 == 2
        got, want = run_both(("accumulate", hip.NN, 256, 256, 1024, 33), ("accumulate", hip.NN, 256, 256, 1024, 34))
    elif case == "group_off":
        hip.set_option("gemm_group", 0)
        try:
            got, want = run_both(("resid_drop_new", hip.NN, 320, 320, 192, 35), ("resid_inplace", hip.NN, 320, 320, 192, 36))
        finally:
            hip.set_option("gemm_group", 1)
    else:
        got, want = run_both(("accumulate", hip.TN, 320, 320, 192, 37), ("plain", hip.NN, 320, 320, 192, 38))
    assert_same(got, want, case)
