"""``pgca_token_nll`` (csrc/misc.hip) against its float64 reference (``caption_refs.token_nll_ref``, proven on the CPU in
``test_caption_refs_cpu.py``): every branch of the kernel as written - the row-by-row head, the 16-byte body and the tail,
one row, part of a wave, one row past a wave, one row past the workgroup's first sweep of vectors - the ``seq_limit``
split, ``accumulate``, the non-finite rules, bitwise repeatability and the argument check."""
import math

import pytest
import torch

import caption_refs as C
from step_kernel_refs import scalar_matches, ulp32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 3.0
# 1 row; part of a wave; one past a wave; one past the workgroup (rows read one by one: 1024 threads); one past the
# workgroup's first sweep of 16-byte vectors (4 * 1024 rows) - the kernel's loops stride by the workgroup, there is no grid
ROWS = (1, 40, C.WAVE + 1, C.WORKGROUP + 1, 4 * C.WORKGROUP + 1, 4 * C.WORKGROUP + 7)


def _inputs(nrows, nseq, seed, offset=0):
    """tok_lp in -11 .. 0 and sorted sequence numbers; ``offset`` elements into a larger 16-byte-aligned allocation."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.empty(nrows + offset + 4, device=DEV)
    seq = torch.empty(nrows + offset + 4, dtype=torch.int32, device=DEV)
    tok[offset:offset + nrows] = -(torch.rand(nrows, generator=g) * 11.0 + 0.01).to(DEV)
    seq[offset:offset + nrows] = torch.sort(torch.randint(0, nseq, (nrows,), generator=g)).values.int().to(DEV)
    return tok[offset:offset + nrows], seq[offset:offset + nrows]


def _run(tok, seq, limit, gs, accumulate, coef_in=None, want_coef=True, want_metrics=True):
    from pgca_amd import hip
    n = tok.numel()
    loss = torch.full((1,), 77.0, device=DEV)
    coef = None
    if want_coef:
        coef = torch.full((n + 8,), SENTINEL, device=DEV)
        if coef_in is not None:
            coef[:n] = coef_in.to(DEV)
    metrics = torch.full((4,), 77.0, device=DEV) if want_metrics else None
    hip.token_nll(tok, seq, limit, n, gs, accumulate, loss, None if coef is None else coef[:n], metrics)
    torch.cuda.synchronize()
    if coef is not None:
        assert bool((coef[n:] == SENTINEL).all()), "row_coef written past nrows"
    return loss, (None if coef is None else coef[:n]), metrics


def _check(case, tok, seq, limit, gs, accumulate, coef_in=None):
    ref = C.token_nll_ref(tok, seq, limit, gs, accumulate, coef_in)
    loss, coef, metrics = _run(tok, seq, limit, gs, accumulate, coef_in)
    got = float(loss)
    print(f"[{case}] loss {got!r} ref {ref['loss']!r} |d| {abs(got - ref['loss']):.3e} bound {ref['loss_bound']:.3e}")
    assert scalar_matches(got, ref["loss"], ref["loss_bound"]), case
    m = metrics.cpu().double()
    assert float(m[1]) == ref["n"] and float(m[3]) == ref["metrics"][3], case
    assert scalar_matches(float(m[2]), ref["loss"], ref["loss_bound"]) and float(m[2]) == got or math.isnan(got), case
    if ref["finite"]:
        # the sum alone: one f32 rounding of a float64-accurate sum is far inside sqrt(n) * eps * sum |terms|
        assert abs(float(m[0]) - ref["metrics"][0]) <= max(ref["loss_bound"] * ref["n"], float(ulp32(ref["metrics"][0]))), case
    err = (coef.cpu().double() - ref["row_coef"]).abs()
    assert bool((err <= ref["coef_bound"]).all()), f"{case}: row_coef off by {float(err.max()):.3e}"
    return loss, coef, metrics


@pytest.mark.parametrize("nrows", ROWS)
def test_loss_and_coefficients_every_row_count(nrows):
    tok, seq = _inputs(nrows, 6, nrows)
    _check(f"n={nrows} all", tok, None, 0, 1.0, False)                    # seq_of_row NULL: every row, limit ignored
    _check(f"n={nrows} end", tok, seq, 6, 0.125, False)                   # limit at the end: every row again
    if nrows > 1:
        _check(f"n={nrows} mid", tok, seq, 3, 0.3, False)                 # in the middle, grad_scale != 1
        base = torch.full((nrows,), SENTINEL)
        _check(f"n={nrows} mid acc", tok, seq, 3, 0.3, True, base)        # accumulate onto the sentinel


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_views(offset):
    """tok_lp 4 * offset bytes past a 16-byte boundary: with seq_of_row offset alike the head rows are read one by one and
    the body in vectors; with seq_of_row aligned (or its own offset) every row is read alone.  Same values either way."""
    n = 4 * C.WORKGROUP + 5
    tok, seq = _inputs(n, 9, 100 + offset, offset)
    assert tok.data_ptr() % 16 == 4 * offset and seq.data_ptr() % 16 == 4 * offset
    l0, c0, _ = _check(f"offset {offset} both", tok, seq, 4, 1.0, False)
    seq_al = seq.clone()
    assert seq_al.data_ptr() % 16 == 0
    l1, c1, _ = _check(f"offset {offset} tok only", tok, seq_al, 4, 1.0, False)
    l2, c2, _ = _check(f"offset {offset} no seq", tok, None, 0, 1.0, False)
    assert torch.equal(c0, c1)
    # ... and against the aligned copy of the same rows
    l3, c3, _ = _check(f"offset {offset} aligned copy", tok.clone(), seq_al, 4, 1.0, False)
    assert torch.equal(c0, c3) and abs(float(l0) - float(l3)) <= 2 * float(ulp32(float(l3)))


def test_seq_limit_zero_is_nan_with_zero_coefficients():
    tok, seq = _inputs(300, 5, 5)
    loss, coef, metrics = _check("limit 0", tok, seq, 0, 1.0, False)
    assert math.isnan(float(loss)) and bool((coef == 0).all()) and float(metrics[1]) == 0 and float(metrics[3]) == 0
    base = torch.full((300,), SENTINEL)
    _, coef, _ = _check("limit 0 acc", tok, seq, 0, 1.0, True, base)
    assert bool((coef == SENTINEL).all())


@pytest.mark.parametrize("bad", [float("-inf"), float("nan")])
@pytest.mark.parametrize("nrows", [40, 4 * C.WORKGROUP + 7])
def test_non_finite_entry(bad, nrows):
    tok, seq = _inputs(nrows, 4, 11)
    tok[nrows // 2] = bad
    loss, coef, metrics = _check("bad acc0", tok, None, 0, 2.0, False)
    assert not math.isfinite(float(loss)) and bool((coef == 0).all()) and float(metrics[3]) == 0.0
    base = torch.full((nrows,), SENTINEL)
    loss, coef, _ = _check("bad acc1", tok, None, 0, 2.0, True, base)
    assert not math.isfinite(float(loss)) and bool((coef == SENTINEL).all())
    # the bad row outside the counted sequences: finite again
    lim = int(seq[nrows // 2])
    if lim > 0:
        loss, _, _ = _check("bad outside", tok, seq, lim, 1.0, False)
        assert math.isfinite(float(loss))


def test_two_launches_are_bitwise_equal():
    tok, seq = _inputs(4 * C.WORKGROUP + 7, 12, 21)
    a = _run(tok, seq, 7, 0.7, False)
    b = _run(tok, seq, 7, 0.7, False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_optional_outputs_and_bad_arguments():
    from pgca_amd import hip
    tok, seq = _inputs(130, 3, 31)
    full = _run(tok, seq, 2, 1.0, False)
    bare = _run(tok, seq, 2, 1.0, False, want_coef=False, want_metrics=False)
    assert torch.equal(full[0], bare[0]) and bare[1] is None and bare[2] is None
    loss = torch.full((1,), 77.0, device=DEV)
    coef = torch.full((130,), SENTINEL, device=DEV)
    for args in ((None, seq, 2, 130, 1.0, False, loss, coef),            # no tok_lp
                 (tok, seq, 2, 0, 1.0, False, loss, coef),               # nrows < 1
                 (tok, seq, -1, 130, 1.0, False, loss, coef),            # negative limit
                 (tok, seq, 2, 130, 1.0, False, None, coef)):            # no loss
        with pytest.raises(RuntimeError, match="pgca_token_nll"):
            hip.token_nll(*args)
    with pytest.raises(RuntimeError, match="pgca_token_nll"):
        hip._call("pgca_token_nll", tok, seq, 2, 130, 1.0, 2, loss, coef, None)   # accumulate is 0 or 1
    torch.cuda.synchronize()
    assert float(loss) == 77.0 and bool((coef == SENTINEL).all())        # nothing was launched
