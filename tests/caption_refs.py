"""Plain float64 reference, error bounds and oracle helpers of the caption (language-model) loss: the kernel
``pgca_token_nll`` (csrc/misc.hip) and the steps built on it (``steps.CaptionStep``, ``steps.DPOStep(sft_alpha=...)``).
Shared by ``test_token_nll_gpu.py`` / ``test_caption_step_gpu.py`` (which run them next to the HIP path) and
``test_caption_refs_cpu.py`` (which proves them against ``torch.nn.functional.cross_entropy`` and autograd, and the
bounds against a float32 evaluation, with no kernel involved).

Nothing here knows about waves or workgroups except ``WAVE`` / ``WORKGROUP``, the documented sizes that decide WHERE a
test looks, never what it expects.
"""
import math

import torch
import torch.nn.functional as F

from step_kernel_refs import EPS23, r32, ulp32

F64 = torch.float64
WAVE, WORKGROUP = 64, 1024      # pgca_token_nll: one workgroup of 16 waves; four rows per 16-byte load


def counted_rows(nrows, seq_of_row, seq_limit):
    """bool [nrows]: row r counts iff there is no ``seq_of_row`` or ``seq_of_row[r] < seq_limit``."""
    if seq_of_row is None:
        return torch.ones(nrows, dtype=torch.bool)
    return torch.as_tensor(seq_of_row).cpu().long() < int(seq_limit)


def token_nll_ref(tok_lp, seq_of_row, seq_limit, grad_scale, accumulate=False, row_coef_in=None):
    """One ``pgca_token_nll`` call in float64 (include/pgca_hip.h).  ``tok_lp`` f32 [nrows]; ``grad_scale`` any float (the
    kernel receives its float32 value).  Returns dict(loss, n, metrics[4], row_coef, loss_bound, coef_bound):

    * n counted rows, loss = -(sum of the counted tok_lp) / n, NaN for n == 0;
    * metrics = {sum of -tok_lp, n, loss, finite flag};
    * row_coef = grad_scale / n on counted rows and 0 elsewhere - every element 0 when the loss is not finite; with
      ``accumulate`` it is ADDED to ``row_coef_in`` (nothing is added when the loss is not finite);
    * loss_bound = sqrt(n) * eps_f32 * sum |counted tok_lp| / n, eps_f32 = 2^-23 (float32's machine epsilon): the
      project's bound of an f32 sum in any order (row_kernel_refs.sum_bound: (sqrt(n) + 1) * 2^-24 * sum |terms|, which
      this is never below for n >= 1) carried through the division;
    * coef_bound: one division, so 1 ulp of the coefficient (plus, accumulated, half an ulp of the sum it is added into).
    """
    t = torch.as_tensor(tok_lp).detach().cpu().to(F64)
    keep = counted_rows(t.numel(), seq_of_row, seq_limit)
    n = int(keep.sum())
    terms = t[keep]
    total = float(-terms.sum()) if n else 0.0
    loss = total / n if n else float("nan")
    finite = math.isfinite(loss)
    gs = r32(grad_scale)
    c = gs / n if finite else 0.0
    coef = torch.where(keep, torch.full_like(t, c), torch.zeros_like(t)) if finite else torch.zeros_like(t)
    coef_bound = ulp32(torch.full_like(t, c)) * (coef != 0).to(F64)
    if accumulate:
        base = torch.as_tensor(row_coef_in).detach().cpu().to(F64)
        coef = base + coef
        coef_bound = torch.where(coef_bound > 0, coef_bound + 0.5 * ulp32(coef), coef_bound)   # untouched rows: exact
    abs_sum = float(terms.abs().sum()) if n else 0.0
    loss_bound = math.sqrt(n) * EPS23 * abs_sum / n if (n and finite) else 0.0
    return dict(loss=loss, n=n, metrics=[total if n else 0.0, float(n), loss, 1.0 if finite else 0.0], row_coef=coef,
                loss_bound=loss_bound, coef_bound=coef_bound, finite=finite)


def token_nll_f32(tok_lp, seq_of_row, seq_limit):
    """The loss with every operation correctly rounded to float32, summed one term after the other (a running sum, the
    order whose rounding error grows fastest): a plain float32 evaluation with no kernel involved."""
    t = torch.as_tensor(tok_lp).detach().cpu().float()
    keep = counted_rows(t.numel(), seq_of_row, seq_limit)
    s = torch.zeros((), dtype=torch.float32)
    for v in t[keep]:
        s = s + v
    n = int(keep.sum())
    return float(-s / torch.tensor(float(n), dtype=torch.float32)) if n else float("nan")


def masked_ce(logits, ids, mask):
    """Token-mean cross-entropy over the scored positions of a batch, the loss of ``steps.CaptionStep``: target
    ``ids[b, t+1]`` where ``mask[b, t+1] != 0`` (the rule of ``pgca_seq_batch_prepare``), everything else set to
    ``ignore_index`` - HF's ForCausalLMLoss on labels whose padded positions are -100."""
    labels = torch.where(mask[:, 1:] != 0, ids[:, 1:], torch.full_like(ids[:, 1:], -100))
    V = logits.shape[-1]
    return F.cross_entropy(logits[:, :-1].reshape(-1, V), labels.reshape(-1), ignore_index=-100)


def cos(a, b):
    a, b = torch.as_tensor(a).double().flatten().cpu(), torch.as_tensor(b).double().flatten().cpu()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))
