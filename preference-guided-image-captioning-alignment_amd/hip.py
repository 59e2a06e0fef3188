"""ctypes binding of ``libpgca_hip.so`` (C ABI: ``include/pgca_hip.h``).

There is NO CPU fallback: if the library is missing or a call fails, a
``RuntimeError`` is raised.  Wrappers take torch tensors that live on the GPU,
pass ``data_ptr()`` + sizes and launch on torch's current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# PGCA_LIB: a diagnostic build of the same ABI (python -m pgca_amd.build --variant=timing -DPGCA_GEMM_TIMING); the product
# library is the in-tree libpgca_hip.so
LIB_PATH = os.environ.get("PGCA_LIB") or os.path.join(_HERE, "libpgca_hip.so")

_K = abi.CONSTANTS  # every value below is the header's
NT, NN, TN = _K["PGCA_NT"], _K["PGCA_NN"], _K["PGCA_TN"]
(EPI_NONE, EPI_GELU_NEW, EPI_QUICK_GELU, EPI_RELU, EPI_TANH, EPI_DGELU_NEW, EPI_DRELU, EPI_DTANH, EPI_ROWSTATS,
 EPI_DLOGITS, EPI_DQUICK_GELU, EPI_GELU_NEW_D, EPI_MUL_AUX) = (_K["PGCA_EPI_" + n] for n in (
     "NONE", "GELU_NEW", "QUICK_GELU", "RELU", "TANH", "DGELU_NEW", "DRELU", "DTANH", "ROWSTATS", "DLOGITS",
     "DQUICK_GELU", "GELU_NEW_D", "MUL_AUX"))
SKINNY_MAX_M = _K["PGCA_SKINNY_MAX_M"]
ABI_VERSION = _K["PGCA_ABI_VERSION"]

GemmArgs, SkinnyArgs, SelectOpts = (abi.STRUCTS[n] for n in ("pgca_gemm_args", "pgca_skinny_args", "pgca_select_opts"))

_SIGS = {name: p.argtypes for name, p in abi.PROTOTYPES.items()}   # entry -> ctypes argtypes
EXPORTS = list(abi.PROTOTYPES)
_STREAMED = frozenset(name for name, p in abi.PROTOTYPES.items() if p.params and p.params[-1][1] == "stream")

_lib = None


def load() -> C.CDLL:
    """Load the HIP library (after torch, so libamdhip64.so.7 resolves to the loaded runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MI355X path has no fallback. Build it with "
            "`python -m pgca_amd.build` (hipcc --offload-arch=gfx950).")
    lib = C.CDLL(LIB_PATH)
    version = lib.pgca_version()
    if version != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} has ABI version {version}, this binding expects {ABI_VERSION}: "
                           "rebuild it with `python -m pgca_amd.build --force`")
    for name, p in abi.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = p.restype, p.argtypes
    for name, struct in abi.STRUCTS.items():
        size = getattr(lib, name.replace("pgca_", "pgca_sizeof_"))()
        if size != C.sizeof(struct):
            raise RuntimeError(f"{name} is {size} bytes in {LIB_PATH} but {C.sizeof(struct)} in the binding: "
                               "stale library, rebuild it")
    _lib = lib
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(entry: str, *args, stream=None):
    """Call the status-returning C entry ``entry``: tensors go as ``data_ptr()`` and ``None`` as NULL, an entry whose
    last parameter is ``stream`` gets torch's current HIP stream (or ``stream``), a non-zero status raises."""
    argv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    if entry in _STREAMED:
        argv.append(_stream() if stream is None else stream)
    rc = getattr(_lib or load(), entry)(*argv)
    if rc != 0:
        raise RuntimeError(f"{entry} failed ({rc}): {load().pgca_last_error().decode()}")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------- GEMM
def _gemm_args(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, layout: int, *, lda: int = None,
               ldb: int = None, epilogue: int = EPI_NONE, alpha: float = 1.0, bias: torch.Tensor = None,
               out_bf16: torch.Tensor = None, ld_out_bf16: int = None, out_f32: torch.Tensor = None,
               ld_out_f32: int = None, accumulate: bool = False, residual: torch.Tensor = None, ld_res: int = None,
               aux_out: torch.Tensor = None, aux_in: torch.Tensor = None, ld_aux: int = None,
               targets: torch.Tensor = None, stat_max: torch.Tensor = None, stat_sum: torch.Tensor = None,
               stat_ld: int = 0, target_val: torch.Tensor = None, row_lse: torch.Tensor = None,
               row_scale: torch.Tensor = None, out_cols: int = 0, drop=None, colsum_part: torch.Tensor = None,
               drop_rows: torch.Tensor = None, into: GemmArgs = None) -> GemmArgs:
    a = GemmArgs() if into is None else into
    a.A, a.B = A.data_ptr(), B.data_ptr()
    a.M, a.N, a.K = M, N, K
    a.lda = lda if lda is not None else (K if layout != TN else M)
    a.ldb = ldb if ldb is not None else (K if layout == NT else N)
    a.layout, a.epilogue, a.alpha = layout, epilogue, alpha
    a.bias = _p(bias)
    a.out_bf16, a.ld_out_bf16 = _p(out_bf16), (ld_out_bf16 if ld_out_bf16 is not None else N)
    a.out_f32, a.ld_out_f32 = _p(out_f32), (ld_out_f32 if ld_out_f32 is not None else N)
    a.accumulate = 1 if accumulate else 0
    a.residual, a.ld_res = _p(residual), (ld_res if ld_res is not None else N)
    a.aux_out, a.aux_in, a.ld_aux = _p(aux_out), _p(aux_in), (ld_aux if ld_aux is not None else N)
    a.targets, a.stat_max, a.stat_sum, a.stat_ld = _p(targets), _p(stat_max), _p(stat_sum), stat_ld
    a.target_val, a.row_lse, a.row_scale = _p(target_val), _p(row_lse), _p(row_scale)
    a.out_cols = out_cols
    if drop is not None:
        a.drop_seed, a.drop_threshold, a.drop_scale = drop
        a.drop_rows = _p(drop_rows)
    if colsum_part is not None:
        a.colsum_part, a.ld_colsum = colsum_part.data_ptr(), colsum_part.shape[1]
    return a


def _probe_begin(first: GemmArgs):
    """``gemm_probe``, if set and interested in the plan of ``first``, gets HIP events on the launch stream that bracket
    the one launch between this call and ``_probe_end`` (bench.py roofline measurement).  Without a probe the pair
    allocates nothing: decoding records its launches into HIP graphs, and a garbage collection that an allocation
    triggers inside a capture aborts the process."""
    probe = gemm_probe
    if probe is None or not probe.want(first.layout, first.epilogue, load().pgca_gemm_plan(C.byref(first))):
        return None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    return probe, e0, e1


def _probe_end(bracket, flops: float) -> None:
    if bracket is not None:
        probe, e0, e1 = bracket
        e1.record()
        probe.add(e0, e1, flops)


def gemm(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, layout: int, **kw) -> None:
    """One GEMM launch; the keywords are those of ``_gemm_args`` (the fields of ``pgca_gemm_args``)."""
    a = _gemm_args(A, B, M, N, K, layout, **kw)
    bracket = _probe_begin(a)
    _call("pgca_gemm_bf16", C.byref(a))
    _probe_end(bracket, 2.0 * M * N * K)


def _gemm_grouped(arr) -> None:
    _call("pgca_gemm_bf16_grouped", arr, len(arr))


def gemm_pair(g0, g1) -> None:
    """Two GEMMs as ONE launch where the library can pair them (two NT or two NN problems of one shape on the
    phase-staggered 256^2 tile: the same layer of the policy and of the reference trunk), else one launch each -
    bit-identical outputs either way.  ``g0`` / ``g1``: ``(args, kwargs)`` of the two ``gemm`` calls."""
    arr = (GemmArgs * 2)()
    for a, (args, kw) in zip(arr, (g0, g1)):
        _gemm_args(*args, **kw, into=a)
    bracket = _probe_begin(arr[0])
    _gemm_grouped(arr)
    _probe_end(bracket, sum(2.0 * a.M * a.N * a.K for a in arr))


def _wgrad_group_args(problems):
    arr = (GemmArgs * len(problems))()
    for a, (X, dY, M, N, K, gout) in zip(arr, problems):
        _gemm_args(X, dY, M, N, K, TN, out_f32=gout, accumulate=True, into=a)
    return arr


def gemm_wgrad_group(problems) -> None:
    """problems: up to four (X [K, M] bf16, dY [K, N] bf16, M, N, K, grad [M, N] f32) tuples -> grad += X^t dY for
    each, in ONE launch (no split-K atomics).  The four weight gradients of a GPT-2 block."""
    _gemm_grouped(_wgrad_group_args(problems))


def gemm_skinny(x, W, M, N, K, scratch, *, lda=None, ldw=None, bias=None, act=EPI_NONE, residual=None, ld_res=None,
                out_f32=None, ld_out_f32=None, out_bf16=None, ld_out_bf16=None, ln=None, ln_out=None, ld_ln=None):
    """y = epilogue(x[M,K] . W[K,N]) for a handful of rows (incremental decoding); ``ln`` = (gamma, beta, eps) runs the
    next LayerNorm on the finished row into ``ln_out``.  ``scratch``: ``gemm_skinny_workspace(M, N, K)`` bytes."""
    a = SkinnyArgs()
    a.x, a.W = x.data_ptr(), W.data_ptr()
    a.M, a.N, a.K = M, N, K
    a.lda, a.ldw = (K if lda is None else lda), (N if ldw is None else ldw)
    a.scratch, a.bias, a.act = scratch.data_ptr(), _p(bias), act
    a.residual, a.ld_res = _p(residual), (N if ld_res is None else ld_res)
    a.out_f32, a.ld_out_f32 = _p(out_f32), (N if ld_out_f32 is None else ld_out_f32)
    a.out_bf16, a.ld_out_bf16 = _p(out_bf16), (N if ld_out_bf16 is None else ld_out_bf16)
    if ln is not None:
        a.ln_gamma, a.ln_beta, a.ln_eps = ln[0].data_ptr(), ln[1].data_ptr(), float(ln[2])
        a.ln_out_bf16, a.ld_ln = ln_out.data_ptr(), (N if ld_ln is None else ld_ln)
    _call("pgca_gemm_skinny", C.byref(a))


def gemm_skinny_workspace(M: int, N: int, K: int) -> int:
    return int(load().pgca_gemm_skinny_workspace(M, N, K))


def drop_args(seed: int, p: float):
    """(seed, threshold, scale) triple understood by every kernel with fused dropout; None when p == 0."""
    if p <= 0.0:
        return None
    return (seed & 0xFFFFFFFF, min(0xFFFFFFFF, int(p * 4294967296.0)), 1.0 / (1.0 - p))


def set_option(name: str, value: int) -> None:
    """Process-wide dispatch knob of the library (names and values: include/pgca_hip.h)."""
    _call("pgca_set_option", name.encode(), int(value))


gemm_probe = None  # optional object with want(layout, epilogue, M, N, K) / add(ev0, ev1, flops)


def rowstats_combine(stat_max, stat_sum, stat_ld, nparts, target_val, M, lse=None, out_logprob=None):
    _call("pgca_rowstats_combine", stat_max, stat_sum, stat_ld, nparts, target_val, M, lse, out_logprob)


# --------------------------------------------------------------------------- LayerNorm / column sums
def layernorm_fwd(x, M, H, gamma, beta, eps=1e-5, row_map=None, y_bf16=None, y_f32=None, mean=None, rstd=None):
    _call("pgca_layernorm_fwd", x, row_map, M, H, gamma, beta, eps, y_bf16, y_f32, mean, rstd)


def layernorm_bwd_blocks(M: int) -> int:
    return load().pgca_layernorm_bwd_blocks(M)


def layernorm_bwd(x, M, H, gamma, mean, rstd, dx_out, *, dy_bf16=None, dy_f32=None, row_map=None, add_to=None,
                  dx_bf16=None, part=None, part_extra=None, drop_add=None, drop_dx=None, drop_rows=None):
    _call("pgca_layernorm_bwd", dy_bf16, dy_f32, x, row_map, M, H, gamma, mean, rstd, add_to, dx_out, dx_bf16, part,
          part_extra, _drop_words(drop_add), _drop_words(drop_dx), drop_rows)


def colsum_finish(part, nparts, H, out, accumulate=False):
    _call("pgca_colsum_finish", part, nparts, H, out, 1 if accumulate else 0)


def colsum_finish4(part, nplanes, nparts, H, outs, accumulate=False):
    o = list(outs) + [None] * (4 - len(outs))
    _call("pgca_colsum_finish4", part, nplanes, nparts, H, o[0], o[1], o[2], o[3], 1 if accumulate else 0)


def colsum_blocks(M: int) -> int:
    return load().pgca_colsum_blocks(M)


def colsum(M, N, ld, part, x_bf16=None, x_f32=None):
    _call("pgca_colsum", x_bf16, x_f32, M, N, ld, part)


# --------------------------------------------------------------------------- attention
_NODROP = (0, 0, 1.0)


def _drop_words(d):
    """(seed, threshold, scale) -> host uint32[3] with the scale's float bits (NULL when dropout is off)."""
    if d is None:
        return None
    import struct
    arr = (C.c_uint32 * 3)(d[0], d[1], struct.unpack("<I", struct.pack("<f", d[2]))[0])
    return C.cast(arr, C.c_void_p)


def attention_fwd(qkv, key_mask, B, S, heads, causal, out, lse=None, drop=None, cu=None):
    """``cu`` (int32 [B+1]): packed rows - sequence b is rows cu[b]..cu[b+1]-1; S stays the padded length."""
    d = drop or _NODROP
    _call("pgca_attention_fwd", qkv, key_mask, B, S, heads, 1 if causal else 0, out, lse, d[0], d[1], d[2], cu)


def attention_bwd(qkv, out, dout, lse, key_mask, B, S, heads, causal, dqkv, drop=None, cu=None):
    d = drop or _NODROP
    _call("pgca_attention_bwd", qkv, out, dout, lse, key_mask, B, S, heads, 1 if causal else 0, dqkv, d[0], d[1],
          d[2], cu)


def attention_bwd_split(qkv, out, dout, lse, key_mask, B, S, heads, causal, dqkv, drop=None, cu=None):
    """``attention_bwd`` on the two-role kernels (dK/dV per key block, dQ per query block): S <= 1024, same results."""
    d = drop or _NODROP
    _call("pgca_attention_bwd_split", qkv, out, dout, lse, key_mask, B, S, heads, 1 if causal else 0, dqkv, d[0],
          d[1], d[2], cu)


# --------------------------------------------------------------------------- embeddings / ViT input
def embed_fwd(ids, B, S, H, wte, wpe, h0, attended=None, gamma=None, beta=None, eps=1e-5, mean=None, rstd=None,
              att_stride=None, U=None, xheads=0, drop_x=None, drop_e=None, row_ids=None, n_rows=0):
    """``row_ids`` (int32 [n_rows]): packed rows - output row r is padded position row_ids[r] (< 0: zero filler)."""
    _call("pgca_embed_fwd", ids, B, S, H, wte, wpe, attended, gamma, beta, eps, h0, mean, rstd, H if att_stride is
          None else att_stride, U, xheads, _drop_words(drop_x), _drop_words(drop_e), row_ids, n_rows)


def embed_bwd_blocks(B: int, S: int) -> int:
    return load().pgca_embed_bwd_blocks(B, S)


def embed_bwd(g, ids, row_mask, B, S, H, dwte, dwpe, wte=None, attended=None, gamma=None, mean=None, rstd=None,
              dattended=None, part=None, att_stride=None, U=None, dU=None, xheads=0, drop_x=None, drop_e=None,
              cu=None):
    _call("pgca_embed_bwd", g, ids, row_mask, B, S, H, wte, attended, gamma, mean, rstd, dwte, dwpe, dattended,
          part, H if att_stride is None else att_stride, U, dU, xheads, _drop_words(drop_x), _drop_words(drop_e),
          cu)


def patchify(pixels, B, image, patch, out_bf16, ld_out=None):
    ld = 3 * patch * patch if ld_out is None else ld_out
    _call("pgca_patchify", pixels, B, image, patch, ld, out_bf16)


def image_preprocess(images_u8, B, H, W, S, xbounds, xcoef, ybounds, ycoef, mean, std, tmp, out, resized_u8=None):
    _call("pgca_image_preprocess", images_u8, B, H, W, S, xbounds, xcoef, xcoef.shape[1], ybounds, ycoef,
          ycoef.shape[1], mean[0], mean[1], mean[2], std[0], std[1], std[2], tmp, resized_u8, out)


def image_train_transform(images_u8, B, H, W, S, params, factors, xbounds, xcoef, ybounds, ycoef, mean, std, tmp, resized_u8,
                          out, aug_u8=None):
    _call("pgca_image_train_transform", images_u8, B, H, W, S, params, factors, xbounds, xcoef, xcoef.shape[-1],
          ybounds, ycoef, ycoef.shape[-1], mean[0], mean[1], mean[2], std[0], std[1], std[2], tmp, resized_u8,
          aug_u8, out)


def vit_assemble(patch_embeds, cls, pos, B, T, H, x):
    _call("pgca_vit_assemble", patch_embeds, cls, pos, B, T, H, x)


def vit_assemble_bwd(dx, B, T, H, dpatch_bf16, dcls, dpos):
    _call("pgca_vit_assemble_bwd", dx, B, T, H, dpatch_bf16, dcls, dpos)


# --------------------------------------------------------------------------- sequence reduce / losses
def seq_reduce(tok_lp, seq_of_row, nrows, nseq, seq_count, mode, seq_lp):
    _call("pgca_seq_reduce", tok_lp, seq_of_row, nrows, nseq, seq_count, mode, seq_lp)


def logits_logprob_bwd(logits, ld, V, row_map, targets, g, R, dlogits):
    _call("pgca_logits_logprob_bwd", logits, ld, V, row_map, targets, g, R, dlogits)


def logits_logprob(logits, ld, V, row_map, targets, R, out):
    _call("pgca_logits_logprob", logits, ld, V, row_map, targets, R, out)


# --------------------------------------------------------------------------- token selection (generation)
def _select_opts(no_repeat_ngram_size, ban_ids):
    n_ban = 0 if ban_ids is None else int(ban_ids.numel())
    return SelectOpts(int(no_repeat_ngram_size), n_ban, _p(ban_ids) if n_ban else None)


def select_token(logits, V, R, prev, n_prev, repetition_penalty, temperature, top_k, top_p, u, done, pad_id, next_ids,
                 next_logp, no_repeat_ngram_size=0, ban_ids=None):
    """``logits`` [R, >= V] f32 rows (row stride % 4 == 0), ``prev`` [R, >= n_prev] int64 rows; ``ban_ids``: device
    int64 ids banned in every row; see pgca_hip.h."""
    opts = _select_opts(no_repeat_ngram_size, ban_ids)
    _call("pgca_select_token_ex", logits, logits.stride(0), V, R, prev, prev.stride(0) if n_prev else 0, n_prev,
          repetition_penalty, temperature, top_k, top_p, u, done, pad_id, next_ids, next_logp, C.byref(opts))


def select_beam_candidates(logits, V, B, nb, prev, n_prev, repetition_penalty, warp, temperature, top_k, top_p,
                           beam_scores, K, use_noise, noise_seed, cand_score, cand_index, no_repeat_ngram_size=0,
                           ban_ids=None):
    opts = _select_opts(no_repeat_ngram_size, ban_ids)
    _call("pgca_select_beam_candidates_ex", logits, logits.stride(0), V, B, nb, prev, prev.stride(0) if n_prev else
          0, n_prev, repetition_penalty, int(warp), temperature, top_k, top_p, beam_scores, K, int(use_noise),
          noise_seed & 0xFFFFFFFF, cand_score, cand_index, C.byref(opts))


EARLY_STOPPING = {False: 0, True: 1, "never": 2}


def beam_step(cand_score, cand_index, B, nb, V, cur, L, eos, length_penalty, early_stopping, running_in, running_out,
              running_beam_scores, sequences_in, sequences_out, beam_scores, is_sent_finished, gen_len, unsat, tok,
              flat_src, hits_all):
    """One step of HF's beam bookkeeping after the candidates are known; ``early_stopping`` is False, True or
    "never"; ``is_sent_finished`` / ``unsat`` / ``hits_all`` are bool or uint8 tensors; see pgca_hip.h."""
    _call("pgca_beam_step", cand_score, cand_index, B, nb, V, cur, L, eos, length_penalty,
          EARLY_STOPPING[early_stopping], running_in, running_out, running_beam_scores, sequences_in, sequences_out,
          beam_scores, is_sent_finished, gen_len, unsat, tok, flat_src, hits_all)


def dpo_loss(pol_w, pol_l, ref_w, ref_l, B, beta, label_smoothing, loss, dpol_w=None, dpol_l=None, metrics=None):
    _call("pgca_dpo_loss", pol_w, pol_l, ref_w, ref_l, B, beta, label_smoothing, loss, dpol_w, dpol_l, metrics)


def seq_batch_prepare(ids, mask, Bq, S, counts, mask32, row_map, targets, seq_of_row, n_rows, stream=None):
    _call("pgca_seq_batch_prepare", ids, mask, Bq, S, counts, mask32, row_map, targets, seq_of_row, n_rows,
          stream=stream)


def seq_pack_prepare(mask32, Bq, S, pad_to, lens, cu, row_ids, n_packed, counts=None, row_map=None):
    _call("pgca_seq_pack_prepare", mask32, Bq, S, pad_to, lens, cu, row_ids, n_packed, counts, row_map)


def row_scale(dseq, seq_of_row, seq_count, nrows, mode, out):
    _call("pgca_row_scale", dseq, seq_of_row, seq_count, nrows, mode, out)


def token_nll(tok_lp, seq_of_row, seq_limit, nrows, grad_scale, accumulate, loss, row_coef=None, metrics=None):
    """Token-mean NLL of the compact rows of sequences < ``seq_limit`` (all rows when ``seq_of_row`` is None) and its
    per-row DLOGITS coefficient; see pgca_hip.h."""
    _call("pgca_token_nll", tok_lp, seq_of_row, seq_limit, nrows, grad_scale, 1 if accumulate else 0, loss, row_coef,
          metrics)


# --------------------------------------------------------------------------- preference-pair mining
MINE_RULES = {"adjacent": 0, "best_worst": 1}


def candidate_rows(cand, lengths, R, S, base_vocab, dec_vocab, dec_pad, text_pad, dec_ids, dec_mask, text_ids, text_mask,
                   text_len, out_len):
    """``cand`` int64 [R, ld] rows of generated decoder ids (row stride = ``cand.stride(0)``) -> decoder rows and
    text-tower rows of width ``S``; see pgca_hip.h."""
    _call("pgca_candidate_rows", cand, cand.stride(0), lengths, R, S, base_vocab, dec_vocab, dec_pad, text_pad, dec_ids,
          dec_mask, text_ids, text_mask, text_len, out_len)


def group_cosine(img, txt, B, n, P, score):
    _call("pgca_group_cosine", img, txt, B, n, P, score)


def mine_pairs(score, dec_ids, out_len, ok, B, n, S, min_tokens, rule, threshold, rank, pair_win, pair_lose, pair_margin,
               pair_count):
    """``rule``: "adjacent" (the reference's) or "best_worst"; ``ok``: optional uint8 / bool [B, n]."""
    _call("pgca_mine_pairs", score, dec_ids, out_len, ok, B, n, S, min_tokens, MINE_RULES[rule], threshold, rank,
          pair_win, pair_lose, pair_margin, pair_count)


def pair_rows(pair_win, pair_lose, pair_margin, pair_count, dec_ids, dec_mask, B, n, S, cap, dec_pad, preferred_ids,
              preferred_mask, rejected_ids, rejected_mask, pair_image, preference_score, n_pairs):
    _call("pgca_pair_rows", pair_win, pair_lose, pair_margin, pair_count, dec_ids, dec_mask, B, n, S, cap, dec_pad,
          preferred_ids, preferred_mask, rejected_ids, rejected_mask, pair_image, preference_score, n_pairs)


# --------------------------------------------------------------------------- caption metrics over token ids
EVAL_MAX_S, EVAL_MAX_K, EVAL_MAX_VOCAB = _K["PGCA_EVAL_MAX_S"], _K["PGCA_EVAL_MAX_K"], _K["PGCA_EVAL_MAX_VOCAB"]


def ngram_keys(ids, lengths, G, K, S, order, base_vocab, distinct_per_group, keys_out):
    """Stripped rows ``ids`` int64 [G, K, S] / ``lengths`` int32 [G, K] -> int64 keys [G, K, S] (-1: no n-gram)."""
    _call("pgca_ngram_keys", ids, lengths, G, K, S, order, base_vocab, int(bool(distinct_per_group)), keys_out)


def cider_rows(pred_ids, pred_len, ref_ids, ref_len, N, K, S, base_vocab, table_keys, table_df, table_off, n_docs,
               sigma, score_out, flag_out):
    """``score_out`` float64 [N], ``flag_out`` int32 [N]; ``table_off`` int64 [5] on the device; see pgca_hip.h."""
    _call("pgca_cider_rows", pred_ids, pred_len, ref_ids, ref_len, N, K, S, base_vocab, table_keys, table_df, table_off,
          table_keys.numel(), n_docs, sigma, score_out, flag_out)


def bleu_stats(pred_ids, pred_len, ref_ids, ref_len, N, K, S, base_vocab, stats_out):
    _call("pgca_bleu_stats", pred_ids, pred_len, ref_ids, ref_len, N, K, S, base_vocab, stats_out)


def token_overlap(a_ids, a_len, b_ids, b_len, R, S, out):
    _call("pgca_token_overlap", a_ids, a_len, b_ids, b_len, R, S, out)


def rouge_stats(pred_ids, pred_len, ref_ids, ref_len, N, K, S, base_vocab, out):
    """``out`` int32 [N, 6]: overlap_1, overlap_2, lcs, pred_len, ref_len, k_used (first present reference, -1: none)."""
    _call("pgca_rouge_stats", pred_ids, pred_len, ref_ids, ref_len, N, K, S, base_vocab, out)


def meteor_stats(pred_ids, pred_len, ref_ids, ref_len, N, K, S, base_vocab, out):
    """``out`` int32 [N, K, 2]: matches and chunks per reference, -1 / -1 for an absent one."""
    _call("pgca_meteor_stats", pred_ids, pred_len, ref_ids, ref_len, N, K, S, base_vocab, out)


def masked_mean_fwd(feats, mask, B, S, H, pooled, cu=None):
    _call("pgca_masked_mean_fwd", feats, mask, B, S, H, pooled, cu)


def masked_mean_bwd(dpooled, mask, B, S, H, dfeats, cu=None):
    _call("pgca_masked_mean_bwd", dpooled, mask, B, S, H, dfeats, cu)


def l2norm_fwd(x, B, P, y, norm=None):
    _call("pgca_l2norm_fwd", x, B, P, y, norm)


def l2norm_bwd(dy, y, norm, B, P, dx):
    _call("pgca_l2norm_bwd", dy, y, norm, B, P, dx)


def ntxent_loss(lse_r, lse_c, diag, n_local, n_total, loss):
    _call("pgca_ntxent_loss", lse_r, lse_c, diag, n_local, n_total, loss)


# --------------------------------------------------------------------------- optimiser
def sqnorm_blocks(n: int) -> int:
    return load().pgca_sqnorm_blocks(n)


def sqnorm(g, n, part):
    _call("pgca_sqnorm", g, n, part)


def step_control(part, nparts, max_norm, base_lr, warmup, total_steps, sched_stride, beta1, beta2, grad_scale, ctrl,
                 gate=None):
    _call("pgca_step_control", part, nparts, max_norm, base_lr, warmup, total_steps, sched_stride, beta1, beta2,
          grad_scale, gate, ctrl)


def clip_coef(part, nparts, max_norm, coef):
    _call("pgca_clip_coef", part, nparts, max_norm, coef)


def scale_dev(x, n, coef):
    _call("pgca_scale_dev", x, n, coef)


def adamw(p, g, m, v, p_bf16, n, ctrl, weight_decay, beta1, beta2, eps, grad_scale=1.0):
    _call("pgca_adamw", p, g, m, v, p_bf16, n, ctrl, weight_decay, beta1, beta2, eps, grad_scale)


def cast_bf16(x, y, n):
    _call("pgca_cast_bf16", x, y, n)


def cast_f32(x_bf16, y, n):
    _call("pgca_cast_f32", x_bf16, y, n)


def split_bf16(x, R, P, rows_out, pattern, y):
    _call("pgca_split_bf16", x, R, P, rows_out, pattern, y)


def axpy(x, alpha, y, n, accumulate=False):
    _call("pgca_axpy", x, alpha, y, n, 1 if accumulate else 0)


def gather_rows_bf16(src, row_map, M, H, dst):
    _call("pgca_gather_rows_bf16", src, row_map, M, H, dst)
