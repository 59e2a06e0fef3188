#!/usr/bin/env python3
"""Launch schedules of the engines, recorded on the CPU: every binding of ``pgca_amd.hip`` is replaced by a recorder, the
engines run on ``Workspace("cpu")`` with a tiny geometry, and each scenario prints its launch count and a SHA-1 of the
trace.  Two commits issue the same launches on the same buffers exactly when their traces are equal (``--out`` writes the
full trace for ``diff``).

A tensor argument is named by its owner and byte offset - the workspace key, the segment's ``fp32`` / ``bf16`` / ``grad``
buffer, or a scenario input - followed by the dtype, shape and (if not contiguous) strides of the view that was passed; a
tensor without an owner has only the latter, so two such tensors of one shape are not told apart.  Small integer tensors
(index vectors) also carry a checksum of their contents.  Scalars and dropout triples are recorded as they are.  Calls are
bound to the binding's signature first, so an omitted argument and its default given explicitly are one trace.

Not reachable without a device: the side-stream branch of ``GptTrunk.backward`` and the HIP-graph branch of
``decode_advance``.
"""
import argparse
import hashlib
import inspect
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pgca_amd import engine as E, hip   # noqa: E402
from pgca_amd.arch import tiny_arch   # noqa: E402
from pgca_amd.params import ParamStore   # noqa: E402

F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64
NOT_LAUNCHES = {"load", "drop_args", "set_option"}
SIZE_QUERIES = {   # fixed stand-ins: the real ones ask the library
    "layernorm_bwd_blocks": lambda M: (M + 63) // 64,
    "colsum_blocks": lambda M: (M + 127) // 128,
    "embed_bwd_blocks": lambda B, S: B,
    "sqnorm_blocks": lambda n: (n + 4095) // 4096,
    "gemm_skinny_workspace": lambda M, N, K: 4 * M * N * 8,
}


class _Stream:
    """Stand-in for ``torch.cuda.current_stream()``: CPU tensors never take the side-stream branch."""
    cuda_stream = 0

    def wait_event(self, ev):
        raise AssertionError("no event is recorded on the CPU path")


class Tracer:
    def __init__(self):
        self.lines = []
        self.inputs = {}          # name -> tensor handed to an engine by a scenario
        self.stores = []
        self.spaces = []

    # -- owners ---------------------------------------------------------------------------------------------------------
    def _roots(self):
        for name, t in self.inputs.items():
            yield "in." + name, t
        for store in self.stores:
            for seg in store.segments.values():
                for kind in ("fp32", "bf16", "grad"):
                    t = getattr(seg, kind)
                    if t is not None:
                        yield f"{seg.name}.{kind}", t
        for ws in self.spaces:
            for key, t in ws.bufs.items():
                yield "ws." + key, t

    def name(self, t: torch.Tensor) -> str:
        p = t.data_ptr()
        out = None
        for owner, root in self._roots():
            base = root.data_ptr()
            if base <= p < base + max(root.numel(), 1) * root.element_size():
                out = f"{owner}+{p - base}"
                break
        view = f"{str(t.dtype).replace('torch.', '')}{list(t.shape)}" + ("" if t.is_contiguous() else f"/{list(t.stride())}")
        out = f"<{view}>" if out is None else f"{out}:{view}"
        if t.dtype in (I32, I64) and t.numel() <= 4096:
            out += "#" + hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest()[:8]
        return out

    def fmt(self, v) -> str:
        if isinstance(v, torch.Tensor):
            return self.name(v)
        if isinstance(v, (list, tuple)):
            return "(" + ", ".join(self.fmt(x) for x in v) + ")"
        return repr(v)

    # -- recording ------------------------------------------------------------------------------------------------------
    def recorder(self, fname, orig):
        sig = inspect.signature(orig)

        def rec(*args, **kwargs):
            ba = sig.bind(*args, **kwargs)
            ba.apply_defaults()
            self.lines.append(f"{fname}(" + ", ".join(f"{k}={self.fmt(v)}" for k, v in ba.arguments.items()) + ")")
        return rec

    def note(self, text: str) -> None:
        self.lines.append("# " + text)

    def install(self):
        for fname, fn in list(vars(hip).items()):
            if fname.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != hip.__name__:
                continue
            if fname in SIZE_QUERIES:
                setattr(hip, fname, SIZE_QUERIES[fname])
            elif fname not in NOT_LAUNCHES:
                setattr(hip, fname, self.recorder(fname, fn))
        torch.cuda.current_stream = lambda *a, **k: _Stream()

    # -- scenario plumbing ------------------------------------------------------------------------------------------------
    def begin(self):
        self.lines, self.inputs, self.stores, self.spaces = [], {}, [], []

    def store(self, frozen=("vit",)) -> ParamStore:
        st = ParamStore(tiny_arch(), "cpu", frozen=frozen)
        for seg in st.segments.values():
            seg.ensure_bf16()
            if seg.trainable:
                seg.ensure_train_state()
        self.stores.append(st)
        return st

    def ws(self) -> "E.Workspace":
        w = E.Workspace("cpu")
        self.spaces.append(w)
        return w

    def inp(self, name: str, t: torch.Tensor) -> torch.Tensor:
        self.inputs[name] = t
        return t


T = Tracer()
ARCH = tiny_arch()


def _randn(name, *shape, dtype=F32):
    g = torch.Generator().manual_seed(len(name) + sum(shape))
    return T.inp(name, torch.randn(*shape, generator=g).to(dtype))


def seq_batch(lens, S, pack: bool) -> "E.SeqBatch":
    """A right-padded batch with the given lengths, and (``pack``) its packed row layout, built on the host the way the
    index kernels lay them out."""
    Bq = len(lens)
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, ARCH.gpt.base_vocab, (Bq, S), generator=g, dtype=I64)
    mask = torch.zeros(Bq, S, dtype=I32)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    nfill = E.n_filler_seqs(S)
    mask1 = torch.ones(Bq + nfill, S, dtype=I32)
    mask1[:Bq] = mask
    kept = [(b, t) for b in range(Bq) for t in range(S - 1) if mask[b, t + 1]]
    row_map = torch.tensor([b * S + t for b, t in kept], dtype=I32)
    targets = torch.tensor([int(ids[b, t + 1]) for b, t in kept], dtype=I64)
    seq_of_row = torch.tensor([b for b, _ in kept], dtype=I32)
    counts = mask[:, 1:].sum(1).to(I32)
    f = dict(ids=ids, mask=mask1[:Bq], row_map=row_map, targets=targets, seq_of_row=seq_of_row, counts=counts)
    pk = rmp = None
    if pack:
        n = sum(lens)
        Mp = (n + E.PACK_PAD - 1) // E.PACK_PAD * E.PACK_PAD
        first = [0]
        for ln in lens:
            first.append(first[-1] + ln)
        for _ in range(nfill):
            first.append(min(first[-1] + S, Mp))
        row_ids = torch.full((Mp,), -1, dtype=I32)
        row_ids[:n] = torch.tensor([b * S + t for b, ln in enumerate(lens) for t in range(ln)], dtype=I32)
        pk = E.RowPack(cu=torch.tensor(first, dtype=I32), row_ids=row_ids, mask=mask1, lens=torch.tensor(lens, dtype=I32),
                       n=n, Mp=Mp, Bq=Bq, S=S)
        rmp = torch.tensor([first[b] + t for b, t in kept], dtype=I32)
        f.update(cu=pk.cu, row_ids=row_ids, lens=pk.lens, row_map_packed=rmp, mask=mask1)
    for k, v in f.items():
        T.inp("sb." + k, v)
    return E.SeqBatch(ids=ids, mask=mask1[:Bq], row_map=row_map, targets=targets, seq_of_row=seq_of_row, counts=counts,
                      n_rows=len(kept), Bq=Bq, S=S, pack=pk, row_map_packed=rmp)


def plan(on: bool):
    return E.DropoutPlan(0.1, base_seed=3) if on else E.DropoutPlan(0.0)


LENS, S = (8, 5, 3), 8


# ---------------------------------------------------------------------------------------------------------------- scenarios
def trunk(packed: bool, drop: bool, recompute: str = "none"):
    def run():
        ws, st = T.ws(), T.store()
        tr = E.GptTrunk(st, "text_encoder.text_model", ARCH.gpt, ws, "t.trunk")
        tr.recompute = recompute
        sb = seq_batch(LENS, S, packed)
        M, H = (sb.pack.Mp if packed else sb.Bq * S), ARCH.gpt.hidden
        h0, g, g_bf = _randn("h0", M, H), _randn("g", M, H), _randn("g_bf", M, H, dtype=BF16)
        d = plan(drop).bind(E.TOWER_TEXT)
        tr.forward(h0, sb.mask, sb.Bq, S, True, d, pack=sb.pack)
        tr.backward(g, g_bf)
        T.note("save=False")
        tr.forward(h0, sb.mask, sb.Bq, S, False, d, pack=sb.pack)
    return run


def vit(trainable: bool):
    def run():
        ws, st = T.ws(), T.store(frozen=() if trainable else ("vit",))
        tower = E.VisionTower(st, ARCH.vit, ws)
        for B in (2, 3, 2):                      # the CLS row index is rebuilt when the batch changes
            T.note(f"B={B}")
            px = _randn(f"pixels{B}", B, 3, ARCH.vit.image, ARCH.vit.image)
            tower.forward(px, save=trainable)
            if trainable:
                tower.backward(_randn(f"dpooled{B}", B, ARCH.vit.hidden))
        T.note("save=False")
        tower.forward(px, save=False)
    return run


def decoder(packed: bool, drop: bool, reduce: str):
    def run():
        ws, st = T.ws(), T.store()
        eng = E.CaptionDecoderEngine(st, ARCH, ws, "pol")
        sb = seq_batch(LENS, S, packed)
        emb, dseq = _randn("emb", sb.Bq, ARCH.proj_dim), _randn("dseq", sb.Bq)
        eng.sequence_logprobs(emb, sb, reduce, True, plan(drop).bind(E.TOWER_DECODER))
        eng.backward(dseq)
        T.note("save=False")
        eng.sequence_logprobs(emb, sb, reduce, False)
    return run


def decoder_logits():
    ws, st = T.ws(), T.store()
    eng = E.CaptionDecoderEngine(st, ARCH, ws, "pol")
    sb = seq_batch(LENS, S, False)
    emb = _randn("emb", sb.Bq, ARCH.proj_dim)
    eng.logits(emb, sb)
    pv = T.inp("pv", eng.prefix_embedding(emb))
    for t in (0, 3):
        T.note(f"next_token_logits t={t}")
        eng.next_token_logits(pv, T.inp(f"ids{t}", sb.ids[:, :t].contiguous()))


def decode(skinny_rows):
    def run():
        ws, st = T.ws(), T.store()
        eng = E.CaptionDecoderEngine(st, ARCH, ws, "pol")
        if skinny_rows is not None:
            eng.trunk.SKINNY_ROWS = skinny_rows
        R = 4
        pv = _randn("pv", R, ARCH.gpt.hidden)
        tok = T.inp("tok", torch.tensor([5, 17, 2, 400], dtype=I64))
        for smax in (8, 6, 6):                   # the sequence offsets are rebuilt when the cache length changes
            T.note(f"decode_begin smax={smax}")
            eng.decode_begin(pv, smax)
            for _ in range(3):
                eng.decode_advance(tok)
        # a beam reorder is a copy, not a launch: its effect on a numbered cache is recorded instead
        kv = ws.bufs["pol.trunk.gen.kv"]
        kv.copy_(torch.arange(kv.numel()) % 251)
        eng.decode_reorder(T.inp("src", torch.tensor([2, 0, 0, 3], dtype=I64)))
        T.note("kv after decode_reorder " + hashlib.sha1(kv.view(torch.int16).numpy().tobytes()).hexdigest())
        eng.decode_advance(tok)
    return run


def text(packed: bool, drop: bool, frozen: bool):
    def run():
        ws, st = T.ws(), T.store(frozen=("vit", "text_tower") if frozen else ("vit",))
        eng = E.TextTowerEngine(st, ARCH, ws, "text")
        sb = seq_batch(LENS, S, packed)
        p = plan(drop)
        eng.forward(sb.ids, sb.mask, True, p.bind(E.TOWER_TEXT), p.site(E.TOWER_THEAD, 0, E.KIND_HEAD), pack=sb.pack)
        eng.backward(_randn("demb", sb.Bq, ARCH.proj_dim))
        T.note("save=False")
        eng.forward(sb.ids, sb.mask, False, pack=sb.pack)
    return run


def proj_head(drop: bool):
    def run():
        ws, st = T.ws(), T.store()
        head = E.ProjHead(st, "vision_encoder.projection", ARCH.vit.hidden, ARCH.proj_dim, ws, "vhead")
        B = 4
        head.forward(_randn("x", B, ARCH.vit.hidden, dtype=BF16), B, True, plan(drop).site(E.TOWER_VHEAD, 0, E.KIND_HEAD))
        head.backward(_randn("demb", B, ARCH.proj_dim), need_dx=True)
    return run


def ntxent():
    ws = T.ws()
    eng = E.NTXentEngine(ws, ARCH.proj_dim, 0.07)
    B, P = 4, ARCH.proj_dim
    img, txt = _randn("img", B, P), _randn("txt", B, P)
    img_all, txt_all = _randn("img_all", 2 * B, P), _randn("txt_all", 2 * B, P)
    lse_r, lse_c = _randn("lse_r_all", 2 * B), _randn("lse_c_all", 2 * B)
    # local, gathered at two offsets, local again: the target index vectors are rebuilt when (B, N, offset) change
    for off in (None, B, 0, B, None):
        T.note(f"offset={off}")
        if off is None:
            eng.forward(img, txt)
            eng.backward()
        else:
            eng.forward(img, txt, img_all, txt_all, offset=off)
            eng.backward(lse_r, lse_c, loss_scale=0.5)
    img3, txt3 = _randn("img3", 3, P), _randn("txt3", 3, P)
    T.note("B=3 offset=5")
    eng.forward(img3, txt3, img_all, txt_all, offset=5)
    eng.backward(lse_r, lse_c)


SCENARIOS = [(f"trunk_{'packed' if p else 'padded'}_{'drop' if d else 'nodrop'}", trunk(p, d))
             for p in (False, True) for d in (False, True)]
SCENARIOS += [(f"trunk_packed_drop_{m}", trunk(True, True, m)) for m in ("mlp", "block")]   # activation recompute
SCENARIOS += [("vit_frozen", vit(False)), ("vit_trainable", vit(True))]
SCENARIOS += [(f"decoder_{'packed' if p else 'padded'}_{'drop' if d else 'nodrop'}", decoder(p, d, "mean" if p else "sum"))
              for p in (False, True) for d in (False, True)]
SCENARIOS += [("decoder_logits", decoder_logits), ("decode_skinny", decode(None)), ("decode_tiles", decode(0))]
SCENARIOS += [(f"text_{'packed' if p else 'padded'}_{'drop' if d else 'nodrop'}", text(p, d, False))
              for p in (False, True) for d in (False, True)]
SCENARIOS += [("text_frozen", text(True, True, True)), ("proj_head_nodrop", proj_head(False)),
              ("proj_head_drop", proj_head(True)), ("ntxent", ntxent)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="write the full trace of every scenario to this file")
    ap.add_argument("--only", help="run the scenarios whose name contains this string")
    args = ap.parse_args()
    T.install()
    full = []
    for name, run in SCENARIOS:
        if args.only and args.only not in name:
            continue
        T.begin()
        run()
        launches = sum(1 for ln in T.lines if not ln.startswith("#"))
        digest = hashlib.sha1("\n".join(T.lines).encode()).hexdigest()
        print(f"{name:24s} {launches:5d} launches  {digest}")
        full += [f"==== {name}"] + T.lines
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write("\n".join(full) + "\n")


if __name__ == "__main__":
    main()
