"""The GEMM kernels at the shapes the benchmark runs them, against plain float64 / exact float32 references.

``test_kernels_gpu.py`` covers layouts and edges at toy sizes (M <= 4096, <= 32 output tiles, V = 1004).  Here:

* the fused LM head (ROWSTATS + ``rowstats_combine``, DLOGITS, the dgrad / wgrad GEMMs of ``CaptionDecoderEngine.backward``)
  at the GPT-2 vocabulary and at one vocabulary of every class of ``V mod 256`` - the 256^2 tile writes four 64-column
  strips per column tile, the ``stat_ld`` contract counts 2 * ceil(N / 128) of them;
* the eight GEMM launches of a GPT-2-M block as ``engine.GptTrunk`` issues them, and the grouped weight gradient, at the
  bench's packed row count (M = 73152: 286 row tiles, 1144-4576 workgroups = several rounds of all CUs) and at an M that
  is a multiple of neither 8 rows nor 8 tiles;
* every output lives inside a larger buffer filled with a sentinel bit pattern (``Guard``): a write past the declared
  rows, past ``ld`` columns or past the end fails the test, as does a tile that never wrote its window.

Two passes per trunk launch: an EXACT pass (small integer operands: every f32 partial sum is an integer below 2^24, so any
summation order gives the same bits and the result must equal float32 torch bitwise) and a RANDOM pass against float64
at the tolerances of ``test_kernels_gpu.py``, which also replays every NN / NT launch with both 256^2 schedules and
requires bitwise equal results (the race screen of ``test_phase_staggered_gemm_race_screen`` at full occupancy).
Run with ``-s`` to see the measured errors.
"""
import contextlib

import pytest
import torch

from oracle import restatement as R

pytestmark = pytest.mark.gpu

H, I = 1024, 4096                     # GPT-2-M width (arch.GPT_ZOO["gpt2-medium"])
M_BENCH = 73152                       # packed C2 rows of the benchmarked batch: 285.75 tiles of 256
M_ODD = 70001                         # M % 8 = 1, ceil(M / 256) = 274 (% 8 = 2)
V_GPT2 = 50257


@pytest.fixture(scope="module")
def hip():
    from pgca_amd import hip as H_
    H_.load()
    return H_


def dev():
    return torch.device("cuda:0")


def gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def ints(shape, seed, lo=-2, hi=2, dtype=torch.bfloat16):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed), device=dev()).to(dtype)


def randn(shape, seed, scale=1.0, dtype=torch.float32):
    return (torch.randn(shape, generator=gen(seed), device=dev()) * scale).to(dtype)


def max_err(a, b):
    return float((a.double() - b.double()).abs().max())


def close(a, b, rel, what):
    """max |a - b| <= rel * max |b|; returns the relative error for the report."""
    scale = float(b.double().abs().max()) + 1e-12
    err = max_err(a, b)
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e} > {rel})"
    return err / scale


class Guard:
    """A [rows, cols] output with row stride ``ld`` inside a buffer of ``rows + pad_rows`` rows plus ``slack`` elements,
    all of it filled with a sentinel bit pattern (a NaN for the float types).  ``check()`` asserts that nothing outside the
    window changed and (``full=True``) that every element inside it was written."""
    BITS = {torch.float32: (torch.int32, 0x7FA5A5A5), torch.bfloat16: (torch.int16, 0x7FA5)}

    def __init__(self, rows, cols, dtype, ld=None, pad_rows=3, slack=64, fill=None):
        self.rows, self.cols, self.ld = rows, cols, ld if ld is not None else cols
        itype, bits = self.BITS[dtype]
        n = (rows + pad_rows) * self.ld + slack
        self.buf = torch.empty(n, dtype=dtype, device=dev())
        self.raw = self.buf.view(itype)
        self.raw.fill_(bits)
        self.sentinel = bits
        self.full = self.buf[:rows * self.ld].view(rows, self.ld)     # what a kernel addresses through ld
        self.view = self.full[:, :cols]
        if fill is not None:
            self.view.copy_(fill)

    def check(self, what, full=True):
        inside = torch.zeros(self.raw.numel(), dtype=torch.bool, device=dev())
        inside[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = True
        touched = (self.raw != self.sentinel) & ~inside
        n = int(touched.sum())
        if n:
            idx = int(touched.nonzero()[0])
            raise AssertionError(f"{what}: {n} sentinel element(s) outside the [{self.rows}, {self.cols}] (ld {self.ld}) "
                                 f"window were overwritten, first at flat index {idx} = row {idx // self.ld}, "
                                 f"column {idx % self.ld}")
        if full:
            missed = int((self.raw.view(-1)[:self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]
                          == self.sentinel).sum())
            assert missed == 0, f"{what}: {missed} element(s) of the window were never written"


class PlanRecorder:
    """Records ``pgca_gemm_plan`` of every ``hip.gemm`` launch (through the binding's probe hook; launches unchanged)."""

    def __init__(self):
        self.plans = []

    def want(self, layout, epilogue, plan):
        self.plans.append(plan)
        return False


@contextlib.contextmanager
def recording(hip):
    rec = PlanRecorder()
    old, hip.gemm_probe = hip.gemm_probe, rec
    try:
        yield rec.plans
    finally:
        hip.gemm_probe = old


@contextlib.contextmanager
def forced(hip, tile, schedule):
    hip.set_option("gemm_tile", tile)
    hip.set_option("gemm_schedule", schedule)
    try:
        yield
    finally:
        hip.set_option("gemm_tile", 0)
        hip.set_option("gemm_schedule", -1)


PLAN_128 = 12801                       # pgca_gemm_plan: 128^2 kernel
PLAN_256 = 25601                       # 256^2, 2-stage BK=64 loop, no split
PLAN_256S = 6 * 1000000 + 25601        # 256^2, phase-staggered loop (gemm256s), no split


def tiles256(M, N):
    return ((M + 255) // 256) * ((N + 255) // 256)


# ============================================================================================== LM head: ROWSTATS
# one vocabulary per class of V mod 256 (0, 1, 1..64, 65..128 incl. GPT-2's 81, 128, 129..192, 193..255)
VOCABS = [50176, 50177, 50200, V_GPT2, 50304, 50350, 50420]
LM_M, LM_K = 300, 1024
_lm_cache = {}


def lm_problem(V):
    """h [M, K], wte [V, K] bf16 and targets whose logits are PEAKED: rows 0, 4, 8, .. put ~98 % of the mass on one id in
    0..127 (the strips the overrun clobbered), rows 1, 5, .. on one id of the last, partial column tile; the rest are
    flat.  Targets include 0, 127, 128 and V - 1."""
    if V in _lm_cache:
        return _lm_cache[V]
    wte = randn((V, LM_K), 7, 0.03, torch.bfloat16)
    g = torch.Generator().manual_seed(V)
    last0 = (V - 1) // 256 * 256
    peak = torch.randint(0, 128, (LM_M,), generator=g)
    peak[1::4] = torch.randint(last0, V, (len(range(1, LM_M, 4)),), generator=g)
    peak = peak.to(dev())
    h = randn((LM_M, LM_K), 8, 0.5)
    sel = torch.zeros(LM_M, dtype=torch.bool, device=dev())
    sel[0::4] = True
    sel[1::4] = True
    h[sel] = 16.0 * wte[peak[sel]].float()
    h = h.bfloat16()
    tgt = torch.randint(0, V, (LM_M,), generator=g).to(dev())
    tgt[0::8] = peak[0::8]                         # the peaked id itself (in 0..127)
    tgt[1::8] = peak[1::8]                         # ... or in the last tile
    tgt[2], tgt[3], tgt[6], tgt[7], tgt[10] = 0, 127, 128, V - 1, V - 1
    tgt[4], tgt[12] = 0, 127                       # peaked rows whose target is NOT the peak
    logits = h.double() @ wte.double().t()
    ref_lse = torch.logsumexp(logits, -1)
    ref_lp = torch.log_softmax(logits, -1).gather(-1, tgt[:, None]).squeeze(-1)
    _lm_cache.clear()
    _lm_cache[V] = (h, wte, tgt, ref_lse, ref_lp)
    return _lm_cache[V]


def rowstats(hip, h, wte, tgt, M, V, K):
    """The engine's LM-head forward (engine.py token_logprobs) with every output guarded; returns lse, log-prob."""
    nparts = 2 * ((V + 127) // 128)                # exactly the documented stat_ld, as the engine allocates it
    smax, ssum = Guard(M, nparts, torch.float32), Guard(M, nparts, torch.float32)
    tval, lse, lp = (Guard(M, 1, torch.float32, slack=16) for _ in range(3))
    hip.gemm(h, wte, M, V, K, hip.NT, epilogue=hip.EPI_ROWSTATS, targets=tgt, stat_max=smax.view, stat_sum=ssum.view,
             stat_ld=nparts, target_val=tval.view)
    torch.cuda.synchronize()
    smax.check("stat_max")
    ssum.check("stat_sum")
    hip.rowstats_combine(smax.view, ssum.view, nparts, nparts, tval.view, M, lse=lse.view, out_logprob=lp.view)
    torch.cuda.synchronize()
    tval.check("target_val")
    lse.check("lse")
    lp.check("log-prob")
    return lse.view[:, 0], lp.view[:, 0]


@pytest.mark.parametrize("mode", ["128", "256-sched0", "256-sched6", "auto"])
@pytest.mark.parametrize("V", VOCABS)
def test_lm_head_rowstats_at_real_vocab(hip, V, mode):
    h, wte, tgt, ref_lse, ref_lp = lm_problem(V)
    tile, sched, want = {"128": (128, -1, PLAN_128), "256-sched0": (256, 0, PLAN_256), "256-sched6": (256, 6, PLAN_256S),
                         "auto": (0, -1, PLAN_256S)}[mode]
    with forced(hip, tile, sched), recording(hip) as plans:
        lse, lp = rowstats(hip, h, wte, tgt, LM_M, V, LM_K)
    assert plans == [want], plans
    e_lse, e_lp = max_err(lse, ref_lse), max_err(lp, ref_lp)
    print(f"ROWSTATS V={V} (mod 256 = {V % 256}) {mode}: plan {plans[0]}, |lse| err {e_lse:.2e}, |logprob| err {e_lp:.2e}")
    assert e_lse <= 2e-4 and e_lp <= 2e-4, (e_lse, e_lp)


# ============================================================================================== LM head: backward
def test_lm_head_backward_at_gpt2_vocab(hip):
    """engine.py CaptionDecoderEngine.backward, LM-head part: DLOGITS into [n, Vp] chunks (out_cols = ld = Vp), the NN data
    gradient with K = Vp (split-K at these chunk sizes) and the TN weight gradient with M = V, accumulated over two
    chunks (one of 1024 rows: 256^2 TN; one of 476: K % 64 != 0, the 128^2 kernel) - against float64 autograd of the
    log-softmax gather."""
    V, K, Mc, ck = V_GPT2, H, 1500, 1024
    Vp = (V + 127) // 128 * 128
    wte = randn((V, K), 11, 0.03, torch.bfloat16)
    wte_pad = torch.zeros(Vp, K, dtype=torch.bfloat16, device=dev())
    wte_pad[:V] = wte
    g = torch.Generator().manual_seed(5)
    peak = torch.randint(0, 128, (Mc,), generator=g).to(dev())
    h = randn((Mc, K), 12, 0.5)
    h[0::3] = 8.0 * wte[peak[0::3]].float()
    h = h.bfloat16()
    tgt = torch.randint(0, V, (Mc,), generator=g).to(dev())
    tgt[0::6] = peak[0::6]
    tgt[1], tgt[2], tgt[3], tgt[4] = 0, 127, 128, V - 1
    lse, _ = rowstats(hip, h, wte, tgt, Mc, V, K)
    rs = randn((Mc,), 13)                                 # row_scale: -dLoss/dtok_lp
    dhf = Guard(Mc, K, torch.float32, fill=torch.zeros(Mc, K, device=dev()))
    dwte = Guard(V, K, torch.float32, fill=torch.zeros(V, K, device=dev()))
    dl = Guard(ck, Vp, torch.bfloat16)
    dl_all = torch.empty(Mc, Vp, dtype=torch.bfloat16, device=dev())
    plans_all = []
    for r0 in range(0, Mc, ck):
        n = min(ck, Mc - r0)
        hfc = h[r0:r0 + n]
        with recording(hip) as plans:
            hip.gemm(hfc, wte, n, V, K, hip.NT, epilogue=hip.EPI_DLOGITS, targets=tgt[r0:r0 + n], row_lse=lse[r0:r0 + n],
                     row_scale=rs[r0:r0 + n], out_bf16=dl.full, ld_out_bf16=Vp, out_cols=Vp)
            hip.gemm(dl.full, wte_pad, n, K, Vp, hip.NN, lda=Vp, ldb=K, out_f32=dhf.view[r0:r0 + n], accumulate=True)
            hip.gemm(dl.full, hfc, V, K, n, hip.TN, lda=Vp, ldb=K, out_f32=dwte.view, accumulate=True)
        torch.cuda.synchronize()
        dl.check(f"dlogits chunk at row {r0}", full=(n == ck))
        dl_all[r0:r0 + n] = dl.view[:n]
        plans_all.append(plans)
    # chunk 1 (1024 rows): DLOGITS 4 x 197 tiles; NN dgrad 16 tiles split 16 ways over K; TN wgrad 197 x 4 tiles, 2-stage
    # chunk 2 (476 rows): DLOGITS 2 x 197; NN 8 tiles (x 16 splits < 192): 128^2; TN has K = 476 (not % 64): 128^2
    assert plans_all == [[PLAN_256S, PLAN_256S + 15, PLAN_256], [PLAN_256S, PLAN_128, PLAN_128]], plans_all
    dhf.check("dhf")
    dwte.check("dwte")
    assert float(dl_all[:, V:].abs().max()) == 0.0, "padding columns of dlogits must be exactly 0"
    hd, wd = h.double().requires_grad_(), wte.double().requires_grad_()
    logp = torch.log_softmax(hd @ wd.t(), -1)
    (-(rs.double() * logp.gather(-1, tgt[:, None]).squeeze(-1)).sum()).backward()
    dlog_ref = rs.double()[:, None] * (logp.detach().exp() - torch.nn.functional.one_hot(tgt, V).double())
    e_dl = close(dl_all[:, :V], dlog_ref, 1.0 / 100, "dlogits")
    # the two GEMMs on the bf16 dlogits they were given: f32 accumulation error only
    e_nn = close(dhf.view, dl_all.double() @ wte_pad.double(), 2e-4, "dh = dlogits @ wte (K = Vp)")
    e_tn = close(dwte.view, dl_all[:, :V].double().t() @ h.double(), 2e-4, "dwte = dlogits^t @ h (M = V)")
    # and end to end against autograd (the bf16 rounding of dlogits included)
    e_h = close(dhf.view, hd.grad, 1.0 / 100, "dh vs autograd")
    e_w = close(dwte.view, wd.grad, 1.0 / 100, "dwte vs autograd")
    print(f"LM-head backward V={V}: plans {plans_all}; rel err dlogits {e_dl:.2e}, dgrad {e_nn:.2e} / {e_h:.2e}, "
          f"wgrad {e_tn:.2e} / {e_w:.2e} (exact-operand / autograd)")


# ============================================================================================== LM head: engine
def test_engine_token_logprobs_at_gpt2_vocab():
    """``CaptionDecoderEngine.token_logprobs`` at GPT-2-M width and the decoder vocabulary (50260: the same 256^2 overrun
    class as 50257), fed a hidden state directly.  Rows are peaked on their own target (ids < 128 for some), so a lost
    strip costs O(1).  Reference: float64 log-softmax over the engine's own bf16 ln_f output and the bf16 wte mirror."""
    from pgca_amd.arch import make_arch, with_layers
    from pgca_amd.engine import make_seq_batch
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    arch = with_layers(make_arch("openai/clip-vit-base-patch32", "gpt2-medium", 512), 1, 1)
    model = PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=arch, seed=4, device="cuda:0")
    eng = model.caption_decoder.engine
    V = eng.V
    assert eng.arch.gpt.hidden == H and V == 50260
    eng.wte.w.mul_(2.0)                                 # N(0, 0.04): peakier logits
    eng.seg.ensure_bf16()
    g = torch.Generator().manual_seed(9)
    Bq, S = 4, 128
    ids = torch.randint(0, V, (Bq, S), generator=g)
    ids[0, 1::2] = torch.randint(0, 128, (len(range(1, S, 2)),), generator=g)
    ids[1, 1:5] = torch.tensor([0, 127, 128, V - 1])
    ids[2, 1::3] = V - 1 - torch.randint(0, V % 256, (len(range(1, S, 3)),), generator=g)   # last, partial tile
    lens = torch.tensor([128, 100, 77, 31])
    mask = (torch.arange(S)[None] < lens[:, None]).long()
    sb = make_seq_batch(ids, mask, dev(), pack=False)
    Mc = sb.n_rows
    hL = randn((Bq * S, H), 21, 1.0)
    # rows scored against ids[b, t + 1] point along that id's embedding (ln_f keeps the direction): peaked on the target
    rows = torch.arange(Bq * S, device=dev())
    aligned = (rows % 3) != 2
    nxt = torch.cat([ids[:, 1:], ids[:, :1]], 1).reshape(-1).to(dev())
    hL[aligned] = 30.0 * eng.wte.w[nxt[aligned]] + 0.05 * hL[aligned]
    tok = eng.token_logprobs(hL, sb, save=False).clone()
    torch.cuda.synchronize()
    hf = eng.ws.bufs[f"{eng.tag}.hf"][:Mc * H].view(Mc, H)
    logp = torch.log_softmax(hf.double() @ eng.wte.b.double().t(), -1)
    ref = logp.gather(-1, sb.targets[:, None]).squeeze(-1)
    err = max_err(tok, ref)
    small = sb.targets < 128
    print(f"engine token_logprobs V={V}: {Mc} rows ({int(small.sum())} with target < 128), max |logprob err| {err:.2e}, "
          f"mean target log-prob {float(ref.mean()):.3f}")
    assert int((ref[small] > -0.5).sum()) >= 32        # the test really is peaked on targets < 128
    assert err <= 1e-3, err


# ============================================================================================== GPT-2-M block at bench M
# The launches of one GptTrunk block (engine.py GptTrunk.forward / .backward, train mode, GELU pair on):
#   name    layout  A          B (stored)      N       K       epilogue / extras
LAUNCHES = {
    "qkv":  ("NN", H, 3 * H, "bias -> bf16"),                   # ln1 @ c_attn.weight + b -> qkv
    "proj": ("NN", H, H, "bias + f32 residual, dropout"),        # att @ c_proj.weight + b, resid dropout, + h -> hm
    "fc":   ("NN", H, I, "GELU_NEW_D -> bf16 + aux_out"),       # ln2 @ c_fc.weight + b -> gelu, gelu' (saved)
    "fc2":  ("NN", I, H, "bias + f32 residual, dropout"),        # act @ mlp.c_proj.weight + b, resid dropout, + hm -> hn
    "dfc2": ("NT", H, I, "MUL_AUX + colsum -> bf16"),           # g_bf @ mlp.c_proj.weight^t * gelu' -> dpre, bias-grad sums
    "dfc":  ("NT", I, H, "-> bf16"),                             # dpre @ c_fc.weight^t -> dln
    "dproj": ("NT", H, H, "-> bf16"),                            # g2_bf @ c_proj.weight^t -> datt
    "dqkv": ("NT", 3 * H, H, "-> bf16"),                         # dqkv @ c_attn.weight^t -> dln
}
DROP_P = 0.1


def drop_rows_for(M):
    """A packed->padded row map that is neither the identity nor monotone (entries < 8191 keep the oracle mask small)."""
    r = torch.arange(M, dtype=torch.int64)
    return ((r * 7919 + 13) % 8191).to(torch.int32).to(dev())


def drop_mult(seed, M, N, rows):
    return R.dropout_multiplier(seed, DROP_P, 8191 * N).view(8191, N).to(dev())[rows.long()]


def run_launch(hip, name, M, ops, outs, drop_seed=None, rows=None):
    """Issue launch ``name`` exactly as GptTrunk does.  ops: A, B, bias, aux_in, residual; outs: Guards."""
    layout, K, N, _ = LAUNCHES[name]
    lay = hip.NN if layout == "NN" else hip.NT
    A, B = ops["A"], ops["B"]
    kw = {}
    if "bf16" in outs:
        kw.update(out_bf16=outs["bf16"].full, ld_out_bf16=outs["bf16"].ld)
    if "f32" in outs:
        kw.update(out_f32=outs["f32"].full, ld_out_f32=outs["f32"].ld)
    if ops.get("bias") is not None:
        kw["bias"] = ops["bias"]
    if name in ("proj", "fc2"):
        res = ops["residual"]
        kw.update(residual=res.full, ld_res=res.ld)
        if drop_seed is not None:
            kw.update(drop=hip.drop_args(drop_seed, DROP_P), drop_rows=rows)
    if name == "fc":
        kw.update(epilogue=hip.EPI_GELU_NEW_D, aux_out=outs["aux"].full, ld_aux=outs["aux"].ld)
    if name == "dfc2":
        kw.update(epilogue=hip.EPI_MUL_AUX, aux_in=ops["aux_in"], ld_aux=N, colsum_part=outs["colsum"].full)
    hip.gemm(A, B, M, N, K, lay, **kw)


def make_outs(name, M, N, f32_fill=None):
    ld = N + 8                                          # every output row strided past N: trailing guard columns
    outs = {}
    if name in ("proj", "fc2"):
        outs["f32"] = Guard(M, N, torch.float32, ld=ld, fill=f32_fill)
    else:
        outs["bf16"] = Guard(M, N, torch.bfloat16, ld=ld)
    if name == "fc":
        outs["aux"] = Guard(M, N, torch.bfloat16, ld=ld)
    if name == "dfc2":
        outs["colsum"] = Guard((M + 63) // 64, N, torch.float32, ld=ld)
    return outs


def make_ops(name, M, exact, seed):
    layout, K, N, _ = LAUNCHES[name]
    if exact:
        A = ints((M, K), seed)
        Bm = ints((K, N), seed + 1)                     # math operand: C = A @ Bm
        bias = lambda: ints((N,), seed + 2, -8, 8, torch.float32)
        aux = lambda: ints((M, N), seed + 3)
        res = lambda: ints((M, N), seed + 4, -64, 64, torch.float32)
    else:
        A = randn((M, K), seed, 1.0, torch.bfloat16)
        Bm = randn((K, N), seed + 1, K ** -0.5, torch.bfloat16)
        bias = lambda: randn((N,), seed + 2, 0.5)
        aux = lambda: randn((M, N), seed + 3, 1.0, torch.bfloat16)
        res = lambda: randn((M, N), seed + 4, 1.0)
    B = Bm if layout == "NN" else Bm.t().contiguous()  # NN: Conv1D [in, out]; NT: the same weight read transposed
    ops = {"A": A, "B": B, "Bm": Bm}
    if name in ("qkv", "proj", "fc", "fc2"):
        ops["bias"] = bias()
    if name == "dfc2":
        ops["aux_in"] = aux()
    if name in ("proj", "fc2"):
        ops["residual_val"] = res()
    return ops


def ref_chunks(M, step=8192):
    for r0 in range(0, M, step):
        yield r0, min(M, r0 + step)


@pytest.fixture
def auto_dispatch(hip):
    hip.set_option("gemm_tile", 0)
    hip.set_option("gemm_schedule", -1)
    yield
    hip.set_option("gemm_tile", 0)
    hip.set_option("gemm_schedule", -1)


@pytest.mark.parametrize("name", [n for n in LAUNCHES if n != "fc"])   # GELU_NEW_D is transcendental: random pass
@pytest.mark.parametrize("M", [M_BENCH, M_ODD])
def test_trunk_gemm_exact_at_bench_rows(hip, auto_dispatch, name, M):
    """Integer operands: the f32 result of every launch is exact, so kernel == float32 torch BITWISE (bf16 outputs: the
    round-to-nearest-even of the exact value).  Sentinel-NaN outputs catch a missing tile, the accumulate pass a
    duplicated one, the guards a write outside the window.  Residual launches run in place (eval-mode GptTrunk)."""
    layout, K, N, _ = LAUNCHES[name]
    ops = make_ops(name, M, True, seed=10 * list(LAUNCHES).index(name))
    res_val = ops.get("residual_val")
    outs = make_outs(name, M, N, f32_fill=res_val)
    if res_val is not None:
        ops["residual"] = outs["f32"]                   # residual=h, out_f32=h: in place
    with recording(hip) as plans:
        run_launch(hip, name, M, ops, outs)
    torch.cuda.synchronize()
    for k, gd in outs.items():
        gd.check(f"{name} {k}")
    want = {}
    for r0, r1 in ref_chunks(M):
        acc = ops["A"][r0:r1].double() @ ops["Bm"].double()
        if "bias" in ops:
            acc = acc + ops["bias"].double()
        if name == "dfc2":
            acc = acc * ops["aux_in"][r0:r1].double()
        if res_val is not None:
            acc = acc + res_val[r0:r1].double()
        assert float(acc.abs().max()) < 2 ** 24
        acc = acc.float()
        if "f32" in outs:
            assert torch.equal(outs["f32"].view[r0:r1], acc), f"{name} f32 rows {r0}..{r1}: not bitwise equal"
        if "bf16" in outs:
            assert torch.equal(outs["bf16"].view[r0:r1], acc.bfloat16()), f"{name} bf16 rows {r0}..{r1}"
        if name == "dfc2":
            want[r0] = acc
    if name == "dfc2":
        cs = torch.cat([want[r0] for r0, _ in ref_chunks(M)])
        nbr = (M + 63) // 64
        ref_cs = torch.nn.functional.pad(cs, (0, 0, 0, nbr * 64 - M)).view(nbr, 64, N).double().sum(1).float()
        assert torch.equal(outs["colsum"].view, ref_cs), "dfc2 colsum partials"
    assert plans == [PLAN_256S], plans
    if name == "qkv":                                   # accumulate on a known value: a duplicated tile / K slice shows
        init = ints((M, N), 99, -1000, 1000, torch.float32)
        acc_out = Guard(M, N, torch.float32, ld=N + 8, fill=init)
        with recording(hip) as plans:
            hip.gemm(ops["A"], ops["B"], M, N, K, hip.NN, out_f32=acc_out.full, ld_out_f32=acc_out.ld, accumulate=True)
        torch.cuda.synchronize()
        acc_out.check("qkv accumulate")
        for r0, r1 in ref_chunks(M):
            ref = (init[r0:r1].double() + ops["A"][r0:r1].double() @ ops["Bm"].double()).float()
            assert torch.equal(acc_out.view[r0:r1], ref), f"accumulate rows {r0}..{r1}"
        assert plans == [PLAN_256S], plans
    print(f"TRUNK exact {name} M={M} N={N} K={K}: plan {PLAN_256S}, {tiles256(M, N)} tiles, bitwise equal")


@pytest.mark.parametrize("name", list(LAUNCHES))
@pytest.mark.parametrize("M", [M_BENCH, M_ODD])
def test_trunk_gemm_random_and_deterministic_at_bench_rows(hip, auto_dispatch, name, M):
    """Random operands against float64 (f32 outputs 2e-4, bf16 outputs one bf16 ulp, the GELU pair 1e-2 as in
    test_kernels_gpu.py), dropout keyed on a packed row map; then the same launch with the phase-staggered schedule
    forced (once more) and with the 2-stage schedule: all three bitwise equal."""
    layout, K, N, _ = LAUNCHES[name]
    ops = make_ops(name, M, False, seed=10 * list(LAUNCHES).index(name) + 107)
    res_val = ops.get("residual_val")
    if res_val is not None:
        ops["residual"] = Guard(M, N, torch.float32, ld=N + 8, fill=res_val)   # training: hm / hn are separate buffers
    seed = 0xBE11C0DE
    rows = drop_rows_for(M)
    results = []
    for tile, sched in ((0, -1), (256, 6), (256, 0)):
        outs = make_outs(name, M, N)
        with forced(hip, tile, sched), recording(hip) as plans:
            run_launch(hip, name, M, ops, outs, drop_seed=seed if res_val is not None else None, rows=rows)
        torch.cuda.synchronize()
        for k, gd in outs.items():
            gd.check(f"{name} {k} (tile {tile}, schedule {sched})")
        assert plans == [PLAN_256S if sched != 0 else PLAN_256], plans
        results.append(outs)
        if len(results) == 1:
            errs = check_random(name, M, N, ops, outs, seed, rows)
    for k in results[0]:
        for i, other in ((1, "schedule 6 again"), (2, "schedule 0")):
            a, b = results[0][k].view, results[i][k].view
            assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                               b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)), \
                f"{name} {k}: {other} differs from the first launch"
    print(f"TRUNK random {name} M={M} N={N} K={K}: plan {PLAN_256S}, {tiles256(M, N)} tiles, "
          + ", ".join(f"{k} rel err {v:.2e}" for k, v in errs.items()) + "; 3 launches bitwise equal")


def check_random(name, M, N, ops, outs, seed, rows):
    err = {}
    mult = drop_mult(seed, M, N, rows) if name in ("proj", "fc2") else None
    worst = {}
    scale = {}
    for r0, r1 in ref_chunks(M):
        pre = ops["A"][r0:r1].double() @ ops["Bm"].double()
        if "bias" in ops:
            pre = pre + ops["bias"].double()
        if name in ("proj", "fc2"):
            want = {"f32": pre * mult[r0:r1].double() + ops["residual_val"][r0:r1].double()}
        elif name == "fc":
            x = pre.clone().requires_grad_()
            y = R.gelu_new(x)
            y.sum().backward()
            want = {"bf16": y.detach(), "aux": x.grad}
        elif name == "dfc2":
            want = {"bf16": pre * ops["aux_in"][r0:r1].double()}
            want["colsum"] = want["bf16"]
        else:
            want = {"bf16": pre}
        for k, w in want.items():
            if k == "colsum":
                continue
            got = outs[k].view[r0:r1]
            worst[k] = max(worst.get(k, 0.0), max_err(got, w))
            scale[k] = max(scale.get(k, 0.0), float(w.abs().max()))
        if name == "dfc2":
            b0, b1 = r0 // 64, (r1 + 63) // 64
            w = torch.nn.functional.pad(want["colsum"], (0, 0, 0, (b1 - b0) * 64 - (r1 - r0)))
            w = w.view(b1 - b0, 64, N).sum(1)
            worst["colsum"] = max(worst.get("colsum", 0.0), max_err(outs["colsum"].view[b0:b1], w))
            scale["colsum"] = max(scale.get("colsum", 0.0), float(w.abs().max()))
    tol = {"f32": 2e-4, "bf16": 1.0 / 100 if name == "fc" else 1.0 / 128, "aux": 1.0 / 100, "colsum": 2e-3}
    for k in worst:
        rel = worst[k] / (scale[k] + 1e-12)
        assert rel <= tol[k], f"{name} {k}: rel err {rel:.3e} > {tol[k]} (max err {worst[k]:.3e}, scale {scale[k]:.3e})"
        err[k] = rel
    return err


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
def test_grouped_weight_gradient_at_bench_tokens(hip, exact):
    """The block's four weight gradients in one grid (gemm256_group_tn_kernel: 2-stage loop, whole K = 73152 tokens per
    tile, 64 + 64 + 16 + 48 = 192 tiles), accumulated on a known value: bitwise equal to float32 torch on integer operands,
    2e-4 of float64 on random ones."""
    K = M_BENCH
    # (X [K, M], dY [K, N]) as GptTrunk.backward lists them: act/g_bf, ln2/dpre, att/g2_bf, ln1/dqkv
    shapes = [(I, H), (H, I), (H, H), (H, 3 * H)]
    probs, inits, guards = [], [], []
    for i, (Mw, Nw) in enumerate(shapes):
        if exact:
            x, dy, g0 = ints((K, Mw), 40 + i), ints((K, Nw), 50 + i), ints((Mw, Nw), 60 + i, -1000, 1000, torch.float32)
        else:
            x, dy, g0 = randn((K, Mw), 40 + i, 1.0, torch.bfloat16), randn((K, Nw), 50 + i, 1.0, torch.bfloat16), \
                randn((Mw, Nw), 60 + i, 30.0)
        gd = Guard(Mw, Nw, torch.float32, fill=g0)
        probs.append((x, dy, Mw, Nw, K, gd.view))
        inits.append(g0)
        guards.append(gd)
    # pgca_gemm_bf16_grouped takes the one-grid path only when every problem qualifies (else one launch each):
    assert len(probs) <= 4 and K % 64 == 0 and all(m % 8 == 0 and n % 8 == 0 for _, _, m, n, _, _ in probs)
    assert sum(tiles256(m, n) for _, _, m, n, _, _ in probs) == 192
    hip.gemm_wgrad_group(probs)
    torch.cuda.synchronize()
    errs = []
    for (x, dy, Mw, Nw, _, out), g0, gd in zip(probs, inits, guards):
        gd.check(f"wgrad {Mw}x{Nw}")
        ref = g0.double()
        for k0, k1 in ref_chunks(K, 16384):
            ref += x[k0:k1].double().t() @ dy[k0:k1].double()
        if exact:
            assert float(ref.abs().max()) < 2 ** 24
            assert torch.equal(out, ref.float()), f"grouped wgrad {Mw}x{Nw}: not bitwise equal"
            errs.append(0.0)
        else:
            errs.append(close(out, ref, 2e-4, f"grouped wgrad {Mw}x{Nw}"))
    print(f"TRUNK wgrad group K={K} ({'exact' if exact else 'random'}): 192 tiles, rel err "
          + ", ".join(f"{e:.2e}" for e in errs))
