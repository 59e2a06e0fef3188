"""The kernels that are NOT GEMMs - attention, LayerNorm, the caption-decoder embedding, the small reductions - at the
geometry the benchmark launches them with, against plain float64 references (tests/row_kernel_refs.py, themselves
checked against autograd by test_row_kernel_references_cpu.py), inside sentinel-filled buffers (``Guard``).

Which case launches which kernel instance (attention_tiled.hip, layernorm.hip, misc.hip):

===========================================  ==============================================================================
case                                         kernels
===========================================  ==============================================================================
test_attention_c2[normal|sharp|exact]        attn_fwd_one_kernel, attn_bwd_tiled_kernel<1,true>: 2049 x 16 = 32784 workgroups
                                             (32 / 64 rounds of 256 CUs at 4 / 2 workgroups per CU), packed + padded
test_attention_tiled[c4_h20|c5_h25]          attn_fwd_tiled_kernel (nqb 2), attn_bwd_tiled_kernel<2,false>, packed, dropout
test_attention_tiled[vit_l14]                attn_fwd_tiled_kernel (nqb 3), attn_bwd_tiled_kernel<3,false>, T = 257, no mask
test_attention_tiled[s512]                   attn_fwd_tiled_kernel (nqb 4), attn_bwd_tiled_kernel<4,false>, 640 workgroups
test_attention_holes[128|256]                both families with key_mask holes and queries that have NO allowed key
test_layernorm_at_packed_rows[M-H]           ln_fwd_kernel<4|5|7>, ln_bwd_kernel<4|5|7,true> and <..,false>, 1024-block cap
test_embedding_at_packed_rows[1024-*]        embed_fwd_kernel<4>, embed_bwd_kernel<4,true>, wpe_grad_kernel (8 slices)
test_embedding_at_packed_rows[1600-*]        embed_fwd_kernel<7>, embed_bwd_kernel<7,false> (nv > 4), wpe_grad_kernel
test_small_reductions_at_2048_sequences      masked_mean_fwd/bwd (padded, cu), seq_reduce (modes 0, 1), colsum (256-block cap)
===========================================  ==============================================================================

Error measure: the error of output row r (attention: of row r of one head) is taken against that row's OWN scale,
max |ref[r]| + FLOOR * max |ref| - a long sequence's output row is ten times smaller than a short one's and must not hide
behind it.  The bounds are the existing constants of test_kernels_gpu.py / test_attention_tiled_gpu.py (now per row); for
attention additionally, per row of a head and for every input distribution, 4 x the error of the float64 emulation with
the kernels' rounding points plus one bf16 ulp of the row scale plus one bf16 ulp of O carried through delta (see
``AttnCase.compare``); for f32 sums sqrt(n) * eps * sum |terms| from the reference (``row_kernel_refs.sum_bound``).  Attention,
LayerNorm and the partial-sum kernels use no atomics: two launches must be bitwise equal.  ``embed_bwd_kernel`` and
``wpe_grad_kernel`` DO use atomics and are compared with float64 only.  Run with ``-s`` for the measured figures.
"""
import pytest
import torch

import row_kernel_refs as K
from test_bench_geometry_gpu import Guard, dev, gen, hip, randn  # noqa: F401  (hip is a fixture)

pytestmark = pytest.mark.gpu

F64 = torch.float64
FLOOR = 1.0 / 64          # floor of a row's scale, as a fraction of the global maximum of the reference
BF16_ULP = 2.0 ** -8
EDGE_LENS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]


def report(case, what, measured, bound, source):
    print(f"[{case}] {what}: measured {measured:.3e}  bound {bound:.3e}  ({source})")


def holds(case, what, err, bound, source):
    """err, bound: tensors of the same shape (per row / element) or floats; asserts err <= bound everywhere and prints the
    entry that is closest to its bound."""
    err = torch.as_tensor(err, dtype=F64)
    bound = torch.as_tensor(bound, dtype=F64, device=err.device).expand_as(err)
    ratio = (err / bound.clamp(min=1e-300)).flatten()
    worst = int(ratio.argmax())
    report(case, what, float(err.flatten()[worst]), float(bound.flatten()[worst]),
           f"{source}; worst entry {worst} at {float(ratio[worst]):.3f} of its bound")
    assert bool((err <= bound).all()), f"[{case}] {what}: entry {worst} is at {float(ratio[worst]):.3f} x its bound ({source})"
    return float(ratio[worst])


# =============================================================================================== attention
class AttnCase:
    """One attention geometry: the layout (packed through ``make_row_pack`` or padded), the inputs of one distribution and
    the per-sequence index maps that the chunked float64 reference gathers with."""

    def __init__(self, lens, S, heads, causal, packed, p, dist, holes=(), seed=1):
        from pgca_amd.engine import PACK_PAD, make_row_pack
        self.S, self.heads, self.causal, self.p, self.dist = S, heads, causal, p, dist
        self.H = heads * 64
        Bq = len(lens)
        lens = torch.as_tensor(lens)
        mask = (torch.arange(S)[None] < lens[:, None]).int()
        for b, t in holes:
            mask[b, t] = 0
        self.mask_padded = mask.to(dev())
        self.Bq = Bq
        if packed:
            pk = make_row_pack(self.mask_padded)
            assert pk.Mp % PACK_PAD == 0 and pk.n == int(lens.sum()) and int(pk.lens.min()) >= 1
            self.pk, self.nseq, self.rows, self.cu, self.kmask = pk, pk.nseq, pk.Mp, pk.cu, pk.mask
            cu = pk.cu.long()
            self.seq_len = cu[1:] - cu[:-1]
            self.row0 = cu[:-1]
        else:
            self.pk, self.nseq, self.rows, self.cu = None, Bq, Bq * S, None
            self.kmask = self.mask_padded if (holes or bool((lens < S).any())) else None
            self.seq_len = torch.full((Bq,), S, device=dev())
            self.row0 = torch.arange(Bq, device=dev()) * S
        assert int(self.seq_len.max()) <= S and int(self.seq_len.sum()) == self.rows
        self.key_ok = self.kmask if self.kmask is not None else torch.ones(self.nseq, S, dtype=torch.int32, device=dev())
        self.seed = 0x5EED0 + seed
        self.make_inputs(seed)

    def make_inputs(self, seed):
        g, rows, H, heads = gen(seed), self.rows, self.H, self.heads
        if self.dist == "normal":
            qkv = torch.randn(rows, 3 * H, generator=g, device=dev())
            dout = torch.randn(rows, H, generator=g, device=dev())
        elif self.dist == "sharp":
            # generated per PADDED position so that key 0 of every sequence is its sink, then gathered to the rows
            qkv = torch.zeros(rows, 3 * H, device=dev())
            for b0 in range(0, self.nseq, 256):
                nb = min(256, self.nseq - b0)
                x = K.sharp_qkv(nb, self.S, heads, g, shift_head=heads - 1).view(nb, self.S, 3 * H)
                idx, ok = self.gather_index(b0, nb)
                qkv[idx[ok]] = x[ok]
            dout = torch.randn(rows, H, generator=g, device=dev())
        else:  # exact: q = 0 (uniform P over the allowed keys), small-integer v and dout
            qkv = torch.randn(rows, 3 * H, generator=g, device=dev())
            qkv[:, :H] = 0.0
            qkv[:, 2 * H:] = torch.randint(-3, 4, (rows, H), generator=g, device=dev()).float()
            dout = torch.randint(-2, 3, (rows, H), generator=g, device=dev()).float()
        if self.pk is not None and self.pk.Mp > self.pk.n:   # the filler rows are zero embeddings in the engine
            qkv[self.pk.n:] = 0.0
            dout[self.pk.n:] = 0.0
        self.qkv, self.dout = qkv.bfloat16(), dout.bfloat16()

    def gather_index(self, b0, nb):
        """[nb, S] row index of position (b, t) and its validity (t < this sequence's row count)."""
        t = torch.arange(self.S, device=dev())[None]
        ok = t < self.seq_len[b0:b0 + nb, None]
        return torch.where(ok, self.row0[b0:b0 + nb, None] + t, torch.zeros_like(t)), ok

    def launch(self, hip):
        """Forward + backward into fresh guards."""
        out = Guard(self.rows, self.H, torch.bfloat16)
        lse = Guard(self.nseq * self.heads, self.S, torch.float32)
        dqkv = Guard(self.rows, 3 * self.H, torch.bfloat16)
        d = hip.drop_args(self.seed, self.p)
        hip.attention_fwd(self.qkv, self.kmask, self.nseq, self.S, self.heads, self.causal, out.view, lse.view, drop=d,
                          cu=self.cu)
        hip.attention_bwd(self.qkv, out.view, self.dout, lse.view, self.kmask, self.nseq, self.S, self.heads, self.causal,
                          dqkv.view, drop=d, cu=self.cu)
        torch.cuda.synchronize()
        return out, lse, dqkv

    def check_guards(self, case, out, lse, dqkv):
        out.check(f"[{case}] out")
        dqkv.check(f"[{case}] dqkv")
        lse.check(f"[{case}] lse", full=False)
        # lse [nseq, heads, S]: slot t of sequence b is written iff t < its row count; every other slot keeps the sentinel
        written = (lse.raw[:self.nseq * self.heads * self.S] != lse.sentinel).view(self.nseq, self.heads, self.S)
        want = (torch.arange(self.S, device=dev())[None] < self.seq_len[:, None])[:, None, :].expand_as(written)
        assert torch.equal(written, want), f"[{case}] lse: written slots differ from t < len in " \
                                           f"{int((written != want).sum())} places"

    def compare(self, case, out, lse, dqkv):
        """Chunked float64 reference; returns the dict of measured figures."""
        S, heads, H = self.S, self.heads, self.H
        sharp = self.dist == "sharp"
        nb_max = max(1, (1 << 25) // (heads * S * S))
        lse_k = lse.view.view(self.nseq, heads, S)
        names = ("out", "dq", "dk", "dv")
        err, emu, mag, ulp_o = ({n: [] for n in names} for _ in range(4))
        dots = {n: [0.0] * 5 for n in names}
        row_err, row_mag = {"out": [], "dqkv": []}, {"out": [], "dqkv": []}
        lse_err, exact_worst = 0.0, 0.0
        zero = torch.zeros((), dtype=torch.bfloat16, device=dev())
        for b0 in range(0, self.nseq, nb_max):
            nb = min(nb_max, self.nseq - b0)
            idx, ok = self.gather_index(b0, nb)
            take = lambda x: torch.where(ok[..., None], x[idx], zero)  # noqa: E731
            x = take(self.qkv).view(nb * S, 3 * H)
            q, k, v = (K.split_heads(x[:, i * H:(i + 1) * H], nb, S, heads) for i in range(3))
            do = K.split_heads(take(self.dout).view(nb * S, H), nb, S, heads)
            allowed = K.attn_allowed(self.key_ok[b0:b0 + nb], S, self.causal) & ok[:, None, None, :]
            mult = K.attn_drop_mult(self.seed, self.p, b0, nb, heads, S, dev()) if self.p > 0 else None
            ref_out, ref_lse, P = K.attn_fwd_ref(q, k, v, allowed, mult)
            ref = dict(zip(names, (ref_out,) + K.attn_bwd_ref(q, k, v, do, allowed, mult)))
            got_x = take(dqkv.view).view(nb * S, 3 * H)
            got = {"out": K.split_heads(take(out.view).view(nb * S, H), nb, S, heads)}
            for i, n in enumerate(("dq", "dk", "dv")):
                got[n] = K.split_heads(got_x[:, i * H:(i + 1) * H], nb, S, heads)
            em = dict(zip(names, K.attn_emulated(q, k, v, do, allowed, mult)))
            rows_ok = ok[:, None, :].expand(nb, heads, S)
            # The backward takes delta[q] = dO[q] . O[q] from the STORED bf16 output.  The kernel's O and the emulation's
            # may differ by one bf16 ulp per element (summation order, hardware exp); through dS = P (dP - delta) / 8 that
            # moves dq[q] by at most A[q] / 8 * max |k| and dk[key] by sum_q P[q, key] A[q] / 8 * max |q[q]|, with
            # A[q] = ulp * sum_d |dO[q, d] O[q, d]| - an amount that does NOT shrink with the row's own scale when all
            # keys share a large common component (the -80 head, the sink channel), where sum_key dS = 0 only holds for
            # the exact delta.  out and dv do not depend on delta.
            A = BF16_ULP * (do * ref_out).abs().sum(-1)                                     # [nb, heads, S]
            kmax = k.abs().amax(-1).masked_fill(~ok[:, None, :], 0.0).amax(-1, keepdim=True)   # [nb, heads, 1]
            zero_p = torch.zeros(nb, heads, S, dtype=F64, device=dev())
            prop = {"out": zero_p, "dv": zero_p, "dq": A * 0.125 * kmax,
                    "dk": (P.transpose(-1, -2) @ (A * 0.125 * q.abs().amax(-1))[..., None]).squeeze(-1)}
            for n in names:
                err[n].append((got[n] - ref[n]).abs().amax(-1)[rows_ok])
                mag[n].append(ref[n].abs().amax(-1)[rows_ok])
                a, b = got[n][rows_ok], ref[n][rows_ok]
                d = dots[n]
                d[0] += float((a * b).sum()); d[1] += float((a * a).sum()); d[2] += float((b * b).sum())
                emu[n].append((em[n] - ref[n]).abs().amax(-1)[rows_ok])
                ulp_o[n].append(prop[n][rows_ok])
                e = em[n][rows_ok]
                d[3] += float((e * b).sum()); d[4] += float((e * e).sum())
            # whole rows of the two output tensors (out [rows, H], dqkv [rows, 3H]), as the existing tests measure them
            for key, group in (("out", ("out",)), ("dqkv", ("dq", "dk", "dv"))):
                ge = torch.stack([(got[n] - ref[n]).abs().amax(-1).amax(1) for n in group]).amax(0)
                gm = torch.stack([ref[n].abs().amax(-1).amax(1) for n in group]).amax(0)
                row_err[key].append(ge[ok]); row_mag[key].append(gm[ok])
            lk = lse_k[b0:b0 + nb].to(F64)
            fin = rows_ok & torch.isfinite(ref_lse)
            assert torch.equal(torch.isinf(lk) & rows_ok, torch.isinf(ref_lse) & rows_ok), f"[{case}] lse: -inf pattern differs"
            assert bool((lk[rows_ok & ~fin] < 0).all())
            lse_err = max(lse_err, float((lk - ref_lse)[fin].abs().max()))
            if self.dist == "exact":   # closed form: P uniform over the allowed keys
                cnt = allowed.sum(-1, keepdim=True).to(F64).expand(nb, heads, S, 1)
                w = allowed.to(F64) / cnt.clamp(min=1) * (mult if mult is not None else 1.0)
                cf = w @ v
                tol = BF16_ULP * cf.abs() + (BF16_ULP * (w @ v.abs()) if mult is not None else 0.0) + 1e-6
                exact_worst = max(exact_worst, float(((got["out"] - cf).abs() / tol)[rows_ok].max()))
                assert float((lk - torch.log(cnt.squeeze(-1)))[fin].abs().max()) <= 1e-5, f"[{case}] lse != log(count)"
                assert float(got["dk"][rows_ok].abs().max()) == 0.0, f"[{case}] dk must be exactly 0 when q = 0"
        fig = {"lse": lse_err}
        # (1) every row of one head, of out / dq / dk / dv separately, against the float64 emulation of the kernels' own
        # rounding points: the finest measure, and the only one with a derived bound for every input distribution
        for n in names:
            e, m, ee = torch.cat(err[n]), torch.cat(mag[n]), torch.cat(emu[n])
            scale = m + FLOOR * m.max()
            room = BF16_ULP * scale + torch.cat(ulp_o[n])
            d = dots[n]
            if d[2] == 0.0:   # the reference is identically zero (dk when q = 0): so must the kernel's be
                assert d[1] == 0.0, f"[{case}] {n}: reference is zero, kernel output is not"
                continue
            cos = d[0] / max((d[1] * d[2]) ** 0.5, 1e-300)
            cos_e = d[3] / max((d[4] * d[2]) ** 0.5, 1e-300)
            fig[n] = holds(case, n + " per row of a head", e, 4.0 * ee + room,
                           "4 x float64 emulation with the kernel's rounding points + 1 bf16 ulp of the row scale"
                           " + 1 bf16 ulp of O carried through delta")
            fig[n + "_x_emulation"] = float((e / (ee + room)).max())
            fig[n + "_rel"] = float((e / scale).max())
            print(f"[{case}] {n}: worst kernel error / (emulation error + 1 ulp) = {fig[n + '_x_emulation']:.3f}; "
                  f"worst error / row scale = {fig[n + '_rel']:.3e}")
            if sharp:   # 4 x the error = 16 x the cosine defect of the emulation, plus the existing 5e-4
                holds(case, n + " cosine defect", 1.0 - cos, 16.0 * max(1.0 - cos_e, 0.0) + 5e-4,
                      "16 x (1 - cosine of the emulation) + existing 5e-4")
            else:
                holds(case, n + " cosine defect", 1.0 - cos, 5e-4, "existing constant 0.9995, global")
            fig[n + "_cos"] = cos
        # (2) the existing constants, per whole row of the output tensor, for the inputs they were stated for (unit
        # normals).  Measured for the record on the exact inputs, where q = 0 makes dk vanish and leaves the row scale to
        # dq and dv alone: 1/40 is met everywhere except S = 512, one head (1.05 x, the delta term above); those inputs are
        # held to the closed form, to (1) and to the global cosine instead.
        if self.dist == "normal":
            for key, rel in (("out", 1.0 / 64), ("dqkv", 1.0 / 40)):
                e, m = torch.cat(row_err[key]), torch.cat(row_mag[key])
                fig[key + "_row"] = holds(case, key + " per row", e / (m + FLOOR * m.max()), rel,
                                          f"existing constant 1/{round(1 / rel)}, per row")
        holds(case, "lse", lse_err, 2e-3, "existing constant, absolute")
        if self.dist == "exact":
            holds(case, "out vs closed form", exact_worst, 1.0, "bf16 rounding of the output (+ of the dropout multiplier)")
        return fig


def run_attention(hip, case, c):
    out, lse, dqkv = c.launch(hip)
    c.check_guards(case, out, lse, dqkv)
    fig = c.compare(case, out, lse, dqkv)
    out2, lse2, dqkv2 = c.launch(hip)   # no atomics anywhere: a second launch is bitwise equal, at full occupancy
    for a, b, n in ((out, out2, "out"), (lse, lse2, "lse"), (dqkv, dqkv2, "dqkv")):
        assert torch.equal(a.raw, b.raw), f"[{case}] {n}: two launches differ"
    return out, lse, dqkv, fig


def c2_lens():
    """2048 caption lengths ~ U{16..128} as bench.synthetic_batch draws them, the first ones replaced by the 16-query-block
    edges and the 64-row split of the two-blocks-per-wave forward."""
    lens = torch.randint(16, 129, (2048,), generator=torch.Generator().manual_seed(2048))
    lens[:len(EDGE_LENS)] = torch.tensor(EDGE_LENS)
    return lens


@pytest.mark.parametrize("dist", ["normal", "sharp", "exact"])
def test_attention_c2(hip, dist):
    """C2 training geometry: 16 heads, S = 128, causal, 2048 packed sequences + the filler, probability dropout 0.1."""
    case = f"c2/{dist}"
    c = AttnCase(c2_lens(), 128, 16, True, True, 0.1, dist)
    assert c.nseq == 2049 and c.heads == 16 and (c.S + 127) // 128 == 1          # attn_fwd_one_kernel / bwd<1, true>
    assert c.nseq * c.heads >= 64 * 256                                          # >= 16 rounds of 4 workgroups per CU
    assert int(c.pk.lens.min()) == 1 and c.rows % 64 == 0
    out, lse, dqkv, _ = run_attention(hip, case, c)
    if dist != "normal":
        return
    # the same batch in the padded layout: every real row bitwise equal to the packed launch
    S, H, heads, Bq = c.S, c.H, c.heads, c.Bq
    rows = c.pk.row_ids[:c.pk.n].long()
    qkv_p = torch.zeros(Bq * S, 3 * H, dtype=torch.bfloat16, device=dev())
    dout_p = torch.zeros(Bq * S, H, dtype=torch.bfloat16, device=dev())
    qkv_p[rows], dout_p[rows] = c.qkv[:c.pk.n], c.dout[:c.pk.n]
    o, l, dq = Guard(Bq * S, H, torch.bfloat16), Guard(Bq * heads, S, torch.float32), Guard(Bq * S, 3 * H, torch.bfloat16)
    d = hip.drop_args(c.seed, c.p)
    hip.attention_fwd(qkv_p, c.mask_padded, Bq, S, heads, True, o.view, l.view, drop=d)
    hip.attention_bwd(qkv_p, o.view, dout_p, l.view, c.mask_padded, Bq, S, heads, True, dq.view, drop=d)
    torch.cuda.synchronize()
    for gd, n in ((o, "out"), (l, "lse"), (dq, "dqkv")):
        gd.check(f"[{case}] padded {n}")                 # the padded layout computes every row, padding included
    assert torch.equal(o.view[rows], out.view[:c.pk.n]), "padded vs packed: forward rows differ"
    assert torch.equal(dq.view[rows], dqkv.view[:c.pk.n]), "padded vs packed: backward rows differ"
    real = c.mask_padded.bool()[:, None, :].expand(Bq, heads, S)
    assert torch.equal(l.view.view(Bq, heads, S)[real], lse.view.view(c.nseq, heads, S)[:Bq][real])


def tiled_case(name, dist):
    g = torch.Generator().manual_seed(len(name))
    if name in ("c4_h20", "c5_h25"):
        lens = torch.randint(16, 257, (256,), generator=g)
        lens[:6] = torch.tensor([1, 127, 128, 129, 255, 256])
        return AttnCase(lens, 256, 20 if name == "c4_h20" else 25, True, True, 0.1, dist), 2
    if name == "vit_l14":
        return AttnCase([257] * 128, 257, 16, False, False, 0.0, dist), 3
    lens = torch.randint(1, 513, (640,), generator=g)      # s512: one head, B >= 600
    lens[:6] = torch.tensor([512, 511, 385, 384, 257, 1])
    return AttnCase(lens, 512, 1, True, False, 0.1, dist), 4


@pytest.mark.parametrize("dist", ["normal", "sharp", "exact"])
@pytest.mark.parametrize("name", ["c4_h20", "c5_h25", "vit_l14", "s512"])
def test_attention_tiled(hip, name, dist):
    """The key-tiled forward and attn_bwd_tiled_kernel<2..4,false> at C4 / C5 (20 / 25 heads, S = 256), ViT-L/14 (T = 257)
    and S = 512 with several rounds of workgroups."""
    c, nqb = tiled_case(name, dist)
    assert (c.S + 127) // 128 == nqb and c.nseq * c.heads >= 600
    if name in ("c4_h20", "c5_h25"):
        assert c.nseq == 257 and 3 * c.H in (3840, 4800) and c.rows % 64 == 0
    run_attention(hip, f"{name}/{dist}", c)


@pytest.mark.parametrize("S", [128, 256])
def test_attention_holes(hip, S):
    """key_mask holes inside captions, some at position 0: the first causal queries of those sequences have NO allowed key.
    Contract (include/pgca_hip.h): out = 0, lse = -inf, no gradient through that row - in the one-tile forward, the tiled
    forward and the backward alike."""
    lens = [S, S // 2 + 3, 40, 17, S - 1, 1, S, 64, 65, S, 33, S]
    holes = ((0, 5), (0, 6), (1, 0), (2, 0), (2, 1), (4, S // 2), (6, 100), (9, S - 2))
    c = AttnCase(lens, S, 4, True, True, 0.1, "normal", holes=holes, seed=S)
    out, lse, dqkv, _ = run_attention(hip, f"holes/{S}", c)
    H = c.H
    lse_k = lse.view.view(c.nseq, 4, S)
    for b, nq in ((1, 1), (2, 2)):                       # sequence 2: keys 0 and 1 masked -> queries 0 and 1 see nothing
        r0 = int(c.row0[b])
        assert float(out.view[r0:r0 + nq].float().abs().max()) == 0.0
        assert bool((lse_k[b, :, :nq] == float("-inf")).all())
        assert float(dqkv.view[r0:r0 + nq, :H].float().abs().max()) == 0.0           # dq of the empty rows
        assert float(dqkv.view[r0:r0 + nq, H:].float().abs().max()) == 0.0           # dk, dv of the masked keys
        assert bool(torch.isfinite(lse_k[b, :, nq:int(c.seq_len[b])]).all())
    assert bool(torch.isfinite(out.view.float()).all()) and bool(torch.isfinite(dqkv.view.float()).all())


# =============================================================================================== LayerNorm
_pack_cache = {}


def c2_row_ids():
    """Packed -> padded position map (row_ids, -1 for filler rows) of the C2 attention batch."""
    if "ids" not in _pack_cache:
        from pgca_amd.engine import make_row_pack
        mask = (torch.arange(128)[None] < c2_lens()[:, None]).int().to(dev())
        _pack_cache["ids"] = make_row_pack(mask).row_ids.clone()
    return _pack_cache["ids"]


def per_row(case, what, got, ref, rel, source, skip_rows=()):
    e, _ = K.row_errors(got, ref, FLOOR)
    if len(skip_rows):
        e = e.clone()
        e[torch.as_tensor(skip_rows, device=e.device)] = 0.0
    return holds(case, what, e, rel, source)


@pytest.mark.parametrize("H", [1024, 1280, 1600])
@pytest.mark.parametrize("M", [73152, 70001])
def test_layernorm_at_packed_rows(hip, M, H):
    case = f"ln/{M}x{H}"
    R_in = M + 300
    nb = hip.layernorm_bwd_blocks(M)
    assert nb == 1024 and (M + 3) // 4 > 4 * nb                       # the grid-stride loop takes > 4 trips
    x = randn((R_in, H), H + M)
    rmap = torch.randperm(R_in, generator=torch.Generator().manual_seed(M))[:M].to(dev())   # a gather without repeats
    x[rmap[:3]] = K.ln_stress_rows(H, gen(5))                         # output rows 0, 1, 2
    MEAN1E3 = 1
    gamma, beta = randn((H,), 1) * 0.1 + 1, randn((H,), 2) * 0.1
    rmap32 = rmap.int()
    yb, yf = Guard(M, H, torch.bfloat16), Guard(M, H, torch.float32)
    mean, rstd = Guard(M, 1, torch.float32), Guard(M, 1, torch.float32)
    hip.layernorm_fwd(x, M, H, gamma, beta, row_map=rmap32, y_bf16=yb.view, y_f32=yf.view, mean=mean.full, rstd=rstd.full)
    torch.cuda.synchronize()
    for gd, n in ((yb, "y_bf16"), (yf, "y_f32"), (mean, "mean"), (rstd, "rstd")):
        gd.check(f"[{case}] {n}")
    xs, g64, b64 = x[rmap].to(F64), gamma.to(F64), beta.to(F64)
    ref, rmean, rrstd = K.ln_fwd_ref(xs, g64, b64)
    per_row(case, "y_f32", yf.view, ref, 1e-5, "existing constant 1e-5, per row", skip_rows=[MEAN1E3])
    per_row(case, "y_bf16", yb.view, ref, 1.0 / 128, "existing constant 1/128, per row")
    holds(case, "mean", (mean.view[:, 0].to(F64) - rmean).abs(), 8 * 2.0 ** -24 * xs.abs().amax(-1), "8 f32 ulps of max |x[r]|")
    holds(case, "rstd", (rstd.view[:, 0].to(F64) - rrstd).abs(), 1e-5 * rrstd, "existing constant 1e-5 of rstd[r]")
    for i, n in enumerate(K.LN_STRESS):
        e = float((yf.view[i].to(F64) - ref[i]).abs().max())
        holds(case, f"stress row {n}: y_f32", e, float(K.ln_stress_fwd_bound(xs[i], g64, ref[i], rrstd[i])),
              "1e-5 of the row + f32 rounding of x - mean")
    assert abs(float(rstd.view[0, 0]) - 1e-5 ** -0.5) <= 1e-5 * 1e-5 ** -0.5          # constant row: variance 0
    del ref

    # ---- backward, both dispatch branches; dropout keyed on the attention batch's packed -> padded map
    rid = c2_row_ids()
    assert rid.numel() >= R_in and int((rid[:R_in] < 0).sum()) == 0
    drop_rows = rid[:R_in].contiguous()
    da, dd = hip.drop_args(111, 0.1), hip.drop_args(222, 0.1)
    dy = randn((M, H), 3)
    add = randn((R_in, H), 4)
    eidx = drop_rows[rmap].long()[:, None] * H + torch.arange(H, device=dev())[None]
    m_add, m_dx = K.drop_mult_at(111, 0.1, eidx), K.drop_mult_at(222, 0.1, eidx)
    del eidx
    grad_rows_skipped = [i for i, n in enumerate(K.LN_STRESS) if n not in K.LN_GRAD_STRESS]
    assert grad_rows_skipped == [MEAN1E3]
    hit = torch.zeros(R_in, dtype=torch.bool, device=dev())
    hit[rmap] = True

    def launch(extra_on, dy_bf16):
        dx = Guard(R_in, H, torch.float32)
        dxb = Guard(R_in, H, torch.bfloat16)
        part = Guard(4 * nb, H, torch.float32)
        p4 = part.view.view(4, nb, H)
        kw = dict(dy_bf16=dy.bfloat16()) if dy_bf16 else dict(dy_f32=dy)
        hip.layernorm_bwd(x, M, H, gamma, mean.view[:, 0], rstd.view[:, 0], dx.view, row_map=rmap32, add_to=add,
                          dx_bf16=dxb.view, part=p4[:2], part_extra=p4[2:] if extra_on else None,
                          drop_add=da if extra_on else None, drop_dx=dd, drop_rows=drop_rows, **kw)
        outs = [Guard(1, H, torch.float32) for _ in range(4 if extra_on else 2)]
        hip.colsum_finish4(part.view, len(outs), nb, H, [o.view[0] for o in outs])
        torch.cuda.synchronize()
        return dx, dxb, part, outs

    for extra_on, dy_bf16 in ((True, False), (False, True)):
        sub = f"{case}/{'EXTRA' if extra_on else 'plain'}"
        dx, dxb, part, outs = launch(extra_on, dy_bf16)
        dx.check(f"[{sub}] dx_out", full=False)
        dxb.check(f"[{sub}] dx_bf16", full=False)
        for gd, n in ((dx, "dx_out"), (dxb, "dx_bf16")):   # exactly the gathered rows are written, all others untouched
            w = (gd.raw[:R_in * H].view(R_in, H) != gd.sentinel)
            assert bool(w[hit].all()) and not bool(w[~hit].any()), f"[{sub}] {n}: written rows differ from row_map"
        part.check(f"[{sub}] part", full=False)
        wp = (part.raw[:4 * nb * H] != part.sentinel).view(4, nb * H)
        assert bool(wp[:2].all()) and bool(wp[2:].all()) == extra_on and bool(wp[2:].any()) == extra_on
        for o in outs:
            o.check(f"[{sub}] column sums")
        dyr = (dy.bfloat16() if dy_bf16 else dy).to(F64)
        r_dx, r_dxb, planes = K.ln_bwd_full_ref(xs, g64, dyr, add[rmap].to(F64), m_add, m_dx)
        per_row(sub, "dx_out", dx.view[rmap], r_dx, 2e-5, "existing constant 2e-5, per row", skip_rows=grad_rows_skipped)
        per_row(sub, "dx_bf16", dxb.view[rmap], r_dxb, 1.0 / 128, "one bf16 rounding, per row", skip_rows=grad_rows_skipped)
        for o, t, n in zip(outs, planes, ("dgamma", "dbeta", "sum add_to * mask", "sum dx * mask")):
            holds(sub, n, (o.view[0].to(F64) - t.sum(0)).abs(), K.sum_bound(M, t.abs().sum(0)),
                  "1 x sqrt(M) * eps_f32 * sum |terms| of the float64 reference")
        del r_dx, r_dxb, planes, dyr
        dx2, dxb2, part2, outs2 = launch(extra_on, dy_bf16)            # no atomics: bitwise repeatable
        assert torch.equal(dx.raw, dx2.raw) and torch.equal(dxb.raw, dxb2.raw) and torch.equal(part.raw, part2.raw)
        assert all(torch.equal(a.raw, b.raw) for a, b in zip(outs, outs2))


# =============================================================================================== embeddings
@pytest.mark.parametrize("xheads", [0, 8])
@pytest.mark.parametrize("H", [1024, 1600])
def test_embedding_at_packed_rows(hip, H, xheads):
    """B = 2048, S = 128, V = 50257; half the ids uniform, half from 32 hot ids (0 and 50256 among them).
    engine.py passes arch.xattn_heads = 8 and nothing larger, so xheads > 8 is not forced at H = 1024.
    The sums of the LayerNorm-backward terms de (dwte, dattended, dU) are given, on top of the f32 summation bound, the
    existing 2e-5 of each term's row scale: a term is itself an f32 LayerNorm backward."""
    from pgca_amd.engine import make_row_pack
    case = f"embed/{H}/xh{xheads}"
    B, S, V = 2048, 128, 50257
    nb = hip.embed_bwd_blocks(B, S)
    assert nb == 1024 and (B * S) // 16 > 4 * nb                      # the cap: every wave walks several chunks
    nv = (H + 255) // 256
    assert (nv > 4) == (H == 1600)                                    # embed_bwd_kernel<NV,false> only at H = 1600
    ys = 8 if B >= 64 else (2 if B >= 8 else 1)                       # wpe_grad_kernel's batch slices, recomputed from B
    bslice = (B + ys - 1) // ys
    assert (B + bslice - 1) // bslice == 8
    g = torch.Generator().manual_seed(H + xheads)
    hot = torch.cat([torch.tensor([0, V - 1]), torch.randint(1, V - 1, (30,), generator=g)])
    ids = torch.randint(0, V, (B, S), generator=g)
    pick = torch.rand(B, S, generator=g) < 0.5
    ids[pick] = hot[torch.randint(0, 32, (int(pick.sum()),), generator=g)]
    ids = ids.to(dev())
    mask = (torch.arange(S)[None] < c2_lens()[:, None]).int().to(dev())
    pk = make_row_pack(mask)
    wte, wpe = randn((V, H), 1, 0.05), randn((S, H), 2, 0.05)
    gamma, beta = randn((H,), 4) * 0.1 + 1, randn((H,), 5) * 0.1
    train = xheads > 0
    att = randn((H,), 3, 0.05) if train else randn((B, H), 3, 0.05)   # b_o alone (att_stride 0) / one row per sequence
    U = randn((B, xheads, H), 6, 0.02) if train else None
    dxa, dea = (hip.drop_args(77, 0.3), hip.drop_args(88, 0.1)) if train else (None, None)
    kw = dict(attended=att, att_stride=0 if train else H, gamma=gamma, U=U, xheads=xheads, drop_x=dxa, drop_e=dea)

    # ---- forward: packed (row_ids, filler rows -> exact zeros) and padded
    h0p, mp, rp = Guard(pk.Mp, H, torch.float32), Guard(pk.Mp, 1, torch.float32), Guard(pk.Mp, 1, torch.float32)
    hip.embed_fwd(ids, B, S, H, wte, wpe, h0p.view, beta=beta, mean=mp.full, rstd=rp.full, row_ids=pk.row_ids,
                  n_rows=pk.Mp, **kw)
    h0, mn, rs = Guard(B * S, H, torch.float32), Guard(B * S, 1, torch.float32), Guard(B * S, 1, torch.float32)
    hip.embed_fwd(ids, B, S, H, wte, wpe, h0.view, beta=beta, mean=mn.full, rstd=rs.full, **kw)
    torch.cuda.synchronize()
    for gd, n in ((h0p, "h0 packed"), (mp, "mean packed"), (rp, "rstd packed"), (h0, "h0"), (mn, "mean"), (rs, "rstd")):
        gd.check(f"[{case}] {n}")
    rows = pk.row_ids[:pk.n].long()
    assert torch.equal(h0p.view[:pk.n], h0.view[rows]) and torch.equal(mp.view[:pk.n], mn.view[rows])
    assert torch.equal(rp.view[:pk.n], rs.view[rows])
    if pk.Mp > pk.n:
        assert float(h0p.view[pk.n:].abs().max()) == 0.0 and float(mp.view[pk.n:].abs().max()) == 0.0
        assert bool((rp.view[pk.n:] == 1.0).all())
    gout = randn((B * S, H), 9)
    nchunk = 8
    acc, seqs, fwd_err = {}, {}, []
    wte64, wpe64, gam64, bet64 = wte.to(F64), wpe.to(F64), gamma.to(F64), beta.to(F64)
    for ci in range(nchunk):                                           # float64 in chunks of 256 sequences
        b0, b1 = ci * B // nchunk, (ci + 1) * B // nchunk
        nbq = b1 - b0
        w = me = U64 = None
        if train:
            w = K.drop_mult_at(77, 0.3, torch.arange(b0 * xheads * S, b1 * xheads * S, device=dev())).view(nbq, xheads, S)
            me = K.drop_mult_at(88, 0.1, torch.arange(b0 * S * H, b1 * S * H, device=dev())).view(nbq, S, H)
            U64 = U[b0:b1].to(F64)
        a64 = att.to(F64) if train else att[b0:b1].to(F64)
        ref, e = K.embed_fwd_ref(ids[b0:b1], wte64, wpe64, a64, U64, w, gam64, bet64, me)
        fwd_err.append(K.row_errors(h0.view[b0 * S:b1 * S], ref.view(nbq * S, H), FLOOR)[0])
        r = K.embed_bwd_ref(gout[b0 * S:b1 * S].to(F64).view(nbq, S, H), ids[b0:b1], mask[b0:b1], e, U64, w, gam64, me, V)
        for k, v in r.items():
            if v is None:
                continue
            if k in K.EMBED_PER_SEQUENCE:
                seqs.setdefault(k, []).append(v)
            elif k in acc:
                acc[k] += v
            else:
                acc[k] = v
        del ref, e, r, me, w
    e = torch.cat(fwd_err)
    holds(case, "h0", e, 1e-5, "existing constant 1e-5, per row")
    seqs = {k: torch.cat(v) for k, v in seqs.items()}

    # ---- backward, padded with row_mask and packed with cu; atomics: float64 only, no bitwise repeat
    g_pk = torch.zeros(pk.Mp, H, device=dev())
    g_pk[:pk.n] = gout[rows]
    n_tok = float(mask.sum())
    TERM = 2e-5
    for layout in ("padded", "packed"):
        sub = f"{case}/{layout}"
        dwte = Guard(V, H, torch.float32, fill=0.0)
        dwpe = Guard(S, H, torch.float32, fill=0.0)
        datt = Guard(B, H, torch.float32, fill=0.0)
        dU = Guard(B * xheads, H, torch.float32, fill=0.0) if train else None
        part = Guard(2 * nb, H, torch.float32)
        packed = layout == "packed"
        hip.embed_bwd(g_pk if packed else gout, ids, mask, B, S, H, dwte.view, dwpe.view, wte=wte, attended=att, gamma=gamma,
                      mean=(mp if packed else mn).view[:, 0], rstd=(rp if packed else rs).view[:, 0],
                      dattended=datt.view, part=part.view.view(2, nb, H), att_stride=0 if train else H, U=U,
                      dU=dU.view.view(B, xheads, H) if train else None, xheads=xheads, drop_x=dxa, drop_e=dea,
                      cu=pk.cu[:B + 1].contiguous() if packed else None)
        dg, db = Guard(1, H, torch.float32), Guard(1, H, torch.float32)
        hip.colsum_finish4(part.view, 2, nb, H, [dg.view[0], db.view[0]])
        torch.cuda.synchronize()
        for gd, n in ((dwte, "dwte"), (dwpe, "dwpe"), (datt, "dattended"), (part, "part"), (dg, "dgamma"), (db, "dbeta")):
            gd.check(f"[{sub}] {n}")
        never = acc["n_dwte"] == 0
        assert int(never.sum()) > 0 and float(dwte.view[never].abs().max()) == 0.0, "rows of ids that never occur stay zero"
        holds(sub, "dwte", (dwte.view.to(F64) - acc["dwte"]).abs(),
              K.sum_bound(acc["n_dwte"][:, None], acc["abs_dwte"]) + TERM * acc["rs_dwte"][:, None] + 1e-30,
              "sqrt(n_id) * eps_f32 * sum |terms| + 2e-5 * sum of the terms' row scales")
        holds(sub, "dwpe", (dwpe.view.to(F64) - acc["dwpe"]).abs(), K.sum_bound(B, acc["abs_dwpe"]), "sqrt(B) * eps_f32 * sum |terms|")
        holds(sub, "dgamma", (dg.view[0].to(F64) - acc["dgamma"]).abs(), K.sum_bound(n_tok, acc["abs_dgamma"]),
              "sqrt(tokens) * eps_f32 * sum |terms|")
        holds(sub, "dbeta", (db.view[0].to(F64) - acc["dbeta"]).abs(), K.sum_bound(n_tok, acc["abs_dbeta"]),
              "sqrt(tokens) * eps_f32 * sum |terms|")
        if train:   # att_stride 0: every sequence's sum lands on its own row of dattended; b_o's gradient is their sum
            dU.check(f"[{sub}] dU")
            holds(sub, "dU", (dU.view.view(B, xheads, H).to(F64) - seqs["dU"]).abs(),
                  K.sum_bound(S, seqs["abs_dU"]) + TERM * seqs["rs_dU"][..., None] + 1e-30,
                  "sqrt(S) * eps_f32 * sum |terms| + 2e-5 * sum of the terms' row scales")
        holds(sub, "dattended", (datt.view.to(F64) - seqs["datt"]).abs(),
              K.sum_bound(S, seqs["abs_datt"]) + TERM * seqs["rs_datt"][:, None] + 1e-30,
              "sqrt(S) * eps_f32 * sum |terms| + 2e-5 * sum of the terms' row scales")


# =============================================================================================== small reductions
def test_small_reductions_at_2048_sequences(hip):
    from pgca_amd.engine import make_row_pack
    case = "reductions"
    B, S, H = 2048, 128, 1024
    lens = c2_lens()
    mask = (torch.arange(S)[None] < lens[:, None]).int().to(dev())
    pk = make_row_pack(mask)
    rows = pk.row_ids[:pk.n].long()
    f = randn((B * S, H), 1)
    fp = torch.zeros(pk.Mp, H, device=dev())
    fp[:pk.n] = f[rows]
    cu = pk.cu[:B + 1].contiguous()
    m64 = mask.to(F64)
    cnt = m64.sum(1, keepdim=True).clamp(min=1)
    terms = f.view(B, S, H).to(F64) * m64[..., None]
    ref, ref_abs = terms.sum(1) / cnt, terms.abs().sum(1) / cnt
    del terms
    dp = randn((B, H), 2)
    ref_d = ((dp.to(F64) / cnt)[:, None, :] * m64[..., None]).view(B * S, H)
    res = {}
    for layout in ("padded", "packed"):
        for rep in range(2):
            pooled = Guard(B, H, torch.float32)
            df = Guard(B * S if layout == "padded" else pk.Mp, H, torch.float32)
            if layout == "padded":
                hip.masked_mean_fwd(f, mask, B, S, H, pooled.view)
                hip.masked_mean_bwd(dp, mask, B, S, H, df.view)
            else:
                hip.masked_mean_fwd(fp, mask, B, S, H, pooled.view, cu=cu)
                hip.masked_mean_bwd(dp, mask, B, S, H, df.view, cu=cu)
            torch.cuda.synchronize()
            pooled.check(f"[{case}] pooled {layout}")
            df.check(f"[{case}] dfeats {layout}", full=layout == "padded")
            res[layout, rep] = (pooled, df)
        assert all(torch.equal(a.raw, b.raw) for a, b in zip(res[layout, 0], res[layout, 1]))   # no atomics
        pooled, df = res[layout, 0]
        holds(f"{case}/{layout}", "masked mean", (pooled.view.to(F64) - ref).abs(), K.sum_bound(cnt, ref_abs) + 2.0 ** -23 * ref.abs(),
              "sqrt(len) * eps_f32 * sum |terms| / len + the division's rounding")
        got = df.view if layout == "padded" else df.view[:pk.n]
        want = ref_d if layout == "padded" else ref_d[rows]
        holds(f"{case}/{layout}", "masked mean bwd", (got.to(F64) - want).abs(), 2.0 ** -22 * want.abs() + 1e-30,
              "two f32 roundings (division, mask product)")
        if layout == "packed" and pk.Mp > pk.n:    # the filler rows belong to no sequence: never written
            assert bool((df.raw[pk.n * H:pk.Mp * H] == df.sentinel).all())
    assert torch.equal(res["padded", 0][0].view, res["packed", 0][0].view)

    # seq_reduce: compact rows sorted by sequence; a caption with ONE real token scores nothing (mode 1: 0/0 = NaN)
    counts = (lens - 1).clamp(min=0).int()
    assert int((counts == 0).sum()) >= 1
    seq_of_row = torch.repeat_interleave(torch.arange(B), counts.long()).int().to(dev())
    n = int(counts.sum())
    tok = randn((n,), 3)
    cd = counts.to(dev())
    c64 = cd.to(F64)
    sums = torch.zeros(B, dtype=F64, device=dev()).index_add_(0, seq_of_row.long(), tok.to(F64))
    asum = torch.zeros(B, dtype=F64, device=dev()).index_add_(0, seq_of_row.long(), tok.to(F64).abs())
    live = cd > 0
    for mode in (0, 1):
        outs = []
        for rep in range(2):
            o = Guard(B, 1, torch.float32, slack=16)
            hip.seq_reduce(tok, seq_of_row, n, B, cd, mode, o.full)
            torch.cuda.synchronize()
            o.check(f"[{case}] seq_reduce mode {mode}")
            outs.append(o)
        assert torch.equal(outs[0].raw, outs[1].raw)
        got = outs[0].view[:, 0].to(F64)
        div = c64.clamp(min=1) if mode else torch.ones_like(c64)
        want = sums / div
        bound = K.sum_bound(c64, asum) / div + 2.0 ** -23 * want.abs()
        holds(f"{case}/seq_reduce{mode}", "sequence sums", (got - want).abs()[live], bound[live] + 1e-30,
              "sqrt(n) * eps_f32 * sum |terms| (+ the division's rounding)")
        if mode:
            assert bool(torch.isnan(got[~live]).all())
        else:
            assert float(got[~live].abs().max()) == 0.0

    # colsum over 73152 x 4096, bf16 and f32: the 256-block cap
    M, N = 73152, 4096
    nb = hip.colsum_blocks(M)
    assert nb == 256 and (M + 63) // 64 > nb
    xf = randn((M, N), 4)
    for name in ("bf16", "f32"):
        src = xf.bfloat16() if name == "bf16" else xf
        outs = []
        for rep in range(2):
            part, o = Guard(nb, N, torch.float32), Guard(1, N, torch.float32)
            hip.colsum(M, N, N, part.view, **({"x_bf16": src} if name == "bf16" else {"x_f32": src}))
            hip.colsum_finish(part.view, nb, N, o.view[0])
            torch.cuda.synchronize()
            part.check(f"[{case}] colsum part {name}")
            o.check(f"[{case}] colsum {name}")
            outs.append((part, o))
        assert torch.equal(outs[0][0].raw, outs[1][0].raw) and torch.equal(outs[0][1].raw, outs[1][1].raw)
        ref_s = torch.zeros(N, dtype=F64, device=dev())
        ref_a = torch.zeros(N, dtype=F64, device=dev())
        for r0 in range(0, M, 8192):
            c = src[r0:r0 + 8192].to(F64)
            ref_s += c.sum(0)
            ref_a += c.abs().sum(0)
        holds(f"{case}/colsum {name}", "column sums", (outs[0][1].view[0].to(F64) - ref_s).abs(), K.sum_bound(M, ref_a),
              "sqrt(M) * eps_f32 * sum |terms|")
