#!/usr/bin/env python3
"""Memory and time of the activation-recompute modes (``GptTrunk.recompute``) on the benchmark's Stage-2 step.

Geometry of ``bench.py``'s headline line: ViT-B/32 + GPT-2-M, S = 128, 4-forward DPO, dropout 0.1, packed rows, the
same synthetic length distribution (``bench.synthetic_batch``), AdamW + clip.  Every (mode, pairs) case runs in a
process of its own, one after the other, so ``torch.cuda.max_memory_allocated()`` and the workspace are that case's alone
and a case that does not fit ends only itself (an allocation failure is reported, not retried).

    python tools/recompute_probe.py --out profiles/recompute_memory_time.json

Per case: ``Workspace.nbytes()``, ``max_memory_allocated``, ms per step as the MEDIAN of ``--steps`` (>= 20) steps timed
one by one with device events after ``--warmup`` steps, and pairs/s from that median.  ``none`` at the base pair count
is the baseline every ratio refers to; it is measured in the same invocation.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run_case(mode: str, pairs: int, steps: int, warmup: int, seq_len: int, vision: str, text: str) -> dict:
    import torch

    from bench import synthetic_batch
    from pgca_amd.arch import make_arch
    from pgca_amd.engine import DropoutPlan
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    from pgca_amd.steps import DPOStep, FusedOptimizer, ReferencePolicy

    if not torch.cuda.is_available():
        raise SystemExit("recompute_probe: no GPU - nothing here can be measured on the host")
    dev = torch.device("cuda", 0)
    res = {"mode": mode, "pairs": pairs, "seq_len": seq_len, "steps": steps, "warmup": warmup}
    try:
        arch = make_arch(vision, text, 512)
        model = PreferenceGuidedCaptioningModel(vision, text, 512, temperature=0.5, freeze_vision_backbone=True,
                                                device=dev, seed=42)
        ref = ReferencePolicy(model.store, model.ws)
        step = DPOStep(model.store, model.ws, model.vision_encoder.tower, model.vision_encoder.head,
                       model.caption_decoder.engine, beta=0.1, reference_free=False, ref=ref,
                       dropout=DropoutPlan(0.1, base_seed=42), packed=True, recompute=mode)
        segs = [model.store.segments["vision_head"], model.store.segments["decoder"]]
        opt = FusedOptimizer(segs, lr=1e-5, weight_decay=0.01, max_grad_norm=1.0, warmup_steps=500, total_steps=100000)
        nbatch = 4
        batches = [DPOStep.prepare(synthetic_batch(pairs, seq_len, arch.gpt.base_vocab, arch.gpt.base_vocab,
                                                   seed=1234 + 1000 * i), dev) for i in range(nbatch)]
        res["packed_rows_per_step"] = sum(b["seq"].pack.Mp for b in batches) / nbatch
        torch.cuda.synchronize()
        res["resident_before_steps_bytes"] = torch.cuda.memory_allocated()

        def one(i):
            p = batches[i % nbatch]
            opt.zero_grad()
            loss = step.loss_and_grads(p["image"], p["seq"])
            opt.step()
            return loss

        for i in range(warmup):
            loss = one(i)
            torch.cuda.synchronize()
        times = []
        for i in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = one(warmup + i)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = statistics.median(times)
        res.update(completed=True, loss=float(loss), workspace_bytes=model.ws.nbytes(),
                   max_memory_allocated_bytes=torch.cuda.max_memory_allocated(), ms_per_step_median=ms,
                   ms_per_step_min=min(times), ms_per_step_max=max(times), pairs_per_s=pairs / (ms * 1e-3))
    except torch.cuda.OutOfMemoryError as exc:
        res.update(completed=False, ran_out="HBM: " + str(exc).splitlines()[0],
                   allocated_at_failure_bytes=torch.cuda.memory_allocated())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512, help="pair count at which the three modes are compared")
    ap.add_argument("--larger", type=int, nargs="*", default=[768, 1024], help="pair counts also tried in mlp and block")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--vision-model", default="openai/clip-vit-base-patch32")
    ap.add_argument("--text-model", default="gpt2-medium")
    ap.add_argument("--case-timeout", type=float, default=240.0, help="seconds one case may take")
    ap.add_argument("--out", default=None, help="write the JSON here as well as to stdout")
    ap.add_argument("--case", nargs=2, metavar=("MODE", "PAIRS"), help="(internal) run one case and print its JSON line")
    args = ap.parse_args()
    if args.steps < 20 and args.case is None:
        ap.error("--steps must be >= 20: the reported figure is a median")

    if args.case is not None:
        print("CASE " + json.dumps(run_case(args.case[0], int(args.case[1]), args.steps, args.warmup, args.seq_len,
                                            args.vision_model, args.text_model)), flush=True)
        return 0

    cases = [(m, args.pairs) for m in ("none", "mlp", "block")]
    cases += [(m, n) for m in ("block", "mlp") for n in args.larger]
    out = {"tool": "tools/recompute_probe.py", "workload": f"Stage-2 4-forward DPO step, {args.vision_model} (frozen) + "
           f"{args.text_model}, seq_len {args.seq_len}, dropout 0.1, packed rows, AdamW + clip",
           "timing": f"median of {args.steps} single steps between device events after {args.warmup} warm-up steps; one "
                     "process per case", "cases": []}
    for mode, n in cases:   # this parent never opens the GPU: each case is a fresh child, one at a time
        cmd = [sys.executable, os.path.abspath(__file__), "--case", mode, str(n), "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--seq-len", str(args.seq_len), "--vision-model", args.vision_model, "--text-model",
               args.text_model]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.case_timeout)
        except subprocess.TimeoutExpired:
            out["cases"].append({"mode": mode, "pairs": n, "completed": False, "ran_out": "time limit of the case"})
            print(f"[probe] {mode} @ {n}: time limit; stopping", file=sys.stderr, flush=True)
            break
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("CASE ")), None)
        if r.returncode != 0 or line is None:   # anything but a clean result or a reported allocation failure: stop here
            out["cases"].append({"mode": mode, "pairs": n, "completed": False, "exit_code": r.returncode,
                                 "stderr_tail": r.stderr[-600:]})
            print(f"[probe] {mode} @ {n}: exit {r.returncode}; stopping", file=sys.stderr, flush=True)
            break
        case = json.loads(line[5:])
        out["cases"].append(case)
        print(f"[probe] {mode} @ {n}: " + (f"{case['ms_per_step_median']:.1f} ms/step, workspace "
                                           f"{case['workspace_bytes'] / 2 ** 30:.1f} GiB, peak "
                                           f"{case['max_memory_allocated_bytes'] / 2 ** 30:.1f} GiB"
                                           if case["completed"] else case["ran_out"]), file=sys.stderr, flush=True)
    base = next((c for c in out["cases"] if c["mode"] == "none" and c.get("completed")), None)
    if base is not None:
        for c in out["cases"]:
            if c.get("completed"):
                c["ms_per_pair_vs_none"] = (c["ms_per_step_median"] / c["pairs"]) / (base["ms_per_step_median"] / base["pairs"])
                if c["pairs"] == base["pairs"]:
                    c["workspace_vs_none"] = c["workspace_bytes"] / base["workspace_bytes"]
        out["largest_pairs_completed"] = {m: max([c["pairs"] for c in out["cases"] if c["mode"] == m and c.get("completed")],
                                                 default=None) for m in ("mlp", "block")}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")
    return 0 if len(out["cases"]) == len(cases) else 1


if __name__ == "__main__":
    raise SystemExit(main())
