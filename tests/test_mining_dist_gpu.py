"""``mine_then_dpo`` under data parallelism: every rank mines its own shard, so the ranks hold different numbers of
pairs; all of them cut to the smallest batch count and leave the loop together (two gloo ranks on one GPU, in the pattern
of ``test_dist_gpu.py``)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pgca_amd import REPO_ROOT
        from pgca_amd.arch import tiny_arch
        from pgca_amd.config import Config
        from pgca_amd.model import PreferenceGuidedCaptioningModel
        from pgca_amd.trainer import PreferenceGuidedTrainer
        cfg = Config(os.path.join(REPO_ROOT, "configs", "default.yaml"))
        for k, v in {"paths.output_dir": os.path.join(out_dir, f"out{rank}"), "training.stage2.num_epochs": 1,
                     "training.stage2.batch_size": 4, "training.stage2.logging_steps": 1,
                     "training.stage2.gradient_accumulation_steps": 1, "training.stage1.gradient_accumulation_steps": 1,
                     "model.dropout": 0.0, "mi355x.gpt2_pdrop": 0.0, "mi355x.stage2.objective": "mine_then_dpo",
                     "mi355x.mining": {"num_candidates": 4, "max_length": 12}}.items():
            cfg.set(k, v)
        arch = tiny_arch()
        model = PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=arch, dropout=0.0, seed=5, device="cuda:0")
        g = torch.Generator().manual_seed(100 + rank)
        images = lambda batches: [{"image": torch.randn(4, 3, arch.vit.image, arch.vit.image, generator=g)}  # noqa: E731
                                  for _ in range(batches)]
        tr = PreferenceGuidedTrainer(model, cfg, None, None, images(3 - rank), images(1))   # rank 0: 12 images, rank 1: 8
        out = tr.train_stage2()
        mined = [h for h in tr.history if h.get("mined") == "train"][0]["mined_pairs"]
        steps = tr.global_step                                   # micro-batches run (step losses are logged by rank 0 only)
        torch.save((mined, steps, out["train_loss"], out["val_loss"]), os.path.join(out_dir, f"mine{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_uneven_yields_run_the_same_number_of_batches(tmp_path):
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0, "a rank hung or failed"
    (m0, s0, t0, v0), (m1, s1, t1, v1) = (torch.load(tmp_path / f"mine{r}.pt", weights_only=False) for r in range(world))
    assert m0 // 4 != m1 // 4                                      # the shards really gave different batch counts
    assert s0 == s1 == min(m0, m1) // 4                            # ... and both ranks ran the smaller one
    assert len(t0) == len(t1) == 1 and v0 == v1                    # one epoch each, the same rank-reduced validation loss
