#!/usr/bin/env python3
"""Measure one training step of MCPNet on the GPU (learn_region_grow_amd.mcpnet_train) -> profiles/mcpnet_train_bench.json.

Batch: 256 points (train_mcpnet.py:17) of 50 synthetic staged rows, 16 points an instance, the weights of initial_weights(0).

  step     device time of MCPNetTrainer.train_step from the upload of the batch to the Adam update, by device events; --repeats steps
           after --warmup, median, minimum and maximum.  Trainer and torch steps alternate, --rounds times each.  The step reads its
           four scalars back before the update (a batch without positives is skipped), so it holds one host round trip.
  stages   the same events recorded between the stages (MCPNetTrainer.forward_backward's mark): forward (upload, repack, the forward
           pass that keeps its layers), loss (lrg_mcp_triplet_semihard), head_backward (layers 4 and 3), branch_backward (the pool's
           gradient, layers 2 and 1), update (the scalars' read-back and Adam).
  torch    the yardstick, not the code under test: the same step composed from torch ops with autograd on the same device (matmul,
           relu, amax, the loss graph of metric_loss_ops.py:157-236 with its [B * B, B] tiles on amin / amax, backward(),
           torch.optim.Adam), the loss and the embeddings read back as the script reads them.

    python tools/mcpnet_train_bench.py [--out profiles/mcpnet_train_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STAGES = ('forward', 'loss', 'head_backward', 'branch_backward', 'update')


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), n=len(xs))


class TorchStep:
    """The trainer's step from torch ops with autograd."""

    def __init__(self, trainer, torch):
        self.torch, self.dev = torch, trainer.dev
        w = trainer.weights_numpy()
        self.p = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(v.reshape(-1, v.shape[-1]) if v.ndim > 1 else v)).to(self.dev))
                  for k, v in w.items()}
        self.opt = torch.optim.Adam(list(self.p.values()), lr=trainer.lr, betas=(trainer.b1, trainer.b2), eps=trainer.eps)

    def loss(self, emb, labels, margin=1.0):
        torch = self.torch
        B = emb.shape[0]
        eye = torch.eye(B, dtype=emb.dtype, device=self.dev)
        sq = (emb * emb).sum(1, keepdim=True)
        D = torch.clamp(sq + sq.t() - 2.0 * emb @ emb.t(), min=0.0)
        D = D * (D > 0).to(emb.dtype) * (1 - eye)
        lab = labels.view(B, 1)
        adj = lab == lab.t()
        tile = D.repeat(B, 1)
        mask = (~adj).repeat(B, 1) & (tile > D.t().reshape(-1, 1))
        mask_final = (mask.sum(1) > 0).view(B, B).t()
        hi = tile.amax(1, keepdim=True)
        outside = (((tile - hi) * mask.to(emb.dtype)).amin(1, keepdim=True) + hi).view(B, B).t()
        lo = D.amin(1, keepdim=True)
        inside = (((D - lo) * (~adj).to(emb.dtype)).amax(1, keepdim=True) + lo).repeat(1, B)
        pos = adj.to(emb.dtype) - eye
        return torch.clamp((margin + (D - torch.where(mask_final, outside, inside))) * pos, min=0.0).sum() / pos.sum()

    def step(self, points4, rows, labels):
        torch, p = self.torch, self.p
        x = torch.from_numpy(rows).to(self.dev)
        c = torch.from_numpy(points4).to(self.dev)
        y = torch.from_numpy(labels).to(self.dev)
        h = torch.relu(torch.matmul(x, p['mcp_kernel1']) + p['mcp_bias1'])
        h = torch.relu(torch.matmul(h, p['mcp_kernel2']) + p['mcp_bias2'])
        cat = torch.cat([c, h.amax(dim=1)], dim=1)
        fc3 = torch.relu(cat @ p['mcp_kernel3'] + p['mcp_bias3'])
        fc4 = fc3 @ p['mcp_kernel4'] + p['mcp_bias4']
        emb = fc4 * torch.rsqrt(torch.clamp((fc4 * fc4).sum(1, keepdim=True), min=1e-12))
        loss = self.loss(emb, y)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        return float(loss.detach()), emb.detach().cpu().numpy()


def timed(torch, fn, warmup, repeats, with_marks):
    """-> (per-stage stats or None, whole-step stats) in seconds from events."""
    for _ in range(warmup):
        fn(None)
    whole, stages = [], {s: [] for s in STAGES}
    for _ in range(repeats):
        ev = [('start', torch.cuda.Event(enable_timing=True))]
        ev[0][1].record()

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((name, e))
        fn(mark if with_marks else None)
        mark('end')
        torch.cuda.synchronize()
        whole.append(ev[0][1].elapsed_time(ev[-1][1]) * 1e-3)
        for (_, a), (name, b) in zip(ev[:-2], ev[1:-1]):
            stages[name].append(a.elapsed_time(b) * 1e-3)
    return ({s: stats(v) for s, v in stages.items() if v} if with_marks else None), stats(whole)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mcpnet_train_bench.json'))
    ap.add_argument('--batch-size', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=1000)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    import torch
    from learn_region_grow_amd.mcpnet_train import MCPNetTrainer
    if not torch.cuda.is_available():
        raise SystemExit('tools/mcpnet_train_bench.py measures on the GPU; none is visible')
    B = args.batch_size
    rs = np.random.RandomState(0)
    inst = np.arange(B) // 16
    rows = np.concatenate([rs.uniform(-0.45, 0.45, (B, 50, 3)), rs.uniform(-0.6, 0.6, (B, 50, 3))], axis=2).astype(np.float32)
    points4 = np.concatenate([rs.uniform(0, 2.5, (B, 1)), np.clip(0.5 + 0.3 * rs.randn(B // 16 + 1, 3)[inst] + 0.05 * rs.randn(B, 3), 0, 1)],
                             axis=1).astype(np.float32)
    labels = inst.astype(np.int32)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    tr = MCPNetTrainer(B).init_weights(0)
    held = torch.cuda.memory_allocated() - before
    composed = TorchStep(tr, torch)
    first = (tr.evaluate(points4, rows, labels)['loss'], composed.step(points4, rows, labels)[0])
    ours, theirs = [], []
    for _ in range(args.rounds):
        ours.append(timed(torch, lambda mark: tr.train_step(points4, rows, labels, mark=mark), args.warmup, args.repeats, True))
        theirs.append(timed(torch, lambda mark: composed.step(points4, rows, labels), args.warmup, args.repeats, False))
    best = lambda rounds: min(rounds, key=lambda r: r[1]['median'])
    stages, whole = best(ours)
    _, t_whole = best(theirs)
    largest = max(stages, key=lambda s: stages[s]['median'])
    out = dict(device=torch.cuda.get_device_name(0), batch_size=B, rows=B * 50, parameters=int(tr.flat.numel()), device_bytes_held=int(held),
               warmup=args.warmup, repeats=args.repeats, rounds=args.rounds, step_s=whole, stages_s=stages, largest_stage=largest,
               step_median_s_by_round=[r[1]['median'] for r in ours], first_loss=dict(trainer=first[0], torch=first[1]),
               torch_autograd=dict(step_s=t_whole, step_median_s_by_round=[r[1]['median'] for r in theirs],
                                   trainer_over_torch_step_time=whole['median'] / t_whole['median']))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
