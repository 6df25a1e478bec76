#!/usr/bin/env python3
"""Measure one training step of the plain PointNet on the GPU (learn_region_grow_amd.pointnet_train) -> profiles/pointnet_train_bench.json.

Batch: --batch-size cells (100, train_pointnet.py:25) of 1024 random rows, 13 classes; both networks: the one train_pointnet.py builds
today ([64,64,64,128,1024] / [512,256]) and the shipped checkpoint's ([64,64,128,512] / [512]), from PointNetTrainer.init_weights.

Reported per network:
  step           device time of PointNetTrainer.train_step from the upload of the batch to the Adam update, by HIP events; --repeats
                 steps after --warmup; median, minimum and maximum.  Trainer and torch steps alternate, --rounds times each, so that
                 the run-to-run spread is recorded beside the ratio.
  stages         the same events recorded between the stages (PointNetTrainer.backward's mark): conv (upload, convolutions, pool,
                 head input), fc (fc layers, batch norms, logits), loss, fc_backward, conv_backward (pool gradient included), update
                 (moving averages, Adam).
  FLOPs          counted from the shapes, 2 per multiply-add on the products only: forward 2 R sum k n, dW the same, dX the same
                 without the first convolution's; over the step's time, as a share of the 157.3 TFLOP/s fp32 matrix peak.  It is a
                 whole-step rate over peak, not a kernel's share: the step also holds the bandwidth-bound passes and the host's
                 launches.
  memory         bytes of device memory the trainer holds (torch.cuda.memory_allocated around its construction).
  torch          the yardstick, not the code under test: the same step composed from torch ops with autograd on the same device
                 (matmul + bias + relu, amax, cat, the batch norm over the batch axis written out, cross_entropy, backward(),
                 torch.optim.Adam, the moving averages).

    python tools/pointnet_train_bench.py [--out profiles/pointnet_train_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_TFLOPS = 157.3
STAGES = ('conv', 'fc', 'loss', 'fc_backward', 'conv_backward', 'update')


def step_flops(conv, fc, num_class, rows):
    """(forward, dW, dX) FLOPs of one step on `rows` rows."""
    shapes, k = [], 6
    for n in conv:
        shapes.append((k, n))
        k = n
    k = conv[-1] + conv[1]
    for n in tuple(fc) + (num_class,):
        shapes.append((k, n))
        k = n
    fwd = sum(2 * rows * k * n for k, n in shapes)
    return fwd, fwd, fwd - 2 * rows * shapes[0][0] * shapes[0][1]


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), n=len(xs))


class TorchStep:
    """The trainer's step from torch ops with autograd."""

    def __init__(self, trainer, torch):
        from learn_region_grow_amd.checkpoint import pointnet_bn_names
        self.torch, self.dev = torch, trainer.dev
        w = trainer.weights_numpy()
        p = lambda a: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev))
        self.conv = [(p(w['kernel%d' % i].reshape(-1, c)), p(w['bias%d' % i])) for i, c in enumerate(trainer.conv)]
        self.fc = [(p(w['fc_weights%d' % j][0]), p(w['fc_bias%d' % j])) for j in range(len(trainer.fc) + 1)]
        self.bn = [(p(w[pointnet_bn_names(j)[0]]), p(w[pointnet_bn_names(j)[1]])) for j in range(len(trainer.fc))]
        self.ema = [[torch.zeros((1024, c), device=self.dev), torch.zeros((1024, c), device=self.dev)] for c in trainer.fc]
        params = [t for pair in self.conv + self.fc + self.bn for t in pair]
        self.opt = torch.optim.Adam(params, lr=trainer.base_lr, betas=(trainer.b1, trainer.b2), eps=trainer.eps)

    def step(self, points, labels):
        torch = self.torch
        x = torch.from_numpy(points).to(self.dev)
        y = torch.from_numpy(labels).to(self.dev).view(-1).long()
        acts = []
        for w, b in self.conv:
            x = torch.relu(torch.matmul(x, w) + b)
            acts.append(x)
        x = torch.cat([acts[-1] - acts[-1].amax(dim=1, keepdim=True), acts[1]], dim=2)
        moments = []
        for (w, b), (beta, gamma) in zip(self.fc[:-1], self.bn):
            z = torch.matmul(x, w) + b
            mean = z.mean(dim=0)
            var = ((z - mean) ** 2).mean(dim=0)
            inv = torch.rsqrt(var + 1e-3) * gamma
            x = torch.relu(z * inv + (beta - mean * inv))
            moments.append((mean.detach(), var.detach()))
        logits = torch.matmul(x, self.fc[-1][0]) + self.fc[-1][1]
        loss = torch.nn.functional.cross_entropy(logits.view(-1, logits.shape[-1]), y)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        with torch.no_grad():
            for shadow, value in zip(self.ema, moments):
                for s, v in zip(shadow, value):
                    s.sub_((s - v) * 0.1)
        self.opt.step()
        return float(loss)


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


def measure(name, conv, fc, args, torch):
    from learn_region_grow_amd.pointnet_train import PointNetTrainer
    B = args.batch_size
    rs = np.random.RandomState(0)
    points = rs.uniform(-0.5, 0.5, (B, 1024, 6)).astype(np.float32)
    points[:, :, 2] = rs.uniform(0, 3, (B, 1024))
    labels = rs.randint(0, args.num_class, (B, 1024)).astype(np.int32)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    tr = PointNetTrainer(B, conv, fc, args.num_class).init_weights(0)
    held = torch.cuda.memory_allocated() - before
    composed = TorchStep(tr, torch)
    first = (tr.backward(points, labels, loss_only=True)['loss'], composed.step(points, labels))
    ours, theirs = [], []
    for _ in range(args.rounds):
        ours.append(timed(torch, lambda mark: tr.train_step(points, labels, mark=mark), args.warmup, args.repeats, True))
        theirs.append(timed(torch, lambda mark: composed.step(points, labels), args.warmup, args.repeats, False))
    best = lambda rounds: min(rounds, key=lambda r: r[1]['median'])
    stages, whole = best(ours)
    _, t_whole = best(theirs)
    fwd, dw, dx = step_flops(conv, fc, args.num_class, B * 1024)
    out = dict(network=name, conv_widths=list(conv), fc_widths=list(fc), num_class=args.num_class, batch_size=B, rows=B * 1024,
               parameters=int(tr.flat.numel()), device_bytes_held=int(held), step_s=whole, stages_s=stages,
               step_median_s_by_round=[r[1]['median'] for r in ours],
               flop=dict(forward=fwd, dW=dw, dX=dx, step=fwd + dw + dx), step_tflops=(fwd + dw + dx) / whole['median'] * 1e-12,
               step_share_of_fp32_matrix_peak=(fwd + dw + dx) / whole['median'] / (PEAK_TFLOPS * 1e12),
               first_loss=dict(trainer=first[0], torch=first[1]),
               torch_autograd=dict(step_s=t_whole, step_median_s_by_round=[r[1]['median'] for r in theirs],
                                   trainer_over_torch_step_time=whole['median'] / t_whole['median']))
    print(json.dumps(out))
    del tr, composed
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pointnet_train_bench.json'))
    ap.add_argument('--batch-size', type=int, default=100)
    ap.add_argument('--num-class', type=int, default=13)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=2)
    args = ap.parse_args()
    import torch
    from learn_region_grow_amd.pointnet_train import ARCHITECTURES
    if not torch.cuda.is_available():
        raise SystemExit('tools/pointnet_train_bench.py measures on the GPU; none is visible')
    out = dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TFLOPS, warmup=args.warmup, repeats=args.repeats, rounds=args.rounds,
               networks=[])
    for name in ('today', 'shipped'):
        out['networks'].append(measure(name, *ARCHITECTURES[name], args, torch))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
