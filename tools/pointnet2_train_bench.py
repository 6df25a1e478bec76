#!/usr/bin/env python3
"""Measure one training step of PointNet++ on the GPU (learn_region_grow_amd.pointnet2_train) -> profiles/pointnet2_train_bench.json.

Batch: --batch-size cells (100, train_pointnet.py:25) of 1024 random rows, 13 classes; both variants: colour features (what
train_pointnet.py builds today) and xyz only (the shipped index), from PointNet2Trainer.init_weights.

Reported per variant:
  step           device time of PointNet2Trainer.train_step from the upload of the batch to the Adam update, by HIP events; --repeats
                 steps after --warmup; median, minimum and maximum.  Trainer and torch steps alternate, --rounds times each, so that
                 the run-to-run spread is recorded beside the ratio.
  stages         the same events recorded between the stages (PointNet2Trainer.backward's mark), a step's intervals of one name added
                 up: upload (the batch, the weights' operand images), fps, ball_query (with the gather of the sampled points),
                 sa_forward, fp_forward (three_nn and the interpolation included, and the head), loss, head_backward, fp_backward,
                 scatter (the gradients of group_point and three_interpolate), sa_backward (the pool's gradient included), update.
  FLOPs          counted from the shapes, 2 per multiply-add on the products only: forward 2 R sum k n per MLP, dW the same, dX the
                 same without layer1's first layer and fa_layer4's colour block (their inputs are data); over the step's time, as a
                 share of the 157.3 TFLOP/s fp32 matrix peak.  It is a whole-step rate over peak, not a kernel's share.
  memory         bytes of device memory the trainer holds (torch.cuda.memory_allocated around its construction), and the share of it
                 that is kept activations of the set-abstraction levels.
  torch          the yardstick, not the code under test: the same step composed from torch ops with autograd on the same device ON
                 THE TRAINER'S INDICES (index_select gathers, matmul + bias + relu, amax, the weighted sum of three gathers, cat,
                 cross_entropy, backward(), torch.optim.Adam).  It does not sample, query or search: the ratio is given against the
                 whole trainer step and against the step without its fps and ball_query stages (three_nn stays inside fp_forward).

    python tools/pointnet2_train_bench.py [--out profiles/pointnet2_train_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_TFLOPS = 157.3
STAGES = ('upload', 'fps', 'ball_query', 'sa_forward', 'fp_forward', 'loss', 'head_backward', 'fp_backward', 'scatter', 'sa_backward', 'update')
INDEX_STAGES = ('fps', 'ball_query')


def step_flops(trainer):
    """(forward, dW, dX) FLOPs of one step."""
    fwd = skipped = 0
    for n, ((scope, ids, cin, mlp), rows) in enumerate(zip(trainer._mlps(), trainer._mlp_rows())):
        k = cin
        for c in mlp:
            fwd += 2 * rows * k * c
            k = c
        if n == 0:
            skipped += 2 * rows * cin * mlp[0]
        if n == 7:
            skipped += 2 * rows * trainer.feat[0] * mlp[0]
    return fwd, fwd, fwd - skipped


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), n=len(xs))


class TorchStep:
    """The trainer's step from torch ops with autograd, on the trainer's indices and interpolation weights."""

    def __init__(self, trainer, torch):
        self.torch, self.dev, self.rgb = torch, trainer.dev, trainer.rgb_features
        w = trainer.weights_numpy()
        p = lambda a: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev))
        self.mlps = [[(p(w['%skernel%d' % (scope, i)].reshape(w['%skernel%d' % (scope, i)].shape[-2:])), p(w['%sbias%d' % (scope, i)])) for i in ids]
                     for scope, ids, _, _ in trainer._mlps()]
        self.opt = torch.optim.Adam([t for m in self.mlps for pair in m for t in pair], lr=trainer.lr, betas=(trainer.b1, trainer.b2), eps=trainer.eps)
        ind = trainer.level_indices()
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.fps = [t(lv['fps']).long() for lv in ind['sa']]
        self.ball = [t(lv['idx']).long() for lv in ind['sa']]
        self.nn = [t(lv['nn_idx']).long() for lv in ind['fp']]
        self.nnw = [t(lv['weight']) for lv in ind['fp']]

    @staticmethod
    def _mlp(torch, x, layers, relu_last=True):
        for n, (w, b) in enumerate(layers):
            x = torch.matmul(x, w) + b
            if relu_last or n + 1 < len(layers):
                x = torch.relu(x)
        return x

    def step(self, points, labels):
        torch = self.torch
        x = torch.from_numpy(points).to(self.dev)
        y = torch.from_numpy(labels).to(self.dev).view(-1).long()
        B = x.shape[0]
        bi = torch.arange(B, device=self.dev)
        xyz, feat = [x[:, :, :3]], [x[:, :, 3:] if self.rgb else None]
        for lv in range(4):
            new_xyz = xyz[lv][bi[:, None], self.fps[lv]]
            idx = self.ball[lv]
            g = xyz[lv][bi[:, None, None], idx] - new_xyz[:, :, None, :]
            if feat[lv] is not None:
                g = torch.cat([g, feat[lv][bi[:, None, None], idx]], dim=-1)
            feat.append(self._mlp(torch, g, self.mlps[lv]).amax(dim=2))
            xyz.append(new_xyz)
        up = feat[4]
        for lv in range(4):
            dst = 3 - lv
            nn, w = self.nn[lv], self.nnw[lv]
            interp = (up[bi[:, None], nn[:, :, 0]] * w[:, :, 0:1] + up[bi[:, None], nn[:, :, 1]] * w[:, :, 1:2]) + up[bi[:, None], nn[:, :, 2]] * w[:, :, 2:3]
            h = interp if feat[dst] is None else torch.cat([interp, feat[dst]], dim=2)
            up = self._mlp(torch, h, self.mlps[4 + lv])
        logits = self._mlp(torch, up, self.mlps[8], relu_last=False)
        loss = torch.nn.functional.cross_entropy(logits.view(-1, logits.shape[-1]), y)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        return float(loss)


def timed(torch, fn, warmup, repeats, with_marks):
    """-> (per-stage stats or None, whole-step stats) in seconds from events; a step's intervals of one stage name are added up."""
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
        per = {}
        for (_, a), (name, b) in zip(ev[:-2], ev[1:-1]):
            per[name] = per.get(name, 0.0) + a.elapsed_time(b) * 1e-3
        for name, v in per.items():
            stages[name].append(v)
    return ({s: stats(v) for s, v in stages.items() if v} if with_marks else None), stats(whole)


def measure(name, rgb, args, torch):
    from learn_region_grow_amd.pointnet2_train import PointNet2Trainer
    B = args.batch_size
    rs = np.random.RandomState(0)
    points = rs.uniform(-0.5, 0.5, (B, 1024, 6)).astype(np.float32)
    points[:, :, 2] = rs.uniform(0, 3, (B, 1024))
    points[:, :, 3:] = rs.uniform(0, 1, (B, 1024, 3))
    labels = rs.randint(0, args.num_class, (B, 1024)).astype(np.int32)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    tr = PointNet2Trainer(B, args.num_class, rgb).init_weights(0)
    held = torch.cuda.memory_allocated() - before
    kept_sa = sum(t.numel() * 4 for lv in range(4) for t in [tr._sa_rows[lv]] + tr._sa_keep[lv])
    first_ours = tr.backward(points, labels, loss_only=True)['loss']
    composed = TorchStep(tr, torch)
    first = (first_ours, composed.step(points, labels))
    ours, theirs = [], []
    for _ in range(args.rounds):
        ours.append(timed(torch, lambda mark: tr.train_step(points, labels, mark=mark), args.warmup, args.repeats, True))
        theirs.append(timed(torch, lambda mark: composed.step(points, labels), args.warmup, args.repeats, False))
    torch_peak = torch.cuda.max_memory_allocated()
    best = lambda rounds: min(rounds, key=lambda r: r[1]['median'])
    stages, whole = best(ours)
    _, t_whole = best(theirs)
    fwd, dw, dx = step_flops(tr)
    index_s = sum(stages[s]['median'] for s in INDEX_STAGES)
    out = dict(variant=name, rgb_features=rgb, num_class=args.num_class, batch_size=B, rows=B * 1024, parameters=int(tr.flat.numel()),
               device_bytes_held=int(held), kept_set_abstraction_activation_bytes=int(kept_sa), peak_bytes_allocated_in_process=int(torch_peak),
               step_s=whole, stages_s=stages, step_median_s_by_round=[r[1]['median'] for r in ours],
               flop=dict(forward=fwd, dW=dw, dX=dx, step=fwd + dw + dx), step_tflops=(fwd + dw + dx) / whole['median'] * 1e-12,
               step_share_of_fp32_matrix_peak=(fwd + dw + dx) / whole['median'] / (PEAK_TFLOPS * 1e12),
               first_loss=dict(trainer=first[0], torch=first[1]),
               torch_autograd=dict(step_s=t_whole, step_median_s_by_round=[r[1]['median'] for r in theirs],
                                   trainer_over_torch_step_time=whole['median'] / t_whole['median'],
                                   trainer_without_fps_and_ball_query_over_torch=(whole['median'] - index_s) / t_whole['median']))
    print(json.dumps(out))
    del tr, composed
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pointnet2_train_bench.json'))
    ap.add_argument('--batch-size', type=int, default=100)
    ap.add_argument('--num-class', type=int, default=13)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--rounds', type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tools/pointnet2_train_bench.py measures on the GPU; none is visible')
    out = dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TFLOPS, warmup=args.warmup, repeats=args.repeats, rounds=args.rounds,
               variants=[])
    for name, rgb in (('rgb', True), ('xyz', False)):
        out['variants'].append(measure(name, rgb, args, torch))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
