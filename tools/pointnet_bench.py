#!/usr/bin/env python3
"""Measure the plain PointNet baseline on the GPU (learn_region_grow_amd.pointnet) -> profiles/pointnet_bench.json.

Set: the 68 Area-5-shaped rooms of tools/pointnet2_bench.py (synthetic.area5_shaped_room at AREA5_POINTS, equalised at 0.1 m, 1 m
cells; a cell of more than 1024 points is cut into pieces of at most 1024 in index order and counted, cells_split).  Both networks:
the shipped checkpoint's ([64,64,128,512] / [512]) and the one train_pointnet.py builds today ([64,64,64,128,1024] / [512,256]),
random weights (tests/pointnet_ref.random_weights), 13 classes.

Reported per network:
  end to end     rooms/s and cells/s from the raw rooms to the labels: device equalisation, the host's cell cut and padding, uploads,
                 the network in chunks of 64 cells, argmax, the scatter back, the segmentation.  Wall clock, --e2e-repeats runs
                 after one warm-up; median, minimum and maximum.
  network pass   device time of lrg_pointnet_features (its memset included) and lrg_pointnet_head by HIP events recorded between
                 the launches, summed over the chunks of one pass over all cells; --repeats passes after --warmup; cells/s.
  kernels        FLOPs counted from the shapes (2 x rows x sum k n over the layers, unpadded; the batch norm's two operations per
                 value not counted) over the stage time, as a share of the 157.3 TFLOP/s fp32 matrix peak; beside it the HBM bytes
                 the kernel must move (its inputs and outputs once) over 8 TB/s, and which of the two is the larger bound.
  torch          the yardstick, not the code under test: the same layers composed from torch ops on the same device and chunks
                 (matmul + bias + relu, amax over the rows, cat, the folded batch norm as a multiply and an add).  Fused and torch
                 passes alternate, --rounds times each, so the run-to-run spread is recorded beside the ratio.

    python tools/pointnet_bench.py [--out profiles/pointnet_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))

from pointnet2_bench import PEAK_TFLOPS, split_cell_inputs, stats, timed_pass  # noqa: E402

HBM_TBPS = 8.0
ROWS = 1024


def flops_and_bytes_per_cell(conv, fc, num_class):
    """((features FLOPs, head FLOPs), (features bytes, head bytes)) of one cell: 2 per multiply-add on the unpadded shapes; the
    bytes are the tensors each kernel reads and writes once (weights and batch-norm tables stay in cache across tiles)."""
    f, k = 0, 6
    for n in conv:
        f += 2 * ROWS * k * n
        k = n
    h, k = 0, conv[-1] + conv[1]
    for n in tuple(fc) + (num_class,):
        h += 2 * ROWS * k * n
        k = n
    fb = 4 * ROWS * (6 + conv[1] + conv[-1]) + 4 * conv[-1]
    hb = 4 * ROWS * (conv[1] + conv[-1] + num_class) + 4 * conv[-1]
    return (f, h), (fb, hb)


class TorchComposed:
    """The layers of PointNetHIP from torch ops."""

    def __init__(self, net, weights, torch):
        from learn_region_grow_amd import pointnet as P
        from learn_region_grow_amd.checkpoint import pointnet_bn_names
        self.torch = torch
        dev = net.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.conv = [(t(weights['kernel%d' % i].reshape(-1, c)), t(weights['bias%d' % i])) for i, c in enumerate(net.conv_widths)]
        self.fc = [(t(weights['fc_weights%d' % j][0]), t(weights['fc_bias%d' % j])) for j in range(len(net.fc_widths) + 1)]
        self.bn = [tuple(t(x) for x in P.fold_batch_norm(*(weights[n] for n in pointnet_bn_names(j)))) for j in range(len(net.fc_widths))]

    def forward(self, x, mark=None):
        torch = self.torch
        acts = []
        for w, b in self.conv:
            x = torch.relu(torch.matmul(x, w) + b)
            acts.append(x)
        pooled = acts[-1].amax(dim=1, keepdim=True)
        if mark:
            mark('features')
        x = torch.cat([acts[-1] - pooled, acts[1]], dim=2)
        for (w, b), (scale, shift) in zip(self.fc[:-1], self.bn):
            x = torch.relu((torch.matmul(x, w) + b) * scale + shift)
        x = torch.matmul(x, self.fc[-1][0]) + self.fc[-1][1]
        if mark:
            mark('head')
        return x


def measure(name, conv, fc, raws, args, torch):
    import pointnet_ref as R
    from learn_region_grow_amd import pointnet as P
    weights = R.random_weights(0, conv, fc, args.num_class)
    net = P.PointNetHIP(weights)
    composed = TorchComposed(net, weights, torch)
    res = P.grid_resolution('5')

    def end_to_end():
        rooms = [P.prepare_room(r) for r in raws]
        parts = [split_cell_inputs(r['points'], res) for r in rooms]
        cls = net.classify_cells(np.concatenate([b for b, _, _ in parts]))
        classes, c = [], 0
        for r, (_, members, _) in zip(rooms, parts):
            out = np.zeros(len(r['points']), dtype=np.int32)
            for idx in members:
                out[idx] = cls[c, :len(idx)]
                c += 1
            classes.append(out)
        return rooms, parts, P.segment(rooms, classes)
    rooms, parts, labels = end_to_end()                              # warm-up
    e2e = []
    for _ in range(args.e2e_repeats):
        torch.cuda.synchronize()
        t0 = time.time()
        end_to_end()
        e2e.append(time.time() - t0)
    batch = np.concatenate([b for b, _, _ in parts])
    n_cells = len(batch)
    chunks = [torch.from_numpy(batch[c0:c0 + P.CHUNK_CELLS]).to(net.device) for c0 in range(0, n_cells, P.CHUNK_CELLS)]
    fused, composed_t = [], []
    for _ in range(args.rounds):                                     # alternate, so that both see the same machine
        fused.append(timed_pass(torch, lambda x, mark: net._forward(x, mark=mark), chunks, args.warmup, args.repeats))
        composed_t.append(timed_pass(torch, composed.forward, chunks, args.warmup, args.repeats))
    diff = max(float((net._forward(x) - composed.forward(x)).abs().max()) for x in chunks[:2])
    best = lambda rounds: min(rounds, key=lambda r: r[1]['median'])
    stages, whole = best(fused)
    t_stages, t_whole = best(composed_t)
    (f_flop, h_flop), (f_bytes, h_bytes) = flops_and_bytes_per_cell(conv, fc, args.num_class)

    def kernel(flop, nbytes, seconds):
        t_flop, t_bytes = flop * n_cells / (PEAK_TFLOPS * 1e12), nbytes * n_cells / (HBM_TBPS * 1e12)
        return dict(flop=flop * n_cells, hbm_bytes=nbytes * n_cells, seconds=seconds, tflops=flop * n_cells / seconds * 1e-12,
                    share_of_fp32_matrix_peak=t_flop / seconds, hbm_TBps=nbytes * n_cells / seconds * 1e-12, share_of_hbm_peak=t_bytes / seconds,
                    larger_bound='matrix' if t_flop >= t_bytes else 'hbm')
    out = dict(network=name, conv_widths=list(conv), fc_widths=list(fc), num_class=args.num_class, rooms=len(raws),
               points=int(sum(len(r['points']) for r in rooms)), cells=n_cells, cells_split=int(sum(s for _, _, s in parts)),
               clusters=int(sum(int(l.max()) for l in labels)),
               end_to_end_s=stats(e2e), rooms_per_s=len(raws) / float(np.median(e2e)), cells_per_s_end_to_end=n_cells / float(np.median(e2e)),
               network_pass_s=whole, network_cells_per_s=n_cells / whole['median'], stages_s=stages,
               network_pass_median_s_by_round=[r[1]['median'] for r in fused],
               features=kernel(f_flop, f_bytes, stages['features']['median']), head=kernel(h_flop, h_bytes, stages['head']['median']),
               torch_composed=dict(network_pass_s=t_whole, stages_s=t_stages, network_pass_median_s_by_round=[r[1]['median'] for r in composed_t],
                                   max_abs_logit_difference=diff, fused_over_torch_pass_time=whole['median'] / t_whole['median']))
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pointnet_bench.json'))
    ap.add_argument('--num-class', type=int, default=13)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--e2e-repeats', type=int, default=3)
    ap.add_argument('--rooms', type=int, default=68)
    args = ap.parse_args()
    import torch
    import pointnet_ref as R
    from learn_region_grow_amd import pointnet as P, synthetic
    if not torch.cuda.is_available():
        raise SystemExit('tools/pointnet_bench.py measures on the GPU; none is visible')
    out = dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TFLOPS, hbm_TBps=HBM_TBPS, chunk_cells=P.CHUNK_CELLS, warmup=args.warmup,
               repeats=args.repeats, rounds=args.rounds, networks=[])
    area5 = [synthetic.area5_shaped_room(t, 1000 + i).astype(np.float32) for i, t in enumerate(synthetic.AREA5_POINTS[:args.rooms])]
    for name, (conv, fc) in (('shipped', R.SHIPPED), ('current', R.CURRENT)):
        out['networks'].append(measure(name, conv, fc, area5, args, torch))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
