#!/usr/bin/env python3
"""Measure the PointNet2 baseline on the GPU (learn_region_grow_amd.pointnet2) -> profiles/pointnet2_bench.json.

Sets: the 68 Area-5-shaped rooms (synthetic.area5_shaped_room at AREA5_POINTS, equalised at 0.1 m, 1 m cells) and one
KITTI-shaped scene (100 k target points at 0.3 m, 3 m cells).  The synthetic rooms fill every surface voxel, so some of their 1 m
cells hold more than 1024 points, where the reference (benchmarks.py:298) and pointnet2.cell_inputs stop; the tool cuts such a cell
into pieces of at most 1024 points in index order and counts them (cells_split), so that every point is still classified.

Reported per set:
  end to end     rooms/s and cells/s from the raw rooms to the labels: device equalisation, the host's cell cut and padding, uploads,
                 the network in chunks of 64 cells, argmax, the scatter back, the segmentation.  Wall clock, --e2e-repeats runs
                 after one warm-up; median, minimum and maximum.
  stages         device time of every launch kind of the network by HIP events recorded between the launches, summed over the
                 chunks of one pass over all cells; --repeats passes after --warmup; median, minimum and maximum.
  MLP kernels    lrg_pointnet2_group_mlp and lrg_pointnet2_row_mlp (head included): FLOPs counted from the shapes (2 x rows x
                 sum k n over the layers, unpadded) over their stage time, as a share of the 157.3 TFLOP/s fp32 matrix peak.
  torch          the same network with the shared MLPs composed from torch ops on the same device and inputs -- index_select of
                 the grouped rows, matmul + bias + relu, amax over the samples; cat + matmul for the propagation levels -- the
                 sampling, ball-query and interpolation launches unchanged.  Its pass time beside the fused pass time, and the
                 largest difference of the logits.

    python tools/pointnet2_bench.py [--out profiles/pointnet2_bench.json] [--num-class 13]
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

PEAK_TFLOPS = 157.3
SA_MLPS = ((32, 32, 64), (64, 64, 128), (128, 128, 256), (256, 256, 512))
FP_MLPS = ((256, 256), (256, 256), (256, 128), (128, 128, 128))
SA_POINTS = (1024, 256, 64, 16)


def mlp_flops_per_cell(num_class, rgb):
    """(grouped, row) FLOPs of one cell, 2 per multiply-add, unpadded shapes."""
    feat = [3 if rgb else 0, 64, 128, 256, 512]
    grouped = 0
    for lv, mlp in enumerate(SA_MLPS):
        k, rows = 3 + feat[lv], SA_POINTS[lv] * 32
        for n in mlp:
            grouped += 2 * rows * k * n
            k = n
    row, up = 0, 512
    dst_points = (64, 256, 1024, 1024)
    for lv, mlp in enumerate(FP_MLPS):
        k = up + feat[3 - lv]
        for n in mlp:
            row += 2 * dst_points[lv] * k * n
            k = n
        up = mlp[-1]
    row += 2 * 1024 * (128 * 128 + 128 * num_class)
    return grouped, row


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), repeats=len(xs))


def split_cell_inputs(points, res):
    """pointnet2.cell_inputs, but a cell of more than 1024 points becomes several of at most 1024 (in index order)."""
    from learn_region_grow_amd import pointnet2 as P
    p = np.asarray(points, dtype=np.float32)[:, :6]
    keys, members = P.cells(p, res)
    pieces, split = [], 0
    for c, idx in enumerate(members):
        split += len(idx) > P.NUM_POINT
        for s in range(0, len(idx), P.NUM_POINT):
            pieces.append((keys[c], idx[s:s + P.NUM_POINT]))
    batch = np.empty((len(pieces), P.NUM_POINT, 6), dtype=np.float32)
    for c, (key, idx) in enumerate(pieces):
        rows = p[idx].copy()
        rows[:, :2] -= (key * float(res)).astype(np.float32)
        rows[:, 2] -= rows[:, 2].min()
        batch[c, :len(idx)] = rows
        batch[c, len(idx):] = rows[0]
    return batch, [idx for _, idx in pieces], split


class TorchComposed:
    """PointNet2HIP with the two shared MLPs replaced by torch ops; every other launch is the package's."""

    def __init__(self, net, weights, torch):
        self.net, self.torch = net, torch
        dev = net.device

        def layers(scope, ids):
            return [(torch.from_numpy(np.ascontiguousarray(weights['%skernel%d' % (scope, i)].reshape(weights['%skernel%d' % (scope, i)].shape[-2:]))).to(dev),
                     torch.from_numpy(np.ascontiguousarray(weights['%sbias%d' % (scope, i)])).to(dev)) for i in ids]
        self.sa = [layers('layer%d/' % (lv + 1), range(3)) for lv in range(4)]
        self.fp = [layers('fa_layer%d/' % (lv + 1), range(len(m))) for lv, m in enumerate(FP_MLPS)]
        self.head = layers('', (1, 2))

    def _mlp(self, x, layers, relu_last=True):
        torch = self.torch
        for n, (w, b) in enumerate(layers):
            x = torch.matmul(x, w) + b
            if relu_last or n + 1 < len(layers):
                x = torch.relu(x)
        return x

    def forward(self, x, mark=None):
        from learn_region_grow_amd import _lib, grouping, sampling
        from learn_region_grow_amd import pointnet2 as P
        torch, net = self.torch, self.net
        mark = mark or (lambda name: None)
        b = x.shape[0]
        xyz = [x[:, :, :3].contiguous()]
        feat = [x[:, :, 3:].contiguous() if net.rgb_features else None]
        for lv, (npoint, radius) in enumerate(P.SA_LEVELS):
            fps = sampling.farthest_point_sample(npoint, xyz[lv])
            mark('fps')
            new_xyz = sampling.gather_point(xyz[lv], fps)
            mark('gather')
            idx, _ = grouping.query_ball_point(radius, P.NSAMPLE, xyz[lv], new_xyz)
            mark('ball_query')
            n = xyz[lv].shape[1]
            flat = (idx.long() + (torch.arange(b, device=x.device) * n).view(b, 1, 1)).reshape(-1)
            g = torch.index_select(xyz[lv].reshape(b * n, 3), 0, flat).view(b, npoint, P.NSAMPLE, 3) - new_xyz.unsqueeze(2)
            if feat[lv] is not None:
                c = feat[lv].shape[2]
                g = torch.cat([g, torch.index_select(feat[lv].reshape(b * n, c), 0, flat).view(b, npoint, P.NSAMPLE, c)], dim=3)
            new_feat = self._mlp(g, self.sa[lv]).amax(dim=2)
            mark('group_mlp')
            xyz.append(new_xyz)
            feat.append(new_feat)
        up = feat[4]
        for lv in range(4):
            dst = 3 - lv
            n, m, c = xyz[dst].shape[1], xyz[dst + 1].shape[1], up.shape[2]
            interp = torch.empty((b, n, c), dtype=torch.float32, device=x.device)
            _lib.check(net.lib.lrg_three_nn_interpolate(b, n, m, c, P._ptr(xyz[dst]), P._ptr(xyz[dst + 1]), P._ptr(up.contiguous()), None, None, None,
                                                        P._ptr(interp), P._stream()), 'lrg_three_nn_interpolate')
            mark('three_nn_interpolate')
            up = self._mlp(interp if feat[dst] is None else torch.cat([interp, feat[dst]], dim=2), self.fp[lv])
            mark('row_mlp')
        out = self._mlp(up, self.head, relu_last=False)
        mark('head')
        return out


def timed_pass(torch, forward, chunks, warmup, repeats):
    """-> ({stage: stats of seconds per pass}, stats of the whole pass), events between the launches."""
    per_stage, whole = {}, []
    for it in range(warmup + repeats):
        events = []
        torch.cuda.synchronize()
        for x in chunks:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            events.append(('start', e))

            def mark(name):
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                events.append((name, ev))
            forward(x, mark)
        torch.cuda.synchronize()
        if it < warmup:
            continue
        acc = {}
        for (_, e0), (name, e1) in zip(events[:-1], events[1:]):
            if name != 'start':
                acc[name] = acc.get(name, 0.0) + e0.elapsed_time(e1) * 1e-3
        for k, v in acc.items():
            per_stage.setdefault(k, []).append(v)
        whole.append(sum(acc.values()))
    return {k: stats(v) for k, v in per_stage.items()}, stats(whole)


def measure_set(name, raws, area, net, composed, weights, args, torch):
    from learn_region_grow_amd import pointnet2 as P
    res = P.grid_resolution(area)

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
        labels = P.segment(rooms, classes)
        return rooms, parts, labels
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
    stages, whole = timed_pass(torch, lambda x, mark: net._forward(x, mark=mark), chunks, args.warmup, args.repeats)
    t_stages, t_whole = timed_pass(torch, composed.forward, chunks, args.warmup, args.repeats)
    diff = max(float((net._forward(x) - composed.forward(x)).abs().max()) for x in chunks[:2])
    g_flop, r_flop = mlp_flops_per_cell(net.num_class, net.rgb_features)
    g_s = stages['group_mlp']['median']
    r_s = stages['row_mlp']['median'] + stages['head']['median']
    out = dict(set=name, area=area, rooms=len(raws), points=int(sum(len(r['points']) for r in rooms)), cells=n_cells,
               cells_split=int(sum(s for _, _, s in parts)), clusters=int(sum(int(l.max()) for l in labels)),
               end_to_end_s=stats(e2e), rooms_per_s=len(raws) / float(np.median(e2e)), cells_per_s=n_cells / float(np.median(e2e)),
               network_pass_s=whole, stages_s=stages,
               group_mlp=dict(flop=g_flop * n_cells, tflops=g_flop * n_cells / g_s * 1e-12, share_of_peak=g_flop * n_cells / g_s * 1e-12 / PEAK_TFLOPS),
               row_mlp=dict(flop=r_flop * n_cells, tflops=r_flop * n_cells / r_s * 1e-12, share_of_peak=r_flop * n_cells / r_s * 1e-12 / PEAK_TFLOPS),
               torch_composed=dict(network_pass_s=t_whole, stages_s=t_stages, max_abs_logit_difference=diff,
                                   fused_over_torch_pass_time=whole['median'] / t_whole['median']))
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pointnet2_bench.json'))
    ap.add_argument('--num-class', type=int, default=13)
    ap.add_argument('--rgb-features', action='store_true', help='the variant of train_pointnet.py:178 (default: :177, the shipped models)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--e2e-repeats', type=int, default=3)
    ap.add_argument('--rooms', type=int, default=68)
    args = ap.parse_args()
    import torch
    import pointnet2_ref as R
    from learn_region_grow_amd import pointnet2 as P, synthetic
    weights = R.random_weights(0, args.num_class, args.rgb_features)
    net = P.PointNet2HIP(weights)
    composed = TorchComposed(net, weights, torch)
    out = dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TFLOPS, num_class=args.num_class, rgb_features=bool(args.rgb_features),
               chunk_cells=P.CHUNK_CELLS, warmup=args.warmup, repeats=args.repeats,
               mlp_flop_per_cell=dict(zip(('group_mlp', 'row_mlp'), mlp_flops_per_cell(args.num_class, args.rgb_features))), sets=[])
    area5 = [synthetic.area5_shaped_room(t, 1000 + i).astype(np.float32) for i, t in enumerate(synthetic.AREA5_POINTS[:args.rooms])]
    out['sets'].append(measure_set('area5_%d_rooms' % len(area5), area5, '5', net, composed, weights, args, torch))
    kitti = [synthetic.area5_shaped_room(100000, 5000, resolution=0.3).astype(np.float32)]
    out['sets'].append(measure_set('kitti_100k_scene', kitti, 'kitti_val', net, composed, weights, args, torch))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
