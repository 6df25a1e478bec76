#!/usr/bin/env python3
"""Measure --save's PLY export on the host and on the device -> profiles/ply_bench.json.

The set: the raw points of the 68 Area-5-shaped rooms of the other benches (synthetic.area5_shaped_room at AREA5_POINTS, seeds 1000 + i),
coloured per point from a label table as the drivers' --save colours them, written as one PLY per room.

  host     io.savePLY room by room, the Python loop of one formatted line per vertex: the baseline
  device   io.save_rooms_ply_device, all rooms in one launch, by the wall clock around work that ends in a synchronise and in closed
           files; and its parts, each measured on its own: the upload, lrg_text_encode alone between two device events (inputs
           resident: length pass + scan + write pass), encode_points_device (upload, kernels, the download into pinned memory), and the
           file writes from the downloaded bodies
  traffic  the bytes the three steps read and write, from the shapes (68 n + text bytes: see kernel_bytes), over the event time, and
           that rate as a share of the HBM peak (8 TB/s, the specification's figure)
  check    every device file equal to the host file, byte for byte

Repeats alternate device and host runs; the first device run is a warm-up and is not kept.

    python tools/ply_bench.py [--out profiles/ply_bench.json] [--repeats 5] [--host-repeats 2] [--rooms 68] [--tmp DIR]
"""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK_BYTES_PER_S = 8.0e12


def spread(xs):
    xs = sorted(xs)
    return dict(median=float(np.median(xs)), min=float(xs[0]), max=float(xs[-1]), repeats=len(xs))


def kernel_bytes(n, text_bytes):
    """What the three steps move for n rows of xyz [n, 3] and rgb [n, 3]: the length pass reads both (24 n) and writes a length (4 n); the
    scan reads the lengths twice and writes the offsets (12 n); the write pass reads the rows again (24 n) and an offset (4 n) and
    writes the text."""
    return 68 * n + text_bytes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ply_bench.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-repeats', type=int, default=2)
    ap.add_argument('--rooms', type=int, default=68)
    ap.add_argument('--tmp', default=None, help='where the files are written (default: a temporary directory)')
    args = ap.parse_args()
    import torch
    from learn_region_grow_amd import io as lio
    from learn_region_grow_amd import synthetic
    if not torch.cuda.is_available():
        raise SystemExit('ply_bench.py needs a GPU: a host run measures nothing of the device path')
    if args.repeats < 5 or args.host_repeats < 1:
        raise SystemExit('--repeats: at least five; --host-repeats: at least one')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    raw = [synthetic.area5_shaped_room(t, 1000 + i).astype(np.float32) for i, t in enumerate(synthetic.AREA5_POINTS[:args.rooms])]
    R = len(raw)
    colours = lio.label_colors(64)
    xyz = [np.ascontiguousarray(r[:, :3]) for r in raw]
    rgb = [colours[r[:, 6].astype(np.int64) % 64].astype(np.int32) for r in raw]
    clouds = [np.hstack([x.astype(np.float64), c.astype(np.float64)]) for x, c in zip(xyz, rgb)]      # what the drivers hand savePLY
    n = int(sum(len(x) for x in xyz))
    start = np.concatenate([[0], np.cumsum([len(x) for x in xyz])])
    top = args.tmp or tempfile.mkdtemp(prefix='ply_bench_')
    hdir, ddir = os.path.join(top, 'host'), os.path.join(top, 'device')
    for d in (hdir, ddir):
        os.makedirs(d, exist_ok=True)
    hnames, dnames = [os.path.join(hdir, '%d.ply' % i) for i in range(R)], [os.path.join(ddir, '%d.ply' % i) for i in range(R)]
    quiet = io.StringIO()
    host_s, path_s = [], []
    for rep in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(quiet):
            routes = lio.save_rooms_ply_device(dnames, xyz, rgb, device=dev)
        if rep:                                               # (the first run loads the code objects and pins for the first time)
            path_s.append(time.perf_counter() - t0)
        assert routes == ['device'] * R
        if rep < args.host_repeats:
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(quiet):
                for name, cloud in zip(hnames, clouds):
                    lio.savePLY(name, cloud)
            host_s.append(time.perf_counter() - t0)
            print('host %.2f s' % host_s[-1])
            sys.stdout.flush()
    same = all(open(a, 'rb').read() == open(b, 'rb').read() for a, b in zip(hnames, dnames))
    file_bytes = int(sum(os.path.getsize(p) for p in hnames))
    # ---- the parts ----
    all_xyz, all_rgb = np.concatenate(xyz), np.concatenate(rgb)
    upload_s, kernel_s, encode_s, write_s = [], [], [], []
    text_bytes = 0
    for rep in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_xyz, d_rgb = torch.from_numpy(all_xyz).to(dev), torch.from_numpy(all_rgb).to(dev)
        torch.cuda.synchronize()
        t_up = time.perf_counter() - t0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ws = lio.text_encode_device(d_xyz, d_rgb, 'ply')      # (allocations warmed: the timed call below reuses the allocator's blocks)
        del ws
        e0.record()
        line_off, text, status = lio.text_encode_device(d_xyz, d_rgb, 'ply')
        e1.record()
        torch.cuda.synchronize()
        t_k = e0.elapsed_time(e1) * 1e-3
        text_bytes = int(line_off[-1].item())
        assert int(status.item()) == 0
        del line_off, text, status, d_xyz, d_rgb
        t0 = time.perf_counter()
        bodies = lio.encode_points_device(all_xyz, all_rgb, start, 'ply', device=dev)
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        for name, body, x in zip(dnames, bodies, xyz):
            with open(name, 'wb') as f:
                f.write(lio._ply_header(len(x)).encode('ascii'))
                f.write(body)
        t_wr = time.perf_counter() - t0
        if rep:
            upload_s.append(t_up), kernel_s.append(t_k), encode_s.append(t_enc), write_s.append(t_wr)
    h, p, k = spread(host_s), spread(path_s), spread(kernel_s)
    moved = kernel_bytes(n, text_bytes)
    out = dict(device=torch.cuda.get_device_name(0), rooms=R, vertices=n, file_bytes=file_bytes, text_bytes=text_bytes,
               host_seconds=h, host_vertices_per_s=n / h['median'],
               device_path_seconds=p, device_path_vertices_per_s=n / p['median'],
               device_parts_seconds=dict(upload=spread(upload_s), kernels_events=k, upload_kernels_download=spread(encode_s), file_writes=spread(write_s)),
               kernel_bytes_moved=moved, kernel_bytes_per_s=moved / k['median'], kernel_share_of_hbm_peak=moved / k['median'] / HBM_PEAK_BYTES_PER_S,
               hbm_peak_bytes_per_s=HBM_PEAK_BYTES_PER_S,
               speedup_median=h['median'] / p['median'], device_beats_host_beyond_spread=bool(p['max'] < h['min']), files_equal=bool(same))
    print('%d rooms, %d vertices, %.1f MB: host %.2f s, device path %.3f s (x%.1f): upload %.4f s, kernels %.5f s (%.0f GB/s, %.1f %% of the HBM peak), '
          'upload + kernels + download %.3f s, file writes %.3f s; files equal %s'
          % (R, n, file_bytes / 1e6, h['median'], p['median'], out['speedup_median'], np.median(upload_s), k['median'], moved / k['median'] / 1e9,
             100 * out['kernel_share_of_hbm_peak'], np.median(encode_s), np.median(write_s), same))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    if args.tmp is None:
        shutil.rmtree(top, ignore_errors=True)
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
