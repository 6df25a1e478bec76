#!/usr/bin/env python3
"""Measure the growth trace and the renderer of animate_region_growing.py -> profiles/animate_bench.json.

Workload: one Area-5-shaped room of about 100 k raw points (synthetic.area5_shaped_room, trained weights, the network's policy, the
counter stream), pictures of 1000 x 1000.  Recorded, each after a warm-up and as the median of its repeats:

  visibility   lrg_render_visibility between two events
  shade        lrg_render_shade of 32 frames (16 step frames with text, 16 seg frames) between two events, per frame
  download     the copy of those 32 frames to the host, per frame
  png          io.encode_png (zlib level 1) of a step frame and of a seg frame on the host, per frame
  lock-step    the room grown by the trace's own loop -- one packed iteration per host call, one synchronisation per batch -- with
               the trace OFF, and the same loop with lrg_trace_snapshot behind every call (the two alternate); `snapshot_per_step` is
               their difference per host call and `trace_adds` that difference as a share of the loop WITHOUT the trace
  end to end   animate_region_growing.run (synthetic weights) for --frames picture pairs: steps and pictures per second of its grow-and-draw loop
  twin         tests/animate_ref.py (NumPy): rasterising the room and shading one step + one seg frame, per frame

    python tools/animate_bench.py [--out profiles/animate_bench.json] [--points 37000] [--size 1000] [--frames 128] [--repeats 5]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, 'tests'))


def median(xs):
    return float(np.median(xs))


def event_ms(torch, fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def lockstep(torch, trace, net, room, uneq, batch, traced):
    """The room grown by the trace's loop; traced False: the same calls and synchronisations without the snapshots.  -> (seconds, host calls, frames)."""
    gr = trace.make_grower(net, seed=0)
    tr = trace.GrowthTrace(gr, room, uneq, frames_per_batch=batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frames = 0
    if traced:
        for b in tr.batches():
            frames += len(b)
    else:
        h = torch.zeros(2, dtype=torch.int64).pin_memory()
        while True:
            for _ in range(batch):
                gr.enqueue_iteration()
                tr.calls += 1
            h.copy_(gr.d_stats[:2], non_blocking=True)
            torch.cuda.current_stream(gr.dev).synchronize()
            if int(h[1]) > 0:
                break
    return time.perf_counter() - t0, tr.calls, frames


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'animate_bench.json'))
    ap.add_argument('--points', type=int, default=37000, help='equalised points of the room (about 2.7 raw points each)')
    ap.add_argument('--size', type=int, default=1000)
    ap.add_argument('--frames', type=int, default=128, help='picture pairs of the end-to-end run')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    args = ap.parse_args()
    import torch
    import animate_ref as ar
    import animate_region_growing as driver
    from learn_region_grow_amd import io as lio
    from learn_region_grow_amd import preprocess_gpu, render, synthetic, trace
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    assert torch.cuda.is_available(), 'animate_bench.py measures on the GPU'
    dev = torch.device('cuda:0')
    raw = synthetic.area5_shaped_room(args.points, 1).astype(np.float32)
    pre = preprocess_gpu.preprocess_room(raw[:, :6], raw[:, 6].astype(int), raw[:, 7].astype(int), device=dev, eig='exact')
    room = dict(points=pre['points'], obj_id=pre['obj_id'], order=pre['order'].astype(np.int32), room_id=0)
    uneq, n, S = pre['unequalized_idx'], len(pre['points']), args.size
    out = dict(room=dict(raw_points=int(len(raw)), equalised_points=int(n)), size=S, repeats=args.repeats, device=torch.cuda.get_device_name(0))
    net = LrgNetHIP(1, 1, 512, 512, 13, 0, device=dev).load_weights(synthetic.load_trained_weights())

    # ---- renderer ----
    rd = render.Renderer(raw[:, :3], uneq, n, S, S, 5, device=dev)
    out['visibility_ms'] = median(event_ms(torch, rd.build_visibility, args.repeats))
    out['pixels_covered'] = int((rd.d_vis != -1).sum().item())
    # frames to shade: a short traced run of the room itself
    tr = trace.GrowthTrace(trace.make_grower(net, seed=0), room, uneq, frames_per_batch=16)
    batch = next(tr.batches())
    k = len(batch)
    index = torch.cat([batch.codes, batch.paints])
    luts = [render.LUT_STEP] * k + [render.LUT_SEG] * k
    texts = [render.text_lines(*[int(x) for x in h[[1, 3, 4, 5, 6]]]) for h in batch.headers] + [None] * k
    out['shade_frames'] = 2 * k
    out['shade_ms_per_frame'] = median(event_ms(torch, lambda: rd.shade(index, luts, texts), args.repeats)) / (2 * k)
    frames = rd.shade(index, luts, texts)
    torch.cuda.synchronize()
    dl = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        host = frames.cpu().numpy()
        dl.append((time.perf_counter() - t0) * 1e3 / (2 * k))
    out['download_ms_per_frame'] = median(dl)
    pal = rd.palette
    for name, fr in (('step', host[k - 1]), ('seg', host[2 * k - 1])):
        ts, size = [], 0
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            size = len(lio.encode_png(fr, pal))
            ts.append((time.perf_counter() - t0) * 1e3)
        out['png_%s_ms_per_frame' % name], out['png_%s_bytes' % name] = median(ts), size

    # ---- what tracing adds to the lock-step loop ----
    lockstep(torch, trace, net, room, uneq, args.batch, True)          # warm-up of both
    lockstep(torch, trace, net, room, uneq, args.batch, False)
    off, on, calls, steps = [], [], 0, 0
    for _ in range(max(3, args.repeats)):                               # alternating
        t, calls_off, _ = lockstep(torch, trace, net, room, uneq, args.batch, False)
        off.append(t)
        t, calls, steps = lockstep(torch, trace, net, room, uneq, args.batch, True)
        on.append(t)
        assert calls == calls_off, (calls, calls_off)
    out['lockstep'] = dict(host_calls=calls, steps=steps, batch=args.batch, untraced_s=sorted(off), traced_s=sorted(on),
                           untraced_us_per_call=median(off) / calls * 1e6, traced_us_per_call=median(on) / calls * 1e6,
                           snapshot_us_per_step=(median(on) - median(off)) / calls * 1e6, trace_adds=(median(on) - median(off)) / median(off))

    # ---- end to end: the driver's loop ----
    with tempfile.TemporaryDirectory() as tmp:
        h5 = os.path.join(tmp, 'room.h5')
        lio.saveToH5(h5, [raw])
        r = driver.run(driver.parse(['--h5', h5, '--room', '0', '--synthetic-weights', '--size', str(S), '--max-frames', str(args.frames), '--out', os.path.join(tmp, 'f')]))
    out['end_to_end'] = dict(steps=r['steps'], pictures=r['pictures'], seconds=r['seconds'], frames_per_s=r['pictures'] / r['seconds'],
                             steps_per_s=r['steps'] / r['seconds'], ms_per_picture=r['seconds'] / r['pictures'] * 1e3)

    # ---- the twin on the host ----
    t0 = time.perf_counter()
    vis = ar.visibility(raw[:, :3], ar.camera_matrix(S, S), S, S, 5)
    out['twin_visibility_ms'] = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(vis, rd.d_vis.cpu().numpy().view(np.uint64))
    idx2 = index[[k - 1, 2 * k - 1]].cpu().numpy()
    t0 = time.perf_counter()
    want = ar.shade(vis, uneq, idx2, [0, 1], [texts[k - 1], None], S, S, render.font_table())
    out['twin_shade_ms_per_frame'] = (time.perf_counter() - t0) * 1e3 / 2
    assert np.array_equal(want, host[[k - 1, 2 * k - 1]])
    gpu_frame = out['shade_ms_per_frame'] + out['download_ms_per_frame'] + 0.5 * (out['png_step_ms_per_frame'] + out['png_seg_ms_per_frame'])
    out['per_frame_ms'] = dict(shade=out['shade_ms_per_frame'], download=out['download_ms_per_frame'],
                               png=0.5 * (out['png_step_ms_per_frame'] + out['png_seg_ms_per_frame']), total=gpu_frame)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
