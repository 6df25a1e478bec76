#!/usr/bin/env python3
"""Generate tests/golden/mcpnet_ref_cpu.npz and tests/golden/mcpnet_model5_weights.npz by executing the REFERENCE's test_mcpnet.py,
unmodified, in the build container (needs the reference checkout; never runs on the GPU box).

    python tests/golden/make_mcpnet_golden.py [<reference checkout>]

TensorFlow comes from tf_numpy_standin; this generator attaches the two symbols MCPNet needs beyond LrgNet: tf.matmul (float32
numpy.matmul) and tf.nn.l2_normalize (float32 x * (1 / sqrt(max(sum(x * x), 1e-12)))).  Saver.restore gets the eight trainables of
the reference's models/mcpnet_model5.ckpt through checkpoint.load_mcpnet_weights (every tensor checked against its CRC-32C).
The room file is three seeded rooms (tests/mcpnet_ref.py: golden_rooms).  What the script computes is recorded by wrapping, before it
runs: numpy.random.choice (candidate count, replace flag and the drawn neighbour indices of every point), the l2_normalize node (the
float32 embeddings) and sklearn.metrics.normalized_mutual_info_score (cluster_label of every room).  The room seeds are walked until
both replace=True and replace=False draws occur, a component is kept and one of 2 .. 10 points dropped, and every 26-neighbour dot of
the embeddings lies at least 1e-5 from the 0.9 threshold; that margin is stored, so no test has to skip on a near-tie.
"""
import contextlib
import io
import os
import runpy
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import tf_numpy_standin as standin  # noqa: E402
import mcpnet_ref as R  # noqa: E402
from learn_region_grow_amd import checkpoint  # noqa: E402

MIN_MARGIN = 1e-5
SEEDS = [(21 + 2 * k, 22 + 2 * k, 11 + k) for k in range(20)]


def run_reference(ref, rooms, weights):
    """test_mcpnet.py --area 5 on the room file `rooms` -> (choice calls, embeddings per room, labels per room, printed lines)."""
    tf = standin.install()
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    tf.matmul = lambda a, b: standin.Node(lambda x, y: np.matmul(f32(x), f32(y)), (a, b))
    embs = []

    def l2n(x, axis=None):
        def run(a):
            a = f32(a)
            out = a * (np.float32(1) / np.sqrt(np.maximum((a * a).sum(axis=axis, keepdims=True), np.float32(1e-12))))
            embs.append(np.array(out, dtype=np.float32))
            return out
        return standin.Node(run, (x,))
    tf.nn.l2_normalize = l2n
    import sklearn.metrics
    sys.modules.pop('learn_region_grow_util', None)
    standin.H5_FILES.clear()
    standin.H5_FILES['data/s3dis_area5.h5'] = {'points': np.vstack(rooms), 'count_room': np.array([len(r) for r in rooms], dtype=np.int32)}
    standin.RESTORE_WEIGHTS.clear()
    standin.RESTORE_WEIGHTS.update(weights)
    labels, calls = [], []
    orig_nmi, orig_choice = sklearn.metrics.normalized_mutual_info_score, np.random.choice

    def recording_nmi(obj_id, cluster_label, *args, **kw):
        labels.append(np.array(cluster_label, dtype=np.int32))
        return orig_nmi(obj_id, cluster_label, *args, **kw)

    def recording_choice(a, size=None, replace=True, p=None):
        r = orig_choice(a, size, replace, p)
        calls.append((len(a), bool(replace), np.array(r, dtype=np.int64)))
        return r
    old_argv, old_cwd, old_path = sys.argv, os.getcwd(), list(sys.path)
    buf = io.StringIO()
    try:
        sklearn.metrics.normalized_mutual_info_score = recording_nmi
        np.random.choice = recording_choice
        os.chdir(ref)
        sys.path.insert(0, ref)
        sys.argv = ['test_mcpnet.py', '--area', '5']
        with contextlib.redirect_stdout(buf):
            runpy.run_path(os.path.join(ref, 'test_mcpnet.py'), run_name='__main__')
    finally:
        sklearn.metrics.normalized_mutual_info_score = orig_nmi
        np.random.choice = orig_choice
        sys.argv = old_argv
        os.chdir(old_cwd)
        sys.path[:] = old_path
    assert len(labels) == len(rooms) and len(embs) == len(calls)
    return calls, np.concatenate(embs), labels, buf.getvalue().rstrip('\n').split('\n')


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    weights = checkpoint.load_mcpnet_weights(os.path.join(ref, 'models', 'mcpnet_model5.ckpt'))
    for seeds in SEEDS:
        rooms = R.golden_rooms(seeds)
        calls, emb_all, labels, lines = run_reference(ref, rooms, weights)
        sizes = [len(l) for l in labels]
        starts = np.concatenate([[0], np.cumsum(sizes)])
        embs = [emb_all[starts[r]:starts[r + 1]] for r in range(len(rooms))]
        pts = [R.equalize(R.center(r))[0] for r in rooms]
        margin = min(float(np.abs(R.edge_pairs(p, e)[2] - 0.9).min()) for p, e in zip(pts, embs))
        kept = sum(int(l.max()) for l in labels)
        dropped = 0
        for p, e in zip(pts, embs):
            c = R.components(p, e, min_cluster_size=1)
            _, cnt = np.unique(c[c > 0], return_counts=True)
            dropped += int(((cnt >= 2) & (cnt <= 10)).sum())
        modes = {c[1] for c in calls}
        print(seeds, 'margin %.3g kept %d dropped %d replace modes %s' % (margin, kept, dropped, sorted(modes)))
        if margin >= MIN_MARGIN and kept > 0 and dropped > 0 and modes == {True, False}:
            break
    else:
        raise SystemExit('no room seeds tried satisfy the golden conditions')
    out = {'rooms_digest': np.array(R.rooms_digest(rooms)), 'seeds': np.array(seeds), 'margin': np.array(margin)}
    nbr_all = []
    for r in range(len(rooms)):
        cs = calls[starts[r]:starts[r + 1]]
        nbr = np.stack([c[2] for c in cs]).astype(np.int32)
        nbr_all.append(nbr)
        out['counts%d' % r] = np.array([c[0] for c in cs], dtype=np.int16)
        out['nbr_head%d' % r] = nbr[:256].astype(np.int16)
        out['emb%d' % r] = embs[r].astype(np.float32)
        out['label%d' % r] = labels[r].astype(np.int16)
    out['nbr_digest'] = np.array(R.nbr_digest(nbr_all))
    out['room_lines'] = np.array([l for l in lines if l.startswith('Area ')])
    out['restored_line'] = np.array(lines[0])
    out['aggregate_line'] = np.array(lines[-1])
    path = os.path.join(HERE, 'mcpnet_ref_cpu.npz')
    np.savez_compressed(path, **out)
    np.savez(os.path.join(HERE, 'mcpnet_model5_weights.npz'), **{k: np.asarray(v, dtype=np.float32) for k, v in weights.items()})
    print('\n'.join(lines))
    print('wrote', path, os.path.getsize(path), 'bytes; margin %.3g' % margin)


if __name__ == '__main__':
    main()
