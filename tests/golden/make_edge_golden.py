"""Writes tests/golden/edge5_weights.npz (the eight arrays of the reference's models/edge5.pkl) and tests/golden/edge_ref_cpu.npz (the
literal twin's labels on rooms A and B of tests/edge_ref.py).  CPU only.

    python tests/golden/make_edge_golden.py <path to models/edge5.pkl>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import baselines_ref  # noqa: E402
import edge_ref  # noqa: E402
from learn_region_grow_amd import edge  # noqa: E402


def main():
    weights = edge.load_edge_model(sys.argv[1])
    np.savez_compressed(os.path.join(HERE, 'edge5_weights.npz'), **dict(zip(edge.WEIGHT_KEYS, weights)))
    raw = edge_ref.raw_rooms()
    out = dict(rooms_digest=np.array(baselines_ref.rooms_digest(raw)))
    for name, r in zip('AB', raw):
        room = edge_ref.equalise(r)
        lit = edge_ref.literal(room['points'], weights)
        st = edge_ref.staged(room['points'], weights)
        assert np.array_equal(lit['labels'], st['labels'])
        out['labels_' + name] = lit['labels'].astype(np.int32)
        out['n_clusters_' + name] = np.int32(lit['n_clusters'])
        out['z_digest_' + name] = np.array(edge_ref.digest(st['z']))
        print(name, len(room['points']), 'points', len(lit['E']), 'directed edges', lit['n_clusters'], 'clusters', 'longest search', lit['pops'],
              'pops; largest visited set', st['largest_visited'], '; label 0 left:', int((lit['labels'] == 0).sum()))
    np.savez_compressed(os.path.join(HERE, 'edge_ref_cpu.npz'), **out)


if __name__ == '__main__':
    main()
