"""Records tests/golden/preprocess_single_room.json: for the six rooms of tests/prep_fixtures.py, every feature size and every
eig_mode, the sha256 of each array lrg_preprocess (and lrg_preprocess_unsafe_normals) writes, the rooms' equalised counts, and the
compiler that built the library (the bits depend on it).  tests/test_gpu_preprocess_batch.py recomputes them.

    python tools/prep_golden_digests.py [--out tests/golden/preprocess_single_room.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'preprocess_single_room.json'))
    args = ap.parse_args()
    import torch
    import prep_fixtures as P
    from learn_region_grow_amd import _lib
    lib, dev = _lib.load(), torch.device('cuda:0')
    rooms = P.six_rooms()
    out = dict(hipcc_version=P.hipcc_version(),
               raw_points=[len(r[0]) for r in rooms], n_equalized=None, digests={})
    for F in P.DIGEST_F:
        for mode in P.DIGEST_MODES:
            got = [P.capi_single(lib, dev, room, F, mode) for room in rooms]
            n = [len(g['eq']) for g in got]
            assert out['n_equalized'] in (None, n)
            out['n_equalized'] = n
            for k, g in enumerate(got):
                out['digests'][P.digest_key(F, mode, k)] = P.digests(g, mode)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out, out['n_equalized'])


if __name__ == '__main__':
    main()
