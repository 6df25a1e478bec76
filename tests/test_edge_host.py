"""CPU: the edge mode's model loader, the two forms of the NumPy twin (tests/edge_ref.py) against each other, the golden and sklearn,
the properties that make rooms A and B fit as fixtures, and the ABI plumbing."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
from scipy.special import expit

from conftest import GOLDEN, REPO
import baselines_ref
import edge_ref as T

REF_PICKLE = '/root/reference/models/edge5.pkl'
OLD_MODULE = 'sklearn.neural_network.multilayer_perceptron'


@pytest.fixture(scope='module')
def weights():
    return T.golden_weights()


@pytest.fixture(scope='module')
def rooms():
    return [T.equalise(r) for r in T.raw_rooms()]


@pytest.fixture(scope='module')
def literal(rooms, weights):
    return [T.literal(r['points'], weights) for r in rooms]


@pytest.fixture(scope='module')
def staged(rooms, weights):
    return [T.staged(r['points'], weights) for r in rooms]


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'edge_ref_cpu.npz')) as z:
        return {k: z[k] for k in z.files}


def _same_arrays(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.skipif(not os.path.exists(REF_PICKLE), reason='the reference checkout with models/edge5.pkl is not on this machine')
def test_loader_reads_the_reference_pickle(weights):
    from learn_region_grow_amd import edge
    got = edge.load_edge_model(REF_PICKLE)
    assert [a.shape for a in got] == [(30, 100), (100,), (100, 50), (50,), (50, 25), (25,), (25, 1), (1,)]
    assert all(a.dtype == np.float64 for a in got)
    assert _same_arrays(got, weights)


def _fake_old_sklearn(monkeypatch):
    """An MLPClassifier class under sklearn 0.19's module name, so that a pickle names it as the reference's does."""
    top, mid, leaf = types.ModuleType('sklearn'), types.ModuleType('sklearn.neural_network'), types.ModuleType(OLD_MODULE)
    cls = type('MLPClassifier', (object,), {'__module__': OLD_MODULE})
    leaf.MLPClassifier = cls
    top.neural_network, mid.multilayer_perceptron = mid, leaf
    for m in (top, mid, leaf):
        monkeypatch.setitem(sys.modules, m.__name__, m)
    return cls


def _write_old_pickle(monkeypatch, path, arrays, activation='relu', out_activation='logistic'):
    import joblib
    m = _fake_old_sklearn(monkeypatch)()
    m.coefs_, m.intercepts_ = list(arrays[0::2]), list(arrays[1::2])
    m.activation, m.out_activation_, m.n_layers_, m.n_outputs_ = activation, out_activation, len(arrays) // 2 + 1, 1
    joblib.dump(m, str(path), protocol=2)
    monkeypatch.undo()
    assert open(str(path), 'rb').read(2) == b'\x80\x02' and OLD_MODULE.encode() in open(str(path), 'rb').read()


def test_loader_reads_an_old_style_pickle_without_sklearn(monkeypatch, tmp_path, weights):
    from learn_region_grow_amd import edge
    path = tmp_path / 'edge9.pkl'
    _write_old_pickle(monkeypatch, path, weights)
    assert _same_arrays(edge.load_edge_model(path), weights)
    np.savez(str(tmp_path / 'w.npz'), **dict(zip(edge.WEIGHT_KEYS, weights)))
    assert _same_arrays(edge.load_edge_model(tmp_path / 'w.npz'), weights)
    assert len(edge.pack_weights(weights)) == 9451
    # in a fresh interpreter: no sklearn module is imported by the loader
    code = ('import sys; sys.path.insert(0, %r)\nfrom learn_region_grow_amd import edge\nw = edge.load_edge_model(%r)\n'
            'assert w[0].shape == (30, 100)\nassert not [m for m in sys.modules if m.split(".")[0] == "sklearn"], "sklearn was imported"\n'
            % (REPO, str(path)))
    subprocess.check_call([sys.executable, '-c', code])


def test_loader_refuses_other_networks(monkeypatch, tmp_path, weights):
    from learn_region_grow_amd import edge
    rs = np.random.RandomState(0)
    three = [rs.randn(30, 20), rs.randn(20), rs.randn(20, 5), rs.randn(5), rs.randn(5, 1), rs.randn(1)]
    _write_old_pickle(monkeypatch, tmp_path / 'three.pkl', three)
    with pytest.raises(ValueError, match='four-layer'):
        edge.load_edge_model(tmp_path / 'three.pkl')
    wide = [a.copy() for a in weights]
    wide[0] = rs.randn(31, 100)
    _write_old_pickle(monkeypatch, tmp_path / 'wide.pkl', wide)
    with pytest.raises(ValueError, match='30-100-50-25-1'):
        edge.load_edge_model(tmp_path / 'wide.pkl')
    _write_old_pickle(monkeypatch, tmp_path / 'tanh.pkl', weights, activation='tanh')
    with pytest.raises(ValueError, match="'relu'"):
        edge.load_edge_model(tmp_path / 'tanh.pkl')
    _write_old_pickle(monkeypatch, tmp_path / 'softmax.pkl', weights, out_activation='softmax')
    with pytest.raises(ValueError, match="'logistic'"):
        edge.load_edge_model(tmp_path / 'softmax.pkl')
    import joblib
    joblib.dump(dict(a=1), str(tmp_path / 'dict.pkl'), protocol=2)
    with pytest.raises(ValueError, match='perceptron'):
        edge.load_edge_model(tmp_path / 'dict.pkl')
    np.savez(str(tmp_path / 'few.npz'), W0=weights[0])
    with pytest.raises(ValueError, match='lacks'):
        edge.load_edge_model(tmp_path / 'few.npz')


def test_rooms_are_the_golden_ones(golden):
    assert baselines_ref.rooms_digest(T.raw_rooms()) == str(golden['rooms_digest'])


def test_staged_twin_equals_literal_twin(rooms, literal, staged):
    for r, (lit, st) in enumerate(zip(literal, staged)):
        assert np.array_equal(lit['labels'], st['labels']) and lit['n_clusters'] == st['n_clusters'], r
        # the slot layout holds every directed edge's probability once
        E = lit['E']
        nb = st['nb']
        o = np.array([np.nonzero(nb[a] == b)[0][0] for a, b in E])
        assert np.array_equal(T.edge_probs(st['p'], nb)[E[:, 0], o], lit['probs']), r


def test_literal_twin_equals_golden(literal, staged, golden):
    for lit, st, name in zip(literal, staged, 'AB'):
        assert np.array_equal(lit['labels'], golden['labels_' + name]) and lit['n_clusters'] == golden['n_clusters_' + name]
        assert T.digest(st['z']) == str(golden['z_digest_' + name])


def test_host_search_of_the_package_equals_the_twin(rooms, staged):
    """edge.search / edge.resolve finish overflowed searches on the host: the same stops and labels as the twin's."""
    from learn_region_grow_amd import edge
    st = staged[0]
    todo = np.nonzero(st['stop'] >= 0)[0]
    for i in todo[:: max(1, len(todo) // 200)]:
        assert edge.search(int(i), st['nb'], st['p'], st['cluster_labels'])[0] == st['stop'][i]
    assert np.array_equal(edge.resolve(st['cluster_labels'], st['stop']), st['labels'])
    assert np.array_equal(edge._voxel_neighbours(rooms[0]['points'][:400], 0.1), baselines_ref.neighbours(rooms[0]['points'][:400], 0.1))


def test_chain_means_sklearns_function(rooms, literal, weights):
    """The twin's probabilities against sklearn 1.7's MLPClassifier with the arrays injected: within 1e-12 relative, same labels."""
    from sklearn.neural_network import MLPClassifier
    from sklearn.preprocessing import LabelBinarizer
    m = MLPClassifier(hidden_layer_sizes=(100, 50, 25), activation='relu')
    m.coefs_, m.intercepts_ = list(weights[0::2]), list(weights[1::2])
    m.n_layers_, m.n_outputs_, m.out_activation_, m.n_features_in_ = 5, 1, 'logistic', 30
    m.classes_ = np.array([0, 1])
    m._label_binarizer = LabelBinarizer().fit([0, 1])
    for r, (room, lit) in enumerate(zip(rooms, literal)):
        seen = {}

        def probs(F):
            seen['p'] = m.predict_proba(F)[:, 1]
            return seen['p']
        sk = T.literal(room['points'], weights, probs_fn=probs)
        rel = np.abs(seen['p'] - lit['probs']) / lit['probs']
        print('room %d: largest relative distance of the chain from sklearn %.3g' % (r, rel.max()))
        assert rel.max() <= 1e-12
        assert np.array_equal(sk['labels'], lit['labels']), r


def test_rooms_fit_as_fixtures(literal, staged):
    a, b = staged
    assert a['n_clusters'] > 0 and b['n_clusters'] > 0
    unl = a['cluster_labels'] == 0
    assert unl.sum() > 1000 and a['labels'].all() and (a['stop'][unl] >= 0).all()
    assert a['largest_visited'] > 64
    dead = (b['cluster_labels'] == 0) & ~b['live']
    assert dead.sum() > 1000 and not b['labels'][dead].any() and (b['stop'] >= 0).sum() > 100
    pe = np.where(a['nb'] >= 0, T.edge_probs(a['p'], a['nb']), -1.0)
    ties = sum(len(row[row >= 0]) - len(np.unique(row[row >= 0])) for row in pe)
    assert ties > 100
    for st in staged:
        ii, ss = np.nonzero(st['nb'][:, 13:] >= 0)
        p = st['p'][ii, ss]
        kk = st['nb'][ii, 13 + ss]
        gap = np.minimum(np.minimum(np.abs(p - 0.99 * st['pmax'][ii]), np.abs(p - 0.99 * st['pmax'][kk])), np.abs(p - 0.9))
        print('smallest distance of a probability from a threshold: %.3g' % gap.min())
        assert gap.min() > 1e-9


def test_abi_plumbing(hip_lib):
    from learn_region_grow_amd import _lib, baselines
    for name in ('lrg_edge_workspace_bytes', 'lrg_edge_logits', 'lrg_edge_sigmoid', 'lrg_edge_segment', 'lrg_edge_status',
                 'lrg_baseline_segment_mask'):
        assert name in _lib.EXPORTS and hasattr(hip_lib, name)
    header = open(os.path.join(REPO, 'include', 'lrg_hip.h')).read()
    assert int(re.search(r'#define\s+LRG_ABI_VERSION\s+(\d+)', header).group(1)) == _lib.LRG_ABI_VERSION >= 19
    assert int(re.search(r'#define\s+LRG_EDGE_WEIGHTS\s+(\d+)', header).group(1)) == 9451
    assert 'lrg_edge.hip' in _lib.SOURCES
    assert baselines.ALL_MODES == baselines.MODES + ('fpfh',) and 'edge' not in baselines.ALL_MODES
    with pytest.raises(ValueError):
        baselines.default_thresholds('edge')
    # workspace arithmetic is host only: the logits prefix does not depend on min_cluster_size or search_cap
    assert hip_lib.lrg_edge_workspace_bytes(1000, 2, 10, 1024) > hip_lib.lrg_edge_workspace_bytes(1000, 2, 10, 8) > 0
    assert hip_lib.lrg_edge_workspace_bytes(1000, 2, 65, 1024) == 0
