"""NumPy restatement of the reference's plain PointNet (train_pointnet.py:31-99) at inference, the checker of
learn_region_grow_amd.pointnet (a plain module the tests import; nothing here is used by the package).

  - ``variable_shapes``: the names and TF shapes from the text of train_pointnet.py:50-51, :66-71, :88-89, :96-97.
  - ``random_weights``: every tensor at its real shape, in ranges that make every tensor matter.
  - ``forward``: :49-99 with ``is_training_pl: False`` (benchmarks.py:296) in ``dtype`` (float64: the exact value the tests measure
    against; float32: NumPy / BLAS float32, whose distance from float64 sets the tests' bound).  ``mutate`` plants one fault (the
    tests confirm that the bound catches each).
  - ``classify``: benchmarks.py:282-298 with the cells of tests/pointnet2_ref.py.
"""
import numpy as np

import pointnet2_ref

F32 = np.float32
NUM_POINT = 1024
BN_EPSILON = 1e-3
SHIPPED = ((64, 64, 128, 512), (512,))                    # models/pointnet_model5.ckpt.index
CURRENT = ((64, 64, 64, 128, 1024), (512, 256))           # NUM_FEATURE_CHANNELS, NUM_FC_CHANNELS of train_pointnet.py:20-22
MEAN = 'moments/Squeeze/ExponentialMovingAverage'
VARIANCE = 'moments/Squeeze_1/ExponentialMovingAverage'


def bn_names(j):
    """(beta, gamma, moving mean, moving variance) of the batch norm after hidden fc layer j.  Block 0: the shipped index.  Block 1:
    inferred from TF 1's scoping (the name scope of the re-entered variable_scope('bn') is 'bn_1', its variable scope still 'bn')."""
    scope = 'bn' if j == 0 else 'bn_%d' % j
    return '%s/beta' % scope, '%s/gamma' % scope, 'bn/%s/%s' % (scope, MEAN), 'bn/%s/%s' % (scope, VARIANCE)


def variable_shapes(conv, fc, num_class):
    """name -> TF shape.  conv: NUM_FEATURE_CHANNELS; fc: NUM_FC_CHANNELS (the hidden layers)."""
    shapes = {}
    for i in range(len(conv)):
        shapes['kernel%d' % i] = (1, 6 if i == 0 else 1, 1 if i == 0 else conv[i - 1], conv[i])          # :50
        shapes['bias%d' % i] = (conv[i],)
    width = conv[-1] + conv[1]                                        # self.concat: tile[0] (conv[-1] wide) and tile[1] = conv[1]
    for i in range(len(fc)):
        shapes['fc_weights%d' % i] = (1, width, fc[i])
        shapes['fc_bias%d' % i] = (fc[i],)
        beta, gamma, mean, variance = bn_names(i)
        shapes[beta] = shapes[gamma] = (fc[i],)
        shapes[mean] = shapes[variance] = (NUM_POINT, fc[i])          # moments over axis 0 of [batch, num_point, c]
        width = fc[i]
    shapes['fc_weights%d' % len(fc)] = (1, width, num_class)
    shapes['fc_bias%d' % len(fc)] = (num_class,)
    return shapes


def random_weights(seed, conv=SHIPPED[0], fc=SHIPPED[1], num_class=13):
    """Kernels from the reference's initialiser (VarianceScaling(1.0, fan_avg, uniform): uniform in +-sqrt(6 / (fan_in + fan_out)),
    fan_in = the receptive field times the input channels); biases, beta and the moving mean of magnitude 0.1 .. 0.2 with a random
    sign; gamma in 0.5 .. 1.5; the moving variance in 0.01 .. 0.5 (so rsqrt(variance + 1e-3) spans 1.4 .. 9.5)."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shp in variable_shapes(conv, fc, num_class).items():
        if name.startswith('kernel') or name.startswith('fc_weights'):
            fan_in, fan_out = int(np.prod(shp[:-1])), int(np.prod(shp[:-2])) * shp[-1]
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            out[name] = rng.uniform(-lim, lim, shp).astype(F32)
        elif name.endswith('gamma'):
            out[name] = rng.uniform(0.5, 1.5, shp).astype(F32)
        elif name.endswith(VARIANCE):
            out[name] = rng.uniform(0.01, 0.5, shp).astype(F32)
        else:
            out[name] = (rng.uniform(0.1, 0.2, shp) * rng.choice([-1.0, 1.0], shp)).astype(F32)
    return out


def widths_of(weights):
    """(conv, fc, num_class) of a weight dict."""
    conv = []
    while 'kernel%d' % len(conv) in weights:
        conv.append(weights['kernel%d' % len(conv)].shape[-1])
    fc = []
    while 'fc_weights%d' % len(fc) in weights:
        fc.append(weights['fc_weights%d' % len(fc)].shape[-1])
    return tuple(conv), tuple(fc[:-1]), fc[-1]


def batch_norm(x, beta, gamma, mean, variance, dtype):
    """tf.nn.batch_normalization(x, mean, variance, beta, gamma, 1e-3): inv = rsqrt(variance + eps) * gamma;
    x * inv + (beta - mean * inv).  mean, variance [1024, c] broadcast over the batch axis of x [B, 1024, c]."""
    inv = (dtype(1) / np.sqrt(variance.astype(dtype) + dtype(BN_EPSILON))) * gamma.astype(dtype)
    return x * inv + (beta.astype(dtype) - mean.astype(dtype) * inv)


def features(batch, weights, dtype=np.float64):
    """:49-54: batch [B, 1024, 6] float32 -> [conv[0], ..., conv[-1]], each [B, 1024, c] in dtype."""
    dtype = np.dtype(dtype).type
    x = np.asarray(batch, F32).astype(dtype)
    conv = []
    for i in range(len(widths_of(weights)[0])):
        k = weights['kernel%d' % i]
        x = np.maximum(x @ k.reshape(-1, k.shape[-1]).astype(dtype) + weights['bias%d' % i].astype(dtype), dtype(0))
        conv.append(x)
    return conv


def head(last, skip, pooled, weights, dtype=np.float64, mutate=None):
    """:57-99: last [B, 1024, c], skip [B, 1024, c1], pooled [B, c] -> (logits [B, 1024, num_class], [hidden fc layers]) in dtype.
    The subtraction is done in the inputs' own type when that is float32 (as :59 does), then widened."""
    dtype = np.dtype(dtype).type
    fc_w = widths_of(weights)[1]
    diff = last if mutate == 'no_subtract' else last - pooled[:, None, :]
    x = np.concatenate([diff.astype(dtype), np.asarray(skip).astype(dtype)], axis=2)
    fc = []
    for j in range(len(fc_w)):
        x = x @ weights['fc_weights%d' % j][0].astype(dtype) + weights['fc_bias%d' % j].astype(dtype)
        beta, gamma, mean, variance = (weights[n] for n in bn_names(j))
        if mutate == 'bn_shift_rows':
            mean, variance = np.roll(mean, 1, axis=0), np.roll(variance, 1, axis=0)
        x = batch_norm(x, beta, gamma, mean, variance, dtype)
        if not (mutate == 'skip_last_relu' and j == len(fc_w) - 1):
            x = np.maximum(x, dtype(0))
        fc.append(x)
    j = len(fc_w)
    return x @ weights['fc_weights%d' % j][0].astype(dtype) + weights['fc_bias%d' % j].astype(dtype), fc


def forward(batch, weights, dtype=np.float64, mutate=None):
    """batch [B, 1024, 6] float32 -> (logits [B, 1024, num_class] in dtype, dict(conv=[...], skip, pooled, fc=[hidden layers])).

    mutate (one fault at a time): 'skip_conv0' (the skip taken from conv[0] -- which must then be as wide as conv[1]),
    'no_subtract' (the pooled row not subtracted), 'bn_shift_rows' (the batch-norm tables rolled by one row position),
    'skip_last_relu' (the ReLU after the last hidden fc layer left off), 'pool_992' (the maximum over the first 992 rows only)."""
    conv = features(batch, weights, dtype)
    pooled = conv[-1][:, :992].max(axis=1) if mutate == 'pool_992' else conv[-1].max(axis=1)
    logits, fc = head(conv[-1], conv[0] if mutate == 'skip_conv0' else conv[1], pooled, weights, dtype, mutate)
    return logits, dict(conv=conv, skip=conv[1], pooled=conv[-1].max(axis=1), fc=fc)


def classify(points, weights, grid_resolution, dtype=np.float64):
    """class_labels of one room (benchmarks.py:282-298) and the top-two logit gap of every point."""
    points = np.asarray(points, F32)
    cls = np.zeros(len(points), np.int64)
    gap = np.zeros(len(points))
    members = pointnet2_ref.cells(points, grid_resolution)
    inputs = pointnet2_ref.cell_inputs(points, grid_resolution)
    keys = sorted(members)
    logits, _ = forward(np.stack([inputs[k] for k in keys]), weights, dtype)
    for c, k in enumerate(keys):
        idx = members[k]
        lg = logits[c, :len(idx)]
        cls[idx] = lg.argmax(axis=1)
        top = np.sort(lg, axis=1)
        gap[idx] = top[:, -1] - top[:, -2]
    return cls, gap
