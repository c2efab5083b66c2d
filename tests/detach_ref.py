"""NumPy restatement of the packed layout of ``mg_unpad_rows`` / ``ops.unpad_rows`` (include/morgana_hip.h): block offsets and item
offsets from the lengths, and the expected bytes.  The GPU tests of tests/test_gpu_detach.py compare against it.  Also the small
inputs that tests/golden/make_golden_detach.py and tests/test_detach_host.py both build (the golden file holds what the reference
made of them)."""
import numpy as np

ALIGN = 64


def clamp_lens(lens, t):
    """len_b = min(max(seq_len[b], 0), T)."""
    return np.clip(np.asarray(lens, dtype=np.int64), 0, int(t))


def item_starts(lens, t, row_bytes):
    """Byte offset of every item inside its feature's block, and the block's size: row_bytes * sum_{b' < b} len_b'."""
    ends = np.cumsum(clamp_lens(lens, t)) * int(row_bytes)
    return np.concatenate((np.zeros(1, np.int64), ends[:-1])), int(ends[-1]) if len(ends) else 0


def block_layout(shapes, lens, guard=0):
    """[(offset, rows)] per (T, row_bytes) and the buffer size: blocks exactly as large as their rows, ``guard`` bytes behind each,
    starts rounded up to ``ALIGN``."""
    blocks, size = [], 0
    for t, row_bytes in shapes:
        rows = int(clamp_lens(lens, t).sum())
        size = (size + ALIGN - 1) // ALIGN * ALIGN
        blocks.append((size, rows))
        size += rows * int(row_bytes) + guard
    return blocks, size


def row_bytes(a):
    return int(np.prod(a.shape[2:], dtype=np.int64)) * a.dtype.itemsize


def packed_stream(a, lens):
    """uint8 array: the valid frames of a (B, T, ...) array, item after item."""
    a = np.ascontiguousarray(a)
    n = clamp_lens(lens, a.shape[1])
    parts = [a[b, :n[b]].reshape(-1).view(np.uint8) for b in range(a.shape[0])]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def pack(arrays, lens, fill=0xA5, guard=0):
    """The whole expected buffer for ``arrays`` (bytes outside the blocks = ``fill``) and its blocks."""
    blocks, size = block_layout([(a.shape[1], row_bytes(a)) for a in arrays], lens, guard)
    buf = np.full(size, fill, np.uint8)
    for a, (off, rows) in zip(arrays, blocks):
        stream = packed_stream(a, lens)
        assert stream.size == rows * row_bytes(a)
        buf[off:off + stream.size] = stream
    return buf, blocks


# ------------------------------------------------------------------------------------------------- shared small inputs (golden g19)
SEQ_LEN = np.array([7, 4, 1, 0], dtype=np.int64)
B, T = 4, 7

# case name -> (feature names, seq_len kind: 'tensor' | 'numpy' | 'none', squeeze)
DETACH_CASES = {
    'single_sq': (['f32_3'], 'tensor', True),
    'single_w1_sq': (['f32_1'], 'tensor', True),
    'single_w1_nosq': (['f32_1'], 'tensor', False),
    'multi_sq': (['f32_1', 'bool_5', 'i64_3', 'f32_5', 'i64_1', 'bool_1'], 'tensor', True),
    'multi_nosq': (['f32_1', 'bool_5', 'i64_3', 'f32_5', 'i64_1', 'bool_1'], 'tensor', False),
    'whole': (['vec', 'mat', 'f32_3'], 'tensor', True),
    'none_len': (['f32_3', 'mat'], 'none', True),
    'numpy_len': (['f32_5', 'i64_1'], 'numpy', True),
}
SELECT_CASES = ['f32_3', 'f32_1', 'i64_3', 'bool_5']
VOICED_CASES = {'one': ['va'], 'two': ['va', 'vb']}
VOICED_DTYPES = ['uint8', 'bool', 'float32']
CHECKPOINT_PATHS = ['exp/checkpoints/epoch_12.pt', 'exp/checkpoints/epoch_7_ema.pt', '/a/b/checkpoints/epoch_003_best.ckpt', 'exp/epoch_3.pt']


def detach_inputs():
    rng = np.random.RandomState(20261018)
    x = {}
    for w in (1, 3, 5):
        x['f32_%d' % w] = rng.standard_normal((B, T, w)).astype(np.float32)
        x['i64_%d' % w] = rng.randint(-5, 50, size=(B, T, w)).astype(np.int64)
        x['bool_%d' % w] = rng.random_sample((B, T, w)) > 0.5
    x['vec'] = rng.standard_normal((B,)).astype(np.float32)
    x['mat'] = rng.standard_normal((B, 3)).astype(np.float32)
    va = rng.standard_normal((B, T, 1)).astype(np.float32)
    vb = rng.standard_normal((B, T, 1)).astype(np.float32)
    va[0, 0], va[0, 1], va[0, 2], va[1, 3] = 0.0, -0.0, np.nan, 0.0
    vb[0, 1], vb[0, 2], vb[0, 3], vb[2, 0], vb[1, 3] = 1.0, 2.0, -0.0, np.nan, 0.0
    x['va'], x['vb'] = va, vb
    return x


def nested_input():
    return {'a': np.arange(3, dtype=np.int64), 'b': [1, (2.5, 3)], 'c': 'ab', 'd': {'e': np.ones((2, 2), np.float32), 'f': ()}}


def double(value):
    return value * 2


LISTIFY_INPUTS = [3, [1, 2], (1, 2), 'ab', None, []]


def encode(obj):
    """A nested result as JSON-able data that keeps the container types apart."""
    if isinstance(obj, np.ndarray):
        return {'ndarray': obj.tolist(), 'dtype': str(obj.dtype)}
    if isinstance(obj, dict):
        return {'dict': {k: encode(v) for k, v in obj.items()}}
    if isinstance(obj, (list, tuple)):
        return {type(obj).__name__: [encode(v) for v in obj]}
    return {type(obj).__name__: obj}


# ------------------------------------------------------------------------------------------------- comparisons with the golden file
def same(got, want):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == 'f')


def check_detach_result(g19, case, names, got):
    """Structure, shapes, dtypes and values of one ``detach_batched_seqs`` result against the golden case (shared with the GPU test)."""
    if int(g19['detach__%s__unwrapped' % case]):
        got = [got]
    else:
        assert isinstance(got, list)
    assert len(got) == len(names)
    for k, value in enumerate(got):
        whole = g19.get('detach__%s__%d__whole' % (case, k))
        if whole is not None:
            assert isinstance(value, np.ndarray)
            same(value, whole)
            continue
        assert isinstance(value, list) and len(value) == B
        for b, item in enumerate(value):
            assert isinstance(item, np.ndarray)
            same(item, g19['detach__%s__%d__%d' % (case, k, b)])
