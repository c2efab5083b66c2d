"""Tensor-level wrappers over the C ABI: validate, allocate outputs (torch is the allocator), launch on torch's current
HIP stream.  No arithmetic happens here and nothing falls back to torch ops: a missing library or a CPU tensor raises.
"""
import ctypes
import math
import numbers

import os

import torch

from . import _lib

# the header's MG_ACT_* / MG_NORM_* (include/morgana_hip.h through _lib), under the names the host layer uses
ACT_NONE, ACT_SIGMOID, ACT_TANH, ACT_RELU = _lib.MG_ACT_NONE, _lib.MG_ACT_SIGMOID, _lib.MG_ACT_TANH, _lib.MG_ACT_RELU
NORM_MVN, DENORM_MVN, NORM_MINMAX, DENORM_MINMAX = _lib.MG_NORM_MVN, _lib.MG_DENORM_MVN, _lib.MG_NORM_MINMAX, _lib.MG_DENORM_MINMAX

_workspaces = {}
SIDE_STREAM_IDS = set()      # raw handles of the side streams functional._Beside launches on (their scratch is their own)
_retired = []


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    # the current stream's raw handle (torch.cuda.current_stream().cuda_stream builds a Stream object first: 9 us a call, five calls
    # per eager F0Model step)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))


def _require(t, dtype, name, contiguous=True, rows=False):
    """The tensor check of every wrapper: ``t`` is a device tensor of ``dtype``.  Returns it contiguous (a copy if need be);
    ``contiguous=False`` returns it as it is, for the entry points that take strides.

    ``rows=True``: a (B, T, C) tensor -> (tensor, row stride) such that frame (b, t) starts at data_ptr + (b T + t) * stride elements:
    the tensor itself when its last dimension is contiguous and its frames are evenly spaced (a column slice of a contiguous
    (B, T, D) tensor), else a contiguous copy."""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor, got %s' % (name, type(t)))
    if not t.is_cuda:
        raise _lib.MorganaHipError('%s is on %s: the morgana_amd ops run only on an MI355X device (no CPU fallback)'
                                   % (name, t.device))
    if t.dtype != dtype:
        raise TypeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    if rows:
        if t.dim() != 3:
            raise ValueError('%s must be (B, T, C), got %s' % (name, tuple(t.shape)))
        b, n, c = t.shape
        ld = t.stride(1)
        if (t.stride(2) == 1 or c == 1) and ld >= c and (b == 1 or t.stride(0) == n * ld) and ld < 2 ** 31:
            return t, ld
        return t.contiguous(), c
    return t if not contiguous or t.is_contiguous() else t.contiguous()


def _aligned16(t):
    """``t`` (contiguous) with a 16-byte aligned base: itself, or a copy when it is a view that starts inside its storage - as
    ``_require`` copies a non-contiguous one.  For the kernels that read 16 bytes per lane and refuse any other base."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _lengths(seq_len, b, what='', flat=True):
    """``seq_len`` of a (B, ...) batch: None, or int64 on the device with one length per item - the kernels read B of them.
    ``flat``: it must be (B,); otherwise any shape of B elements will do (the models pass (B, 1))."""
    if seq_len is None:
        return None
    seq_len = _require(seq_len, torch.int64, 'seq_len')
    if flat and tuple(seq_len.shape) != (b,):
        raise ValueError('%sseq_len must be (B,) = (%d,), got %s' % (what, b, tuple(seq_len.shape)))
    if seq_len.numel() != b:
        raise ValueError('%sseq_len must hold B = %d lengths, got %s' % (what, b, tuple(seq_len.shape)))
    return seq_len


def _one_element(grad_loss):
    """The upstream gradient of a scalar loss: a one-element float32 device tensor that the kernel reads (no host read)."""
    grad_loss = _require(grad_loss, torch.float32, 'grad_loss')
    if grad_loss.numel() != 1:
        raise ValueError('grad_loss must hold one element, got %s' % (tuple(grad_loss.shape),))
    return grad_loss


def _loss_and_grad_out(what, pred, width, col0, want_grad, grad_out, loss_out):
    """Where a column-slice loss (``masked_ce``, ``masked_mdn``) leaves its results -> (loss, grad returned, grad written, ldg, gcol0).
    ``grad_out``: a buffer shaped like ``pred`` whose columns [col0, col0 + width) take the gradient; else a new (B, T, width)."""
    loss = torch.empty((), dtype=torch.float32, device=pred.device) if loss_out is None else loss_out
    if not want_grad:
        return loss, None, None, 0, 0
    if grad_out is None:
        grad = torch.empty((pred.shape[0], pred.shape[1], width), dtype=torch.float32, device=pred.device)
        return loss, grad, grad, width, 0
    g, ldg = _require(grad_out, torch.float32, 'grad_out', rows=True)
    if g is not grad_out or tuple(g.shape) != tuple(pred.shape):
        raise ValueError('%s: grad_out must be a (B, T, D) tensor with evenly spaced rows, shaped like predictions' % what)
    return loss, grad_out, g, ldg, col0


def workspace(nbytes, device):
    """One grow-only scratch buffer per device; all kernels of a step run on one stream, so it is shared.  A buffer that is
    outgrown is kept alive (``_retired``): a captured HIP graph (morgana_amd/graphs.py) may still launch kernels that point at it."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    # ... and one more for launches that run BESIDE the step on a side stream (functional._Beside): they must not share scratch with it
    key = (index, bool(SIDE_STREAM_IDS) and device.type == 'cuda' and torch._C._cuda_getCurrentRawStream(index) in SIDE_STREAM_IDS)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _retired.append(buf)
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


_tail_slab_bufs = {}


def _tail_slabs(nbytes, device):
    """Grow-only buffer per device for the fused tail's slabs when their sum is deferred (f0_l2tail_rows_expand(defer=True)); an
    outgrown one is retired, not dropped (captured graphs keep its address)."""
    key = (device.index if device.index is not None else torch.cuda.current_device())
    buf = _tail_slab_bufs.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _retired.append(buf)
        buf = torch.empty(max(int(nbytes), 1 << 16), dtype=torch.uint8, device=device)
        _tail_slab_bufs[key] = buf
    return buf


def _slab_buffer(slab, nbytes, device):
    """A per-layer slab buffer of at least ``nbytes``: ``slab`` itself when it is large enough, else a new one - and the outgrown
    buffer is RETIRED, not dropped (as `workspace` does): a HIP graph captured at the smaller shape still launches the weight-gradient
    and update kernels with its address baked in, and torch's caching allocator would hand that memory to the next tensor."""
    if slab is not None and slab.numel() >= nbytes:
        return slab
    if slab is not None:
        _retired.append(slab)
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def pad_ld(n):
    """Leading dimension of a bf16 buffer with n columns: a multiple of 64 (the large-tile kernels' K step) once the
    row is at least 64 wide, a multiple of 8 (one 16-byte chunk) below that.  Padding columns hold zeros."""
    return (n + 63) // 64 * 64 if n >= 64 else (n + 7) // 8 * 8


pad8 = pad_ld


# ----------------------------------------------------------------------------------------------------------------- K1
MAX_PHONES = 12288      # csrc/upsample.hip MG_MAX_PHONES: the scan of one utterance's durations lives in LDS (4 bytes a phone + 1 KB)


def _phones(p, what):
    """The library refuses more than MAX_PHONES phones (segments) per utterance; said here, before the call, with the same limit."""
    if not 0 < p <= MAX_PHONES:
        raise ValueError('%s: %d phones per utterance, the kernels take 1..%d' % (what, p, MAX_PHONES))


def upsample_lengths(dur):
    """dur int64 (B, P) -> (n_frames int64 (B,), tmax int64 0-d), both on device (no sync)."""
    lib = _lib.load()
    dur = _require(dur, torch.int64, 'dur')
    b, p = dur.shape
    n_frames = torch.empty((b,), dtype=torch.int64, device=dur.device)
    tmax = torch.empty((), dtype=torch.int64, device=dur.device)
    _lib.check(lib.mg_upsample_lengths(_p(dur), b, p, _p(n_frames), _p(tmax), _stream()), 'mg_upsample_lengths')
    return n_frames, tmax


def upsample_index(dur, t_cap, want_idx64=False, want_rows=True):
    lib = _lib.load()
    dur = _require(dur, torch.int64, 'dur')
    b, p = dur.shape
    _phones(p, 'upsample_index')
    idx64 = torch.empty((b, t_cap), dtype=torch.int64, device=dur.device) if want_idx64 else None
    rows = torch.empty((b, t_cap), dtype=torch.int32, device=dur.device) if want_rows else None
    _lib.check(lib.mg_upsample_index(_p(dur), b, p, int(t_cap), _p(idx64), _p(rows), _stream()), 'mg_upsample_index')
    return idx64, rows


def upsample_index_maps(dur, t_cap):
    """(rows (B, T) int32 with -1 padding, rows_mapped (-1 -> B*P), seg (2, B*P) frame runs) in one launch (mg_upsample_index_maps)."""
    lib = _lib.load()
    dur = _require(dur, torch.int64, 'dur')
    b, p = dur.shape
    _phones(p, 'upsample_index_maps')
    rows = torch.empty((2, b, t_cap), dtype=torch.int32, device=dur.device)
    seg = torch.empty((2, b * p), dtype=torch.int32, device=dur.device)
    _lib.check(lib.mg_upsample_index_maps(_p(dur), b, p, int(t_cap), _p(rows[0]), _p(rows[1]), b * p, _p(seg[0]), _p(seg[1]),
                                          _stream()), 'mg_upsample_index_maps')
    return rows[0], rows[1], seg


def gather_rows(src2d, rows, out_bf16=False, ld=None):
    lib = _lib.load()
    src2d = _require(src2d, torch.float32, 'src')
    rows = _require(rows, torch.int32, 'rows')
    m, f = rows.numel(), src2d.shape[1]
    if out_bf16:
        src2d = _aligned16(src2d)
        ldo = pad8(f) if ld is None else int(ld)
        out = torch.empty((m, ldo), dtype=torch.bfloat16, device=src2d.device)
        _lib.check(lib.mg_gather_rows_bf16(_p(src2d), _p(rows), _p(out), m, f, ldo, _stream()), 'mg_gather_rows_bf16')
    else:
        out = torch.empty((m, f), dtype=torch.float32, device=src2d.device)
        _lib.check(lib.mg_gather_rows_f32(_p(src2d), _p(rows), _p(out), m, f, _stream()), 'mg_gather_rows_f32')
    return out


def segment_index(seg_lens2d, t, max_len=None, want_split=True, want_ends=True):
    """Flat row maps of split_to_segments / get_segment_ends (mg_segment_index): (split int32 (B,S,L) or None, ends (B,S))."""
    lib = _lib.load()
    seg_lens2d = _require(seg_lens2d, torch.int64, 'segment_lens')
    b, s = seg_lens2d.shape
    _phones(s, 'segment_index')
    length = int(max_len) if want_split else 0
    split = torch.empty((b, s, length), dtype=torch.int32, device=seg_lens2d.device) if want_split else None
    ends = torch.empty((b, s), dtype=torch.int32, device=seg_lens2d.device) if want_ends else None
    _lib.check(lib.mg_segment_index(_p(seg_lens2d), b, s, int(t), length, _p(split), _p(ends), _stream()), 'mg_segment_index')
    return split, ends


def scatter_rows(src2d, rows, n_dst_rows):
    """Adjoint of gather_rows for distinct targets: zeros (n_dst_rows, F) with dst[rows[m]] = src2d[m]."""
    lib = _lib.load()
    src2d = _require(src2d, torch.float32, 'src')
    rows = _require(rows, torch.int32, 'rows')
    dst = torch.zeros((n_dst_rows, src2d.shape[1]), dtype=torch.float32, device=src2d.device)
    _lib.check(lib.mg_scatter_rows_f32(_p(src2d), _p(rows), _p(dst), rows.numel(), src2d.shape[1], _stream()),
               'mg_scatter_rows_f32')
    return dst


def frame_layout(seq_len, t, total):
    """Packed-frame maps of a ragged (B, t, .) batch (mg_frame_layout): (offsets (B+1,), rows (total+1,), inverse (B*t,)) int32.
    ``total`` = sum of min(seq_len, t), known on the host."""
    lib = _lib.load()
    seq_len = _require(seq_len, torch.int64, 'seq_len')
    b = seq_len.numel()
    offsets = torch.empty(b + 1, dtype=torch.int32, device=seq_len.device)
    rows = torch.empty(int(total) + 1, dtype=torch.int32, device=seq_len.device)
    inverse = torch.empty(b * int(t), dtype=torch.int32, device=seq_len.device)
    _lib.check(lib.mg_frame_layout(_p(seq_len), b, int(t), int(total), _p(offsets), _p(rows), _p(inverse), _stream()), 'mg_frame_layout')
    return offsets, rows, inverse


def pad_rows_colsum(g, seq_len, out):
    """out (D,) = sum of g[b, t, :] over the padded frames t >= seq_len[b] (mg_pad_rows_colsum_f32); g (B, T, D) f32."""
    lib = _lib.load()
    g = _require(g, torch.float32, 'gradient')
    if g.dim() != 3:
        raise ValueError('pad_rows_colsum: the gradient must be (B, T, D), got %s' % (tuple(g.shape),))
    b, t, d = g.shape
    seq_len = _lengths(seq_len, b, 'pad_rows_colsum: ', flat=False)
    if seq_len is None:
        raise ValueError('pad_rows_colsum: seq_len is required (without it no frame is padding)')
    # the result is written in place (a row of the caller's tensor): a copy made here would be lost
    if _require(out, torch.float32, 'out', contiguous=False).numel() != d or not out.is_contiguous() or out.device != g.device:
        raise ValueError('pad_rows_colsum: out must be %d contiguous float32 elements on %s, got %s' % (d, g.device, tuple(out.shape)))
    ws = torch.empty(lib.mg_pad_rows_colsum_workspace_bytes(b, t, d), dtype=torch.uint8, device=g.device)
    _lib.check(lib.mg_pad_rows_colsum_f32(_p(g), _p(seq_len), b, t, d, _p(out), _p(ws), ws.numel(), _stream()), 'mg_pad_rows_colsum_f32')
    return out


def gather_concat(src2d, rows, extra2d, out_bf16=False):
    """[src2d[rows] | extra2d] per frame (mg_gather_concat_*): f32 (M, F+C), or bf16 (M, pad_ld(F+C)) zero padded."""
    lib = _lib.load()
    src2d = _require(src2d, torch.float32, 'src')
    extra2d = _require(extra2d, torch.float32, 'extra')
    rows = _require(rows, torch.int32, 'rows')
    m, f, c = rows.numel(), src2d.shape[1], extra2d.shape[1]
    if extra2d.shape[0] != m:
        raise ValueError('gather_concat: %d frame rows but %d rows of frame-level features' % (m, extra2d.shape[0]))
    if out_bf16:
        src2d = _aligned16(src2d)
        ldo = pad_ld(f + c)
        out = torch.empty((m, ldo), dtype=torch.bfloat16, device=src2d.device)
        _lib.check(lib.mg_gather_concat_bf16(_p(src2d), _p(rows), _p(extra2d), _p(out), m, f, c, ldo, _stream()),
                   'mg_gather_concat_bf16')
    else:
        out = torch.empty((m, f + c), dtype=torch.float32, device=src2d.device)
        _lib.check(lib.mg_gather_concat_f32(_p(src2d), _p(rows), _p(extra2d), _p(out), m, f, c, f + c, _stream()),
                   'mg_gather_concat_f32')
    return out


def upsample_backward(grad_out, dur, n_phones):
    lib = _lib.load()
    grad_out = _require(grad_out, torch.float32, 'grad_out')
    dur = _require(dur, torch.int64, 'dur')
    b, t, f = grad_out.shape
    _phones(n_phones, 'upsample_backward')
    grad_src = torch.empty((b, n_phones, f), dtype=torch.float32, device=grad_out.device)
    _lib.check(lib.mg_upsample_backward_f32(_p(grad_out), _p(dur), _p(grad_src), b, n_phones, t, f, _stream()),
               'mg_upsample_backward_f32')
    return grad_src


# --------------------------------------------------------------------------------------------------- mask / K4 / K5
_MASK_TYPES = {torch.uint8: (1, 0), torch.bool: (1, 0), torch.int8: (1, 0), torch.float32: (4, 1), torch.int32: (4, 0),
               torch.int64: (8, 0), torch.float64: (8, 1)}


def sequence_mask(seq_len, max_len, dtype):
    lib = _lib.load()
    seq_len = _require(seq_len, torch.int64, 'seq_len')
    if dtype not in _MASK_TYPES:
        raise TypeError('sequence_mask: unsupported mask dtype %s' % dtype)
    elem, as_float = _MASK_TYPES[dtype]
    b = seq_len.shape[0]
    mask = torch.empty((b, max_len, 1), dtype=dtype, device=seq_len.device)
    if mask.numel() == 0:      # max_len = 0: nothing to write, and an empty tensor has no address to hand the library
        return mask
    _lib.check(lib.mg_sequence_mask(_p(seq_len), b, int(max_len), _p(mask), elem, as_float, _stream()),
               'mg_sequence_mask')
    return mask


def all_nonzero(tensors, dtype):
    """out = all_k (tensors[k] != 0) in ``dtype`` for up to ``_lib.MG_ALL_NONZERO_MAX`` float32 device tensors of one shape
    (mg_all_nonzero_f32): NaN counts as non-zero, -0.0 as zero."""
    lib = _lib.load()
    if not 1 <= len(tensors) <= _lib.MG_ALL_NONZERO_MAX:
        raise ValueError('all_nonzero: %d inputs, the kernel takes 1..%d' % (len(tensors), _lib.MG_ALL_NONZERO_MAX))
    if dtype not in _MASK_TYPES:
        raise TypeError('all_nonzero: unsupported mask dtype %s' % dtype)
    tensors = [_require(t, torch.float32, 'sequence_feature') for t in tensors]
    for t in tensors[1:]:
        if t.shape != tensors[0].shape:
            raise ValueError('all_nonzero: shapes %s and %s differ' % (tuple(tensors[0].shape), tuple(t.shape)))
    elem, as_float = _MASK_TYPES[dtype]
    out = torch.empty(tensors[0].shape, dtype=dtype, device=tensors[0].device)
    ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    _lib.check(lib.mg_all_nonzero_f32(ctypes.cast(ptrs, ctypes.c_void_p), len(tensors), tensors[0].numel(), _p(out), elem, as_float,
                                      _stream()), 'mg_all_nonzero_f32')
    return out


UNPAD_ALIGN = 64      # every feature's block of the packed buffer starts on a multiple of this many bytes


def row_bytes(t):
    """Bytes of one frame of a (B, T, ...) tensor: trailing elements x element size."""
    n = t.element_size()
    for k in t.shape[2:]:
        n *= int(k)
    return n


def unpad_layout(shapes_and_sizes, lens_host):
    """Blocks of the packed buffer of ``unpad_rows``: for every (T, row_bytes) the (offset, rows) of its block - rows =
    sum_b min(max(lens_host[b], 0), T), blocks exactly as large as their rows, starts on multiples of ``UNPAD_ALIGN`` - and the
    buffer's size.  Host arithmetic only."""
    blocks, size = [], 0
    for t, rb in shapes_and_sizes:
        rows = sum(min(max(int(n), 0), int(t)) for n in lens_host)
        size = (size + UNPAD_ALIGN - 1) // UNPAD_ALIGN * UNPAD_ALIGN
        blocks.append((size, rows))
        size += rows * int(rb)
    return blocks, size


def unpad_rows(tensors, seq_len, lens_host):
    """The valid frames of padded device features, utterance after utterance, as ONE byte buffer (mg_unpad_rows: one launch per
    ``_lib.MG_UNPAD_MAX`` features; beyond ``_lib.MG_UNPAD_MAX_ITEMS`` items one launch per feature and group of that many items).  tensors: contiguous device tensors (B, T_f, ...) of any dtype; seq_len: int64 (B,) on the same device
    - the kernel reads the lengths there; lens_host: the same lengths on the host, which size the blocks (a frame beyond a block is
    dropped, never written).  Returns (uint8 device buffer, [(byte offset, rows)] per feature)."""
    lib = _lib.load()
    seq_len = _require(seq_len, torch.int64, 'seq_len')
    b = seq_len.numel()
    if len(lens_host) != b:
        raise ValueError('unpad_rows: %d host lengths for %d items' % (len(lens_host), b))
    feats = []
    for k, t in enumerate(tensors):
        t = _require(t, getattr(t, 'dtype', None), 'sequence_feature %d' % k)      # any dtype: a device tensor, made contiguous
        if t.dim() < 2 or t.shape[0] != b or t.device != seq_len.device:
            raise ValueError('unpad_rows: feature %d is %s on %s, expected (%d, T, ...) on %s' % (k, tuple(t.shape), t.device, b, seq_len.device))
        if row_bytes(t) <= 0:
            raise ValueError('unpad_rows: feature %d of shape %s has empty frames' % (k, tuple(t.shape)))
        feats.append((t, int(t.shape[1]), row_bytes(t)))
    blocks, size = unpad_layout([(t_len, rb) for _, t_len, rb in feats], lens_host)
    buf = torch.empty(max(size, 1), dtype=torch.uint8, device=seq_len.device)
    if b > _lib.MG_UNPAD_MAX_ITEMS:
        _unpad_rows_in_item_groups(lib, feats, blocks, seq_len, lens_host, buf)
        return buf, blocks
    for first in range(0, len(feats), _lib.MG_UNPAD_MAX):
        chunk = feats[first:first + _lib.MG_UNPAD_MAX]
        descs = (_lib.mg_unpad_desc * len(chunk))()
        for i, (t, t_len, rb) in enumerate(chunk):
            offset, rows = blocks[first + i]
            descs[i].src, descs[i].T, descs[i].row_bytes = t.data_ptr(), t_len, rb
            descs[i].dst_offset, descs[i].block_bytes = offset, rows * rb
        _lib.check(lib.mg_unpad_rows(ctypes.cast(descs, ctypes.c_void_p), len(chunk), _p(seq_len), b, _p(buf), size, _stream()),
                   'mg_unpad_rows')
    return buf, blocks


def _unpad_rows_in_item_groups(lib, feats, blocks, seq_len, lens_host, buf):
    """``unpad_rows`` for more items than one launch scans (``_lib.MG_UNPAD_MAX_ITEMS``): per feature, one launch per group of that many
    items, each writing behind the rows of the groups before it.  A group's first byte is wherever those rows end, so the launch gets
    the destination pointer moved there and a block at offset 0 (the kernel aligns by address, only ``dst_offset`` must be a
    multiple of 16)."""
    b = seq_len.numel()
    desc = (_lib.mg_unpad_desc * 1)()
    for (t, t_len, rb), (offset, _) in zip(feats, blocks):
        done = 0                                                           # rows of the groups already packed
        for b0 in range(0, b, _lib.MG_UNPAD_MAX_ITEMS):
            b1 = min(b0 + _lib.MG_UNPAD_MAX_ITEMS, b)
            rows = sum(min(max(int(n), 0), t_len) for n in lens_host[b0:b1])
            desc[0].src, desc[0].T, desc[0].row_bytes = t.data_ptr() + b0 * t_len * rb, t_len, rb
            desc[0].dst_offset, desc[0].block_bytes = 0, rows * rb
            _lib.check(lib.mg_unpad_rows(ctypes.cast(desc, ctypes.c_void_p), 1, ctypes.c_void_p(seq_len.data_ptr() + 8 * b0), b1 - b0,
                                         ctypes.c_void_p(buf.data_ptr() + offset + done * rb), rows * rb, _stream()), 'mg_unpad_rows')
            done += rows


def masked_mse(pred, target, seq_len, want_grad, grad_scale=1.0, kind='mse'):
    """Returns (loss 0-d f32 tensor, grad or None).  kind: 'mse' or 'bce'."""
    lib = _lib.load()
    pred = _require(pred, torch.float32, 'predictions')
    target = _require(target, torch.float32, 'targets')
    if pred.shape != target.shape or pred.dim() != 3:
        raise ValueError('mse: predictions %s and targets %s must both be (B, T, D)' % (tuple(pred.shape),
                                                                                     tuple(target.shape)))
    b, t, d = pred.shape
    seq_len = _lengths(seq_len, b, '%s: ' % kind, flat=False)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    nbytes = lib.mg_masked_mse_workspace_bytes(b, t, d)
    ws = workspace(nbytes, pred.device)
    fn = lib.mg_masked_mse_f32 if kind == 'mse' else lib.mg_masked_bce_f32
    _lib.check(fn(_p(pred), _p(target), _p(seq_len), b, t, d, float(grad_scale), _p(loss), _p(grad), _p(ws), ws.numel(),
                  _stream()), 'mg_masked_%s_f32' % kind)
    return loss, grad


def masked_seq_mean(x, seq_len):
    """Masked sequence mean of a feature loss (mg_seq_mean_f32, csrc/seqmean.hip): x (B, T, D) float32, read in place through its
    strides (a column slice, a misaligned base, an expanded operand); seq_len (B,) int64 or None.  Returns the 0-d float32 loss
    ``mean_{b,d}( sum_{t} x[b,t,d] [t < n_b] / n_b )`` on the device, accumulated in float64 in a fixed order."""
    lib = _lib.load()
    x = _require(x, torch.float32, 'feature loss', contiguous=False)
    if x.dim() != 3 or 0 in x.shape:
        raise ValueError('feature loss must be a non-empty (B, T, D) tensor, got %s' % (tuple(x.shape),))
    b, t, d = x.shape
    seq_len = _lengths(seq_len, b)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws = workspace(lib.mg_seq_mean_workspace_bytes(b, t, d), x.device)
    _lib.check(lib.mg_seq_mean_f32(_p(x), x.stride(0), x.stride(1), x.stride(2), _p(seq_len), b, t, d, _p(loss), _p(ws), ws.numel(),
                                   _stream()), 'mg_seq_mean_f32')
    return loss


def masked_seq_mean_bwd(grad_loss, seq_len, shape):
    """d masked_seq_mean / d x for a feature loss of ``shape`` (B, T, D) (mg_seq_mean_bwd_f32): a dense float32 tensor, grad_loss / (n_b
    B D) on valid frames, 0 on pad frames, NaN on an utterance without a valid frame.  ``grad_loss``: the upstream gradient, a
    one-element float32 device tensor that the kernel reads (no host read)."""
    lib = _lib.load()
    grad_loss = _one_element(grad_loss)
    if len(shape) != 3 or min(shape) <= 0:
        raise ValueError('shape must be a non-empty (B, T, D), got %s' % (tuple(shape),))
    b, t, d = (int(v) for v in shape)
    seq_len = _lengths(seq_len, b)
    grad = torch.empty((b, t, d), dtype=torch.float32, device=grad_loss.device)
    _lib.check(lib.mg_seq_mean_bwd_f32(_p(grad_loss), _p(seq_len), b, t, d, _p(grad), _stream()), 'mg_seq_mean_bwd_f32')
    return grad


def _gv_operand(x, name):
    x = _require(x, torch.float32, name, contiguous=False)
    if x.dim() != 3 or 0 in x.shape:
        raise ValueError('%s must be a non-empty (B, T, D) tensor, got %s' % (name, tuple(x.shape)))
    if min(x.stride()) < 0:
        x = x.contiguous()
    return x


def gv(pred, target, seq_len=None, log=True, eps=1e-6, want_variances=False):
    """Global-variance loss (mg_gv_f32, csrc/gv.hip): pred and target (B, T, D) float32, both read in place through their strides;
    seq_len (B,) int64 or None.  Returns (loss 0-d float32, state (B, D, 2) float64 = (mean of pred, gradient coefficient) for
    ``gv_backward``, v_pred, v_target): the (B, D) float32 per-utterance variances when ``want_variances``, else None.
    ``target`` None: only the variances of ``pred`` are computed, (None, None, v_pred, None)."""
    lib = _lib.load()
    pred = _gv_operand(pred, 'predictions')
    b, t, d = pred.shape
    if target is not None:
        target = _gv_operand(target, 'targets')
        if target.shape != pred.shape:
            raise ValueError('gv: predictions %s and targets %s must both be (B, T, D)' % (tuple(pred.shape), tuple(target.shape)))
    seq_len = _lengths(seq_len, b)
    dev = pred.device
    loss = state = v_pred = v_tgt = None
    if target is not None:
        loss = torch.empty((), dtype=torch.float32, device=dev)
        state = torch.empty((b, d, 2), dtype=torch.float64, device=dev)
    if want_variances or target is None:
        v_pred = torch.empty((b, d), dtype=torch.float32, device=dev)
        v_tgt = torch.empty((b, d), dtype=torch.float32, device=dev) if target is not None else None
    ws = workspace(lib.mg_gv_workspace_bytes(b, t, d), dev)
    ts = target.stride() if target is not None else (0, 0, 0)
    _lib.check(lib.mg_gv_f32(_p(pred), pred.stride(0), pred.stride(1), pred.stride(2), _p(target), ts[0], ts[1], ts[2], _p(seq_len), b, t, d,
                             1 if log else 0, float(eps), _p(loss), _p(state), _p(v_pred), _p(v_tgt), _p(ws), ws.numel(), _stream()),
               'mg_gv_f32')
    return loss, state, v_pred, v_tgt


def gv_backward(grad_loss, state, pred, seq_len=None):
    """d gv / d pred (mg_gv_bwd_f32): a dense (B, T, D) float32 tensor, ``grad_loss * c * (pred - mean)`` on valid frames, 0 on pad
    frames, NaN on an utterance without a valid frame.  ``grad_loss``: the upstream gradient, a one-element float32 device tensor
    that the kernel reads (no host read); ``state``: what ``gv`` returned; ``pred`` is read in place through its strides."""
    lib = _lib.load()
    grad_loss = _one_element(grad_loss)
    pred = _gv_operand(pred, 'predictions')
    b, t, d = pred.shape
    state = _require(state, torch.float64, 'state')
    if tuple(state.shape) != (b, d, 2):
        raise ValueError('state must be (B, D, 2) = (%d, %d, 2), got %s' % (b, d, tuple(state.shape)))
    seq_len = _lengths(seq_len, b)
    grad = torch.empty((b, t, d), dtype=torch.float32, device=pred.device)
    _lib.check(lib.mg_gv_bwd_f32(_p(grad_loss), _p(state), _p(pred), pred.stride(0), pred.stride(1), pred.stride(2), _p(seq_len), b, t, d,
                                 _p(grad), _stream()), 'mg_gv_bwd_f32')
    return grad


POOL_MODES = {'sum': _lib.MG_POOL_SUM, 'mean': _lib.MG_POOL_MEAN, 'max': _lib.MG_POOL_MAX, 'min': _lib.MG_POOL_MIN}


def _pool_mode(mode):
    if mode not in POOL_MODES:
        raise ValueError("pool_segments: mode must be one of 'sum', 'mean', 'max', 'min', got %r" % (mode,))
    return POOL_MODES[mode]


def _pool_lens(seg_lens2d, b, what):
    seg_lens2d = _require(seg_lens2d, torch.int64, 'segment_lens')
    if seg_lens2d.dim() != 2 or seg_lens2d.shape[0] != b:
        raise ValueError('%s: segment_lens must be (B, S) with B = %d, got %s' % (what, b, tuple(seg_lens2d.shape)))
    _phones(seg_lens2d.shape[1], what)
    return seg_lens2d


def segment_pool(x, seg_lens2d, seq_len, mode):
    """Ragged segment pooling (mg_segment_pool_f32, csrc/segpool.hip): x (B, T, F) float32, read in place through its strides (a
    column slice, a misaligned base, a transposed view, an expanded operand); seg_lens2d (B, S) int64; seq_len (B,) int64 or None;
    mode 'sum' | 'mean' | 'max' | 'min'.  Returns (out (B, S, F) float32, arg): the (B, S, F) int32 frame index of each extremum for
    'max' / 'min' (-1 for an empty segment), else None.  No host read: S is the shape of ``seg_lens2d``.  An empty dimension of
    ``x`` and S = 0 are refused here (ValueError), as the other wrappers refuse them, although the C entry point takes them as
    zero work."""
    lib = _lib.load()
    code = _pool_mode(mode)
    x = _require(x, torch.float32, 'sequence_feature', contiguous=False)
    if x.dim() != 3 or 0 in x.shape:
        raise ValueError('sequence_feature must be a non-empty (B, T, F) tensor, got %s' % (tuple(x.shape),))
    if min(x.stride()) < 0:
        x = x.contiguous()
    b, t, f = x.shape
    seg_lens2d = _pool_lens(seg_lens2d, b, 'segment_pool')
    s = seg_lens2d.shape[1]
    seq_len = _lengths(seq_len, b, 'segment_pool: ')
    out = torch.empty((b, s, f), dtype=torch.float32, device=x.device)
    arg = torch.empty((b, s, f), dtype=torch.int32, device=x.device) if mode in ('max', 'min') else None
    _lib.check(lib.mg_segment_pool_f32(_p(x), x.stride(0), x.stride(1), x.stride(2), _p(seg_lens2d), _p(seq_len), b, s, t, f, code, _p(out),
                                       _p(arg), _stream()), 'mg_segment_pool_f32')
    return out, arg


def segment_pool_backward(grad_out, seg_lens2d, seq_len, arg, mode, t):
    """d segment_pool / d x (mg_segment_pool_bwd_f32): the dense (B, t, F) float32 gradient from grad_out (B, S, F), written once by
    one launch - grad_out at the segment of each frame ('sum'), divided by the segment's frame count in float64 ('mean'), at the
    frame ``arg`` names and +0 elsewhere ('max' / 'min'), +0 on every frame outside all segments."""
    lib = _lib.load()
    code = _pool_mode(mode)
    grad_out = _require(grad_out, torch.float32, 'grad_out')
    if grad_out.dim() != 3 or 0 in grad_out.shape or int(t) <= 0:
        raise ValueError('grad_out must be a non-empty (B, S, F) tensor and t positive, got %s, t=%r' % (tuple(grad_out.shape), t))
    b, s, f = grad_out.shape
    seg_lens2d = _pool_lens(seg_lens2d, b, 'segment_pool_backward')
    if seg_lens2d.shape[1] != s:
        raise ValueError('segment_pool_backward: grad_out has %d segments, segment_lens %d' % (s, seg_lens2d.shape[1]))
    seq_len = _lengths(seq_len, b, 'segment_pool_backward: ')
    if mode in ('max', 'min'):
        arg = _require(arg, torch.int32, 'arg')
        if tuple(arg.shape) != (b, s, f):
            raise ValueError('arg must be (B, S, F) = %s, got %s' % ((b, s, f), tuple(arg.shape)))
    else:
        arg = None
    grad = torch.empty((b, int(t), f), dtype=torch.float32, device=grad_out.device)
    _lib.check(lib.mg_segment_pool_bwd_f32(_p(grad_out), _p(seg_lens2d), _p(seq_len), _p(arg), b, s, int(t), f, code, _p(grad), _stream()),
               'mg_segment_pool_bwd_f32')
    return grad


def stream_loss(pred, targets, kinds, seq_len, want_grad, want_prob=False, grad_scale=1.0):
    """Multi-stream loss (mg_stream_loss_f32): pred (B, T, sum of widths), targets[k] (B, T, width_k) scored side by side
    in column order, kinds[k] in {'mse', 'sigmoid_bce'}.  Returns (loss 0-d, grad or None, prob or None)."""
    lib = _lib.load()
    pred = _require(pred, torch.float32, 'predictions')
    if pred.dim() != 3 or len(targets) != len(kinds) or not 1 <= len(targets) <= _lib.MG_STREAMS_MAX:
        raise ValueError('stream_loss: predictions must be (B, T, D) with 1..%d streams' % _lib.MG_STREAMS_MAX)
    b, t, d = pred.shape
    if sum(int(y.shape[-1]) for y in targets) != d:
        raise ValueError('stream_loss: stream widths %s do not add up to D=%d' % ([int(y.shape[-1]) for y in targets], d))
    seq_len = _lengths(seq_len, b, 'stream_loss: ', flat=False)
    descs = (_lib.mg_stream_desc * len(targets))()
    keep, col0, prob = [], 0, None
    for k, (y, kind) in enumerate(zip(targets, kinds)):
        y = _require(y, torch.float32, 'targets[%d]' % k)
        if y.dim() != 3 or y.shape[0] != b or y.shape[1] != t:
            raise ValueError('stream_loss: targets[%d] %s does not match predictions (%d, %d, *)' % (k, tuple(y.shape), b, t))
        keep.append(y)
        w = int(y.shape[2])
        descs[k].target, descs[k].ldt, descs[k].col0, descs[k].width = y.data_ptr(), w, col0, w
        descs[k].kind = {'mse': _lib.MG_LOSS_MSE, 'sigmoid_bce': _lib.MG_LOSS_SIGMOID_BCE}[kind]
        if kind == 'sigmoid_bce' and want_prob:
            prob = torch.empty((b, t, w), dtype=torch.float32, device=pred.device)
        col0 += w
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    ws = workspace(lib.mg_stream_loss_workspace_bytes(b, t, d), pred.device)
    _lib.check(lib.mg_stream_loss_f32(_p(pred), ctypes.cast(descs, ctypes.c_void_p), len(targets), _p(seq_len), b, t, d,
                                      float(grad_scale), _p(loss), _p(grad), _p(prob), _p(ws), ws.numel(), _stream()),
               'mg_stream_loss_f32')
    return loss, grad, prob


def masked_ce(pred, target, seq_len, want_grad, grad_scale=1.0, want_argmax=False, col0=0, width=None, grad_out=None, loss_out=None,
              loss_weight=1.0, loss_keep=0.0):
    """Masked categorical cross entropy (mg_masked_ce_f32) of columns [col0, col0 + width) of ``pred`` (B, T, D) f32 - all of them by
    default - against ``target`` (B, T) int64 class indices.  Returns (loss 0-d f32, grad or None, argmax (B, T) int64 or None).

    ``pred`` is read in place when its last dimension is contiguous (a column slice of a wider prediction).  ``grad_out``: a
    (B, T, D) f32 buffer whose columns [col0, col0 + width) receive the gradient (the other columns are not touched) instead of a
    new (B, T, width) tensor.  ``loss_out`` / ``loss_weight`` / ``loss_keep``: loss_out = loss_weight * loss + loss_keep * loss_out
    on the device (``loss_keep == 0``: loss_out is only written)."""
    lib = _lib.load()
    pred, ldp = _require(pred, torch.float32, 'predictions', rows=True)
    b, t, d = pred.shape
    c = d - col0 if width is None else int(width)
    if col0 < 0 or c < 1 or col0 + c > d:
        raise ValueError('ce: columns [%d, %d) do not fit predictions %s' % (col0, col0 + c, tuple(pred.shape)))
    target = _require(target, torch.int64, 'targets')
    if tuple(target.shape) != (b, t):
        raise ValueError('ce: targets %s do not match predictions %s: (B, T) class indices wanted' % (tuple(target.shape), tuple(pred.shape)))
    seq_len = _lengths(seq_len, b, 'ce: ', flat=False)
    loss, grad, g, ldg, gcol0 = _loss_and_grad_out('ce', pred, c, col0, want_grad, grad_out, loss_out)
    argmax = torch.empty((b, t), dtype=torch.int64, device=pred.device) if want_argmax else None
    ws = workspace(lib.mg_masked_ce_workspace_bytes(b, t, c), pred.device)
    _lib.check(lib.mg_masked_ce_f32(_p(pred), ldp, col0, _p(target), _p(seq_len), b, t, c, float(grad_scale), float(loss_weight),
                                    float(loss_keep), _p(loss), _p(g), ldg, gcol0, _p(argmax), _p(ws), ws.numel(), _stream()),
               'mg_masked_ce_f32')
    return loss, grad, argmax


def _mdn_shape(what, pred, n_components, dim, col0):
    """(B, T, D_total) predictions whose columns [col0, col0 + K (1 + 2 dim)) are one mixture-density stream -> that width, after the
    caps of include/morgana_hip.h (refused here, before anything is allocated or launched)."""
    k, d = int(n_components), int(dim)
    if k < 1 or d < 1:
        raise ValueError('%s: n_components=%d and a target width of %d must both be positive' % (what, k, d))
    if k > _lib.MG_MDN_MAX_COMPONENTS:
        raise _lib.MorganaHipError('%s: n_components=%d exceeds the cap of %d components (MG_MDN_MAX_COMPONENTS)'
                                   % (what, k, _lib.MG_MDN_MAX_COMPONENTS))
    if k * d > _lib.MG_MDN_MAX_ROW:
        raise _lib.MorganaHipError('%s: n_components * D = %d exceeds the cap of %d means per frame (MG_MDN_MAX_ROW)'
                                   % (what, k * d, _lib.MG_MDN_MAX_ROW))
    w = k * (1 + 2 * d)
    if col0 < 0 or col0 + w > pred.shape[2]:
        raise ValueError('%s: columns [%d, %d) = %d components x (1 + 2 x %d) do not fit predictions %s'
                         % (what, col0, col0 + w, k, d, tuple(pred.shape)))
    return k, d, w


def masked_mdn(pred, target, seq_len, n_components, want_grad, min_log_std=None, grad_scale=1.0, col0=0, grad_out=None, loss_out=None,
               loss_weight=1.0, loss_keep=0.0):
    """Masked mixture-density negative log likelihood (mg_masked_mdn_f32, csrc/mdn.hip) of columns [col0, col0 + K (1 + 2 D)) of
    ``pred`` (B, T, *) f32 - K = ``n_components`` logits, K D means (component-major), K D log standard deviations - against
    ``target`` (B, T, D) f32, in nats per dimension.  Returns (loss 0-d f32, grad or None).

    ``pred`` is read in place when its last dimension is contiguous (a column slice of a wider prediction).  ``min_log_std``: a floor
    under the log standard deviations (None = none); a floored one gets gradient 0.  ``grad_out``: a (B, T, *) f32 buffer shaped
    like ``pred`` whose columns [col0, col0 + K (1 + 2 D)) receive the gradient (the other columns are not touched) instead of a new
    (B, T, K (1 + 2 D)) tensor.  ``loss_out`` / ``loss_weight`` / ``loss_keep``: loss_out = loss_weight * loss + loss_keep *
    loss_out on the device (``loss_keep == 0``: loss_out is only written)."""
    lib = _lib.load()
    pred, ldp = _require(pred, torch.float32, 'predictions', rows=True)
    target, ldt = _require(target, torch.float32, 'targets', rows=True)
    b, t, _ = pred.shape
    if target.shape[0] != b or target.shape[1] != t:
        raise ValueError('mdn: targets %s do not match predictions %s: (B, T, D) wanted' % (tuple(target.shape), tuple(pred.shape)))
    k, d, w = _mdn_shape('mdn', pred, n_components, target.shape[2], col0)
    seq_len = _lengths(seq_len, b, 'mdn: ')
    loss, grad, g, ldg, gcol0 = _loss_and_grad_out('mdn', pred, w, col0, want_grad, grad_out, loss_out)
    ws = workspace(lib.mg_masked_mdn_workspace_bytes(b, t, k, d), pred.device)
    _lib.check(lib.mg_masked_mdn_f32(_p(pred), ldp, col0, _p(target), ldt, _p(seq_len), b, t, k, d,
                                     0.0 if min_log_std is None else float(min_log_std), int(min_log_std is not None), float(grad_scale),
                                     float(loss_weight), float(loss_keep), _p(loss), _p(g), ldg, gcol0, _p(ws), ws.numel(), _stream()),
               'mg_masked_mdn_f32')
    return loss, grad


def mdn_select(pred, seq_len, n_components, dim, min_log_std=None, col0=0):
    """The most probable component of every frame of a mixture-density stream (mg_mdn_select_f32; the column layout of
    ``masked_mdn``, D = ``dim``): (component (B, T) int64 - the lowest index among the largest logits, mean (B, T, D) - that
    component's means, copied, variance (B, T, D) = exp(2 max(log std, min_log_std)) of that component).  Pad frames hold 0, 0 and 1."""
    lib = _lib.load()
    pred, ldp = _require(pred, torch.float32, 'predictions', rows=True)
    b, t, _ = pred.shape
    k, d, _ = _mdn_shape('mdn_select', pred, n_components, dim, col0)
    seq_len = _lengths(seq_len, b, 'mdn_select: ')
    component = torch.empty((b, t), dtype=torch.int64, device=pred.device)
    mean = torch.empty((b, t, d), dtype=torch.float32, device=pred.device)
    variance = torch.empty((b, t, d), dtype=torch.float32, device=pred.device)
    _lib.check(lib.mg_mdn_select_f32(_p(pred), ldp, col0, _p(seq_len), b, t, k, d, 0.0 if min_log_std is None else float(min_log_std),
                                     int(min_log_std is not None), _p(component), _p(mean), _p(variance), _stream()), 'mg_mdn_select_f32')
    return component, mean, variance


def mdn_sample_arguments(what, temperature, noise_scale):
    """(temperature, noise_scale) of a mixture draw as floats, or ValueError: ``temperature`` a finite Python number > 0,
    ``noise_scale`` a finite Python number >= 0.  No device is needed."""
    for name, value in (('temperature', temperature), ('noise_scale', noise_scale)):
        if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value):
            raise ValueError('%s: %s must be a finite Python number, got %r' % (what, name, value))
    if temperature == 0:
        raise ValueError('%s: temperature=0 is the most probable component of every frame: that is mdn_select, not a draw' % what)
    if temperature < 0:
        raise ValueError('%s: temperature must be > 0, got %r' % (what, temperature))
    if noise_scale < 0:
        raise ValueError('%s: noise_scale must be >= 0, got %r' % (what, noise_scale))
    inv = 1.0 / float(temperature)
    if not 0.0 < inv <= 3.4028234663852886e38:
        raise ValueError('%s: 1 / temperature = %r is no positive finite float32' % (what, inv))
    return float(temperature), float(noise_scale)


def mdn_sample_shape(pred, n_components, dim, col0=0):
    """The refusals of ``mdn_sample`` that depend on the tensor alone (device, dtype, the caps, the column range), for a caller
    that wants them before it reserves a draw of the step counter."""
    pred = _require(pred, torch.float32, 'predictions', contiguous=False)
    if pred.dim() != 3:
        raise ValueError('predictions must be (B, T, C), got %s' % (tuple(pred.shape),))
    return _mdn_shape('mdn_sample', pred, n_components, dim, col0)


def mdn_sample(pred, seq_len, n_components, dim, seed, used, min_log_std=None, temperature=1., noise_scale=0., col0=0):
    """A DRAW from every frame of a mixture-density stream (mg_mdn_sample_f32; the column layout of ``masked_mdn``, D = ``dim``):
    (component (B, T) int64 ~ softmax(logits / temperature), mean (B, T, D) - that component's means, plus ``noise_scale`` of its
    standard deviations times N(0, 1) noise when ``noise_scale`` > 0, variance (B, T, D) = exp(2 max(log std, min_log_std)) of that
    component).  The uniform of frame (b, t) and the noise of element (b, t, d) come from (seed, MDN_COMPONENT_SITE / MDN_NOISE_SITE,
    used[0], b T + t [, d]): the same four numbers give the same bits.  ``used``: a 1-element int64 DEVICE tensor (``dropout_draw``).
    Pad frames hold 0, 0 and 1."""
    temperature, noise_scale = mdn_sample_arguments('mdn_sample', temperature, noise_scale)
    lib = _lib.load()
    pred, ldp = _require(pred, torch.float32, 'predictions', rows=True)
    b, t, _ = pred.shape
    k, d, _ = _mdn_shape('mdn_sample', pred, n_components, dim, col0)
    seq_len = _lengths(seq_len, b, 'mdn_sample: ')
    component = torch.empty((b, t), dtype=torch.int64, device=pred.device)
    mean = torch.empty((b, t, d), dtype=torch.float32, device=pred.device)
    variance = torch.empty((b, t, d), dtype=torch.float32, device=pred.device)
    _lib.check(lib.mg_mdn_sample_f32(_p(pred), ldp, col0, _p(seq_len), b, t, k, d, 0.0 if min_log_std is None else float(min_log_std),
                                     int(min_log_std is not None), 1.0 / temperature, noise_scale, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     MDN_COMPONENT_SITE, MDN_NOISE_SITE, _p(used), _p(component), _p(mean), _p(variance), _stream()),
               'mg_mdn_sample_f32')
    return component, mean, variance


def stream_loss_ce(pred, targets, kinds, widths, seq_len, want_grad, want_prob=False, want_argmax=False):
    """``stream_loss`` for a stream table that holds 'ce' streams: the mse / sigmoid_bce streams take ONE mg_stream_loss_f32 launch
    over a descriptor table of their own (gradient weight n_rest / n through ``grad_scale``), every 'ce' stream (``targets[k]`` (B, T) int64, ``widths[k]`` classes) one mg_masked_ce_f32
    launch that writes its column slice of the same gradient tensor with weight 1 / n and adds its loss on the device
    (loss = loss_rest * n_rest / n + sum_k ce_k / n: the reference-style mean over all n streams).  No host read.  Returns
    (loss 0-d, grad or None, prob or None, [argmax per stream or None])."""
    lib = _lib.load()
    pred = _require(pred, torch.float32, 'predictions')
    if pred.dim() != 3 or len(targets) != len(kinds) or not 1 <= len(targets) <= _lib.MG_STREAMS_MAX:
        raise ValueError('stream_loss: predictions must be (B, T, D) with 1..%d streams' % _lib.MG_STREAMS_MAX)
    b, t, d = pred.shape
    seq_len = _lengths(seq_len, b, 'stream_loss: ', flat=False)
    n = len(kinds)
    widths = [int(w) for w in widths]
    if len(widths) != n or min(widths) < 1 or sum(widths) != d:
        raise ValueError('stream_loss: stream widths %s do not add up to D=%d' % (widths, d))
    rest = [k for k in range(n) if kinds[k] != 'ce']
    descs = (_lib.mg_stream_desc * max(len(rest), 1))()
    keep, prob, col0s = [], None, [sum(widths[:k]) for k in range(n)]
    for j, k in enumerate(rest):
        y = _require(targets[k], torch.float32, 'targets[%d]' % k)
        if y.dim() != 3 or y.shape[0] != b or y.shape[1] != t or y.shape[2] != widths[k]:
            raise ValueError('stream_loss: targets[%d] %s does not match predictions (%d, %d, *)' % (k, tuple(y.shape), b, t))
        keep.append(y)
        descs[j].target, descs[j].ldt, descs[j].col0, descs[j].width = y.data_ptr(), widths[k], col0s[k], widths[k]
        descs[j].kind = {'mse': _lib.MG_LOSS_MSE, 'sigmoid_bce': _lib.MG_LOSS_SIGMOID_BCE}[kinds[k]]
        if kinds[k] == 'sigmoid_bce' and want_prob:
            prob = torch.empty((b, t, widths[k]), dtype=torch.float32, device=pred.device)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    if rest:
        # zero in the columns no descriptor covers (the 'ce' streams' columns: overwritten below)
        ws = workspace(lib.mg_stream_loss_workspace_bytes(b, t, d), pred.device)
        _lib.check(lib.mg_stream_loss_f32(_p(pred), ctypes.cast(descs, ctypes.c_void_p), len(rest), _p(seq_len), b, t, d,
                                          float(len(rest)) / n, _p(loss), _p(grad), _p(prob), _p(ws), ws.numel(), _stream()),
                   'mg_stream_loss_f32')
    argmaxes, first = [None] * n, True
    for k in range(n):
        if kinds[k] != 'ce':
            continue
        keep_w = (float(len(rest)) / n if rest else 0.0) if first else 1.0
        _, _, argmaxes[k] = masked_ce(pred, targets[k], seq_len, want_grad, grad_scale=1.0 / n, want_argmax=want_argmax,
                                      col0=col0s[k], width=widths[k], grad_out=grad, loss_out=loss, loss_weight=1.0 / n, loss_keep=keep_w)
        first = False
    return loss, grad, prob, argmaxes


def pad_normalise(packed, offsets, t, p0=None, p1=None, kind=None, want_raw=True, bf16_extra_rows=None):
    """Packed utterances (sum len, D) + offsets (B+1) -> (raw (B,t,D) or None, normalised (B,t,D) or None).
    ``bf16_extra_rows`` (an int, needs ``kind``): the same pass also writes the normalised feature's bf16 operand table
    (B*t + bf16_extra_rows, pad_ld(D)) - what cast_pad_bf16 would make of the normalised output - and it is returned as a third value."""
    lib = _lib.load()
    packed = _require(packed, torch.float32, 'packed feature')
    offsets = _require(offsets, torch.int64, 'offsets')
    b, d = offsets.numel() - 1, packed.shape[1]
    raw = torch.empty((b, t, d), dtype=torch.float32, device=packed.device) if want_raw else None
    norm = None
    if kind is not None:
        p0, p1 = _norm_vectors(p0, p1, d)
        norm = torch.empty((b, t, d), dtype=torch.float32, device=packed.device)
    if bf16_extra_rows is not None:
        if kind is None:
            raise ValueError('pad_normalise: the bf16 table is the NORMALISED feature: it needs normaliser parameters')
        ldb = pad_ld(d)
        table = torch.empty((b * int(t) + int(bf16_extra_rows), ldb), dtype=torch.bfloat16, device=packed.device)
        if table.numel() == 0:      # t = 0 without extra rows: every output is empty (no address to hand the library)
            return raw, norm, table
        _lib.check(lib.mg_pad_normalise_bf16_f32(_p(packed), _p(offsets), b, int(t), d, _p(p0), _p(p1), kind, _p(raw), _p(norm), _p(table), ldb,
                                                 int(bf16_extra_rows), _stream()), 'mg_pad_normalise_bf16_f32')
        return raw, norm, table
    if int(t) == 0:                 # empty outputs: the library would see NULL for both and call it "no output requested"
        return raw, norm
    _lib.check(lib.mg_pad_normalise_f32(_p(packed), _p(offsets), b, int(t), d, _p(p0), _p(p1), -1 if kind is None else kind,
                                        _p(raw), _p(norm), _stream()), 'mg_pad_normalise_f32')
    return raw, norm


def _item_tables(p0, p1, item_row, b, d, what):
    """The (S, D) parameter tables and the (B,) int32 row index of the per-item kernels, checked against B items of D columns."""
    p0 = _require(p0, torch.float32, 'param0 table')
    p1 = _require(p1, torch.float32, 'param1 table')
    item_row = _require(item_row, torch.int32, 'item_row')
    if p0.dim() != 2 or p0.shape != p1.shape or p0.shape[1] != d:
        raise ValueError('%s: parameter tables %s / %s must both be (speakers, %d)' % (what, tuple(p0.shape), tuple(p1.shape), d))
    if item_row.dim() != 1 or item_row.numel() != b:
        raise ValueError('%s: item_row %s must hold one row index for each of the %d batch items' % (what, tuple(item_row.shape), b))
    return p0, p1, item_row


def _norm_vectors(p0, p1, width, columns=('feature dim is %d',)):
    """The two (width,) parameter vectors of a normaliser; ``columns``: (format, values in front of ``width``), what the error says
    ``width`` counts (formatted only when it is raised: these wrappers are timed per call)."""
    p0 = _require(p0, torch.float32, 'param0')
    p1 = _require(p1, torch.float32, 'param1')
    if p0.numel() != width or p1.numel() != width:
        raise ValueError('normaliser parameters have %d / %d entries, ' % (p0.numel(), p1.numel()) + columns[0] % (columns[1:] + (width,)))
    return p0, p1


def _norm_twin(what, kind, p0, p1, item_row, b, width, columns, kind_name='kind', want_raw=None):
    """The normalised twin a data-path launch writes next to its raw output -> (p0, p1, item_row, parameter rows, kind code): vectors
    (width,) and 0 rows, or with ``item_row`` (B,) int32 tables (S, width) and S rows; (None, None, None, 0, -1) without a ``kind``.
    ``columns``: as ``_norm_vectors`` takes it.  ``want_raw``: the caller's flag where it has one - no raw output needs a kind too."""
    if kind is None:
        if want_raw is False or p0 is not None or p1 is not None or item_row is not None:
            raise ValueError('%s: normaliser parameters%s go with a %s (NORM_MVN or NORM_MINMAX)' % (
                what, ' and item_row' if want_raw is None else ', item_row and want_raw=False', kind_name))
        return None, None, None, 0, -1
    if kind not in (NORM_MVN, NORM_MINMAX):
        raise ValueError('%s: %s %r is not NORM_MVN or NORM_MINMAX' % (what, kind_name, kind))
    if item_row is None:
        return _norm_vectors(p0, p1, width, columns) + (None, 0, kind)
    p0, p1, item_row = _item_tables(p0, p1, item_row, b, width, what)
    return p0, p1, item_row, p0.shape[0], kind


def _ragged_input(what, x, offsets, seq_len, width=None):
    """A float32 feature in exactly one layout -> (offsets, seq_len, B, T_in, D): ``offsets`` (B + 1,) int64 with x the packed rows
    (N, D) (T_in = 0), or ``seq_len`` (B,) int64 with x padded (B, T_in, D).  ``width``: the D the caller expects."""
    if (offsets is None) == (seq_len is None):
        raise ValueError('%s: give exactly one of offsets (packed rows) and seq_len (padded batch)' % what)
    cols = 'features' if width is None else '%d' % width
    if offsets is not None:
        offsets = _require(offsets, torch.int64, 'offsets')
        if x.dim() != 2 or (width is not None and x.shape[1] != width) or offsets.dim() != 1 or offsets.numel() < 1:
            raise ValueError('%s: packed rows %s must be (rows, %s) and offsets %s (items + 1,)' % (
                what, tuple(x.shape), cols, tuple(offsets.shape)))
        return offsets, None, offsets.numel() - 1, 0, x.shape[1]
    seq_len = _require(seq_len, torch.int64, 'seq_len')
    if x.dim() != 3 or (width is not None and x.shape[2] != width) or seq_len.dim() != 1 or seq_len.numel() != x.shape[0]:
        raise ValueError('%s: padded batch %s must be (items, frames, %s) and seq_len %s (items,)' % (
            what, tuple(x.shape), cols, tuple(seq_len.shape)))
    return (None, seq_len) + tuple(x.shape)


def normalise_items(x, p0, p1, item_row, kind, grad=False):
    """``normalise`` with a parameter row per batch item: x (B, ..., D) f32, tables p0 / p1 (S, D), item_row (B,) int32; item b is mapped
    with row item_row[b] (NaN for an index outside [0, S)).  ``grad=True``: x is a gradient and the result is x * d out / d x of
    ``kind`` - the per-item, per-column scale, in the same launch."""
    lib = _lib.load()
    x = _require(x, torch.float32, 'feature')
    if x.dim() < 2:
        raise ValueError('normalise_items: the feature must be (batch, ..., features), got %s' % (tuple(x.shape),))
    b, d = x.shape[0], x.shape[-1]
    p0, p1, item_row = _item_tables(p0, p1, item_row, b, d, 'normalise_items')
    out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    _lib.check(lib.mg_normalise_items_f32(_p(x), _p(out), _p(p0), _p(p1), _p(item_row), b, x.numel() // (b * d), d, p0.shape[0], kind,
                                          int(bool(grad)), _stream()), 'mg_normalise_items_f32')
    return out


def normalise_items_backward(grad, p0, p1, item_row, kind):
    """Gradient of ``normalise_items`` with respect to its feature."""
    return normalise_items(grad, p0, p1, item_row, kind, grad=True)


def pad_normalise_items(packed, offsets, t, p0, p1, item_row, kind, want_raw=True):
    """``pad_normalise`` with tables (S, D) and one row index per utterance (speaker-dependent normalisers in the device loader):
    packed (sum len, D) + offsets (B+1) -> (raw (B,t,D) or None, normalised (B,t,D))."""
    lib = _lib.load()
    packed = _require(packed, torch.float32, 'packed feature')
    offsets = _require(offsets, torch.int64, 'offsets')
    b, d = offsets.numel() - 1, packed.shape[1]
    p0, p1, item_row = _item_tables(p0, p1, item_row, b, d, 'pad_normalise_items')
    raw = torch.empty((b, t, d), dtype=torch.float32, device=packed.device) if want_raw else None
    norm = torch.empty((b, t, d), dtype=torch.float32, device=packed.device)
    _lib.check(lib.mg_pad_normalise_items_f32(_p(packed), _p(offsets), b, int(t), d, _p(p0), _p(p1), _p(item_row), p0.shape[0], kind,
                                              _p(raw), _p(norm), _stream()), 'mg_pad_normalise_items_f32')
    return raw, norm


def item_rows(table, item_row):
    """table (S, D) f32, item_row (B,) int32 -> (B, D): row item_row[b] for every batch item, NaN for an index outside [0, S) (the
    guarded form of ``table[item_row]``: a bad index must not fault a device that others share)."""
    lib = _lib.load()
    table = _require(table, torch.float32, 'table')
    item_row = _require(item_row, torch.int32, 'item_row')
    if table.dim() != 2 or item_row.dim() != 1 or item_row.numel() == 0:
        raise ValueError('item_rows: table %s must be (speakers, features) and item_row %s (batch,)' % (
            tuple(table.shape), tuple(item_row.shape)))
    out = torch.empty((item_row.numel(), table.shape[1]), dtype=torch.float32, device=table.device)
    _lib.check(lib.mg_item_rows_f32(_p(table), table.shape[0], table.shape[1], _p(item_row), item_row.numel(), _p(out), _stream()),
               'mg_item_rows_f32')
    return out


def column_stats(state, x, *, offsets=None, seq_len=None, item_row=None, max_rows=None):
    """state (S, 5, D) float64 += the per-column count / mean / M2 / min / max of the valid rows of one batch (mg_column_stats_f32:
    shifted float64 chunks merged by Chan's update in a fixed order, updated in place, nothing read back).  Exactly one layout:
    ``offsets`` (B + 1,) int64 with x the packed rows (N, D), or ``seq_len`` (B,) int64 with x padded (B, T, D).  ``item_row`` (B,)
    int32 names the group (state row) of every item; an index outside [0, S) contributes to nothing.  ``max_rows``: the longest
    item of a packed batch when the host knows it (it only sets how many workgroups share an item; default: one chunk per item)."""
    lib = _lib.load()
    if isinstance(state, torch.Tensor) and not state.is_contiguous():
        raise ValueError('column_stats: state is updated in place and must be contiguous')
    state = _require(state, torch.float64, 'state')
    x = _require(x, torch.float32, 'feature')
    if state.dim() != 3 or state.shape[1] != _lib.MG_COLSTATS_FIELDS:
        raise ValueError('column_stats: state %s must be (groups, %d, features)' % (tuple(state.shape), _lib.MG_COLSTATS_FIELDS))
    groups = state.shape[0]
    offsets, seq_len, b, t, d = _ragged_input('column_stats', x, offsets, seq_len, width=state.shape[2])
    if offsets is not None:
        rows = max(1, min(int(max_rows), x.shape[0])) if max_rows is not None else 1
    else:
        rows = t
    if item_row is not None:
        item_row = _require(item_row, torch.int32, 'item_row')
        if item_row.dim() != 1 or item_row.numel() != b:
            raise ValueError('column_stats: item_row %s must hold one group for each of the %d items' % (tuple(item_row.shape), b))
    elif groups != 1:
        raise ValueError('column_stats: a state of %d groups needs item_row' % groups)
    if b == 0 or x.numel() == 0:
        return state
    need = int(lib.mg_column_stats_workspace_bytes(b, rows, d))
    buf = workspace(need, x.device)
    _lib.check(lib.mg_column_stats_f32(_p(x), d, d, b, int(t), _p(offsets), _p(seq_len), _p(item_row), groups, _p(state), _p(buf), need,
                                       _stream()), 'mg_column_stats_f32')
    return state


def normalise(x, p0, p1, kind):
    lib = _lib.load()
    x = _require(x, torch.float32, 'feature')
    d = x.shape[-1]
    p0, p1 = _norm_vectors(p0, p1, d)
    out = torch.empty_like(x)
    _lib.check(lib.mg_normalise_f32(_p(x), _p(out), _p(p0), _p(p1), x.numel() // d, d, kind, _stream()),
               'mg_normalise_f32')
    return out


# ----------------------------------------------------------------------------------------------------------------- K2
def linear_fwd_f32(a, rows, m, weight, bias, act):
    """a: (R, K) f32 table/input; rows: int32 (m,) or None.  Returns (m, N) f32."""
    lib = _lib.load()
    n, k = weight.shape
    y = torch.empty((m, n), dtype=torch.float32, device=weight.device)
    _lib.check(lib.mg_linear_fwd_f32(_p(a), a.shape[1], _p(rows), m, k, _p(weight), _p(bias), n, _p(y), n, act,
                                     _stream()), 'mg_linear_fwd_f32')
    return y


def linear_dgrad_f32(dy, weight, h, act=ACT_SIGMOID):
    """dX = (dY W) * f'(h): ``h`` None or the OUTPUT of activation ``act`` (ACT_SIGMOID / ACT_TANH / ACT_RELU) feeding the layer."""
    lib = _lib.load()
    n, k = weight.shape
    m = dy.shape[0]
    dx = torch.empty((m, k), dtype=torch.float32, device=dy.device)
    if h is None:
        act = ACT_NONE
    _lib.check(lib.mg_linear_dgrad_act_f32(_p(dy), m, n, _p(weight), k, _p(h), act, _p(dx), _stream()), 'mg_linear_dgrad_act_f32')
    return dx


def linear_wgrad_f32(dy, a, rows, n, k, want_bias=True):
    lib = _lib.load()
    m = dy.shape[0]
    dw = torch.empty((n, k), dtype=torch.float32, device=dy.device)
    db = torch.empty((n,), dtype=torch.float32, device=dy.device) if want_bias else None
    nbytes = lib.mg_linear_wgrad_workspace_bytes(m, n, k)
    ws = workspace(nbytes, dy.device)
    _lib.check(lib.mg_linear_wgrad_f32(_p(dy), _p(a), a.shape[1], _p(rows), m, n, k, _p(dw), _p(db), 0, _p(ws),
                                       ws.numel(), _stream()), 'mg_linear_wgrad_f32')
    return dw, db


def cast_pad_bf16(x2d, ld=None, extra_rows=0):
    """(rows, cols) f32 -> (rows + extra_rows, ld) bf16, padding columns and the extra rows zero."""
    lib = _lib.load()
    rows, cols = x2d.shape
    ld = pad8(cols) if ld is None else ld
    out = torch.empty((rows + extra_rows, ld), dtype=torch.bfloat16, device=x2d.device)
    if extra_rows:
        out[rows:].zero_()
    _lib.check(lib.mg_cast_pad_bf16(_p(x2d), x2d.shape[1], _p(out), ld, rows, cols, _stream()), 'mg_cast_pad_bf16')
    return out


def cast_transpose_bf16(x2d):
    """(rows, cols) f32 -> (cols, pad8(rows)) bf16."""
    lib = _lib.load()
    rows, cols = x2d.shape
    ld = pad8(rows)
    out = torch.empty((cols, ld), dtype=torch.bfloat16, device=x2d.device)
    _lib.check(lib.mg_cast_transpose_bf16(_p(x2d), cols, _p(out), ld, rows, cols, _stream()), 'mg_cast_transpose_bf16')
    return out


def cast_bf16_f32(x_bf16, cols):
    lib = _lib.load()
    rows, ld = x_bf16.shape
    out = torch.empty((rows, cols), dtype=torch.float32, device=x_bf16.device)
    _lib.check(lib.mg_cast_bf16_f32(_p(x_bf16), ld, _p(out), cols, rows, cols, _stream()), 'mg_cast_bf16_f32')
    return out


ACT_ROWS_RUNS = _lib.MG_ACT_ROWS_RUNS      # `rows` is a frame map of upsample_to_repetitions (runs of equal indices); a hint only


def linear_fwd_bf16(a, rows, m, k, w_bf16, bias, n, act, out_f32=False, rows_runs=False):
    """a: (R, lda) bf16; w_bf16: (n, ldw) bf16.  Returns (m, pad8(n)) bf16 (or (m, n rounded up to 8) f32), padding columns zero.
    ``rows_runs``: the row map consists of runs of equal consecutive indices (performance hint, same results)."""
    lib = _lib.load()
    # a bf16 result is the next layer's operand (rows padded to the large tiles' k step); an fp32 one leaves the stack: padded to the
    # 16-byte chunk only, so that its consumer needs no slice-and-copy pass (N = 80: 64,000 x 128 -> x 80 was a 41 MB copy at C4)
    ldy = (n + 7) // 8 * 8 if out_f32 else pad8(n)
    y = torch.empty((m, ldy), dtype=torch.float32 if out_f32 else torch.bfloat16, device=a.device)
    if rows_runs and rows is not None:
        act = act | ACT_ROWS_RUNS
    _lib.check(lib.mg_linear_fwd_bf16(_p(a), a.shape[1], _p(rows), m, k, _p(w_bf16), w_bf16.shape[1], _p(bias), n,
                                      _p(y), ldy, 1 if out_f32 else 0, act, _stream()), 'mg_linear_fwd_bf16')
    return y


def linear_dgrad_bf16(dy, m, n, wt_bf16, k, h, out_f32=False, act=ACT_SIGMOID):
    """dy (m, lddy) bf16; wt_bf16 = W^T (k, pad8(n)) bf16; h None or (m, ldh) bf16, the OUTPUT of activation ``act`` feeding the
    layer.  Returns (m, pad8(k)) bf16/f32."""
    lib = _lib.load()
    lddx = pad8(k)
    dx = torch.empty((m, lddx), dtype=torch.float32 if out_f32 else torch.bfloat16, device=dy.device)
    if h is None:
        act = ACT_NONE
    _lib.check(lib.mg_linear_dgrad_act_bf16(_p(dy), dy.shape[1], m, n, _p(wt_bf16), wt_bf16.shape[1], k, _p(h),
                                            h.shape[1] if h is not None else 0, act, _p(dx), lddx, 1 if out_f32 else 0,
                                            _stream()), 'mg_linear_dgrad_act_bf16')
    return dx


def linear_wgrad_bf16(dy, a, rows, m, n, k, want_bias=True, out_w=None, out_b=None, accumulate=False):
    """out_w / out_b: optional preallocated fp32 destinations (e.g. slices of one gradient buffer); accumulate adds into them."""
    lib = _lib.load()
    if out_w is None and out_b is None and want_bias:
        # db right behind dW in one buffer: the wide-tile path then finishes both with ONE reduce launch (a slab is [dW | db])
        both = torch.empty((n * k + n,), dtype=torch.float32, device=dy.device)
        dw, db = both[:n * k].view(n, k), both[n * k:]
    else:
        dw = out_w if out_w is not None else torch.empty((n, k), dtype=torch.float32, device=dy.device)
        db = None
        if want_bias:
            db = out_b if out_b is not None else torch.empty((n,), dtype=torch.float32, device=dy.device)
    nbytes = lib.mg_linear_wgrad_workspace_bytes(m, n, k)
    ws = workspace(nbytes, dy.device)
    _lib.check(lib.mg_linear_wgrad_bf16(_p(dy), dy.shape[1], _p(a), a.shape[1], _p(rows), m, n, k, _p(dw), _p(db), int(bool(accumulate)),
                                        _p(ws), ws.numel(), _stream()), 'mg_linear_wgrad_bf16')
    return dw, db


def wgrad_rows_ok(m, n, k, lda, lddy):
    """Shapes mg_linear_wgrad_rows_bf16 takes (both operands gathered: the valid frames of a ragged batch out of padded arrays): the
    128 x 512 wide tiles, not their half-width plan (csrc/gemm_bf16_big.hip: wgrad_ksplit)."""
    return (m >= 4096 and n % 128 == 0 and lddy >= n and lddy % 8 == 0 and lda == 512 and 384 < k <= 512 and
            not (n == 128 and m <= 32768))


def linear_wgrad_rows_bf16(dy, dy_rows, a, rows, m, n, k, want_bias=True, out_w=None, out_b=None, accumulate=False):
    """dW = sum_{i < m} dy[dy_rows[i]]^T a[rows[i]] (rows None: a[dy_rows[i]]), db = sum_i dy[dy_rows[i]]: linear_wgrad_bf16 on the m
    index pairs only (``dy_rows`` int32, every entry a valid row of ``dy``).  out_w / out_b / accumulate as linear_wgrad_bf16."""
    lib = _lib.load()
    dy_rows = _require(dy_rows, torch.int32, 'dy_rows')
    if out_w is not None or out_b is not None:
        dw = out_w if out_w is not None else torch.empty((n, k), dtype=torch.float32, device=dy.device)
        db = (out_b if out_b is not None else torch.empty((n,), dtype=torch.float32, device=dy.device)) if want_bias else None
    elif want_bias:                                # db right behind dW: one reduce launch for both
        both = torch.empty((n * k + n,), dtype=torch.float32, device=dy.device)
        dw, db = both[:n * k].view(n, k), both[n * k:]
    else:
        dw, db = torch.empty((n, k), dtype=torch.float32, device=dy.device), None
    nbytes = lib.mg_linear_wgrad_workspace_bytes(m, n, k)
    ws = workspace(nbytes, dy.device)
    _lib.check(lib.mg_linear_wgrad_rows_bf16(_p(dy), dy.shape[1], _p(dy_rows), _p(a), a.shape[1], _p(rows), m, n, k, _p(dw), _p(db),
                                             int(bool(accumulate)), _p(ws), ws.numel(), _stream()), 'mg_linear_wgrad_rows_bf16')
    return dw, db


def wgrad_slabs_ok(m, n, k, lda, lddy):
    """Shapes whose weight gradient runs on the wide-tile kernel and can leave its split-M slabs to the optimiser
    (mg_linear_wgrad_slabs_bf16; the plan of csrc/gemm_bf16_big.hip)."""
    # m <= 32768: the plan then cuts 48-96 slabs; at frame-rate row counts it cuts 192-256, which a reduce launch of its own sums as
    # fast as the update kernel would (A/B after the update kernel's rework: 0.591 vs 0.592 ms per frame-rate step; before it 101 us
    # for 256 slabs of the 128 x 512 gradient on one thread per element)
    return (4096 <= m <= 32768 and n % 128 == 0 and lddy >= n and lddy % 8 == 0 and
            ((lda == 640 and 512 < k <= 640) or (lda == 512 and 384 < k <= 512)))


def wgrad_wide_ok(m, n, k, lda, lddy):
    """Shapes whose weight gradient runs on the wide-tile kernel at all (any row count from 4096 up): its slabs can be taken with
    linear_wgrad_slabs_bf16 and summed by ONE slab_reduce launch (dW | db together) instead of linear_wgrad_bf16's two."""
    return (m >= 4096 and n % 128 == 0 and lddy >= n and lddy % 8 == 0 and
            ((lda == 640 and 512 < k <= 640) or (lda == 512 and 384 < k <= 512)))


def linear_wgrad_slabs_bf16(dy, a, rows, m, n, k, slab=None):
    """linear_wgrad_bf16 without the reduce: returns (slab buffer, n_slabs, stride); slab s holds [n*k weight partials | n bias
    partials].  ``slab`` = a buffer to reuse (kept by the caller until the optimiser has consumed it)."""
    lib = _lib.load()
    nbytes = lib.mg_linear_wgrad_workspace_bytes(m, n, k)
    slab = _slab_buffer(slab, nbytes, dy.device)
    n_slabs, stride = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(lib.mg_linear_wgrad_slabs_bf16(_p(dy), dy.shape[1], _p(a), a.shape[1], _p(rows), m, n, k, _p(slab), slab.numel(),
                                              ctypes.byref(n_slabs), ctypes.byref(stride), _stream()), 'mg_linear_wgrad_slabs_bf16')
    return slab, n_slabs.value, stride.value


def linear_wgrad_dgrad_bf16(dy, a, m, n, k, wt_bf16, slab=None, tail=None):
    """linear_wgrad_slabs_bf16(dy, a) and linear_dgrad_bf16(dy, wt_bf16, h=a) of a Linear(k -> n) whose input ``a`` (m, lda) is the
    output of the Sigmoid below it - one grid for both where the shapes allow (mg_linear_wgrad_dgrad_bf16), the two launches otherwise.
    Returns (slab buffer, n_slabs, stride, dx (m, pad8(k)) bf16).  Needs wgrad_slabs_ok(m, n, k, lda, lddy).
    ``tail``: the deferred end of f0_l2tail_rows_expand (its ``defer=True`` return) - the repeated prediction and the tail's slab sum
    then ride at the end of this grid (mg_linear_wgrad_dgrad_expand_bf16)."""
    lib = _lib.load()
    nbytes = lib.mg_linear_wgrad_workspace_bytes(m, n, k)
    slab = _slab_buffer(slab, nbytes, dy.device)
    lddx = pad8(k)
    dx = torch.empty((m, lddx), dtype=torch.bfloat16, device=dy.device)
    n_slabs, stride = ctypes.c_int(0), ctypes.c_int64(0)
    if tail is not None:
        _lib.check(lib.mg_linear_wgrad_dgrad_expand_bf16(
            _p(dy), dy.shape[1], _p(a), a.shape[1], m, n, k, _p(wt_bf16), wt_bf16.shape[1], _p(dx), lddx, _p(slab), slab.numel(),
            ctypes.byref(n_slabs), ctypes.byref(stride), _p(tail['pred_rows']), _p(tail['rows']), tail['rows'].numel(), _p(tail['out']),
            _p(tail['partials']), tail['n_table_rows'], tail['extra'], _p(tail['ws']), tail['n'], tail['stride'], tail['n_slabs'],
            _p(tail['grads_out']), 1 if tail.get('loss_only') else 0, _stream()), 'mg_linear_wgrad_dgrad_expand_bf16')
        return slab, n_slabs.value, stride.value, dx
    _lib.check(lib.mg_linear_wgrad_dgrad_bf16(_p(dy), dy.shape[1], _p(a), a.shape[1], m, n, k, _p(wt_bf16), wt_bf16.shape[1], _p(dx), lddx,
                                              _p(slab), slab.numel(), ctypes.byref(n_slabs), ctypes.byref(stride), _stream()),
               'mg_linear_wgrad_dgrad_bf16')
    return slab, n_slabs.value, stride.value, dx


def finish_deferred_tail(tail):
    """The deferred end of f0_l2tail_rows_expand as its own launch (mg_expand_column_reduce_f32) - for a backward pass that turns
    out not to run the launch the tail was meant to ride in; of f0_l2tail(defer=True): its reduce launch (mg_slab_reduce_f32)."""
    if tail.get('rows') is None:
        slab_reduce(tail['ws'], tail['n_slabs'], tail['stride'], tail['n'], tail['grads_out'])
        return
    _lib.check(_lib.load().mg_expand_column_reduce_f32(_p(tail['pred_rows']), _p(tail['rows']), tail['rows'].numel(), _p(tail['out']),
                                                        _p(tail['partials']), tail['n_table_rows'], tail['extra'], _p(tail['ws']), tail['n'],
                                                        tail['stride'], tail['n_slabs'], _p(tail['grads_out']), _stream()),
               'mg_expand_column_reduce_f32')


def slab_reduce(slab, n_slabs, stride, count, dst, accumulate=False):
    """dst[:count] (+)= ordered sum of the n_slabs slabs (f32, ``stride`` floats apart) in ``slab`` (a byte or float buffer): the reduce
    launch of linear_wgrad_bf16 on slabs taken from linear_wgrad_slabs_bf16 / linear_wgrad_dgrad_bf16 (mg_slab_reduce_f32)."""
    dst = _require(dst, torch.float32, 'dst')
    if dst.numel() < count:
        raise ValueError('slab_reduce: destination of %d floats for %d sums' % (dst.numel(), count))
    _lib.check(_lib.load().mg_slab_reduce_f32(_p(slab), int(n_slabs), int(stride), int(count), _p(dst), int(bool(accumulate)), _stream()),
               'mg_slab_reduce_f32')
    return dst


def can_fuse_bwd(m, n2, n_hidden, k0, lda0):
    """Shapes mg_linear_bwd_fused_bf16 handles (the README F0Model's first two layers at training batch sizes)."""
    return n2 == 128 and n_hidden % 128 == 0 and 512 < k0 <= 608 and lda0 == 640 and m >= 4096


def linear_bwd_fused_bf16(dz2, wt2, h1, a, rows, m, n_hidden, k0, out_w=None, out_b=None, accumulate=False):
    """dW, db of Linear(k0 -> n_hidden)+Sigmoid from dz2 = dL/d(pre-activation of the following Linear(n_hidden -> 128))."""
    lib = _lib.load()
    dw = out_w if out_w is not None else torch.empty((n_hidden, k0), dtype=torch.float32, device=dz2.device)
    db = out_b if out_b is not None else torch.empty((n_hidden,), dtype=torch.float32, device=dz2.device)
    nbytes = lib.mg_linear_bwd_fused_workspace_bytes(m, n_hidden, k0)
    ws = workspace(nbytes, dz2.device)
    _lib.check(lib.mg_linear_bwd_fused_bf16(_p(dz2), dz2.shape[1], 128, _p(wt2), wt2.shape[1], _p(h1), h1.shape[1], _p(a),
                                            a.shape[1], _p(rows), m, n_hidden, k0, _p(dw), _p(db), int(bool(accumulate)), _p(ws), ws.numel(),
                                            _stream()), 'mg_linear_bwd_fused_bf16')
    return dw, db


def linear_bwd_fused_slabs_bf16(dz2, wt2, h1, a, rows, m, n_hidden, k0, slab=None):
    """linear_bwd_fused_bf16 without the reduce (mg_linear_bwd_fused_slabs_bf16): returns (slab buffer, n_slabs, stride) for the
    optimiser's update kernel to sum; ``slab`` = a buffer to reuse (kept by the caller until the optimiser has consumed it)."""
    lib = _lib.load()
    nbytes = lib.mg_linear_bwd_fused_workspace_bytes(m, n_hidden, k0)
    slab = _slab_buffer(slab, nbytes, dz2.device)
    n_slabs, stride = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(lib.mg_linear_bwd_fused_slabs_bf16(_p(dz2), dz2.shape[1], 128, _p(wt2), wt2.shape[1], _p(h1), h1.shape[1], _p(a), a.shape[1],
                                                  _p(rows), m, n_hidden, k0, _p(slab), slab.numel(), ctypes.byref(n_slabs),
                                                  ctypes.byref(stride), _stream()), 'mg_linear_bwd_fused_slabs_bf16')
    return slab, n_slabs.value, stride.value


def linear_bwd_fused2_slabs_bf16(dz2, wt2, h1, a, rows, m, n_hidden, k0, slab=None):
    """The fused backward with the second layer's weight gradient riding along (mg_linear_bwd_fused2_slabs_bf16): ONE launch leaves the
    split-M slabs of (dW1 | db1) and of (dW2 | db2) of a Linear(k0 -> n_hidden) + Sigmoid -> Linear(n_hidden -> 128) pair whose input
    is gathered through ``rows``.  Returns (slab buffer, n_slabs, (float offset, stride, count) of the first layer's slabs, the same
    for the second layer's): slab i of a layer starts at float offset + i * stride and holds ``count`` partial sums."""
    lib = _lib.load()
    if rows is None:
        raise ValueError('linear_bwd_fused2_slabs_bf16 needs the row map of the gathered input')
    nbytes = lib.mg_linear_bwd_fused2_workspace_bytes(m, n_hidden, k0)
    slab = _slab_buffer(slab, nbytes, dz2.device)
    n_slabs, stride1, off2, stride2 = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.mg_linear_bwd_fused2_slabs_bf16(_p(dz2), dz2.shape[1], 128, _p(wt2), wt2.shape[1], _p(h1), h1.shape[1], _p(a), a.shape[1],
                                                   _p(rows), m, n_hidden, k0, _p(slab), slab.numel(), ctypes.byref(n_slabs),
                                                   ctypes.byref(stride1), ctypes.byref(off2), ctypes.byref(stride2), _stream()),
               'mg_linear_bwd_fused2_slabs_bf16')
    return (slab, n_slabs.value, (0, stride1.value, n_hidden * k0 + n_hidden), (off2.value, stride2.value, 128 * n_hidden + 128))


def copy_many(pairs):
    """dst.copy_(src) for every (dst, src) pair of equal-sized contiguous device tensors, MG_COPY_MAX pairs per launch (mg_copy_many):
    the tensors of a new batch into a captured step's static buffers as one launch instead of one per tensor."""
    lib = _lib.load()
    pairs = list(pairs)
    for i in range(0, len(pairs), _lib.MG_COPY_MAX):
        chunk = pairs[i:i + _lib.MG_COPY_MAX]
        descs = (_lib.mg_copy_desc * len(chunk))()
        for j, (dst, src) in enumerate(chunk):
            if (not dst.is_cuda or not src.is_cuda or dst.device != src.device or not dst.is_contiguous() or not src.is_contiguous()
                    or dst.dtype != src.dtype or dst.numel() != src.numel()):
                raise ValueError('copy_many: pairs of contiguous tensors of one device, dtype and size are required')
            descs[j].src, descs[j].dst, descs[j].bytes = src.data_ptr(), dst.data_ptr(), src.numel() * src.element_size()
        _lib.check(lib.mg_copy_many(ctypes.cast(descs, ctypes.c_void_p), len(chunk), _stream()), 'mg_copy_many')


def cast_params_bf16(weights, want_plain=True, want_t=()):
    """One launch: bf16 copies [N, pad_ld(K)] of every fp32 weight and, for the indices in `want_t`, the transposed
    copies [K, pad_ld(N)].  Returns (plain list, transposed list with None where not requested)."""
    lib = _lib.load()
    if len(weights) > _lib.MG_CAST_MAX:
        raise ValueError('cast_params_bf16: at most %d matrices per call' % _lib.MG_CAST_MAX)
    descs = (_lib.mg_cast_desc * len(weights))()
    plain, trans = [], []
    for i, w in enumerate(weights):
        w = _require(w, torch.float32, 'weight')
        n, k = w.shape
        wb = torch.empty((n, pad_ld(k)), dtype=torch.bfloat16, device=w.device) if want_plain else None
        wt = torch.empty((k, pad_ld(n)), dtype=torch.bfloat16, device=w.device) if i in want_t else None
        descs[i].src, descs[i].rows, descs[i].cols = w.data_ptr(), n, k
        descs[i].dst, descs[i].ldd = (wb.data_ptr() if wb is not None else None), (wb.shape[1] if wb is not None else 0)
        descs[i].dst_t, descs[i].ldt = (wt.data_ptr() if wt is not None else None), (wt.shape[1] if wt is not None else 0)
        plain.append(wb)
        trans.append(wt)
    _lib.check(lib.mg_cast_params_bf16(ctypes.cast(descs, ctypes.c_void_p), len(weights), _stream()),
               'mg_cast_params_bf16')
    return plain, trans


WEIGHT_SHADOWS = os.environ.get('MORGANA_WEIGHT_SHADOWS', '1') != '0'      # A/B: 0 = a cast launch per weight and step, as before


def weight_operands(weights, transposed=False):
    """bf16 operands ([N, pad_ld(K)], or the transposes [K, pad_ld(N)]) of a list of fp32 weights: the shadows that live on the
    parameters (param_shadows: kept current by the optimiser's update kernel, stale ones re-cast by ONE batched launch), or a cast
    launch each (MORGANA_WEIGHT_SHADOWS=0)."""
    weights = list(weights)
    if not WEIGHT_SHADOWS:
        return [cast_transpose_bf16(w) if transposed else cast_pad_bf16(_require(w, torch.float32, 'weight')) for w in weights]
    out = []
    for i in range(0, len(weights), _lib.MG_CAST_MAX):      # mg_cast_params_bf16 takes at most MG_CAST_MAX descriptors per launch
        part = weights[i:i + _lib.MG_CAST_MAX]
        plain, trans = param_shadows(part, want_t=tuple(range(len(part))) if transposed else ())
        out += trans if transposed else plain
    return out


def mark_updated(param):
    """A parameter's storage was written by something torch's version counter does not see (a HIP kernel on ``param.data``, a
    collective on ``param.data``): its bf16 operand copies (param_shadows) are stale from here on."""
    param._mg_updates = getattr(param, '_mg_updates', 0) + 1


def param_shadows(weights, want_t=()):
    """bf16 operands of a run of fp32 weight matrices: ([N, pad_ld(K)] copies, transposes [K, pad_ld(N)] for the indices in
    ``want_t``, None elsewhere).  The copies live ON the parameter (``w._mg_shadow``) and are kept current by
    ``morgana_amd.optim.Adam``'s update kernel, which re-casts every weight it has just changed (mg_adam_step_plan_f32), so a training
    step launches no cast at all; a weight changed by anything else (``load_state_dict``, another optimiser: its torch version
    counter moves; or one of our updates that did not refresh it: ``_mg_updates`` moves) is simply cast again here."""
    stale = []
    for i, w in enumerate(weights):
        sh = getattr(w, '_mg_shadow', None)
        ok = (sh is not None and sh['version'] == (w._version, getattr(w, '_mg_updates', 0)) and sh['plain'].device == w.device
              and (i not in want_t or sh['t'] is not None))
        if not ok:
            stale.append(i)
    if stale:
        descs = (_lib.mg_cast_desc * len(stale))()
        for j, i in enumerate(stale):
            w = _require(weights[i], torch.float32, 'weight')
            n, k = w.shape
            old = getattr(w, '_mg_shadow', None)
            plain = old['plain'] if old is not None and old['plain'].device == w.device else \
                torch.zeros((n, pad_ld(k)), dtype=torch.bfloat16, device=w.device)
            trans = old['t'] if old is not None and old['t'] is not None and old['t'].device == w.device else None
            if trans is None and i in want_t:
                trans = torch.zeros((k, pad_ld(n)), dtype=torch.bfloat16, device=w.device)
            descs[j].src, descs[j].rows, descs[j].cols = w.data_ptr(), n, k
            descs[j].dst, descs[j].ldd = plain.data_ptr(), plain.shape[1]
            descs[j].dst_t, descs[j].ldt = (trans.data_ptr(), trans.shape[1]) if trans is not None else (None, 0)
            w._mg_shadow = {'plain': plain, 't': trans, 'version': (w._version, getattr(w, '_mg_updates', 0))}
        _lib.check(_lib.load().mg_cast_params_bf16(ctypes.cast(descs, ctypes.c_void_p), len(stale), _stream()), 'mg_cast_params_bf16')
    return [w._mg_shadow['plain'] for w in weights], [w._mg_shadow['t'] if i in want_t else None for i, w in enumerate(weights)]


def invalidate_operand_copies(params):
    """Mark every operand copy of ``params`` stale - bf16 copies (param_shadows), pair planes (pair_shadows), 'bf16x3' splits
    (x3_weight_operands): the next reader casts or splits it again.  For a HIP-graph capture that failed
    (graphs.GraphedTrainStep): the casts it recorded never ran, the stamps it set say they did."""
    for p in params:
        for attr in ('_mg_shadow', '_mg_pair', '_mg_x3'):
            sh = getattr(p, attr, None)
            if sh is not None:
                sh['version'] = None


def refresh_shadows(params):
    """Re-cast the EXISTING bf16 operand copies of ``params`` (plain, and transposed where one is allocated) from their fp32 weights:
    one batched launch per MG_CAST_MAX parameters on the current stream, no allocation, no stamp (the caller stamps).  Used by
    ``optim.Adam`` for the copies its update kernel's plan has no room for, so that EVERY copy is current when an update ends -
    inside a captured step as well, where nothing on the host can notice a stale copy later."""
    lib = _lib.load()
    for i in range(0, len(params), _lib.MG_CAST_MAX):
        chunk = params[i:i + _lib.MG_CAST_MAX]
        descs = (_lib.mg_cast_desc * len(chunk))()
        for j, w in enumerate(chunk):
            sh = w._mg_shadow
            n, k = w.shape
            descs[j].src, descs[j].rows, descs[j].cols = w.data_ptr(), n, k
            descs[j].dst, descs[j].ldd = sh['plain'].data_ptr(), sh['plain'].shape[1]
            descs[j].dst_t, descs[j].ldt = (sh['t'].data_ptr(), sh['t'].shape[1]) if sh['t'] is not None else (None, 0)
        _lib.check(lib.mg_cast_params_bf16(ctypes.cast(descs, ctypes.c_void_p), len(chunk), _stream()), 'mg_cast_params_bf16')


# ------------------------------------------------------------------------------------------------------------------ active dropout
_dropout_state = {}      # device index -> int64 (1,) step counter on the device (mg_dropout_advance increments it per call)


def dropout_seed():
    """The 64-bit key of the dropout masks: torch's seed (``torch.manual_seed`` makes runs repeatable, as it does for nn.Dropout)."""
    return int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF


def dropout_state(device):
    """The device's dropout step counter (created on first use, OUTSIDE any stream capture: a counter zero-filled inside a capture would
    live in the graph's private pool and be reset by every replay - all replays would then draw the same masks, silently)."""
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    state = _dropout_state.get(index)
    if state is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('dropout: the device step counter does not exist yet and cannot be created inside a stream capture (every '
                               'replay would reset it and repeat its masks): call morgana_amd.ops.dropout_state(device) - or run one eager '
                               'step - before the capture (graphs.GraphedTrainStep does)')
        state = _dropout_state[index] = torch.zeros(1, dtype=torch.int64, device=device)
    return state


def dropout_draw(device):
    """Reserve one draw of the device's dropout step counter: returns a (1,) int64 device tensor holding the counter value this call
    (and its backward) uses; the device counter moves on in stream order - also inside a replayed HIP graph (csrc/dropout.hip)."""
    state = dropout_state(device)
    used = torch.empty(1, dtype=torch.int64, device=device)
    _lib.check(_lib.load().mg_dropout_advance(_p(state), _p(used), _stream()), 'mg_dropout_advance')
    return used


def dropout(x, p, seed, site, used, out=None):
    """y = x * keep / (1 - p) with the mask of (seed, site, used[0], element index) - mg_dropout.  x: contiguous fp32 or bf16; ``out``
    may be x (in place).  The same call on a gradient with the same (seed, site, used) is the backward."""
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
        raise TypeError('dropout: a contiguous float32 or bfloat16 tensor is required')
    y = torch.empty_like(x) if out is None else out
    _lib.check(_lib.load().mg_dropout(_p(x), _p(y), x.numel(), int(x.dtype == torch.bfloat16), float(p), int(seed), int(site) & 0xFFFFFFFF,
                                      _p(used), _stream()), 'mg_dropout')
    return y


# ------------------------------------------------------------------------------------------------ latent-conditioned models (VAE)
SAMPLE_SITE = 0x56414500     # the Philox site of the VAE sampler's noise (dropout masks use the module index of their layer)
SPHERE_SITE = 0x53504800     # the Philox sites of sampling.UniformSphereSurfaceSampler's noise ...
ELLIPSOID_SITE = 0x454C4C00  # ... and of sampling.UniformEllipsoidSurfaceApproximateSampler's angles: three streams, never one
MDN_COMPONENT_SITE = 0x4D444300   # mdn_sample: the uniform that picks a frame's mixture component ...
MDN_NOISE_SITE = 0x4D444E00       # ... and the N(0, 1) noise around its mean: two more streams, independent of each other


def _latent_rows(t, name):
    """(rows, Z) f32 view of ``t`` with unit column stride (a column view of a wider row stays a view) and its row stride."""
    _require(t[..., :0], torch.float32, name)                  # type and device only: the view itself may be strided
    t2 = t.reshape(-1, t.shape[-1]) if t.dim() != 2 else t
    if t2.stride(-1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < t2.shape[1]):
        t2 = t2.contiguous()
    return t2, (t2.stride(0) if t2.shape[0] > 1 else t2.shape[1])


def vae_sample(mean, logvar, seed, site, used):
    """z = mean + exp(0.5 logvar) eps with eps ~ N(0, 1) drawn from (seed, site, used[0], element) - mg_vae_sample_f32.  mean, logvar:
    (..., Z) f32, column views allowed.  Returns (z, eps), both contiguous with mean's shape."""
    if tuple(mean.shape) != tuple(logvar.shape):
        raise ValueError('vae_sample: mean %s and log_variance %s differ in shape' % (tuple(mean.shape), tuple(logvar.shape)))
    m2, ldm = _latent_rows(mean, 'mean')
    v2, ldv = _latent_rows(logvar, 'log_variance')
    z = torch.empty(tuple(mean.shape), dtype=torch.float32, device=mean.device)
    eps = torch.empty_like(z)
    _lib.check(_lib.load().mg_vae_sample_f32(_p(m2), ldm, _p(v2), ldv, m2.shape[0], m2.shape[1], int(seed), int(site) & 0xFFFFFFFF, _p(used),
                                             _p(z), _p(eps), _stream()), 'mg_vae_sample_f32')
    return z, eps


def vae_sample_backward(dz, eps, logvar):
    """(dmean, dlogvar) of vae_sample: dz and 0.5 dz eps exp(0.5 logvar) - mg_vae_sample_bwd_f32."""
    dz = _require(dz, torch.float32, 'gradient')
    v2, ldv = _latent_rows(logvar, 'log_variance')
    dmean = torch.empty_like(eps)
    dlogvar = torch.empty_like(eps)
    _lib.check(_lib.load().mg_vae_sample_bwd_f32(_p(dz), _p(eps), _p(v2), ldv, v2.shape[0], v2.shape[1], _p(dmean), _p(dlogvar), _stream()),
               'mg_vae_sample_bwd_f32')
    return dmean, dlogvar


def kld_standard_normal(mean, logvar):
    """mean over the leading dims of -0.5 sum_z (1 + logvar - mean^2 - exp(logvar)): a 0-dim f32 device tensor (mg_kld_standard_normal_f32)."""
    if tuple(mean.shape) != tuple(logvar.shape):
        raise ValueError('KLD_standard_normal: mean %s and log_variance %s differ in shape' % (tuple(mean.shape), tuple(logvar.shape)))
    m2, ldm = _latent_rows(mean, 'mean')
    v2, ldv = _latent_rows(logvar, 'log_variance')
    out = torch.empty((), dtype=torch.float32, device=mean.device)
    _lib.check(_lib.load().mg_kld_standard_normal_f32(_p(m2), ldm, _p(v2), ldv, m2.shape[0], m2.shape[1], _p(out), _stream()),
               'mg_kld_standard_normal_f32')
    return out


def kld_standard_normal_backward(grad, mean, logvar):
    """(dmean, dlogvar) = (g mean / rows, g 0.5 (exp(logvar) - 1) / rows) with g = grad (a 1-element device tensor, read on the device)."""
    grad = _require(grad.reshape(1), torch.float32, 'gradient')
    m2, ldm = _latent_rows(mean, 'mean')
    v2, ldv = _latent_rows(logvar, 'log_variance')
    dmean = torch.empty(tuple(mean.shape), dtype=torch.float32, device=mean.device)
    dlogvar = torch.empty_like(dmean)
    _lib.check(_lib.load().mg_kld_standard_normal_bwd_f32(_p(grad), _p(m2), ldm, _p(v2), ldv, m2.shape[0], m2.shape[1], _p(dmean), _p(dlogvar),
                                                          _stream()), 'mg_kld_standard_normal_bwd_f32')
    return dmean, dlogvar


# --------------------------------------------------------------------------------------------- vector quantisation (csrc/vq.hip)
VQ_EMA_EPS = 1e-5


def _vq_rows(z, name, seq_len=None):
    """``z`` (N, D) or (B, S, D) float32 -> (the tensor the kernel reads in place, row stride, N, D, S, seq_len): unit column
    stride and evenly spaced rows (a column slice of a wider tensor) stay views, anything else becomes a contiguous copy."""
    _require(z[..., :0], torch.float32, name)                  # type and device only: the view itself may be strided
    if z.dim() not in (2, 3) or 0 in z.shape:
        raise ValueError('%s must be a non-empty (N, D) or (B, S, D) tensor, got %s' % (name, tuple(z.shape)))
    if seq_len is not None and z.dim() != 3:
        raise ValueError('%s must be (B, S, D) when seq_len is given, got %s' % (name, tuple(z.shape)))
    d = z.shape[-1]
    if z.dim() == 3:
        b, s, _ = z.shape
        ld = z.stride(1) if s > 1 else (z.stride(0) if b > 1 else d)
        even = (z.stride(2) == 1 or d == 1) and ld >= d and (b == 1 or s == 1 or z.stride(0) == s * ld)
        n = b * s
    else:
        b, s, n = 1, z.shape[0], z.shape[0]
        ld = z.stride(0) if n > 1 else d
        even = (z.stride(1) == 1 or d == 1) and ld >= d
    if not even:
        z, ld = z.contiguous(), d
    return z, ld, n, d, s, _lengths(seq_len, b)


def _vq_codebook(codebook, d):
    codebook = _require(codebook, torch.float32, 'codebook')
    if codebook.dim() != 2 or codebook.shape[0] == 0 or codebook.shape[1] != d:
        raise ValueError('codebook must be (K, D) with D = %d, got %s' % (d, tuple(codebook.shape)))
    return codebook


def vq_assign(z, codebook, seq_len=None, counts=None):
    """Nearest code of every row (mg_vq_assign_f32, csrc/vq.hip): z (N, D) or (B, S, D) float32, read in place through its row stride;
    codebook (K, D) float32; seq_len (B,) int64 or None - the rows at or past seq_len[b] are never read.  Returns (index int64,
    shaped like z without its last dimension, -1 on pad rows; quantised, contiguous, shaped like z, ``codebook[index]`` bit for bit
    and zero on pad rows; vq 0-d float32, the mean squared distance to the chosen code; counts (K,) int32; perplexity 0-d float32;
    n_valid 0-d int64 for ``vq_backward``).  Distances are float64 sums of direct differences; ties go to the lowest index.
    ``counts``: a contiguous (K,) int32 device tensor of the caller's to fill in place of a new one."""
    lib = _lib.load()
    z2, ld, n, d, s, seq_len = _vq_rows(z, 'z', seq_len)
    codebook = _vq_codebook(codebook, d)
    k, dev = codebook.shape[0], z2.device
    index = torch.empty(tuple(z.shape[:-1]), dtype=torch.int64, device=dev)
    quantised = torch.empty(tuple(z.shape), dtype=torch.float32, device=dev)
    vq = torch.empty((), dtype=torch.float32, device=dev)
    perplexity = torch.empty((), dtype=torch.float32, device=dev)
    if counts is None:
        counts = torch.empty((k,), dtype=torch.int32, device=dev)
    elif _require(counts, torch.int32, 'counts', contiguous=False).shape != (k,) or not counts.is_contiguous():
        raise ValueError('vq_assign: counts must be a contiguous (K,) = (%d,) int32 tensor, got %s' % (k, tuple(counts.shape)))
    n_valid = torch.empty((), dtype=torch.int64, device=dev)
    ws = workspace(lib.mg_vq_workspace_bytes(n, k), dev)
    _lib.check(lib.mg_vq_assign_f32(_p(z2), ld, n, d, _p(seq_len), s, _p(codebook), k, _p(index), _p(quantised), _p(vq), _p(counts),
                                    _p(perplexity), _p(n_valid), _p(ws), ws.numel(), _stream()), 'mg_vq_assign_f32')
    return index, quantised, vq, counts, perplexity, n_valid


def vq_backward(grad_latent, grad_loss, z, quantised, index, n_valid, n_codes, codebook_weight, commitment_weight, want_dz=True,
                want_de=True):
    """The gradients of ``vq_assign``'s loss and straight-through latent (mg_vq_bwd_f32) -> (dz shaped like z, dE (n_codes, D)), either
    None when not wanted.  dz = grad_latent + grad_loss * commitment_weight * 2 (z - q) / (N_valid D), zero on pad rows; dE[k] =
    grad_loss * codebook_weight * 2 sum_{index == k} (q - z) / (N_valid D), members in ascending order, exactly 0 for an unused
    code.  ``grad_latent`` may be None; ``grad_loss`` is a one-element float32 device tensor that the kernel reads (no host read);
    z, quantised, index, n_valid as ``vq_assign`` took and left them (the codebook is not needed: quantised holds its rows)."""
    lib = _lib.load()
    grad_loss = _one_element(grad_loss)
    z2, ld, n, d, _, _ = _vq_rows(z, 'z')
    quantised = _require(quantised, torch.float32, 'quantised')
    index = _require(index, torch.int64, 'index')
    n_valid = _require(n_valid, torch.int64, 'n_valid')
    if tuple(quantised.shape) != tuple(z.shape) or tuple(index.shape) != tuple(z.shape[:-1]) or n_valid.numel() != 1:
        raise ValueError('vq_backward: quantised %s and index %s do not go with z %s' % (tuple(quantised.shape), tuple(index.shape),
                                                                                        tuple(z.shape)))
    if grad_latent is not None:
        grad_latent = _require(grad_latent, torch.float32, 'grad_latent')
        if tuple(grad_latent.shape) != tuple(z.shape):
            raise ValueError('vq_backward: grad_latent %s must be shaped like z %s' % (tuple(grad_latent.shape), tuple(z.shape)))
    if not (want_dz or want_de):
        return None, None
    dev = z2.device
    dz = torch.empty(tuple(z.shape), dtype=torch.float32, device=dev) if want_dz else None
    de = torch.empty((int(n_codes), d), dtype=torch.float32, device=dev) if want_de else None
    _lib.check(lib.mg_vq_bwd_f32(_p(grad_latent), _p(grad_loss), _p(z2), ld, _p(quantised), _p(index), _p(n_valid), n, d, int(n_codes),
                                 float(codebook_weight), float(commitment_weight), _p(dz), _p(de), _stream()), 'mg_vq_bwd_f32')
    return dz, de


def vq_ema_update(z, index, counts, cluster_size, ema_sum, codebook, decay, eps=VQ_EMA_EPS):
    """The EMA codebook update (mg_vq_ema_f32), IN PLACE on cluster_size (K,), ema_sum (K, D) and codebook (K, D), all float32 and
    contiguous: cluster_size <- decay cluster_size + (1 - decay) counts, ema_sum <- decay ema_sum + (1 - decay) (sum of the rows
    assigned to each code, ascending, float64), codebook <- ema_sum / the Laplace-smoothed cluster size.  z, index and counts as
    ``vq_assign`` took and left them."""
    lib = _lib.load()
    z2, ld, n, d, _, _ = _vq_rows(z, 'z')
    index = _require(index, torch.int64, 'index')
    counts = _require(counts, torch.int32, 'counts')
    k = counts.numel()
    for name, t, shape in (('cluster_size', cluster_size, (k,)), ('ema_sum', ema_sum, (k, d)), ('codebook', codebook, (k, d))):
        if _require(t, torch.float32, name, contiguous=False).shape != shape or not t.is_contiguous():
            raise ValueError('vq_ema_update: %s must be a contiguous %s tensor (updated in place), got %s' % (name, shape, tuple(t.shape)))
    if tuple(index.shape) != tuple(z.shape[:-1]) or k == 0:
        raise ValueError('vq_ema_update: index %s does not go with z %s' % (tuple(index.shape), tuple(z.shape)))
    ws = workspace(8, z2.device)                               # one float64: the sum of the new cluster sizes
    _lib.check(lib.mg_vq_ema_f32(_p(z2), ld, _p(index), _p(counts), n, d, k, float(decay), float(eps), _p(cluster_size), _p(ema_sum),
                                 _p(codebook), _p(ws), ws.numel(), _stream()), 'mg_vq_ema_f32')


# ------------------------------------------------------------------------------------------- latent surface samplers (sampling)
def _site_args(seed, site, used):
    return int(seed), int(site) & 0xFFFFFFFF, _p(used)


def sphere_sample(centre, radius, rows, seed, site, used):
    """``rows`` points on the sphere's surface: out = centre + radius g / |g|, g ~ N(0, 1) drawn from (seed, site, used[0], element) -
    mg_sphere_sample_f32.  centre: (D,) f32; radius: a 1-element f32 DEVICE tensor.  Returns (out, unit), both (rows, D); unit = g / |g|
    is what the backward needs."""
    centre = _require(centre, torch.float32, 'centre')
    radius = _require(radius, torch.float32, 'radius')
    if centre.dim() != 1 or radius.numel() != 1:
        raise ValueError('sphere_sample: centre must be (D,) and radius one element, got %s and %s' % (tuple(centre.shape), tuple(radius.shape)))
    out = torch.empty((int(rows), centre.shape[0]), dtype=torch.float32, device=centre.device)
    unit = torch.empty_like(out)
    _lib.check(_lib.load().mg_sphere_sample_f32(_p(centre), _p(radius), int(rows), centre.shape[0], *_site_args(seed, site, used), _p(out),
                                                _p(unit), _stream()), 'mg_sphere_sample_f32')
    return out, unit


def sphere_sample_backward(dout, unit):
    """(dcentre (D,), dradius (1,)) of sphere_sample: the column sums of dout and sum(dout * unit) - mg_sphere_sample_bwd_f32."""
    dout = _require(dout, torch.float32, 'gradient')
    unit = _require(unit, torch.float32, 'unit')
    if dout.dim() != 2 or tuple(dout.shape) != tuple(unit.shape):
        raise ValueError('sphere_sample_backward: gradient %s and unit %s must be one (rows, D) shape' % (tuple(dout.shape), tuple(unit.shape)))
    dcentre = torch.empty(dout.shape[1], dtype=torch.float32, device=dout.device)
    dradius = torch.empty(1, dtype=torch.float32, device=dout.device)
    _lib.check(_lib.load().mg_sphere_sample_bwd_f32(_p(dout), _p(unit), dout.shape[0], dout.shape[1], _p(dcentre), _p(dradius), _stream()),
               'mg_sphere_sample_bwd_f32')
    return dcentre, dradius


def ellipsoid_sample(radii, rows, seed, site, used):
    """``rows`` points on the ellipsoid's surface from D - 1 uniform angles each: out = radii * factor, factor[n] = prod_{j < n}
    sin(angle_j) * cos(angle_n) - mg_ellipsoid_sample_f32.  radii: (D,) f32, D >= 2.  Returns (out, factor), both (rows, D)."""
    radii = _require(radii, torch.float32, 'radii')
    if radii.dim() != 1:
        raise ValueError('ellipsoid_sample: radii must be (D,), got %s' % (tuple(radii.shape),))
    out = torch.empty((int(rows), radii.shape[0]), dtype=torch.float32, device=radii.device)
    factor = torch.empty_like(out)
    _lib.check(_lib.load().mg_ellipsoid_sample_f32(_p(radii), int(rows), radii.shape[0], *_site_args(seed, site, used), _p(out), _p(factor),
                                                   _stream()), 'mg_ellipsoid_sample_f32')
    return out, factor


def ellipsoid_angles(rows, ndims, device, seed, site, used):
    """The (rows, ndims - 1) angles ellipsoid_sample draws from the same (seed, site, used[0]) - mg_ellipsoid_angles_f32."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.MorganaHipError('angles on %s: the morgana_amd ops run only on an MI355X device (no CPU fallback)' % device)
    angles = torch.empty((int(rows), max(int(ndims) - 1, 0)), dtype=torch.float32, device=device)
    _lib.check(_lib.load().mg_ellipsoid_angles_f32(int(rows), int(ndims), *_site_args(seed, site, used), _p(angles), _stream()),
               'mg_ellipsoid_angles_f32')
    return angles


def ellipsoid_sample_backward(dout, factor):
    """dradii (D,) of ellipsoid_sample: the column sums of dout * factor - mg_ellipsoid_sample_bwd_f32."""
    dout = _require(dout, torch.float32, 'gradient')
    factor = _require(factor, torch.float32, 'factor')
    if dout.dim() != 2 or tuple(dout.shape) != tuple(factor.shape):
        raise ValueError('ellipsoid_sample_backward: gradient %s and factor %s must be one (rows, D) shape'
                         % (tuple(dout.shape), tuple(factor.shape)))
    dradii = torch.empty(dout.shape[1], dtype=torch.float32, device=dout.device)
    _lib.check(_lib.load().mg_ellipsoid_sample_bwd_f32(_p(dout), _p(factor), dout.shape[0], dout.shape[1], _p(dradii), _stream()),
               'mg_ellipsoid_sample_bwd_f32')
    return dradii


def gather_concat_latent(src2d, rows, extra2d, z2d, rows_per_item, out_bf16=False):
    """[src2d[rows] | extra2d | z2d[m / rows_per_item]] per row (mg_gather_concat_latent_*): f32 (M, F+C+Z), or bf16 (M, pad_ld(F+C+Z))
    zero padded.  rows None: src2d is already one row per output row; extra2d None: no frame features (C = 0)."""
    lib = _lib.load()
    src2d = _require(src2d, torch.float32, 'src')
    z2d = _require(z2d, torch.float32, 'latent')
    rows = _require(rows, torch.int32, 'rows') if rows is not None else None
    extra2d = _require(extra2d, torch.float32, 'extra') if extra2d is not None else None
    m = rows.numel() if rows is not None else src2d.shape[0]
    f, c, zd = src2d.shape[1], (extra2d.shape[1] if extra2d is not None else 0), z2d.shape[1]
    if extra2d is not None and extra2d.shape[0] != m:
        raise ValueError('gather_concat_latent: %d rows but %d rows of frame-level features' % (m, extra2d.shape[0]))
    if z2d.shape[0] * int(rows_per_item) != m:
        raise ValueError('gather_concat_latent: %d latent rows x %d rows per item != %d rows' % (z2d.shape[0], int(rows_per_item), m))
    if out_bf16:
        ldo = pad_ld(f + c + zd)
        out = torch.empty((m, ldo), dtype=torch.bfloat16, device=src2d.device)
        _lib.check(lib.mg_gather_concat_latent_bf16(_p(src2d), _p(rows), _p(extra2d), _p(z2d), _p(out), m, f, c, zd, int(rows_per_item), ldo,
                                                    _stream()), 'mg_gather_concat_latent_bf16')
    else:
        out = torch.empty((m, f + c + zd), dtype=torch.float32, device=src2d.device)
        _lib.check(lib.mg_gather_concat_latent_f32(_p(src2d), _p(rows), _p(extra2d), _p(z2d), _p(out), m, f, c, zd, int(rows_per_item), f + c + zd,
                                                   _stream()), 'mg_gather_concat_latent_f32')
    return out


def rows_add_per_item(p, u, rows, rows_per_item):
    """In place: p[r, :N] += u[r / rows_per_item, :N] for r < rows (mg_rows_add_per_item_f32); p, u f32 with unit column stride."""
    if p.dtype != torch.float32 or u.dtype != torch.float32 or p.stride(-1) != 1 or u.stride(-1) != 1 or not p.is_cuda or not u.is_cuda:
        raise TypeError('rows_add_per_item: f32 device tensors with unit column stride are required')
    n = u.shape[1]
    _lib.check(_lib.load().mg_rows_add_per_item_f32(_p(p), p.stride(0), int(rows), n, _p(u), u.stride(0), int(rows_per_item), _stream()),
               'mg_rows_add_per_item_f32')
    return p


def rows_sum_per_item(g, n_items, rows_per_item, n=None, h=None):
    """(n_items, n) f32: the sum of g's rows of every item (item b owns rows b rows_per_item ...), times h (1 - h) when h is given
    (mg_rows_sum_per_item).  g: f32 or bf16 (padded columns past n are not read), unit column stride; h: f32 like g."""
    if g.dtype not in (torch.float32, torch.bfloat16) or g.stride(-1) != 1 or not g.is_cuda:
        raise TypeError('rows_sum_per_item: an f32 or bf16 device tensor with unit column stride is required')
    n = g.shape[1] if n is None else int(n)
    if h is not None:
        h = _require(h, torch.float32, 'sigmoid output')
    s = torch.empty((int(n_items), n), dtype=torch.float32, device=g.device)
    _lib.check(_lib.load().mg_rows_sum_per_item(_p(g), g.stride(0), int(g.dtype == torch.bfloat16), _p(h), h.stride(0) if h is not None else 0,
                                                int(n_items), int(rows_per_item), n, _p(s), n, _stream()), 'mg_rows_sum_per_item')
    return s


# ----------------------------------------------------------------------------------------- precision 'bf16x3' (split-bf16 operands)
CAPTURE_EPOCH = [0]      # bumped by graphs.GraphedTrainStep at the start of every capture (see x3_weight_operands)


def begin_capture_epoch():
    CAPTURE_EPOCH[0] += 1


SPLIT3_COLSUM_BLOCKS = int(os.environ.get('MORGANA_SPLIT3_COLSUM_BLOCKS', '512'))      # workgroups (= slabs) of a split that also sums its columns; C2 bf16x3 step by count: 64 0.555, 128 0.488, 256 0.458, 512 0.457, 1024 0.463, 2048 0.480 ms


def split3_colsum_ok(cols):
    """Plane widths whose 8-column chunks divide a 256-thread workgroup (mg_split3_bf16's column-sum form)."""
    return 256 % (pad_ld(cols) // 8) == 0


def split3(jobs):
    """Operand splits of precision mode 'bf16x3' (csrc/split3.hip): ``jobs`` = [(fp32 2-D tensor, order, transpose)] with order 0 =
    [hi | hi | lo] (activation side), 1 = [hi | lo | hi] (weight side), 2 = two separate planes, 3 / 4 = three row-stacked planes
    [hi ; hi ; lo] / [hi ; lo ; hi]; one batched launch per MG_SPLIT3_MAX jobs.  Returns one bf16 tensor per job: (rows, 3 ldp) -
    (cols, 3 ldp) with ``transpose`` - or (2 or 3, rows, ldp) for orders 2-4, where ldp = pad_ld(columns of a plane).  A job with a
    sixth element True (plain layouts) returns (planes, slabs): the per-workgroup column sums of the split values (``slab_reduce``)."""
    lib = _lib.load()
    outs = []
    for i in range(0, len(jobs), _lib.MG_SPLIT3_MAX):
        chunk = jobs[i:i + _lib.MG_SPLIT3_MAX]
        descs = (_lib.mg_split3_desc * len(chunk))()
        for j, job in enumerate(chunk):
            x, order, transpose = job[:3]
            extra = int(job[3]) if len(job) > 3 else 0          # zero rows appended behind the split (not with transpose)
            sig = job[4] if len(job) > 4 else None              # fp32 sigmoid outputs of x's shape: split x * s * (1 - s) instead of x
            want_colsum = bool(job[5]) if len(job) > 5 else False
            if sig is not None and (transpose or sig.dtype != torch.float32 or tuple(sig.shape) != tuple(x.shape) or sig.stride(1) != 1):
                raise ValueError('split3: the fused sigmoid gradient needs an fp32 tensor of the operand\'s shape (plain layouts)')
            if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
                raise TypeError('split3: operands must be 2-D float32 with unit column stride')
            if extra and transpose:
                raise ValueError('split3: extra zero rows go with the plain layouts')
            rows, cols = x.shape
            ldp = pad_ld(rows if transpose else cols)
            stacked = order >= 2
            out = torch.empty((2 if order == 2 else 3, rows + extra, ldp) if stacked else ((cols if transpose else rows) + extra, 3 * ldp),
                              dtype=torch.bfloat16, device=x.device)
            if extra:
                (out[:, rows:] if stacked else out[rows:]).zero_()
            descs[j].src, descs[j].rows, descs[j].cols, descs[j].lds = x.data_ptr(), rows, cols, x.stride(0)
            descs[j].dst, descs[j].ldp, descs[j].order, descs[j].transpose = out.data_ptr(), ldp, int(order), int(bool(transpose))
            descs[j].plane_rows = rows + extra if stacked else 0
            descs[j].sig, descs[j].ldsig = (sig.data_ptr(), sig.stride(0)) if sig is not None else (None, 0)
            if want_colsum:
                if transpose or 256 % (ldp // 8) != 0:
                    raise ValueError('split3: column sums go with the plain layouts and plane widths that divide 2048')
                slabs = torch.empty((SPLIT3_COLSUM_BLOCKS, ldp), dtype=torch.float32, device=x.device)
                descs[j].colsum, descs[j].colsum_blocks = slabs.data_ptr(), SPLIT3_COLSUM_BLOCKS
                outs.append((out, slabs))
            else:
                descs[j].colsum, descs[j].colsum_blocks = None, 0
                outs.append(out)
        if chunk:
            _lib.check(lib.mg_split3_bf16(ctypes.cast(descs, ctypes.c_void_p), len(chunk), _stream()), 'mg_split3_bf16')
    return outs


def x3_weight_operands(weights, want_t=()):
    """Weight-side operands of 'bf16x3' for a run of fp32 weight matrices [N, K]: ([N, 3 pad_ld(K)] splits in order 1, and for the
    indices in ``want_t`` the order-0 splits of W^T [K, 3 pad_ld(N)] (the dgrad operand, against gradients in order 1), None elsewhere).  Cached on the parameter
    under the same version stamps as the bf16 operand copies (param_shadows); every stale one is re-split by ONE batched launch."""
    jobs, slots = [], []
    # inside a stream capture a split that is current NOW says nothing about the replays: every step of a captured graph re-splits
    # the weights it reads (once per capture epoch and update count - graphs.GraphedTrainStep opens an epoch per capture)
    capturing = bool(weights) and weights[0].is_cuda and torch.cuda.is_current_stream_capturing()
    for i, w in enumerate(weights):
        st = getattr(w, '_mg_x3', None)
        stamp = (w._version, getattr(w, '_mg_updates', 0), CAPTURE_EPOCH[0] if capturing else -1)
        if st is None or st['version'] != stamp or st['plain'].device != w.device:
            st = w._mg_x3 = {'plain': None, 't': None, 'version': stamp}
        if st['plain'] is None:
            jobs.append((_require(w, torch.float32, 'weight'), 1, False))
            slots.append((st, 'plain'))
        if i in want_t and st['t'] is None:
            jobs.append((_require(w, torch.float32, 'weight'), 0, True))          # W^T [hi | hi | lo]: against gradients split [hi | lo | hi]
            slots.append((st, 't'))
    for (st, key), out in zip(slots, split3(jobs)):
        st[key] = out
    return [w._mg_x3['plain'] for w in weights], [w._mg_x3['t'] if i in want_t else None for i, w in enumerate(weights)]


def linear_fwd_x3(a3, rows, m, w3, bias, n, act):
    """fp32 (m, n) = act(gather(A, rows) W^T + bias) from split operands: a3 (R, 3 ldp) order 0, w3 (n, 3 ldp) order 1 - the bf16
    tile programs over a contraction index of 3 ldp (mg_linear_fwd_bf16, fp32 output)."""
    if a3.shape[1] != w3.shape[1]:
        raise ValueError('linear_fwd_x3: operand planes differ (%d vs %d columns)' % (a3.shape[1], w3.shape[1]))
    y = linear_fwd_bf16(a3, rows, m, a3.shape[1], w3, bias, n, act, out_f32=True)
    return y if y.shape[1] == n else y[:, :n].contiguous()


def linear_dgrad_x3(g3, m, wt3, k):
    """fp32 (m, k) = dY W from split operands: g3 (m, 3 ldp(n)) order 1 [hi | lo | hi], wt3 = split of W^T (k, 3 ldp(n)) order 0."""
    if g3.shape[1] != wt3.shape[1]:
        raise ValueError('linear_dgrad_x3: operand planes differ (%d vs %d columns)' % (g3.shape[1], wt3.shape[1]))
    dx = linear_dgrad_bf16(g3, m, g3.shape[1], wt3, k, None, out_f32=True)
    return dx if dx.shape[1] == k else dx[:, :k].contiguous()


def linear_wgrad_x3_rows(g1, colsum, a0, n, k, out_w=None, out_b=None, accumulate=False):
    """dW (n, k), db (n,) as ONE launch from the three-plane buffers the other products of the layer use anyway: g1 (m, 3 ldp(n)) = the
    gradient split [hi | lo | hi] (order 1), a0 (m, 3 ldp(k)) = the forward's activation split [hi | hi | lo] (order 0).  Read as
    (3 m, ldp) matrices they are row-interleaved stacks pairing (hi, hi), (lo, hi), (hi, lo): the three products of the weight
    gradient in one contraction over 3 m rows.  db = the ordered sum of ``colsum`` (split3's column sums of the fp32 gradient)."""
    lib = _lib.load()
    if g1.dim() != 2 or a0.dim() != 2 or g1.shape[0] != a0.shape[0] or g1.shape[1] % 3 or a0.shape[1] % 3:
        raise ValueError('linear_wgrad_x3_rows: operands must be three-plane buffers of equal row count')
    m3, ldn, ldk = 3 * g1.shape[0], g1.shape[1] // 3, a0.shape[1] // 3
    if out_w is None:
        both = torch.empty((n * k + n,), dtype=torch.float32, device=g1.device)
        dw, db = both[:n * k].view(n, k), (both[n * k:] if colsum is not None else None)
    else:
        dw, db = out_w, (out_b if colsum is not None else None)
    ws = workspace(lib.mg_linear_wgrad_workspace_bytes(m3, n, k), g1.device)
    _lib.check(lib.mg_linear_wgrad_bf16(_p(g1), ldn, _p(a0), ldk, None, m3, n, k, _p(dw), None, int(bool(accumulate)), _p(ws), ws.numel(),
                                        _stream()), 'mg_linear_wgrad_bf16')
    if db is not None:
        slab_reduce(colsum, colsum.shape[0], colsum.shape[1], n, db, accumulate=accumulate)
    return dw, db


def linear_wgrad_x3_stacked(g3, colsum, a3, n, k, out_w=None, out_b=None, accumulate=False):
    """dW (n, k), db (n,) of split operands as ONE launch: g3 (3, m, ldp(n)) = [hi ; hi ; lo] (split3 order 3), a3 (3, m, ldp(k)) =
    [hi ; lo ; hi] (order 4): [hi ; hi ; lo]^T [hi ; lo ; hi] over 3 m rows = the three products of ``linear_wgrad_x3``.  db = the
    ordered sum of ``colsum`` (the split pass's per-workgroup column sums of the fp32 gradient: exact), or None."""
    lib = _lib.load()
    if g3.shape[0] != 3 or a3.shape[0] != 3 or g3.shape[1] != a3.shape[1]:
        raise ValueError('linear_wgrad_x3_stacked: operands must be three row-stacked planes of equal row count')
    m3 = 3 * g3.shape[1]
    if out_w is None:
        both = torch.empty((n * k + n,), dtype=torch.float32, device=g3.device)
        dw, db = both[:n * k].view(n, k), (both[n * k:] if colsum is not None else None)
    else:
        dw, db = out_w, (out_b if colsum is not None else None)
    ws = workspace(lib.mg_linear_wgrad_workspace_bytes(m3, n, k), g3.device)
    _lib.check(lib.mg_linear_wgrad_bf16(_p(g3), g3.shape[2], _p(a3), a3.shape[2], None, m3, n, k, _p(dw), None, int(bool(accumulate)),
                                        _p(ws), ws.numel(), _stream()), 'mg_linear_wgrad_bf16')
    if db is not None:
        slab_reduce(colsum, colsum.shape[0], colsum.shape[1], n, db, accumulate=accumulate)
    return dw, db


def linear_wgrad_x3(g2, a2, rows, m, n, k, out_w=None, out_b=None, accumulate=False):
    """dW (n, k), db (n,) from split operands in separate planes (split3 order 2): g2 (2, m, ldp(n)), a2 (2, R, ldp(k)).  A weight
    gradient contracts over the ROWS, so the three products are three accumulating launches on plane pairs: hi^T hi (+ the bias
    sums of hi), hi^T lo, lo^T hi (+ the bias sums of lo)."""
    lib = _lib.load()
    if out_w is None:
        both = torch.empty((n * k + n,), dtype=torch.float32, device=g2.device)
        dw, db = both[:n * k].view(n, k), both[n * k:]
    else:
        dw, db = out_w, out_b
    ws = workspace(lib.mg_linear_wgrad_workspace_bytes(m, n, k), g2.device)
    plans = ((0, 0, True), (0, 1, False), (1, 0, True))                   # (dY plane, A plane, with bias sums)
    for idx, (gp, ap, with_b) in enumerate(plans):
        acc = int(bool(accumulate)) if idx == 0 else 1
        _lib.check(lib.mg_linear_wgrad_bf16(_p(g2[gp]), g2.shape[2], _p(a2[ap]), a2.shape[2], _p(rows), m, n, k, _p(dw),
                                            _p(db) if (with_b and db is not None) else None, acc, _p(ws), ws.numel(), _stream()),
                   'mg_linear_wgrad_bf16')
    return dw, db


# ------------------------------------------------------------------------------- precision 'bf16x3', the FUSED step on pair planes
# (include/morgana_hip.h, "The FUSED step of precision mode 'bf16x3' on PAIR PLANES").  A pair is a bf16 (rows, 2 ldp) buffer [hi | lo].
F0_TAIL_X3_SLAB = _lib.MG_F0_TAIL_X3_SLAB      # db2 128 | dW3 4096 | db3 32 | dW4 32 | db4 | loss | 2 unused
F0_TAIL_X3_N = F0_TAIL_X3_SLAB - 2     # ... up to and including the loss


def split_pair(x2d, transpose=False, extra_rows=0):
    """[hi | lo] pair planes of an fp32 matrix (mg_split3_bf16 order 5): (rows + extra_rows, 2 pad_ld(cols)) bf16, the extra rows zero;
    ``transpose``: the pair of x2d^T, (cols, 2 pad_ld(rows))."""
    lib = _lib.load()
    x2d = _require(x2d, torch.float32, 'operand')
    if x2d.dim() != 2:
        raise ValueError('split_pair: a 2-D operand is required')
    rows, cols = x2d.shape
    if transpose and extra_rows:
        raise ValueError('split_pair: extra zero rows go with the plain layout')
    ldp = pad_ld(rows if transpose else cols)
    out = torch.empty(((cols if transpose else rows) + extra_rows, 2 * ldp), dtype=torch.bfloat16, device=x2d.device)
    if extra_rows:
        out[rows:].zero_()
    descs = (_lib.mg_split3_desc * 1)()
    d = descs[0]
    d.src, d.rows, d.cols, d.lds = x2d.data_ptr(), rows, cols, x2d.stride(0)
    d.dst, d.ldp, d.order, d.transpose, d.plane_rows = out.data_ptr(), ldp, 5, int(bool(transpose)), 0
    d.sig, d.ldsig, d.colsum, d.colsum_blocks = None, 0, None, 0
    _lib.check(lib.mg_split3_bf16(ctypes.cast(descs, ctypes.c_void_p), 1, _stream()), 'mg_split3_bf16')
    return out


def pair_shadows(weights, want_t=()):
    """Pair-plane operands of a run of fp32 weight matrices: ([N, 2 pad_ld(K)] pairs, pairs of W^T [K, 2 pad_ld(N)] for the indices in
    ``want_t``, None elsewhere).  As ``param_shadows``: the pairs live ON the parameter (``w._mg_pair``), ``morgana_amd.optim.Adam``'s
    update kernel re-splits every weight it has just changed (mg_adam_shadow.pair), so a training step launches no split; a weight
    changed by anything else is split again here."""
    plain, trans = [], []
    for i, w in enumerate(weights):
        sh = getattr(w, '_mg_pair', None)
        ok = (sh is not None and sh['version'] == (w._version, getattr(w, '_mg_updates', 0)) and sh['plain'].device == w.device
              and (i not in want_t or sh['t'] is not None))
        if not ok:
            w32 = _require(w, torch.float32, 'weight')
            n, k = w32.shape
            old = sh if sh is not None and sh['plain'].device == w.device else None
            # re-split INTO the existing buffers (a captured graph reads them by address)
            new_plain = split_pair(w32.detach())
            if old is not None:
                old['plain'].copy_(new_plain)
                new_plain = old['plain']
            new_t = old['t'] if old is not None else None
            if i in want_t or new_t is not None:
                fresh = split_pair(w32.detach(), transpose=True)
                if new_t is not None:
                    new_t.copy_(fresh)
                else:
                    new_t = fresh
            w._mg_pair = {'plain': new_plain, 't': new_t, 'version': (w._version, getattr(w, '_mg_updates', 0))}
        plain.append(w._mg_pair['plain'])
        trans.append(w._mg_pair['t'] if i in want_t else None)
    return plain, trans


def x3_step_ok(n_table_rows, m, k0, n0, n1, extra=None):
    """Shapes of the fused 'bf16x3' phone-rate step: Linear(k0 -> 512) + Sigmoid, Linear(512 -> 128) on a phone table whose row
    count takes the wide weight-gradient tiles, k0's plane 640 or 512 columns wide."""
    extra = PHONE_RATE_EXTRA if extra is None else extra
    rows = n_table_rows + extra
    ldp = pad_ld(k0)
    return (n0 == 512 and n1 == 128 and 4096 <= rows and rows < m and
            ((ldp == 640 and 512 < k0 <= 640) or (ldp == 512 and 384 < k0 <= 512)))


def phone_front_x3(front, linear):
    """``phone_front`` with the first layer on PAIR PLANES: ``front`` = (dur, target, seq_len, t, extra) or None (the GEMM alone),
    ``linear`` = (a pair (M, 2 pa), k, w pair (n, 2 pw), bias, n, act).  Returns the front's six results (when asked for) + y, the pair
    (M, 2 n) of act(a w^T + bias) (mg_phone_front_linear_fwd_x3)."""
    lib = _lib.load()
    a, k, w2, bias, n, act = linear
    m = a.shape[0]
    y = torch.empty((m, 2 * n), dtype=torch.bfloat16, device=a.device)
    if front is None:
        _lib.check(lib.mg_phone_front_linear_fwd_x3(None, 0, 0, 0, None, None, 0, None, None, 0, None, None, None, None, None, 0,
                                                    _p(a), a.shape[1], m, k, _p(w2), w2.shape[1], _p(bias), n, _p(y), 2 * n, act, _stream()),
                   'mg_phone_front_linear_fwd_x3')
        return (y,)
    dur, target, seq_len, t, extra = front
    dur = _require(dur, torch.int64, 'dur')
    target = _require(target, torch.float32, 'targets')
    b, p = dur.shape
    if target.numel() != b * t:
        raise ValueError('phone_front_x3: %d targets for %d x %d frames' % (target.numel(), b, t))
    r = b * p
    rows = torch.empty((2, b, t), dtype=torch.int32, device=dur.device)
    seg = torch.empty((2, r), dtype=torch.int32, device=dur.device)
    stats = torch.empty((2, r + extra), dtype=torch.float32, device=dur.device)
    ws = torch.empty(lib.mg_phone_target_stats_workspace_bytes(r, extra), dtype=torch.uint8, device=dur.device)
    _lib.check(lib.mg_phone_front_linear_fwd_x3(_p(dur), b, p, int(t), _p(target), _p(seq_len), extra, _p(rows[0]), _p(rows[1]), r, _p(seg[0]),
                                                _p(seg[1]), _p(stats[0]), _p(stats[1]), _p(ws), ws.numel(), _p(a), a.shape[1], m, k, _p(w2),
                                                w2.shape[1], _p(bias), n, _p(y), 2 * n, act, _stream()), 'mg_phone_front_linear_fwd_x3')
    return rows[0], rows[1], seg, stats[0], stats[1], ws, y


X3_FWD_PARTS = int(os.environ.get('MORGANA_X3_FWD_PARTS', '3'))      # A/B: 1 = the 128-wide layer's three passes in one workgroup per tile


def linear_fwd_x3_f32(a2, k, w2, bias, n, act, parts=1):
    """fp32 (M, n) = act(a w^T + bias) from pair-plane operands a2 (M, 2 pa), w2 (n, 2 pw) (mg_linear_fwd_x3_f32).  ``parts`` = 3
    (no activation): (3, M, n) partial sums of the three products, from three sets of workgroups - the consumer adds them."""
    m = a2.shape[0]
    y = torch.empty((m, n) if parts == 1 else (parts, m, n), dtype=torch.float32, device=a2.device)
    _lib.check(_lib.load().mg_linear_fwd_x3_f32(_p(a2), a2.shape[1], m, k, _p(w2), w2.shape[1], _p(bias), n, _p(y), n, act, int(parts), _stream()),
               'mg_linear_fwd_x3_f32')
    return y


def f0_tail_rows_x3(z2, w3, b3, w4, b4, ybar, weight, keep_slabs=False):
    """``f0_tail_rows_f32`` of the fused 'bf16x3' step (mg_f0_tail_rows_x3): returns (pred (rows,), dz2 PAIR (rows, 256) bf16, slab buffer,
    n_slabs, stride); the slabs [db2 | dW3 | db3 | dW4 | db4 | loss | pad] are left unreduced for the caller (``slab_reduce``,
    mg_expand_column_reduce_f32 or the update kernel's plan).  ``keep_slabs``: a buffer of their own (they outlive the next launches)."""
    lib = _lib.load()
    z2 = _require(z2, torch.float32, 'pre-activations')
    z_parts = z2.shape[0] if z2.dim() == 3 else 1              # (3, rows, 128): three partial sums to add (linear_fwd_x3_f32 parts = 3)
    m = z2.shape[-2]
    if (z_parts not in (1, 3) or z2.shape[-1] != 128 or tuple(w3.shape) != (32, 128) or tuple(w4.shape) != (1, 32) or ybar.numel() != m
            or weight.numel() != m):
        raise ValueError('f0_tail_rows_x3: needs (rows, 128) pre-activations, a 128 -> 32 -> 1 tail and one statistics row per table row')
    pred = torch.empty((m,), dtype=torch.float32, device=z2.device)
    dz2 = torch.empty((m, 256), dtype=torch.bfloat16, device=z2.device)
    ws = (_tail_slabs if keep_slabs else workspace)(lib.mg_f0_tail_rows_x3_workspace_bytes(m), z2.device)
    n_slabs, stride = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(lib.mg_f0_tail_rows_x3(_p(z2), z2.shape[-1], z_parts, _p(_require(w3, torch.float32, 'w3')), _p(b3), _p(_require(w4, torch.float32, 'w4')),
                                      _p(b4), _p(ybar), _p(weight), m, _p(pred), _p(dz2), 256, None, _p(ws), ws.numel(),
                                      ctypes.byref(n_slabs), ctypes.byref(stride), _stream()), 'mg_f0_tail_rows_x3')
    return pred, dz2, ws, n_slabs.value, stride.value


X3_L2TAIL = os.environ.get('MORGANA_X3_L2TAIL', '1') != '0'      # A/B: 0 = the 128-wide layer and the fp32 tail as two launches


def f0_l2tail_x3(h1, w2p, b2, w3, b3, w4, b4, ybar, weight, keep_slabs=False):
    """``linear_fwd_x3_f32`` of the 512 -> 128 layer and ``f0_tail_rows_x3`` as ONE launch (mg_f0_l2tail_x3): h1 pair (rows, 1024), w2p
    pair (128, 1024).  Returns what ``f0_tail_rows_x3`` returns."""
    lib = _lib.load()
    m = h1.shape[0]
    if (h1.shape[1] != 1024 or tuple(w2p.shape) != (128, 1024) or tuple(w3.shape) != (32, 128) or tuple(w4.shape) != (1, 32)
            or ybar.numel() != m or weight.numel() != m):
        raise ValueError('f0_l2tail_x3: needs the (rows, 1024) pair of a 512-wide activation, a 512 -> 128 -> 32 -> 1 tail and one statistics row per table row')
    pred = torch.empty((m,), dtype=torch.float32, device=h1.device)
    dz2 = torch.empty((m, 256), dtype=torch.bfloat16, device=h1.device)
    ws = (_tail_slabs if keep_slabs else workspace)(lib.mg_f0_l2tail_x3_workspace_bytes(m), h1.device)
    n_slabs, stride = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(lib.mg_f0_l2tail_x3(_p(h1), h1.shape[1], _p(w2p), w2p.shape[1], _p(b2), _p(_require(w3, torch.float32, 'w3')), _p(b3),
                                   _p(_require(w4, torch.float32, 'w4')), _p(b4), _p(ybar), _p(weight), m, _p(pred), _p(dz2), 256, None,
                                   _p(ws), ws.numel(), ctypes.byref(n_slabs), ctypes.byref(stride), _stream()), 'mg_f0_l2tail_x3')
    return pred, dz2, ws, n_slabs.value, stride.value


def linear_wgrad_dgrad_x3(dy2, a2, m, n, k, wt2, slab=None, colsum=None):
    """The 512 -> 128 layer's backward of the fused 'bf16x3' step as one grid (mg_linear_wgrad_dgrad_x3): dy2 pair (m, 2 * 128), a2 = the
    sigmoid output's pair (m, 2 * 512), wt2 = the pair of W^T (k, 2 * 128).  Returns (slab buffer, n_slabs, stride, dx pair (m, 2 k),
    colsum buffer (n_colsum, k) f32 - its ordered sum is the bias gradient of the layer below, n_colsum)."""
    lib = _lib.load()
    slab = _slab_buffer(slab, lib.mg_linear_wgrad_workspace_bytes(m, n, k), dy2.device)
    need = lib.mg_linear_wgrad_dgrad_x3_colsum_floats(m, k)
    colsum = _slab_buffer(colsum, 4 * need, dy2.device)
    dx = torch.empty((m, 2 * k), dtype=torch.bfloat16, device=dy2.device)
    n_slabs, stride, n_colsum = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int(0)
    _lib.check(lib.mg_linear_wgrad_dgrad_x3(_p(dy2), dy2.shape[1], _p(a2), a2.shape[1], m, n, k, _p(wt2), wt2.shape[1], _p(dx), 2 * k, _p(slab),
                                            slab.numel(), ctypes.byref(n_slabs), ctypes.byref(stride), _p(colsum), colsum.numel() // 4,
                                            ctypes.byref(n_colsum), _stream()), 'mg_linear_wgrad_dgrad_x3')
    return slab, n_slabs.value, stride.value, dx, colsum, n_colsum.value


def linear_wgrad_slabs_x3(dy2, a2, m, n, k, slab=None):
    """``linear_wgrad_slabs_bf16`` on pair planes (mg_linear_wgrad_slabs_x3): slabs of n k weight partials (stride n k + n), no bias sums."""
    lib = _lib.load()
    slab = _slab_buffer(slab, lib.mg_linear_wgrad_workspace_bytes(m, n, k), dy2.device)
    n_slabs, stride = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(lib.mg_linear_wgrad_slabs_x3(_p(dy2), dy2.shape[1], _p(a2), a2.shape[1], m, n, k, _p(slab), slab.numel(), ctypes.byref(n_slabs),
                                            ctypes.byref(stride), _stream()), 'mg_linear_wgrad_slabs_x3')
    return slab, n_slabs.value, stride.value


def f0_tail(h2, w3, b3, w4, b4, target, seq_len, b, t, grads_out, grad_scale=1.0):
    """Fused layers 3-4 + masked MSE, forward and backward (mg_f0_tail_bf16).  Returns (pred (b*t,), loss 0-d, dz2)."""
    lib = _lib.load()
    m = b * t
    pred = torch.empty((m,), dtype=torch.float32, device=h2.device)
    n_grads = 32 * 128 + 32 + 32 + 1
    # a gradient buffer with one spare float behind the tail's gradients receives the loss from the same reduce launch
    loss = grads_out[n_grads] if grads_out.numel() > n_grads else torch.empty((), dtype=torch.float32, device=h2.device)
    dz2 = torch.empty_like(h2)
    nbytes = lib.mg_f0_tail_workspace_bytes(m)
    ws = workspace(nbytes, h2.device)
    _lib.check(lib.mg_f0_tail_bf16(_p(h2), h2.shape[1], w3.shape[1], _p(w3), _p(b3), _p(w4), _p(b4), _p(target),
                                   _p(seq_len), b, t, float(grad_scale), _p(pred), _p(loss), _p(dz2), _p(grads_out), 0,
                                   _p(ws), ws.numel(), _stream()), 'mg_f0_tail_bf16')
    return pred, loss, dz2


def f0_tail_rows(h2, w3, b3, w4, b4, target_rows, row_weight, grads_out, grad_scale=1.0):
    """f0_tail on table rows that each stand for a group of frames (mg_f0_tail_rows_bf16): loss = sum_m w[m] (pred[m] - y[m])^2.
    Returns (pred (rows,), loss 0-d, dz2 (rows, ld))."""
    lib = _lib.load()
    m = h2.shape[0]
    pred = torch.empty((m,), dtype=torch.float32, device=h2.device)
    n_grads = 32 * 128 + 32 + 32 + 1
    loss = grads_out[n_grads] if grads_out.numel() > n_grads else torch.empty((), dtype=torch.float32, device=h2.device)
    dz2 = torch.empty_like(h2)
    ws = workspace(lib.mg_f0_tail_workspace_bytes(m), h2.device)
    _lib.check(lib.mg_f0_tail_rows_bf16(_p(h2), h2.shape[1], w3.shape[1], _p(w3), _p(b3), _p(w4), _p(b4), _p(target_rows), _p(row_weight),
                                        m, float(grad_scale), _p(pred), _p(loss), _p(dz2), _p(grads_out), 0, _p(ws), ws.numel(),
                                        _stream()), 'mg_f0_tail_rows_bf16')
    return pred, loss, dz2


def l2tail_ok(w2, w3, w4, act2):
    """The 512 -> 128 sigmoid layer and the 128 -> 32 -> 1 tail as ONE kernel (csrc/l2tail_bf16.hip): shapes it is built for."""
    return (tuple(w2.shape) == (128, 512) and tuple(w3.shape) == (32, 128) and tuple(w4.shape) == (1, 32) and act2 == ACT_SIGMOID
            and os.environ.get('MORGANA_L2TAIL', '1') != '0')


def f0_l2tail(h1, w2_bf, b2, w3, b3, w4, b4, target, seq_len, b, t, grads_out, grad_scale=1.0, defer=False):
    """Layer 2 (512 -> 128, sigmoid) + layers 3-4 + masked MSE, forward and backward, in one pass over H1 (mg_f0_l2tail_bf16).
    Returns (pred (b*t,), loss 0-d, dz2 (b*t, 128) bf16); the 128-wide activation is never written.
    ``defer``: the reduce launch is NOT made (mg_f0_l2tail_slabs_bf16); a fourth return value describes what is left - the sum of the
    workgroups' slabs into ``grads_out`` (gradients and, behind them, the loss) - for optim.Adam.defer_tail / finish_deferred_tail."""
    lib = _lib.load()
    m = b * t
    pred = torch.empty((m,), dtype=torch.float32, device=h1.device)
    n_grads = 32 * 128 + 32 + 32 + 1
    loss = grads_out[n_grads] if grads_out.numel() > n_grads else torch.empty((), dtype=torch.float32, device=h1.device)
    dz2 = torch.empty((m, 128), dtype=torch.bfloat16, device=h1.device)
    if defer:
        if grads_out.numel() <= n_grads:
            raise ValueError('f0_l2tail(defer=True): the gradient buffer needs one float behind the gradients for the loss')
        ws = _tail_slabs(lib.mg_f0_l2tail_workspace_bytes(m), h1.device)
        n_slabs = ctypes.c_int(0)
        _lib.check(lib.mg_f0_l2tail_slabs_bf16(_p(h1), h1.shape[1], 512, _p(w2_bf), w2_bf.shape[1], 128, _p(b2), _p(w3), _p(b3), _p(w4),
                                               _p(b4), _p(target), _p(seq_len), b, t, float(grad_scale), _p(pred), _p(dz2), 128, _p(ws),
                                               ws.numel(), ctypes.byref(n_slabs), _stream()), 'mg_f0_l2tail_slabs_bf16')
        tail = dict(rows=None, partials=None, ws=ws, n=n_grads + 1, stride=int(lib.mg_f0_l2tail_slab_stride()), n_slabs=n_slabs.value,
                    grads_out=grads_out)
        return pred, loss, dz2, tail
    ws = workspace(lib.mg_f0_l2tail_workspace_bytes(m), h1.device)
    _lib.check(lib.mg_f0_l2tail_bf16(_p(h1), h1.shape[1], 512, _p(w2_bf), w2_bf.shape[1], 128, _p(b2), _p(w3), _p(b3), _p(w4), _p(b4),
                                     _p(target), _p(seq_len), b, t, float(grad_scale), _p(pred), _p(loss), _p(dz2), 128,
                                     _p(grads_out), 0, _p(ws), ws.numel(), _stream()), 'mg_f0_l2tail_bf16')
    return pred, loss, dz2


def f0_l2tail_rows(h1, w2_bf, b2, w3, b3, w4, b4, target_rows, row_weight, grads_out, grad_scale=1.0):
    """f0_l2tail on table rows that each stand for a group of frames (mg_f0_l2tail_rows_bf16, the phone-rate step)."""
    lib = _lib.load()
    m = h1.shape[0]
    pred = torch.empty((m,), dtype=torch.float32, device=h1.device)
    n_grads = 32 * 128 + 32 + 32 + 1
    loss = grads_out[n_grads] if grads_out.numel() > n_grads else torch.empty((), dtype=torch.float32, device=h1.device)
    dz2 = torch.empty((m, 128), dtype=torch.bfloat16, device=h1.device)
    ws = workspace(lib.mg_f0_l2tail_workspace_bytes(m), h1.device)
    _lib.check(lib.mg_f0_l2tail_rows_bf16(_p(h1), h1.shape[1], 512, _p(w2_bf), w2_bf.shape[1], 128, _p(b2), _p(w3), _p(b3), _p(w4),
                                          _p(b4), _p(target_rows), _p(row_weight), m, float(grad_scale), _p(pred), _p(loss), _p(dz2),
                                          128, _p(grads_out), 0, _p(ws), ws.numel(), _stream()), 'mg_f0_l2tail_rows_bf16')
    return pred, loss, dz2


def f0_l2tail_rows_expand(h1, w2_bf, b2, w3, b3, w4, b4, target_rows, row_weight, grads_out, rows, loss_const, grad_scale=1.0, defer=False):
    """f0_l2tail_rows + expand_column with the tail's reduce folded into the expansion's launch (mg_f0_l2tail_rows_slabs_bf16 +
    mg_expand_column_reduce_f32): one node less in the phone-rate step, same sums in the same order.  ``grads_out`` must have room for
    the loss behind the tail's gradients; ``loss_const`` = (partials, n_table_rows, extra).  Returns (pred (frames,), loss, dz2).
    ``defer``: the second launch is NOT made; a fourth return value describes it, for linear_wgrad_dgrad_bf16(tail=...) /
    finish_deferred_tail - pred, loss and the tail's gradients are valid only after one of them ran (a step captured whole into a
    HIP graph: functional.DEFER_TAIL)."""
    lib = _lib.load()
    m = h1.shape[0]
    n = 32 * 128 + 32 + 32 + 2                           # dW3 | db3 | dW4 | db4 | loss
    if grads_out.numel() < n:
        raise ValueError('f0_l2tail_rows_expand: the gradient buffer needs one float behind the gradients for the loss')
    pred_rows = torch.empty((m,), dtype=torch.float32, device=h1.device)
    dz2 = torch.empty((m, 128), dtype=torch.bfloat16, device=h1.device)
    # deferred: the slabs must outlive this call (they are summed at the end of a later launch), so they do not go to the scratch
    # buffer every kernel of the step shares
    ws = (_tail_slabs if defer else workspace)(lib.mg_f0_l2tail_workspace_bytes(m), h1.device)
    n_slabs = ctypes.c_int(0)
    _lib.check(lib.mg_f0_l2tail_rows_slabs_bf16(_p(h1), h1.shape[1], 512, _p(w2_bf), w2_bf.shape[1], 128, _p(b2), _p(w3), _p(b3), _p(w4),
                                                _p(b4), _p(target_rows), _p(row_weight), m, float(grad_scale), _p(pred_rows), _p(dz2),
                                                128, _p(ws), ws.numel(), ctypes.byref(n_slabs), _stream()),
               'mg_f0_l2tail_rows_slabs_bf16')
    partials, n_table_rows, extra = loss_const
    out = torch.empty((rows.numel(),), dtype=torch.float32, device=h1.device)
    stride = int(lib.mg_f0_l2tail_slab_stride())
    if defer:
        tail = dict(pred_rows=pred_rows, rows=rows, out=out, partials=partials, n_table_rows=int(n_table_rows), extra=int(extra), ws=ws,
                    n=n, stride=stride, n_slabs=n_slabs.value, grads_out=grads_out)
        return out, grads_out[n - 1], dz2, tail
    _lib.check(lib.mg_expand_column_reduce_f32(_p(pred_rows), _p(rows), rows.numel(), _p(out), _p(partials), n_table_rows, extra, _p(ws),
                                               n, stride, n_slabs.value, _p(grads_out), _stream()), 'mg_expand_column_reduce_f32')
    return out, grads_out[n - 1], dz2


def phone_target_stats(target, rows, seg, seq_len, b, t, n_table_rows, extra):
    """(ybar (R + extra,), weight (R + extra,), partials) of the masked MSE per table row (mg_phone_target_stats); ``partials`` holds
    the per-block sums of the loss's constant term for ``phone_loss_const_add``."""
    lib = _lib.load()
    target = _require(target, torch.float32, 'targets')
    if extra < 1:
        raise ValueError('phone_target_stats: extra=%d: at least one extra row must take the padding frames\' loss terms' % extra)
    stats = torch.empty((2, n_table_rows + extra), dtype=torch.float32, device=target.device)
    ws = torch.empty(lib.mg_phone_target_stats_workspace_bytes(n_table_rows, extra), dtype=torch.uint8, device=target.device)
    _lib.check(lib.mg_phone_target_stats(_p(target), _p(rows), rows.numel(), _p(seg[0]), _p(seg[1]), _p(seq_len), b, t, n_table_rows,
                                         extra, _p(stats[0]), _p(stats[1]), None, _p(ws), ws.numel(), _stream()),
               'mg_phone_target_stats')
    return stats[0], stats[1], ws


def phone_front_ok(b, p, t, extra):
    """Shapes the one-launch front of the phone-rate step takes (mg_phone_front): a partial-sum slot per utterance (about 16 phones per
    utterance or more) and extra rows whose frame chunks span few utterances."""
    if not (b > 0 and p > 0 and t > 0 and extra > 0 and p <= 12288 and b <= -(-(b * p) // 16)):
        return False
    chunk = -(-(b * t) // extra)
    return 512 + max(p + t + 1, -(-(4 * chunk) // t) + 2) <= 16000


def phone_front(dur, target, seq_len, t, extra, linear=None):
    """upsample_index_maps + phone_target_stats in ONE launch (mg_phone_front): returns (rows (B, t), rows_mapped (B, t), seg (2, B*P),
    ybar, weight, partials).  ``linear`` = (a bf16 (M, lda), k, w_bf16, bias, n, act): additionally y = act(a w^T + bias) (bf16 (M, n)),
    appended to the result, in the SAME grid where the GEMM leaves CUs idle (mg_phone_front_linear_fwd_bf16)."""
    lib = _lib.load()
    dur = _require(dur, torch.int64, 'dur')
    target = _require(target, torch.float32, 'targets')
    b, p = dur.shape
    if target.numel() != b * t:
        raise ValueError('phone_front: %d targets for %d x %d frames' % (target.numel(), b, t))
    r = b * p
    rows = torch.empty((2, b, t), dtype=torch.int32, device=dur.device)
    seg = torch.empty((2, r), dtype=torch.int32, device=dur.device)
    stats = torch.empty((2, r + extra), dtype=torch.float32, device=dur.device)
    ws = torch.empty(lib.mg_phone_target_stats_workspace_bytes(r, extra), dtype=torch.uint8, device=dur.device)
    front = (_p(dur), b, p, int(t), _p(target), _p(seq_len), extra, _p(rows[0]), _p(rows[1]), r, _p(seg[0]), _p(seg[1]), _p(stats[0]),
             _p(stats[1]), _p(ws), ws.numel())
    if linear is None:
        _lib.check(lib.mg_phone_front(*front, _stream()), 'mg_phone_front')
        return rows[0], rows[1], seg, stats[0], stats[1], ws
    a, k, w_bf16, bias, n, act = linear
    m = a.shape[0]
    y = torch.empty((m, pad8(n)), dtype=torch.bfloat16, device=a.device)
    _lib.check(lib.mg_phone_front_linear_fwd_bf16(*front, _p(a), a.shape[1], m, k, _p(w_bf16), w_bf16.shape[1], _p(bias), n, _p(y), pad8(n), act,
                                                  _stream()), 'mg_phone_front_linear_fwd_bf16')
    return rows[0], rows[1], seg, stats[0], stats[1], ws, y


F0_TAIL_F32_GRADS = 32 * 128 + 32 + 32 + 1          # dW3 | db3 | dW4 | db4, then the loss (and two unused floats)


def f0_tail_rows_f32(z2, w3, b3, w4, b4, ybar, weight, seq_len=None, frames=None):
    """The README tail 128 -> 32 -> 1 with the per-phone masked MSE, forward and backward, exact fp32, one launch (mg_f0_tail_rows_f32).
    z2 (rows, 128) f32 pre-activations of the 128-wide layer.  Returns (pred (rows,), dz2 (rows, 128), flat (4164,) = the tail's
    parameter gradients in parameter order, the loss without its constant term at index F0_TAIL_F32_GRADS).
    ``weight`` None with ``frames`` = (B, T): the rows are the frames, ``ybar`` the targets, the weights the masked MSE's own (from seq_len)."""
    lib = _lib.load()
    z2 = _require(z2, torch.float32, 'pre-activations')
    m = z2.shape[0]
    if (z2.shape[1] != 128 or tuple(w3.shape) != (32, 128) or tuple(w4.shape) != (1, 32) or ybar.numel() != m
            or (weight.numel() != m if weight is not None else (frames is None or frames[0] * frames[1] != m))):
        raise ValueError('f0_tail_rows_f32: needs (rows, 128) pre-activations, a 128 -> 32 -> 1 tail and one statistics row per table row')
    pred = torch.empty((m,), dtype=torch.float32, device=z2.device)
    dz2 = torch.empty((m, 128), dtype=torch.float32, device=z2.device)
    flat = torch.empty((F0_TAIL_F32_GRADS + 3,), dtype=torch.float32, device=z2.device)
    ws = workspace(lib.mg_f0_tail_rows_f32_workspace_bytes(m), z2.device)
    _lib.check(lib.mg_f0_tail_rows_f32(_p(z2), z2.shape[1], _p(_require(w3, torch.float32, 'w3')), _p(b3), _p(_require(w4, torch.float32, 'w4')),
                                       _p(b4), _p(ybar), _p(weight), _p(seq_len), frames[0] if frames else 0, frames[1] if frames else 0, m,
                                       _p(pred), _p(dz2), dz2.shape[1], _p(flat), _p(ws), ws.numel(), _stream()),
               'mg_f0_tail_rows_f32')
    return pred, dz2, flat


def phone_mse_rows(pred_table, ybar, weight):
    """(loss (1,) without the constant term, dpred (rows,)) of the masked MSE of a one-column prediction per table row
    (mg_phone_mse_rows_f32); pred_table (rows, ld) f32, column 0."""
    pred_table = _require(pred_table, torch.float32, 'prediction')
    n = ybar.numel()
    if pred_table.shape[0] != n:
        raise ValueError('phone_mse_rows: %d prediction rows for %d statistics rows' % (pred_table.shape[0], n))
    out = torch.empty((n + 1,), dtype=torch.float32, device=pred_table.device)
    _lib.check(_lib.load().mg_phone_mse_rows_f32(_p(pred_table), pred_table.shape[1], _p(ybar), _p(weight), n, _p(out[n:]), _p(out), _stream()),
               'mg_phone_mse_rows_f32')
    return out[n:], out[:n]


def phone_loss_const_add(partials, n_table_rows, extra, loss):
    """loss (0-d f32, in place) += the constant term left by phone_target_stats."""
    _lib.check(_lib.load().mg_phone_loss_const_add(_p(partials), n_table_rows, extra, _p(loss), _stream()), 'mg_phone_loss_const_add')


def expand_column(table, rows, loss_const=None):
    """out[f] = table[rows[f]] for a (rows,) f32 table and an int32 map without negative entries (mg_expand_column_f32).
    ``loss_const`` = (partials, n_table_rows, extra, loss): the same launch adds phone_target_stats' constant to ``loss`` in place."""
    lib = _lib.load()
    table = _require(table, torch.float32, 'table')
    out = torch.empty((rows.numel(),), dtype=torch.float32, device=table.device)
    if loss_const is None:
        _lib.check(lib.mg_expand_column_f32(_p(table), _p(rows), rows.numel(), _p(out), _stream()), 'mg_expand_column_f32')
    else:
        partials, n_table_rows, extra, loss = loss_const
        _lib.check(lib.mg_expand_column_loss_f32(_p(table), _p(rows), rows.numel(), _p(out), _p(partials), n_table_rows, extra,
                                                 _p(loss), _stream()), 'mg_expand_column_loss_f32')
    return out


def sigmoid(x):
    lib = _lib.load()
    x = _require(x, torch.float32, 'input')
    y = torch.empty_like(x)
    _lib.check(lib.mg_sigmoid_f32(_p(x), _p(y), x.numel(), _stream()), 'mg_sigmoid_f32')
    return y


def sigmoid_grad(dy, y):
    lib = _lib.load()
    dy = _require(dy, torch.float32, 'grad')
    dx = torch.empty_like(y)
    _lib.check(lib.mg_sigmoid_grad_f32(_p(dy), _p(y), _p(dx), y.numel(), _stream()), 'mg_sigmoid_grad_f32')
    return dx


def act(x, act):
    """Elementwise ACT_SIGMOID / ACT_TANH / ACT_RELU of an fp32 tensor (a stand-alone nn.Sigmoid / nn.Tanh / nn.ReLU)."""
    lib = _lib.load()
    x = _require(x, torch.float32, 'input')
    y = torch.empty_like(x)
    _lib.check(lib.mg_act_f32(_p(x), _p(y), x.numel(), act, _stream()), 'mg_act_f32')
    return y


def act_grad(dy, y, act):
    """dy * f'(y) with f' in the activation's output ``y``: y (1 - y), 1 - y^2, y > 0."""
    lib = _lib.load()
    dy = _require(dy, torch.float32, 'grad')
    y = _require(y, torch.float32, 'activation')
    dx = torch.empty_like(y)
    _lib.check(lib.mg_act_grad_f32(_p(dy), _p(y), _p(dx), y.numel(), act, _stream()), 'mg_act_grad_f32')
    return dx


# ----------------------------------------------------------------------------------------------------------------- K3
def _initial_state(init, b, t, h, dev, dtype=torch.float32):
    """The (b, t + 1, h) state tensor of a recurrence: step 0 zeroed, or copied from ``init`` (anything of b * h elements); the
    steps behind it are the kernel's to write."""
    state = torch.empty((b, t + 1, h), dtype=dtype, device=dev)
    if init is None:
        state[:, 0].zero_()
    else:
        state[:, 0].copy_(init.reshape(b, h))
    return state


def gru_persist_f32_ok(b, t, h):
    return PERSISTENT_RECURRENCE and bool(_lib.load().mg_gru_persist_f32_supported(b, t, h))


def gru_fwd(xproj, w_hh, b_hh, seq_len, h0, b, t, h, persistent=None):
    """xproj (b, t, 3h) f32.  Returns (out (b,t,h), hstate (b,t+1,h), saved (b,t,4h)).  persistent: the one-launch fp32 kernel
    (None = whenever the shape is covered; bit-identical to the per-step kernels on the live steps)."""
    lib = _lib.load()
    dev = xproj.device
    if persistent is None:
        persistent = gru_persist_f32_ok(b, t, h)
    hstate = _initial_state(h0, b, t, h, dev)
    out = torch.empty((b, t, h), dtype=torch.float32, device=dev)
    saved = torch.empty((b, t, 4 * h), dtype=torch.float32, device=dev)
    if persistent:
        ws = _persist_workspace(dev, b, h)
        _lib.check(lib.mg_gru_fwd_persist_f32(_p(xproj), _p(w_hh), _p(b_hh), _p(seq_len), b, t, h, _p(hstate), _p(out), _p(saved),
                                              _p(ws), ws.numel(), _stream()), 'mg_gru_fwd_persist_f32')
        return out, hstate, saved
    _lib.check(lib.mg_gru_fwd_f32(_p(xproj), _p(w_hh), _p(b_hh), _p(seq_len), b, t, h, _p(hstate), _p(out), _p(saved),
                                  _stream()), 'mg_gru_fwd_f32')
    return out, hstate, saved


def gru_bwd(grad_out, grad_hn, hstate, saved, w_hh, seq_len, b, t, h, persistent=None):
    lib = _lib.load()
    dev = grad_out.device
    dxproj = torch.empty((b, t, 3 * h), dtype=torch.float32, device=dev)
    dhproj = torch.empty((b, t, 3 * h), dtype=torch.float32, device=dev)
    dh0 = torch.empty((b, h), dtype=torch.float32, device=dev)
    if persistent is None:
        persistent = gru_persist_f32_ok(b, t, h)
    if persistent:
        ws = _persist_workspace(dev, b, h)
        _lib.check(lib.mg_gru_bwd_persist_f32(_p(grad_out), _p(grad_hn), _p(hstate), _p(saved), _p(w_hh), _p(seq_len), b, t, h,
                                              _p(dxproj), _p(dhproj), _p(dh0), _p(ws), ws.numel(), _stream()), 'mg_gru_bwd_persist_f32')
        return dxproj, dhproj, dh0
    nbytes = lib.mg_gru_bwd_workspace_bytes(b, h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)   # own buffer: lives across the wgrad calls that follow
    _lib.check(lib.mg_gru_bwd_f32(_p(grad_out), _p(grad_hn), _p(hstate), _p(saved), _p(w_hh), _p(seq_len), b, t, h,
                                  _p(dxproj), _p(dhproj), _p(dh0), _p(ws), ws.numel(), _stream()), 'mg_gru_bwd_f32')
    return dxproj, dhproj, dh0


def gru_bf16_ok(h):
    """The bf16-operand recurrence needs H % 128 == 0 and H <= 1024 (include/morgana_hip.h: mg_gru_fwd_bf16)."""
    return h % 128 == 0 and h <= 1024


_PERSIST_WORKSPACES = {}          # (device, stream) -> sync block shared by the persistent launches of that stream
PERSISTENT_RECURRENCE = os.environ.get('MORGANA_PERSISTENT', '1') != '0'


def gru_persist_ok(b, t, h):
    return PERSISTENT_RECURRENCE and bool(_lib.load().mg_gru_persist_supported(b, t, h))


def _persist_workspace(dev, b, h):
    key = (dev, torch.cuda.current_stream().cuda_stream)
    need = _lib.load().mg_gru_persist_workspace_bytes(b, h)
    ws = _PERSIST_WORKSPACES.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            check_persistent_status()                 # read the old block's status word before dropping it
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        _PERSIST_WORKSPACES[key] = ws
    return ws


def check_persistent_status():
    """Synchronise and raise if a persistent recurrent kernel launched since the last call gave up waiting for a peer workgroup
    (its results are invalid).  Called once per epoch by ExperimentBuilder, by bench.py, smoke() and the GPU tests."""
    lib = _lib.load()
    for key, ws in list(_PERSIST_WORKSPACES.items()):
        _lib.check(lib.mg_gru_persist_status(_p(ws), ctypes.c_void_p(key[1])), 'mg_gru_persist_status')


def gru_fwd_bf16(xproj, w_hh, b_hh, seq_len, h0, b, t, h, persistent=None, xrows=None, out_bf=None, w_bf=None):
    """gru_fwd with bf16 matmul operands.  Returns (out, hstate, saved, hstate_bf (b,t+1,h) bf16).
    out_bf (persistent launch only): a (b, t, h) bf16 tensor that receives the bf16 copy of ``out`` from the recurrence itself.
    persistent: one launch for all steps (None = whenever the shape is covered).
    xrows (persistent launch only): int32 (b, t) row map - ``xproj`` is then a table (rows, 3h) and frame (b, t) takes row
    ``xrows[b, t]`` of it (mg_gru_fwd_persist_rows_bf16: the repetition applied inside the recurrence).
    w_bf: the (3h, pad_ld(h)) bf16 copy of ``w_hh`` if the caller holds a current one (param_shadows); cast here otherwise."""
    lib = _lib.load()
    if persistent is None:
        persistent = gru_persist_ok(b, t, h)
    if xrows is not None and not persistent:
        raise ValueError('gru_fwd_bf16: a row map needs the persistent launch (gather the rows first)')
    if out_bf is not None and (not persistent or out_bf.dtype != torch.bfloat16 or tuple(out_bf.shape) != (b, t, h) or not out_bf.is_contiguous()):
        raise ValueError('gru_fwd_bf16: out_bf must be a contiguous (b, t, h) bfloat16 tensor and needs the persistent launch')
    dev = xproj.device
    hstate = _initial_state(h0, b, t, h, dev)
    hstate_bf = _initial_state(h0, b, t, h, dev, torch.bfloat16)
    if w_bf is None or w_bf.dtype != torch.bfloat16 or w_bf.shape[0] != 3 * h or w_bf.shape[1] < h or not w_bf.is_contiguous():
        w_bf = cast_pad_bf16(w_hh)
    out = torch.empty((b, t, h), dtype=torch.float32, device=dev)
    saved = torch.empty((b, t, 4 * h), dtype=torch.float32, device=dev)
    if persistent:
        ws = _persist_workspace(dev, b, h)
        if xrows is not None:
            xrows = _require(xrows, torch.int32, 'xrows')
            if xrows.numel() != b * t or xproj.ndim != 2 or xproj.shape[1] != 3 * h:
                raise ValueError('gru_fwd_bf16: row map of %d entries / table %s for b=%d t=%d h=%d' % (xrows.numel(), tuple(xproj.shape), b, t, h))
        n_rows = xproj.shape[0] if xrows is not None else 0
        _lib.check(lib.mg_gru_fwd_persist_out_bf16(_p(xproj), _p(xrows), n_rows, _p(w_bf), w_bf.shape[1], _p(b_hh), _p(seq_len), b, t, h,
                                                   _p(hstate), _p(hstate_bf), _p(out), _p(out_bf), _p(saved), _p(ws), ws.numel(), _stream()),
                   'mg_gru_fwd_persist_out_bf16')
    else:
        _lib.check(lib.mg_gru_fwd_bf16(_p(xproj), _p(w_bf), w_bf.shape[1], _p(b_hh), _p(seq_len), b, t, h, _p(hstate), _p(hstate_bf),
                                       _p(out), _p(saved), _stream()), 'mg_gru_fwd_bf16')
    return out, hstate, saved, hstate_bf


def gru_bwd_bf16(grad_out, grad_hn, hstate, saved, w_hh, seq_len, b, t, h, persistent=None, shadows_only=False, wt_bf=None):
    """gru_bwd with bf16 matmul operands.  Returns (dxproj, dhproj, dh0, dhproj_bf (b,t,3h) bf16).
    shadows_only (persistent kernel only): returns (dxproj_bf, dhproj_bf, dh0) and does not write the fp32 arrays.
    wt_bf: the (h, pad_ld(3h)) bf16 transpose of ``w_hh`` if the caller holds a current one (param_shadows); cast here otherwise."""
    lib = _lib.load()
    if persistent is None:
        persistent = gru_persist_ok(b, t, h)
    dev = grad_out.device
    if wt_bf is not None and (wt_bf.dtype != torch.bfloat16 or wt_bf.shape[0] != h or wt_bf.shape[1] < 3 * h or not wt_bf.is_contiguous()):
        wt_bf = None
    shadows_only = shadows_only and persistent
    dxproj = dhproj = dxproj_bf = None                             # fp32 gradients, or (shadows_only) the bf16 copy of dxproj
    if shadows_only:
        dxproj_bf = torch.empty((b, t, 3 * h), dtype=torch.bfloat16, device=dev)
    else:
        dxproj = torch.empty((b, t, 3 * h), dtype=torch.float32, device=dev)
        dhproj = torch.empty((b, t, 3 * h), dtype=torch.float32, device=dev)
    dhproj_bf = torch.empty((b, t, 3 * h), dtype=torch.bfloat16, device=dev)
    dh0 = torch.empty((b, h), dtype=torch.float32, device=dev)
    if wt_bf is None:
        wt_bf = cast_transpose_bf16(w_hh)                          # (h, 3h)
    if persistent:
        ws = _persist_workspace(dev, b, h)
        _lib.check(lib.mg_gru_bwd_persist_bf16(_p(grad_out), _p(grad_hn), _p(hstate), _p(saved), _p(wt_bf), wt_bf.shape[1], _p(seq_len),
                                               b, t, h, _p(dxproj), _p(dhproj), _p(dhproj_bf), _p(dxproj_bf), _p(dh0), _p(ws), ws.numel(),
                                               _stream()), 'mg_gru_bwd_persist_bf16')
        return (dxproj_bf, dhproj_bf, dh0) if shadows_only else (dxproj, dhproj, dh0, dhproj_bf)
    nbytes = lib.mg_gru_bwd_workspace_bytes(b, h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.mg_gru_bwd_bf16(_p(grad_out), _p(grad_hn), _p(hstate), _p(saved), _p(wt_bf), wt_bf.shape[1], _p(seq_len), b, t, h,
                                   _p(dxproj), _p(dhproj), _p(dhproj_bf), _p(dh0), _p(ws), ws.numel(), _stream()),
               'mg_gru_bwd_bf16')
    return dxproj, dhproj, dh0, dhproj_bf


def lstm_persist_f32_ok(b, t, h):
    """The one-launch fp32 LSTM recurrence covers this shape (include/morgana_hip.h: mg_lstm_fwd_persist_f32)."""
    return PERSISTENT_RECURRENCE and bool(_lib.load().mg_lstm_persist_f32_supported(b, t, h))


def lstm_fwd(xproj, w_hh, b_hh, seq_len, h0, c0, b, t, h, persistent=None):
    """xproj (b, t, 4h) f32.  Returns (out (b,t,h), hstate (b,t+1,h), cstate (b,t+1,h), saved (b,t,4h)).  persistent: the one-launch
    fp32 kernel (None = whenever the shape is covered; bit-identical to the per-step kernels on the live steps)."""
    lib = _lib.load()
    dev = xproj.device
    if persistent is None:
        persistent = lstm_persist_f32_ok(b, t, h)
    hstate = _initial_state(h0, b, t, h, dev)
    cstate = _initial_state(c0, b, t, h, dev)
    out = torch.empty((b, t, h), dtype=torch.float32, device=dev)
    saved = torch.empty((b, t, 4 * h), dtype=torch.float32, device=dev)
    if persistent:
        ws = _persist_workspace(dev, b, h)
        _lib.check(lib.mg_lstm_fwd_persist_f32(_p(xproj), _p(w_hh), _p(b_hh), _p(seq_len), b, t, h, _p(hstate), _p(cstate), _p(out),
                                               _p(saved), _p(ws), ws.numel(), _stream()), 'mg_lstm_fwd_persist_f32')
        return out, hstate, cstate, saved
    _lib.check(lib.mg_lstm_fwd_f32(_p(xproj), _p(w_hh), _p(b_hh), _p(seq_len), b, t, h, _p(hstate), _p(cstate), _p(out),
                                   _p(saved), _stream()), 'mg_lstm_fwd_f32')
    return out, hstate, cstate, saved


def lstm_bwd(grad_out, grad_hn, grad_cn, cstate, saved, w_hh, seq_len, b, t, h, persistent=None):
    lib = _lib.load()
    dev = grad_out.device
    dgates = torch.empty((b, t, 4 * h), dtype=torch.float32, device=dev)
    dh0 = torch.empty((b, h), dtype=torch.float32, device=dev)
    dc0 = torch.empty((b, h), dtype=torch.float32, device=dev)
    if persistent is None:
        persistent = lstm_persist_f32_ok(b, t, h)
    if persistent:
        ws = _persist_workspace(dev, b, h)
        _lib.check(lib.mg_lstm_bwd_persist_f32(_p(grad_out), _p(grad_hn), _p(grad_cn), _p(cstate), _p(saved), _p(w_hh), _p(seq_len), b, t, h,
                                               _p(dgates), _p(dh0), _p(dc0), _p(ws), ws.numel(), _stream()), 'mg_lstm_bwd_persist_f32')
        return dgates, dh0, dc0
    nbytes = lib.mg_lstm_bwd_workspace_bytes(b, h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.mg_lstm_bwd_f32(_p(grad_out), _p(grad_hn), _p(grad_cn), _p(cstate), _p(saved), _p(w_hh), _p(seq_len), b,
                                   t, h, _p(dgates), _p(dh0), _p(dc0), _p(ws), ws.numel(), _stream()), 'mg_lstm_bwd_f32')
    return dgates, dh0, dc0


def lstm_persist_ok(b, t, h):
    """The one-launch bf16-operand LSTM recurrence covers this shape (include/morgana_hip.h: mg_lstm_fwd_persist_bf16)."""
    return PERSISTENT_RECURRENCE and bool(_lib.load().mg_lstm_persist_supported(b, t, h))


def lstm_fwd_bf16(xproj, w_hh, b_hh, seq_len, h0, c0, b, t, h):
    """lstm_fwd with bf16 matmul operands, one persistent launch.  Returns (out, hstate, cstate, saved, hstate_bf)."""
    lib = _lib.load()
    dev = xproj.device
    hstate = _initial_state(h0, b, t, h, dev)
    cstate = _initial_state(c0, b, t, h, dev)
    hstate_bf = _initial_state(h0, b, t, h, dev, torch.bfloat16)
    w_bf = cast_pad_bf16(w_hh)
    out = torch.empty((b, t, h), dtype=torch.float32, device=dev)
    saved = torch.empty((b, t, 4 * h), dtype=torch.float32, device=dev)
    ws = _persist_workspace(dev, b, h)
    _lib.check(lib.mg_lstm_fwd_persist_bf16(_p(xproj), _p(w_bf), w_bf.shape[1], _p(b_hh), _p(seq_len), b, t, h, _p(hstate), _p(cstate),
                                            _p(hstate_bf), _p(out), _p(saved), _p(ws), ws.numel(), _stream()),
               'mg_lstm_fwd_persist_bf16')
    return out, hstate, cstate, saved, hstate_bf


def lstm_bwd_bf16(grad_out, grad_hn, grad_cn, cstate, saved, w_hh, seq_len, b, t, h, want_f32=True):
    """lstm_bwd with bf16 matmul operands, one persistent launch.  Returns (dgates, dh0, dc0, dgates_bf); want_f32=False: the
    fp32 gate gradients are not written (dgates = None) - bf16 mode's GEMMs take the shadow."""
    lib = _lib.load()
    dev = grad_out.device
    dgates = torch.empty((b, t, 4 * h), dtype=torch.float32, device=dev) if want_f32 else None
    dgates_bf = torch.empty((b, t, 4 * h), dtype=torch.bfloat16, device=dev)
    dh0 = torch.empty((b, h), dtype=torch.float32, device=dev)
    dc0 = torch.empty((b, h), dtype=torch.float32, device=dev)
    wt_bf = cast_transpose_bf16(w_hh)                              # (h, 4h)
    ws = _persist_workspace(dev, b, h)
    _lib.check(lib.mg_lstm_bwd_persist_bf16(_p(grad_out), _p(grad_hn), _p(grad_cn), _p(cstate), _p(saved), _p(wt_bf), wt_bf.shape[1],
                                            _p(seq_len), b, t, h, _p(dgates), _p(dgates_bf), _p(dh0), _p(dc0), _p(ws), ws.numel(),
                                            _stream()), 'mg_lstm_bwd_persist_bf16')
    return dgates, dh0, dc0, dgates_bf


def lstm_pstack_ok(b, t, h, n_layers):
    """The whole-stack forward wavefront (mg_lstm_pstack_fwd_bf16) covers this shape."""
    return PERSISTENT_RECURRENCE and bool(_lib.load().mg_lstm_pstack_supported(b, t, h, n_layers))


def lstm_pstack_fwd(xproj0, w_ih, w_hh, b_ih, b_hh, seq_len, h0s, c0s, b, t, h):
    """L stacked LSTM layers forward in one persistent launch.  xproj0 (b,t,4h) f32 = layer 0's input projection incl. b_ih;
    w_ih[l] (l >= 1), w_hh[l] f32 (cast to bf16 here).  Returns (out of the top layer, per-layer lists hstate, cstate, saved,
    hstate_bf); of hstate[l] only the rows 0 (h0) and T (h_n) are valid."""
    lib = _lib.load()
    dev = xproj0.device
    n_layers = len(w_hh)
    hstate, cstate, saved, hstate_bf, keep, o = [], [], [], [], [], None
    descs = (_lib.mg_lstm_pstack_layer * n_layers)()
    # the state arrays of all layers in three allocations: their initial rows are set by three launches, not three per layer
    if os.environ.get('MORGANA_LSTM_BATCH_STATES', '1') != '0':
        hs_all = torch.empty((n_layers, b, t + 1, h), dtype=torch.float32, device=dev)
        cs_all = torch.empty((n_layers, b, t + 1, h), dtype=torch.float32, device=dev)
        hb_all = torch.empty((n_layers, b, t + 1, h), dtype=torch.bfloat16, device=dev)
        for state, init in ((hs_all, h0s), (cs_all, c0s), (hb_all, h0s)):
            if init is None:
                state[:, :, 0].zero_()
            else:
                state[:, :, 0].copy_(init.reshape(n_layers, b, h))
    else:
        layer_init = lambda inits, l: None if inits is None else inits[l]
        hs_all = [_initial_state(layer_init(h0s, l), b, t, h, dev) for l in range(n_layers)]
        cs_all = [_initial_state(layer_init(c0s, l), b, t, h, dev) for l in range(n_layers)]
        hb_all = [_initial_state(layer_init(h0s, l), b, t, h, dev, torch.bfloat16) for l in range(n_layers)]
    # bf16 operands of W_hh (every layer) and W_ih (layers 1..): the parameters' shadows, stale ones re-cast by one batched launch
    wh_bf = weight_operands(w_hh)
    wi_bf = [None] + weight_operands(w_ih[1:])
    for l in range(n_layers):
        hs, cs, hb = hs_all[l], cs_all[l], hb_all[l]
        if l == n_layers - 1:
            o = torch.empty((b, t, h), dtype=torch.float32, device=dev)
        sv = torch.empty((b, t, 4 * h), dtype=torch.float32, device=dev)
        whb = wh_bf[l]
        d = descs[l]
        d.w_hh_bf, d.ldwh, d.b_hh = whb.data_ptr(), whb.shape[1], b_hh[l].data_ptr()
        if l == 0:
            d.xproj = xproj0.data_ptr()
        else:
            wib = wi_bf[l]
            d.w_ih_bf, d.ldwi, d.b_ih = wib.data_ptr(), wib.shape[1], b_ih[l].data_ptr()
            keep.append(wib)
        d.hstate, d.cstate, d.hstate_bf, d.saved = hs.data_ptr(), cs.data_ptr(), hb.data_ptr(), sv.data_ptr()
        d.out = o.data_ptr() if o is not None else sv.data_ptr()         # never written below the top layer
        keep.append(whb)
        hstate.append(hs); cstate.append(cs); saved.append(sv); hstate_bf.append(hb)
    key = (dev, torch.cuda.current_stream().cuda_stream, 'pstack')
    need = lib.mg_lstm_pstack_workspace_bytes(b, h, n_layers)
    ws = _PERSIST_WORKSPACES.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            check_persistent_status()
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        _PERSIST_WORKSPACES[key] = ws
    _lib.check(lib.mg_lstm_pstack_fwd_bf16(ctypes.cast(descs, ctypes.c_void_p), n_layers, _p(seq_len), b, t, h, _p(ws), ws.numel(),
                                           _stream()), 'mg_lstm_pstack_fwd_bf16')
    return o, hstate, cstate, saved, hstate_bf


def gru_stack_small_ok(b, t, h, n_layers):
    """The small-GRU stack wavefront (mg_gru_stack_fwd_small_f32 / _bwd_small_f32) covers this shape."""
    return PERSISTENT_RECURRENCE and bool(_lib.load().mg_gru_stack_small_supported(b, t, h, n_layers))


def _gru_stack_workspace(dev):
    lib = _lib.load()
    key = (dev, torch.cuda.current_stream().cuda_stream, 'gru_stack')
    ws = _PERSIST_WORKSPACES.get(key)
    if ws is None:
        ws = torch.zeros(lib.mg_gru_stack_small_workspace_bytes(), dtype=torch.uint8, device=dev)
        _PERSIST_WORKSPACES[key] = ws
    return ws


def gru_stack_small_fwd(xproj0, w_ih, w_hh, b_ih, b_hh, seq_len, h0s, b, t, h, fast=False):
    """L stacked small GRU layers forward in one launch.  xproj0 (b,t,3h) f32 = layer 0's input projection incl. b_ih; w_ih[l], b_ih[l]
    for l >= 1 (input size == h); h0s None or (L,b,h).  Returns per-layer lists (out, hstate, saved).
    fast: the cell's sigmoid / tanh on the hardware exp / reciprocal (mg_gru_stack_fwd_small_fast_f32: throughput mode)."""
    lib = _lib.load()
    dev = xproj0.device
    n_layers = len(w_hh)
    descs = (_lib.mg_gru_stack_layer * n_layers)()
    outs, hstates, saveds = [], [], []
    for l in range(n_layers):
        hs = _initial_state(None if h0s is None else h0s[l], b, t, h, dev)
        o = torch.empty((b, t, h), dtype=torch.float32, device=dev)
        sv = torch.empty((b, t, 4 * h), dtype=torch.float32, device=dev)
        d = descs[l]
        d.w_hh, d.b_hh = w_hh[l].data_ptr(), b_hh[l].data_ptr()
        if l == 0:
            d.xproj = xproj0.data_ptr()
        else:
            d.w_ih, d.b_ih = w_ih[l].data_ptr(), b_ih[l].data_ptr()
        d.hstate, d.out, d.saved = hs.data_ptr(), o.data_ptr(), sv.data_ptr()
        outs.append(o); hstates.append(hs); saveds.append(sv)
    ws = _gru_stack_workspace(dev)
    entry = lib.mg_gru_stack_fwd_small_fast_f32 if fast else lib.mg_gru_stack_fwd_small_f32
    _lib.check(entry(ctypes.cast(descs, ctypes.c_void_p), n_layers, _p(seq_len), b, t, h, _p(ws), ws.numel(), _stream()),
               'mg_gru_stack_fwd_small_fast_f32' if fast else 'mg_gru_stack_fwd_small_f32')
    return outs, hstates, saveds


def gru_stack_small_bwd(grad_out, grad_hn, hstate, saved, w_ih, w_hh, seq_len, b, t, h, fast=False):
    """The backward of gru_stack_small_fwd in one launch.  grad_out (b,t,h) = gradient of the TOP layer's outputs; grad_hn None or a
    per-layer list of (b,h) tensors / None.  Returns per-layer lists (dxproj, dhproj) and dh0 (L,b,h)."""
    lib = _lib.load()
    dev = grad_out.device
    n_layers = len(w_hh)
    descs = (_lib.mg_gru_stack_layer * n_layers)()
    dxprojs, dhprojs, keep = [], [], []
    dh0 = torch.empty((n_layers, b, h), dtype=torch.float32, device=dev)
    for l in range(n_layers):
        d = descs[l]
        d.w_hh = w_hh[l].data_ptr()
        if l > 0:
            d.w_ih = w_ih[l].data_ptr()
        d.hstate, d.saved = hstate[l].data_ptr(), saved[l].data_ptr()
        if l + 1 == n_layers:
            d.grad_out = grad_out.data_ptr()
        else:
            dxin = torch.empty((b, t, h), dtype=torch.float32, device=dev)
            keep.append(dxin)
            d.dxin = dxin.data_ptr()
        if grad_hn is not None and grad_hn[l] is not None:
            g = _require(grad_hn[l].reshape(b, h), torch.float32, 'grad_hn')
            keep.append(g)
            d.grad_hn = g.data_ptr()
        dxp = torch.empty((b, t, 3 * h), dtype=torch.float32, device=dev)
        dhp = torch.empty((b, t, 3 * h), dtype=torch.float32, device=dev)
        d.dxproj, d.dhproj, d.dh0 = dxp.data_ptr(), dhp.data_ptr(), dh0[l].data_ptr()
        dxprojs.append(dxp); dhprojs.append(dhp)
    ws = _gru_stack_workspace(dev)
    entry = lib.mg_gru_stack_bwd_small_fast_f32 if fast else lib.mg_gru_stack_bwd_small_f32      # fast: bf16-operand products (throughput mode)
    _lib.check(entry(ctypes.cast(descs, ctypes.c_void_p), n_layers, _p(seq_len), b, t, h, _p(ws), ws.numel(), _stream()),
               'mg_gru_stack_bwd_small_fast_f32' if fast else 'mg_gru_stack_bwd_small_f32')
    return dxprojs, dhprojs, dh0


def lstm_pstack_bwd_ok(b, t, h, n_layers):
    """The whole-stack backward wavefront (mg_lstm_pstack_bwd_bf16) covers this shape."""
    return PERSISTENT_RECURRENCE and bool(_lib.load().mg_lstm_pstack_bwd_supported(b, t, h, n_layers))


def lstm_pstack_bwd(grad_out, grad_hn, grad_cn, cstate, saved, w_ih, w_hh, seq_len, b, t, h, want_f32=False):
    """L stacked LSTM layers backward in one persistent launch.  grad_out (b,t,h) f32 = gradient of the TOP layer's outputs; grad_hn /
    grad_cn None or per-layer lists of (b,h) tensors (None entries allowed); cstate[l], saved[l] from lstm_pstack_fwd; w_ih[l] (l >= 1)
    and w_hh[l] f32.  Returns per-layer lists (dgates or None, dgates_bf) and dh0, dc0 as (L,b,h) tensors."""
    lib = _lib.load()
    dev = grad_out.device
    n_layers = len(w_hh)
    descs = (_lib.mg_lstm_pstack_bwd_layer * n_layers)()
    dgates, dgates_bf, keep = [], [], []
    dh0 = torch.empty((n_layers, b, h), dtype=torch.float32, device=dev)
    dc0 = torch.empty((n_layers, b, h), dtype=torch.float32, device=dev)
    wh_t = weight_operands(w_hh, transposed=True)                        # (h, 4h) each: the parameters' shadows
    wi_t = [None] + weight_operands(w_ih[1:], transposed=True)
    for l in range(n_layers):
        d = descs[l]
        wt = wh_t[l]
        keep.append(wt)
        d.w_hh_t_bf, d.ldt = wt.data_ptr(), wt.shape[1]
        if l + 1 < n_layers:
            wu = wi_t[l + 1]                                             # (h, 4h): the layer above reads this layer's outputs
            keep.append(wu)
            d.w_ih_up_t_bf, d.ldt_up = wu.data_ptr(), wu.shape[1]
        else:
            d.grad_out = grad_out.data_ptr()
        for name, src in (('grad_hn', grad_hn), ('grad_cn', grad_cn)):
            if src is not None and src[l] is not None:
                g = _require(src[l].reshape(b, h), torch.float32, name)
                keep.append(g)
                setattr(d, name, g.data_ptr())
        dg = torch.empty((b, t, 4 * h), dtype=torch.float32, device=dev) if want_f32 else None
        dgb = torch.empty((b, t, 4 * h), dtype=torch.bfloat16, device=dev)
        d.cstate, d.saved = cstate[l].data_ptr(), saved[l].data_ptr()
        d.dgates, d.dgates_bf = (dg.data_ptr() if dg is not None else None), dgb.data_ptr()
        d.dh0, d.dc0 = dh0[l].data_ptr(), dc0[l].data_ptr()
        dgates.append(dg)
        dgates_bf.append(dgb)
    key = (dev, torch.cuda.current_stream().cuda_stream, 'pstack_bwd')
    need = lib.mg_lstm_pstack_bwd_workspace_bytes(b, h, n_layers)
    ws = _PERSIST_WORKSPACES.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            check_persistent_status()
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        _PERSIST_WORKSPACES[key] = ws
    _lib.check(lib.mg_lstm_pstack_bwd_bf16(ctypes.cast(descs, ctypes.c_void_p), n_layers, _p(seq_len), b, t, h, _p(ws), ws.numel(),
                                           _stream()), 'mg_lstm_pstack_bwd_bf16')
    return dgates, dgates_bf, dh0, dc0


def lstm_stack_fwd(descs, n_layers, seq_len, b, t, h, lag, s_begin, s_end):
    lib = _lib.load()
    _lib.check(lib.mg_lstm_stack_fwd_f32(ctypes.cast(descs, ctypes.c_void_p), n_layers, _p(seq_len), b, t, h, lag, s_begin, s_end,
                                         _stream()), 'mg_lstm_stack_fwd_f32')


def lstm_stack_bwd(descs, n_layers, seq_len, b, t, h, lag, u_begin, u_end):
    lib = _lib.load()
    _lib.check(lib.mg_lstm_stack_bwd_f32(ctypes.cast(descs, ctypes.c_void_p), n_layers, _p(seq_len), b, t, h, lag, u_begin, u_end,
                                         _stream()), 'mg_lstm_stack_bwd_f32')


# ------------------------------------------------------------------------------------------------------- optimiser
def adam_step(param, grad, exp_avg, exp_avg_sq, lr, betas, eps, weight_decay, step, grad_scale=1.0):
    lib = _lib.load()
    for name, t in (('param', param), ('grad', grad), ('exp_avg', exp_avg), ('exp_avg_sq', exp_avg_sq)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError('adam_step: %s must be a contiguous float32 device tensor' % name)
    _lib.check(lib.mg_adam_step_f32(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), float(lr),
                                    float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                                    float(grad_scale), _stream()), 'mg_adam_step_f32')


def adam_scalars(lr, betas, step):
    """(step_size, bc2_sqrt) of one Adam step as two float32, formed as mg_adam_step_f32 forms them."""
    out = (ctypes.c_float * 2)()
    _lib.load().mg_adam_scalars(float(lr), float(betas[0]), float(betas[1]), int(step), out)
    return out[0], out[1]


def store_pair(dst, a, b):
    """dst[0:2] = (a, b) in stream order; the values are kernel arguments, not a host buffer read later."""
    _lib.check(_lib.load().mg_store_pair_f32(_p(dst), float(a), float(b), _stream()), 'mg_store_pair_f32')


STORE_PAIRS_MAX = _lib.MG_STORE_PAIRS_MAX


def store_pairs(dst, pairs):
    """dst[2 j : 2 j + 2] = pairs[j] in stream order (mg_store_pairs_f32): the Adam scalars of the steps of one multi-step replay."""
    flat = (ctypes.c_float * (2 * len(pairs)))(*[float(x) for pair in pairs for x in pair])
    _lib.check(_lib.load().mg_store_pairs_f32(_p(dst), ctypes.cast(flat, ctypes.c_void_p), len(pairs), _stream()), 'mg_store_pairs_f32')


def adam_step_dev(param, grad, exp_avg, exp_avg_sq, betas, eps, weight_decay, scalars, grad_scale=1.0):
    """adam_step with (step_size, bc2_sqrt) read from the 2-float device tensor ``scalars`` (capturable in a HIP graph)."""
    lib = _lib.load()
    _lib.check(lib.mg_adam_step_dev_f32(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), float(betas[0]),
                                        float(betas[1]), float(eps), float(weight_decay), _p(scalars), float(grad_scale), _stream()),
               'mg_adam_step_dev_f32')


def adam_step_plan(param, grad, exp_avg, exp_avg_sq, betas, eps, weight_decay, scalars, grad_scale=1.0, slab_srcs=(), shadows=(),
                   clear_grad=False, tail=None):
    """The update as the last node of a step (mg_adam_step_plan_f32): ``slab_srcs`` = [(begin, count, slab tensor, n_slabs, stride)]
    are summed into the gradient on the fly (split-M partial results of the weight-gradient GEMMs, in the slab reduce's order),
    ``shadows`` = [(offset, rows, cols, bf16 [rows, ldd] or None, bf16 transpose [cols, ldt] or None)] are refreshed from the
    updated weights, ``clear_grad`` zeroes the flat gradient behind the read."""
    lib = _lib.load()
    if len(slab_srcs) > _lib.MG_ADAM_MAX_SLABS or len(shadows) > _lib.MG_ADAM_MAX_SHADOWS:
        raise ValueError('adam_step_plan: at most %d slab sources and %d shadows' % (_lib.MG_ADAM_MAX_SLABS, _lib.MG_ADAM_MAX_SHADOWS))
    plan = _lib.mg_adam_plan()
    plan.n_slab_srcs, plan.n_shadows, plan.clear_grad = len(slab_srcs), len(shadows), int(bool(clear_grad))
    for i, (begin, count, slab, n_slabs, stride) in enumerate(slab_srcs):
        src = plan.slabs[i]
        src.begin, src.count, src.slab, src.n_slabs, src.stride = int(begin), int(count), slab.data_ptr(), int(n_slabs), int(stride)
    for i, entry in enumerate(shadows):
        offset, rows, cols, dst, dst_t = entry[:5]
        sh = plan.shadows[i]
        sh.pair = int(bool(entry[5])) if len(entry) > 5 else 0        # [hi | lo] pair planes (pair_shadows)
        sh.offset, sh.rows, sh.cols = int(offset), int(rows), int(cols)
        sh.dst, sh.ldd = (dst.data_ptr(), dst.shape[1]) if dst is not None else (None, 0)
        sh.dst_t, sh.ldt = (dst_t.data_ptr(), dst_t.shape[1]) if dst_t is not None else (None, 0)
    if tail is not None:
        # the forward's deferred tail (f0_l2tail_rows_expand(defer=True) / f0_l2tail(defer=True)): the launch's first blocks repeat the
        # prediction and form the loss
        t = plan.tail
        if tail.get('rows') is not None:
            t.table, t.rows, t.frames, t.out = tail['pred_rows'].data_ptr(), tail['rows'].data_ptr(), tail['rows'].numel(), tail['out'].data_ptr()
        if tail.get('partials') is not None:
            t.partial = tail['partials'].data_ptr()
            t.n_partial = (int(tail['n_table_rows']) + 15) // 16 + (int(tail['extra']) + 3) // 4
        t.slab, t.n, t.stride, t.n_slabs, t.dst = tail['ws'].data_ptr(), int(tail['n']), int(tail['stride']), int(tail['n_slabs']), \
            tail['grads_out'].data_ptr()
    _lib.check(lib.mg_adam_step_plan_f32(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), float(betas[0]),
                                         float(betas[1]), float(eps), float(weight_decay), _p(scalars), float(grad_scale),
                                         ctypes.byref(plan), _stream()), 'mg_adam_step_plan_f32')


def grad_clip_blocks(n):
    """(chunk floats, workgroups) of mg_grad_sumsq_f32 / mg_grad_clip_scale_f32 on a buffer of ``n`` floats: a function of n alone."""
    lib = _lib.load()
    return int(lib.mg_grad_clip_chunk(int(n))), int(lib.mg_grad_clip_blocks(int(n)))


def _clip_buffer(grad, name):
    if not (isinstance(grad, torch.Tensor) and grad.is_cuda and grad.dtype == torch.float32 and grad.dim() == 1 and grad.is_contiguous()):
        raise ValueError('%s: grad must be a contiguous 1-D float32 device tensor' % name)


def grad_sumsq(grad, partials, offset):
    """partials[offset + c] = float64 sum of squares of chunk c of the flat gradient ``grad`` (mg_grad_sumsq_f32: fixed order, no
    atomics).  ``partials``: the float64 device array that all buffers sharing one norm write into, each at its own offset."""
    _clip_buffer(grad, 'grad_sumsq')
    if not (partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()):
        raise ValueError('grad_sumsq: partials must be a contiguous float64 device tensor')
    _lib.check(_lib.load().mg_grad_sumsq_f32(_p(grad), grad.numel(), _p(partials), int(offset), partials.numel(), _stream()),
               'mg_grad_sumsq_f32')


def grad_clip_scale(grad, partials, inv_world, max_norm, out=None):
    """grad *= min(1, max_norm / (sqrt(sum(partials)) * inv_world + 1e-6)) in place (mg_grad_clip_scale_f32; not written when the
    coefficient is exactly 1).  ``out``: 2 floats on the device that receive (norm, coefficient), or None."""
    _clip_buffer(grad, 'grad_clip_scale')
    if not (partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()):
        raise ValueError('grad_clip_scale: partials must be a contiguous float64 device tensor')
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= 2):
        raise ValueError('grad_clip_scale: out must hold two float32 on the device')
    _lib.check(_lib.load().mg_grad_clip_scale_f32(_p(grad), grad.numel(), _p(partials), partials.numel(), float(inv_world), float(max_norm),
                                                  _p(out), _stream()), 'mg_grad_clip_scale_f32')


def ema_update(shadow, param, decay):
    lib = _lib.load()
    if not (shadow.is_cuda and shadow.is_contiguous() and param.is_contiguous()):
        raise ValueError('ema_update: tensors must be contiguous device tensors')
    _lib.check(lib.mg_ema_update_f32(_p(shadow), _p(param), shadow.numel(), float(decay), _stream()),
               'mg_ema_update_f32')


# ----------------------------------------------------------------------------------------------------------- metrics
METRIC_MEAN, METRIC_SQDIFF, METRIC_ABSDIFF, METRIC_ROOT_SQ, METRIC_SQDIFF_VOICED, METRIC_SQDIFF_VOICED_EXP = (
    _lib.MG_METRIC_MEAN, _lib.MG_METRIC_SQDIFF, _lib.MG_METRIC_ABSDIFF, _lib.MG_METRIC_ROOT_SQ, _lib.MG_METRIC_SQDIFF_VOICED,
    _lib.MG_METRIC_SQDIFF_VOICED_EXP)


def metric_accumulate(kind, accum, target, pred=None, voiced=None, seq_len=None, col0=0, width=None):
    """accum (2,) float64 on the device: accum += (sum, count) of one batch (csrc/metrics.hip).  target / pred (B, T, D) f32."""
    lib = _lib.load()
    target = _require(target, torch.float32, 'target')
    if target.dim() != 3:
        raise ValueError('metric inputs must have shape (batch, time, features), got %s' % (tuple(target.shape),))
    b, t, d = target.shape
    width = d - col0 if width is None else width
    seq_len = _lengths(seq_len, b, 'metric_accumulate: ', flat=False)
    # accum is added to in place: a copy made here would be lost
    if (_require(accum, torch.float64, 'accum', contiguous=False).numel() != 2 or not accum.is_contiguous()
            or accum.device != target.device):
        raise ValueError('metric_accumulate: accum must be 2 contiguous float64 elements on %s, got %s' % (target.device, tuple(accum.shape)))
    if pred is not None:
        pred = _require(pred, torch.float32, 'pred')
        if pred.shape != target.shape:
            raise ValueError('target %s and prediction %s differ in shape' % (tuple(target.shape), tuple(pred.shape)))
    if voiced is not None:
        voiced = voiced.reshape(b, t).to(torch.float32).contiguous()
    ws = torch.empty(lib.mg_metric_workspace_bytes(), dtype=torch.uint8, device=target.device)
    _lib.check(lib.mg_metric_accumulate_f32(kind, _p(target), _p(pred), _p(voiced), _p(seq_len), b, t, d, col0, width, _p(accum), _p(ws),
                                            ws.numel(), _stream()), 'mg_metric_accumulate_f32')


MLPG_MAX_WINDOWS, MLPG_MAX_COEFF = _lib.MG_MLPG_MAX_WINDOWS, _lib.MG_MLPG_MAX_COEFF
MLPG_VAR_ITEM = _lib.MG_MLPG_VAR_ITEM      # variances (B, W*D), one row per utterance


def mlpg(means, variances, windows, padding_size=0, seq_len=None, out_dtype=torch.float32):
    """Most probable trajectories of (B, T, W*D) f32 delta-stream means (csrc/mlpg.hip, morgana/viz/synthesis.py:79-178).
    variances (W*D,) global, (B, T, W*D) per frame or (B, W*D) per item (one row per utterance: speaker-dependent variances, the same
    result as that row repeated over T), f32; windows [(l, u, coeffs)]; returns (B, T, D), zero past seq_len."""
    lib = _lib.load()
    means = _require(means, torch.float32, 'means')
    variances = _require(variances, torch.float32, 'variances')
    if means.dim() != 3:
        raise ValueError('means must have shape (batch, time, windows * features), got %s' % (tuple(means.shape),))
    b, t, width = means.shape
    n_win = len(windows)
    if n_win == 0 or n_win > MLPG_MAX_WINDOWS or width % n_win != 0:
        raise ValueError('%d windows for %d stream columns (1..%d windows, columns a multiple of it)' % (n_win, width, MLPG_MAX_WINDOWS))
    d = width // n_win
    if variances.dim() == 1 and variances.shape[0] == width:
        per_frame = 0
    elif variances.shape == means.shape:
        per_frame = 1
    elif variances.dim() == 2 and tuple(variances.shape) == (b, width):
        per_frame = MLPG_VAR_ITEM
    else:
        raise ValueError('variances %s fit neither (%d,) nor %s nor (%d, %d)' % (tuple(variances.shape), width, tuple(means.shape), b, width))
    win_l, win_u, win_c = _window_arrays(windows)
    if seq_len is not None:
        seq_len = _require(seq_len, torch.int64, 'seq_len')
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError('out_dtype must be torch.float32 or torch.float64')
    out = torch.empty((b, t, d), dtype=out_dtype, device=means.device)
    nbytes = lib.mg_mlpg_workspace_bytes(b, t, d, int(padding_size), n_win, win_l, win_u)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=means.device)
    _lib.check(lib.mg_mlpg_f32(_p(means), _p(variances), per_frame, _p(seq_len), b, t, d, n_win, win_l, win_u, win_c, int(padding_size),
                               _p(out), int(out_dtype == torch.float64), _p(ws), ws.numel(), _stream()), 'mg_mlpg_f32')
    return out


def mlpg_gv(means, variances, gv_mean, gv_variance, windows, padding_size=0, seq_len=None, gv_weight=1., max_iter=48,
            out_dtype=torch.float32, want_info=False):
    """``mlpg`` under a global-variance prior (csrc/mlpg_gv.hip, mg_mlpg_gv_f32; Toda & Tokuda 2007): per (utterance, dimension) the
    trajectory x that minimises  omega (x'Px/2 - x'rhs) + gv_weight/2 (v(x) - gv_mean)^2 / gv_variance  with P, rhs of ``mlpg``,
    omega = 1 / (windows x frames) and v the biased variance of x over the utterance's frames - an exact root search on the one
    multiplier of its stationarity system, inside one launch.  means, variances (all three layouts), windows, padding_size and seq_len
    as given to ``mlpg``; gv_mean and gv_variance (D,) or (B, D) f32 (tensors, arrays or sequences): mean and variance of the
    per-utterance variances (``data.fit_global_variance``).  Returns (B, T, D), zero past seq_len; with want_info also a float64
    (B, D, 4) tensor of (kappa, final |h|, evaluations used, flag), flag 1 where the plain ``mlpg`` solution came back: fewer than two
    frames, gv_weight 0, a non-positive gv_variance, or a search that did not converge.  gv_weight=0 is ``mlpg`` bit for bit."""
    lib = _lib.load()
    means = _require(means, torch.float32, 'means')
    variances = _require(variances, torch.float32, 'variances')
    if means.dim() != 3:
        raise ValueError('means must have shape (batch, time, windows * features), got %s' % (tuple(means.shape),))
    b, t, width = means.shape
    n_win = len(windows)
    if n_win == 0 or n_win > MLPG_MAX_WINDOWS or width % n_win != 0:
        raise ValueError('%d windows for %d stream columns (1..%d windows, columns a multiple of it)' % (n_win, width, MLPG_MAX_WINDOWS))
    d = width // n_win
    if variances.dim() == 1 and variances.shape[0] == width:
        per_frame = 0
    elif variances.shape == means.shape:
        per_frame = 1
    elif variances.dim() == 2 and tuple(variances.shape) == (b, width):
        per_frame = MLPG_VAR_ITEM
    else:
        raise ValueError('variances %s fit neither (%d,) nor %s nor (%d, %d)' % (tuple(variances.shape), width, tuple(means.shape), b, width))
    if not isinstance(gv_variance, torch.Tensor) or gv_variance.device.type == 'cpu':      # a host value: checked here
        if not bool((torch.as_tensor(gv_variance, dtype=torch.float64) > 0).all()):
            raise ValueError('gv_variance must be positive everywhere')
    stats = []
    for name, value in (('gv_mean', gv_mean), ('gv_variance', gv_variance)):
        value = torch.as_tensor(value).to(device=means.device, dtype=torch.float32).contiguous()
        if tuple(value.shape) not in ((d,), (b, d)):
            raise ValueError('%s %s fits neither (%d,) nor (%d, %d)' % (name, tuple(value.shape), d, b, d))
        stats.append(value)
    if stats[0].dim() != stats[1].dim():
        raise ValueError('gv_mean %s and gv_variance %s differ in layout' % (tuple(stats[0].shape), tuple(stats[1].shape)))
    gv_weight = float(gv_weight)
    if not 0.0 <= gv_weight < float('inf'):
        raise ValueError('gv_weight must be finite and >= 0, got %r' % gv_weight)
    if int(max_iter) < 3:
        raise ValueError('max_iter must be at least 3, got %r' % (max_iter,))
    win_l, win_u, win_c = _window_arrays(windows)
    if seq_len is not None:
        seq_len = _require(seq_len, torch.int64, 'seq_len')
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError('out_dtype must be torch.float32 or torch.float64')
    out = torch.empty((b, t, d), dtype=out_dtype, device=means.device)
    info = torch.empty((b, d, 4), dtype=torch.float64, device=means.device) if want_info else None
    nbytes = lib.mg_mlpg_gv_workspace_bytes(b, t, d, int(padding_size), n_win, win_l, win_u)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=means.device)
    _lib.check(lib.mg_mlpg_gv_f32(_p(means), _p(variances), per_frame, _p(stats[0]), _p(stats[1]), int(stats[0].dim() == 2), _p(seq_len),
                                  b, t, d, n_win, win_l, win_u, win_c, int(padding_size), gv_weight, int(max_iter), _p(out),
                                  int(out_dtype == torch.float64), _p(info), _p(ws), ws.numel(), _stream()), 'mg_mlpg_gv_f32')
    return (out, info) if want_info else out


def mlpg_backward(grad_out, variances, windows, padding_size=0, seq_len=None, out_dtype=torch.float32):
    """The gradient of ``mlpg``'s trajectory with respect to its means (csrc/mlpg.hip, mg_mlpg_grad_f32): grad_out (B, T, D) f32 ->
    (B, T, W*D), zero past seq_len (whose frames of grad_out are never read).  One more solve with the forward's matrix and a window
    pass; variances (all three layouts), windows, padding_size and seq_len as given to ``mlpg``.  The variances get no gradient."""
    lib = _lib.load()
    grad_out = _require(grad_out, torch.float32, 'grad_out')
    variances = _require(variances, torch.float32, 'variances')
    if grad_out.dim() != 3:
        raise ValueError('grad_out must have shape (batch, time, features), got %s' % (tuple(grad_out.shape),))
    b, t, d = grad_out.shape
    n_win = len(windows)
    if n_win == 0 or n_win > MLPG_MAX_WINDOWS:
        raise ValueError('%d windows (1..%d supported)' % (n_win, MLPG_MAX_WINDOWS))
    width = n_win * d
    if variances.dim() == 1 and variances.shape[0] == width:
        per_frame = 0
    elif tuple(variances.shape) == (b, t, width):
        per_frame = 1
    elif variances.dim() == 2 and tuple(variances.shape) == (b, width):
        per_frame = MLPG_VAR_ITEM
    else:
        raise ValueError('variances %s fit neither (%d,) nor %s nor (%d, %d)' % (tuple(variances.shape), width, (b, t, width), b, width))
    win_l, win_u, win_c = _window_arrays(windows)
    if seq_len is not None:
        seq_len = _require(seq_len, torch.int64, 'seq_len')
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError('out_dtype must be torch.float32 or torch.float64')
    grad_means = torch.empty((b, t, width), dtype=out_dtype, device=grad_out.device)
    nbytes = lib.mg_mlpg_workspace_bytes(b, t, d, int(padding_size), n_win, win_l, win_u)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=grad_out.device)
    _lib.check(lib.mg_mlpg_grad_f32(_p(grad_out), _p(variances), per_frame, _p(seq_len), b, t, d, n_win, win_l, win_u, win_c,
                                    int(padding_size), _p(grad_means), int(out_dtype == torch.float64), _p(ws), ws.numel(), _stream()),
               'mg_mlpg_grad_f32')
    return grad_means


def mlpg_backward_mv(grad_out, means, variances, windows, padding_size=0, seq_len=None, out_dtype=torch.float32):
    """The gradients of ``mlpg``'s trajectory with respect to its means AND its per-frame variances (csrc/mlpg.hip,
    mg_mlpg_grad_mv_f32): grad_out (B, T, D), means and variances (B, T, W*D) f32 -> (grad_means, grad_variances), both (B, T, W*D),
    zero past seq_len (whose frames are read in no input).  The forward's system and the adjoint one are solved side by side in one
    launch, then one window pass; grad_means equals ``mlpg_backward``'s bit for bit.  Per-frame variances only: a global (W*D,) or
    per-item (B, W*D) table is expanded by the caller, and autograd sums the expansion."""
    lib = _lib.load()
    for name, value in (('grad_out', grad_out), ('means', means), ('variances', variances)):
        if not isinstance(value, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor, got %s' % (name, type(value)))
    if grad_out.dim() != 3:
        raise ValueError('grad_out must have shape (batch, time, features), got %s' % (tuple(grad_out.shape),))
    b, t, d = grad_out.shape
    n_win = len(windows)
    if n_win == 0 or n_win > MLPG_MAX_WINDOWS:
        raise ValueError('%d windows (1..%d supported)' % (n_win, MLPG_MAX_WINDOWS))
    width = n_win * d
    if tuple(means.shape) != (b, t, width):
        raise ValueError('means %s do not fit grad_out %s under %d windows: %s wanted' % (tuple(means.shape), (b, t, d), n_win, (b, t, width)))
    if tuple(variances.shape) != (b, t, width):
        raise ValueError('mlpg_backward_mv: variances %s are not per frame %s: expand them to (B, T, W*D) (variances.expand(%d, %d, %d)) so '
                         'that autograd sums the expansion' % (tuple(variances.shape), (b, t, width), b, t, width))
    grad_out = _require(grad_out, torch.float32, 'grad_out')
    means = _require(means, torch.float32, 'means')
    variances = _require(variances, torch.float32, 'variances')
    win_l, win_u, win_c = _window_arrays(windows)
    if seq_len is not None:
        seq_len = _require(seq_len, torch.int64, 'seq_len')
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError('out_dtype must be torch.float32 or torch.float64')
    grad_means = torch.empty((b, t, width), dtype=out_dtype, device=grad_out.device)
    grad_variances = torch.empty((b, t, width), dtype=out_dtype, device=grad_out.device)
    nbytes = lib.mg_mlpg_grad_mv_workspace_bytes(b, t, d, int(padding_size), n_win, win_l, win_u)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=grad_out.device)
    _lib.check(lib.mg_mlpg_grad_mv_f32(_p(grad_out), _p(means), _p(variances), _p(seq_len), b, t, d, n_win, win_l, win_u, win_c,
                                       int(padding_size), _p(grad_means), _p(grad_variances), int(out_dtype == torch.float64), _p(ws),
                                       ws.numel(), _stream()), 'mg_mlpg_grad_mv_f32')
    return grad_means, grad_variances


DELTAS_EDGE_REPLICATE, DELTAS_EDGE_ZERO =_lib.MG_DELTAS_EDGE_REPLICATE, _lib.MG_DELTAS_EDGE_ZERO
DELTAS_EDGES = {'replicate': DELTAS_EDGE_REPLICATE, 'zero': DELTAS_EDGE_ZERO}


def _window_arrays(windows):
    """[(l, u, coeffs)] -> the parallel host arrays of mg_mlpg_f32 / mg_deltas_f32 (checked as synthesis.py:30-31 asserts)."""
    n_win = len(windows)
    if n_win == 0 or n_win > _lib.MG_MLPG_MAX_WINDOWS:
        raise ValueError('%d windows (1..%d supported)' % (n_win, _lib.MG_MLPG_MAX_WINDOWS))
    win_l = (ctypes.c_int * n_win)()
    win_u = (ctypes.c_int * n_win)()
    win_c = (ctypes.c_double * (n_win * _lib.MG_MLPG_MAX_COEFF))()
    for w, (l, u, coeff) in enumerate(windows):
        l, u = int(l), int(u)
        if l < 0 or u < 0 or len(coeff) != l + u + 1:
            raise ValueError('window %d: %d coefficients for extents l=%d, u=%d' % (w, len(coeff), l, u))
        if l + u + 1 > _lib.MG_MLPG_MAX_COEFF:
            raise ValueError('window %d is wider than %d coefficients' % (w, _lib.MG_MLPG_MAX_COEFF))
        win_l[w], win_u[w] = l, u
        for k, c in enumerate(coeff):
            win_c[w * _lib.MG_MLPG_MAX_COEFF + k] = float(c)
    return win_l, win_u, win_c


def deltas(x, windows, *, offsets=None, seq_len=None, edge='replicate', t=None, packed_rows=None, p0=None, p1=None, kind=None,
           item_row=None, want_raw=True):
    """Delta features of a float32 feature (csrc/deltas.hip, mg_deltas_f32): column w*D + d of the result at frame t is
    sum_k coeff[w][k] x[t - l_w + k, d], float64 accumulation rounded once - the forward of the operator ``mlpg`` inverts.

    Input, exactly one of: ``offsets`` (B + 1,) int64 with x the packed rows (N, D), or ``seq_len`` (B,) int64 with x padded (B, T, D)
    (frames past the length are never read).  Output, exactly one of: ``t`` - padded (B, t, W*D), zeros past each length, an item
    longer than t cut to t frames - or ``packed_rows`` - packed (packed_rows, W*D): the rows of a packed input, or the valid frames of
    a padded input back to back.  ``edge``: 'replicate' (a tap outside the item reads its first / last frame) or 'zero' (it
    contributes nothing: MLPG's window matrix).  ``kind`` (NORM_MVN / NORM_MINMAX) with p0 / p1 (W*D,) adds the normalised twin; with
    ``item_row`` (B,) int32 they are tables (S, W*D) and item b takes row item_row[b] (NaN for an index outside [0, S)).
    Returns (raw or None, normalised or None)."""
    lib = _lib.load()
    x = _require(x, torch.float32, 'feature')
    offsets, seq_len, b, t_in, d = _ragged_input('deltas', x, offsets, seq_len)
    if (t is None) == (packed_rows is None):
        raise ValueError('deltas: give exactly one of t (padded output) and packed_rows (packed output)')
    if edge not in DELTAS_EDGES:
        raise ValueError("deltas: edge must be 'replicate' or 'zero', got %r" % (edge,))
    win_l, win_u, win_c = _window_arrays(windows)
    n_win = len(windows)
    width = n_win * d
    if d == 0:
        raise ValueError('deltas: the feature has no columns')
    p0, p1, item_row, s, code = _norm_twin('deltas', kind, p0, p1, item_row, b, width,
                                           ('%d windows of %d columns need %d', n_win, d), want_raw=want_raw)
    if t is not None:
        form, rows, shape = _lib.MG_DELTAS_OUT_PADDED, int(t), (b, int(t), width)
    else:
        form, rows, shape = _lib.MG_DELTAS_OUT_PACKED, int(packed_rows), (int(packed_rows), width)
    if rows < 0:
        raise ValueError('deltas: a negative output size %d' % rows)
    raw = torch.empty(shape, dtype=torch.float32, device=x.device) if want_raw else None
    norm = torch.empty(shape, dtype=torch.float32, device=x.device) if kind is not None else None
    _lib.check(lib.mg_deltas_f32(_p(x), d, b, _p(offsets), _p(seq_len), int(t_in), n_win, win_l, win_u, win_c, DELTAS_EDGES[edge], _p(p0),
                                 _p(p1), _p(item_row), s, code, form, rows, _p(raw), _p(norm), _stream()), 'mg_deltas_f32')
    return raw, norm


F0_VOICED_ABOVE = 0.0            # a raw F0 track is 0 where unvoiced
F0_VOICED_ABOVE_LOG = -1e9       # a log-F0 track carries the HTS / Merlin marker -1e10 there


def f0_voiced_above(voiced_above, log_input):
    """The voicing threshold as the float32 the kernel and the host form compare with: the argument, or the default of the input kind."""
    if voiced_above is None:
        voiced_above = F0_VOICED_ABOVE_LOG if log_input else F0_VOICED_ABOVE
    value = ctypes.c_float(float(voiced_above)).value
    if value != value:
        raise ValueError('continuous_lf0: voiced_above is NaN: no frame would be voiced')
    return value


def continuous_lf0(x, *, offsets=None, seq_len=None, t=None, packed_rows=None, want_packed=False, log_input=False, voiced_above=None,
                   fill=0., p0=None, p1=None, kind=None, item_row=None):
    """Continuous log-F0 and voicing of a float32 F0 track (csrc/f0.hip, mg_continuous_lf0_f32), one launch: per item and column
    ``vuv = x > voiced_above`` and ``lf0 = log(x)`` (``x`` itself with ``log_input``) on voiced frames, interpolated linearly in float64
    through the unvoiced ones, the first / last voiced value held at the edges, ``fill`` for an item without a voiced frame.

    Input, exactly one of: ``offsets`` (B + 1,) int64 with x the packed rows (N, D), or ``seq_len`` (B,) int64 with x padded (B, T, D)
    (frames past the length are never read).  Outputs: ``t`` - padded (B, t, D) lf0 and vuv, zeros past each length, and with ``kind``
    (NORM_MVN / NORM_MINMAX) and p0 / p1 (D,) the normalised twin of lf0 (``item_row`` (B,) int32: tables (S, D), NaN for an index
    outside [0, S)); ``want_packed`` adds the packed lf0 (packed_rows, D) the delta and statistics kernels read next (``packed_rows``
    defaults to the rows of a packed input).  Without ``t``: ``packed_rows`` alone gives lf0 and vuv packed.
    Returns (lf0 padded or None, normalised or None, vuv, lf0 packed or None)."""
    lib = _lib.load()
    x = _require(x, torch.float32, 'f0')
    offsets, seq_len, b, t_in, d = _ragged_input('continuous_lf0', x, offsets, seq_len)
    if offsets is not None and packed_rows is None and (t is None or want_packed):
        packed_rows = x.shape[0]
    if d == 0:
        raise ValueError('continuous_lf0: the feature has no columns')
    if t is None and packed_rows is None:
        raise ValueError('continuous_lf0: give t (padded outputs), packed_rows (packed outputs) or both')
    if want_packed and packed_rows is None:
        raise ValueError('continuous_lf0: want_packed of a padded input needs packed_rows')
    if t is not None and packed_rows is not None and not want_packed:
        raise ValueError('continuous_lf0: packed_rows next to t goes with want_packed=True')
    if (t is not None and int(t) < 0) or (packed_rows is not None and int(packed_rows) < 0):
        raise ValueError('continuous_lf0: a negative output size (t=%r, packed_rows=%r)' % (t, packed_rows))
    if kind is not None and t is None:
        raise ValueError('continuous_lf0: the normalised twin is a padded output: give t')
    p0, p1, item_row, s, code = _norm_twin('continuous_lf0', kind, p0, p1, item_row, b, d, ('the feature has %d columns',))
    threshold = f0_voiced_above(voiced_above, log_input)
    padded = norm = packed = None
    if t is not None:
        padded = torch.empty((b, int(t), d), dtype=torch.float32, device=x.device)
        vuv, vuv_form = torch.empty_like(padded), _lib.MG_F0_VUV_PADDED
        norm = torch.empty_like(padded) if kind is not None else None
    else:
        vuv, vuv_form = torch.empty((int(packed_rows), d), dtype=torch.float32, device=x.device), _lib.MG_F0_VUV_PACKED
    if t is None or want_packed:
        packed = torch.empty((int(packed_rows), d), dtype=torch.float32, device=x.device)
    _lib.check(lib.mg_continuous_lf0_f32(_p(x), d, b, _p(offsets), _p(seq_len), int(t_in), 1 if log_input else 0, threshold, float(fill),
                                         _p(p0), _p(p1), _p(item_row), s, code, 0 if t is None else int(t),
                                         0 if packed_rows is None else int(packed_rows), _p(packed), _p(padded), _p(norm), _p(vuv),
                                         vuv_form, _stream()), 'mg_continuous_lf0_f32')
    return padded, norm, vuv, packed


COUNTERS_KINDS = {'full': (_lib.MG_COUNTERS_FULL, _lib.MG_COUNTERS_FULL_COLS), 'phone': (_lib.MG_COUNTERS_PHONE, _lib.MG_COUNTERS_PHONE_COLS)}


def frame_counters(dur, *, t, kind='full', seq_len=None, n_phones=None, p0=None, p1=None, norm_kind=None, item_row=None, want_raw=True,
                   blocks_per_item=None):
    """Frame-level positional features of integer durations (csrc/counters.hip, mg_frame_counters_f32), one launch.  ``dur`` int64
    (B, P) or (B, P, S) - P phones of S sub-phone states - is read in place through its strides (a ``[..., 0]`` view, a transposed view
    and a slice are not copied); a negative duration owns no frame.  For frame ``t`` of segment (p, s), i frames into the state and j
    frames into the phone, with n_s / n_p the state's / phone's length:

    ``kind='full'`` (9 columns): (i+1)/n_s, (n_s-i)/n_s, n_s, s+1, S-s, n_p, n_s/n_p, (n_p-j)/n_p, (j+1)/n_p;
    ``kind='phone'`` (3 columns): (j+1)/n_p, (n_p-j)/n_p, n_p - every quotient a float64 division rounded once to float32.

    Output (B, t, C): frames below min(t, the item's sum of durations, ``seq_len[b]`` if given) hold the counters, every other frame
    zeros; ``n_phones`` (B,) int64 drops the phones from n_phones[b] on.  ``norm_kind`` (NORM_MVN / NORM_MINMAX) with p0 / p1 (C,) adds
    the normalised twin; with ``item_row`` (B,) int32 they are tables (S, C) and item b takes row item_row[b] (NaN for an index outside
    [0, S)).  ``blocks_per_item``: workgroups per item (None: the library's choice; the bits do not depend on it).
    Returns (raw or None, normalised or None)."""
    lib = _lib.load()
    dur = _require(dur, torch.int64, 'dur', contiguous=False)
    if kind not in COUNTERS_KINDS:
        raise ValueError("frame_counters: kind must be 'full' or 'phone', got %r" % (kind,))
    code, c = COUNTERS_KINDS[kind]
    if dur.dim() not in (2, 3):
        raise ValueError('frame_counters: dur must be (B, P) or (B, P, S), got %s' % (tuple(dur.shape),))
    b, p = dur.shape[0], dur.shape[1]
    s = dur.shape[2] if dur.dim() == 3 else 1
    strides = (dur.stride(0), dur.stride(1), dur.stride(2) if dur.dim() == 3 else 0)
    if p == 0 or s == 0 or p * s > MAX_PHONES:
        raise ValueError('frame_counters: %d phones of %d states per utterance, the kernel takes 1..%d segments' % (p, s, MAX_PHONES))
    if min(strides) < 0:
        raise ValueError('frame_counters: dur has a negative stride %s' % (strides,))
    frames = int(t)
    if frames < 0:
        raise ValueError('frame_counters: a negative output size t=%r' % (t,))
    seq_len = _lengths(seq_len, b, 'frame_counters: ')
    if n_phones is not None:
        n_phones = _require(n_phones, torch.int64, 'n_phones')
        if tuple(n_phones.shape) != (b,):
            raise ValueError('frame_counters: n_phones must be (B,) = (%d,), got %s' % (b, tuple(n_phones.shape)))
    p0, p1, item_row, rows, norm_code = _norm_twin('frame_counters', norm_kind, p0, p1, item_row, b, c,
                                                   ('%r counters have %d columns', kind), kind_name='norm_kind', want_raw=want_raw)
    if blocks_per_item is not None and int(blocks_per_item) < 1:
        raise ValueError('frame_counters: blocks_per_item=%r must be positive' % (blocks_per_item,))
    raw = torch.empty((b, frames, c), dtype=torch.float32, device=dur.device) if want_raw else None
    norm = torch.empty((b, frames, c), dtype=torch.float32, device=dur.device) if norm_kind is not None else None
    if b == 0 or frames == 0:           # empty outputs: no address to hand the library
        return raw, norm
    _lib.check(lib.mg_frame_counters_f32(_p(dur), b, p, s, strides[0], strides[1], strides[2], _p(n_phones), _p(seq_len), frames, code,
                                         _p(p0), _p(p1), _p(item_row), rows, norm_code, _p(raw), _p(norm),
                                         0 if blocks_per_item is None else int(blocks_per_item), _stream()), 'mg_frame_counters_f32')
    return raw, norm


DUR_ROUNDINGS = {'carry': _lib.MG_DUR_CARRY, 'nearest': _lib.MG_DUR_NEAREST}
DUR_FLAG_INVALID, DUR_FLAG_NO_FIT, DUR_FLAG_PUSHED, DUR_FLAG_NO_ROW = (_lib.MG_DUR_FLAG_INVALID, _lib.MG_DUR_FLAG_NO_FIT,
                                                                       _lib.MG_DUR_FLAG_PUSHED, _lib.MG_DUR_FLAG_NO_ROW)
DUR_MAX_FRAMES = _lib.MG_DUR_MAX_FRAMES
DUR_MAX_ITEMS, DUR_MAX_SEGMENTS = 65535, 2 ** 24 - 1


def duration_arguments(what, scale, lo, hi, rounding):
    """The scalar arguments of the quantiser, checked -> (scale, lo, hi, rounding code); ``hi=None``: the largest the kernel takes."""
    if rounding not in DUR_ROUNDINGS:
        raise ValueError("%s: rounding must be 'carry' or 'nearest', got %r" % (what, rounding))
    scale = float(scale)
    if not 0. < scale < float('inf'):
        raise ValueError('%s: scale must be positive and finite, got %r' % (what, scale))
    if isinstance(lo, bool) or not isinstance(lo, numbers.Integral) or (hi is not None and (isinstance(hi, bool) or
                                                                                             not isinstance(hi, numbers.Integral))):
        raise TypeError('%s: the frame bounds must be integers, got %r and %r' % (what, lo, hi))
    hi = DUR_MAX_FRAMES if hi is None else int(hi)
    lo = int(lo)
    if not 0 <= lo <= hi <= DUR_MAX_FRAMES:
        raise ValueError('%s: need 0 <= lo <= hi <= %d frames, got lo=%d, hi=%d' % (what, DUR_MAX_FRAMES, lo, hi))
    return scale, lo, hi, DUR_ROUNDINGS[rounding]


def quantise_durations(pred, *, n_phones=None, p0=None, p1=None, item_row=None, log_input=False, scale=1., lo=1, hi=None, rounding='carry',
                       total=None):
    """Integer durations from a real-valued prediction (csrc/durations.hip, mg_quantise_durations_f32), one launch.  ``pred`` float32
    (B, P) or (B, P, S) - P phones of S sub-phone states - is read in place through its strides (a column slice of a wider prediction and
    a transposed view are not copied).  p0 / p1 (S,): the mean and std_dev that take ``pred`` back to frames (``pred * p1 + p0`` in
    float64); with ``item_row`` (B,) int32 they are tables (rows, S) and item b takes row item_row[b] (an index outside [0, rows): the
    item's outputs are 0 and its flags DUR_FLAG_NO_ROW); without them ``pred`` is in frames.  ``log_input``: the value is a log-duration;
    ``scale``: a speaking-rate factor on the durations; a NaN, infinite or negative value counts as 0 (DUR_FLAG_INVALID), a value above
    ``hi`` as ``hi``.  The values are rounded to 16 fractional bits and everything after is integer arithmetic:

    ``rounding='nearest'``: every segment on its own, ``max(lo, round(x))``;
    ``rounding='carry'``: the rounding error is carried along the item - every segment boundary is the rounded predicted boundary unless
    the minimum ``lo`` pushes it out (DUR_FLAG_PUSHED when that changes the item's length).

    ``total`` (B,) int64: every item's values are first scaled so that they add up to total[b] frames (DUR_FLAG_NO_FIT and no scaling
    where total[b] <= 0 or the values add up to 0).  ``n_phones`` (B,) int64 drops the phones from n_phones[b] on: never read, outputs 0.
    Returns (dur int64 shaped like pred, phone_dur int64 (B, P), n_frames int64 (B,), flags int32 (B,))."""
    lib = _lib.load()
    pred = _require(pred, torch.float32, 'pred', contiguous=False)
    scale, lo, hi, code = duration_arguments('quantise_durations', scale, lo, hi, rounding)
    if pred.dim() not in (2, 3):
        raise ValueError('quantise_durations: pred must be (B, P) or (B, P, S), got %s' % (tuple(pred.shape),))
    b, p = pred.shape[0], pred.shape[1]
    s = pred.shape[2] if pred.dim() == 3 else 1
    strides = (pred.stride(0), pred.stride(1), pred.stride(2) if pred.dim() == 3 else 0)
    if p == 0 or s == 0 or p * s > DUR_MAX_SEGMENTS:
        raise ValueError('quantise_durations: %d phones of %d states per utterance, the kernel takes 1..%d segments' % (p, s, DUR_MAX_SEGMENTS))
    if b > DUR_MAX_ITEMS:
        raise ValueError('quantise_durations: %d items, the kernel takes at most %d' % (b, DUR_MAX_ITEMS))
    if min(strides) < 0:
        raise ValueError('quantise_durations: pred has a negative stride %s' % (strides,))
    if n_phones is not None:
        n_phones = _require(n_phones, torch.int64, 'n_phones')
        if tuple(n_phones.shape) != (b,):
            raise ValueError('quantise_durations: n_phones must be (B,) = (%d,), got %s' % (b, tuple(n_phones.shape)))
    if total is not None:
        total = _require(total, torch.int64, 'total')
        if tuple(total.shape) != (b,):
            raise ValueError('quantise_durations: total must be (B,) = (%d,), got %s' % (b, tuple(total.shape)))
    rows = 0
    if p0 is None and p1 is None:
        if item_row is not None:
            raise ValueError('quantise_durations: item_row goes with the parameter tables p0 / p1')
    elif p0 is None or p1 is None:
        raise ValueError('quantise_durations: p0 and p1 go together')
    elif item_row is None:
        p0, p1 = _norm_vectors(p0, p1, s, ('the prediction has %d states per phone',))
    else:
        p0, p1, item_row = _item_tables(p0, p1, item_row, b, s, 'quantise_durations')
        rows = p0.shape[0]
    dev = pred.device
    dur = torch.empty(tuple(pred.shape), dtype=torch.int64, device=dev)
    phone_dur = torch.empty((b, p), dtype=torch.int64, device=dev)
    n_frames = torch.empty((b,), dtype=torch.int64, device=dev)
    flags = torch.empty((b,), dtype=torch.int32, device=dev)
    if b == 0:                          # empty outputs: no address to hand the library
        return dur, phone_dur, n_frames, flags
    _lib.check(lib.mg_quantise_durations_f32(_p(pred), b, p, s, strides[0], strides[1], strides[2], _p(n_phones), _p(p0), _p(p1),
                                             _p(item_row), rows, 1 if log_input else 0, scale, lo, hi, code, _p(total), _p(dur),
                                             _p(phone_dur), _p(n_frames), _p(flags), _stream()), 'mg_quantise_durations_f32')
    return dur, phone_dur, n_frames, flags


# ---------------------------------------------------------------------------------------------- vocoder features (csrc/vocoder.hip)
VOC_MAX_ORDER, VOC_MAX_WINDOW, VOC_MAX_ITEMS = _lib.MG_VOC_MAX_ORDER, _lib.MG_VOC_MAX_WINDOW, _lib.MG_VOC_MAX_ITEMS
_mcep_bases = {}


def spectrum_bins(fft_size, what='fft_size'):
    """K = fft_size / 2 + 1 bins of a power-of-two FFT size in [8, 8192]; anything else is a ValueError."""
    if isinstance(fft_size, bool) or not isinstance(fft_size, numbers.Integral) or not 8 <= fft_size <= 8192 or fft_size & (fft_size - 1):
        raise ValueError('%s=%r must be a power of two in [8, 8192]' % (what, fft_size))
    return int(fft_size) // 2 + 1


def mcep_basis_table(order, alpha, fft_size):
    """The (order, fft_size / 2 + 1) float32 table ``cos(m w~_k)`` of mg_mcep_spectrum_f32 as a host array: ``w_k = 2 pi k / fft_size``
    warped by the all-pass of ``alpha``, ``w~ = w + 2 atan(alpha sin w / (1 - alpha cos w))``, evaluated in float64, rounded once."""
    import numpy as np
    k = spectrum_bins(fft_size)
    if isinstance(order, bool) or not isinstance(order, numbers.Integral) or not 1 <= order <= VOC_MAX_ORDER:
        raise ValueError('mcep_spectrum: %r cepstral coefficients per frame, outside [1, %d]' % (order, VOC_MAX_ORDER))
    alpha = float(alpha)
    if not -1. < alpha < 1.:
        raise ValueError('mcep_spectrum: alpha=%r must lie inside (-1, 1)' % alpha)
    w = 2. * np.pi * np.arange(k, dtype=np.float64) / float(fft_size)
    warped = w + 2. * np.arctan2(alpha * np.sin(w), 1. - alpha * np.cos(w))
    return np.cos(np.arange(int(order), dtype=np.float64)[:, None] * warped[None, :]).astype(np.float32)


def mcep_basis(order, alpha, fft_size, device):
    """``mcep_basis_table`` on ``device``, built once per (order, alpha, fft_size, device) and kept."""
    device = torch.device(device)
    key = (int(order), float(alpha), int(fft_size), device.type, device.index if device.index is not None else torch.cuda.current_device())
    table = _mcep_bases.get(key)
    if table is None:
        table = _mcep_bases[key] = torch.from_numpy(mcep_basis_table(order, alpha, fft_size)).to(device)
    return table


def _vocoder_output(what, x, offsets, seq_len, cols, packed_rows, out, out_dtype, width=None):
    """What the three vocoder wrappers share -> (offsets, seq_len, B, T_in, D, packed_rows, out, out_f64): the ragged input, the rows of
    the packed output (default: the rows of a packed input, B * T of a padded one - an upper bound that needs no host read; the rows
    behind the last item are then not written) and the output buffer, allocated here unless ``out`` is given."""
    offsets, seq_len, b, t_in, d = _ragged_input(what, x, offsets, seq_len, width)
    if d == 0:
        raise ValueError('%s: the feature has no columns' % what)
    if seq_len is not None and b > VOC_MAX_ITEMS:
        raise ValueError('%s: a padded batch takes at most %d items, got %d (pack it and give offsets)' % (what, VOC_MAX_ITEMS, b))
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError('%s: out_dtype must be torch.float32 or torch.float64, got %s' % (what, out_dtype))
    if packed_rows is None:
        packed_rows = x.shape[0] if offsets is not None else b * t_in
    if isinstance(packed_rows, bool) or not isinstance(packed_rows, numbers.Integral) or packed_rows < 0:
        raise ValueError('%s: packed_rows=%r must be a non-negative integer' % (what, packed_rows))
    n_cols = d if cols is None else cols
    if out is None:
        out = torch.empty((int(packed_rows), n_cols), dtype=out_dtype, device=x.device)
    else:
        out = _require(out, out_dtype, 'out', contiguous=False)
        if out.dim() != 2 or out.shape[1] != n_cols or out.shape[0] < packed_rows or not out.is_contiguous() or out.device != x.device:
            raise ValueError('%s: out %s must be a contiguous (at least %d, %d) tensor on the input\'s device' % (
                what, tuple(out.shape), packed_rows, n_cols))
    return offsets, seq_len, b, int(t_in), d, int(packed_rows), out, 1 if out_dtype == torch.float64 else 0


def mcep_spectrum(mcep, alpha, fft_size, *, offsets=None, seq_len=None, packed_rows=None, log=False, out_dtype=torch.float32, out=None):
    """Mel-cepstrum to power spectrum (csrc/vocoder.hip, mg_mcep_spectrum_f32), one launch: ``exp(2 L)`` with
    ``L[t, k] = sum_m c[t, m] cos(m w~_k)`` over the ``fft_size / 2 + 1`` bins, ``w~`` the frequency warped by the all-pass of ``alpha``
    (``log``: ``2 L`` itself).  The cosine table is ``mcep_basis`` (float64, rounded once, cached per order, alpha, size and device).

    Input, exactly one of: ``offsets`` (B + 1,) int64 with mcep the packed rows (N, M), or ``seq_len`` (B,) int64 with mcep padded
    (B, T, M) (frames past the length are never read).  Returns the PACKED (packed_rows, fft_size / 2 + 1) tensor of ``out_dtype``
    (float64: the float32 result widened on the device); ``packed_rows`` defaults to N, or to B * T for a padded input (no host read;
    rows behind the last item are not written).  ``out``: a buffer to write into - rows from ``packed_rows`` on are left alone."""
    lib = _lib.load()
    mcep = _require(mcep, torch.float32, 'mcep')
    k = spectrum_bins(fft_size)
    offsets, seq_len, b, t_in, m, packed_rows, out, f64 = _vocoder_output('mcep_spectrum', mcep, offsets, seq_len, k, packed_rows, out,
                                                                          out_dtype)
    if b == 0 or packed_rows == 0:          # nothing to write: no address to hand the library
        return out
    basis = mcep_basis(m, alpha, fft_size, mcep.device)
    _lib.check(lib.mg_mcep_spectrum_f32(_p(mcep), m, b, _p(offsets), _p(seq_len), t_in, _p(basis), basis.shape[1], int(fft_size),
                                        1 if log else 0, f64, packed_rows, _p(out), _stream()), 'mg_mcep_spectrum_f32')
    return out


def bap_aperiodicity(bap, sample_rate, fft_size, *, offsets=None, seq_len=None, packed_rows=None, out_dtype=torch.float32, out=None):
    """Coded band aperiodicity (dB, one column per 3 kHz band) to full-band aperiodicity (csrc/vocoder.hip, mg_bap_aperiodicity_f32),
    one launch: every value clamped to [-60, 0], interpolated linearly in dB between (0 Hz, -60), (3000 i Hz, band i) and
    (sample_rate / 2, 0) at the ``fft_size / 2 + 1`` bin frequencies, then ``10 ** (dB / 20)``.  ``3000 * bands < sample_rate / 2``.
    Layouts, ``packed_rows``, ``out_dtype`` and ``out`` as ``mcep_spectrum``."""
    lib = _lib.load()
    bap = _require(bap, torch.float32, 'bap')
    k = spectrum_bins(fft_size)
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, numbers.Integral) or sample_rate <= 0:
        raise ValueError('bap_aperiodicity: sample_rate=%r must be a positive integer (Hz)' % (sample_rate,))
    offsets, seq_len, b, t_in, nb, packed_rows, out, f64 = _vocoder_output('bap_aperiodicity', bap, offsets, seq_len, k, packed_rows, out,
                                                                           out_dtype)
    if 6000 * nb >= sample_rate:
        raise ValueError('bap_aperiodicity: %d bands of 3000 Hz do not end below sample_rate / 2 = %g Hz' % (nb, sample_rate / 2.))
    if b == 0 or packed_rows == 0:          # nothing to write: no address to hand the library
        return out
    _lib.check(lib.mg_bap_aperiodicity_f32(_p(bap), nb, b, _p(offsets), _p(seq_len), t_in, int(sample_rate), int(fft_size), f64,
                                           packed_rows, _p(out), _stream()), 'mg_bap_aperiodicity_f32')
    return out


def smooth_f0(lf0, vuv, *, offsets=None, seq_len=None, packed_rows=None, window=7, threshold=0.5, out_dtype=torch.float32, out=None):
    """Log-F0 and voicing to the F0 track a vocoder takes (csrc/vocoder.hip, mg_smooth_f0_f32), one launch: per item and column
    ``exp(lf0)`` in float64, smoothed by ``scipy.signal.savgol_filter(., window, 1)`` (a moving average of ``window`` frames; the first
    and last ``window // 2`` frames on the least-squares line of the item's first / last ``window`` frames; an item shorter than the
    window, and ``window=1``, unsmoothed), then 0 wherever ``vuv <= threshold``.  ``window`` is odd, at most VOC_MAX_WINDOW.
    lf0 and vuv share one layout and shape; layouts, ``packed_rows``, ``out_dtype`` and ``out`` as ``mcep_spectrum``."""
    lib = _lib.load()
    lf0 = _require(lf0, torch.float32, 'lf0')
    vuv = _require(vuv, torch.float32, 'vuv')
    if vuv.shape != lf0.shape or vuv.device != lf0.device:
        raise ValueError('smooth_f0: vuv %s on %s does not match lf0 %s on %s' % (tuple(vuv.shape), vuv.device, tuple(lf0.shape), lf0.device))
    if isinstance(window, bool) or not isinstance(window, numbers.Integral) or window < 1 or window > VOC_MAX_WINDOW or window % 2 == 0:
        raise ValueError('smooth_f0: window=%r must be an odd integer in [1, %d]' % (window, VOC_MAX_WINDOW))
    threshold = ctypes.c_float(float(threshold)).value
    if threshold != threshold:
        raise ValueError('smooth_f0: threshold is NaN: no frame would be voiced')
    offsets, seq_len, b, t_in, d, packed_rows, out, f64 = _vocoder_output('smooth_f0', lf0, offsets, seq_len, None, packed_rows, out,
                                                                          out_dtype)
    if b == 0 or packed_rows == 0:          # nothing to write: no address to hand the library
        return out
    _lib.check(lib.mg_smooth_f0_f32(_p(lf0), _p(vuv), d, b, _p(offsets), _p(seq_len), t_in, int(window), threshold, f64, packed_rows,
                                    _p(out), _stream()), 'mg_smooth_f0_f32')
    return out


# ---------------------------------------------------------------------------------------------- vocoder analysis (csrc/analysis.hip)
_mcep_analysis = {}


def mcep_analysis_table(order, alpha, fft_size):
    """The (order, fft_size / 2 + 1) float64 table of mg_spectrum_mcep as a host array: ``c = table @ l`` takes the half log power
    spectrum ``l = 0.5 log(sp)`` of a frame to its mel-cepstrum.  It is the composition of the one-sided cepstrum on the FFT grid,
    ``g_n = (kappa_n / F) [l_0 + (-1)^n l_{F/2} + 2 sum_k l_k cos(2 pi n k / F)]``, and SPTK's ``freqt`` recursion from order F / 2 to
    ``order - 1`` with ``alpha``, run once for all K unit spectra side by side: F / 2 + 1 steps of ``order`` vector operations.  Where the
    warped series does not alias it is the left inverse of ``mcep_basis_table`` (``table @ basis.T = I`` to 2e-15)."""
    import numpy as np
    k = spectrum_bins(fft_size)
    if isinstance(order, bool) or not isinstance(order, numbers.Integral) or not 1 <= order <= VOC_MAX_ORDER:
        raise ValueError('spectrum_mcep: %r cepstral coefficients per frame, outside [1, %d]' % (order, VOC_MAX_ORDER))
    alpha = float(alpha)
    if not -1. < alpha < 1.:
        raise ValueError('spectrum_mcep: alpha=%r must lie inside (-1, 1)' % alpha)
    order, f, half = int(order), int(fft_size), int(fft_size) // 2
    cosines = np.cos(2. * np.pi * np.arange(f, dtype=np.float64) / float(f))      # cos(2 pi n k / F) = cosines[n k mod F]
    bins = np.arange(k, dtype=np.int64)
    weight = np.full(k, 2. / f)
    weight[0] = weight[half] = 1. / f
    table = np.zeros((order, k), dtype=np.float64)
    beta = 1. - alpha * alpha
    for i in range(half, -1, -1):
        g = (1. if i in (0, half) else 2.) * weight * cosines[(i * bins) % f]    # row i of the cepstrum map
        d = table.copy()
        table[0] = g + alpha * d[0]
        if order > 1:
            table[1] = beta * d[0] + alpha * d[1]
        for j in range(2, order):
            table[j] = d[j - 1] + alpha * (d[j] - table[j - 1])
    return table


def mcep_analysis_matrix(order, alpha, fft_size, device):
    """``mcep_analysis_table`` on ``device`` (float64), built once per (order, alpha, fft_size, device) and kept."""
    device = torch.device(device)
    key = (int(order), float(alpha), int(fft_size), device.type, device.index if device.index is not None else torch.cuda.current_device())
    table = _mcep_analysis.get(key)
    if table is None:
        table = _mcep_analysis[key] = torch.from_numpy(mcep_analysis_table(order, alpha, fft_size)).to(device)
    return table


def default_n_bands(sample_rate):
    """WORLD's number of coded aperiodicity bands: floor(min(15000, fs / 2 - 3000) / 3000) - 1 at 16 kHz, 2 at 22.05 kHz, 5 at 44.1 and
    48 kHz.  A rate too low for one band raises."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, numbers.Integral) or sample_rate <= 0:
        raise ValueError('sample_rate=%r must be a positive integer (Hz)' % (sample_rate,))
    bands = int(min(15000., sample_rate / 2. - 3000.) // 3000)
    if bands < 1:
        raise ValueError('a sample rate of %d Hz has no 3000 Hz band below fs / 2 - 3000 Hz' % sample_rate)
    return bands


def _analysis_input(what, x, name, fft_size):
    """A spectrum-like input of the analysis family: a float32 or float64 device tensor whose last dimension is the fft_size / 2 + 1
    bins -> (tensor contiguous, fft_size, K, in_f64)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor, got %s' % (name, type(x)))
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError('%s: %s must be torch.float32 or torch.float64, got %s' % (what, name, x.dtype))
    x = _require(x, x.dtype, name)
    if x.dim() not in (2, 3):
        raise ValueError('%s: %s must be packed (rows, bins) or padded (items, frames, bins), got %s' % (what, name, tuple(x.shape)))
    if fft_size is None:
        fft_size = 2 * (x.shape[-1] - 1)
    k = spectrum_bins(fft_size)
    if x.shape[-1] != k:
        raise ValueError('%s: %s has %d bins per frame, fft_size=%d has %d' % (what, name, x.shape[-1], fft_size, k))
    return x, int(fft_size), k, 1 if x.dtype == torch.float64 else 0


def spectrum_mcep(sp, order, alpha, fft_size=None, *, offsets=None, seq_len=None, packed_rows=None, log_input=False,
                  out_dtype=torch.float32, out=None):
    """Power spectrum to mel-cepstrum (csrc/analysis.hip, mg_spectrum_mcep), one launch: ``c = table @ (0.5 log(sp))`` per frame in
    float64 on the matrix unit, the logarithm taken once per bin.  ``table`` is ``mcep_analysis_matrix`` (the one-sided cepstrum followed
    by SPTK's ``freqt``; float64, cached per order, alpha, size and device); where the warped series does not alias this is the left
    inverse of ``mcep_spectrum``.  ``sp`` is float32 or float64 (what analysers write) and is read as it is; ``fft_size`` None is
    ``2 (bins - 1)``; ``log_input``: ``sp`` is the log power spectrum (``mcep_spectrum(..., log=True)``).  A frame with a zero, negative
    or non-finite bin comes out non-finite; no other frame changes.

    Input, exactly one of: ``offsets`` (B + 1,) int64 with sp the packed rows (N, K), or ``seq_len`` (B,) int64 with sp padded (B, T, K)
    (frames past the length are never read).  Returns the PACKED (packed_rows, order) tensor of ``out_dtype`` (float32: the float64
    result rounded once); ``packed_rows`` and ``out`` as ``mcep_spectrum``."""
    lib = _lib.load()
    sp, fft_size, k, in_f64 = _analysis_input('spectrum_mcep', sp, 'sp', fft_size)
    if isinstance(order, bool) or not isinstance(order, numbers.Integral) or not 1 <= order <= VOC_MAX_ORDER:
        raise ValueError('spectrum_mcep: %r cepstral coefficients per frame, outside [1, %d]' % (order, VOC_MAX_ORDER))
    offsets, seq_len, b, t_in, _, packed_rows, out, f64 = _vocoder_output('spectrum_mcep', sp, offsets, seq_len, int(order), packed_rows,
                                                                          out, out_dtype)
    if b == 0 or packed_rows == 0:          # nothing to write: no address to hand the library
        return out
    table = mcep_analysis_matrix(order, alpha, fft_size, sp.device)
    _lib.check(lib.mg_spectrum_mcep(_p(sp), in_f64, 1 if log_input else 0, fft_size, b, _p(offsets), _p(seq_len), t_in, _p(table),
                                    table.shape[1], int(order), f64, packed_rows, _p(out), _stream()), 'mg_spectrum_mcep')
    return out


def aperiodicity_bap(ap, sample_rate, n_bands=None, fft_size=None, *, offsets=None, seq_len=None, packed_rows=None,
                     out_dtype=torch.float32, out=None):
    """Full-band aperiodicity to coded band aperiodicity in dB (csrc/analysis.hip, mg_aperiodicity_bap), one launch: band b is
    ``20 log10(ap)`` clamped to [-60, 0], interpolated linearly between the two bins around 3000 (b + 1) Hz, in float64.  ``ap`` is
    float32 or float64 and is read as it is; ``n_bands`` None is WORLD's rule (``default_n_bands``); ``fft_size`` None is
    ``2 (bins - 1)``.  Where every anchor is a bin (16 kHz / 1024, 48 kHz / 2048) this inverts ``bap_aperiodicity``; elsewhere the round
    trip is off by up to 0.17 dB.  Layouts, ``packed_rows``, ``out_dtype`` and ``out`` as ``spectrum_mcep``."""
    lib = _lib.load()
    ap, fft_size, k, in_f64 = _analysis_input('aperiodicity_bap', ap, 'ap', fft_size)
    if n_bands is None:
        n_bands = default_n_bands(sample_rate)
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, numbers.Integral) or sample_rate <= 0:
        raise ValueError('aperiodicity_bap: sample_rate=%r must be a positive integer (Hz)' % (sample_rate,))
    if isinstance(n_bands, bool) or not isinstance(n_bands, numbers.Integral) or n_bands < 1 or 6000 * n_bands >= sample_rate:
        raise ValueError('aperiodicity_bap: %r bands of 3000 Hz do not end below sample_rate / 2 = %g Hz' % (n_bands, sample_rate / 2.))
    offsets, seq_len, b, t_in, _, packed_rows, out, f64 = _vocoder_output('aperiodicity_bap', ap, offsets, seq_len, int(n_bands),
                                                                          packed_rows, out, out_dtype)
    if b == 0 or packed_rows == 0:          # nothing to write: no address to hand the library
        return out
    _lib.check(lib.mg_aperiodicity_bap(_p(ap), in_f64, fft_size, int(sample_rate), int(n_bands), b, _p(offsets), _p(seq_len), t_in, f64,
                                       packed_rows, _p(out), _stream()), 'mg_aperiodicity_bap')
    return out


# ---------------------------------------------------------------------------------------------- waveform synthesis (csrc/synth.hip)
SYNTH_NOISE_SITE = 0x53594E00     # the Philox site of the synthesiser's noise track: one more stream
SYNTH_MIN_FFT, SYNTH_MAX_FFT, SYNTH_MAX_ITEMS = _lib.MG_SYNTH_MIN_FFT, _lib.MG_SYNTH_MAX_FFT, _lib.MG_SYNTH_MAX_ITEMS
SYNTH_WORKSPACE_BYTES = 256 << 20
_synth_tables = {}


def synth_fft_size(fft_size):
    """``fft_size`` as an int if it is a power of two in [SYNTH_MIN_FFT, SYNTH_MAX_FFT]; anything else is a ValueError."""
    if (isinstance(fft_size, bool) or not isinstance(fft_size, numbers.Integral) or not SYNTH_MIN_FFT <= fft_size <= SYNTH_MAX_FFT
            or fft_size & (fft_size - 1)):
        raise ValueError('world_synthesise: fft_size=%r must be a power of two in [%d, %d]' % (fft_size, SYNTH_MIN_FFT, SYNTH_MAX_FFT))
    return int(fft_size)


def synth_table(fft_size):
    """The (2 fft_size,) float64 table of mg_synth_responses as a host array: ``(cos, sin)(2 pi q / F)`` for q < F / 2, then the
    DC-removal window ``d[p] = .5 - .5 cos(2 pi (p + 1) / (F + 1))`` normalised to sum 1."""
    import numpy as np
    f = synth_fft_size(fft_size)
    angle = 2. * np.pi * np.arange(f // 2, dtype=np.float64) / float(f)
    d = .5 - .5 * np.cos(2. * np.pi * (np.arange(f, dtype=np.float64) + 1.) / (f + 1.))
    return np.concatenate([np.stack([np.cos(angle), np.sin(angle)], axis=1).reshape(-1), d / d.sum()])


def synth_table_on(fft_size, device):
    """``synth_table`` on ``device``, built once per (fft_size, device) and kept."""
    device = torch.device(device)
    key = (int(fft_size), device.type, device.index if device.index is not None else torch.cuda.current_device())
    table = _synth_tables.get(key)
    if table is None:
        table = _synth_tables[key] = torch.from_numpy(synth_table(fft_size)).to(device)
    return table


def synth_samples_per_frame(sample_rate, frame_period):
    """S = sample_rate * frame_period / 1000 samples per frame (frame_period in ms), at least 1; it need not be an integer."""
    for name, value in (('sample_rate', sample_rate), ('frame_period', frame_period)):
        if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) or value <= 0:
            raise ValueError('world_synthesise: %s=%r must be a positive finite number' % (name, value))
    if sample_rate > 1 << 20:
        raise ValueError('world_synthesise: sample_rate=%r Hz is above 2^20' % (sample_rate,))
    s = float(sample_rate) * float(frame_period) / 1000.
    if not 1. <= s <= float(1 << 20):
        raise ValueError('world_synthesise: %g samples per frame (sample_rate * frame_period / 1000) outside [1, 2^20]' % s)
    return s


def synth_sample_counts(n_frames, samples_per_frame):
    """Samples per utterance: ``floor((n - 1) S) + 1`` for n >= 1 frames, 0 for none - a list of Python integers."""
    return [0 if n <= 0 else int(math.floor((int(n) - 1) * samples_per_frame)) + 1 for n in n_frames]


def synth_pulse_ranges(n_pulses, fft_size, workspace_bytes=SYNTH_WORKSPACE_BYTES):
    """The plan of ``world_synthesise``: ``n_pulses`` responses of ``fft_size`` float64 each cut into ascending ranges [lo, hi) that
    fit ``workspace_bytes`` (one response at the least).  No pulse: one empty range - the overlap-add still casts the output."""
    f = synth_fft_size(fft_size)
    if isinstance(workspace_bytes, bool) or not isinstance(workspace_bytes, numbers.Integral) or workspace_bytes <= 0:
        raise ValueError('world_synthesise: workspace_bytes=%r must be a positive integer' % (workspace_bytes,))
    per = min(max(int(workspace_bytes) // (8 * f), 1), 0x7FFFFFFF)
    n_pulses = int(n_pulses)
    if n_pulses <= 0:
        return [(0, 0)]
    return [(lo, min(lo + per, n_pulses)) for lo in range(0, n_pulses, per)]


def synth_noise(total_samples, seed, used, out=None):
    """The synthesiser's N(0, 1) noise track (mg_synth_noise): float64 (total_samples,), element i from
    (seed, SYNTH_NOISE_SITE, used[0], i) - the same numbers give the same bits.  ``used``: a 1-element int64 DEVICE tensor
    (``dropout_draw``)."""
    lib = _lib.load()
    used = _require(used, torch.int64, 'used')
    if used.numel() != 1:
        raise ValueError('synth_noise: used must hold one element, got %s' % (tuple(used.shape),))
    if isinstance(total_samples, bool) or not isinstance(total_samples, numbers.Integral) or total_samples < 0:
        raise ValueError('synth_noise: total_samples=%r must be a non-negative integer' % (total_samples,))
    z = torch.empty((int(total_samples),), dtype=torch.float64, device=used.device) if out is None else out
    if total_samples:
        _lib.check(lib.mg_synth_noise(_p(z), int(total_samples), int(seed) & 0xFFFFFFFFFFFFFFFF, SYNTH_NOISE_SITE, _p(used), _stream()),
                   'mg_synth_noise')
    return z


def _synth_layout(f0, sp, ap, seq_len, offsets):
    """The host side of the ragged input of ``world_synthesise`` -> (frame_start, n_frames) as lists of Python integers and the rows
    of the feature tensors.  Needs no device: lengths given as device tensors are read once (they are host-known everywhere the
    package calls this)."""
    if (seq_len is None) == (offsets is None):
        raise ValueError('world_synthesise: exactly one of seq_len (padded (B, T, K) input) and offsets (packed (rows, K) input) must be given')
    for name, x in (('sp', sp), ('ap', ap)):
        if not isinstance(x, torch.Tensor):
            raise TypeError('world_synthesise: %s must be a torch.Tensor, got %s' % (name, type(x)))
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError('world_synthesise: %s must be torch.float32 or torch.float64, got %s' % (name, x.dtype))
    if not isinstance(f0, torch.Tensor):
        raise TypeError('world_synthesise: f0 must be a torch.Tensor, got %s' % type(f0))
    if sp.shape != ap.shape:
        raise ValueError('world_synthesise: sp %s and ap %s differ in shape' % (tuple(sp.shape), tuple(ap.shape)))
    lengths = (seq_len if seq_len is not None else offsets)
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().reshape(-1).cpu().tolist()
    lengths = [int(v) for v in lengths]
    if seq_len is not None:
        if sp.dim() != 3:
            raise ValueError('world_synthesise: with seq_len, sp must be padded (B, T, K), got %s' % (tuple(sp.shape),))
        b, t = sp.shape[:2]
        if len(lengths) != b:
            raise ValueError('world_synthesise: seq_len holds %d lengths for %d items' % (len(lengths), b))
        n_frames = [min(max(n, 0), t) for n in lengths]
        frame_start = [i * t for i in range(b)]
        rows = b * t
    else:
        if sp.dim() != 2:
            raise ValueError('world_synthesise: with offsets, sp must be packed (rows, K), got %s' % (tuple(sp.shape),))
        rows = sp.shape[0]
        if not lengths or lengths[0] < 0 or any(hi < lo for lo, hi in zip(lengths, lengths[1:])) or lengths[-1] > rows:
            raise ValueError('world_synthesise: offsets must be (B + 1,) ascending inside the %d packed rows' % rows)
        n_frames = [hi - lo for lo, hi in zip(lengths, lengths[1:])]
        frame_start = lengths[:-1]
    if f0.numel() != rows:
        raise ValueError('world_synthesise: f0 %s does not hold one value for each of the %d frames of sp' % (tuple(f0.shape), rows))
    if len(n_frames) > SYNTH_MAX_ITEMS:
        raise ValueError('world_synthesise: at most %d utterances, got %d' % (SYNTH_MAX_ITEMS, len(n_frames)))
    return frame_start, n_frames, rows


def world_synthesise(f0, sp, ap, sample_rate, frame_period=5., seq_len=None, *, offsets=None, noise=None, seed=None, used=None,
                     out_dtype=torch.float32, workspace_bytes=SYNTH_WORKSPACE_BYTES, want_info=False, out=None, timings=None):
    """WORLD-style waveform synthesis of a batch (csrc/synth.hip; the definition is include/morgana_hip.h K34): pulse positions from
    the F0 track by an integer phase scan, per pulse a minimum-phase periodic response and a shaped-noise response from the
    interpolated ``sp`` and ``ap`` (real FFTs of size ``2 (K - 1)`` in LDS, float64), and an overlap-add in ascending pulse order.

    f0 : one value per frame, 0 where unvoiced (any float dtype; padded (B, T) / (B, T, 1) or packed (rows,) / (rows, 1));
    sp, ap : power spectrum and aperiodicity in [0, 1], float32 or float64, read in place - padded (B, T, K) with ``seq_len`` (B,)
    or packed (rows, K) with ``offsets`` (B + 1,).  The lengths must be known to the host (a device tensor is read once).
    noise : the float64 N(0, 1) track of the packed samples (total_samples,); None draws it with ``synth_noise(total, seed, used)`` -
    ``seed`` None is ``dropout_seed()``, ``used`` None reserves one draw of the device step counter (two calls then differ).
    workspace_bytes : the budget of the responses of one pulse range; the output's bits do not depend on it.

    Returns (wav (total_samples,) of ``out_dtype`` - float32 is the float64 waveform rounded once -, sample_offsets (B + 1,) int64 on
    the device); utterance b is ``wav[sample_offsets[b]:sample_offsets[b + 1]]``, ``floor((n_b - 1) S) + 1`` samples.  ``out``: a
    buffer of at least total_samples elements to write into.  ``want_info``: also a dict of the pulse arrays (``index``, ``delta``,
    ``period``, ``voiced``: the padded-by-capacity records, ``region_offsets`` and ``counts`` to cut them with, and ``ranges``).
    ``timings``: a dict that receives, per kernel name, the (start, end) device events of its launches (scripts/bench_synth.py).
    The pulse counts are read back once, (B,) integers: this operator ends in host arrays and cannot be captured into a graph.
    There is no host implementation: without the HIP library this raises."""
    import numpy as np
    frame_start, n_frames, rows = _synth_layout(f0, sp, ap, seq_len, offsets)
    s_per = synth_samples_per_frame(sample_rate, frame_period)
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError('world_synthesise: out_dtype must be torch.float32 or torch.float64, got %s' % (out_dtype,))
    fft_size = synth_fft_size(2 * (sp.shape[-1] - 1))
    synth_pulse_ranges(0, fft_size, workspace_bytes)          # the budget's own checks, before anything is launched
    if sample_rate > 500 * fft_size:
        raise ValueError('world_synthesise: sample_rate=%r above 500 * fft_size = %d Hz: the 500 Hz unvoiced pulses would lie more than '
                         'fft_size samples apart' % (sample_rate, 500 * fft_size))
    counts_n = synth_sample_counts(n_frames, s_per)
    b = len(n_frames)
    sample_off = np.zeros(b + 1, np.int64)
    np.cumsum(counts_n, out=sample_off[1:])
    region_off = np.zeros(b + 1, np.int64)
    np.cumsum([n // 2 + 1 for n in counts_n], out=region_off[1:])
    total, capacity = int(sample_off[-1]), int(region_off[-1])
    if any(n >= 1 << 31 for n in counts_n):
        raise ValueError('world_synthesise: an utterance of 2^31 samples or more')

    lib = _lib.load()
    sp = _require(sp, sp.dtype, 'sp')
    ap = _require(ap, ap.dtype, 'ap')
    dev = sp.device
    f0 = _require(f0, f0.dtype, 'f0').reshape(-1).to(torch.float64)
    if ap.device != dev or f0.device != dev:
        raise ValueError('world_synthesise: f0, sp and ap live on different devices')
    if noise is not None:
        noise = _require(noise, torch.float64, 'noise')
        if noise.dim() != 1 or noise.shape[0] < total or noise.device != dev:
            raise ValueError('world_synthesise: noise %s must be a float64 (at least %d,) tensor on the input\'s device' % (
                tuple(noise.shape), total))
    if out is None:
        out = torch.empty((total,), dtype=out_dtype, device=dev)
    else:
        out = _require(out, out_dtype, 'out', contiguous=False)
        if out.dim() != 1 or out.shape[0] < total or not out.is_contiguous() or out.device != dev:
            raise ValueError('world_synthesise: out %s must be a contiguous (at least %d,) tensor on the input\'s device' % (
                tuple(out.shape), total))
    wav = out[:total]
    layout = torch.from_numpy(np.concatenate([np.asarray(frame_start, np.int64).reshape(-1), np.asarray(n_frames, np.int64).reshape(-1),
                                              sample_off, region_off])).to(dev)
    frame_start_d, n_frames_d = layout[:b], layout[b:2 * b]
    sample_off_d, region_off_d = layout[2 * b:3 * b + 1], layout[3 * b + 1:]
    index = torch.zeros((capacity,), dtype=torch.int32, device=dev)
    delta = torch.zeros((capacity,), dtype=torch.float64, device=dev)
    period = torch.zeros((capacity,), dtype=torch.int32, device=dev)
    voiced = torch.zeros((capacity,), dtype=torch.int32, device=dev)
    counts = torch.zeros((b,), dtype=torch.int64, device=dev)
    info = {'index': index, 'delta': delta, 'period': period, 'voiced': voiced, 'region_offsets': region_off, 'counts': np.zeros(b, np.int64),
            'ranges': []}
    if b == 0 or total == 0:              # an empty batch launches nothing
        return (wav, sample_off_d, info) if want_info else (wav, sample_off_d)

    def timed(name, rc):
        _lib.check(rc, name)
        if timings is not None:
            end = torch.cuda.Event(enable_timing=True)
            end.record()
            timings.setdefault(name, []).append((mark[0], end))
            mark[0] = torch.cuda.Event(enable_timing=True)
            mark[0].record()

    mark = [None]
    if timings is not None:
        mark[0] = torch.cuda.Event(enable_timing=True)
        mark[0].record()
    timed('mg_synth_pulses', lib.mg_synth_pulses(
        _p(f0), b, _p(frame_start_d), _p(n_frames_d), _p(sample_off_d), _p(region_off_d), s_per, float(sample_rate),
        4294967296. / float(sample_rate), fft_size, _p(index), _p(delta), _p(period), _p(voiced), _p(counts), _stream()))
    if noise is None:
        noise = synth_noise(total, dropout_seed() if seed is None else seed, dropout_draw(dev) if used is None else used)
    counts_host = counts.cpu().numpy()                        # the one read: (B,) integers
    pulse_off = np.zeros(b + 1, np.int64)
    np.cumsum(counts_host, out=pulse_off[1:])
    pulse_off_d = torch.from_numpy(pulse_off).to(dev)
    ranges = synth_pulse_ranges(int(pulse_off[-1]), fft_size, workspace_bytes)
    info['counts'], info['ranges'] = counts_host, ranges
    y = wav if out_dtype == torch.float64 else torch.empty((total,), dtype=torch.float64, device=dev)
    y.zero_()
    table = synth_table_on(fft_size, dev)
    space = workspace(max(hi - lo for lo, hi in ranges) * fft_size * 8, dev)
    if timings is not None:
        mark[0] = torch.cuda.Event(enable_timing=True)
        mark[0].record()
    for r, (lo, hi) in enumerate(ranges):
        timed('mg_synth_responses', lib.mg_synth_responses(
            _p(sp), int(sp.dtype == torch.float64), _p(ap), int(ap.dtype == torch.float64), b, _p(frame_start_d), _p(n_frames_d),
            _p(sample_off_d), _p(region_off_d), _p(pulse_off_d), _p(index), _p(delta), _p(period), _p(voiced), _p(noise), _p(table), s_per,
            fft_size, lo, hi, _p(space), _stream()))
        timed('mg_synth_overlap_add', lib.mg_synth_overlap_add(
            _p(space), b, _p(sample_off_d), _p(region_off_d), _p(pulse_off_d), _p(index), fft_size, lo, hi, total, _p(y),
            int(r == len(ranges) - 1), int(out_dtype == torch.float64), _p(wav), _stream()))
    return (wav, sample_off_d, info) if want_info else (wav, sample_off_d)


# ---------------------------------------------------------------------------------------------- phone-rate first layer
# MORGANA_PHONE_RATE=0: every product at frame rate (the reference's order of operations).  This is only the DEFAULT of a per-call
# choice: utils.upsample_to_repetitions(..., phone_rate=) records the choice on the lazy sequence it returns, the layers that consume
# the sequence read it there (models pass their own ``phone_rate`` attribute), so two models with different orders of operations
# live in one process without anybody writing a global.
PHONE_RATE = os.environ.get('MORGANA_PHONE_RATE', '1') != '0'


def phone_rate_choice(choice=None):
    """The order of operations a call asks for: ``choice`` if given, else the process default (MORGANA_PHONE_RATE)."""
    return PHONE_RATE if choice is None else bool(choice)
PHONE_RATE_EXTRA = 1024          # rows behind the table that collect the gradients of padding frames (for the bias gradient)


def segment_bounds(rows, n_table_rows, pad_row=None):
    """(2, R) int32 frame runs per table row; with ``pad_row`` also the map with -1 replaced by that row (returned second)."""
    lib = _lib.load()
    rows = _require(rows, torch.int32, 'rows')
    seg = torch.empty((2, n_table_rows), dtype=torch.int32, device=rows.device)
    mapped = torch.empty_like(rows) if pad_row is not None else None
    _lib.check(lib.mg_segment_bounds(_p(rows), rows.numel(), n_table_rows, _p(seg[0]), _p(seg[1]), _p(mapped),
                                     -1 if pad_row is None else int(pad_row), _stream()), 'mg_segment_bounds')
    return seg if pad_row is None else (seg, mapped)


def phone_rate_table_ok(n_table_rows, m, n0, n1, act, enabled=None):
    """The table form of the phone-rate first layer (bf16 mode): sigmoid(X_phone W0^T + b0) is kept per phone and the second
    layer's GEMMs gather its rows, so the frame-rate activation never exists.  Needs the wide-tile kernels' shapes."""
    return (phone_rate_choice(enabled) and act == ACT_SIGMOID and n_table_rows < m and m >= 4096 and n_table_rows >= 2048
            and n0 % 128 == 0 and 384 < n0 <= 512 and pad8(n1) % 64 == 0)


def phone_rate_gru_ok(n_table_rows, m, width, enabled=None):
    """Linear / Sigmoid layers between an upsample and a GRU wrapper on the phone rows (utils.PhoneTable): worth it when there are
    several frames per phone; the table's width must suit mg_segment_sum (multiple of 8)."""
    return phone_rate_choice(enabled) and width % 8 == 0 and 2 * (n_table_rows + PHONE_RATE_EXTRA) <= m


def linear_dgrad_gathered_bf16(dy, m, n, wt_bf16, k, h_table, h_rows):
    """linear_dgrad_bf16 with the sigmoid outputs read from the per-phone table: dx[f] = (dy[f] W) h (1 - h), h = h_table[h_rows[f]]."""
    lib = _lib.load()
    dx = torch.empty((m, pad8(k)), dtype=torch.bfloat16, device=dy.device)
    _lib.check(lib.mg_linear_dgrad_gathered_bf16(_p(dy), dy.shape[1], m, n, _p(wt_bf16), wt_bf16.shape[1], k, _p(h_table),
                                                 h_table.shape[1], _p(h_rows), _p(dx), dx.shape[1], 0, _stream()),
               'mg_linear_dgrad_gathered_bf16')
    return dx


def phone_concat_layer(table_bf16, k_lab, rows_mapped, feat, w, w_bf16, bias, n, act, out_f32=False):
    """First Linear of ``cat(upsampled lab, frame counters)`` with the lab part at phone rate: ``act(P[rows] + feat W_cnt^T + b)``
    with P = table W_lab^T (one small GEMM, f32).  table_bf16 (R + extra, ld) bf16; feat (M, C) f32; w (n, k_lab + C) f32 and
    its bf16 copy w_bf16 (n, ldw).  Returns (M, pad8(n)) bf16 - the operand of the next layer - or (M, n rounded up to 8) f32."""
    lib = _lib.load()
    feat = _require(feat, torch.float32, 'frame features')
    w = _require(w, torch.float32, 'weight')
    m, c = feat.shape
    part = linear_fwd_bf16(table_bf16, None, table_bf16.shape[0], k_lab, w_bf16, None, n, ACT_NONE, out_f32=True)
    y = torch.empty((m, (n + 7) // 8 * 8 if out_f32 else pad8(n)), dtype=torch.float32 if out_f32 else torch.bfloat16, device=feat.device)
    _lib.check(lib.mg_phone_concat_layer_bf16(_p(part), part.shape[1], _p(rows_mapped), m, _p(feat), c, _p(w), w.shape[1], k_lab, _p(bias), n,
                                              act, _p(y), y.shape[1], int(bool(out_f32)), _stream()), 'mg_phone_concat_layer_bf16')
    return y


def segment_sum_feat(g, rows, seg, n_table_rows, n, feat, extra=PHONE_RATE_EXTRA):
    """``segment_sum`` of a bf16 gradient plus, from the same pass, the slabs of the frame features' weight gradient (g^T feat):
    returns (sums (R + extra, ld) bf16, slabs) - ``feat_wgrad_reduce`` adds the slabs into the features' columns of dW."""
    lib = _lib.load()
    g = _require(g, torch.bfloat16, 'gradient')
    feat = _require(feat, torch.float32, 'frame features')
    if g.data_ptr() % 16:
        raise ValueError('segment_sum_feat: the gradient must start on a 16-byte boundary')
    c = feat.shape[1]
    out = torch.empty((n_table_rows + extra, g.shape[1]), dtype=g.dtype, device=g.device)
    nbytes = lib.mg_segment_sum_feat_workspace_bytes(c, out.shape[1])
    slabs = torch.empty((nbytes // 4,), dtype=torch.float32, device=g.device)
    _lib.check(lib.mg_segment_sum_feat_bf16(_p(g), g.shape[1], _p(rows), rows.numel(), _p(seg[0]), _p(seg[1]), n_table_rows, extra, n, _p(out),
                                            out.shape[1], _p(feat), c, _p(slabs), nbytes, _stream()), 'mg_segment_sum_feat_bf16')
    return out, slabs


def feat_wgrad_reduce(slabs, c, ldo, n, dw, col0, accumulate=True):
    """dw[:, col0 : col0 + c] (+)= the sum of segment_sum_feat's slabs; dw (n, ldw) f32 contiguous."""
    lib = _lib.load()
    _lib.check(lib.mg_feat_wgrad_reduce(_p(slabs), c, ldo, n, _p(dw), dw.shape[1], col0, int(bool(accumulate)), _stream()), 'mg_feat_wgrad_reduce')


def segment_sum(g, rows, seg, n_table_rows, n, extra=PHONE_RATE_EXTRA):
    """(R + extra, ld) sums of the frame-rate rows of g per table row; the extra rows take the frames with row -1."""
    lib = _lib.load()
    bf16 = g.dtype == torch.bfloat16
    g = _require(g, torch.bfloat16 if bf16 else torch.float32, 'gradient')
    if g.data_ptr() % 16:
        raise ValueError('segment_sum: the gradient must start on a 16-byte boundary (the kernel reads 16 bytes per lane)')
    out = torch.empty((n_table_rows + extra, g.shape[1]), dtype=g.dtype, device=g.device)
    _lib.check(lib.mg_segment_sum(_p(g), g.shape[1], int(bf16), _p(rows), rows.numel(), _p(seg[0]), _p(seg[1]), n_table_rows, extra, n,
                                  _p(out), out.shape[1], _stream()), 'mg_segment_sum')
    return out
