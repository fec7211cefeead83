"""Frames of different sizes without a GPU: the layout of a `FrameBatch` (utils/frames.py) and the argument checks of everything that
takes one.  Bad arguments raise RuntimeError before the native library or the device is touched, so all of this runs on a CPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import draw_ref as R
from yolact_minimal_amd import hip
from yolact_minimal_amd.utils.frames import FrameBatch, frame_layout

SIZES = [(1, 1), (5, 7), (37, 53), (64, 130), (97, 301), (120, 128), (480, 640), (3, 85), (85, 3)]


@pytest.mark.parametrize('itemsize', [1, 4])
def test_frame_layout_alignment_order_and_total(itemsize):
    offsets, total = frame_layout(SIZES, itemsize)
    assert len(offsets) == len(SIZES) and offsets[0] == 0
    end = 0
    for (h, w), o in zip(SIZES, offsets):
        assert (o * itemsize) % 256 == 0, 'every frame starts at a multiple of 256 bytes'
        assert o >= end, 'frames are disjoint and in order'
        assert o - end < 256 // itemsize, 'no more than the alignment gap between two frames'
        end = o + h * w * 3
    assert total == end, 'total ends the last frame'


def test_frame_layout_is_ragged_layouts_rule():
    """One table type serves frames and mask blocks: a frame is a mask block of 3 * w "pixels" per row and one detection."""
    from yolact_minimal_amd.utils.output_utils import ragged_layout
    assert frame_layout(SIZES, 4) == ragged_layout([(h, 3 * w) for h, w in SIZES], 1)


@pytest.mark.parametrize('sizes', [[], [(4, 4)] * 33, [(0, 5)], [(5, 0)], [(4, 4), (-1, 3)], [(4, 4), (3, -2)]],
                         ids=['none', '33', 'h0', 'w0', 'h-1', 'w-2'])
def test_frame_layout_raises(sizes):
    with pytest.raises(RuntimeError):
        frame_layout(sizes)


def test_frame_layout_error_texts_are_ragged_layouts():
    from yolact_minimal_amd.utils.output_utils import ragged_layout
    for sizes in ([], [(4, 4)] * 33, [(0, 5)]):
        with pytest.raises(RuntimeError) as a:
            frame_layout(sizes)
        with pytest.raises(RuntimeError) as b:
            ragged_layout(sizes, 1)
        assert str(a.value).replace('frame_layout', 'ragged_layout') == str(b.value)


def test_ragged_image_mirror_is_16_bytes():
    assert ctypes.sizeof(hip.RaggedImage) == 16
    assert hip.RaggedImage.offset.offset == 8 and hip.RAGGED_MAX_IMAGES == 32 and hip.RAGGED_ALIGN_BYTES == 256


def test_the_three_entries_are_declared_and_bound():
    for name in ('ym_val_preprocess_batch', 'ym_draw_detections_ragged', 'ym_draw_detections_ragged_packed'):
        assert name in hip.ABI_SYMBOLS
        assert getattr(hip.lib(), name).argtypes is not None


def _no_library(monkeypatch):
    def boom():
        raise AssertionError('the native library was touched')
    monkeypatch.setattr(hip, 'lib', boom)


def _host_batch(sizes):
    _, total = frame_layout(sizes)
    return FrameBatch(torch.zeros(total, dtype=torch.uint8), sizes)


def test_frame_batch_views_on_a_host_buffer():
    fb = _host_batch(SIZES[:4])
    assert len(fb) == 4 and [tuple(f.shape) for f in fb.frames] == [(h, w, 3) for h, w in SIZES[:4]]
    fb.frames[2].fill_(7)
    o = fb.offsets[2]
    assert int(fb.data.sum()) == 7 * 37 * 53 * 3 and int(fb.data[o:o + 37 * 53 * 3].min()) == 7
    with pytest.raises(RuntimeError):
        FrameBatch(torch.zeros(10, dtype=torch.uint8), [(5, 7)])            # buffer too small
    with pytest.raises(RuntimeError):
        FrameBatch(torch.zeros(4, 4, dtype=torch.uint8), [(1, 1)])          # not flat
    with pytest.raises(RuntimeError):
        FrameBatch(torch.zeros(64, dtype=torch.int32), [(1, 1)])            # wrong dtype


def test_from_tensors_refuses_bad_arguments(monkeypatch):
    _no_library(monkeypatch)
    ok = torch.zeros(5, 7, 3, dtype=torch.uint8)
    for bad in ([ok],                                                        # CPU tensors
                [],                                                          # empty list
                [ok] * 33,                                                   # more than 32
                [torch.zeros(5, 7, 3, dtype=torch.int32)],                   # dtype
                [torch.zeros(5, 7, dtype=torch.uint8)],                      # rank
                [torch.zeros(5, 7, 4, dtype=torch.uint8)],                   # channels
                [ok, ok.float()],                                            # mixed dtypes
                [np.zeros((5, 7, 3), np.uint8)],                             # numpy where tensors are required
                ok):                                                         # not a list
        with pytest.raises(RuntimeError):
            FrameBatch.from_tensors(bad)


def test_from_numpy_refuses_bad_arguments(monkeypatch):
    _no_library(monkeypatch)
    ok = np.zeros((5, 7, 3), np.uint8)
    for bad in ([], [ok] * 33, [ok.astype(np.float32)], [ok[:, :, 0]], [torch.zeros(5, 7, 3, dtype=torch.uint8)], ok):
        with pytest.raises(RuntimeError):
            FrameBatch.from_numpy(bad, 'cuda:0')
    with pytest.raises(RuntimeError):
        FrameBatch.from_numpy([ok], 'cpu')


def test_val_aug_batch_refuses_cpu_inputs(monkeypatch):
    from yolact_minimal_amd.utils.augmentations import val_aug_batch
    _no_library(monkeypatch)
    with pytest.raises(RuntimeError):
        val_aug_batch([torch.zeros(5, 7, 3, dtype=torch.uint8)], 64)
    with pytest.raises(RuntimeError):
        val_aug_batch(_host_batch([(5, 7), (3, 3)]), 64)
    with pytest.raises(RuntimeError):
        val_aug_batch([], 64)
    with pytest.raises(RuntimeError):
        val_aug_batch([torch.zeros(5, 7, 3, dtype=torch.uint8)] * 33, 64)


def test_draw_batch_with_a_frame_batch_refuses_cpu_inputs(monkeypatch):
    from yolact_minimal_amd.utils.draw import draw_batch
    _no_library(monkeypatch)
    sizes = [(5, 7), (8, 8)]
    md = 3
    dets = (torch.zeros(2, md, dtype=torch.int64), torch.zeros(2, md), torch.zeros(2, md, 4, dtype=torch.int32),
            [torch.zeros(md, h, w) for h, w in sizes], torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        draw_batch(dets, _host_batch(sizes), R.make_cfg())
    with pytest.raises(RuntimeError):
        draw_batch(dets, _host_batch(sizes), R.make_cfg(hide_mask=True))


def test_submit_frames_checks_the_length_first(monkeypatch):
    from yolact_minimal_amd.pipeline import RequestPipeline
    _no_library(monkeypatch)
    pipe = RequestPipeline.__new__(RequestPipeline)             # (no engines: the checks come before anything that needs them)
    pipe.batch, pipe.with_post, pipe.vt, pipe.cfg = 3, True, 0.0, SimpleNamespace()
    with pytest.raises(RuntimeError, match='2 frames for a pipeline of batch 3'):
        pipe.submit_frames(_host_batch([(5, 7), (8, 8)]))
    with pytest.raises(RuntimeError):
        pipe.submit_frames([torch.zeros(5, 7, 3, dtype=torch.uint8)] * 3)          # not a FrameBatch
    with pytest.raises(RuntimeError):
        pipe.submit_frames(_host_batch([(5, 7), (8, 8), (2, 2)]))                   # right length, frames on the host


# ---- the C entries' own table checks: refused on the host before any launch, so no device is needed ------------------------------
def _table(entries):
    return (hip.RaggedImage * len(entries))(*[hip.RaggedImage(*e) for e in entries])


def _val_batch_rc(entries, batch=None, is_uint8=1, size=64):
    lib = hip.lib()
    three = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    mem = torch.zeros(4096, dtype=torch.uint8)                      # a non-null pointer; a refused call never follows it
    p = ctypes.c_void_p(mem.data_ptr())
    rc = lib.ym_val_preprocess_batch(p, is_uint8, _table(entries), len(entries) if batch is None else batch, size, three, three, p, None)
    return rc, lib.ym_last_error().decode()


@pytest.mark.parametrize('entries, batch, is_uint8, text', [
    ([(4, 4, 0)], 0, 1, 'images per call'),
    ([(4, 4, 256 * i) for i in range(33)], 33, 1, 'images per call'),
    ([(0, 4, 0)], None, 1, 'is 0 x 4'),
    ([(4, 4, 0), (4, -1, 256)], None, 1, 'is 4 x -1'),
    ([(4, 4, 0), (4, 4, 100)], None, 1, 'not a multiple of 256 bytes'),
    ([(4, 4, 0), (4, 4, 32)], None, 0, 'not a multiple of 256 bytes'),           # float32 frames: 32 floats are 128 bytes
    ([(4, 4, 0), (4, 4, -256)], None, 1, 'not a multiple of 256 bytes'),
    ([(16, 16, 0), (4, 4, 256)], None, 1, 'overlap'),                            # 16 * 16 * 3 = 768 bytes reach past 256
    ([(4, 4, 512), (16, 16, 0)], None, 1, 'overlap'),                            # order does not matter
    ([(16, 16, 0), (4, 4, 64)], None, 0, 'overlap'),                             # in floats
], ids=['B0', 'B33', 'h0', 'w-1', 'misaligned', 'misaligned_f32', 'negative', 'overlap', 'overlap_unordered', 'overlap_f32'])
def test_val_preprocess_batch_refuses_bad_tables(entries, batch, is_uint8, text):
    rc, err = _val_batch_rc(entries, batch, is_uint8)
    assert rc == -1 and text in err, (rc, err)                       # YM_EINVAL


def test_val_preprocess_batch_refuses_null_pointers_and_sizes():
    lib = hip.lib()
    three = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    mem = torch.zeros(64, dtype=torch.uint8)
    p = ctypes.c_void_p(mem.data_ptr())
    tab = _table([(4, 4, 0)])
    assert lib.ym_val_preprocess_batch(None, 1, tab, 1, 64, three, three, p, None) == -1
    assert lib.ym_val_preprocess_batch(p, 1, tab, 1, 64, three, three, None, None) == -1
    assert lib.ym_val_preprocess_batch(p, 1, None, 1, 64, three, three, p, None) == -1
    assert lib.ym_val_preprocess_batch(p, 1, tab, 1, 0, three, three, p, None) == -1


def _draw_ragged_rc(frames, blocks, packed=False, flags=0, max_det=2):
    lib = hip.lib()
    batch = len(frames)
    mem = torch.zeros(1 << 16, dtype=torch.uint8)                   # 64-byte aligned host memory standing in for every buffer
    p = ctypes.c_void_p(mem.data_ptr())
    fn = lib.ym_draw_detections_ragged_packed if packed else lib.ym_draw_detections_ragged
    rc = fn(p, p, p, p, p, p, batch, max_det, _table(frames), _table(blocks) if blocks is not None else None, p, 100, 81, p, 80, p,
            flags, 0.0, None, p, p, lib.ym_draw_workspace_bytes(batch, max_det), None)
    return rc, lib.ym_last_error().decode()


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
def test_draw_detections_ragged_refuses_bad_tables(packed):
    frames = [(8, 8, 0), (5, 7, 256)]
    step = 256 // (8 if packed else 4)                               # elements per 256 bytes of a mask buffer
    good_blocks = [(8, 8, 0), (5, 7, 2 * step)]
    for bad_frames, text in (([(8, 8, 0), (5, 7, 100)], 'not a multiple of 256 bytes'), ([(8, 8, 0), (5, 7, 0)], 'overlap'),
                             ([(8, 8, 0), (0, 7, 256)], 'is 0 x 7'), ([(8, 8, 0), (5, 20000, 256)], 'out of range')):
        rc, err = _draw_ragged_rc(bad_frames, good_blocks, packed)
        assert rc == -1 and text in err, (bad_frames, rc, err)
    for bad_blocks, text in (([(8, 8, 0), (5, 8, 2 * step)], 'masks of 5 x 8 for a frame of 5 x 7'),       # sizes must equal the frames'
                             ([(8, 8, 0), (5, 7, 1)], 'not a multiple of 256 bytes'), ([(8, 8, 0), (5, 7, 0)], 'overlap'),
                             (None, 'mask block table')):
        rc, err = _draw_ragged_rc(frames, bad_blocks, packed)
        assert rc == -1 and text in err, (bad_blocks, rc, err)
    rc, err = _draw_ragged_rc([(4, 4, 256 * i) for i in range(33)], None, packed, flags=hip.DRAW_HIDE_MASK)
    assert rc == -1 and '1 .. 32 images per call' in err, (rc, err)


def _draw_uniform_rc(packed, batch, max_det, palette_n=100):
    lib = hip.lib()
    mem = torch.zeros(1 << 16, dtype=torch.uint8)
    p = ctypes.c_void_p(mem.data_ptr())
    fn = lib.ym_draw_detections_batch_packed if packed else lib.ym_draw_detections_batch
    rc = fn(p, p, p, p, p, p, batch, max_det, 4, 8, p, palette_n, 81, p, 80, p, 0, 0.0, None, p, None, p, 1 << 16, None)
    return rc, lib.ym_last_error().decode()


def test_uniform_draw_entries_take_33_frames_and_every_entry_names_itself():
    """The uniform entries share their launch path with the ragged ones but not their limit of 32 images: a batch of 33 gets past the
    batch check (here it is refused for a LATER argument, an empty palette), and each of the four entries reports under its own name."""
    rc, err = _draw_uniform_rc(False, 33, 1, palette_n=0)
    assert rc == -1 and err.startswith('ym_draw_detections_batch: num_classes=81 needs a palette'), (rc, err)
    rc, err = _draw_uniform_rc(False, 33, -1)
    assert rc == -1 and err.startswith('ym_draw_detections_batch: 1 <= B <= 65535 and 0 <= max_det'), (rc, err)
    rc, err = _draw_uniform_rc(True, 33, -1)
    assert rc == -1 and err.startswith('ym_draw_detections_batch_packed: 1 <= B <= 65535 and 0 <= max_det'), (rc, err)
    for packed, name in ((False, 'ym_draw_detections_ragged'), (True, 'ym_draw_detections_ragged_packed')):
        rc, err = _draw_ragged_rc([(8, 8, 0), (5, 7, 256)], None, packed, flags=hip.DRAW_HIDE_MASK, max_det=-1)
        assert rc == -1 and err.startswith(name + ': 1 <= B <= 32 and 0 <= max_det'), (rc, err)
        rc, err = _draw_ragged_rc([(4, 4, 256 * i) for i in range(33)], None, packed, flags=hip.DRAW_HIDE_MASK)
        assert rc == -1 and err.startswith(name + ': 1 .. 32 images per call'), (rc, err)
