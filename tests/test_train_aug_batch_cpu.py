"""Batched train_aug without a GPU: the `ym_aug_item` mirror, the host-side refusals of `ym_train_aug_image_batch` /
`ym_train_aug_masks_batch` (refused before any launch, so no device is needed), the host half `sample_train_aug_batch` (draw order,
the `train_collate` batch composition) and the Python / loader refusals, which come before the native library is touched."""
import ctypes
import random
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from yolact_minimal_amd import hip
from yolact_minimal_amd.utils import augmentations as A
from yolact_minimal_amd.utils.synthetic import synth_sample

SIZES = [(96, 128), (120, 110), (104, 104), (128, 96), (100, 100), (37, 53)]
N = [2, 4, 1, 3, 1, 2]
TRAIN_SIZE = 288


def batch_samples(count=18):
    return [synth_sample(i, *SIZES[i % 6], N[i % 6]) for i in range(count)]


def sliver_sample():
    """A sample every draw rejects: one box 4 px wide and 0.001 px high never reaches an area of 20 px^2 at 288."""
    img, masks, _, _ = synth_sample(4, 100, 100, 1)
    return img, masks, np.array([[10.0, 10.0, 14.0, 10.001]]), np.array([3])


def test_aug_item_mirror_has_the_c_size():
    assert ctypes.sizeof(hip.AugItemC) == hip.lib().ym_sizeof_aug_item()
    assert hip.AugItemC.plan.offset == 0 and ctypes.sizeof(hip.AugPlanC) == 27 * 4 and hip.AUG_MAX_SAMPLES == hip.RAGGED_MAX_IMAGES == 32


def test_the_new_entries_are_declared_and_bound():
    for name in ('ym_sizeof_aug_item', 'ym_train_aug_image_batch', 'ym_train_aug_masks_batch'):
        assert name in hip.ABI_SYMBOLS
    for name in ('ym_train_aug_image_batch', 'ym_train_aug_masks_batch'):
        assert getattr(hip.lib(), name).argtypes is not None


# ---- the C entries' refusals ----------------------------------------------------------------------------------------------------
_MEM = torch.zeros(4096, dtype=torch.uint8)                         # a non-null pointer; a refused call never follows it
_P = _MEM.data_ptr()


def _good_items(ks=(2, 0, 3), size=64):
    """Valid items of 32 x 40 samples (full-image crop, padded to 40, resized to `size`), 4 masks each, k surviving."""
    items = (hip.AugItemC * len(ks))()
    row = 0
    for it, k in zip(items, ks):
        p = it.plan
        p.H, p.W, p.cx, p.cy, p.cw, p.ch, p.q, p.px, p.py, p.r, p.S = 32, 40, 0, 0, 40, 32, 40, 0, 4, size, size
        p.saturation, p.contrast = 1.0, 1.0
        for c in range(3):
            p.mean[c], p.std[c] = 100.0, 50.0
        it.n_masks, it.img, it.masks, it.k, it.row0 = 4, _P, _P, k, row
        row += k
    return items, row


def _image_rc(items, batch=None, size=64, out=_P, null_table=False):
    lib = hip.lib()
    rc = lib.ym_train_aug_image_batch(None if null_table else items, len(items) if batch is None else batch, size, 1,
                                      ctypes.c_void_p(out), None)
    return rc, lib.ym_last_error().decode()


def _masks_rc(items, total, batch=None, size=64, keep=_P, out=_P, null_table=False):
    lib = hip.lib()
    rc = lib.ym_train_aug_masks_batch(None if null_table else items, len(items) if batch is None else batch, size, 1,
                                      ctypes.c_void_p(keep), total, ctypes.c_void_p(out), None)
    return rc, lib.ym_last_error().decode()


def _edit(fn, ks=(2, 0, 3)):
    items, total = _good_items(ks)
    fn(items)
    return items, total


@pytest.mark.parametrize('entry', ['image', 'masks'])
def test_both_entries_refuse_bad_tables_and_plans(entry):
    name = f'train_aug_{entry}_batch'

    def rc(items, total, **kw):
        return _image_rc(items, **kw) if entry == 'image' else _masks_rc(items, total, **kw)

    items, total = _good_items()
    for batch in (0, -1, 33):
        got, err = rc(items, total, batch=batch)
        assert got == -1 and err.startswith(name) and '1 .. 32 samples per call' in err, (batch, got, err)
    got, err = rc(items, total, null_table=True)
    assert got == -1 and err.startswith(name) and 'null item table' in err, (got, err)
    got, err = rc(items, total, size=65)
    assert got == -1 and err.startswith(name) and 'sample 0: plan.S = 64' in err, (got, err)
    got, err = rc(*_edit(lambda t: setattr(t[2].plan, 'S', 96)))
    assert got == -1 and 'sample 2: plan.S = 96' in err, (got, err)
    for change, text in ((lambda t: setattr(t[1].plan, 'cw', 41), 'sample 1: train_aug: crop outside the image'),
                         (lambda t: setattr(t[2].plan, 'py', 9), 'sample 2: train_aug: pad-to-square inconsistent'),
                         (lambda t: setattr(t[0].plan, 'final_mode', 3), 'sample 0: train_aug: bad sizes'),
                         (lambda t: setattr(t[1].plan, 'r', 32), 'sample 1: train_aug: final_mode 0 needs r == S')):
        got, err = rc(*_edit(change))
        assert got == -1 and err.startswith(name) and text in err, (got, err)


def test_image_entry_refuses_null_pointers():
    items, _ = _good_items()
    rc, err = _image_rc(items, out=None)
    assert rc == -1 and 'train_aug_image_batch: null output pointer' in err, (rc, err)
    rc, err = _image_rc(_edit(lambda t: setattr(t[1], 'img', None))[0])
    assert rc == -1 and 'train_aug_image_batch: sample 1: null image pointer' in err, (rc, err)


def test_masks_entry_refuses_inconsistent_rows():
    for change, text in ((lambda t: setattr(t[0], 'k', -1), 'sample 0: k = -1 < 0'),
                         (lambda t: setattr(t[2], 'masks', None), 'sample 2: k = 3 with a null masks pointer'),
                         (lambda t: setattr(t[0], 'n_masks', 0), 'sample 0: k = 2 with n_masks <= 0'),
                         (lambda t: setattr(t[1], 'row0', 0), 'sample 1: row0 = 0, the earlier samples hold 2 rows'),
                         (lambda t: setattr(t[2], 'row0', 3), 'sample 2: row0 = 3, the earlier samples hold 2 rows'),
                         (lambda t: setattr(t[0], 'row0', 1), 'sample 0: row0 = 1, the earlier samples hold 0 rows')):
        rc, err = _masks_rc(*_edit(change))
        assert rc == -1 and err.startswith('train_aug_masks_batch') and text in err, (rc, err)
    items, total = _good_items()
    for wrong in (total - 1, total + 1, 0):
        rc, err = _masks_rc(items, wrong)
        assert rc == -1 and f'the samples hold 5 rows, total_k = {wrong}' in err, (rc, err)
    for kw in ({'keep': None}, {'out': None}):
        rc, err = _masks_rc(items, total, **kw)
        assert rc == -1 and 'total_k = 5 with a null keep or output pointer' in err, (rc, err)


def test_masks_entry_with_no_rows_is_a_no_op():
    items, total = _good_items(ks=(0, 0))
    for it in items:
        it.masks, it.n_masks = None, 0                               # masks may be null when k == 0
    assert total == 0 and _masks_rc(items, 0, keep=None, out=None)[0] == 0


# ---- the host half --------------------------------------------------------------------------------------------------------------
_FIELDS = ('brightness', 'contrast', 'saturation', 'hue', 'mirror', 'crop', 'square', 'pad', 'resize', 'final_pad', 'final_crop', 'size')


def _same_plan(a, b):
    assert all(getattr(a, f) == getattr(b, f) for f in _FIELDS), [(f, getattr(a, f), getattr(b, f)) for f in _FIELDS]
    np.testing.assert_array_equal(a.boxes, b.boxes)
    np.testing.assert_array_equal(a.labels, b.labels)
    np.testing.assert_array_equal(a.keep, b.keep)


def test_sample_train_aug_batch_draws_what_sequential_calls_draw():
    samples = batch_samples()
    plans, order = A.sample_train_aug_batch([s[0].shape[:2] for s in samples], [s[2] for s in samples], [s[3] for s in samples],
                                            TRAIN_SIZE, random.Random(2))
    rng = random.Random(2)
    want = [A.sample_train_aug(s[0].shape[0], s[0].shape[1], s[2], s[3], TRAIN_SIZE, rng) for s in samples]
    assert len(plans) == 18 and order == list(range(18))
    for a, b in zip(plans, want):
        _same_plan(a, b)
    # what this set covers (the GPU test leans on it): every final mode, both mirror values, the square-crop branch, no rejection
    assert all(p is not None for p in plans)
    modes = {0 if p.resize == TRAIN_SIZE else (1 if p.resize < TRAIN_SIZE else 2) for p in plans}
    assert modes == {0, 1, 2}
    assert {(p.final_pad is not None, p.final_crop is not None) for p in plans} == {(False, False), (True, False), (False, True)}
    assert {p.mirror for p in plans} == {False, True}
    assert sum(p.crop[2] == p.crop[3] for p in plans) == 5
    assert sum(len(p.keep) for p in plans) == 28


def test_the_sliver_sample_is_always_rejected():
    _, _, boxes, labels = sliver_sample()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for seed in range(300):
            assert A.sample_train_aug(100, 100, boxes, labels, TRAIN_SIZE, random.Random(seed)) is None


def test_order_follows_the_train_collate_rule():
    good, bad = batch_samples(3), sliver_sample()

    def run(samples, seed=7):
        return A.sample_train_aug_batch([s[0].shape[:2] for s in samples], [s[2] for s in samples], [s[3] for s in samples],
                                        TRAIN_SIZE, random.Random(seed))

    plans, order = run([good[0], bad, good[2], bad])
    assert [p is None for p in plans] == [False, True, False, True] and order == [0, 2, 0, 2]
    plans, order = run([bad, good[1], bad])
    assert [p is None for p in plans] == [True, False, True] and order == [1, 1, 1]       # valid_batch grows while it is read
    with pytest.raises(RuntimeError, match='none of the 2 samples'):
        run([bad, bad])
    # the rule is train_collate's own: the same composition from the same list of (rejected / valid) samples
    from yolact_minimal_amd.utils.coco import train_collate
    plans, order = run([bad, good[0], good[1], bad, bad])
    fake = [(None, None, None) if p is None else (torch.full((1,), float(b)), np.zeros((1, 5)), torch.zeros(1)) for b, p in enumerate(plans)]
    assert train_collate(fake)[0][:, 0].tolist() == [float(b) for b in order] == [1.0, 2.0, 1.0, 2.0, 1.0]


def test_a_sample_without_boxes_consumes_no_draw():
    samples = batch_samples(3)
    sizes, labels = [s[0].shape[:2] for s in samples], [s[3] for s in samples]
    rng = random.Random(5)
    plans, order = A.sample_train_aug_batch(sizes, [samples[0][2], None, samples[2][2]], [labels[0], None, labels[2]], TRAIN_SIZE, rng)
    after = rng.random()
    ref = random.Random(5)
    want = [A.sample_train_aug(*sizes[b], samples[b][2], labels[b], TRAIN_SIZE, ref) for b in (0, 2)]
    assert plans[1] is None and order == [0, 2, 0] and after == ref.random()
    _same_plan(plans[0], want[0])
    _same_plan(plans[2], want[1])


# ---- Python refusals: before the native library is touched ------------------------------------------------------------------------
def _no_library(monkeypatch):
    def boom():
        raise AssertionError('the native library was touched')
    monkeypatch.setattr(hip, 'lib', boom)


def test_python_entries_refuse_bad_arguments(monkeypatch):
    _no_library(monkeypatch)
    img, masks, boxes, labels = synth_sample(0, 32, 40, 2)
    plan = A.sample_train_aug(32, 40, boxes, labels, TRAIN_SIZE, random.Random(0))
    assert plan is not None
    ti, tm = torch.from_numpy(img), torch.from_numpy(masks)
    for imgs, ms, plans in (([ti], [tm], [plan]),                                        # CPU tensors
                            ([ti] * 33, [tm] * 33, [plan] * 33),                           # more than 32 samples
                            ([], [], []),                                                  # none
                            ([ti, ti], [tm], [plan, plan]),                                # list lengths
                            ([ti, ti], [tm, tm], [plan]),
                            ([ti, ti.float()], [tm, tm], [plan, plan]),                    # mixed image dtypes
                            ([ti, ti], [tm, tm.float()], [plan, plan]),                    # mixed mask dtypes
                            ([ti], [tm], [None]),                                          # a rejected sample left in
                            (ti, [tm], [plan])):                                           # not a list
        with pytest.raises(RuntimeError):
            A.apply_train_aug_batch(imgs, ms, plans)
    from yolact_minimal_amd.utils.frames import FrameBatch, frame_layout
    host = FrameBatch(torch.zeros(frame_layout([(32, 40)])[1], dtype=torch.uint8), [(32, 40)])
    with pytest.raises(RuntimeError, match='there is no CPU path'):
        A.apply_train_aug_batch(host, [tm], [plan])
    rng = random.Random(3)
    state = rng.getstate()
    for imgs, ms, bx, lb in (([ti], [tm], [boxes], [labels]),                            # CPU tensors
                             ([ti] * 33, [tm] * 33, [boxes] * 33, [labels] * 33),
                             ([ti, ti], [tm, tm], [boxes], [labels, labels]),
                             ([ti, ti.float()], [tm, tm], [boxes] * 2, [labels] * 2),
                             ([ti, ti], [tm, tm.float()], [boxes] * 2, [labels] * 2)):
        with pytest.raises(RuntimeError):
            A.train_aug_batch(imgs, ms, bx, lb, TRAIN_SIZE, rng)
    assert rng.getstate() == state, 'a refused call draws nothing'


def test_batched_loader_refuses_at_construction(monkeypatch):
    _no_library(monkeypatch)
    from yolact_minimal_amd.utils.coco import BatchLoader, COCODetection, train_collate, val_collate
    train, val = SimpleNamespace(mode='train'), SimpleNamespace(mode='val')
    with pytest.raises(RuntimeError, match="mode 'train'"):
        BatchLoader(val, 2, train_collate, batched=True)
    with pytest.raises(RuntimeError, match='train_collate'):
        BatchLoader(train, 2, val_collate, batched=True)
    with pytest.raises(RuntimeError, match='train_collate'):
        BatchLoader(train, 2, lambda b: b, batched=True)
    with pytest.raises(RuntimeError, match='1 .. 32 samples per batch, got 33'):
        BatchLoader(train, 33, train_collate, batched=True)
    assert BatchLoader(train, 32, train_collate, batched=True).batched and not BatchLoader(val, 64, val_collate).batched
    ds = COCODetection.__new__(COCODetection)
    ds.mode = 'val'
    with pytest.raises(RuntimeError, match="mode 'train' only"):
        ds.finish_batch([])
