"""Batched train_aug on the device: `train_aug_batch` / `apply_train_aug_batch` (one launch pair per 16 samples) against the
per-sample path bit for bit -- the single entries are the one-item instances of the same kernels -- and against the oracle's
restatement of the reference chain; rejection and repetition, `out=`, a non-identity `keep`, and the batched loader."""
import random
import types

import numpy as np
import pytest
import torch

from oracle import augment_ref as R
from oracle import coco_ref as C
from tests.test_train_aug_batch_cpu import TRAIN_SIZE, batch_samples, sliver_sample
from yolact_minimal_amd.utils import augmentations as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(arr, dtype):
    return torch.from_numpy(arr).to(DEV).to(dtype)


@pytest.fixture(scope='module')
def samples():
    return batch_samples()


@pytest.fixture(scope='module')
def plans(samples):
    rng = random.Random(2)
    return [A.sample_train_aug(s[0].shape[0], s[0].shape[1], s[2], s[3], TRAIN_SIZE, rng) for s in samples]


@pytest.fixture(scope='module', params=[torch.uint8, torch.float32], ids=['u8', 'f32'])
def batch(request, samples):
    """The 18-sample batch (two launches per entry) through `train_aug_batch`, once per dtype."""
    dt = request.param
    imgs, masks = [_dev(s[0], dt) for s in samples], [_dev(s[1], dt) for s in samples]
    got = A.train_aug_batch(imgs, masks, [s[2] for s in samples], [s[3] for s in samples], TRAIN_SIZE, random.Random(2))
    return dt, imgs, masks, got


def test_batch_equals_the_per_sample_path_bit_for_bit(batch, samples, plans):
    dt, imgs, masks, (images, mlist, boxes, labels) = batch
    assert tuple(images.shape) == (18, 3, TRAIN_SIZE, TRAIN_SIZE) and images.dtype == torch.float32 and images.is_contiguous()
    assert len(mlist) == len(boxes) == len(labels) == 18
    rng = random.Random(2)
    square = 0
    for b, s in enumerate(samples):
        img, m, bx, lb = A.train_aug(imgs[b], masks[b], s[2], s[3], TRAIN_SIZE, rng)
        assert img is not None
        assert torch.equal(images[b], img), f'image {b}'
        assert mlist[b].shape == m.shape and torch.equal(mlist[b], m), f'masks {b}'
        np.testing.assert_array_equal(boxes[b], bx)
        np.testing.assert_array_equal(labels[b], lb)
        square += plans[b].crop[2] == plans[b].crop[3]
    assert square == 5 and {p.mirror for p in plans} == {False, True}
    assert {(p.final_pad is not None, p.final_crop is not None) for p in plans} == {(False, False), (True, False), (False, True)}
    # the masks are views into ONE [K, S, S] allocation of exactly K rows
    total = sum(m.shape[0] for m in mlist)
    assert total == 28
    base = mlist[0].untyped_storage()
    assert base.nbytes() == total * TRAIN_SIZE * TRAIN_SIZE * 4
    assert all(m.untyped_storage().data_ptr() == base.data_ptr() and m.is_contiguous() for m in mlist)
    assert [m.storage_offset() for m in mlist] == list(np.cumsum([0] + [m.shape[0] for m in mlist[:-1]]) * TRAIN_SIZE * TRAIN_SIZE)


def test_batch_matches_the_reference_chain(batch, samples, plans):
    dt, _, _, (images, mlist, _, _) = batch
    got_img = images.cpu().numpy()
    seen_square = 0
    for b, (s, plan) in enumerate(zip(samples, plans)):
        want_img, _ = R.apply_plan(s[0], s[1], plan)
        np.testing.assert_allclose(got_img[b], want_img, rtol=0, atol=2e-3)
        want_masks = R.apply_plan(s[0], s[1].astype(np.uint8 if dt == torch.uint8 else np.float32), plan)[1]
        got = mlist[b].cpu().numpy()
        assert got.shape == want_masks.shape
        if dt == torch.uint8 and plan.crop[2] == plan.crop[3]:
            assert np.array_equal(got, want_masks) and set(np.unique(got)) <= {0.0, 1.0}, f'masks {b}'
            seen_square += 1
        else:
            np.testing.assert_allclose(got, want_masks, rtol=0, atol=1e-5)
    assert seen_square == (5 if dt == torch.uint8 else 0)


def test_rejected_samples_are_replaced_like_train_collate():
    from yolact_minimal_amd.utils.coco import train_collate
    good, bad = batch_samples(3), sliver_sample()
    four = [good[0], bad, good[2], bad]
    imgs, masks = [_dev(s[0], torch.uint8) for s in four], [_dev(s[1], torch.uint8) for s in four]
    images, mlist, boxes, labels = A.train_aug_batch(imgs, masks, [s[2] for s in four], [s[3] for s in four], TRAIN_SIZE, random.Random(9))
    rng = random.Random(9)
    single = []
    for b, s in enumerate(four):
        img, m, bx, lb = A.train_aug(imgs[b], masks[b], s[2], s[3], TRAIN_SIZE, rng)
        single.append((None, None, None) if img is None else (img, np.hstack((bx, np.expand_dims(lb, axis=1))), m))
    assert [s[0] is None for s in single] == [False, True, False, True]
    want_imgs, want_targets, want_masks = train_collate(single)
    assert torch.equal(images, want_imgs)
    for b in range(4):
        assert torch.equal(mlist[b], want_masks[b])
        got_t = torch.as_tensor(np.hstack((boxes[b], np.expand_dims(labels[b], axis=1))), dtype=torch.float32)
        assert torch.equal(got_t, want_targets[b].cpu())
    assert torch.equal(images[0], images[2]) and torch.equal(images[1], images[3]) and not torch.equal(images[0], images[1])


def test_out_rows_past_the_batch_are_untouched_and_keep_selects_the_source_mask():
    """`out=` with two spare rows that keep their canary; a plan that keeps instance 2 of 4 reads THAT mask (`keep` is no identity),
    next to samples whose keep starts at 0, in a FrameBatch (one allocation) as well as in a list."""
    from yolact_minimal_amd.utils.frames import FrameBatch
    samples = batch_samples(4)                                      # sample 1 has four instances
    rng = random.Random(2)
    plans = [A.sample_train_aug(s[0].shape[0], s[0].shape[1], s[2], s[3], TRAIN_SIZE, rng) for s in samples]
    assert all(p is not None for p in plans) and len(plans[1].keep) >= 1
    plans[1].keep = np.array([2])                                   # one instance out of four, not the first
    masks = [_dev(s[1], torch.float32) for s in samples]
    planes = np.ones_like(samples[1][1], dtype=np.float32) * np.array([1, 2, 3, 4], np.float32).reshape(4, 1, 1)
    masks[1] = _dev(planes, torch.float32)                          # every instance a plane of its own value
    frames = FrameBatch.from_numpy([s[0] for s in samples], DEV)
    out = torch.full((6, 3, TRAIN_SIZE, TRAIN_SIZE), -77.0, device=DEV)
    images, mlist = A.apply_train_aug_batch(frames, masks, plans, out=out)
    assert images.data_ptr() == out.data_ptr() and tuple(images.shape) == (4, 3, TRAIN_SIZE, TRAIN_SIZE)
    assert bool((out[4:] == -77.0).all()), 'rows past the batch were written'
    assert mlist[0].untyped_storage().nbytes() == sum(len(p.keep) for p in plans) * TRAIN_SIZE * TRAIN_SIZE * 4
    for b, s in enumerate(samples):
        img, m = A.apply_train_aug(frames.frames[b], masks[b], plans[b])
        assert torch.equal(images[b], img) and torch.equal(mlist[b], m), b
    assert tuple(mlist[1].shape) == (1, TRAIN_SIZE, TRAIN_SIZE)
    want = R.apply_plan(samples[1][0], planes, plans[1])[1]
    np.testing.assert_allclose(mlist[1].cpu().numpy(), want, rtol=0, atol=3e-5)          # (1e-5 of the single path x the value 3)
    assert float(mlist[1].max()) > 2.5 and float(mlist[1].max()) <= 3.0 + 3e-5, 'instance 2 carries the value 3'
    # a list of lone tensors gives the same rows as the FrameBatch views
    images2, mlist2 = A.apply_train_aug_batch([_dev(s[0], torch.uint8) for s in samples], masks, plans)
    assert torch.equal(images2, images) and all(torch.equal(a, b) for a, b in zip(mlist2, mlist))
    for bad in (torch.empty(3, 3, TRAIN_SIZE, TRAIN_SIZE, device=DEV), torch.empty(6, 3, TRAIN_SIZE, TRAIN_SIZE),
                torch.empty(6, 3, TRAIN_SIZE, TRAIN_SIZE, device=DEV, dtype=torch.float64),
                torch.empty(6, 3, TRAIN_SIZE, TRAIN_SIZE + 1, device=DEV)[..., :TRAIN_SIZE]):
        with pytest.raises(RuntimeError):
            A.apply_train_aug_batch(frames, masks, plans, out=bad)
    plans[1].keep = np.array([4])
    with pytest.raises(RuntimeError, match='sample 1: keep index outside its 4 masks'):
        A.apply_train_aug_batch(frames, masks, plans)


def test_batched_loader_yields_the_per_sample_loaders_batches(tmp_path):
    from yolact_minimal_amd.config import COCO_LABEL_MAP
    from yolact_minimal_amd.utils import coco as K
    root = str(tmp_path)
    ann = C.write_synth_dataset(root, n_images=6, seed=4)
    cfg = types.SimpleNamespace(train_imgs=root + '/imgs', val_imgs=root + '/imgs', train_ann=ann, val_ann=ann, img_size=256,
                                continuous_id=COCO_LABEL_MAP, val_num=-1, image=root + '/imgs')

    def run(batched):
        ds = K.COCODetection(cfg, 'train', device=DEV, rng=random.Random(11))
        return list(K.BatchLoader(ds, 3, K.train_collate, shuffle=True, seed=1, batched=batched))

    got, want = run(True), run(False)
    assert len(got) == len(want) == 2
    for (gi, gt, gm), (wi, wt, wm) in zip(got, want):
        assert torch.equal(gi, wi) and gi.dtype == wi.dtype and gi.device == wi.device and gi.is_contiguous()
        assert len(gt) == len(wt) == len(gm) == len(wm) == 3
        for a, b in zip(gt, wt):
            assert a.dtype == b.dtype == torch.float32 and a.device == b.device and a.is_contiguous() and torch.equal(a, b)
        for a, b in zip(gm, wm):
            assert a.dtype == b.dtype == torch.float32 and a.device == b.device and a.is_contiguous() and torch.equal(a, b)
