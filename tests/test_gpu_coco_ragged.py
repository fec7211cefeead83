"""GPU parity of the ragged annotation rasteriser: `ym_ann_to_mask_ragged` behind `anns_to_masks_batch` / `COCO.annsToMasksBatch` /
`COCODetection.finish_batch`, bit-exact against the oracle's restatement of pycocotools (oracle/coco_ref.py) and against the
per-image entries, which are the one-image instances of the same kernel."""
import random
import types

import numpy as np
import pytest
import torch

from oracle import coco_ref as C
from oracle import rle_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 0xA5


def _oracle(segs, h, w):
    return np.stack([C.segm_to_mask(s, h, w) for s in segs]) if segs else np.zeros((0, h, w), np.uint8)


def _edge_cases(h, w):
    """The four of tests/test_gpu_coco.py: the whole image, a degenerate polygon, repeated / far-outside vertices, no polygon."""
    return [[[0, 0, 0, h, w, h, w, 0]], [[1.0, 1.0]], [[2, 1, 2, 1, 2.4, 3.3, w + 30, h + 20, w - 1, 0.2, w - 1, 0.2]], []]


def _rle(m, as_string):
    counts = R.rle_counts(m)
    return {'size': list(m.shape), 'counts': R.rle_to_string(counts) if as_string else counts}


def _small_batch():
    """[(segmentations, (h, w)) per image]: the smallest shapes at which each mechanism of the kernel can go wrong."""
    images = []
    for h, w in ((48, 64),             # H * W a multiple of 4: word stores
                 (37, 53),             # H * W odd: byte stores, and the blocks behind it start aligned all the same
                 (1, 9), (9, 1),
                 (33, 4)):             # a column crosses one 32-row word
        images.append((C.synth_polygons(h * 1000 + w, h, w, n=7) + _edge_cases(h, w), (h, w)))
    h, w = 64, 520                     # H a multiple of 32; W > 512: the column-parity carry crosses a 512-thread chunk
    images.append((C.synth_polygons(3, h, w, n=3) + [[[0, 0, 0, h, w, h, w, 0]], [[300.5, 3, 519.5, 3, 519.5, 60, 300.5, 60]]], (h, w)))
    images.append(([], (20, 30)))      # no annotation, in the middle
    h, w = 128, 96                     # run lengths only, as counts and as the compressed string
    rng = np.random.default_rng(2)
    dense = [(rng.random((h, w)) < p).astype(np.uint8) for p in (0.0, 0.02, 0.5, 1.0)]
    checker = ((np.arange(h)[:, None] // 2 + np.arange(w)[None, :]) % 2).astype(np.uint8)
    assert len(R.rle_counts(checker)) > 2048          # > 512 runs: the run scan crosses its chunks
    images.append(([_rle(m, s) for s in (False, True) for m in dense + [checker]], (h, w)))
    h, w = 61, 47                      # polygon lists and run lengths mixed
    polys = C.synth_polygons(9, h, w, n=3)
    dense = [(rng.random((h, w)) < p).astype(np.uint8) for p in (0.3, 0.6)]
    images.append(([polys[0], _rle(dense[0], False), polys[1], _rle(dense[1], True), [], polys[2]], (h, w)))
    return images


@pytest.fixture(scope='module')
def small():
    """The small batch through ONE `anns_to_masks_batch` call into a sentinel-filled allocation; the oracle's masks, computed once."""
    from yolact_minimal_amd.utils.coco import anns_to_masks_batch, pack_annotations
    images = _small_batch()
    segs, sizes = [s for s, _ in images], [hw for _, hw in images]
    layout = pack_annotations(segs, sizes)
    out = torch.full((layout.total_bytes + 300,), SENTINEL, dtype=torch.uint8, device=DEV)
    views = anns_to_masks_batch(segs, sizes, DEV, out=out)
    want = [_oracle(s, h, w) for s, (h, w) in images]
    return types.SimpleNamespace(segs=segs, sizes=sizes, layout=layout, out=out, views=views, want=want)


def test_small_shapes_match_the_oracle_bit_exact(small):
    assert len(small.views) == len(small.sizes) == 9 <= 32                 # one launch
    for b, (got, want, segs, (h, w)) in enumerate(zip(small.views, small.want, small.segs, small.sizes)):
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(segs), h, w) and got.is_contiguous(), b
        assert not segs or got.data_ptr() == small.out.data_ptr() + small.layout.block_offsets[b]      # (an empty view has no pointer)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'image {b} ({h} x {w})')


def test_small_shapes_equal_the_per_image_entries(small):
    from yolact_minimal_amd.utils.coco import anns_to_masks
    for b, (got, segs, (h, w)) in enumerate(zip(small.views, small.segs, small.sizes)):
        alone = anns_to_masks(segs, h, w, DEV)
        assert alone.shape == got.shape and torch.equal(got, alone), (b, h, w)


def test_bytes_between_the_blocks_are_untouched(small):
    host = small.out.cpu().numpy()
    inside = np.zeros(host.shape, bool)
    for o, segs, (h, w) in zip(small.layout.block_offsets, small.segs, small.sizes):
        assert o % 256 == 0
        inside[o:o + len(segs) * h * w] = True
    assert (~inside).sum() >= 300 and inside.sum() == sum(len(s) * h * w for s, (h, w) in zip(small.segs, small.sizes))
    assert (host[~inside] == SENTINEL).all()
    assert (host[inside] <= 1).all()                                           # ... and every byte of every block was written


def test_lds_and_workspace_images_share_one_launch():
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.utils.coco import anns_to_masks_batch
    sizes, counts = [(48, 64), (900, 1100), (240, 320)], [2, 3, 2]
    assert hip.lib().ym_ann_to_mask_workspace_bytes(1, 900, 1100) > 0 and hip.lib().ym_ann_to_mask_workspace_bytes(1, 240, 320) == 0
    segs = [C.synth_polygons(70 + b, h, w, n=n) for b, ((h, w), n) in enumerate(zip(sizes, counts))]
    got = anns_to_masks_batch(segs, sizes, DEV)
    for g, s, (h, w) in zip(got, segs, sizes):
        np.testing.assert_array_equal(g.cpu().numpy(), _oracle(s, h, w))


def test_thirty_three_images_take_two_launches():
    from yolact_minimal_amd.utils.coco import anns_to_masks_batch
    sizes = [((9, 1), (1, 9), (33, 4))[i % 3] for i in range(33)]
    segs = [[C.synth_polygons(500 + i, h, w, n=1)[0]] for i, (h, w) in enumerate(sizes)]
    got = anns_to_masks_batch(segs, sizes, DEV)
    assert len(got) == 33 and len({g.untyped_storage().data_ptr() for g in got}) == 1
    for i, (g, s, (h, w)) in enumerate(zip(got, segs, sizes)):
        assert tuple(g.shape) == (1, h, w)
        np.testing.assert_array_equal(g.cpu().numpy(), _oracle(s, h, w), err_msg=f'image {i}')


def test_a_batch_without_annotations_launches_nothing():
    from yolact_minimal_amd.utils.coco import anns_to_masks_batch
    got = anns_to_masks_batch([[], []], [(10, 12), (5, 7)], DEV)
    assert [tuple(g.shape) for g in got] == [(0, 10, 12), (0, 5, 7)] and all(g.dtype == torch.uint8 and g.is_cuda for g in got)
    assert anns_to_masks_batch([], [], DEV) == []
    with pytest.raises(ValueError):
        anns_to_masks_batch([[{'size': [11, 12], 'counts': [132]}]], [(10, 12)], DEV)


def _cfg(root, ann, img_size):
    from yolact_minimal_amd.config import COCO_LABEL_MAP
    return types.SimpleNamespace(train_imgs=root + '/imgs', val_imgs=root + '/imgs', train_ann=ann, val_ann=ann, img_size=img_size,
                                 continuous_id=COCO_LABEL_MAP, val_num=-1, image=root + '/imgs')


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('coco_ragged'))
    return root, C.write_synth_dataset(root, n_images=6, seed=4)


def test_anns_to_masks_batch_of_the_index_equals_the_per_image_call(dataset):
    from yolact_minimal_amd.utils import coco as K
    _, ann = dataset
    idx = K.COCO(ann, device=DEV)
    per_image = [idx.imgToAnns[i] for i in idx.imgToAnns]                       # polygons, the RLE crowd region, the tiny box
    assert len(per_image) == 6
    got = idx.annsToMasksBatch(per_image)
    for g, anns in zip(got, per_image):
        rec = idx.imgs[anns[0]['image_id']]
        assert torch.equal(g, idx.annsToMasks(anns))
        np.testing.assert_array_equal(g.cpu().numpy(), _oracle([a['segmentation'] for a in anns], rec['height'], rec['width']))


@pytest.mark.parametrize('reject', [None, 1], ids=['all_valid', 'one_without_a_valid_box'])
def test_finish_batch_rasterises_in_one_launch_and_equals_the_per_sample_path(dataset, monkeypatch, reject):
    from yolact_minimal_amd import hip
    from yolact_minimal_amd.utils import coco as K
    root, ann = dataset
    ds = K.COCODetection(_cfg(root, ann, 256), 'train', device=DEV)
    recs = [ds.read(i) for i in range(3)]
    if reject is not None:
        recs[reject] = dict(recs[reject], boxes=[], labels=[], anns=[])
    ds.rng = random.Random(11)
    wi, wt, wm = K.train_collate([ds.finish(r) for r in recs])

    lib, calls = hip.lib(), {}
    for name in ('ym_ann_to_mask_ragged', 'ym_poly_to_mask', 'ym_runs_to_mask'):
        def counted(*args, _fn=getattr(lib, name), _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*args)
        monkeypatch.setattr(lib, name, counted)
    ds.rng = random.Random(11)
    gi, gt, gm = ds.finish_batch(recs)
    assert calls == {'ym_ann_to_mask_ragged': 1}, calls

    assert torch.equal(gi, wi) and gi.dtype == wi.dtype and gi.device == wi.device and gi.is_contiguous()
    assert len(gt) == len(wt) == len(gm) == len(wm) == 3
    for a, b in zip(gt, wt):
        assert a.dtype == b.dtype == torch.float32 and a.device == b.device and a.is_contiguous() and torch.equal(a, b)
    for a, b in zip(gm, wm):
        assert a.dtype == b.dtype == torch.float32 and a.device == b.device and a.is_contiguous() and torch.equal(a, b)
