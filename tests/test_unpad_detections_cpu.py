"""`unpad_detections` without a GPU: the padded rows of `after_nms_batch(sync=False)` and a host list of counts -> per-image 4-tuples,
for the three forms the padded masks take (one tensor, a list of per-image views, a `PackedMasks`), with and without `visual_thre`."""
import numpy as np
import pytest
import torch

from yolact_minimal_amd.utils.output_utils import PackedMasks, pack_reference, unpad_detections

MD, COUNTS, H, W = 4, [2, 0, 3], 6, 70
SIZES = [(6, 70), (3, 5), (9, 130)]
THRE = 0.5


def _padded():
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 80, (3, MD), generator=g)
    scores = torch.tensor([[0.9, 0.3, 0.8, 0.7],          # image 0: THRE removes row 1 (rows 2, 3 are past its count)
                           [0.9, 0.9, 0.9, 0.9],          # image 1: no detections, whatever its rows hold
                           [0.4, 0.2, 0.1, 0.9]])         # image 2: THRE removes all three rows (row 3 is past its count)
    box_px = torch.randint(0, 640, (3, MD, 4), generator=g).int()
    return ids, scores, box_px, g


def _masks(kind, g):
    """(the padded masks in the form `kind`, the same rows as plain tensors: what the expectations are sliced from)."""
    if kind == 'views':
        views = [(torch.rand(MD, h, w, generator=g) > 0.5).float() for h, w in SIZES]
        return views, views, views
    dense = (torch.rand(3, MD, H, W, generator=g) > 0.5).float()
    if kind == 'dense':
        return dense, dense, dense
    bits = torch.from_numpy(pack_reference(dense.numpy()))
    return PackedMasks._wrap(bits, H, W), bits, dense


@pytest.mark.parametrize('thre', [0.0, THRE])
@pytest.mark.parametrize('kind', ['dense', 'views', 'packed'])
def test_unpad_detections(kind, thre):
    ids, scores, box_px, g = _padded()
    masks, plain, dense = _masks(kind, g)
    out = unpad_detections(ids, scores, box_px, masks, COUNTS, thre)
    assert len(out) == 3 and all(isinstance(r, tuple) and len(r) == 4 for r in out)
    assert out[1] == (None, None, None, None)
    # image 0 keeps rows [0, 1], or row [0] under the threshold; image 2 keeps rows [0, 1, 2], or nothing
    rows0 = [0] if thre else [0, 1]
    want = {0: (ids[0, rows0], scores[0, rows0], box_px[0, rows0], plain[0][rows0])}
    if thre:
        assert out[2] == (None, None, None, None)
    else:
        want[2] = (ids[2, :3], scores[2, :3], box_px[2, :3], plain[2][:3])
    for b, w in want.items():
        got = out[b]
        assert isinstance(got[3], PackedMasks) == (kind == 'packed')
        if kind == 'packed':
            assert (got[3].height, got[3].width) == (H, W) and got[3].shape == (len(w[0]), H, W)
            np.testing.assert_array_equal(got[3].numpy(), dense[b][:len(w[0])].numpy())      # (kept rows are leading rows here)
        for x, y in zip(got[:3] + (got[3].bits if kind == 'packed' else got[3],), w):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
