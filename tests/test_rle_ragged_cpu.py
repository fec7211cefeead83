"""The ragged RLE stage without a GPU: `ym_rle_encode_ragged_packed` is exported and bound, its record type is 40 bytes on both
sides, its workspace query is a host function of the sizes, every refusal happens on the host before any HIP call (a 4 KB host
buffer stands for every device pointer: a refused call never follows it), and `BatchMakeJson` assembles the files `MakeJson` writes
from record blocks."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import rle_ref
from yolact_minimal_amd import hip
from yolact_minimal_amd.utils.common_utils import BatchMakeJson, MakeJson

EINVAL, ENOSPC = -1, -2           # YM_EINVAL, YM_ENOSPC
NAME = 'rle_encode_ragged_packed:'
POINTERS = ('ids', 'scores', 'boxes', 'counts', 'det_bits', 'records', 'strings', 'header', 'ws')
DTYPE = np.dtype(hip.RLE_RECORD_DTYPE)


def _words(h, w):
    return h * ((w + 63) // 64)


def _layout(sizes, max_det):
    offsets, end = [], 0
    for h, w in sizes:
        offsets.append(end)
        end += max_det * _words(h, w)
    return offsets


def _call(sizes=((8, 70), (5, 3)), max_det=4, cap_runs=64, batch=None, det_off=None, null=(), table=True, live=True, short_ws=0,
          short_strings=0, misalign=False):
    lib = hip.lib()
    sizes = list(sizes)
    n = len(sizes)
    mem = torch.zeros(4096, dtype=torch.uint8)                      # a non-null pointer; a refused call never follows it
    p = ctypes.c_void_p(mem.data_ptr())
    det = hip.ragged_table(sizes, _layout(sizes, max_det) if det_off is None else det_off) if table else None
    b = n if batch is None else batch
    ws = lib.ym_rle_encode_ragged_workspace_bytes(det, b, max_det, cap_runs)
    a = {k: (None if k in null else p) for k in POINTERS}
    if misalign:
        a['det_bits'] = ctypes.c_void_p(mem.data_ptr() + 4)
    live_c = (ctypes.c_uint8 * max(n, 1))(*([1] * n)) if live else None
    worst = max(b, 0) * max(max_det, 0) * 4 * max(cap_runs, 0)
    rc = lib.ym_rle_encode_ragged_packed(a['ids'], a['scores'], a['boxes'], a['counts'], b, max_det, a['det_bits'], det, live_c, cap_runs,
                                         a['records'], a['strings'], worst - short_strings, a['header'], a['ws'],
                                         ws - short_ws if short_ws else max(ws, 1 << 20), None)
    return rc, lib.ym_last_error().decode(), ws


def test_the_symbols_are_exported_and_bound():
    lib = hip.lib()
    for name in ('ym_sizeof_rle_record', 'ym_rle_encode_ragged_workspace_bytes', 'ym_rle_encode_ragged_packed'):
        assert name in hip.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert lib.ym_sizeof_rle_record.restype is ctypes.c_size_t
    assert lib.ym_rle_encode_ragged_workspace_bytes.restype is ctypes.c_size_t
    assert lib.ym_rle_encode_ragged_packed.restype is ctypes.c_int


def test_the_record_is_40_bytes_on_both_sides():
    assert ctypes.sizeof(hip.RleRecord) == hip.lib().ym_sizeof_rle_record() == 40 == DTYPE.itemsize
    for name, _ in hip.RleRecord._fields_:                          # (the numpy view used for the D2H block has the same offsets)
        assert getattr(hip.RleRecord, name).offset == DTYPE.fields[name][1]


@pytest.mark.parametrize('sizes, max_det, cap_runs', [
    ([(8, 70), (5, 3)], 4, 64), ([(1, 1)], 1, 1), ([(480, 640)] * 32, 100, 4096), ([(65, 130), (1100, 1000), (7, 4096)], 5, 16384)])
def test_workspace_bytes_is_the_documented_formula(sizes, max_det, cap_runs):
    """include/yolact_hip.h: B * max_det * cap_runs * 4 bytes of positions + B * max_det slabs of 4 * cap_runs bytes."""
    det = hip.ragged_table(sizes, _layout(sizes, max_det))
    rows = len(sizes) * max_det
    assert hip.lib().ym_rle_encode_ragged_workspace_bytes(det, len(sizes), max_det, cap_runs) == rows * cap_runs * 4 + rows * 4 * cap_runs


REFUSED = [
    (dict(sizes=[(4, 4)] * 33), 'images per call'),                                                                     # B = 33
    (dict(batch=0), 'images per call'),
    (dict(max_det=0), 'max_det'),
    (dict(cap_runs=0), 'cap_runs'),
    (dict(sizes=[(8, 4097), (5, 3)]), 'need 0 < W <= 4096'),
    (dict(sizes=[(1 << 20, 2048), (5, 3)]), 'mask too large'),                                                          # h * w = 2^31
    (dict(sizes=[(0, 5), (5, 3)]), 'is 0 x 5'),
    (dict(det_off=[0, -1]), 'block offset'),
    (dict(det_off=[0, 4 * 8 * 2 - 1]), 'overlap'),                                                                      # one word short
    (dict(det_off=[0, 0]), 'overlap'),
    (dict(sizes=[(8, 8)] * 32, max_det=1024, cap_runs=16384), '< 2^31'),                                                 # rows * slab = 2^31
    (dict(table=False), 'null'),
]


@pytest.mark.parametrize('kw, text', REFUSED + [
    (dict(live=False), 'null pointer'),
    (dict(misalign=True), '8-byte aligned'),
] + [(dict(null=(k,)), 'null pointer') for k in POINTERS])
def test_refusals_happen_on_the_host_and_name_the_entry(kw, text):
    rc, msg, _ = _call(**kw)
    assert rc == EINVAL, msg
    assert msg.startswith(NAME) and text in msg, msg


@pytest.mark.parametrize('kw', [kw for kw, _ in REFUSED])
def test_workspace_bytes_is_zero_for_a_refused_table(kw):
    assert _call(**kw)[2] == 0


@pytest.mark.parametrize('kw, text', [(dict(short_ws=1), 'workspace'), (dict(short_strings=1), 'worst case')])
def test_short_buffers_are_enospc(kw, text):
    rc, msg, ws = _call(**kw)
    assert ws > 0 and rc == ENOSPC, msg
    assert msg.startswith(NAME) and text in msg, msg


# ---- BatchMakeJson from record blocks ------------------------------------------------------------------------------------------
LABELS = {k + 1: k + 1 for k in range(80)}


def _blocks(rng, sizes, max_det, counts, live):
    """Hand-made records of one request, the blob of their strings, and the same rows as (b, class, score, box, rle) for the
    per-record path.  Row 1 of image 0 has a zero-area box: no record."""
    rec = np.zeros((len(sizes), max_det), dtype=DTYPE)
    blob, rows = bytearray(), []
    for b, (h, w) in enumerate(sizes):
        for r in range(counts[b] if live[b] else 0):
            x1, y1 = int(rng.integers(0, w)), int(rng.integers(0, h))
            box = [x1, y1, x1 + int(rng.integers(1, 50)), y1 + int(rng.integers(1, 50))]
            if (b, r) == (0, 1):
                box[2] = box[0]
            if (box[3] - box[1]) * (box[2] - box[0]) <= 0:
                continue
            rle = rle_ref.encode(rng.random((h, w)) < 0.3)
            s = rle['counts'].encode('ascii')
            score = np.float32(rng.random())
            cls = int(rng.integers(0, 80))
            rec[b, r] = (cls, score, box, len(blob), len(s), 0, 1)
            blob += s
            rows.append((b, cls, score, np.asarray(box, dtype=np.int32), rle))
    return rec, bytes(blob), rows


def test_batch_make_json_from_blocks_equals_make_json_record_by_record(tmp_path):
    rng = np.random.default_rng(5)
    one, many = MakeJson(LABELS), BatchMakeJson(LABELS)
    extra = (7, 3, np.asarray([1, 2, 30, 41], dtype=np.int32), 0.625, rle_ref.encode(np.eye(6, 9) > 0))
    requests = [([(6, 70), (9, 5), (12, 12)], 4, [3, 4, 2], [True, True, False], [101, 102, None]),
                ([(5, 5)], 3, [0], [True], [103]),
                ([(20, 3), (3, 20)], 2, [2, 1], [True, True], [104, 105])]
    for k, (sizes, md, counts, live, image_ids) in enumerate(requests):
        rec, blob, rows = _blocks(rng, sizes, md, counts, live)
        many.add_records(rec, blob, image_ids, sizes)
        for b, cls, score, box, rle in rows:
            one.add_bbox(image_ids[b], cls, box, score)
            one.add_mask(image_ids[b], cls, rle, score)
        if k != 1:                                                  # records added one by one keep their place between the requests
            for mj in (one, many):
                mj.add_bbox(extra[0] + k, extra[1], extra[2], extra[3])
                mj.add_mask(extra[0] + k, extra[1], extra[4], extra[3])
    paths = {}
    for name, mj in (('one', one), ('many', many)):
        paths[name] = (tmp_path / f'{name}_bbox.json', tmp_path / f'{name}_mask.json')
        mj.dump(*map(str, paths[name]))
    for a, b in zip(paths['one'], paths['many']):
        assert a.read_bytes() == b.read_bytes()
    assert len(one.bbox_data) == len(many.bbox_data) > 8 and many.bbox_data[0]['image_id'] == 101


def test_add_batch_refuses_dense_masks_and_host_tensors():
    mj = BatchMakeJson(LABELS)
    with pytest.raises(RuntimeError, match='CUDA'):
        mj.add_batch(torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 4), torch.zeros(1, 4, 4, dtype=torch.int32),
                     torch.zeros(1, 4, 8, 8), torch.zeros(1, dtype=torch.int32), [1])
