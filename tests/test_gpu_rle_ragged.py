"""GPU: `ym_rle_encode_ragged_packed` and `BatchMakeJson.add_batch` against the CPU restatement of maskApi.c (`oracle.rle_ref`) and
against the per-image path (`rle_encode` -> `MakeJson.add_bbox` / `add_mask` under eval.py:65's filter): edge sizes, overflow and
what it leaves untouched, rows that are no records, long runs, batch sizes, the mask input forms, two streams, and a mixed-size
`RequestPipeline` end to end."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from oracle import rle_ref
from oracle import yolact_ref as R
from yolact_minimal_amd import hip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPE = np.dtype(hip.RLE_RECORD_DTYPE)
LABELS = {k + 1: k + 1 for k in range(80)}
GUARD = 256
EDGE_SIZES = [(1, 1), (1, 65), (63, 64), (64, 63), (65, 130), (129, 1), (7, 200), (480, 640)]
EDGE_COUNTS = [0, 2, 5, 3, 5, 1, 4, 3]                      # every count from 0 to 5 (1 x 1 is encoded in test_thirty_two_images)
KINDS = ('zero', 'one', 'random', 'checker', 'blob')
# Row r of image b is KINDS[(r + shift_b) % 5].  The pixel-level random and checkerboard rows of 480 x 640 have about 153 600 and
# 307 200 runs, more than the largest cap_runs used here, so that image starts at the blob and they lie past its count of 3.  The
# shifts put the busy rows (random, checkerboard, blob) below the counts of the other images: at cap_runs = 64 most records overflow.
EDGE_SHIFT = [0, 3, 0, 2, 0, 3, 2, 4]


def _mask(kind, h, w, rng):
    yy, xx = np.mgrid[:h, :w]
    if kind == 'zero':
        return np.zeros((h, w), dtype=bool)
    if kind == 'one':
        return np.ones((h, w), dtype=bool)
    if kind == 'random':
        return rng.random((h, w)) < 0.5
    if kind == 'checker':
        return (yy + xx) % 2 == 1
    return ((yy - h / 2) / max(h / 3, 1)) ** 2 + ((xx - w / 2) / max(w / 4, 1)) ** 2 <= 1.0        # a blob around the centre


class _Request:
    """Hand-made `after_nms_batch(..., sync=False, packed=True)` rows: numpy masks [max_det, h, w] per image and their device form."""

    def __init__(self, sizes, masks, counts, boxes=None, garbage=None):
        from yolact_minimal_amd.utils.output_utils import ragged_layout
        from yolact_minimal_amd.utils.packed_masks import PackedMasks, pack_reference
        self.sizes, self.masks_np, self.count_list = list(sizes), masks, list(counts)
        b_, md = len(sizes), masks[0].shape[0]
        self.batch, self.max_det = b_, md
        self.offsets, total = ragged_layout(sizes, md, True)
        flat = np.zeros(total, dtype=np.int64)
        for b, (h, w) in enumerate(sizes):
            words = pack_reference(masks[b]).reshape(md, -1)
            if garbage is not None:                                 # rows nobody may read: random words, pad bits included
                for r in range(md):
                    if r >= counts[b] or b in garbage[1]:
                        words[r] = garbage[0].integers(-2 ** 63, 2 ** 63 - 1, size=words.shape[1], dtype=np.int64)
            flat[self.offsets[b]:self.offsets[b] + words.size] = words.reshape(-1)
        self.flat = torch.from_numpy(flat).to(DEV)
        self.views = [PackedMasks(self.flat[o:o + md * h * ((w + 63) // 64)].view(md, h, (w + 63) // 64), h, w)
                      for o, (h, w) in zip(self.offsets, sizes)]
        g = np.arange(b_ * md).reshape(b_, md)
        self.ids_np = (g * 7) % 80
        self.scores_np = (1.0 - g / (b_ * md + 1)).astype(np.float32)
        if boxes is None:
            boxes = np.asarray([[[r, b, r + w, b + h] for r in range(md)] for b, (h, w) in enumerate(sizes)], dtype=np.int32)
        self.boxes_np = np.asarray(boxes, dtype=np.int32)
        self.ids = torch.from_numpy(self.ids_np).to(DEV)
        self.scores = torch.from_numpy(self.scores_np).to(DEV)
        self.boxes = torch.from_numpy(self.boxes_np).to(DEV)
        self.counts = torch.tensor(self.count_list, dtype=torch.int32, device=DEV)

    def args(self):
        return self.ids, self.scores, self.boxes, self.views, self.counts

    def is_record(self, b, r, live=None):
        x1, y1, x2, y2 = (int(v) for v in self.boxes_np[b, r])
        return (live is None or bool(live[b])) and r < self.count_list[b] and (y2 - y1) * (x2 - x1) > 0

    @functools.lru_cache(maxsize=None)
    def oracle(self, b, r):
        return rle_ref.encode(self.masks_np[b][r])['counts'], len(rle_ref.rle_counts_fast(self.masks_np[b][r]))


@functools.lru_cache(maxsize=None)
def _edge_request(garbage=False, dead=()):
    rng = np.random.default_rng(1)
    masks = [np.stack([_mask(KINDS[(r + s) % 5], h, w, rng) for r in range(5)]) for (h, w), s in zip(EDGE_SIZES, EDGE_SHIFT)]
    return _Request(EDGE_SIZES, masks, EDGE_COUNTS, garbage=(np.random.default_rng(9), set(dead)) if garbage else None)


def _encode(req, cap_runs, live=None):
    """The C entry on canary-filled buffers -> (header, records [B, max_det], strings with GUARD bytes on either side, workspace with
    GUARD bytes behind it)."""
    lib = hip.lib()
    b_, md = req.batch, req.max_det
    rows = b_ * md
    table = hip.ragged_table(req.sizes, req.offsets)
    nws = lib.ym_rle_encode_ragged_workspace_bytes(table, b_, md, cap_runs)
    assert nws == rows * cap_runs * 8
    ws = torch.full((nws + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    nstr = rows * 4 * cap_runs
    sbuf = torch.full((nstr + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    out = torch.full((16 + rows * 40,), 0xEE, dtype=torch.uint8, device=DEV)
    live_c = (ctypes.c_uint8 * b_)(*([1] * b_ if live is None else [int(v) for v in live]))
    hip.check(lib.ym_rle_encode_ragged_packed(
        hip.ptr(req.ids, torch.int64), hip.ptr(req.scores), hip.ptr(req.boxes, torch.int32), hip.ptr(req.counts, torch.int32), b_, md,
        hip.ptr(req.flat, torch.int64), table, live_c, cap_runs, ctypes.c_void_p(out.data_ptr() + 16),
        ctypes.c_void_p(sbuf.data_ptr() + GUARD), nstr, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nws,
        hip.stream_ptr()), 'ym_rle_encode_ragged_packed')
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    return host[:16].view('<i4').copy(), host[16:].view(DTYPE).reshape(b_, md).copy(), sbuf.cpu().numpy(), ws.cpu().numpy()


def _check_against_oracle(req, cap_runs, header, rec, sbuf, ws, live=None):
    """Every row's state, fields and string; the tiling of [0, header[0]); and that nothing else was written: the bytes around and
    behind the strings, the tail of every slab and of every position row, the bytes behind the workspace."""
    rows = req.batch * req.max_det
    strings = sbuf[GUARD:-GUARD]
    pos = ws[:rows * cap_runs * 4].view('<u4').reshape(rows, cap_runs)
    slabs = ws[rows * cap_runs * 4:rows * cap_runs * 8].reshape(rows, 4 * cap_runs)
    at, n_rec, n_over = 0, 0, 0
    for b in range(req.batch):
        for r in range(req.max_det):
            one, g = rec[b, r], b * req.max_det + r
            if not req.is_record(b, r, live):
                assert one['state'] == 0 and one['str_len'] == 0, (b, r, one)
                assert (slabs[g] == 0xA5).all() and (pos[g] == 0xA5A5A5A5).all(), (b, r)
                assert one['str_off'] == at
                continue
            want, runs = req.oracle(b, r)
            n_rec += 1
            assert one['class_id'] == req.ids_np[b, r] and one['score'] == req.scores_np[b, r] and (one['box'] == req.boxes_np[b, r]).all()
            assert one['nruns'] == runs, (b, r, one, runs)
            assert one['str_off'] == at, (b, r, one, at)
            if runs > cap_runs:
                n_over += 1
                assert one['state'] == 2 and one['str_len'] == 0, (b, r, one)
                assert (slabs[g] == 0xA5).all() and (pos[g] == 0xA5A5A5A5).all(), (b, r)
                continue
            assert one['state'] == 1 and one['str_len'] == len(want), (b, r, one)
            assert strings[at:at + len(want)].tobytes().decode('ascii') == want, (b, r)
            assert (slabs[g, len(want):] == 0xA5).all() and (pos[g, runs - 1:] == 0xA5A5A5A5).all(), (b, r)
            at += len(want)
    assert header.tolist() == [at, n_rec, n_over, 0]
    assert (sbuf[:GUARD] == 0x5A).all() and (sbuf[GUARD + at:] == 0x5A).all()
    assert (ws[-GUARD:] == 0xA5).all()
    return n_rec, n_over


def _oracle_files(tmp_path, name, requests):
    """The two files `MakeJson` writes for `requests` = [(request, image ids)] with the oracle's strings, as bytes."""
    from yolact_minimal_amd.utils.common_utils import MakeJson
    mj = MakeJson(LABELS)
    for req, image_ids in requests:
        for b in range(req.batch):
            for r in range(req.max_det):
                if image_ids[b] is not None and req.is_record(b, r):
                    mj.add_bbox(image_ids[b], req.ids_np[b, r], req.boxes_np[b, r, :], float(req.scores_np[b, r]))
                    mj.add_mask(image_ids[b], req.ids_np[b, r], {'size': list(req.sizes[b]), 'counts': req.oracle(b, r)[0]},
                                float(req.scores_np[b, r]))
    return _dump(tmp_path, name, mj)


def _dump(tmp_path, name, mj):
    paths = (tmp_path / f'{name}_bbox.json', tmp_path / f'{name}_mask.json')
    mj.dump(*map(str, paths))
    return tuple(p.read_bytes() for p in paths)


# ---- 1, 2: edge sizes, overflow -------------------------------------------------------------------------------------------------
def test_edge_sizes_in_one_request():
    req = _edge_request()
    n_rec, n_over = _check_against_oracle(req, 16384, *_encode(req, 16384))
    assert n_rec == sum(EDGE_COUNTS) and n_over == 0


def test_overflow_at_the_default_cap_runs(tmp_path):
    from yolact_minimal_amd.utils.common_utils import BatchMakeJson
    req = _edge_request()
    assert req.oracle(4, 3)[1] == 8450 and 4096 < req.oracle(4, 2)[1] < 4400        # 65 x 130: the checkerboard and the random row
    header, rec, sbuf, ws = _encode(req, 4096)
    _, n_over = _check_against_oracle(req, 4096, header, rec, sbuf, ws)
    assert n_over == 2 and rec['state'][4].tolist() == [1, 1, 2, 2, 1]
    assert rec['nruns'][4, 3] == 8450 and rec['nruns'][4, 2] == req.oracle(4, 2)[1]
    n_rec, n_over = _check_against_oracle(req, 64, *_encode(req, 64))
    assert n_over > n_rec // 2
    image_ids = list(range(100, 108))
    want = _oracle_files(tmp_path, 'want', [(req, image_ids)])
    for cap in (4096, 64):                                          # the rows that did not fit come from the re-encode path
        mj = BatchMakeJson(LABELS)
        mj.add_batch(*req.args(), image_ids, cap_runs=cap)
        assert _dump(tmp_path, f'got{cap}', mj) == want
    assert len(json.loads(want[1])) == sum(EDGE_COUNTS)


# ---- 3, 4: rows that are no records ---------------------------------------------------------------------------------------------
def test_rows_past_the_count_and_padding_images_are_never_read():
    clean, dirty = _edge_request(), _edge_request(True, (4, 7))
    live = [b not in (4, 7) for b in range(8)]
    got = _encode(dirty, 16384, live)
    _check_against_oracle(clean, 16384, *got, live=live)             # (the oracle of the clean masks: garbage rows are state 0)
    assert (got[1]['state'][[4, 7]] == 0).all()
    ref = _encode(clean, 16384)[1]
    for b in range(8):
        if live[b]:
            for name in ('class_id', 'score', 'box', 'str_len', 'nruns', 'state'):
                assert (got[1][name][b] == ref[name][b]).all()


def test_zero_area_boxes_are_no_records():
    base = _edge_request()
    boxes = base.boxes_np.copy()
    boxes[2, 1, 2] = boxes[2, 1, 0]                                  # x2 == x1
    boxes[4, 0, 3] = boxes[4, 0, 1]                                  # y2 == y1
    boxes[2, 3] = [5, 9, 3, 7]                                       # both differences negative: the product is positive, a record
    req = _Request(EDGE_SIZES, base.masks_np, EDGE_COUNTS, boxes=boxes)
    header, rec, sbuf, ws = _encode(req, 16384)
    n_rec, _ = _check_against_oracle(req, 16384, header, rec, sbuf, ws)
    assert n_rec == sum(EDGE_COUNTS) - 2 and rec['state'][2, 1] == 0 and rec['state'][4, 0] == 0 and rec['state'][2, 3] == 1


# ---- 5, 6: long runs, batch sizes -----------------------------------------------------------------------------------------------
def test_long_runs_one_image():
    m = np.zeros((1, 1100, 1000), dtype=bool)
    m[0, 500, 500] = True
    req = _Request([(1100, 1000)], [m], [1])
    header, rec, sbuf, ws = _encode(req, 4096)
    _check_against_oracle(req, 4096, header, rec, sbuf, ws)
    assert sbuf[GUARD:GUARD + header[0]].tobytes() == b'Tci`01kch`0' and rec['nruns'][0, 0] == 3


def test_thirty_two_images():
    rng = np.random.default_rng(3)
    sizes = [(1, 1), (1, 1)] + [(3 + 5 * b % 41, 2 + 9 * b % 150) for b in range(2, 32)]
    masks = [np.stack([_mask(KINDS[(r + b) % 5], h, w, rng) for r in range(3)]) for b, (h, w) in enumerate(sizes)]
    req = _Request(sizes, masks, [(b + 1) % 4 for b in range(32)])
    n_rec, n_over = _check_against_oracle(req, 8192, *_encode(req, 8192))         # (at most 43 x 151 = 6493 pixels)
    assert n_rec == sum((b + 1) % 4 for b in range(32)) and n_over == 0


# ---- 7, 8: BatchMakeJson's inputs ---------------------------------------------------------------------------------------------------
def test_the_mask_input_forms_agree(tmp_path):
    from yolact_minimal_amd.utils.common_utils import BatchMakeJson
    from yolact_minimal_amd.utils.packed_masks import PackedMasks, pack_reference
    rng = np.random.default_rng(4)
    sizes = [(37, 70)] * 4                                           # (5 x 37 x 2 words per block: no multiple of 256 bytes)
    masks = [np.stack([_mask(KINDS[(r + b) % 5], 37, 70, rng) for r in range(5)]) for b in range(4)]
    req = _Request(sizes, masks, [5, 0, 3, 4])
    uniform = PackedMasks(torch.from_numpy(pack_reference(np.stack(masks))).to(DEV), 37, 70)
    assert uniform.shape == (4, 5, 37, 70)
    image_ids = [11, 12, 13, None]
    blocks = []
    for form in ('list', 'table', 'uniform'):
        mj = BatchMakeJson(LABELS)
        if form == 'table':
            mj.add_batch(req.ids, req.scores, req.boxes, req.views[0], req.counts, image_ids, mask_table=hip.ragged_table(sizes, req.offsets))
        else:
            mj.add_batch(req.ids, req.scores, req.boxes, req.views if form == 'list' else uniform, req.counts, image_ids)
        (rec, blob, ids), = mj.wait()
        assert ids == image_ids and (rec['state'][3] == 0).all() and rec['state'].sum() == 8
        blocks.append((rec, blob, _dump(tmp_path, form, mj)))
    for rec, blob, files in blocks[1:]:
        assert rec.tobytes() == blocks[0][0].tobytes() and blob.tobytes() == blocks[0][1].tobytes() and files == blocks[0][2]
    assert blocks[0][2] == _oracle_files(tmp_path, 'want', [(req, image_ids)])
    with pytest.raises(RuntimeError, match='packed masks only'):
        BatchMakeJson(LABELS).add_batch(req.ids, req.scores, req.boxes, torch.zeros(4, 5, 37, 70, device=DEV), req.counts, image_ids)


def test_two_streams_dump_what_one_stream_dumps(tmp_path):
    from yolact_minimal_amd.utils.common_utils import BatchMakeJson
    rng = np.random.default_rng(6)
    reqs = []
    for k, sizes in enumerate(([(40, 100), (129, 65)], [(64, 64), (20, 300)])):
        masks = [np.stack([_mask(KINDS[(r + b + k) % 5], h, w, rng) for r in range(4)]) for b, (h, w) in enumerate(sizes)]
        reqs.append(_Request(sizes, masks, [4, 3 - k]))
    ids = [[1, 2], [3, 4]]
    torch.cuda.synchronize()
    one = BatchMakeJson(LABELS)
    for req, image_ids in zip(reqs, ids):
        one.add_batch(*req.args(), image_ids)
    two = BatchMakeJson(LABELS)
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    for req, image_ids, s in zip(reqs, ids, streams):
        with torch.cuda.stream(s):
            two.add_batch(*req.args(), image_ids)
    want = _dump(tmp_path, 'one', one)
    assert _dump(tmp_path, 'two', two) == want == _oracle_files(tmp_path, 'want', list(zip(reqs, ids)))
    torch.cuda.synchronize()


# ---- 9: the pipeline --------------------------------------------------------------------------------------------------------------
QUADS = [[(97, 301), (333, 64), (48, 70), (120, 128)], [(64, 64), (96, 128), (200, 150), (301, 97)], [(257, 256), (50, 75), (50, 75), (50, 75)]]


def test_pipeline_consumer_dumps_what_the_per_image_path_dumps(tmp_path):
    """`RequestPipeline(batch=4, depth=2)` on synthetic head outputs, three requests at mixed output sizes, the last one a short group
    of two images padded with copies of its last image: the consumer is `BatchMakeJson.add_batch`; the yardstick reads every
    request back (`finish`) and feeds a `MakeJson` image by image (dropin/reference_loops.py's `coco_api='device'` branch)."""
    import bench
    from yolact_minimal_amd.pipeline import RequestPipeline
    from yolact_minimal_amd.utils.common_utils import BatchMakeJson, MakeJson, rle_encode
    dev = torch.device(DEV)
    net, cfg = bench.build_net('res50_coco', 128, dev)
    n_anchors = len(net.anchors) // 4

    def head(seeds):
        parts = [R.synth_head_outputs(n_anchors, num_classes=cfg.num_classes, proto_hw=32, seed=s, bg_bias=b) for s, b in seeds]
        return [torch.cat([p[i] for p in parts], 0).to(DEV) for i in range(4)]

    heads = [head([(3, 5.0), (4, 30.0), (5, 3.0), (6, 4.0)]), head([(7, 6.0), (8, 5.0), (9, 4.0), (10, 5.0)]),
             head([(11, 5.0), (12, 4.0), (12, 4.0), (12, 4.0)])]
    real = [4, 4, 2]
    image_ids = [[900 + 4 * k + b if b < real[k] else None for b in range(4)] for k in range(3)]
    many, one = BatchMakeJson(), MakeJson()
    try:
        img = torch.randn(4, 3, 128, 128, generator=torch.Generator().manual_seed(5)).to(dev)
        pipe = RequestPipeline(net, cfg, 128, 128, dev, depth=2, out_hw=(96, 128), batch=4, packed_masks=True)
        pipe.warm_up(img, rounds=0)
        for k in range(3):
            pipe.submit(img, heads[k], out_hw=QUADS[k],
                        consumer=lambda *r, k=k: many.add_batch(*r, image_ids[k]))
        pipe.drain()
        got = [pipe.submit(img, heads[k], out_hw=QUADS[k]) for k in range(3)]
        got = [r for r in got if r is not None] + pipe.drain()
    finally:
        net._engines.clear()
    assert len(got) == 3
    for k, request in enumerate(got):
        for b in range(real[k]):
            ids_p, class_p, boxes_p, masks_p = request[b]
            if ids_p is None:
                continue
            ids_l, class_l = list(ids_p.cpu().numpy().astype(int)), list(class_p.cpu().numpy().astype(float))
            boxes_l, rles = boxes_p.cpu().numpy(), rle_encode(masks_p)
            for j in range(len(rles)):
                if (boxes_l[j, 3] - boxes_l[j, 1]) * (boxes_l[j, 2] - boxes_l[j, 0]) > 0:
                    one.add_bbox(image_ids[k][b], ids_l[j], boxes_l[j, :], class_l[j])
                    one.add_mask(image_ids[k][b], ids_l[j], rles[j], class_l[j])
    want = _dump(tmp_path, 'one', one)
    assert _dump(tmp_path, 'many', many) == want
    assert len(one.mask_data) > 20 and {d['image_id'] for d in one.mask_data} >= {900, 904, 908, 909}


def test_evaluate_json_pipelined_at_batch_one_equals_the_per_image_path(tmp_path):
    """res50 at 128 px with seeded weights, five images of mixed output sizes, depth 2, requests of one image (the uniform entry's
    batch of one) on one pipeline: `evaluate_json_pipelined` against reading every request back and feeding a `MakeJson`."""
    import bench
    from yolact_minimal_amd.evaluate import eval_pipeline, evaluate_json_pipelined
    from yolact_minimal_amd.utils.common_utils import BatchMakeJson, MakeJson, rle_encode
    dev = torch.device(DEV)
    net, cfg, _ = bench.detecting_net('res50_coco', 128, dev)
    sizes = [(48, 64), (64, 48), (37, 50), (64, 64), (33, 70)]
    image_ids = [70, 10, 30, 20, 60]
    g = torch.Generator().manual_seed(23)
    samples = [(torch.randn(1, 3, 128, 128, generator=g).to(dev), None, None, h, w) for h, w in sizes]
    one = MakeJson()
    try:
        pipe = eval_pipeline(net, cfg, samples[0][0], 48, 64, depth=2, packed_masks=True)
        many = evaluate_json_pipelined(net, cfg, list(samples), image_ids, pipe=pipe)
        got = [pipe.submit(img, out_hw=(h, w)) for img, _, _, h, w in samples]
        got = [r for r in got if r is not None] + pipe.drain()
    finally:
        net._engines.clear()
    assert isinstance(many, BatchMakeJson) and len(got) == 5
    for image_id, (ids_p, class_p, boxes_p, masks_p) in zip(image_ids, got):
        if ids_p is None:
            continue
        ids_l, class_l = list(ids_p.cpu().numpy().astype(int)), list(class_p.cpu().numpy().astype(float))
        boxes_l, rles = boxes_p.cpu().numpy(), rle_encode(masks_p)
        for j in range(len(rles)):
            if (boxes_l[j, 3] - boxes_l[j, 1]) * (boxes_l[j, 2] - boxes_l[j, 0]) > 0:
                one.add_bbox(image_id, ids_l[j], boxes_l[j, :], class_l[j])
                one.add_mask(image_id, ids_l[j], rles[j], class_l[j])
    assert len(one.mask_data) >= 5, 'the network must detect something for this test to mean anything'
    assert _dump(tmp_path, 'many', many) == _dump(tmp_path, 'one', one)
