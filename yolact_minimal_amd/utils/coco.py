"""The COCO reader feeding the hot path.

Reference: `/root/reference/utils/coco.py` — `COCODetection :47-134`, `train_collate :14-28`, `val_collate :31-35`,
`detect_collate :38-40`; it leans on `pycocotools.coco.COCO` (annotation index, `annToMask`) and `cv2.imread`, neither of which
exists in the build image.

What is rebuilt and how:

* `COCO` — the annotation index (`imgToAnns`, `getAnnIds`, `loadAnns`, `loadImgs`, `annToMask`), same method names; plain
  JSON bookkeeping on the host, like pycocotools' own Python class.
* `anns_to_masks` / `COCO.annToMask` — polygon / RLE annotation -> dense uint8 mask **on the device** (`ym_poly_to_mask`,
  `ym_runs_to_mask`): the reference rasterises every instance on the CPU and later ships n x H x W floats over PCIe; here
  only the vertices cross and the masks are born in HBM, where `train_aug` / `val_aug` / the loss kernels consume them.
* `pack_annotations` / `anns_to_masks_batch` / `COCO.annsToMasksBatch` — the same for the images of a whole batch, whatever their
  sizes: one packed host buffer, one pinned upload, one `ym_ann_to_mask_ragged` launch per 32 images (`finish_batch`).
* image decode — PIL (libjpeg) instead of `cv2.imread`; BGR channel order and EXIF orientation handled like cv2.  Host I/O,
  "parity unpinned" (no cv2 here to compare with).
* `COCODetection.__getitem__` — same three modes and return shapes as the reference, with CUDA tensors for the image and the
  masks (boxes / labels stay small host arrays).  Because samples are produced on the GPU there are no DataLoader worker
  processes: `BatchLoader` shards indices per rank like `DistributedSampler`, decodes JPEGs on a small thread pool (PIL releases
  the GIL) and collates with the reference's rules (`train_collate`: a rejected sample is replaced by a repeated valid one).
"""
import glob
import json
import os.path as osp
import random as _random
from collections import defaultdict, namedtuple
from concurrent.futures import ThreadPoolExecutor

import ctypes

import numpy as np
import torch

from .. import hip
from .augmentations import _train_window, train_aug, train_aug_batch, val_aug


def _rle_string_to_counts(s):
    """cocoapi rleFrString: 5 data bits per character (+48), bit 5 = continuation, sign-extended, delta-coded from the third on."""
    if isinstance(s, bytes):
        s = s.decode('ascii')
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def anns_to_masks(segmentations, height, width, device='cuda'):
    """[n] COCO `segmentation` entries (polygon lists or RLE dicts) of one image -> uint8 CUDA tensor [n, height, width]
    (what `np.stack([coco.annToMask(a) for a in anns])` is in the reference, utils/coco.py:96,102)."""
    n = len(segmentations)
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('yolact_minimal_amd.utils.coco rasterises masks with HIP kernels: a CUDA/HIP device is required')
    masks = torch.empty(n, height, width, dtype=torch.uint8, device=dev)
    if n == 0:
        return masks
    poly_idx = [i for i, s in enumerate(segmentations) if isinstance(s, list)]
    run_idx = [i for i in range(n) if i not in set(poly_idx)]
    L = hip.lib()
    with torch.cuda.device(dev):
        def _ws(count):
            nbytes = L.ym_ann_to_mask_workspace_bytes(count, height, width)
            return torch.empty(max(nbytes, 4) // 4 + 1, dtype=torch.int32, device=dev), nbytes

        def _dev(arr, dtype):
            return torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).to(dev)

        for idx, is_poly in ((poly_idx, True), (run_idx, False)):
            if not idx:
                continue
            whole = len(idx) == n
            out = masks if whole else torch.empty(len(idx), height, width, dtype=torch.uint8, device=dev)
            ws, ws_bytes = _ws(len(idx))
            if is_poly:
                xy, poly_off, ann_off = [], [0], [0]
                for i in idx:
                    for poly in segmentations[i]:
                        k = len(poly) // 2                       # frPyObjects: k = len / 2, a trailing odd value is ignored
                        xy.extend(poly[:2 * k])
                        poly_off.append(poly_off[-1] + k)
                    ann_off.append(len(poly_off) - 1)
                d_xy = _dev(xy if xy else [0.0], np.float64)
                d_po, d_ao = _dev(poly_off, np.int32), _dev(ann_off, np.int32)
                hip.check(L.ym_poly_to_mask(ctypes.c_void_p(d_xy.data_ptr()), ctypes.c_void_p(d_po.data_ptr()),
                                            ctypes.c_void_p(d_ao.data_ptr()), len(idx), height, width, ctypes.c_void_p(out.data_ptr()),
                                            ctypes.c_void_p(ws.data_ptr()), ws_bytes, hip.stream_ptr()), 'ym_poly_to_mask')
            else:
                counts, run_off = [], [0]
                for i in idx:
                    seg = segmentations[i]
                    c = seg['counts']
                    c = _rle_string_to_counts(c) if isinstance(c, (str, bytes)) else list(c)
                    if list(seg.get('size', [height, width])) != [height, width]:
                        raise ValueError(f"RLE annotation of size {seg.get('size')} in a {height} x {width} image")
                    counts.extend(c)
                    run_off.append(len(counts))
                d_c, d_ro = _dev(counts if counts else [0], np.uint32), _dev(run_off, np.int32)
                hip.check(L.ym_runs_to_mask(ctypes.c_void_p(d_c.data_ptr()), ctypes.c_void_p(d_ro.data_ptr()), len(idx), height, width,
                                            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws_bytes, hip.stream_ptr()),
                          'ym_runs_to_mask')
            if not whole:
                masks[torch.as_tensor(idx, device=dev)] = out
    return masks


PackedAnnotations = namedtuple('PackedAnnotations', 'xy counts item_off ann_off ann_kind ann_first sizes block_offsets total_bytes '
                                                    'buffer array_offsets')
PackedAnnotations.__doc__ = """What `pack_annotations` returns: the five arrays of `ym_ann_to_mask_ragged` (views of `buffer`, a flat
uint8 host array, each starting at its 8-byte aligned `array_offsets[name]`), `ann_first` = [len(images) + 1] ints, and the layout of the
masks: image b's `[n_b, h_b, w_b]` block starts at byte `block_offsets[b]` of an allocation of `total_bytes`."""


def _mask_block_layout(sizes, n_per_image):
    """Byte offsets of the images' `[n_b, h_b, w_b]` uint8 blocks and where the last one ends: `frame_layout`'s rule (`hip.aligned_layout`:
    every block at a multiple of 256 bytes) with a block's own extent, applied per launch of at most 32 images, one launch's blocks
    behind the other's."""
    offsets, end = [], 0
    for i0 in range(0, len(sizes), hip.RAGGED_MAX_IMAGES):
        base = -(-end // hip.RAGGED_ALIGN_BYTES) * hip.RAGGED_ALIGN_BYTES
        count = iter(n_per_image[i0:i0 + hip.RAGGED_MAX_IMAGES])               # (aligned_layout asks for the extents in image order)
        offs, total = hip.aligned_layout('pack_annotations', sizes[i0:i0 + hip.RAGGED_MAX_IMAGES], 1, lambda h, w: next(count) * h * w)
        offsets += [base + o for o in offs]
        end = base + total
    return offsets, end


def pack_annotations(segs_per_image, sizes, alloc=None):
    """Host half of `anns_to_masks_batch` (numpy only, no GPU, no library): `segs_per_image` = [[COCO `segmentation`, ...] per image],
    `sizes` = [(h, w) per image] -> `PackedAnnotations`.  The rules are `anns_to_masks`': k = len(poly) // 2 vertices per polygon, a
    compressed RLE string is decoded, an RLE whose `size` is not its image's raises ValueError.  Annotation a (global, in image order)
    owns the entries `item_off[ann_off[a] : ann_off[a + 1]]`: the start of each of its items and one closing end -- (x, y) pairs of
    `xy` for a polygon list (`ann_kind` 0), one item in `counts` for run lengths (`ann_kind` 1).  `alloc(nbytes)` supplies the flat
    uint8 buffer (default `np.empty`; `anns_to_masks_batch` hands out pinned memory)."""
    segs_per_image = [list(segs) for segs in segs_per_image]
    sizes = [(int(h), int(w)) for h, w in sizes]
    if len(segs_per_image) != len(sizes):
        raise ValueError(f'pack_annotations: {len(segs_per_image)} annotation lists for {len(sizes)} image sizes')
    xy, counts, item_off, ann_off, ann_kind, ann_first = [], [], [], [0], [], [0]
    n_xy = 0
    for segs, (height, width) in zip(segs_per_image, sizes):
        for seg in segs:
            if isinstance(seg, list):
                for poly in seg:
                    k = len(poly) // 2                               # frPyObjects: k = len / 2, a trailing odd value is ignored
                    xy.extend(poly[:2 * k])
                    item_off.append(n_xy)
                    n_xy += k
                item_off.append(n_xy)
                ann_kind.append(0)
            else:
                c = seg['counts']
                c = _rle_string_to_counts(c) if isinstance(c, (str, bytes)) else list(c)
                if list(seg.get('size', [height, width])) != [height, width]:
                    raise ValueError(f"RLE annotation of size {seg.get('size')} in a {height} x {width} image")
                item_off.append(len(counts))
                counts.extend(c)
                item_off.append(len(counts))
                ann_kind.append(1)
            ann_off.append(len(item_off))
        ann_first.append(len(ann_kind))
    block_offsets, total_bytes = _mask_block_layout(sizes, [len(segs) for segs in segs_per_image])
    arrays = (('xy', xy, np.float64), ('counts', counts, np.uint32), ('item_off', item_off, np.int32), ('ann_off', ann_off, np.int32),
              ('ann_kind', ann_kind, np.int32))
    array_offsets, end = {}, 0
    for name, values, dtype in arrays:
        array_offsets[name] = end
        end += -(-len(values) * np.dtype(dtype).itemsize // 8) * 8
    buffer = (alloc or (lambda nbytes: np.empty(nbytes, np.uint8)))(max(end, 8))
    views = {}
    for name, values, dtype in arrays:
        views[name] = buffer[array_offsets[name]:array_offsets[name] + len(values) * np.dtype(dtype).itemsize].view(dtype)
        views[name][:] = np.asarray(values, dtype=dtype)
    return PackedAnnotations(views['xy'], views['counts'], views['item_off'], views['ann_off'], views['ann_kind'], ann_first, sizes,
                             block_offsets, total_bytes, buffer, array_offsets)


def anns_to_masks_batch(segs_per_image, sizes, device='cuda', out=None):
    """`anns_to_masks` for the images of a batch, of any sizes: [[segmentation, ...] per image], [(h, w) per image] -> a list of
    `[n_b, h_b, w_b]` uint8 views of ONE device allocation (an image without annotations: an empty `[0, h_b, w_b]` view), each what
    `anns_to_masks` returns for that image alone.  ONE pinned, non-blocking upload of the packed annotations (the pinned buffer goes
    back to torch's host allocator, which holds it until the copy is done: `FrameBatch.from_numpy`'s rule), one workspace allocation
    if an image's bitmaps do not fit the LDS, ONE `ym_ann_to_mask_ragged` launch per 32 images.  `out`: a flat uint8 device tensor to
    rasterise into instead of a new allocation (bytes between the blocks are not written)."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('yolact_minimal_amd.utils.coco rasterises masks with HIP kernels: a CUDA/HIP device is required')
    pinned = []

    def alloc(nbytes):
        pinned.append(torch.empty(nbytes, dtype=torch.uint8).pin_memory())
        return pinned[0].numpy()
    pk = pack_annotations(segs_per_image, sizes, alloc)
    if out is None:
        out = torch.empty(pk.total_bytes, dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous() and out.device == dev
              and out.numel() >= pk.total_bytes):
        raise RuntimeError(f'anns_to_masks_batch: `out` is a flat contiguous uint8 tensor of at least {pk.total_bytes} bytes on {dev}')
    counts = [pk.ann_first[b + 1] - pk.ann_first[b] for b in range(len(pk.sizes))]
    views = [out[o:o + n * h * w].view(n, h, w) for n, (h, w), o in zip(counts, pk.sizes, pk.block_offsets)]
    if pk.ann_first[-1] == 0:
        return views
    L = hip.lib()
    i32p = ctypes.POINTER(ctypes.c_int32)
    launches = []
    for i0 in range(0, len(pk.sizes), hip.RAGGED_MAX_IMAGES):
        i1 = min(i0 + hip.RAGGED_MAX_IMAGES, len(pk.sizes))
        a0 = pk.ann_first[i0]
        if pk.ann_first[i1] == a0:
            continue
        table = hip.ragged_table(pk.sizes[i0:i1], pk.block_offsets[i0:i1])
        first = (ctypes.c_int32 * (i1 - i0 + 1))(*[f - a0 for f in pk.ann_first[i0:i1 + 1]])
        launches.append((table, first, i1 - i0, a0, L.ym_ann_to_mask_ragged_workspace_bytes(table, ctypes.cast(first, i32p), i1 - i0)))
    with torch.cuda.device(dev):
        packed = pinned[0].to(dev, non_blocking=True)
        at = {name: packed.data_ptr() + o for name, o in pk.array_offsets.items()}
        ws_bytes = max(l[4] for l in launches)
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev) if ws_bytes else None
        for table, first, count, a0, _ in launches:
            # (the annotations of a launch are a0 ...: its ann_off / ann_kind start there, their values stay global)
            hip.check(L.ym_ann_to_mask_ragged(ctypes.c_void_p(at['xy']), ctypes.c_void_p(at['counts']), ctypes.c_void_p(at['item_off']),
                                              ctypes.c_void_p(at['ann_off'] + 4 * a0), ctypes.c_void_p(at['ann_kind'] + 4 * a0), table,
                                              ctypes.cast(first, i32p), count, ctypes.c_void_p(out.data_ptr()),
                                              ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, ws_bytes, hip.stream_ptr()),
                      'ym_ann_to_mask_ragged')
    return views


class COCO:
    """The part of `pycocotools.coco.COCO` the reader uses, same attribute / method names."""

    def __init__(self, annotation_file=None, device='cuda'):
        self.dataset, self.anns, self.cats, self.imgs = {}, {}, {}, {}
        self.imgToAnns, self.catToImgs = defaultdict(list), defaultdict(list)
        self.device = device
        if annotation_file is not None:
            with open(annotation_file, 'r') as f:
                dataset = json.load(f)
            assert type(dataset) == dict, f'annotation file format {type(dataset)} not supported'
            self.dataset = dataset
            self.createIndex()

    def createIndex(self):
        for ann in self.dataset.get('annotations', []):
            self.imgToAnns[ann['image_id']].append(ann)
            self.anns[ann['id']] = ann
        for img in self.dataset.get('images', []):
            self.imgs[img['id']] = img
        for cat in self.dataset.get('categories', []):
            self.cats[cat['id']] = cat
        if 'annotations' in self.dataset and 'categories' in self.dataset:
            for ann in self.dataset['annotations']:
                self.catToImgs[ann['category_id']].append(ann['image_id'])

    @staticmethod
    def _as_list(v):
        return v if isinstance(v, (list, tuple)) else [v]

    def getAnnIds(self, imgIds=[], catIds=[], areaRng=[], iscrowd=None):
        imgIds, catIds = self._as_list(imgIds), self._as_list(catIds)
        if len(imgIds) == len(catIds) == len(areaRng) == 0:
            anns = self.dataset['annotations']
        else:
            if len(imgIds) > 0:
                anns = [a for i in imgIds if i in self.imgToAnns for a in self.imgToAnns[i]]
            else:
                anns = self.dataset['annotations']
            if len(catIds) > 0:
                anns = [a for a in anns if a['category_id'] in catIds]
            if len(areaRng) > 0:
                anns = [a for a in anns if areaRng[0] < a['area'] < areaRng[1]]
        if iscrowd is not None:
            return [a['id'] for a in anns if a['iscrowd'] == iscrowd]
        return [a['id'] for a in anns]

    def loadAnns(self, ids=[]):
        return [self.anns[i] for i in ids] if isinstance(ids, (list, tuple)) else [self.anns[ids]]

    def loadImgs(self, ids=[]):
        return [self.imgs[i] for i in ids] if isinstance(ids, (list, tuple)) else [self.imgs[ids]]

    def annToMask(self, ann):
        """Dense uint8 mask [h, w] of one annotation, on the device (h, w from the image record, like annToRLE)."""
        rec = self.imgs[ann['image_id']]
        return anns_to_masks([ann['segmentation']], rec['height'], rec['width'], self.device)[0]

    def annsToMasks(self, anns):
        """All the annotations of ONE image in one launch -> [n, h, w] uint8 CUDA tensor."""
        rec = self.imgs[anns[0]['image_id']]
        return anns_to_masks([a['segmentation'] for a in anns], rec['height'], rec['width'], self.device)

    def annsToMasksBatch(self, anns_per_image):
        """`annsToMasks` for several images (each list non-empty, of one image) in one launch per 32 images -> a list of
        [n_b, h_b, w_b] uint8 CUDA views of one allocation."""
        recs = [self.imgs[anns[0]['image_id']] for anns in anns_per_image]
        return anns_to_masks_batch([[a['segmentation'] for a in anns] for anns in anns_per_image],
                                   [(rec['height'], rec['width']) for rec in recs], self.device)


def imread_bgr(path):
    """`cv2.imread(path)`: HWC uint8, BGR, EXIF orientation applied (cv2's IMREAD_COLOR default)."""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        im = ImageOps.exif_transpose(im).convert('RGB')
        rgb = np.asarray(im, dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def train_collate(batch):
    """utils/coco.py:14-28: rejected samples (None) are replaced by repeating valid ones; images are stacked."""
    imgs, targets, masks = [], [], []
    valid_batch = [aa for aa in batch if aa[0] is not None]
    lack_len = len(batch) - len(valid_batch)
    for i in range(lack_len):
        valid_batch.append(valid_batch[i])
    for img, boxes, m in valid_batch:
        imgs.append(img)
        targets.append(torch.as_tensor(boxes, dtype=torch.float32).to(img.device))
        masks.append(m.to(torch.float32))
    return torch.stack(imgs, 0), targets, masks


def val_collate(batch):
    img, boxes, masks, h, w = batch[0]
    return img.unsqueeze(0), torch.as_tensor(boxes, dtype=torch.float32), masks.to(torch.float32), h, w


def detect_collate(batch):
    return batch[0][0].unsqueeze(0), batch[0][1], batch[0][2]


class COCODetection:
    """`COCODetection(cfg, mode)` of the reference (utils/coco.py:47-134), samples produced on `device`."""

    def __init__(self, cfg, mode='train', device='cuda', rng=_random, window=None):
        """`window=(Hn, Wn)` (mode 'train' only): samples are the top-left window of the `cfg.img_size` square ones, the input of
        window training (utils/rect.py): images `[3, Hn, Wn]`, masks `[k, Hn, Wn]`, boxes in 0..1 of the square."""
        self.mode, self.cfg, self.device, self.rng = mode, cfg, torch.device(device), rng
        if window is not None and mode != 'train':
            raise RuntimeError(f"COCODetection(window=) serves mode 'train' only, got '{mode}'")
        self.window = _train_window(window, int(cfg.img_size), 'COCODetection')
        if mode in ('train', 'val'):
            self.image_path = cfg.train_imgs if mode == 'train' else cfg.val_imgs
            self.coco = COCO(cfg.train_ann if mode == 'train' else cfg.val_ann, device=self.device)
            self.ids = list(self.coco.imgToAnns.keys())
        elif mode == 'detect':
            self.image_path = sorted(glob.glob(cfg.image + '/*.jpg'))
        self.continuous_id = cfg.continuous_id

    def __len__(self):
        if self.mode == 'train':
            return len(self.ids)
        if self.mode == 'val':
            return len(self.ids) if self.cfg.val_num == -1 else min(self.cfg.val_num, len(self.ids))
        return len(self.image_path)

    def read(self, index):
        """Host half of `__getitem__`: file read + JPEG decode + annotation bookkeeping (thread-safe; BatchLoader runs it on its
        thread pool).  Returns a record for `finish`."""
        if self.mode == 'detect':
            img_name = self.image_path[index]
            return {'img': imread_bgr(img_name), 'name': img_name.split(osp.sep)[-1]}
        img_id = self.ids[index]
        target = self.coco.loadAnns(self.coco.getAnnIds(imgIds=img_id))
        target = [aa for aa in target if not aa['iscrowd']]
        file_name = self.coco.loadImgs(img_id)[0]['file_name']
        img_path = osp.join(self.image_path, file_name)
        assert osp.exists(img_path), f'Image path does not exist: {img_path}'
        img = imread_bgr(img_path)
        assert len(target) > 0, 'No annotation in this image!'
        box_list, label_list, kept = [], [], []
        for aa in target:
            bbox = aa['bbox']
            if self.mode == 'train' and (bbox[0] < 0 or bbox[1] < 0 or bbox[2] < 4 or bbox[3] < 4):
                continue                                         # "some boxes are wrong, ignore them" (:86-88)
            box_list.append(np.array([bbox[0], bbox[1], bbox[0] + bbox[2], bbox[1] + bbox[3]]))
            label_list.append(self.continuous_id[aa['category_id']] - 1)
            kept.append(aa)
        return {'img': img, 'img_id': img_id, 'boxes': box_list, 'labels': label_list, 'anns': kept}

    def finish(self, rec):
        """Device half: H2D of the decoded image, mask rasterisation, augmentation (and the `random` draws, in sample order)."""
        img = rec['img']
        img_dev = torch.from_numpy(img).to(self.device)
        if self.mode == 'detect':
            return val_aug(img_dev, self.cfg.img_size), img, rec['name']
        height, width, _ = img.shape
        if len(rec['boxes']) == 0:
            if self.mode == 'val':
                raise RuntimeError('Error, no valid object in this image.')
            print(f"No valid object in image: {rec['img_id']}. Use a repeated image in this batch.")
            return None, None, None
        boxes, labels = np.array(rec['boxes']), np.array(rec['labels'])
        masks = self.coco.annsToMasks(rec['anns'])
        assert tuple(masks.shape) == (boxes.shape[0], height, width), 'Unmatched annotations.'
        if self.mode == 'train':
            img_out, masks_out, boxes, labels = train_aug(img_dev, masks, boxes, labels, self.cfg.img_size, self.rng, window=self.window)
            if img_out is None:
                return None, None, None
            return img_out, np.hstack((boxes, np.expand_dims(labels, axis=1))), masks_out
        img_out = val_aug(img_dev, self.cfg.img_size)
        boxes = boxes / np.array([width, height, width, height])     # to 0~1 scale
        return img_out, np.hstack((boxes, np.expand_dims(labels, axis=1))), masks, height, width

    def finish_batch(self, recs):
        """`finish` for a whole training batch + `train_collate`, batch-native: ONE pinned upload of the B decoded images
        (`FrameBatch.from_numpy`), ONE rasteriser launch for the masks of all of them (`COCO.annsToMasksBatch`), ONE
        `train_aug_batch` (a launch pair per 16 samples, the images written straight into their rows of the batch tensor), ONE upload of all the targets.  The `random`
        draws are those of B `finish` calls in order.  Returns what `train_collate` returns:
        `(images [B, 3, S, S], [targets_b float32 [k_b, 5]], [masks_b float32 [k_b, S, S]])`."""
        from .frames import FrameBatch
        if self.mode != 'train':
            raise RuntimeError(f"COCODetection.finish_batch serves mode 'train' only, this dataset is in mode '{self.mode}'")
        recs = list(recs)
        frames = FrameBatch.from_numpy([rec['img'] for rec in recs], self.device)
        valid = [rec for rec in recs if len(rec['boxes']) > 0]
        rasters = iter(self.coco.annsToMasksBatch([rec['anns'] for rec in valid]) if valid else [])
        masks, boxes, labels = [], [], []
        for rec, frame in zip(recs, frames.frames):
            if len(rec['boxes']) == 0:
                print(f"No valid object in image: {rec['img_id']}. Use a repeated image in this batch.")
                masks.append(None)
                boxes.append(None)
                labels.append(None)
                continue
            bx = np.array(rec['boxes'])
            m = next(rasters)
            assert tuple(m.shape) == (bx.shape[0], frame.shape[0], frame.shape[1]), 'Unmatched annotations.'
            masks.append(m)
            boxes.append(bx)
            labels.append(np.array(rec['labels']))
        images, masks_out, boxes_out, labels_out = train_aug_batch(frames, masks, boxes, labels, self.cfg.img_size, self.rng,
                                                                    window=self.window)
        rows = [np.hstack((b, np.expand_dims(l, axis=1))) for b, l in zip(boxes_out, labels_out)]
        host = torch.from_numpy(np.concatenate(rows, 0).astype(np.float32)).pin_memory()
        targets = list(host.to(images.device, non_blocking=True).split([r.shape[0] for r in rows], 0))
        return images, targets, masks_out

    def __getitem__(self, index):
        return self.finish(self.read(index))


class BatchLoader:
    """The DataLoader + DistributedSampler pair of train.py:78-81 / eval.py:30 for GPU-resident samples: rank-sharded
    (optionally shuffled, seeded per epoch) indices, `batch_size` samples per step, `dataset.read` (file + JPEG decode) one batch
    ahead on `threads` host threads, `dataset.finish` (HIP launches, `random` draws) in sample order on the caller's thread,
    collated by `collate_fn`."""

    def __init__(self, dataset, batch_size, collate_fn, shuffle=False, rank=0, world_size=1, seed=0, threads=4, drop_last=False,
                 batched=False):
        """`batched=True` (train mode, `train_collate` only): one `dataset.finish_batch` per batch in place of `batch_size` `finish`
        calls + `collate_fn` -- the same batches from the same `random` draws."""
        self.batched = bool(batched)
        if self.batched:
            if getattr(dataset, 'mode', None) != 'train':
                raise RuntimeError(f"BatchLoader(batched=True) needs a dataset in mode 'train', got '{getattr(dataset, 'mode', None)}'")
            if collate_fn is not train_collate:
                raise RuntimeError('BatchLoader(batched=True) produces what train_collate produces: pass collate_fn=train_collate')
            if not 1 <= batch_size <= hip.AUG_MAX_SAMPLES:
                raise RuntimeError(f'BatchLoader(batched=True): 1 .. {hip.AUG_MAX_SAMPLES} samples per batch, got {batch_size}')
        self.dataset, self.batch_size, self.collate_fn = dataset, batch_size, collate_fn
        self.shuffle, self.rank, self.world_size, self.seed, self.threads, self.drop_last = shuffle, rank, world_size, seed, threads, drop_last
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def indices(self):
        """DistributedSampler: permutation seeded by seed + epoch, padded to a multiple of world_size, strided by rank."""
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        total = -(-n // self.world_size) * self.world_size
        order += order[:total - n]
        return order[self.rank:total:self.world_size]

    def __len__(self):
        n = len(self.indices())
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        idx = self.indices()
        batches = [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]
        if self.drop_last and batches and len(batches[-1]) < self.batch_size:
            batches.pop()
        with ThreadPoolExecutor(max_workers=max(1, self.threads)) as pool:
            pending = [pool.submit(self.dataset.read, i) for i in batches[0]] if batches else []
            for b in range(len(batches)):
                ahead = [pool.submit(self.dataset.read, i) for i in batches[b + 1]] if b + 1 < len(batches) else []
                if self.batched:
                    recs = [f.result() for f in pending]
                    pending = ahead
                    yield self.dataset.finish_batch(recs)                       # one upload, one launch pair, draws in sample order
                    continue
                samples = [self.dataset.finish(f.result()) for f in pending]    # GPU work + random draws: consumer thread, in order
                pending = ahead
                yield self.collate_fn(samples)
