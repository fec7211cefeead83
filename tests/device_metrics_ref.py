"""Host model of the device-resident mAP accumulator (include/yolact_hip.h, "device-resident mAP accumulator") and the shared inputs
of its tests.  TEST INFRASTRUCTURE ONLY: NumPy, no GPU.

The model follows the kernel's CONTRACT, not its code: log rows (score, class, 2T flag bits) plus gt counts in, AP grid and empty
flags out; rows sorted by (class ascending, score descending, log position ascending); per cell fp64 quotients tp / (rank + 1) and
tp / num_gt, the suffix maximum, 101 samples added left to right.  `ap_cell_passes` restates the same cell the way `k_eval_ap` walks
it (backwards, in passes with carried state) so that the walk itself can be checked without a GPU.
"""
import numpy as np
import torch

from oracle import metrics_ref as M

THRES = [x / 100 for x in range(50, 100, 5)]
SEQUENCE = [(11, 12, 4, 40, 56), (12, 7, 6, 40, 56), (13, 12, 1, 33, 47), (14, 1, 3, 40, 56), (15, 9, 5, 64, 70), (16, 12, 6, 40, 56)]
SEQUENCE_CLASSES = 5


def sort_order(score, cls):
    """Log positions by (class ascending, score descending, position ascending): np.lexsort is stable."""
    return np.lexsort((-np.asarray(score, dtype=np.float64), np.asarray(cls)))


def ap_cell(bits, num_gt):
    """One cell from its hit bits in sorted order."""
    n = len(bits)
    if num_gt == 0 or n == 0:
        return 0.0
    tp = np.cumsum(np.asarray(bits, dtype=np.int64))
    precision = tp.astype(np.float64) / np.arange(1, n + 1, dtype=np.float64)
    recall = tp.astype(np.float64) / np.float64(num_gt)
    envelope = np.maximum.accumulate(precision[::-1])[::-1]
    total = 0.0
    for k in range(101):
        reached = np.nonzero(recall >= float(k) / 100.0)[0]
        total += float(envelope[reached[0]]) if len(reached) else 0.0
    return total / 101.0


def ap_cell_passes(bits, num_gt, rows_per_pass):
    """The same cell walked like the kernel: count the true positives, then go backwards in passes carrying (true positives before
    the pass, envelope behind it); grid value k is sampled in the one pass whose tp range holds t_k, the smallest tp whose recall
    quotient reaches k / 100.0."""
    bits = np.asarray(bits, dtype=np.int64)
    n = len(bits)
    if num_gt == 0 or n == 0:
        return 0.0
    t_k = []
    for k in range(101):
        t = 0
        while t < num_gt and np.float64(t) / np.float64(num_gt) < float(k) / 100.0:
            t += 1
        t_k.append(t)
    samples = [0.0] * 101
    remaining, carry = int(bits.sum()), -1.0
    for r0 in range((n - 1) // rows_per_pass * rows_per_pass, -1, -rows_per_pass):
        chunk = bits[r0:r0 + rows_per_pass]
        tp_in = remaining - int(chunk.sum())
        tp = tp_in + np.cumsum(chunk)
        precision = tp.astype(np.float64) / np.arange(r0 + 1, r0 + len(chunk) + 1, dtype=np.float64)
        envelope = np.maximum(np.maximum.accumulate(precision[::-1])[::-1], carry)
        for k, t in enumerate(t_k):
            if (r0 == 0) if t == 0 else (tp_in < t <= remaining):
                samples[k] = float(envelope[int(np.searchsorted(tp, t, side='left'))])
        carry, remaining = float(envelope[0]), tp_in
    total = 0.0
    for s in samples:
        total += s
    return total / 101.0


def ap_grid(score, cls, flags, gt_count, num_thres, num_classes, cell=ap_cell):
    """(ap float64 [2, T, classes], empty bool [classes]) of a log."""
    score, cls, flags = np.asarray(score, dtype=np.float32), np.asarray(cls, dtype=np.int64), np.asarray(flags, dtype=np.uint32)
    order = sort_order(score, cls)
    ap = np.zeros((2, num_thres, num_classes), dtype=np.float64)
    empty = np.zeros(num_classes, dtype=bool)
    for c in range(num_classes):
        seg = flags[order[cls[order] == c]]
        empty[c] = len(seg) == 0 and gt_count[c] == 0
        for b in range(2 * num_thres):
            ap[b // num_thres, b % num_thres, c] = cell((seg >> np.uint32(b)) & np.uint32(1), int(gt_count[c]))
    return ap, empty


def quantise(scores):
    """floor(s * 8) / 8 + 1 / 16: exact in fp32, the order of distinct values is kept, and images share score values (ties)."""
    return [float(np.floor(s * 8) / 8 + 1 / 16) for s in scores]


def sequence_images(quantised=True):
    """The six-image sequence: [(ids, scores, boxes, masks, gt, gt_masks, h, w)], synth_eval_case with 5 classes."""
    out = []
    for seed, n, g, h, w in SEQUENCE:
        ids, scores, boxes, masks, gt, gt_masks, h, w = M.synth_eval_case(seed, n, g, h, w, SEQUENCE_CLASSES)
        out.append((ids, quantise(scores) if quantised else scores, boxes, masks, gt, gt_masks, h, w))
    return out


def golden_images(gold, case):
    n, g, h, w, nc = (int(v) for v in gold[f'c{case}_shape'])
    return [M.synth_eval_case(int(gold[f'c{case}_seed']), n, g, h, w, nc)], nc


def oracle_accumulate(images, num_classes, thres=THRES):
    """The oracle's ap_data after prep_metrics over the images, in order."""
    ap = M.new_ap_data(num_classes, len(thres))
    for ids, scores, boxes, masks, gt, gt_masks, h, w in images:
        M.prep_metrics(ap, ids, scores, boxes, masks, gt, gt_masks, h, w, thres)
    return ap


def oracle_log(images, num_classes, max_det, thres=THRES):
    """The log the accumulator should hold after these images, from the oracle run on each image alone: (score fp32, class int32,
    flags uint32) of len(images) * max_det rows and gt_count int64."""
    t = len(thres)
    score = np.zeros(len(images) * max_det, dtype=np.float32)
    cls = np.full(len(images) * max_det, -1, dtype=np.int32)
    flags = np.zeros(len(images) * max_det, dtype=np.uint32)
    gt_count = np.zeros(num_classes, dtype=np.int64)
    for slot, (ids, scores, boxes, masks, gt, gt_masks, h, w) in enumerate(images):
        one = M.new_ap_data(num_classes, t)
        M.prep_metrics(one, ids, scores, boxes, masks, gt, gt_masks, h, w, thres)
        base = slot * max_det
        score[base:base + len(ids)] = np.asarray(scores, dtype=np.float32)
        cls[base:base + len(ids)] = ids
        for c in range(num_classes):
            gt_count[c] += one['box'][0][c].num_gt_positives
            rows = [i for i, pc in enumerate(ids) if pc == c]
            for b in range(2 * t):
                pts = one['box' if b < t else 'mask'][b % t][c].data_points
                for i, p in zip(rows, pts):
                    if p[1]:
                        flags[base + i] |= np.uint32(1 << b)
    return score, cls, flags, gt_count


def grid_rows(ap_data, num_classes, thres=THRES):
    """tests/golden/metrics.npz `c*_ap_grid`: [num_gt, points, true positives, AP] per (kind, threshold, class)."""
    rows = []
    for kind in ('box', 'mask'):
        for k in range(len(thres)):
            for c in range(num_classes):
                a = ap_data[kind][k][c]
                rows.append([a.num_gt_positives, len(a.data_points), sum(1 for p in a.data_points if p[1]), a.get_ap()])
    return np.array(rows, dtype=np.float64)


def log_grid_rows(score, cls, flags, gt_count, num_classes, thres=THRES, cell=ap_cell):
    """The same rows from a log through the host model."""
    ap, _ = ap_grid(score, cls, flags, gt_count, len(thres), num_classes, cell)
    rows = []
    for b in range(2 * len(thres)):
        for c in range(num_classes):
            mine = np.asarray(cls) == c
            rows.append([gt_count[c], int(mine.sum()), int(((np.asarray(flags)[mine] >> np.uint32(b)) & 1).sum()),
                         ap[b // len(thres), b % len(thres), c]])
    return np.array(rows, dtype=np.float64)


def to_device(image, dev, max_det=None, packed=False):
    """One image's `DeviceAPData.add` arguments on `dev`.  `max_det`: pad the detection tensors to that many rows with NaN scores,
    class 3 and all-ones masks past the count (what a kernel must not look at) and pass the count on the device."""
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    ids, scores, boxes, masks, gt, gt_masks, h, w = image
    n = len(ids)
    rows = n if max_det is None else max_det
    ids_t = torch.full((rows,), 3, dtype=torch.int64)
    ids_t[:n] = torch.tensor(ids, dtype=torch.int64)
    sc_t = torch.full((rows,), float('nan'), dtype=torch.float32)
    sc_t[:n] = torch.tensor(scores, dtype=torch.float32)
    bx_t = torch.zeros(rows, 4, dtype=torch.int32)
    bx_t[:n] = boxes
    m_t = torch.ones(rows, h, w, dtype=torch.float32)
    m_t[:n] = masks
    m_d = m_t.to(dev)
    counts = None if max_det is None else torch.tensor([n], dtype=torch.int32).to(dev)
    return (ids_t.to(dev), sc_t.to(dev), bx_t.to(dev), PackedMasks.pack(m_d) if packed else m_d, counts, gt.clone().to(dev),
            gt_masks.to(dev), h, w)
