"""Host restatement of the COCO evaluation protocol, the yardstick of `utils/coco_eval.DeviceCOCOeval` (no GPU, no torch needed).

`pycocotools` does not exist on this stack, so this file restates the published cocoapi algorithm in plain python / numpy, loop for
loop and name for name, with no shortcuts:

* `bbIou`, `maskIou`            <- cocoapi `common/maskApi.c` `bbIou` / `rleIou` (the mask version counts pixels of dense boolean
                                   masks, which is what the run walk of `rleIou` counts),
* `Params`                      <- `cocoeval.py` `Params.setDetParams`,
* `COCOevalRef._prepare / evaluate / computeIoU / evaluateImg / accumulate / summarize` <- the methods of the same names of
                                   `cocoeval.py` `COCOeval`,
* `scene_annotations`           <- `coco.py` `COCO.loadRes` (ids from 1, `area` of a bbox result = w * h, of a segm result = its pixels).

Parity with the real cocoapi is unpinned: nothing here was ever compared with it.

Below the restatement: the hand-derived known-answer scenes A..H and the seeded random sequence that `tests/test_coco_eval_cpu.py`
and `tests/test_gpu_coco_eval.py` share.  A SCENE is a list of images `{'h', 'w', 'dets': [...], 'gts': [...]}`:
  det = {'cls', 'score' (a float32 value), 'box' (x1, y1, x2, y2 integer pixels), 'mask' (bool [h, w])} in `after_nms` row order,
  gt  = {'cls', 'bbox' [x, y, w, h] floats, 'area', 'iscrowd', 'mask' (bool [h, w])} in annotation-file order.
"""
import copy
import functools
from collections import defaultdict

import numpy as np


# ---- maskApi.c ------------------------------------------------------------------------------------------------------------------
def bbIou(dt, gt, iscrowd):
    """maskApi.c bbIou: dt [m][4], gt [n][4] as [x, y, w, h] doubles -> o [m][n]."""
    m, n = len(dt), len(gt)
    o = np.zeros((m, n), dtype=np.float64)
    for g in range(n):
        G = [np.float64(v) for v in gt[g]]
        ga = G[2] * G[3]
        crowd = iscrowd is not None and iscrowd[g]
        for d in range(m):
            D = [np.float64(v) for v in dt[d]]
            da = D[2] * D[3]
            o[d, g] = 0
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d, g] = i / u
    return o


def maskIou(dt, gt, iscrowd):
    """maskApi.c rleIou on dense boolean masks: i = |d & g|; i == 0 -> 0 (u = 1); crowd -> u = |d|; else u = |d | g|."""
    m, n = len(dt), len(gt)
    o = np.zeros((m, n), dtype=np.float64)
    for g in range(n):
        crowd = iscrowd is not None and iscrowd[g]
        for d in range(m):
            i = int(np.count_nonzero(dt[d] & gt[g]))
            if i == 0:
                u = 1
            elif crowd:
                u = int(np.count_nonzero(dt[d]))
            else:
                u = int(np.count_nonzero(dt[d])) + int(np.count_nonzero(gt[g])) - i
            o[d, g] = np.float64(i) / np.float64(u)
    return o


# ---- cocoeval.py ----------------------------------------------------------------------------------------------------------------
class Params:
    """cocoeval.py Params.setDetParams."""

    def __init__(self, iouType='segm'):
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.iouType = iouType


class COCOevalRef:
    """cocoeval.py COCOeval over plain lists: `gts` / `dts` are annotation dicts (`image_id`, `category_id`, `id`, `bbox`, `area`,
    `iscrowd` for gts, `score` for dts, and `mask`, a boolean array, for `iouType='segm'`)."""

    def __init__(self, gts, dts, iouType, imgIds, catIds):
        self.gts_in, self.dts_in = gts, dts
        self.params = Params(iouType)
        self.params.imgIds = sorted(imgIds)
        self.params.catIds = sorted(catIds)
        self.evalImgs = defaultdict(list)
        self.eval = {}
        self._gts = defaultdict(list)
        self._dts = defaultdict(list)
        self.stats = []
        self.ious = {}

    def _prepare(self):
        p = self.params
        gts = [copy.copy(g) for g in self.gts_in if g['image_id'] in p.imgIds and g['category_id'] in p.catIds]
        dts = [copy.copy(d) for d in self.dts_in if d['image_id'] in p.imgIds and d['category_id'] in p.catIds]
        for gt in gts:
            gt['ignore'] = gt['ignore'] if 'ignore' in gt else 0
            gt['ignore'] = 'iscrowd' in gt and gt['iscrowd']
        self._gts = defaultdict(list)
        self._dts = defaultdict(list)
        for gt in gts:
            self._gts[gt['image_id'], gt['category_id']].append(gt)
        for dt in dts:
            self._dts[dt['image_id'], dt['category_id']].append(dt)
        self.evalImgs = defaultdict(list)
        self.eval = {}

    def evaluate(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self._prepare()
        catIds = p.catIds
        self.ious = {(imgId, catId): self.computeIoU(imgId, catId) for imgId in p.imgIds for catId in catIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(imgId, catId, areaRng, maxDet) for catId in catIds for areaRng in p.areaRng
                         for imgId in p.imgIds]

    def computeIoU(self, imgId, catId):
        p = self.params
        gt = self._gts[imgId, catId]
        dt = self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in inds]
        if len(dt) > p.maxDets[-1]:
            dt = dt[0:p.maxDets[-1]]
        if p.iouType == 'segm':
            g = [g['mask'] for g in gt]
            d = [d['mask'] for d in dt]
        else:
            g = [g['bbox'] for g in gt]
            d = [d['bbox'] for d in dt]
        iscrowd = [int(o['iscrowd']) for o in gt]
        if len(d) == 0 or len(g) == 0:                          # (pycocotools.mask.iou returns [] for an empty side)
            return []
        return maskIou(d, g, iscrowd) if p.iouType == 'segm' else bbIou(d, g, iscrowd)

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        p = self.params
        gt = self._gts[imgId, catId]
        dt = self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            if g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1]):
                g['_ignore'] = 1
            else:
                g['_ignore'] = 0
        # sort dt highest score first, sort gt ignore last
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        ious = self.ious[imgId, catId][:, gtind] if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T = len(p.iouThrs)
        G = len(gt)
        D = len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gtIg = np.array([g['_ignore'] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(p.iouThrs):
                for dind, d in enumerate(dt):
                    # information about best match so far (m=-1 -> unmatched)
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        # if this gt already matched, and not a crowd, continue
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        # if dt matched to reg gt, and on ignore gt, stop
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        # continue to next gt unless better match made
                        if ious[dind, gind] < iou:
                            continue
                        # if match successful and best so far, store appropriately
                        iou = ious[dind, gind]
                        m = gind
                    # if match made store id of match for both dt and gt
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        # set unmatched detections outside of area range to ignore
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {'image_id': imgId, 'category_id': catId, 'aRng': aRng, 'maxDet': maxDet, 'dtIds': [d['id'] for d in dt],
                'gtIds': [g['id'] for g in gt], 'dtMatches': dtm, 'gtMatches': gtm, 'dtScores': [d['score'] for d in dt],
                'gtIgnore': gtIg, 'dtIgnore': dtIg}

    def accumulate(self):
        p = self.params
        T = len(p.iouThrs)
        R = len(p.recThrs)
        K = len(p.catIds)
        A = len(p.areaRng)
        M = len(p.maxDets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        I0 = len(p.imgIds)
        A0 = len(p.areaRng)
        for k in range(K):
            Nk = k * A0 * I0
            for a in range(A):
                Na = a * I0
                for m, maxDet in enumerate(p.maxDets):
                    E = [self.evalImgs[Nk + Na + i] for i in range(I0)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                    # different sorting method generates slightly different results.
                    # mergesort is used to be consistent as Matlab implementation.
                    inds = np.argsort(-dtScores, kind='mergesort')
                    dtScoresSorted = dtScores[inds]
                    dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e['gtIgnore'] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp = np.array(tp)
                        fp = np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,))
                        ss = np.zeros((R,))
                        if nd:
                            recall[t, k, a, m] = rc[-1]
                        else:
                            recall[t, k, a, m] = 0
                        # numpy is slow without cython optimization for accessing elements; use python array gets significant speed improvement
                        pr = pr.tolist()
                        q = q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, p.recThrs, side='left')
                        try:
                            for ri, pi in enumerate(inds):
                                q[ri] = pr[pi]
                                ss[ri] = dtScoresSorted[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
                        scores[t, :, k, a, m] = np.array(ss)
        self.eval = {'params': p, 'counts': [T, R, K, A, M], 'precision': precision, 'recall': recall, 'scores': scores}

    def summarize(self):
        """-> (stats [12], text): cocoapi prints the lines; here they are joined by newlines."""
        lines = []

        def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
            p = self.params
            iStr = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
            titleStr = 'Average Precision' if ap == 1 else 'Average Recall'
            typeStr = '(AP)' if ap == 1 else '(AR)'
            iouStr = '{:0.2f}:{:0.2f}'.format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else '{:0.2f}'.format(iouThr)
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
            if ap == 1:
                # dimension of precision: [TxRxKxAxM]
                s = self.eval['precision']
                # IoU
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, :, aind, mind]
            else:
                # dimension of recall: [TxKxAxM]
                s = self.eval['recall']
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, aind, mind]
            if len(s[s > -1]) == 0:
                mean_s = -1
            else:
                mean_s = np.mean(s[s > -1])
            lines.append(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
            return mean_s

        stats = np.zeros((12,))
        stats[0] = _summarize(1)
        stats[1] = _summarize(1, iouThr=.5, maxDets=self.params.maxDets[2])
        stats[2] = _summarize(1, iouThr=.75, maxDets=self.params.maxDets[2])
        stats[3] = _summarize(1, areaRng='small', maxDets=self.params.maxDets[2])
        stats[4] = _summarize(1, areaRng='medium', maxDets=self.params.maxDets[2])
        stats[5] = _summarize(1, areaRng='large', maxDets=self.params.maxDets[2])
        stats[6] = _summarize(0, maxDets=self.params.maxDets[0])
        stats[7] = _summarize(0, maxDets=self.params.maxDets[1])
        stats[8] = _summarize(0, maxDets=self.params.maxDets[2])
        stats[9] = _summarize(0, areaRng='small', maxDets=self.params.maxDets[2])
        stats[10] = _summarize(0, areaRng='medium', maxDets=self.params.maxDets[2])
        stats[11] = _summarize(0, areaRng='large', maxDets=self.params.maxDets[2])
        self.stats = stats
        return stats, '\n'.join(lines)


# ---- coco.py loadRes + eval.py:60-67 for a scene -------------------------------------------------------------------------------
def scene_annotations(scene, kind):
    """(gts, dts) as `COCO(ann_file)` / `loadRes` hold them for IoU type `kind`.  image_id = position in the scene, category_id =
    class index, ids from 1.  Rows whose pixel box has no area never reach the JSON (eval.py:65).  Detections carry `_row` (their
    `after_nms` row), which the protocol never reads."""
    gts, dts = [], []
    for img_id, im in enumerate(scene):
        for g in im['gts']:
            gts.append({'image_id': img_id, 'category_id': int(g['cls']), 'id': len(gts) + 1, 'bbox': [float(v) for v in g['bbox']],
                        'area': g['area'], 'iscrowd': int(g['iscrowd']), 'mask': np.asarray(g['mask'], bool)})
        for row, d in enumerate(im['dets']):
            x1, y1, x2, y2 = (int(v) for v in d['box'])
            if (y2 - y1) * (x2 - x1) > 0:
                bbox = [float(x1), float(y1), float(x2 - x1), float(y2 - y1)]
                mask = np.asarray(d['mask'], bool)
                area = bbox[2] * bbox[3] if kind == 'bbox' else int(np.count_nonzero(mask))
                dts.append({'image_id': img_id, 'category_id': int(d['cls']), 'id': len(dts) + 1, 'bbox': bbox, 'area': area,
                            'score': float(np.float32(d['score'])), 'mask': mask, 'iscrowd': 0, '_row': row})
    return gts, dts


def evaluate_scene(scene, num_classes, kinds=('bbox', 'segm')):
    """{kind: COCOevalRef after evaluate() + accumulate()} over every image of the scene and the categories 0 .. num_classes-1."""
    out = {}
    for kind in kinds:
        gts, dts = scene_annotations(scene, kind)
        e = COCOevalRef(gts, dts, kind, list(range(len(scene))), list(range(num_classes)))
        e.evaluate()
        e.accumulate()
        out[kind] = e
    return out


def scene_log(evals, scene, num_classes, max_det):
    """What the device log must hold after the scene: (cls int32 [rows], rank int32 [rows], flags uint32 [rows][8], npig int64
    [4][num_classes]) with rows = len(scene) * max_det, taken from the restatement's `evalImgs` (word type * 4 + a of a row: bit k =
    dtMatches[k] != 0, bit 16 + k = dtIgnore[k]; rank = position in `dtIds`)."""
    rows = len(scene) * max_det
    cls = np.full(rows, -1, np.int32)
    rank = np.zeros(rows, np.int32)
    flags = np.zeros((rows, 8), np.uint32)
    npig = np.zeros((4, num_classes), np.int64)
    for type_idx, kind in enumerate(('bbox', 'segm')):
        if kind not in evals:
            continue
        e = evals[kind]
        p = e.params
        row_of = {d['id']: (d['image_id'], d['_row']) for d in e.dts_in}
        I0, A0 = len(p.imgIds), len(p.areaRng)
        for k in range(num_classes):
            for a in range(A0):
                for i in range(I0):
                    ev = e.evalImgs[k * A0 * I0 + a * I0 + i]
                    if ev is None:
                        continue
                    if type_idx == 0 or 'bbox' not in evals:
                        npig[a, k] += int(np.count_nonzero(ev['gtIgnore'] == 0))
                    for r, did in enumerate(ev['dtIds']):
                        img, row = row_of[did]
                        pos = img * max_det + row
                        cls[pos], rank[pos] = k, r
                        word = 0
                        for t in range(len(p.iouThrs)):
                            word |= (1 << t) if ev['dtMatches'][t, r] != 0 else 0
                            word |= (1 << (16 + t)) if ev['dtIgnore'][t, r] else 0
                        flags[pos, type_idx * 4 + a] = word
    return cls, rank, flags, npig


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _rect_mask(h, w, x1, y1, x2, y2):
    m = np.zeros((h, w), bool)
    m[max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = True
    return m


def _det(h, w, cls, score, box):
    return {'cls': cls, 'score': np.float32(score), 'box': tuple(int(v) for v in box), 'mask': _rect_mask(h, w, *box)}


def _gt(h, w, cls, xywh, iscrowd=0, area=None):
    x, y, bw, bh = xywh
    return {'cls': cls, 'bbox': [float(x), float(y), float(bw), float(bh)], 'area': bw * bh if area is None else area,
            'iscrowd': iscrowd, 'mask': _rect_mask(h, w, x, y, x + bw, y + bh)}


def known_answer_scenes():
    """{'A' .. 'H': (scene, num_classes)}: integer rectangles whose masks are the filled boxes, so both IoU types see the same
    rationals and one derivation (tests/test_coco_eval_cpu.py) covers both."""
    S = {}
    h, w = 100, 200
    S['A'] = ([{'h': h, 'w': w,
                'gts': [_gt(h, w, 0, (0, 0, 50, 50)), _gt(h, w, 0, (100, 0, 50, 50))],
                'dets': [_det(h, w, 0, .9, (0, 0, 50, 50)), _det(h, w, 0, .8, (0, 50, 50, 100)), _det(h, w, 0, .7, (100, 0, 150, 50))]}], 1)
    S['B'] = ([{'h': h, 'w': w,
                'gts': [_gt(h, w, 0, (0, 0, 50, 50)), _gt(h, w, 0, (100, 0, 100, 100), iscrowd=1)],
                'dets': [_det(h, w, 0, .9, (0, 0, 50, 50)), _det(h, w, 0, .8, (100, 0, 150, 50)), _det(h, w, 0, .7, (150, 50, 200, 100))]}], 1)
    h, w = 10, 220
    S['C'] = ([{'h': h, 'w': w,
                'gts': [_gt(h, w, 0, (0, 0, 100, 10)), _gt(h, w, 0, (6, 0, 200, 10), iscrowd=1)],
                'dets': [_det(h, w, 0, .9, (0, 0, 60, 10))]}], 1)
    h, w = 16, 16
    S['D'] = ([{'h': h, 'w': w, 'gts': [_gt(h, w, 0, (0, 0, 10, 10))], 'dets': [_det(h, w, 0, .9, (0, 0, 10, 5))]}], 1)
    h, w = 128, 128
    S['E'] = ([{'h': h, 'w': w, 'gts': [_gt(h, w, 0, (0, 0, 32, 32))],
                'dets': [_det(h, w, 0, .95, (100, 100, 120, 120)), _det(h, w, 0, .9, (0, 0, 32, 32))]}], 1)
    h, w = 50, 720
    S['F'] = ([{'h': h, 'w': w, 'gts': [_gt(h, w, 0, (60 * i, 0, 50, 50)) for i in range(12)],
                'dets': [_det(h, w, 0, (12 - i) / 16, (60 * i, 0, 60 * i + 50, 50)) for i in range(12)]}], 1)
    h, w = 64, 128
    S['G'] = ([{'h': h, 'w': w, 'gts': [_gt(h, w, 0, (0, 0, 50, 50))], 'dets': [_det(h, w, 0, .5, (70, 0, 120, 50))]},
               {'h': h, 'w': w, 'gts': [_gt(h, w, 0, (0, 0, 50, 50))], 'dets': [_det(h, w, 0, .5, (0, 0, 50, 50))]}], 1)
    S['H'] = ([{'h': h, 'w': w, 'gts': [_gt(h, w, 0, (0, 0, 50, 50))], 'dets': [_det(h, w, 0, .9, (0, 0, 50, 50))]},
               {'h': h, 'w': w, 'gts': [_gt(h, w, 0, (0, 0, 50, 50))], 'dets': []}], 1)
    return S


RANDOM_CLASSES = 5


@functools.lru_cache(maxsize=None)
def random_sequence(seed=3):
    """6 images of 128 x 160, 5 classes, up to 12 detections and 9 gts per image; about a fifth of the gts are crowds; gt areas on
    both sides of 32^2 and 96^2; scores in eighths; a few empty pixel boxes; image 4 has no detection; class 4 has no gt.  Masks are
    rectangles with a notch, so mask IoU != box IoU and the `area` field (the mask's pixels) != w * h."""
    rng = np.random.default_rng(seed)
    h, w = 128, 160
    sizes = [(8, 30), (34, 90), (100, 128)]
    scene = []
    for img in range(6):
        gts = []
        for _ in range(int(rng.integers(5, 10))):
            lo, hi = sizes[int(rng.integers(0, 3))]
            bw, bh = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
            x, y = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
            m = _rect_mask(h, w, x, y, x + bw, y + bh)
            m[y:y + bh // 4, x:x + bw // 4] = False
            gts.append({'cls': int(rng.integers(0, 4)), 'bbox': [float(x), float(y), float(bw), float(bh)], 'area': int(m.sum()),
                        'iscrowd': int(rng.random() < 0.2), 'mask': m})
        dets = []
        for _ in range(0 if img == 4 else int(rng.integers(8, 13))):
            if rng.random() < 0.8:
                g = gts[int(rng.integers(0, len(gts)))]
                x, y, bw, bh = (int(v) for v in g['bbox'])
                j = rng.integers(-4, 5, 4)
                x1, y1 = min(max(x + j[0], 0), w - 2), min(max(y + j[1], 0), h - 2)
                x2, y2 = min(max(x + bw + j[2], x1 + 1), w), min(max(y + bh + j[3], y1 + 1), h)
                cls = g['cls'] if rng.random() < 0.85 else int(rng.integers(0, 5))
            else:
                x1, y1 = int(rng.integers(0, w - 20)), int(rng.integers(0, h - 20))
                x2, y2 = x1 + int(rng.integers(4, 20)), y1 + int(rng.integers(4, 20))
                cls = int(rng.integers(0, 5))
            if rng.random() < 0.08:
                x2 = x1                                          # an empty pixel box: no detection (eval.py:65)
            m = _rect_mask(h, w, x1, y1, x2, y2)
            m[y2 - (y2 - y1) // 5:y2, x2 - (x2 - x1) // 5:x2] = False
            dets.append({'cls': cls, 'score': np.float32(int(rng.integers(1, 9)) / 8), 'box': (x1, y1, x2, y2), 'mask': m})
        dets.sort(key=lambda d: -float(d['score']))              # after_nms' rows: score descending (stable)
        scene.append({'h': h, 'w': w, 'gts': gts, 'dets': dets})
    return scene


def random_sequence_situations(scene):
    """The situations the random sequence is there for, as booleans (the tests assert every one)."""
    gts = [g for im in scene for g in im['gts']]
    dets = [d for im in scene for d in im['dets']]
    areas = [g['area'] for g in gts]
    crowds = sum(g['iscrowd'] for g in gts)
    per_img = [defaultdict(list) for _ in scene]
    for i, im in enumerate(scene):
        for d in im['dets']:
            per_img[i][d['cls']].append(float(d['score']))
    best = defaultdict(list)
    for i, pi in enumerate(per_img):
        for c, sc in pi.items():
            best[c, max(sc)].append(i)
    return {
        'crowds about a fifth': 0.1 <= crowds / len(gts) <= 0.35,
        'small, medium and large gts': min(areas) < 32 ** 2 and any(32 ** 2 < a < 96 ** 2 for a in areas) and max(areas) > 96 ** 2,
        'equal scores inside an image and class': any(len(sc) != len(set(sc)) for pi in per_img for sc in pi.values()),
        'equal scores across images in a class': any(len(v) > 1 for v in best.values()),
        'empty pixel boxes': sum((d['box'][2] - d['box'][0]) * (d['box'][3] - d['box'][1]) <= 0 for d in dets) >= 2,
        'an image without detections': any(len(im['dets']) == 0 and len(im['gts']) > 0 for im in scene),
        'a category without gt': any(d['cls'] == 4 for d in dets) and all(g['cls'] != 4 for g in gts),
        'up to 12 detections and 9 gts': max(len(im['dets']) for im in scene) <= 12 and max(len(im['gts']) for im in scene) <= 9,
    }


def many_rows_scene(n_img=12, n_det=100):
    """`n_img` images of 16 x 16 with `n_det` detections of ONE class each (more rows than one accumulate pass holds): 3 gts per
    image, detections = a gt moved by 0 / 1 pixel, scores from 16 values."""
    rng = np.random.default_rng(11)
    h = w = 16
    scene = []
    for _ in range(n_img):
        gts = [_gt(h, w, 0, (int(rng.integers(0, 6)), int(rng.integers(0, 6)), 9, 9), iscrowd=int(q == 2)) for q in range(3)]
        dets = []
        for _ in range(n_det):
            x, y = (int(v) for v in gts[int(rng.integers(0, 3))]['bbox'][:2])
            dx, dy = (int(v) for v in rng.integers(0, 2, 2))
            dets.append(_det(h, w, 0, (int(rng.integers(0, 16)) + 0.5) / 16, (x + dx, y + dy, min(x + dx + 9, w), min(y + dy + 9, h))))
        dets.sort(key=lambda d: -float(d['score']))
        scene.append({'h': h, 'w': w, 'gts': gts, 'dets': dets})
    return scene


# ---- scenes as the package's inputs (torch: the GPU tests only) -----------------------------------------------------------------
def image_to_device(im, device, max_det, packed=True, pad=True):
    """One scene image -> `DeviceCOCOeval.add`'s arguments (ids, scores, boxes_px, masks, counts, gt).  With `pad` the rows are
    padded to `max_det` with class 0, a NaN score, a full box and all-ones masks past the count, like `after_nms_batch(sync=False)`."""
    import torch
    from yolact_minimal_amd.utils.coco_eval import COCOGt
    from yolact_minimal_amd.utils.packed_masks import PackedMasks
    h, w, dets, gts = im['h'], im['w'], im['dets'], im['gts']
    g = len(gts)
    gt = COCOGt.from_arrays(np.array([q['cls'] for q in gts], np.int32), np.array([q['iscrowd'] for q in gts], np.uint8),
                            np.array([q['area'] for q in gts], np.float64), np.array([q['bbox'] for q in gts], np.float64).reshape(g, 4),
                            torch.from_numpy(np.stack([q['mask'] for q in gts]).astype(np.uint8) if g else np.zeros((0, h, w), np.uint8)),
                            h, w, device)
    n = len(dets)
    if n == 0:
        return None, None, None, None, None, gt
    rows = max_det if pad else n
    ids = np.zeros(rows, np.int64)
    scores = np.full(rows, np.nan, np.float32)
    boxes = np.tile(np.array([0, 0, w, h], np.int32), (rows, 1))
    masks = np.ones((rows, h, w), np.float32)
    ids[:n] = [d['cls'] for d in dets]
    scores[:n] = [d['score'] for d in dets]
    boxes[:n] = [d['box'] for d in dets]
    masks[:n] = np.stack([d['mask'] for d in dets])
    t = [torch.from_numpy(a).to(device) for a in (ids, scores, boxes, masks)]
    if packed:
        t[3] = PackedMasks.pack(t[3])
    counts = torch.tensor([n], dtype=torch.int32).to(device) if pad else None
    return t[0], t[1], t[2], t[3], counts, gt


def mask_to_counts(mask):
    """Uncompressed COCO RLE counts of a boolean mask: column-major run lengths, starting with the zeros run."""
    flat = np.asarray(mask, bool).reshape(-1, order='F')
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    runs = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return ([0] if flat.size and flat[0] else []) + runs


def scene_annotation_dict(scene, image_ids, cat_ids):
    """The scene's ground truth as an annotation file's dict: image i has id `image_ids[i]`, class c is category `cat_ids[c]`,
    segmentations are uncompressed RLE."""
    anns = []
    for img_id, im in zip(image_ids, scene):
        for g in im['gts']:
            anns.append({'id': len(anns) + 1, 'image_id': img_id, 'category_id': cat_ids[g['cls']], 'bbox': list(g['bbox']),
                         'area': g['area'], 'iscrowd': int(g['iscrowd']),
                         'segmentation': {'size': [im['h'], im['w']], 'counts': mask_to_counts(g['mask'])}})
    return {'images': [{'id': i, 'height': im['h'], 'width': im['w'], 'file_name': f'{i}.jpg'} for i, im in zip(image_ids, scene)],
            'categories': [{'id': c, 'name': f'c{c}'} for c in cat_ids], 'annotations': anns}
