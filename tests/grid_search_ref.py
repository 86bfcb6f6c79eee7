"""Shared by tests/test_grid_search.py and tests/test_gpu_grid_search.py: the oracle of the grid
search - the literal loop of the reference's tools/test_net_wsl_grid_search.py written against the
existing host functions (core/test_wsl.py::nms, the np.sort cut of box_results_with_nms_and_limit,
voc_dataset_evaluator.result_line, voc_eval.evaluate_arrays(route='host')), each pinned to
reference captures by its own tests - and the case builders.

The oracle has the three decisions a restatement can get wrong as switches (nms_ge, rounded_order,
cut_ge); with all of them True it is the reference's behaviour."""
from collections import OrderedDict

import numpy as np

import voc_eval_cases as vc

U = vc.U


# ---- the oracle -----------------------------------------------------------------------------------
def nms_strict(dets, thresh):
    """core/test_wsl.py::nms with `>` where the reference has `>=` (a WRONG restatement)."""
    dets = np.asarray(dets, np.float32)
    n = dets.shape[0]
    x1, y1, x2, y2, sc = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1 + np.float32(1)) * (y2 - y1 + np.float32(1))
    order = np.argsort(-sc, kind='stable')
    suppressed = np.zeros((n,), bool)
    thresh = np.float32(thresh)
    for _i in range(n):
        i = order[_i]
        if suppressed[i]:
            continue
        rest = order[_i + 1:]
        xx1, yy1 = np.maximum(x1[i], x1[rest]), np.maximum(y1[i], y1[rest])
        xx2, yy2 = np.minimum(x2[i], x2[rest]), np.minimum(y2[i], y2[rest])
        inter = (np.maximum(np.float32(0), xx2 - xx1 + np.float32(1)) *
                 np.maximum(np.float32(0), yy2 - yy1 + np.float32(1)))
        with np.errstate(divide='ignore', invalid='ignore'):
            ovr = inter / (areas[i] + areas[rest] - inter)
        suppressed[rest[ovr > thresh]] = True
    return np.where(~suppressed)[0].tolist()


def kept_rows(scores, boxes, nms_thresh, score_thresh, nms_ge=True):
    """{class j: kept rows, ascending} of one image: the host branch of nms_all_classes."""
    from detectron.core import test_wsl
    out = {}
    score_thresh = np.float32(score_thresh)
    for j in range(1, scores.shape[1]):
        inds = np.where(scores[:, j] > score_thresh)[0]
        dets = np.hstack((boxes[inds], scores[inds, j][:, np.newaxis])).astype(np.float32, copy=False)
        with np.errstate(divide='ignore', invalid='ignore'):
            keep = test_wsl.nms(dets, nms_thresh) if nms_ge else nms_strict(dets, nms_thresh)
        out[j] = inds[np.asarray(keep, np.int64)]
    return out


def cut_rows(scores, kept, limit, cut_ge=True):
    """The DETECTIONS_PER_IM cut of box_results_with_nms_and_limit over one image's kept rows."""
    if limit <= 0:
        return kept
    all_scores = np.hstack([scores[kept[j], j] for j in sorted(kept)])
    if len(all_scores) <= limit:
        return kept
    th = np.sort(all_scores)[-limit]
    return {j: r[(scores[r, j] >= th) if cut_ge else (scores[r, j] > th)] for j, r in kept.items()}


class Oracle(object):
    """The literal sweep over one case; the per-(nms, score) NMS results are computed once and
    shared by the limits, which changes nothing (the cut comes after the NMS)."""

    def __init__(self, recs, names, classes, candidates, use_07_metric=True):
        self.recs, self.names, self.classes = recs, names, [str(c) for c in classes]
        self.candidates, self.use_07 = candidates, use_07_metric
        self._kept, self._rows = {}, {}

    def kept(self, nms, thresh, nms_ge=True):
        key = (nms, thresh, nms_ge)
        if key not in self._kept:
            self._kept[key] = [kept_rows(s, b, nms, thresh, nms_ge) for s, b in self.candidates]
        return self._kept[key]

    def detections(self, nms, thresh, limit, nms_ge=True, cut_ge=True):
        """-> ({class: (ids, confidence, boxes)} through the result-file line, n_dets, the fp32
        scores of the lines per class)."""
        from detectron.datasets.voc_dataset_evaluator import result_line
        per_class = [([], [], [], []) for _ in self.classes]
        n_dets = 0
        for name, (scores, boxes), kept in zip(self.names, self.candidates, self.kept(nms, thresh, nms_ge)):
            rows = cut_rows(scores, kept, limit, cut_ge)
            for j in range(1, len(self.classes)):
                ids, conf, bb, raw = per_class[j]
                for r in rows[j]:
                    det = np.hstack((boxes[r], scores[r, j:j + 1])).astype(np.float32)
                    f = result_line(name, det).strip().split(' ')
                    ids.append(f[0]); conf.append(float(f[1])); bb.append([float(z) for z in f[2:]])
                    raw.append(scores[r, j])
                    n_dets += 1
        dets, raws = OrderedDict(), OrderedDict()
        for j in range(1, len(self.classes)):
            ids, conf, bb, raw = per_class[j]
            dets[self.classes[j]] = (ids, np.array(conf, np.float64), np.array(bb, np.float64).reshape(-1, 4))
            raws[self.classes[j]] = np.array(raw, np.float32)
        return dets, n_dets, raws

    def row(self, nms, thresh, limit, nms_ge=True, rounded_order=True, cut_ge=True):
        """One setting -> dict(n_dets, mAP, mCorLoc, per class: tp, fp, rec, prec, ap07, ap_area,
        corloc)."""
        from detectron.datasets import voc_eval
        key = (nms, thresh, limit, nms_ge, rounded_order, cut_ge)
        if key in self._rows:
            return self._rows[key]
        dets, n_dets, raws = self.detections(nms, thresh, limit, nms_ge, cut_ge)
        if not rounded_order:
            # the WRONG order: a stable sort by the fp32 score; strictly decreasing stand-in
            # confidences make the evaluator visit the lines in exactly that order
            for c, (ids, conf, bb) in list(dets.items()):
                o = np.argsort(-raws[c], kind='stable')
                dets[c] = ([ids[i] for i in o], -np.arange(len(o), dtype=np.float64), bb[o])
        res = voc_eval.evaluate_arrays(self.recs, self.names, dets, ovthresh=0.5,
                                       use_07_metric=self.use_07, route='host')
        aps = [r['ap'] for r in res.values()]
        out = dict(n_dets=n_dets, mAP=float(np.mean(aps)),
                   mCorLoc=float(np.mean([r['corloc'] for r in res.values()])), classes=res)
        self._rows[key] = out
        return out


def assert_row_matches(row, ref, classes, use_07_metric=True):
    """A grid_search row (curves=True) against an Oracle.row: n_dets equal; flags, rec, prec, the
    11-point AP and CorLoc bit-equal; the area AP within (D + 2) * 2^-52 - the device sums the
    reference's terms in another, fixed order (tests/test_gpu_voc_eval.py)."""
    tag = (row['nms'], row['score_thresh'], row['detections_per_im'])
    assert row['n_dets'] == ref['n_dets'], (tag, row['n_dets'], ref['n_dets'])
    got = row['curves']
    vc.assert_same_results(
        OrderedDict((c, got[c]) for c in classes[1:]),
        OrderedDict((c, ref['classes'][c]) for c in classes[1:]))
    for c in classes[1:]:
        r = ref['classes'][c]
        assert row['CorLoc_' + c] == r['corloc'], (tag, c)
        if use_07_metric:
            assert row['AP_' + c] == r['ap07'], (tag, c)
    if use_07_metric:
        assert row['mAP'] == ref['mAP'], (tag, row['mAP'], ref['mAP'])
    assert row['mCorLoc'] == ref['mCorLoc'], tag


# ---- case builders --------------------------------------------------------------------------------
def build_candidates(recs, names, classes, seed, max_boxes, width=240, height=220):
    """Seeded candidates around a set's ground truth: per image (scores fp32 [n, K], boxes fp32
    [n, 4]).  Image 0 holds max_boxes rows, image 1 none, image 2 one; boxes lie on a quarter-pixel
    grid (so '%.1f' meets ties such as x.25) and a tenth of them are exact copies of another row
    (IoU exactly 1); scores spread over 1e-11 .. 1, a third of them rounded to two digits (ties,
    also across classes of one image), below 1e-3 close enough for '%.9f' to merge neighbours."""
    rng = np.random.default_rng(seed)
    k = len(classes)
    out = []
    for i, name in enumerate(names):
        n = int(rng.integers(2, max(3, max_boxes // 3)))
        n = {0: max_boxes, 1: 0, 2: 1}.get(i, n)
        gt = [(o['bbox'], classes.index(o['name'])) for o in recs[name] if o['name'] in classes]
        boxes = np.zeros((n, 4), np.float32)
        scores = np.full((n, k), -1, np.float32)
        for r in range(n):
            near = bool(gt) and rng.random() < 0.6
            if near:
                g, gc = gt[int(rng.integers(0, len(gt)))]
                b = np.array(g, np.float64) - 1 + np.round(rng.normal(0, 4, 4) * 4) / 4
                b[2:] = np.maximum(b[2:], b[:2])
            else:
                x, y = rng.integers(0, width - 20), rng.integers(0, height - 20)
                b = np.array([x, y, x + rng.integers(4, 120), y + rng.integers(4, 120)], np.float64)
                b += np.round(rng.random(4) * 4) / 4
            if r > 0 and rng.random() < 0.1:
                b = boxes[int(rng.integers(0, r))].astype(np.float64)
            boxes[r] = b
            s = 10.0 ** rng.uniform(-11, 0, k)
            if near:
                s[gc] = 10.0 ** rng.uniform(-3, 0)
            tie = rng.random(k) < 0.33
            s = np.where(tie, np.array([float('%.1e' % v) for v in s]), s)
            scores[r, 1:] = s[1:].astype(np.float32)
        out.append((scores, boxes))
    return out


def tiny_case(seed=5, max_boxes=40):
    """The tiny devkit (12 images, bird / cat / dog) with seeded candidates."""
    names, recs = vc.tiny_annotations()
    classes = [str(c) for c in vc.fixture()['classes']]
    return recs, names, classes, build_candidates(recs, names, classes, seed, max_boxes)


def synthetic_case(seed=21, n_images=30, n_classes=3, max_boxes=300):
    recs, names, _dets = vc.synthetic_set(seed, n_images, n_classes, 1, special=False)
    classes = ['__background__'] + ['c%d' % i for i in range(n_classes)]
    return recs, names, classes, build_candidates(recs, names, classes, seed, max_boxes, 520, 520)


def _one_class(objs_per_image):
    names = ['%06d' % (i + 1) for i in range(len(objs_per_image))]
    recs = {n: [{'name': 'c0', 'pose': 'Unspecified', 'truncated': 0, 'difficult': 0, 'bbox': list(b)}
                for b in boxes] for n, boxes in zip(names, objs_per_image)}
    return recs, names, ['__background__', 'c0']


def _cand(boxes, scores):
    b = np.array(boxes, np.float32).reshape(-1, 4)
    s = np.full((b.shape[0], 2), -1, np.float32)
    s[:, 1] = np.array(scores, np.float32)
    return s, b


def case_nms_on_threshold():
    """(0,0,9,14) / (0,5,9,19): areas 150 and 150, intersection 100, IoU 100 / 200 = 0.5 exactly.
    At TEST.NMS 0.5 the second box goes (`>=`); it is the one that sits on the ground truth, so a
    `>` restatement keeps a true positive more."""
    recs, names, classes = _one_class([[(1, 6, 10, 20)]])
    return recs, names, classes, [_cand([(0, 0, 9, 14), (0, 5, 9, 19)], [0.9, 0.8])], (0.5, 1e-3, 0)


def case_rounded_confidence_tie():
    """Two detections of two images whose fp32 scores differ but print as the same '%.9f': the
    file-first one (image 1, a true positive) has the LOWER score.  Sorted by the rounded
    confidence it stays first: prec = [1, 0.5]; sorted by the fp32 score the false positive of
    image 2 comes first: prec = [0, 0.5]."""
    lo = np.float32(0.0010000001)
    hi = np.nextafter(np.nextafter(lo, np.float32(1)), np.float32(1))
    assert lo < hi and '%.9f' % lo == '%.9f' % hi
    recs, names, classes = _one_class([[(11, 11, 51, 51)], [(11, 11, 51, 51)]])
    cands = [_cand([(10, 10, 50, 50)], [lo]), _cand([(100, 100, 150, 150)], [hi])]
    return recs, names, classes, cands, (0.5, 1e-9, 0)


def case_tie_across_the_cut():
    """Three disjoint boxes, the two lower scores equal, limit 2: np.sort(...)[-2] is the tied
    score and `>=` keeps all three; `> th` keeps one."""
    recs, names, classes = _one_class([[(1, 1, 21, 21)]])
    cands = [_cand([(0, 0, 20, 20), (40, 40, 60, 60), (80, 80, 100, 100)], [0.9, 0.5, 0.5])]
    return recs, names, classes, cands, (0.5, 1e-3, 2)


# ---- the design of the device route, restated in numpy --------------------------------------------
def nms_words(boxes, thresholds):
    """naws_nms_multi_fwd for one list (boxes fp32 [n, 4] in visiting order): bit t of word j = box
    j survives at thresholds[t].  One IoU per pair, a T-bit `suppressed` word per box."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    thr = np.asarray(thresholds, np.float32)
    n, t = b.shape[0], len(thr)
    full = (1 << t) - 1
    supp = np.zeros(n, np.int64)
    areas = (b[:, 2] - b[:, 0] + np.float32(1)) * (b[:, 3] - b[:, 1] + np.float32(1))
    for i in range(n):
        alive = ~supp[i] & full
        if alive == 0:
            continue
        r = slice(i + 1, n)
        xx1, yy1 = np.maximum(b[i, 0], b[r, 0]), np.maximum(b[i, 1], b[r, 1])
        xx2, yy2 = np.minimum(b[i, 2], b[r, 2]), np.minimum(b[i, 3], b[r, 3])
        inter = (np.maximum(np.float32(0), xx2 - xx1 + np.float32(1)) *
                 np.maximum(np.float32(0), yy2 - yy1 + np.float32(1)))
        with np.errstate(divide='ignore', invalid='ignore'):
            ovr = inter / (areas[i] + areas[r] - inter)
        m = np.zeros(n - i - 1, np.int64)
        for q in range(t):
            m |= (ovr >= thr[q]).astype(np.int64) << q
        supp[r] |= m & alive
    return (~supp & full).astype(np.uint32)


def cut_tables(words, scores, num_nms, score_thresholds, limits):
    """naws_grid_cut_fwd for one image (its candidates in descending score) -> (count [T, S],
    kth [T, Lc]; -inf when fewer survive or the limit is 0)."""
    words, scores = np.asarray(words, np.int64), np.asarray(scores, np.float32)
    sthr = np.asarray(score_thresholds, np.float32)
    count = np.zeros((num_nms, len(sthr)), np.int32)
    kth = np.full((num_nms, len(limits)), -np.inf, np.float32)
    for t in range(num_nms):
        sv = scores[((words >> t) & 1) == 1]
        for s, th in enumerate(sthr):
            count[t, s] = int((sv > th).sum())
        for l, lim in enumerate(limits):
            if 0 < lim <= len(sv):
                kth[t, l] = sv[lim - 1]
    return count, kth


def design_rows(recs, names, classes, candidates, nmses, threshs, limits, use_07_metric=True):
    """The device route's design end to end in numpy: one NMS pass per list for all thresholds on
    the list cut at the smallest score threshold, the cut from (count, kth), a setting = a mask
    over ONE evaluation order.  -> {(nms, thresh, limit): (dets in evaluate_arrays' form, already
    in evaluation order, n_dets)}."""
    from detectron.core import grid_search_wsl as gs
    k = len(classes)
    sthr = np.asarray(threshs, np.float32)
    p = gs.prepare_candidates(candidates, k, sthr.min())
    n = len(p['score'])
    off = p['list_off']
    words = np.zeros(n, np.uint32)
    for a, b in zip(off[:-1], off[1:]):
        words[a:b] = nms_words(p['box'][a:b], nmses)
    count = np.zeros((len(names), len(nmses), len(threshs)), np.int32)
    kth = np.zeros((len(names), len(nmses), len(limits)), np.float32)
    for i in range(len(names)):
        idx = np.flatnonzero(p['img'] == i)
        idx = idx[np.argsort(-p['score'][idx], kind='stable')]
        count[i], kth[i] = cut_tables(words[idx], p['score'][idx], len(nmses), sthr, limits)
    e = np.lexsort((p['row'], p['img'], -p['conf'], p['cls']))      # last key first
    out = {}
    for t, nms in enumerate(nmses):
        for s, th in enumerate(threshs):
            for l, lim in enumerate(limits):
                sel = (((words >> t) & 1) == 1) & (p['score'] > sthr[s])
                if lim > 0:
                    sel &= (count[p['img'], t, s] <= lim) | (p['score'] >= kth[p['img'], t, l])
                pick = e[sel[e]]
                dets = OrderedDict()
                for j in range(1, k):
                    q = pick[p['cls'][pick] == j - 1]
                    dets[classes[j]] = ([names[i] for i in p['img'][q]], p['conf'][q], p['bb'][q])
                out[(nms, th, lim)] = (dets, int(sel.sum()))
    return out
