"""Test-time grid search over TEST.NMS x TEST.SCORE_THRESH x TEST.DETECTIONS_PER_IM (reference:
tools/test_net_wsl_grid_search.py, grid_search() :109-192): every setting is what
box_results_with_nms_and_limit and the VOC evaluation would give on the unsuppressed detections
of one test run.  Two routes, the same numbers:

  host    the literal loop: set the three cfg keys (and NAWS.HOST_NMS), run
          box_results_with_nms_and_limit per image, take the numbers a result file would hold,
          evaluate on the host.  Nothing is written per setting.
  device  the work a setting shares with the others is done once (csrc/grid_ops.hip):
            1. greedy NMS keeps a box or not by the boxes visited before it, so the survivors at
               score threshold s are the survivors of the list cut at the SMALLEST threshold of
               the grid, filtered by score > s: NMS runs once per NMS threshold;
            2. and all NMS thresholds share one pass (naws_nms_multi_fwd: a T-bit word per box);
            3. the image-wide cut keeps score >= the L-th best surviving score when more than L
               survive; that score does not depend on s, only the count does (naws_grid_cut_fwd):
               selected = bit_t and score > s and (L == 0 or count[img, t, s] <= L or
                          score >= kth[img, t, L]);
            4. the evaluated numbers - float('%.9f' % score), float('%.1f' % (x + 1)) - and the
               evaluation order (class, descending ROUNDED confidence, then file order = image,
               row) are fixed per candidate: a setting selects a subsequence of one order, so no
               setting sorts.  Several settings are matched and scored per launch pair
               (naws_voc_match_fwd / naws_voc_ap_fwd take any number of segments and classes).
          torch is the plumbing: sorts once, masks, prefix sums, gathers.

Thresholds are rounded to fp32 once, as both NMS routes of core/test_wsl.py do.  Without box
regression every class holds the same boxes: that is the only form this path has."""
import logging
import time
from collections import OrderedDict
from contextlib import contextmanager

import numpy as np

from detectron.core.config import cfg
from detectron.datasets import voc_eval
from detectron.datasets.voc_dataset_evaluator import result_line, voc_info

logger = logging.getLogger(__name__)

# the reference's lists (tools/test_net_wsl_grid_search.py:153-155)
DEFAULT_NMSES = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.0)
DEFAULT_THRESHS = (1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)
DEFAULT_LIMITS = (10000, 1000, 100, 10, 1)
# what a collection run is tested with: nothing suppressed, nothing cut (the reference has this
# commented out, :217-227)
COLLECT_OPTS = ('TEST.NMS', 1.1, 'TEST.SCORE_THRESH', -1e10, 'TEST.DETECTIONS_PER_IM', 0)
_REFUSED_KEYS = ('TEST.SOFT_NMS.ENABLED', 'TEST.BBOX_VOTE.ENABLED', 'TEST.BBOX_REG')
MAX_NMS_THRESHOLDS = 32                  # naws_nms_multi_fwd's word
_CHUNK_ELEMS = 1 << 27                   # settings per evaluation chunk x candidates, at most


# ---- the numbers a result file holds --------------------------------------------------------------
def round_confidence(score):
    """float('{:.9f}'.format(s)) for every fp32 score s, as float64.  Exact, not a
    multiply-and-round: s = M * 2^-k with an integer M < 2^24, so M * 10^9 < 2^54 is an exact
    int64, its shift by k with round-half-even is the correctly rounded integer q that the format
    prints, and q / 1e9 (one correctly rounded division of two exact doubles) is the double that
    float() parses from 'q * 10^-9'.  Values of 2^20 and above, NaN and inf go through the format
    itself."""
    s = np.asarray(score, np.float32)
    x = s.astype(np.float64)
    a = np.abs(x)
    fast = np.isfinite(x) & (a < 2.0 ** 20)
    m, e = np.frexp(np.where(fast, a, 0.0))
    big = np.ldexp(m, 24).astype(np.int64) * np.int64(1000000000)        # a * 2^k * 10^9, exact
    k = 24 - e.astype(np.int64)                                          # >= 4 on the fast path
    kk = np.clip(k, 1, 62)
    one = np.int64(1)
    q = big >> kk
    r = big & ((one << kk) - one)
    half = one << (kk - one)
    q = q + ((r > half) | ((r == half) & ((q & one) == one)))
    q = np.where(k > 62, 0, q)                                           # below 2^-9 of a unit
    out = np.copysign(q.astype(np.float64) / 1e9, x)
    if not fast.all():
        flat, idx = out.reshape(-1), np.flatnonzero(~fast.reshape(-1))
        src = x.reshape(-1)
        for i in idx:
            flat[i] = float('{:.9f}'.format(float(src[i])))
        out = flat.reshape(x.shape)
    return out


def round_coordinate(x):
    """float('{:.1f}'.format(x + 1)) for every fp32 coordinate, x + 1 in fp32 as result_line gets
    it, as float64.  v * 10 is exact in double for an fp32 v (28 significant bits), np.rint rounds
    half to even as the format does, and q / 10 is the double float() parses."""
    v = (np.asarray(x, np.float32) + np.float32(1)).astype(np.float64)
    return np.rint(v * 10.0) / 10.0


# ---- candidates -----------------------------------------------------------------------------------
def candidates_from_detections(all_boxes):
    """The unsuppressed detections of a collection run, all_boxes[cls][image] = [n, 5], back into
    per-image (scores fp32 [n, K], boxes fp32 [n, 4]) - the reference's reconstruction
    (grid_search() :128-149; column 0, the background, stays -1).  Every class of an image must
    hold the same rows: a run whose NMS, score threshold or per-image limit removed something is
    refused."""
    num_classes = len(all_boxes)
    if num_classes < 2:
        raise ValueError('grid search: all_boxes holds no foreground class')
    num_images = len(all_boxes[1])
    out = []
    for i in range(num_images):
        first = np.asarray(all_boxes[1][i], np.float32).reshape(-1, 5)
        n = first.shape[0]
        scores = np.full((n, num_classes), -1, np.float32)
        for j in range(1, num_classes):
            if len(all_boxes[j]) != num_images:
                raise ValueError('grid search: class {} holds {} images, class 1 holds {}'.format(
                    j, len(all_boxes[j]), num_images))
            d = np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5)
            if d.shape[0] != n or not np.array_equal(d[:, :4], first[:, :4]):
                raise ValueError(
                    'grid search: image {} holds different rows for class {} and class 1 ({} and {}): '
                    'the detections are not those of a collection run (TEST.NMS 1.1, '
                    'TEST.SCORE_THRESH -1e10, TEST.DETECTIONS_PER_IM 0)'.format(i, j, d.shape[0], n))
            scores[:, j] = d[:, 4]
        out.append((scores, np.ascontiguousarray(first[:, :4])))
    return out


def check_cfg():
    """The sweep restates the greedy, class-agnostic-box path only."""
    for key in _REFUSED_KEYS:
        node = cfg
        for part in key.split('.'):
            node = node[part]
        if node:
            raise NotImplementedError('grid search: {} True is not part of the sweep'.format(key))


def device_route_available():
    """cfg.NAWS.DEVICE_EVAL and a GPU, as the evaluator decides."""
    return voc_eval.device_route_available()


def settings_of(nmses, threshs, limits):
    """The reference's loop order: NMS outer, score threshold, limit inner."""
    return [(a, b, c) for a in nmses for b in threshs for c in limits]


# ---- the host route: the literal loop -------------------------------------------------------------
@contextmanager
def _cfg_keys(num_classes):
    """The cfg keys of one sweep, put back afterwards."""
    frozen = cfg.is_immutable()
    saved = (cfg.TEST.NMS, cfg.TEST.SCORE_THRESH, cfg.TEST.DETECTIONS_PER_IM, cfg.NAWS.HOST_NMS,
             cfg.MODEL.NUM_CLASSES)
    cfg.immutable(False)
    cfg.NAWS.HOST_NMS = True
    cfg.MODEL.NUM_CLASSES = num_classes
    try:
        yield
    finally:
        cfg.immutable(False)
        (cfg.TEST.NMS, cfg.TEST.SCORE_THRESH, cfg.TEST.DETECTIONS_PER_IM, cfg.NAWS.HOST_NMS,
         cfg.MODEL.NUM_CLASSES) = saved
        cfg.immutable(frozen)


def _host_detections(imagenames, classes, candidates):
    """One setting (the cfg holds it): box_results_with_nms_and_limit per image, then the round
    trip through the result-file line.  -> ({class: (ids, confidence, boxes)}, n_dets)."""
    from detectron.core.test_wsl import box_results_with_nms_and_limit
    per_class = [([], [], []) for _ in classes]
    n_dets = 0
    for name, (scores, boxes) in zip(imagenames, candidates):
        _s, _b, cls_boxes = box_results_with_nms_and_limit(scores, boxes)
        for j in range(1, len(classes)):
            ids, conf, bb = per_class[j]
            for det in cls_boxes[j]:
                f = result_line(name, det).strip().split(' ')
                ids.append(f[0])
                conf.append(float(f[1]))
                bb.append([float(z) for z in f[2:]])
                n_dets += 1
    dets = OrderedDict()
    for j in range(1, len(classes)):
        ids, conf, bb = per_class[j]
        dets[classes[j]] = (ids, np.array(conf, np.float64), np.array(bb, np.float64).reshape(-1, 4))
    return dets, n_dets


def _row(setting, n_dets, classes, res, use_07_metric, curves):
    aps = [r['ap07'] if use_07_metric else r['ap_area'] for r in res]
    corlocs = [r['corloc'] for r in res]
    mean = lambda v: float(np.mean(v)) if len(v) else 0.0
    row = OrderedDict([('nms', setting[0]), ('score_thresh', setting[1]),
                       ('detections_per_im', setting[2]), ('n_dets', int(n_dets)),
                       ('mAP', mean(aps)), ('mCorLoc', mean(corlocs))])
    for c, v in zip(classes[1:], aps):
        row['AP_' + c] = float(v)
    for c, v in zip(classes[1:], corlocs):
        row['CorLoc_' + c] = float(v)
    if curves:
        row['curves'] = OrderedDict(
            (c, {k: r[k] for k in ('tp', 'fp', 'rec', 'prec', 'ap07', 'ap_area', 'corloc')})
            for c, r in zip(classes[1:], res))
    return row


def _grid_host(recs, imagenames, classes, candidates, settings, use_07_metric, curves):
    rows = []
    with _cfg_keys(len(classes)):
        for setting in settings:
            cfg.TEST.NMS, cfg.TEST.SCORE_THRESH, cfg.TEST.DETECTIONS_PER_IM = setting
            dets, n_dets = _host_detections(imagenames, classes, candidates)
            res = voc_eval.evaluate_arrays(recs, imagenames, dets, ovthresh=0.5,
                                           use_07_metric=use_07_metric, route='host')
            rows.append(_row(setting, n_dets, classes, list(res.values()), use_07_metric, curves))
    return rows


# ---- the device route -----------------------------------------------------------------------------
def prepare_candidates(candidates, num_classes, s_min):
    """Host work, once per sweep: every (image, class, row) with score > s_min (fp32), image-major,
    class-major inside an image, inside an (image, class) list in NMS visiting order
    (np.argsort(-score, kind='stable'), core/test_wsl.py::nms).  -> dict of numpy arrays: img, cls
    (0-based foreground index), row int64 [N]; score fp32 [N]; box fp32 [N, 4]; conf, bb float64
    (the rounded numbers); list_off int64 [I * C + 1]."""
    c = num_classes - 1
    img, cls, row, score, box, bb, counts = [], [], [], [], [], [], []
    s_min = np.float32(s_min)
    for i, (scores, boxes) in enumerate(candidates):
        sc = np.asarray(scores, np.float32)[:, 1:num_classes]
        bx = np.asarray(boxes, np.float32)
        if bx.shape[1] > 4:                       # class-tiled copies of one box set
            assert np.array_equal(bx[:, 4:8], bx[:, -4:])
            bx = bx[:, 4:8]
        # only the live scores are sorted: class-major, inside a class by descending score, equal
        # scores by ascending row (np.nonzero lists the rows in ascending order and np.lexsort is
        # stable) - np.argsort(-score, kind='stable') of the class's rows above the threshold
        cls_i, rows_i = np.nonzero((sc > s_min).T)
        live = sc[rows_i, cls_i]
        o = np.lexsort((-live, cls_i))
        cls_i, rows_i, live = cls_i[o], rows_i[o], live[o]
        counts.append(np.bincount(cls_i, minlength=c))
        img.append(np.full(rows_i.shape, i, np.int64))
        cls.append(cls_i.astype(np.int64))
        row.append(rows_i.astype(np.int64))
        score.append(live)
        box.append(bx[rows_i])
        bb.append(round_coordinate(bx)[rows_i])
    cat = lambda v, dt, tail=(): (np.concatenate(v) if v else np.zeros((0,) + tail, dt)).astype(dt, copy=False)
    out = dict(img=cat(img, np.int64), cls=cat(cls, np.int64), row=cat(row, np.int64),
               score=cat(score, np.float32), box=cat(box, np.float32, (4,)).reshape(-1, 4),
               bb=cat(bb, np.float64, (4,)).reshape(-1, 4))
    out['conf'] = round_confidence(out['score'])
    off = np.zeros(len(candidates) * c + 1, np.int64)
    if counts:
        np.cumsum(np.concatenate(counts), out=off[1:])
    out['list_off'] = off
    return out


class _Stages(object):
    """Wall seconds (device idle at both ends) and device-event milliseconds per stage, when a
    timings dict is asked for; nothing otherwise."""

    def __init__(self, timings):
        self.t = timings

    @contextmanager
    def stage(self, name):
        if self.t is None:
            yield
            return
        import torch
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        try:
            yield
        finally:
            b.record()
            torch.cuda.synchronize()
            self.t[name + '_wall_s'] = self.t.get(name + '_wall_s', 0.0) + time.perf_counter() - t0
            self.t[name + '_device_ms'] = self.t.get(name + '_device_ms', 0.0) + a.elapsed_time(b)


def _gt_device(gts, n, dev):
    """The ground truth of every (class, image) pair, class-major, on the device."""
    import torch
    k = len(gts)
    counts = np.array([[len(dif) for _b, dif in per_image] for per_image, _p, _q in gts], np.int64)
    gt_off = np.zeros(k * n + 1, np.int64)
    np.cumsum(counts.reshape(-1), out=gt_off[1:])
    boxes = [b for per_image, _p, _q in gts for b, _d in per_image if len(b)]
    diffs = [dif for per_image, _p, _q in gts for _b, dif in per_image if len(dif)]
    gt_all = np.concatenate(boxes) if boxes else np.zeros((0, 4))
    dif_all = np.concatenate(diffs).astype(np.uint8) if diffs else np.zeros(0, np.uint8)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    return up(gt_off, np.int64), up(gt_all, np.float64), up(dif_all, np.uint8)


def _grid_device(recs, imagenames, classes, candidates, nmses, threshs, limits, use_07_metric, curves,
                 timings, device='cuda'):
    import torch
    from naws_hip import ops
    dev = torch.device(device)
    st = _Stages(timings)
    k, c, n_img = len(classes), len(classes) - 1, len(imagenames)
    if len(nmses) > MAX_NMS_THRESHOLDS:
        raise NotImplementedError('grid search: at most {} NMS thresholds per sweep'.format(
            MAX_NMS_THRESHOLDS))
    nms_thr = np.asarray(nmses, np.float32)
    sthr = np.asarray(threshs, np.float32)
    lims = np.asarray(limits, np.int64)
    if (lims >= 2 ** 31).any() or (lims < 0).any():
        raise ValueError('grid search: a per-image limit must lie in [0, 2^31)')
    t0 = time.perf_counter()
    prep = prepare_candidates(candidates, k, sthr.min())
    gts = voc_eval.ground_truth_tables(recs, imagenames, classes[1:])
    if timings is not None:
        timings['prep_host_s'] = time.perf_counter() - t0
    n = int(prep['score'].shape[0])
    settings = settings_of(range(len(nmses)), range(len(threshs)), range(len(limits)))
    i64 = torch.int64

    with st.stage('order'):
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        img, cls, score = up(prep['img'], np.int64), up(prep['cls'], np.int64), up(prep['score'], np.float32)
        conf, box = up(prep['conf'], np.float64), up(prep['box'], np.float32)
        list_off = up(prep['list_off'], np.int64)
        gt_off_d, gt_d, dif_d = _gt_device(gts, n_img, dev)
        npos = up([p for _g, p, _q in gts], np.int64)
        # an image's candidates of all classes in descending score (the cut's scan order)
        o1 = torch.sort(score, descending=True, stable=True).indices
        by_img = o1[torch.sort(img[o1], stable=True).indices]
        img_off = torch.zeros(n_img + 1, dtype=i64, device=dev)
        img_off[1:] = torch.cumsum(torch.bincount(img, minlength=n_img), 0)
        # the evaluation order E: class, descending ROUNDED confidence, then file order
        rows_max = int(prep['row'].max()) + 1 if n else 1
        p = torch.sort(img * rows_max + up(prep['row'], np.int64), stable=True).indices
        p = p[torch.sort(conf[p], descending=True, stable=True).indices]
        e_ord = p[torch.sort(cls[p], stable=True).indices]
        cls_e, img_e, score_e = cls[e_ord], img[e_ord], score[e_ord]
        bb_e = up(prep['bb'], np.float64)[e_ord]
        # E regrouped by (class, image), stably: the matching kernel's segments
        g_pos = torch.sort(cls_e * n_img + img_e, stable=True).indices
    with st.stage('nms'):
        survive, status = ops.nms_multi(box, list_off, nms_thr)
    if n and bool((status != 0).any()):
        raise RuntimeError('grid search: a candidate list was refused (status {})'.format(
            int(status[status != 0][0])))
    with st.stage('cut'):
        count, kth, status = ops.grid_cut(survive[by_img].contiguous(), score[by_img].contiguous(),
                                          img_off, len(nmses), sthr, lims.astype(np.int32))
    if bool((status != 0).any()):
        raise RuntimeError('grid search: inconsistent image offsets')
    surv_e = survive[e_ord]
    sthr_d = up(sthr, np.float32)

    q_max = max(1, min(65535 // max(c, 1), _CHUNK_ELEMS // max(n, 1), 64))
    rows = []
    for lo in range(0, len(settings), q_max):
        chunk = settings[lo:lo + q_max]
        q = len(chunk)
        with st.stage('select'):
            masks, base_key, base = [], None, None
            for t, s, l in chunk:
                if base_key != (t, s):
                    base = (((surv_e >> t) & 1) != 0) & (score_e > sthr_d[s])
                    base_key = (t, s)
                m = base
                if lims[l] > 0:
                    m = base & ((count[:, t, s][img_e] <= int(lims[l])) | (score_e >= kth[:, t, l][img_e]))
                masks.append(m)
            sel_e = torch.stack(masks) if n else torch.zeros((q, 0), dtype=torch.bool, device=dev)
            n_dets = sel_e.sum(1)
            d_all = int(n_dets.sum())
        if d_all == 0:
            e = np.zeros(0)
            for j, (t, s, l) in enumerate(chunk):
                res = [dict(tp=e, fp=e, rec=e, prec=e, ap07=0.0, ap_area=0.0, corloc=0.0) for _ in range(c)]
                rows.append(_row((nmses[t], threshs[s], limits[l]), 0, classes, res, use_07_metric, curves))
            continue
        with st.stage('eval'):
            # position of every selected candidate in the chunk's detections, E order: setting-major,
            # inside a setting class-major in descending confidence
            rank_e = torch.cumsum(sel_e.reshape(-1).to(i64), 0) - 1
            gq, gg = sel_e[:, g_pos].nonzero(as_tuple=True)       # the same detections, segment-major
            e_idx = g_pos[gg]
            dest = rank_e[gq * n + e_idx]
            sup_cls = gq * c + cls_e[e_idx]                        # a (setting, class) pair = a "class"
            seg_key, seg_len = torch.unique_consecutive(sup_cls * n_img + img_e[e_idx], return_counts=True)
            s_cnt = seg_key.numel()
            det_off = torch.zeros(s_cnt + 1, dtype=i64, device=dev)
            det_off[1:] = torch.cumsum(seg_len, 0)
            pair = seg_key % (c * n_img)
            g_begin = gt_off_d[pair]
            g_len = gt_off_d[pair + 1] - g_begin
            seg_gt_off = torch.zeros(s_cnt + 1, dtype=i64, device=dev)
            seg_gt_off[1:] = torch.cumsum(g_len, 0)
            g_seg = int(seg_gt_off[-1])
            g_rows = torch.arange(g_seg, device=dev) + torch.repeat_interleave(
                g_begin - seg_gt_off[:-1], g_len, output_size=g_seg)
            tp_s, fp_s, code, _taken = ops.voc_match(bb_e[e_idx].contiguous(), det_off,
                                                     gt_d[g_rows].contiguous(), dif_d[g_rows].contiguous(),
                                                     seg_gt_off, 0.5)
            tp, fp = torch.empty_like(tp_s), torch.empty_like(fp_s)
            tp[dest], fp[dest] = tp_s, fp_s
            cls_off = torch.zeros(q * c + 1, dtype=i64, device=dev)
            cls_off[1:] = torch.cumsum(torch.bincount(sup_cls, minlength=q * c), 0)
            rec, prec, ap07, ap_area = ops.voc_ap(tp, fp, cls_off, npos.repeat(q))
            hits = torch.bincount(torch.div(seg_key, n_img, rounding_mode='floor')[code == 1],
                                  minlength=q * c)
            if bool((code == -2).any()) or bool(torch.isnan(ap07).any()):
                raise RuntimeError('grid search: inconsistent segment offsets')
            ap07, ap_area, hits, n_dets, cls_off = [x.cpu().numpy() for x in
                                                    (ap07, ap_area, hits, n_dets, cls_off)]
            if curves:
                tp, fp, rec, prec = [x.cpu().numpy() for x in (tp, fp, rec, prec)]
        for j, (t, s, l) in enumerate(chunk):
            res = []
            for ci in range(c):
                u = j * c + ci
                npos_im = gts[ci][2]
                r = dict(ap07=float(ap07[u]), ap_area=float(ap_area[u]),
                         corloc=1.0 * int(hits[u]) / npos_im if npos_im > 0 else 0.0)
                if curves:
                    sl = slice(int(cls_off[u]), int(cls_off[u + 1]))
                    r.update(tp=tp[sl], fp=fp[sl], rec=rec[sl], prec=prec[sl])
                res.append(r)
            rows.append(_row((nmses[t], threshs[s], limits[l]), n_dets[j], classes, res, use_07_metric,
                             curves))
    if timings is not None:
        timings['candidates'] = n
        timings['settings'] = len(settings)
        timings['settings_per_chunk'] = q_max
    return rows


# ---- entry points ---------------------------------------------------------------------------------
def grid_search_arrays(recs, imagenames, classes, candidates, nmses=DEFAULT_NMSES,
                       threshs=DEFAULT_THRESHS, limits=DEFAULT_LIMITS, use_07_metric=True, route=None,
                       curves=False, timings=None):
    """The sweep over annotations that are already parsed.  recs {image name: parse_rec objects},
    imagenames the image set in order, classes with '__background__' first, candidates
    [(scores fp32 [n, K], boxes fp32 [n, 4])] per image.  -> one OrderedDict per setting in the
    reference's loop order: nms, score_thresh, detections_per_im, n_dets, mAP, mCorLoc,
    AP_<class>..., CorLoc_<class>...; with curves=True also 'curves' {class: tp, fp, rec, prec,
    ap07, ap_area, corloc}.  timings (device route): a dict that receives the stages' seconds."""
    check_cfg()
    nmses, threshs, limits = list(nmses), list(threshs), [int(v) for v in limits]
    if not (nmses and threshs and limits):
        raise ValueError('grid search: an empty list of NMS thresholds, score thresholds or limits')
    if len(candidates) != len(imagenames):
        raise ValueError('grid search: {} images of candidates, the image set holds {}'.format(
            len(candidates), len(imagenames)))
    for scores, _boxes in candidates:
        if scores.shape[1] != len(classes):
            raise ValueError('grid search: scores of {} classes, the dataset has {}'.format(
                scores.shape[1], len(classes)))
    if route is None:
        route = 'device' if device_route_available() else 'host'
    assert route in ('device', 'host'), route
    logger.info('Grid search: %s route (%s), %d x %d x %d = %d settings, %d images, %d classes',
                route, 'HIP kernels' if route == 'device' else 'the literal loop', len(nmses),
                len(threshs), len(limits), len(nmses) * len(threshs) * len(limits), len(imagenames),
                len(classes) - 1)
    classes = [str(x) for x in classes]
    if route == 'device':
        return _grid_device(recs, imagenames, classes, candidates, nmses, threshs, limits,
                            use_07_metric, curves, timings)
    return _grid_host(recs, imagenames, classes, candidates, settings_of(nmses, threshs, limits),
                      use_07_metric, curves)


def grid_search(dataset, candidates, nmses=DEFAULT_NMSES, threshs=DEFAULT_THRESHS,
                limits=DEFAULT_LIMITS, route=None, curves=False, timings=None):
    """The sweep for a dataset (name, classes, get_roidb()); only the PASCAL VOC sets have an
    evaluator.  The images of the dataset must come in the order of the image set, as the
    evaluator demands."""
    import os
    if dataset.name[:4] != 'voc_':
        raise NotImplementedError('No evaluator for dataset: {}'.format(dataset.name))
    check_cfg()
    info = voc_info(dataset)
    imagenames, recs = voc_eval.load_annotations(info['anno_path'], info['image_set_path'])
    for i, entry in enumerate(dataset.get_roidb()):
        index = os.path.splitext(os.path.split(entry['image'])[1])[0]
        assert index == imagenames[i], \
            'image {} of the dataset is {}, the image set has {}'.format(i, index, imagenames[i])
    return grid_search_arrays(recs, imagenames, list(dataset.classes), candidates, nmses, threshs,
                              limits, use_07_metric=int(info['year']) < 2010, route=route,
                              curves=curves, timings=timings)


def best_setting(rows):
    """The best-mAP row; the first in loop order on a tie."""
    best = 0
    for i, r in enumerate(rows):
        if r['mAP'] > rows[best]['mAP']:
            best = i
    return best


def boxes_of_setting(candidates, num_classes, setting):
    """all_boxes[cls][image] of one setting (nms, score_thresh, detections_per_im), as the test
    engine would have left them: what evaluate_boxes takes for the winner."""
    from detectron.core.test_wsl import box_results_with_nms_and_limit
    all_boxes = [[[] for _ in candidates] for _ in range(num_classes)]
    with _cfg_keys(num_classes):
        cfg.TEST.NMS, cfg.TEST.SCORE_THRESH, cfg.TEST.DETECTIONS_PER_IM = setting
        for i, (scores, boxes) in enumerate(candidates):
            _s, _b, cls_boxes = box_results_with_nms_and_limit(scores, boxes)
            for j in range(1, num_classes):
                all_boxes[j][i] = cls_boxes[j]
    return all_boxes


def table(rows):
    """-> (header, list of value lists): the csv layout, curves left out."""
    header = [k for k in rows[0] if k != 'curves'] if rows else []
    return header, [[r[k] for k in header] for r in rows]
