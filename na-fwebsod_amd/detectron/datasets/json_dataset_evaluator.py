"""Box-proposal recall of a json dataset (reference: detectron/datasets/json_dataset_evaluator.py
:255-336; the COCO AP functions of that file are not part of this tree).

evaluate_box_proposals is the reference's function, one numpy operation per reference operation:
the host route.  evaluate_box_proposals_sweep evaluates a whole (area range x limit) sweep over
one roidb on either route:

  host    evaluate_box_proposals once per setting.
  device  the matching of every image under every setting in ONE launch of
          csrc/proposal_eval_ops.hip (one wave per (image, setting)); torch does the plumbing -
          the crowd / class filter and the flattening on the CPU before the upload, the
          per-threshold counts and the sort after it.  Taken when cfg.NAWS.DEVICE_EVAL is set and
          a GPU is present.

Both routes return equal dicts: num_pos equal, gt_overlaps equal element for element (its length
included), recalls and ar equal as float64 bits."""
import logging
from collections import OrderedDict

import numpy as np

import detectron.utils.boxes as box_utils

logger = logging.getLogger(__name__)

AREA_NAMES = ('all', 'small', 'medium', 'large', '96-128', '128-256', '256-512', '512-inf')
AREA_RANGES = [
    [0**2, 1e5**2],    # all
    [0**2, 32**2],     # small
    [32**2, 96**2],    # medium
    [96**2, 1e5**2],   # large
    [96**2, 128**2],   # 96-128
    [128**2, 256**2],  # 128-256
    [256**2, 512**2],  # 256-512
    [512**2, 1e5**2]]  # 512-inf


def evaluate_box_proposals(json_dataset, roidb, thresholds=None, area='all', limit=None):
    """Evaluate detection proposal recall metrics (reference :255-336) -> dict(ar, recalls,
    thresholds, gt_overlaps, num_pos).

    A ground-truth box whose area sits exactly on a bound belongs to both neighbouring ranges
    (`>=` and `<=`); num_pos counts the valid ground truth of every image, but an image without
    proposals appends nothing, so gt_overlaps may be shorter than num_pos.  num_pos == 0 keeps the
    reference's behaviour: the division by zero gives NaN recalls (and numpy's RuntimeWarning)."""
    # Record max overlap value for each gt box
    # Return vector of overlap values
    areas = {name: i for i, name in enumerate(AREA_NAMES)}
    assert area in areas, 'Unknown area range: {}'.format(area)
    area_range = AREA_RANGES[areas[area]]
    gt_overlaps = np.zeros(0)
    num_pos = 0
    for entry in roidb:
        gt_inds = np.where((entry['gt_classes'] > 0) & (entry['is_crowd'] == 0))[0]
        gt_boxes = entry['boxes'][gt_inds, :]
        gt_areas = entry['seg_areas'][gt_inds]
        valid_gt_inds = np.where((gt_areas >= area_range[0]) & (gt_areas <= area_range[1]))[0]
        gt_boxes = gt_boxes[valid_gt_inds, :]
        num_pos += len(valid_gt_inds)
        non_gt_inds = np.where(entry['gt_classes'] == 0)[0]
        boxes = entry['boxes'][non_gt_inds, :]
        if boxes.shape[0] == 0:
            continue
        if limit is not None and boxes.shape[0] > limit:
            boxes = boxes[:limit, :]
        overlaps = box_utils.bbox_overlaps(boxes.astype(dtype=np.float32, copy=False),
                                           gt_boxes.astype(dtype=np.float32, copy=False))
        _gt_overlaps = np.zeros((gt_boxes.shape[0]))
        for j in range(min(boxes.shape[0], gt_boxes.shape[0])):
            # find which proposal box maximally covers each gt box
            argmax_overlaps = overlaps.argmax(axis=0)
            # and get the iou amount of coverage for each gt box
            max_overlaps = overlaps.max(axis=0)
            # find which gt box is 'best' covered (i.e. 'best' = most iou)
            gt_ind = max_overlaps.argmax()
            gt_ovr = max_overlaps.max()
            assert gt_ovr >= 0
            # find the proposal box that covers the best covered gt box
            box_ind = argmax_overlaps[gt_ind]
            # record the iou coverage of this gt box
            _gt_overlaps[j] = overlaps[box_ind, gt_ind]
            assert _gt_overlaps[j] == gt_ovr
            # mark the proposal box and the gt box as used
            overlaps[box_ind, :] = -1
            overlaps[:, gt_ind] = -1
        # append recorded iou coverage level
        gt_overlaps = np.hstack((gt_overlaps, _gt_overlaps))

    gt_overlaps = np.sort(gt_overlaps)
    return _summarize(gt_overlaps, num_pos, thresholds)


def _summarize(gt_overlaps, num_pos, thresholds):
    """The reference's tail (:326-336) over the sorted overlaps."""
    if thresholds is None:
        step = 0.05
        thresholds = np.arange(0.5, 0.95 + 1e-5, step)
    recalls = np.zeros_like(thresholds)
    # compute recall for each iou threshold
    for i, t in enumerate(thresholds):
        recalls[i] = (gt_overlaps >= t).sum() / float(num_pos)
    # ar = 2 * np.trapz(recalls, thresholds)
    ar = recalls.mean()
    return {'ar': ar, 'recalls': recalls, 'thresholds': thresholds,
            'gt_overlaps': gt_overlaps, 'num_pos': num_pos}


def device_route_available():
    """cfg.NAWS.DEVICE_EVAL and a GPU."""
    from detectron.core.config import cfg
    if not cfg.NAWS.DEVICE_EVAL:
        return False
    import torch
    return torch.cuda.is_available()


def flatten_roidb(roidb):
    """The kernel's inputs as numpy: (boxes fp32 [P, 4], box_off int64 [S + 1], gt fp32 [G, 4],
    gt_area fp32 [G], gt_off int64 [S + 1]) - per image the rows with gt_classes == 0 in file
    order and the rows with gt_classes > 0 and is_crowd == 0 in roidb order."""
    pb, gb, ga = [np.zeros((0, 4), np.float32)], [np.zeros((0, 4), np.float32)], [np.zeros(0, np.float32)]
    box_off, gt_off = [0], [0]
    for entry in roidb:
        gt_inds = np.where((entry['gt_classes'] > 0) & (entry['is_crowd'] == 0))[0]
        non_gt_inds = np.where(entry['gt_classes'] == 0)[0]
        pb.append(entry['boxes'][non_gt_inds, :].astype(np.float32, copy=False))
        gb.append(entry['boxes'][gt_inds, :].astype(np.float32, copy=False))
        ga.append(entry['seg_areas'][gt_inds].astype(np.float32, copy=False))
        box_off.append(box_off[-1] + len(non_gt_inds))
        gt_off.append(gt_off[-1] + len(gt_inds))
    return (np.ascontiguousarray(np.concatenate(pb)), np.array(box_off, np.int64),
            np.ascontiguousarray(np.concatenate(gb)), np.ascontiguousarray(np.concatenate(ga)),
            np.array(gt_off, np.int64))


def match_on_device(roidb, areas, limits, device='cuda', timings=None):
    """-> gt_iou fp32 tensor [len(areas) * len(limits), G] on the device, setting (a, l) in row
    a * len(limits) + l; see naws_proposal_match_fwd for the values."""
    import time
    import torch
    from naws_hip import ops
    t0 = time.perf_counter()
    arrays = flatten_roidb(roidb)
    t1 = time.perf_counter()
    boxes, box_off, gt, gt_area, gt_off = [torch.from_numpy(a).to(device) for a in arrays]
    lo = [AREA_RANGES[AREA_NAMES.index(a)][0] for a in areas]
    hi = [AREA_RANGES[AREA_NAMES.index(a)][1] for a in areas]
    lim = [0 if l is None else int(l) for l in limits]
    if timings is not None:
        torch.cuda.synchronize()
    t2 = time.perf_counter()
    out = ops.proposal_match(boxes, box_off, gt, gt_area, gt_off, lo, hi, lim)
    if timings is not None:
        torch.cuda.synchronize()
        timings.update(flatten_s=t1 - t0, upload_s=t2 - t1, kernel_s=time.perf_counter() - t2)
    return out


def summarize_device(gt_iou_row, thresholds=None):
    """One setting's dict from its gt_iou row (a device tensor): the per-threshold counts are
    taken on the device over the entries >= 0 as float64, everything else is the host tail."""
    import torch
    if thresholds is None:
        step = 0.05
        thresholds = np.arange(0.5, 0.95 + 1e-5, step)
    num_pos = int((gt_iou_row != -1).sum())
    kept = gt_iou_row[gt_iou_row >= 0].double()
    gt_overlaps = np.sort(kept.cpu().numpy())
    t = torch.from_numpy(np.asarray(thresholds, np.float64)).to(kept.device)
    counts = (kept[None, :] >= t[:, None]).sum(1).cpu().numpy()
    recalls = np.zeros_like(thresholds)
    for i in range(len(thresholds)):
        recalls[i] = counts[i] / float(num_pos)
    ar = recalls.mean()
    return {'ar': ar, 'recalls': recalls, 'thresholds': thresholds,
            'gt_overlaps': gt_overlaps, 'num_pos': num_pos}


def evaluate_box_proposals_sweep(json_dataset, roidb, areas=('all',), limits=(None,), thresholds=None,
                                 route=None, timings=None):
    """-> OrderedDict {(area, limit): evaluate_box_proposals' dict}, limit-outer / area-inner as the
    reference's task_evaluation loops.  limits: None (no limit) or positive ints.  route: 'device',
    'host' or None (device_route_available() decides)."""
    if route is None:
        route = 'device' if device_route_available() else 'host'
    assert route in ('device', 'host'), route
    for area in areas:
        assert area in AREA_NAMES, 'Unknown area range: {}'.format(area)
    for limit in limits:
        assert limit is None or int(limit) > 0, 'limit must be None or positive: {}'.format(limit)
    logger.info('Box proposal recall: %s route (%s), %d images, %d settings', route,
                'HIP kernel' if route == 'device' else 'numpy', len(roidb), len(areas) * len(limits))
    res = OrderedDict()
    if route == 'host':
        for limit in limits:
            for area in areas:
                res[(area, limit)] = evaluate_box_proposals(json_dataset, roidb, thresholds=thresholds,
                                                            area=area, limit=limit)
        return res
    import time
    gt_iou = match_on_device(roidb, list(areas), list(limits), timings=timings)
    t0 = time.perf_counter()
    for li, limit in enumerate(limits):
        for ai, area in enumerate(areas):
            res[(area, limit)] = summarize_device(gt_iou[ai * len(limits) + li], thresholds)
    if timings is not None:
        timings['tail_s'] = time.perf_counter() - t0
    return res
