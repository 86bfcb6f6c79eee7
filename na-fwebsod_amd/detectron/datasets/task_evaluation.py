"""Evaluation interface for the supported tasks (reference: detectron/datasets/task_evaluation.py).

Box detection on the PASCAL VOC sets is the one detection task / evaluator pair of this tree (box
proposals are evaluated on any json dataset: evaluate_box_proposals); masks and
keypoints are pinned off (config._OFF_PATH_SWITCHES), and a dataset without an evaluator raises as
in the reference.  results[dataset.name]['box'] holds AP (per class), mAP, CorLoc (per class) and
mCorLoc - the reference returns empty VOC results and only logs the numbers."""
import logging
from collections import OrderedDict

from detectron.datasets import voc_dataset_evaluator

logger = logging.getLogger(__name__)


def evaluate_all(dataset, all_boxes, all_segms, all_keyps, output_dir, use_matlab=False):
    """Evaluate "all" tasks: box detection (reference :53-71)."""
    all_results = evaluate_boxes(dataset, all_boxes, output_dir, use_matlab=use_matlab)
    logger.info('Evaluating bounding boxes is done!')
    return all_results


def evaluate_boxes(dataset, all_boxes, output_dir, use_matlab=False):
    """Evaluate bounding box detection (reference :74-100)."""
    logger.info('Evaluating detections')
    if _use_voc_evaluator(dataset):
        box_results = voc_dataset_evaluator.evaluate_boxes(dataset, all_boxes, output_dir,
                                                           use_matlab=use_matlab)
    else:
        raise NotImplementedError('No evaluator for dataset: {}'.format(dataset.name))
    return OrderedDict([(dataset.name, OrderedDict([('box', box_results)]))])


def evaluate_box_proposals(dataset, roidb, limits=(100, 1000),
                           areas=('all', 'small', 'medium', 'large'), route=None):
    """Evaluate bounding box object proposals (reference :159-170): AR at every limit, overall and
    per area range, in the reference's key order (limit outer, area inner).  The defaults give the
    reference's eight keys; other limits (None = no limit, key suffix '@all') and the other area
    names (the key carries the name: 'AR96-128@100') extend the sweep.  route: 'device', 'host'
    or None (cfg.NAWS.DEVICE_EVAL and a GPU decide)."""
    from detectron.datasets import json_dataset_evaluator
    stats = json_dataset_evaluator.evaluate_box_proposals_sweep(dataset, roidb, areas=areas,
                                                                limits=limits, route=route)
    return box_proposal_results(dataset.name, stats)


def box_proposal_results(dataset_name, stats):
    """{(area, limit): stats} in sweep order -> the results dict, keys 'AR<suffix>@<limit>'."""
    suffixes = {'all': '', 'small': 's', 'medium': 'm', 'large': 'l'}
    res = OrderedDict([('box_proposal', OrderedDict())])
    for (area, limit), s in stats.items():
        key = 'AR{}@{}'.format(suffixes.get(area, area),
                               'all' if limit is None else '{:d}'.format(limit))
        res['box_proposal'][key] = s['ar']
    return OrderedDict([(dataset_name, res)])


def log_box_proposal_results(results):
    """Log bounding box proposal results (reference :173-180)."""
    for dataset in results.keys():
        keys = results[dataset]['box_proposal'].keys()
        pad = max([len(k) for k in keys])
        logger.info(dataset)
        for k, v in results[dataset]['box_proposal'].items():
            logger.info('{}: {:.3f}'.format(k.ljust(pad), v))


def log_copy_paste_friendly_results(results):
    """Lines prefixed with 'copypaste: ' (reference :183-194); a per-class metric is one value per
    class."""
    for dataset in results.keys():
        logger.info('copypaste: Dataset: {}'.format(dataset))
        for task, metrics in results[dataset].items():
            logger.info('copypaste: Task: {}'.format(task))
            names, vals = [], []
            for name, v in metrics.items():
                for sub, x in (v.items() if isinstance(v, dict) else [(None, v)]):
                    names.append(name if sub is None else '{}/{}'.format(name, sub))
                    vals.append('{:.4f}'.format(x))
            logger.info('copypaste: ' + ','.join(names))
            logger.info('copypaste: ' + ','.join(vals))


def _use_voc_evaluator(dataset):
    return dataset.name[:4] == 'voc_'
