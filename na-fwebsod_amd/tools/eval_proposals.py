#!/usr/bin/env python3
"""Recall of a proposal file on a dataset (reference: rpn_generator.evaluate_proposal_file and
task_evaluation.evaluate_box_proposals): AR at every limit, overall and per area range.

    python tools/eval_proposals.py --cfg YAML [--dataset NAME] [--proposal-file F]
        [--limits 100 1000] [--areas all small medium large] [--route host|device]
        [--output-dir D] [-- KEY VALUE ...]

--dataset defaults to TEST.DATASETS[0], --proposal-file to the matching TEST.PROPOSAL_FILES entry;
--limits takes positive ints or `none`.  Loads get_roidb(gt=True, proposal_file=F), evaluates,
logs the reference's lines and writes into the output directory:

    rpn_proposal_recall.pkl   the results dict (the reference's file name)
    proposal_recall.csv       area, limit, num_pos, ar, recall@0.50 ... recall@0.95 per setting

The route is the device route (csrc/proposal_eval_ops.hip) when NAWS.DEVICE_EVAL is set and a GPU
is present, else the host route; --route forces one."""
import argparse
import csv
import logging
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import detectron.core.config as core_config  # noqa: E402
from detectron.core.config import cfg  # noqa: E402

logger = logging.getLogger(__name__)


def _limit(text):
    if text.lower() in ('none', 'all'):
        return None
    v = int(text)
    if v <= 0:
        raise argparse.ArgumentTypeError('a limit is a positive int or `none`')
    return v


def parse_args(argv=None):
    from detectron.datasets.json_dataset_evaluator import AREA_NAMES
    p = argparse.ArgumentParser(description='Evaluate the recall of a proposal file')
    p.add_argument('--cfg', dest='cfg_file', default=None, type=str, help='config file')
    p.add_argument('--dataset', dest='dataset_name', default=None, type=str,
                   help='dataset (default: TEST.DATASETS[0])')
    p.add_argument('--proposal-file', dest='proposal_file', default=None, type=str,
                   help='proposal file (default: the TEST.PROPOSAL_FILES entry of the dataset)')
    p.add_argument('--limits', nargs='+', type=_limit, default=[100, 1000])
    p.add_argument('--areas', nargs='+', choices=AREA_NAMES, default=['all', 'small', 'medium', 'large'])
    p.add_argument('--route', choices=('host', 'device'), default=None)
    p.add_argument('--output-dir', dest='output_dir', default=None, type=str)
    p.add_argument('opts', default=None, nargs=argparse.REMAINDER,
                   help='-- KEY VALUE pairs merged into the config')
    return p.parse_args(argv)


def resolve(args):
    """(dataset name, proposal file) from the arguments and the config."""
    name = args.dataset_name
    if name is None:
        if not cfg.TEST.DATASETS:
            sys.exit('no --dataset and TEST.DATASETS is empty')
        name = cfg.TEST.DATASETS[0]
    pf = args.proposal_file
    if pf is None:
        names = list(cfg.TEST.DATASETS)
        if name not in names or len(cfg.TEST.PROPOSAL_FILES) <= names.index(name):
            sys.exit('no --proposal-file and TEST.PROPOSAL_FILES has no entry for {}'.format(name))
        pf = cfg.TEST.PROPOSAL_FILES[names.index(name)]
    return name, pf


def write_csv(path, stats):
    thresholds = next(iter(stats.values()))['thresholds']
    with open(path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['area', 'limit', 'num_pos', 'ar'] + ['recall@%.2f' % t for t in thresholds])
        for (area, limit), s in stats.items():
            w.writerow([area, 'none' if limit is None else limit, s['num_pos'], repr(float(s['ar']))]
                       + [repr(float(r)) for r in s['recalls']])


def evaluate_proposal_file(dataset_name, proposal_file, output_dir, limits, areas, route=None):
    from detectron.datasets import dataset_catalog, json_dataset_evaluator, task_evaluation
    from detectron.datasets.json_dataset_wsl import JsonDataset
    from detectron.utils.net_wsl import save_object
    if not dataset_catalog.contains(dataset_name):
        sys.exit('unknown dataset: {}'.format(dataset_name))
    for what, path in (('annotation file', dataset_catalog.get_ann_fn(dataset_name)),
                       ('image directory', dataset_catalog.get_im_dir(dataset_name)),
                       ('proposal file', proposal_file)):
        if not os.path.exists(path):
            sys.exit('{} of {} not found: {}'.format(what, dataset_name, path))
    dataset = JsonDataset(dataset_name)
    roidb = dataset.get_roidb(gt=True, proposal_file=proposal_file)
    stats = json_dataset_evaluator.evaluate_box_proposals_sweep(dataset, roidb, areas=areas,
                                                                limits=limits, route=route)
    results = task_evaluation.box_proposal_results(dataset.name, stats)
    task_evaluation.log_box_proposal_results(results)
    if not os.path.isdir(output_dir):
        os.makedirs(output_dir)
    save_object(results, os.path.join(output_dir, 'rpn_proposal_recall.pkl'))
    write_csv(os.path.join(output_dir, 'proposal_recall.csv'), stats)
    logger.info('Wrote rpn_proposal_recall.pkl and proposal_recall.csv to %s', output_dir)
    return results


def main(argv=None):
    logging.basicConfig(level=logging.INFO, stream=sys.stdout,
                        format='%(levelname)s %(filename)s:%(lineno)4d: %(message)s')
    args = parse_args(argv)
    if args.cfg_file is not None:
        core_config.merge_cfg_from_file(args.cfg_file)
    opts = [o for o in (args.opts or []) if o != '--']
    if opts:
        core_config.merge_cfg_from_list(opts)
    name, pf = resolve(args)
    out = args.output_dir or core_config.get_output_dir((name,), training=False)
    return evaluate_proposal_file(name, pf, os.path.abspath(out), args.limits, args.areas, args.route)


if __name__ == '__main__':
    main()
