#!/usr/bin/env python3
"""Grid search over TEST.NMS x TEST.SCORE_THRESH x TEST.DETECTIONS_PER_IM on the unsuppressed
detections of one test run (reference CLI: tools/test_net_wsl_grid_search.py `--cfg FILE KEY VALUE
...`, whose lists are the defaults here):

    python tools/test_net_wsl_grid_search.py --cfg configs/flickr_voc/na_wsddn_V-16-C5_1x.yaml \
        [--collect] [--nms 0.5 0.4 0.3] [--thresh 1e-5 1e-3] [--max-per-image 100 10] \
        [-- TEST.WEIGHTS model_final.pkl ...]

--collect first runs the test engine with TEST.NMS 1.1, TEST.SCORE_THRESH -1e10 and
TEST.DETECTIONS_PER_IM 0 (nothing suppressed, nothing cut) into <output_dir>/grid_search/; without
it <output_dir>/grid_search/detections.pkl must exist.  Written into that directory:
grid_search.csv (a header and one row per setting, in the loop order NMS / score threshold /
limit), grid_search.pkl (the rows, the lists and the best setting) and, for the best-mAP setting
(the first on a tie), the result files and pickles of the usual evaluation.  A list option takes
its values separated by blanks or commas; KEY VALUE pairs follow a `--`."""
import argparse
import csv
import logging
import os
import pprint
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from detectron.core.config import (assert_and_infer_cfg, cfg, get_output_dir,  # noqa: E402
                                   merge_cfg_from_file, merge_cfg_from_list)

GRID_DIR = 'grid_search'


def _list_of(kind):
    def parse(text):
        return [kind(v) for v in text.split(',') if v != '']
    return parse


def parse_args(argv=None):
    from detectron.core import grid_search_wsl as gs
    p = argparse.ArgumentParser(description='Grid search over the test-time NMS, score and per-image limits')
    p.add_argument('--cfg', dest='cfg_file', default=None, type=str)
    p.add_argument('--collect', action='store_true',
                   help='run the test engine without suppression first (else detections.pkl must exist)')
    p.add_argument('--nms', nargs='+', type=_list_of(float), default=None, help='TEST.NMS values')
    p.add_argument('--thresh', nargs='+', type=_list_of(float), default=None,
                   help='TEST.SCORE_THRESH values')
    p.add_argument('--max-per-image', dest='max_per_image', nargs='+', type=_list_of(int), default=None,
                   help='TEST.DETECTIONS_PER_IM values (0 = no limit)')
    p.add_argument('--route', choices=('device', 'host'), default=None,
                   help='default: NAWS.DEVICE_EVAL and a GPU decide')
    p.add_argument('--num-images', type=int, default=None,
                   help='synthetic fallback only: number of images (NAWS.SYNTHETIC_TEST_IMAGES)')
    p.add_argument('opts', default=None, nargs=argparse.REMAINDER)
    args = p.parse_args(argv)
    flat = lambda v, d: list(d) if v is None else [x for part in v for x in part]
    args.nms = flat(args.nms, gs.DEFAULT_NMSES)
    args.thresh = flat(args.thresh, gs.DEFAULT_THRESHS)
    args.max_per_image = flat(args.max_per_image, gs.DEFAULT_LIMITS)
    if args.opts and args.opts[0] == '--':
        args.opts = args.opts[1:]
    return args


def synthetic_annotations(roidb, num_classes):
    """Datasets that are not on disk: the synthetic roidb's image-level label rides on its first
    box (datasets/synthetic.py), which stands in as the image's one annotated object."""
    classes = ['__background__'] + ['class%02d' % j for j in range(1, num_classes)]
    names, recs = [], {}
    for e in roidb:
        name = os.path.splitext(os.path.basename(e['image']))[0]
        names.append(name)
        j = int(e['gt_classes'][e['gt_classes'] > 0][-1])
        b = e['boxes'][0]
        recs[name] = [{'name': classes[j], 'pose': 'Unspecified', 'truncated': 0, 'difficult': 0,
                       'bbox': [int(b[0]) + 1, int(b[1]) + 1, int(b[2]) + 1, int(b[3]) + 1]}]
    return recs, names, classes


def write_table(rows, out_dir, lists, best):
    from detectron.core import grid_search_wsl as gs
    from detectron.utils.net_wsl import save_object
    header, values = gs.table(rows)
    with open(os.path.join(out_dir, 'grid_search.csv'), 'w', newline='') as f:
        w = csv.writer(f, dialect='excel')
        w.writerow(header)
        w.writerows(values)
    save_object(dict(rows=[dict(r) for r in rows], header=header, nmses=lists[0], threshs=lists[1],
                     max_per_images=lists[2], best=best), os.path.join(out_dir, 'grid_search.pkl'))


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format='%(levelname)s %(filename)s:%(lineno)4d: %(message)s')
    logger = logging.getLogger(__name__)
    args = parse_args(argv)
    if args.cfg_file:
        merge_cfg_from_file(args.cfg_file)
    if args.opts:
        merge_cfg_from_list(args.opts)
    if args.num_images is not None:
        merge_cfg_from_list(['NAWS.SYNTHETIC_TEST_IMAGES', args.num_images])
    assert_and_infer_cfg(make_immutable=False)
    from detectron.core import grid_search_wsl as gs
    from detectron.core import test_engine_wsl
    from detectron.utils.net_wsl import load_object
    gs.check_cfg()
    dataset_name, proposal_file = test_engine_wsl.get_inference_dataset(0)
    out_dir = os.path.join(get_output_dir(dataset_name, training=False), GRID_DIR)
    os.makedirs(out_dir, exist_ok=True)
    det_file = os.path.join(out_dir, 'detections.pkl')
    if args.collect:
        test_engine_wsl.check_weights_file(cfg.TEST.WEIGHTS)
        saved = (cfg.TEST.NMS, cfg.TEST.SCORE_THRESH, cfg.TEST.DETECTIONS_PER_IM)
        merge_cfg_from_list(list(gs.COLLECT_OPTS))
        logger.info('Collecting unsuppressed detections with config:')
        logger.info(pprint.pformat(cfg.TEST))
        test_engine_wsl.test_net_on_dataset(cfg.TEST.WEIGHTS, dataset_name, proposal_file, out_dir)
        cfg.TEST.NMS, cfg.TEST.SCORE_THRESH, cfg.TEST.DETECTIONS_PER_IM = saved
    elif not os.path.exists(det_file):
        raise FileNotFoundError('{} does not exist: run with --collect first'.format(det_file))
    candidates = gs.candidates_from_detections(load_object(det_file)['all_boxes'])
    lists = (args.nms, args.thresh, args.max_per_image)
    real = test_engine_wsl.dataset_on_disk(dataset_name)
    if real:
        from detectron.datasets.json_dataset_wsl import JsonDataset
        dataset = JsonDataset(dataset_name)
        rows = gs.grid_search(dataset, candidates, *lists, route=args.route)
    else:
        roidb = test_engine_wsl.get_roidb_and_dataset(dataset_name, proposal_file, None)[0]
        recs, names, classes = synthetic_annotations(roidb, cfg.MODEL.NUM_CLASSES)
        rows = gs.grid_search_arrays(recs, names, classes, candidates, *lists, route=args.route)
    best = gs.best_setting(rows)
    write_table(rows, out_dir, lists, best)
    b = rows[best]
    logger.info('Best of %d settings: TEST.NMS %s TEST.SCORE_THRESH %s TEST.DETECTIONS_PER_IM %s: mAP %.4f, '
                'mCorLoc %.4f, %d detections', len(rows), b['nms'], b['score_thresh'],
                b['detections_per_im'], b['mAP'], b['mCorLoc'], b['n_dets'])
    if real:
        from detectron.datasets import task_evaluation
        all_boxes = gs.boxes_of_setting(candidates, cfg.MODEL.NUM_CLASSES,
                                        (b['nms'], b['score_thresh'], b['detections_per_im']))
        results = task_evaluation.evaluate_boxes(dataset, all_boxes, out_dir)
        task_evaluation.log_copy_paste_friendly_results(results)
    else:
        logger.info('%s is not on disk (synthetic images stood in): no result files for the best '
                    'setting', dataset_name)
    logger.info('Wrote %s', os.path.join(out_dir, 'grid_search.csv'))
    return rows


if __name__ == '__main__':
    main()
