"""Test-time grid search (detectron/core/grid_search_wsl.py, tools/test_net_wsl_grid_search.py)
without a GPU: the host route against the oracle (tests/grid_search_ref.py), the reconstruction of
the candidates, the claims the device route's design rests on (in numpy), the exact rounding
helpers, the C-ABI refusals of the two new entries, the cfg refusals, the table files and the
tool's command line."""
import csv
import ctypes as C
import os
import sys

import numpy as np
import pytest

import grid_search_ref as gr
import voc_eval_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = ([1.0, 0.5, 0.0], [1e-10, 1e-4, 1e-1], [0, 5, 1])


@pytest.fixture(scope='module')
def tiny():
    recs, names, classes, cands = gr.tiny_case()
    return recs, names, classes, cands, gr.Oracle(recs, names, classes, cands)


@pytest.fixture
def gs(cfgmod):
    cfgmod.cfg.TEST.BBOX_REG = False
    cfgmod.cfg.NAWS.DEVICE_EVAL = False
    from detectron.core import grid_search_wsl
    return grid_search_wsl


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'na-fwebsod_amd', 'tools'))
    try:
        import test_net_wsl_grid_search as tool
    finally:
        sys.path.pop(0)
    return tool


# ---- the host route -------------------------------------------------------------------------------
def test_host_route_equals_the_oracle_on_the_tiny_devkit(gs, tiny, monkeypatch, tmp_path, caplog):
    import logging
    recs, names, classes, cands, oracle = tiny
    fx = vc.fixture()
    vc.register_tiny(monkeypatch, tmp_path, fx)
    with caplog.at_level(logging.INFO):
        rows = gs.grid_search(vc.StandInDataset(fx), cands, *GRID, curves=True)
    assert 'Grid search: host route' in caplog.text            # NAWS.DEVICE_EVAL False: route None = host
    settings = [(a, b, c) for a in GRID[0] for b in GRID[1] for c in GRID[2]]
    assert [(r['nms'], r['score_thresh'], r['detections_per_im']) for r in rows] == settings
    for r in rows:
        gr.assert_row_matches(r, oracle.row(r['nms'], r['score_thresh'], r['detections_per_im']), classes)
    assert list(rows[0])[:6] == ['nms', 'score_thresh', 'detections_per_im', 'n_dets', 'mAP', 'mCorLoc']
    assert list(rows[0])[6:12] == ['AP_bird', 'AP_cat', 'AP_dog', 'CorLoc_bird', 'CorLoc_cat', 'CorLoc_dog']
    # the sweep is not vacuous: the settings differ, something is found, and the cfg is put back
    assert len({r['n_dets'] for r in rows}) > 5 and max(r['mAP'] for r in rows) > 0
    from detectron.core.config import cfg
    assert (cfg.TEST.NMS, cfg.TEST.SCORE_THRESH, cfg.TEST.DETECTIONS_PER_IM, cfg.NAWS.HOST_NMS) == \
        (0.3, 0.05, 100, False)


def test_candidates_round_trip_and_a_suppressed_run_is_refused(gs, tiny):
    _recs, _names, classes, cands, _o = tiny
    all_boxes = gs.boxes_of_setting(cands, len(classes), (1.1, -1e10, 0))      # a collection run
    back = gs.candidates_from_detections(all_boxes)
    assert len(back) == len(cands)
    for (s0, b0), (s1, b1) in zip(cands, back):
        assert np.array_equal(b0, b1) and np.array_equal(s0[:, 1:], s1[:, 1:])
        assert s1.dtype == np.float32 and b1.dtype == np.float32 and (s1[:, 0] == -1).all()
    with pytest.raises(ValueError, match='not those of a collection run'):
        gs.candidates_from_detections(gs.boxes_of_setting(cands, len(classes), (0.3, 1e-3, 0)))


# ---- the claims of the design, in numpy -----------------------------------------------------------
def _random_list(rng, n):
    xy = rng.integers(0, 60, (n, 2)).astype(np.float32)
    wh = rng.integers(4, 50, (n, 2)).astype(np.float32)
    boxes = np.hstack([xy, xy + wh])
    boxes[n // 2:] = boxes[rng.integers(0, max(1, n // 2), n - n // 2)]      # exact copies
    scores = np.round(10.0 ** rng.uniform(-6, 0, n), 4).astype(np.float32)    # ties
    return boxes, scores


def test_claim_score_threshold_is_a_prefix():
    """NMS of the list cut at s = NMS of the list cut at the smallest threshold, filtered by
    score > s; and the word pass gives every threshold's survivors at once."""
    from detectron.core import test_wsl
    rng = np.random.default_rng(3)
    thr = [1.0, 0.7, 0.5, 0.3, 0.0]
    for n in (0, 1, 2, 17, 90):
        boxes, scores = _random_list(rng, n)
        s_min = np.float32(1e-6)
        base = np.where(scores > s_min)[0]
        order = base[np.argsort(-scores[base], kind='stable')]
        words = gr.nms_words(boxes[order], thr)
        for t, nms_t in enumerate(thr):
            with np.errstate(divide='ignore', invalid='ignore'):
                full = base[test_wsl.nms(np.hstack([boxes[base], scores[base, None]]), nms_t)]
            assert np.array_equal(np.sort(order[((words >> t) & 1) == 1]), full)
            for s in (1e-4, 1e-2, 0.5):
                inds = np.where(scores > np.float32(s))[0]
                with np.errstate(divide='ignore', invalid='ignore'):
                    direct = inds[test_wsl.nms(np.hstack([boxes[inds], scores[inds, None]]), nms_t)]
                assert np.array_equal(direct, full[scores[full] > np.float32(s)]), (n, nms_t, s)


def test_claim_cut_formula_with_ties_keeping_more_than_the_limit():
    """selected = survives and score > s and (count <= L or score >= kth): equal to the np.sort
    cut, on random images and on a tie across the cut (more than L kept)."""
    rng = np.random.default_rng(4)
    sthr, limits = [1e-5, 1e-2, 0.3], [0, 1, 3, 7, 1000]
    for trial in range(6):
        n, k = int(rng.integers(1, 40)), 4
        scores = np.full((n, k), -1, np.float32)
        scores[:, 1:] = np.round(10.0 ** rng.uniform(-6, 0, (n, k - 1)), 2 if trial % 2 else 5)
        alive = rng.random((n, k)) < 0.6                                   # any survivor set
        rows, cls = np.nonzero(alive[:, 1:])
        sc = scores[rows, cls + 1]
        o = np.argsort(-sc, kind='stable')
        count, kth = gr.cut_tables(np.ones(len(o), np.int64), sc[o], 1, sthr, limits)
        for s, th in enumerate(sthr):
            kept = {j: np.where(alive[:, j] & (scores[:, j] > np.float32(th)))[0] for j in range(1, k)}
            for l, lim in enumerate(limits):
                ref = gr.cut_rows(scores, kept, lim)
                sel = sc > np.float32(th)
                if lim > 0:
                    sel &= (count[0, s] <= lim) | (sc >= kth[0, l])
                for j in range(1, k):
                    assert np.array_equal(np.sort(rows[sel & (cls == j - 1)]), ref[j]), (trial, th, lim)
    _recs, _names, _classes, cands, (nms, th, lim) = gr.case_tie_across_the_cut()
    sc = cands[0][0][:, 1]
    count, kth = gr.cut_tables(np.ones(3, np.int64), sc, 1, [th], [lim])
    assert count[0, 0] == 3 and kth[0, 0] == np.float32(0.5)
    assert int(((count[0, 0] <= lim) | (sc >= kth[0, 0])).sum()) == 3          # more than L = 2


def test_claim_one_evaluation_order_for_every_setting(gs, tiny):
    """A setting's detections are a subsequence of ONE order (class, descending rounded
    confidence, image, row): the design in numpy gives the oracle's flags and curves, and its
    lists already are in the evaluator's order.  The rounded-confidence tie case has distinct fp32
    scores that print alike."""
    from detectron.datasets import voc_eval
    recs, names, classes, cands, oracle = tiny
    cases = [(recs, names, classes, cands, oracle, GRID)]
    r2, n2, c2, k2, setting = gr.case_rounded_confidence_tie()
    cases.append((r2, n2, c2, k2, gr.Oracle(r2, n2, c2, k2), [[v] for v in setting]))
    for recs, names, classes, cands, oracle, grid in cases:
        for key, (dets, n_dets) in gr.design_rows(recs, names, classes, cands, *grid).items():
            ref = oracle.row(*key)
            assert n_dets == ref['n_dets'], key
            res = voc_eval.evaluate_arrays(recs, names, dets, use_07_metric=True, route='host')
            vc.assert_same_results(res, ref['classes'])
            for c in classes[1:]:
                conf = dets[c][1]
                assert np.array_equal(np.argsort(-conf, kind='stable'), np.arange(len(conf))), (key, c)
    conf = gr.design_rows(r2, n2, c2, k2, *[[v] for v in setting])[setting][0]['c0']
    assert conf[0] == ['000001', '000002'] and conf[1][0] == conf[1][1]       # a tie, in file order


# ---- the rounding helpers -------------------------------------------------------------------------
def _line_fields(det):
    from detectron.datasets.voc_dataset_evaluator import result_line
    return [float(v) for v in result_line('x', det).split(' ')[1:]]


def test_round_confidence_equals_the_result_line(gs):
    rng = np.random.default_rng(6)
    vals = [np.float32(0), np.float32(-0.0), np.float32(1), np.float32(1e-10), np.float32(4.9999999e-10),
            np.float32(5e-10), np.float32(0.1), np.float32(123456.789), np.float32(2.0 ** 20),
            np.float32(3.0e7), np.float32(-0.3), np.float32(1e-45), np.float32(np.inf)]
    # m / 1024 with m odd: m * 976562.5 is an exact '%.9f' tie (round half to even); and its
    # fp32 neighbours, one ulp to either side
    for m in (1, 3, 5, 7, 333, 1023, 2047):
        v = np.float32(m / 1024.0)
        vals += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(4))]
    # the fp32 numbers nearest to a tie (q + 0.5) * 1e-9 that is not representable, and neighbours
    for q in (0, 1, 7, 12345, 999999, 5000000):
        v = np.float32((q + 0.5) * 1e-9)
        vals += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(1))]
    vals += list((10.0 ** rng.uniform(-12, 0, 4000)).astype(np.float32))
    vals = np.array(vals, np.float32)
    got = gs.round_confidence(vals)
    assert got.dtype == np.float64
    ref = np.array([_line_fields(np.array([0, 0, 0, 0, v], np.float32))[0] for v in vals])
    assert np.array_equal(got, ref) and np.array_equal(np.signbit(got), np.signbit(ref))
    assert gs.round_confidence(np.float32(1 / 1024.0)) == 0.000976562          # the tie went to even
    assert np.isnan(gs.round_confidence(np.array([np.nan], np.float32))[0])


def test_round_coordinate_equals_the_result_line(gs):
    rng = np.random.default_rng(7)
    vals = np.concatenate([np.arange(0, 300, 0.25), [0.05, 0.15, 0.25, 0.35, -0.75, -1.0, -1.05, 16777216.0],
                           rng.uniform(-5, 2000, 3000)]).astype(np.float32)
    got = gs.round_coordinate(vals)
    ref = np.array([_line_fields(np.array([v, 0, 0, 0, 0], np.float32))[1] for v in vals])
    assert got.dtype == np.float64 and np.array_equal(got, ref)
    assert gs.round_coordinate(np.float32(0.25)) == 1.2 and gs.round_coordinate(np.float32(0.75)) == 1.8


# ---- the C ABI ------------------------------------------------------------------------------------
def test_cabi_refusals_come_before_any_launch():
    from naws_hip import lib as L
    assert 'naws_nms_multi_fwd' in L.ALL_SYMBOLS and 'naws_grid_cut_fwd' in L.ALL_SYMBOLS
    buf = (C.c_float * 64)()                       # host memory: no entry below gets to a launch
    thr = (C.c_float * 40)(*([0.5] * 40))
    lim = (C.c_int32 * 4)(1, 2, 3, 4)
    p = C.addressof(buf)
    t, l = C.addressof(thr), C.addressof(lim)

    def code(name, *args):
        with pytest.raises(L.NawsError) as e:
            L.call(name, *args)
        return e.value.code

    nms = lambda **k: code('naws_nms_multi_fwd', k.get('boxes', p), k.get('off', p), k.get('total', 4),
                           k.get('lists', 1), k.get('thr', t), k.get('T', 3), k.get('out', p),
                           k.get('status', p), None)
    assert nms(T=0) == L.ERR_ARG and nms(T=-1) == L.ERR_ARG
    assert nms(T=33) == L.ERR_UNSUPPORTED
    assert nms(total=-1) == L.ERR_SHAPE and nms(lists=-1) == L.ERR_SHAPE
    assert nms(total=-1, T=0, off=None) == L.ERR_SHAPE                       # SHAPE before ARG before NULL
    assert nms(T=0, off=None) == L.ERR_ARG
    assert nms(boxes=p + 4) == L.ERR_ARG                                     # not on 16 bytes
    for k in ('boxes', 'off', 'thr', 'out', 'status'):
        assert nms(**{k: None}) == L.ERR_NULL, k
    assert nms(T=33, off=None) == L.ERR_NULL                                 # NULL before UNSUPPORTED
    nan = (C.c_float * 3)(0.5, float('nan'), 0.3)
    assert nms(thr=C.addressof(nan)) == L.ERR_ARG
    assert L.call('naws_nms_multi_fwd', None, p, 0, 0, t, 32, None, None, None) == L.OK   # nothing to do

    cut = lambda **k: code('naws_grid_cut_fwd', k.get('surv', p), k.get('score', p), k.get('off', p),
                           k.get('N', 4), k.get('I', 1), k.get('T', 3), k.get('sthr', t), k.get('S', 2),
                           k.get('lim', l), k.get('Lc', 2), k.get('count', p), k.get('kth', p),
                           k.get('status', p), None)
    assert cut(T=0) == L.ERR_ARG and cut(T=33) == L.ERR_UNSUPPORTED
    assert cut(S=65) == L.ERR_UNSUPPORTED and cut(Lc=65) == L.ERR_UNSUPPORTED
    assert cut(N=-1) == L.ERR_SHAPE and cut(I=-1) == L.ERR_SHAPE and cut(S=-1) == L.ERR_SHAPE
    for k in ('surv', 'score', 'off', 'sthr', 'lim', 'count', 'kth', 'status'):
        assert cut(**{k: None}) == L.ERR_NULL, k
    assert cut(sthr=C.addressof(nan), S=3) == L.ERR_ARG
    assert L.call('naws_grid_cut_fwd', None, None, p, 0, 0, 3, t, 2, l, 2, None, None, None, None) == L.OK


# ---- refusals, files, command line ----------------------------------------------------------------
@pytest.mark.parametrize('key', ['TEST.SOFT_NMS.ENABLED', 'TEST.BBOX_VOTE.ENABLED', 'TEST.BBOX_REG'])
def test_cfg_keys_outside_the_sweep_are_refused(gs, tiny, cfgmod, key):
    recs, names, classes, cands, _o = tiny
    node, parts = cfgmod.cfg, key.split('.')
    for part in parts[:-1]:
        node = node[part]
    node[parts[-1]] = True
    with pytest.raises(NotImplementedError, match=key.replace('.', r'\.')):
        gs.grid_search_arrays(recs, names, classes, cands, [0.5], [1e-3], [0], route='host')


def test_a_dataset_without_an_evaluator_and_bad_inputs_are_refused(gs, tiny):
    recs, names, classes, cands, _o = tiny
    fx = vc.fixture()
    with pytest.raises(NotImplementedError, match='No evaluator for dataset: coco_2014_minival'):
        gs.grid_search(vc.StandInDataset(fx, name='coco_2014_minival'), cands)
    with pytest.raises(ValueError, match='images of candidates'):
        gs.grid_search_arrays(recs, names, classes, cands[:-1], [0.5], [1e-3], [0], route='host')
    with pytest.raises(ValueError, match='empty list'):
        gs.grid_search_arrays(recs, names, classes, cands, [], [1e-3], [0], route='host')


def test_default_lists_are_the_references(gs):
    assert list(gs.DEFAULT_NMSES) == [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.0]
    assert list(gs.DEFAULT_THRESHS) == [1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1]
    assert list(gs.DEFAULT_LIMITS) == [10000, 1000, 100, 10, 1]
    assert len(gs.settings_of(gs.DEFAULT_NMSES, gs.DEFAULT_THRESHS, gs.DEFAULT_LIMITS)) == 550
    assert gs.settings_of([1, 2], [3], [4, 5]) == [(1, 3, 4), (1, 3, 5), (2, 3, 4), (2, 3, 5)]
    assert gs.best_setting([{'mAP': 0.1}, {'mAP': 0.4}, {'mAP': 0.4}, {'mAP': 0.2}]) == 1


def test_tool_arguments(gs):
    tool = _tool()
    a = tool.parse_args(['--cfg', 'x.yaml'])
    assert (a.nms, a.thresh, a.max_per_image) == (list(gs.DEFAULT_NMSES), list(gs.DEFAULT_THRESHS),
                                                  list(gs.DEFAULT_LIMITS))
    assert a.collect is False and a.route is None and a.opts == []
    a = tool.parse_args(['--cfg', 'x.yaml', '--collect', '--nms', '0.5', '0.3', '--thresh', '1e-5,1e-3',
                         '--max-per-image', '100', '0', '--route', 'host', '--', 'TEST.WEIGHTS', 'w.pkl'])
    assert a.collect and a.nms == [0.5, 0.3] and a.thresh == [1e-5, 1e-3] and a.max_per_image == [100, 0]
    assert a.route == 'host' and a.opts == ['TEST.WEIGHTS', 'w.pkl'] and a.cfg_file == 'x.yaml'


def test_tool_writes_the_table_and_evaluates_the_winner(gs, tiny, cfgmod, monkeypatch, tmp_path):
    from detectron.core import test_engine_wsl as te
    from detectron.core.config import get_output_dir
    from detectron.utils.net_wsl import load_object
    tool = _tool()
    _recs, _names, classes, cands, oracle = tiny
    fx = vc.fixture()
    vc.register_tiny(monkeypatch, tmp_path, fx)
    opts = ['--', 'OUTPUT_DIR', str(tmp_path / 'out'), 'TEST.DATASETS', "('voc_2007_test',)",
            'MODEL.NUM_CLASSES', '4', 'TEST.BBOX_REG', 'False', 'NAWS.DEVICE_EVAL', 'False']
    grid = ['--nms', '0.5', '0.0', '--thresh', '1e-4', '--max-per-image', '0', '5']
    with pytest.raises(FileNotFoundError, match='--collect'):
        tool.main(grid + opts)
    out = os.path.join(get_output_dir('voc_2007_test', training=False), 'grid_search')
    te.save_detections(os.path.join(out, 'detections.pkl'), gs.boxes_of_setting(cands, 4, (1.1, -1e10, 0)),
                       None, None)
    cfgmod.reset_cfg()
    rows = tool.main(grid + opts)
    assert [(r['nms'], r['score_thresh'], r['detections_per_im']) for r in rows] == \
        [(0.5, 1e-4, 0), (0.5, 1e-4, 5), (0.0, 1e-4, 0), (0.0, 1e-4, 5)]
    for r in rows:
        ref = oracle.row(r['nms'], r['score_thresh'], r['detections_per_im'])
        assert (r['n_dets'], r['mAP'], r['mCorLoc']) == (ref['n_dets'], ref['mAP'], ref['mCorLoc'])
    with open(os.path.join(out, 'grid_search.csv'), newline='') as f:
        table = list(csv.reader(f))
    assert table[0] == ['nms', 'score_thresh', 'detections_per_im', 'n_dets', 'mAP', 'mCorLoc', 'AP_bird',
                        'AP_cat', 'AP_dog', 'CorLoc_bird', 'CorLoc_cat', 'CorLoc_dog']
    assert len(table) == 5 and [float(v) for v in table[2][:3]] == [0.5, 1e-4, 5]
    assert float(table[1][4]) == rows[0]['mAP'] and int(table[3][3]) == rows[2]['n_dets']
    saved = load_object(os.path.join(out, 'grid_search.pkl'))
    best = gs.best_setting(rows)
    assert saved['best'] == best and saved['header'] == table[0] and len(saved['rows']) == 4
    assert (saved['nmses'], saved['threshs'], saved['max_per_images']) == ([0.5, 0.0], [1e-4], [0, 5])
    # the winner went through the usual evaluation: its files are there and hold the winner's AP
    pr = load_object(os.path.join(out, 'dog_pr.pkl'))
    assert pr['ap'] == rows[best]['AP_dog']
    assert any(f.startswith('comp4') and f.endswith('_dog.txt') for f in os.listdir(out))


# ---- three wrong restatements ---------------------------------------------------------------------
def test_wrong_restatements_miss_the_oracle_on_their_named_cases(gs):
    """`>` for `>=` in the NMS, the fp32 score order for the rounded-confidence order, `> th` for
    `>= th` in the cut: each changes the result of the case built for it - and route='host'
    agrees with the oracle there."""
    def both(case, **wrong):
        recs, names, classes, cands, setting = case
        o = gr.Oracle(recs, names, classes, cands)
        right, bad = o.row(*setting), o.row(*setting, **wrong)
        row = gs.grid_search_arrays(recs, names, classes, cands, *[[v] for v in setting], route='host',
                                    curves=True)[0]
        gr.assert_row_matches(row, right, classes)
        return right, bad

    right, bad = both(gr.case_nms_on_threshold(), nms_ge=False)
    assert (right['n_dets'], bad['n_dets']) == (1, 2)
    assert right['classes']['c0']['tp'].tolist() == [0] and bad['classes']['c0']['tp'].tolist() == [0, 1]
    right, bad = both(gr.case_rounded_confidence_tie(), rounded_order=False)
    assert right['classes']['c0']['tp'].tolist() == [1, 0] and bad['classes']['c0']['tp'].tolist() == [0, 1]
    assert right['classes']['c0']['prec'].tolist() == [1.0, 0.5]
    assert bad['classes']['c0']['prec'].tolist() == [0.0, 0.5] and right['mAP'] != bad['mAP']
    right, bad = both(gr.case_tie_across_the_cut(), cut_ge=False)
    assert (right['n_dets'], bad['n_dets']) == (3, 1)


def test_tool_on_the_synthetic_stand_in(gs, cfgmod, tmp_path):
    """A dataset that is not on disk: the synthetic test images stand in, their first proposal is
    the image's one annotated object, and the table is written without result files."""
    from detectron.core import test_engine_wsl as te
    from detectron.core.config import cfg, get_output_dir
    tool = _tool()
    opts = ['--', 'OUTPUT_DIR', str(tmp_path / 'out'), 'MODEL.NUM_CLASSES', '4', 'TEST.BBOX_REG', 'False',
            'NAWS.DEVICE_EVAL', 'False', 'TEST.PROPOSAL_LIMIT', '30']
    args = ['--nms', '0.5', '--thresh', '1e-3', '--max-per-image', '0,3', '--num-images', '3']
    with pytest.raises(FileNotFoundError):
        tool.main(args + opts)
    roidb = te.get_roidb_and_dataset(te.SYNTHETIC, None, None)[0]
    assert len(roidb) == 3 and roidb[0]['boxes'].shape == (30, 4)
    rng = np.random.default_rng(8)
    all_boxes = [[[] for _ in roidb] for _ in range(4)]
    labels = []
    for i, e in enumerate(roidb):
        labels.append(int(e['gt_classes'][0]))
        for j in range(1, 4):
            sc = rng.uniform(0.01, 0.5, 30).astype(np.float32)
            if j == labels[-1]:
                sc[0] = 0.99                                   # the labelled box, found
            all_boxes[j][i] = np.hstack([e['boxes'], sc[:, None]]).astype(np.float32)
    out = os.path.join(get_output_dir(te.SYNTHETIC, training=False), 'grid_search')
    te.save_detections(os.path.join(out, 'detections.pkl'), all_boxes, None, None)
    cfgmod.reset_cfg()
    rows = tool.main(args + opts)
    assert [r['detections_per_im'] for r in rows] == [0, 3] and rows[0]['n_dets'] > rows[1]['n_dets'] == 9
    for r in rows:                                             # every labelled class is localised
        for j in set(labels):
            assert r['CorLoc_class%02d' % j] == 1.0 and r['AP_class%02d' % j] > 0
    assert sorted(os.listdir(out)) == ['detections.pkl', 'grid_search.csv', 'grid_search.pkl']
