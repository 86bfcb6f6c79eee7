"""Box-proposal recall on the CPU: the host route (detectron/datasets/json_dataset_evaluator.py)
and the tests' own literal loop (tests/box_proposals_ref.py) against the recorded run of the
reference's evaluate_box_proposals (tests/golden/reference_box_proposals.npz: 8 area ranges x
limits {None, 1, 3, 100}), bit for bit; task_evaluation's keys, order and log lines; the C ABI of
naws_proposal_match_fwd (error codes return before any launch); the wrapper's refusals; and
tools/eval_proposals.py end to end on the host route."""
import ctypes
import csv
import json
import logging
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest

import box_proposals_ref as bp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(a, l) for a in bp.AREAS for l in bp.FIXTURE_LIMITS]
REFERENCE_KEYS = ['AR@100', 'ARs@100', 'ARm@100', 'ARl@100', 'AR@1000', 'ARs@1000', 'ARm@1000', 'ARl@1000']


@pytest.fixture(scope='module')
def fx():
    return bp.fixture()


@pytest.fixture(scope='module')
def roidb(fx):
    return bp.fixture_roidb(fx)


@pytest.fixture(scope='module')
def cache():
    return {}


class _Dataset(object):
    name = 'toy_2007_test'


def test_fixture_holds_the_cases(fx, roidb):
    props = [int((e['gt_classes'] == 0).sum()) for e in roidb]
    gts = [int(((e['gt_classes'] > 0) & (e['is_crowd'] == 0)).sum()) for e in roidb]
    assert props[0] == 0 and gts[0] > 0 and gts[1] == 0 and props[1] > 0
    assert any(e['is_crowd'].any() for e in roidb)
    assert any(g > p > 0 for p, g in zip(props, gts))
    # every limit of the fixture has images above it and images below it
    assert max(props) > 100 and any(1 < p < 3 for p in props) and any(3 < p < 100 for p in props)
    areas = np.concatenate([e['seg_areas'][e['gt_classes'] > 0] for e in roidb])
    for bound in (32 ** 2, 96 ** 2, 128 ** 2):
        assert (areas == bound).any()
    assert any((e['boxes'] != np.round(e['boxes'])).any() for e in roidb)
    # a gt without proposals is counted and not recorded; an overlap of exactly 0.5 is recorded
    s = bp.fixture_stats(fx, 'all', None)
    assert s['num_pos'] == len(s['gt_overlaps']) + gts[0] and (s['gt_overlaps'] == 0.5).any()
    assert (s['gt_overlaps'] == 0).any()


@pytest.mark.parametrize('area,limit', SETTINGS)
def test_host_route_equals_the_reference(fx, roidb, area, limit):
    from detectron.datasets import json_dataset_evaluator as jde
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = jde.evaluate_box_proposals(None, roidb, area=area, limit=limit)
    assert sorted(got) == ['ar', 'gt_overlaps', 'num_pos', 'recalls', 'thresholds']
    bp.assert_same_stats(got, bp.fixture_stats(fx, area, limit))


@pytest.mark.parametrize('area,limit', SETTINGS)
def test_literal_loop_equals_the_reference(fx, roidb, cache, area, limit):
    bp.assert_same_stats(bp.evaluate(roidb, area, limit, cache=cache), bp.fixture_stats(fx, area, limit))


@pytest.mark.parametrize('mode', ['tie_high_gt', 'no_marking', 'limit_after'])
def test_wrong_matchings_differ_from_the_reference(fx, roidb, cache, mode):
    """The test of the test: the fixture's roidb tells each of three wrong rules from the right
    one - the tie broken towards the higher gt, every gt taking its best proposal without the
    one-to-one marking, the limit applied after the matching."""
    differs = 0
    for area, limit in SETTINGS:
        want = bp.fixture_stats(fx, area, limit)
        got = bp.evaluate(roidb, area, limit, mode=mode, cache=cache)
        assert got['num_pos'] == want['num_pos']
        differs += not np.array_equal(got['gt_overlaps'], want['gt_overlaps'])
    assert differs > 0


def test_num_pos_zero_gives_nan_as_the_reference():
    from detectron.datasets import json_dataset_evaluator as jde
    db = [bp.make_entry([], [], [], [], [[1, 1, 9, 9]])]
    with pytest.warns(RuntimeWarning):
        got = jde.evaluate_box_proposals(None, db)
    assert got['num_pos'] == 0 and np.isnan(got['recalls']).all() and np.isnan(got['ar'])


def test_task_evaluation_keys_order_and_values(fx, roidb, caplog):
    from detectron.datasets import task_evaluation
    with caplog.at_level(logging.INFO):
        res = task_evaluation.evaluate_box_proposals(_Dataset(), roidb, route='host')
    assert 'Box proposal recall: host route' in caplog.text
    assert list(res) == ['toy_2007_test'] and list(res['toy_2007_test']) == ['box_proposal']
    m = res['toy_2007_test']['box_proposal']
    assert list(m) == REFERENCE_KEYS
    # no image of the fixture has more than 1000 proposals: @1000 is the unlimited run
    for suffix, area in (('', 'all'), ('s', 'small'), ('m', 'medium'), ('l', 'large')):
        assert m['AR%s@100' % suffix] == fx['%s_100_ar' % area][()]
        assert m['AR%s@1000' % suffix] == fx['%s_none_ar' % area][()]
    ext = task_evaluation.evaluate_box_proposals(_Dataset(), roidb, limits=(3, None),
                                                 areas=('all', '96-128'), route='host')
    e = ext['toy_2007_test']['box_proposal']
    assert list(e) == ['AR@3', 'AR96-128@3', 'AR@all', 'AR96-128@all']
    assert e['AR96-128@3'] == fx['96-128_3_ar'][()] and e['AR@all'] == fx['all_none_ar'][()]
    with pytest.raises(AssertionError):
        task_evaluation.evaluate_box_proposals(_Dataset(), roidb, limits=(0,), route='host')
    with pytest.raises(AssertionError):
        task_evaluation.evaluate_box_proposals(_Dataset(), roidb, areas=('tiny',), route='host')


def test_log_lines(caplog):
    from collections import OrderedDict
    from detectron.datasets import task_evaluation
    res = OrderedDict([('toy_2007_test', OrderedDict([('box_proposal', OrderedDict(
        [('AR@100', 0.25), ('ARs@100', 0.5), ('AR@1000', 0.123456)]))]))])
    with caplog.at_level(logging.INFO, logger='detectron.datasets.task_evaluation'):
        task_evaluation.log_box_proposal_results(res)
    lines = [r.getMessage() for r in caplog.records if r.name == 'detectron.datasets.task_evaluation']
    assert lines == ['toy_2007_test', 'AR@100 : 0.250', 'ARs@100: 0.500', 'AR@1000: 0.123']


def test_default_route_without_a_gpu_is_the_host_route(cfgmod, monkeypatch):
    import torch
    from detectron.datasets import json_dataset_evaluator as jde
    assert cfgmod.cfg.NAWS.DEVICE_EVAL
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    assert not jde.device_route_available()
    cfgmod.cfg.NAWS.DEVICE_EVAL = False
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    assert not jde.device_route_available()


def test_flatten_roidb(roidb):
    from detectron.datasets import json_dataset_evaluator as jde
    boxes, box_off, gt, area, gt_off = jde.flatten_roidb(roidb)
    assert boxes.dtype == gt.dtype == area.dtype == np.float32 and box_off.dtype == gt_off.dtype == np.int64
    assert box_off[0] == gt_off[0] == 0 and box_off[-1] == len(boxes) and gt_off[-1] == len(gt) == len(area)
    for i, e in enumerate(roidb):
        p, g, a = bp.split_entry(e)
        assert np.array_equal(boxes[box_off[i]:box_off[i + 1]], p)
        assert np.array_equal(gt[gt_off[i]:gt_off[i + 1]], g)
        assert np.array_equal(area[gt_off[i]:gt_off[i + 1]], a)
    assert jde.flatten_roidb([])[1].tolist() == [0]


# ---- C ABI ------------------------------------------------------------------------------------
NAMES = ['naws_proposal_match_fwd', 'naws_proposal_match_max_grid', 'naws_proposal_match_workspace_bytes']


def test_symbols_are_declared_bound_and_exported():
    from naws_hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'naws.h')).read()
    L = lib.load()
    for name in NAMES:
        assert name in lib.ALL_SYMBOLS and name + '(' in hdr and hasattr(L, name)
    assert len(lib.PROTOTYPES['naws_proposal_match_fwd']) == 19
    assert L.naws_proposal_match_max_grid() >= 1
    one = L.naws_proposal_match_workspace_bytes(1, 1)
    assert one > 0 and one % 16 == 0
    assert L.naws_proposal_match_workspace_bytes(2000, 64) >= one
    assert L.naws_proposal_match_workspace_bytes(-1, 1) == -1 == L.naws_proposal_match_workspace_bytes(1, 2 ** 31)


def test_header_compiles_as_c_and_cpp(tmp_path):
    for cc, lang, ext in (('gcc', 'c', 'c'), ('g++', 'c++', 'cc')):
        src = tmp_path / ('use.' + ext)
        src.write_text('#include "naws.h"\nint use(void) { return naws_proposal_match_fwd(0, 0, 0, 0, 0, 0, 0, 0, '
                       '0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0) + naws_proposal_match_max_grid() + '
                       '(int)naws_proposal_match_workspace_bytes(1, 1); }\n')
        subprocess.check_call([cc, '-fsyntax-only', '-Wall', '-Werror', '-x', lang,
                               '-I', os.path.join(ROOT, 'include'), str(src)])


def test_every_error_code_returns_before_a_launch():
    """No GPU here: a launch would fail with NAWS_ERR_LAUNCH, so each expected code shows that the
    entry returned first.  The order is the header's: SHAPE, ARG, NULL, UNSUPPORTED, then the NaN
    bound and the workspace size."""
    from naws_hip import lib
    L = lib.load()
    vp = ctypes.c_void_p
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    a = (base + 15) // 16 * 16                         # on 16 bytes
    lo = (ctypes.c_float * 2)(0., 1024.)
    hi = (ctypes.c_float * 2)(1024., 1e10)
    lim = (ctypes.c_int32 * 2)(0, 100)
    f = lambda x: ctypes.cast(x, vp)
    big = L.naws_proposal_match_workspace_bytes(8, 4)

    def call(**kw):
        d = dict(boxes=a, box_off=a, P=8, gt=a, gt_area=a, gt_off=a, G=4, S=2, lo=f(lo), hi=f(hi), na=2,
                 lim=f(lim), nl=2, mp=8, mg=4, ws=a, wsb=big, out=a, stream=0)
        d.update(kw)
        return L.naws_proposal_match_fwd(*[vp(v) if k in ('boxes', 'box_off', 'gt', 'gt_area', 'gt_off', 'ws',
                                                          'out', 'stream') else v for k, v in d.items()])

    for kw in (dict(S=-1), dict(P=-1), dict(G=-2), dict(mp=-1), dict(mg=-1), dict(wsb=-1)):
        assert call(**kw) == lib.ERR_SHAPE, kw
    for kw in (dict(na=0), dict(nl=0), dict(nl=-3), dict(boxes=a + 4), dict(gt=a + 8), dict(ws=a + 4)):
        assert call(**kw) == lib.ERR_ARG, kw
    assert call(S=-1, na=0, boxes=0) == lib.ERR_SHAPE            # the order: SHAPE before ARG before NULL
    assert call(na=0, boxes=0) == lib.ERR_ARG
    for kw in (dict(lo=vp(0)), dict(hi=vp(0)), dict(lim=vp(0)), dict(box_off=0), dict(gt_off=0), dict(ws=0),
               dict(boxes=0), dict(gt=0), dict(gt_area=0), dict(out=0)):
        assert call(**kw) == lib.ERR_NULL, kw
    assert call(boxes=0, P=0, gt=0, gt_area=0, out=0, G=0) == lib.OK      # nothing to read or write
    assert call(S=0) == lib.OK
    for kw in (dict(na=65), dict(nl=65), dict(P=2 ** 31), dict(G=2 ** 31), dict(S=2 ** 31)):
        assert call(**kw) == lib.ERR_UNSUPPORTED, kw
    nan_lo = (ctypes.c_float * 2)(0., float('nan'))
    assert call(lo=f(nan_lo)) == lib.ERR_ARG
    assert call(wsb=big - 16) == lib.ERR_SHAPE
    assert call(mp=10 ** 6, mg=10 ** 4) == lib.ERR_SHAPE              # the workspace no longer suffices


def test_wrapper_refuses_bad_offsets_and_strided_views():
    """Layout and offsets are checked before residence, so the refusals show without a GPU; inputs
    that pass them all are then refused as host tensors (no CPU path)."""
    import torch
    from naws_hip import lib, ops
    boxes = torch.zeros((6, 4))
    gt = torch.zeros((3, 4))
    area = torch.zeros(3)
    off = lambda *v: torch.tensor(v, dtype=torch.int64)
    good = dict(boxes=boxes, box_off=off(0, 4, 6), gt=gt, gt_area=area, gt_off=off(0, 1, 3))
    run = lambda **kw: ops.proposal_match(area_lo=[0.], area_hi=[1e10], limits=[0], **dict(good, **kw))
    for kw in (dict(box_off=off(0, 4, 5)), dict(box_off=off(0, 4, 7)), dict(box_off=off(1, 4, 6)),
               dict(box_off=off(0, 7, 6)), dict(gt_off=off(0, 2, 1)), dict(gt_off=off(0, 1, 2)),
               dict(gt_off=off(0, 3)), dict(gt_area=torch.zeros(4)), dict(boxes=torch.zeros((6, 5))),
               dict(out=torch.zeros((2, 3)))):
        with pytest.raises(lib.NawsError) as e:
            run(**kw)
        assert e.value.code == lib.ERR_SHAPE, kw
    for kw in (dict(boxes=torch.zeros((6, 8))[:, :4]), dict(boxes=torch.zeros((12, 4))[::2]),
               dict(gt=torch.zeros((4, 3)).t()[:3]), dict(gt_area=torch.zeros(6)[::2]),
               dict(box_off=off(0, 0, 4, 0, 6)[::2]), dict(out=torch.zeros((1, 6))[:, ::2])):
        with pytest.raises(ValueError):
            run(**kw)
    for kw in (dict(boxes=boxes.double()), dict(box_off=off(0, 4, 6).int()), dict(gt_area=area.half())):
        with pytest.raises(TypeError):
            run(**kw)
    with pytest.raises(TypeError, match='HIP device tensor'):
        run()
    with pytest.raises(lib.NawsError):
        ops.proposal_match(area_lo=[0., 1.], area_hi=[1e10], limits=[0], **good)


# ---- the tool -----------------------------------------------------------------------------------
def _toy_files(tmp_path, roidb):
    """A COCO-format json and a proposal pickle holding the fixture's roidb (integer-valued gt:
    the json's xywh boxes pass through the loader's clipping), one image per entry that has gt."""
    images, anns, pb, ps, pi = [], [], [], [], []
    aid = 0
    for i, e in enumerate(roidb[:7]):
        iid = 100 + i
        images.append(dict(id=iid, file_name='im_%03d.jpg' % iid, height=1000, width=1000))
        isgt = e['gt_classes'] > 0
        for b, c, crowd, ar in zip(e['boxes'][isgt], e['gt_classes'][isgt], e['is_crowd'][isgt],
                                   e['seg_areas'][isgt]):
            aid += 1
            anns.append(dict(id=aid, image_id=iid, category_id=int(c), iscrowd=int(crowd), area=float(ar),
                             bbox=[float(b[0]), float(b[1]), float(b[2] - b[0] + 1), float(b[3] - b[1] + 1)],
                             segmentation=[]))
        p = e['boxes'][~isgt]
        pb.append(p.astype(np.float32))
        ps.append(np.linspace(1, 0.5, len(p), dtype=np.float32).reshape(-1, 1))
        pi.append(iid)
    cats = [dict(id=k, name='c%02d' % k) for k in range(1, 10)]
    annf = tmp_path / 'toy.json'
    annf.write_text(json.dumps(dict(images=images, annotations=anns, categories=cats)))
    pf = tmp_path / 'props.pkl'
    with open(str(pf), 'wb') as f:
        pickle.dump(dict(boxes=pb, scores=ps, indexes=pi), f, 2)
    imdir = tmp_path / 'images'
    imdir.mkdir()
    for im in images:                                   # the loader only asks that they exist
        (imdir / im['file_name']).write_bytes(b'')
    return str(imdir), str(annf), str(pf)


def _run_tool(argv, imdir, annf):
    registry = {'toy_2007_test': {'image_directory': imdir, 'annotation_file': annf}}
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1', NAWS_DATASET_REGISTRY=json.dumps(registry))
    return subprocess.run([sys.executable, os.path.join(ROOT, 'na-fwebsod_amd', 'tools', 'eval_proposals.py')]
                          + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_eval_proposals_tool_host_route_end_to_end(tmp_path, roidb, cfgmod):
    from detectron.datasets import dataset_catalog, json_dataset_evaluator as jde
    from detectron.datasets.json_dataset_wsl import JsonDataset
    imdir, annf, pf = _toy_files(tmp_path, roidb)
    out = tmp_path / 'out'
    r = _run_tool(['--dataset', 'toy_2007_test',
                   '--proposal-file', pf, '--route', 'host', '--output-dir', str(out),
                   '--limits', '3', '100', '--areas', 'all', 'small', '96-128'], imdir, annf)
    assert r.returncode == 0, r.stdout
    assert 'Box proposal recall: host route' in r.stdout
    # what the tool evaluated is what the loader makes of the files
    dataset_catalog.register('toy_2007_test', imdir, annf)
    want_db = JsonDataset('toy_2007_test').get_roidb(gt=True, proposal_file=pf)
    with open(str(out / 'rpn_proposal_recall.pkl'), 'rb') as f:
        saved = pickle.load(f)
    m = saved['toy_2007_test']['box_proposal']
    assert list(m) == ['AR@3', 'ARs@3', 'AR96-128@3', 'AR@100', 'ARs@100', 'AR96-128@100']
    with open(str(out / 'proposal_recall.csv')) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ['area', 'limit', 'num_pos', 'ar'] + ['recall@%.2f' % t for t in bp.THRESHOLDS]
    assert [(r_[0], r_[1]) for r_ in rows[1:]] == [(a, str(l)) for l in (3, 100) for a in ('all', 'small', '96-128')]
    for row in rows[1:]:
        s = jde.evaluate_box_proposals(None, want_db, area=row[0], limit=int(row[1]))
        assert int(row[2]) == s['num_pos'] and float(row[3]) == s['ar']
        assert [float(v) for v in row[4:]] == s['recalls'].tolist()
        key = 'AR%s@%s' % ({'all': '', 'small': 's'}.get(row[0], row[0]), row[1])
        assert m[key] == s['ar'] and '%s: %.3f' % (key.ljust(12), s['ar']) in r.stdout
    assert any(int(row[2]) > 0 and float(row[3]) > 0 for row in rows[1:])


def test_eval_proposals_tool_names_the_missing_file(tmp_path, roidb):
    imdir, annf, pf = _toy_files(tmp_path, roidb)
    gone = str(tmp_path / 'nowhere.pkl')
    r = _run_tool(['--dataset', 'toy_2007_test',
                   '--proposal-file', gone, '--route', 'host', '--output-dir', str(tmp_path / 'o')], imdir, annf)
    assert r.returncode != 0 and gone in r.stdout and 'Traceback' not in r.stdout
    gone_json = str(tmp_path / 'nowhere.json')
    r = _run_tool(['--dataset', 'toy_2007_test',
                   '--proposal-file', pf, '--route', 'host', '--output-dir', str(tmp_path / 'o')], imdir,
                  gone_json)
    assert r.returncode != 0 and gone_json in r.stdout and 'Traceback' not in r.stdout
