"""Test-time grid search on the GPU: naws_nms_multi_fwd against core/test_wsl.py::nms per threshold,
naws_grid_cut_fwd against numpy, and grid_search(route='device') against the oracle of
tests/grid_search_ref.py with the equalities of tests/test_gpu_voc_eval.py (n_dets, tp / fp flags,
rec, prec, the 11-point AP and CorLoc bit-equal; the area AP within (D + 2) * 2^-52).

Shapes, each the smallest that reaches its branch: lists of 0, 1, 63, 64, 65 and 300 boxes and one
of 2049 (one more than the LDS form holds: the form that walks in memory), all in ONE launch;
exact copies of boxes (IoU exactly 1), tied scores, an IoU of exactly 0.5; T = 1, 11 and 32
thresholds, 0.0 and 1.0 among them.  The host references are computed once per module."""
import numpy as np
import pytest
import torch

import grid_search_ref as gr
import guard
import voc_eval_cases as vc

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 300, 2049, 0, 7)
HALF_UP = float(np.nextafter(np.float32(0.5), np.float32(1)))
# 32 thresholds; the first 11 are the reference's list, the first one alone is T = 1
THR32 = [1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.0, HALF_UP, 0.05, 0.15, 0.25, 0.35, 0.45,
         0.55, 0.65, 0.75, 0.85, 0.95, 0.99, 0.01, 0.5, 1.0, 0.0, 0.33, 0.66, 0.125, 0.875, 0.999]
GRID = ([1.0, 0.5, 0.0], [1e-10, 1e-4, 1e-1], [0, 20, 1])


def _lists():
    """Boxes of every list in visiting order (descending score, ties by row) + offsets."""
    rng = np.random.default_rng(16)
    boxes, off = [], [0]
    for n in LENGTHS:
        span = 60 if n < 1000 else 150
        xy = rng.integers(0, span, (n, 2)).astype(np.float32) + rng.integers(0, 4, (n, 2)) / np.float32(4)
        wh = rng.integers(6, 50, (n, 2)).astype(np.float32)
        b = np.hstack([xy, xy + wh]).astype(np.float32)
        if n > 8:
            b[n // 2::3] = b[rng.integers(0, n // 2, len(b[n // 2::3]))]    # exact copies: IoU = 1
        boxes.append(b)
        off.append(off[-1] + n)
    return np.concatenate(boxes), np.array(off, np.int64)


@pytest.fixture(scope='module')
def lists():
    """(boxes, offsets, kept [32][total] bool): test_wsl.nms per threshold and list, once."""
    from detectron.core import test_wsl
    boxes, off = _lists()
    kept = np.zeros((len(THR32), len(boxes)), bool)
    for a, b in zip(off[:-1], off[1:]):
        n = int(b - a)
        # tied scores in blocks of three: the stable sort keeps the list's own order
        sc = (1.0 - (np.arange(n) // 3) / np.float32(max(n, 1))).astype(np.float32)
        dets = np.hstack([boxes[a:b], sc[:, None]])
        for t, thr in enumerate(THR32):
            with np.errstate(divide='ignore', invalid='ignore'):
                kept[t, a + np.asarray(test_wsl.nms(dets, thr), np.int64)] = True
    return boxes, off, kept


def _nms_multi_guarded(dev, boxes, off, thr):
    from naws_hip import lib as L
    bd = torch.from_numpy(boxes).to(dev)
    od = torch.from_numpy(off).to(dev)
    out = guard.carve((max(len(boxes), 1),), torch.int32, dev)
    status = guard.carve((max(len(off) - 1, 1),), torch.int32, dev)
    th = np.ascontiguousarray(thr, np.float32)
    L.call('naws_nms_multi_fwd', bd.data_ptr(), od.data_ptr(), len(boxes), len(off) - 1, th.ctypes.data,
           len(th), out.t.data_ptr(), status.t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out.check('survive'); status.check('status')
    return out.t[:len(boxes)].cpu().numpy().view(np.uint32), status.t[:len(off) - 1].cpu().numpy()


@pytest.mark.parametrize('T', [1, 11, 32])
def test_nms_multi_equals_host_nms_at_every_threshold(dev, lists, T):
    boxes, off, kept = lists
    words, status = _nms_multi_guarded(dev, boxes, off, THR32[:T])
    assert (status == 0).all()
    for t in range(T):
        got = ((words >> np.uint32(t)) & 1).astype(bool)
        bad = np.flatnonzero(got != kept[t])
        assert bad.size == 0, (T, t, THR32[t], bad[:5])
    assert T == 32 or (words >> np.uint32(T)).max() == 0                      # bits T.. stay 0
    # the references are not vacuous: thresholds differ, copies go at 1.0, 0.0 keeps one per list
    assert kept[0].sum() < len(boxes) and kept[10].sum() == sum(1 for n in LENGTHS if n > 0)
    assert len({int(k.sum()) for k in kept[:11]}) >= 8


def test_nms_multi_ops_wrapper_and_repeatability(dev, lists):
    from naws_hip import ops
    boxes, off, kept = lists
    bd, od = torch.from_numpy(boxes).to(dev), torch.from_numpy(off).to(dev)
    a, sa = ops.nms_multi(bd, od, THR32[:11])
    b, sb = ops.nms_multi(bd, od, THR32[:11])
    assert torch.equal(a, b) and torch.equal(sa, sb) and a.dtype == torch.int32
    w = a.cpu().numpy().view(np.uint32)
    assert np.array_equal(((w >> np.uint32(5)) & 1).astype(bool), kept[5])


def test_iou_exactly_on_the_threshold_falls_as_in_the_reference(dev):
    """(0,0,9,14) / (0,5,9,19): IoU = 100 / 200 = 0.5 exactly.  Suppressed at 0.5 (`>=`), kept at
    the next fp32 above 0.5 and at 1.0; at 0.0 everything behind the first box goes.  An exact copy
    (IoU 1) is suppressed at 1.0."""
    boxes = np.array([[0, 0, 9, 14], [0, 5, 9, 19], [0, 0, 9, 14]], np.float32)
    words, status = _nms_multi_guarded(dev, boxes, np.array([0, 3], np.int64), [0.5, HALF_UP, 0.0, 1.0])
    assert status.tolist() == [0]
    assert words.tolist() == [0b1111, 0b1010, 0b0000]


def test_nms_multi_reports_bad_lists_and_touches_nothing(dev):
    n = 16385                                                        # one more than a list may hold
    boxes = np.tile(np.array([[0, 0, 9, 9]], np.float32), (n, 1))
    from naws_hip import lib as L
    bd = torch.from_numpy(boxes).to(dev)
    th = np.array([0.5], np.float32)
    for off, want in (([0, n], [-3]), ([0, 5, 3, n + 1, 8], [0, -2, -2, -2]), ([-1, 4], [-2])):
        od = torch.tensor(off, dtype=torch.int64, device=dev)
        out = guard.carve((n,), torch.int32, dev)
        status = guard.carve((len(off) - 1,), torch.int32, dev)
        L.call('naws_nms_multi_fwd', bd.data_ptr(), od.data_ptr(), n, len(off) - 1, th.ctypes.data, 1,
               out.t.data_ptr(), status.t.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out.check('survive'); status.check('status')
        assert status.t.tolist() == want
        first = 5 if want[0] == 0 else 0                            # the one good list: five copies
        assert out.t[:first].tolist() == [1, 0, 0, 0, 0][:first]
        assert guard.holds_sentinel(out.t[first:])                  # a refused list wrote nothing


def _cut_case():
    """Images in descending score: no candidate, one, no survivor at threshold 1, a tie across
    the cut, 64 / 65 / 200 candidates."""
    rng = np.random.default_rng(17)
    words, scores, off = [], [], [0]
    for n in (0, 1, 5, 6, 64, 65, 200):
        sc = np.sort(np.round(10.0 ** rng.uniform(-6, 0, n), 3).astype(np.float32))[::-1]
        w = rng.integers(0, 8, n).astype(np.uint32)
        if n == 5:
            w &= np.uint32(0b101)                                    # nobody survives at t = 1
        if n == 6:
            sc = np.array([0.9, 0.5, 0.5, 0.5, 0.2, 0.1], np.float32)
            w[:] = 7
        words.append(w); scores.append(sc); off.append(off[-1] + n)
    return np.concatenate(words), np.concatenate(scores), np.array(off, np.int64)


def test_grid_cut_equals_numpy(dev):
    from naws_hip import lib as L
    words, scores, off = _cut_case()
    sthr, limits, T = [1e-6, 1e-3, 0.3, 0.5], [0, 1, 2, 3, 64, 65, 1000], 3
    n_img = len(off) - 1
    count = guard.carve((n_img * T, len(sthr)), torch.int32, dev)
    kth = guard.carve((n_img * T, len(limits)), torch.float32, dev)
    status = guard.carve((n_img,), torch.int32, dev)
    wd = torch.from_numpy(words.view(np.int32)).to(dev)
    sd, od = torch.from_numpy(scores).to(dev), torch.from_numpy(off).to(dev)
    s_h, l_h = np.array(sthr, np.float32), np.array(limits, np.int32)
    L.call('naws_grid_cut_fwd', wd.data_ptr(), sd.data_ptr(), od.data_ptr(), len(words), n_img, T,
           s_h.ctypes.data, len(sthr), l_h.ctypes.data, len(limits), count.t.data_ptr(), kth.t.data_ptr(),
           status.t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for g, what in ((count, 'count'), (kth, 'kth'), (status, 'status')):
        g.check(what)
    assert status.t.tolist() == [0] * n_img
    got_c = count.t.cpu().numpy().reshape(n_img, T, len(sthr))
    got_k = kth.t.cpu().numpy().reshape(n_img, T, len(limits))
    for i, (a, b) in enumerate(zip(off[:-1], off[1:])):
        ref_c, ref_k = gr.cut_tables(words[a:b], scores[a:b], T, sthr, limits)
        assert np.array_equal(got_c[i], ref_c), i
        assert np.array_equal(got_k[i], ref_k), i
    assert (got_c[2, 1] == 0).all() and np.isneginf(got_k[2, 1]).all()       # no survivor
    assert np.isneginf(got_k[3, 0, 6]) and got_c[3, 0, 0] == 6                # a limit above the count
    assert got_k[3, 0, 2] == np.float32(0.5) and got_k[3, 0, 3] == np.float32(0.5)   # the tie: L = 2, 3
    # the ops wrapper, twice
    from naws_hip import ops
    a = ops.grid_cut(wd, sd, od, T, sthr, limits)
    b = ops.grid_cut(wd, sd, od, T, sthr, limits)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(a[0].cpu().numpy(), got_c) and np.array_equal(a[1].cpu().numpy(), got_k)
    # an image whose offsets leave the array is reported and writes nothing
    bad = od.clone()
    bad[3] = len(words) + 1
    c2, k2, st = ops.grid_cut(wd, sd, bad, T, sthr, limits)
    assert st.tolist()[:4] == [0, 0, -2, -2] and not c2[2:4].any() and not k2[2:4].any()


# ---- the whole sweep ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cases():
    out = {}
    for name, case in (('tiny', gr.tiny_case()), ('synthetic', gr.synthetic_case())):
        recs, names, classes, cands = case
        out[name] = (recs, names, classes, cands, gr.Oracle(recs, names, classes, cands))
    return out


@pytest.fixture
def gs(cfgmod):
    cfgmod.cfg.TEST.BBOX_REG = False
    from detectron.core import grid_search_wsl
    return grid_search_wsl


@pytest.mark.parametrize('name', ['tiny', 'synthetic'])
def test_device_route_equals_the_oracle(dev, gs, cases, name):
    recs, names, classes, cands, oracle = cases[name]
    if name == 'synthetic':
        assert len(names) == 30 and len(classes) == 4 and max(len(b) for _s, b in cands) == 300
    rows = gs.grid_search_arrays(recs, names, classes, cands, *GRID, route='device', curves=True)
    assert [(r['nms'], r['score_thresh'], r['detections_per_im']) for r in rows] == \
        [(a, b, c) for a in GRID[0] for b in GRID[1] for c in GRID[2]]
    for r in rows:
        gr.assert_row_matches(r, oracle.row(r['nms'], r['score_thresh'], r['detections_per_im']), classes)
    assert len({r['n_dets'] for r in rows}) > 5 and max(r['mAP'] for r in rows) > 0
    again = gs.grid_search_arrays(recs, names, classes, cands, *GRID, route='device', curves=True)
    for a, b in zip(rows, again):                                    # two device runs: bit for bit
        assert [a[k] for k in a if k != 'curves'] == [b[k] for k in b if k != 'curves']
        for c in classes[1:]:
            for key in ('tp', 'fp', 'rec', 'prec'):
                assert np.array_equal(a['curves'][c][key], b['curves'][c][key], equal_nan=True)
            assert a['curves'][c]['ap_area'] == b['curves'][c]['ap_area'] or \
                np.isnan(a['curves'][c]['ap_area'])


def test_device_route_on_the_named_cases_and_in_small_chunks(dev, gs, cases, monkeypatch):
    """The three cases a wrong restatement misses, and the tiny sweep again with one setting per
    evaluation chunk (the chunking changes nothing)."""
    for case in (gr.case_nms_on_threshold(), gr.case_rounded_confidence_tie(), gr.case_tie_across_the_cut()):
        recs, names, classes, cands, setting = case
        row = gs.grid_search_arrays(recs, names, classes, cands, *[[v] for v in setting], route='device',
                                    curves=True)[0]
        gr.assert_row_matches(row, gr.Oracle(recs, names, classes, cands).row(*setting), classes)
    recs, names, classes, cands, oracle = cases['tiny']
    monkeypatch.setattr(gs, '_CHUNK_ELEMS', 1)
    timings = {}
    rows = gs.grid_search_arrays(recs, names, classes, cands, *GRID, route='device', curves=True,
                                 timings=timings)
    assert timings['settings_per_chunk'] == 1 and timings['settings'] == 27
    for r in rows:
        gr.assert_row_matches(r, oracle.row(r['nms'], r['score_thresh'], r['detections_per_im']), classes)


def test_default_route_is_the_device_route(dev, gs, cases, caplog):
    import logging
    recs, names, classes, cands, oracle = cases['tiny']
    with caplog.at_level(logging.INFO):
        rows = gs.grid_search_arrays(recs, names, classes, cands, [0.5], [1e-4], [5])
    assert 'Grid search: device route' in caplog.text
    ref = oracle.row(0.5, 1e-4, 5)
    assert (rows[0]['n_dets'], rows[0]['mAP']) == (ref['n_dets'], ref['mAP'])
