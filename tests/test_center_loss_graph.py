"""WSL.CENTER_LOSS, the multi-centre feature loss, without a GPU: the builders against the op trace
recorded from the reference (tests/golden/make_golden_center_loss.py), the backward plan, the cfg
switches and knobs, and the numpy restatement the GPU tests compare against
(tests/center_loss_ref.py) on a hand-computed case."""
import json
import os

import numpy as np
import pytest

import center_loss_ref as clr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_center_loss.json')))
NA = ['NUM_GPUS', 4, 'WSL.CENTER_LOSS', True]
PLAIN = NA + ['WEBLY.WEBLY_ON', False, 'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head']
STATE = ('center_feature', 'center_feature_g', 'center_feature_n_u')


def _norm_ops(ops_, want):
    """The recorded form of an op list: Conv / FC made by the model helper are recorded with their
    data input only; hidden outputs (leading underscore) of Dropout / CenterLoss are ours."""
    out = []
    for o, w in zip(ops_, want):
        ins, outs, args = list(o.inputs), list(o.outputs), dict(o.args)
        if o.type in ('Conv', 'FC'):
            ins = ins[:len(w[1])]
        if o.type in ('Dropout', 'CenterLoss'):
            assert all(n.startswith('_') for n in outs[len(w[2]):]), outs
            outs = outs[:len(w[2])]
        out.append([o.type, ins, outs, args])
    return json.loads(json.dumps(out))


@pytest.mark.parametrize('extra,key,n', [(NA, 'na_wsddn_center_train', 105),
                                         (PLAIN, 'wsl_center_train', 55)])
def test_center_loss_builders_reproduce_reference_trace(cfgmod, extra, key, n):
    c = cfgmod
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(extra)
    c.assert_and_infer_cfg(make_immutable=False)
    import detectron.modeling.model_builder_wsl as mb
    m = mb.create(c.cfg.MODEL.TYPE, train=True)
    want = GOLD[key]
    assert len(want['ops']) == n and len(m.net.ops) == n
    got = _norm_ops(m.net.ops, want['ops'])
    assert [g[:3] for g in got] == [w[:3] for w in want['ops']]
    for g, w in zip(got, want['ops']):
        if g[0] in ('CenterLoss', 'ConstantFill', 'Softmax', 'Transpose', 'ReduceSum',
                    'CrossEntropyWithLogits', 'WeightedCrossEntropyWithLogits'):
            assert g[3] == w[3], g
    cl = [g for g in got if g[0] == 'CenterLoss']
    assert len(cl) == 1
    assert cl[0][1] == ['labels_oh', 'rois_pred', 'drop7'] + list(STATE)
    assert cl[0][2] == ['loss_center', 'D', 'S']
    assert cl[0][3] == {'max_iter': 35000, 'top_k': 10, 'display': 320, 'update': 32}
    # the seed of the loss gradient: ConstantFill 0.4096, no 1 / NUM_GPUS factor
    seed = [g for g in got if g[0] == 'ConstantFill' and g[2] == ['loss_center_grad']]
    assert len(seed) == 1 and seed[0][3] == {'value': 0.4096}
    assert m.losses == want['losses'] and m.metrics == want['metrics']
    assert 'loss_center' in m.losses
    # parameters: the reference's names, shapes and initialisers
    assert [p['name'] for p in want['params']] == list(STATE)
    for p in want['params']:
        assert list(m.param_shapes[p['name']]) == p['shape']
        kind, args = m.param_inits[p['name']]
        assert [kind, dict(args)] == p['initializer']
    assert want['params'][0]['shape'] == [20, 5, 4096]
    # the knobs stand for the reference's keys at the reference's values
    assert GOLD['cfg'] == {'CENTER_LOSS_NUMBER': c.cfg.NAWS.CENTER_LOSS_NUMBER,
                           'CENTER_LOSS_TOP_K': c.cfg.NAWS.CENTER_LOSS_TOP_K,
                           'CSC_MAX_ITER': c.cfg.NAWS.CENTER_LOSS_MAX_ITER}


def test_center_loss_cfg_switches(cfgmod):
    c = cfgmod
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(NA)
    c.assert_and_infer_cfg(make_immutable=False)           # an accepted switch now
    c.merge_cfg_from_list(['WSL.PCL', True])
    with pytest.raises(NotImplementedError):
        c.assert_and_infer_cfg(make_immutable=False)       # the other methods still are not
    c.merge_cfg_from_list(['WSL.PCL', False, 'NAWS.CENTER_LOSS_NUMBER', 3, 'NAWS.CENTER_LOSS_TOP_K', 4,
                           'NAWS.CENTER_LOSS_MAX_ITER', 7])
    import detectron.modeling.model_builder_wsl as mb
    m = mb.create(c.cfg.MODEL.TYPE, train=True)
    assert m.param_shapes['center_feature'] == (20, 3, 4096)
    assert m.param_shapes['center_feature_n_u'] == (20, 3)
    op = [o for o in m.net.ops if o.type == 'CenterLoss'][0]
    assert op.args['top_k'] == 4 and op.args['max_iter'] == 7


def test_center_loss_backward_plan(cfgmod):
    c = cfgmod
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(NA)
    import detectron.modeling.model_builder_wsl as mb
    m = mb.create(c.cfg.MODEL.TYPE, train=True)
    g = [o for o in m.grad_ops if o.type == 'CenterLossGradient']
    assert len(g) == 1
    g = g[0]
    assert g.outputs == ['drop7_grad']                     # input 2 only (center_loss_op.cc:55-58)
    assert g.args['_gin'] == [None, None, 'drop7_grad', None, None, None]
    assert g.args['_gout'][0] == 'loss_center_grad'
    # it receives D, S and the hidden selection next to the op's inputs
    assert g.inputs == ['labels_oh', 'rois_pred', 'drop7'] + list(STATE) + \
        ['loss_center', 'D', 'S', '_center_picks']
    # it runs first and writes; the two fc8 FCs that read drop7 then ADD to drop7_grad
    order = [i for i, o in enumerate(m.grad_ops) if 'drop7_grad' in o.outputs]
    assert m.grad_ops[order[0]] is g and not g.args['_accumulate'][2]
    fcs = [m.grad_ops[i] for i in order[1:]]
    assert sorted(o.inputs[1] for o in fcs) == ['fc8c_w', 'fc8d_w']
    for o in fcs:
        assert o.type == 'FCGradient' and o.inputs[0] == 'drop7' and o.args['_accumulate'][0]
    # the state blobs are parameters of the net that SGD leaves alone
    for p in STATE:
        assert p in m.params and p not in m.param_to_grad and p not in m.TrainableParams()
    # the switch off: the plan is the one it was
    c.merge_cfg_from_list(['WSL.CENTER_LOSS', False])
    m0 = mb.create(c.cfg.MODEL.TYPE, train=True)
    assert not [o for o in m0.net.ops if o.type == 'CenterLoss']
    assert not [p for p in STATE if p in m0.params]
    off = [i for i, o in enumerate(m0.grad_ops) if 'drop7_grad' in o.outputs]
    assert not m0.grad_ops[off[0]].args['_accumulate'][0]


def test_reference_format_cfg_dump_ignores_the_knobs(cfgmod):
    """The cfg string of weights / detections files is the reference's format: it has
    WSL.CENTER_LOSS and none of the NAWS keys, so the recorded dump
    (tests/golden/reference_cfg_load.json) stays valid."""
    import detectron.utils.env as envu
    c = cfgmod
    c.merge_cfg_from_file(YAML)
    before = envu.yaml_dump(c.cfg, reference_format=True)
    c.merge_cfg_from_list(['NAWS.CENTER_LOSS_NUMBER', 3, 'NAWS.CENTER_LOSS_TOP_K', 4,
                           'NAWS.CENTER_LOSS_MAX_ITER', 7])
    after = envu.yaml_dump(c.cfg, reference_format=True)
    assert before == after
    assert 'CENTER_LOSS: false' in before.replace('False', 'false')
    for k in ('CENTER_LOSS_NUMBER', 'CENTER_LOSS_TOP_K', 'CENTER_LOSS_MAX_ITER', 'CSC_MAX_ITER'):
        assert k not in before


def test_restatement_known_answer():
    """C = 2, M = 2, top_k = 2, Dm = 3, R = 4, worked out by hand.
    Scores: class 0 has the tie 0.7 at rois 1, 2 -> picks {1, 2}; class 1 (label exactly 0.5) the
    tie 0.9 at rois 0, 2 -> {0, 2}: roi 2 serves both.
    Class 0: centre 0 = 0 gives |(0,2,0)|^2 + |(0,0,2)|^2 = 8, centre 1 = (0,1,0) gives
    |(0,1,0)|^2 + |(0,-1,2)|^2 = 6 -> S = 1.  Class 1: both centres (1,0,1) give
    |(0,0,-1)|^2 + |(-1,0,1)|^2 = 3 -> the first, S = 0.  L = (6 + 3) / 2 / 2 / 3 / 2 = 0.375."""
    X = np.array([[1.0, 0.5]], np.float32)
    P = np.array([[0.1, 0.9], [0.7, 0.2], [0.7, 0.9], [0.3, 0.5]], np.float32)
    F = np.array([[1, 0, 0], [0, 2, 0], [0, 0, 2], [5, 5, 5]], np.float32)
    CF = np.array([[[0, 0, 0], [0, 1, 0]], [[1, 0, 1], [1, 0, 1]]], np.float64)
    dCF = np.full((2, 2, 3), 7.0)            # loaded state that the first call must zero
    ndCF = np.full((2, 2), 7.0)
    op = clr.CenterLossRef(top_k=2, update=2, lr=0.5, max_iter=3)
    L, D, S, picks = op.forward(X, P, F, CF)
    assert picks.tolist() == [[1, 2], [0, 2]]
    assert S.tolist() == [1.0, 0.0]
    assert D.dtype == np.float32
    assert D.tolist() == [[[0, 1, 0], [0, -1, 2]], [[0, 0, -1], [-1, 0, 1]]]
    assert L == 0.375
    assert op.counts.tolist() == [[0, 1], [1, 0]]
    # dL = 1.2: alpha = 1.2 / 2 / 2 / 3 = 0.1
    dF = op.gradient(D, S, picks, 1.2, 4, CF, dCF, ndCF)
    np.testing.assert_allclose(dF, [[0, 0, -.1], [0, .1, 0], [-.1, -.1, .3], [0, 0, 0]], atol=1e-15)
    assert ndCF.tolist() == [[0, 1], [1, 0]]
    assert dCF.tolist() == [[[0, 0, 0], [0, 0, -2]], [[1, 0, 0], [0, 0, 0]]]
    assert not op.acc_dCF.any() and not op.acc_ndCF.any()       # the loaded 7s are gone
    # call 2 (update = 2): the accumulators take call 1's contribution - doubled, as a two-rank sum
    # would - and the centres move by it; call 2's own contribution is not in that update
    dCF *= 2
    ndCF *= 2
    L2, D2, S2, picks2 = op.forward(X, P, F, CF)
    assert L2 == 0.375
    op.gradient(D2, S2, picks2, 1.2, 4, CF, dCF, ndCF)
    # CF[0,1] -= 0.5 / (2 * 2 + 1) * (0,0,-4);  CF[1,0] -= 0.5 / 5 * (2,0,0)
    np.testing.assert_allclose(CF, [[[0, 0, 0], [0, 1, 0.4]], [[0.8, 0, 1], [1, 0, 1]]], atol=1e-15)
    assert not op.acc_dCF.any() and not op.acc_ndCF.any()
    assert ndCF.tolist() == [[0, 1], [1, 0]]                    # this call's, still to be taken in
    # call 3: taken in, no update; call 4 is past max_iter = 3: nothing moves, dF = 0
    L3, D3, S3, picks3 = op.forward(X, P, F, CF)
    op.gradient(D3, S3, picks3, 1.2, 4, CF, dCF, ndCF)
    assert op.acc_ndCF.tolist() == [[0, 1], [1, 0]]
    L4, D4, S4, picks4 = op.forward(X, P, F, CF)
    keep = dCF.copy()
    dF4 = op.gradient(D4, S4, picks4, 1.2, 4, CF, dCF, ndCF)
    assert L4 == 0.0 and not D4.any() and S4.tolist() == [-1, -1] and (picks4 == -1).all()
    assert not dF4.any() and np.array_equal(dCF, keep)
    # label 0.49, the ignored class, fewer rois than top_k: inactive
    assert clr.select([0.49, 1], P, 2)[0].tolist() == [-1, -1]
    assert clr.select([1, 1], P, 2, ignore_label=1)[1].tolist() == [-1, -1]
    assert (clr.select([1, 1], P[:1], 2) == -1).all()
    # NaN and -FLT_MAX never win: an active class then runs out of rois
    bad = P.copy()
    bad[:3, 0] = [np.nan, -clr.FLT_MAX, np.nan]
    assert clr.select([1, 0], bad, 2) is None


def test_center_loss_abi_error_codes():
    """SHAPE for n < 0 and c, m, d, top_k <= 0, NULL for a null required pointer - returned before
    any launch, so no GPU is needed; the workspace size is 0 for an invalid shape."""
    import ctypes
    from naws_hip import lib
    L = lib.load()
    p = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    a, none = ctypes.cast(buf, p), p(0)
    fwd = lambda n, c, m, d, k, ptrs=None: L.naws_center_loss_fwd(
        *(ptrs or (a, a, a, a)), n, c, m, d, k, -1, 1, a, a, a, a, none, none)
    bwd = lambda n, c, m, d, k: L.naws_center_loss_bwd(a, a, a, n, c, m, d, k, 1, a, a, a, a, none)
    upd = lambda c, m, d, k: L.naws_center_loss_update(a, a, a, a, a, c, m, d, k, 0.5, 0, 0, none)
    for bad in ((-1, 2, 2, 4, 2), (4, 0, 2, 4, 2), (4, 2, 0, 4, 2), (4, 2, 2, 0, 2), (4, 2, 2, 4, 0),
                (4, -3, 2, 4, 2), (4, 2, 2, 4, -1)):
        assert fwd(*bad) == lib.ERR_SHAPE, bad
        assert bwd(*bad) == lib.ERR_SHAPE, bad
        if bad[0] >= 0:
            assert upd(*bad[1:]) == lib.ERR_SHAPE, bad
    for i in range(4):                                   # X, P, F, CF
        ptrs = [a] * 4
        ptrs[i] = none
        assert fwd(4, 2, 2, 4, 2, tuple(ptrs)) == lib.ERR_NULL, i
    assert L.naws_center_loss_fwd(a, a, a, a, 4, 2, 2, 4, 2, -1, 1, none, a, a, a, none,
                                  none) == lib.ERR_NULL                    # workspace
    for i in (12, 13, 14):                               # L, D, S
        args = [a, a, a, a, 4, 2, 2, 4, 2, -1, 1, a, a, a, a, none, none]
        args[i] = none
        assert L.naws_center_loss_fwd(*args) == lib.ERR_NULL, i
    for i in (0, 1, 2, 9, 10, 11, 12):                   # D, S, dL, workspace, dF, dCF, ndCF
        args = [a, a, a, 4, 2, 2, 4, 2, 1, a, a, a, a, none]
        args[i] = none
        assert L.naws_center_loss_bwd(*args) == lib.ERR_NULL, i
    for i in range(5):
        args = [a, a, a, a, a, 2, 2, 4, 2, 0.5, 0, 0, none]
        args[i] = none
        assert L.naws_center_loss_update(*args) == lib.ERR_NULL, i
    assert L.naws_center_loss_workspace_bytes(0, 5, 10) == 0
    assert L.naws_center_loss_workspace_bytes(20, 5, 10) >= (2 * 200 + 20 + 1 + 100 + 20) * 4
    assert L.naws_center_loss_workspace_bytes(20, 5, 10) % 16 == 0
