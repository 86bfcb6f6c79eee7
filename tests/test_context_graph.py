"""WSL.CONTEXT, the contextual WSDDN head (ContextLocNet's "frame minus context" detection stream),
without a GPU: the builders against the op trace recorded from the reference
(tests/golden/make_golden_context.py), the backward plan over shared parameters, the cfg switches,
and the numpy restatements the GPU tests compare against (tests/context_ref.py)."""
import json
import os

import numpy as np
import pytest

import context_ref as cr
from helpers import make_rois

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_context.json')))
CONTEXT = ['NUM_GPUS', 4, 'WEBLY.WEBLY_ON', False, 'WSL.CONTEXT', True,
           'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head']


def _norm_ops(ops_, want):
    """The recorded form of an op list: Conv / FC made by the model helper are recorded with their
    data input only, an FC emitted on existing parameters (the shared ones) with all three."""
    out = []
    for o, w in zip(ops_, want):
        ins, outs, args = list(o.inputs), list(o.outputs), dict(o.args)
        if o.type in ('Conv', 'FC'):
            ins = ins[:len(w[1])]
        if o.type == 'Dropout':
            outs = outs[:1]
        if 'uuid' in args:
            args['uuid'] = 0             # random per build upstream (uuid4)
        out.append([o.type, ins, outs, args])
    return json.loads(json.dumps(out))       # tuples -> lists, as the recorded file holds them


@pytest.mark.parametrize('oicr,n_train,n_test', [(False, 74, 65), (True, 90, 72)])
def test_context_builders_reproduce_reference_trace(cfgmod, oicr, n_train, n_test):
    c = cfgmod
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(CONTEXT + ['WSL.OICR', oicr])
    c.assert_and_infer_cfg(make_immutable=False)
    import detectron.modeling.model_builder_wsl as mb
    tag = 'wsl_context_oicr_' if oicr else 'wsl_context_'
    for train, key, n in ((True, tag + 'train', n_train), (False, tag + 'test', n_test)):
        m = mb.create(c.cfg.MODEL.TYPE, train=train)
        want = GOLD[key]
        assert len(want['ops']) == n and len(m.net.ops) == n
        got = _norm_ops(m.net.ops, want['ops'])
        assert [g[:3] for g in got] == [w[:3] for w in want['ops']]
        for g, w in zip(got, want['ops']):
            if g[0] in ('RoILabel', 'SoftmaxWithLossN', 'Mean', 'Split', 'Concat', 'RoIContext',
                        'Sub', 'Softmax', 'Transpose', 'ReduceSum', 'CrossEntropyWithLogits'):
                assert g[3] == w[3], g
            if g[0] in ('RoIPoolF', 'RoILoopPool'):
                assert {k: g[3][k] for k in w[3]} == w[3], g
        assert m.losses == want['losses'] and m.metrics == want['metrics']
        # the shared FCs are emitted on the plain stream's parameters: nothing new is created
        assert 'fc8d_w' not in m.params and 'fc6_frame_w' not in m.params
        assert m.param_shapes['fc8d_frame_w'] == (20, 4096)
    # RoIContext carries no argument: cfg.WSL.CONTEXT_RATIO never reaches the graph upstream either
    ctx = [o for o in m.net.ops if o.type == 'RoIContext']
    assert len(ctx) == 1 and ctx[0].args == {} and ctx[0].inputs == ['rois', 'data']
    # (upstream declares it, 1.8 = the op's default; it is not declared here: an option without
    # effect, and the dumped cfg of the weights / detections files stays the recorded one)
    assert GOLD['context_ratio_cfg'] == 1.8 and 'CONTEXT_RATIO' not in c.cfg.WSL


def test_context_backward_plan_accumulates_shared_parameters(cfgmod):
    c = cfgmod
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(CONTEXT)
    import detectron.modeling.model_builder_wsl as mb
    m = mb.create(c.cfg.MODEL.TYPE, train=True)
    fcg = [o for o in m.grad_ops if o.type == 'FCGradient']
    for p, n in (('fc6_w', 3), ('fc6_b', 3), ('fc7_w', 3), ('fc7_b', 3), ('fc8d_frame_w', 2),
                 ('fc8d_frame_b', 2), ('fc8c_w', 1), ('fc8c_b', 1)):
        flags = [o.args['_accumulate'][list(o.inputs).index(p)] for o in fcg if p in o.inputs[:3]]
        assert flags == [False] + [True] * (n - 1), (p, flags)     # first writes, the others add
        assert m.param_to_grad[p] == p + '_grad'
    assert set(m.TrainableParams()) == {'fc6_w', 'fc6_b', 'fc7_w', 'fc7_b', 'fc8c_w', 'fc8c_b',
                                        'fc8d_frame_w', 'fc8d_frame_b'}
    gtypes = [o.type for o in m.grad_ops]
    assert gtypes.count('SubGradient') == 1
    sub = m.grad_ops[gtypes.index('SubGradient')]
    assert sub.outputs == ['fc8d_frame_grad', 'fc8d_context_grad']
    # nothing for the pooling ops, RoIContext or anything upstream of them
    assert not [t for t in gtypes if t.startswith(('RoI', 'Conv', 'MaxPool', 'StopGradient'))]
    # the three FCs that read roi_feat* behind StopGradient emit no input gradient (a 25088-wide
    # GEMM per stream that nothing would read); every other FC still does
    for o in fcg:
        behind_stop = o.inputs[0].startswith('roi_feat')
        assert (o.args['_gin'][0] is None) == behind_stop, o.inputs
        assert (o.inputs[0] + '_grad' in o.outputs) != behind_stop
    assert sum(o.inputs[0].startswith('roi_feat') for o in fcg) == 3
    # a gradient INTO RoILoopPool (a trainable conv body) is not built: loud, not silent
    c.merge_cfg_from_list(['TRAIN.FREEZE_CONV_BODY', False])
    with pytest.raises(NotImplementedError):
        mb.create(c.cfg.MODEL.TYPE, train=True)


def test_unshared_graph_backward_plan_is_unchanged(cfgmod):
    """Without sharing no parameter accumulates, and the plain head's fc6 drops its dead dX too."""
    c = cfgmod
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 4])
    import detectron.modeling.model_builder_wsl as mb
    m = mb.create(c.cfg.MODEL.TYPE, train=True)
    params = set(m.params)
    for o in m.grad_ops:
        n_in = len(o.args['_gin'])
        for i, name in enumerate(o.inputs[:n_in]):
            if name in params:
                assert not o.args['_accumulate'][i], (o.type, name)
    dead = [o for o in m.grad_ops if o.type == 'FCGradient' and o.args['_gin'][0] is None]
    assert sorted(o.outputs[0] for o in dead) == ['_[noisy]_fc6_w_grad', 'fc6_w_grad']


def test_context_cfg_switches(cfgmod):
    c = cfgmod
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(CONTEXT)
    c.assert_and_infer_cfg(make_immutable=False)           # WSL.CONTEXT is an accepted switch now
    c.merge_cfg_from_list(['WSL.PCL', True])
    with pytest.raises(NotImplementedError):
        c.assert_and_infer_cfg(make_immutable=False)       # the other methods still are not
    c.merge_cfg_from_list(['WSL.PCL', False, 'WEBLY.WEBLY_ON', True,
                           'FAST_RCNN.ROI_BOX_HEAD', 'webly_heads.add_VGG16_roi_2fc_noise_head'])
    import detectron.modeling.model_builder_wsl as mb
    with pytest.raises(AttributeError, match='add_VGG16_roi_context_2fc_noise_head'):
        mb.create(c.cfg.MODEL.TYPE, train=True)            # dead upstream as well


def test_restatements_known_answers():
    """roi (10, 20, 100, 80) at ratio 1.8 in a 600 x 1000 image; and the two ties of the restated
    RoILoopPool to the existing RoIPoolF oracle that the GPU tests lean on."""
    from oracle import oracle
    f, ctx = cr.roi_context(np.array([[0, 10, 20, 100, 80]], np.float32), 600, 1000, 1.8)
    assert np.array_equal(ctx[0], np.array([0, 0, 0, 136, 104, 10, 20, 100, 80], np.float32))
    assert np.array_equal(f[0, :5], np.array([0, 10, 20, 100, 80], np.float32))
    np.testing.assert_allclose(f[0, 5:], [30, 100 / 3, 80, 200 / 3], rtol=1e-6)
    assert f.dtype == np.float32 and ctx.dtype == np.float32
    rng = np.random.default_rng(1)
    rois = make_rois(rng, 1, 300, 480, 640, degenerate=True)
    x = np.maximum(rng.standard_normal((1, 16, 60, 80)), 0).astype(np.float32)
    plain, _ = oracle.roi_pool_f(x, rois, 7, 7, 0.125)
    no_hole = np.concatenate([rois, np.zeros((300, 4), np.float32)], 1)
    y0, a0 = cr.roi_loop_pool(x, no_hole, 7, 7, 0.125)
    assert np.array_equal(y0, plain)                       # degenerate rois included
    assert ((a0 == -1) == (y0 == 0)).all()                 # maxima start at 0: an all-zero bin is -1
    frame, context = cr.roi_context(rois, 480, 640)
    yf, _ = cr.roi_loop_pool(x, frame, 7, 7, 0.125)
    yc, _ = cr.roi_loop_pool(x, context, 7, 7, 0.125)
    assert (yf <= plain).all()
    assert (yf != plain).mean() >= 0.05 and (yc != plain).mean() >= 0.30
    # signed features: nothing negative survives
    xs = rng.standard_normal((1, 4, 60, 80)).astype(np.float32)
    ys, as_ = cr.roi_loop_pool(xs, frame, 7, 7, 0.125)
    assert (ys >= 0).all() and ((as_ == -1) == (ys == 0)).all() and (ys == 0).any()
