"""TRAIN.FREEZE_CONV_BODY False without a GPU: the builders against the op trace recorded from the
reference (tests/golden/make_golden_trainable_body.py), the backward plan through RoIPoolF and
conv5_3..conv3_1, what is refused, and the C ABI of the new entries."""
import ctypes
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_trainable_body.json')))
WSDDN = ['WEBLY.WEBLY_ON', False, 'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head']
MODELS = [('na_wsddn_train', []), ('wsddn_train', WSDDN)]
BODY = ['conv%d_%d' % (i, j) for i in (3, 4, 5) for j in (1, 2, 3)]
HEAD = {'na_wsddn_train': ['fc6', 'fc7', 'fc8c', 'fc8d', '_[noisy]_fc6', '_[noisy]_fc7',
                           'noisy_fc8c', 'noisy_fc8d'],
        'wsddn_train': ['fc6', 'fc7', 'fc8c', 'fc8d']}


def _create(c, extra, train=True, frozen=False):
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 4, 'TRAIN.FREEZE_CONV_BODY', frozen] + extra)
    c.assert_and_infer_cfg(make_immutable=False)
    import detectron.modeling.model_builder_wsl as mb
    return mb.create(c.cfg.MODEL.TYPE, train=train)


def _norm(ops_, want):
    """The recorded form (tests/test_context_graph.py): helper-made Conv / FC carry their data input
    only, Dropout its first output, uuid is random per build."""
    out = []
    for o, w in zip(ops_, want):
        ins, outs, args = list(o.inputs), list(o.outputs), dict(o.args)
        if o.type in ('Conv', 'FC'):
            ins = ins[:len(w[1])]
        if o.type == 'Dropout':
            outs = outs[:1]
        if 'uuid' in args:
            args['uuid'] = 0
        out.append([o.type, ins, outs, args])
    return json.loads(json.dumps(out))


@pytest.mark.parametrize('key,extra', MODELS)
def test_builders_reproduce_reference_trace(cfgmod, key, extra):
    assert GOLD['freeze_conv_body'] is False and GOLD['freeze_at'] == 2
    m = _create(cfgmod, extra)              # raised NotImplementedError before the trainable body
    want = GOLD[key]
    assert len(m.net.ops) == len(want['ops'])
    got = _norm(m.net.ops, want['ops'])
    assert [g[:3] for g in got] == [w[:3] for w in want['ops']]
    for g, w in zip(got, want['ops']):
        if g[0] in ('Conv', 'MaxPool'):
            assert {k: g[3][k] for k in w[3] if k != 'dims'} == \
                {k: v for k, v in w[3].items() if k != 'dims'}, g
        if g[0] == 'RoIPoolF':
            assert {k: g[3][k] for k in w[3]} == w[3], g
    assert m.losses == want['losses'] and m.metrics == want['metrics']
    stops = [o.inputs[0] for o in m.net.ops if o.type == 'StopGradient']
    assert 'pool2' in stops and 'conv5_3' not in stops and 'roi_feat' not in stops
    # the frozen build of the same model differs by exactly those two StopGradient ops
    cfgmod.reset_cfg()
    f = _create(cfgmod, extra, frozen=True)
    fstops = [o.inputs[0] for o in f.net.ops if o.type == 'StopGradient']
    assert sorted(fstops) == sorted(stops + ['conv5_3', 'roi_feat'])
    assert len(f.net.ops) == len(m.net.ops) + 2


@pytest.mark.parametrize('key,extra', MODELS)
def test_backward_plan_reaches_conv3_1(cfgmod, key, extra):
    m = _create(cfgmod, extra)
    types = [o.type for o in m.grad_ops]
    first = types.index('RoIFeatureBoostGradient')
    body = ['RoIFeatureBoostGradient', 'RoIPoolFGradient']
    for blk in (5, 4, 3):
        for _ in range(3):
            body += ['ReluGradient', 'ConvGradient']
        if blk > 3:
            body.append('MaxPoolGradient')
    assert types[first:] == body                   # nothing after conv3_1, nothing in between
    tail = m.grad_ops[first:]
    convs = [o for o in tail if o.type == 'ConvGradient']
    assert [o.inputs[3] for o in convs] == BODY[::-1]       # inputs X, W, b | output Y
    assert [o.inputs[1] for o in tail if o.type == 'MaxPoolGradient'] == ['pool4', 'pool3']
    for o in convs:
        x, w, b = o.inputs[:3]
        if o.inputs[3] == 'conv3_1':               # behind pool2's StopGradient: no dX
            assert x == 'pool2' and o.args['_gin'][0] is None
            assert o.outputs == ['conv3_1_w_grad', 'conv3_1_b_grad']
        else:
            assert o.args['_gin'] == [x + '_grad', w + '_grad', b + '_grad']
        assert o.args['_accumulate'] == [False, False, False]
    roi = tail[1]
    assert roi.inputs == ['conv5_3', 'rois', 'roi_feat', '_argmax_roi_feat']
    assert roi.outputs == ['conv5_3_grad'] and roi.args['_gout'] == ['roi_feat_grad', None]
    assert roi.args['_gin'] == ['conv5_3_grad', None]
    # roi_feat_grad: one writer per fc6 that reads roi_feat, the later ones accumulate
    fc6 = [o for o in m.grad_ops if o.type == 'FCGradient' and o.inputs[0] == 'roi_feat']
    flags = [o.args['_accumulate'][0] for o in fc6]
    assert all(o.args['_gin'][0] == 'roi_feat_grad' for o in fc6)
    assert flags == ([False, True] if key == 'na_wsddn_train' else [False])
    assert not [t for t in types if t.startswith('StopGradient')]
    # parameters: the head's plus exactly conv3_1_w .. conv5_3_b, biases at lr x2 / no decay
    body_params = [b + s for b in BODY for s in ('_w', '_b')]
    head_params = [h + s for h in HEAD[key] for s in ('_w', '_b')]
    assert sorted(m.TrainableParams()) == sorted(body_params + head_params)
    assert len(body_params) == 18
    for p in ('conv1_1_w', 'conv1_2_b', 'conv2_1_w', 'conv2_2_b'):
        assert p in m.params and p not in m.param_to_grad
    upd = {o.inputs[3]: o.args for o in m.update_ops}
    for b in BODY:
        assert b + '_b' in m.biases and b + '_w' in m.weights
        assert (upd[b + '_b']['lr_mult'], upd[b + '_b']['weight_decay']) == (2.0, 0.0)
        assert (upd[b + '_w']['lr_mult'], upd[b + '_w']['weight_decay']) == \
            (1.0, cfgmod.cfg.SOLVER.WEIGHT_DECAY)
    assert len(m.allreduce_ops) == len(m.TrainableParams())
    # the frozen plan is what it was: no gradient op upstream of fc6
    cfgmod.reset_cfg()
    f = _create(cfgmod, extra, frozen=True)
    assert not [o for o in f.grad_ops if o.type.startswith(('RoI', 'Conv', 'MaxPool'))]
    assert sorted(f.TrainableParams()) == sorted(head_params)


def test_other_heads_build_with_a_trainable_body(cfgmod):
    for extra in (WSDDN + ['WSL.OICR', True], WSDDN + ['WSL.CENTER_LOSS', True],
                  ['WSL.MIN_ENTROPY_LOSS', True]):
        cfgmod.reset_cfg()
        m = _create(cfgmod, extra)
        assert [o.type for o in m.grad_ops].count('ConvGradient') == 9
        assert 'conv3_1_w' in m.TrainableParams() and 'conv2_2_w' not in m.TrainableParams()


def test_unfrozen_body_refusals(cfgmod):
    c = cfgmod
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 4, 'TRAIN.FREEZE_CONV_BODY', False, 'TRAIN.FREEZE_AT', 0])
    import detectron.modeling.model_builder_wsl as mb
    with pytest.raises(NotImplementedError, match='TRAIN.FREEZE_AT'):
        mb.create(c.cfg.MODEL.TYPE, train=True)
    mb.create(c.cfg.MODEL.TYPE, train=False)                # inference never asks
    c.merge_cfg_from_list(['TRAIN.FREEZE_CONV_BODY', True])
    mb.create(c.cfg.MODEL.TYPE, train=True)                 # a frozen body takes any FREEZE_AT
    # RoILoopPool has no gradient: WSL.CONTEXT still needs the frozen body
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 4, 'TRAIN.FREEZE_CONV_BODY', False, 'WSL.CONTEXT', True] + WSDDN)
    with pytest.raises(NotImplementedError, match='RoILoopPool'):
        mb.create(c.cfg.MODEL.TYPE, train=True)
    # the fused engine keeps refusing the switch
    src = open(os.path.join(ROOT, 'na-fwebsod_amd', 'detectron', 'core', 'executor.py')).read()
    assert 'cfg.TRAIN.FREEZE_CONV_BODY and' in src


def test_new_entries_validate_before_any_launch():
    """SHAPE for a non-positive dim, ARG for a stride / dilation / layout out of range, UNSUPPORTED
    for channels that are not a multiple of 32, NULL for a missing pointer - all before a launch."""
    from naws_hip import lib
    L = lib.load()
    p = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    a, none = ctypes.cast(buf, p), p(0)
    # naws_roi_pool_f_bwd(dY, argmax, rois, R, layout, N, C, H, W, ph, pw, dX, stream)
    roi = lambda **k: L.naws_roi_pool_f_bwd(
        k.get('dy', a), a, a, k.get('R', 4), k.get('layout', lib.LAYOUT_NCHW), 1, k.get('C', 32),
        k.get('H', 8), 8, 7, k.get('pw', 7), k.get('dx', a), none)
    assert roi(R=-1) == lib.ERR_SHAPE and roi(C=0) == lib.ERR_SHAPE and roi(pw=0) == lib.ERR_SHAPE
    assert roi(H=0) == lib.ERR_SHAPE
    assert roi(layout=2) == lib.ERR_ARG
    assert roi(dx=none) == lib.ERR_NULL and roi(dy=none) == lib.ERR_NULL
    # naws_maxpool2x2_nhwc_bwd(X, Y, dY, N, H, W, C, stride, dX, stream)
    pool = lambda **k: L.naws_maxpool2x2_nhwc_bwd(
        k.get('x', a), a, k.get('dy', a), k.get('N', 1), k.get('H', 8), 8, k.get('C', 32),
        k.get('stride', 2), k.get('dx', a), none)
    assert pool(N=0) == lib.ERR_SHAPE and pool(H=1) == lib.ERR_SHAPE and pool(C=0) == lib.ERR_SHAPE
    assert pool(stride=3) == lib.ERR_ARG and pool(stride=0) == lib.ERR_ARG
    assert pool(C=30) == lib.ERR_ARG                         # float4 lanes, as the forward
    assert pool(x=none) == lib.ERR_NULL and pool(dy=none) == lib.ERR_NULL
    assert pool(dx=none) == lib.ERR_NULL
    # naws_conv3x3_dgrad_pack_weight(W_oihw, Cout, Cin, W_packed, stream)
    assert L.naws_conv3x3_dgrad_pack_weight(a, 0, 32, a, none) == lib.ERR_SHAPE
    assert L.naws_conv3x3_dgrad_pack_weight(a, 32, -1, a, none) == lib.ERR_SHAPE
    assert L.naws_conv3x3_dgrad_pack_weight(a, 32, 48, a, none) == lib.ERR_UNSUPPORTED
    assert L.naws_conv3x3_dgrad_pack_weight(a, 3, 32, a, none) == lib.ERR_UNSUPPORTED
    assert L.naws_conv3x3_dgrad_pack_weight(none, 32, 32, a, none) == lib.ERR_NULL
    assert L.naws_conv3x3_dgrad_pack_weight(a, 32, 32, none, none) == lib.ERR_NULL
    # naws_conv3x3_nhwc_wgrad(X, dY, N, H, W, Cin, Cout, dilation, workspace, dW, db, stream)
    wg = lambda **k: L.naws_conv3x3_nhwc_wgrad(
        k.get('x', a), k.get('dy', a), k.get('N', 1), 8, k.get('W', 8), k.get('cin', 32),
        k.get('cout', 64), k.get('d', 1), k.get('ws', a), k.get('dw', a), k.get('db', a), none)
    assert wg(N=0) == lib.ERR_SHAPE and wg(W=0) == lib.ERR_SHAPE and wg(cin=0) == lib.ERR_SHAPE
    assert wg(d=0) == lib.ERR_ARG and wg(d=3) == lib.ERR_ARG
    assert wg(cin=3) == lib.ERR_UNSUPPORTED and wg(cout=48) == lib.ERR_UNSUPPORTED
    for k in ('x', 'dy', 'ws', 'dw', 'db'):
        assert wg(**{k: none}) == lib.ERR_NULL, k
    # workspace: the two staged copies, nine tap gradients, the split-K partial products
    size = L.naws_conv3x3_nhwc_wgrad_workspace_floats
    assert size(0, 8, 8, 32, 64, 1) == 0 and size(1, 8, 8, 32, 64, 3) == 0
    assert size(1, 8, 8, 30, 64, 1) == 0
    for n, h, w, ci, co, d in ((1, 9, 13, 32, 64, 1), (2, 9, 13, 64, 32, 2), (1, 75, 125, 256, 512, 2)):
        rows = n * (h + 2 * d) * (w + 2 * d)
        fixed = rows * (ci + co) + 9 * ci * co
        extra = size(n, h, w, ci, co, d) - fixed
        assert extra > 0 and extra % (3 * ci * co) == 0 and extra // (3 * ci * co) <= 32


def test_header_with_the_new_entries_is_plain_c_and_cpp(tmp_path):
    """include/naws.h still compiles as C and as C++, and a C caller sees the five prototypes."""
    hdr = os.path.join(ROOT, 'include', 'naws.h')
    for cc, lang in (('gcc', 'c'), ('g++', 'c++')):
        subprocess.check_call([cc, '-fsyntax-only', '-Wall', '-Werror', '-x', lang, hdr])
    src = tmp_path / 'use.c'
    src.write_text(
        '#include "naws.h"\n'
        'int (*f1)(const float*, const int32_t*, const float*, int, int, int, int, int, int, int, int,\n'
        '          float*, void*) = naws_roi_pool_f_bwd;\n'
        'int (*f2)(const float*, const float*, const float*, int, int, int, int, int, float*, void*)\n'
        '    = naws_maxpool2x2_nhwc_bwd;\n'
        'int (*f3)(const float*, int, int, float*, void*) = naws_conv3x3_dgrad_pack_weight;\n'
        'int64_t (*f4)(int, int, int, int, int, int) = naws_conv3x3_nhwc_wgrad_workspace_floats;\n'
        'int (*f5)(const float*, const float*, int, int, int, int, int, int, float*, float*, float*,\n'
        '          void*) = naws_conv3x3_nhwc_wgrad;\n')
    for cc, lang in (('gcc', 'c'), ('g++', 'c++')):
        subprocess.check_call([cc, '-fsyntax-only', '-Wall', '-Werror', '-Wno-unused-variable',
                               '-I', os.path.join(ROOT, 'include'), '-x', lang, str(src)])
    from naws_hip import lib
    for name in ('naws_roi_pool_f_bwd', 'naws_maxpool2x2_nhwc_bwd', 'naws_conv3x3_dgrad_pack_weight',
                 'naws_conv3x3_nhwc_wgrad', 'naws_conv3x3_nhwc_wgrad_workspace_floats'):
        assert name in lib.ALL_SYMBOLS and hasattr(lib.load(), name)
