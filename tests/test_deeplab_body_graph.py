"""MODEL.CONV_BODY without a GPU: the DeepLab body (kernel-3 / pad-1 pools) and the conv4 body
against the op traces recorded from the reference (tests/golden/make_golden_deeplab_body.py), what
is refused, the fused engine's conv plan for the DeepLab body, and the C ABI of the new pool."""
import ctypes
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_deeplab_body.json')))
ORIGIN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_trainable_body.json')))
DEEPLAB = 'VGG16.add_VGG16_conv5_body_deeplab'
CONV4 = 'VGG16.add_VGG16_conv4_body_origin'
BODIES = [('deeplab_d2', 'add_VGG16_conv5_body_deeplab', 2),
          ('deeplab_d1', 'add_VGG16_conv5_body_deeplab', 1),
          ('conv4', 'add_VGG16_conv4_body_origin', 1)]


def _cfg(c, extra):
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 4] + extra)
    c.assert_and_infer_cfg(make_immutable=False)


def _norm(ops_):
    """The recorded form: helper-made Conv carries its data input only."""
    out = []
    for o in ops_:
        ins = list(o.inputs)[:1] if o.type == 'Conv' else list(o.inputs)
        out.append([o.type, ins, list(o.outputs), dict(o.args)])
    return json.loads(json.dumps(out))


def _same_ops(got, want):
    assert len(got) == len(want)
    assert [g[:3] for g in got] == [w[:3] for w in want]
    for g, w in zip(got, want):
        if g[0] in ('Conv', 'MaxPool'):
            args = {k: v for k, v in w[3].items() if k != 'dims'}
            assert {k: g[3].get(k) for k in args} == args, g
            if g[0] == 'MaxPool':
                assert sorted(g[3]) == sorted(args), g            # nothing but kernel / pad / stride


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('key,builder,dilation', BODIES)
def test_body_builders_reproduce_reference_trace(cfgmod, key, builder, dilation, train):
    from detectron.modeling import VGG16
    from detectron.modeling.detector import DetectionModelHelper
    _cfg(cfgmod, ['WSL.DILATION', dilation, 'TRAIN.FREEZE_CONV_BODY', True])
    assert cfgmod.cfg.TRAIN.FREEZE_AT == GOLD['freeze_at']
    want = GOLD['%s_%s' % (key, 'train' if train else 'test')]
    m = DetectionModelHelper(name=key, train=train, num_classes=21, init_params=train)
    blob, dim, scale = getattr(VGG16, builder)(m)
    assert (blob, dim, scale) == (want['blob'], want['dim'], want['scale'])
    _same_ops(_norm(m.net.ops), want['ops'])
    convs = [o for o in m.net.ops if o.type == 'Conv']
    assert [o.outputs[0] for o in convs] == \
        ['conv%d_%d' % (i, j) for i, n in ((1, 2), (2, 2), (3, 3), (4, 3), (5, 3))
         for j in range(1, n + 1)][:len(convs)]
    stops = [o.inputs[0] for o in m.net.ops if o.type == 'StopGradient']
    assert stops == (['pool2'] if key == 'conv4' else [])


@pytest.mark.parametrize('dilation', [1, 2])
def test_whole_model_over_the_deeplab_body(cfgmod, dilation):
    """generalized_wsl with MODEL.CONV_BODY set (it died in get_func): the body's ops, then the head
    of the shipped model unchanged; parameter names and shapes are the origin body's."""
    import detectron.modeling.model_builder_wsl as mb
    _cfg(cfgmod, ['WSL.DILATION', dilation, 'TRAIN.FREEZE_CONV_BODY', True])
    o = mb.create(cfgmod.cfg.MODEL.TYPE, train=True)
    cfgmod.reset_cfg()
    _cfg(cfgmod, ['WSL.DILATION', dilation, 'TRAIN.FREEZE_CONV_BODY', True,
                  'MODEL.CONV_BODY', DEEPLAB])
    for train in (True, False):
        m = mb.create(cfgmod.cfg.MODEL.TYPE, train=train)
        want = GOLD['deeplab_d%d_%s' % (dilation, 'train' if train else 'test')]['ops']
        _same_ops(_norm(m.net.ops[:len(want)]), want)
        assert m.net.ops[len(want)].type == 'StopGradient'
        assert m.net.ops[len(want)].inputs == ['conv5_3']
    m = mb.create(cfgmod.cfg.MODEL.TYPE, train=True)
    assert m.params == o.params and m.param_shapes == o.param_shapes
    n_o = [i for i, op in enumerate(o.net.ops) if op.outputs[0] == 'conv5_3'][-1]
    n_m = [i for i, op in enumerate(m.net.ops) if op.outputs[0] == 'conv5_3'][-1]
    assert [tuple(x) for x in m.net.ops[n_m:]] == [tuple(x) for x in o.net.ops[n_o:]]
    assert not [g for g in m.grad_ops if g.type.startswith(('RoI', 'Conv', 'MaxPool'))]
    assert sorted(m.TrainableParams()) == sorted(o.TrainableParams())


def test_refusals_and_unchanged_origin_body(cfgmod):
    import detectron.modeling.model_builder_wsl as mb
    c = cfgmod
    _cfg(c, ['TRAIN.FREEZE_CONV_BODY', False, 'MODEL.CONV_BODY', DEEPLAB])
    with pytest.raises(NotImplementedError, match='TRAIN.FREEZE_CONV_BODY') as e:
        mb.create(c.cfg.MODEL.TYPE, train=True)
    assert 'add_VGG16_conv5_body_deeplab' in str(e.value)
    mb.create(c.cfg.MODEL.TYPE, train=False)                       # inference never asks
    c.merge_cfg_from_list(['TRAIN.FREEZE_CONV_BODY', True, 'TRAIN.FREEZE_AT', 0])
    mb.create(c.cfg.MODEL.TYPE, train=True)                        # a frozen body builds
    # the conv4 body follows the origin body's FREEZE_AT rule
    c.reset_cfg()
    _cfg(c, ['TRAIN.FREEZE_CONV_BODY', False, 'MODEL.CONV_BODY', CONV4, 'WSL.DILATION', 1])
    m = mb.create(c.cfg.MODEL.TYPE, train=True)
    assert 'conv3_1_w' in m.TrainableParams() and 'conv2_2_w' not in m.TrainableParams()
    assert 'conv5_1_w' not in m.params
    c.merge_cfg_from_list(['TRAIN.FREEZE_AT', 0])
    with pytest.raises(NotImplementedError, match='TRAIN.FREEZE_AT'):
        mb.create(c.cfg.MODEL.TYPE, train=True)
    # the origin body: the trace the reference recorded for it, as tests/test_trainable_body_graph.py
    # compares it
    c.reset_cfg()
    _cfg(c, ['TRAIN.FREEZE_CONV_BODY', False])
    m = mb.create(c.cfg.MODEL.TYPE, train=True)
    want = ORIGIN['na_wsddn_train']['ops']
    assert len(m.net.ops) == len(want)
    assert [[o.type, list(o.outputs)[:1]] for o in m.net.ops] == [[w[0], w[2][:1]] for w in want]
    pools = [(o.args['kernel'], o.args['pad'], o.args['stride']) for o in m.net.ops
             if o.type == 'MaxPool']
    assert pools == [(w[3]['kernel'], w[3]['pad'], w[3]['stride']) for w in want if w[0] == 'MaxPool']
    assert pools == [(2, 0, 2)] * 3 + [(2, 0, 1)]


def test_conv_plan_for_the_deeplab_body():
    from naws_hip.engine import PoolStep, conv_plan, pooled_size
    for plan in ('fp16x2', 'fp32x3', 'fp32', 'bf16'):
        for dilation, strides in ((2, (2, 2, 2, 1)), (1, (2, 2, 2, 2))):
            for f4 in (256, 512, 0):
                origin = conv_plan(plan, dilation, f4)
                assert origin == conv_plan(plan, dilation, f4, body='origin')
                got = conv_plan(plan, dilation, f4, body='deeplab')
                assert len(got) == len(origin) == 17
                pools = [s for s in got if isinstance(s, PoolStep)]
                assert [(s.form, s.stride) for s in pools] == [('pool3', s) for s in strides]
                assert [(s.form, s.stride) for s in origin if isinstance(s, PoolStep)] == \
                    [('pool', s) for s in strides]
                for a, b in zip(got, origin):
                    assert isinstance(a, PoolStep) == isinstance(b, PoolStep)
                    if not isinstance(a, PoolStep):
                        assert a.pool2 is False
                        assert a == b._replace(pool2=False)       # every conv form choice stays
        assert any(s.pool2 for s in conv_plan(plan, 2, 256) if not isinstance(s, PoolStep)) == \
            (plan != 'fp32')
    with pytest.raises(ValueError):
        conv_plan('fp16x2', 2, 256, body='conv4')
    # the step's own size rule: 600 x 1000 -> 75 x 125 (a true 1/8), the origin body 74 x 124
    for body, want in (('deeplab', (75, 125)), ('origin', (74, 124))):
        h, w = 600, 1000
        for s in conv_plan('fp16x2', 2, 256, body=body):
            if isinstance(s, PoolStep):
                h, w = pooled_size(s, h, w)
        assert (h, w) == want
    h, w = 50, 66
    sizes = []
    for s in conv_plan('fp32', 1, 256, body='deeplab'):
        if isinstance(s, PoolStep):
            h, w = pooled_size(s, h, w)
            sizes.append((h, w))
    assert sizes == [(25, 33), (13, 17), (7, 9), (4, 5)]


def test_executor_body_choice(cfgmod):
    """MODEL.CONV_BODY -> the engine's body; a body without a fused chain has no canonical list."""
    from detectron.core import executor as E
    from naws_hip.engine import body_of
    assert body_of('VGG16.add_VGG16_conv5_body_origin') == 'origin'
    assert body_of(DEEPLAB) == 'deeplab' and body_of(CONV4) is None and body_of('x.y') is None
    import detectron.modeling.model_builder_wsl as mb
    for body, pool in ((DEEPLAB, (3, 1)), ('VGG16.add_VGG16_conv5_body_origin', (2, 0))):
        cfgmod.reset_cfg()
        _cfg(cfgmod, ['MODEL.CONV_BODY', body, 'TRAIN.FREEZE_CONV_BODY', True])
        for train in (True, False):
            m = mb.create(cfgmod.cfg.MODEL.TYPE, train=train)
            assert E._signature(m.net.ops) == E.canonical_na_wsddn_signature(train, m.num_classes)
            assert {p[:2] for p in E._pool_args(m.net.ops)} == {pool}
    cfgmod.reset_cfg()
    _cfg(cfgmod, ['MODEL.CONV_BODY', CONV4, 'WSL.DILATION', 1, 'TRAIN.FREEZE_CONV_BODY', True])
    assert E.canonical_na_wsddn_signature(True, 21) is None


def test_new_entry_validates_before_any_launch():
    """SHAPE for a non-positive dim, ARG for a stride other than 1 / 2, for C % 4 != 0 and for a
    pointer off 16 bytes, NULL for a missing pointer - all before a launch (no GPU here)."""
    from naws_hip import lib
    L = lib.load()
    p = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    a = p(base + (-base) % 16)
    off = p(a.value + 4)
    none = p(0)
    # naws_maxpool3x3_nhwc_fwd(X, N, H, W, C, stride, Y, stream)
    pool = lambda **k: L.naws_maxpool3x3_nhwc_fwd(
        k.get('x', a), k.get('N', 1), k.get('H', 2), k.get('W', 2), k.get('C', 4),
        k.get('stride', 2), k.get('y', a), none)
    for dim in ('N', 'H', 'W', 'C'):
        assert pool(**{dim: 0}) == lib.ERR_SHAPE and pool(**{dim: -3}) == lib.ERR_SHAPE, dim
    assert pool(stride=3) == lib.ERR_ARG and pool(stride=0) == lib.ERR_ARG
    assert pool(C=6) == lib.ERR_ARG and pool(C=30) == lib.ERR_ARG
    assert pool(x=off) == lib.ERR_ARG and pool(y=off) == lib.ERR_ARG
    assert pool(x=none) == lib.ERR_NULL and pool(y=none) == lib.ERR_NULL
    assert pool(N=0, x=none) == lib.ERR_SHAPE                 # the shape is looked at first
    import detectron.ops as O
    src = open(os.path.join(ROOT, 'na-fwebsod_amd', 'detectron', 'ops', '__init__.py')).read()
    assert 'maxpool3x3_nhwc' in src and O.MaxPool.__defaults__ == (2, 0, 2)


def test_header_with_the_new_entry_is_plain_c_and_cpp(tmp_path):
    hdr = os.path.join(ROOT, 'include', 'naws.h')
    for cc, lang in (('gcc', 'c'), ('g++', 'c++')):
        subprocess.check_call([cc, '-fsyntax-only', '-Wall', '-Werror', '-x', lang, hdr])
    src = tmp_path / 'use.c'
    src.write_text('#include "naws.h"\n'
                   'int (*f1)(const float*, int, int, int, int, int, float*, void*)\n'
                   '    = naws_maxpool3x3_nhwc_fwd;\n')
    for cc, lang in (('gcc', 'c'), ('g++', 'c++')):
        subprocess.check_call([cc, '-fsyntax-only', '-Wall', '-Werror', '-Wno-unused-variable',
                               '-I', os.path.join(ROOT, 'include'), '-x', lang, str(src)])
    from naws_hip import lib
    assert 'naws_maxpool3x3_nhwc_fwd' in lib.ALL_SYMBOLS
    assert hasattr(lib.load(), 'naws_maxpool3x3_nhwc_fwd')
    assert 'UNPINNED' in open(hdr).read().split('naws_maxpool3x3_nhwc_fwd')[0][-1500:]
