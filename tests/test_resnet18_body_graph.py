"""MODEL.CONV_BODY ResNet18 without a GPU: the ResNet18-WS builders and the 2-fc head against the op
traces recorded from the reference (tests/golden/make_golden_resnet18_body.py), the RESNETS cfg
node, what is refused, the float64 restatement of tests/resnet_ref.py against an independent
formulation, and the C ABI of the two new entries."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
GOLD = rref.golden()
CONV5, CONV4 = 'ResNet18.add_ResNet18_conv5_body', 'ResNet18.add_ResNet18_conv4_body'
HEAD = 'wsl_heads.add_ResNet_roi_2fc_head'
RESNET = ['WEBLY.WEBLY_ON', False, 'RESNETS.TRANS_FUNC', 'residual_transformation',
          'FAST_RCNN.ROI_BOX_HEAD', HEAD, 'FAST_RCNN.MLP_HEAD_DIM', 4096, 'TRAIN.FREEZE_CONV_BODY', True]
BODIES = [('conv5_d1', 'add_ResNet18_conv5_body', 1), ('conv5_d2', 'add_ResNet18_conv5_body', 2),
          ('conv4', 'add_ResNet18_conv4_body', 1)]


def _cfg(c, extra):
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 4] + RESNET + extra)
    c.assert_and_infer_cfg(make_immutable=False)


def _helper(train):
    from detectron.modeling.detector import DetectionModelHelper
    return DetectionModelHelper(name='m', train=train, num_classes=21, init_params=train)


def _same_trace(model, want):
    """Types, inputs (a helper-made Conv / FC is recorded with its data input only; our ops also
    name their parameters), outputs and every recorded geometry argument; a Conv recorded with
    no_bias has two inputs here, any other three."""
    ops_ = model.net.ops
    assert len(ops_) == len(want['ops'])
    for o, (t, ins, outs, kw) in zip(ops_, want['ops']):
        mine = list(o.outputs)
        if t == 'Dropout':                 # this package's Dropout also names its mask blob
            assert mine[1:] == ['_' + mine[0] + '_mask']
            mine = mine[:1]
        assert o.type == t and mine == outs, (o, t, outs)
        if t in ('Conv', 'FC') and len(ins) == 1:
            assert o.inputs[0] == ins[0] and o.inputs[1] == outs[0] + '_w', o
            assert len(o.inputs) == (2 if kw.get('no_bias') else 3), o
            if len(o.inputs) == 3:
                assert o.inputs[2] == outs[0] + '_b'
        else:
            assert list(o.inputs) == ins, (o, ins)
        if t == 'Conv':
            dims = kw['dims']
            kernel = dims[2] if len(dims) > 2 else kw['kernel']
            assert o.args['kernel'] == kernel and kw.get('group', 1) == 1
            for k in ('stride', 'pad', 'dilation'):
                assert o.args.get(k) == kw.get(k), (o, k)      # an absent argument is absent here too
            assert 'group' not in o.args and 'no_bias' not in o.args
        elif t == 'AffineChannel':
            assert o.args == {}
        elif t in ('MaxPool', 'Dropout', 'RoIPoolF'):
            assert {k: o.args.get(k) for k in kw} == kw, o
    got = [[n, list(model.param_shapes[n])] for n in model.params]
    assert got == want['params']


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('key,builder,dilation', BODIES)
def test_body_builders_reproduce_reference_trace(cfgmod, key, builder, dilation, train):
    from detectron.modeling import ResNet18
    _cfg(cfgmod, ['RESNETS.RES5_DILATION', dilation])
    assert cfgmod.cfg.TRAIN.FREEZE_AT == GOLD['freeze_at']
    want = GOLD['%s_%s' % (key, 'train' if train else 'test')]
    m = _helper(train)
    blob, dim, scale = getattr(ResNet18, builder)(m)
    assert (blob, dim, scale) == (want['blob'], want['dim'], want['scale'])
    _same_trace(m, want)
    # the stage strides: 1, 2, 2, 2 at RES5_DILATION 1; 1, 2, 2, 1 with dilated res5 convs at 2
    first = {o.outputs[0]: o.args for o in m.net.ops if o.type == 'Conv'}
    strides = [first['res%d_0_branch2a' % s]['stride'] for s in (2, 3, 4, 5)[:3 if key == 'conv4' else 4]]
    assert strides == [1, 2, 2, 2 if dilation == 1 else 1][:len(strides)]
    if key != 'conv4':
        for blk in (0, 1):
            for br in ('a', 'b'):
                a = first['res5_%d_branch2%s' % (blk, br)]
                assert (a['pad'], a['dilation']) == (dilation, dilation)
        assert first['res5_0_branch1']['stride'] == (2 if dilation == 1 else 1)
        assert scale == dilation / 32.0
    assert first['conv1'] == {'kernel': 7, 'pad': 3, 'stride': 2}
    # in-place Sum in a stage's first block, a `_sum` blob in its last; StopGradient after res2
    sums = [(o.inputs[0], o.outputs[0]) for o in m.net.ops if o.type == 'Sum']
    assert all((a == b) == a.startswith(('res2_0', 'res3_0', 'res4_0', 'res5_0')) for a, b in sums)
    assert [o.inputs[0] for o in m.net.ops if o.type == 'StopGradient'] == ['res2_1_sum']


@pytest.mark.parametrize('train', [True, False])
def test_2fc_head_reproduces_reference_trace(cfgmod, train):
    from detectron.modeling import wsl_heads
    _cfg(cfgmod, [])
    want = GOLD['head_2fc_%s' % ('train' if train else 'test')]
    m = _helper(train)
    blob, dim = wsl_heads.add_ResNet_roi_2fc_head(m, 'res5_1_sum', 512, 1. / 16.)
    assert (blob, dim) == (want['blob'], want['dim'])
    _same_trace(m, want)
    # WSL.MLP_HEAD_DIM's two widths, and the other two heads
    cfgmod.merge_cfg_from_list(['WSL.MLP_HEAD_DIM', '[512, 128]'])
    m = _helper(train)
    assert wsl_heads.add_ResNet_roi_2fc_head(m, 'x', 512, 1. / 16.)[1] == 128
    assert m.param_shapes['fc6_w'] == (512, 512 * 49) and m.param_shapes['fc7_w'] == (128, 512)
    m = _helper(train)
    assert wsl_heads.add_ResNet_roi_1fc_head(m, 'x', 512, 1. / 16.) == \
        ('drop6' if train else 'fc6', 4096)
    assert m.param_shapes['fc6_w'] == (4096, 512 * 49) and 'fc7_w' not in m.params
    m = _helper(train)
    assert wsl_heads.add_ResNet_roi_0fc_head(m, 'x', 512, 1. / 16.) == ('roi_feat', 512 * 49)
    assert m.params == [] and [o.type for o in m.net.ops] == ['RoIPoolF', 'RoIFeatureBoost',
                                                                'StopGradient']


def test_cfg_defaults_equal_the_reference(cfgmod):
    c = cfgmod.cfg
    assert dict(c.RESNETS) == GOLD['resnets']
    assert list(c.WSL.MLP_HEAD_DIM) == GOLD['wsl_mlp_head_dim'] == []
    # the reference-format dump of a run that leaves them alone is the text it always was
    import detectron.utils.env as envu
    text = envu.yaml_dump(c, reference_format=True)
    assert 'RESNETS' not in text and 'MLP_HEAD_DIM: []' not in text
    assert 'RESNETS' in envu.yaml_dump(c)
    cfgmod.merge_cfg_from_list(['RESNETS.RES5_DILATION', 2, 'WSL.MLP_HEAD_DIM', '[512, 128]'])
    tree = cfgmod.load_cfg(envu.yaml_dump(c, reference_format=True))
    assert tree['RESNETS']['RES5_DILATION'] == 2 and tree['WSL']['MLP_HEAD_DIM'] == [512, 128]
    assert tree['RESNETS']['TRANS_FUNC'] == 'bottleneck_transformation'


@pytest.mark.parametrize('name', ['flickr_clean', 'flickr_coco'])
def test_tta_yaml_check_still_passes(cfgmod, name):
    """tests/test_tta_host.py's yaml-against-reference check, run again over the grown cfg tree."""
    spec = importlib.util.spec_from_file_location('tta_host', os.path.join(ROOT, 'tests',
                                                                          'test_tta_host.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.test_the_other_hot_path_yamls_match_the_reference_cfg(cfgmod, name)


def test_whole_model_and_refusals(cfgmod):
    import detectron.modeling.model_builder_wsl as mb
    from detectron.core import executor as E
    c = cfgmod
    _cfg(c, ['MODEL.CONV_BODY', CONV5, 'RESNETS.RES5_DILATION', 2])
    for train in (True, False):
        m = mb.create(c.cfg.MODEL.TYPE, train=train)
        want = GOLD['conv5_d2_%s' % ('train' if train else 'test')]
        n = len(want['ops'])
        assert [o.outputs[0] for o in m.net.ops[:n]] == [w[2][0] for w in want['ops']]
        assert m.net.ops[n].type == 'StopGradient' and m.net.ops[n].inputs == ['res5_1_sum']
        assert m.net.ops[n + 1].type == 'RoIPoolF' and m.net.ops[n + 1].args['spatial_scale'] == 1 / 16.
        assert E.canonical_na_wsddn_signature(train, 21) is None      # no fused chain: op by op
    m = mb.create(c.cfg.MODEL.TYPE, train=True)
    body = [p for p, _s in GOLD['conv5_d2_train']['params']]
    assert m.params[:len(body)] == body
    assert sorted(m.TrainableParams()) == ['fc6_b', 'fc6_w', 'fc7_b', 'fc7_w', 'fc8c_b', 'fc8c_w',
                                           'fc8d_b', 'fc8d_w']
    assert not [g for g in m.grad_ops if g.type.startswith(('RoI', 'Conv', 'MaxPool', 'Affine', 'Sum'))]
    c.merge_cfg_from_list(['WSL.OICR', True])
    m = mb.create(c.cfg.MODEL.TYPE, train=True)
    assert not set(body) & set(m.TrainableParams()) and 'cls_score3_w' in m.TrainableParams()
    c.merge_cfg_from_list(['WSL.OICR', False])
    # every refusal names its key
    for key, value, where in (('TRAIN.FREEZE_CONV_BODY', False, 'train'),
                              ('RESNETS.TRANS_FUNC', 'bottleneck_transformation', 'both'),
                              ('RESNETS.STEM_FUNC', 'basic_gn_stem', 'both'),
                              ('RESNETS.SHORTCUT_FUNC', 'basic_gn_shortcut', 'both'),
                              ('RESNETS.NUM_GROUPS', 2, 'both'),
                              ('WSL.CONTEXT', True, 'both')):
        node, leaf = key.split('.')
        old = c.cfg[node][leaf]
        c.merge_cfg_from_list([key, value])
        with pytest.raises(NotImplementedError, match=key.replace('.', r'\.')):
            mb.create(c.cfg.MODEL.TYPE, train=True)
        if where == 'both':
            with pytest.raises(NotImplementedError, match=key.replace('.', r'\.')):
                mb.create(c.cfg.MODEL.TYPE, train=False)
        else:
            mb.create(c.cfg.MODEL.TYPE, train=False)                  # inference never asks
        c.merge_cfg_from_list([key, old])
    mb.create(c.cfg.MODEL.TYPE, train=True)
    from detectron.modeling import wsl_heads
    c.merge_cfg_from_list(['WSL.CONTEXT', True])
    for fn in (wsl_heads.add_ResNet_roi_0fc_head, wsl_heads.add_ResNet_roi_1fc_head,
               wsl_heads.add_ResNet_roi_context_0fc_head, wsl_heads.add_ResNet_roi_context_2fc_head):
        with pytest.raises(NotImplementedError, match=r'WSL\.CONTEXT'):
            fn(_helper(True), 'x', 512, 1. / 16.)
    with pytest.raises(NotImplementedError, match='group'):
        _helper(True).Conv('x', 'y', 64, 64, 3, group=2)


def test_helper_and_table_entries():
    from detectron.core import op_table as T
    m = _helper(True)
    assert m.Conv('x', 'c', 64, 128, 1, stride=2, no_bias=1) == 'c'
    assert m.net.ops[-1].inputs == ['x', 'c_w'] and 'c_b' not in m.params
    assert m.net.ops[-1].args == {'stride': 2, 'kernel': 1}
    assert m.AffineChannel('c', 'c_bn', dim=128) == 'c_bn'
    assert m.AffineChannel('c', 'c_bn2', dim=128, inplace=True) == 'c'
    assert m.param_inits['c_bn_s'] == ('ConstantFill', {'value': 1.0})
    assert m.param_inits['c_bn_b'] == ('ConstantFill', {'value': 0.0})
    assert 'c_bn_s' in m.weights and 'c_bn_b' in m.biases
    assert m.ConvAffine('x', 'd', 64, 64, 3, 1, 1, inplace=True) == 'd'
    assert [o.type for o in m.net.ops[-2:]] == ['Conv', 'AffineChannel']
    assert m.Conv('x', 'e', 64, 64, 3, pad=1, stride=1) == 'e' and m.net.ops[-1].inputs == ['x', 'e_w', 'e_b']
    for t in ('AffineChannel', 'Sum'):
        e = T.TABLE[t]
        assert e.grad_inputs is None and e.gradient is None and not e.cuts and e.state is None
    assert T.TABLE['AffineChannel'].n_in == 3 and T.TABLE['Sum'].n_in == 2 and T.TABLE['Conv'].n_in == 3
    # a Conv op without a pad argument has pad 0 (the 1x1 shortcuts), not O.Conv's keyword default
    assert T._conv(m.net.ops[0]) == {'pad': 0, 'stride': 2, 'kernel': 1}
    import detectron.ops as O
    with pytest.raises(O.NawsError):
        O.Sum(torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3, 4))


# ------------------------------------------------------------------------- float64 reference ----
def test_reference_agrees_with_unfold_matmul():
    """conv64 against im2col (F.unfold) + matmul on the strided layer forms, in float64."""
    g = torch.Generator().manual_seed(1)
    for cin, cout, k, s, p, d, h, w in ((3, 8, 7, 2, 3, 1, 19, 14), (8, 16, 3, 2, 1, 1, 9, 12),
                                        (8, 16, 1, 2, 0, 1, 9, 12), (8, 8, 3, 1, 2, 2, 5, 6)):
        x = torch.randn((2, cin, h, w), generator=g, dtype=torch.float64)
        wt = torch.randn((cout, cin, k, k), generator=g, dtype=torch.float64)
        got = rref.conv64(x, wt, s, p, d)
        ho, wo = (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1
        cols = F.unfold(x, k, dilation=d, padding=p, stride=s)                  # [2, cin*k*k, ho*wo]
        want = (wt.reshape(cout, -1) @ cols).reshape(2, cout, ho, wo)
        assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12
        # the shifted (wrong) form is the same sum over a window that starts `pad` further on
        bad = rref.conv64(x, wt, s, p, d, shifted=True)
        assert bad.shape == want.shape
        assert (p == 0) == bool(float((bad - want).abs().max()) < 1e-12)


@pytest.mark.parametrize('body,dilation,shape', [('conv5', 1, (1, 512, 3, 3)), ('conv5', 2, (1, 512, 5, 6)),
                                                 ('conv4', 1, (1, 256, 5, 6))])
def test_each_wrong_variant_moves_the_output(body, dilation, shape):
    ref = rref.reference(body, dilation)
    assert ref['fmap'].shape == shape and ref['scale'] == rref.scale_of(body, dilation)
    assert rref.channel_error(ref['fmap'], ref['fmap'], ref['rms']) == 0.0
    blobs, mb = rref.inputs()
    for wrong in ('pad0', 'sc_affine', 'res2'):
        bad, brms = rref.body64(mb['data'], blobs, body, dilation, wrong=wrong)
        assert bad.shape == shape
        assert rref.channel_error(ref['fmap'], bad.numpy(), brms) >= 1e-2, wrong
    # an omitted affine shows: scales and shifts are far from (1, 0)
    assert all(float((blobs[n] - 1).abs().mean()) > 0.2 for n in blobs if n.endswith('_bn_s'))
    if body == 'conv5' and dilation == 1:
        assert np.isfinite(ref['loss']) and ref['logits'].shape == (rref.R, 2 * rref.NFG)


# ------------------------------------------------------------------------------------ C ABI ----
def _ptrs():
    p = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    a = p(base + (-base) % 16)
    return buf, a, p(a.value + 4), p(0)


def test_new_entries_validate_before_any_launch():
    from naws_hip import lib
    L = lib.load()
    _buf, a, off, none = _ptrs()
    # naws_conv2d_nhwc_fwd(X, Wp, bias, N, H, W, Cin, Cout, kernel, stride, pad, dilation, relu, Y, stream)
    conv = lambda **k: L.naws_conv2d_nhwc_fwd(
        k.get('x', a), k.get('wp', a), k.get('bias', none), k.get('N', 1), k.get('H', 8), k.get('W', 8),
        k.get('Cin', 32), k.get('Cout', 32), k.get('kernel', 3), k.get('stride', 2), k.get('pad', 1),
        k.get('dilation', 1), 0, k.get('y', a), none)
    for dim in ('N', 'H', 'W', 'Cin', 'Cout'):
        assert conv(**{dim: 0}) == lib.ERR_SHAPE and conv(**{dim: -2}) == lib.ERR_SHAPE, dim
    for bad in (dict(kernel=2), dict(kernel=5), dict(kernel=0), dict(stride=0), dict(stride=3),
                dict(dilation=0), dict(dilation=3), dict(pad=-1), dict(pad=3), dict(kernel=1, pad=1),
                dict(kernel=7, pad=7), dict(dilation=2, pad=5)):
        assert conv(**bad) == lib.ERR_ARG, bad
    assert conv(dilation=2, pad=4, H=9, W=9, x=none) == lib.ERR_NULL       # pad <= dilation * (kernel-1)
    for bad in (dict(Cout=48), dict(Cin=16), dict(Cin=4), dict(Cin=33)):
        assert conv(**bad) == lib.ERR_UNSUPPORTED, bad
    assert conv(Cin=3, x=none) == lib.ERR_NULL                             # Cin 3 is accepted
    assert conv(kernel=7, pad=0, H=6) == lib.ERR_SHAPE and conv(kernel=7, pad=0, W=6) == lib.ERR_SHAPE
    assert conv(kernel=3, pad=0, dilation=2, H=4) == lib.ERR_SHAPE        # Ho < 1
    for ptr in ('x', 'wp', 'y'):
        assert conv(**{ptr: none}) == lib.ERR_NULL and conv(**{ptr: off}) == lib.ERR_ARG, ptr
    assert conv(N=0, x=none) == lib.ERR_SHAPE and conv(kernel=5, x=none) == lib.ERR_ARG
    assert conv(Cin=16, x=none) == lib.ERR_UNSUPPORTED
    # naws_conv2d_pack_weight(W_oihw, Cout, Cin, kernel, Wp, stream)
    pack = lambda **k: L.naws_conv2d_pack_weight(k.get('w', a), k.get('Cout', 32), k.get('Cin', 32),
                                                 k.get('kernel', 3), k.get('wp', a), none)
    assert pack(Cout=0) == lib.ERR_SHAPE and pack(Cin=-1) == lib.ERR_SHAPE
    assert pack(kernel=5) == lib.ERR_ARG and pack(Cout=40) == lib.ERR_UNSUPPORTED
    assert pack(Cin=5) == lib.ERR_UNSUPPORTED
    assert pack(w=none) == lib.ERR_NULL and pack(wp=none) == lib.ERR_NULL
    assert [L.naws_conv2d_packed_k(c, k) for c, k in ((3, 7), (64, 3), (64, 1), (32, 7), (3, 3), (3, 5),
                                                      (0, 3))] == [160, 576, 64, 1568, 32, 0, 0]
    assert L.naws_conv2d_max_grid_m() >= 256
    # naws_affine_channel_fwd(X, scale, shift, N, C, HW, relu, Y, stream)
    aff = lambda **k: L.naws_affine_channel_fwd(k.get('x', a), k.get('s', a), k.get('b', a), k.get('N', 1),
                                                k.get('C', 2), k.get('HW', 3), 0, k.get('y', a), none)
    for dim in ('N', 'C', 'HW'):
        assert aff(**{dim: 0}) == lib.ERR_SHAPE and aff(**{dim: -1}) == lib.ERR_SHAPE, dim
    for ptr in ('x', 's', 'b', 'y'):
        assert aff(**{ptr: none}) == lib.ERR_NULL, ptr
    assert aff(N=0, x=none) == lib.ERR_SHAPE
    import detectron.ops as O
    assert O.Conv.__defaults__ == (None, 3, 1, 1, 1, False)
    assert O.AffineChannel.__defaults__ == (False, None)


def test_header_with_the_new_entries_is_plain_c_and_cpp(tmp_path):
    hdr = os.path.join(ROOT, 'include', 'naws.h')
    src = tmp_path / 'use.c'
    src.write_text('#include "naws.h"\n'
                   'int (*f1)(const float*, const float*, const float*, int, int, int, int, int, int,\n'
                   '          int, int, int, int, float*, void*) = naws_conv2d_nhwc_fwd;\n'
                   'int (*f2)(const float*, int, int, int, float*, void*) = naws_conv2d_pack_weight;\n'
                   'int (*f3)(const float*, const float*, const float*, int, int, int64_t, int, float*,\n'
                   '          void*) = naws_affine_channel_fwd;\n'
                   'int64_t (*f4)(int, int) = naws_conv2d_packed_k;\n')
    for cc, lang in (('gcc', 'c'), ('g++', 'c++')):
        subprocess.check_call([cc, '-fsyntax-only', '-Wall', '-Werror', '-x', lang, hdr])
        subprocess.check_call([cc, '-fsyntax-only', '-Wall', '-Werror', '-Wno-unused-variable',
                               '-I', os.path.join(ROOT, 'include'), '-x', lang, str(src)])
    from naws_hip import lib
    for name in ('naws_conv2d_nhwc_fwd', 'naws_conv2d_pack_weight', 'naws_affine_channel_fwd',
                 'naws_conv2d_packed_k', 'naws_conv2d_max_grid_m'):
        assert name in lib.ALL_SYMBOLS and hasattr(lib.load(), name)
    text = open(hdr).read()
    assert 'UNPINNED' in text.split('naws_conv2d_packed_k')[0][-1500:]
    assert 'conv2d.hip' in open(os.path.join(ROOT, 'na-fwebsod_amd', 'csrc', 'Makefile')).read()
