"""FAST_RCNN.ROI_XFORM_METHOD RoIAlign without a GPU: the float64 reference against an independent
grid_sample formulation (and five wrong restatements the bound must reject), the builders against
the op trace recorded from the reference (tests/golden/make_golden_roi_align.py), the backward
plan, the plan choice, the unchanged RoIPoolF graphs and the C ABI of the two entries."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import roi_align_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
GOLD = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_roi_align.json')))
BEFORE = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'roipoolf_signatures_before.json')))
ALIGN = ['FAST_RCNN.ROI_XFORM_METHOD', 'RoIAlign', 'FAST_RCNN.ROI_XFORM_SAMPLING_RATIO', 2]
WSDDN = ['WEBLY.WEBLY_ON', False, 'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head']
MODELS = [('na_wsddn_train', [], True), ('na_wsddn_test', [], False), ('wsddn_train', WSDDN, True)]
TOL = 1e-12           # float64 against float64, of max|X| (resp. max|dY|)
C = 5


def _x(seed=0):
    return np.random.default_rng(seed).standard_normal(
        (ref.MAP_N, C, ref.MAP_H, ref.MAP_W)).astype(np.float32)


def _pair(x, rois, ph, pw, scale, sampling, seed=1):
    """max |literal - grid| of the forward and of the backward, over max|X| and max|dY|."""
    y, n, S = ref.forward64(x, rois, ph, pw, scale, sampling)
    yg = ref.forward_grid(x, rois, ph, pw, scale, sampling)
    dy = np.random.default_rng(seed).standard_normal(y.shape)
    dx, T, A = ref.backward64(dy, rois, x.shape, scale, sampling)
    dg = ref.backward_grid(dy, rois, x.shape, scale, sampling)
    assert y.shape == yg.shape == (len(rois), C, ph, pw) and dx.shape == dg.shape == x.shape
    ef = float(np.abs(y - yg).max()) / float(np.abs(x).max()) if y.size else 0.0
    eb = float(np.abs(dx - dg).max()) / float(np.abs(dy).max()) if dy.size else 0.0
    return ef, eb, (y, n, S, dx, T, A)


# ------------------------------------------------------------------------------- reference ----
@pytest.mark.parametrize('sampling', ref.SAMPLINGS)
@pytest.mark.parametrize('ph,pw', ref.POOLINGS)
def test_reference_against_grid_sample(ph, pw, sampling):
    x = _x()
    ef, eb, (y, n, S, dx, T, A) = _pair(x, ref.case_rois(), ph, pw, 0.125, sampling)
    print('%dx%d sampling %d: forward %.3g backward %.3g (of the bound %.0e)'
          % (ph, pw, sampling, ef, eb, TOL))
    assert ef <= TOL and eb <= TOL
    names = [k for k, _ in ref.CASE_ROIS]
    out = names.index('wholly_outside')
    assert not y[out].any() and not n[out].any() and not S[out].any()      # exact zeros
    assert y[names.index('reversed')].any()          # max(., 1): a 1 x 1 roi at (x1, y1), not empty
    assert (n[names.index('interior')] > 0).all()
    # the term counts: 4 per valid sample pair; dX's window is where T > 0
    assert n.max() <= 4 * (max(sampling, 1) if sampling else 17 * 13) ** 2
    assert (np.abs(dx)[np.broadcast_to(T == 0, dx.shape)] == 0).all()
    assert (A >= np.abs(dx) - 1e-12).all() and (S >= np.abs(y) - 1e-12).all()


def test_reference_against_grid_sample_other_scale():
    ef, eb, _ = _pair(_x(2), ref.case_rois(), 7, 7, 0.0625, 0)
    assert ef <= TOL and eb <= TOL


@pytest.mark.parametrize('name,roi', ref.INVALID_ROIS)
def test_reference_invalid_rois(name, roi):
    """A batch index outside [0,N), a NaN coordinate, an adaptive grid above 1024: Y = 0, no
    gradient, in both formulations."""
    rois = np.array([ref.CASE_ROIS[0][1], roi], np.float32)
    ef, eb, (y, n, S, dx, T, A) = _pair(_x(3), rois, 7, 7, 0.125, 0)
    assert ef <= TOL and eb <= TOL
    assert not y[1].any() and not n[1].any() and y[0].any()
    _, _, _, dx0, T0, _ = _pair(_x(3), rois[:1], 7, 7, 0.125, 0)[2]
    assert np.array_equal(T, T0)
    if name == 'cap_1024':
        # (valid as a whole there - the cap is on the ADAPTIVE grid - though no sample of its
        # 17857-pixel bins falls on the map)
        ef, eb, _ = _pair(_x(3), rois, 7, 7, 0.125, 2)
        assert ef <= TOL and eb <= TOL
        assert ref.roi_geometry(rois[1], 7, 7, 0.125, 2, 2, 13, 17) is not None
        assert ref.roi_geometry(rois[1], 7, 7, 0.125, 0, 2, 13, 17) is None


@pytest.mark.parametrize('count', [0, 1, 130])
def test_reference_roi_counts(count):
    rois = ref.rois_many(count)
    ef, eb, (y, n, S, dx, T, A) = _pair(_x(4), rois, 7, 7, 0.125, 0)
    assert ef <= TOL and eb <= TOL and y.shape[0] == count
    if count == 0:
        assert not dx.any() and not T.any()


# case on which each wrong restatement must miss the bound by >= 100x (forward AND backward)
SHARP = {'aligned': 'interior', 'rounded': 'interior', 'no_max': 'sub_pixel',
         'clamp': 'outside_low', 'floor': 'interior'}


@pytest.mark.parametrize('variant', ref.VARIANTS)
def test_reference_is_sharp(variant):
    """The half-pixel shift of aligned = true, roi coordinates rounded as RoIPoolF does, no
    max(., 1), clamping instead of zero beyond [-1, H], floor for the adaptive grid: each misses
    the 1e-12 bound by at least 100x on its named case (7 x 7, adaptive sampling)."""
    names = [k for k, _ in ref.CASE_ROIS]
    rois = ref.case_rois()[names.index(SHARP[variant])][None]
    x = _x(5)
    y, _, _ = ref.forward64(x, rois, 7, 7, 0.125, 0)
    yw, _, _ = ref.forward64(x, rois, 7, 7, 0.125, 0, variant)
    ywg = ref.forward_grid(x, rois, 7, 7, 0.125, 0, variant)
    dy = np.random.default_rng(6).standard_normal(y.shape)
    dx, _, _ = ref.backward64(dy, rois, x.shape, 0.125, 0)
    dw, _, _ = ref.backward64(dy, rois, x.shape, 0.125, 0, variant)
    ef = float(np.abs(y - yw).max() / np.abs(x).max())
    eb = float(np.abs(dx - dw).max() / np.abs(dy).max())
    print('%s on %s: forward %.3g backward %.3g' % (variant, SHARP[variant], ef, eb))
    assert ef >= 100 * TOL and eb >= 100 * TOL
    # (the wrong geometry is wrong in both formulations alike: they still agree with each other)
    assert float(np.abs(yw - ywg).max() / np.abs(x).max()) <= TOL


# ------------------------------------------------------------------------------- builders ----
def _create(c, extra, train=True, frozen=True):
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 4, 'TRAIN.FREEZE_CONV_BODY', frozen] + extra)
    c.assert_and_infer_cfg(make_immutable=False)
    import detectron.modeling.model_builder_wsl as mb
    return mb.create(c.cfg.MODEL.TYPE, train=train)


def _norm(ops_, want):
    """The recorded form (tests/test_trainable_body_graph.py): helper-made Conv / FC carry their
    data input only, Dropout its first output, uuid is random per build."""
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


@pytest.mark.parametrize('frozen', [True, False])
@pytest.mark.parametrize('key,extra,train', MODELS)
def test_builders_reproduce_reference_trace(cfgmod, key, extra, train, frozen):
    assert GOLD['roi_xform_method'] == 'RoIAlign' and GOLD['sampling_ratio'] == 2
    m = _create(cfgmod, ALIGN + extra, train=train, frozen=frozen)
    want = GOLD['frozen' if frozen else 'trainable'][key]
    assert len(m.net.ops) == len(want['ops'])
    got = _norm(m.net.ops, want['ops'])
    assert [g[:3] for g in got] == [w[:3] for w in want['ops']]
    roi = [(g, w) for g, w in zip(got, want['ops']) if g[0] == 'RoIAlign']
    assert len(roi) == 1
    g, w = roi[0]
    assert g[2] == ['roi_feat'] and w[2] == ['roi_feat']                  # ONE output
    assert g[3] == w[3] == dict(pooled_h=7, pooled_w=7, spatial_scale=0.125, sampling_ratio=2)
    assert not [b for o in m.net.ops for b in o.outputs if b.startswith('_argmax_')]
    assert not [o for o in m.net.ops if o.type == 'RoIPoolF']
    assert m.losses == want['losses'] and m.metrics == want['metrics']


@pytest.mark.parametrize('key,extra', [('na_wsddn_train', []), ('wsddn_train', WSDDN)])
def test_backward_plan_through_roi_align(cfgmod, key, extra):
    m = _create(cfgmod, ALIGN + extra, frozen=False)
    types = [o.type for o in m.grad_ops]
    first = types.index('RoIFeatureBoostGradient')
    body = ['RoIFeatureBoostGradient', 'RoIAlignGradient']
    for blk in (5, 4, 3):
        for _ in range(3):
            body += ['ReluGradient', 'ConvGradient']
        if blk > 3:
            body.append('MaxPoolGradient')
    assert types[first:] == body
    roi = m.grad_ops[first + 1]
    assert roi.inputs == ['conv5_3', 'rois', 'roi_feat']                  # X, R | Y
    assert roi.outputs == ['conv5_3_grad'] and roi.args['_gout'] == ['roi_feat_grad']
    assert roi.args['_gin'] == ['conv5_3_grad', None] and roi.args['sampling_ratio'] == 2
    last = m.grad_ops[-1]
    assert last.type == 'ConvGradient' and last.inputs[3] == 'conv3_1'
    assert 'conv3_1_w' in m.TrainableParams() and 'conv2_2_w' not in m.TrainableParams()
    # the frozen plan: the StopGradient on roi_feat cuts the flow as it does for RoIPoolF
    cfgmod.reset_cfg()
    f = _create(cfgmod, ALIGN + extra, frozen=True)
    assert not [o for o in f.grad_ops if o.type.startswith(('RoI', 'Conv', 'MaxPool'))]


def test_other_heads_build_with_roi_align(cfgmod):
    for extra in (WSDDN + ['WSL.OICR', True], WSDDN + ['WSL.CENTER_LOSS', True],
                  ['WSL.MIN_ENTROPY_LOSS', True], WSDDN + ['WSL.CONTEXT', True]):
        for frozen in (True, False):
            if 'WSL.CONTEXT' in extra and not frozen:
                continue
            cfgmod.reset_cfg()
            m = _create(cfgmod, ALIGN + extra, frozen=frozen)
            assert [o.type for o in m.net.ops].count('RoIAlign') == 1
            assert [o.type for o in m.grad_ops].count('RoIAlignGradient') == (0 if frozen else 1)
    # the plain stream of the contextual head pools with RoIAlign, the other two with RoILoopPool
    pools = [o.type for o in m.net.ops if o.type in ('RoIAlign', 'RoILoopPool', 'RoIPoolF')]
    assert sorted(pools) == ['RoIAlign', 'RoILoopPool', 'RoILoopPool']


def test_roi_align_never_takes_the_fused_plan(cfgmod):
    """The canonical na_wsddn signature is built under the current cfg, so with RoIAlign it matches
    the model's: without the clause in fused_ok the engine would run RoIPoolF in its place."""
    import torch
    from detectron.core import executor as E
    m = _create(cfgmod, ALIGN, frozen=True)
    assert E._signature(m.net.ops) == E.canonical_na_wsddn_signature(True, m.num_classes)
    assert E.NetExecutor(m, torch.device('cpu')).plan == 'interpreted'
    t = _create(cfgmod, ALIGN, train=False, frozen=True)
    assert E.NetExecutor(t, torch.device('cpu')).plan == 'interpreted'
    src = open(os.path.join(ROOT, 'na-fwebsod_amd', 'detectron', 'core', 'executor.py')).read()
    assert "cfg.FAST_RCNN.ROI_XFORM_METHOD == 'RoIPoolF' and" in src


def test_roipoolf_builds_are_unchanged():
    """With ROI_XFORM_METHOD RoIPoolF every forward and backward op list equals what the parent
    commit built (digests recorded there by tests/golden/make_golden_roipoolf_signatures.py)."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    try:
        import make_golden_roipoolf_signatures as sig
        now = sig.record()
    finally:
        sys.path.pop(0)
    assert sorted(now) == sorted(BEFORE) and len(BEFORE) == 14
    assert now == BEFORE


# ----------------------------------------------------------------------------------- C ABI ----
def test_entries_validate_before_any_launch():
    """SHAPE for R < 0 or a non-positive dim, ARG for sampling_ratio < 0 or a spatial_scale that is
    not > 0, NULL for a missing pointer, UNSUPPORTED beyond the LDS staging - in that order, all
    before a launch (this runs without a GPU)."""
    from naws_hip import lib
    L = lib.load()
    p = ctypes.c_void_p
    buf = (ctypes.c_float * 64)()
    a, none = ctypes.cast(buf, p), p(0)
    # naws_roi_align_fwd(X, N, C, H, W, rois, R, ph, pw, scale, sampling, Y, stream)
    fwd = lambda **k: L.naws_roi_align_fwd(
        k.get('x', a), k.get('N', 1), k.get('C', 32), k.get('H', 8), k.get('W', 8), k.get('rois', a),
        k.get('R', 4), k.get('ph', 7), k.get('pw', 7), k.get('scale', 0.125), k.get('sampling', 0),
        k.get('y', a), none)
    # naws_roi_align_bwd(dY, rois, R, N, C, H, W, ph, pw, scale, sampling, dX, stream)
    bwd = lambda **k: L.naws_roi_align_bwd(
        k.get('dy', a), k.get('rois', a), k.get('R', 4), k.get('N', 1), k.get('C', 32),
        k.get('H', 8), k.get('W', 8), k.get('ph', 7), k.get('pw', 7), k.get('scale', 0.125),
        k.get('sampling', 0), k.get('dx', a), none)
    for f in (fwd, bwd):
        for bad in (dict(R=-1), dict(N=0), dict(C=0), dict(H=0), dict(W=-3), dict(ph=0), dict(pw=0)):
            assert f(**bad) == lib.ERR_SHAPE, bad
        assert f(sampling=-1) == lib.ERR_ARG
        for s in (0.0, -0.125, float('nan')):
            assert f(scale=s) == lib.ERR_ARG, s
        assert f(R=-1, sampling=-1, rois=none) == lib.ERR_SHAPE       # the order of the checks
        assert f(sampling=-1, rois=none) == lib.ERR_ARG
        assert f(rois=none) == lib.ERR_NULL
        assert f(rois=none, ph=300, pw=300) == lib.ERR_NULL
        assert f(ph=300, pw=300) == lib.ERR_UNSUPPORTED
        assert f(H=30000) == lib.ERR_UNSUPPORTED                     # the ph*H weight table
    assert fwd(x=none) == lib.ERR_NULL and fwd(y=none) == lib.ERR_NULL
    assert bwd(dy=none) == lib.ERR_NULL and bwd(dx=none) == lib.ERR_NULL
    assert bwd(dx=none, R=0) == lib.ERR_NULL                          # dX is filled also at R == 0
    assert fwd(R=0, x=none, rois=none, y=none) == lib.OK              # nothing to do, no launch
    assert fwd(C=33, rois=none) == lib.ERR_NULL and bwd(C=1, rois=none) == lib.ERR_NULL  # any C > 0


def test_header_with_the_entries_is_plain_c_and_cpp(tmp_path):
    hdr = os.path.join(ROOT, 'include', 'naws.h')
    for cc, lang in (('gcc', 'c'), ('g++', 'c++')):
        subprocess.check_call([cc, '-fsyntax-only', '-Wall', '-Werror', '-x', lang, hdr])
    src = tmp_path / 'use.c'
    src.write_text(
        '#include "naws.h"\n'
        'int (*f1)(const float*, int, int, int, int, const float*, int, int, int, float, int,\n'
        '          float*, void*) = naws_roi_align_fwd;\n'
        'int (*f2)(const float*, const float*, int, int, int, int, int, int, int, float, int,\n'
        '          float*, void*) = naws_roi_align_bwd;\n')
    for cc, lang in (('gcc', 'c'), ('g++', 'c++')):
        subprocess.check_call([cc, '-fsyntax-only', '-Wall', '-Werror', '-Wno-unused-variable',
                               '-I', os.path.join(ROOT, 'include'), '-x', lang, str(src)])
    from naws_hip import lib
    for name in ('naws_roi_align_fwd', 'naws_roi_align_bwd'):
        assert name in lib.ALL_SYMBOLS and hasattr(lib.load(), name)
    doc = open(hdr).read()
    assert 'UNPINNED' in doc and 'reproducible to rounding, not to the bit' in doc


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from naws_hip import ops
    import detectron.ops as O
    with pytest.raises(TypeError):
        ops.roi_align(torch.zeros((1, 4, 8, 8)), torch.zeros((2, 5)))
    with pytest.raises(TypeError):
        ops.roi_align_grad(torch.zeros((2, 4, 7, 7)), torch.zeros((2, 5)), (1, 4, 8, 8))
    assert callable(O.RoIAlign) and callable(O.RoIAlignGradient)
    assert 'RoIAlign' in O.__doc__
