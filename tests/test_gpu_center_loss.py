"""GPU parity of WSL.CENTER_LOSS, the multi-centre feature loss, against the numpy restatement of
tests/center_loss_ref.py: the ops-level functions (selection, centre choice and D bit for bit, the
scalar loss, the feature gradient, the in-place state over a sequence of calls), the error sites,
a captured graph of one forward + update + backward (a capture cannot hold a host
synchronisation), the graph on the op-by-op plan for the plain WSDDN model and for na_wsddn, the
checkpoint, the training tool, and two ranks on one GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import center_loss_ref as clr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
STATE = ('center_feature', 'center_feature_g', 'center_feature_n_u')
EPS = 2.0 ** -23

SHAPES = [(300, 20, 5, 10, 4096), (70, 3, 1, 1, 96), (10, 4, 5, 10, 100), (9, 4, 5, 10, 100),
          (257, 20, 5, 10, 130)]
VARIANTS = ['labels', 'ignore', 'nolabel']


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_case(R, C, M, top_k, Dm, variant='labels', seed=0):
    """Labels cycle through {1, 0.5, 0.49, 0} (classes 0 and 1 are active when there are enough
    rois); all scores are distinct except the planted ones: in class 0 the top_k - 1 best rois are
    followed by an exact tie of two rois (the lower index must win the last place), and the first
    of those two also leads class 1, so one roi serves two classes."""
    rng = np.random.default_rng(1000 * seed + R + C + Dm)
    X = np.array([[1.0, 0.5, 0.49, 0.0][c % 4] for c in range(C)], np.float32)[None, :]
    ignore = -1
    if variant == 'ignore':
        ignore = 0
    elif variant == 'nolabel':
        X = np.where(X >= 0.5, np.float32(0.25), X).astype(np.float32)
    P = ((rng.permutation(R * C) + 1.0) / (R * C + 1.0)).astype(np.float32).reshape(R, C)
    planted = np.zeros((R, C), bool)
    rois = rng.permutation(R)
    lead, pair = rois[:min(top_k - 1, max(R - 2, 0))], np.sort(rois[-2:])
    P[lead, 0] = 3.0 + 0.01 * np.arange(len(lead), dtype=np.float32)
    P[pair, 0] = 2.5
    P[pair[0], 1] = 5.0
    planted[lead, 0] = planted[pair, 0] = planted[pair[0], 1] = True
    F = rng.standard_normal((R, Dm)).astype(np.float32)
    CF = rng.standard_normal((C, M, Dm)).astype(np.float32)
    return dict(X=X, P=P, F=F, CF=CF, ignore=ignore, planted=planted, pair=pair,
                dims=(R, C, M, top_k, Dm))


def check_inputs(case, ref):
    """The conditions on the INPUTS, asserted on the restatement alone: every active class's best
    centre leads the second best by at least 1e-4 of its distance in float64 (an fp32 tree sum of
    this length rounds near 1e-6), and all non-planted scores are distinct."""
    free = case['P'][~case['planted']]
    assert len(np.unique(free)) == free.size
    for row in ref.dots:
        if np.isnan(row).all() or row.size < 2:
            continue
        best, second = np.sort(row)[:2]
        assert second - best >= 1e-4 * best, (best, second)


def reference_forward(case, max_iter=1):
    R, C, M, top_k, Dm = case['dims']
    ref = clr.CenterLossRef(top_k=top_k, update=128, max_iter=max_iter, ignore_label=case['ignore'])
    out = ref.forward(case['X'], case['P'], case['F'], case['CF'])
    check_inputs(case, ref)
    return ref, out


def gpu_forward(case, dev, enabled=True, counts=None):
    from naws_hip import ops
    R, C, M, top_k, Dm = case['dims']
    return ops.center_loss(_t(case['X'], dev).reshape(-1), _t(case['P'], dev), _t(case['F'], dev),
                           _t(case['CF'], dev), top_k, case['ignore'], enabled, counts=counts)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_center_loss_forward(dev, shape, variant):
    from naws_hip import ops
    case = make_case(*shape, variant=variant)
    R, C, M, top_k, Dm = shape
    ref, (L, D, S, picks) = reference_forward(case)
    n_active = int((picks[:, 0] >= 0).sum())
    if R < top_k or variant == 'nolabel':
        assert n_active == 0 and L == 0.0
    elif variant == 'ignore':
        assert picks[0, 0] == -1 and n_active == len([c for c in range(1, C) if c % 4 < 2])
    else:
        assert n_active == len([c for c in range(C) if c % 4 < 2])
        if R > top_k:                      # the tie: only the lower index gets the last place
            assert case['pair'][0] in picks[0] and case['pair'][1] not in picks[0]
        if C > 1:                          # one roi in the selection of two classes
            assert case['pair'][0] in picks[1]
    counts = torch.zeros((C, M), device=dev, dtype=torch.int32)
    gl, gd, gs, ws = gpu_forward(case, dev, counts=counts)
    torch.cuda.synchronize()
    assert np.array_equal(ops.center_loss_picks(ws, C, top_k).cpu().numpy(), picks)
    assert np.array_equal(gs.cpu().numpy(), S)
    assert gd.shape == (C, top_k, Dm)
    assert np.array_equal(_bits(gd.cpu().numpy()), _bits(D))
    got = float(gl[0])
    print('L %.9g (float64 %.9g)' % (got, L))
    assert abs(got - L) <= 1e-5 * abs(L)
    assert np.array_equal(counts.cpu().numpy(), ref.counts)
    if n_active == 0:
        assert got == 0.0 and not gd.any() and bool((gs == -1).all())
    # past max_iter: L = 0, D = 0, S = -1 whatever the inputs
    gl, gd, gs, ws = gpu_forward(case, dev, enabled=False)
    assert float(gl[0]) == 0.0 and not gd.any() and bool((gs == -1).all())
    assert bool((ops.center_loss_picks(ws, C, top_k) == -1).all())


def test_center_loss_runs_out_of_rois_is_nan(dev):
    """An active class with fewer than top_k selectable scores (NaN and -FLT_MAX never win): the
    reference fails the net (center_loss_op.cu:161-166); here the loss is NaN and the training
    loop's NaN stop fires."""
    case = make_case(70, 3, 2, 4, 96)
    case['P'][:, 0] = np.nan
    case['P'][:3, 0] = [0.5, -clr.FLT_MAX, 0.25]
    assert clr.select(case['X'], case['P'], 4) is None
    gl, gd, gs, ws = gpu_forward(case, dev)
    assert bool(torch.isnan(gl[0]))
    assert float(gs[0]) == -1.0 and float(gs[1]) >= 0       # the other class is still served


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_center_loss_backward(dev, shape, variant):
    """dF against float64 within (labelled classes + 1) * 2^-23 * max|dF| (one rounding per
    accumulation into an element; FMA contraction is on in the build); rows of unselected rois are
    exactly zero; this iteration's dCF / ndCF; two runs are bit-identical."""
    from naws_hip import ops
    case = make_case(*shape, variant=variant, seed=1)
    R, C, M, top_k, Dm = shape
    ref, (L, D, S, picks) = reference_forward(case)
    dl = float(np.float32(0.4096))         # the seed blob is float32
    dCF, ndCF = np.full((C, M, Dm), 7.0), np.full((C, M), 7.0)
    want = ref.gradient(D, S, picks, dl, R, case['CF'].astype(np.float64), dCF, ndCF)
    runs = []
    for _ in range(2):
        gl, gd, gs, ws = gpu_forward(case, dev)
        g_dcf = torch.full((C, M, Dm), 7.0, device=dev)
        g_ndcf = torch.full((C, M), 7.0, device=dev)
        df = ops.center_loss_grad(gd, gs, torch.full((1,), dl, device=dev), R, ws, g_dcf, g_ndcf)
        torch.cuda.synchronize()
        runs.append([x.cpu().numpy() for x in (gl, gd, gs, df, g_dcf, g_ndcf)])
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b))
    df, g_dcf, g_ndcf = runs[0][3:]
    labelled = int((picks[:, 0] >= 0).sum())
    bound = (labelled + 1) * EPS * np.abs(want).max()
    err = np.abs(df - want).max()
    print('dF max %.4g  max err %.3g  bound %.3g' % (np.abs(want).max(), err, bound))
    assert df.shape == (R, Dm) and err <= bound
    unselected = np.setdiff1d(np.arange(R), picks[picks >= 0])
    assert not df[unselected].any()
    if labelled:
        assert df.any()
    assert np.array_equal(g_ndcf, ndCF.astype(np.float32))
    # -sum_k D[c][k] in sequence: top_k - 1 roundings, each at most 2^-24 of sum_k |D|
    tol = top_k * 2.0 ** -24 * np.abs(D.astype(np.float64)).sum(1).max()
    assert np.abs(g_dcf - dCF).max() <= tol
    inactive = picks[:, 0] < 0
    assert not g_dcf[inactive].any() and not g_ndcf[inactive].any()


def test_center_loss_state_sequence(dev):
    """2 * update + 1 calls of the operator object with update = 3, max_iter = 6, new inputs every
    call and dCF / ndCF doubled between calls (what a two-rank sum of equal contributions does):
    after every call dCF, ndCF, CF, the accumulators and the display counters against the
    restatement.  Covers the first-call zeroing of loaded non-zero state, the one-iteration lag,
    the update that excludes the iteration that triggers it, and the max_iter cut-off.
    Bounds: dCF as in the backward test; an accumulator after j additions carries j doubled dCF
    errors and j roundings of at most 2^-24 max|acc|; CF within 1e-6 max|CF|.  After a checked
    centre update the restatement continues from the device's float32 centres, so that every call
    is compared from the same starting state."""
    import detectron.ops as O
    R, C, M, top_k, Dm = 40, 4, 3, 4, 36
    update, max_iter = 3, 6
    lines = []
    op = O.CenterLoss(top_k=top_k, update=update, lr=0.5, display=4, max_iter=max_iter,
                      printer=lines.append)
    ref = clr.CenterLossRef(top_k=top_k, update=update, lr=0.5, display=4, max_iter=max_iter)
    first = make_case(R, C, M, top_k, Dm, seed=10)
    CF = first['CF'].astype(np.float64)
    dCF, ndCF = np.full((C, M, Dm), 3.0), np.full((C, M), 5.0)      # loaded, non-zero
    g_cf, g_dcf, g_ndcf = _t(CF, dev), _t(dCF, dev), _t(ndCF, dev)
    dl = torch.full((1,), 0.4096, device=dev)
    since_zero, tol_in = 0, 0.0         # additions since the accumulators were zeroed; their inputs' error
    for it in range(1, 2 * update + 2):
        case = make_case(R, C, M, top_k, Dm, seed=10 + it)
        case['CF'] = CF.astype(np.float32)
        L, D, S, picks = ref.forward(case['X'], case['P'], case['F'], CF)
        if it <= max_iter:
            check_inputs(case, ref)
        gl, gd, gs, gp = op.forward(_t(case['X'], dev), _t(case['P'], dev), _t(case['F'], dev), g_cf,
                                    g_dcf, g_ndcf)
        assert np.array_equal(gp.cpu().numpy(), picks) and np.array_equal(gs.cpu().numpy(), S)
        assert np.array_equal(_bits(gd.cpu().numpy()), _bits(D))
        assert abs(float(gl) - L) <= 1e-5 * abs(L)
        before = (CF.copy(), dCF.copy(), ndCF.copy())
        want = ref.gradient(D, S, picks, float(np.float32(0.4096)), R, CF, dCF, ndCF)
        df = op.gradient(gd, gs, dl, R, g_cf, g_dcf, g_ndcf).cpu().numpy()
        labelled = int((picks[:, 0] >= 0).sum())
        assert np.abs(df - want).max() <= (labelled + 1) * EPS * np.abs(want).max()
        tol_d = top_k * 2.0 ** -24 * max(np.abs(D.astype(np.float64)).sum(1).max(), 1e-30)
        if it > max_iter:       # cut off: nothing moves, dF = 0
            assert L == 0.0 and not df.any()
            for a, b in zip(before, (CF, dCF, ndCF)):
                assert np.array_equal(a, b)
        else:
            assert df.any()
            since_zero = 0 if it % update == 0 else since_zero + (it > 1)
        assert np.array_equal(g_ndcf.cpu().numpy(), ndCF.astype(np.float32))
        # (past max_iter the blobs are not rewritten: they hold call 6's, doubled with its rounding)
        assert np.abs(g_dcf.cpu().numpy() - dCF).max() <= (tol_d if it <= max_iter else 2 * tol_in)
        assert np.array_equal(op.acc_ndCF.cpu().numpy(), ref.acc_ndCF.astype(np.float32))
        tol_a = since_zero * (2 * tol_in + 2.0 ** -24 * np.abs(ref.acc_dCF).max())
        assert np.abs(op.acc_dCF.cpu().numpy() - ref.acc_dCF).max() <= tol_a
        tol_in = max(tol_in, tol_d)
        if it % update == 0 and it <= max_iter:
            assert not ref.acc_dCF.any() and not op.acc_dCF.any()
            assert not np.array_equal(CF, before[0])                   # the centres moved
        elif 1 < it <= max_iter:
            assert ref.acc_ndCF.any()                                   # last call's contribution, lagged
            assert np.array_equal(CF, before[0])
        else:
            assert np.array_equal(CF, before[0])
        got_cf = g_cf.cpu().numpy()
        assert np.abs(got_cf - CF).max() <= 1e-6 * np.abs(CF).max()
        CF[...] = got_cf
        # the two-rank sum of equal contributions
        dCF *= 2
        ndCF *= 2
        g_dcf.mul_(2)
        g_ndcf.mul_(2)
    assert op.cur_iter == op.cur_iter_grad == max_iter == ref.cur_iter
    # the display line at call 1 and every `display` calls, the counters zeroed after each
    assert [l for l in lines if l.startswith('CenterLoss #iter_: ')][0].startswith(
        'CenterLoss #iter_: 1 #loss_: ')
    assert len([l for l in lines if l.startswith('CenterLoss #iter_: ')]) == 2      # calls 1 and 4
    assert int(op.counts.sum()) == 2 * 2                    # calls 5 and 6, two active classes each


def test_center_loss_small_and_empty_inputs(dev):
    """n < top_k is no error (every class inactive) and n == 0 succeeds; CPU tensors are refused."""
    from naws_hip import ops
    C, M, top_k, Dm = 4, 2, 3, 8
    x = torch.ones((C,), device=dev)
    cf = torch.randn((C, M, Dm), device=dev)
    for n in (0, 2):
        p, f = torch.rand((n, C), device=dev), torch.randn((n, Dm), device=dev)
        L, D, S, ws = ops.center_loss(x, p, f, cf, top_k)
        dcf, ndcf = torch.ones_like(cf), torch.ones((C, M), device=dev)
        df = ops.center_loss_grad(D, S, torch.ones((1,), device=dev), n, ws, dcf, ndcf)
        assert float(L[0]) == 0.0 and not D.any() and bool((S == -1).all())
        assert df.shape == (n, Dm) and not df.any() and not dcf.any() and not ndcf.any()
    with pytest.raises(TypeError):
        ops.center_loss(x.cpu(), p, f, cf, top_k)
    with pytest.raises(TypeError):
        ops.center_loss_grad(D.cpu(), S, torch.ones((1,), device=dev), n, ws, dcf, ndcf)
    with pytest.raises(TypeError):
        ops.center_loss_update(cf.cpu(), dcf, ndcf, torch.zeros_like(dcf), torch.zeros_like(ndcf))
    with pytest.raises(ops.L.NawsError):
        ops.center_loss(x[:3].contiguous(), p, f, cf, top_k)         # ENFORCE :42


def test_center_loss_refuses_mismatched_buffers(dev):
    """A caller-supplied workspace sized for other (c, m, top_k), a counts that is not [c, m] and
    an out that is not [n, d] would be written out of bounds: SHAPE, before any launch."""
    from naws_hip import ops
    n, C, M, top_k, Dm = 12, 4, 2, 3, 8
    x = torch.ones((C,), device=dev)
    p, f = torch.rand((n, C), device=dev), torch.randn((n, Dm), device=dev)
    cf = torch.randn((C, M, Dm), device=dev)
    small = ops.center_loss_workspace(1, 1, 1, dev)         # 24 words; (4, 2, 3) needs 44
    for kw in (dict(workspace=small),
               dict(counts=torch.zeros((C, M + 1), device=dev, dtype=torch.int32)),
               dict(counts=torch.zeros((C - 1, M), device=dev, dtype=torch.int32))):
        with pytest.raises(ops.L.NawsError) as e:
            ops.center_loss(x, p, f, cf, top_k, **kw)
        assert e.value.code == ops.L.ERR_SHAPE
    L, D, S, ws = ops.center_loss(x, p, f, cf, top_k)
    dl = torch.ones((1,), device=dev)
    dcf, ndcf = torch.zeros_like(cf), torch.zeros((C, M), device=dev)
    for args, kw in (((n, small), {}),
                     ((n, ws), dict(out=torch.empty((n - 1, Dm), device=dev))),
                     ((n, ws), dict(out=torch.empty((n, Dm + 1), device=dev)))):
        with pytest.raises(ops.L.NawsError) as e:
            ops.center_loss_grad(D, S, dl, args[0], args[1], dcf, ndcf, **kw)
        assert e.value.code == ops.L.ERR_SHAPE
    out = torch.empty((n, Dm), device=dev)
    assert ops.center_loss_grad(D, S, dl, n, ws, dcf, ndcf, out=out) is out


def test_center_loss_forward_unaligned_pointers(dev):
    """Dm % 4 == 0 with F and CF that are NOT 16-byte aligned (views one float into a flat
    buffer): the distance kernel must leave its float4 form.  Same selection, centres and D bits as
    the aligned call; L within 1e-5 of float64 (the two forms sum in different fixed orders)."""
    case = make_case(70, 3, 2, 4, 96, seed=11)
    R, C, M, top_k, Dm = case['dims']
    from naws_hip import ops
    _, want = reference_forward(case)

    def shifted(a):
        flat = torch.empty((a.size + 1,), device=dev, dtype=torch.float32)
        v = flat[1:].view(*a.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
        assert v.data_ptr() % 16 == 4
        return v

    x = _t(case['X'], dev).reshape(-1)
    L, D, S, ws = ops.center_loss(x, _t(case['P'], dev), shifted(case['F']), shifted(case['CF']),
                                  top_k, case['ignore'])
    assert np.array_equal(ops.center_loss_picks(ws, C, top_k).cpu().numpy(), want[3])
    assert np.array_equal(S.cpu().numpy(), want[2])
    assert np.array_equal(_bits(D.cpu().numpy()), _bits(want[1]))
    assert abs(float(L[0]) - want[0]) <= 1e-5 * abs(want[0])


def test_center_loss_sequence_is_capturable(dev):
    """One forward + update + backward of the ops-level functions captured in a graph and replayed
    once: a captured sequence cannot contain a host synchronisation, an allocation by the library
    or a copy to the host.  The replay writes the same bits as the eager calls."""
    from naws_hip import ops
    case = make_case(120, 6, 3, 5, 64, seed=3)
    R, C, M, top_k, Dm = case['dims']
    x, p, f = _t(case['X'], dev).reshape(-1), _t(case['P'], dev), _t(case['F'], dev)
    dl = torch.full((1,), 0.4096, device=dev)
    rng = np.random.default_rng(5)
    state0 = [_t(case['CF'], dev), _t(rng.standard_normal((C, M, Dm)), dev),
              _t(rng.integers(0, 3, (C, M)), dev), _t(rng.standard_normal((C, M, Dm)), dev),
              _t(rng.integers(0, 3, (C, M)), dev)]

    def sequence(state, ws, counts):
        cf, dcf, ndcf, acc_d, acc_n = state
        L, D, S, _ = ops.center_loss(x, p, f, cf, top_k, workspace=ws, counts=counts)
        ops.center_loss_update(cf, dcf, ndcf, acc_d, acc_n, top_k, 0.5, first=False, apply=True)
        df = ops.center_loss_grad(D, S, dl, R, ws, dcf, ndcf)
        return L, D, S, df

    eager = [t.clone() for t in state0]
    ws_e = ops.center_loss_workspace(C, M, top_k, dev)
    cnt_e = torch.zeros((C, M), device=dev, dtype=torch.int32)
    out_e = sequence(eager, ws_e, cnt_e)
    torch.cuda.synchronize()
    assert not torch.equal(eager[0], state0[0])             # the centres moved
    static = [t.clone() for t in state0]
    ws_g = ops.center_loss_workspace(C, M, top_k, dev)
    cnt_g = torch.zeros((C, M), device=dev, dtype=torch.int32)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = sequence(static, ws_g, cnt_g)
    for dst, src in zip(static, state0):                    # (capture runs nothing)
        dst.copy_(src)
    cnt_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(list(out_e) + eager + [cnt_e], list(out_g) + static + [cnt_g]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------ in the graph
def _blobs(nfg, m, seed=3):
    from detectron.datasets import synthetic
    blobs = synthetic.init_blobs(nfg, seed=seed)
    g = torch.Generator().manual_seed(17)
    blobs['center_feature'] = torch.randn((nfg, m, 4096), generator=g)
    blobs['center_feature_g'] = torch.zeros((nfg, m, 4096))
    blobs['center_feature_n_u'] = torch.zeros((nfg, m))
    return blobs


def _minibatch(nfg, seed=5):
    from detectron.datasets import synthetic
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, 48, nfg, 64, 96, seed=seed), nfg)
    second = (int(mb['labels_int32'][0]) + 7) % nfg
    mb['labels_oh'][0, second] = 1.0                       # two labelled classes
    return mb


def _cfg_list(webly, on):
    base = ['NUM_GPUS', 1, 'WSL.CENTER_LOSS', on, 'NAWS.CENTER_LOSS_TOP_K', 4]
    if not webly:
        base += ['WEBLY.WEBLY_ON', False, 'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head']
    return base


def _executor(c, dev, webly, on, blobs):
    from detectron.core.executor import NetExecutor
    import detectron.modeling.model_builder_wsl as mbld
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(_cfg_list(webly, on))
    c.assert_and_infer_cfg(make_immutable=False)
    model = mbld.create('generalized_wsl', train=True)
    ex = NetExecutor(model, dev, disable_dropout=True, force_interpreted=not on)
    ex.load_blobs(blobs)
    return model, ex


_GRAPH_RUNS = {}


def _graph_run(dev, webly):
    """One lr-0 iteration of the graph with the switch on and of the same graph with it off (same
    blobs, same minibatch), and the restatement on the fetched rois_pred / drop7; run once per
    model and shared by the tests below."""
    if webly in _GRAPH_RUNS:
        return _GRAPH_RUNS[webly]
    from detectron.core import config as c
    nfg, m = 20, 5
    try:
        blobs = _blobs(nfg, m)
        mb = _minibatch(nfg)
        t = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
        r = dict(blobs=blobs, mb=mb, t=t)
        for on in (True, False):
            model, ex = _executor(c, dev, webly, on, blobs)
            assert ex.plan == 'interpreted'        # never the fused engine: it has no such loss
            model.UpdateWorkspaceLr(0, 0.0)
            ex.feed(t)
            ex.run()
            r['on' if on else 'off'] = (model, ex)
            r['grad_on' if on else 'grad_off'] = ex.ws['drop7_grad'].cpu().numpy().copy()
        ws = r['on'][1].ws
        ref = clr.CenterLossRef(top_k=4, update=128, max_iter=35000)
        cf = blobs['center_feature'].numpy()
        r['fwd'] = ref.forward(mb['labels_oh'], ws['rois_pred'].cpu().numpy(),
                               ws['drop7'].cpu().numpy(), cf)
        L, D, S, picks = r['fwd']
        r['dCF'], r['ndCF'] = np.zeros((nfg, m, 4096)), np.zeros((nfg, m))
        r['dF'] = ref.gradient(D, S, picks, float(np.float32(0.4096)), 48, cf.astype(np.float64),
                               r['dCF'], r['ndCF'])
        r['got'] = {k: ws[k].cpu().numpy().copy() for k in ('loss_center', '_center_picks', 'S', 'D',
                                                            'center_feature_n_u', 'center_feature_g',
                                                            'loss_center_grad')}
    finally:
        c.reset_cfg()
    _GRAPH_RUNS[webly] = r
    return r


@pytest.mark.parametrize('webly', [False, True], ids=['wsddn', 'na_wsddn'])
def test_center_loss_graph_feature_gradient(dev, webly):
    """drop7_grad(switch on) - drop7_grad(switch off) equals the restatement's dF within
    (labelled classes + 1) * 2^-23 * max|dF|, the bound of the ops-level test.  The figures are
    printed before the assertion."""
    r = _graph_run(dev, webly)
    L, D, S, picks = r['fwd']
    want, on_grad, off_grad = r['dF'], r['grad_on'], r['grad_off']
    assert int((picks[:, 0] >= 0).sum()) == 2
    selected = np.unique(picks[picks >= 0])
    bound = (2 + 1) * EPS * np.abs(want).max()
    err = np.abs((on_grad - off_grad) - want).max()
    print('drop7_grad on - off: max|dF| %.4g  max err %.3g  bound %.3g  (max|drop7_grad off| on the '
          'selected rows %.4g)'
          % (np.abs(want).max(), err, bound, np.abs(off_grad[selected]).max()))
    assert err <= bound


@pytest.mark.parametrize('webly', [False, True], ids=['wsddn', 'na_wsddn'])
def test_center_loss_graph_gradient_rows(dev, webly):
    """Where the loss's gradient lands in the graph, which the difference of two blobs does not
    show on its own: (1) the gradient op's own output - recomputed from the graph's D, S,
    selection and seed into scratch blobs - equals the restatement's dF within (labelled classes
    + 1) * 2^-23 * max|dF| and is exactly zero on unselected rois; (2) those rows of drop7_grad
    are bit-identical with the switch on and off, so the fc8 gradients were accumulated into the
    blob, not overwritten; (3) the selected rows differ."""
    from naws_hip import ops
    r = _graph_run(dev, webly)
    L, D, S, picks = r['fwd']
    want, on_grad, off_grad = r['dF'], r['grad_on'], r['grad_off']
    model, ex = r['on']
    ws = ex.ws
    obj = [ex._state[i] for i, o in enumerate(model.net.ops) if o.type == 'CenterLoss'][0]
    own = ops.center_loss_grad(ws['D'], ws['S'], ws['loss_center_grad'].reshape(1).contiguous(), 48,
                               obj.workspace, torch.zeros_like(ws['center_feature_g']),
                               torch.zeros_like(ws['center_feature_n_u'])).cpu().numpy()
    bound = (2 + 1) * EPS * np.abs(want).max()
    print('own dF err %.3g (bound %.3g)' % (np.abs(own - want).max(), bound))
    assert np.abs(own - want).max() <= bound
    unselected = np.setdiff1d(np.arange(48), picks[picks >= 0])
    selected = np.unique(picks[picks >= 0])
    assert not own[unselected].any()
    assert np.array_equal(on_grad[unselected], off_grad[unselected])
    assert off_grad[unselected].any()
    assert not np.array_equal(on_grad[selected], off_grad[selected])


@pytest.mark.parametrize('webly', [False, True], ids=['wsddn', 'na_wsddn'])
def test_center_loss_in_the_graph(dev, tmp_path, webly):
    """The switch on top of the plain WSDDN model and of na_wsddn (op-by-op plan, 64 x 96 image,
    48 rois, dropout off, NAWS.CENTER_LOSS_TOP_K 4): loss_center, the selection, S and D against
    the restatement on the fetched rois_pred / drop7, one real step, the checkpoint."""
    from detectron.core import config as c
    import detectron.utils.net_wsl as nu
    r = _graph_run(dev, webly)
    blobs, t = r['blobs'], r['t']
    (model, ex), (model0, ex0) = r['on'], r['off']
    L, D, S, picks = r['fwd']
    got = r['got']
    try:
        assert [p for p in STATE if p in model.params] == list(STATE)
        assert 'center_feature' not in model0.params
        assert int((picks[:, 0] >= 0).sum()) == 2
        print('loss_center %.9g (float64 %.9g)' % (float(got['loss_center']), L))
        assert abs(float(got['loss_center']) - L) <= 1e-5 * abs(L)
        assert np.array_equal(got['_center_picks'], picks)
        assert np.array_equal(got['S'], S)
        assert np.array_equal(_bits(got['D']), _bits(D))
        assert np.array_equal(got['center_feature_n_u'], r['ndCF'].astype(np.float32))
        tol = 4 * 2.0 ** -24 * np.abs(D.astype(np.float64)).sum(1).max()
        assert np.abs(got['center_feature_g'] - r['dCF']).max() <= tol
        assert float(got['loss_center_grad'].reshape(-1)[0]) == np.float32(0.4096)
        # ---- one real step: the loss reaches fc7 through drop7; the centres wait for `update`
        c.merge_cfg_from_file(YAML)
        c.merge_cfg_from_list(_cfg_list(webly, True))
        for mdl, e in ((model, ex), (model0, ex0)):
            mdl.UpdateWorkspaceLr(1, 1e-2)
            e.feed(t)
            e.run()
        a, a0 = ex.blobs(with_momentum=False), ex0.blobs(with_momentum=False)
        assert not torch.equal(a['fc7_w'], a0['fc7_w'])
        assert not torch.equal(a['fc7_w'].cpu(), blobs['fc7_w'])
        assert torch.equal(a['center_feature'].cpu(), blobs['center_feature'])
        assert bool(a['center_feature_g'].any()) and float(a['center_feature_n_u'].sum()) == 2.0
        # ---- checkpoint round trip
        f = str(tmp_path / 'model_iter1.pkl')
        nu.save_model_to_weights_file(f, model, ex)
        saved = nu.load_object(f)['blobs']
        for p in STATE:
            assert p in saved and p + '_momentum' not in saved
        assert 'fc7_w_momentum' in saved
        model2, ex2 = _executor(c, dev, webly, True, blobs)
        ex2.init_params(seed=11)
        nu.initialize_from_weights_file(model2, f, ex2, broadcast=False)
        b1, b2 = ex.blobs(with_momentum=False), ex2.blobs(with_momentum=False)
        assert sorted(b1) == sorted(b2) == sorted(model.params)
        for n in model.params:
            assert torch.equal(b1[n], b2[n]), n
            assert np.array_equal(saved[n], b1[n].cpu().numpy()), n
    finally:
        c.reset_cfg()
        _GRAPH_RUNS.pop(webly, None)       # (the executors hold a few GB)


def test_center_loss_train_cli(dev, cfgmod, tmp_path, capsys):
    """The training tool on na_wsddn with the switch on: two iterations on the op-by-op plan, the
    json_stats lines carry loss_center, the final checkpoint the three state blobs."""
    import importlib.util
    import detectron.utils.net_wsl as nu
    cfgmod.reset_cfg()
    spec = importlib.util.spec_from_file_location(
        'train_net_wsl', os.path.join(ROOT, 'na-fwebsod_amd', 'tools', 'train_net_wsl.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(['--cfg', YAML, '--skip-test', '--max-iter', '2', 'OUTPUT_DIR', str(tmp_path),
               'TRAIN.SCALES', '(64,)', 'TRAIN.MAX_SIZE', '96', 'TRAIN.BATCH_SIZE_PER_IM', '32',
               'WSL.USE_DISTORTION', 'False', 'DATA_LOADER.NUM_THREADS', '1',
               'SOLVER.BASE_LR', '1e-5', 'NUM_GPUS', '1', 'WSL.CENTER_LOSS', 'True'])
    out = capsys.readouterr().out
    assert 'json_stats: {' in out and '"loss_center"' in out and '"loss_cls_noise"' in out
    assert 'CenterLoss #iter_: 1 #loss_: ' in out
    final = os.path.join(str(tmp_path), 'train', 'flickr_voc', 'generalized_wsl', 'model_final.pkl')
    saved = nu.load_object(final)['blobs']
    assert saved['center_feature'].shape == (20, 5, 4096) and np.isfinite(saved['center_feature']).all()
    assert saved['center_feature_n_u'].shape == (20, 5)


# ------------------------------------------------------------------------------ two ranks
STEPS, UPDATE = 3, 2


def _rank(rank, world, port, outdir):
    sys.path.insert(0, os.path.join(ROOT, 'na-fwebsod_amd'))
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import faulthandler
    faulthandler.dump_traceback_later(float(os.environ.get('NAWS_RANK_LIMIT', '150')), exit=True)
    import torch.distributed as dist
    from detectron.core import config as c
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from detectron.core.executor import NetExecutor
    import detectron.modeling.model_builder_wsl as mbld
    nfg, m = 20, 5
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(_cfg_list(False, True) + ['NUM_GPUS', world])
    c.assert_and_infer_cfg(make_immutable=False)
    model = mbld.create('generalized_wsl', train=True)
    for op in model.net.ops:
        if op.type == 'CenterLoss':
            op.args['update'] = UPDATE
    ex = NetExecutor(model, dev, process_group=dist.group.WORLD, world_size=world, rank=rank,
                     disable_dropout=True)
    assert ex.plan == 'interpreted'
    blobs = _blobs(nfg, m)
    if rank != 0:       # only rank 0's centres may survive the broadcast
        blobs['center_feature'] = blobs['center_feature'] + 1.0
    ex.load_blobs(blobs)
    ex.broadcast_parameters()
    model.UpdateWorkspaceLr(0, 1e-3)
    rec = {}
    for it in range(STEPS):
        mb = _minibatch(nfg, seed=5 + 10 * rank + it)        # different minibatches
        ex.feed({k: torch.from_numpy(v).to(dev) for k, v in mb.items()})
        ex.run()
        rec['labels%d' % it] = mb['labels_oh']
        rec['pred%d' % it] = ex.ws['rois_pred'].cpu().numpy()
        rec['feat%d' % it] = ex.ws['drop7'].cpu().numpy()
        rec['g%d' % it] = ex.ws['center_feature_g'].cpu().numpy()
        rec['n%d' % it] = ex.ws['center_feature_n_u'].cpu().numpy()
    rec['cf'] = ex.ws['center_feature'].cpu().numpy()
    np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **rec)
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(procs, limit=200.0):
    import time
    for p in procs:
        p.start()
    t0 = time.time()
    for p in procs:
        p.join(timeout=max(1.0, limit - (time.time() - t0)))
    stuck = [p for p in procs if p.is_alive()]
    for p in stuck:
        p.kill()
        p.join(timeout=30)
    assert not stuck, 'ranks did not finish within %.0f s' % limit
    for p in procs:
        assert p.exitcode == 0


def test_center_loss_two_ranks(dev, tmp_path):
    """Two processes share the GPU and exchange over gloo, different minibatches, update = 2, three
    iterations: the contribution blobs are summed over the ranks after backward, so both ranks
    move their centres by the same sum - bit-identical centres - and those equal the restatement
    fed both ranks' contributions."""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_rank, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    _run_ranks(procs)
    r0, r1 = (np.load(str(tmp_path / ('rank%d.npz' % r))) for r in range(2))
    assert np.array_equal(_bits(r0['cf']), _bits(r1['cf']))
    nfg, m = 20, 5
    cf0 = _blobs(nfg, m)['center_feature'].numpy()
    assert not np.array_equal(r0['cf'], cf0)                 # the update at iteration 2 happened
    refs = [clr.CenterLossRef(top_k=4, update=UPDATE, max_iter=35000) for _ in range(2)]
    CF = [cf0.astype(np.float64), cf0.astype(np.float64)]
    dCF = [np.zeros((nfg, m, 4096)) for _ in range(2)]
    ndCF = [np.zeros((nfg, m)) for _ in range(2)]
    for it in range(STEPS):
        for r, rec in enumerate((r0, r1)):
            L, D, S, picks = refs[r].forward(rec['labels%d' % it], rec['pred%d' % it],
                                             rec['feat%d' % it], CF[r])
            refs[r].gradient(D, S, picks, 0.4096, 48, CF[r], dCF[r], ndCF[r])
        total_d, total_n = dCF[0] + dCF[1], ndCF[0] + ndCF[1]      # the all-reduce
        for r, rec in enumerate((r0, r1)):
            dCF[r][...], ndCF[r][...] = total_d, total_n
            assert np.array_equal(rec['n%d' % it], total_n.astype(np.float32))
            assert np.abs(rec['g%d' % it] - total_d).max() <= 1e-5 * max(np.abs(total_d).max(), 1e-30)
    assert np.array_equal(CF[0], CF[1])
    err = np.abs(r0['cf'] - CF[0]).max()
    print('max |center_feature - restatement| %.3g (bound %.3g)' % (err, 1e-6 * np.abs(CF[0]).max()))
    assert err <= 1e-6 * np.abs(CF[0]).max()
