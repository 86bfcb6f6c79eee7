"""The trainable conv body's backward (csrc/body_bwd.hip) at the shapes where its kernels take
another path than at the tiny shapes of tests/test_gpu_body_backward.py: more than one K slice in
the weight gradient (2, 4, 6 and the cap of 32; tests/test_body_backward_plan.py holds the case
table to those counts), several 64-wide tiles with a 64 + 32 residue in M and N, two images, K of
1 and K that is no multiple of 32, the 64 x 128 x 16 conv form of the data gradient, and every
elementwise kernel past its grid cap, where it loops.

Two kinds of check.  On integer operands every float32 sum is exact in any order, so the result
must be THE float32 of the float64 reference, bit for bit: one dropped or doubled term shows.  On
Gaussian operands the project's bound (5e-4 of max|ref| per tensor) holds and two calls agree to
the bit.  Zeros that the staging promises (across images, across the padded row seam) are checked
as exact zeros, and the workspace is neither read where unwritten nor written past its size."""
import numpy as np
import pytest
import torch

import body_grad_ref as bgr
from test_gpu_body_backward import BOUND, _bits, _conv_case, _ratio, _t

pytestmark = pytest.mark.gpu

CASES = list(bgr.WGRAD_CASES)
_id = lambda c: 'x'.join(str(v) for v in c) if isinstance(c, tuple) else str(c)


def _nhwc(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))


def _nchw(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 3, 1, 2))


def _same_bits(got, ref64):
    """got (float32 from the GPU) is the float32 of the exact value, bit for bit.  An exact zero is
    +0 on both sides: a float32 sum that starts at +0 cannot end at -0 (round to nearest), and the
    + 0.0 takes the sign off a zero the float64 library may have left."""
    want = np.asarray(ref64, np.float64).astype(np.float32) + np.float32(0.0)
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _diff(got, ref64):
    d = np.abs(np.asarray(got, np.float64) - ref64)
    return '%d of %d differ, max |diff| %.3g' % (np.count_nonzero(d), d.size, d.max())


def _grads(dev, x, wt, dy, d):
    """The two C-ABI routes (NHWC) -> numpy dw [Cout,Cin,3,3], db [Cout], dx [N,Cin,H,W] and the
    device tensors."""
    from naws_hip import ops
    xh, dyh = _t(_nhwc(x), dev), _t(_nhwc(dy), dev)
    gw, gb = ops.conv3x3_nhwc_wgrad(xh, dyh, d)
    gx = ops.conv3x3_nhwc(dyh, ops.conv3x3_dgrad_pack_weight(_t(wt, dev)), None, d, relu=False)
    return dict(dw=gw.cpu().numpy(), db=gb.cpu().numpy(), dx=_nchw(gx.cpu().numpy())), (gw, gb, gx)


def _op_grads(dev, x, wt, dy, d):
    """detectron.ops.ConvGradient (NCHW) -> the same dict."""
    import detectron.ops as O
    gw, gb, gx = O.ConvGradient(_t(x, dev), _t(wt, dev), _t(dy, dev), pad=d, dilation=d)
    return dict(dw=gw.cpu().numpy(), db=gb.cpu().numpy(), dx=gx.cpu().numpy())


# ------------------------------------------------------- 1. conv gradients across the plan ----
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_conv_gradients_exact_on_integer_operands(dev, case):
    """X, W, dY integers in -2..2: dW, db and dX bit-equal to the float64 reference cast to
    float32, whatever the slice, tile and tap order (bgr.conv_case_int states the bound)."""
    n, h, w, cin, cout, d = case
    x, wt, dy = bgr.conv_case_int(case, 1000 + CASES.index(case))
    dx, dw, db = bgr.conv_grads(x, wt, np.zeros(cout), dy, d)
    ref = dict(dx=dx, dw=dw, db=db)
    got, _ = _grads(dev, x, wt, dy, d)
    routes = [('C ABI', got)]
    if bgr.WGRAD_CASES[case] == 4:
        routes.append(('ConvGradient', _op_grads(dev, x, wt, dy, d)))
    for name, g in routes:
        for k in ('dw', 'db', 'dx'):
            print('%s %s %s: %s' % (_id(case), name, k, _diff(g[k], ref[k])))
    for name, g in routes:
        for k in ('dw', 'db', 'dx'):
            assert _same_bits(g[k], ref[k]), (name, k)
    if h == 1 and w == 1:        # K = 1: every tap but the centre reads only staged zeros
        off = np.ones((3, 3), bool)
        off[1, 1] = False
        assert not _bits(got['dw'])[:, :, off].any() and got['dw'][:, :, 1, 1].any()


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_conv_gradients_gaussian_within_the_bound(dev, case):
    """The Gaussian operands of the tiny-shape tests at the plan's other branches: each tensor
    within 5e-4 of max|ref| of float64 autograd; a second call is bit-identical (the slices are
    summed in a fixed order)."""
    n, h, w, cin, cout, d = case
    x, wt, b, dy = _conv_case(cin, cout, n, h, w, 2000 + CASES.index(case))
    dx, dw, db = bgr.conv_grads(x, wt, b, dy, d)
    ref = dict(dx=dx, dw=dw, db=db)
    got, first = _grads(dev, x, wt, dy, d)
    _, second = _grads(dev, x, wt, dy, d)
    routes = [('C ABI', got)]
    if bgr.WGRAD_CASES[case] == 4:
        routes.append(('ConvGradient', _op_grads(dev, x, wt, dy, d)))
    for name, g in routes:
        for k in ('dw', 'db', 'dx'):
            print('%s ks %d %s %s: max err / max|ref| = %.3g'
                  % (_id(case), bgr.WGRAD_CASES[case], name, k, _ratio(g[k], ref[k])))
    for name, g in routes:
        for k in ('dw', 'db', 'dx'):
            assert g[k].shape == ref[k].shape and _ratio(g[k], ref[k]) <= BOUND, (name, k)
    for a, b2 in zip(first, second):
        assert torch.equal(a, b2)


# ------------------------------------------------------------- 2. exact zeros of the staging ----
@pytest.mark.parametrize('dilation', [1, 2])
@pytest.mark.parametrize('shape', [(2, 9, 13, 32, 64), (2, 20, 24, 96, 160)], ids=_id)
def test_wgrad_nothing_leaks_across_images_or_rows(dev, shape, dilation):
    """X and dY non-zero on pixel sets that no tap connects - different images; the last column
    against the first (neighbours across the padded row seam) and the mirror; the last row against
    the first and the mirror: every product that reaches dW has a staged zero as a factor, so dW
    is all +0 bits, and db is the (exact, integer) column sum of dY.  One connected pair as the
    control: X on column d and dY on column 0 meet in the taps kx = 2 and nowhere else."""
    from naws_hip import ops
    n, h, w, cin, cout = shape
    d = dilation
    assert w - 1 not in (0, d) and h - 1 not in (0, d)
    rng = np.random.default_rng(40 + d)
    vals = np.array([-2, -1, 1, 2], np.float32)
    x = vals[rng.integers(0, 4, (n, h, w, cin))]
    dy = vals[rng.integers(0, 4, (n, h, w, cout))]
    img = np.arange(n).reshape(n, 1, 1, 1)
    row = np.arange(h).reshape(1, h, 1, 1)
    col = np.arange(w).reshape(1, 1, w, 1)
    pairs = [('image 0 | image 1', img == 0, img == 1), ('image 1 | image 0', img == 1, img == 0),
             ('last column | first', col == w - 1, col == 0),
             ('first column | last', col == 0, col == w - 1),
             ('last row | first', row == h - 1, row == 0),
             ('first row | last', row == 0, row == h - 1)]
    results = []
    for name, mx, my in pairs:
        xs, dys = np.where(mx, x, np.float32(0)), np.where(my, dy, np.float32(0))
        assert xs.any() and dys.any()
        gw, gb = ops.conv3x3_nhwc_wgrad(_t(xs, dev), _t(dys, dev), d)
        results.append((name, gw.cpu().numpy(), gb.cpu().numpy(), dys.astype(np.float64)))
    for name, gw, gb, dys in results:
        print('%s d %d %s: %d non-zero words in dW' % (_id(shape), d, name,
                                                      np.count_nonzero(_bits(gw))))
    for name, gw, gb, dys in results:
        assert not _bits(gw).any(), name
        assert _same_bits(gb, dys.sum((0, 1, 2))), name
    xs, dys = np.where(col == d, x, np.float32(0)), np.where(col == 0, dy, np.float32(0))
    gw, _ = ops.conv3x3_nhwc_wgrad(_t(xs, dev), _t(dys, dev), d)
    gw = gw.cpu().numpy()
    _, dw, _ = bgr.conv_grads(_nchw(xs), np.zeros((cout, cin, 3, 3)), np.zeros(cout), _nchw(dys), d)
    assert _same_bits(gw, dw) and not _bits(gw)[:, :, :, :2].any() and gw[:, :, :, 2].any()


# ------------------------------------------------------------------ 3. workspace discipline ----
@pytest.mark.parametrize('case', [(2, 9, 13, 32, 64, 2), (2, 20, 24, 96, 160, 1)], ids=_id)
def test_wgrad_workspace_is_written_before_read_and_not_overrun(dev, case):
    """One slice and four: on a workspace of `need` NaNs the result is bit-equal to the call with a
    fresh one (nothing unwritten is read), and the 4096 floats behind `need` keep their pattern."""
    from naws_hip import lib, ops
    n, h, w, cin, cout, d = case
    need = lib.load().naws_conv3x3_nhwc_wgrad_workspace_floats(*case)
    ks = bgr.wgrad_slices(need, case)
    assert ks == 1 or ks >= 4
    x, _, _, dy = _conv_case(cin, cout, n, h, w, 77 + ks)
    xh, dyh = _t(_nhwc(x), dev), _t(_nhwc(dy), dev)
    pattern = 0x5A5AA5A5
    ws = torch.empty((need + 4096,), device=dev, dtype=torch.float32)
    ws[:need] = float('nan')
    ws[need:].view(torch.int32).fill_(pattern)
    gw, gb = ops.conv3x3_nhwc_wgrad(xh, dyh, d, workspace=ws)
    fw, fb = ops.conv3x3_nhwc_wgrad(xh, dyh, d)
    torch.cuda.synchronize()
    print('%s ks %d need %d: NaNs in dW %d, in db %d' % (_id(case), ks, need, int(gw.isnan().sum()),
                                                        int(gb.isnan().sum())))
    assert torch.isfinite(fw).all() and torch.isfinite(fb).all()
    assert torch.equal(gw.view(torch.int32), fw.view(torch.int32))
    assert torch.equal(gb.view(torch.int32), fb.view(torch.int32))
    assert bool((ws[need:].view(torch.int32) == pattern).all())


# ----------------------------------------------------------------------- 4. dgrad weight pack ----
@pytest.mark.parametrize('cout,cin', [(512, 512), (32, 96)])
def test_dgrad_pack_weight_is_the_permutation(dev, cout, cin):
    """[Cin,3,3,Cout] = W flipped in both taps, (ci, ky, kx, co): a pure permutation, bit-equal to
    numpy's; 512 x 512 x 9 elements are more than the grid holds, so the kernel loops."""
    from naws_hip import ops
    if cout == 512:
        assert cout * cin * 9 > 256 * 8 * 256
    wt = np.random.default_rng(cout + cin).standard_normal((cout, cin, 3, 3)).astype(np.float32)
    got = ops.conv3x3_dgrad_pack_weight(_t(wt, dev)).cpu().numpy()
    want = np.ascontiguousarray(wt[:, :, ::-1, ::-1].transpose(1, 2, 3, 0))
    assert got.shape == want.shape == (cin, 3, 3, cout)
    assert np.array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------------- 5. max-pool gradient ----
def _pool_pair(dev, x, dy, stride):
    from naws_hip import ops
    xd = _t(x, dev)
    gy = ops.maxpool2x2_nhwc(xd, stride)
    return gy.cpu().numpy(), ops.maxpool2x2_nhwc_grad(xd, gy, _t(dy, dev), stride).cpu().numpy()


@pytest.mark.parametrize('stride', [2, 1])
def test_maxpool_gradient_loops_and_breaks_ties(dev, stride):
    """1 x 67 x 127 x 512 is 1,089,152 float4 lanes, more than the grid holds: the kernel loops.
    Integers 0..3, so most windows tie (on each of a, b, d, e at least once); forward and gradient
    bit-equal to the first-of-a,b,d,e restatement, and with an integer dY every window's gradient
    lands exactly once: the two sums are the same number."""
    shape = (1, 67, 127, 512)
    assert shape[1] * shape[2] * shape[3] // 4 > 256 * 16 * 256
    x = bgr.pool_tie_input(shape, stride)
    tied, selected = bgr.tie_census(x, stride)
    assert (tied > 0).all() and (selected > 0).all()
    y, _ = bgr.maxpool_select(x, stride)
    dy = np.random.default_rng(50 + stride).integers(-3, 4, y.shape).astype(np.float32)
    want = bgr.maxpool_grad32(x, dy, stride)
    gy, got = _pool_pair(dev, x, dy, stride)
    assert np.array_equal(_bits(gy), _bits(y))
    print('stride %d: %d of %d gradient words differ; tied windows per position %s'
          % (stride, np.count_nonzero(_bits(got) != _bits(want)), got.size, tied.tolist()))
    assert np.array_equal(_bits(got), _bits(want))
    assert got.astype(np.float64).sum() == dy.astype(np.float64).sum()
    if stride == 2:
        assert not got[:, 66].any() and not got[:, :, 126].any() and got[:, :66, :126].any()


@pytest.mark.parametrize('shape,stride', [((1, 2, 2, 4), 2), ((1, 2, 2, 4), 1), ((1, 2, 3, 4), 2),
                                          ((1, 2, 3, 4), 1), ((1, 3, 3, 8), 1)], ids=_id)
def test_maxpool_gradient_minimum_shapes(dev, shape, stride):
    """One window of one float4; a dropped last column; two windows that share the middle column;
    four windows around one pixel.  Integer input (ties), Gaussian dY (the order of the adds)."""
    rng = np.random.default_rng(60 + 10 * shape[2] + stride)
    x = rng.integers(0, 4, shape).astype(np.float32)
    y, _ = bgr.maxpool_select(x, stride)
    dy = rng.standard_normal(y.shape).astype(np.float32)
    want = bgr.maxpool_grad32(x, dy, stride)
    gy, got = _pool_pair(dev, x, dy, stride)
    assert np.array_equal(_bits(gy), _bits(y)) and np.array_equal(_bits(got), _bits(want))
    assert np.count_nonzero(got) <= dy.size and got.any()
    if shape[2] == 3 and stride == 2:
        assert y.shape == (1, 1, 1, 4) and not got[:, :, 2].any()


# ---------------------------------------------------------------------- 6. RoIPoolF gradient ----
def test_roi_pool_f_gradient_loops_under_contention(dev):
    """Feature 2 x 512 x 10 x 14, 176 rois: 176 * 512 * 49 elements of dY are more than the grid
    holds, so the kernel loops; 40 copies of one box pile 40 atomic adds on single addresses.
    Gaussian dY: per element within n_e 2^-24 sum|terms| of the float64 scatter through the
    forward's own argmax, untouched elements exactly 0.  Integer dY: the sum no longer depends on
    the order, so the result is the float32 of the float64 scatter, bit for bit.  Both layouts."""
    import detectron.ops as O
    from helpers import make_rois
    from naws_hip import ops
    rng = np.random.default_rng(23)
    n, c, h, w = 2, 512, 10, 14
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    rois = make_rois(rng, n, 88, h * 8, w * 8, degenerate=False)
    rois[1, 1:] = [40, 24, 40, 24]                                   # 1-pixel
    rois[2, 1:] = [w * 16, h * 16, w * 16 + 50, h * 16 + 50]         # outside: all bins empty
    rois[3:43, 1:] = [8, 8, 70, 60]                                  # 40 identical
    assert rois.shape == (176, 5) and set(rois[:, 0]) == {0.0, 1.0}
    assert 176 * c * 49 > 256 * 64 * 256
    xr, rr = _t(x, dev), _t(rois, dev)
    y, am = O.RoIPoolF(xr, rr, 7, 7, 0.125)
    amn = am.cpu().numpy()
    assert (amn[2] == -1).all() and (amn[1] >= 0).all() and (amn[3:43] == amn[3]).all()
    gauss = rng.standard_normal(y.shape).astype(np.float32)
    whole = rng.integers(-3, 4, y.shape).astype(np.float32)
    out = {}
    for name, dy in (('gauss', gauss), ('integer', whole)):
        dyd = _t(dy, dev)
        nchw = O.RoIPoolFGradient(xr, rr, am, dyd).cpu().numpy()
        nhwc = ops.roi_pool_f_grad(dyd, am, rr, (n, h, w, c), layout='NHWC').cpu().numpy()
        out[name] = (bgr.roi_pool_grad64(dy, amn, rois, (n, c, h, w)), nchw, _nchw(nhwc))
    (ref, cnt, asum), g1, g2 = out['gauss']
    assert cnt.max() >= 40 and (cnt == 0).any()
    bound = cnt * 2.0 ** -24 * asum
    for lay, g in (('NCHW', g1), ('NHWC', g2)):
        err = np.abs(g - ref)
        print('RoIPoolF grad %s: max err %.3g, max err / bound %.3g, up to %d terms per element'
              % (lay, err.max(), (err[cnt > 0] / np.maximum(bound[cnt > 0], 1e-300)).max(),
                 cnt.max()))
    for g in (g1, g2):
        assert g.shape == x.shape and (np.abs(g - ref) <= bound).all()
        assert not _bits(g)[cnt == 0].any()
    (ref, cnt, _), g1, g2 = out['integer']
    for lay, g in (('NCHW', g1), ('NHWC', g2)):
        print('RoIPoolF grad %s, integer dY: %s' % (lay, _diff(g, ref)))
    assert _same_bits(g1, ref) and _same_bits(g2, ref)
