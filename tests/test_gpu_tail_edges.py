"""GPU parity at the edge shapes of the loss tail (csrc/head_ops.hip) and of the op-by-op
executor's built-ins (csrc/misc_ops.hip): ragged and one-roi segments, class counts on both sides
of every template step, launches past the grid cap, strided and misaligned operands - each HIP
result against the float64 references of tests/tail_ref.py, with the comparisons that
tests/test_tail_ref_cpu.py holds the fp32 oracle to and shows to reject wrong references.

Bounds (tail_ref.check_*): bit-exact where the operation is one IEEE operation or a move (SCALE,
RELU up to the sign of zero, LEAKY_RELU, CLIP, REPLACE_NAN, ADD, SUB, MUL, DIV, GATE_POS,
transpose, Stat, the dropout prefix); LOG <= 2 ulp (the kernel takes the double-precision log and
rounds once).  DIV is asserted exact because the library is
built without fast-math flags: hipcc then emits the v_div_scale / v_div_fmas / v_div_fixup
sequence with fp32 denormals on (.amdhsa_float_denorm_mode_32 3), i.e. a correctly rounded
quotient.  Probabilities <= 1e-5 of the output's maximum and <= 1e-4 relative above 1e-30; gate
outputs <= 2e-5 of max per image, NaN exactly where the reference is; WSDDN gradients <= 2e-5 of
max |reference| per output (C = 1, where the exact gradient is zero: tail_ref.
wsddn_one_class_bound); GEMM-backed wrappers <= 5e-6 of max; column sums <= (L + 8) 2^-24
sum |x| per column; WCE rtol 1e-6 against the fp32 oracle and N C 2^-24 sum |terms| against
float64; the row-softmax gradient per entry (tail_ref.check_softmax_grad).

Largest errors observed on an MI355X (gfx950), all cases of a family together (`pytest -s` prints
one `tail-edge <family> <figure>` line per comparison; look here before tightening anything):

  family                                   observed       bound
  ---------------------------------------  -------------  ---------------------------------
  WSDDN probabilities, relative            4.03e-6        1e-4 (entries above 1e-30)
  WSDDN probabilities, of max              3.13e-7        1e-5
  WSDDN gradients, of max |reference|      8.34e-6        2e-5
  WSDDN gradients at C = 1                 0.25 of bound  wsddn_one_class_bound
  gate outputs, of max per image           2.93e-7        2e-5
  softmax_rows, relative / of max          3.98e-6 / 1.33e-7   1e-4 / 1e-5
  softmax_rows gradient, per entry         0.50 of bound  check_softmax_grad
  softmax_rows gradient, scale 1, of max   7.74e-8        2e-5
  unary LOG                                0.50 ulp       2 ulp
  other unary ops, binary ops, transpose,
    Stat, dropout mask                     bit-exact      bit-exact
  colsum float4 / scalar kernel            0.080 / 0.095 of bound   (L + 8) 2^-24 sum |x|
  reduce_sum_axis0                         0.095 of bound same
  WCE loss / gradient vs float64           0.044 / 0.23 of bound    N C 2^-24 sum |terms| / WCE_GRAD_EPS
  WCE shared labels loss / gradient        0.12 / 0.27 of bound     same
  FC / FCGradient dW / dX, of max          3.39e-7 / 2.33e-7 / 2.44e-7   5e-6
  FCGradient db                            0.062 of bound (L + 8) 2^-24 sum |x|
  MatMul, of max                           6.38e-7        5e-6

For orientation, the fp32 oracle on the same inputs (tests/test_tail_ref_cpu.py): probabilities
4.1e-6 relative and 9.5e-7 of max, WSDDN gradients 8.3e-6 of max, gate outputs 2.9e-6 of max,
row-softmax gradient 0.49 of its bound, WCE 0.023 and its gradient 0.23 of their bounds, column
sums 0.15 of theirs.
"""
import numpy as np
import pytest
import torch

import tail_ref as T

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.tensor(np.asarray(a), device=dev)      # (a copy: the shared inputs are read-only)


def _n(t):
    return t.detach().cpu().numpy()


def _iou(rois):
    from oracle import oracle
    return oracle.roi_iou(rois)


# ------------------------------------------------------------------------ WSDDN outputs ----
def _wsddn_run(dev, lens, c, scale, nb, rows=None):
    """Forward and backward of the batch (or of rows [lo, hi) as a batch of one image) with the
    four logit matrices as column slices of one [Rt, 4C + 3] buffer and the four gradients as
    slices of a wider `out`.  -> (ac, ad, rp, cp, out, col_offsets) as numpy."""
    from naws_hip import ops
    z = T.wsddn_inputs(lens, c, scale)
    g = z[4]
    seg = T.seg_of(lens)
    if rows is not None:
        s = rows
        z = [a[seg[s]:seg[s + 1]] for a in z[:4]]
        g = g[:, s:s + 1]
        seg = np.array([0, lens[s]], np.int32)
    rt = int(seg[-1])
    buf = np.full((rt, 4 * c + 3), np.nan, np.float32)       # one NaN column between the slices
    offs = [i * (c + 1) for i in range(4)]
    for o, a in zip(offs, z[:4]):
        buf[:, o:o + c] = a
    bufd = _t(buf, dev)
    v = [bufd[:, o:o + c] for o in offs]
    segd = _t(seg, dev)
    ac, ad, rp, cp = ops.wsddn_outputs(v[0], v[1], v[2] if nb == 2 else None,
                                       v[3] if nb == 2 else None, segd)
    out = torch.full((rt, 4 * c + 5), -7.0, device=dev)
    goffs = [1 + i * (c + 1) for i in range(4)]
    ops.wsddn_outputs_grad(ac, ad, rp, cp, _t(g[:nb], dev), segd, out=out, col_offsets=goffs)
    return _n(ac), _n(ad), _n(rp), _n(cp), _n(out), goffs


def _wsddn_case(dev, lens, c, scale, nb):
    ac, ad, rp, cp, out, goffs = _wsddn_run(dev, lens, c, scale, nb)
    ref = T.wsddn_forward_ref(lens, c, scale, nb)
    for got, want, name in zip((ac, ad, rp, cp), ref, ('alpha_cls', 'alpha_det', 'rois_pred',
                                                      'cls_prob')):
        T.check_prob(got, want, 'wsddn ' + name)
    g = T.wsddn_inputs(lens, c, scale)[4][:nb]
    grads = [out[:, o:o + c] for o in goffs]
    written = np.zeros(out.shape[1], bool)
    for o in goffs[:2 * nb]:
        written[o:o + c] = True
    assert (out[:, ~written] == -7.0).all()                  # gaps, and the noisy slices at nb = 1
    got4 = grads if nb == 2 else grads[:2] + [None, None]
    T.check_wsddn_grads(got4, T.wsddn_backward_ref(lens, ac, ad, g), lens, ad, g)
    # every image bit-identical to the same operators run on that image alone
    seg = T.seg_of(lens)
    for s in range(len(lens)):
        lo, hi = seg[s], seg[s + 1]
        a1, d1, p1, c1, o1, _ = _wsddn_run(dev, lens, c, scale, nb, rows=s)
        for whole, alone in ((ac[:, lo:hi], a1), (ad[:, lo:hi], d1), (rp[:, lo:hi], p1),
                             (cp[:, s:s + 1], c1), (out[lo:hi], o1)):
            assert np.array_equal(whole.view(np.int32), alone.view(np.int32)), (s, lens[s])


@pytest.mark.parametrize('nb', [1, 2])
@pytest.mark.parametrize('scale', T.SCALES)
@pytest.mark.parametrize('c', T.WSDDN_CLASSES)
def test_wsddn_outputs_ragged_segments(dev, c, scale, nb):
    _wsddn_case(dev, T.WSDDN_LENS, c, scale, nb)


def test_wsddn_outputs_forty_segments(dev):
    _wsddn_case(dev, T.WSDDN_MANY, 21, 1.0, 2)


# ------------------------------------------------------------------------- entropy gate ----
@pytest.mark.parametrize('lens,c,max_is_rt', T.GATE_CASES,
                         ids=['%s-C%d%s' % ('_'.join(map(str, l)), c, '-maxRt' if m else '')
                              for l, c, m in T.GATE_CASES])
def test_entropy_gate_ragged_segments(dev, lens, c, max_is_rt):
    from naws_hip import ops
    rois, rp, cp, labels = T.gate_inputs(lens, c)
    assert (rp == 0).any() and (labels == np.float32(0.4)).any()
    outs = ops.entropy_gate(_t(rois, dev), _t(rp, dev), _t(cp, dev), _t(labels, dev),
                            _t(T.seg_of(lens), dev), sum(lens) if max_is_rt else max(lens))
    T.check_gate4([_n(o) for o in outs], T.gate_ref(lens, c, _iou))


# ------------------------------------------------------------------------------ built-ins ----
@pytest.mark.parametrize('name', T.UNARY_OPS)
def test_unary_past_the_launch_cap(dev, name):
    from naws_hip import ops, lib
    op = getattr(lib, 'UN_' + name)
    a, b = T.UNARY_ARGS[name]
    ones = [np.float32(0.75)] + list(T.SPECIALS)
    for x in [T.unary_input(T.LAUNCH_CAP + 37)] + [np.array([v], np.float32) for v in ones]:
        ref = T.unary_ref(name, x, a, b)
        xd = _t(x, dev)
        y = ops.unary(op, xd, a, b)
        same = ops.unary(op, xd, a, b, out=xd)               # in place (the momentum rescale)
        assert same.data_ptr() == xd.data_ptr()
        for got in (_n(y), _n(xd)):
            if name == 'LOG':
                T.check_ulp(got, ref, 2, 'unary LOG')
            else:
                T.check_exact(got, ref, 'unary ' + name, zero_sign=(name != 'RELU'))


@pytest.mark.parametrize('sa,sb', T.BINARY_SHAPES, ids=['%dx%d.%dx%d' % (a + b)
                                                       for a, b in T.BINARY_SHAPES])
def test_binary_broadcast_forms(dev, sa, sb):
    from naws_hip import ops, lib
    a, b = T.binary_inputs(sa, sb)
    ad, bd = _t(a, dev), _t(b, dev)
    for name in T.BINARY_OPS:
        y = ops.binary(getattr(lib, 'BIN_' + name), ad, bd)
        T.check_exact(y, T.binary_ref(name, a, b), 'binary ' + name)


def test_dropout_mask_is_counter_based_past_the_launch_cap(dev):
    from naws_hip import ops
    big = _n(ops.dropout_mask(1234567, 0.5, T.LAUNCH_CAP + 37, dev))
    small = _n(ops.dropout_mask(1234567, 0.5, 740, dev))
    assert np.array_equal(big[:740], small)
    assert np.isin(big, (0.0, 1.0)).all()
    assert abs(big.mean() - 0.5) <= 0.01
    assert np.array_equal(big, T.dropout_mask_ref(1234567, 0.5, big.size))   # the tail past the cap too
    other = _n(ops.dropout_mask(1234568, 0.5, 740, dev))
    assert not np.array_equal(other, small)


@pytest.mark.parametrize('scale', T.SCALES)
def test_softmax_rows_past_one_lane_pass(dev, scale):
    from naws_hip import ops
    for rows in T.SOFTMAX_ROWS:
        for cols in T.SOFTMAX_COLS:
            x, dy = T.softmax_inputs(rows, cols, scale)
            y = ops.softmax_rows(_t(x, dev))
            T.check_prob(y, T.softmax_rows64(x), 'softmax rows')
            dx = ops.softmax_rows_grad(y, _t(dy, dev))
            T.check_softmax_grad(dx, _n(y), dy, of_max=(scale == 1.0))


@pytest.mark.parametrize('shape', [(1, 1), (31, 33), (32, 32), (33, 65), (1, 4099)])
def test_transpose2d_tile_edges(dev, shape):
    from naws_hip import ops
    x = np.random.default_rng(shape).standard_normal(shape).astype(np.float32)
    T.check_exact(ops.transpose2d(_t(x, dev)), x.T, 'transpose')


def _colsum_check(dev, xd, x, accumulate, family):
    """xd: the device view [m, n] (any row stride / base); x: its values."""
    from naws_hip import ops
    m, n = x.shape
    chain, f4 = T.colsum_chain(m, xd.stride(0), n, xd.data_ptr())
    out0 = np.random.default_rng([m, n]).uniform(1, 2, n + 5).astype(np.float32)
    out = _t(out0, dev)
    ops.colsum(xd, out=out, accumulate=accumulate)
    got = _n(out)
    assert np.array_equal(got[n:], out0[n:])                 # nothing written beyond N
    x64 = x.astype(np.float64)
    ref, mass = x64.sum(0), np.abs(x64).sum(0)
    if accumulate:
        ref, mass = ref + out0[:n], mass + out0[:n]
    T.check_colsum(got[:n], ref, mass, chain, family + (' float4' if f4 else ' scalar'))
    return f4


@pytest.mark.parametrize('accumulate', [False, True])
def test_colsum_both_kernels(dev, accumulate):
    from naws_hip import ops
    for m, n in T.COLSUM_F4:
        x = T.colsum_input(m, n)
        assert _colsum_check(dev, _t(x, dev), x, accumulate, 'colsum')
        wide = T.colsum_input(m, n, 8)                       # ld > N, still 16-byte aligned
        assert _colsum_check(dev, _t(wide, dev)[:, 4:4 + n], wide[:, 4:4 + n], accumulate, 'colsum')
        odd = T.colsum_input(m, n, 3)                        # ld not a multiple of 4
        assert not _colsum_check(dev, _t(odd, dev)[:, :n], odd[:, :n], accumulate, 'colsum')
        flat = torch.zeros((m * n + 1,), device=dev)         # base 4 bytes past 16-byte alignment
        view = flat[1:].view(m, n)
        view.copy_(_t(x, dev))
        assert view.data_ptr() % 16 == 4
        assert not _colsum_check(dev, view, x, accumulate, 'colsum')
    for m, n in T.COLSUM_SCALAR:
        x = T.colsum_input(m, n)
        assert not _colsum_check(dev, _t(x, dev), x, accumulate, 'colsum')
        wide = T.colsum_input(m, n, 6)
        assert not _colsum_check(dev, _t(wide, dev)[:, 2:2 + n], wide[:, 2:2 + n], accumulate, 'colsum')
    if not accumulate:
        for m, n in T.COLSUM_F4 + T.COLSUM_SCALAR:
            x = T.colsum_input(m, n)
            chain, _ = T.colsum_chain(m, n, n, 0)
            y = ops.reduce_sum_axis0(_t(x, dev))
            assert tuple(y.shape) == (1, n)
            T.check_colsum(y, x.astype(np.float64).sum(0), np.abs(x).astype(np.float64).sum(0),
                           chain, 'reduce_sum_axis0')


@pytest.mark.parametrize('n', [1, 81, 300, 1025])
def test_stat_accumulate_sizes(dev, n):
    from naws_hip import ops
    from oracle import oracle
    rng = np.random.default_rng([7, n])
    ai = np.full(n, 7.0, np.float32); al = np.full(n, 3.0, np.float32)
    aid, ald = _t(ai, dev), _t(al, dev)
    for it in range(3):
        i = rng.uniform(0, 1, n).astype(np.float32)
        l = (rng.uniform(0, 1, n) > 0.5).astype(np.float32)
        ops.stat_accumulate(_t(i, dev), _t(l, dev), aid, ald, it == 0)
        oracle.stat(i, l, ai, al, it == 0)
    assert np.array_equal(_n(aid), ai) and np.array_equal(_n(ald), al)


@pytest.mark.parametrize('weighted', [True, False])
@pytest.mark.parametrize('is_mean', [True, False])
def test_weighted_ce_rows_per_problem(dev, weighted, is_mean):
    from naws_hip import ops
    from oracle import oracle
    for n, c in T.WCE_SHAPES:
        x, l, w, dy = T.wce_inputs(n, c)
        wd = _t(w, dev) if weighted else None
        y = _n(ops.weighted_ce(_t(x, dev), _t(l, dev), wd, is_mean, 3))
        dx = _n(ops.weighted_ce_grad(_t(x, dev), _t(l, dev), wd, _t(dy, dev), is_mean, 3))
        capped = 0
        for p in range(3):
            wp = w[p] if weighted else None
            np.testing.assert_allclose(y[p], oracle.weighted_ce(x[p], l[p], wp, is_mean), rtol=1e-6,
                                       atol=1e-6)
            np.testing.assert_allclose(dx[p], oracle.weighted_ce_grad(x[p], l[p], wp, dy[p:p + 1],
                                                                      is_mean), rtol=1e-6, atol=1e-6)
            T.check_wce(y[p], T.wce64(x[p], l[p], wp, is_mean), T.wce_bound64(x[p], l[p], wp, is_mean))
            ref, mag = T.wce_grad64(x[p], l[p], wp, dy[p], is_mean)
            T.check_wce(dx[p], ref, T.WCE_GRAD_EPS * mag, 'wce grad')
            capped += int((ref == T.WCE_CAP * (1.0 if wp is None else wp.astype(np.float64)) / n).sum())
        assert capped >= 1                                   # the 1e4 cap was reached


@pytest.mark.parametrize('is_mean', [True, False])
def test_weighted_ce_shared_labels_rows_per_problem(dev, is_mean):
    """The shared-labels form ([lab_period, N, C] labels, problem p scored against p % lab_period,
    gradient seeded by a constant) at N > 1 rows per problem: the Python wrapper fixes N = 1, so
    the entry points are called as the wrapper calls them."""
    from naws_hip import ops, lib
    stream = torch.cuda.current_stream().cuda_stream
    for n, c in T.WCE_SHAPES:
        x6, _, w6, _ = T.wce_inputs(n, c, nprob=6)           # 2 branches x 3 images
        _, l3, _, _ = T.wce_inputs(n, c, nprob=3)
        xd, ld, wd = _t(x6, dev), _t(l3, dev), _t(w6, dev)
        y = torch.empty((6,), device=dev)
        dx = torch.empty_like(xd)
        lib.call('naws_weighted_ce_shared_fwd', xd.data_ptr(), ld.data_ptr(), wd.data_ptr(), n, c,
                 int(is_mean), 6, 3, y.data_ptr(), stream)
        lib.call('naws_weighted_ce_shared_bwd', xd.data_ptr(), ld.data_ptr(), wd.data_ptr(), 0, 0.5,
                 n, c, int(is_mean), 6, 3, dx.data_ptr(), stream)
        l6 = _t(np.concatenate([l3, l3]), dev)
        half = torch.full((6,), 0.5, device=dev)
        assert torch.equal(y, ops.weighted_ce(xd, l6, wd, is_mean, 6))
        assert torch.equal(dx, ops.weighted_ce_grad(xd, l6, wd, half, is_mean, 6))
        y, dx = _n(y), _n(dx)
        for p in range(6):
            lp = l3[p % 3]
            T.check_wce(y[p], T.wce64(x6[p], lp, w6[p], is_mean), T.wce_bound64(x6[p], lp, w6[p], is_mean),
                        'wce shared')
            ref, mag = T.wce_grad64(x6[p], lp, w6[p], 0.5, is_mean)
            T.check_wce(dx[p], ref, T.WCE_GRAD_EPS * mag, 'wce shared grad')
    # and the wrapper's own N = 1 form at the OICR class counts
    for c in (21, 81):
        x, _, w, _ = T.wce_inputs(1, c, nprob=6)
        x, w = x.reshape(2, 3, c), w.reshape(2, 3, c)
        l = T.wce_inputs(1, c, nprob=3)[1].reshape(3, c)
        y = _n(ops.weighted_ce_shared(_t(x, dev), _t(l, dev), _t(w, dev), is_mean))
        dx = _n(ops.weighted_ce_shared_grad(_t(x, dev), _t(l, dev), _t(w, dev), is_mean))
        for b in range(2):
            for s in range(3):
                xs, ls, ws = x[b, s:s + 1], l[s:s + 1], w[b, s:s + 1]
                T.check_wce(y[b * 3 + s], T.wce64(xs, ls, ws, is_mean), T.wce_bound64(xs, ls, ws, is_mean),
                            'wce shared')
                ref, mag = T.wce_grad64(xs, ls, ws, 1.0, is_mean)
                T.check_wce(dx[b, s:s + 1], ref, T.WCE_GRAD_EPS * mag, 'wce shared grad')


# ------------------------------------------------------------------------------- wrappers ----
@pytest.mark.parametrize('need_dx', [True, False])
@pytest.mark.parametrize('n_out,k', [(21, 128), (81, 64)])
def test_fc_wrappers_pad_odd_output_counts(dev, n_out, k, need_dx):
    from detectron import ops as dops
    rng = np.random.default_rng([n_out, k])
    x = rng.uniform(-1, 1, (37, k)).astype(np.float32)
    w = rng.uniform(-1, 1, (n_out, k)).astype(np.float32)
    b = rng.uniform(-1, 1, n_out).astype(np.float32)
    dy = rng.uniform(-1, 1, (37, n_out)).astype(np.float32)
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    y = dops.FC(_t(x, dev), _t(w, dev), _t(b, dev))
    assert tuple(y.shape) == (37, n_out) and y.is_contiguous()
    T.check_gemm(y, x64 @ w64.T + b, 'FC')
    dw, db, dx = dops.FCGradient(_t(x, dev), _t(w, dev), _t(dy, dev), need_dx=need_dx)
    assert tuple(dw.shape) == (n_out, k) and tuple(db.shape) == (n_out,)
    T.check_gemm(dw, dy64.T @ x64, 'FCGradient dW')
    T.check_colsum(db, dy64.sum(0), np.abs(dy64).sum(0), T.colsum_chain(37, n_out + 3, n_out + 3, 0)[0],
                   'FCGradient db')
    if need_dx:
        assert tuple(dx.shape) == (37, k)
        T.check_gemm(dx, dy64 @ w64, 'FCGradient dX')
    else:
        assert dx is None


@pytest.mark.parametrize('m,k,n', [(333, 333, 21), (5, 7, 3)])
def test_matmul_wrapper_pads_odd_dims(dev, m, k, n):
    from detectron import ops as dops
    rng = np.random.default_rng([m, k, n])
    a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    b = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    y = dops.MatMul(_t(a, dev), _t(b, dev))
    assert tuple(y.shape) == (m, n)
    T.check_gemm(y, a.astype(np.float64) @ b.astype(np.float64), 'MatMul')
