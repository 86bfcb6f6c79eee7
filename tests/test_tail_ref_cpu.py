"""The float64 references of tests/tail_ref.py, pinned without a GPU.

(1) On the exact inputs of tests/test_gpu_tail_edges.py the fp32 oracle (oracle/naws_oracle.c)
passes the very comparisons the HIP kernels are held to: the bounds are a property of the
operation, its inputs and fp32, not of the code under test.
(2) Each comparison rejects references that are wrong the way a kernel's index arithmetic goes
wrong: a segment reduction that leaves the segment's last row out, a segment that reads its
neighbour's class vector, a column sum that drops a row, a softmax that does not subtract the
maximum, a gate normalised by the longest segment's length, a broadcast that reads column 0."""
import functools

import numpy as np
import pytest

import tail_ref as T


def _oracle():
    from oracle import oracle
    return oracle


@functools.lru_cache(maxsize=None)
def _iou_cached(key, shape):
    return _oracle().roi_iou(np.frombuffer(key, np.float32).reshape(shape))


def iou(rois):
    rois = np.ascontiguousarray(rois, np.float32)
    return _iou_cached(rois.tobytes(), rois.shape)


@functools.lru_cache(maxsize=None)
def oracle_wsddn(lens, c, scale):
    """The fp32 oracle image by image -> ac, ad, rp [2, Rt, C], cp [2, nseg, C] (fp32)."""
    fc8c, fc8d, nc, nd, _ = T.wsddn_inputs(lens, c, scale)
    seg = T.seg_of(lens)
    ac, ad, rp = (np.zeros((2, int(seg[-1]), c), np.float32) for _ in range(3))
    cp = np.zeros((2, len(lens), c), np.float32)
    for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        sl = slice(lo, hi)
        for b, noisy in enumerate(((None, None), (nc[sl], nd[sl]))):
            r = _oracle().wsddn_outputs(fc8c[sl], fc8d[sl], *noisy)
            ac[b, sl], ad[b, sl], rp[b, sl], cp[b, s] = r[0], r[1], r[2], r[3][0]
    return ac, ad, rp, cp


WSDDN_CASES = [(T.WSDDN_LENS, c, s) for c in T.WSDDN_CLASSES for s in T.SCALES] + \
              [(T.WSDDN_MANY, 21, 1.0)]
WSDDN_IDS = ['%dseg-C%d-x%d' % (len(l), c, s) for l, c, s in WSDDN_CASES]


# ------------------------------------------------- (1) the oracle inside the GPU module's bounds
@pytest.mark.parametrize('lens,c,scale', WSDDN_CASES, ids=WSDDN_IDS)
def test_oracle_wsddn_outputs_inside_the_bounds(lens, c, scale):
    got = oracle_wsddn(lens, c, scale)
    ref = T.wsddn_forward_ref(lens, c, scale, 2)
    for g, r, name in zip(got, ref, ('alpha_cls', 'alpha_det', 'rois_pred', 'cls_prob')):
        T.check_prob(g, r, 'oracle wsddn ' + name)


@pytest.mark.parametrize('lens,c,scale', WSDDN_CASES, ids=WSDDN_IDS)
def test_oracle_wsddn_gradients_inside_the_bounds(lens, c, scale):
    ac, ad, _, _ = oracle_wsddn(lens, c, scale)
    g = T.wsddn_inputs(lens, c, scale)[4]
    seg = T.seg_of(lens)
    d = np.zeros((2, 2, ac.shape[1], c), np.float32)
    for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        for b in range(2):
            d[b, 0, lo:hi], d[b, 1, lo:hi] = _oracle().wsddn_outputs_grad(ac[b, lo:hi], ad[b, lo:hi],
                                                                         g[b, s])
    got = (d[0, 0] + d[1, 0], d[0, 1] + d[1, 1], d[1, 0], d[1, 1])
    T.check_wsddn_grads(got, T.wsddn_backward_ref(lens, ac, ad, g), lens, ad, g, 'oracle wsddn grad')
    T.check_wsddn_grads((d[0, 0], d[0, 1], None, None), T.wsddn_backward_ref(lens, ac[:1], ad[:1], g[:1]),
                        lens, ad[:1], g[:1], 'oracle wsddn grad')


GATE_INPUTS = sorted(set((l, c) for l, c, _ in T.GATE_CASES))


@pytest.mark.parametrize('lens,c', GATE_INPUTS, ids=['%s-C%d' % ('_'.join(map(str, l)), c)
                                                     for l, c in GATE_INPUTS])
def test_oracle_entropy_gate_inside_the_bounds(lens, c):
    rois, rp, cp, labels = T.gate_inputs(lens, c)
    seg = T.seg_of(lens)
    got = np.zeros((4, len(lens), c), np.float32)
    for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        for k, o in enumerate(_oracle().entropy_gate(rois[lo:hi], rp[lo:hi], cp[s], labels[s])):
            got[k, s] = o[0]
    ref = T.gate_ref(lens, c, iou)
    T.check_gate4(got, ref, 'oracle gate')
    nan = np.isnan(ref)                     # the inputs do hold the NaN case, and only there
    assert nan[:, 1, T.GATE_NAN_CLASS].all() and nan.sum() == 4


@pytest.mark.parametrize('scale', T.SCALES)
def test_oracle_softmax_rows_inside_the_bounds(scale):
    for rows in T.SOFTMAX_ROWS:
        for cols in T.SOFTMAX_COLS:
            x, dy = T.softmax_inputs(rows, cols, scale)
            y = _oracle().wsddn_outputs(x, x)[0]          # alpha_cls: the oracle's row softmax
            T.check_prob(y, T.softmax_rows64(x), 'oracle softmax')
            d32 = y * (dy - (y * dy).sum(1, keepdims=True, dtype=np.float32))
            T.check_softmax_grad(d32, y, dy, 'oracle softmax grad', of_max=(scale == 1.0))
            if cols > 1 and scale == 1.0:           # (scale 30: rows nearly one-hot, a column is nothing)
                rejects(T.check_softmax_grad, y * (dy - (y * dy)[:, :-1].sum(1, keepdims=True)), y, dy)


def test_fp32_column_sums_inside_the_bound():
    for m, n in T.COLSUM_F4 + T.COLSUM_SCALAR:
        x = T.colsum_input(m, n)
        chain, _ = T.colsum_chain(m, n, n, 0)
        acc = np.zeros(n, np.float32)
        for r in range(m):                                # one serial fp32 chain: the worst order
            acc = acc + x[r]
        T.check_colsum(acc, x.astype(np.float64).sum(0), np.abs(x).astype(np.float64).sum(0), m,
                       'serial colsum')
        T.check_colsum(x.sum(0, dtype=np.float32), x.astype(np.float64).sum(0),
                       np.abs(x).astype(np.float64).sum(0), chain, 'numpy colsum')
        assert (np.abs(x).min(0) >= np.abs(x).sum(0) / (3 * m)).all()


@pytest.mark.parametrize('weighted', [True, False])
@pytest.mark.parametrize('is_mean', [True, False])
def test_oracle_weighted_ce_inside_the_bounds(weighted, is_mean):
    for n, c in T.WCE_SHAPES:
        x, l, w, dy = T.wce_inputs(n, c)
        capped = 0
        for p in range(x.shape[0]):
            wp = w[p] if weighted else None
            T.check_wce(_oracle().weighted_ce(x[p], l[p], wp, is_mean), T.wce64(x[p], l[p], wp, is_mean),
                        T.wce_bound64(x[p], l[p], wp, is_mean), 'oracle wce')
            ref, mag = T.wce_grad64(x[p], l[p], wp, dy[p], is_mean)
            T.check_wce(_oracle().weighted_ce_grad(x[p], l[p], wp, dy[p:p + 1], is_mean), ref,
                        T.WCE_GRAD_EPS * mag, 'oracle wce grad')
            capped += int((ref == T.WCE_CAP * (1.0 if wp is None else wp.astype(np.float64)) / n).sum())
        assert capped >= 1                                # the inputs do reach the 1e4 cap


def test_elementwise_references_on_the_special_values():
    x = T.unary_input(12)[:6]
    assert np.array_equal(T.unary_ref('RELU', x, 0, 0), np.float32([0, np.inf, 0, 0, 1e-40, 0]))
    clip = T.unary_ref('CLIP', x, -0.5, 1.0)
    assert np.isnan(clip[0]) and np.array_equal(clip[1:], np.float32([1, -0.5, -0.0, 1e-40, -3e-42]))
    leaky = T.unary_ref('LEAKY_RELU', x, 0.01, 0)
    assert np.signbit(leaky[3]) and leaky[3] == 0 and np.isnan(leaky[0]) and leaky[2] == -np.inf
    big = T.unary_input(T.LAUNCH_CAP + 37)
    for at in (0, T.LAUNCH_CAP - 1, T.LAUNCH_CAP, T.LAUNCH_CAP + 36):
        assert np.isnan(big[at]) or big[at] in T.SPECIALS
    assert np.isnan(big[[0, T.LAUNCH_CAP - 1, T.LAUNCH_CAP, -1]]).all()


# ------------------------------------------------------------- (2) wrong references are rejected
def rejects(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


@pytest.mark.parametrize('c', T.WSDDN_CLASSES)
def test_a_segment_sum_without_its_last_row_is_rejected_wsddn(c):
    lens = T.WSDDN_LENS
    seg = T.seg_of(lens)
    ref = T.wsddn_forward_ref(lens, c, 1.0, 2)
    bad = T.wsddn_forward_ref(lens, c, 1.0, 2, last_row=False)
    ac32, ad32 = ref[0].astype(np.float32), ref[1].astype(np.float32)
    g = T.wsddn_inputs(lens, c, 1.0)[4]
    gref = T.wsddn_backward_ref(lens, ac32, ad32, g)
    gbad = T.wsddn_backward_ref(lens, ac32, ad32, g, last_row=False)
    for s, n in enumerate(lens):
        sl = slice(seg[s], seg[s + 1])             # each segment on its own, the longest included
        if c > 1:                                  # (C = 1: the exact gradient is zero whatever y is)
            rejects(T.check_grad, gbad[1][sl], gref[1][sl])
        if n < 2:                                  # (one roi: the forward mutant divides by nothing)
            continue
        rejects(T.check_prob, bad[1][:, sl], ref[1][:, sl])
        rejects(T.check_prob, bad[2][:, sl], ref[2][:, sl])
        if c > 1:                                  # (C = 1: cls_prob = sum alpha_det = 1 either way)
            rejects(T.check_prob, bad[3][:, s], ref[3][:, s])


@pytest.mark.parametrize('lens,c', [(T.GATE_RAGGED, 20), (T.GATE_RAGGED, 81), ((2049, 16, 700), 20),
                                    ((5, 40), 300)])
def test_wrong_gate_references_are_rejected(lens, c):
    ref = T.gate_ref(lens, c, iou)
    short = T.gate_ref(lens, c, iou, last_row=False)
    shifted = T.gate_ref(lens, c, iou, shift_class_vector=True)
    nmax = T.gate_ref(lens, c, iou, n_is_max=True)
    for s, n in enumerate(lens):
        one = slice(s, s + 1)
        if n >= 2:
            rejects(T.check_gate4, short[:, one], ref[:, one])
        rejects(T.check_gate4, shifted[:, one], ref[:, one])
        if n != max(lens):
            # the normalised outputs alone (hatE_sum does not depend on n)
            rejects(T.check_gate, nmax[3, one], ref[3, one])
            rejects(T.check_gate, nmax[1, one], ref[1, one])
            rejects(T.check_gate, nmax[0, one], ref[0, one])


def test_a_neighbours_class_vector_is_rejected_wsddn():
    for lens, c in ((T.WSDDN_LENS, 20), (T.WSDDN_LENS, 81), (T.WSDDN_MANY, 21)):
        ref = T.wsddn_forward_ref(lens, c, 1.0, 2)
        ac32, ad32 = ref[0].astype(np.float32), ref[1].astype(np.float32)
        g = T.wsddn_inputs(lens, c, 1.0)[4]
        good = T.wsddn_backward_ref(lens, ac32, ad32, g)
        bad = T.wsddn_backward_ref(lens, ac32, ad32, g, shift_class_vector=True)
        seg = T.seg_of(lens)
        for k in range(4):
            rejects(T.check_grad, bad[k], good[k])
            if c > 1:
                for s in range(len(lens)):
                    if lens[s] > 1:                 # (one roi: alpha_det = 1 and dzd = 0 whatever g)
                        rejects(T.check_grad, bad[k][seg[s]:seg[s + 1]], good[k][seg[s]:seg[s + 1]])


def test_a_dropped_row_is_rejected_colsum():
    for m, n in T.COLSUM_F4 + T.COLSUM_SCALAR:
        x = T.colsum_input(m, n).astype(np.float64)
        for ld, off in ((n, 0), (n + 3, 4)):
            chain, _ = T.colsum_chain(m, ld, n, off)
            for r in sorted({0, m // 2, m - 1}):
                rejects(T.check_colsum, x.sum(0) - x[r], x.sum(0), np.abs(x).sum(0), chain)


@pytest.mark.parametrize('c', T.WSDDN_CLASSES)
def test_a_softmax_that_keeps_the_maximum_is_rejected(c):
    ref = T.wsddn_forward_ref(T.WSDDN_LENS, c, 30.0, 2)
    bad = T.wsddn_forward_ref(T.WSDDN_LENS, c, 30.0, 2, subtract_max=False)
    for k in (1, 2, 3) + ((0,) if c > 1 else ()):       # (C = 1: exp(z) / exp(z) survives to |z| < 88)
        rejects(T.check_prob, bad[k], ref[k])
    for cols in T.SOFTMAX_COLS[1:]:
        x, _ = T.softmax_inputs(129, cols, 30.0)
        with np.errstate(all='ignore'):
            e = np.exp(x)
            rejects(T.check_prob, e / e.sum(1, keepdims=True, dtype=np.float32), T.softmax_rows64(x))


def test_a_broadcast_that_reads_column_0_is_rejected():
    for sa, sb in T.BINARY_SHAPES[1:]:
        a, b = T.binary_inputs(sa, sb)
        for op in T.BINARY_OPS:
            if max(sa[1], sb[1]) > 1 and (sa[1] > 1 or sb[1] > 1):
                rejects(T.check_exact, T.binary_ref(op, a, b, column0=True), T.binary_ref(op, a, b))
    a, b = T.binary_inputs((129, 65), (129, 1))
    good = T.binary_ref('MUL', a, b)
    rejects(T.check_exact, T.binary_ref('MUL', a, b[:1]), good)      # row 0 instead of row r
    rejects(T.check_exact, -good, good)
    rejects(T.check_exact, np.where(good == 0, np.float32(0.0), good), good)   # -0.0 -> +0.0
    T.check_exact(np.where(good == 0, np.float32(0.0), good), good, zero_sign=False)
    rejects(T.check_ulp, np.float32(np.log(2.0)) * np.float32(1 + 4e-7), np.log(np.float64(2.0)), 2, 'log')
    T.check_ulp(np.float32([np.log(2.0), -np.inf, np.nan]), np.float64([np.log(2.0), -np.inf, np.nan]), 2, 'log')
