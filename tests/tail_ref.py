"""float64 numpy restatements of the loss-tail operators (csrc/head_ops.hip) and of the graph
executor's small built-ins (csrc/misc_ops.hip), the seeded inputs of their edge-shape tests, and
the comparisons those tests assert.  The arbiter of tests/test_tail_ref_cpu.py (which holds the
fp32 oracle to the same comparisons on the same inputs and feeds them deliberately wrong
references) and of tests/test_gpu_tail_edges.py.

Every sum, exp, log and division below is float64.  Where the graph hands an fp32 blob from one
operator to the next (the residual Add of the noise branch, the probabilities that feed a gradient
or the gate) the blob is taken as given, in fp32, and only the operator under test is restated."""
import functools

import numpy as np

from helpers import make_rois

F32_EPS = 2.0 ** -24            # half an fp32 ulp of 1: one rounding's relative error
WCE_MIN = float(np.float32(1e-20))   # cross_entropy_wsl_op.h:90, an fp32 constant
WCE_CAP = 1e4                        # cross_entropy_wsl_op.cc:170
# the fp32 gradient of one element: 1 - x, 1 - l, l / p, (1 - l) / q, their difference, x dy,
# / norm, x w, x (1 / N) and the constant 1 / N itself are ten roundings; two more of slack
WCE_GRAD_EPS = 12 * 2.0 ** -24


# ------------------------------------------------------------------------------ references ----
def softmax_rows64(x):
    """Caffe2 Softmax over axis 1 (caffe2/operators/softmax_shared.cc, v1.3.0): subtract the row
    maximum, exp, divide by the row sum."""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def softmax_rows_grad64(y, dy):
    y, dy = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    return y * (dy - (y * dy).sum(1, keepdims=True))


def wsddn_outputs64(fc8c, fc8d, nc=None, nd=None):
    """One image (wsl_heads.py:51-55, :227; webly_heads.py:57-74) -> alpha_cls, alpha_det,
    rois_pred [R, C], cls_prob [C].  The residual Add is an operator of its own whose fp32 output
    blob is what the softmaxes read, so it is rounded to fp32 here as well."""
    zc, zd = np.asarray(fc8c, np.float32), np.asarray(fc8d, np.float32)
    if nc is not None:
        zc = zc + np.asarray(nc, np.float32)
        zd = zd + np.asarray(nd, np.float32)
    ac = softmax_rows64(zc)
    ad = softmax_rows64(zd.T).T
    rp = ac * ad
    return ac, ad, rp, rp.sum(0)


def wsddn_outputs_grad64(alpha_cls, alpha_det, g):
    """One image, one branch: d cls_prob [C] -> dzc, dzd [R, C] (gradients with respect to the
    branch's summed logits).  dzc = ac (g ad - sum_k g ad ac), dzd = ad (g ac - g y) with
    y = sum_r ac ad summed here, in float64, from the given ac and ad."""
    ac, ad = np.asarray(alpha_cls, np.float64), np.asarray(alpha_det, np.float64)
    g = np.asarray(g, np.float64).reshape(1, -1)
    y = (ac * ad).sum(0, keepdims=True)
    dzc = ac * (g * ad - (g * ad * ac).sum(1, keepdims=True))
    dzd = ad * (g * ac - g * y)
    return dzc, dzd


def entropy_gate64(J, rois_pred, cls_prob, labels, n=None):
    """One image, statement for statement after oracle_entropy_gate (webly_heads.py:265-391):
    E = ReplaceNaN(-(p log p), 0); D = LeakyRelu(J E, 0.01); hatE_sum = sum_r E * (E / D);
    norm = (log n - log y) y; v = Clip(hatE_sum / norm, 0, 1) (NaN passes); w_noise = v (1 - l);
    w = 1 - w_noise.  J is the fp32 IoU matrix, taken as given.  `n` (default: the image's own
    number of rois) exists so that a test can put a wrong one in.
    -> class_weight, class_weight_noise, hatE_sum, hatE_sum_norm, each [C]."""
    J = np.asarray(J, np.float64)
    p = np.asarray(rois_pred, np.float64)
    y = np.asarray(cls_prob, np.float64).reshape(-1)
    lab = np.asarray(labels, np.float64).reshape(-1)
    n = p.shape[0] if n is None else n
    with np.errstate(all='ignore'):
        E = -(p * np.log(p))
        E = np.where(np.isnan(E), 0.0, E)
        D = J @ E
        D = np.where(D >= 0, D, 0.01 * D)
        s = (E * (E / D)).sum(0)
        norm = (np.log(float(n)) - np.log(y)) * y
        v = s / norm
        v = np.where(v < 0, 0.0, v)
        v = np.where(v > 1, 1.0, v)
    wn = v * (1.0 - lab)
    return 1.0 - wn, wn, s, v


def _wce_terms64(x, l, w):
    x, l = np.asarray(x, np.float64), np.asarray(l, np.float64)
    prob = np.maximum(x, WCE_MIN)
    one_prob = np.maximum(1.0 - x, WCE_MIN)
    t = l * np.log(prob) + (1.0 - l) * np.log(one_prob)
    return t if w is None else t * np.asarray(w, np.float64)


def wce64(x, l, w, is_mean):
    """(Weighted)CrossEntropyWithLogits of one [N, C] problem (cross_entropy_wsl_op.cc:7-45,
    :87-132): both arguments of log clamped at 1e-20, / C when is_mean, then / N."""
    n, c = np.shape(x)
    return -_wce_terms64(x, l, w).sum() / (c if is_mean else 1.0) / n


def wce_bound64(x, l, w, is_mean):
    """N C 2^-24 sum |terms| (scaled like the loss): the worst case of a serial fp32 sum of N C
    terms, each of which carries a handful of roundings of its own."""
    n, c = np.shape(x)
    return n * c * F32_EPS * np.abs(_wce_terms64(x, l, w)).sum() / (c if is_mean else 1.0) / n


def wce_grad64(x, l, w, dy, is_mean):
    """cross_entropy_wsl_op.cc:47-85, :134-180: capped at 1e4 BEFORE the weight.
    -> (gradient [N, C], magnitude [N, C] its roundings scale with: |error| <= WCE_GRAD_EPS x it)."""
    x, l = np.asarray(x, np.float64), np.asarray(l, np.float64)
    n, c = x.shape
    norm = c if is_mean else 1.0
    prob = np.maximum(x, WCE_MIN)
    one_prob = np.maximum(1.0 - x, WCE_MIN)
    wt = 1.0 if w is None else np.asarray(w, np.float64)
    raw = float(dy) * (-l / prob + (1.0 - l) / one_prob) / norm
    mag = abs(float(dy)) * (l / prob + (1.0 - l) / one_prob) / norm
    mag = np.where(raw > WCE_CAP, WCE_CAP, mag)
    return np.minimum(raw, WCE_CAP) * wt / n, mag * wt / n


# ---------------------------------------------------------------------------------- inputs ----
WSDDN_LENS = (1, 255, 256, 257, 2, 700)        # around TB = 256 rows, and the shortest segments
WSDDN_MANY = tuple(range(1, 41))               # 40 segments: the backward's find_segment walk
WSDDN_CLASSES = (1, 20, 21, 81)
SCALES = (1.0, 30.0)                           # 30: |z| passes 88, where expf alone overflows


def seg_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def wsddn_inputs(lens, c, scale):
    """-> fc8c, fc8d, noisy_fc8c, noisy_fc8d [Rt, C] fp32, d_cls_prob [2, nseg, C] fp32."""
    rng = np.random.default_rng([31, sum(lens), c, int(scale)])
    rt = sum(lens)
    z = [(rng.standard_normal((rt, c)) * s * scale).astype(np.float32) for s in (1.0, 1.0, 0.25, 0.25)]
    g = rng.standard_normal((2, len(lens), c)).astype(np.float32)
    for a in z + [g]:
        a.setflags(write=False)
    return z[0], z[1], z[2], z[3], g


@functools.lru_cache(maxsize=None)
def wsddn_forward_ref(lens, c, scale, nb, last_row=True, subtract_max=True):
    """float64 forward of a whole batch -> ac, ad, rp [nb, Rt, C], cp [nb, nseg, C].
    last_row False / subtract_max False build the wrong references of the CPU module: every
    segment reduction skips the segment's last row / the softmaxes run in fp32 on the raw logits."""
    fc8c, fc8d, nc, nd, _ = wsddn_inputs(lens, c, scale)
    seg = seg_of(lens)
    rt = int(seg[-1])
    ac, ad, rp = (np.zeros((nb, rt, c)) for _ in range(3))
    cp = np.zeros((nb, len(lens), c))
    for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        sl = slice(lo, hi)
        for b in range(nb):
            noisy = (nc[sl], nd[sl]) if b == 1 else (None, None)
            if not subtract_max:
                r = _wsddn_naive32(fc8c[sl], fc8d[sl], *noisy)
            elif not last_row:
                r = _wsddn_short64(fc8c[sl], fc8d[sl], *noisy)
            else:
                r = wsddn_outputs64(fc8c[sl], fc8d[sl], *noisy)
            ac[b, sl], ad[b, sl], rp[b, sl], cp[b, s] = r
    return ac, ad, rp, cp


def _wsddn_short64(fc8c, fc8d, nc, nd):
    """WRONG on purpose: the column softmax's sum and the cls_prob sum leave the last row out."""
    zc, zd = np.asarray(fc8c, np.float32), np.asarray(fc8d, np.float32)
    if nc is not None:
        zc, zd = zc + nc, zd + nd
    ac = softmax_rows64(zc)
    with np.errstate(all='ignore'):
        e = np.exp(zd.astype(np.float64) - zd.max(0, keepdims=True))
        ad = e / e[:-1].sum(0, keepdims=True)
    rp = ac * ad
    return ac, ad, rp, rp[:-1].sum(0)


def _wsddn_naive32(fc8c, fc8d, nc, nd):
    """WRONG on purpose: fp32 softmaxes that do not subtract the maximum."""
    zc, zd = np.asarray(fc8c, np.float32), np.asarray(fc8d, np.float32)
    if nc is not None:
        zc, zd = zc + nc, zd + nd
    with np.errstate(all='ignore'):
        ec, ed = np.exp(zc), np.exp(zd)
        ac = ec / ec.sum(1, keepdims=True, dtype=np.float32)
        ad = ed / ed.sum(0, keepdims=True, dtype=np.float32)
    rp = ac * ad
    return ac, ad, rp, rp.sum(0)


def wsddn_backward_ref(lens, ac, ad, g, shift_class_vector=False, last_row=True):
    """float64 backward of a whole batch from the given fp32 ac, ad [nb, Rt, C] and g
    [nb, nseg, C] -> d_fc8c, d_fc8d, d_noisy_fc8c, d_noisy_fc8d [Rt, C] (the last two None for
    nb = 1).  shift_class_vector / last_row False build the wrong references: segment s reads
    segment s + 1's d_cls_prob / y leaves the segment's last row out."""
    nb, rt, c = ac.shape
    seg = seg_of(lens)
    d = np.zeros((nb, 2, rt, c))
    for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        sl = slice(lo, hi)
        gs = (s + 1) % len(lens) if shift_class_vector else s
        for b in range(nb):
            if last_row:
                d[b, 0, sl], d[b, 1, sl] = wsddn_outputs_grad64(ac[b, sl], ad[b, sl], g[b, gs])
            else:
                a, e = np.asarray(ac[b, sl], np.float64), np.asarray(ad[b, sl], np.float64)
                gg = np.asarray(g[b, gs], np.float64).reshape(1, -1)
                y = (a * e)[:-1].sum(0, keepdims=True)
                d[b, 0, sl] = a * (gg * e - (gg * e * a).sum(1, keepdims=True))
                d[b, 1, sl] = e * (gg * a - gg * y)
    if nb == 1:
        return d[0, 0], d[0, 1], None, None
    return d[0, 0] + d[1, 0], d[0, 1] + d[1, 1], d[1, 0], d[1, 1]


def wsddn_one_class_bound(lens, ad, g):
    """C = 1 is the one class count at which the exact gradient is identically zero: alpha_cls = 1,
    so dzc = g ad - g ad, and y = sum_r alpha_det = 1, so dzd = ad g (1 - y) is nothing but the
    rounding of that sum.  A fraction of max |reference| is then a fraction of noise; what can be
    asserted instead is |dzc| <= 4 2^-24 |g| ad (the product g ad rounded on one side of the
    difference and, under fma contraction, not on the other) and |dzd| <= (len + 8) 2^-24 |g| ad,
    the worst case of an fp32 sum of len terms that each carry a few roundings.
    -> bounds for d_fc8c, d_fc8d, d_noisy_fc8c, d_noisy_fc8d [Rt, 1]."""
    nb, rt, c = ad.shape
    assert c == 1
    seg = seg_of(lens)
    b = np.zeros((nb, rt, 1))
    n = np.zeros((rt, 1))
    for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        b[:, lo:hi] = np.abs(np.asarray(g, np.float64)[:, s, None, :]) * np.asarray(ad, np.float64)[:, lo:hi]
        n[lo:hi] = (hi - lo) + 8
    b *= F32_EPS
    return 4 * b.sum(0), n * b.sum(0), 4 * b[-1], n * b[-1]


# (segment lengths, C, pass max_seg_len = Rt instead of the true maximum)
GATE_RAGGED = (1, 17, 64, 65, 333)
GATE_NAN_CLASS = 4
GATE_CASES = tuple([(GATE_RAGGED, c, False) for c in (20, 21, 40, 41, 81)] +
                   [(GATE_RAGGED, 21, True),
                    ((2049, 16, 700), 20, False),       # JCH cap, 33 row blocks, 129 finish chunks
                    ((5, 40), 300, False)])             # C > TB in the finish, four GCC passes


@functools.lru_cache(maxsize=None)
def gate_inputs(lens, c):
    """-> rois [Rt, 5], rois_pred [Rt, C], cls_prob [nseg, C], labels [nseg, C], all fp32.
    rois: helpers.make_rois per segment (degenerate boxes from 8 rois up) with the batch index
    rewritten; rois_pred / cls_prob: the float64 WSDDN outputs of random logits, rounded; one
    fractional label; rois_pred = 0 at one roi of the longest image, and in a whole class column of
    image 1 (there E = 0, D = 0 and 0 / 0 = NaN in all four outputs)."""
    rng = np.random.default_rng([41, sum(lens), c])
    rois, rp, cp = [], [], []
    for s, n in enumerate(lens):
        r = make_rois(rng, 1, n, 600, 1000)
        r[:, 0] = s
        rois.append(r)
        z = rng.standard_normal((2, n, c)).astype(np.float32)
        _, _, p, y = wsddn_outputs64(z[0] * 2, z[1] * 3)
        rp.append(p.astype(np.float32))
        cp.append(y.astype(np.float32))
    labels = np.zeros((len(lens), c), np.float32)
    for s in range(len(lens)):
        labels[s, (3 + 5 * s) % c] = 1.0
    labels[-1, 7] = 0.4                                   # mixup-style fractional label
    big = int(np.argmax(lens))
    rp[big][min(6, lens[big] - 1), 2] = 0.0               # p = 0 -> 0 log 0 = NaN -> ReplaceNaN -> 0
    rp[1][:, GATE_NAN_CLASS] = 0.0                        # image 1: a class with E = 0, D = 0: 0 / 0
    out = (np.concatenate(rois), np.concatenate(rp), np.stack(cp), labels)
    for a in out:
        a.setflags(write=False)
    return out


def gate_ref(lens, c, J_of, last_row=True, shift_class_vector=False, n_is_max=False):
    """float64 gate of a whole batch -> 4 x [nseg, C].  J_of(rois) -> the fp32 IoU matrix of one
    image (oracle.roi_iou).  The three flags build the wrong references of the CPU module."""
    rois, rp, cp, labels = gate_inputs(lens, c)
    seg = seg_of(lens)
    outs = np.zeros((4, len(lens), c))
    for s, (lo, hi) in enumerate(zip(seg[:-1], seg[1:])):
        J = np.asarray(J_of(rois[lo:hi]), np.float64)
        p = rp[lo:hi].astype(np.float64)
        if not last_row:                 # the last roi drops out of J E and of the sum over rois
            J = J[:, :-1][:-1]
            p = p[:-1]
        cs = (s + 1) % len(lens) if shift_class_vector else s
        r = entropy_gate64(J, p, cp[cs], labels[cs], n=max(lens) if n_is_max else hi - lo)
        for k in range(4):
            outs[k, s] = r[k]
    return outs


def softmax_inputs(rows, cols, scale):
    rng = np.random.default_rng([51, rows, cols, int(scale)])
    return ((rng.standard_normal((rows, cols)) * scale).astype(np.float32),
            rng.standard_normal((rows, cols)).astype(np.float32))


SOFTMAX_ROWS, SOFTMAX_COLS = (1, 5, 129), (1, 63, 64, 65, 81, 300)

COLSUM_F4 = ((1, 4), (31, 36), (127, 64), (128, 64), (129, 200), (1027, 32))
COLSUM_SCALAR = ((1, 1), (5, 21), (1000, 81), (257, 63))


def colsum_input(m, n, extra=0):
    """[m, n + extra] fp32 with |x| in [0.5, 1.5] and a random sign: every row is at least
    1 / (3 m) of its column's sum |x|."""
    rng = np.random.default_rng([61, m, n, extra])
    return (rng.uniform(0.5, 1.5, (m, n + extra)) * rng.choice([-1.0, 1.0], (m, n + extra))
            ).astype(np.float32)


def colsum_chain(m, ld, n, byte_offset):
    """The longest serial chain of the kernel naws_colsum_f32 picks: the float4 kernel (N and ld
    multiples of 4, a 16-byte aligned base) gives each of 32 row lanes ceil(m / 32) rows, the
    scalar one each of 4 row lanes ceil(m / 4)."""
    f4 = n % 4 == 0 and ld % 4 == 0 and byte_offset % 16 == 0
    return (-(-m // 32) if f4 else -(-m // 4)), f4


WCE_SHAPES = ((3, 21), (5, 81))


def wce_inputs(n, c, nprob=3):
    """x, l, w [nprob, N, C], dy [nprob]: the edge probabilities 0, 1, 1e-30, 0.9999999 of the
    existing tests; x = 1 with label 0 is the gradient the 1e4 cap cuts (1 / 1e-20)."""
    rng = np.random.default_rng([71, n, c])
    x = rng.uniform(0, 1, (nprob, n, c)).astype(np.float32)
    x[0, 0, :4] = [0.0, 1.0, 1e-30, 0.9999999]
    x[1, n - 1, c - 1] = 1.0
    l = (rng.uniform(0, 1, (nprob, n, c)) > 0.8).astype(np.float32)
    l[1, 0, 2] = 0.37
    l[0, 0, 1] = 0.0
    l[1, n - 1, c - 1] = 0.0
    l[0, 0, 2] = 1.0
    w = rng.uniform(0, 1, (nprob, n, c)).astype(np.float32)
    dy = np.array([1.0, 0.5, 2.0], np.float32)[:nprob]
    return x, l, w, dy


LAUNCH_CAP = 2048 * 256                       # grid_for: lanes of the largest elementwise launch
UNARY_OPS = ('LOG', 'SCALE', 'REPLACE_NAN', 'LEAKY_RELU', 'CLIP', 'RELU')     # lib.UN_*
UNARY_ARGS = {'LOG': (0.0, 0.0), 'SCALE': (-1.7, 0.0), 'REPLACE_NAN': (0.25, 0.0),
              'LEAKY_RELU': (0.01, 0.0), 'CLIP': (-0.5, 1.0), 'RELU': (0.0, 0.0)}
BINARY_OPS = ('ADD', 'SUB', 'MUL', 'DIV', 'GATE_POS')                         # lib.BIN_*
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -3e-42], np.float32)
BINARY_SHAPES = (((129, 4099), (129, 4099)),   # past the launch cap, odd cols
                 ((129, 65), (129, 1)),        # column broadcast of B
                 ((1, 65), (129, 1)),          # row x column outer form
                 ((1, 1), (129, 65)))          # scalar A


def unary_input(n):
    """n values in (-2, 2); from 6 elements up the six SPECIALS sit at the head, on both sides of
    the launch cap (when n reaches it) and at the tail."""
    rng = np.random.default_rng([81, n])
    x = rng.uniform(-2, 2, n).astype(np.float32)
    k = len(SPECIALS)
    if n >= k:
        x[:k] = SPECIALS
        x[n - k:] = SPECIALS[::-1]
    if n >= LAUNCH_CAP + k:
        x[LAUNCH_CAP - k:LAUNCH_CAP] = SPECIALS[::-1]
        x[LAUNCH_CAP:LAUNCH_CAP + k] = SPECIALS
    return x


def unary_ref(name, x, a, b):
    """fp32 for the one-operation ops (bit-comparable), float64 for LOG.  RELU is Caffe2's
    `x > 0 ? x : 0` (NaN -> 0; the sign of a zero result is not part of the statement)."""
    x = np.asarray(x, np.float32)
    a, b = np.float32(a), np.float32(b)
    with np.errstate(all='ignore'):
        if name == 'LOG':
            return np.log(x.astype(np.float64))
        if name == 'SCALE':
            return x * a
        if name == 'REPLACE_NAN':
            return np.where(np.isnan(x), a, x)
        if name == 'LEAKY_RELU':
            return np.where(x >= 0, x, a * x)
        if name == 'CLIP':
            y = np.where(x < a, a, x)
            return np.where(y > b, b, y)
        assert name == 'RELU'
        return np.where(x > 0, x, np.float32(0))


def dropout_mask_ref(seed, ratio, n):
    """The counter-based keep decision of csrc/naws_common.h (naws_hash_u32 / naws_keep): one
    64-bit mix of (seed, index), keep <=> its top 24 bits >= ratio 2^24.  -> fp32 0 / 1 [n]."""
    with np.errstate(over='ignore'):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.arange(n, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    thr = np.uint64(min(max(float(np.float32(ratio)) * 16777216.0, 0.0), 16777216.0))
    return ((z >> np.uint64(40)) >= thr).astype(np.float32)


def binary_inputs(sa, sb):
    rng = np.random.default_rng([91, sa[0], sa[1], sb[0], sb[1]])
    a = rng.standard_normal(sa).astype(np.float32)
    b = rng.standard_normal(sb).astype(np.float32)
    b.reshape(-1)[3::7] = 0.0                   # x / 0 and the edge of GATE_POS's `b > 0`
    a.reshape(-1)[3::21] = 0.0                  # 0 / 0
    return a, b


def binary_ref(name, a, b, column0=False):
    """numpy broadcasting of [ra, ca] with [rb, cb] in fp32.  column0: WRONG on purpose - a
    column-broadcast that reads column 0 of an operand that has a column per output column."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    shape = (max(a.shape[0], b.shape[0]), max(a.shape[1], b.shape[1]))
    if column0:
        a, b = a[:, :1], b[:, :1]
    with np.errstate(all='ignore'):
        if name == 'ADD':
            y = a + b
        elif name == 'SUB':
            y = a - b
        elif name == 'MUL':
            y = a * b
        elif name == 'DIV':
            y = a / b
        else:
            assert name == 'GATE_POS'
            y = np.where(b > 0, a, np.float32(0))
    return np.ascontiguousarray(np.broadcast_to(y, shape), np.float32)


# ----------------------------------------------------------------------------- comparisons ----
def _note(family, value):
    """One `tail-edge <family> <figure>` line per comparison (pytest -s shows them): where the
    measured-error table of tests/test_gpu_tail_edges.py comes from."""
    print('tail-edge %-28s %.3e' % (family, float(value)))


def _f64(a):
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


def check_prob(got, ref, family='prob'):
    """Probabilities (softmax outputs, rois_pred, cls_prob): finite, <= 1e-5 of the output's
    maximum, <= 1e-4 relative on every entry whose reference exceeds 1e-30."""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), '%s: %d non-finite entries' % (family, (~np.isfinite(got)).sum())
    err = np.abs(got - ref)
    e_max = err.max() / np.abs(ref).max()
    big = ref > 1e-30
    e_rel = (err[big] / ref[big]).max() if big.any() else 0.0
    _note(family + ' /max', e_max)
    _note(family + ' rel', e_rel)
    assert e_max <= 1e-5, (family, e_max)
    assert e_rel <= 1e-4, (family, e_rel)


def check_of_max(got, ref, bound, family):
    """max |got - ref| <= bound * max |ref|, both finite."""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), '%s: non-finite entries' % family
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    e = err / scale if scale > 0 else (0.0 if err == 0 else np.inf)
    _note(family, e)
    assert e <= bound, (family, e)


def check_grad(got, ref, family='wsddn grad'):
    """WSDDN / softmax gradients: <= 2e-5 of max |reference| per output."""
    check_of_max(got, ref, 2e-5, family)


def check_wsddn_grads(got4, ref4, lens, ad, g, family='wsddn grad'):
    """d_fc8c, d_fc8d, d_noisy_fc8c, d_noisy_fc8d (the noisy pair None for one branch) against
    wsddn_backward_ref; C = 1 against zero (wsddn_one_class_bound)."""
    assert np.all([np.isfinite(_f64(o)).all() for o in got4 if o is not None]), family
    if ad.shape[2] > 1:
        for o, r in zip(got4, ref4):
            if r is not None:
                check_grad(o, r, family)
        return
    bound = wsddn_one_class_bound(lens, ad, g)
    for k, o in enumerate(got4):
        if ref4[k] is None:
            continue
        o, bd = _f64(o), bound[k]
        assert (np.abs(o) <= bd).all(), (family, 'C = 1', k, float(np.abs(o).max()))
        if (bd > 0).any():
            _note(family + ' C=1 /bound', (np.abs(o)[bd > 0] / bd[bd > 0]).max())


def check_softmax_grad(got, y, dy, family='softmax grad', of_max=False):
    """dX = y (dy - d), d = sum_c y dy, from the given fp32 y and dy, against float64.  Where the
    row is nearly one-hot (logit scale 30) dy - d cancels and every entry of dX is small against
    its operands, so a fraction of max |dX| would be a fraction of the rounding itself.  Per entry:
    |error| <= 2^-24 y (3 (|dy| + |d|) + (cols + 2) sum_c |y dy|): three roundings on the entry's
    own product and difference, and the worst case of an fp32 sum of cols products (plus one step
    of the fp32 denormal grid, 2^-149, where y itself is denormal).  of_max (logit scale 1, where
    the rows are not one-hot and max |dX| is a scale): also <= 2e-5 of max |reference|."""
    got, y, dy = _f64(got), _f64(y), _f64(dy)
    assert np.isfinite(got).all(), family
    d = (y * dy).sum(1, keepdims=True)
    bound = F32_EPS * y * (3 * (np.abs(dy) + np.abs(d)) +
                           (y.shape[1] + 2) * np.abs(y * dy).sum(1, keepdims=True)) + 2.0 ** -149
    err = np.abs(got - y * (dy - d))
    assert (err <= bound).all(), (family, float((err[bound > 0] / bound[bound > 0]).max()))
    _note(family + ' /bound', (err[bound > 0] / bound[bound > 0]).max())
    if of_max:
        check_grad(got, y * (dy - d), family + ' /max')


def check_gemm(got, ref, family='gemm wrapper'):
    check_of_max(got, ref, 5e-6, family)


GATE_OUTPUTS = ('class_weight', 'class_weight_noise', 'hatE_sum', 'hatE_sum_norm')


def check_gate(got, ref, family='gate'):
    """One gate output [nseg, C]: NaN exactly where the reference is NaN, and per image <= 2e-5 of
    the output's maximum elsewhere."""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape and ref.ndim == 2, (got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (family, np.argwhere(np.isnan(got) != nan)[:8])
    for s in range(ref.shape[0]):
        ok = ~nan[s]
        if not ok.any():
            continue
        g, r = got[s][ok], ref[s][ok]
        assert np.isfinite(g).all(), (family, s)
        scale = np.abs(r).max()
        err = np.abs(g - r).max()
        e = err / scale if scale > 0 else (0.0 if err == 0 else np.inf)
        _note(family, e)
        assert e <= 2e-5, (family, s, e)


def check_gate4(got4, ref4, family='gate'):
    for k, name in enumerate(GATE_OUTPUTS):
        check_gate(got4[k], ref4[k], family)


def check_colsum(got, ref, abs_sum, chain, family='colsum'):
    """Per column |error| <= (L + 8) 2^-24 sum_r |x[r, c]| with L the longest serial chain."""
    got, ref, abs_sum = _f64(got).reshape(-1), _f64(ref).reshape(-1), _f64(abs_sum).reshape(-1)
    assert got.shape == ref.shape
    assert np.isfinite(got).all()
    e = (np.abs(got - ref) / ((chain + 8) * F32_EPS * abs_sum)).max()
    _note(family + ' /bound', e)
    assert e <= 1.0, (family, e)


def check_exact(got, ref, family='exact', zero_sign=True):
    """Bit for bit (the sign of zero included unless zero_sign is False); NaN where and only where
    the reference has one."""
    if hasattr(got, 'detach'):
        got = got.detach().cpu().numpy()
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), family
    same = (got.view(np.int32) == ref.view(np.int32)) | nan
    if not zero_sign:
        same |= (got == 0) & (ref == 0)
    assert same.all(), (family, int((~same).sum()), np.argwhere(~same)[:8])


def check_ulp(got, ref64, ulps, family):
    """|got - ref| <= ulps fp32 ulps of the reference; inf, NaN where the reference has them."""
    if hasattr(got, 'detach'):
        got = got.detach().cpu().numpy()
    got = np.atleast_1d(np.asarray(got, np.float32))
    ref64 = np.atleast_1d(np.asarray(ref64, np.float64))
    r32 = ref64.astype(np.float32)
    fin = np.isfinite(r32)
    assert np.array_equal(np.isnan(got), np.isnan(r32)), family
    assert np.array_equal(got[~fin & ~np.isnan(r32)], r32[~fin & ~np.isnan(r32)]), family
    assert np.isfinite(got[fin]).all(), family
    ulp = np.spacing(np.abs(r32[fin])).astype(np.float64)
    e = (np.abs(got[fin].astype(np.float64) - ref64[fin]) / ulp).max() if fin.any() else 0.0
    _note(family + ' ulp', e)
    assert e <= ulps, (family, e)


def check_wce(got, ref, bound, family='wce'):
    """Against float64: |error| <= bound (N C 2^-24 sum |terms| for the loss)."""
    got, ref, bound = _f64(got), _f64(ref), _f64(bound)
    assert np.isfinite(got).all(), family
    with np.errstate(all='ignore'):
        e = np.where(bound > 0, np.abs(got - ref) / bound, np.where(got == ref, 0.0, np.inf)).max()
    _note(family + ' /bound', e)
    assert e <= 1.0, (family, e)
