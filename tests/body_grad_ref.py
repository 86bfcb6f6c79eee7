"""Float64 references of the trainable conv body's backward (torch CPU double / numpy), shared by
tests/test_gpu_body_backward.py, tests/test_gpu_body_backward_shapes.py and
tests/test_body_backward_plan.py:

  conv_grads / conv_grads_wrong   Conv(+bias) gradients through torch autograd, and three
                                  deliberately wrong statements that the tests' bound must reject
  WGRAD_CASES / wgrad_slices      the shapes that reach the weight gradient's split-K branches and
                                  the slice count behind a workspace size
  conv_case_int                   integer operands: every float32 sum exact, so the reference is
                                  the answer bit for bit
  maxpool_select / maxpool_grad32 the element naws_maxpool2x2_nhwc_fwd selects (first of a, b, d, e
                                  equal to the maximum) and the float32 gather that adds the windows
                                  in ascending index - bit for bit what the kernel computes
  pool_tie_input / tie_census     a feature map full of tied windows, and the count of them
  roi_pool_grad64                 float64 scatter through a given argmax, with the per-element
                                  number of contributions and sum of |terms| for the bound
  graph_grads64                   a recorded DetectionModelHelper graph restated in torch double:
                                  the parameter gradients of the sum of the seeded losses
"""
import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------ conv ----
def conv_grads(x, w, b, dy, dilation):
    """x [N,Cin,H,W], w [Cout,Cin,3,3], b [Cout], dy [N,Cout,H,W] -> dx, dw, db (float64)."""
    x = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    w = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
    b = torch.tensor(np.asarray(b, np.float64), requires_grad=True)
    y = F.conv2d(x, w, b, stride=1, padding=dilation, dilation=dilation)
    y.backward(torch.tensor(np.asarray(dy, np.float64)))
    return x.grad.numpy(), w.grad.numpy(), b.grad.numpy()


def conv_grads_wrong(kind, x, w, b, dy, dilation):
    """-> (dx, dw) of a WRONG backward:
    'no_flip'   the taps of the data gradient's weight not flipped (and dW's taps reversed)
    'dilation1' dilation 1 (pad 1) where `dilation` is meant
    'no_swap'   the OIHW buffer read as [Cin,Cout,3,3] without transposing (and dW written so)"""
    w = np.asarray(w, np.float64)
    cout, cin = w.shape[:2]
    if kind == 'dilation1':
        dx, dw, _ = conv_grads(x, w, b, dy, 1)
        return dx, dw
    dx, dw, _ = conv_grads(x, w, b, dy, dilation)
    dy_t = torch.tensor(np.asarray(dy, np.float64))
    if kind == 'no_flip':
        wp = torch.tensor(w.transpose(1, 0, 2, 3).copy())                    # [Cin,Cout,ky,kx]
        return (F.conv2d(dy_t, wp, None, padding=dilation, dilation=dilation).numpy(),
                dw[:, :, ::-1, ::-1].copy())
    if kind == 'no_swap':
        wp = torch.tensor(w.reshape(cin, cout, 3, 3)[:, :, ::-1, ::-1].copy())
        return (F.conv2d(dy_t, wp, None, padding=dilation, dilation=dilation).numpy(),
                dw.transpose(1, 0, 2, 3).copy().reshape(cout, cin, 3, 3))
    raise ValueError(kind)


# The shapes of tests/test_gpu_body_backward_shapes.py: (N, H, W, Cin, Cout, dilation) -> the number
# of K slices naws_conv3x3_nhwc_wgrad's plan takes there (tests/test_body_backward_plan.py holds the
# library to it, so a change of the plan cannot quietly turn these back into one-slice cases).
#   K = 1 (only the centre tap is non-zero) | H <= dilation | the smallest split, K = 518 / 556 (no
#   multiple of 32) | a 64 + 32 residue in M and in N, 2 x 3 tiles, two images | slices limited by
#   the tile count (8 x 8 tiles), the dgrad pack loops | the slice cap, the staging kernel loops,
#   dgrad in the 64 x 128 x 16 conv form
WGRAD_CASES = {
    (1, 1, 1, 32, 32, 1): 1, (1, 1, 1, 32, 32, 2): 1,
    (1, 2, 3, 32, 32, 2): 1,
    (1, 20, 24, 64, 64, 1): 2, (1, 20, 24, 64, 64, 2): 2,
    (2, 20, 24, 96, 160, 1): 4, (2, 20, 24, 96, 160, 2): 4,
    (2, 28, 30, 512, 512, 1): 6,
    (1, 100, 124, 512, 32, 1): 32,
}


def wgrad_slices(floats, case):
    """The K slices behind naws_conv3x3_nhwc_wgrad_workspace_floats(*case) = the two staged
    operands + the nine tap products + 3 partial planes per slice."""
    n, h, w, cin, cout, d = case
    rows = n * (h + 2 * d) * (w + 2 * d)
    ks, rest = divmod(floats - rows * (cin + cout) - 9 * cin * cout, 3 * cin * cout)
    assert rest == 0 and ks >= 1, (case, floats)
    return ks


def conv_case_int(case, seed, lo=-2, hi=2):
    """x [N,Cin,H,W], w [Cout,Cin,3,3], dy [N,Cout,H,W]: integers lo..hi stored as float32.  Every
    product and partial sum of the three gradients is then an integer below 2^24 (at most
    4 N (H+2d) (W+2d) <= 4 * 12,852 for dW, 4 * 9 * 512 for dX), so float32 adds are exact in ANY
    order and the float64 reference cast to float32 is the one right answer, bit for bit."""
    n, h, w, cin, cout, _ = case
    rng = np.random.default_rng(seed)
    draw = lambda *s: rng.integers(lo, hi + 1, s).astype(np.float32)
    return draw(n, cin, h, w), draw(cout, cin, 3, 3), draw(n, cout, h, w)


# --------------------------------------------------------------------------------- max-pool ----
def tie_census(x, stride):
    """-> (t [4], s [4]) over the windows of x [N,H,W,C]: t[j] = windows in which element j (a, b, d,
    e) equals the maximum together with at least one other element; s[j] = windows whose selected
    element (the first at the maximum) is j."""
    win = _windows(np.asarray(x, np.float32), stride)
    top = win == win.max(axis=3, keepdims=True)
    tied = top.sum(axis=3, keepdims=True) >= 2
    return ((top & tied).sum(axis=(0, 1, 2, 4)),
            np.bincount(np.argmax(top, axis=3).ravel(), minlength=4))


def pool_tie_input(shape, stride):
    """NHWC integers 0..3 as float32 (what a feature map looks like after ReLU: most windows tie)."""
    return np.random.default_rng(31 + stride).integers(0, 4, shape).astype(np.float32)


def _windows(x, stride):
    """x [N,H,W,C] -> [N,Ho,Wo,4,C] in the forward's order a = (y,x), b = (y,x+1), d, e."""
    n, h, w, c = x.shape
    ho, wo = (h - 2) // stride + 1, (w - 2) // stride + 1
    ys, xs = np.arange(ho) * stride, np.arange(wo) * stride
    return np.stack([x[:, ys + dy][:, :, xs + dx] for dy in (0, 1) for dx in (0, 1)], 3)


def maxpool_select(x, stride):
    """NHWC float32 -> (y [N,Ho,Wo,C], k [N,Ho,Wo,C]): the window maxima as the forward kernel
    takes them and the index 0..3 of the element it selects: the first equal to the maximum."""
    win = _windows(np.asarray(x, np.float32), stride)
    y = np.maximum(np.maximum(win[:, :, :, 0], win[:, :, :, 1]),
                   np.maximum(win[:, :, :, 2], win[:, :, :, 3]))
    k = np.argmax(win == y[:, :, :, None, :], axis=3)
    return y, k


def tie_free(x, stride):
    win = np.sort(_windows(np.asarray(x, np.float32), stride), axis=3)
    return bool((win[:, :, :, 1:] != win[:, :, :, :-1]).all())


def maxpool_grad32(x, dy, stride):
    """The kernel's gather restated: float32 dX [N,H,W,C], windows added in ascending index."""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    _, k = maxpool_select(x, stride)
    dx = np.zeros_like(x)
    n, ho, wo, c = dy.shape
    for yo in range(ho):
        for xo in range(wo):
            for j in range(4):
                m = k[:, yo, xo] == j
                t = dx[:, yo * stride + j // 2, xo * stride + j % 2]
                t[...] = np.where(m, t + dy[:, yo, xo], t).astype(np.float32)
    return dx


# ---------------------------------------------------------------------------------- RoIPoolF ----
def roi_pool_grad64(dy, argmax, rois, shape):
    """dy / argmax [R,C,ph,pw], rois [R,5], shape (N,C,H,W) -> (dx float64, count, abs_sum):
    dx[b,c,argmax] += dy; count / abs_sum = the number of terms and sum of |terms| per element."""
    n, c, h, w = shape
    dy = np.asarray(dy, np.float64)
    r = dy.shape[0]
    dx, cnt, asum = (np.zeros((n, c, h * w)) for _ in range(3))
    b = np.broadcast_to(rois[:, 0].astype(np.int64)[:, None, None, None], dy.shape)
    ch = np.broadcast_to(np.arange(c)[None, :, None, None], dy.shape)
    ok = argmax >= 0
    idx = (b[ok], ch[ok], argmax[ok].astype(np.int64))
    np.add.at(dx, idx, dy[ok])
    np.add.at(cnt, idx, 1.0)
    np.add.at(asum, idx, np.abs(dy[ok]))
    assert r == rois.shape[0]
    return dx.reshape(shape), cnt.reshape(shape), asum.reshape(shape)


# ------------------------------------------------------------------------------------ graph ----
def _d(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu()
        return v.double() if v.is_floating_point() else v
    return v


def graph_grads64(model, params, fed, snapshots):
    """The recorded graph of `model` (train mode, dropout disabled) in torch CPU double.

    params: {name: float32 tensor} the initial parameters; fed: the minibatch blobs; snapshots:
    [per forward op: the list of its outputs as the GPU run produced them].  Every op that takes
    part in the backward (op_table.grad_inputs) is restated; the discrete choices come from the
    GPU forward as constants - ReLU masks, the max-pool selections (derived from the GPU input /
    output by the kernel's rule), RoIPoolF's argmax - so a near-tie that falls differently in
    float32 cannot turn into an O(1) mismatch.  Every other op (the ones behind StopGradient or that
    op_table.cuts_flow: the entropy gate, RoILabel, Stat ...) contributes its GPU output as a
    constant.  SoftmaxWithLossN is restated by the surrogate whose autograd IS the reference
    gradient op (softmax_with_loss_n_op.cc:265-357 divides by the count of non-zero weights where
    the forward divides by their sum).
    -> ({param: float64 gradient} of sum(seed * loss), {FC bias: max_c sum_r |dY[r,c]|}): the second
    is the size of the terms an FC bias gradient sums - what its error scales with when the exact sum
    cancels (fc8d_b: the detection softmax runs over the rois, so a per-class bias moves nothing and
    its gradient is identically zero)."""
    from detectron.core.op_table import cuts_flow, grad_inputs
    env = {k: _d(torch.as_tensor(v)) for k, v in fed.items()}
    leaves = {}
    for n in model.params:
        leaves[n] = params[n].detach().cpu().double().clone().requires_grad_(True)
        env[n] = leaves[n]
    prev = {}                     # blob -> the GPU tensor an in-place op read (for the pool rule)
    fc_out = []                   # (bias name, FC output) for the bias-gradient term sizes
    for op, outs_gpu in zip(model.net.ops, snapshots):
        t, a = op.type, op.args
        x = [env.get(n) for n in op.inputs]
        if cuts_flow(t) or grad_inputs(t) is None:
            res = [_d(v) for v in outs_gpu]
        elif t == 'Conv':
            d = a.get('dilation', 1)
            res = [F.conv2d(x[0], x[1], x[2], stride=1, padding=a.get('pad', 1), dilation=d)]
        elif t == 'Relu':
            res = [x[0] * (_d(outs_gpu[0]) > 0).double()]
        elif t == 'MaxPool':
            s = a['stride']
            xin = prev[op.inputs[0]].detach().cpu().numpy().transpose(0, 2, 3, 1)
            y32, k = maxpool_select(xin, s)
            assert np.array_equal(y32, outs_gpu[0].cpu().numpy().transpose(0, 2, 3, 1))
            n, c, h, w = x[0].shape
            ho, wo = k.shape[1:3]
            win = F.unfold(x[0], kernel_size=2, stride=s).view(n, c, 4, ho * wo)
            kk = torch.from_numpy(k.transpose(0, 3, 1, 2).reshape(n, c, 1, ho * wo))
            res = [torch.gather(win, 2, kk).view(n, c, ho, wo)]
        elif t == 'RoIPoolF':
            am = outs_gpu[1].cpu().long()
            r, c = am.shape[:2]
            b = x[1][:, 0].long()
            planes = x[0].flatten(2)[b]                                  # [R,C,HW]
            y = torch.gather(planes, 2, am.clamp(min=0).view(r, c, -1)).view(am.shape)
            res = [y * (am >= 0).double(), am]
        elif t == 'RoIFeatureBoost':
            res = [x[0] * x[1].reshape(-1, 1, 1, 1)]
        elif t == 'FC':
            res = [F.linear(x[0].flatten(1), x[1], x[2])]
            res[0].retain_grad()
            fc_out.append((op.inputs[2], res[0]))
        elif t == 'Dropout':
            assert outs_gpu[1] is None, 'the restatement wants dropout disabled'
            res = [x[0], None]
        elif t == 'Softmax':
            res = [torch.softmax(x[0], dim=a.get('axis', 1))]
        elif t == 'Transpose':
            res = [x[0].t()]
        elif t in ('Mul', 'Add', 'Sub'):
            p, q = (v.reshape(1, -1) if v.dim() == 1 else v for v in x[:2])
            res = [p * q if t == 'Mul' else (p + q if t == 'Add' else p - q)]
        elif t == 'ReduceSum':
            res = [x[0].sum(0, keepdim=a.get('keepdims', True))]
        elif t == 'AveragedLoss':
            res = [x[0].mean()]
        elif t in ('WeightedCrossEntropyWithLogits', 'CrossEntropyWithLogits'):
            p, l = x[0], x[1]
            # far from the op's clamp (log arguments at 1e-20) and from its gradient cap (1e4,
            # reachable only through 1 / (1 - p)): plain autograd of the forward is the op pair
            lo, hi = float(p.detach().min()), float(p.detach().max())
            assert lo > 1e-12 and 1.0 - hi > 1e-3, (lo, hi)
            term = l * torch.log(p) + (1 - l) * torch.log(1 - p)
            if t.startswith('Weighted'):
                term = term * x[2]
            res = [-term.sum() / (p.shape[1] if a.get('is_mean', False) else 1.0) / p.shape[0]]
        elif t == 'SoftmaxWithLossN':
            lab = x[1].reshape(-1).long()
            w = x[2].reshape(-1) if len(x) > 2 and x[2] is not None else torch.ones(len(lab)).double()
            total = float((w > 1e-12).sum()) if len(x) > 2 else float(len(lab))
            logp = torch.log_softmax(x[0], dim=1)
            nll = -logp[torch.arange(len(lab)), lab]
            res = [torch.softmax(x[0], dim=1), a.get('scale', 1.0) * (w * nll).sum() / max(total, 1.0)]
        else:
            raise NotImplementedError('no float64 restatement of ' + t)
        for n, v, g in zip(op.outputs, res, outs_gpu):
            env[n] = v
            prev[n] = g
    total = 0.0
    for loss in model.losses:
        total = total + env[loss].reshape(()) * float(_d(env[loss + '_grad']).reshape(-1)[0])
    total.backward()
    terms = {}
    for b, y in fc_out:
        if y.grad is not None:
            terms[b] = terms.get(b, 0.0) + float(y.grad.abs().sum(0).max())
    return {n: leaves[n].grad.numpy() for n in model.param_to_grad}, terms
