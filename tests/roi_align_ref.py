"""Float64 references of RoIAlign / RoIAlignGradient as include/naws.h (a-2b) states them, shared by
tests/test_roi_align.py and tests/test_gpu_roi_align.py:

  axis_samples / roi_geometry   the geometry in numpy float32, every operation rounded on its own:
                                per axis sample (valid, lo, hi, l) and the float32 coordinate y
  forward64 / backward64        the literal restatement, values in float64 from the float32 l
                                (h = 1 - l exact in float64), sample by sample and tap by tap; with
                                every element the number of reference terms and the sum of their
                                absolute values, which the GPU bounds are made of
  forward_grid / backward_grid  a second, independent formulation: torch grid_sample (bilinear,
                                border padding, align_corners) in float64 at the same float32
                                coordinates, masked by validity, summed per bin; backward by autograd
  VARIANTS                      five deliberately wrong restatements of the geometry
  CASE_ROIS / EXTRA_ROIS ...    the case list of both suites
  graph64                       a recorded graph that pools with RoIAlign in torch double, as
                                body_grad_ref.graph_grads64 restates the RoIPoolF graphs
"""
import numpy as np
import torch
import torch.nn.functional as F

import body_grad_ref as bref

f32 = np.float32
MAX_GRID = 1024

# (batch, x1, y1, x2, y2) on a 13 x 17 map, N = 2, spatial_scale 0.125
CASE_ROIS = [
    ('interior', (0, 8, 16, 90, 70)),
    ('whole_map', (1, 0, 0, 135, 103)),
    ('outside_low', (0, -30, -20, 40, 50)),
    ('outside_high', (1, 100, 60, 180, 140)),
    ('sub_pixel', (0, 33.3, 21.7, 35.1, 22.2)),
    ('integer_aligned', (1, 16, 8, 72, 64)),
    ('reversed', (0, 120, 90, 100, 80)),
    ('wholly_outside', (0, 300, 300, 400, 400)),
    ('overhang_one', (1, -9, -9, 136, 104)),
    ('last_row_col', (0, 128, 96, 136, 104)),
]
# each its own case; the whole roi is invalid (Y = 0, no gradient) in all four
INVALID_ROIS = [
    ('batch_2', (2, 8, 16, 90, 70)),
    ('batch_minus_1', (-1, 8, 16, 90, 70)),
    ('nan_coordinate', (0, 8, float('nan'), 90, 70)),
    ('cap_1024', (0, -500000, 16, 500000, 70)),          # 1e6 image pixels wide: adaptive gw > 1024
]
MAP_H, MAP_W, MAP_N = 13, 17, 2
POOLINGS = [(7, 7), (1, 1), (3, 5)]
SAMPLINGS = [0, 1, 2, 3]
VARIANTS = ('aligned', 'rounded', 'no_max', 'clamp', 'floor')


def case_rois():
    return np.array([r for _, r in CASE_ROIS], f32)


def rois_many(count, seed=5):
    """`count` rois over the 13 x 17 map at scale 0.125, some reaching outside."""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(-20, 120, count)
    y1 = rng.uniform(-20, 90, count)
    w = rng.uniform(0.5, 90, count)
    h = rng.uniform(0.5, 70, count)
    b = rng.integers(0, MAP_N, count)
    return np.stack([b, x1, y1, x1 + w, y1 + h], 1).astype(f32)


# ------------------------------------------------------------------------------- geometry ----
def axis_samples(start, bin_, g, bins, L, variant=None):
    """Samples (p, i), p < bins, i < g, of one axis of length L -> dict of [bins, g] arrays:
    y (float32, before clamping), valid, lo, hi, l (float32)."""
    with np.errstate(all='ignore'):
        p = np.arange(bins, dtype=f32)[:, None]
        i = np.arange(g, dtype=f32)[None, :]
        y = (start + p * bin_) + ((i + f32(0.5)) * bin_) / f32(g)          # float32 throughout
        assert y.dtype == f32
        valid = (y >= f32(-1.0)) & (y <= f32(L))
        if variant == 'clamp':
            valid = np.isfinite(y)
            y = np.clip(y, f32(0), f32(L))
        yc = np.where(valid, y, f32(0))
        yc = np.where(yc <= 0, f32(0), yc)
        lo = yc.astype(np.int64)
        edge = lo >= L - 1
        lo = np.where(edge, L - 1, lo)
        hi = np.where(edge, L - 1, lo + 1)
        yc = np.where(edge, lo.astype(f32), yc)
        l = (yc - lo.astype(f32)).astype(f32)
    return dict(y=y, valid=valid, lo=lo, hi=hi, l=l)


def roi_geometry(roi, ph, pw, scale, sampling, N, H, W, variant=None):
    """None for a roi that is invalid as a whole, else dict(b, gh, gw, rows, cols)."""
    with np.errstate(all='ignore'):
        roi = np.asarray(roi, f32)
        s = f32(scale)
        bf = roi[0]
        if not (bf > -1 and bf < N):
            return None
        xs, ys, xe, ye = roi[1] * s, roi[2] * s, roi[3] * s, roi[4] * s
        if variant == 'rounded':
            xs, ys, xe, ye = (f32(np.round(v)) for v in (xs, ys, xe, ye))
        if variant == 'aligned':
            xs, ys, xe, ye = (v - f32(0.5) for v in (xs, ys, xe, ye))
        if not all(np.isfinite(v) for v in (xs, ys, xe, ye)):
            return None
        rw, rh = xe - xs, ye - ys
        if variant != 'no_max':
            rw, rh = max(rw, f32(1.0)), max(rh, f32(1.0))
        bw, bh = f32(rw / f32(pw)), f32(rh / f32(ph))
        if sampling > 0:
            gh = gw = int(sampling)
        else:
            rnd = np.floor if variant == 'floor' else np.ceil
            gwf, ghf = rnd(f32(rw / f32(pw))), rnd(f32(rh / f32(ph)))
            if not (gwf <= MAX_GRID and ghf <= MAX_GRID):
                return None
            gw, gh = max(int(gwf), 1), max(int(ghf), 1)       # (floor / no_max can give 0 or less)
        return dict(b=int(bf), gh=gh, gw=gw,
                    rows=axis_samples(ys, bh, gh, ph, H, variant),
                    cols=axis_samples(xs, bw, gw, pw, W, variant))


def _taps(ax, p):
    """The valid samples of bin p as (pixel index [k,2], weight float64 [k,2]): lo then hi."""
    v = ax['valid'][p]
    l = ax['l'][p][v].astype(np.float64)
    return (np.stack([ax['lo'][p][v], ax['hi'][p][v]], 1), np.stack([1.0 - l, l], 1))


# ------------------------------------------------------------------- literal restatement ----
def forward64(x, rois, ph, pw, scale, sampling, variant=None):
    """x [N,C,H,W], rois [R,5] -> (Y float64 [R,C,ph,pw], n [R,1,ph,pw] the number of reference
    terms of an element, S [R,C,ph,pw] the sum of their absolute values)."""
    x = np.asarray(x, np.float64)
    N, C, H, W = x.shape
    R = len(rois)
    y = np.zeros((R, C, ph, pw))
    n = np.zeros((R, 1, ph, pw))
    S = np.zeros((R, C, ph, pw))
    for r in range(R):
        g = roi_geometry(rois[r], ph, pw, scale, sampling, N, H, W, variant)
        if g is None:
            continue
        xb = x[g['b']]
        count = float(g['gh'] * g['gw'])
        for p in range(ph):
            iy, wy = _taps(g['rows'], p)
            for q in range(pw):
                ix, wx = _taps(g['cols'], q)
                if not len(iy) or not len(ix):
                    continue
                # terms [C, ky, 2, kx, 2]: one per (sample pair, tap)
                t = xb[:, iy[:, :, None, None], ix[None, None, :, :]] * \
                    (wy[:, :, None, None] * wx[None, None, :, :])
                y[r, :, p, q] = t.sum(axis=(1, 2, 3, 4)) / count
                S[r, :, p, q] = np.abs(t).sum(axis=(1, 2, 3, 4)) / count
                n[r, 0, p, q] = 4 * len(iy) * len(ix)
    return y, n, S


def backward64(dy, rois, shape, scale, sampling, variant=None):
    """dy [R,C,ph,pw], shape (N,C,H,W) -> (dX float64, T [N,1,H,W] the number of terms
    dY * weight / (gh gw) an element sums, A [N,C,H,W] the sum of their absolute values)."""
    dy = np.asarray(dy, np.float64)
    N, C, H, W = shape
    R, _, ph, pw = dy.shape
    dx, A = np.zeros(shape), np.zeros(shape)
    T = np.zeros((N, 1, H, W))
    for r in range(R):
        g = roi_geometry(rois[r], ph, pw, scale, sampling, N, H, W, variant)
        if g is None:
            continue
        b, count = g['b'], float(g['gh'] * g['gw'])
        for p in range(ph):
            iy, wy = _taps(g['rows'], p)
            for q in range(pw):
                ix, wx = _taps(g['cols'], q)
                if not len(iy) or not len(ix):
                    continue
                wgt = (wy[:, :, None, None] * wx[None, None, :, :]) / count
                t = dy[r, :, p, q][:, None, None, None, None] * wgt[None]
                idx = (iy[:, :, None, None] * W + ix[None, None, :, :]).ravel()
                t = t.reshape(C, -1)
                np.add.at(dx[b].reshape(C, H * W), (slice(None), idx), t)        # (views of dx, A, T)
                np.add.at(A[b].reshape(C, H * W), (slice(None), idx), np.abs(t))
                np.add.at(T[b, 0].reshape(H * W), idx, 1.0)
    return dx, T, A


# ---------------------------------------------------------------- grid_sample formulation ----
def _grid_forward(xt, rois, ph, pw, scale, sampling, variant=None):
    N, C, H, W = xt.shape
    out = []
    for r in range(len(rois)):
        g = roi_geometry(rois[r], ph, pw, scale, sampling, N, H, W, variant)
        if g is None:
            out.append(torch.zeros((C, ph, pw), dtype=torch.float64))
            continue
        gh, gw = g['gh'], g['gw']
        vy = g['rows']['valid'].reshape(-1)
        vx = g['cols']['valid'].reshape(-1)
        ys = np.where(vy, g['rows']['y'].reshape(-1), 0).astype(np.float64)     # [ph*gh]
        xs = np.where(vx, g['cols']['y'].reshape(-1), 0).astype(np.float64)     # [pw*gw]
        gy = torch.from_numpy(2.0 * ys / (H - 1) - 1.0)
        gx = torch.from_numpy(2.0 * xs / (W - 1) - 1.0)
        grid = torch.stack([gx[None, :].expand(len(gy), -1), gy[:, None].expand(-1, len(gx))], -1)
        v = F.grid_sample(xt[g['b']:g['b'] + 1], grid[None], mode='bilinear', padding_mode='border',
                          align_corners=True)[0]                                  # [C, ph*gh, pw*gw]
        mask = torch.from_numpy(np.outer(vy, vx).astype(np.float64))
        v = (v * mask).view(C, ph, gh, pw, gw).sum(dim=(2, 4)) / float(gh * gw)
        out.append(v)
    if not out:
        return torch.zeros((0, C, ph, pw), dtype=torch.float64)
    return torch.stack(out)


def forward_grid(x, rois, ph, pw, scale, sampling, variant=None):
    return _grid_forward(torch.tensor(np.asarray(x, np.float64)), rois, ph, pw, scale, sampling,
                         variant).numpy()


def backward_grid(dy, rois, shape, scale, sampling, variant=None):
    xt = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    dy = torch.tensor(np.asarray(dy, np.float64))
    y = _grid_forward(xt, rois, dy.shape[2], dy.shape[3], scale, sampling, variant)
    if y.numel() == 0 or not y.requires_grad:
        return np.zeros(shape)
    (y * dy).sum().backward()
    return xt.grad.numpy()


# ------------------------------------------------------------------------------------ graph ----
def graph64(model, params, fed, snapshots):
    """A recorded DetectionModelHelper graph that pools with RoIAlign, restated in torch CPU double
    the way body_grad_ref.graph_grads64 restates the RoIPoolF graphs (same rules: ReLU masks and
    max-pool selections come from the GPU forward as constants, ops behind StopGradient or that
    op_table.cuts_flow contribute their GPU output, SoftmaxWithLossN by the surrogate whose autograd
    is the reference gradient op), with two differences: RoIAlign is restated in the grid_sample
    form - it has no discrete choice - and the float64 blobs are returned too, so that forward
    values can be compared; a test-mode model (no losses) gets no backward.
    -> ({param: float64 gradient}, {FC bias: max_c sum_r |dY[r,c]|}, {blob: float64 tensor})."""
    from detectron.core.op_table import cuts_flow, grad_inputs
    _d = bref._d
    env = {k: _d(torch.as_tensor(v)) for k, v in fed.items()}
    leaves = {}
    for n in model.params:
        leaves[n] = params[n].detach().cpu().double().clone().requires_grad_(True)
        env[n] = leaves[n]
    prev = {}
    fc_out = []
    for op, outs_gpu in zip(model.net.ops, snapshots):
        t, a = op.type, op.args
        x = [env.get(n) for n in op.inputs]
        if t == 'StopGradient':
            res = [x[0].detach()]
        elif t == 'Split':              # (test mode: cls_prob = [first foreground column | rois_pred])
            res = list(torch.split(x[0], a['split'], dim=a.get('axis', 1)))
        elif t == 'Concat':
            res = [torch.cat(x, dim=a.get('axis', 1)), None]
        elif cuts_flow(t) or grad_inputs(t) is None:
            res = [_d(v) for v in outs_gpu]
        elif t == 'Conv':
            res = [F.conv2d(x[0], x[1], x[2], stride=1, padding=a.get('pad', 1),
                            dilation=a.get('dilation', 1))]
        elif t == 'Relu':
            res = [x[0] * (_d(outs_gpu[0]) > 0).double()]
        elif t == 'MaxPool':
            s = a['stride']
            xin = prev[op.inputs[0]].detach().cpu().numpy().transpose(0, 2, 3, 1)
            y32, k = bref.maxpool_select(xin, s)
            assert np.array_equal(y32, outs_gpu[0].cpu().numpy().transpose(0, 2, 3, 1))
            n, c, h, w = x[0].shape
            ho, wo = k.shape[1:3]
            win = F.unfold(x[0], kernel_size=2, stride=s).view(n, c, 4, ho * wo)
            kk = torch.from_numpy(k.transpose(0, 3, 1, 2).reshape(n, c, 1, ho * wo))
            res = [torch.gather(win, 2, kk).view(n, c, ho, wo)]
        elif t == 'RoIAlign':
            assert len(op.outputs) == 1
            res = [_grid_forward(x[0], x[1].numpy().astype(f32), a['pooled_h'], a['pooled_w'],
                                 a['spatial_scale'], a.get('sampling_ratio', 0))]
        elif t == 'RoIFeatureBoost':
            res = [x[0] * x[1].reshape(-1, 1, 1, 1)]
        elif t == 'FC':
            res = [F.linear(x[0].flatten(1), x[1], x[2])]
            if res[0].requires_grad:
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
            lo, hi = float(p.detach().min()), float(p.detach().max())
            assert lo > 1e-12 and 1.0 - hi > 1e-3, (lo, hi)   # far from the op's clamp and cap
            term = l * torch.log(p) + (1 - l) * torch.log(1 - p)
            if t.startswith('Weighted'):
                term = term * x[2]
            res = [-term.sum() / (p.shape[1] if a.get('is_mean', False) else 1.0) / p.shape[0]]
        else:
            raise NotImplementedError('no float64 restatement of ' + t)
        for n, v, g in zip(op.outputs, res, outs_gpu):
            env[n] = v
            prev[n] = g
    if not model.train or not model.losses:
        return {}, {}, env
    total = 0.0
    for loss in model.losses:
        total = total + env[loss].reshape(()) * float(_d(env[loss + '_grad']).reshape(-1)[0])
    total.backward()
    terms = {}
    for b, y in fc_out:
        if y.grad is not None:
            terms[b] = terms.get(b, 0.0) + float(y.grad.abs().sum(0).max())
    return {n: leaves[n].grad.numpy() for n in model.param_to_grad}, terms, env
