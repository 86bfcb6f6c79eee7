"""RoIPoolF off the 7x7, 1/8 geometry: the case lists of tests/test_gpu_roi_pool_geometry.py and a
numpy restatement of the operator's integer geometry (a helper module, imported by the CPU test
test_roi_geometry_cases.py and by the GPU tests; it needs neither a GPU nor the library).

The restatement follows RoIPoolF's definition (the reference's ROIPoolForward, restated in the
comment of csrc/roi_ops.hip): every roi coordinate is multiplied by spatial_scale IN FP32 and
rounded half away from zero (C's roundf); the extents are max(end - start + 1, 1); bin p of P over
an extent e covers [floor(p * e/P), ceil((p + 1) * e/P)) in fp32, moved by the roi's start and
clipped to [0, limit].  A window is what one bin covers: [hs, he) x [ws, we).

The hierarchical kernel sorts windows by dmin = min(he - hs, we - ws): 1 -> the pixel loop,
2..3 -> the 2x2 block-maxima map (M2), >= 4 -> the 4x4 map (M4).  Its loops step by 2 * L (L = 2 or
4) with the last block clamped back inside the window, so how they end depends on the sides modulo
2 * L: 12 residue classes (dh mod 4, dw mod 4) can occur in the M2 class ((0|1, 0|1) cannot: a
side of 2 or 3 is 2 or 3 modulo 4) and all 64 classes (dh mod 8, dw mod 8) in the M4 class."""
import numpy as np

from helpers import make_rois

# (pooled_h, pooled_w, spatial_scale)
GEOMETRIES = [
    (1, 1, 1 / 8), (2, 2, 1 / 16),       # fewer (bin row, bin group) steps than waves per roi
    (3, 5, 1 / 8), (5, 3, 1 / 16),       # odd PH*PW; PW = 5: two bin groups, one live quarter-wave
    (6, 6, 1 / 8), (7, 7, 1 / 16),
    (4, 9, 1 / 8),                       # three bin groups
    (1, 41, 1 / 8),                      # eleven bin groups; a bin row past the float4 kernel's LDS
    (8, 10, 1 / 8),                      # 80 bins: the general kernel's argmax tile is exactly 160 KB
    (12, 12, 1 / 16),                    # 144 bins: > 64 KB of LDS for two rois; no argmax tile
    (10, 16, 1 / 16),                    # 160 bins: the general kernel's tile is exactly 160 KB
    (14, 14, 1 / 8),                     # the configuration default; past every staged tile
    (16, 16, 1 / 8),                     # the largest PH*PW the fast entries accept
    (16, 17, 1 / 8),                     # one past it
]
FAST_LIMIT = 256                          # PH*PW the plane / slab / hierarchical entries accept
MAP_H, MAP_W = 20, 30                     # the feature map of the sweeps and the random set
SMALL_H, SMALL_W = 5, 7                   # the map on which every bin of a large grid is <= 1 pixel


def roundf(x):
    """C's roundf on fp32 values: half away from zero, as int64 (x - trunc(x) is exact)."""
    x = np.asarray(x, np.float32)
    t = np.trunc(x)
    return (t + np.sign(x) * (np.abs(x - t) >= np.float32(0.5))).astype(np.int64)


def scaled(rois, scale):
    """The four coordinates times spatial_scale, the product rounded to fp32."""
    return np.asarray(rois, np.float32)[:, 1:5] * np.float32(scale)


def roi_frame(rois, scale, rounding=roundf):
    """-> (batch, start_w, start_h, roi_w, roi_h), int64 [R] each."""
    q = rounding(scaled(rois, scale))
    sw, sh, ew, eh = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return (np.asarray(rois)[:, 0].astype(np.int64), sw, sh,
            np.maximum(ew - sw + 1, 1), np.maximum(eh - sh + 1, 1))


def bin_range(extent, start, pooled, limit):
    """-> (lo, hi) int64 [R, pooled]: bin p covers [lo, hi) of [0, limit)."""
    size = extent.astype(np.float32) / np.float32(pooled)                     # fp32 quotient
    p = np.arange(pooled, dtype=np.float32)[None, :]
    s = np.floor(p * size[:, None]).astype(np.int64)                          # fp32 products
    e = np.ceil((p + np.float32(1)) * size[:, None]).astype(np.int64)
    lo = np.minimum(np.maximum(s + start[:, None], 0), limit)
    hi = np.minimum(np.maximum(e + start[:, None], 0), limit)
    return lo, hi


def windows(rois, H, W, PH, PW, scale, rounding=roundf):
    """-> (batch [R], hs, he [R, PH], ws, we [R, PW])."""
    b, sw, sh, rw, rh = roi_frame(rois, scale, rounding)
    hs, he = bin_range(rh, sh, PH, H)
    ws, we = bin_range(rw, sw, PW, W)
    return b, hs, he, ws, we


def census(rois, H, W, PH, PW, scale):
    """What a roi list exercises at one geometry (see the module docstring for the classes)."""
    _, hs, he, ws, we = windows(rois, H, W, PH, PW, scale)
    dh = np.broadcast_to((he - hs)[:, :, None], (len(rois), PH, PW)).ravel()
    dw = np.broadcast_to((we - ws)[:, None, :], (len(rois), PH, PW)).ravel()
    empty = (dh <= 0) | (dw <= 0)
    dmin = np.minimum(dh, dw)
    m2 = ~empty & (dmin >= 2) & (dmin <= 3)
    m4 = ~empty & (dmin >= 4)
    s = scaled(rois, scale)
    tie = np.abs(s - np.trunc(s)) == np.float32(0.5)
    return {
        'windows': int(dh.size),
        'empty': int(empty.sum()),
        'dmin1': int((~empty & (dmin == 1)).sum()),
        'm2': int(m2.sum()),
        'm4': int(m4.sum()),
        'side9': int((~empty & (np.maximum(dh, dw) >= 9)).sum()),
        'm2_residues': set(zip((dh[m2] % 4).tolist(), (dw[m2] % 4).tolist())),
        'm4_residues': set(zip((dh[m4] % 8).tolist(), (dw[m4] % 8).tolist())),
        'ties_pos': int((tie & (s > 0)).sum()),
        'ties_neg': int((tie & (s < 0)).sum()),
    }


M2_RESIDUES = {(a, b) for a in range(4) for b in range(4) if a >= 2 or b >= 2}     # 12
M4_RESIDUES = {(a, b) for a in range(8) for b in range(8)}                         # 64
SWEEP_SIDES = range(1, 18)


def _sweep(H, W, scale, place):
    step = np.float32(1.0 / scale)
    assert float(step) * scale == 1.0 and step == np.round(step)      # a power of two: exact
    out = []
    for dh in SWEEP_SIDES:
        for dw in SWEEP_SIDES:
            i = len(out)
            x0, y0 = place(i, dh, dw)
            out.append([i % 2, x0 * step, y0 * step, (x0 + dw - 1) * step, (y0 + dh - 1) * step])
    return np.array(out, np.float32)


def window_sweep(H=MAP_H, W=MAP_W, scale=1 / 8):
    """One roi per (dh, dw) in 1..17 x 1..17 (289 rois, an odd count), its coordinates exact
    multiples of 1/scale so that the frame is exactly dh x dw, inside the map, at an offset that
    varies with (dh, dw); batch indices alternate.  Pooled 1x1 makes every window one roi."""
    return _sweep(H, W, scale,
                  lambda i, dh, dw: ((3 * dh + 5 * dw) % (W - dw + 1), (7 * dh + 2 * dw) % (H - dh + 1)))


def clipped_sweep(H=MAP_H, W=MAP_W, scale=1 / 8):
    """The same 289 frames, each hanging over one border of the map by half its size (left, right,
    top, bottom in turn; a side of 1 stays inside): the clipping of start and end is exercised on
    every side, and no window is empty."""
    def place(i, dh, dw):
        x0, y0 = (3 * dh + 5 * dw) % (W - dw + 1), (7 * dh + 2 * dw) % (H - dh + 1)
        side = i % 4
        if side == 0:
            x0 = -(dw // 2)
        elif side == 1:
            x0 = W - dw + dw // 2
        elif side == 2:
            y0 = -(dh // 2)
        else:
            y0 = H - dh + dh // 2
        return x0, y0
    return _sweep(H, W, scale, place)


def rounding_rois(scale):
    """Rois whose coordinates sit on .5 ties of both signs after scaling: with t = 1 / (2 scale),
    t, 5t, -t, -3t (8, 40, -8, -24 at 1/16; 4, 20, -4, -12 at 1/8) and larger odd multiples of t.
    Half away from zero and half to even differ on t (1 | 0), 5t (3 | 2), -t (-1 | 0), 9t (5 | 4),
    21t (11 | 10), 41t (21 | 20); they agree on -3t (-2) and 3t (2)."""
    t = 0.5 / scale
    rows = [
        (-1, -3, 5, 5), (-3, -1, 5, 9), (-1, -1, 1, 1), (-3, -3, 21, 5), (-1, 5, 41, 21),
        (1, -1, 5, 21), (5, -3, 41, 9), (-1, 1, 9, 29), (1, -3, 57, 37), (-3, 5, 21, 13),
        (9, -1, 13, 3),
    ]
    out = []
    for i, (a, b, c, d) in enumerate(rows):
        out.append([i % 2, a * t, b * t, c * t, d * t])
    out.sort(key=lambda r: r[0])                                   # grouped by image
    return np.array(out, np.float32)


def random_rois(H, W, scale, seed=7):
    """helpers.make_rois, 41 rois on each of two images, the last one dropped (R = 81, odd): the
    degenerate rows (1-px, malformed, outside, negative, whole image) included."""
    rng = np.random.default_rng(seed)
    return make_rois(rng, 2, 41, int(round(H / scale)), int(round(W / scale)))[:-1]


def features(c, H=MAP_H, W=MAP_W, seed=5, nan=True):
    """[2, c, H, W] standard-normal fp32 with one tied pair of pixels (the first index must win),
    one constant negative channel and - nan=True - one NaN pixel in image 0 (the strict '>' of the
    operator never lets a NaN win)."""
    rng = np.random.default_rng(seed + 1000 * c + H)
    x = rng.standard_normal((2, c, H, W)).astype(np.float32)
    x[:, :, H // 4, W // 4] = x[:, :, H // 4, W // 4 + 1]
    x[1, min(5, c - 1), :, :] = -3.0
    if nan:
        x[0, :, H // 2, W // 3] = np.nan
    return x


def boost_for(r, seed=3):
    """[r] fp32 in [1, 2)."""
    return (np.random.default_rng(seed).uniform(0, 1, r) + 1).astype(np.float32)


def pool_bruteforce(x, rois, PH, PW, scale, rounding=roundf):
    """RoIPoolF by definition over the restated windows: (y fp32, argmax int32) [R, C, PH, PW].
    Strict '>' from -FLT_MAX in h-major order: the first of equal maxima wins, a NaN never does;
    an empty window is (0, -1)."""
    n, c, H, W = x.shape
    b, hs, he, ws, we = windows(rois, H, W, PH, PW, scale, rounding)
    y = np.zeros((len(rois), c, PH, PW), np.float32)
    am = np.full((len(rois), c, PH, PW), -1, np.int32)
    fmax = np.finfo(np.float32).max
    for r in range(len(rois)):
        for ph in range(PH):
            for pw in range(PW):
                h0, h1, w0, w1 = hs[r, ph], he[r, ph], ws[r, pw], we[r, pw]
                if h1 <= h0 or w1 <= w0:
                    continue
                win = x[b[r], :, h0:h1, w0:w1].reshape(c, -1)
                win = np.where(win > -fmax, win, -np.inf)          # NaN and <= -FLT_MAX never win
                k = win.argmax(1)                                   # the first of equal maxima
                v = win[np.arange(c), k]
                won = v > -np.inf
                idx = (h0 + k // (w1 - w0)) * W + w0 + k % (w1 - w0)
                y[r, :, ph, pw] = np.where(won, v, -fmax)
                am[r, :, ph, pw] = np.where(won, idx, -1)
    return y, am
