"""numpy-float32 restatements of the two operators of the contextual WSDDN head (WSL.CONTEXT),
written from the arithmetic in include/naws.h: every operation is one float32 operation, so the
HIP kernels have to agree bit for bit."""
import numpy as np

F = np.float32


def roi_context(rois, max_h, max_w, ratio=1.8):
    """rois [R,5] -> (frame [R,9], context [R,9])."""
    r = np.ascontiguousarray(rois, F)
    ratio, two = F(ratio), F(2)
    b, x1, y1, x2, y2 = (r[:, i] for i in range(5))
    w, h = x2 - x1, y2 - y1
    iw, ih = w / ratio, h / ratio
    ow, oh = w * ratio, h * ratio
    ri_w, ri_h = w - iw, h - ih
    ro_w, ro_h = ow - w, oh - h
    hi_w, hi_h = ri_w / two, ri_h / two
    ho_w, ho_h = ro_w / two, ro_h / two

    def clamp(v, m):
        m = F(m)
        return np.where(v < 0, F(0), np.where(v > m, m, v)).astype(F)

    frame = np.stack([b, x1, y1, x2, y2, clamp(x1 + hi_w, max_w), clamp(y1 + hi_h, max_h),
                      clamp(x2 - hi_w, max_w), clamp(y2 - hi_h, max_h)], 1)
    context = np.stack([b, clamp(x1 - ho_w, max_w), clamp(y1 - ho_h, max_h),
                        clamp(x2 + ho_w, max_w), clamp(y2 + ho_h, max_h), x1, y1, x2, y2], 1)
    for a in (w, iw, ow, ri_w, ro_w, hi_w, ho_w, frame, context):
        assert a.dtype == F
    return np.ascontiguousarray(frame), np.ascontiguousarray(context)


def _roundf(v):
    """C roundf of float32 values (halves away from zero) -> int64."""
    v = np.asarray(v, F).astype(np.float64)          # exact; so is the sum below
    return np.trunc(v + np.copysign(0.5, v)).astype(np.int64)


def _bins(start, extent, pooled, limit):
    """[lo, hi) of each of the `pooled` bins along one axis (RoIPoolF: float bin size, floor /
    ceil, shifted by the roi start, clipped to [0, limit])."""
    size = F(extent) / F(pooled)
    p = np.arange(pooled, dtype=F)
    lo = np.floor(p * size).astype(np.int64) + start
    hi = np.ceil((p + F(1)) * size).astype(np.int64) + start
    return np.clip(lo, 0, limit), np.clip(hi, 0, limit)


def roi_loop_pool(x_nchw, rois9, pooled_h=7, pooled_w=7, spatial_scale=0.125, boost=None):
    """x [N,C,H,W], rois9 [R,9] -> (Y [R,C,ph,pw] float32, argmax int32 = h*W+w or -1).  The
    window walk of RoIPoolF over columns 1..4, skipping the pixels strictly inside the rectangle
    of columns 5..8, with the running maximum starting at 0 (strict '>')."""
    x = np.ascontiguousarray(x_nchw, F)
    r9 = np.ascontiguousarray(rois9, F)
    _n, c, H, W = x.shape
    R = r9.shape[0]
    y = np.zeros((R, c, pooled_h, pooled_w), F)
    am = np.full((R, c, pooled_h, pooled_w), -1, np.int32)
    e = _roundf(r9[:, 1:9] * F(spatial_scale))       # float32 products, then roundf
    for r in range(R):
        b = int(r9[r, 0])
        sw, sh, ew, eh, sw_in, sh_in, ew_in, eh_in = (int(v) for v in e[r])
        roi_w, roi_h = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
        hlo, hhi = _bins(sh, roi_h, pooled_h, H)
        wlo, whi = _bins(sw, roi_w, pooled_w, W)
        for ph in range(pooled_h):
            hs, he = int(hlo[ph]), int(hhi[ph])
            if he <= hs:
                continue
            hh = np.arange(hs, he)
            for pw in range(pooled_w):
                ws, we = int(wlo[pw]), int(whi[pw])
                if we <= ws:
                    continue
                ww = np.arange(ws, we)
                hole = ((hh > sh_in) & (hh < eh_in))[:, None] & ((ww > sw_in) & (ww < ew_in))[None, :]
                keep = ~hole.reshape(-1)
                if not keep.any():
                    continue
                idx = (hh[:, None] * W + ww[None, :]).reshape(-1)[keep]
                win = x[b, :, hs:he, ws:we].reshape(c, -1)[:, keep]
                first = win.argmax(1)                 # first maximum in h-major scan order
                m = win[np.arange(c), first]
                pos = m > 0
                y[r, :, ph, pw] = np.where(pos, m, F(0))
                am[r, :, ph, pw] = np.where(pos, idx[first], -1)
        if boost is not None:
            y[r] = y[r] * F(np.asarray(boost, F).reshape(-1)[r])
    return y, am
