"""The case lists of the RoIPoolF geometry tests are not vacuous, and the C oracle they compare
the GPU with equals RoIPoolF by definition at every geometry (CPU only).

The census conditions are conditions on the INPUTS, computed from the numpy restatement in
roi_geometry_cases.py alone: a change of the lists that loses a window class fails here, not
silently on the GPU."""
import numpy as np
import pytest

import roi_geometry_cases as g

H, W = g.MAP_H, g.MAP_W
SCALES = (1 / 8, 1 / 16)


def test_geometry_list_holds_the_required_entries():
    want = [(1, 1, 1 / 8), (2, 2, 1 / 16), (3, 5, 1 / 8), (5, 3, 1 / 16), (6, 6, 1 / 8),
            (7, 7, 1 / 16), (4, 9, 1 / 8), (14, 14, 1 / 8), (16, 16, 1 / 8), (16, 17, 1 / 8)]
    assert all(e in g.GEOMETRIES for e in want)
    assert max(ph * pw for ph, pw, _ in g.GEOMETRIES if ph * pw <= g.FAST_LIMIT) == g.FAST_LIMIT
    assert any(ph * pw > g.FAST_LIMIT for ph, pw, _ in g.GEOMETRIES)
    assert len(g.M2_RESIDUES) == 12 and len(g.M4_RESIDUES) == 64


def test_roundf_is_half_away_from_zero_on_fp32():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, -0.49999997, 3.0, -3.0, 0.0, 8388609.0],
                 np.float32)
    assert g.roundf(x).tolist() == [1, 2, 3, -1, -2, -3, 0, 0, 3, -3, 0, 8388609]


@pytest.mark.parametrize('scale', SCALES)
def test_interior_sweep_reaches_every_window_class(scale):
    rois = g.window_sweep(H, W, scale)
    assert rois.shape == (289, 5) and set(rois[:, 0]) == {0.0, 1.0}
    c = g.census(rois, H, W, 1, 1, scale)
    # pooled 1x1: one window per roi, exactly dh x dw for every (dh, dw) in 1..17 x 1..17
    assert (c['empty'], c['dmin1'], c['m2'], c['m4'], c['side9']) == (0, 33, 60, 196, 225)
    assert c['m2_residues'] == g.M2_RESIDUES                        # 12 of 12
    assert c['m4_residues'] == g.M4_RESIDUES                        # 64 of 64
    _, hs, he, ws, we = g.windows(rois, H, W, 1, 1, scale)
    sides = sorted(zip((he - hs).ravel().tolist(), (we - ws).ravel().tolist()))
    assert sides == sorted((a, b) for a in g.SWEEP_SIDES for b in g.SWEEP_SIDES)
    assert len({(int(a), int(b)) for a, b in zip(hs.ravel(), ws.ravel())}) > 100    # offsets vary
    c2 = g.census(rois, H, W, 2, 2, scale)
    assert (c2['empty'], c2['dmin1'], c2['m2'], c2['m4']) == (0, 256, 416, 484)
    assert c2['m2_residues'] == g.M2_RESIDUES and len(c2['m4_residues']) == 36


@pytest.mark.parametrize('scale', SCALES)
def test_clipped_sweep_hangs_over_every_border_with_every_class(scale):
    rois = g.clipped_sweep(H, W, scale)
    assert rois.shape == (289, 5)
    c = g.census(rois, H, W, 1, 1, scale)
    assert (c['empty'], c['dmin1'], c['m2'], c['m4']) == (0, 49, 86, 154)
    assert len(c['m2_residues']) == 11 and len(c['m4_residues']) == 50
    _, sw, sh, rw, rh = g.roi_frame(rois, scale)
    assert (sw < 0).any() and (sh < 0).any() and (sw + rw > W).any() and (sh + rh > H).any()
    c2 = g.census(rois, H, W, 2, 2, scale)      # (a bin that lies wholly outside is empty here)
    assert min(c2['empty'], c2['dmin1'], c2['m2'], c2['m4']) > 0


def test_random_set_covers_every_class_over_the_geometries():
    total = dict(empty=0, dmin1=0, m2=0, m4=0, side9=0, ties_pos=0, ties_neg=0)
    for ph, pw, scale in g.GEOMETRIES:
        rois = g.random_rois(H, W, scale)
        assert rois.shape == (81, 5) and set(rois[:, 0]) == {0.0, 1.0}
        c = g.census(rois, H, W, ph, pw, scale)
        assert c['windows'] == 81 * ph * pw
        assert min(c['empty'], c['dmin1']) > 0                       # at every single geometry
        for k in total:
            total[k] += c[k]
    assert min(total.values()) > 0, total
    # the degenerate rows of helpers.make_rois are in the list
    r = g.random_rois(H, W, 1 / 8)
    assert (r[1, 1:] == 5).all() and r[2, 3] < r[2, 1] and (r[4, 1:] < 0).all()
    assert r[3, 1] >= 2 * W * 8 and r[5, 3] >= W * 8
    # 7x7 at 1/8 on this set (the geometry every other test uses): the M4 class is all but absent
    c = g.census(r, H, W, 7, 7, 1 / 8)
    assert c['m4'] < 0.02 * c['windows'] and len(c['m4_residues']) <= 8


@pytest.mark.parametrize('scale', SCALES)
def test_rounding_rois_carry_ties_of_both_signs(scale):
    rois = g.rounding_rois(scale)
    s = g.scaled(rois, scale)
    tie = np.abs(s - np.trunc(s)) == 0.5
    assert ((tie & (s > 0)).any(1) & (tie & (s < 0)).any(1)).all()   # every roi, each sign
    away = g.roundf(s)
    even = np.rint(s).astype(np.int64)
    assert (away != even).any(1).all()                               # every roi tells them apart
    assert ((away != even) & (s < 0)).any() and ((away != even) & (s > 0)).any()
    t = 0.5 / scale
    assert {t, 5 * t, -t, -3 * t} <= set(rois[:, 1:].ravel().tolist())
    assert list(rois[:, 0]) == sorted(rois[:, 0])                    # grouped by image


@pytest.mark.parametrize('ph,pw,scale', g.GEOMETRIES)
def test_oracle_equals_pooling_by_definition(ph, pw, scale):
    """oracle.roi_pool_f (known-answer tested at 7x7 only) == brute-force numpy pooling over the
    restated windows, bin for bin, argmax included (first index wins; a NaN never does)."""
    from oracle import oracle
    x = g.features(3)
    rois = np.concatenate([g.random_rois(H, W, scale), g.rounding_rois(scale)])
    if ph * pw <= 4:
        rois = np.concatenate([rois, g.window_sweep(H, W, scale), g.clipped_sweep(H, W, scale)])
    y, am = oracle.roi_pool_f(x, rois, ph, pw, scale)
    yb, amb = g.pool_bruteforce(x, rois, ph, pw, scale)
    assert np.array_equal(am, amb)
    assert np.array_equal(y, yb)
    assert (am == -1).any() and (am >= 0).any()


def test_a_half_to_even_restatement_is_told_apart():
    """The comparison above bites: pooling with rint in place of roundf differs from the oracle on
    the rounding rois."""
    from oracle import oracle
    x = g.features(3)
    for scale in SCALES:
        rois = g.rounding_rois(scale)
        y, _ = oracle.roi_pool_f(x, rois, 3, 5, scale)
        yb, _ = g.pool_bruteforce(x, rois, 3, 5, scale, rounding=lambda v: np.rint(v).astype(np.int64))
        assert not np.array_equal(y, yb, equal_nan=True)
