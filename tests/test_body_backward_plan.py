"""Host-side guards of tests/test_gpu_body_backward_shapes.py (no GPU): the case table really
reaches the weight gradient's split-K plan, and the helpers the GPU tests lean on say what they
claim."""
import numpy as np

import body_grad_ref as bgr


def test_wgrad_case_table_reaches_every_slice_count():
    """naws_conv3x3_nhwc_wgrad_workspace_floats is a host-only call: per case the slice count the
    plan takes is the one the table states, and together they are {1, 2, 4, 6, 32}."""
    from naws_hip import lib
    L = lib.load()
    got = {c: bgr.wgrad_slices(L.naws_conv3x3_nhwc_wgrad_workspace_floats(*c), c)
           for c in bgr.WGRAD_CASES}
    print(got)
    assert got == bgr.WGRAD_CASES
    assert set(got.values()) == {1, 2, 4, 6, 32}
    # the shapes the older tests run stay at one slice: that is the gap the table closes
    for c in ((1, 9, 13, 32, 64, 1), (2, 9, 13, 32, 64, 2), (1, 12, 16, 256, 256, 1)):
        assert bgr.wgrad_slices(L.naws_conv3x3_nhwc_wgrad_workspace_floats(*c), c) == 1


def test_integer_operands_keep_float32_sums_exact():
    """The bound behind the bit-exact checks: the largest |partial sum| any of the three gradients
    can reach with operands in -2..2 stays below 2^24."""
    for n, h, w, cin, cout, d in bgr.WGRAD_CASES:
        assert 4 * n * h * w < 2 ** 24 and 4 * 9 * max(cin, cout) < 2 ** 24
        assert 2 * n * h * w < 2 ** 24                                     # db
    x, w, dy = bgr.conv_case_int((2, 20, 24, 96, 160, 2), 5)
    for a in (x, w, dy):
        assert a.dtype == np.float32 and set(np.unique(a)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    # float64 autograd on such operands is exact: two summation orders agree to the bit
    dx, dw, db = bgr.conv_grads(x, w, np.zeros(160), dy, 2)
    dw2 = np.zeros_like(dw)
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (2, 2), (2, 2)))
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, :, 2 * ky:2 * ky + 20, 2 * kx:2 * kx + 24]
            dw2[:, :, ky, kx] = np.einsum('nohw,nihw->oi', dy.astype(np.float64), xs)
    assert np.array_equal(dw, dw2) and np.array_equal(db, dy.astype(np.float64).sum((0, 2, 3)))
    assert np.array_equal(dw, np.round(dw)) and np.array_equal(dx, np.round(dx))


def test_tie_census_and_pool_reference_on_a_hand_case():
    """One 2 x 3 image, stride 1, two windows that share the middle column."""
    x = np.array([[[3.], [3.], [1.]], [[0.], [2.], [2.]]], np.float32)[None]     # [1,2,3,1]
    x[0, 1, 1, 0] = 3.5          # windows (3, 3, 0, 3.5): e alone, and (3, 1, 3.5, 2): d alone
    t, s = bgr.tie_census(x, 1)
    assert t.tolist() == [0, 0, 0, 0] and s.tolist() == [0, 0, 1, 1]
    x[0, 1, 1, 0] = 2.0          # windows (3, 3, 0, 2): a, b tied, a selected; (3, 1, 2, 2): a
    t, s = bgr.tie_census(x, 1)
    assert t.tolist() == [1, 1, 0, 0] and s.tolist() == [2, 0, 0, 0]
    dy = np.array([5.0, 7.0], np.float32).reshape(1, 1, 2, 1)
    dx = bgr.maxpool_grad32(x, dy, 1)
    assert dx.reshape(2, 3).tolist() == [[5.0, 7.0, 0.0], [0.0, 0.0, 0.0]]


def test_pool_tie_input_ties_on_every_position():
    """The input of the looping max-pool test: integers 0..3, so most windows tie, on each of
    a, b, d, e; every position is also the selected one somewhere (e only where it is alone)."""
    for stride in (2, 1):
        x = bgr.pool_tie_input((1, 67, 127, 512), stride)
        t, s = bgr.tie_census(x, stride)
        assert (t > 0).all() and (s > 0).all(), (t, s)
        assert not bgr.tie_free(x, stride)
