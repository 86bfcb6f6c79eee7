#!/usr/bin/env python3
"""fc6 weight gradient (8192 x 25088 x 4000) from the forward planes, csrc/gemm_btr.hip: the K-loop
forms of the 256 x 256 kernel interleaved in ONE process on the same random operands (h2 = 0: the
default, software-pipelined loop; h2 = 18: the two-phase loop), plain and with the SGD update in the
epilogue, over the engine's 24576-column main block; median ms per form.

    python tools/bench_xk.py [--rounds 9] [--knobs 0 18]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from naws_hip import lib as L, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--knobs', type=int, nargs='+', default=[0, 18])
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(1)
    r, m, n, nc = 4000, 8192, 25088, 24576
    x = torch.randn((r, n), device=dev, generator=g).relu_()
    dy = torch.randn((r, m), device=dev, generator=g) * 1e-3
    dy[torch.rand((r, m), device=dev, generator=g) < 0.75] = 0
    xp = ops.split_f16x2(x)
    del x
    a2 = ops.split_f16x2(dy, transpose=True, rowmul=xp.inv_scale)
    out = torch.empty((m, nc), device=dev)
    w = torch.randn((m, n), device=dev, generator=g) * 0.02
    mom = torch.zeros_like(w)
    planes = ops.split_f16x2(w)
    bound = (planes.scales[0].view(torch.int32) + (2 << 23)).clone()     # 4x the row maxima: no overflow
    rowmax = torch.zeros((m,), device=dev, dtype=torch.int32)
    inv = torch.zeros((m,), device=dev)
    ovf = torch.zeros((1,), device=dev, dtype=torch.int32)
    lr = torch.tensor([1e-5], device=dev)
    forms = {
        'xk     ': lambda: ops.gemm_f32_f16x2_nt_xk(a2, xp, ncols=(0, nc), out=out),
        'xk sgd ': lambda: ops.gemm_f32_f16x2_nt_xk_sgd(a2, xp, w, mom, lr, 1.0, 5e-4, 0.9, 0, 1, 1,
                                                        planes.planes, bound, rowmax, inv, ovf, 7,
                                                        ncols=(0, nc)),
    }
    times = {(f, k): [] for f in forms for k in a.knobs}
    try:
        for rnd in range(a.rounds + 1):
            for f, fn in forms.items():
                for k in a.knobs:
                    L.set_variant('h2', k)
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize()
                    if rnd > 0:
                        times[(f, k)].append(s.elapsed_time(e))
    finally:
        L.set_variant('h2', 0)
    fl = 2.0 * m * nc * r
    for f in forms:
        print('fc6 wgrad %s M=%d N=%d K=%d  ' % (f, m, nc, r) + '   '.join(
            'h2=%d: med %.3f ms %.0f TF (min %.3f)' % (
                k, sorted(times[(f, k)])[len(times[(f, k)]) // 2],
                fl / sorted(times[(f, k)])[len(times[(f, k)]) // 2] / 1e9, min(times[(f, k)]))
            for k in a.knobs))
    assert int(ovf.item()) == 0


if __name__ == '__main__':
    main()
