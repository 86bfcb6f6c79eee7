"""Fused execution plan of the na_wsddn graph (VGG16-C5 -> RoIPoolF -> two 2-fc
branches -> WSDDN dual softmax -> entropy-gated weighted CE -> backward ->
all-reduce -> ACM momentum SGD) on one MI355X.

This is the plan the graph executor (detectron/modeling/detector.py) selects when
the recorded op list is the reference's na_wsddn graph; it runs
the same named blobs through a handful of fused HIP kernels instead of 103 ops:

  * conv body in NHWC, bias+ReLU in the implicit-GEMM epilogue (frozen, fwd only);
  * RoIPoolF fused with RoIFeatureBoost, written straight in (c,ph,pw) order;
  * fc6 of BOTH branches as ONE GEMM (N = 8192): `fc6_w` and `_[noisy]_fc6_w` are
    adjacent in one parameter arena, so the shared 400 MB `roi_feat` is read once;
  * fc7 / fc8 as batch-2 GEMMs over the interleaved [Rt, 8192] activations;
  * ReLU + Dropout in the GEMM epilogues (counter-based mask, never stored: the
    backward gate is `drop_out > 0`);
  * the whole loss tail in ~8 small kernels, per-image segments keyed on rois[:,0];
  * fc6 wgrad cut into row chunks, each all-reduced (RCCL) while the next runs;
  * one fused SGD launch over the whole parameter arena.

Blob names, shapes and update rule follow the reference:
  detectron/modeling/VGG16.py:9-48, wsl_heads.py:23-56,213-227,654-681,
  webly_heads.py:32-74,123-216,265-391,463-502, optimizer_wsl.py:52-137,
  detectron/ops/acm_weightdecay_momentum_sgd_op.h:48-112.
"""

import collections
import contextlib
import os

import numpy as np
import torch

from . import head_arith
from . import lib as L
from . import ops
from .planes import ALL, FcPlanes
from .reducer import ArenaReducer, message_slice, owner_pieces
from .update import HIDDEN, UpdateSchedule

VGG16_CONVS = [
    # (name, cin, cout, dilation) and pool markers
    ('conv1_1', 3, 64, 1), ('conv1_2', 64, 64, 1), ('pool', 2),
    ('conv2_1', 64, 128, 1), ('conv2_2', 128, 128, 1), ('pool', 2),
    ('conv3_1', 128, 256, 1), ('conv3_2', 256, 256, 1), ('conv3_3', 256, 256, 1), ('pool', 2),
    ('conv4_1', 256, 512, 1), ('conv4_2', 512, 512, 1), ('conv4_3', 512, 512, 1), ('pool4',),
    ('conv5_1', 512, 512, None), ('conv5_2', 512, 512, None), ('conv5_3', 512, 512, None),
]

# The entries of conv_plan().  form: c3 (conv1_1: three input channels, NCHW in); h2_direct,
# h2_wino2, h2_wino4 (fp16x2: the direct halo-tile kernel, Winograd F(2x2,3x3), F(4x4,3x3));
# x3_direct, x3_wino (fp32x3: 3 x bf16 weight planes); f32_direct, f32_wino (fp32); bf16_wp (the
# wave-private halo-tile kernel on one bf16 plane).  direct_alt: the layer also carries h2_direct,
# taken per input size (DIRECT_MIN_TILES); pool2: the 2x2 / stride-2 max-pool that follows may be
# taken in the direct kernel's epilogue; weight_bound: the layer hands the next one an upper bound
# of max|y| from its weights.
ConvStep = collections.namedtuple('ConvStep',
                                  'name form cin cout dilation direct_alt pool2 weight_bound')
# form 'pool': kernel 2 / pad 0 (the origin body); 'pool3': kernel 3 / pad 1 (the DeepLab body)
PoolStep = collections.namedtuple('PoolStep', 'form stride')
_POOL_FORMS = ('pool', 'pool3')
_H2_FORMS = ('h2_direct', 'h2_wino2', 'h2_wino4')
BODIES = ('origin', 'deeplab')


def pooled_size(step, h, w):
    """The output size of PoolStep `step` on an h x w map (floor, the legacy pooling rule)."""
    pad2, k = (2, 3) if step.form == 'pool3' else (0, 2)
    return (h + pad2 - k) // step.stride + 1, (w + pad2 - k) // step.stride + 1


def body_of(conv_body):
    """MODEL.CONV_BODY -> the conv_plan() body it names, or None (no fused chain for it)."""
    return {'VGG16.add_VGG16_conv5_body_origin': 'origin',
            'VGG16.add_VGG16_conv5_body_deeplab': 'deeplab'}.get(conv_body)


def conv_plan(mfma_dtype, dilation, wino_f4_min_cin, body='origin'):
    """The form of every VGG16_CONVS entry (a ConvStep or PoolStep each) under the arithmetic plan
    `mfma_dtype`; dilation: the engine's (2: conv5_x dilated behind a stride-1 pool4).  body
    'deeplab' (VGG16.py:94-140): the four pools are kernel 3 / pad 1 ('pool3') at the same strides
    and none is taken in a conv epilogue (that pool is the 2x2 one); every conv form stays."""
    if mfma_dtype not in ('fp32', 'fp32x3', 'fp16x2', 'bf16'):
        raise ValueError('unknown mfma_dtype %r' % (mfma_dtype,))
    if body not in BODIES:
        raise ValueError('unknown conv body %r' % (body,))
    plan = []
    for i, item in enumerate(VGG16_CONVS):
        if item[0].startswith('pool'):
            plan.append(PoolStep('pool3' if body == 'deeplab' else 'pool',
                                 item[1] if len(item) > 1 else 1 if dilation == 2 else 2))
            continue
        name, cin, cout, dil = item
        wino = cin >= 128 and cout >= 256          # conv3_1 .. conv5_3
        if name == 'conv1_1':
            form = 'c3'
        elif mfma_dtype == 'bf16':
            form = 'bf16_wp'
        elif mfma_dtype == 'fp32':
            form = 'f32_wino' if wino else 'f32_direct'
        elif mfma_dtype == 'fp32x3':
            # conv3_x: the 3-plane direct kernel fills the chip there
            form = 'x3_wino' if wino and cout > 256 else 'x3_direct'
        elif not wino:
            form = 'h2_direct'
        elif 0 < wino_f4_min_cin <= cin and cout >= 512:
            # (conv3_2 / conv3_3, 256 -> 256 at 150 x 250, stay off F(4x4): their V and M are 88 MB
            # each way for a quarter of conv4_2's products - 0.24 vs 0.19 ms per layer-image inside
            # a step)
            form = 'h2_wino4'
        else:
            form = 'h2_wino2'
        # (F(4x4) layers never switch to the direct form: 42.4 vs 43.5 ms per TTA image with it
        # taking over at the large scales, 44.5 for F(2x2) with it)
        direct_alt = form == 'h2_wino2'
        pool2 = (body == 'origin' and i + 1 < len(VGG16_CONVS) and VGG16_CONVS[i + 1][0] == 'pool'
                 and (direct_alt or form in ('h2_direct', 'x3_direct', 'bf16_wp')))
        plan.append(ConvStep(name, form, cin, cout, dil or (2 if dilation == 2 else 1), direct_alt,
                             pool2, form == 'c3' and mfma_dtype == 'fp16x2'))
    return plan


def _conv_operand(form, w):
    """The weight operand of a layer run in `form`, from its fp32 OIHW weight: the packed weight
    [Cout][9 Cin] or U [16 | 36][Cout][Cin], split into 16-bit planes unless the form is fp32."""
    if form == 'c3':
        return w
    if form == 'h2_wino4':
        m = ops.winograd4_weight_transform(w)
    elif 'wino' in form:
        m = ops.winograd_weight_transform(w)
    else:
        m = ops.conv3x3_pack_weight(w).view(w.shape[0], -1)
    ar = next(a for a in head_arith.PLANS.values() if form.startswith(a.conv_prefix + '_'))
    return ar.split(m) if ar.planes16 else m


# An entry packed by set_conv_blobs: the step and, for a conv, the fp32 weight and bias, its form's
# operand, the direct form's (direct_alt) and the (mul, add) of its weight bound (weight_bound)
ConvLayer = collections.namedtuple('ConvLayer', 'step w b operand direct affine')
# What a conv chain carries between layers: the activation, the int32 word of an upper bound of
# max|x| (or None), the (mul, add) to apply to it, and whether the pool that follows is done
ChainState = collections.namedtuple('ChainState', 'x bound affine pooled')
_IDENTITY = (1.0, 0.0)

# The side streams of every engine of a process, by (device, role): 'conv0', 'conv1', ... (one
# chain per image) and 'update'.  HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues
# round-robin as they are first used, and two streams on one queue run in order; a process that
# builds several engines one after another (bench.py's plans, the test suite) would otherwise
# keep drawing new streams from torch's pool until the image chains of one engine share a queue
# with each other or with the main stream (measured: the bf16 plan inside the default bench line
# at 242 instead of 280 img/s).  Shared streams keep the process at main + B + 2 streams; engines
# that are driven one at a time - the only way they are used - lose nothing.
_SIDE_STREAMS = {}


def side_stream(device, role):
    key = (str(device), role)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


def head_param_specs(num_fg_classes, dim_in=512, roi_size=7):
    """Arena order.  Adjacent pairs form the fused GEMM operands."""
    k6, c = dim_in * roi_size * roi_size, num_fg_classes
    return [
        ('fc6_w', (HIDDEN, k6)), ('_[noisy]_fc6_w', (HIDDEN, k6)),
        ('fc6_b', (HIDDEN,)), ('_[noisy]_fc6_b', (HIDDEN,)),
        ('fc7_w', (HIDDEN, HIDDEN)), ('_[noisy]_fc7_w', (HIDDEN, HIDDEN)),
        ('fc7_b', (HIDDEN,)), ('_[noisy]_fc7_b', (HIDDEN,)),
        ('fc8c_w', (c, HIDDEN)), ('fc8d_w', (c, HIDDEN)),
        ('noisy_fc8c_w', (c, HIDDEN)), ('noisy_fc8d_w', (c, HIDDEN)),
        ('fc8c_b', (c,)), ('fc8d_b', (c,)), ('noisy_fc8c_b', (c,)), ('noisy_fc8d_b', (c,)),
    ]


class ParamArena(object):
    """One flat fp32 buffer cut into named blobs (params / grads / momentum share the cut)."""

    def __init__(self, specs, device):
        self.specs = specs
        self.offsets = {}
        off = 0
        for name, shape in specs:
            n = int(np.prod(shape))
            self.offsets[name] = (off, n, shape)
            off += n
        self.total = off
        self.device = device

    def alloc(self, zero=True):
        return (torch.zeros if zero else torch.empty)((self.total,), device=self.device,
                                                      dtype=torch.float32)

    def view(self, flat, name):
        off, n, shape = self.offsets[name]
        return flat[off:off + n].view(shape)

    def span(self, flat, first, last):
        """Contiguous slice covering blobs first..last (inclusive, arena order)."""
        o0 = self.offsets[first][0]
        o1, n1, _ = self.offsets[last]
        return flat[o0:o1 + n1]


class WsddnEngine(object):
    def __init__(self, num_classes, device, dilation=2, roi_size=7, dropout=0.5, is_mean=True,
                 momentum=0.9, weight_decay=5e-4, iter_size=1, gpu_num=1, seed=11,
                 process_group=None, world_size=1, allreduce_chunks=0, freeze_conv_body=True,
                 mfma_dtype='fp16x2', scale_momentum=True, scale_momentum_threshold=1.1,
                 sharded_update=False, rank=None, pipeline_update=None, body='origin'):
        if body not in BODIES:
            raise ValueError('unknown conv body %r' % (body,))
        if not freeze_conv_body:
            raise NotImplementedError('only TRAIN.FREEZE_CONV_BODY: True is on the hot path '
                                      '(SURVEY.md fact 2): the conv body has no backward')
        ar = self.arith = head_arith.plan(mfma_dtype)      # what each plan is: head_arith.PLANS
        L.load()
        self.mfma_dtype = mfma_dtype
        self.C = num_classes - 1
        self.device = device
        self.dilation = dilation
        self.body = body             # 'origin' | 'deeplab' (3x3 / pad-1 pools): conv_plan()
        self.roi_size = roi_size
        self.spatial_scale = 1.0 / 8.0 if dilation == 2 else 1.0 / 16.0
        self.dropout = float(dropout)
        self.is_mean = bool(is_mean)
        self.momentum = float(momentum)
        self.iter_size = int(iter_size)
        self.gpu_num = int(gpu_num)
        self.seed = int(seed)
        # SOLVER.SCALE_MOMENTUM / SCALE_MOMENTUM_THRESHOLD (detector.py:527-559)
        self.scale_momentum = bool(scale_momentum)
        self.scale_momentum_threshold = float(scale_momentum_threshold)
        self.pg, self.world_size = process_group, int(world_size)
        self.reducer = ArenaReducer(process_group, world_size)
        # NAWS.SHARDED_UPDATE (N > 1, fp16x2 plan): fc6_w's gradient rows are reduced to ONE owner
        # each (reduce-scatter), the owner updates its 8192 / N rows (fp32 master rows + momentum
        # live there only), and the updated fp32 rows + their scale words come back by all-gather;
        # every rank then splits the rows into operand planes with the owners' scales.  Same bytes
        # on the links as the all-reduce; the update's HBM traffic beside the next conv body drops
        # from 4.9 GB to 4.9 / N GB for the owned rows plus 1.6 (N-1)/N GB for the planes of the
        # rows the other ranks own (their fp32 rows read once after the gather, planes written);
        # parameters bit-identical to the all-reduce route
        # (tests/test_distributed_cpu.py, tests/test_gpu_two_ranks.py).  See update._apply_sharded.
        self.sharded_update = bool(sharded_update)
        # NAWS.PIPELINE_UPDATE (N > 1, fp16x2 plan; None = on whenever there is an exchange): the
        # deferred update runs PIECE BY PIECE - fc6's biases, then fc6_w in two 4096-row pieces,
        # each as soon as the messages covering it have arrived, then the rest - and the next
        # iteration's fc6 forward starts each piece behind ITS update (naws_gemm_f32_f16x2_nt_cols),
        # so the tail of the exchange hides under fc6 forward too instead of stalling the head
        # (2 ranks: the one xGMI link needs ~10 ms for the 958 MB, the conv body + RoIPool hide 3).
        # Same sums, same update arithmetic, same Dropout masks: parameters bit-identical to the
        # unpipelined route (tests/test_gpu_two_ranks.py).  See update._apply_pipelined.
        self.pipeline_update = pipeline_update
        if rank is None and process_group is not None:
            import torch.distributed as dist
            rank = dist.get_rank(process_group)
        self.rank = int(rank or 0)
        # when, where and by which route a step's update runs, and all the state of that (update.py)
        self.sched = UpdateSchedule(self, lambda: side_stream(device, 'update'))
        # fc6_w's gradient (822 MB of the 958 MB all-reduce) can be reduced in row chunks while
        # the rest of its wgrad GEMM still runs.  0 = auto.  The collective has the tail of the
        # backward pass + the next iteration's parameter-free conv body + RoIPool (~5.7 ms) to
        # hide in; expected exchange: ~4 ms at 8 ranks (7 xGMI links per GPU, less when RCCL shares
        # the CUs with the conv kernels), ~7 ms at 4 (3 links), ~11-13 ms at 2 (one link).  Chunking
        # starts it earlier at the price of wgrad tile quantisation, measured on one GPU with
        # --force-dist: 2 chunks +0.15 ms, 4 chunks +0.4 ms per step.  Auto: 4 chunks at 2 ranks,
        # 2 chunks from 3 ranks up (cheap insurance at 8), 1 for a single rank.
        ac = int(allreduce_chunks)
        ws = int(world_size)
        self.allreduce_chunks = ac if ac >= 1 else (4 if ws == 2 else 2 if ws > 2 else 1)
        self.k6 = 512 * roi_size * roi_size
        self.ld8 = (2 * self.C + 3) // 4 * 4       # per-branch column block of the logit matrices

        self.arena = ParamArena(head_param_specs(self.C, 512, roi_size), device)
        self.params = self.arena.alloc()
        self.grads = self.arena.alloc()
        self.momentum_buf = self.arena.alloc()
        self.acmgrad = self.arena.alloc() if self.iter_size != 1 else None
        ends, lr_mult, wd = [], [], []
        for name, _ in self.arena.specs:
            off, n, _s = self.arena.offsets[name]
            is_bias = name.endswith('_b')
            # biases: no weight decay, 2x lr (optimizer_wsl.py:106-123); '_lrm10_' -> x10 (:125)
            lm = 2.0 if is_bias else 1.0
            if '_lrm10_' in name:
                lm *= 10.0
            w = 0.0 if is_bias else float(weight_decay)
            ends.append(off + n)
            if len(lr_mult) and lr_mult[-1] == lm and wd[-1] == w:
                ends.pop()
                ends[-1] = off + n          # same hyper-parameters as the previous blob: one run
                continue
            lr_mult.append(lm)
            wd.append(w)
        # the fused SGD kernel works on float4s: run boundaries must not split one (they are
        # 4096-multiples or the four fc8 biases = 4C floats, for any class count)
        if any(e % 4 for e in ends):
            raise NotImplementedError('SGD hyper-parameter runs must end on multiples of 4 floats')
        self._seg_host = (list(ends), list(lr_mult), list(wd))
        self.seg_end = torch.tensor(ends, dtype=torch.int64, device=device)
        self.seg_lr_mult = torch.tensor(lr_mult, dtype=torch.float32, device=device)
        self.seg_wd = torch.tensor(wd, dtype=torch.float32, device=device)
        self.lr = torch.zeros((1,), dtype=torch.float32, device=device)
        self._lr_host = 0.0
        self.sgd_iter_count = 0      # the SGD op's iter_count_ state
        self.step_count = 0          # forward/backward passes run (dropout stream)
        self.conv_layers = []        # one ConvLayer per VGG16_CONVS entry (set_conv_blobs)
        self.stat_state = None
        # ---- the public toggles (everything else about the plan is fixed; the arms that lost
        # their A/B are gone - docs/history/ has each measurement) ---------------------------------
        #   mfma_dtype           the arithmetic plan (constructor)
        #   sharded_update       NAWS.SHARDED_UPDATE (constructor)
        #   allreduce_chunks     fc6_w wgrad / exchange row chunks (constructor)
        self.conv_streams = True     # one HIP stream per image for the conv body (bench --no-conv-streams)
        # the SGD kernel writes the updated fc6_w / fc7_w operand planes itself (fp16x2: scale from
        # twice the row maximum before the update, a device-side conditional re-split covers a row
        # that outgrows it; fp32x3 / bf16: exact / rounded planes); False: update, then re-split
        self.fused_planes = True
        # train_step() without a gradient exchange: fc6_w (86 % of the parameters) is updated in
        # the epilogue of its own wgrad GEMM - the gradient is never written (see train_step)
        self.fuse_wgrad_update = True
        # With the conv body frozen, the next iteration's conv + RoIPool do not depend on the
        # parameters: the all-reduce wait and the SGD kernel run on a side stream underneath
        # them (see sgd_step).  Same arithmetic, same order of updates; flush() joins the
        # streams (before the head, checkpoints, lr changes, end of run).
        self.defer_update = None     # None/True -> side stream; False -> inline on the main stream
        # ---- fixed choices, named where the code branches on them ------------------------------
        # Winograd for conv4_1..conv5_3 (and conv3_x in the fp32 plan); under F(2x2) the layers with
        # >= 256 halo tiles per launch (conv1_2..conv3_3 at 600x1000, the deep layers of the larger
        # TTA scales) take the direct kernel: 512 / 1024 / never measured 45.3 / 47.5 / 47.4 vs 44.6
        # ms per TTA image
        self.DIRECT_MIN_TILES = 256
        # fp16x2 plan: Winograd F(4x4,3x3) (csrc/winograd4.hip) for the Winograd layers with at
        # least this many input channels (256: conv4_1..conv5_3; 512 leaves conv4_1 to F(2x2)'s
        # fused kernel: conv body 2.099 vs 2.082 ms, tools/ab_wino4.py); 0 = F(2x2) everywhere
        self.WINO_F4_MIN_CIN = 256
        # fc8's products (tiny output, long K): K in 4 slices + a deterministic second pass (58 vs
        # 97 us, tools/bench_fc8.py)
        self.FC8_KSPLIT = 4
        # entries of VGG16_CONVS each image runs before the deferred update is queued beside the
        # chains (1: conv1_1; 2: conv1_1 + conv1_2 with pool1) where the plan queues it there
        self.UPDATE_AFTER = max(1, ar.update_after)
        self._update_behind_heads = ar.update_after > 0
        # fp16x2 plan: each image's proposals are pooled on that image's conv stream (conv_body)
        self.ROI_POOL_ON_CHAINS = True
        self._fc8_ws = None
        self._seg_ring = None
        self._amax5 = None
        self._streams = []
        self._fc = None              # FcPlanes: fc6_w / fc7_w / fc7_w^T operand planes (16-bit plans)
        self._planes_dirty = True
        # MEASUREMENT AID: NAWS_ENGINE_SET="DIRECT_MIN_TILES=100000,WINO_F4_MIN_CIN=0" overrides the
        # upper-case integer choices above for every engine of the process (A/B runs of entry points
        # that build their engine themselves: bench.py --infer, the CLIs)
        for kv in filter(None, os.environ.get('NAWS_ENGINE_SET', '').split(',')):
            k, v = kv.split('=')
            if not (k.isupper() and isinstance(getattr(self, k, None), int)):
                raise ValueError('NAWS_ENGINE_SET: %r is not an integer engine choice' % k)
            setattr(self, k, int(v))

    # ------------------------------------------------------------------ params
    def blob(self, name):
        self.flush()
        self._planes_dirty = True     # the caller may write through the view
        return self.arena.view(self.params, name)

    def blob_ro(self, name):
        """Read-only view of a parameter (checkpoint saves, statistics): the pending update is
        applied first, but the operand planes stay valid - a save in the middle of a run must not
        change the arithmetic of the steps after it (the planes the update kernels maintain carry
        bound-derived scales, a fresh split exact ones: both correct, not bit-identical)."""
        self.flush()
        return self.arena.view(self.params, name)

    def _one_hyper_run(self, start, count):
        """True when arena elements [start, start + count) share one (lr_mult, weight decay):
        the plane-writing SGD kernel takes ONE pair per region (head_ops.hip sgd_segment)."""
        ends = self._seg_host[0]
        i = next((k for k, e in enumerate(ends) if e > start), None)
        return i is not None and ends[i] >= start + count

    def _head_views(self, flat):
        """Both branches' fc6_w [8192, k6], fc6_b, fc7_w [2, 4096, 4096], fc7_b [2, 4096], fc8's weights
        [2, 2C, 4096] and biases [2, 2C]: views of the arena `flat` (params, grads or momentum)."""
        sp, C = self.arena.span, self.C
        return (sp(flat, 'fc6_w', '_[noisy]_fc6_w').view(2 * HIDDEN, self.k6),
                sp(flat, 'fc6_b', '_[noisy]_fc6_b'),
                sp(flat, 'fc7_w', '_[noisy]_fc7_w').view(2, HIDDEN, HIDDEN),
                sp(flat, 'fc7_b', '_[noisy]_fc7_b').view(2, HIDDEN),
                sp(flat, 'fc8c_w', 'noisy_fc8d_w').view(2, 2 * C, HIDDEN),
                sp(flat, 'fc8c_b', 'noisy_fc8d_b').view(2, 2 * C))

    def _weight_views(self):
        return self._head_views(self.params)[0:3:2]

    # (what tools, tests and bench.py read of the operand planes, under the names they know)
    _wplanes = property(lambda self: getattr(self._fc, 'operands', None))     # w6 / w7 / w7t
    _wovf = property(lambda self: getattr(self._fc, 'ovf', None))
    _rm_table = property(lambda self: getattr(self._fc, 'rm_table', None))
    _sgd_regions = property(lambda self: getattr(self._fc, 'whole', None))
    _sgd_regions_rest = property(lambda self: getattr(self._fc, 'rest', None))
    # (the schedule's state under the names others assign: bench.py resets _shard, _mom_synced and
    # _pipe_sent around its projections, tests/test_gpu_state.py injects _upd_stream)
    _shard = property(lambda self: self.sched.shard,
                      lambda self, v: setattr(self.sched, 'shard', v))
    _mom_synced = property(lambda self: self.sched.mom_synced,
                           lambda self, v: setattr(self.sched, 'mom_synced', v))
    _upd_stream = property(lambda self: self.sched.stream,
                           lambda self, v: setattr(self.sched, 'stream', v))
    _pipe_sent = property(lambda self: self.sched.step.sent,
                          lambda self, v: setattr(self.sched.step, 'sent', v))

    def grad_blob(self, name):
        return self.arena.view(self.grads, name)

    def momentum_blob(self, name):
        self.flush()
        return self.arena.view(self.momentum_buf, name)

    def set_conv_blobs(self, blobs):
        """blobs: name_w [O,I,3,3], name_b [O] (reference layout).  Packs each layer once, for the
        form conv_plan() gives it."""
        layers = []
        for s in conv_plan(self.mfma_dtype, self.dilation, self.WINO_F4_MIN_CIN, body=self.body):
            if s.form in _POOL_FORMS:
                layers.append(ConvLayer(s, None, None, None, None, None))
                continue
            for key, shape in ((s.name + '_w', (s.cout, s.cin, 3, 3)), (s.name + '_b', (s.cout,))):
                if tuple(blobs[key].shape) != shape:
                    raise ValueError('%s has shape %s, the layer needs %s'
                                     % (key, tuple(blobs[key].shape), shape))
            w = blobs[s.name + '_w'].to(self.device, torch.float32).contiguous()
            b = blobs[s.name + '_b'].to(self.device, torch.float32).contiguous()
            # |conv1_1(x)| <= max|x| * max_c sum|w_c| + max|b|: the operand-scale bound of the
            # layer that consumes it, without a pass over its 154 MB output
            affine = ((float(w.abs().sum(dim=(1, 2, 3)).max().item()), float(b.abs().max().item()))
                      if s.weight_bound else None)
            operand = _conv_operand(s.form, w)
            direct = _conv_operand('h2_direct', w) if s.direct_alt else None
            layers.append(ConvLayer(s, w, b, operand, direct, affine))
        self.conv_layers = layers

    def set_head_blobs(self, blobs):
        for name, shape in self.arena.specs:
            if name in blobs:
                self.blob(name).copy_(blobs[name].to(self.device, torch.float32).view(shape))

    def broadcast_parameters(self, src=0):
        """COLLECTIVE (every rank): rank `src`'s parameters, momentum and conv body to every rank
        (reference: utils/net_wsl.py:183-207 copies GPU 0's blobs to the other GPUs through the
        host; here one RCCL broadcast per buffer).  The conv weights are re-packed from what
        arrived, the operand planes re-split on the next forward.  No-op without a process group."""
        if self.pg is None:
            return
        import torch.distributed as dist
        self.flush()
        root = dist.get_global_rank(self.pg, src)
        dist.broadcast(self.params, root, group=self.pg)
        dist.broadcast(self.momentum_buf, root, group=self.pg)
        if self.conv_layers:
            for lay in self.conv_layers:
                if lay.w is not None:
                    dist.broadcast(lay.w, root, group=self.pg)
                    dist.broadcast(lay.b, root, group=self.pg)
            self.set_conv_blobs({k: v for k, v in self.export_blobs(False).items()
                                 if k.startswith('conv')})
        # self.params was written directly: the operand planes no longer match it
        self._planes_dirty = True

    def state_tensors(self):
        """Every buffer that must be bit-identical on all ranks of a data-parallel job after an
        update: parameters, momentum, and (16-bit MFMA plans) the operand planes of fc6_w / fc7_w /
        fc7_w^T with their scale words.  The pending update is joined first; under
        NAWS.SHARDED_UPDATE call gather_sharded_state() (collective) before comparing momentum."""
        self.flush()
        out = dict(params=self.params, momentum=self.momentum_buf)
        if self._wplanes is not None and not self._planes_dirty:
            for k, v in self._wplanes.items():
                if isinstance(v, ops.F16x2):
                    out['planes_' + k], out['scales_' + k] = v.planes, v.scales
                else:
                    out['planes_' + k] = v
        return out

    def set_update_route(self, pipeline_update=None, sharded_update=False):
        """COLLECTIVE when leaving the sharded route (the owners' momentum rows are gathered
        first).  Switch how the deferred update of an N > 1 step runs, at a step boundary:
        pipeline_update None = the default (piece by piece whenever there is an exchange), False =
        one launch behind the whole exchange; sharded_update = NAWS.SHARDED_UPDATE.  All three
        routes hold bit-identical state across the ranks, so a job may change route mid-run
        (bench.py's in-run A/B, the fallback of a training job)."""
        self.sched.set_route(pipeline_update, sharded_update)

    def export_blobs(self, with_momentum=True):
        self.flush()
        if with_momentum and not self.sched.mom_synced:
            raise RuntimeError('NAWS.SHARDED_UPDATE: fc6_w momentum rows live with their owners; '
                               'call gather_sharded_state() on EVERY rank before a checkpoint')
        out = {}
        for lay in self.conv_layers:
            if lay.w is not None:
                out[lay.step.name + '_w'], out[lay.step.name + '_b'] = lay.w, lay.b
        for name, _ in self.arena.specs:
            out[name] = self.blob_ro(name)
            if with_momentum:
                out[name + '_momentum'] = self.momentum_blob(name)
        return out

    # ---------------------------------------------------------------- forward
    def _conv_chain(self, layers, st, out=None, amax_out=None):
        """Run `layers` (a slice of self.conv_layers) on the current stream from ChainState `st`;
        returns the state after them.  The last layer of the slice writes into `out` and, fp16x2
        plan, max|y| into the int32 word `amax_out` (conv5_3: fc6's RoIPool operand scale).

        fp16x2 layers hand max|y| to the next layer (its operand scale needs an upper bound of
        max|x|; a max-pool in between only lowers it), saving that layer's own pass; the words
        the direct kernel max-es into are zeroed by one fill per call."""
        x, bound, aff, pooled = st
        words = (torch.zeros((len(layers),), device=self.device, dtype=torch.int32)
                 if any(lay.step.form in _H2_FORMS for lay in layers) else None)
        for k, lay in enumerate(layers):
            s = lay.step
            if s.form == 'pool3':
                # (a max over real pixels only lowers max|x|: the bound handed on stays valid)
                x = ops.maxpool3x3_nhwc(x, s.stride)
                continue
            if s.form == 'pool':
                if not pooled:
                    x = ops.maxpool2x2_nhwc(x, s.stride)
                pooled = False
                continue
            form, w, b, d = s.form, lay.operand, lay.b, s.dilation
            if lay.direct is not None:
                # direct 2 x f16 halo-tile kernel where it fills the chip (>= one 8x32-pixel x
                # 128-channel tile per CU: conv3_x at 600x1000, and every deep layer once the
                # images share a launch), Winograd below that
                tiles = x.shape[0] * ((x.shape[1] + 7) // 8) * ((x.shape[2] + 31) // 32)
                if tiles * (s.cout // 128) >= self.DIRECT_MIN_TILES:
                    form, w = 'h2_direct', lay.direct
            if aff != _IDENTITY and form != 'h2_direct':
                raise ValueError('%s: its input bound carries (mul, add) = %r, which the %s form '
                                 'cannot apply' % (s.name, aff, form))
            last = k == len(layers) - 1
            dst = out if last else None
            pooled = s.pool2 and form in ('h2_direct', 'x3_direct', 'bf16_wp')
            word, word_aff = None, _IDENTITY          # the bound this layer hands on
            if form in _H2_FORMS:
                word = amax_out if last and amax_out is not None else words[k:k + 1]
            if form == 'c3':
                y = ops.conv3x3_c3_nchw_to_nhwc(x, w, b, True)
                if lay.affine is not None:
                    word, word_aff = ops.amax_word(x), lay.affine     # 7 MB: the network input
                x = y
            elif form == 'h2_direct':
                x = ops.conv3x3_nhwc_f16x2(x, w, b, True, out=dst, amax_in=bound, in_mul=aff[0],
                                           in_add=aff[1], amax_out=word, pool2=pooled,
                                           amax_out_zeroed=word is not amax_out, dilation=d)
            elif form in ('h2_wino2', 'h2_wino4'):
                x = ops.conv3x3_winograd_nhwc_f16x2(x, w, b, d, True, out=dst, amax_in=bound,
                                                    amax_out=word)
            elif form == 'x3_direct':
                x = ops.conv3x3_nhwc_f32x3(x, w, b, d, True, out=dst, pool2=pooled)
            elif form == 'x3_wino':
                x = ops.conv3x3_winograd_nhwc_f32x3(x, w, b, d, True, out=dst)
            elif form == 'f32_direct':
                x = ops.conv3x3_nhwc(x, w, b, d, True, out=dst)
            elif form == 'f32_wino':
                x = ops.conv3x3_winograd_nhwc(x, w, b, d, True, out=dst)
            elif form == 'bf16_wp':
                x = ops.conv3x3_nhwc_bf16_wp(x, w, b, d, True, out=dst, pool2=pooled)
            bound, aff = word, word_aff
        return ChainState(x, bound, aff, pooled)

    def conv_body(self, data, roi_job=None):
        """data NCHW [B,3,H,W] -> conv5_3 NHWC [B,H/8-1,W/8-1,512].

        roi_job = (rois, obn_scores, seg) (fp16x2 plan, one chain per image): every image's
        proposals are pooled at the tail of ITS chain, on its stream, beside the other images'
        last layers - RoIPoolF + boost straight into fc6's operand planes, rows seg[i]..seg[i+1];
        the finished operand is then in self._roi_operand (consumed by _roi_features).

        The 13 layers of one image are a dependent chain, and the deep layers have only a
        couple of workgroup-tiles per CU, so every layer ends on a partially filled chip.
        Images are independent: each image's chain is queued on its own HIP stream and the
        hardware packs the tail of one image's layer with the head of the other's."""
        n = data.shape[0]
        # fp16x2: max|conv5_3| per image (per chain) for the RoIPool -> fc6 operand scale
        planes = self.conv_layers[-1].step.form in _H2_FORMS
        per_image = n > 1 and self.conv_streams
        self._roi_maps = None
        self._roi_operand = None
        self._amax5 = (torch.empty((n if per_image else 1,), device=self.device,
                                   dtype=torch.int32) if planes else None)
        # a waiting update goes behind the per-image conv1_1 heads (below), or - none - out at once
        split = self.sched.waits_for_heads(per_image and self._update_behind_heads)
        if not per_image:
            res = self._conv_chain(self.conv_layers, ChainState(data, None, _IDENTITY, False),
                                   amax_out=self._amax5).x
            self._roi_maps_of = (res.data_ptr(), res._version)
            return res
        h, w = data.shape[2], data.shape[3]
        for s in (lay.step for lay in self.conv_layers if lay.step.form in _POOL_FORMS):
            h, w = pooled_size(s, h, w)
        out = torch.empty((n, h, w, 512), device=self.device, dtype=torch.float32)
        # (bf16 plan: RoIPoolF writes fc6's one-plane operand over the same maps)
        self._roi_maps = ((torch.empty_like(out), torch.empty_like(out))
                          if self.arith.roi_maps_on_chains else None)
        # the maps belong to THIS tensor in THIS state (_take_roi_maps)
        self._roi_maps_of = (out.data_ptr(), out._version)
        pooled = None
        if (roi_job is not None and planes and self.ROI_POOL_ON_CHAINS
                and roi_job[0].shape[0] > 0 and len(roi_job[2]) == n + 1):
            self._check_rows_grouped_by_image(roi_job[0], roi_job[2])
            pooled = ops.roi_pool_operand(roi_job[0].shape[0], self.k6, self.device)
        main = torch.cuda.current_stream(self.device)
        start = main.record_event()
        while len(self._streams) < n:
            self._streams.append(side_stream(self.device, 'conv%d' % len(self._streams)))
        chains = [ChainState(data[i:i + 1], None, _IDENTITY, False) for i in range(n)]
        layers = self.conv_layers
        if split:
            # the head of every image's chain first (conv1_1: HBM-bound, 0.06 ms alone), THEN the
            # deferred parameter update, then the rest of the chains: started together, the SGD
            # kernel's workgroups fill the CUs and the two conv1_1 launches at the head of the
            # dependent chains took 0.7 ms each (kernel trace)
            ua = min(max(1, self.UPDATE_AFTER), len(layers) - 1)
            evs = []
            for i in range(n):
                st = self._streams[i]
                st.wait_event(start)
                with torch.cuda.stream(st):
                    chains[i] = self._conv_chain(layers[:ua], chains[i])
                    evs.append(st.record_event())
            self.sched.launch(evs)
            layers = layers[ua:]
        for i in range(n):
            st = self._streams[i]
            if not split:
                st.wait_event(start)
            with torch.cuda.stream(st):
                af = None if self._amax5 is None else self._amax5[i:i + 1]
                self._conv_chain(layers, chains[i], out=out[i:i + 1], amax_out=af)
                if self._roi_maps is not None:
                    # RoIPoolF's block-maxima maps of this image, beside the other image's tail
                    ops.roi_maxmaps(out[i:i + 1], self._roi_maps[0][i:i + 1], self._roi_maps[1][i:i + 1])
                    if pooled is not None and roi_job[2][i + 1] > roi_job[2][i]:
                        # ... and its proposals pooled right behind them (batch index i: the maps
                        # and conv5_3 of the other images are not touched)
                        ops.roi_pool_f_f16x2_range(out, roi_job[0], self._amax5, pooled, roi_job[2][i],
                                                   roi_job[2][i + 1], self._roi_maps, self.roi_size,
                                                   self.roi_size, self.spatial_scale,
                                                   boost=roi_job[1].reshape(-1))
                done = st.record_event()
            main.wait_event(done)
        if pooled is not None:
            # the operand belongs to exactly these tensors in exactly this state (_roi_features)
            self._roi_operand = (pooled, out.data_ptr(), self._roi_job_key(roi_job[0], roi_job[1]))
        return out

    @staticmethod
    def _roi_job_key(rois, obn_scores):
        return (rois.data_ptr(), rois._version, obn_scores.data_ptr(), obn_scores._version)

    def _check_rows_grouped_by_image(self, rois, seg):
        """Precondition of the per-image pooling on the conv streams: rows seg[i]..seg[i+1] of
        `rois` carry batch index i (the kernel takes the image from rois[:,0], the stream from
        seg).  Checked on the device, with a host sync, under NAWS_DEBUG_CHECKS=1 only."""
        import os
        if os.environ.get('NAWS_DEBUG_CHECKS') != '1':
            return
        want = torch.repeat_interleave(
            torch.arange(len(seg) - 1, device=rois.device, dtype=rois.dtype),
            torch.tensor([seg[i + 1] - seg[i] for i in range(len(seg) - 1)], device=rois.device))
        if want.numel() != rois.shape[0] or not bool((rois[:, 0] == want).all().item()):
            raise ValueError('rois must be grouped by image in order: rows seg[i]..seg[i+1] must '
                             'carry batch index i (seg = %r)' % (list(seg),))

    def _seg_to_device(self, seg):
        """Per-image row offsets -> int32 device tensor WITHOUT stalling the host: a copy from
        pageable memory (torch.tensor(list, device=...)) is synchronous and waits for everything
        queued on the stream before it, i.e. once per step the host stopped running ahead of the GPU
        and queued the next conv body just in time (the second image's chain started 1.5 ms after
        the first one's in the kernel trace).  Here: a small ring of pinned slots, async copies."""
        n = len(seg)
        if self._seg_ring is None or self._seg_ring[0][0].numel() < n:
            self._seg_ring = [[torch.empty((max(n, 64),), dtype=torch.int32).pin_memory(), None]
                              for _ in range(8)]
            self._seg_next = 0
        slot = self._seg_ring[self._seg_next]
        self._seg_next = (self._seg_next + 1) % len(self._seg_ring)
        if slot[1] is not None:
            slot[1].synchronize()          # eight copies ago: long done
        slot[0][:n] = torch.tensor(seg, dtype=torch.int32)
        out = slot[0][:n].to(self.device, non_blocking=True)
        slot[1] = torch.cuda.current_stream(self.device).record_event()
        return out

    @staticmethod
    def segments(rois, n_img):
        """seg_off (host list) from rois[:,0]; rows must be grouped by image in order."""
        b = rois[:, 0].to(torch.int64)
        counts = torch.bincount(b, minlength=n_img).cpu().tolist()
        seg = [0]
        for c in counts:
            seg.append(seg[-1] + c)
        return seg

    def _seed(self, layer):
        return (self.seed * 0x9E3779B1 + self.step_count * 1000003 + layer * 7919) & ((1 << 62) - 1)

    @contextlib.contextmanager
    def _timed(self, name, on=True):
        """bench.py's HIP event lists (timing_events, comm_events, update_events): if the engine
        carries a list called `name` (and `on`), a pair of timing events recorded on the current
        stream around the body is appended to it; otherwise nothing is recorded."""
        evs = getattr(self, name, None) if on else None
        pair = evs is not None and (torch.cuda.Event(enable_timing=True),
                                    torch.cuda.Event(enable_timing=True))
        if pair:
            pair[0].record()
        yield
        if pair:
            pair[1].record()
            evs.append(pair)

    def _take_roi_maps(self, conv5):
        """The block-maxima maps conv_body() built beside the chains, if `conv5` is the very
        tensor it returned, unmodified (same storage, same version counter); None for any other
        tensor of the same shape - the pooling wrapper then builds maps of what it is given."""
        maps, self._roi_maps = getattr(self, '_roi_maps', None), None
        if maps is not None and getattr(self, '_roi_maps_of', None) != (conv5.data_ptr(), conv5._version):
            maps = None
        return maps

    def _roi_features(self, conv5, rois, obn_scores):
        """RoIPoolF + boost -> the fc6 input: fp32 [Rt, k6], or (fp16x2 plan) the GEMM operand
        planes written by the pooling kernel itself."""
        done = getattr(self, '_roi_operand', None)
        self._roi_operand = None
        if done is not None and done[1] == conv5.data_ptr() \
                and done[2] == self._roi_job_key(rois, obn_scores) \
                and getattr(self, '_roi_maps_of', None) == (conv5.data_ptr(), conv5._version):
            self._roi_maps = None
            return done[0]                    # pooled per image at the tails of the conv chains
        if self._amax5 is not None:
            mine = getattr(self, '_roi_maps_of', None) == (conv5.data_ptr(), conv5._version)
            maps = self._take_roi_maps(conv5)
            if not mine:
                # a caller's own feature map (or conv_body's, modified): max|conv5_3| - the
                # bound behind the operand scale of the planes - is taken from what was passed
                self._amax5 = torch.cat([ops.amax_word(conv5[i:i + 1].contiguous())
                                         for i in range(self._amax5.numel())]) \
                    if self._amax5.numel() == conv5.shape[0] else ops.amax_word(conv5.contiguous())
            return ops.roi_pool_f_f16x2(conv5, rois, self._amax5, self.roi_size, self.roi_size,
                                        self.spatial_scale, boost=obn_scores.reshape(-1),
                                        hier=True, maps=maps)
        if self.arith.roi_pool_slab and self.k6 % 64 == 0 and conv5.shape[-1] % 64 == 0:
            maps = self._take_roi_maps(conv5)
            if maps is None:
                maps = (torch.empty_like(conv5), torch.empty_like(conv5))
                ops.roi_maxmaps(conv5, maps[0], maps[1])
            return ops.roi_pool_f_bf16_slab(conv5, rois, maps, self.roi_size, self.roi_size,
                                            self.spatial_scale, boost=obn_scores.reshape(-1))
        roi_feat = ops.roi_pool_f(conv5, rois, self.roi_size, self.roi_size, self.spatial_scale,
                                  boost=obn_scores.reshape(-1), layout='NHWC', hier=True)
        return roi_feat.view(rois.shape[0], self.k6)

    def _fc_operands(self):
        """w6 / w7 / w7t as the plan's GEMM operands: fp32, the arena's own views; otherwise the
        16-bit planes FcPlanes keeps, re-split first when a caller wrote the parameters."""
        ar, (w6, w7) = self.arith, self._weight_views()
        if not ar.planes16:
            return dict(w6=ar.operand(w6), w7=ar.operand(w7), w7t=ar.operand(w7, transpose=True))
        if self._fc is None:
            n6 = 2 * HIDDEN
            o6, ob, o7 = (self.arena.offsets[k][0] for k in ('fc6_w', 'fc6_b', 'fc7_w'))
            self._fc = FcPlanes(ar, n6, self.k6, HIDDEN, o6, ob, o7, self.arena.total, self.device,
                                self._one_hyper_run(o6, n6 * self.k6),
                                self._one_hyper_run(o7, n6 * HIDDEN))
        if self._planes_dirty:
            self._fc.split_all(w6, w7)
            self._planes_dirty = False
        return self._fc.operands

    def head_forward(self, roi_feat, train, both_branches=True, pieces=None):
        """roi_feat [Rt, k6] (or its operand form, written by the pooling kernel) -> H6, H7
        [Rt, nb*4096], logits L [Rt, nb*2C].  pieces: the pipelined update's events
        (UpdateSchedule.join_for_head)."""
        ar = self.arith
        nb = 2 if both_branches else 1
        _w6, b6, _w7, b7, w8, b8 = self._head_views(self.params)
        drop = train and self.dropout > 0
        epi6, epi7 = (dict(epilogue=L.EPI_BIAS_RELU_DROP if drop else L.EPI_BIAS_RELU, bias=b,
                           drop_ratio=self.dropout if drop else 0.0, seed=self._seed(layer))
                      for layer, b in ((6, b6), (7, b7)))
        if pieces is not None and not (ar.reports_maxima and nb == 2):
            self.sched.finish_pieces(pieces)     # (a caller's own plan: join the whole update first)
            pieces = None
        W = self._fc_operands()
        # the activation operand in the plan's form (its own kernels, outside the timed launch)
        xp = ar.operand(roi_feat)
        # bench.py: HIP events around the dominant kernel (piece by piece: around each piece)
        with self._timed('timing_events', on=pieces is None):
            if ar.reports_maxima:
                h6, sc6n, sc6t = self._fc6_forward_maxima(xp, W['w6'], nb, train, epi6, pieces)
            else:
                h6 = ar.gemm_nt(xp, ar.rows(W['w6'], 0, nb * HIDDEN), **epi6)
        xp = None
        rt = h6.shape[0]
        h6v = h6.view(rt, nb, HIDDEN).permute(1, 0, 2)       # [nb, Rt, 4096] strided views
        h7 = torch.empty((rt, nb * HIDDEN), device=self.device, dtype=torch.float32)
        h7v = h7.view(rt, nb, HIDDEN).permute(1, 0, 2)
        if ar.reports_maxima:
            # one pass over h6 writes both operand forms (rows for fc7, columns for fc7's wgrad)
            h6n, self._h6t = ops.split_f16x2_dual(h6v, sc6n, sc6t)
        else:
            h6n = ar.operand(h6v)
        ar.gemm_nt(h6n, ar.batches(W['w7'], nb), out=h7v, **epi7)
        del h6n
        # logits [Rt, nb * ld8]: branch b holds fc8c | fc8d in columns b*ld8 .. b*ld8 + 2C.  ld8 = 2C
        # rounded up to 4 floats so the batch-2 GEMM operands stay 16-byte aligned for any class
        # count (odd C: the weights / bias are copied into zero-padded [ld8, 4096] operands)
        w8g, b8g = self._fc8_operands(w8, b8)
        lg = torch.empty((rt, nb * self.ld8), device=self.device, dtype=torch.float32)
        lgv = lg.view(rt, nb, self.ld8).permute(1, 0, 2)
        self._fc8_gemm(h7v, w8g[:nb], False, True, lgv, L.EPI_BIAS, b8g)
        return h6, h7, lg

    def _fc6_forward_maxima(self, xp, w6, nb, train, epi, pieces):
        """fp16x2's fc6 forward: the GEMM epilogue reports max|h6| per row of each branch (fc7's
        operand scale) and, in training, per column (fc7 wgrad's) - no pass over h6 for them.
        Returns h6 and the two scale blocks.  pieces (the pipelined update): piece (r0, r1) = weight
        rows / h6 columns r0..r1 of one branch, launched behind the event of ITS update; same kernel,
        same K order, same Dropout counters as the one launch (naws_gemm_f32_f16x2_nt_cols)."""
        ar, rt = self.arith, xp.planes.shape[-2]
        self._new_amax_arena(rt, nb)
        sc6n = self._scales(nb, rt)
        sc6t = self._scales(nb, HIDDEN) if train else None
        rowwords = ops.amax_words(sc6n)                       # [nb, Rt]
        colwords = None if sc6t is None else ops.amax_words(sc6t)
        if pieces is None:
            h6 = ar.gemm_nt(xp, ar.rows(w6, 0, nb * HIDDEN), rowmax=rowwords, rowmax_seg=HIDDEN,
                            colmax=colwords, **epi)
            return h6, sc6n, sc6t
        h6 = torch.empty((rt, nb * HIDDEN), device=self.device, dtype=torch.float32)
        main = torch.cuda.current_stream(self.device)
        for r0, r1, ev in pieces['fc6']:
            main.wait_event(ev)
            if r0 // HIDDEN != (r1 - 1) // HIDDEN:
                raise RuntimeError('a forward piece must lie inside one branch')
            with self._timed('timing_events'):
                ops.gemm_f32_f16x2_nt_cols(
                    xp, ar.rows(w6, r0, r1), h6[:, r0:r1], r0, nb * HIDDEN,
                    **dict(epi, bias=epi['bias'][r0:r1]), rowmax=rowwords[r0 // HIDDEN],
                    rowmax_seg=HIDDEN, colmax=None if colwords is None else colwords.view(-1)[r0:r1])
        self.sched.finish_pieces(pieces)     # fc7 / fc8 read the rest of the update
        return h6, sc6n, sc6t

    def _fc8_gemm(self, a, b, trans_a, trans_b, out, epilogue=L.EPI_NONE, bias=None):
        """fc8's products have a small output and a long inner dimension (K = 4096 forward,
        K = proposals for dW8): K in FC8_KSPLIT slices + a deterministic second pass
        (ops.gemm_splitk: 58 vs 97 us on the bench shape, tools/bench_fc8.py); 0 = one pass."""
        ks = int(self.FC8_KSPLIT)
        if ks <= 1:
            return ops.gemm(a, b, trans_a, trans_b, out=out, epilogue=epilogue, bias=bias)
        need = out.shape[-2] * out.shape[-1] * (out.shape[0] if out.dim() == 3 else 1) * ks
        if self._fc8_ws is None or self._fc8_ws.numel() < need:
            self._fc8_ws = torch.empty((need,), device=self.device, dtype=torch.float32)
        return ops.gemm_splitk(a, b, trans_a, trans_b, out=out, epilogue=epilogue, bias=bias,
                               ksplit=ks, workspace=self._fc8_ws)

    def _new_amax_arena(self, rt, nb):
        """One zero-fill per step for every |.| maxima vector the GEMM epilogues accumulate into
        (h6 rows + columns, dZ7 rows + columns, dZ6 columns)."""
        need = 2 * (2 * nb * rt + 2 * nb * HIDDEN + 2 * HIDDEN) + 64
        self._amax_arena = torch.zeros((need,), device=self.device, dtype=torch.float32)
        self._amax_used = 0

    def _scales(self, batch, outer):
        n = 2 * batch * outer
        o = self._amax_used
        self._amax_used = (o + n + 3) // 4 * 4
        assert self._amax_used <= self._amax_arena.numel()
        return self._amax_arena[o:o + n].view(2, batch, outer)

    def _fc8_operands(self, w8, b8):
        C, ld8 = self.C, self.ld8
        if ld8 == 2 * C:
            return w8, b8
        w8p = torch.zeros((2, ld8, HIDDEN), device=self.device, dtype=torch.float32)
        b8p = torch.zeros((2, ld8), device=self.device, dtype=torch.float32)
        w8p[:, :2 * C].copy_(w8)
        b8p[:, :2 * C].copy_(b8)
        return w8p, b8p

    def forward_backward(self, data, rois, obn_scores, labels_oh, compute_grads=True, seg=None,
                         _fuse_update=False):
        """One training pass over this GPU's images.  Returns dict of loss tensors
        (per image) and keeps what backward / stats need.  `seg` = host list of per-image row
        offsets [0, R0, R0+R1, ...] (the loader knows it); when omitted it is derived from
        rois[:,0] on the device, which costs a device->host sync per iteration."""
        C = self.C
        n_img = data.shape[0]
        if seg is None:
            seg = self.segments(rois, n_img)
        rt = rois.shape[0]
        max_seg = max(seg[i + 1] - seg[i] for i in range(n_img))
        seg_off = self._seg_to_device(seg)
        pev = getattr(self, 'phase_events', None)   # bench.py: per-stage HIP events (main stream)

        def mark(name):
            if pev is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                pev.append((name, e))
        mark('start')
        conv5 = self.conv_body(data, roi_job=(rois, obn_scores, seg))
        mark('conv_body')
        x = self._roi_features(conv5, rois, obn_scores)
        del conv5
        mark('roi_pool')
        # previous iteration's all-reduce + SGD, now overlapped: joined here as a whole, or - the
        # pipelined N > 1 update - piece by piece inside the head forward
        pieces = self.sched.join_for_head()
        mark('join_update')
        h6, h7, lg = self.head_forward(x, train=True, pieces=pieces)
        mark('head_fwd')
        ld8 = self.ld8
        cols = [0, C, ld8, ld8 + C]                          # fc8c, fc8d, noisy_fc8c, noisy_fc8d
        lv = [lg[:, o:o + C] for o in cols]
        ac, ad, rp, cp = ops.wsddn_outputs(lv[0], lv[1], lv[2], lv[3], seg_off)
        cw, cwn, hs, hsn = ops.entropy_gate(rois, rp[0], cp[0], labels_oh, seg_off, max_seg)
        # [class_weight | class_weight_noise] as one [2, nseg, C] view of the gate's output buffer;
        # both branches score against the same labels_oh (no stack / expand / ones kernels: the
        # loss tail is the hand-written kernels only)
        wts = cw._base[:2] if cw._base is not None and cw._base.dim() == 3 else torch.stack([cw, cwn])
        lab = labels_oh if labels_oh.is_contiguous() else labels_oh.contiguous()
        losses = ops.weighted_ce_shared(cp, lab, wts, self.is_mean)        # [2*nseg]
        out = dict(loss_cls=losses[:n_img], loss_cls_noise=losses[n_img:], cls_prob=cp[0],
                   cls_prob_noise=cp[1], class_weight=cw, class_weight_noise=cwn,
                   hatE_sum=hs, hatE_sum_norm=hsn, rois_pred=rp[0],
                   logits=torch.cat(lv, 1) if ld8 != 2 * C else lg)   # fc8c|fc8d|noisy_fc8c|noisy_fc8d
        self.step_count += 1
        mark('loss_tail')
        if not compute_grads:
            return out
        # ---- backward (loss gradient seed 1.0 per loss, blob.py:167-173)
        g = ops.weighted_ce_shared_grad(cp, lab, wts, self.is_mean, dy_const=1.0)
        dl = (torch.zeros if ld8 != 2 * C else torch.empty)((rt, 2 * ld8), device=self.device,
                                                            dtype=torch.float32)
        ops.wsddn_outputs_grad(ac, ad, rp, cp, g, seg_off, out=dl, col_offsets=cols)
        self._head_backward(x, h6, h7, dl, fuse_update=_fuse_update)
        mark('head_bwd')
        out['d_logits'] = dl if ld8 == 2 * C else torch.cat([dl[:, o:o + C] for o in cols], 1)
        return out

    def _head_backward(self, x, h6, h7, dl, fuse_update=False):
        C, rt, G = self.C, h6.shape[0], self.grads
        scale = 1.0 / (1.0 - self.dropout) if self.dropout > 0 else 1.0
        gw6, gb6, gw7, gb7, gw8, gb8 = self._head_views(G)
        ld8, pad = self.ld8, self.ld8 != 2 * C
        dz7, dz6 = torch.empty_like(h7), torch.empty_like(h6)
        dlv, h7v, h6v, dz7v, dz6v = (t.view(rt, 2, -1).permute(1, 0, 2)      # [2, Rt, ld8 | 4096]
                                     for t in (dl, h7, h6, dz7, dz6))
        ar, amax = self.arith, self.arith.reports_maxima
        W = self._fc_operands()
        red = self.reducer
        # x: the pooling kernel's own operand (fp16x2 planes with per-roi scales, the bf16 slab), or a
        # caller's fp32 features
        pooled = ar.is_operand(x)
        # Order: the data-gradient chain first, then fc6_w's gradient (86 % of the all-reduce
        # bytes) so that its exchange starts as early as possible, the small gradients last.
        # 1. dZ7 = dL W8 and dZ6 = dZ7 W7, each gated by the ReLU / Dropout of its layer
        w8g = self._fc8_operands(*self._head_views(self.params)[4:])[0]      # (ld8 rows when padded)
        amax7, gate6 = {}, dict(epilogue=L.EPI_GATE_POS, aux=h6v, alpha=scale)
        if amax:
            # every GEMM reports the maxima its consumer's operand split needs; each of dZ7 / dZ6
            # is then read once by a split that writes all the forms in which it is multiplied.
            # x's planes carry per-roi scales s_r: dW6 = sum_r (dZ6[r] / s_r) (x[r] s_r), so dZ6's
            # column maxima are taken over dZ6[r] / s_r (exact: powers of two)
            sc7n, sc7t, sc6t = self._scales(2, rt), self._scales(2, HIDDEN), self._scales(1, 2 * HIDDEN)
            amax7 = dict(rowmax=ops.amax_words(sc7n), colmax=ops.amax_words(sc7t))
            rowmul = x.inv_scale if pooled else None
            gate6.update(colmax=ops.amax_words(sc6t), colmax_rowmul=rowmul)
        ops.gemm(dlv, w8g, False, False, out=dz7v, epilogue=L.EPI_GATE_POS, aux=h7v, alpha=scale,
                 **amax7)
        # dX = dZ W: W^T's operand is kept beside W's
        if amax:
            dz7n, dz7t = ops.split_f16x2_dual(dz7v, sc7n, sc7t)
        else:
            dz7n = ar.operand(dz7v)
        ar.gemm_nt(dz7n, W['w7t'], out=dz6v, **gate6)
        del dz7n
        # 2. fc6: dW = dZ6^T X in row chunks (both operands K(=rows)-contiguous through the
        # transposing split); each chunk's all-reduce starts while the next one is computed
        if amax:
            # planes [2, Rt/16, 8192, 16] of (diag(1/s_r) dZ6)^T
            dz6t = ops.split_f16x2_dual(dz6, None, sc6t.view(2, 2 * HIDDEN), rowmul=rowmul)[1]
        else:
            dz6t = ar.operand(dz6, transpose=True)             # [(3,) Rt/16, 8192, 16]
        # x^T [.., Rt/16, 25088, 16]: a caller's fp32 features are split transposed; the pooling
        # kernel's planes are read as they are, through transposing LDS reads (fp16x2:
        # csrc/gemm_btr.hip), or transposed plane to plane (bf16)
        if not pooled:
            xt = ar.operand(x, transpose=True)
        else:
            xt = None if amax else ops.bf16_slab_transpose(x)
        fuse = fuse_update and self._can_fuse_wgrad_update() and (pooled or not amax)
        # the messages of this step; pipelined train_step(): its update queued part by part behind them
        st = self.sched.begin_backward(fuse_update)
        plan, pipelined = st.plan, st.sent
        if pipelined:
            # fc6's bias gradients first (the first forward piece of the next iteration needs the
            # updated biases): a column sum of dZ6, known before the weight gradient
            ops.colsum(dz6, out=gb6)
            red.reduce_async(message_slice(self.arena, G, 'fc6_b', None, self.k6))
            plan = plan[1:]
            st.bias_sent()
        for kind, rows in plan[:-1]:
            r0, r1 = rows
            a = ar.rows(dz6t, r0, r1)
            if amax:
                self._fc6_wgrad_cut(a, x, xt, gw6, r0, r1, fuse)
            elif fuse:
                self._wgrad_update_w6(a, xt, r0, r1)
            else:
                ar.gemm_nt(a, xt, out=gw6[r0:r1])
            blocks = self._shard_blocks()
            if blocks is None:
                red.reduce_async(message_slice(self.arena, G, kind, rows, self.k6))
            else:      # each owner's rows of this chunk go to that owner only
                for o, p0, p1 in owner_pieces(r0, r1, blocks):
                    red.reduce_to_owner_async(gw6[p0:p1].reshape(-1), o)
            st.chunk_sent(r1)
        # 3. the small gradients (under the fc6_w exchange): fc6 db; fc7 dW = dZ7^T H6, db;
        # fc8 dW = dL^T H7, db
        if not pipelined:
            ops.colsum(dz6, out=gb6)
        if amax:
            a7, h6t, self._h6t = dz7t, self._h6t, None
        else:
            a7, h6t = ar.operand(dz7v, transpose=True), ar.operand(h6v, transpose=True)
        ar.gemm_nt(a7, h6t, out=gw7)
        del a7, h6t
        ops.colsum(dz7, out=gb7)
        if pad:
            gw8p = torch.empty((2, ld8, HIDDEN), device=self.device, dtype=torch.float32)
            self._fc8_gemm(dlv, h7v, True, False, gw8p)
            gw8.copy_(gw8p[:, :2 * C])
            gb8.copy_(ops.colsum(dl).view(2, ld8)[:, :2 * C])
        else:
            self._fc8_gemm(dlv, h7v, True, False, gw8)
            ops.colsum(dl, out=gb8)
        red.reduce_async(message_slice(self.arena, G, *plan[-1], self.k6))
        st.tail_sent()

    def _can_fuse_wgrad_update(self):
        return self.sched.can_fuse_wgrad_update()

    def _fc6_wgrad_cut(self, a, x, xt, gw6, r0, r1, fuse):
        """fp16x2: rows r0..r1 of fc6_w's gradient (a: those rows of dZ6^T's operand; xt: x^T's, or
        None: x is the pooling kernel's operand, read as it is) or, `fuse`, their update.  25088 =
        98 column tiles of 256: 32 x 98 = 12.25 waves of 256 CUs.  96 column tiles make 12 full
        waves; the last 512 columns go out as one wave of 128x128 tiles."""
        ncut = self._wgrad_column_cut(r1 - r0)
        cuts = ((0, ncut), (ncut, self.k6)) if ncut else ((0, self.k6),)
        if fuse:
            return self._wgrad_update_w6(a, x, r0, r1, cuts)
        for c0, c1 in cuts:
            if xt is None:
                ops.gemm_f32_f16x2_nt_xk(a, x, ncols=(c0, c1), out=gw6[r0:r1, c0:c1])
            else:
                self.arith.gemm_nt(a, self.arith.rows(xt, c0, c1), out=gw6[r0:r1, c0:c1])

    def _wgrad_update_w6(self, a, x, r0, r1, cuts=None):
        """fc6_w's rows r0..r1 updated (parameters, momentum, operand planes) in the epilogue of
        their wgrad GEMM, on the main stream.  fp16x2 (cuts: the column ranges, x: the pooling
        kernel's planes): the first chunk makes the rows' maxima the bounds of this update, the last
        one queues the conditional exact re-split.  bf16 (x: x^T's slab): one rounded plane, no
        scales, nothing to bound or re-split."""
        fc, tag, (ends, lr_mult, wd) = self._fc, self.sgd_iter_count + 1, self._seg_host
        o6, last = self.arena.offsets['fc6_w'][0], r1 == 2 * HIDDEN
        sg = next(i for i, e in enumerate(ends) if e > o6)      # (one run: _can_fuse_wgrad_update)
        w6, m6 = self._weight_views()[0], self._head_views(self.momentum_buf)[0]
        sgd = (self.lr, lr_mult[sg], wd[sg], self.momentum, 0, self.gpu_num, self.sgd_iter_count)
        if cuts is None:
            ops.gemm_bf16_slab_nt_sgd(a, x, w6, m6, *sgd, fc.operands['w6'], rows=(r0, r1))
        else:
            if r0 == 0:
                fc.begin(ALL, with7=False)
            for c0, c1 in cuts:
                ops.gemm_f32_f16x2_nt_xk_sgd(a, x, w6, m6, *sgd, fc.operands['w6'].planes,
                                             fc.bound(6), fc.maxima(6), fc.inv_scale(6), fc.ovf, tag,
                                             ncols=(c0, c1), rows=(r0, r1))
            if last:
                fc.resplit6(w6, ALL, fc.ovf, tag)
        if last:
            self.sched.w6_done(fc.rest)

    def train_step(self, data, rois, obn_scores, labels_oh, seg=None):
        """forward_backward + sgd_step as one call.  With no gradient exchange between the two
        (one process; the reference adds its all-reduce ops only for NUM_GPUS > 1,
        optimizer_wsl.py:52-72) fc6_w's update runs in the epilogue of its wgrad GEMM: same
        arithmetic, same planes, but the gradient (0.82 GB written and read back) never exists
        and the update's traffic hides inside an MFMA-bound kernel instead of time-slicing with
        the next conv body.  `self.grads` then holds no fc6_w gradient.  With an exchange, or
        fuse_wgrad_update = False, this is exactly forward_backward(); sgd_step()."""
        out = self.forward_backward(data, rois, obn_scores, labels_oh, seg=seg, _fuse_update=True)
        self.sgd_step()
        return out

    def _wgrad_column_cut(self, rows, cus=256):
        """fc6 wgrad tile quantisation: with 256x256 tiles the [rows, k6] output is tm x tn tiles;
        if the last partial wave of `cus` tiles is less than half full, return the column where
        to cut so that the first launch is whole waves (the rest runs as small tiles), else 0."""
        tm, tn = (rows + 255) // 256, (self.k6 + 255) // 256
        tail = (tm * tn) % cus
        if tail == 0 or tail * 2 > cus or tail % tm != 0:
            return 0
        ncut = (tn - tail // tm) * 256
        return ncut if 0 < ncut < self.k6 else 0

    def wait_allreduce(self):
        self.reducer.wait()

    # -------------------------------------------------------------------- SGD
    def set_lr(self, new_lr):
        """UpdateWorkspaceLr + momentum correction (detector.py:509-559)."""
        new_lr = float(np.float32(new_lr))
        if self._lr_host == new_lr:
            return new_lr
        self.flush()                 # a pending update must see the lr it was computed under
        cur = self._lr_host
        self._lr_host = new_lr
        if cur != new_lr:
            ratio = max(new_lr / max(cur, 1e-10), cur / max(new_lr, 1e-10))
            self.lr.fill_(new_lr)
            if self.scale_momentum and cur > 1e-7 and ratio > self.scale_momentum_threshold:
                # the correction is a float32 quotient in the reference (np.float32 / np.float32,
                # detector.py:536) and the Scale op's float argument
                corr = float(np.float32(new_lr) / np.float32(cur))
                ops.unary(L.UN_SCALE, self.momentum_buf, corr, out=self.momentum_buf)
        return new_lr

    def sgd_step(self):
        """Queue this iteration's update (UpdateSchedule.queue: by default on a side stream, under
        the next iteration's conv body; `flush()` - called before anything touches the parameters -
        joins the two streams)."""
        self.sched.queue()

    def flush(self):
        self.sched.flush()

    def _pipelined(self):
        return self.sched.pipelined()

    def _shard_blocks(self):
        return self.sched.shard_blocks()

    def gather_sharded_state(self):
        """COLLECTIVE (every rank): the owners' momentum rows of fc6_w to all ranks (NAWS.SHARDED_UPDATE;
        before a checkpoint).  No-op otherwise."""
        self.sched.gather_sharded_state()

    # -------------------------------------------------------------- inference
    def infer(self, data, rois, obn_scores, seg=None):
        """Test-mode forward: cls_prob [R, C+1] = Concat(rois_pred[:, :1], rois_pred)
        (wsl_heads.py:58-67); no dropout; only the clean branch is fetched (test_wsl.py:151)."""
        if rois.shape[0] == 0:
            raise ValueError('infer: no proposals (rois is empty)')
        self.flush()
        n_img = data.shape[0]
        if seg is None:
            seg = self.segments(rois, n_img)
        seg_off = self._seg_to_device(seg)
        conv5 = self.conv_body(data, roi_job=(rois, obn_scores, seg))
        x = self._roi_features(conv5, rois, obn_scores)
        _h6, _h7, lg = self.head_forward(x, train=False, both_branches=False)
        C = self.C
        _ac, _ad, rp, _cp = ops.wsddn_outputs(lg[:, :C], lg[:, C:2 * C], None, None, seg_off)
        return torch.cat([rp[0][:, :1], rp[0]], dim=1)

    # ------------------------------------------------------------------ Stat
    def stat_update(self, out, labels_oh, display, printer=print):
        """The six Stat ops of webly_heads.py:400-440 (image 0 of this process)."""
        C = self.C
        if self.stat_state is None:
            self.stat_state = dict(AI=torch.zeros((6, C), device=self.device),
                                   AL=torch.zeros((6, C), device=self.device), it=0, init=True)
        st = self.stat_state
        lab = labels_oh[0].contiguous()
        bg = ops.unary(L.UN_SCALE, lab, -1.0)
        bg = ops.binary(L.BIN_ADD, bg.view(1, C), torch.ones((1, 1), device=self.device)).view(C)
        pairs = [('class_weight      ', out['class_weight'][0], bg),
                 ('class_weight_noise', out['class_weight_noise'][0], bg),
                 ('hatE_sum bg       ', out['hatE_sum'][0], bg),
                 ('hatE_sum fg       ', out['hatE_sum'][0], lab),
                 ('hatE_sum_norm bg  ', out['hatE_sum_norm'][0], bg),
                 ('hatE_sum_norm fg  ', out['hatE_sum_norm'][0], lab)]
        for k, (_p, i_, l_) in enumerate(pairs):
            ops.stat_accumulate(i_.contiguous(), l_, st['AI'][k], st['AL'][k], st['init'])
        st['init'] = False
        st['it'] += 1
        if st['it'] % display == 0 or st['it'] == 1:
            ai, al = st['AI'].cpu().numpy(), st['AL'].cpu().numpy()
            with np.errstate(divide='ignore', invalid='ignore'):
                ratio = ai / al
            for k, (p, _i, _l) in enumerate(pairs):
                printer('\t' + p + ' Stat #iter_: ' + str(st['it']) + ''.join(
                    ' %.2f' % v for v in ratio[k]))
            st['init'] = True
