"""Net executor: runs the graph a DetectionModelHelper recorded on one MI355X.

Replaces `workspace.RunNet(model.net)` + the Caffe2 dag executor of the reference
(detectron/utils/train_wsl.py:59, detectron/modeling/detector.py:63-64).  Two plans:

  * FUSED — chosen when the recorded op list is exactly the na_wsddn graph (the one
    `VGG16.add_VGG16_conv5_body_origin` + `webly_heads.add_VGG16_roi_2fc_noise_head` +
    `add_webly_outputs` + `add_webly_losses` emit): the blobs run through
    naws_hip.engine.WsddnEngine (fused kernels, any number of images per process).  The same
    graph over `VGG16.add_VGG16_conv5_body_deeplab` (MODEL.CONV_BODY) is fused too: its chain
    pools with kernel 3 / pad 1.  Any other body (`add_VGG16_conv4_body_origin`) runs op by op.
  * INTERPRETED — any other graph made of the supported operators runs op by op through
    detectron.ops (same HIP kernels, one launch group per op, reference semantics of one
    image per process); detectron/core/op_table.py declares each operator once.  It is also
    the cross-check of the fused plan in the tests.

Blob names are the reference's unscoped names (one process per GPU).
"""
import numpy as np
import torch

from detectron.core.config import cfg
from detectron.core.op_table import TABLE
import detectron.ops as O
from naws_hip import lib as L
from naws_hip import ops as K


def _signature(ops_list):
    return [(o.type, tuple(o.inputs), o.outputs[0]) for o in ops_list]


def _pool_args(ops_list):
    """(kernel, pad, stride) of every MaxPool: what tells the conv bodies apart (the signature
    carries names only, and the DeepLab body's are the origin body's)."""
    return [(o.args.get('kernel'), o.args.get('pad'), o.args.get('stride'))
            for o in ops_list if o.type == 'MaxPool']


def _canonical_na_wsddn_ops(train, num_classes):
    """The canonical model's ops with the conv body MODEL.CONV_BODY names (the origin body when the
    key is empty, as before there was a second one); None for a body the fused engine does not run."""
    from detectron.modeling.detector import DetectionModelHelper
    from detectron.modeling import VGG16, webly_heads
    from naws_hip.engine import body_of
    body = body_of(cfg.MODEL.CONV_BODY or 'VGG16.add_VGG16_conv5_body_origin')
    if body is None:
        return None
    m = DetectionModelHelper(name='canon', train=train, num_classes=num_classes, init_params=train)
    blob, dim, scale = getattr(VGG16, 'add_VGG16_conv5_body_' + body)(m)
    m.StopGradient(blob, blob)
    ls, dims = webly_heads.add_VGG16_roi_2fc_noise_head(m, blob, dim, scale)
    webly_heads.add_webly_outputs(m, ls, dims)
    if train:
        webly_heads.add_webly_losses(m)
    return m.net.ops


def canonical_na_wsddn_signature(train, num_classes):
    """The op list the reference builders emit for the hot-path config under the current cfg, over
    the configured conv body; None when that body has no fused plan (the caller then runs op by
    op)."""
    ops_list = _canonical_na_wsddn_ops(train, num_classes)
    return None if ops_list is None else _signature(ops_list)


def _is_canonical_na_wsddn(model, sig):
    """The model's op list is the canonical one: the same names AND the same pools (the DeepLab
    body differs from the origin body by its MaxPool arguments and, under FREEZE_AT: 2, the
    StopGradient at pool2 alone)."""
    canon = _canonical_na_wsddn_ops(model.train, model.num_classes)
    return (canon is not None and sig == _signature(canon) and
            _pool_args(model.net.ops) == _pool_args(canon))


def _fill(init, shape, gen, device):
    kind, args = init
    if kind == 'ConstantFill':
        return torch.full(shape, float(args.get('value', 0.0)), device=device)
    if kind == 'GaussianFill':
        return (torch.randn(shape, generator=gen) * args.get('std', 1.0) +
                args.get('mean', 0.0)).to(device)
    if kind == 'XavierFill':       # U(+-sqrt(3/fan_in)), fan_in = prod(shape[1:])
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
        lim = (3.0 / fan_in) ** 0.5
        return ((torch.rand(shape, generator=gen) * 2 - 1) * lim).to(device)
    if kind == 'MSRAFill':
        fan_out = int(np.prod(shape)) // shape[1] if len(shape) > 1 else shape[0]
        return (torch.randn(shape, generator=gen) * (2.0 / fan_out) ** 0.5).to(device)
    raise NotImplementedError('initializer ' + kind)


class NetExecutor(object):
    def __init__(self, model, device, process_group=None, world_size=1, rank=0,
                 force_interpreted=False, images_per_process=1, disable_dropout=False):
        self.model, self.device = model, device
        self.pg, self.world, self.rank = process_group, int(world_size), int(rank)
        self.ws = {}
        self.step = 0
        self.lr = torch.zeros((1,), device=device)
        self.ims = int(images_per_process)
        self.disable_dropout = bool(disable_dropout)   # parity tests only
        model.executor = self
        sig = _signature(model.net.ops)
        fused_ok = (not force_interpreted and cfg.WEBLY.WEBLY_ON and cfg.WEBLY.ENTROPY and
                    cfg.TRAIN.FREEZE_CONV_BODY and
                    # the canonical list is built under the current cfg, so it contains CenterLoss
                    # too: the fused engine does not compute that loss and must not be chosen
                    not cfg.WSL.CENTER_LOSS and
                    # likewise RoIAlign: the engine pools with RoIPoolF whatever the op list says
                    cfg.FAST_RCNN.ROI_XFORM_METHOD == 'RoIPoolF' and
                    # the canonical list is built over the conv body MODEL.CONV_BODY names; a body
                    # without a fused chain (the conv4 body, a user's own) has none and runs op by op
                    _is_canonical_na_wsddn(model, sig))
        self.plan = 'fused' if fused_ok else 'interpreted'
        self.engine = None
        if fused_ok:
            from naws_hip.engine import WsddnEngine, body_of
            self.engine = WsddnEngine(
                model.num_classes, device, dilation=cfg.WSL.DILATION,
                body=body_of(cfg.MODEL.CONV_BODY or 'VGG16.add_VGG16_conv5_body_origin'),
                roi_size=cfg.FAST_RCNN.ROI_XFORM_RESOLUTION,
                dropout=0.0 if disable_dropout else 0.5,
                is_mean=cfg.WSL.MEAN_LOSS, momentum=cfg.SOLVER.MOMENTUM,
                weight_decay=cfg.SOLVER.WEIGHT_DECAY, iter_size=cfg.WSL.ITER_SIZE,
                gpu_num=self.world * self.ims, seed=cfg.RNG_SEED, process_group=process_group,
                world_size=world_size, allreduce_chunks=cfg.NAWS.ALLREDUCE_CHUNKS,
                mfma_dtype=cfg.NAWS.MFMA_DTYPE, scale_momentum=cfg.SOLVER.SCALE_MOMENTUM,
                scale_momentum_threshold=cfg.SOLVER.SCALE_MOMENTUM_THRESHOLD,
                sharded_update=cfg.NAWS.SHARDED_UPDATE, rank=self.rank,
                pipeline_update=cfg.NAWS.PIPELINE_UPDATE)
        else:
            if self.ims != 1:
                raise NotImplementedError('the op-by-op plan follows the reference: one image '
                                          'per process (wsl_heads.py:214)')
            self._state, self._sgd = {}, {}     # per-op objects by forward op index; SGD by param

    # -------------------------------------------------------------- parameters
    def init_params(self, seed=None):
        gen = torch.Generator().manual_seed(cfg.RNG_SEED if seed is None else seed)
        blobs = {n: _fill(self.model.param_inits[n], self.model.param_shapes[n], gen, self.device)
                 for n in self.model.params}
        self.load_blobs(blobs)

    def load_blobs(self, blobs):
        """blobs: {unscoped name: tensor} in the reference layouts (FC [out,in], conv OIHW)."""
        if self.engine is not None:
            self.engine.set_conv_blobs(blobs)
            self.engine.set_head_blobs(blobs)
            for n in self.model.params:
                if n + '_momentum' in blobs and n in self.engine.arena.offsets:
                    self.engine.momentum_blob(n).copy_(blobs[n + '_momentum'].to(self.device))
        else:
            for n in self.model.params:
                self.ws[n] = blobs[n].to(self.device, torch.float32).contiguous()
                if n in self.model.computed_params:     # op state: SGD never touches it
                    continue
                self.ws[n + '_momentum'] = torch.zeros_like(self.ws[n])
                self.ws[n + '_acmgrad'] = torch.zeros_like(self.ws[n])

    def blobs(self, with_momentum=True):
        if self.engine is not None:
            return self.engine.export_blobs(with_momentum)
        out = {}
        for n in self.model.params:
            out[n] = self.ws[n]
            if with_momentum and n not in self.model.computed_params:
                out[n + '_momentum'] = self.ws[n + '_momentum']
        return out

    def broadcast_parameters(self):
        """Rank 0's parameters to every rank (net_wsl.py:183-207 does host copies)."""
        if self.pg is None or self.world <= 1:
            return
        import torch.distributed as dist
        if self.engine is not None:
            self.engine.broadcast_parameters(0)
        else:
            for n in self.model.params:
                dist.broadcast(self.ws[n], 0, group=self.pg)

    # ---------------------------------------------------------------------- lr
    def update_lr(self, cur_iter, new_lr):
        new_lr = float(np.float32(new_lr))
        if self.engine is not None:
            self.lr.fill_(new_lr)
            return self.engine.set_lr(new_lr)
        cur = float(self.lr.item())
        if cur != new_lr:
            ratio = max(new_lr / max(cur, 1e-10), cur / max(new_lr, 1e-10))
            self.lr.fill_(new_lr)
            if cfg.SOLVER.SCALE_MOMENTUM and cur > 1e-7 and \
                    ratio > cfg.SOLVER.SCALE_MOMENTUM_THRESHOLD:
                for n in self.model.TrainableParams():
                    m = self.ws[n + '_momentum']
                    # a float32 quotient, as in the reference (detector.py:536-537) and the engine
                    K.unary(L.UN_SCALE, m, float(np.float32(new_lr) / np.float32(cur)), out=m)
        return new_lr

    # -------------------------------------------------------------------- run
    def feed(self, blobs):
        self.ws.pop('_seg', None)      # host-side row offsets only ever describe the current rois
        for k, v in blobs.items():
            self.ws[k] = v

    def fetch(self, name):
        return self.ws[name]

    def run(self):
        """One iteration: forward (+ backward, all-reduce, SGD when training)."""
        if self.engine is not None:
            self._run_fused()
        else:
            self._run_interpreted()
        self.step += 1

    def _run_fused(self):
        ws, eng = self.ws, self.engine
        if self.model.train:
            out = eng.train_step(ws['data'], ws['rois'], ws['obn_scores'], ws['labels_oh'],
                                 seg=ws.get('_seg'))
            ws['loss_cls'], ws['loss_cls_noise'] = out['loss_cls'], out['loss_cls_noise']
            ws['cls_prob'], ws['cls_prob_noise'] = out['cls_prob'], out['cls_prob_noise']
            ws['rois_class_weight'] = out['class_weight']
            ws['rois_class_weight_noise'] = out['class_weight_noise']
            ws['rois_pred'] = out['rois_pred']
            if self.rank == 0:
                eng.stat_update(out, ws['labels_oh'], max(1, int(1280 / cfg.NUM_GPUS)))
        else:
            ws['cls_prob'] = eng.infer(ws['data'], ws['rois'], ws['obn_scores'], seg=ws.get('_seg'))

    # ------------------------------------------------------ op-by-op plan
    def _run_interpreted(self):
        ws = self.ws
        for idx, op in enumerate(self.model.net.ops):
            self._forward(idx, op, ws)
        if not self.model.train:
            return
        for op, fwd_idx in zip(self.model.grad_ops, self.model.grad_fwd_idx):
            self._backward(op, ws, fwd_idx)
        params = self.model.TrainableParams()
        if self.pg is not None and self.world > 1:
            import torch.distributed as dist
            for p in params:
                dist.all_reduce(ws[self.model.param_to_grad[p]], group=self.pg)
            # Center_loss_surgery (cpg_utils.py:270-289): the centre contributions are summed over
            # the ranks; the gradient half of the op takes them in at the next iteration.  Past
            # max_iter the op no longer rewrites the blobs: summing the stale values again every
            # iteration would multiply them by `world` until they overflow (the reference's appended
            # all-reduce does; harmless there too, as nothing reads them), so the sum stops with it.
            for idx, op in enumerate(self.model.net.ops):
                if op.type == 'CenterLoss' and self._state[idx].contributed:
                    dist.all_reduce(ws[op.inputs[4]], group=self.pg)
                    dist.all_reduce(ws[op.inputs[5]], group=self.pg)
        for p in params:
            if p not in self._sgd:
                bias = p in self.model.biases
                lm = (2.0 if bias else 1.0) * (10.0 if '_lrm10_' in p else 1.0)
                self._sgd[p] = O.ACMWeightDecayMomentumSGDUpdate(
                    momentum=cfg.SOLVER.MOMENTUM, weight_decay=0.0 if bias else
                    cfg.SOLVER.WEIGHT_DECAY, iter_size=cfg.WSL.ITER_SIZE, gpu_num=self.world,
                    lr_mult=lm)
            self._sgd[p](ws[self.model.param_to_grad[p]].contiguous(), ws[p + '_momentum'],
                         self.lr, ws[p], ws[p + '_acmgrad'])

    def dropout_seed(self, idx):
        """A Dropout op's seed: the run's, the iteration and the op's place in the net."""
        return cfg.RNG_SEED * 1000003 + self.step * 131 + idx

    @staticmethod
    def _gather(op, ws):
        """The values of op.inputs; a name the workspace does not hold is an error before any
        kernel runs, never a shift of the later inputs."""
        for n in op.inputs:
            if n not in ws:
                raise KeyError('{} -> {}: input blob {} is not in the workspace'.format(
                    op.type, op.outputs[0] if op.outputs else '', n))
        return [ws[n] for n in op.inputs]

    def _forward(self, idx, op, ws):
        e = TABLE.get(op.type)
        if e is None or e.forward is None:
            raise NotImplementedError('operator {} is not on the MI355X hot path'.format(op.type))
        x = self._gather(op, ws)
        if e.state is not None and idx not in self._state:
            self._state[idx] = e.state(op)      # one object per op: the gradient half shares it
        for n, v in zip(op.outputs, e.forward(self, idx, op, x)):
            ws[n] = v

    def _backward(self, op, ws, fwd_idx=None):
        """fwd_idx: the forward op's index (model.grad_fwd_idx), where its state is kept."""
        t, a = op.type[:-len('Gradient')], op.args
        e = TABLE.get(t)
        if e is None or e.gradient is None:
            raise NotImplementedError('gradient of ' + t)
        n_in = len(a['_gin'])
        v = self._gather(op, ws)                # the forward op's inputs, then its outputs
        gout = [ws[g] if g else None for g in a['_gout']]
        res = e.gradient(self, fwd_idx, op, v[:n_in], v[n_in:], gout)
        for i, r in enumerate(res):
            g = a['_gin'][i]
            if g is None or r is None:
                continue
            if a['_accumulate'][i] and g in ws:
                ws[g] = O.Add(ws[g], r).view(r.shape)
            else:
                ws[g] = r
