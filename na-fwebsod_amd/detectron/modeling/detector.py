"""DetectionModelHelper: records the operator graph the model-builder functions emit and
generates its backward ops — the role Caffe2's CNNModelHelper + core.Net + AddGradientOperators
play for the reference (detectron/modeling/detector.py:43-586).

Same builder-facing surface for the hot path: `model.Conv/AffineChannel/ConvAffine/Relu/MaxPool/
FC/Dropout/Softmax/Transpose/StopGradient/Accuracy/RoIFeatureTransform`, `model.net.<AnyOp>(inputs, outputs,
**args)`, `model.param_init_net.ConstantFill`, `AddLosses/AddMetrics/TrainableParams`,
`UpdateWorkspaceLr`.  One process drives one GPU, so blob names carry no `gpu_i/` scope.
Execution lives in detectron/core/executor.py (fused MI355X plan or op-by-op).
"""
import collections

from detectron.core.config import cfg
from detectron.core.op_table import cuts_flow, grad_inputs

Op = collections.namedtuple('Op', ['type', 'inputs', 'outputs', 'args'])


def _as_list(x):
    if x is None:
        return []
    return [str(b) for b in x] if isinstance(x, (list, tuple)) else [str(x)]


class Net(object):
    """An ordered op list; `net.SomeOp(inputs, outputs, **args)` appends one op."""

    def __init__(self, name):
        self.name = name
        self.ops = []

    def Proto(self):
        return self

    def add(self, op_type, inputs, outputs, args):
        ins, outs = _as_list(inputs), _as_list(outputs if outputs is not None else inputs)
        self.ops.append(Op(op_type, ins, outs, dict(args)))
        return outs[0] if len(outs) == 1 else tuple(outs)

    def __getattr__(self, op_type):
        if op_type.startswith('_'):
            raise AttributeError(op_type)

        def emit(inputs, outputs=None, **args):
            return self.add(op_type, inputs, outputs, args)
        return emit


class DetectionModelHelper(object):
    def __init__(self, name='', train=False, num_classes=-1, init_params=False):
        assert num_classes > 0, 'num_classes must be > 0'
        self.name = name
        self.train = train
        self.num_classes = num_classes
        self.init_params = init_params
        self.net = Net(name)
        self.param_init_net = Net(name + '_init')
        self.params, self.weights, self.biases = [], [], []
        self.param_shapes, self.param_inits = {}, {}
        self.param_to_grad = {}
        self.computed_params = []      # state an op keeps in the net: never trained, no SGD twins
        self.losses, self.metrics = [], []
        self.do_not_update_params, self.gn_params = [], []
        self.roi_data_loader = None
        self.only_build_forward_pass = False
        self.target_gpu_id = 0
        self.grad_ops = []
        self.grad_fwd_idx = []         # parallel to grad_ops: the forward index of each one's op
        self.update_ops = []
        self.allreduce_ops = []
        self.executor = None

    # ---------------------------------------------------------------- parameters
    def _create_param(self, name, shape, init, is_bias):
        if name not in self.param_shapes:
            self.params.append(name)
            (self.biases if is_bias else self.weights).append(name)
            self.param_shapes[name] = tuple(int(s) for s in shape)
            self.param_inits[name] = init
            self.param_init_net.add(init[0], [], [name], dict(init[1], shape=list(shape)))
        return name

    def create_param(self, param_name, shape, initializer):
        """A parameter outside any layer helper (ref: ModelHelper.create_param as
        wsl_heads.py:231-254 uses it): state that an op updates itself.  Saved and broadcast
        with the others; no gradient op writes `<name>_grad`, so it is never trained and the
        executor keeps no momentum / accumulated-gradient twin for it."""
        if param_name not in self.computed_params:
            self.computed_params.append(param_name)
        return self._create_param(param_name, shape, initializer, False)

    def TrainableParams(self, gpu_id=-1):
        return [p for p in self.params
                if p in self.param_to_grad and p not in self.do_not_update_params]

    # --------------------------------------------------------------- layer helpers
    def Conv(self, blob_in, blob_out, dim_in, dim_out, kernel, weight_init=None, bias_init=None,
             no_bias=0, group=1, **kwargs):
        """stride / pad / dilation ride in kwargs to the op.  no_bias (the ResNet builders, whose
        AffineChannel carries the shift): no `<out>_b` parameter, a two-input op."""
        if group != 1:
            raise NotImplementedError('Conv group: {} is not on the hot path (RESNETS.NUM_GROUPS '
                                      'must be 1)'.format(group))
        w = self._create_param(blob_out + '_w', (dim_out, dim_in, kernel, kernel),
                               weight_init or ('XavierFill', {}), False)
        if no_bias:
            return self.net.add('Conv', [blob_in, w], [blob_out], dict(kwargs, kernel=kernel))
        b = self._create_param(blob_out + '_b', (dim_out,),
                               bias_init or ('ConstantFill', {'value': 0.0}), True)
        return self.net.add('Conv', [blob_in, w, b], [blob_out], dict(kwargs, kernel=kernel))

    def AffineChannel(self, blob_in, blob_out, dim, inplace=False):
        """ref: detector.py:81-105: the per-channel affine that stands for BatchNorm in a
        fine-tuned ResNet; `<out>_s` starts at 1, `<out>_b` at 0."""
        s = self._create_param(blob_out + '_s', (dim,), ('ConstantFill', {'value': 1.0}), False)
        b = self._create_param(blob_out + '_b', (dim,), ('ConstantFill', {'value': 0.0}), True)
        return self.net.add('AffineChannel', [blob_in, s, b], [blob_in if inplace else blob_out], {})

    def ConvAffine(self, blob_in, prefix, dim_in, dim_out, kernel, stride, pad, group=1, dilation=1,
                   weight_init=None, bias_init=None, suffix='_bn', inplace=False):
        """ref: detector.py:428-456: a bias-free Conv followed by AffineChannel."""
        conv_blob = self.Conv(blob_in, prefix, dim_in, dim_out, kernel, stride=stride, pad=pad,
                              group=group, dilation=dilation, weight_init=weight_init,
                              bias_init=bias_init, no_bias=1)
        return self.AffineChannel(conv_blob, prefix + suffix, dim=dim_out, inplace=inplace)

    def FC(self, blob_in, blob_out, dim_in, dim_out, weight_init=None, bias_init=None, **kwargs):
        w = self._create_param(blob_out + '_w', (dim_out, dim_in),
                               weight_init or ('XavierFill', {}), False)
        b = self._create_param(blob_out + '_b', (dim_out,),
                               bias_init or ('ConstantFill', {'value': 0.0}), True)
        return self.net.add('FC', [blob_in, w, b], [blob_out], kwargs)

    def FCShared(self, blob_in, blob_out, dim_in, dim_out, weight=None, bias=None, **kwargs):
        return self.net.add('FC', [blob_in, weight, bias], [blob_out], kwargs)

    def Relu(self, blob_in, blob_out):
        return self.net.add('Relu', [blob_in], [blob_out], {})

    def MaxPool(self, blob_in, blob_out, **kwargs):
        return self.net.add('MaxPool', [blob_in], [blob_out], kwargs)

    def Dropout(self, blob_in, blob_out, **kwargs):
        return self.net.add('Dropout', [blob_in], [blob_out, '_' + str(blob_out) + '_mask'],
                            kwargs)[0]

    def Softmax(self, blob_in, blob_out, **kwargs):
        return self.net.add('Softmax', [blob_in], [blob_out], kwargs)

    def Transpose(self, blob_in, blob_out, **kwargs):
        return self.net.add('Transpose', [blob_in], [blob_out], kwargs)

    def StopGradient(self, blob_in, blob_out):
        return self.net.add('StopGradient', [blob_in], [blob_out], {})

    def Accuracy(self, blobs_in, blob_out, **kwargs):
        return self.net.add('Accuracy', blobs_in, [blob_out], kwargs)

    def DropoutIfTraining(self, blob_in, dropout_rate):
        if self.train and dropout_rate > 0:
            return self.Dropout(blob_in, blob_in, ratio=dropout_rate, is_test=False)
        return blob_in

    def RoIFeatureTransform(self, blobs_in, blob_out, blob_rois='rois', method='RoIPoolF',
                            resolution=7, spatial_scale=1. / 16., sampling_ratio=0):
        """Single feature level only (FPN is outside the hot path).  ref: detector.py:268-331."""
        assert method in {'RoIPoolF', 'RoILoopPool', 'RoIAlign'}, \
            'Unknown pooling method: {}'.format(method)
        assert not isinstance(blobs_in, list), 'FPN RoI transforms are not on the hot path'
        # the two max poolings carry an argmax blob, RoIAlign has one output (ref :287, :321)
        has_argmax = method in {'RoIPoolF', 'RoILoopPool'}
        out = self.net.add(method, [blobs_in, blob_rois],
                           [blob_out] + (['_argmax_' + blob_out] if has_argmax else []),
                           dict(pooled_w=resolution, pooled_h=resolution,
                                spatial_scale=spatial_scale, sampling_ratio=sampling_ratio))
        return out[0] if has_argmax else out

    # ---------------------------------------------------------- losses / metrics
    def AddLosses(self, losses):
        for l in _as_list(losses):
            if l not in self.losses:
                self.losses.append(l)

    def AddMetrics(self, metrics):
        for m in _as_list(metrics):
            if m not in self.metrics:
                self.metrics.append(m)

    def GetLossScale(self):
        return 1.0 / cfg.NUM_GPUS

    # ------------------------------------------------------------------ backward
    def AddGradientOperators(self, loss_gradients):
        """Reverse-mode op generation over the recorded forward ops.  `loss_gradients` maps a
        loss blob to the blob holding its gradient seed (blob.py:167-173).  Blobs consumed by
        several ops accumulate (`<name>_grad` summed), parameters shared by several FC ops
        (the context head's fc6 / fc7 / fc8d_frame) included; StopGradient and the other ops that
        core/op_table.py marks `cuts` stop the flow, so nothing upstream of `roi_feat` / `conv5_3`
        (frozen body) or of pool2 (TRAIN.FREEZE_CONV_BODY False, FREEZE_AT 2) or inside the entropy
        gate gets a gradient op.  An FC or Conv whose input comes from such an op
        (or from outside the net) emits no input gradient: nothing would read it."""
        grad_of = {str(k): str(v) for k, v in loss_gradients.items()}
        ops, fwd_idx = [], []
        producer = {}           # forward index of an op -> {input blob: type of its latest producer}
        latest = {}
        for idx, op in enumerate(self.net.ops):
            producer[idx] = {n: latest.get(n) for n in op.inputs}
            for o in op.outputs:
                latest[o] = op.type
        for idx in range(len(self.net.ops) - 1, -1, -1):
            op = self.net.ops[idx]
            if cuts_flow(op.type):
                for o in op.outputs:
                    grad_of.pop(o, None)
                continue
            gouts = [grad_of.get(o) for o in op.outputs]
            if not any(gouts):
                continue
            wanted = grad_inputs(op.type)
            if wanted is None:
                raise NotImplementedError('no gradient for op {} (blob {} needs one)'.format(
                    op.type, op.outputs[0]))
            gin = []
            for i, name in enumerate(op.inputs):
                gin.append(name + '_grad' if i in wanted else None)
            if op.type in ('FC', 'Conv') and (producer[idx][op.inputs[0]] is None or
                                              cuts_flow(producer[idx][op.inputs[0]])):
                # dX behind StopGradient (fc6 over a frozen body, conv3_1 over pool2): a GEMM /
                # a convolution nobody consumes
                gin[0] = None
            # in-place ops (Relu fc6->fc6): the output's gradient is consumed here
            for o in op.outputs:
                if o in op.inputs:
                    grad_of.pop(o, None)
            accumulate = [g is not None and op.inputs[i] in grad_of for i, g in enumerate(gin)]
            ops.append(Op(op.type + 'Gradient', list(op.inputs) + list(op.outputs),
                          [g for g in gin if g], dict(op.args, _gout=gouts, _gin=gin,
                                                      _accumulate=accumulate)))
            fwd_idx.append(idx)
            for i, g in enumerate(gin):
                if g:
                    grad_of[op.inputs[i]] = g
        for p in self.params:
            if p in grad_of:
                self.param_to_grad[p] = grad_of[p]
        self.grad_ops, self.grad_fwd_idx = ops, fwd_idx
        return ops

    # ------------------------------------------------------------------------ lr
    def UpdateWorkspaceLr(self, cur_iter, new_lr):
        """ref: detector.py:509-559 (lr feed + momentum correction); the executor owns the
        device-side lr scalar and the momentum buffers."""
        return self.executor.update_lr(cur_iter, new_lr)
