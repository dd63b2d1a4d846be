"""BinaryClassificationTask and RegressionTask: host-side mirror of transformers4rec/torch/model/prediction_task.py
  BinaryClassificationTask :66-173    (SequenceSummary -> Linear(D, 1, bias=False) -> Sigmoid -> squeeze, BCELoss)
  RegressionTask           :206-303   (SequenceSummary -> Linear(D, 1) -> squeeze, MSELoss)
  PredictionTask           model/base.py:52-232 (build, forward, task_name, metrics)
with the same arguments, output dict {"loss", "labels", "predictions"}, task names and state_dict names
(`pre.0.weight` [1, D], `pre.0.bias` [1] for regression only).  One label per session, predicted from a summary of the body's
[B, L, D] output.  Arithmetic: csrc/seq_task.hip (include/t4r_hip_seqtask.h) -- two launches forward, two backward, where the
reference's op chain is about six and eight.  The metrics (torchmetrics in the reference) are small classes of this module
that keep their counts on the device.
"""
import re

import torch
from torch import nn

from . import ops
from .masking import _grad_buf

_SUMMARIES = {"first": ops.SUMMARY["first"], "last": ops.SUMMARY["last"], "mean": ops.SUMMARY["mean"],
              # HF's SequenceSummary takes the last position when no cls_index is passed, and the reference passes none
              "cls_index": ops.SUMMARY["last"]}


def _snake(name):
    return re.sub(r"(?<!^)(?=[A-Z])", "_", name).lower()


# ------------------------------------------------------------------------------------------------ metrics
class _CountMetric(nn.Module):
    """a metric as a ratio of two counts accumulated on the device (fp64): forward(predictions, targets) adds the batch and
    returns the batch's own value, compute() the value over everything since reset()"""
    _n_state = 2

    def __init__(self):
        super().__init__()
        self._state = None

    def _counts(self, predictions, targets):       # -> (numerator, denominator) of the batch, 0-dim tensors
        raise NotImplementedError

    @staticmethod
    def _ratio(st):
        return torch.where(st[1] > 0, st[0] / st[1].clamp(min=1), torch.zeros_like(st[0])).float()

    def forward(self, predictions, targets):
        st = torch.stack([c.to(torch.float64) for c in self._counts(predictions, targets)])
        self._state = st if self._state is None else self._state.to(st.device) + st
        return self._ratio(st)

    def compute(self):
        return torch.zeros(()) if self._state is None else self._ratio(self._state)

    def reset(self):
        self._state = None


class Precision(_CountMetric):
    """binary precision over hard predictions: true positives / predicted positives (0 when there are none)"""

    def _counts(self, predictions, targets):
        p, t = predictions.reshape(-1) == 1, targets.reshape(-1) == 1
        return (p & t).sum(), p.sum()


class Recall(_CountMetric):
    """binary recall over hard predictions: true positives / positives (0 when there are none)"""

    def _counts(self, predictions, targets):
        p, t = predictions.reshape(-1) == 1, targets.reshape(-1) == 1
        return (p & t).sum(), t.sum()


class Accuracy(_CountMetric):
    """share of hard predictions equal to their target"""

    def _counts(self, predictions, targets):
        p, t = predictions.reshape(-1), targets.reshape(-1)
        return (p == t).sum(), torch.tensor(p.numel(), device=p.device)


class MeanSquaredError(_CountMetric):
    """mean of (prediction - target)^2"""

    def _counts(self, predictions, targets):
        d = predictions.reshape(-1).double() - targets.reshape(-1).double()
        return (d * d).sum(), torch.tensor(d.numel(), device=d.device)


_BINARY_METRICS = (Precision, Recall, Accuracy)


# ------------------------------------------------------------------------------------------------ autograd
class _SessionTaskFn(torch.autograd.Function):
    """x [B, L, D] -> (loss [], predictions [B]); the backward returns the gradient of x and ACCUMULATES the parameter gradients
    into masking._grad_buf (the package's convention); a frozen parameter gets no buffer (NULL)."""

    @staticmethod
    def forward(ctx, x, anchor, task, lengths, target):
        lin = task.pre[0]
        w = lin.weight.detach().view(-1)
        b = lin.bias.detach() if lin.bias is not None else None
        s, pred, loss = ops.seq_task_fwd(x.detach().contiguous(), lengths, w, b, target, task._summary, task._act, task._loss_kind)
        ctx.task, ctx.L, ctx.lengths = task, x.shape[1], lengths
        ctx.save_for_backward(s, pred, target)
        ctx.mark_non_differentiable(pred)
        ctx.set_materialize_grads(False)
        return loss.view(()), pred

    @staticmethod
    def backward(ctx, dloss, _dpred_unused):
        if dloss is None:
            return (None,) * 5
        s, pred, target = ctx.saved_tensors
        task = ctx.task
        lin = task.pre[0]
        d_w = _grad_buf(lin.weight).view(-1) if lin.weight.requires_grad else None
        d_b = _grad_buf(lin.bias) if (lin.bias is not None and lin.bias.requires_grad) else None
        dx = ops.seq_task_bwd_(dloss.contiguous().view(1), pred, target, s, ctx.lengths, ctx.L, lin.weight.detach().view(-1),
                               task._summary, task._act, task._loss_kind, d_w, d_b)
        return dx, None, None, None, None


# ------------------------------------------------------------------------------------------------ tasks
class _SessionTask(nn.Module):
    """what the two tasks share (reference PredictionTask, model/base.py:52-232)"""
    _loss_type = None
    _act = ops.ACT_NONE
    _loss_kind = ops.LOSS_MSE
    _bias = True
    _default_metrics = ()

    def __init__(self, target_name=None, task_name=None, task_block=None, loss=None, metrics=None, summary_type="first",
                 mask_padding=False):
        super().__init__()
        cls = type(self).__name__
        if task_block is not None:
            raise NotImplementedError(f"{cls}(task_block=...) is not on the HIP path: the fused kernels run summary -> "
                                      "Linear(D, 1) -> loss with nothing in between; pass task_block=None")
        loss = self._loss_type() if loss is None else loss
        if type(loss) is not self._loss_type or loss.reduction != "mean" or getattr(loss, "weight", None) is not None:
            raise NotImplementedError(f"{cls}(loss=...) is not on the HIP path: the fused kernels compute "
                                      f"torch.nn.{self._loss_type.__name__}(reduction='mean') without a weight")
        if summary_type == "attn":
            raise NotImplementedError("summary_type='attn' is not implemented (nor is it by transformers' SequenceSummary)")
        if summary_type is None:
            raise NotImplementedError(f"{cls}(summary_type=None) is not on the HIP path: the fused kernels predict one value "
                                      "per session from a summary of the [B, L, D] output")
        if summary_type not in _SUMMARIES:
            raise ValueError(f"summary_type must be one of {sorted(_SUMMARIES)}, got {summary_type!r}")
        self.target_dim = 1
        self.target_name = target_name
        self._task_name = task_name
        self.summary_type = summary_type
        self._summary = _SUMMARIES[summary_type]
        self.mask_padding = bool(mask_padding)
        self.loss = loss
        self.task_block = None
        self.metrics = nn.ModuleList([m() for m in self._default_metrics] if metrics is None else list(metrics))
        self.pre = None
        self.built = False
        self._inputs = None          # the input module (not a submodule: the body owns it), for mask_padding

    @property
    def task_name(self):
        if self._task_name:
            return self._task_name
        base = _snake(type(self).__name__)
        return f"{self.target_name}/{base}" if self.target_name else base

    def child_name(self, name):
        return f"{self.task_name}/{name}"

    def build(self, body=None, input_size=None, inputs=None, device=None, task_block=None, pre=None):
        """Called by the Head / Model (model/base.py:104-150)."""
        if task_block is not None or pre is not None:
            raise NotImplementedError(f"{type(self).__name__}.build(task_block=..., pre=...) is not on the HIP path: "
                                      "the output layer is Linear(D, 1) inside the fused kernels")
        if input_size is None or len(input_size) != 3:
            raise ValueError(f"{type(self).__name__} needs a 3-dim vector as input, found:{input_size}")
        D = int(input_size[-1])
        if not 1 <= D <= 1024:
            raise ValueError(f"{type(self).__name__}: the fused kernels take 1 <= D <= 1024 (got {D})")
        self.pre = nn.Sequential(nn.Linear(D, 1, bias=self._bias))
        object.__setattr__(self, "_inputs", inputs)
        if device is not None:
            self.to(device)
        self.built = True
        return self

    def _lengths(self):
        if not self.mask_padding:
            return None
        cat = getattr(self._inputs, "categorical_module", None)
        if cat is None:
            raise ValueError(f"{type(self).__name__}(mask_padding=True) needs the input module: build the task with `inputs`")
        if cat.item_seq is None:
            raise ValueError("mask_padding needs the input module to have seen the item ids of this batch")
        return ops.session_lengths(cat.item_seq.contiguous(), cat.padding_idx)

    def forward(self, inputs, targets=None, training=False, testing=False, **kwargs):
        """Training / evaluation: {"loss", "labels", "predictions"} with labels the float targets [B] and predictions [B]
        (probabilities for the binary task).  Inference (neither flag): predictions [B]."""
        if self.pre is None:
            raise RuntimeError(f"{type(self).__name__}: the task is not built yet")
        if isinstance(inputs, (tuple, list)):
            inputs = inputs[0]
        x = inputs.float()
        if x.dim() != 3:
            raise NotImplementedError(f"{type(self).__name__}: a [B, L, D] body output is needed (got {tuple(x.shape)}); "
                                      "2-D outputs are not on the HIP path")
        lengths = self._lengths()
        lin = self.pre[0]
        if training or testing:
            if targets is None:
                raise ValueError(f"{self.task_name}: training / testing needs targets"
                                 + (f" (key '{self.target_name}')" if self.target_name else ""))
            labels = targets.detach().float().reshape(-1).contiguous()
            if labels.shape[0] != x.shape[0]:
                raise ValueError(f"{self.task_name}: one target per session is needed ({x.shape[0]}), got {tuple(targets.shape)}")
            loss, pred = _SessionTaskFn.apply(x, lin.weight, self, lengths, labels)
            return {"loss": loss, "labels": labels, "predictions": pred}
        _s, pred, _ = ops.seq_task_fwd(x.detach().contiguous(), lengths, lin.weight.detach().view(-1),
                                       lin.bias.detach() if lin.bias is not None else None, None, self._summary, self._act,
                                       self._loss_kind)
        return pred

    # ------------------------------------------------------------------ metrics
    def forward_to_prediction_fn(self, predictions):
        return predictions

    def metric_name(self, metric):
        return self.child_name(metric if isinstance(metric, str) else _snake(type(metric).__name__))

    def calculate_metrics(self, predictions, targets):
        predictions = self.forward_to_prediction_fn(predictions.detach())
        out = {}
        for metric in self.metrics:
            t = targets.int() if isinstance(metric, _BINARY_METRICS) else targets
            out[self.metric_name(metric)] = metric(predictions, t)
        return out

    def compute_metrics(self, mode=None, **kwargs):
        return {self.metric_name(metric): metric.compute() for metric in self.metrics}

    def reset_metrics(self):
        for metric in self.metrics:
            metric.reset()


class BinaryClassificationTask(_SessionTask):
    """Drop-in for tr.BinaryClassificationTask on the hot path.  mask_padding (beyond the reference's signature, default off =
    the reference's arithmetic): "last" is the last real item and "mean" averages the real positions only."""
    _loss_type = nn.BCELoss
    _act = ops.ACT_SIGMOID
    _loss_kind = ops.LOSS_BCE
    _bias = False
    _default_metrics = (Precision, Recall, Accuracy)

    def forward_to_prediction_fn(self, predictions):
        return torch.round(predictions).int()


class RegressionTask(_SessionTask):
    """Drop-in for tr.RegressionTask on the hot path (mask_padding as BinaryClassificationTask's)."""
    _loss_type = nn.MSELoss
    _act = ops.ACT_NONE
    _loss_kind = ops.LOSS_MSE
    _bias = True
    _default_metrics = (MeanSquaredError,)
