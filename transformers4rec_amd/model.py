"""Thin caller of the hot path: the reference's Model -> Head -> SequentialBlock composition
(transformers4rec/torch/model/base.py:235-425, 544-598; block/base.py:236-262) reduced to one head
-- with one or several prediction tasks, task_weights and loss_reduction --, with the reference's module tree names so
state_dicts interchange:
  heads.0.body.0 (TabularSequenceFeatures), heads.0.body.1 (TransformerBlock) -- or, with mlp_block=, heads.0.body.1 (the built
  MLPBlock, block.py) and heads.0.body.2 (TransformerBlock), the reference's SequentialBlock(inputs, MLPBlock, TransformerBlock),
  heads.0.prediction_task_dict.next-item (NextItemPredictionTask),
  heads.0.prediction_task_dict.<target>/binary_classification_task, .<target>/regression_task (session_task.py).
Rewriting Model/Head/Trainer is out of scope; this exists so the path can
be driven stand-alone (tests, bench) where the reference package is not installed.
"""
from typing import Optional

import torch
from torch import nn

from . import ops


class _Body(nn.ModuleList):
    @property
    def inputs(self):
        return self[0]

    def forward(self, inputs, training=False, testing=False, out_rows=None, **kwargs):
        """out_rows: () -> (rows, n) or None, handed on to the transformer block, which asks it just before its last layer"""
        x = self[0](inputs, training=training, testing=testing)
        if len(self) == 3:          # [inputs, MLP stack, transformer]
            x = self[1](x, training=training)
        return self[-1](x) if out_rows is None else self[-1](x, out_rows=out_rows)


def last_rows_gate(model, training, B, L, n_labels=None):
    """The number of label rows n when the LAST XLNet layer of `model` may run its row-wise half (feed-forward block,
    LayerNorm-1 backward) on the label rows only, else None (every row is computed, as ever).  It may when nothing reads the
    other rows of the body's output and their gradient is exactly zero:
      * a training step with gradients enabled (evaluation and inference compute every row);
      * the XLNet body behind a plain TransformerBlock without mask_padding, nobody hooked onto the body's output;
      * the task is NextItemPredictionTask itself with the tied head: it gathers the rows at the masking module's label
        positions and scatters its gradient to them (prediction_task._NextItemHeadFn) -- a subclass or another head may read
        more;
      * the token-tile kernels and the one-kernel attention forward take the shape;
      * the row rule: n <= transformer._LAST_ROWS_MAX_FRACTION * B * L (CLM training, labels at nearly every position, stays
        on the full path).
    n_labels: the count when the caller has it (tests); default: masking.n_labels(), the 4-byte copy started right after the
    masking kernel -- asked here, just before the last layer is enqueued, instead of at the head."""
    from . import transformer as tfm

    if not (tfm._LAST_ROWS and training and torch.is_grad_enabled()):
        return None
    # this runs on the host's critical path of every training step: the modules and what their classes say are looked up once
    parts = model.__dict__.get("_last_rows_parts")
    if parts is None:
        from .masking import CausalLanguageModeling, MaskedLanguageModeling
        from .prediction_task import NextItemPredictionTask

        block, task, body = model.transformer_block, model.prediction_task, model.heads[0].body
        # a session-level task reads every row of the body's output: the one task of the head must be the next-item task;
        # so does a post-context fusion: the body must be the plain one
        kinds = (type(body) is _Body and len(model.heads[0].prediction_task_dict) == 1 and type(block) is tfm.TransformerBlock and type(block.transformer) is tfm.XLNetModel
                 and type(task) is NextItemPredictionTask and task.masking is not None and task.masking is body[0].masking
                 and type(task.masking) in (MaskedLanguageModeling, CausalLanguageModeling))
        parts = model.__dict__["_last_rows_parts"] = (block, getattr(block, "transformer", None), task, body, kinds, {})   # a GRUBlock has none: kinds is False
    block, xl, task, body, kinds, shapes = parts
    if not kinds or block.mask_padding or not task.weight_tying or not xl.training or not tfm._FUSED_ON:
        return None
    for m in (body, block, xl, task):
        if m._forward_hooks or m._forward_pre_hooks:
            return None
    ok = shapes.get(L)
    if ok is None:
        cfg = xl.config
        ok = shapes[L] = bool(ops.xlnet_fused_supported(cfg.d_model) and ops.xlnet_attn_block_supported(L, cfg.d_model, cfg.n_head))
    if not ok:
        return None
    n = int(task.masking.n_labels() if n_labels is None else n_labels)
    if n < 1 or n > tfm._LAST_ROWS_MAX_FRACTION * B * L:
        return None
    return n


def _block_widths(block):
    """(input width, output width) of the sequence model in the body's last slot: a TransformerBlock or a block.GRUBlock"""
    from .block import GRUBlock

    if isinstance(block, GRUBlock):
        return block.input_size, block.hidden_size
    d_model = int(block.transformer.config.hidden_size)
    return d_model, d_model


class Head(nn.Module):
    """one body, one or several prediction tasks (reference Head, model/base.py:235-425): `prediction_task_dict` keyed by
    task_name in list order, `task_weights` zipped with the tasks (default 1.0), the step's loss
    getattr(torch.stack([loss_i * w_i]), loss_reduction)()"""

    def __init__(self, body: _Body, tasks, task_weights=None, loss_reduction: str = "mean"):
        super().__init__()
        self.body = body
        self.loss_reduction = loss_reduction
        tasks = list(tasks) if isinstance(tasks, (list, tuple)) else [tasks]
        if not tasks:
            raise ValueError("Head needs at least one prediction task")
        self.prediction_task_dict = nn.ModuleDict()
        for task in tasks:
            if task.task_name in self.prediction_task_dict:
                raise ValueError(f"two prediction tasks are named '{task.task_name}': give them a target_name or a task_name")
            self.prediction_task_dict[task.task_name] = task
        self._task_weights = {}
        if task_weights:
            for task, val in zip(tasks, task_weights):
                self._task_weights[task.task_name] = val

    def task_weight(self, name):
        return self._task_weights.get(name, 1.0)


class Model(nn.Module):
    def __init__(self, input_features, transformer_block, prediction_task, max_sequence_length: Optional[int] = None,
                 top_k: Optional[int] = None, exclude_seen: bool = False, task_weights=None, loss_reduction: str = "mean",
                 post_context_module=None, fusion_aggregation: str = "elementwise-mul", mlp_block=None):
        """prediction_task: one task or a list of them (NextItemPredictionTask, BinaryClassificationTask, RegressionTask), all
        over the one body.  post_context_module: context that does not go through the sequence model; the body then is
        experimental.PostContextFusion around [input_features, transformer_block] (state-dict names
        heads.0.body.sequential_module.{0,1}.*, .post_context_module.*, .context_projection.*) and the tasks see its last_dim.
        mlp_block: a block.MLPBlock (built here on input_features.output_size()) or a built one; the body then is
        [input_features, the stack, transformer_block] (state-dict names heads.0.body.1.<i>.0.{weight,bias}, the transformer
        under heads.0.body.2); the input block keeps its own width and the stack's last width must be the transformer's.
        transformer_block: a TransformerBlock, or a block.GRUBlock (the reference's Block(torch.nn.GRU)): the slot keeps its
        name, the widths are the block's input_size / hidden_size, any masking module is accepted"""
        super().__init__()
        d_in, hidden = _block_widths(transformer_block)
        if post_context_module is not None and not hasattr(transformer_block, "transformer"):
            raise NotImplementedError("Model: post_context_module together with a GRUBlock is not supported.")
        if mlp_block is None:
            body = _Body([input_features, transformer_block])
        else:
            from .block import MLPBlock, MLPStack

            if post_context_module is not None:
                raise NotImplementedError("Model: mlp_block together with post_context_module is not supported.")
            stack = mlp_block.build(input_features.output_size()) if isinstance(mlp_block, MLPBlock) else mlp_block
            if not isinstance(stack, MLPStack):
                raise TypeError(f"Model: mlp_block must be a block.MLPBlock or a built one, got {type(mlp_block).__name__}")
            width = int(input_features.output_size()[-1])
            if stack.in_features != width or stack.out_features != d_in:
                raise ValueError(f"Model: mlp_block maps {stack.in_features} -> {stack.out_features} columns, the input block "
                                 f"gives {width} and the transformer takes {d_in}")
            body = _Body([input_features, stack, transformer_block])
        if post_context_module is not None:
            from .experimental import PostContextFusion

            body = PostContextFusion(body, post_context_module, fusion_aggregation)
            hidden = body.last_dim
        tasks = list(prediction_task) if isinstance(prediction_task, (list, tuple)) else [prediction_task]
        for task in tasks:
            task.build(body=body, input_size=(-1, -1, hidden), inputs=input_features)
        self.heads = nn.ModuleList([Head(body, tasks, task_weights=task_weights, loss_reduction=loss_reduction)])
        self.max_sequence_length = max_sequence_length or getattr(input_features, "max_sequence_length", None)
        self.top_k = top_k
        self.exclude_seen = exclude_seen      # inference: drop the session's own items (NextItemPredictionTask.forward)

    @property
    def _sequential(self):
        body = self.heads[0].body
        return body if isinstance(body, _Body) else body.sequential_module

    @property
    def input_features(self):
        return self._sequential[0]

    @property
    def transformer_block(self):
        return self._sequential[-1]

    @property
    def mlp_block(self):
        """the built MLPBlock of a three-entry body, else None"""
        seq = self._sequential
        return seq[1] if len(seq) == 3 else None

    @property
    def prediction_task(self):
        return next(iter(self.heads[0].prediction_task_dict.values()))

    def pad_inputs(self, inputs):
        """pad_inputs (torch/utils/padding.py:126-164): ragged __values/__offsets -> dense [B, L],
        L = min(max_sequence_length, longest row in the batch)."""
        ragged = [k[: -len("__offsets")] for k in inputs if k.endswith("__offsets")]
        if not ragged:
            return inputs
        L = 0
        for n in ragged:
            L = max(L, int(ops.ragged_max_len(inputs[n + "__offsets"].view(-1).contiguous()).item()))
        if self.max_sequence_length is not None:
            L = min(L, self.max_sequence_length)
        out = {k: v for k, v in inputs.items() if not (k.endswith("__offsets") or k.endswith("__values"))}
        for n in ragged:
            out[n] = ops.ragged_to_padded(inputs[n + "__values"].view(-1).contiguous(),
                                          inputs[n + "__offsets"].view(-1).contiguous(), L)
        return out

    def forward(self, inputs, targets=None, training=False, testing=False, **kwargs):
        inputs = {k: (v.to(torch.float32) if torch.is_floating_point(v) else v) for k, v in inputs.items()}
        inputs = self.pad_inputs(inputs)
        head = self.heads[0]

        def out_rows(B, L):
            # the last layer on the label rows only, where nothing reads the others (last_rows_gate); asked by XLNetModel.forward
            # just before it enqueues its last layer: the wait for the label count (masking.n_labels) sits there, not at the head
            n = last_rows_gate(self, training, B, L)
            return None if n is None else (self.prediction_task.masking.compact_labels()[1], n)

        if not self._single_next_item():
            return self._forward_tasks(head, inputs, targets, training, testing)
        h = head.body(inputs, training=training, testing=testing, out_rows=out_rows if training else None)
        task = self.prediction_task
        if training or testing:
            return task(h, targets=targets, training=training, testing=testing)
        return task(h, training=False, testing=False, top_k=self.top_k, exclude_seen=self.exclude_seen)

    def _single_next_item(self):
        """the head holds exactly one task and it is a next-item task: the path this model took before heads had several"""
        single = self.__dict__.get("_single_next_item_cached")      # asked on every forward: looked up once
        if single is None:
            from .prediction_task import NextItemPredictionTask

            tasks = self.heads[0].prediction_task_dict
            single = self.__dict__["_single_next_item_cached"] = (len(tasks) == 1
                                                                  and isinstance(self.prediction_task, NextItemPredictionTask))
        return single

    def _forward_tasks(self, head, inputs, targets, training, testing):
        """reference Head.forward + Model.forward (model/base.py:371-425, 544-598) over the head's tasks: the body runs once,
        every row of its output is computed (a session-level task reads them all)"""
        from .prediction_task import NextItemPredictionTask

        if isinstance(targets, dict) and len(targets) == 0:
            targets = None
        h = head.body(inputs, training=training, testing=testing)
        if training or testing:
            losses, labels, predictions = [], {}, {}
            for name, task in head.prediction_task_dict.items():
                if isinstance(task, NextItemPredictionTask):
                    out = task(h, targets=None, training=training, testing=testing)     # its labels come from the masking
                else:
                    label = targets.get(task.target_name, None) if isinstance(targets, dict) else targets
                    out = task(h, targets=None if label is None else label.float(), training=training, testing=testing)
                labels[name], predictions[name] = out["labels"], out["predictions"]
                losses.append(out["loss"].reshape(()) * head.task_weight(name))
            loss = getattr(torch.stack(losses), head.loss_reduction)()
            if len(labels) == 1:
                labels, predictions = next(iter(labels.values())), next(iter(predictions.values()))
            return {"loss": loss, "labels": labels, "predictions": predictions}
        outputs = {}
        for name, task in head.prediction_task_dict.items():
            if isinstance(task, NextItemPredictionTask):
                outputs[name] = task(h, training=False, testing=False, top_k=self.top_k, exclude_seen=self.exclude_seen)
            else:
                outputs[name] = task(h, training=False, testing=False)
        return next(iter(outputs.values())) if len(outputs) == 1 else outputs

    @property
    def prediction_tasks(self):
        return list(self.heads[0].prediction_task_dict.values())

    def calculate_metrics(self, predictions, targets):
        if len(self.heads[0].prediction_task_dict) == 1:
            return self.prediction_task.calculate_metrics(predictions, targets)
        out = {}
        for name, task in self.heads[0].prediction_task_dict.items():
            out.update(task.calculate_metrics(predictions[name], targets[name]))
        return out

    def compute_metrics(self, mode=None):
        if len(self.heads[0].prediction_task_dict) == 1:
            return self.prediction_task.compute_metrics(mode)
        out = {}
        for task in self.prediction_tasks:
            out.update(task.compute_metrics(mode))
        return out

    def reset_metrics(self):
        for task in self.prediction_tasks:
            task.reset_metrics()
