"""Replaced-token detection (RTD, the ELECTRA objective; the reference's fourth training scheme: rtd_* arguments of
examples/t4rec_paper_experiments/t4r_paper_repro/transf_exp_args.py:162-195).  The reference library stops at the replacement
draw (masking.ReplacementLanguageModeling.get_fake_tokens); the discriminator's arithmetic is HuggingFace transformers'
ElectraForPreTraining: ElectraDiscriminatorPredictions (dense -> activation -> dense_prediction) and BCEWithLogitsLoss over the
attended positions.

  ReplacedTokenDetectionHead  the head and its loss, with HF's parameter names; csrc/rtd_head.hip (include/t4r_hip_rtd.h):
                              two launches forward, three backward, no [T, D] tensor kept between them
  RTDModel                    generator Model (MLM step, unchanged) -> device-side draw of the replacements from its lazy
                              predictions -> discriminator input block and body on the corrupted ids -> the head;
                              loss = generator_loss_weight * L_gen + discriminator_loss_weight * L_disc

The two passes use different module instances (one forward in flight per instance); with share_item_embeddings the two
input blocks hold the SAME item EmbeddingTable module, whose gradient both backward passes accumulate into.
Not implemented (each raises): rtd_tied_generator, rtd_use_batch_interaction, sample_from_batch with the lazy head, and
autograd-visible gradient mode (masking.enable_autograd_gradients) on an RTDModel.
"""
import torch
from torch import nn

from . import ops
from .masking import ReplacementLanguageModeling, _grad_buf


class _RTDHeadFn(torch.autograd.Function):
    """x [T, D] -> (loss [], logits [T]); the backward returns the gradient of x and ACCUMULATES the parameter gradients into
    masking._grad_buf (the package's convention); a frozen parameter gets no buffer (NULL)."""

    @staticmethod
    def forward(ctx, x, anchor, head, active, labels):
        x = x.detach().contiguous()
        z, n, loss = ops.rtd_head_fwd(x, active, labels, head.dense.weight.detach(), head.dense.bias.detach(),
                                      head.dense_prediction.weight.detach().view(-1), head.dense_prediction.bias.detach(), head._act)
        ctx.head, ctx.active, ctx.labels = head, active, labels
        ctx.save_for_backward(x, z, n)
        ctx.mark_non_differentiable(z)
        ctx.set_materialize_grads(False)
        return loss.view(()), z

    @staticmethod
    def backward(ctx, dloss, _dz_unused):
        if dloss is None:
            return (None,) * 5
        x, z, n = ctx.saved_tensors
        head = ctx.head
        W1, b1, w2, b2 = head.dense.weight, head.dense.bias, head.dense_prediction.weight, head.dense_prediction.bias
        dx = ops.rtd_head_bwd_(dloss.contiguous().view(1), x, ctx.active, ctx.labels, z, n, W1.detach(), b1.detach(),
                               w2.detach().view(-1), head._act,
                               _grad_buf(W1) if W1.requires_grad else None, _grad_buf(b1) if b1.requires_grad else None,
                               _grad_buf(w2).view(-1) if w2.requires_grad else None, _grad_buf(b2) if b2.requires_grad else None)
        return dx, None, None, None, None


class ReplacedTokenDetectionHead(nn.Module):
    """HF ElectraDiscriminatorPredictions + BCEWithLogitsLoss over the active positions, fused.  Parameters as HF's
    (`dense.weight` [D, D], `dense.bias`, `dense_prediction.weight` [1, D], `dense_prediction.bias`): a HF checkpoint of the
    head loads.  Weights N(0, 0.01), biases zero.  No active position: loss 0 and zero gradients (HF: NaN)."""

    def __init__(self, hidden_size, hidden_act="gelu"):
        super().__init__()
        if hidden_act not in ops.RTD_ACT:
            raise ValueError(f"ReplacedTokenDetectionHead: hidden_act must be one of {sorted(ops.RTD_ACT)}, got {hidden_act!r}")
        hidden_size = int(hidden_size)
        if hidden_size % 16 != 0 or not 16 <= hidden_size <= 512:
            raise ValueError(f"ReplacedTokenDetectionHead: the fused kernels take a hidden_size that is a multiple of 16 with "
                             f"16 <= hidden_size <= 512 (got {hidden_size})")
        self.hidden_size, self.hidden_act, self._act = hidden_size, hidden_act, ops.RTD_ACT[hidden_act]
        self.dense = nn.Linear(hidden_size, hidden_size)
        self.dense_prediction = nn.Linear(hidden_size, 1)
        for lin in (self.dense, self.dense_prediction):
            nn.init.normal_(lin.weight, mean=0.0, std=0.01)
            nn.init.zeros_(lin.bias)

    def forward(self, hidden, labels=None, active=None):
        """hidden [B, L, D]; labels bool [B, L] or None; active bool [B, L] or None (every position).
        -> {"loss": mean BCE over the active positions ([] tensor; None without labels), "logits": [B, L]}"""
        if hidden.dim() != 3 or hidden.shape[-1] != self.hidden_size:
            raise ValueError(f"ReplacedTokenDetectionHead: hidden must be [B, L, {self.hidden_size}], got {tuple(hidden.shape)}")
        B, L, D = hidden.shape
        for name, m in (("labels", labels), ("active", active)):
            if m is not None and (tuple(m.shape) != (B, L) or m.dtype != torch.bool):
                raise ValueError(f"ReplacedTokenDetectionHead: {name} must be bool [{B}, {L}], got {m.dtype} {tuple(m.shape)}")
        x = hidden.float().reshape(B * L, D)
        act = None if active is None else active.reshape(-1)
        if labels is None:
            z, _, _ = ops.rtd_head_fwd(x.detach().contiguous(), act, None, self.dense.weight.detach(), self.dense.bias.detach(),
                                       self.dense_prediction.weight.detach().view(-1), self.dense_prediction.bias.detach(), self._act)
            return {"loss": None, "logits": z.view(B, L)}
        loss, z = _RTDHeadFn.apply(x, self.dense.weight, self, act, labels.reshape(-1))
        return {"loss": loss, "logits": z.view(B, L)}


class RTDModel(nn.Module):
    """Generator + discriminator training (ELECTRA) over the hot path.  Training forward: the generator's MLM step, the draw of
    the replacement items from its lazy predictions, the discriminator body over the corrupted ids, the head.  Evaluation
    (testing=True) and inference are the generator Model's, unchanged: next-item metrics are the generator's."""

    def __init__(self, generator, discriminator_inputs, discriminator_block, head=None, generator_loss_weight=1.0,
                 discriminator_loss_weight=50.0, share_item_embeddings=True, rtd_tied_generator=False,
                 rtd_use_batch_interaction=False):
        super().__init__()
        from .features import TabularSequenceFeatures
        from .model import Model
        from .transformer import TransformerBlock

        if rtd_tied_generator:
            raise NotImplementedError("RTDModel(rtd_tied_generator=True) is not on the HIP path: it runs one body instance twice "
                                      "in one step, and an instance holds one forward in flight")
        if rtd_use_batch_interaction:
            raise NotImplementedError("RTDModel(rtd_use_batch_interaction=True) is not implemented")
        if not isinstance(generator, Model) or not generator._single_next_item():
            raise ValueError("RTDModel: the generator must be a Model with exactly one NextItemPredictionTask")
        masking = generator.input_features.masking
        if not isinstance(masking, ReplacementLanguageModeling):
            raise ValueError("RTDModel: the generator's masking must be ReplacementLanguageModeling (masking='rtd'), got "
                             f"{type(masking).__name__}")
        if masking.sample_from_batch:
            raise NotImplementedError("RTDModel: sample_from_batch=True is not on the HIP path (the draw comes from the "
                                      "generator's lazy predictions over the whole catalogue)")
        if not isinstance(discriminator_inputs, TabularSequenceFeatures) or not isinstance(discriminator_block, TransformerBlock):
            raise ValueError("RTDModel: discriminator_inputs must be a TabularSequenceFeatures and discriminator_block a "
                             "TransformerBlock")
        if discriminator_inputs.masking is not None:
            raise ValueError("RTDModel: discriminator_inputs must have masking=None (the discriminator sees every token)")
        if discriminator_block.masking is not None or discriminator_block.mask_padding:
            raise ValueError("RTDModel: discriminator_block must have no masking module and mask_padding=False")
        gen_cat, disc_cat = generator.input_features.categorical_module, discriminator_inputs.categorical_module
        if disc_cat.item_id != gen_cat.item_id:
            raise ValueError(f"RTDModel: the two input blocks must name the same item-id column (got {gen_cat.item_id!r} and "
                             f"{disc_cat.item_id!r})")
        hidden = discriminator_block.transformer.config.hidden_size
        head = ReplacedTokenDetectionHead(hidden) if head is None else head
        if not isinstance(head, ReplacedTokenDetectionHead) or head.hidden_size != hidden:
            raise ValueError(f"RTDModel: head must be a ReplacedTokenDetectionHead of the discriminator's hidden size {hidden}")
        if share_item_embeddings:
            g_tab, d_tab = gen_cat.item_embedding_table, disc_cat.item_embedding_table
            if g_tab.embedding_dim != d_tab.embedding_dim or g_tab.num_embeddings != d_tab.num_embeddings:
                raise ValueError("RTDModel(share_item_embeddings=True): the two item tables differ in shape "
                                 f"({g_tab.num_embeddings} x {g_tab.embedding_dim} and {d_tab.num_embeddings} x "
                                 f"{d_tab.embedding_dim}); give both the same embedding dim or pass share_item_embeddings=False")
            disc_cat.embedding_tables[disc_cat.item_id] = g_tab
        self.generator = generator
        self.discriminator_inputs = discriminator_inputs
        self.discriminator_block = discriminator_block
        self.head = head
        self.generator_loss_weight = float(generator_loss_weight)
        self.discriminator_loss_weight = float(discriminator_loss_weight)
        self.share_item_embeddings = bool(share_item_embeddings)

    def forward(self, inputs, targets=None, training=False, testing=False, **kwargs):
        gen = self.generator
        if not training:
            return gen(inputs, targets=targets, training=training, testing=testing, **kwargs)
        for block in (gen.input_features, self.discriminator_inputs):
            if block.__dict__.get("_t4r_carrier_params"):
                raise NotImplementedError("RTDModel: autograd-visible gradient mode (enable_autograd_gradients) is not supported: "
                                          "the second input block's forward would release the first pass's gradient carriers")
        inputs = {k: (v.to(torch.float32) if torch.is_floating_point(v) else v) for k, v in inputs.items()}
        inputs = gen.pad_inputs(inputs)
        out = gen(inputs, targets=targets, training=True, **kwargs)
        masking = gen.input_features.masking
        cat = gen.input_features.categorical_module
        item_seq = cat.item_seq
        corrupted, disc_labels, _ = masking.get_fake_tokens(item_seq, masking.masked_targets.flatten(), out["predictions"])
        d_inputs = dict(inputs)
        d_inputs[cat.item_id] = corrupted
        h = self.discriminator_block(self.discriminator_inputs(d_inputs, training=True))
        d_out = self.head(h, labels=disc_labels, active=item_seq != cat.padding_idx)
        g_loss, d_loss = out["loss"], d_out["loss"]
        return {"loss": self.generator_loss_weight * g_loss + self.discriminator_loss_weight * d_loss,
                "generator_loss": g_loss, "discriminator_loss": d_loss, "labels": out["labels"], "predictions": out["predictions"],
                "discriminator_logits": d_out["logits"], "discriminator_labels": disc_labels}

    def calculate_metrics(self, predictions, targets):
        return self.generator.calculate_metrics(predictions, targets)

    def compute_metrics(self, mode=None):
        return self.generator.compute_metrics(mode)

    def reset_metrics(self):
        self.generator.reset_metrics()
