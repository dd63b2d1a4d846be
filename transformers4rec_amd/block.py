"""MLPBlock: host-side mirror of transformers4rec/torch/block/mlp.py for the hot path -- the dense stack the reference's
examples put between the input block and the transformer,

    body = SequentialBlock(input_module, MLPBlock([d_model]), TransformerBlock(...))      ->      Model(..., mlp_block=MLPBlock([d_model]))

Same constructor arguments; `.build(input_shape)` gives the built stack with the reference's parameter names `<i>.0.weight` and
`<i>.0.bias` (layer i is a DenseBlock whose member 0 is the Linear) initialised as torch.nn.Linear initialises.  Arithmetic:
csrc/mlp_block.hip (include/t4r_hip_mlpblock.h) -- the whole stack is one launch forward and at most three backward; in evaluation
and inference the intermediate activations never reach memory.

On the HIP path: activation torch.nn.ReLU or None, with or without bias, dropout; 1 .. 4 layers, input width <= 1024, layer widths
<= 512.  Everything else (another activation, normalization, filter_features, wider or deeper stacks) raises NotImplementedError.

GRUBlock / Block: the recurrent sequence model of the reference's session-based tutorial,

    tr.Block(torch.nn.GRU(d, d, num_layers=1, batch_first=True), [None, L, d])      ->      Model(inputs, GRUBlock(d, d), task, mlp_block=...)

csrc/gru.hip (include/t4r_hip_gru.h): per layer one product for the input gates of all tokens and ONE launch for the whole time
loop, W_hh resident in registers.  The parameters live under the child `module` with torch.nn.GRU's names.  forward returns the
output tensor [B, L, H] (the reference's Block returns torch.nn.GRU's (output, h_n) tuple, which its task unwraps).
"""
import math

import torch
from torch import nn

from . import ops
from .features import _Linear
from .masking import _grad_buf
from .rng import SeedMixin


class _MLPStackFn(torch.autograd.Function):
    """x [..., K0] -> a_{n-1} [..., N_{n-1}]; the backward returns d x and ACCUMULATES the parameter gradients into
    masking._grad_buf (the package's convention; a frozen parameter gets a scratch buffer) and returns None for them."""

    @staticmethod
    def forward(ctx, x, anchor, stack, drop, save):
        """save: a backward may follow (grad mode was on at the call): every a_i is stored; else only the last one is written"""
        x = x.detach().contiguous()
        Ws, bs = stack._weights(), stack._biases()
        if not save:
            return ops.mlp_stack_fwd(x, Ws, bs, stack.relu, drop)
        acts = ops.mlp_stack_fwd(x, Ws, bs, stack.relu, drop, save_acts=True)
        ctx.stack, ctx.drop = stack, drop
        ctx.save_for_backward(x, *acts)
        return acts[-1]

    @staticmethod
    def backward(ctx, dout):
        x, *acts = ctx.saved_tensors
        stack = ctx.stack
        lins = [dense[0] for dense in stack]
        d_w = [_grad_buf(lin.weight) for lin in lins]
        d_b = [_grad_buf(lin.bias) for lin in lins] if stack.use_bias else None
        dx = ops.mlp_stack_bwd_(dout.contiguous(), x, stack._weights(), acts, stack.relu, ctx.drop, d_w, d_b,
                                want_dx=ctx.needs_input_grad[0])
        return dx, None, None, None, None


class DenseBlock(nn.ModuleList):
    """one layer of the stack: member 0 is the Linear (the reference's DenseBlock, block/mlp.py:90-150, holds the activation and
    the dropout as further members without parameters; here they are the stack's kernel arguments)"""

    def __init__(self, in_features, out_features, use_bias=True):
        super().__init__([_Linear(in_features, out_features, bias=use_bias)])
        self._output_size = out_features

    def _get_name(self):
        return "DenseBlock"

    def forward_output_size(self, input_size):
        return torch.Size(list(input_size[:-1]) + [self._output_size])


class MLPStack(SeedMixin, nn.ModuleList):
    """The built MLPBlock: DenseBlocks `0 .. n-1`.  `_drop_offset` is the stream position of its dropout masks (advanced once per
    training forward; rng.get_rng_state / set_rng_state carry it), `seed` the key (rng.SeedMixin)."""
    _t4r_hip = True         # masking.hip_parameters: every parameter below this module is on the HIP path
    _seed_salt = 8

    def __init__(self, input_shape, dimensions, relu=True, use_bias=True, dropout=None):
        in_width = int(input_shape[-1])
        dims = [int(d) for d in dimensions]
        if not ops.mlp_stack_supported(in_width, dims):
            raise NotImplementedError(f"MLPBlock: the fused stack takes 1 .. {ops.MLP_MAX_LAYERS} layers, an input of 1 .. "
                                      f"{ops.MLP_MAX_K0} columns and layers of 1 .. {ops.MLP_MAX_N} (got {in_width} -> {dims})")
        super().__init__([DenseBlock(k, n, use_bias) for k, n in zip([in_width] + dims[:-1], dims)])
        self.input_size = input_shape
        self.relu, self.use_bias = bool(relu), bool(use_bias)
        self.dropout = float(dropout) if dropout else 0.0
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"MLPBlock: dropout must be in [0, 1), got {dropout}")
        self._drop_offset = 0

    def _weights(self):
        return [dense[0].weight.detach() for dense in self]

    def _biases(self):
        return [dense[0].bias.detach() for dense in self] if self.use_bias else None

    @property
    def in_features(self):
        return self[0][0].in_features

    @property
    def out_features(self):
        return self[-1][0].out_features

    def forward(self, x, training=None, **kwargs):
        """x [..., in_features] fp32 on the GPU -> [..., out_features].  training: default self.training; evaluation and
        dropout in (None, 0) take drop_p = 0"""
        training = self.training if training is None else training
        drop = ops.NO_DROP
        if training and self.dropout > 0:
            self._drop_offset += 1
            drop = (self.dropout, self.seed, self._drop_offset)
        return _MLPStackFn.apply(x, self[0][0].weight, self, drop, torch.is_grad_enabled())

    def _get_name(self):
        return "SequentialBlock"

    def output_size(self, input_size=None):
        return self.forward_output_size(self.input_size if input_size is None else input_size)

    def forward_output_size(self, input_size):
        return torch.Size(list(input_size[:-1]) + [self.out_features])


class MLPBlock:
    """Drop-in for transformers4rec.torch.MLPBlock (block/mlp.py:23-87): the recipe of a dense stack; `build(input_shape)` makes
    the module.  Model(..., mlp_block=MLPBlock(dims)) builds it on the input block's output size."""

    def __init__(self, dimensions, activation=torch.nn.ReLU, use_bias=True, dropout=None, normalization=None, filter_features=None):
        if isinstance(dimensions, int):
            dimensions = [dimensions]
        if activation is not None and activation is not torch.nn.ReLU:
            raise NotImplementedError(f"MLPBlock: activation {activation!r} is off the HIP hot path: the fused stack has "
                                      "torch.nn.ReLU or None.")
        if normalization:
            raise NotImplementedError("MLPBlock: normalization (batch_norm) is off the HIP hot path.")
        if filter_features:
            raise NotImplementedError("MLPBlock: filter_features selects from a dictionary of features; in the body the block "
                                      "takes the input block's one tensor, so it is not supported.")
        self.dimensions = [int(d) for d in dimensions]
        self.activation, self.use_bias, self.dropout = activation, bool(use_bias), dropout
        self.normalization, self.filter_features = None, None

    def build(self, input_shape):
        return MLPStack(input_shape, self.dimensions, relu=self.activation is not None, use_bias=self.use_bias, dropout=self.dropout)


class _GRUFn(torch.autograd.Function):
    """x [B, L, K0] -> h [B, L, H]; the backward returns d x and ACCUMULATES the parameter gradients into masking._grad_buf (as
    _MLPStackFn does) and returns None for them."""

    @staticmethod
    def forward(ctx, x, anchor, block, drop, save):
        """save: a backward may follow (grad mode was on at the call): the gate values are stored; else only the output is"""
        x = x.detach().contiguous()
        w_ih, w_hh, b_ih, b_hh = block._params()
        if not save:
            return ops.gru_fwd(x, w_ih, w_hh, b_ih, b_hh, None, drop)
        out, saved = ops.gru_fwd(x, w_ih, w_hh, b_ih, b_hh, None, drop, save=True)
        ctx.block, ctx.drop = block, drop
        ctx.save_for_backward(x, out, saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out, saved = ctx.saved_tensors
        block = ctx.block
        w_ih, w_hh, _, _ = block._params()
        m, n = block.module, block.num_layers
        grads = [[_grad_buf(getattr(m, f"{name}_l{k}")) for k in range(n)] if have else None
                 for name, have in (("weight_ih", True), ("weight_hh", True), ("bias_ih", block.bias), ("bias_hh", block.bias))]
        dx = ops.gru_bwd_(dout.contiguous(), x, w_ih, w_hh, out, saved, None, ctx.drop, *grads, want_dx=ctx.needs_input_grad[0])
        return dx, None, None, None, None


class _GRUParams(nn.Module):
    """the parameters of a torch.nn.GRU under its names (weight_ih_l{k} [3H, K_k], weight_hh_l{k} [3H, H], bias_ih_l{k},
    bias_hh_l{k} [3H]; gate order r | z | n), created in its order and initialised as it initialises: U(-1/sqrt(H), 1/sqrt(H))"""

    def __init__(self, input_size, hidden_size, num_layers, bias):
        super().__init__()
        stdv = 1.0 / math.sqrt(hidden_size)
        for k in range(num_layers):
            shapes = [("weight_ih", (3 * hidden_size, input_size if k == 0 else hidden_size)), ("weight_hh", (3 * hidden_size, hidden_size))]
            if bias:
                shapes += [("bias_ih", (3 * hidden_size,)), ("bias_hh", (3 * hidden_size,))]
            for name, shape in shapes:
                self.register_parameter(f"{name}_l{k}", nn.Parameter(torch.empty(shape).uniform_(-stdv, stdv)))

    def _get_name(self):
        return "GRU"


class GRUBlock(SeedMixin, nn.Module):
    """A stack of 1 .. 4 GRU layers over a session, batch_first: x [B, L, input_size] -> [B, L, hidden_size].  `dropout` acts
    between the layers in training, as torch.nn.GRU(dropout=) does.  `_drop_offset` is the stream position of its masks (advanced
    once per training forward; rng.get_rng_state / set_rng_state carry it), `seed` the key (rng.SeedMixin).  Every position is
    computed, padded ones included; a right-padded session's real positions do not depend on its padding."""
    _t4r_hip = True         # masking.hip_parameters: every parameter below this module is on the HIP path
    _seed_salt = 9

    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, dropout=0.0):
        super().__init__()
        input_size, hidden_size, num_layers = int(input_size), int(hidden_size), int(num_layers)
        if not (1 <= num_layers <= ops.GRU_MAX_LAYERS and 1 <= input_size <= ops.GRU_MAX_K0 and 1 <= hidden_size <= ops.GRU_MAX_H):
            raise NotImplementedError(f"GRUBlock: the fused recurrence takes 1 .. {ops.GRU_MAX_LAYERS} layers, an input of 1 .. "
                                      f"{ops.GRU_MAX_K0} columns and a hidden width of 1 .. {ops.GRU_MAX_H}: W_hh stays in the "
                                      f"registers of one workgroup (got {input_size} -> {hidden_size} x {num_layers})")
        self.dropout = float(dropout) if dropout else 0.0
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"GRUBlock: dropout must be in [0, 1), got {dropout}")
        self.input_size, self.hidden_size, self.num_layers, self.bias = input_size, hidden_size, num_layers, bool(bias)
        self.module = _GRUParams(input_size, hidden_size, num_layers, self.bias)
        self._drop_offset = 0

    def _params(self):
        m, n = self.module, self.num_layers
        get = lambda name: [getattr(m, f"{name}_l{k}").detach() for k in range(n)]  # noqa: E731
        return get("weight_ih"), get("weight_hh"), get("bias_ih") if self.bias else None, get("bias_hh") if self.bias else None

    def forward(self, x, training=None, out_rows=None, **kwargs):
        """x [B, L, input_size] fp32 on the GPU -> [B, L, hidden_size].  training: default self.training.  out_rows is ignored:
        a recurrence computes every row."""
        training = self.training if training is None else training
        drop = ops.NO_DROP
        if training and self.dropout > 0:
            self._drop_offset += 1
            drop = (self.dropout, self.seed, self._drop_offset)
        return _GRUFn.apply(x, self.module.weight_ih_l0, self, drop, torch.is_grad_enabled())

    def _get_name(self):
        return "Block"

    def output_size(self, input_size=None):
        return self.forward_output_size(input_size if input_size is not None else [-1, -1, self.input_size])

    def forward_output_size(self, input_size):
        return torch.Size(list(input_size[:-1]) + [self.hidden_size])


def Block(module, output_size=None):
    """Drop-in for transformers4rec.torch.Block (block/base.py:87-106) around a recurrent module: a torch.nn.GRU with
    batch_first=True becomes a GRUBlock that carries the module's parameter values (copies of them).  output_size is accepted
    and not needed: the block knows its widths."""
    if not isinstance(module, nn.GRU):
        raise NotImplementedError(f"Block: only torch.nn.GRU has a HIP path here (got {type(module).__name__}); an arbitrary "
                                  "torch module would run off the hot path, and there is no fall-back.")
    if not module.batch_first:
        raise NotImplementedError("Block: torch.nn.GRU(batch_first=False) runs its recurrence over the FIRST axis, which for the "
                                  "[B, L, D] tensor the input block gives is the batch, not the session; build the GRU with "
                                  "batch_first=True.")
    if module.bidirectional:
        raise NotImplementedError("Block: a bidirectional GRU reads the future positions a next-item model must not see.")
    if getattr(module, "proj_size", 0) != 0:
        raise NotImplementedError("Block: torch.nn.GRU(proj_size != 0) is not supported.")
    blk = GRUBlock(module.input_size, module.hidden_size, module.num_layers, module.bias, module.dropout)
    with torch.no_grad():
        for name, p in blk.module.named_parameters():
            p.copy_(getattr(module, name))
    return blk
