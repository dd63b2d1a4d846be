"""Flat parameter / gradient buffers and the fused Adam / AdamW step with global-norm clipping.

The reference trains with torch.optim.Adam (Model.fit, transformers4rec/torch/model/base.py:
669-718) and lets torch DDP bucket the gradients.  On MI355X every parameter lives in one of
two flat fp32 buffers -- "dense" (everything but the embedding tables) and "tables" -- so that
  * the Adam update is ONE launch per buffer (csrc/elementwise.hip adam_kernel),
  * the data-parallel exchange is ONE RCCL all-reduce per buffer (distributed.py),
  * XLNet's q,k,v weights are adjacent and go through one batched GEMM.
`nn.Parameter.data` / `.grad` become views into the flat buffers; names and shapes are untouched.
"""
import torch

from . import ops


class FlatParams:
    def __init__(self, named_params, align=4):
        params = []
        seen = set()
        for name, p in named_params:
            if id(p) in seen or not p.requires_grad:
                continue
            seen.add(id(p))
            params.append((name, p))
        if not params:
            raise ValueError("no parameters to flatten")
        dev = params[0][1].device
        offs, n = [], 0
        for _, p in params:
            offs.append(n)
            n += (p.numel() + align - 1) // align * align
        self.data = torch.zeros(n, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(n, device=dev, dtype=torch.float32)
        self.entries = []
        for (name, p), o in zip(params, offs):
            view = self.data[o: o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p.grad = self.grad[o: o + p.numel()].view(p.shape)
            self.entries.append((name, p, o))
        self.numel = n

    def ensure_grads(self):
        """Re-attach .grad views (e.g. after zero_grad(set_to_none=True))."""
        for _, p, o in self.entries:
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                g = self.grad[o: o + p.numel()].view(p.shape)
                if p.grad is not None:
                    g.copy_(p.grad)
                p.grad = g


def flatten_model(model):
    """-> (dense FlatParams, tables FlatParams or None).  Embedding tables (and an untied output
    layer) form their own bucket: they dominate the bytes."""
    dense, tables = [], []
    for name, p in model.named_parameters():
        is_table = (".embedding_tables." in name and name.endswith(".weight") and p.ndim == 2
                    and "continuous_module" not in name) or name.endswith("output_layer")
        (tables if is_table else dense).append((name, p))
    return FlatParams(dense), (FlatParams(tables) if tables else None)


def warmup_schedule(name, num_warmup_steps, num_training_steps=None, num_cycles=0.5):
    """-> f(step) -> learning-rate multiplier: the lambdas of transformers.optimization.get_constant_schedule_with_warmup /
    get_linear_schedule_with_warmup / get_cosine_schedule_with_warmup, which the reference's Trainer.get_scheduler
    (transformers4rec/torch/trainer.py:259-313) hands to LambdaLR.  `step` counts the optimizer steps already taken."""
    import math

    if name not in ("constant_with_warmup", "linear", "cosine"):
        raise ValueError(f"unknown schedule '{name}': constant_with_warmup, linear or cosine")
    if num_warmup_steps is None:
        raise ValueError(f"{name} requires num_warmup_steps")
    if name != "constant_with_warmup" and num_training_steps is None:
        raise ValueError(f"{name} requires num_training_steps")
    w, T = num_warmup_steps, num_training_steps

    def f(step):
        if name == "constant_with_warmup":
            return float(step) / float(max(1.0, w)) if step < w else 1.0
        if step < w:
            return float(step) / float(max(1, w))
        if name == "linear":
            return max(0.0, float(T - step) / float(max(1, T - w)))
        progress = float(step - w) / float(max(1, T - w))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))

    return f


class FusedAdam:
    """torch.optim.Adam semantics over FlatParams buffers; zeroes the gradients in the same pass.

    decoupled_weight_decay=True makes it torch.optim.AdamW; max_grad_norm clips the global norm of the (grad_scale-d) gradient
    over all buckets as torch.nn.utils.clip_grad_norm_ does, with the norm and the coefficient left on the device.  The
    reference's Trainer recipe (AdamW, max_grad_norm 1.0, warm-up) is
        FusedAdam(flats, lr, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0) + set_schedule(warmup_schedule(...)).
    With both new arguments at their defaults step() launches exactly what it always has.

    link(opt_s) hands it a RowSparseAdam whose tables this optimizer steps WITH its buckets -- the linked pair,
        opt_d = FusedAdam([dense], lr, ..., max_grad_norm=1.0).link(opt_s)
    (a method, as set_schedule: the constructor's parameter list is as it was).  One step() then steps both, and with max_grad_norm the norm is the global one, over the buckets and over the rows the tables received
    (csrc/row_adam.hip, include/t4r_hip_rowclip.h): the sum of squares of every bucket, then of every table's summed rows
    (ops.row_adam_reduce_: the non-zero rows of the dense gradient clip_grad_norm_ would have seen, bit for bit), ONE coefficient,
    the buckets' steps, the tables' steps (ops.row_adam_apply_) with the same device coefficient; last_grad_norm is the joint
    norm.  The RowSparseAdam keeps its own step count, schedule, hyper-parameters and state_dict; calling its step() directly
    raises.  Without max_grad_norm the linked pair runs the two unclipped paths: the bits of stepping the two objects one after the other.
    Data parallel needs no further collective: after GradReducer.reduce_all the buckets are equal on every rank and, with
    SparseRowExchange(apply_fn=opt_s.add_rows), every rank holds the same concatenation of (ids, rows) -- no float atomics
    anywhere, so every rank computes the same partials and the same coefficient bits.  The linked step() must therefore run
    AFTER reduce_all."""

    def __init__(self, flats, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 decoupled_weight_decay=False):
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be greater than 0 (or None: no clipping), got {max_grad_norm}")
        self.flats = [f for f in flats if f is not None]
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm, self.decoupled_weight_decay = max_grad_norm, bool(decoupled_weight_decay)
        self.base_lr, self._schedule = lr, None
        self.state = [(torch.zeros_like(f.data), torch.zeros_like(f.data)) for f in self.flats]
        self.step_count = 0
        # clipping: the partial sums of squares of every bucket (and of every linked table) side by side, and (norm,
        # coefficient); allocated at the first clipped step (the partial counts come from the library) and, with linked tables,
        # grown when a step's lookups need more: their count depends on n
        self._clip_part = self._clip_out = None
        self.row_sparse = None                         # the linked RowSparseAdam (link()); not state: no state_dict carries it
        # per bucket: (parameter, offset, partial-maxima buffer) of its largest 2-D table on the GPU, or None
        self._amax_targets = []
        for f in self.flats:
            tabs = [(p.numel(), p, o) for name, p, o in f.entries if p.ndim == 2 and ".embedding_tables." in name and "continuous_module" not in name and f.data.is_cuda]
            if tabs:
                _, p, o = max(tabs, key=lambda t: t[0])
                self._amax_targets.append((p, o, torch.zeros(1024, device=f.data.device, dtype=torch.float32)))
            else:
                self._amax_targets.append(None)

    @staticmethod
    def _join():
        # weight-gradient streams a failed backward pass left unjoined (transformer.py; no-op normally)
        from .transformer import _join_weight_gradient_streams
        _join_weight_gradient_streams()

    def link(self, row_sparse):
        """row_sparse: the RowSparseAdam this optimizer steps with its buckets from now on (see the class docstring).  One
        RowSparseAdam per FusedAdam and one FusedAdam per RowSparseAdam.  -> self"""
        if not isinstance(row_sparse, RowSparseAdam):
            raise TypeError(f"link: expected a RowSparseAdam, got {type(row_sparse).__name__}")
        if row_sparse._linked not in (None, self) or self.row_sparse not in (None, row_sparse):
            raise RuntimeError("link: one of the two optimizers is already linked to another")
        self.row_sparse, row_sparse._linked = row_sparse, self
        return self

    def set_schedule(self, f):
        """f(step) -> multiplier of the constructor's lr (warmup_schedule); None: constant.  The step that makes step_count == t
        runs at base_lr * f(t - 1): a torch scheduler is stepped AFTER the optimizer, so its first step runs at f(0)."""
        self._schedule = f
        return self

    @property
    def last_grad_norm(self):
        """0-d device tensor: the norm of the scaled gradient over all buckets (and the linked tables' rows) BEFORE the clip of the last step; None when
        clipping is off or no step was taken.  Reading it synchronises the caller, not step()."""
        return None if self._clip_out is None else self._clip_out[0]

    def step(self, grad_scale=1.0):
        self._join()
        self.step_count += 1
        if self._schedule is not None:
            self.lr = self.base_lr * self._schedule(self.step_count - 1)
        rs = self.row_sparse
        if rs is not None:
            rs._advance()
        if self.max_grad_norm is not None or self.decoupled_weight_decay:
            return self._step_ext(grad_scale)
        self._step_plain(grad_scale)
        if rs is not None:
            rs._step_tables(grad_scale)

    def _step_plain(self, grad_scale):
        for k, (f, (m, v)) in enumerate(zip(self.flats, self.state)):
            f.ensure_grads()
            tgt = self._amax_targets[k]
            if tgt is None:
                ops.adam_step_(f.data, f.grad, m, v, self.step_count, self.lr, self.betas, self.eps,
                               self.weight_decay, grad_scale, zero_grad=True)
                continue
            # the bucket's largest table (the tied item table of a next-item model): its maximum after the update comes out
            # of this launch, for the head of the NEXT step (ops.w_amax_of checks that nothing wrote the table in between)
            p, lo, part = tgt
            n = ops.adam_step_amax_(f.data, f.grad, m, v, self.step_count, lo, lo + p.numel(), part, self.lr, self.betas, self.eps,
                                    self.weight_decay, grad_scale, zero_grad=True)
            p._t4r_w_amax = (part, n, p.data_ptr(), p._version, f.data, f.data._version)

    def _step_ext(self, grad_scale):
        """sum of squares per bucket (and per linked table) -> one coefficient launch -> one t4r_adamw_step per bucket (and one
        t4r_row_adam_apply per table)"""
        for f in self.flats:
            f.ensure_grads()
        rs = self.row_sparse
        coef, reduced = None, None
        if self.max_grad_norm is not None:
            tables = rs._take_pending() if rs is not None else []
            need = (sum(ops.grad_sumsq_parts(f.numel) for f in self.flats)
                    + sum(ops.row_grad_sumsq_parts(ids.numel(), p.shape[1]) for p, _, _, ids, _, _ in tables))
            dev = self.flats[0].data.device
            if self._clip_part is None or self._clip_part.numel() < need:
                self._clip_part = torch.zeros(need, device=dev, dtype=torch.float64)
            if self._clip_out is None:
                self._clip_out = torch.zeros(2, device=dev, dtype=torch.float32)
            n_part = 0
            for f in self.flats:
                n_part += ops.grad_sumsq_(f.grad, self._clip_part[n_part:])
            reduced = []
            for p, m, v, ids, rows, pad in tables:
                k, st = ops.row_adam_reduce_(ids, rows, p.shape[0], pad, self._clip_part[n_part:])
                n_part += k
                reduced.append((p, m, v, st))
            ops.grad_clip_coef_(self._clip_part, n_part, grad_scale, self.max_grad_norm, self._clip_out)
            coef = self._clip_out[1:]
        for k, (f, (m, v)) in enumerate(zip(self.flats, self.state)):
            tgt = self._amax_targets[k]
            amax = None if tgt is None else (tgt[1], tgt[1] + tgt[0].numel(), tgt[2])
            n = ops.adamw_step_(f.data, f.grad, m, v, self.step_count, self.lr, self.betas, self.eps, self.weight_decay,
                                self.decoupled_weight_decay, grad_scale, zero_grad=True, clip_coef=coef, amax=amax)
            if tgt is not None:       # as step(): the table's maximum after the update, for the head of the next step
                p = tgt[0]
                p._t4r_w_amax = (tgt[2], n, p.data_ptr(), p._version, f.data, f.data._version)
        if rs is None:
            return
        if reduced is None:                             # decoupled weight decay without a clip: the unclipped lazy step
            return rs._step_tables(grad_scale)
        for p, m, v, st in reduced:
            ops.row_adam_apply_(p.data, m, v, st, rs.step_count, rs.lr, rs.betas, rs.eps, rs.weight_decay,
                                rs.decoupled_weight_decay, grad_scale, clip_coef=coef)
            rs._wrote(p)

    def state_dict(self):
        """moments per bucket (copies), step count and hyper-parameters; a schedule is code and is set again by the caller"""
        return {"step_count": self.step_count,
                "state": [{"exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()} for m, v in self.state],
                "hyper": {"lr": self.base_lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                          "max_grad_norm": self.max_grad_norm, "decoupled_weight_decay": self.decoupled_weight_decay}}

    def load_state_dict(self, sd):
        if len(sd["state"]) != len(self.state):
            raise ValueError(f"state_dict has {len(sd['state'])} buckets, the optimizer {len(self.state)}")
        for (m, v), s in zip(self.state, sd["state"]):
            if s["exp_avg"].shape != m.shape or s["exp_avg_sq"].shape != v.shape:
                raise ValueError("state_dict bucket sizes do not match the optimizer's")
        h = sd["hyper"]
        if h["max_grad_norm"] is not None and not h["max_grad_norm"] > 0:
            raise ValueError("max_grad_norm must be greater than 0")
        for (m, v), s in zip(self.state, sd["state"]):
            m.copy_(s["exp_avg"])
            v.copy_(s["exp_avg_sq"])
        self.step_count = int(sd["step_count"])
        self.base_lr = self.lr = h["lr"]
        self.betas, self.eps, self.weight_decay = tuple(h["betas"]), h["eps"], h["weight_decay"]
        self.max_grad_norm, self.decoupled_weight_decay = h["max_grad_norm"], bool(h["decoupled_weight_decay"])

    def zero_grad(self):
        self._join()
        for f in self.flats:
            f.grad.zero_()


def _is_table(name, p):
    return ((".embedding_tables." in name and name.endswith(".weight") and p.ndim == 2 and "continuous_module" not in name)
            or name.endswith("output_layer"))


def row_sparse_tables(model):
    """-> [(name, param)]: the tables of `model` (flatten_model's "tables" bucket) whose whole gradient arrives as (ids, rows)
    and which RowSparseAdam may therefore step.  With a sampled-softmax head that is every table.  A full-softmax head writes
    a dense d W into its weight's .grad -- the tied item table, or an untied output_layer -- and that one is left out."""
    task = model.prediction_task
    dense_w = None
    if not getattr(task, "sampled_softmax", False):
        dense_w = task.pre.module.output_weights
    out, seen = [], set()
    for name, p in model.named_parameters():
        if id(p) in seen or not p.requires_grad or not _is_table(name, p) or p is dense_w:
            continue
        seen.add(id(p))
        out.append((name, p))
    return out


class RowSparseAdam:
    """torch.optim.SparseAdam semantics for embedding tables whose gradient arrives as (ids, rows): one step reads and writes
    only the rows that have a gradient (csrc/row_adam.hip), so neither a dense [V, D] gradient nor a pass over the table exists.

    "Lazy": a row without a gradient keeps its parameters and its moments -- they do not decay -- while the bias corrections use
    the global step count; weight_decay (coupled, or decoupled with decoupled_weight_decay=True) applies to touched rows only.
    A dense Adam step agrees with it exactly while the untouched rows' moments are zero (the first step; always for rows never
    seen), and moves a row seen earlier a little further on its decaying first moment where this one leaves it alone.

    The object is the sink of its tables: attach() routes the HIP backward of every table (features._table_scatter, the sampled
    head) here instead of into .grad.  A table that also receives a DENSE gradient -- the weight of a full-softmax head -- cannot
    be stepped lazily; row_sparse_tables(model) names the ones that can.  The recipe:

        sparse = dict(optim.row_sparse_tables(model))
        dense = optim.FlatParams((n, p) for n, p in model.named_parameters() if n not in sparse)
        opt_d = optim.FusedAdam([dense], lr)
        opt_s = optim.RowSparseAdam(sparse.values(), lr).attach()
        ... loss.backward(); opt_d.step(); opt_s.step()

    or, linked, for the reference's Trainer recipe (AdamW, max_grad_norm over ALL parameters):

        opt_s = optim.RowSparseAdam(sparse.values(), lr, weight_decay=0.01, decoupled_weight_decay=True).attach()
        opt_d = optim.FusedAdam([dense], lr, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0).link(opt_s)
        ... loss.backward(); opt_d.step()               # steps both; opt_s.step() raises while linked

    Gradient clipping: FusedAdam(max_grad_norm=).link(this optimizer) clips the global norm over the dense buckets and
    these tables' rows together, with one device coefficient (see FusedAdam); under data parallel that step runs after
    GradReducer.reduce_all, which delivers the exchanged rows here.  Clipping by value is out of scope.

    params: 2-D fp32 contiguous parameters on the GPU (views into a FlatParams buffer are fine).  Several entries for one table in one step (a tied sampled head's rows and the lookups' rows) are summed as
    ONE list in arrival order; the dense route sums each scatter on its own and adds the sums, so a row that several entries
    name can differ from it in the last bits of its gradient."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False):
        self.params = []
        for p in params:
            if any(p is q for q in self.params):
                continue
            if p.ndim != 2 or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("RowSparseAdam: every parameter is a 2-D fp32 contiguous table")
            self.params.append(p)
        if not self.params:
            raise ValueError("no tables to step")
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        self.base_lr, self._schedule = lr, None
        self.state = [(torch.zeros_like(p.data), torch.zeros_like(p.data)) for p in self.params]
        self.step_count = 0
        self._pending = []
        self._linked = None                        # the FusedAdam that steps these tables (FusedAdam.link), if any

    # ---- the sink (distributed.SparseRowExchange has the same three)
    def attach(self):
        for p in self.params:
            sink = getattr(p, "_t4r_sparse_sink", None)
            if sink is not None and sink is not self:
                raise RuntimeError("RowSparseAdam.attach: the table already has a row-sparse sink; detach that one first (for data "
                                   "parallel, keep the SparseRowExchange attached and hand it this optimizer's add_rows as apply_fn)")
        for p in self.params:
            p._t4r_sparse_sink = self
        return self

    def detach(self):
        for p in self.params:
            if getattr(p, "_t4r_sparse_sink", None) is self:
                del p._t4r_sparse_sink
        return self

    def add(self, tab, ids, grad_rows, col, dim, ids_div, padding_idx):
        """lookup scatter of one feature (called from the backward pass): as SparseRowExchange.add"""
        from .distributed import lookup_rows

        self.add_rows(tab, ids.reshape(-1), lookup_rows(ids, grad_rows, col, dim, ids_div), padding_idx)

    def add_rows(self, tab, ids, rows, padding_idx=-1):
        if not any(tab is p for p in self.params):
            raise ValueError("RowSparseAdam.add_rows: not a table of this optimizer")
        self._pending.append((tab, ids.reshape(-1), rows, int(padding_idx)))

    # ---- the optimizer
    def set_schedule(self, f):
        """as FusedAdam.set_schedule"""
        self._schedule = f
        return self

    def step(self, grad_scale=1.0):
        if self._linked is not None:
            raise RuntimeError("RowSparseAdam.step: this optimizer is linked to a FusedAdam (link()); the pair is stepped "
                               "through the FusedAdam's step()")
        FusedAdam._join()
        self._advance()
        self._step_tables(grad_scale)

    def _advance(self):
        self.step_count += 1
        if self._schedule is not None:
            self.lr = self.base_lr * self._schedule(self.step_count - 1)

    def _take_pending(self):
        """-> [(param, exp_avg, exp_avg_sq, ids, rows, padding_idx)]: one entry per table that received rows since the last
        step, in table order; the pending list is empty afterwards"""
        pending, self._pending = self._pending, []
        out = []
        for p, (m, v) in zip(self.params, self.state):
            mine = [(ids, rows, pad) for tab, ids, rows, pad in pending if tab is p]
            if not mine:
                continue
            if len(mine) == 1:
                ids, rows, pad = mine[0]
            else:
                # one list in arrival order.  Entries that disagree on the padding id: each one's padding lookups get the
                # out-of-range id V, which carries nothing
                pads = {pad for _, _, pad in mine}
                pad = pads.pop() if len(pads) == 1 else -1
                V = p.shape[0]
                ids = torch.cat([i if (q == pad or q < 0) else torch.where(i == q, torch.full_like(i, V), i) for i, _, q in mine])
                rows = torch.cat([r for _, r, _ in mine])
            out.append((p, m, v, ids, rows, pad))
        return out

    @staticmethod
    def _wrote(p):
        # the kernel wrote the table behind torch's version counter: a maximum FusedAdam left for the head is stale now
        if hasattr(p, "_t4r_w_amax"):
            del p._t4r_w_amax

    def _step_tables(self, grad_scale):
        for p, m, v, ids, rows, pad in self._take_pending():
            ops.row_adam_step_(p.data, m, v, ids, rows, self.step_count, self.lr, self.betas, self.eps, self.weight_decay,
                               self.decoupled_weight_decay, grad_scale, padding_idx=pad)
            self._wrote(p)

    def zero_grad(self):
        """drops the rows collected since the last step"""
        FusedAdam._join()
        self._pending = []

    def state_dict(self):
        """moments per table (copies), step count and hyper-parameters; a schedule is code and is set again by the caller"""
        return {"step_count": self.step_count,
                "state": [{"exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()} for m, v in self.state],
                "hyper": {"lr": self.base_lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
                          "decoupled_weight_decay": self.decoupled_weight_decay}}

    def load_state_dict(self, sd):
        if len(sd["state"]) != len(self.state):
            raise ValueError(f"state_dict has {len(sd['state'])} tables, the optimizer {len(self.state)}")
        for (m, v), s in zip(self.state, sd["state"]):
            if s["exp_avg"].shape != m.shape or s["exp_avg_sq"].shape != v.shape:
                raise ValueError("state_dict table shapes do not match the optimizer's")
        for (m, v), s in zip(self.state, sd["state"]):
            m.copy_(s["exp_avg"])
            v.copy_(s["exp_avg_sq"])
        h = sd["hyper"]
        self.step_count = int(sd["step_count"])
        self.base_lr = self.lr = h["lr"]
        self.betas, self.eps, self.weight_decay = tuple(h["betas"]), h["eps"], h["weight_decay"]
        self.decoupled_weight_decay = bool(h["decoupled_weight_decay"])
