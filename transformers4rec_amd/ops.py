"""Thin functional layer over the C ABI (include/t4r_hip.h): tensor checks, output allocation
with the torch caching allocator, launch on torch's current HIP stream.  No arithmetic happens
here and nothing falls back to torch ops: a missing library raises (see _lib.load).
"""
import ctypes

import torch

from . import _lib
from ._lib import call, int_array, long_array, ptr_array

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RELU, EPI_BIAS_RESID = 0, 1, 2, 3, 4
AGG = {"concat": 0, "element-wise-sum": 1, "element-wise-sum-item-multi": 2}
MASK_NONE, MASK_MLM, MASK_CLM, MASK_CLM_INFER = 0, 1, 2, 3
MLM_TRAIN, MLM_EVAL_LAST, MLM_EVAL_ALL, MLM_INFER, CLM_TRAIN, CLM_LAST, CLM_INFER = range(7)


_GPU_OK = False


def _stream():
    global _GPU_OK
    if not _GPU_OK:
        if not torch.cuda.is_available():
            raise _lib.T4RHipError("no GPU visible to torch: the HIP path cannot run and there is no CPU path")
        _GPU_OK = True
    return torch.cuda.current_stream().cuda_stream


def _chk(t, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise _lib.T4RHipError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.data_ptr()


def _p(t, dtype=None, name="tensor"):
    return None if t is None else _chk(t, dtype, name)


_LD_ALIGN = int(_lib.exp_env("T4R_LOGITS_LD_ALIGN", "64"))


def pad_ld(V):
    """leading dimension used for [N, V] logits: rows start on a 256-byte boundary, so the 128-byte
    row segments the GEMM epilogue stores (and the CE / backward kernels read) never straddle a cache line"""
    return (V + _LD_ALIGN - 1) // _LD_ALIGN * _LD_ALIGN


def _row_pitch(t, single):
    """row pitch (elements) of the 2-D tensor t for the C ABI; a one-row tensor's stride(0) is arbitrary: `single` stands in"""
    return t.stride(0) if t.shape[0] > 1 else single


# ------------------------------------------------------------------------------------ GEMM
PRECISIONS = {"fp32": 0, "fp32_bf16x3": 1, "bf16": 2, "fp16": 3, "auto": 4}


def set_precision(mode):
    """precision of every dense contraction launched from now on (include/t4r_hip.h: t4r_set_precision):
    "fp32" (fp32 matrix cores) | "fp32_bf16x3" (fp32-accurate on the bf16 cores, exact 3-way split) |
    "bf16" / "fp16" (mixed precision as the reference's AMP: half operands, fp32 accumulation, fp32 master
    weights) | "auto" (default: fp32 accuracy, the split form where it is faster).  Returns the previous mode."""
    prev = get_precision()
    _lib.load().t4r_set_precision(PRECISIONS[mode] if isinstance(mode, str) else int(mode))
    return prev


def get_precision():
    m = _lib.load().t4r_get_precision()
    return next(k for k, v in PRECISIONS.items() if v == m)


class precision:
    """with ops.precision("bf16"): ...  (restores the previous mode)"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = set_precision(self.mode)

    def __exit__(self, *exc):
        set_precision(self.prev)


def gemm(a, b, trans_a=False, trans_b=False, alpha=1.0, bias=None, epilogue=EPI_NONE, out=None,
         aux=None, splitk=1, accumulate=False, ldc=None, drop=(0.0, 0, 0)):
    """out[M,N] = alpha * op(a) @ op(b) (+epilogue).  a, b 2-D row-major fp32."""
    for t, name in ((a, "a"), (b, "b"), (out, "out"), (aux, "aux")):
        if t is not None and not t.is_cuda:     # (strided views are fine here: _chk would demand contiguity)
            raise _lib.T4RHipError(f"gemm: {name} must be a HIP device tensor (got {t.device}); there is no CPU path")
    M = a.shape[1] if trans_a else a.shape[0]
    K = a.shape[0] if trans_a else a.shape[1]
    N = b.shape[0] if trans_b else b.shape[1]
    Kb = b.shape[1] if trans_b else b.shape[0]
    if K != Kb:
        raise ValueError(f"gemm: inner dims differ ({K} vs {Kb})")
    lda, ldb = a.stride(0), b.stride(0)
    if a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError("gemm: operands must be row-major with unit inner stride")
    if out is None:
        ldc = N if ldc is None else ldc
        buf = torch.empty((M, ldc), device=a.device, dtype=torch.float32)
        out = buf[:, :N]
    ldc = out.stride(0)
    call("t4r_gemm_f32", _stream(), int(trans_a), int(trans_b), M, N, K, float(alpha),
         a.data_ptr(), lda, b.data_ptr(), ldb, out.data_ptr(), ldc,
         _p(bias, torch.float32, "bias"), int(epilogue),
         None if aux is None else aux.data_ptr(), 0 if aux is None else aux.stride(0),
         int(splitk), int(accumulate), 1, 0, 0, 0, float(drop[0]), int(drop[1]), int(drop[2]))
    return out


def gemm_wgrad(a, b, out):
    """out[M, N] += a[K, M]^T @ b[K, N] over a long K (a weight gradient: K = tokens) with DETERMINISTIC split-K: the partial
    tiles go to a scratch buffer and one more launch adds them in split order (include/t4r_hip.h: t4r_gemm_wgrad_f32, one
    call that keeps nothing armed) instead of fp32 atomics in arrival order.  Needs a dense `out`; otherwise plain
    gemm(splitk=-1).  The scratch is sized by the launcher's own query; if the product still finds no room there, it uses
    atomics and this function warns."""
    M, N, K = a.shape[1], b.shape[1], a.shape[0]
    if not (out.is_contiguous() and (M * N) % 4 == 0 and out.data_ptr() % 16 == 0):
        return gemm(a, b, True, False, splitk=-1, accumulate=True, out=out)
    if not (a.is_cuda and b.is_cuda and out.is_cuda):
        raise _lib.T4RHipError("gemm_wgrad: a, b and out must be HIP device tensors; there is no CPU path")
    if b.shape[0] != K or a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError(f"gemm_wgrad: operands must be row-major [K, M] and [K, N] with unit inner stride (K {K} vs {b.shape[0]})")
    ws = torch.empty(_gemm_wgrad_ws_floats(M, N, K), device=a.device, dtype=torch.float32)
    bypassed = ctypes.c_int(0)
    call("t4r_gemm_wgrad_f32", _stream(), M, N, K, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(),
         ws.data_ptr(), ws.numel(), ctypes.addressof(bypassed))
    if bypassed.value:  # say so instead of silently losing the bit-reproducibility this function exists for (the sum is still correct)
        import warnings

        warnings.warn(f"gemm_wgrad: the product found no room in its {ws.numel()}-float split-K workspace (M={M} N={N} K={K}) "
                      "and used fp32 atomics: this gradient is not bit-reproducible", RuntimeWarning)
    return out


def _gemm_wgrad_ws_floats(M, N, K):
    return _lib.load().t4r_gemm_wgrad_ws_floats(M, N, K)


def gemm_softmax_grad(logits, lse, labels, grad_out, V, b, trans_a, alpha=1.0, label_smoothing=0.0,
                      out=None, splitk=1, accumulate=False):
    """trans_a=False: out[N_rows, N] = alpha * dlogits @ b[V, N] ; True: out[V, N] = alpha * dlogits^T @ b[N_rows, N]
    with dlogits = softmax-CE gradient formed on the fly from (logits, lse, labels, grad_out)."""
    n_rows = logits.shape[0]
    N = b.shape[1]
    ld = logits.stride(0) if n_rows > 1 else max(logits.shape[1], V)
    if out is None:
        out = torch.empty((V if trans_a else n_rows, N), device=logits.device, dtype=torch.float32)
    call("t4r_gemm_softmax_grad_f32", _stream(), int(trans_a), n_rows, V, N, float(alpha), logits.data_ptr(), ld,
         _chk(lse, torch.float32), _chk(labels, torch.int64), _p(grad_out), float(label_smoothing),
         b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), int(splitk), int(accumulate))
    return out


class tok_gemm_min_rows:
    """context manager: row threshold of the token-stationary body GEMM (csrc/tok_gemm.hip; default 32 768)"""

    def __init__(self, rows):
        self.rows = int(rows)

    def __enter__(self):
        lib = _lib.load()
        self.prev = lib.t4r_get_tok_gemm_min_rows()
        lib.t4r_set_tok_gemm_min_rows(self.rows)
        return self

    def __exit__(self, *exc):
        _lib.load().t4r_set_tok_gemm_min_rows(self.prev)
        return False


# ---- materialised head for d_model <= 128 (csrc/head_split.hip)
def head_split_supported(D):
    return bool(_lib.load().t4r_head_split_supported(int(D)))


def head_split_ws_bytes(N, V, D):
    """bytes of workspace head_split_prepare allocates for these sizes (0: unsupported width)"""
    return int(_lib.load().t4r_head_split_ws_bytes(int(N), int(V), int(D)))


def head_split_prepare(x, V):
    """cuts the head's input rows x [N, D] into the plane blocks of the three products; returns the workspace"""
    N, D = x.shape
    nbytes = _lib.load().t4r_head_split_ws_bytes(N, int(V), D)
    ws = torch.empty(max(nbytes, 16), device=x.device, dtype=torch.uint8)
    call("t4r_head_split_prepare", _stream(), _chk(x, torch.float32), x.stride(0), N, D, int(V), ws.data_ptr())
    # the host note the forward product leaves for d X / d W (include/t4r_hip.h: t4r_head_note, 64 bytes) lives and dies with
    # the workspace: a CPU int64[8] tensor, so that it can also travel through the dispatcher as an operator output
    # (torch_ops.next_item_head) and be re-attached to the workspace tensor its backward operator receives
    ws.t4r_note = torch.zeros(8, dtype=torch.int64)
    return ws


def _note(ws):
    n = getattr(ws, "t4r_note", None)
    return None if n is None else n.data_ptr()


def head_split_dw_form(ws):
    """which kernel the last head_split_dw on this workspace ran: 0 none yet, 1 three bf16 planes, 2 two-way fp16 split
    with per-item scales"""
    return _lib.load().t4r_head_note_dw_form(_note(ws))


def head_split_logits(ws, x, W, alpha=1.0, ldc=None):
    N, D = x.shape
    V = W.shape[0]
    ldc = V if ldc is None else ldc
    buf = torch.empty((N, ldc), device=x.device, dtype=torch.float32)
    call("t4r_head_split_logits", _stream(), ws.data_ptr(), _chk(W, torch.float32), W.stride(0), buf.data_ptr(), ldc,
         N, V, D, float(alpha), _note(ws))
    return buf[:, :V]


def head_split_logits_ce(ws, x, W, labels, alpha=1.0, label_smoothing=0.0, ldc=None):
    """logits [N, V] (view of an [N, ldc] buffer) + (mean loss, loss rows, lse) in one pass over the vocabulary"""
    N, D = x.shape
    V = W.shape[0]
    ldc = V if ldc is None else ldc
    dev = x.device
    buf = torch.empty((N, ldc), device=dev, dtype=torch.float32)
    loss_rows = torch.empty(N, device=dev, dtype=torch.float32)
    lse = torch.empty(N, device=dev, dtype=torch.float32)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    call("t4r_head_split_logits_ce", _stream(), ws.data_ptr(), _chk(W, torch.float32), W.stride(0), buf.data_ptr(), ldc,
         _chk(labels, torch.int64), loss_rows.data_ptr(), lse.data_ptr(), loss.data_ptr(), N, V, D, float(alpha),
         float(label_smoothing), _note(ws))
    return buf[:, :V], loss, loss_rows, lse


def head_split_fdx_supported(D):
    return bool(_lib.load().t4r_head_split_fdx_supported(int(D)))


def head_split_logits_ce_dx(ws, x, W, labels, alpha=1.0, label_smoothing=0.0, ldc=None, w_amax=None):
    """the one-pass forward (csrc/head_split.hip: head_fwd_dx_kernel): logits [N, V] (view of an [N, ldc] buffer), mean loss,
    loss rows, lse AND dx_unit [N, D] = d (mean loss) / d x for an upstream gradient of 1 -- the backward is dx_unit * grad_out
    plus head_split_dw on the same workspace; the logits are never read for d X"""
    N, D = x.shape
    V = W.shape[0]
    ldc = V if ldc is None else ldc
    dev = x.device
    buf = torch.empty((N, ldc), device=dev, dtype=torch.float32)
    loss_rows = torch.empty(N, device=dev, dtype=torch.float32)
    lse = torch.empty(N, device=dev, dtype=torch.float32)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    dx = torch.empty((N, D), device=dev, dtype=torch.float32)
    wsum = None
    if label_smoothing > 0:
        wsum = torch.zeros(D, device=dev, dtype=torch.float32)
        colsum_(W, wsum)
    args = (_stream(), ws.data_ptr(), _chk(x, torch.float32), x.stride(0), _chk(W, torch.float32),
            W.stride(0), buf.data_ptr(), ldc, _chk(labels, torch.int64), loss_rows.data_ptr(), lse.data_ptr(), loss.data_ptr(),
            dx.data_ptr(), dx.stride(0), _p(wsum), N, V, D, float(alpha), float(label_smoothing), _note(ws))
    if w_amax is not None:      # (partials, n) of ops.w_amax_of(the table's Parameter): max |W| without a pass over W
        call("t4r_head_split_logits_ce_dx_amax", *args, _chk(w_amax[0], torch.float32), int(w_amax[1]))
    else:
        call("t4r_head_split_logits_ce_dx", *args)
    return buf[:, :V], loss, loss_rows, lse, dx


def head_split_dw(ws, logits, lse, labels, grad_out, V, D, out, alpha=1.0, label_smoothing=0.0, accumulate=True, yoff=0):
    N, Vc = logits.shape
    call("t4r_head_split_dw", _stream(), ws.data_ptr(), logits.data_ptr(), logits.stride(0), _chk(lse, torch.float32),
         _chk(labels, torch.int64), _p(grad_out), float(label_smoothing), out.data_ptr(), out.stride(0), N, Vc, int(V),
         int(yoff), int(D), float(alpha), int(accumulate), _note(ws))
    return out


def head_split_dx(ws, logits, lse, labels, grad_out, V, W, alpha=1.0, label_smoothing=0.0, out=None, accumulate=False, yoff=0):
    N, Vc = logits.shape
    D = W.shape[1]
    if out is None:
        out = torch.empty((N, D), device=logits.device, dtype=torch.float32)
    call("t4r_head_split_dx", _stream(), ws.data_ptr(), logits.data_ptr(), logits.stride(0), _chk(lse, torch.float32),
         _chk(labels, torch.int64), _p(grad_out), float(label_smoothing), W.data_ptr(), W.stride(0), out.data_ptr(),
         out.stride(0), N, Vc, int(V), int(yoff), D, float(alpha), int(accumulate), _note(ws))
    return out


# ---- the recomputing form: no [N, V] tensor (csrc/head_split.hip: head_ce_stats_h / head_dw_rc / head_dx_rc kernels)
def head_split_recompute_supported(D):
    return bool(_lib.load().t4r_head_split_recompute_supported(int(D)))


def head_split_ce(ws, x, W, labels, alpha=1.0, label_smoothing=0.0):
    """mean loss, loss rows, lse of softmax(alpha x W^T) vs labels from the prepared workspace; nothing of size [N, V] is written"""
    N, D = x.shape
    V = W.shape[0]
    dev = x.device
    loss_rows = torch.empty(N, device=dev, dtype=torch.float32)
    lse = torch.empty(N, device=dev, dtype=torch.float32)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    # the image of x only this form's d W reads (kept out of head_split_prepare: the materialised head would pay a launch for it)
    call("t4r_head_split_prepare_rc", _stream(), _chk(x, torch.float32), x.stride(0), N, D, int(V), ws.data_ptr())
    call("t4r_head_split_ce", _stream(), ws.data_ptr(), _chk(W, torch.float32), W.stride(0), _chk(labels, torch.int64),
         loss_rows.data_ptr(), lse.data_ptr(), loss.data_ptr(), N, V, D, float(alpha), float(label_smoothing), _note(ws))
    return loss, loss_rows, lse


def head_split_dw_rc(ws, W, lse, labels, grad_out, out, alpha=1.0, label_smoothing=0.0, accumulate=True):
    N = lse.shape[0]
    V, D = W.shape
    call("t4r_head_split_dw_rc", _stream(), ws.data_ptr(), _chk(W, torch.float32), W.stride(0), _chk(lse, torch.float32),
         _chk(labels, torch.int64), _p(grad_out), float(label_smoothing), out.data_ptr(), out.stride(0), N, V, D, float(alpha),
         int(accumulate), _note(ws))
    return out


def head_split_dx_rc(ws, x, W, lse, labels, grad_out, alpha=1.0, label_smoothing=0.0, out=None, accumulate=False):
    N, D = x.shape
    V = W.shape[0]
    if out is None:
        out = torch.empty((N, D), device=x.device, dtype=torch.float32)
    call("t4r_head_split_dx_rc", _stream(), ws.data_ptr(), _chk(x, torch.float32), x.stride(0), _chk(W, torch.float32), W.stride(0),
         _chk(lse, torch.float32), _chk(labels, torch.int64), _p(grad_out), float(label_smoothing), out.data_ptr(), out.stride(0),
         N, V, D, float(alpha), int(accumulate), _note(ws))
    return out


# ------------------------------------------------------------------------------------ LN / act
SITE_INPUT, SITE_POS, SITE_PROB, SITE_ATTN_OUT, SITE_FF_ACT, SITE_FF_OUT, SITE_FINAL = range(7)
SITE_GUMBEL = 7              # the Gumbel noise of the sampling heads: ctr_hi = dropout_ctr_hi(offset, 255, SITE_GUMBEL)
LAYER_FUSE_FINAL = 0x100     # flag in xlnet_layer_fwd / _bwd's layer_idx: this layer also applies the model's output dropout
LAYER_FUSE_INPUT = 0x200     # ... this (first) layer applies the model's input dropout: h is the undropped input
LAYER_STACK_PREPARED = 0x400  # ... (_fwd only) the workspace already holds the layer's weight planes and k_r (xlnet_stack_prepare)
LAYER_DEFER_JOIN = 0x800     # ... (_bwd only) return without joining the weight-gradient streams (xlnet_layer_bwd_join is owed)
NO_DROP = (0.0, 0, 0)


def dropout_ctr_hi(offset, layer, site):
    return _lib.load().t4r_dropout_ctr_hi(int(offset), int(layer), int(site))


def dropout(x, p, seed, ctr_hi, n_total=None, want_mask=False, out=None):
    """out[i] = x[i % x.numel()] * keep(i)/(1-p), i < n_total (default x.numel())."""
    n_src = x.numel()
    n = n_src if n_total is None else n_total
    if out is None:
        out = torch.empty(n, device=x.device, dtype=torch.float32)
    mask = torch.empty(n, device=x.device, dtype=torch.uint8) if want_mask else None
    call("t4r_dropout", _stream(), _chk(x, torch.float32), out.data_ptr(), _p(mask), n, n_src, float(p),
         int(seed), int(ctr_hi))
    return (out, mask) if want_mask else out


def add_layernorm_fwd(a, b, gamma, beta, eps, drop=NO_DROP):
    rows, D = a.shape[0], a.shape[1]
    y = torch.empty_like(a)
    mean = torch.empty(rows, device=a.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    call("t4r_add_layernorm_fwd", _stream(), _chk(a, torch.float32), _p(b, torch.float32),
         _chk(gamma), _chk(beta), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, D, float(eps),
         float(drop[0]), int(drop[1]), int(drop[2]))
    return y, mean, rstd


def add_layernorm_bwd(a, b, gamma, mean, rstd, dy, dgamma, dbeta, dx=None, accumulate_dx=False,
                      drop=NO_DROP):
    """-> dx (gradient of b), or (dx, dxa) with dropout (dxa = gradient of the dropped operand a)."""
    rows, D = a.shape
    if dx is None:
        dx = torch.empty_like(a)
    dxa = torch.empty_like(a) if drop[0] > 0 else None
    ws = _colred_ws(rows, 2 * D, a.device)
    call("t4r_add_layernorm_bwd", _stream(), _chk(a), _p(b), _chk(gamma), _chk(mean), _chk(rstd),
         _chk(dy), dx.data_ptr(), _p(dxa), _p(dgamma), _p(dbeta), ws.data_ptr(), rows, D,
         int(accumulate_dx), float(drop[0]), int(drop[1]), int(drop[2]))
    return dx if dxa is None else (dx, dxa)


def _colred_ws(rows, ncols, device):
    return torch.empty(_lib.load().t4r_colreduce_ws_floats(rows, ncols), device=device, dtype=torch.float32)


def act_bwd_bias(dact, pre, dbias, mode, out=None, drop=NO_DROP):
    rows, N = dact.shape
    out = dact if out is None else out
    ws = None if dbias is None else _colred_ws(rows, N, dact.device)
    call("t4r_act_bwd_bias", _stream(), _chk(dact), _chk(pre), out.data_ptr(), _p(dbias), _p(ws), rows, N,
         mode, float(drop[0]), int(drop[1]), int(drop[2]))
    return out


def colsum_(x, out):
    ws = _colred_ws(x.shape[0], x.shape[1], x.device)
    call("t4r_colsum", _stream(), _chk(x), _chk(out), ws.data_ptr(), x.shape[0], x.shape[1], x.stride(0))
    return out


# ------------------------------------------------------------------------------------ input block
def ragged_to_padded(values, offsets, L):
    rows = offsets.numel() - 1
    out = torch.empty((rows, L), device=values.device, dtype=values.dtype)
    if values.dtype not in (torch.int64, torch.float32):
        raise TypeError("ragged_to_padded: int64 or float32 values")
    call("t4r_ragged_to_padded", _stream(), _chk(values), _chk(offsets, torch.int64), out.data_ptr(),
         rows, L, values.element_size())
    return out


def ragged_gather_to_padded(values, offsets, row_ids, L):
    """out[i, :] = the list of row row_ids[i] of the ragged column (values, offsets), zero-padded /
    truncated to L; offsets=None gathers a scalar column (returns [rows])."""
    rows = row_ids.numel()
    if values.dtype not in (torch.int64, torch.float32):
        raise TypeError("ragged_gather_to_padded: int64 or float32 values")
    scalar = offsets is None
    out = torch.empty((rows,) if scalar else (rows, L), device=values.device, dtype=values.dtype)
    call("t4r_ragged_gather_to_padded", _stream(), _chk(values), _p(offsets, torch.int64),
         _chk(row_ids, torch.int64), out.data_ptr(), rows, 1 if scalar else L, values.element_size())
    return out


def ragged_max_len(offsets):
    out = torch.empty(1, device=offsets.device, dtype=torch.int32)
    call("t4r_ragged_max_len", _stream(), _chk(offsets, torch.int64), offsets.numel() - 1, out.data_ptr())
    return out


def seq_features_fwd(feats, agg, B, L_in, L_out, W, item_feat=-1, mask_mode=MASK_NONE, mask=None,
                     masked_emb=None, err_flag=None):
    """feats: list of dicts(kind, input, table, dim, col, rows).  Returns out [B, L_out, W]."""
    n = len(feats)
    dev = feats[0]["input"].device
    out = torch.empty((B, L_out, W), device=dev, dtype=torch.float32)
    kinds, _k = int_array([f["kind"] for f in feats])
    inputs, _i = ptr_array([_chk(f["input"]) for f in feats])
    tables, _t = ptr_array([0 if f.get("table") is None else _chk(f["table"], torch.float32) for f in feats])
    dims, _d = int_array([f["dim"] for f in feats])
    cols, _c = int_array([f.get("col", 0) for f in feats])
    rows, _r = long_array([f.get("rows", 0) for f in feats])
    call("t4r_seq_features_fwd", _stream(), n, kinds, inputs, tables, dims, cols, rows, AGG[agg] if
         isinstance(agg, str) else agg, item_feat, B, L_in, L_out, W, mask_mode,
         _p(mask), _p(masked_emb), out.data_ptr(), _p(err_flag))
    return out


def embedding_bwd(dout, ids, d_table, col, dim, padding_idx=0):
    """ids [B, L] (sequence feature) or [B] (per-session context feature, gradient summed over L)"""
    W = dout.shape[-1]
    ntok = dout.numel() // W
    ids_div = ntok // ids.numel()
    call("t4r_embedding_bwd", _stream(), _chk(dout, torch.float32), _chk(ids, torch.int64),
         _chk(d_table, torch.float32), ntok, W, col, dim, d_table.shape[0], padding_idx, ids_div)


def sort_ids(ids, rows, padding_idx=0):
    """stable sort of the lookups by table row -> (keys_sorted int32 [n], perm int32 [n]); padding /
    out-of-range ids carry the key `rows` and come last.  Depends on the ids only (forward-pass work)."""
    ids = ids.contiguous().view(-1)
    n = ids.numel()
    keys = torch.empty(n, device=ids.device, dtype=torch.int32)
    perm = torch.empty(n, device=ids.device, dtype=torch.int32)
    nb = _lib.load().t4r_sort_ids_ws_bytes(n)
    ws = torch.empty(max(nb, 1), device=ids.device, dtype=torch.uint8)
    call("t4r_sort_ids", _stream(), _chk(ids, torch.int64), n, int(rows), int(padding_idx), keys.data_ptr(),
         perm.data_ptr(), ws.data_ptr(), nb)
    return keys, perm


def sort_ids_multi(ids_list, rows_list, padding_idx_list):
    """sort_ids for several tables in ONE device sort (csrc/embedding_sorted.hip: t4r_sort_ids_multi): every ids tensor has
    the same number of lookups n -> [(keys_sorted, perm)] per table, each exactly what sort_ids gives for it alone (views
    of two [F * n] buffers)."""
    F = len(ids_list)
    ids_list = [i.contiguous().view(-1) for i in ids_list]
    n = ids_list[0].numel()
    if F > 16 or any(i.numel() != n for i in ids_list):
        return [sort_ids(i, r, p) for i, r, p in zip(ids_list, rows_list, padding_idx_list)]
    dev = ids_list[0].device
    keys = torch.empty(F * n, device=dev, dtype=torch.int32)
    perm = torch.empty(F * n, device=dev, dtype=torch.int32)
    nb = _lib.load().t4r_sort_ids_multi_ws_bytes(n, F)
    ws = torch.empty(max(nb, 1), device=dev, dtype=torch.uint8)
    parr, _k0 = ptr_array([_chk(i, torch.int64) for i in ids_list])
    rows, _k1 = long_array([int(r) for r in rows_list])
    pads, _k2 = int_array([int(p) for p in padding_idx_list])
    call("t4r_sort_ids_multi", _stream(), parr, F, n, rows, pads, keys.data_ptr(), perm.data_ptr(), ws.data_ptr(), nb)
    return [(keys[f * n:(f + 1) * n], perm[f * n:(f + 1) * n]) for f in range(F)]


def embedding_bwd_sorted(dout, keys, perm, d_table, col, dim, ids_div=1):
    """deterministic d_table[id] += gradient rows (ascending lookup order, one owner per row, no atomics).
    dout [n * ids_div, W]; (keys, perm) from sort_ids."""
    W = dout.shape[-1]
    n = keys.numel()
    if dout.numel() != n * ids_div * W:
        raise ValueError("embedding_bwd_sorted: dout rows != lookups * ids_div")
    ws = torch.empty(max(1, _lib.load().t4r_embedding_bwd_sorted_ws_floats(n, dim)), device=dout.device,
                     dtype=torch.float32)
    call("t4r_embedding_bwd_sorted", _stream(), _chk(dout, torch.float32), _chk(keys, torch.int32),
         _chk(perm, torch.int32), _chk(d_table, torch.float32), n, W, col, dim, d_table.shape[0], int(ids_div),
         ws.data_ptr())


BAG_COMBINER = {"sum": 0, "mean": 1, "sqrtn": 2}


def embedding_bag_fwd(table, values, offsets=None, combiner="mean", out=None, col=0, err_flag=None):
    """torch.nn.EmbeddingBag(mode=combiner) without a padding index.  values: int64 [B, K] / [B] (matrix form,
    offsets None) or [n] with offsets int64 [B] (ragged form).  -> [B, dim] (or the columns [col, col + dim) of `out`)."""
    rows, dim = table.shape
    if offsets is None:
        v2 = values.view(values.shape[0], -1)
        n_bags, fixed_k = v2.shape[0], v2.shape[1]
    else:
        n_bags, fixed_k = offsets.numel(), 0
    if out is None:
        out = torch.empty((n_bags, dim), device=table.device, dtype=torch.float32)
    call("t4r_embedding_bag_fwd", _stream(), _chk(table, torch.float32), rows, dim, _chk(values, torch.int64),
         _p(offsets, torch.int64), n_bags, values.numel(), fixed_k, BAG_COMBINER[combiner], out.data_ptr(),
         out.stride(0), col, _p(err_flag))
    return out


def embedding_bag_bwd_rows(dout, n_values, dim, offsets=None, fixed_k=0, combiner="mean", col=0):
    """gradient row of every member lookup, [n_values, dim] in lookup order (see t4r_embedding_bag_bwd_rows)"""
    rows = torch.empty((n_values, dim), device=dout.device, dtype=torch.float32)
    n_bags = dout.shape[0]
    call("t4r_embedding_bag_bwd_rows", _stream(), _chk(dout, torch.float32), dout.stride(0), col, dim,
         _p(offsets, torch.int64), n_bags, n_values, fixed_k, BAG_COMBINER[combiner], rows.data_ptr())
    return rows


def swap_noise(x, item_ids, p, pad_token=0, bern=None, perm=None, seed=0, ctr_hi=0):
    """tr.StochasticSwapNoise.augment for one feature: x [B, L] or [B] (int64 ids / fp32 values);
    item_ids [B, L] gives the padding mask.  bern (uint8, x.shape) / perm (int64 [#non-pad]) inject
    the draws; None -> device Philox draws."""
    if x.dtype not in (torch.int64, torch.float32):
        raise TypeError("swap_noise: int64 ids or fp32 values")
    n = x.numel()
    out = torch.empty_like(x)
    stride = item_ids.shape[1] if x.ndim == item_ids.ndim - 1 else 1
    nb = _lib.load().t4r_swap_noise_ws_bytes(n)
    ws = torch.empty(max(nb, 1), device=x.device, dtype=torch.uint8)
    if bern is not None:
        bern = bern.to(torch.uint8).contiguous()
    call("t4r_swap_noise", _stream(), _chk(x), out.data_ptr(), x.element_size(), n,
         _chk(item_ids, torch.int64), int(pad_token), stride, float(p), _p(bern, torch.uint8),
         _p(perm, torch.int64), int(seed), int(ctr_hi), ws.data_ptr(), nb)
    return out


def copy_cols_out(wide2d, col, dim):
    """-> contiguous [rows, dim] copy of wide2d[:, col:col+dim]"""
    rows, ldw = wide2d.shape
    out = torch.empty((rows, dim), device=wide2d.device, dtype=torch.float32)
    call("t4r_copy_cols", _stream(), _chk(wide2d, torch.float32), ldw, col, out.data_ptr(), dim, rows, 0)
    return out


def seq_sum_cols(wide2d, col, dim, B, L):
    """-> [B, dim] = sum over the L tokens of each session of wide2d[:, col:col+dim]"""
    out = torch.empty((B, dim), device=wide2d.device, dtype=torch.float32)
    call("t4r_seq_sum_cols", _stream(), _chk(wide2d, torch.float32), wide2d.shape[1], col, out.data_ptr(), dim,
         B, L)
    return out


def apply_mask_fwd_(x, mask, memb, mode):
    B, L, H = x.shape
    call("t4r_apply_mask_fwd", _stream(), _chk(x), _chk(mask), _chk(memb), B, L, H, mode)
    return x


def apply_mask_bwd_(dy, mask, d_memb, mode):
    B, L, H = dy.shape
    ws = torch.empty(max(1, _lib.load().t4r_apply_mask_bwd_ws_floats(B, L, H)), device=dy.device, dtype=torch.float32)
    call("t4r_apply_mask_bwd", _stream(), _chk(dy), _chk(mask), _chk(d_memb), B, L, H, mode, ws.data_ptr())
    return dy


def apply_mask_bwd(dy, mask, d_memb, mode):
    """out of place: -> dx (dy untouched); d_memb accumulated"""
    B, L, H = dy.shape
    dy = dy.contiguous()
    dx = torch.empty_like(dy)
    ws = torch.empty(max(1, _lib.load().t4r_apply_mask_bwd_ws_floats(B, L, H)), device=dy.device, dtype=torch.float32)
    call("t4r_apply_mask_bwd_to", _stream(), _chk(dy), dx.data_ptr(), _chk(mask), _chk(d_memb), B, L, H, mode, ws.data_ptr())
    return dx


def mul(a, b):
    out = torch.empty_like(a)
    call("t4r_mul", _stream(), _chk(a), _chk(b), out.data_ptr(), a.numel())
    return out


def soft_embedding_fwd(x, proj_w, proj_b, table, ln_w, ln_b, eps=1e-5):
    K, D = table.shape
    out = torch.empty(x.shape + (D,), device=x.device, dtype=torch.float32)
    call("t4r_soft_embedding_fwd", _stream(), _chk(x, torch.float32), _chk(proj_w), _chk(proj_b),
         _chk(table), _p(ln_w), _p(ln_b), out.data_ptr(), x.numel(), K, D, float(eps))
    return out


def soft_embedding_bwd(dout, x, proj_w, proj_b, table, ln_w, d_proj_w, d_proj_b, d_table, d_ln_w,
                       d_ln_b, col, eps=1e-5):
    K, D = table.shape
    W = dout.shape[-1]
    ws = torch.empty(max(1, _lib.load().t4r_soft_embedding_bwd_ws_floats(x.numel(), K, D)), device=dout.device, dtype=torch.float32)
    call("t4r_soft_embedding_bwd", _stream(), _chk(dout), _chk(x), _chk(proj_w), _chk(proj_b),
         _chk(table), _p(ln_w), _chk(d_proj_w), _chk(d_proj_b), _chk(d_table), _p(d_ln_w), _p(d_ln_b),
         x.numel(), W, col, K, D, float(eps), ws.data_ptr())


# ------------------------------------------------------------------------------------ masking
def mask_targets(item_ids, mode, padding_idx=0, bern=None, j1=None, j2=None, p=0.15, seed=0,
                 offset=0, want_counts=True):
    B, L = item_ids.shape
    Lout = L + 1 if mode == MLM_INFER else L
    dev = item_ids.device
    mask = torch.empty((B, Lout), device=dev, dtype=torch.bool)
    labels = torch.empty((B, Lout), device=dev, dtype=torch.int64)
    counts = torch.empty(B, device=dev, dtype=torch.int32) if want_counts else None
    if bern is not None:
        bern = bern.to(torch.uint8) if bern.dtype != torch.uint8 else bern
    call("t4r_mask_targets", _stream(), _chk(item_ids, torch.int64), B, L, mode, padding_idx,
         _p(bern), _p(j1, torch.int64), _p(j2, torch.int64), float(p), int(seed), int(offset),
         mask.data_ptr(), labels.data_ptr(), _p(counts))
    return mask, labels, counts


def compact_labels(labels, counts, padding_idx=0):
    """-> (n_labels [1] int32 device, label_pos [B*L] int32, labels_compact [B*L] int64)"""
    B, L = labels.shape
    dev = labels.device
    row_off = torch.empty(B, device=dev, dtype=torch.int32)
    n = torch.empty(1, device=dev, dtype=torch.int32)
    pos = torch.empty(B * L, device=dev, dtype=torch.int32)
    lab = torch.empty(B * L, device=dev, dtype=torch.int64)
    call("t4r_compact_labels", _stream(), _chk(labels, torch.int64), _chk(counts, torch.int32), B, L,
         padding_idx, row_off.data_ptr(), n.data_ptr(), pos.data_ptr(), lab.data_ptr())
    return n, pos, lab


def gather_rows(x2d, pos, n):
    D = x2d.shape[1]
    out = torch.empty((n, D), device=x2d.device, dtype=torch.float32)
    call("t4r_gather_rows", _stream(), _chk(x2d, torch.float32), _chk(pos, torch.int32), out.data_ptr(), n, D)
    return out


def scatter_rows_add_(dout, pos, dx2d):
    n, D = dout.shape
    call("t4r_scatter_rows_add", _stream(), _chk(dout), _chk(pos, torch.int32), _chk(dx2d), n, D)
    return dx2d


def scatter_rows_dense(src, pos, n, scale, T):
    """[T, D] zeros with row pos[r] = scale * src[r] (r < n; pos ascending, scale a device scalar or None): one launch"""
    D = src.shape[1]
    dx = torch.empty((T, D), device=src.device, dtype=torch.float32)
    call("t4r_scatter_rows_dense", _stream(), _chk(src), _chk(pos, torch.int32), int(n), _p(scale), dx.data_ptr(), int(T), D)
    return dx


def last_positions(item_ids, Lgrid, is_mlm, padding_idx=0):
    B, L = item_ids.shape
    pos = torch.empty(B, device=item_ids.device, dtype=torch.int32)
    call("t4r_last_positions", _stream(), _chk(item_ids, torch.int64), B, L, Lgrid, int(is_mlm),
         padding_idx, pos.data_ptr())
    return pos


# ------------------------------------------------------------------------------------ attention / layer
def session_lengths(item_ids, padding_idx=0, extra=0):
    """int32 [B]: number of non-padding positions of every session (+ extra: the [MASK] slot of the MLM
    inference grid) -- the key_len of the opt-in attention padding mask"""
    B, L = item_ids.shape
    out = torch.empty(B, device=item_ids.device, dtype=torch.int32)
    call("t4r_session_lengths", _stream(), _chk(item_ids, torch.int64), B, L, int(padding_idx), int(extra),
         out.data_ptr())
    return out


def xlnet_attn_fwd(q, k, v, k_r, r_w_bias, r_r_bias, B, L, n_head, drop=NO_DROP, key_len=None):
    """k_r [2L, D] (shared) or [B*2L, D] (per session).  key_len int32 [B]: opt-in padding mask."""
    D = q.shape[-1]
    per_b = int(k_r.shape[0] == B * 2 * L and B > 1)
    out = torch.empty((B * L, D), device=q.device, dtype=torch.float32)
    lse = torch.empty((B, n_head, L), device=q.device, dtype=torch.float32)
    call("t4r_xlnet_attn_fwd", _stream(), _chk(q), _chk(k), _chk(v), _chk(k_r), _chk(r_w_bias),
         _chk(r_r_bias), out.data_ptr(), lse.data_ptr(), B, L, n_head, D // n_head, per_b,
         float(drop[0]), int(drop[1]), int(drop[2]), _p(key_len, torch.int32))
    return out, lse


def xlnet_attn_bwd(q, k, v, k_r, r_w_bias, r_r_bias, out, lse, dout, d_rw, d_rr, B, L, n_head,
                   drop=NO_DROP, key_len=None):
    D = q.shape[-1]
    dev = q.device
    per_b = int(k_r.shape[0] == B * 2 * L and B > 1)
    # planes of one [3, T, D] buffer, as the layer holds them
    dq, dk, dv = torch.empty((3, B * L, D), device=dev, dtype=torch.float32).unbind(0)
    dkr = torch.empty_like(k_r)
    nws = _lib.load().t4r_xlnet_attn_bwd_ws_floats(B, L, D, n_head)
    ws = torch.empty(nws, device=dev, dtype=torch.float32)
    call("t4r_xlnet_attn_bwd", _stream(), _chk(q), _chk(k), _chk(v), _chk(k_r), _chk(r_w_bias),
         _chk(r_r_bias), _chk(out), _chk(lse), _chk(dout), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
         dkr.data_ptr(), _chk(d_rw), _chk(d_rr), ws.data_ptr(), B, L, n_head, D // n_head, per_b,
         float(drop[0]), int(drop[1]), int(drop[2]), _p(key_len, torch.int32))
    return dq, dk, dv, dkr


def xlnet_attn_bwd_prob(q, k, v, k_r, r_w_bias, r_r_bias, prob, dout, d_rw, d_rr, B, L, n_head, drop=NO_DROP):
    """xlnet_attn_bwd reading the probabilities before dropout [B, n_head, L, L] that xlnet_attn_block_fwd(prob=...) left
    (include/t4r_hip_attn.h; L <= 32, d_head 16 / 32)"""
    D = q.shape[-1]
    dev = q.device
    per_b = int(k_r.shape[0] == B * 2 * L and B > 1)
    dq, dk, dv = torch.empty((3, B * L, D), device=dev, dtype=torch.float32).unbind(0)
    dkr = torch.empty_like(k_r)
    nws = _lib.load().t4r_xlnet_attn_bwd_ws_floats(B, L, D, n_head)
    ws = torch.empty(nws, device=dev, dtype=torch.float32)
    call("t4r_xlnet_attn_bwd_prob", _stream(), _chk(q), _chk(k), _chk(v), _chk(k_r), _chk(r_w_bias), _chk(r_r_bias),
         _chk(prob), _chk(dout), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dkr.data_ptr(), _chk(d_rw), _chk(d_rr),
         ws.data_ptr(), B, L, n_head, D // n_head, per_b, float(drop[0]), int(drop[1]), int(drop[2]))
    return dq, dk, dv, dkr


def xlnet_attn_uni_fwd(q, k, v, k_r, r_w_bias, r_r_bias, B, L, n_head, drop=NO_DROP, key_len=None):
    """xlnet_attn_fwd with the causal dead set of attn_type='uni' (include/t4r_hip_uni.h): key j of row i is dead when j > i,
    or under the padding rule of key_len.  k_r keeps the [2L, D] layout; rows 1 .. L are read."""
    D = q.shape[-1]
    per_b = int(k_r.shape[0] == B * 2 * L and B > 1)
    out = torch.empty((B * L, D), device=q.device, dtype=torch.float32)
    lse = torch.empty((B, n_head, L), device=q.device, dtype=torch.float32)
    call("t4r_xlnet_attn_uni_fwd", _stream(), _chk(q), _chk(k), _chk(v), _chk(k_r), _chk(r_w_bias),
         _chk(r_r_bias), out.data_ptr(), lse.data_ptr(), B, L, n_head, D // n_head, per_b,
         float(drop[0]), int(drop[1]), int(drop[2]), _p(key_len, torch.int32))
    return out, lse


def xlnet_attn_uni_bwd(q, k, v, k_r, r_w_bias, r_r_bias, out, lse, dout, d_rw, d_rr, B, L, n_head,
                       drop=NO_DROP, key_len=None):
    """-> dq, dk, dv, dkr (rows 0 and L + 1 .. 2L - 1 of dkr exact zeros); d_rw / d_rr accumulated"""
    D = q.shape[-1]
    dev = q.device
    per_b = int(k_r.shape[0] == B * 2 * L and B > 1)
    dq, dk, dv = torch.empty((3, B * L, D), device=dev, dtype=torch.float32).unbind(0)
    dkr = torch.empty_like(k_r)
    nws = _lib.load().t4r_xlnet_attn_bwd_ws_floats(B, L, D, n_head)
    ws = torch.empty(nws, device=dev, dtype=torch.float32)
    call("t4r_xlnet_attn_uni_bwd", _stream(), _chk(q), _chk(k), _chk(v), _chk(k_r), _chk(r_w_bias),
         _chk(r_r_bias), _chk(out), _chk(lse), _chk(dout), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
         dkr.data_ptr(), _chk(d_rw), _chk(d_rr), ws.data_ptr(), B, L, n_head, D // n_head, per_b,
         float(drop[0]), int(drop[1]), int(drop[2]), _p(key_len, torch.int32))
    return dq, dk, dv, dkr


def mha_fwd(q, k, v, B, L, n_head, causal, drop=NO_DROP, key_len=None):
    """q,k,v: [B*L, D] views that may be column slices of one [B*L, 3D] buffer (row stride = ld)."""
    D = q.shape[1]
    ld = q.stride(0)
    assert k.stride(0) == ld and v.stride(0) == ld and q.stride(1) == 1
    out = torch.empty((B * L, D), device=q.device, dtype=torch.float32)
    lse = torch.empty((B, n_head, L), device=q.device, dtype=torch.float32)
    call("t4r_mha_fwd", _stream(), q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, out.data_ptr(), D,
         lse.data_ptr(), B, L, n_head, D // n_head, int(causal), float(drop[0]), int(drop[1]), int(drop[2]),
         _p(key_len, torch.int32))
    return out, lse


def mha_bwd(q, k, v, out, lse, dout, B, L, n_head, causal, drop=NO_DROP, fused_out=False, key_len=None):
    """-> dq, dk, dv.  fused_out: one [B*L, 3D] buffer (column blocks q|k|v), returned as the single tensor."""
    D = q.shape[1]
    ld = q.stride(0)
    dev = q.device
    if fused_out:
        buf = torch.empty((B * L, 3 * D), device=dev, dtype=torch.float32)
        dq, dk, dv, ldd = buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:], 3 * D
    else:
        dq, dk, dv = (torch.empty((B * L, D), device=dev, dtype=torch.float32) for _ in range(3))
        buf, ldd = None, D
    call("t4r_mha_bwd", _stream(), q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, _chk(out), _chk(dout), D,
         _chk(lse), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ldd, B, L, n_head, D // n_head, int(causal),
         float(drop[0]), int(drop[1]), int(drop[2]), _p(key_len, torch.int32))
    return buf if fused_out else (dq, dk, dv)


def add_pos_fwd(x, pos, token_type=None):
    B, L, D = x.shape
    out = torch.empty_like(x)
    call("t4r_add_pos_fwd", _stream(), _chk(x, torch.float32), _chk(pos), _p(token_type), out.data_ptr(), B, L, D)
    return out


def add_pos_bwd_(dy, d_pos):
    B, L, D = dy.shape
    call("t4r_add_pos_bwd", _stream(), _chk(dy), _chk(d_pos), B, L, D)


XLNET_PARAM_ORDER = ("q", "k", "v", "o", "r", "r_w_bias", "r_r_bias", "ln1_w", "ln1_b", "w1", "b1",
                     "w2", "b2", "ln2_w", "ln2_b")


def xlnet_layer_ws_floats(B, L, D, n_head, dropout=False):
    return _lib.load().t4r_xlnet_layer_ws_floats(B, L, D, n_head, int(bool(dropout)))


def xlnet_layer_bwd_ws_floats(B, L, D, n_head, dropout=False):
    return _lib.load().t4r_xlnet_layer_bwd_ws_floats(B, L, D, n_head, int(bool(dropout)))


def xlnet_pos_emb_dropout(pos_emb, B, p, seed, offset):
    """dropout(pos_emb expanded over the batch) [B, 2L, D] with the key every layer uses (HF modeling_xlnet.py:1143
    drops it once per forward): pass the result as `pos_emb_b` to xlnet_layer_fwd / _bwd of all layers"""
    return dropout(pos_emb.contiguous().view(-1), p, seed, dropout_ctr_hi(offset, 255, SITE_POS), n_total=B * pos_emb.numel())


def xlnet_layer_fwd(h, pos_emb, params, B, L, n_head, eps, ws=None, drop_p=0.0, seed=0, offset=0,
                    layer_idx=0, key_len=None, pos_emb_b=None, stack_prepared=False, rows=None, n_rows=None, causal=False):
    """h [B*L, D]; params: sequence of 15 tensors in XLNET_PARAM_ORDER.  -> (h_out, ws)
    causal: the layer of attn_type='uni' (include/t4r_hip_uni.h: t4r_xlnet_layer_uni_fwd; no row map, no LAYER_FUSE_INPUT)
    stack_prepared: `ws` already holds this layer's weight planes and k_r (xlnet_stack_prepare)
    rows (int32, ascending, unique, first n_rows entries valid): the feed-forward block runs on these rows only and h_out is
    zero elsewhere (include/t4r_hip_rows.h: t4r_xlnet_layer_fwd_rows); the backward must be given the same map"""
    D = h.shape[-1]
    if ws is None:
        ws = torch.empty(xlnet_layer_ws_floats(B, L, D, n_head, drop_p > 0), device=h.device,
                         dtype=torch.float32)
    out = torch.empty_like(h)
    parr, _keep = ptr_array([_chk(p, torch.float32, "xlnet param") for p in params])
    flags = LAYER_STACK_PREPARED if stack_prepared else 0
    args = (_stream(), _chk(h, torch.float32), _chk(pos_emb, torch.float32), parr,
            ws.data_ptr(), out.data_ptr(), B, L, D, n_head, float(eps), float(drop_p), int(seed),
            int(offset), int(layer_idx) | flags, _p(key_len, torch.int32), _p(pos_emb_b, torch.float32))
    if causal:
        if rows is not None:
            raise ValueError("xlnet_layer_fwd: no row map with causal=True")
        call("t4r_xlnet_layer_uni_fwd", *args)
    elif rows is None:
        call("t4r_xlnet_layer_fwd", *args)
    else:
        call("t4r_xlnet_layer_fwd_rows", *args, _chk(rows, torch.int32), int(n_rows))
    return out, ws


def xlnet_stack_prepare(params_all, B, L, n_head, pos, drop, pos_dropout=None):
    """The prologue of a whole XLNet stack in two launches (csrc/xlnet_fused_attn.hip: t4r_xlnet_stack_prepare): the
    weight planes of every layer and every layer's k_r = pos @ r.  params_all: per layer the 15 tensors in
    XLNET_PARAM_ORDER; pos: what the layers would project ([B * 2L, D] dropped positional encoding, or [2L, D]).
    -> one workspace per layer, to be passed to xlnet_layer_fwd(..., ws=, stack_prepared=True)."""
    import ctypes

    D = params_all[0][0].shape[0]
    dev = params_all[0][0].device
    n_fl = xlnet_layer_ws_floats(B, L, D, n_head, drop)
    po, ko = ctypes.c_long(0), ctypes.c_long(0)
    call("t4r_xlnet_layer_ws_offsets", B, L, D, n_head, int(bool(drop)), ctypes.addressof(po), ctypes.addressof(ko))
    if po.value < 0:
        raise ValueError("xlnet_stack_prepare: no fused kernels for this width")
    ws = [torch.empty(n_fl, device=dev, dtype=torch.float32) for _ in params_all]
    flat = [_chk(t, torch.float32, "xlnet param") for layer in params_all for t in layer]
    parr, _k0 = ptr_array(flat)
    n = len(params_all)
    planes, _k1 = ptr_array([w.data_ptr() + 4 * po.value for w in ws])
    kr, _k2 = ptr_array([w.data_ptr() + 4 * ko.value for w in ws])
    pos2 = pos.reshape(-1, D)
    rows = pos2.shape[0]
    if pos_dropout is not None:
        # (p, seed, offset, out): `pos` is the plain [2L, D] encoding; the projection kernel masks it per session with this
        # forward's pos_emb dropout and leaves the dropped rows in out [B * 2L, D] (what xlnet_pos_emb_dropout returned)
        pd, seed, offset, out = pos_dropout
        call("t4r_xlnet_stack_prepare_drop", _stream(), parr, n, D, planes, _chk(pos2, torch.float32), B * rows, kr,
             float(pd), int(seed), dropout_ctr_hi(offset, 255, SITE_POS), rows, _chk(out, torch.float32))
    else:
        call("t4r_xlnet_stack_prepare", _stream(), parr, n, D, planes, _chk(pos2, torch.float32), rows, kr)
    return ws


def xlnet_layer_bwd(h, pos_emb, params, grads, ws, dh_out, B, L, n_head, eps, bws=None, drop_p=0.0,
                    seed=0, offset=0, layer_idx=0, key_len=None, pos_emb_b=None, defer_join=None, rows=None, n_rows=None,
                    causal=False):
    """causal: the forward was xlnet_layer_fwd(..., causal=True).
    rows, n_rows: the map the forward was given (xlnet_layer_fwd): dh_out is read at these rows only.
    defer_join: a list -> the call returns without waiting for its weight-gradient streams (csrc/xlnet_layer.hip:
    deferred join) and appends every buffer those streams may still be using to the list; the caller keeps the list
    alive until it has called xlnet_layer_bwd_join()."""
    D = h.shape[-1]
    if bws is None:
        bws = torch.empty(xlnet_layer_bwd_ws_floats(B, L, D, n_head, drop_p > 0), device=h.device,
                          dtype=torch.float32)
    dh_in = torch.empty_like(h)
    parr, _k1 = ptr_array([_chk(p, torch.float32) for p in params])
    garr, _k2 = ptr_array([_chk(g, torch.float32) for g in grads])
    flags = LAYER_DEFER_JOIN if defer_join is not None else 0
    args = (_stream(), _chk(h), _chk(pos_emb), parr, garr, _chk(ws),
            bws.data_ptr(), _chk(dh_out), dh_in.data_ptr(), B, L, D, n_head, float(eps), float(drop_p),
            int(seed), int(offset), int(layer_idx) | flags, _p(key_len, torch.int32), _p(pos_emb_b, torch.float32))
    if causal:
        if rows is not None:
            raise ValueError("xlnet_layer_bwd: no row map with causal=True")
        call("t4r_xlnet_layer_uni_bwd", *args)
    elif rows is None:
        call("t4r_xlnet_layer_bwd", *args)
    else:
        call("t4r_xlnet_layer_bwd_rows", *args, _chk(rows, torch.int32), int(n_rows))
    if defer_join is not None:
        defer_join.append((h, pos_emb, list(params), list(grads), ws, bws, dh_out, key_len, pos_emb_b, rows))
    return dh_in


def xlnet_layer_bwd_join():
    """the current stream waits for the weight-gradient streams of every deferred xlnet_layer_bwd call so far"""
    call("t4r_xlnet_layer_bwd_join", _stream())


# ------------------------------------------------------------------------------------ head
# ------------------------------------------------------------------------------------ fused XLNet layer pieces
def xlnet_fused_supported(D):
    return bool(_lib.load().t4r_xlnet_fused_supported(int(D)))


def xlnet_layer_prepare(params, D):
    """bf16 planes of a layer's nine weight matrices (csrc/xlnet_fused_attn.hip); params in XLNET_PARAM_ORDER"""
    planes = torch.empty(_lib.load().t4r_xlnet_layer_planes_floats(D), device=params[0].device, dtype=torch.float32)
    ptrs, _keep = ptr_array([_chk(t, torch.float32) for t in params])
    call("t4r_xlnet_layer_prepare", _stream(), ptrs, D, planes.data_ptr())
    return planes


def xlnet_qkv_proj(h, planes):
    T, D = h.shape
    qkv = torch.empty((3, T, D), device=h.device, dtype=torch.float32)
    call("t4r_xlnet_qkv_proj", _stream(), _chk(h, torch.float32), planes.data_ptr(), qkv.data_ptr(), T, D)
    return qkv


def xlnet_kr_proj(pos, planes):
    rows, D = pos.shape
    kr = torch.empty((rows, D), device=pos.device, dtype=torch.float32)
    call("t4r_xlnet_kr_proj", _stream(), _chk(pos, torch.float32), planes.data_ptr(), kr.data_ptr(), rows, D)
    return kr


def xlnet_oproj_ln(av, h, planes, gamma, beta, eps, drop=NO_DROP, train=True):
    T, D = av.shape
    h1 = torch.empty_like(av)
    ao = torch.empty_like(av) if train else None
    mean = torch.empty(T, device=av.device) if train else None
    rstd = torch.empty(T, device=av.device) if train else None
    call("t4r_xlnet_oproj_ln", _stream(), _chk(av, torch.float32), _chk(h, torch.float32), planes.data_ptr(), _chk(gamma),
         _chk(beta), _p(ao), _p(mean), _p(rstd), h1.data_ptr(), T, D, float(eps), float(drop[0]), int(drop[1]), int(drop[2]))
    return h1, ao, mean, rstd


def xlnet_ln1_bwd(dy, ao, h, mean, rstd, gamma, planes, d_gamma, d_beta, drop=NO_DROP):
    T, D = dy.shape
    dh, dao, dav = torch.empty_like(dy), torch.empty_like(dy), torch.empty_like(dy)
    part = torch.empty(max(1, _lib.load().t4r_xlnet_ln1_bwd_part_floats(T, D)), device=dy.device)
    call("t4r_xlnet_ln1_bwd", _stream(), _chk(dy), _chk(ao), _chk(h), _chk(mean), _chk(rstd), _chk(gamma), planes.data_ptr(),
         dh.data_ptr(), dao.data_ptr(), dav.data_ptr(), _chk(d_gamma), _chk(d_beta), part.data_ptr(), T, D, float(drop[0]),
         int(drop[1]), int(drop[2]))
    return dh, dao, dav


def xlnet_dh_(dqkv, planes, dh):
    _, T, D = dqkv.shape
    call("t4r_xlnet_dh", _stream(), _chk(dqkv, torch.float32), planes.data_ptr(), _chk(dh, torch.float32), T, D)
    return dh


_CU_BUDGET_SET = False


def xlnet_set_cu_budget(cus):
    """CUs the backward's token-tile kernels may plan for (0 = the whole chip); process-wide (csrc/xlnet_fused.hip)"""
    global _CU_BUDGET_SET
    _lib.load().t4r_xlnet_set_cu_budget(int(cus))
    _CU_BUDGET_SET = int(cus) > 0


def xlnet_clear_cu_budget():
    """no-op unless a budget is set: the safety net of a backward pass that raised before its reducer cleared it"""
    if _CU_BUDGET_SET:
        xlnet_set_cu_budget(0)


def device_cus():
    return int(_lib.load().t4r_device_cus())


def xlnet_get_cu_budget():
    return int(_lib.load().t4r_xlnet_get_cu_budget())


def xlnet_attn_block_supported(L, D, n_head):
    return bool(_lib.load().t4r_xlnet_attn_block_supported(int(L), int(D), int(n_head)))


def xlnet_attn_block_fwd(h, planes, o, kr, r_w_bias, r_r_bias, gamma, beta, B, L, n_head, eps, drop_p=0.0, seed=0, ctr_prob=0,
                         ctr_out=0, key_len=None, train=True, prob=None):
    """the attention half of a layer in one launch (csrc/xlnet_attn_block.hip): h [B L, D] -> h1, and what the backward needs.
    prob: a contiguous fp32 buffer of B n_head L L elements (16-byte aligned) that receives the probabilities before dropout
    (include/t4r_hip_attn.h)"""
    T, D = h.shape
    dev = h.device
    qkv = torch.empty((3, T, D), device=dev)
    av, h1 = torch.empty((T, D), device=dev), torch.empty((T, D), device=dev)
    lse = torch.empty((B, n_head, L), device=dev)
    ao = torch.empty((T, D), device=dev) if train else None
    mean = torch.empty(T, device=dev) if train else None
    rstd = torch.empty(T, device=dev) if train else None
    per_session = kr.shape[0] == B * 2 * L and B > 1
    head = (_stream(), _chk(h, torch.float32), planes.data_ptr(), _chk(o, torch.float32), _chk(kr, torch.float32),
            2 * L * D if per_session else 0, _chk(r_w_bias), _chk(r_r_bias), _chk(gamma), _chk(beta), qkv.data_ptr(), av.data_ptr(),
            lse.data_ptr())
    tail = (_p(ao), _p(mean), _p(rstd), h1.data_ptr(), B, L, D, n_head, float(eps), float(drop_p), int(seed),
            int(ctr_prob), int(ctr_out), _p(key_len, torch.int32))
    if prob is None:
        call("t4r_xlnet_attn_block_fwd", *head, *tail)
    else:
        call("t4r_xlnet_attn_block_fwd_prob", *head, _chk(prob, torch.float32), *tail)
    return h1, dict(qkv=qkv, av=av, lse=lse, ao=ao, mean=mean, rstd=rstd)


def xlnet_ff_fwd(h1, planes, b1, b2, gamma, beta, eps, drop_p=0.0, seed=0, ctr_act=0, ctr_out=0, train=True):
    T, D = h1.shape
    dev = h1.device
    hout = torch.empty_like(h1)
    saved = None
    if train:
        saved = dict(ffpre=torch.empty((T, 4 * D), device=dev), ffact=torch.empty((T, 4 * D), device=dev),
                     ffout=torch.empty((T, D), device=dev), mean=torch.empty(T, device=dev), rstd=torch.empty(T, device=dev))
    g = (lambda k: saved[k].data_ptr()) if train else (lambda k: None)
    call("t4r_xlnet_ff_fwd", _stream(), _chk(h1, torch.float32), planes.data_ptr(), _chk(b1), _chk(b2), _chk(gamma), _chk(beta),
         g("ffpre"), g("ffact"), g("ffout"), g("mean"), g("rstd"), hout.data_ptr(), T, D, float(eps), float(drop_p), int(seed),
         int(ctr_act), int(ctr_out))
    return hout, saved


def xlnet_ff_bwd(dy, h1, saved, gamma, planes, d_gamma, d_beta, d_b2, d_b1, drop_p=0.0, seed=0, ctr_act=0, ctr_out=0):
    T, D = dy.shape
    dh1, dffout = torch.empty_like(dy), torch.empty_like(dy)
    dpre = torch.empty((T, 4 * D), device=dy.device)
    part = torch.empty(max(1, _lib.load().t4r_xlnet_ff_bwd_part_floats(T, D)), device=dy.device)
    call("t4r_xlnet_ff_bwd", _stream(), _chk(dy), _chk(saved["ffout"]), _chk(h1), _chk(saved["mean"]), _chk(saved["rstd"]),
         _chk(gamma), _chk(saved["ffpre"]), planes.data_ptr(), dh1.data_ptr(), dffout.data_ptr(), dpre.data_ptr(),
         _chk(d_gamma), _chk(d_beta), _chk(d_b2), _chk(d_b1), part.data_ptr(), T, D, float(drop_p), int(seed), int(ctr_act),
         int(ctr_out))
    return dh1, dffout, dpre


def softmax_ce_fwd(logits, labels, V, label_smoothing=0.0):
    """logits [N, ld] view or buffer whose row stride is the leading dimension."""
    N = logits.shape[0]
    ld = logits.stride(0) if N > 1 else max(logits.shape[1], V)
    dev = logits.device
    loss_rows = torch.empty(N, device=dev, dtype=torch.float32)
    lse = torch.empty(N, device=dev, dtype=torch.float32)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    call("t4r_softmax_ce_fwd", _stream(), logits.data_ptr(), _chk(labels, torch.int64),
         loss_rows.data_ptr(), lse.data_ptr(), loss.data_ptr(), N, V, ld, float(label_smoothing))
    return loss, loss_rows, lse


def softmax_ce_bwd(logits, labels, lse, grad_out, V, label_smoothing=0.0):
    N = logits.shape[0]
    ld = logits.stride(0) if N > 1 else max(logits.shape[1], V)
    buf = torch.empty((N, ld), device=logits.device, dtype=torch.float32)
    call("t4r_softmax_ce_bwd", _stream(), logits.data_ptr(), _chk(labels, torch.int64), _chk(lse),
         _p(grad_out), buf.data_ptr(), N, V, ld, float(label_smoothing))
    return buf


_CHUNK_BYTES = int(__import__("os").environ.get("T4R_HEAD_CHUNK_MB", "96")) << 20


def head_chunk_cols(N, V):
    """columns per vocabulary chunk of the non-materialising head: the [N, chunk] logits buffer stays
    inside the 256 MB Infinity Cache (default 96 MB), a multiple of 1024 columns, at most V rounded up"""
    c = max(1024, (_CHUNK_BYTES // (4 * max(N, 1))) // 1024 * 1024)
    return int(min(c, (V + 1023) // 1024 * 1024))


def linear_softmax_ce_fwd(x, W, labels, alpha=1.0, label_smoothing=0.0, chunk_cols=None):
    """mean CE of softmax(alpha * x @ W^T) vs labels without an [N, V] tensor -> (loss, loss_rows, lse)"""
    N, D = x.shape
    V = W.shape[0]
    c = chunk_cols or head_chunk_cols(N, V)
    dev = x.device
    buf = torch.empty(_lib.load().t4r_linear_softmax_ce_chunk_floats(N, c), device=dev, dtype=torch.float32)
    stats = torch.empty(4 * N, device=dev, dtype=torch.float32)
    loss_rows = torch.empty(N, device=dev, dtype=torch.float32)
    lse = torch.empty(N, device=dev, dtype=torch.float32)
    loss = torch.empty((), device=dev, dtype=torch.float32)
    call("t4r_linear_softmax_ce_fwd", _stream(), _chk(x, torch.float32), x.stride(0), W.data_ptr(), W.stride(0),
         _chk(labels, torch.int64), N, V, D, float(alpha), float(label_smoothing), c, buf.data_ptr(),
         stats.data_ptr(), loss_rows.data_ptr(), lse.data_ptr(), loss.data_ptr())
    return loss, loss_rows, lse


def linear_softmax_ce_bwd(x, W, labels, lse, grad_out, dW=None, alpha=1.0, label_smoothing=0.0, chunk_cols=None):
    """-> dx [N, D]; dW [V, D] is accumulated into when given"""
    N, D = x.shape
    V = W.shape[0]
    c = chunk_cols or head_chunk_cols(N, V)
    buf = torch.empty(_lib.load().t4r_linear_softmax_ce_chunk_floats(N, c), device=x.device, dtype=torch.float32)
    dx = torch.empty((N, D), device=x.device, dtype=torch.float32)
    call("t4r_linear_softmax_ce_bwd", _stream(), _chk(x, torch.float32), x.stride(0), W.data_ptr(), W.stride(0),
         _chk(labels, torch.int64), _chk(lse, torch.float32), _p(grad_out), N, V, D, float(alpha),
         float(label_smoothing), c, buf.data_ptr(), dx.data_ptr(), D,
         None if dW is None else _chk(dW, torch.float32), 0 if dW is None else dW.stride(0))
    return dx


def sampled_logits_fwd(x, labels, W, neg, dist, temperature=1.0):
    N, D = x.shape
    S = neg.numel()
    out = torch.empty((N, S + 1), device=x.device, dtype=torch.float32)
    ws = torch.empty(max(1, S * D), device=x.device, dtype=torch.float32)
    call("t4r_sampled_logits_fwd", _stream(), _chk(x), _chk(labels, torch.int64), _chk(W),
         _chk(neg, torch.int64), _chk(dist, torch.float32), out.data_ptr(), N, D, S, float(temperature),
         ws.data_ptr())
    return out


def log_uniform_sample(n, min_id, max_id, seed, ctr_hi, device):
    """n ids ~ LogUniformSampler's distribution over [min_id, max_id) (with replacement), int64 [n]"""
    out = torch.empty(n, device=device, dtype=torch.int64)
    call("t4r_log_uniform_sample", _stream(), out.data_ptr(), int(n), int(min_id), int(max_id), int(seed), int(ctr_hi))
    return out


def sampled_logits_bwd(dlogits, x, labels, W, neg, dW, temperature=1.0):
    """dlogits is modified in place (entries of accidental hits are zeroed)"""
    N, D = x.shape
    dx = torch.empty_like(x)
    ws = torch.empty(2 * neg.numel() * D, device=x.device, dtype=torch.float32)
    call("t4r_sampled_logits_bwd", _stream(), _chk(dlogits), _chk(x), _chk(labels, torch.int64),
         _chk(W), _chk(neg, torch.int64), dx.data_ptr(), _chk(dW), ws.data_ptr(), N, D, neg.numel(),
         float(temperature))
    return dx


def sampled_logits_bwd_rows(dlogits, x, labels, W, neg, temperature=1.0):
    """row-sparse form: -> (dx [N, D], ids [N + S] = labels ++ neg, rows [N + S, D] gradient rows of W[ids]);
    dlogits is modified in place (entries of accidental hits are zeroed)"""
    N, D = x.shape
    S = neg.numel()
    dx = torch.empty_like(x)
    rows = torch.empty((N + S, D), device=x.device, dtype=torch.float32)
    ws = torch.empty(2 * S * D, device=x.device, dtype=torch.float32)
    call("t4r_sampled_logits_bwd_rows", _stream(), _chk(dlogits), _chk(x), _chk(labels, torch.int64),
         _chk(W), _chk(neg, torch.int64), dx.data_ptr(), rows.data_ptr(), ws.data_ptr(), N, D, S,
         float(temperature))
    ids = torch.cat([labels, neg.to(labels.dtype)])        # index glue (N + S int64)
    return dx, ids, rows


def scatter_rows_sorted(d_table, ids, rows, padding_idx=-1):
    """d_table[ids[i]] += rows[i], deterministic (sort + segmented sum); padding_idx = -1: every id counts"""
    keys, perm = sort_ids(ids, d_table.shape[0], padding_idx)
    embedding_bwd_sorted(rows, keys, perm, d_table, 0, rows.shape[1], 1)


def topk(scores, k, V=None):
    N = scores.shape[0]
    V = scores.shape[1] if V is None else V
    ld = _row_pitch(scores, scores.shape[1])
    vals = torch.empty((N, k), device=scores.device, dtype=torch.float32)
    idx = torch.empty((N, k), device=scores.device, dtype=torch.int64)
    call("t4r_topk", _stream(), scores.data_ptr(), N, V, ld, k, vals.data_ptr(), idx.data_ptr())
    return vals, idx


_ITEM_TOPK_WS_LIMIT = 2 << 30      # rows are chunked only where one call's workspace would pass 2 GiB


_H16 = {torch.bfloat16: 2, torch.float16: 3}      # serving-image dtypes -> the codes of T4R_GEMM_PREC
_H16_NAMES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def image_ld(D):
    """row pitch (elements) of a packed serving image of width D: a multiple of 16 >= D (t4r_item_table_image_ld)"""
    return int(_lib.load().t4r_item_table_image_ld(int(D)))


def item_topk_h16_supported(D):
    """True where the 16-bit head takes an item table of width D (1 <= D <= 512)"""
    return bool(_lib.load().t4r_item_topk_h16_supported(int(D)))


def pack_item_table(W, dtype="fp16"):
    """The SERVING IMAGE of an item table: W [V, D] fp32 rounded once (to nearest even) to fp16 / bf16, as a [V, D] view of
    a [V, image_ld(D)] buffer whose pad columns are zero and whose rows are 16-byte aligned -- `image.float()` is its exact
    value, W.to(dtype) its bits.  item_topk / item_scores take it in place of W (csrc/item_topk_h16.hip).  Raises for a table
    whose rounding is not finite (fp16 overflows above 65 504: no operand scaling, as under the reference's autocast)."""
    if dtype not in _H16_NAMES:
        raise ValueError(f"pack_item_table: dtype must be 'fp16' or 'bf16' (got {dtype!r})")
    if not W.is_cuda:
        raise _lib.T4RHipError(f"pack_item_table: W must be a HIP device tensor (got {W.device}); there is no CPU path")
    if W.dtype != torch.float32:
        raise TypeError(f"pack_item_table: W: expected torch.float32, got {W.dtype}")
    if W.dim() != 2 or W.stride(1) != 1:
        raise ValueError("pack_item_table: W must be 2-D row-major with unit inner stride")
    V, D = W.shape
    td = _H16_NAMES[dtype]
    ldp = image_ld(D)
    buf = torch.empty((V, ldp), device=W.device, dtype=td)
    call("t4r_item_table_pack_h16", _stream(), W.data_ptr(), _row_pitch(W, D), V, D, _H16[td], buf.data_ptr(), ldp)
    if not bool(torch.isfinite(buf).all()):         # once per table: the image is reused by every call
        raise ValueError(f"pack_item_table: the table does not round to finite {dtype} values")
    return buf[:, :D]


def _check_image(what, W, D):
    if W.shape[1] != D:
        raise ValueError(f"{what}: inner dims differ ({D} vs {W.shape[1]})")
    ldp = _row_pitch(W, image_ld(D))
    if ldp < image_ld(D) or ldp % 8 or W.data_ptr() % 16:
        raise ValueError(f"{what}: a 16-bit table must be a serving image (ops.pack_item_table): rows 16-byte aligned, "
                         f"pitch >= image_ld(D) = {image_ld(D)} with zero pad columns")
    if not _lib.load().t4r_item_topk_h16_supported(D):
        raise ValueError(f"{what}: the 16-bit head takes 1 <= D <= 512 (D = {D})")
    return ldp


def _check_x_w(what, x, W):
    for t, name in ((x, "x"), (W, "W")):
        if not t.is_cuda:
            raise _lib.T4RHipError(f"{what}: {name} must be a HIP device tensor (got {t.device}); there is no CPU path")
        if t.dtype != torch.float32 and not (name == "W" and t.dtype in _H16):
            raise TypeError(f"{what}: {name}: expected torch.float32" + (", torch.float16 or torch.bfloat16 (a serving image)"
                                                                         if name == "W" else "") + f", got {t.dtype}")
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{what}: {name} must be 2-D row-major with unit inner stride")


def item_scores(x, W, alpha=1.0):
    """alpha * x[N, D] @ W[V, D]^T as the [N, V] fp32 view of a row-padded buffer.  W fp32: gemm() under the current
    precision mode (what the task's inference call has always returned).  W a serving image (pack_item_table): one
    16-bit matrix-core product per multiply over x rounded to the image's dtype, fp32 accumulation -- the arithmetic of
    item_topk over that image, bit for bit."""
    _check_x_w("item_scores", x, W)
    N, D = x.shape
    V = W.shape[0]
    if W.dtype == torch.float32:
        if W.shape[1] != D:
            raise ValueError(f"item_scores: inner dims differ ({D} vs {W.shape[1]})")
        return gemm(x.contiguous(), W, False, True, alpha=alpha, ldc=pad_ld(V))[:, :V]
    ldp = _check_image("item_scores", W, D)
    ldc = pad_ld(V)
    out = torch.empty((N, ldc), device=x.device, dtype=torch.float32)
    if N and V:
        ws = torch.empty(N * image_ld(D) * 2, device=x.device, dtype=torch.uint8)
        call("t4r_item_scores_h16", _stream(), N, V, D, float(alpha), x.data_ptr(), _row_pitch(x, D), W.data_ptr(),
             ldp, _H16[W.dtype], out.data_ptr(), ldc, ws.data_ptr(), ws.numel())
    return out[:, :V]


def item_topk(x, W, k, alpha=1.0, *, allow_bits=None, exclude=None):
    """(values [N, k] fp32, ids [N, k] int64) of the k best items per row of alpha * x[N, D] @ W[V, D]^T, values descending,
    ties to the lower index: bit for bit topk(gemm(x, W, False, True, alpha), k) under precision("fp32"), without an [N, V]
    tensor (csrc/item_topk.hip).  x and W may be row-strided views (unit inner stride).
    W a serving image (pack_item_table, fp16 / bf16; x stays fp32): the same from one 16-bit matrix-core product per multiply,
    bit for bit topk(item_scores(x, W, alpha), k) (csrc/item_topk_h16.hip); the precision mode plays no part.
    allow_bits (pack_item_filter) / exclude (int64 [N, E], the items row n must not return; any order, -1 pads): only allowed
    items come back -- bit for bit topk(item_mask_(item_scores(x, W, alpha).clone(), allow_bits, exclude), k) with id -1 in
    every slot whose value is -inf (a row with fewer than k allowed items).  Both None: the unfiltered entry, as before."""
    return _item_head("item_topk", x, W, k, alpha, None, allow_bits, exclude)


def pack_item_filter(allow):
    """The catalogue filter of item_topk / item_sample / item_mask_: allow [V] bool or uint8 on the device (non-zero = the item
    may be returned) -> int32 [2 * ceil(V / 64)] bit words, bit (v & 31) of word (v >> 5) for item v, pad bits zero
    (include/t4r_hip_filter.h).  Pack once per catalogue state; every call reads it."""
    if not allow.is_cuda:
        raise _lib.T4RHipError(f"pack_item_filter: allow must be a HIP device tensor (got {allow.device}); there is no CPU path")
    if allow.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"pack_item_filter: allow: expected torch.bool or torch.uint8, got {allow.dtype}")
    if allow.dim() != 1:
        raise ValueError(f"pack_item_filter: allow must be [V] (got {tuple(allow.shape)})")
    V = allow.shape[0]
    bits = torch.empty(int(_lib.load().t4r_item_allow_words(V)), device=allow.device, dtype=torch.int32)
    if V:
        call("t4r_item_allow_pack", _stream(), allow.contiguous().view(torch.uint8).data_ptr(), V, bits.data_ptr())
    return bits


def _item_filter(what, ref, n_items, allow_bits, exclude):
    """checks of the two filter tensors against ref (a device tensor of the call with one row per list row) and the number of
    items the bits must cover; None if there is no filter, else (allow_bits or None, exclude sorted per row or None)"""
    if allow_bits is None and exclude is None:
        return None
    if allow_bits is not None:
        if not allow_bits.is_cuda:
            raise _lib.T4RHipError(f"{what}: allow_bits must be a HIP device tensor (got {allow_bits.device}); there is no CPU path")
        if allow_bits.dtype != torch.int32:
            raise TypeError(f"{what}: allow_bits: expected torch.int32 (ops.pack_item_filter), got {allow_bits.dtype}")
        words = int(_lib.load().t4r_item_allow_words(int(n_items)))
        if allow_bits.dim() != 1 or not allow_bits.is_contiguous() or allow_bits.shape[0] < words:
            raise ValueError(f"{what}: allow_bits must be a contiguous [>= {words}] word tensor for {n_items} items "
                             f"(ops.pack_item_filter; got {tuple(allow_bits.shape)})")
        if allow_bits.device != ref.device:
            raise ValueError(f"{what}: allow_bits is on {allow_bits.device}, the call on {ref.device}")
    if exclude is not None:
        if not exclude.is_cuda:
            raise _lib.T4RHipError(f"{what}: exclude must be a HIP device tensor (got {exclude.device}); there is no CPU path")
        if exclude.dtype != torch.int64:
            raise TypeError(f"{what}: exclude: expected torch.int64, got {exclude.dtype}")
        if exclude.dim() != 2 or exclude.shape[0] != ref.shape[0] or exclude.shape[1] > 1024:
            raise ValueError(f"{what}: exclude must be [N, E] = [{ref.shape[0]}, <= 1024] (got {tuple(exclude.shape)})")
        if exclude.device != ref.device:
            raise ValueError(f"{what}: exclude is on {exclude.device}, the call on {ref.device}")
        exclude = torch.sort(exclude, dim=1).values.contiguous() if exclude.shape[1] else None
    return allow_bits, exclude


def _filter_args(filt, s0):
    """the four trailing C arguments (allow_bits, excl, n_excl, ld_excl) with the list advanced to row s0"""
    bits, excl = filt
    if excl is None:
        return _p(bits), None, 0, 0
    return _p(bits), excl[s0:].data_ptr(), excl.shape[1], excl.shape[1]


def item_mask_(scores, allow_bits=None, exclude=None, item_stride=1):
    """in place: scores[r, c] = -inf where item c * item_stride is not allowed for row r -- its bit of allow_bits
    (pack_item_filter) is clear or it is in exclude[r] (int64 [N, E], any order, entries outside the items ignored) -- whatever
    the column held; allowed columns are not touched and the scores are never read (csrc/item_filter.hip).  scores fp32 [N, V],
    row-strided views allowed; returns scores.  The materialised form of the filter of item_topk / item_sample."""
    item_stride = int(item_stride)
    if item_stride < 1:
        raise ValueError(f"item_mask_: item_stride >= 1 (got {item_stride})")
    _check_scores("item_mask_", scores)
    N, V = scores.shape
    filt = _item_filter("item_mask_", scores, (V - 1) * item_stride + 1 if V else 0, allow_bits, exclude)
    if filt is not None and N and V:
        call("t4r_item_mask_f32", _stream(), scores.data_ptr(), N, V, _row_pitch(scores, V), item_stride, *_filter_args(filt, 0))
    return scores


def _item_head(what, x, W, k, alpha, noise, allow_bits=None, exclude=None):
    """item_topk (noise None) / item_sample (noise = (row0, seed, ctr_hi)): checks, workspace, row chunks, the stats record;
    with a filter part: the filtered entries, same workspaces"""
    _check_x_w(what, x, W)
    filt = _item_filter(what, x, W.shape[0], allow_bits, exclude)
    N, D = x.shape
    V = W.shape[0]
    k = int(k)
    if W.shape[1] != D:
        raise ValueError(f"{what}: inner dims differ ({D} vs {W.shape[1]})")
    if not 1 <= k <= min(256, V):
        raise ValueError(f"{what}: 1 <= k <= min(256, V) (k = {k}, V = {V})")
    h16 = W.dtype in _H16
    ldw = _check_image(what, W, D) if h16 else _row_pitch(W, D)
    vals = torch.empty((N, k), device=x.device, dtype=torch.float32)
    idx = torch.empty((N, k), device=x.device, dtype=torch.int64)
    if N == 0:
        return vals, idx
    lib = _lib.load()
    stem = "t4r_item_topk" if noise is None else "t4r_item_sample"
    entry = stem + ("_filtered" if filt is not None else "") + ("_h16" if h16 else "_f32")
    ws_bytes = getattr(lib, stem + ("_h16_ws_bytes" if h16 else "_ws_bytes"))
    rows = N
    while rows > 1 and ws_bytes(rows, V, D, k) > _ITEM_TOPK_WS_LIMIT:
        rows = (rows + 1) // 2
    ws = torch.empty(ws_bytes(rows, V, D, k), device=x.device, dtype=torch.uint8)
    ldx = _row_pitch(x, D)
    st = (ctypes.c_long * 8)()
    tot = dict(fallback_rows=0, cand_sum=0, cand_max=0)
    for s0 in range(0, N, rows):
        n = min(rows, N - s0)
        st[7] = int(_ITEM_TOPK["collect_counts"])
        table = (W.data_ptr(), ldw, _H16[W.dtype]) if h16 else (W.data_ptr(), ldw)
        tail = () if noise is None else (int(noise[0]) + s0, int(noise[1]), int(noise[2]))
        if filt is not None:
            tail += _filter_args(filt, s0)
        call(entry, _stream(), n, V, D, float(alpha), x[s0:].data_ptr(), ldx, *table, k, vals[s0:].data_ptr(),
             idx[s0:].data_ptr(), ws.data_ptr(), ws.numel(), ctypes.cast(st, ctypes.c_void_p), *tail)
        tot["fallback_rows"] += int(st[0])
        tot["cand_sum"] += int(st[3])
        tot["cand_max"] = max(tot["cand_max"], int(st[4]))
        _ITEM_TOPK["calls"] += 1
        _ITEM_TOPK["calls_h16"] += int(h16)
    _ITEM_TOPK.update(tot, sample_rows=int(st[1]), list_capacity=int(st[2]),       # summed over the row chunks of this call
                      dtype={torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}[W.dtype])
    return vals, idx


def _check_scores(what, scores):
    if not scores.is_cuda:
        raise _lib.T4RHipError(f"{what}: scores must be a HIP device tensor (got {scores.device}); there is no CPU path")
    if scores.dtype != torch.float32:
        raise TypeError(f"{what}: scores: expected torch.float32, got {scores.dtype}")
    if scores.dim() != 2 or (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise ValueError(f"{what}: scores must be 2-D row-major with unit inner stride")


def gumbel_add_(scores, seed, ctr_hi, row0=0):
    """in place: scores[r, c] = fp32(scores[r, c] + g(seed, ctr_hi, row0 + r, c)), g the Gumbel noise of
    include/t4r_hip_sampling.h (a pure function of its four arguments).  scores fp32 [N, V], row-strided views allowed;
    returns scores.  topk(gumbel_add_(s.clone(), ...), k) is a sample of k items without replacement from softmax(s)."""
    _check_scores("gumbel_add_", scores)
    N, V = scores.shape
    if N and V:
        call("t4r_gumbel_add_f32", _stream(), scores.data_ptr(), N, V, _row_pitch(scores, V), int(row0), 1, int(seed), int(ctr_hi))
    return scores


def gumbel_argmax(scores, seed, ctr_hi, row0=0):
    """(values [N] fp32, ids [N] int64): per row the largest fp32(scores[r, c] + g(seed, ctr_hi, row0 + r, c)) and its column,
    ties to the lower column -- one draw per row from softmax(scores[r]) -- in one pass and without a perturbed copy of scores;
    bit for bit topk(gumbel_add_(scores.clone(), ...), 1)."""
    _check_scores("gumbel_argmax", scores)
    N, V = scores.shape
    if V < 1:
        raise ValueError("gumbel_argmax: scores has no columns")
    vals = torch.empty(N, device=scores.device, dtype=torch.float32)
    idx = torch.empty(N, device=scores.device, dtype=torch.int64)
    if N:
        call("t4r_gumbel_argmax_f32", _stream(), scores.data_ptr(), N, V, _row_pitch(scores, V), int(row0), int(seed), int(ctr_hi),
             vals.data_ptr(), idx.data_ptr())
    return vals, idx


def item_sample(x, W, k, seed, ctr_hi, alpha=1.0, row0=0, *, allow_bits=None, exclude=None):
    """(values [N, k] fp32, ids [N, k] int64): k items per row drawn WITHOUT replacement in proportion to
    softmax(alpha * x @ W^T) (Gumbel top-k), without an [N, V] tensor: item_topk over the perturbed score
    fp32(s[r, v] + g(seed, ctr_hi, row0 + r, v)).  values are the perturbed scores, descending.  Bit for bit
    topk(gumbel_add_(item_scores(x, W, alpha).clone(), seed, ctr_hi, row0), k) -- for an fp32 W under precision("fp32").
    W fp32 or a serving image, x and W row-strided views as item_topk takes them; item_topk_stats() records the call.
    ctr_hi = dropout_ctr_hi(offset, 255, SITE_GUMBEL) by convention; the same (seed, ctr_hi, row0) replays the draw, and
    item_sample(x[a:b], ..., row0=a) is rows a..b-1 of the whole call.
    allow_bits / exclude as item_topk takes them: the draw is over the allowed items only (exclude[a:b] goes with x[a:b]);
    slots of value -inf have id -1."""
    if int(row0) < 0:
        raise ValueError(f"item_sample: row0 must not be negative (got {row0})")
    return _item_head("item_sample", x, W, k, alpha, (row0, seed, ctr_hi), allow_bits, exclude)


def item_eval(x, image, labels, alpha=1.0):
    """(lse, target, score_sum fp32 [N], rank int32 [N]) of the rows of item_scores(x, image, alpha) in ONE pass over the serving
    image, without the [N, V] scores (csrc/item_eval_h16.hip): lse = logsumexp of the row, target = its score of labels[n] (the
    bits item_scores returns), score_sum = the row's sum, rank = how many items beat the target (ties to the lower index, the
    rule of rank_of_target).  Cross entropy with label smoothing eps: (1 - eps)(lse - target) + eps (lse - score_sum / V).
    A label outside [0, V) gives target NaN and rank V.  image must be a serving image (pack_item_table); labels int64 [N].
    No synchronisation; a row's outputs do not depend on the other rows of the call."""
    if image.dtype == torch.float32:       # before the device checks: the one mistake a caller of item_scores / item_topk makes
        raise TypeError("item_eval: W must be a serving image (ops.pack_item_table(W, 'fp16' | 'bf16')), got torch.float32; "
                        "for an fp32 table use rank_of_target and linear_softmax_ce_fwd")
    _check_x_w("item_eval", x, image)
    if not labels.is_cuda:
        raise _lib.T4RHipError(f"item_eval: labels must be a HIP device tensor (got {labels.device}); there is no CPU path")
    if labels.dtype != torch.int64:
        raise TypeError(f"item_eval: labels: expected torch.int64, got {labels.dtype}")
    N, D = x.shape
    V = image.shape[0]
    if labels.dim() != 1 or labels.shape[0] != N:
        raise ValueError(f"item_eval: labels must be [N] = [{N}] (got {tuple(labels.shape)})")
    if V < 1:
        raise ValueError("item_eval: the image has no rows")
    ldp = _check_image("item_eval", image, D)
    labels = labels.contiguous()
    lse, target, score_sum = (torch.empty(N, device=x.device, dtype=torch.float32) for _ in range(3))
    rank = torch.empty(N, device=x.device, dtype=torch.int32)
    if N:
        ws = torch.empty(_lib.load().t4r_item_eval_h16_ws_bytes(N, V, D), device=x.device, dtype=torch.uint8)
        call("t4r_item_eval_h16", _stream(), N, V, D, float(alpha), x.data_ptr(), _row_pitch(x, D), image.data_ptr(),
             ldp, _H16[image.dtype], labels.data_ptr(), lse.data_ptr(), target.data_ptr(), score_sum.data_ptr(), rank.data_ptr(),
             ws.data_ptr(), ws.numel())
    return lse, target, score_sum, rank


# the record behind item_topk_stats(): kept here, the library has no state of its own
_ITEM_TOPK = dict(calls=0, calls_h16=0, dtype=None, fallback_rows=0, sample_rows=0, list_capacity=0, cand_sum=0, cand_max=0,
                  collect_counts=False)


def item_topk_stats():
    """{"calls": fused top-k launches of this process so far, "calls_h16": those of them over a 16-bit serving image; and of
    the last item_topk call: "dtype": "fp32" | "fp16" | "bf16" (what its table was), "fallback_rows": rows that
    overflowed their candidate list and were recomputed through the materialised path, "sample_rows" / "list_capacity": the
    sizes the launch chose, "cand_sum" / "cand_max": its candidate counts (only under item_topk_collect_counts(True))}"""
    return {k: v for k, v in _ITEM_TOPK.items() if k != "collect_counts"}


def item_topk_collect_counts(on):
    """tools: have every item_topk launch copy its per-row candidate counts back (item_topk_stats: cand_sum / cand_max)"""
    _ITEM_TOPK["collect_counts"] = bool(on)


# ------------------------------------------------------------------------------------ optimizer
def rank_of_target(x, W, labels, alpha=1.0, chunk=1024):
    """0-based rank of labels[i] among alpha * x[i] @ W^T (ties -> lower index first), int32 [N];
    the [N, V] scores are never materialised."""
    N, D = x.shape
    V = W.shape[0]
    rank = torch.empty(N, device=x.device, dtype=torch.int32)
    labels = labels.contiguous()
    # Target scores through the SAME kernel (diagonal of x_c @ W[y_c]^T), not a separate row-dot product: an output
    # element's bits do not depend on its tile position, so `score == target` detects exact ties (duplicated item rows)
    # and "ties go to the lower index" holds bit for bit, as in the top-k of the materialised scores.  A row-dot kernel
    # was tried in round 3 (cheaper by ~10 us) and broke exactly that: its rounding differs from the product's, so a tie
    # with a duplicate row turns into an arbitrary </> (tests/test_kernels_gpu.py::test_rank_of_target_matches_topk_and_sort).
    for s0 in range(0, N, chunk):
        xc, yc = x[s0: s0 + chunk], labels[s0: s0 + chunk]
        n = xc.shape[0]
        pos = yc.to(torch.int32)
        wy = gather_rows(W, pos, n)
        with precision("fp32"):         # the rank epilogue always runs on the fp32 matrix cores: same arithmetic here
            tgt = gemm(xc, wy, False, True, alpha=alpha).diagonal().contiguous()
        call("t4r_rank_of_target_f32", _stream(), n, V, D, float(alpha), _chk(xc, torch.float32), xc.stride(0),
             _chk(W, torch.float32), W.stride(0), _chk(tgt, torch.float32), _chk(yc, torch.int64),
             rank[s0: s0 + chunk].data_ptr())
    return rank


def adam_step_amax_(param, grad, exp_avg, exp_avg_sq, step, lo, hi, part, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                    weight_decay=0.0, grad_scale=1.0, zero_grad=True):
    """adam_step_ that also leaves the per-workgroup maxima of |param[lo:hi]| after the update in part[:n]; -> n"""
    lib = _lib.load()
    n = lib.t4r_adam_step_amax(_stream(), _chk(param, torch.float32), _chk(grad, torch.float32), _chk(exp_avg),
                               _chk(exp_avg_sq), param.numel(), int(step), float(lr), float(betas[0]), float(betas[1]),
                               float(eps), float(weight_decay), float(grad_scale), int(zero_grad), int(lo), int(hi),
                               _chk(part, torch.float32))
    if n < 0:
        raise _lib.T4RHipError(lib.t4r_last_error().decode())
    return n


def w_amax_of(W):
    """(partials, n) the optimizer left for parameter W (optim.FusedAdam: the maximum of the tied item table comes out of the
    Adam launch) if NOTHING has written W since -- same storage, same version counters -- else None"""
    rec = getattr(W, "_t4r_w_amax", None)
    if rec is None:
        return None
    part, n, ptr, v_param, flat, v_flat = rec
    if W.data_ptr() != ptr or W._version != v_param or flat._version != v_flat or not W.is_contiguous():
        return None
    return part, n


def adam_step_(param, grad, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
               weight_decay=0.0, grad_scale=1.0, zero_grad=True):
    call("t4r_adam_step", _stream(), _chk(param, torch.float32), _chk(grad, torch.float32),
         _chk(exp_avg), _chk(exp_avg_sq), param.numel(), int(step), float(lr), float(betas[0]),
         float(betas[1]), float(eps), float(weight_decay), float(grad_scale), int(zero_grad))


# ---- include/t4r_hip_optim.h: global-norm clipping and AdamW over flat buckets (optim.FusedAdam drives them)
def grad_sumsq_parts(n):
    """how many partials grad_sumsq_ over n elements writes (a pure function of n, <= 2048)"""
    return _lib.load().t4r_grad_sumsq_parts(int(n))


def grad_sumsq_(grad, part):
    """part[:count] (float64) = per-workgroup sums of grad^2, squared and added in double; -> count"""
    _chk(grad, torch.float32, "grad"), _chk(part, torch.float64, "part")
    lib = _lib.load()
    need = lib.t4r_grad_sumsq_parts(grad.numel())
    if part.numel() < need:
        raise ValueError(f"part holds {part.numel()} partials, {need} are written")
    n = lib.t4r_grad_sumsq(_stream(), grad.data_ptr(), grad.numel(), part.data_ptr())
    if n < 0:
        raise _lib.T4RHipError(lib.t4r_last_error().decode())
    return n


def grad_clip_coef_(part, n_part, grad_scale, max_norm, out):
    """out[0] = fp32(|grad_scale| * sqrt(sum part[:n_part])), out[1] = min(max_norm / (out[0] + 1e-6), 1): no host read"""
    _chk(part, torch.float64, "part"), _chk(out, torch.float32, "out")
    if not 1 <= n_part <= part.numel() or out.numel() < 2:
        raise ValueError("grad_clip_coef_: 1 <= n_part <= part.numel() and out of at least 2 floats")
    call("t4r_grad_clip_coef", _stream(), part.data_ptr(), int(n_part), float(grad_scale), float(max_norm), out.data_ptr())


def adamw_step_(param, grad, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                decoupled=False, grad_scale=1.0, zero_grad=True, clip_coef=None, amax=None):
    """adam_step_ with the gradient multiplied by the device scalar clip_coef (a 1-element fp32 tensor, or None) after
    grad_scale, and with torch.optim.AdamW's decoupled weight decay when `decoupled`.  amax = (lo, hi, part) as
    adam_step_amax_.  -> the number of workgroups (= partial maxima written when amax is given)"""
    lo, hi, part = amax if amax is not None else (0, 0, None)
    if clip_coef is not None and clip_coef.numel() != 1:
        raise ValueError("clip_coef is one float")
    lib = _lib.load()
    n = lib.t4r_adamw_step(_stream(), _chk(param, torch.float32), _chk(grad, torch.float32), _chk(exp_avg), _chk(exp_avg_sq),
                           param.numel(), int(step), float(lr), float(betas[0]), float(betas[1]), float(eps),
                           float(weight_decay), int(bool(decoupled)), float(grad_scale), int(zero_grad),
                           _p(clip_coef, torch.float32, "clip_coef"), int(lo), int(hi), _p(part, torch.float32, "amax part"))
    if n < 0:
        raise _lib.T4RHipError(lib.t4r_last_error().decode())
    return n


# ---- include/t4r_hip_rowadam.h: the row-sparse (lazy) Adam step of a table (optim.RowSparseAdam drives it)
def row_adam_step_(param, exp_avg, exp_avg_sq, ids, rows, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                   decoupled=False, grad_scale=1.0, padding_idx=-1):
    """One Adam / AdamW step of the rows of `param` [V, D] that `ids` names, with the gradient of row r = the sum of rows[i]
    over ids[i] == r in lookup order (the bits of scatter_rows_sorted into a zeroed buffer); every other row of param and of
    the two moments is neither read nor written.  ids int64 [n]; rows fp32 [n, D], unit inner stride, any row pitch >= D;
    ids equal to padding_idx or outside [0, V) carry nothing."""
    for t, name in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (ids, "ids"), (rows, "rows")):
        if not t.is_cuda:
            raise _lib.T4RHipError(f"row_adam_step_: {name} must live on the GPU (got {t.device}); there is no CPU path")
    if param.dim() != 2 or exp_avg.shape != param.shape or exp_avg_sq.shape != param.shape:
        raise ValueError("row_adam_step_: param, exp_avg and exp_avg_sq are [V, D] tensors of one shape")
    V, D = param.shape
    ids = ids.reshape(-1)
    n = ids.numel()
    if rows.dim() != 2 or rows.shape != (n, D) or rows.dtype != torch.float32 or (D > 1 and rows.stride(1) != 1):
        raise ValueError(f"row_adam_step_: rows must be fp32 [{n}, {D}] with unit inner stride")
    if n == 0:
        return
    ld = _row_pitch(rows, D)
    if ld < D:
        raise ValueError("row_adam_step_: the row pitch of rows must be at least D")
    keys, perm = sort_ids(ids, V, padding_idx)
    nb = _lib.load().t4r_row_adam_ws_bytes(n, D)
    ws = torch.empty(max(nb, 1), device=param.device, dtype=torch.uint8)
    call("t4r_row_adam_step", _stream(), _chk(param, torch.float32, "param"), _chk(exp_avg, torch.float32, "exp_avg"),
         _chk(exp_avg_sq, torch.float32, "exp_avg_sq"), V, D, keys.data_ptr(), perm.data_ptr(), rows.data_ptr(), ld, n,
         int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(bool(decoupled)),
         float(grad_scale), ws.data_ptr(), nb)


# ---- include/t4r_hip_rowclip.h: the same step in two halves, for a global norm over dense buckets and lazily stepped tables
# (optim.FusedAdam(max_grad_norm=).link(RowSparseAdam) drives them)
def row_grad_sumsq_parts(n, D):
    """how many partials row_adam_reduce_ over n lookups of width D writes (a pure function of (n, D), <= 2048)"""
    return _lib.load().t4r_row_grad_sumsq_parts(int(n), int(D))


class RowAdamReduced:
    """what row_adam_reduce_ leaves for row_adam_apply_: the workspace (ranks, table rows, the compact summed gradient) and the
    (n, V, D) it was laid out for.  Opaque; good for one apply."""
    __slots__ = ("ws", "nbytes", "n", "V", "D")

    def __init__(self, ws, nbytes, n, V, D):
        self.ws, self.nbytes, self.n, self.V, self.D = ws, nbytes, n, V, D


def row_adam_reduce_(ids, rows, V, padding_idx, part):
    """The first half of row_adam_step_ for a table of V rows: sorts the ids, sums rows[i] per distinct valid id into a compact
    buffer (the bits of scatter_rows_sorted into a zeroed [V, D] buffer) and writes part[:count] (float64) = per-workgroup sums
    of the squares of those sums, squared and added in double -- the table's share of the global gradient norm, ready to stand
    beside grad_sumsq_'s partials in front of grad_clip_coef_.  count = row_grad_sumsq_parts(n, D) whatever the ids are;
    slots beyond it are untouched.  -> (count, state for row_adam_apply_).  ids int64 [n]; rows fp32 [n, D], unit inner stride, any
    row pitch >= D; ids equal to padding_idx or outside [0, V) carry nothing."""
    for t, name in ((ids, "ids"), (rows, "rows"), (part, "part")):
        if not t.is_cuda:
            raise _lib.T4RHipError(f"row_adam_reduce_: {name} must live on the GPU (got {t.device}); there is no CPU path")
    ids = ids.reshape(-1)
    n = ids.numel()
    if rows.dim() != 2 or rows.shape[0] != n or rows.dtype != torch.float32 or (rows.shape[1] > 1 and rows.stride(1) != 1):
        raise ValueError(f"row_adam_reduce_: rows must be fp32 [{n}, D] with unit inner stride")
    D = rows.shape[1]
    V = int(V)
    if V < 1 or D < 1:
        raise ValueError("row_adam_reduce_: V and D must be at least 1")
    _chk(part, torch.float64, "part")
    lib = _lib.load()
    need = lib.t4r_row_grad_sumsq_parts(n, D)
    if part.numel() < need:
        raise ValueError(f"part holds {part.numel()} partials, {need} are written")
    if n == 0:
        return 0, RowAdamReduced(None, 0, 0, V, D)
    ld = _row_pitch(rows, D)
    if ld < D:
        raise ValueError("row_adam_reduce_: the row pitch of rows must be at least D")
    keys, perm = sort_ids(ids, V, padding_idx)
    nb = lib.t4r_row_adam_ws_bytes(n, D)
    ws = torch.empty(max(nb, 1), device=rows.device, dtype=torch.uint8)
    cnt = lib.t4r_row_adam_reduce(_stream(), V, D, keys.data_ptr(), perm.data_ptr(), rows.data_ptr(), ld, n, ws.data_ptr(), nb,
                                  part.data_ptr())
    if cnt < 0:
        raise _lib.T4RHipError(lib.t4r_last_error().decode())
    return cnt, RowAdamReduced(ws, nb, n, V, D)


def row_adam_apply_(param, exp_avg, exp_avg_sq, state, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                    decoupled=False, grad_scale=1.0, clip_coef=None):
    """The second half: one Adam / AdamW step of the rows of `param` [V, D] that the ids of `state`'s row_adam_reduce_ named,
    with the gradient (sum * grad_scale) * clip_coef -- clip_coef a 1-element fp32 device tensor (grad_clip_coef_'s out[1:]) or
    None (1: the bits of row_adam_step_).  Every other row of param and of the two moments is neither read nor written."""
    for t, name in ((param, "param"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        if not t.is_cuda:
            raise _lib.T4RHipError(f"row_adam_apply_: {name} must live on the GPU (got {t.device}); there is no CPU path")
    if not isinstance(state, RowAdamReduced):
        raise TypeError("row_adam_apply_: state is what row_adam_reduce_ returned")
    if param.dim() != 2 or exp_avg.shape != param.shape or exp_avg_sq.shape != param.shape:
        raise ValueError("row_adam_apply_: param, exp_avg and exp_avg_sq are [V, D] tensors of one shape")
    if tuple(param.shape) != (state.V, state.D):
        raise ValueError(f"row_adam_apply_: the rows were reduced for a [{state.V}, {state.D}] table, param is {tuple(param.shape)}")
    if clip_coef is not None and clip_coef.numel() != 1:
        raise ValueError("clip_coef is one float")
    if state.n == 0:
        return
    if state.ws is None:
        raise RuntimeError("row_adam_apply_: this state was applied already; the workspace is good for one apply")
    call("t4r_row_adam_apply", _stream(), _chk(param, torch.float32, "param"), _chk(exp_avg, torch.float32, "exp_avg"),
         _chk(exp_avg_sq, torch.float32, "exp_avg_sq"), state.V, state.D, state.n, int(step), float(lr), float(betas[0]),
         float(betas[1]), float(eps), float(weight_decay), int(bool(decoupled)), float(grad_scale),
         _p(clip_coef, torch.float32, "clip_coef"), state.ws.data_ptr(), state.nbytes)
    state.ws = None                            # consumed: the workspace is undefined after the apply


# ------------------------------------------------------------------------------------ pretrained-embedding features
# (include/t4r_hip_pretrained.h, csrc/pretrained_proj.hip)
def _pretrained_image(what, image, ids, E):
    for t, name in ((image, "image"), (ids, "ids")):
        if not t.is_cuda:
            raise _lib.T4RHipError(f"{what}: {name} must be a HIP device tensor (got {t.device}); there is no CPU path")
    if image.dtype not in _H16:
        raise TypeError(f"{what}: image: expected a 16-bit serving image (ops.pack_item_table), got {image.dtype}")
    if image.dim() != 2 or image.stride(1) != 1 or image.shape[1] != E:
        raise ValueError(f"{what}: image must be a row-major [rows, {E}] view of a packed table")
    return _row_pitch(image, image_ld(E))


def pretrained_proj_ws_bytes(E, P):
    return int(_lib.load().t4r_pretrained_proj_ws_bytes(int(E), int(P)))


def pretrained_proj_fwd(image, ids, W, b, ln_w=None, ln_b=None, eps=1e-5, T=None, out=None, col=0, err_flag=None, save=True):
    """rows of the packed fp16 table `image` [V, E] gathered by ids (int64, T tokens or T / L per-session ids) and projected by
    W [P, E], b [P] (+ LayerNorm ln_w, ln_b) in one kernel -> (out, xhat, rstd): out [T, P] fp32, or columns [col, col + P) of the
    given 2-D `out`; xhat [T, P], rstd [T] what pretrained_proj_bwd needs (None without LayerNorm or with save=False)."""
    P, E = W.shape
    ldp = _pretrained_image("pretrained_proj_fwd", image, ids, E)
    T = ids.numel() if T is None else int(T)
    if ids.numel() == 0 or T % ids.numel():
        raise ValueError(f"pretrained_proj_fwd: {ids.numel()} ids do not divide {T} tokens")
    if out is None:
        out = torch.empty((T, P), device=image.device, dtype=torch.float32)
    ln = ln_w is not None
    xhat = torch.empty((T, P), device=image.device, dtype=torch.float32) if ln and save else None
    rstd = torch.empty(T, device=image.device, dtype=torch.float32) if ln and save else None
    ws = torch.empty(max(16, pretrained_proj_ws_bytes(E, P)), device=image.device, dtype=torch.uint8)
    call("t4r_pretrained_proj_fwd", _stream(), _H16[image.dtype], image.data_ptr(), ldp, image.shape[0],
         _chk(ids, torch.int64, "ids"), T, T // ids.numel(), _chk(W, torch.float32, "W"), _p(b, torch.float32, "b"),
         _p(ln_w, torch.float32, "ln_w"), _p(ln_b, torch.float32, "ln_b"), float(eps), E, P,
         out.data_ptr(), _row_pitch(out, out.shape[1]), int(col), _p(xhat), _p(rstd), ws.data_ptr(), _p(err_flag, torch.int32, "err_flag"))
    return out, xhat, rstd


def pretrained_proj_bwd(dout, image, ids, ln_w, xhat, rstd, d_W, d_b, d_ln_w=None, d_ln_b=None, col=0):
    """the parameter gradients of pretrained_proj_fwd, ACCUMULATED into d_W [P, E], d_b [P] (and d_ln_w, d_ln_b [P]), from
    columns [col, col + P) of dout [..., ld]; the table has no gradient.  Bit-reproducible (no float atomics)."""
    P, E = d_W.shape
    ldp = _pretrained_image("pretrained_proj_bwd", image, ids, E)
    ld = dout.shape[-1]
    T = dout.numel() // ld
    if ids.numel() == 0 or T % ids.numel():
        raise ValueError(f"pretrained_proj_bwd: {ids.numel()} ids do not divide {T} tokens")
    ws = torch.empty(max(4, _lib.load().t4r_pretrained_proj_bwd_ws_floats(T, E, P)), device=dout.device, dtype=torch.float32)
    call("t4r_pretrained_proj_bwd", _stream(), _H16[image.dtype], image.data_ptr(), ldp, image.shape[0],
         _chk(ids, torch.int64, "ids"), T, T // ids.numel(), _chk(dout, torch.float32, "dout"), ld, int(col),
         _p(ln_w, torch.float32, "ln_w"), _p(xhat), _p(rstd), E, P, _chk(d_W, torch.float32, "d_W"), _p(d_b, torch.float32, "d_b"),
         _p(d_ln_w), _p(d_ln_b), ws.data_ptr())


# ------------------------------------------------------------------------------------ continuous-feature projection
# (include/t4r_hip_contproj.h, csrc/cont_proj.hip): the first layer of `continuous_projection`
def cont_proj_supported(C, P):
    return bool(_lib.load().t4r_cont_proj_supported(int(C), int(P)))


def _cont_proj_args(what, xs, per_session, weight, bias, T=None):
    """checks of the arguments both directions share -> (T, L, C, P, host array of the C column pointers, host array of the
    flags); T (tokens) is the size of the [B, L] columns, and has to be given where every column is per-session.  (Kept short:
    at the sizes of an input block the call is a few launches, and the host's share of it counts.)"""
    C = len(xs)
    if C == 0 or C != len(per_session):
        raise ValueError(f"{what}: xs and per_session must be non-empty lists of one length")
    if weight.dim() != 2 or weight.shape[1] != C or bias.dim() != 1 or bias.shape[0] != weight.shape[0]:
        raise ValueError(f"{what}: weight must be [P, {C}] and bias [P], got {tuple(weight.shape)} and {tuple(bias.shape)}")
    P = weight.shape[0]
    if C > 64 or not 1 <= P <= 1024:
        raise ValueError(f"{what}: C = {C}, P = {P} outside 1 <= C <= 64, 1 <= P <= 1024")
    ptrs, flags = (ctypes.c_void_p * C)(), (ctypes.c_int * C)()
    n_seq = n_ses = None
    for i, x in enumerate(xs):
        ptrs[i] = _chk(x, torch.float32, "xs")
        n = x.numel()
        if per_session[i]:
            flags[i] = 1
            if n_ses is not None and n != n_ses:
                raise ValueError(f"{what}: the per-session columns must share one size")
            n_ses = n
        else:
            if n_seq is not None and n != n_seq:
                raise ValueError(f"{what}: the sequence columns must share one size")
            n_seq = n
    _chk(weight, torch.float32, "weight")
    _chk(bias, torch.float32, "bias")
    if T is None:
        if n_seq is None:
            raise ValueError(f"{what}: every column is per-session: the token count T has to be given")
        T = n_seq
    elif n_seq is not None and n_seq != T:
        raise ValueError(f"{what}: the sequence columns hold {n_seq} values for {T} tokens")
    L = 1
    if n_ses is not None:
        if n_ses == 0 or T % n_ses:
            raise ValueError(f"{what}: {n_ses} per-session values do not divide {T} tokens")
        L = T // n_ses
    return int(T), L, C, P, ptrs, flags


def cont_proj_fwd(xs, per_session, weight, bias, T=None):
    """relu(bias + weight @ [x_0 .. x_{C-1}]) per token without the [T, C] operand: xs the C column tensors, fp32 [B, L] or --
    where per_session[c] -- [B] (broadcast over the sequence); weight [P, C], bias [P] -> rows [T, P], T = B * L (taken
    from the [B, L] columns; to be given where there is none)"""
    T, L, C, P, ptrs, flags = _cont_proj_args("cont_proj_fwd", xs, per_session, weight, bias, T)
    out = torch.empty((T, P), device=weight.device, dtype=torch.float32)
    call("t4r_cont_proj_fwd", _stream(), ptrs, flags, T, L, C, P, weight.data_ptr(), bias.data_ptr(), out.data_ptr())
    return out


def cont_proj_bwd_(dout2d, col, xs, per_session, weight, bias, d_w, d_b, want_dpre=False):
    """the parameter gradients of cont_proj_fwd, ACCUMULATED into d_w [P, C] and d_b [P], from columns [col, col + P) of dout2d
    [T, ld]; the ReLU mask is recomputed from the inputs.  Bit-reproducible (no float atomics).  -> the masked gradient [T, P]
    when want_dpre, else None"""
    if not dout2d.is_cuda:
        raise _lib.T4RHipError(f"cont_proj_bwd_: dout2d must live on the GPU (got {dout2d.device}); there is no CPU path")
    if dout2d.dim() != 2:
        raise ValueError(f"cont_proj_bwd_: dout2d must be 2-D, got {tuple(dout2d.shape)}")
    T, L, C, P, ptrs, flags = _cont_proj_args("cont_proj_bwd_", xs, per_session, weight, bias, dout2d.shape[0])
    if col < 0 or dout2d.shape[1] < col + P:
        raise ValueError(f"cont_proj_bwd_: dout2d must be [{T}, >= col + {P}], got {tuple(dout2d.shape)} with col = {col}")
    if d_w.shape != weight.shape or d_b.shape != bias.shape:
        raise ValueError("cont_proj_bwd_: d_w and d_b must have the shapes of weight and bias")
    ld = dout2d.shape[1]
    dpre = torch.empty((T, P), device=weight.device, dtype=torch.float32) if want_dpre else None
    ws = torch.empty(max(1, _lib.load().t4r_cont_proj_bwd_ws_floats(T, C, P)), device=weight.device, dtype=torch.float32)
    call("t4r_cont_proj_bwd", _stream(), _chk(dout2d, torch.float32, "dout2d"), ld, int(col), ptrs, flags, T, L, C, P,
         weight.data_ptr(), bias.data_ptr(), _chk(d_w, torch.float32, "d_w"), _chk(d_b, torch.float32, "d_b"), _p(dpre),
         ws.data_ptr())
    return dpre


# ------------------------------------------------------------------------------------------------ session-level tasks
# (include/t4r_hip_seqtask.h, csrc/seq_task.hip): summary over the sequence + Linear(D, 1) + sigmoid / identity + BCE / MSE
SUMMARY = {"first": 0, "last": 1, "mean": 2}
ACT_NONE, ACT_SIGMOID = 0, 1
LOSS_MSE, LOSS_BCE = 0, 1


def seq_task_supported(L, D):
    return bool(_lib.load().t4r_seq_task_supported(int(L), int(D)))


def _seq_task_args(what, x, lengths, weight, bias, target, summary, act, loss_kind):
    if not x.is_cuda:
        raise _lib.T4RHipError(f"{what}: x must live on the GPU (got {x.device}); there is no CPU path")
    if x.dim() != 3:
        raise ValueError(f"{what}: x must be [B, L, D], got {tuple(x.shape)}")
    B, L, D = x.shape
    if B and not seq_task_supported(L, D):
        raise ValueError(f"{what}: 1 <= L <= 1023 and 1 <= D <= 1024 (got L = {L}, D = {D})")
    if weight.numel() != D:
        raise ValueError(f"{what}: weight must hold D = {D} values, got {tuple(weight.shape)}")
    if bias is not None and bias.numel() != 1:
        raise ValueError(f"{what}: bias must hold one value, got {tuple(bias.shape)}")
    if lengths is not None and tuple(lengths.shape) != (B,):
        raise ValueError(f"{what}: lengths must be int32 [{B}], got {tuple(lengths.shape)}")
    if target is not None and tuple(target.shape) != (B,):
        raise ValueError(f"{what}: target must be [{B}], got {tuple(target.shape)}")
    if summary not in (0, 1, 2) or act not in (0, 1) or loss_kind not in (0, 1) or (loss_kind == LOSS_BCE and act == ACT_NONE):
        raise ValueError(f"{what}: summary in 0..2, act in 0..1, loss_kind in 0..1, BCE over act 1 only "
                         f"(got {summary}, {act}, {loss_kind})")
    return B, L, D


def _seq_task_ws(B, D, device):
    return torch.empty(max(1, _lib.load().t4r_seq_task_ws_floats(B, D)), device=device, dtype=torch.float32)


def seq_task_fwd(x, lengths, weight, bias, target, summary, act, loss_kind):
    """x [B, L, D] -> (s [B, D], pred [B], loss [1]): the summary of every session (summary 0 first, 1 last, 2 mean; lengths
    int32 [B] or None = all L positions), pred = act(bias + weight . s) (act 1 sigmoid, 0 identity) and, with a target [B], the
    mean row loss (loss_kind 0 MSE, 1 BCE).  target None: inference, loss is an empty tensor.  Two launches (one)."""
    B, L, D = _seq_task_args("seq_task_fwd", x, lengths, weight, bias, target, summary, act, loss_kind)
    s = torch.empty((B, D), device=x.device, dtype=torch.float32)
    pred = torch.empty((B,), device=x.device, dtype=torch.float32)
    loss = torch.empty((1 if target is not None else 0,), device=x.device, dtype=torch.float32)
    if target is not None and B == 0:
        loss.fill_(float("nan"))                # the mean of no rows, as torch's losses
    ws = _seq_task_ws(B, D, x.device) if target is not None else None
    call("t4r_seq_task_fwd", _stream(), _chk(x, torch.float32, "x"), _p(lengths, torch.int32, "lengths"), B, L, D, int(summary),
         _chk(weight, torch.float32, "weight"), _p(bias, torch.float32, "bias"), int(act), int(loss_kind),
         _p(target, torch.float32, "target"), s.data_ptr(), pred.data_ptr(), loss.data_ptr() if target is not None else None,
         _p(ws))
    return s, pred, loss


def seq_task_bwd_(g, pred, target, s, lengths, L, weight, summary, act, loss_kind, d_w=None, d_b=None):
    """the backward of seq_task_fwd from its notes (s, pred): -> dx [B, L, D], every element written; the parameter gradients are
    ACCUMULATED into d_w (weight's shape) and d_b ([1]), either may be None.  g: device tensor of one value, the gradient of
    the loss.  Bit-reproducible (no float atomics).  Two launches (one without d_w and d_b)."""
    if not s.is_cuda:
        raise _lib.T4RHipError(f"seq_task_bwd_: s must live on the GPU (got {s.device}); there is no CPU path")
    if s.dim() != 2:
        raise ValueError(f"seq_task_bwd_: s must be [B, D], got {tuple(s.shape)}")
    B, D = s.shape
    if B and not seq_task_supported(L, D):
        raise ValueError(f"seq_task_bwd_: 1 <= L <= 1023 and 1 <= D <= 1024 (got L = {L}, D = {D})")
    if weight.numel() != D or tuple(pred.shape) != (B,) or tuple(target.shape) != (B,) or g.numel() != 1:
        raise ValueError("seq_task_bwd_: weight must hold D values, pred and target must be [B], g one value")
    if lengths is not None and tuple(lengths.shape) != (B,):
        raise ValueError(f"seq_task_bwd_: lengths must be int32 [{B}], got {tuple(lengths.shape)}")
    if (d_w is not None and d_w.numel() != D) or (d_b is not None and d_b.numel() != 1):
        raise ValueError("seq_task_bwd_: d_w must hold D values and d_b one")
    if summary not in (0, 1, 2) or act not in (0, 1) or loss_kind not in (0, 1) or (loss_kind == LOSS_BCE and act == ACT_NONE):
        raise ValueError(f"seq_task_bwd_: summary in 0..2, act in 0..1, loss_kind in 0..1, BCE over act 1 only "
                         f"(got {summary}, {act}, {loss_kind})")
    dx = torch.empty((B, int(L), D), device=s.device, dtype=torch.float32)
    ws = _seq_task_ws(B, D, s.device)
    call("t4r_seq_task_bwd", _stream(), _chk(g, torch.float32, "g"), _chk(pred, torch.float32, "pred"),
         _chk(target, torch.float32, "target"), _chk(s, torch.float32, "s"), _p(lengths, torch.int32, "lengths"), B, int(L), D,
         int(summary), _chk(weight, torch.float32, "weight"), int(act), int(loss_kind), dx.data_ptr(),
         _p(d_w, torch.float32, "d_w"), _p(d_b, torch.float32, "d_b"), ws.data_ptr())
    return dx


# ------------------------------------------------------------------------------------------------ replaced-token detection
# (include/t4r_hip_rtd.h, csrc/rtd_head.hip): Linear(D, D) + erf-GELU / ReLU + Linear(D, 1) + BCE-with-logits over the active tokens
RTD_ACT = {"gelu": 0, "relu": 1}


def rtd_head_supported(D):
    return bool(_lib.load().t4r_rtd_head_supported(int(D)))


def _rtd_head_args(what, x, active, labels, W1, b1, w2, act):
    if not x.is_cuda:
        raise _lib.T4RHipError(f"{what}: x must live on the GPU (got {x.device}); there is no CPU path")
    if x.dim() != 2:
        raise ValueError(f"{what}: x must be [T, D], got {tuple(x.shape)}")
    T, D = x.shape
    if not rtd_head_supported(D):
        raise ValueError(f"{what}: D must be a multiple of 16 with 16 <= D <= 512 (got D = {D})")
    if tuple(W1.shape) != (D, D) or b1.numel() != D or w2.numel() != D:
        raise ValueError(f"{what}: W1 must be [{D}, {D}], b1 and w2 must hold D = {D} values "
                         f"(got {tuple(W1.shape)}, {tuple(b1.shape)}, {tuple(w2.shape)})")
    for name, m in (("active", active), ("labels", labels)):
        if m is not None and (tuple(m.shape) != (T,) or m.dtype not in (torch.bool, torch.uint8)):
            raise ValueError(f"{what}: {name} must be bool / uint8 [{T}], got {m.dtype} {tuple(m.shape)}")
    if act not in (0, 1):
        raise ValueError(f"{what}: act must be 0 (erf-GELU) or 1 (ReLU), got {act}")
    return T, D


def _rtd_u8(m):
    if m is None:
        return None
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _rtd_head_ws(T, D, device):
    return torch.empty(max(1, _lib.load().t4r_rtd_head_ws_floats(T, D)), device=device, dtype=torch.float32)


def rtd_head_fwd(x, active, labels, W1, b1, w2, b2, act):
    """x [T, D] -> (z [T], n_active int32 [1], loss [1]): z = b2 + w2 . act(b1 + W1 x) for every token (act 0 erf-GELU, 1 ReLU)
    and, with labels (bool / uint8 [T]), the mean of binary_cross_entropy_with_logits(z, labels) over the tokens where active
    (bool / uint8 [T]; None = all) is set, and their count n; n = 0 gives loss 0.  labels None: inference, n_active and loss
    are empty tensors.  Two launches (one)."""
    T, D = _rtd_head_args("rtd_head_fwd", x, active, labels, W1, b1, w2, act)
    if b2.numel() != 1:
        raise ValueError(f"rtd_head_fwd: b2 must hold one value, got {tuple(b2.shape)}")
    train = labels is not None
    z = torch.empty((T,), device=x.device, dtype=torch.float32)
    n_active = torch.zeros((1 if train else 0,), device=x.device, dtype=torch.int32)
    loss = torch.zeros((1 if train else 0,), device=x.device, dtype=torch.float32)
    ws = _rtd_head_ws(T, D, x.device) if train else None
    act_u8, lab_u8 = _rtd_u8(active), _rtd_u8(labels)
    call("t4r_rtd_head_fwd", _stream(), _chk(x, torch.float32, "x"), _p(act_u8, torch.uint8, "active"),
         _p(lab_u8, torch.uint8, "labels"), T, D, _chk(W1, torch.float32, "W1"), _chk(b1, torch.float32, "b1"),
         _chk(w2, torch.float32, "w2"), _chk(b2, torch.float32, "b2"), int(act), z.data_ptr(),
         n_active.data_ptr() if train else None, loss.data_ptr() if train else None, _p(ws))
    return z, n_active, loss


def rtd_head_bwd_(g, x, active, labels, z, n_active, W1, b1, w2, act, d_W1=None, d_b1=None, d_w2=None, d_b2=None):
    """the backward of rtd_head_fwd from what it wrote (z, n_active): -> dx [T, D], every element written; the parameter
    gradients are ACCUMULATED into d_W1 [D, D], d_b1 [D], d_w2 (D values), d_b2 [1], each of which may be None.  g: device
    tensor of one value, the gradient of the loss.  Bit-reproducible (no float atomics).  Three launches (two without d_W1,
    one without any parameter gradient)."""
    T, D = _rtd_head_args("rtd_head_bwd_", x, active, labels, W1, b1, w2, act)
    if labels is None:
        raise ValueError("rtd_head_bwd_: labels are needed")
    if tuple(z.shape) != (T,) or n_active.numel() != 1 or g.numel() != 1:
        raise ValueError(f"rtd_head_bwd_: z must be [{T}], n_active and g one value each")
    if ((d_W1 is not None and tuple(d_W1.shape) != (D, D)) or (d_b1 is not None and d_b1.numel() != D)
            or (d_w2 is not None and d_w2.numel() != D) or (d_b2 is not None and d_b2.numel() != 1)):
        raise ValueError("rtd_head_bwd_: d_W1 must be [D, D], d_b1 and d_w2 must hold D values and d_b2 one")
    dx = torch.empty((T, D), device=x.device, dtype=torch.float32)
    ws = _rtd_head_ws(T, D, x.device)
    act_u8, lab_u8 = _rtd_u8(active), _rtd_u8(labels)
    call("t4r_rtd_head_bwd", _stream(), _chk(g, torch.float32, "g"), _chk(x, torch.float32, "x"),
         _p(act_u8, torch.uint8, "active"), _chk(lab_u8, torch.uint8, "labels"), _chk(z, torch.float32, "z"),
         _chk(n_active, torch.int32, "n_active"), T, D, _chk(W1, torch.float32, "W1"), _chk(b1, torch.float32, "b1"),
         _chk(w2, torch.float32, "w2"), int(act), dx.data_ptr(), _p(d_W1, torch.float32, "d_W1"),
         _p(d_b1, torch.float32, "d_b1"), _p(d_w2, torch.float32, "d_w2"), _p(d_b2, torch.float32, "d_b2"), ws.data_ptr())
    return dx


# ------------------------------------------------------------------------------------------------ post-context fusion
# (include/t4r_hip_postfusion.h, csrc/post_fusion.hip): seq * (1 + Linear(ctx)), seq + Linear(ctx) or seq | ctx per token
FUSION = {"elementwise-mul": 0, "elementwise-sum": 1, "concat": 2}
FUSION_MUL, FUSION_SUM, FUSION_CONCAT = 0, 1, 2


def post_fusion_supported(D, C):
    return bool(_lib.load().t4r_post_fusion_supported(int(D), int(C)))


def _post_fusion_args(what, seq, ctx, weight, bias, mode, width=None):
    """checks both directions share -> (T, L, D, C, per_session); seq [B, L, D] (its place is taken by dout [B, L, width] in the
    backward), ctx [B, L, C] or [B, C]"""
    if not seq.is_cuda or not ctx.is_cuda:
        raise _lib.T4RHipError(f"{what}: the tensors must live on the GPU (got {seq.device}, {ctx.device}); there is no CPU path")
    if mode not in (0, 1, 2):
        raise ValueError(f"{what}: mode must be 0 (elementwise-mul), 1 (elementwise-sum) or 2 (concat), got {mode}")
    if seq.dim() != 3 or ctx.dim() not in (2, 3) or ctx.shape[0] != seq.shape[0] or (ctx.dim() == 3 and ctx.shape[1] != seq.shape[1]):
        raise ValueError(f"{what}: seq must be [B, L, D] and ctx [B, L, C] or [B, C], got {tuple(seq.shape)} and {tuple(ctx.shape)}")
    B, L, Dw = seq.shape
    C = ctx.shape[-1]
    D = Dw if width is None else width
    if not (1 <= D <= 1024 and 1 <= C <= 256):
        raise ValueError(f"{what}: D = {D}, C = {C} outside 1 <= D <= 1024, 1 <= C <= 256")
    if mode == FUSION_CONCAT:
        if weight is not None or bias is not None:
            raise ValueError(f"{what}: concat has no parameters")
    elif weight is None or bias is None or tuple(weight.shape) != (D, C) or tuple(bias.shape) != (D,):
        raise ValueError(f"{what}: weight must be [{D}, {C}] and bias [{D}]")
    return B * L, max(L, 1), D, C, int(ctx.dim() == 2)


def post_fusion_fwd(seq, ctx, weight, bias, mode):
    """seq [B, L, D], ctx [B, L, C] or -- session-level, row b serves every position of session b -- [B, C]; weight [D, C], bias
    [D] (None for concat) -> out [B, L, D] = seq * (1 + p) (mode 0) or seq + p (1) with p = bias + ctx weight^T, or [B, L, D + C]
    = seq | ctx (2).  One launch."""
    T, L, D, C, per_session = _post_fusion_args("post_fusion_fwd", seq, ctx, weight, bias, mode)
    out = torch.empty((seq.shape[0], seq.shape[1], D + C if mode == FUSION_CONCAT else D), device=seq.device, dtype=torch.float32)
    call("t4r_post_fusion_fwd", _stream(), _chk(seq, torch.float32, "seq"), _chk(ctx, torch.float32, "ctx"),
         _p(weight, torch.float32, "weight"), _p(bias, torch.float32, "bias"), out.data_ptr(), T, L, D, C, int(mode), per_session)
    return out


def post_fusion_bwd_(dout, seq, ctx, weight, bias, mode, d_w=None, d_b=None, want_dseq=True, want_dctx=True):
    """the backward of post_fusion_fwd (p is recomputed; nothing is saved): -> (dseq [B, L, D] or None, dctx of ctx's shape or
    None); the parameter gradients are ACCUMULATED into d_w [D, C] and d_b [D], either may be None.  seq may be None where it is
    not read (modes 1 and 2).  Bit-reproducible (no float atomics).  At most three launches."""
    D = weight.shape[0] if weight is not None else dout.shape[-1] - ctx.shape[-1]
    T, L, D, C, per_session = _post_fusion_args("post_fusion_bwd_", dout, ctx, weight, bias, mode, width=D)
    if dout.shape[-1] != (D + C if mode == FUSION_CONCAT else D):
        raise ValueError(f"post_fusion_bwd_: dout's width {dout.shape[-1]} does not fit D = {D}, C = {C}, mode {mode}")
    if mode == FUSION_MUL and (seq is None or tuple(seq.shape) != tuple(dout.shape)):
        raise ValueError("post_fusion_bwd_: elementwise-mul needs seq of dout's shape")
    if (d_w is not None and (weight is None or d_w.shape != weight.shape)) or (d_b is not None and (bias is None or d_b.shape != bias.shape)):
        raise ValueError("post_fusion_bwd_: d_w and d_b must have the shapes of weight and bias")
    dseq = torch.empty(tuple(dout.shape[:2]) + (D,), device=dout.device, dtype=torch.float32) if want_dseq else None
    dctx = torch.empty_like(ctx) if want_dctx else None
    ws = torch.empty(max(1, _lib.load().t4r_post_fusion_bwd_ws_floats(T, L, D, C, int(mode), per_session)), device=dout.device,
                     dtype=torch.float32)
    call("t4r_post_fusion_bwd", _stream(), _chk(dout, torch.float32, "dout"), _p(seq, torch.float32, "seq"),
         _chk(ctx, torch.float32, "ctx"), _p(weight, torch.float32, "weight"), _p(bias, torch.float32, "bias"), _p(dseq), _p(dctx),
         _p(d_w, torch.float32, "d_w"), _p(d_b, torch.float32, "d_b"), ws.data_ptr(), T, L, D, C, int(mode), per_session)
    return dseq, dctx


# ------------------------------------------------------------------------------------------------ MLP block
# (include/t4r_hip_mlpblock.h, csrc/mlp_block.hip): a stack of 1 .. 4 layers dropout(relu(Linear(.))) per token, one launch forward
SITE_MLP_BLOCK = 8          # the dropout site of the block: ctr_hi of layer i = dropout_ctr_hi(offset, i, SITE_MLP_BLOCK)
MLP_MAX_LAYERS, MLP_MAX_K0, MLP_MAX_N = 4, 1024, 512


def mlp_stack_supported(K0, dims):
    dims = [int(d) for d in dims]
    if not dims:
        return False
    _, keep = int_array(dims)
    return bool(_lib.load().t4r_mlp_stack_supported(len(dims), int(K0), keep))


def _mlp_stack_args(what, x, weights, biases):
    """checks both directions share -> (T, K0, dims); x [..., K0] (its place is taken by dout [..., N_last] in the backward)"""
    if not x.is_cuda:
        raise _lib.T4RHipError(f"{what}: the tensors must live on the GPU (got {x.device}); there is no CPU path")
    n = len(weights)
    if not 1 <= n <= MLP_MAX_LAYERS:
        raise ValueError(f"{what}: 1 <= n <= {MLP_MAX_LAYERS} layers, got {n}")
    if biases is not None and len(biases) != n:
        raise ValueError(f"{what}: biases must be None or one entry (a tensor or None) per layer")
    K0 = weights[0].shape[1]
    dims, k = [], K0
    for i, w in enumerate(weights):
        if w.dim() != 2 or w.shape[1] != k:
            raise ValueError(f"{what}: weight {i} must be [N_{i}, {k}], got {tuple(w.shape)}")
        k = w.shape[0]
        dims.append(k)
        b = None if biases is None else biases[i]
        if b is not None and tuple(b.shape) != (k,):
            raise ValueError(f"{what}: bias {i} must be [{k}], got {tuple(b.shape)}")
    if not (1 <= K0 <= MLP_MAX_K0 and all(1 <= d <= MLP_MAX_N for d in dims)):
        raise ValueError(f"{what}: widths {K0} -> {dims} outside 1 <= K0 <= {MLP_MAX_K0}, 1 <= N_i <= {MLP_MAX_N}")
    if x.dim() < 1:
        raise ValueError(f"{what}: the input must have at least one dimension")
    return (x.numel() // x.shape[-1] if x.shape[-1] else 0), K0, dims


def mlp_stack_fwd(x, weights, biases=None, relu=True, drop=(0.0, 0, 0), save_acts=False):
    """x [..., K0]; weights: n tensors [N_i, K_i] (torch.nn.Linear's layout), biases: None or n entries (tensor [N_i] or None);
    drop = (p, seed, offset): dropout after every layer at site SITE_MLP_BLOCK of stream position `offset`.
    -> out [..., N_last], or, save_acts (training), the list of every layer's output a_i [..., N_i] (the backward reads them).
    One launch; without save_acts the intermediate activations never reach memory."""
    T, K0, dims = _mlp_stack_args("mlp_stack_fwd", x, weights, biases)
    if x.shape[-1] != K0:
        raise ValueError(f"mlp_stack_fwd: the input is {x.shape[-1]} wide, the first weight takes {K0}")
    n, lead = len(dims), tuple(x.shape[:-1])
    outs = [torch.empty(lead + (d,), device=x.device, dtype=torch.float32) for d in (dims if save_acts else dims[-1:])]
    Np, keepN = int_array(dims)
    Wp, keepW = ptr_array([_chk(w, torch.float32, "weight") for w in weights])
    Bp, keepB = (None, None) if biases is None else ptr_array([_p(b, torch.float32, "bias") for b in biases])
    Ap, keepA = ptr_array([o.data_ptr() for o in outs]) if save_acts else (None, None)
    call("t4r_mlp_stack_fwd", _stream(), _chk(x, torch.float32, "x"), Wp, Bp, Ap, None if save_acts else outs[0].data_ptr(), T, n, K0,
         Np, int(bool(relu)), float(drop[0]), int(drop[1]), int(drop[2]))
    return outs if save_acts else outs[0]


def mlp_stack_bwd_(dout, x, weights, acts, relu=True, drop=(0.0, 0, 0), d_weights=None, d_biases=None, want_dx=True):
    """the backward of mlp_stack_fwd(save_acts=True): -> dx [..., K0] or None; the parameter gradients are ACCUMULATED into
    d_weights[i] [N_i, K_i] and d_biases[i] [N_i] (either list, and any entry, may be None).  x may be None where d_weights[0] and
    d_biases[0] are.  Bit-reproducible (no float atomics).  At most three launches."""
    T, K0, dims = _mlp_stack_args("mlp_stack_bwd_", dout, weights, None)
    n = len(dims)
    if dout.shape[-1] != dims[-1]:
        raise ValueError(f"mlp_stack_bwd_: dout is {dout.shape[-1]} wide, the last layer gives {dims[-1]}")
    if acts is None or len(acts) != n:
        raise ValueError("mlp_stack_bwd_: acts must be the n tensors mlp_stack_fwd(save_acts=True) returned (entries may be None "
                         "where they are not read)")
    for name, lst, like in (("d_weights", d_weights, weights), ("d_biases", d_biases, [w[:, 0] for w in weights])):
        if lst is not None and (len(lst) != n or any(g is not None and g.shape != p.shape for g, p in zip(lst, like))):
            raise ValueError(f"mlp_stack_bwd_: {name} must be None or one entry (a tensor of the parameter's shape, or None) per layer")
    lead = tuple(dout.shape[:-1])
    dx = torch.empty(lead + (K0,), device=dout.device, dtype=torch.float32) if want_dx else None
    Np, keepN = int_array(dims)
    ws = torch.empty(max(1, _lib.load().t4r_mlp_stack_bwd_ws_floats(T, n, K0, Np)), device=dout.device, dtype=torch.float32)
    Wp, keepW = ptr_array([_chk(w, torch.float32, "weight") for w in weights])
    Ap, keepA = ptr_array([_p(t, torch.float32, "acts") for t in acts])
    Gp, keepG = (None, None) if d_weights is None else ptr_array([_p(g, torch.float32, "d_weights") for g in d_weights])
    Hp, keepH = (None, None) if d_biases is None else ptr_array([_p(g, torch.float32, "d_biases") for g in d_biases])
    call("t4r_mlp_stack_bwd", _stream(), _chk(dout, torch.float32, "dout"), _p(x, torch.float32, "x"), Wp, Ap, _p(dx), Gp, Hp,
         ws.data_ptr(), T, n, K0, Np, int(bool(relu)), float(drop[0]), int(drop[1]), int(drop[2]))
    return dx


# ------------------------------------------------------------------------------------------------ GRU body
# (include/t4r_hip_gru.h, csrc/gru.hip): a stack of 1 .. 4 GRU layers over [B, L, K0], one launch per layer for the time loop
SITE_GRU = 9                # the dropout site between the layers: ctr_hi of layer k = dropout_ctr_hi(offset, k, SITE_GRU)
GRU_MAX_LAYERS, GRU_MAX_K0, GRU_MAX_H, GRU_MAX_L = 4, 1024, 128, 1023


def gru_supported(n, K0, H, L=1):
    return bool(_lib.load().t4r_gru_supported(int(n), int(K0), int(H), int(L)))


def _gru_args(what, x, w_ih, w_hh, b_ih, b_hh, h0, width):
    """checks both directions share -> (B, L, n, K0, H); x [B, L, width] (its place is taken by dout [B, L, H] in the backward)"""
    if not x.is_cuda:
        raise _lib.T4RHipError(f"{what}: the tensors must live on the GPU (got {x.device}); there is no CPU path")
    n = len(w_ih)
    if not 1 <= n <= GRU_MAX_LAYERS or len(w_hh) != n:
        raise ValueError(f"{what}: 1 <= n <= {GRU_MAX_LAYERS} layers with one W_ih and one W_hh each, got {n} and {len(w_hh)}")
    if x.dim() != 3:
        raise ValueError(f"{what}: the input must be [B, L, width] (batch_first), got {tuple(x.shape)}")
    H, K0 = w_hh[0].shape[1], w_ih[0].shape[1]
    for k in range(n):
        K = K0 if k == 0 else H
        if tuple(w_ih[k].shape) != (3 * H, K) or tuple(w_hh[k].shape) != (3 * H, H):
            raise ValueError(f"{what}: layer {k} must have W_ih [{3 * H}, {K}] and W_hh [{3 * H}, {H}], got "
                             f"{tuple(w_ih[k].shape)} and {tuple(w_hh[k].shape)}")
        for name, bs in (("b_ih", b_ih), ("b_hh", b_hh)):
            if bs is not None and (len(bs) != n or (bs[k] is not None and tuple(bs[k].shape) != (3 * H,))):
                raise ValueError(f"{what}: {name} must be None or one entry ([{3 * H}] or None) per layer")
    B, L = int(x.shape[0]), int(x.shape[1])
    if x.shape[2] != (K0 if width == "in" else H):
        raise ValueError(f"{what}: the tensor is {x.shape[2]} wide, expected {K0 if width == 'in' else H}")
    if not gru_supported(n, K0, H, max(L, 1)) or L < 1:
        raise ValueError(f"{what}: n {n}, K0 {K0}, H {H}, L {L} outside 1 <= n <= {GRU_MAX_LAYERS}, 1 <= K0 <= {GRU_MAX_K0}, "
                         f"1 <= H <= {GRU_MAX_H}, 1 <= L <= {GRU_MAX_L}")
    if h0 is not None and tuple(h0.shape) != (n, B, H):
        raise ValueError(f"{what}: h0 must be None or [{n}, {B}, {H}], got {tuple(h0.shape)}")
    return B, L, n, K0, H


def _gru_ptrs(lst, name):
    return (None, None) if lst is None else ptr_array([_p(t, torch.float32, name) for t in lst])


def gru_fwd(x, w_ih, w_hh, b_ih=None, b_hh=None, h0=None, drop=(0.0, 0, 0), save=False):
    """x [B, L, K0]; w_ih: n tensors [3H, K_k], w_hh: n tensors [3H, H] (torch.nn.GRU's layout, gates r | z | n), b_ih / b_hh: None
    or n entries (tensor [3H] or None); h0: None or [n, B, H]; drop = (p, seed, offset): dropout between the layers at site
    SITE_GRU of stream position `offset`.  -> out [B, L, H], or, save (training), (out, saved) with `saved` what gru_bwd_ reads.
    Two launches per layer, none per time step."""
    B, L, n, K0, H = _gru_args("gru_fwd", x, w_ih, w_hh, b_ih, b_hh, h0, "in")
    lib = _lib.load()
    out = torch.empty((B, L, H), device=x.device, dtype=torch.float32)
    saved = torch.empty(max(1, lib.t4r_gru_saved_floats(B, L, n, K0, H)), device=x.device, dtype=torch.float32) if save else None
    ws = torch.empty(max(1, lib.t4r_gru_fwd_ws_floats(B, L, n, K0, H)), device=x.device, dtype=torch.float32)
    Ip, keepI = ptr_array([_chk(w, torch.float32, "w_ih") for w in w_ih])
    Hp, keepH = ptr_array([_chk(w, torch.float32, "w_hh") for w in w_hh])
    Bi, keepBi = _gru_ptrs(b_ih, "b_ih")
    Bh, keepBh = _gru_ptrs(b_hh, "b_hh")
    call("t4r_gru_fwd", _stream(), _chk(x, torch.float32, "x"), _p(h0, torch.float32, "h0"), Ip, Hp, Bi, Bh, out.data_ptr(),
         _p(saved), ws.data_ptr(), B, L, n, K0, H, float(drop[0]), int(drop[1]), int(drop[2]))
    return (out, saved) if save else out


def gru_bwd_(dout, x, w_ih, w_hh, out, saved, h0=None, drop=(0.0, 0, 0), d_w_ih=None, d_w_hh=None, d_b_ih=None, d_b_hh=None,
             want_dx=True):
    """the backward of gru_fwd(save=True): -> dx [B, L, K0] or None; the parameter gradients are ACCUMULATED into d_w_ih[k],
    d_w_hh[k], d_b_ih[k], d_b_hh[k] (any list, and any entry, may be None).  x may be None where d_w_ih[0] and d_b_ih[0] are.
    Bit-reproducible (no float atomics).  At most four launches per layer."""
    B, L, n, K0, H = _gru_args("gru_bwd_", dout, w_ih, w_hh, None, None, h0, "out")
    for name, lst, like in (("d_w_ih", d_w_ih, w_ih), ("d_w_hh", d_w_hh, w_hh), ("d_b_ih", d_b_ih, [w[:, 0] for w in w_ih]),
                            ("d_b_hh", d_b_hh, [w[:, 0] for w in w_hh])):
        if lst is not None and (len(lst) != n or any(g is not None and g.shape != p.shape for g, p in zip(lst, like))):
            raise ValueError(f"gru_bwd_: {name} must be None or one entry (a tensor of the parameter's shape, or None) per layer")
    lib = _lib.load()
    if tuple(out.shape) != (B, L, H) or saved is None or saved.numel() < lib.t4r_gru_saved_floats(B, L, n, K0, H):
        raise ValueError("gru_bwd_: out and saved must be what gru_fwd(save=True) returned")
    dx = torch.empty((B, L, K0), device=dout.device, dtype=torch.float32) if want_dx else None
    ws = torch.empty(max(1, lib.t4r_gru_bwd_ws_floats(B, L, n, K0, H)), device=dout.device, dtype=torch.float32)
    Ip, keepI = ptr_array([_chk(w, torch.float32, "w_ih") for w in w_ih])
    Hp, keepH = ptr_array([_chk(w, torch.float32, "w_hh") for w in w_hh])
    G = [_gru_ptrs(g, nm) for g, nm in ((d_w_ih, "d_w_ih"), (d_w_hh, "d_w_hh"), (d_b_ih, "d_b_ih"), (d_b_hh, "d_b_hh"))]
    call("t4r_gru_bwd", _stream(), _chk(dout, torch.float32, "dout"), _p(x, torch.float32, "x"), _p(h0, torch.float32, "h0"), Ip, Hp,
         _chk(out, torch.float32, "out"), _chk(saved, torch.float32, "saved"), _p(dx), G[0][0], G[1][0], G[2][0], G[3][0],
         ws.data_ptr(), B, L, n, K0, H, float(drop[0]), int(drop[1]), int(drop[2]))
    return dx
