"""Red-zone and poison tests of the C ABI (include/t4r_hip.h): where an entry point writes, and what it reads that it was
never given.

Every case builds ALL device buffers of one entry-point call inside an abi_arena.Arena -- guards of 64 KiB on both sides of
every payload, workspaces of exactly the bytes the size query returns, pad columns and neighbouring column blocks at the fill
byte or at live values -- and runs

  1. under fill 0x00: arena.check() (no byte outside the entry's output windows changed), outputs against an fp64 torch
     reference at the tolerance the entry's existing value test uses (cited per case), integer outputs bit-exact;
  2. under fill 0xFF (NaN in every float format, -1 in every integer type): arena.check(), outputs bit-identical to run 1
     (entries that sum with fp32 atomics: ATOMIC_ENTRIES, run 1's tolerance), no non-finite value in a logical output;
  3. another case of the same family, then run 1's case again: bit-identical to run 1 (state carried between calls).

Buffers are handed to the library with _lib.call (the ops.* wrappers allocate outputs and workspaces themselves); ops.gemm
takes caller-owned strided views and is used as is.
"""
import ctypes
import math
import os
import sys

import pytest
import torch

from abi_arena import Arena

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8

# Entries whose sums go through fp32 atomics (arrival order): compared at run 1's tolerance, not bit for bit, under the second
# fill and in the rerun.  Each with the source line of its atomic.
ATOMIC_ENTRIES = {
    "t4r_embedding_bwd": "csrc/embedding.hip:533-544 embedding_bwd kernels, atomicAdd(dtable + id * dim + c, ...)",
    "t4r_add_pos_bwd": "csrc/elementwise.hip:559 add_pos_bwd_kernel, atomicAdd(dpos + l * D + c, acc)",
    "t4r_gemm_f32 (splitk != 1)": "csrc/gemm_kernel.h:772 split-K epilogue, atomicAdd(cp, v)",
    "t4r_gemm_wgrad_f32 (*bypassed == 1 only)": "csrc/gemm_kernel.h:772, the same split-K epilogue",
    "t4r_gemm_softmax_grad_f32 (splitk != 1)": "csrc/gemm_kernel.h:772, the same split-K epilogue",
    "t4r_sampled_logits_bwd": "csrc/head.hip:353 sampled_bwd kernel, atomicAdd(dW + yi * D + d, ...)",
}


def _lib():
    from transformers4rec_amd import _lib as L

    return L


def _ops():
    from transformers4rec_amd import ops

    return ops


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, scale=1.0):
    return scale * torch.randn(*shape, generator=g)


_MEMO = {}


def memo(key, thunk):
    """references are computed once per case and shared by its three runs"""
    if key not in _MEMO:
        _MEMO[key] = thunk()
    return _MEMO[key]


class Out:
    """one checked output: the arena buffer, its reference (None: checked for containment / reproducibility only), the
    tolerance (None: bit-exact against the reference) and the existing test the tolerance is taken from"""

    def __init__(self, buf, ref=None, tol=None, cite="", atomic=False, sel=None):
        # sel: a quantity derived from the buffer on the host (compared at its tolerance in every run; the buffer's own bits are
        # a separate Out)
        self.buf, self.ref, self.tol, self.cite, self.atomic, self.sel = buf, ref, tol, cite, atomic or sel is not None, sel

    def value(self):
        v = self.buf.win
        return v if self.sel is None else self.sel(v)


def call(a, name, *args):
    if not a.sealed:
        a.seal()
    _lib().call(name, *args)


def rc_call(a, name, *args):
    """entries whose return value is a count, not a status"""
    if not a.sealed:
        a.seal()
    return getattr(_lib().load(), name)(*args)


class Case:
    def __init__(self, family, cid, entries, fn):
        self.family, self.id, self.entries, self.fn = family, cid, tuple(entries), fn


CASES = []


def case(family, cid, entries):
    def deco(fn):
        CASES.append(Case(family, cid, entries, fn))
        return fn
    return deco


def cased_entries():
    return sorted({e for c in CASES for e in c.entries})


# =========================================================================================== element-wise and optimiser
def _mul(n):
    def fn(a, key):
        g = gen(n)
        x, y = rn(g, n), rn(g, n)
        A, B = a.new("a", "in", F32, n).set(x), a.new("b", "in", F32, n).set(y)
        O = a.new("out", "out", F32, n)
        call(a, "t4r_mul", stream(), A.ptr, B.ptr, O.ptr, n)
        return [Out(O, x * y, None, "fp32 product is correctly rounded: exact")]
    return fn


for _n in (1, 255, 256, 257):       # mul_kernel: 256 threads per workgroup, one element each
    case("elementwise", f"mul-{_n}", ["t4r_mul"])(_mul(_n))


def _dropout(n, n_src, p):
    def fn(a, key):
        import device_rng as R
        ops = _ops()
        g = gen(n + n_src)
        x = rn(g, n_src)
        seed, ctr = 11, ops.dropout_ctr_hi(3, 1, ops.SITE_INPUT)
        X = a.new("x", "in", F32, n_src).set(x)
        O = a.new("out", "out", F32, n)
        M = a.new("mask", "out", U8, n)
        call(a, "t4r_dropout", stream(), X.ptr, O.ptr, M.ptr, n, n_src, p, seed, ctr)
        keep = memo(key, lambda: torch.from_numpy(R.dropout_keep(seed, ctr, n, p).copy()))
        ref = x.double()[torch.arange(n) % n_src] * keep.double() / (1 - float(torch.tensor(p, dtype=F32)))
        return [Out(M, keep, None, "integer output"),
                Out(O, ref, dict(rtol=2e-5, atol=1e-6), "test_kernels_gpu.py::test_dropout_mask_properties")]
    return fn


# dropout_kernel: 4 elements per thread, 256 threads: tails of 1..3 elements, one workgroup +- 1 element, a broadcast source
for _n, _s in ((1, 1), (1023, 1023), (1024, 1024), (1027, 1027), (1030, 103)):
    case("elementwise", f"dropout-{_n}-{_s}", ["t4r_dropout"])(_dropout(_n, _s, 0.3))


def _ln_ref(a, b, gam, bet, eps, keep, p, dy):
    a_, b_, g_, be_ = (t.double().clone().requires_grad_() for t in (a, b, gam, bet))
    x = (a_ * keep.double() / (1 - p) if p > 0 else a_) + b_
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    y = (x - mu) * rstd * g_ + be_
    y.backward(dy.double())
    return dict(y=y.detach(), mean=mu.detach().view(-1), rstd=rstd.detach().view(-1), da=a_.grad, db=b_.grad,
                dg=g_.grad, dbe=be_.grad)


def _layernorm(rows, D, p):
    def fn(a, key):
        import device_rng as R
        ops = _ops()
        lib = _lib().load()
        g = gen(rows * 1000 + D)
        x, r = rn(g, rows, D), rn(g, rows, D)
        gam, bet, dy = 1 + 0.1 * rn(g, D), 0.1 * rn(g, D), rn(g, rows, D)
        eps, seed, ctr = 0.03, 5, ops.dropout_ctr_hi(2, 0, ops.SITE_ATTN_OUT)
        pf = float(torch.tensor(p, dtype=F32))
        ref = memo(key, lambda: _ln_ref(x, r, gam, bet, eps, torch.from_numpy(
            R.dropout_keep(seed, ctr, rows * D, p).copy()).view(rows, D) if p > 0 else None, pf, dy))
        A, B = a.new("a", "in", F32, (rows, D)).set(x), a.new("b", "in", F32, (rows, D)).set(r)
        Gm, Bt = a.new("gamma", "in", F32, D).set(gam), a.new("beta", "in", F32, D).set(bet)
        DY = a.new("dy", "in", F32, (rows, D)).set(dy)
        Y, MU, RS = a.new("y", "out", F32, (rows, D)), a.new("mean", "out", F32, rows), a.new("rstd", "out", F32, rows)
        DX = a.new("dx", "out", F32, (rows, D))
        DXA = a.new("dxa", "out", F32, (rows, D)) if p > 0 else None
        # include/t4r_hip.h: "backward recomputes x = a + b; dgamma/dbeta accumulated"
        DG, DB = a.new("dgamma", "inout", F32, D).set(1.0), a.new("dbeta", "inout", F32, D).set(1.0)
        WS = a.ws("ws", 4 * lib.t4r_colreduce_ws_floats(rows, 2 * D))
        call(a, "t4r_add_layernorm_fwd", stream(), A.ptr, B.ptr, Gm.ptr, Bt.ptr, Y.ptr, MU.ptr, RS.ptr, rows, D, eps, p, seed, ctr)
        call(a, "t4r_add_layernorm_bwd", stream(), A.ptr, B.ptr, Gm.ptr, MU.ptr, RS.ptr, DY.ptr, DX.ptr,
             None if DXA is None else DXA.ptr, DG.ptr, DB.ptr, WS.ptr, rows, D, 0, p, seed, ctr)
        t1 = "test_kernels_gpu.py::test_add_layernorm_fwd_bwd / test_add_layernorm_dropout_fwd_bwd"
        outs = [Out(Y, ref["y"], dict(rtol=2e-5, atol=2e-5), t1), Out(MU), Out(RS),
                Out(DX, ref["db"], dict(rtol=2e-5, atol=5e-5), t1),
                Out(DG, ref["dg"] + 1, dict(rtol=2e-5, atol=1e-4), t1), Out(DB, ref["dbe"] + 1, dict(rtol=2e-5, atol=1e-4), t1)]
        if DXA is not None:
            outs.append(Out(DXA, ref["da"], dict(rtol=2e-5, atol=5e-5), t1))
        return outs
    return fn


for _D in (8, 336, 512):
    for _p in (0.0, 0.3):
        case("elementwise", f"layernorm-33-{_D}-p{_p}", ["t4r_add_layernorm_fwd", "t4r_add_layernorm_bwd"])(_layernorm(33, _D, _p))
case("elementwise", "layernorm-65-64-p0.0", ["t4r_add_layernorm_fwd", "t4r_add_layernorm_bwd"])(_layernorm(65, 64, 0.0))


def _act_bwd_bias(rows, N, mode, p):
    def fn(a, key):
        import device_rng as R
        ops = _ops()
        lib = _lib().load()
        g = gen(rows + N + mode)
        pre, dact = rn(g, rows, N), rn(g, rows, N)
        seed, ctr = 9, ops.dropout_ctr_hi(1, 0, ops.SITE_FF_ACT)
        pf = float(torch.tensor(p, dtype=F32))

        def mk():
            d = dact.double()
            if p > 0:
                d = d * torch.from_numpy(R.dropout_keep(seed, ctr, rows * N, p).copy()).view(rows, N).double() / (1 - pf)
            x = pre.double()
            if mode == 0:
                grad = 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
            else:
                grad = (x > 0).double()
            return d * grad
        ref = memo(key, mk)
        DA, PR = a.new("dact", "in", F32, (rows, N)).set(dact), a.new("pre", "in", F32, (rows, N)).set(pre)
        DP = a.new("dpre", "out", F32, (rows, N))
        DBI = a.new("dbias", "inout", F32, N).set(1.0)       # include/t4r_hip.h: "dbias (accumulated) may be NULL"
        WS = a.ws("ws", 4 * lib.t4r_colreduce_ws_floats(rows, N))
        call(a, "t4r_act_bwd_bias", stream(), DA.ptr, PR.ptr, DP.ptr, DBI.ptr, WS.ptr, rows, N, mode, p, seed, ctr)
        t = "test_kernels_gpu.py::test_act_bwd_bias_and_colsum / test_act_bwd_dropout"
        return [Out(DP, ref, dict(rtol=2e-5, atol=1e-5), t), Out(DBI, ref.sum(0) + 1, dict(rtol=2e-5, atol=1e-4), t)]
    return fn


# act_bwd_bias_kernel: 64 rows per workgroup (T4R_COLRED_ROWS), float4 columns
for _r, _N, _m, _p in ((1, 4, 0, 0.0), (63, 100, 0, 0.0), (64, 96, 1, 0.0), (65, 100, 0, 0.3), (33, 1028, 1, 0.0)):
    case("elementwise", f"act_bwd_bias-{_r}-{_N}-m{_m}-p{_p}", ["t4r_act_bwd_bias", "t4r_colreduce_ws_floats"])(_act_bwd_bias(_r, _N, _m, _p))


def _colsum(rows, N, ld):
    def fn(a, key):
        lib = _lib().load()
        g = gen(rows + N + ld)
        x = rn(g, rows, N)
        X = a.new("x", "in", F32, (rows, ld), 0, N).set(x)
        O = a.new("out", "inout", F32, N).set(1.0)    # include/t4r_hip.h (t4r_colsum): "out[c] += ... (accumulated)"
        WS = a.ws("ws", 4 * lib.t4r_colreduce_ws_floats(rows, N))
        call(a, "t4r_colsum", stream(), X.ptr, O.ptr, WS.ptr, rows, N, ld)
        return [Out(O, x.double().sum(0) + 1, dict(rtol=2e-5, atol=1e-4), "test_kernels_gpu.py::test_act_bwd_bias_and_colsum")]
    return fn


for _r, _N, _ld in ((1, 4, 8), (63, 100, 104), (64, 96, 100), (65, 100, 104), (129, 12, 16)):
    case("elementwise", f"colsum-{_r}-{_N}-ld{_ld}", ["t4r_colsum", "t4r_colreduce_ws_floats"])(_colsum(_r, _N, _ld))


def _add_pos(B, L, D, tt):
    def fn(a, key):
        g = gen(B + L + D)
        x, pos, tok, dy = rn(g, B * L, D), rn(g, L, D), rn(g, D), rn(g, B * L, D)
        X, P = a.new("x", "in", F32, (B * L, D)).set(x), a.new("pos", "in", F32, (L, D)).set(pos)
        T = a.new("token_type", "in", F32, D).set(tok) if tt else None
        DY = a.new("dy", "in", F32, (B * L, D)).set(dy)
        O = a.new("out", "out", F32, (B * L, D))
        DP = a.new("d_pos", "inout", F32, (L, D)).set(1.0)   # include/t4r_hip.h: "backward accumulates d_pos[l] += sum_b dy[b,l]"
        call(a, "t4r_add_pos_fwd", stream(), X.ptr, P.ptr, None if T is None else T.ptr, O.ptr, B, L, D)
        call(a, "t4r_add_pos_bwd", stream(), DY.ptr, DP.ptr, B, L, D)
        ref = x.double().view(B, L, D) + pos.double() + (tok.double() if tt else 0)
        t = "test_kernels_gpu.py::test_gemm_resid_dropout_epilogue_and_pos_emb"
        return [Out(O, ref.view(B * L, D), dict(rtol=2e-5, atol=1e-6), t),
                Out(DP, dy.double().view(B, L, D).sum(0) + 1, dict(rtol=2e-5, atol=1e-4), t, atomic=True)]
    return fn


for _B, _L, _D, _tt in ((1, 1, 4, False), (3, 21, 64, True), (37, 7, 36, False)):
    case("elementwise", f"add_pos-{_B}-{_L}-{_D}", ["t4r_add_pos_fwd", "t4r_add_pos_bwd"])(_add_pos(_B, _L, _D, _tt))


def _adam_ref(p, g, m, v, step, lr, b1, b2, eps, wd, gs):
    p, g, m, v = (t.double() for t in (p, g, m, v))
    g = g * gs + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr * (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps)
    return p, m, v


def _adam(n, amax):
    def fn(a, key):
        g = gen(n)
        p0, gr, m0, v0 = rn(g, n), rn(g, n), 0.1 * rn(g, n), 0.01 * rn(g, n).abs()
        step, lr, b1, b2, eps, wd, gs = 3, 1e-2, 0.9, 0.999, 1e-8, 0.01, 0.5
        P, Gd = a.new("param", "inout", F32, n).set(p0), a.new("grad", "inout", F32, n).set(gr)
        M, V = a.new("exp_avg", "inout", F32, n).set(m0), a.new("exp_avg_sq", "inout", F32, n).set(v0)
        rp, rm, rv = memo(key, lambda: _adam_ref(p0, gr, m0, v0, step, lr, b1, b2, eps, wd, gs))
        t = "test_kernels_gpu.py::test_adam_matches_torch"
        tol = dict(rtol=1e-5, atol=1e-6)
        outs = [Out(P, rp, tol, t), Out(M, rm, tol, t), Out(V, rv, tol, t), Out(Gd, torch.zeros(n), None, "zero_grad clears grad")]
        if not amax:
            call(a, "t4r_adam_step", stream(), P.ptr, Gd.ptr, M.ptr, V.ptr, n, step, lr, b1, b2, eps, wd, gs, 1)
            return outs
        lo, hi = min(3, n - 1), n
        # include/t4r_hip.h: "returns the number of workgroups (<= 1024: the capacity amax_part must have)"
        PART = a.new("amax_part", "out", F32, 1024)
        nb = rc_call(a, "t4r_adam_step_amax", stream(), P.ptr, Gd.ptr, M.ptr, V.ptr, n, step, lr, b1, b2, eps, wd, gs, 1, lo, hi, PART.ptr)
        assert 1 <= nb <= 1024, nb
        torch.cuda.synchronize()
        # exact: the maximum of the updated parameters the kernel itself stored
        amax_ref = P.win[lo:hi].abs().max().cpu().view(1)
        outs.append(Out(PART, amax_ref, None, "max |param| over [lo, hi) of the stored update: exact",
                        sel=lambda v, nb=nb: v[:nb].max().view(1)))
        outs[-1].atomic = False
        return outs
    return fn


# adam_kernel: float4 per thread, 256 threads per workgroup: vector width +- 1, one workgroup +- 1 element
for _n in (1, 3, 4, 5, 1023, 1024, 1025):
    case("elementwise", f"adam-{_n}", ["t4r_adam_step"])(_adam(_n, False))
    case("elementwise", f"adam_amax-{_n}", ["t4r_adam_step_amax"])(_adam(_n, True))


def _apply_mask(B, L, H, mode, to):
    def fn(a, key):
        lib = _lib().load()
        g = gen(B * L + H + mode)
        x, memb, dy = rn(g, B, L, H), rn(g, H), rn(g, B, L, H)
        mask = torch.rand(B, L, generator=g) < 0.4
        m3 = mask[:, :, None]
        last = (torch.arange(L) == L - 1)[None, :, None]
        if mode == 1:      # MLM: out = mask ? memb : x
            ref, rep = torch.where(m3, memb.expand(B, L, H), x), m3.expand(B, L, H)
        elif mode == 2:    # CLM train/eval: mask ? (l == L-1 ? 0 : x) : memb
            ref, rep = torch.where(m3, torch.where(last, torch.zeros(()), x), memb.expand(B, L, H)), (~m3).expand(B, L, H)
        else:              # CLM inference: mask ? x : memb
            ref, rep = torch.where(m3, x, memb.expand(B, L, H)), (~m3).expand(B, L, H)
        keep = ~rep if mode != 2 else (m3 & ~last).expand(B, L, H)
        dx_ref = torch.where(keep, dy, torch.zeros(()))
        dm_ref = torch.where(rep, dy, torch.zeros(())).double().sum((0, 1)) + 1
        X = a.new("x", "inout", F32, (B * L, H)).set(x.view(B * L, H))
        MK = a.new("mask", "in", U8, B * L).set(mask.view(-1))
        ME = a.new("masked_emb", "in", F32, H).set(memb)
        DM = a.new("d_masked_emb", "inout", F32, H).set(1.0)     # include/t4r_hip.h: "d_memb[H] += ... (accumulated)"
        WS = a.ws("ws", 4 * lib.t4r_apply_mask_bwd_ws_floats(B, L, H))
        t = "test_kernels_gpu.py::test_seq_features_concat_and_mask_modes (d masked_emb atol 1e-4; the rest is a copy)"
        DY = a.new("dy", "in" if to else "inout", F32, (B * L, H)).set(dy.view(B * L, H))
        DX = a.new("dx", "out", F32, (B * L, H)) if to else None
        call(a, "t4r_apply_mask_fwd", stream(), X.ptr, MK.ptr, ME.ptr, B, L, H, mode)
        outs = [Out(X, ref.view(B * L, H), None, t), Out(DM, dm_ref, dict(rtol=2e-5, atol=1e-4), t)]
        if to:
            call(a, "t4r_apply_mask_bwd_to", stream(), DY.ptr, DX.ptr, MK.ptr, DM.ptr, B, L, H, mode, WS.ptr)
            outs.append(Out(DX, dx_ref.view(B * L, H), None, t))
        else:
            call(a, "t4r_apply_mask_bwd", stream(), DY.ptr, MK.ptr, DM.ptr, B, L, H, mode, WS.ptr)
            outs.append(Out(DY, dx_ref.view(B * L, H), None, t))
        return outs
    return fn


for _B, _L, _H, _mode in ((1, 1, 4, 1), (3, 21, 64, 1), (5, 13, 100, 2), (70, 20, 36, 3), (2, 33, 7, 1)):
    case("elementwise", f"apply_mask-{_B}-{_L}-{_H}-m{_mode}",
         ["t4r_apply_mask_fwd", "t4r_apply_mask_bwd", "t4r_apply_mask_bwd_ws_floats"])(_apply_mask(_B, _L, _H, _mode, False))
    case("elementwise", f"apply_mask_to-{_B}-{_L}-{_H}-m{_mode}",
         ["t4r_apply_mask_fwd", "t4r_apply_mask_bwd_to", "t4r_apply_mask_bwd_ws_floats"])(_apply_mask(_B, _L, _H, _mode, True))


# ================================================================================================================ input block
def _ragged(rows, L, dtype, gather):
    def fn(a, key):
        g = gen(rows * 10 + L)
        lens = torch.randint(0, L + 3, (rows,), generator=g)
        lens[0] = L + 2                                            # a truncated row
        if rows > 2:
            lens[1] = 0                                            # an empty row
        offs = torch.cat([torch.zeros(1, dtype=I64), lens.cumsum(0)])
        nv = int(offs[-1])
        vals = (torch.randint(1, 1000, (nv,), generator=g)).to(dtype) if dtype == I64 else rn(g, nv)
        ids = torch.randperm(rows, generator=g) if gather else torch.arange(rows)
        ref = torch.zeros(rows, L, dtype=dtype)
        for i, r in enumerate(ids.tolist()):
            n = min(int(lens[r]), L)
            ref[i, :n] = vals[int(offs[r]):int(offs[r]) + n]
        V = a.new("values", "in", dtype, nv).set(vals)
        OF = a.new("offsets", "in", I64, rows + 1).set(offs)
        O = a.new("out", "out", dtype, (rows, L))
        MX = a.new("out_max", "out", I32, 1)
        es = 8 if dtype == I64 else 4
        call(a, "t4r_ragged_max_len", stream(), OF.ptr, rows, MX.ptr)
        if gather:
            R = a.new("row_ids", "in", I64, rows).set(ids)
            call(a, "t4r_ragged_gather_to_padded", stream(), V.ptr, OF.ptr, R.ptr, O.ptr, rows, L, es)
        else:
            call(a, "t4r_ragged_to_padded", stream(), V.ptr, OF.ptr, O.ptr, rows, L, es)
        return [Out(O, ref, None, "copy: exact (test_kernels_gpu.py::test_ragged_to_padded_golden)"),
                Out(MX, lens.max().to(I32).view(1), None, "integer output")]
    return fn


for _rows, _L, _dt in ((1, 1, I64), (5, 3, F32), (65, 20, I64), (257, 7, F32)):
    case("input", f"ragged-{_rows}-{_L}-{'i64' if _dt == I64 else 'f32'}",
         ["t4r_ragged_max_len", "t4r_ragged_to_padded"])(_ragged(_rows, _L, _dt, False))
    case("input", f"ragged_gather-{_rows}-{_L}-{'i64' if _dt == I64 else 'f32'}",
         ["t4r_ragged_max_len", "t4r_ragged_gather_to_padded"])(_ragged(_rows, _L, _dt, True))


def _ragged_gather_scalar(rows):
    def fn(a, key):
        g = gen(rows)
        vals = rn(g, rows + 5)
        ids = torch.randperm(rows + 5, generator=g)[:rows]
        V, R = a.new("values", "in", F32, rows + 5).set(vals), a.new("row_ids", "in", I64, rows).set(ids)
        O = a.new("out", "out", F32, rows)
        # include/t4r_hip.h: "offsets == NULL with L = 1 gathers a scalar column"
        call(a, "t4r_ragged_gather_to_padded", stream(), V.ptr, None, R.ptr, O.ptr, rows, 1, 4)
        return [Out(O, vals[ids], None, "copy: exact")]
    return fn


case("input", "ragged_gather_scalar-257", ["t4r_ragged_gather_to_padded"])(_ragged_gather_scalar(257))


def _session_ids(g, B, L, hi=999):
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    return torch.randint(1, hi, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None]), lens


def _mask_targets(B, L, mode):
    def fn(a, key):
        import t4r_oracle as Orc
        g = gen(B * 1000 + L)
        ids, lens = _session_ids(g, B, L)
        bern = torch.rand(B, L, generator=g) < 0.5
        j1 = (torch.rand(B, generator=g) * lens).long()
        m0 = bern & (ids != 0)
        tmp = torch.where(m0, ids, torch.zeros_like(ids))
        tmp[torch.arange(B), j1] = ids[torch.arange(B), j1]
        j2 = (tmp != 0).float().argmax(1)
        if mode == 0:
            rm, rl = memo(key, lambda: Orc.mlm_targets_train(ids, bern, j1, lambda mm: mm.float().argmax(1)))
        else:
            rm, rl = memo(key, lambda: Orc.clm_targets(ids, True, False))
        ID = a.new("item_ids", "in", I64, (B, L)).set(ids)
        BE = a.new("bern", "in", U8, (B, L)).set(bern)
        J1, J2 = a.new("j1", "in", I64, B).set(j1), a.new("j2", "in", I64, B).set(j2)
        MS, MT, RC = a.new("mask_schema", "out", U8, (B, L)), a.new("masked_targets", "out", I64, (B, L)), a.new("row_count", "out", I32, B)
        call(a, "t4r_mask_targets", stream(), ID.ptr, B, L, mode, 0, BE.ptr, J1.ptr, J2.ptr, 0.15, 0, 0, MS.ptr, MT.ptr, RC.ptr)
        t = "integer output (test_kernels_gpu.py::test_mask_targets_vs_oracle_random)"
        return [Out(MS, rm.to(U8), None, t), Out(MT, rl, None, t), Out(RC, (rl != 0).sum(1).to(I32), None, t)]
    return fn


# mask_targets_kernel: one wave per session, 4 sessions per workgroup, L <= 255 / L > 255 instances, 64 positions per ballot
for _B, _L, _mode in ((1, 1, 0), (5, 63, 0), (9, 64, 4), (7, 65, 0), (5, 300, 0), (6, 20, 4)):
    case("input", f"mask_targets-{_B}-{_L}-m{_mode}", ["t4r_mask_targets"])(_mask_targets(_B, _L, _mode))


def _compact(B, L, D):
    def fn(a, key):
        g = gen(B * 100 + L + D)
        labels = torch.randint(1, 50, (B, L), generator=g) * (torch.rand(B, L, generator=g) < 0.3)
        labels[0, L - 1] = 7
        if B > 1:
            labels[B - 1] = 0                                      # a session without labels
        cnt = (labels != 0).sum(1).to(I32)
        pos = (labels.view(-1) != 0).nonzero().view(-1)
        n = pos.numel()
        x, scale = rn(g, B * L, D), torch.tensor([1.7])
        ids, lens = _session_ids(g, B, L)
        LB, CT = a.new("masked_targets", "in", I64, (B, L)).set(labels), a.new("row_count", "in", I32, B).set(cnt)
        RO, NL = a.new("row_offset", "out", I32, B), a.new("n_labels", "out", I32, 1)
        # include/t4r_hip.h: "label_pos[>= n_labels] ... labels_compact[>= n_labels]": exactly n_labels elements
        LP, LC = a.new("label_pos", "out", I32, n), a.new("labels_compact", "out", I64, n)
        X = a.new("x", "in", F32, (B * L, D)).set(x)
        GO = a.new("gathered", "out", F32, (n, D))
        DX = a.new("dx", "inout", F32, (B * L, D)).set(1.0)        # scatter_rows_add: "dx[pos[n], :] += dout[n, :]"
        SC = a.new("scale", "in", F32, 1).set(scale)
        DD = a.new("dx_dense", "out", F32, (B * L, D))
        LS, SL = a.new("last_pos", "out", I32, B), a.new("session_len", "out", I32, B)
        ID = a.new("item_ids", "in", I64, (B, L)).set(ids)
        call(a, "t4r_compact_labels", stream(), LB.ptr, CT.ptr, B, L, 0, RO.ptr, NL.ptr, LP.ptr, LC.ptr)
        call(a, "t4r_gather_rows", stream(), X.ptr, LP.ptr, GO.ptr, n, D)
        call(a, "t4r_scatter_rows_add", stream(), GO.ptr, LP.ptr, DX.ptr, n, D)
        call(a, "t4r_scatter_rows_dense", stream(), GO.ptr, LP.ptr, n, SC.ptr, DD.ptr, B * L, D)
        call(a, "t4r_last_positions", stream(), ID.ptr, B, L, L + 1, 1, 0, LS.ptr)
        call(a, "t4r_session_lengths", stream(), ID.ptr, B, L, 0, 1, SL.ptr)
        ref_dx = torch.ones(B * L, D)
        ref_dx[pos] += x[pos]
        ref_dd = torch.zeros(B * L, D)
        ref_dd[pos] = x[pos] * scale
        t = "copies / integer outputs: exact (test_kernels_gpu.py::test_compact_gather_scatter)"
        return [Out(RO, (cnt.cumsum(0) - cnt).to(I32), None, t), Out(NL, torch.tensor([n], dtype=I32), None, t),
                Out(LP, pos.to(I32), None, t), Out(LC, labels.view(-1)[pos], None, t), Out(GO, x[pos], None, t),
                Out(DX, ref_dx, None, t), Out(DD, ref_dd, None, t),
                Out(LS, (torch.arange(B) * (L + 1) + lens).to(I32), None, t), Out(SL, (lens + 1).to(I32), None, t)]
    return fn


_COMPACT = ["t4r_compact_labels", "t4r_gather_rows", "t4r_scatter_rows_add", "t4r_scatter_rows_dense", "t4r_last_positions",
            "t4r_session_lengths"]
for _B, _L, _D in ((1, 1, 4), (5, 63, 8), (9, 65, 36), (1030, 3, 4), (3, 130, 64)):
    case("input", f"compact-{_B}-{_L}-{_D}", _COMPACT)(_compact(_B, _L, _D))


def _seq_features(B, L, dims, agg, left, right):
    def fn(a, key):
        g = gen(B * 100 + L + sum(dims) + agg)
        T = B * L
        cards = [50 + 7 * i for i in range(len(dims))]
        ids = [torch.randint(0, c, (T,), generator=g) for c in cards]
        tabs = [rn(g, c, d) for c, d in zip(cards, dims)]
        width = sum(dims) if agg == 0 else dims[0]
        W = left + width + right
        if agg == 0:
            ref = torch.cat([t[i] for t, i in zip(tabs, ids)], 1)
            cols = [left + sum(dims[:f]) for f in range(len(dims))]
        else:
            ref = sum(t.double()[i] for t, i in zip(tabs, ids))
            cols = [0] * len(dims)
        IDs = [a.new(f"ids{f}", "in", I64, T).set(i) for f, i in enumerate(ids)]
        TBs = [a.new(f"table{f}", "in", F32, (c, d)).set(t) for f, (c, d, t) in enumerate(zip(cards, dims, tabs))]
        O = a.new("out", "out", F32, (T, W), left, width)
        O.t[:, :left] = 7.0                                         # live neighbours: the columns of other features
        O.t[:, left + width:] = 9.0
        # include/t4r_hip.h: "a column of [0, W) that no feature covers is left untouched when W <= 1024 and W, every dim[f] and
        # every col[f] are multiples of 4 ... and is written 0 otherwise"
        keeps = agg != 0 or (W <= 1024 and W % 4 == 0 and all(d % 4 == 0 for d in dims) and all(c % 4 == 0 for c in cols))
        if not keeps:
            O.allow(0, left).allow(left + width, W)
        ER = a.new("err_flag", "inout", I32, 1).set(0)              # "set to 1 if an id is outside [0, rows)": the caller clears it
        L_ = _lib()
        kinds, _k = L_.int_array([0] * len(dims))
        inputs, _i = L_.ptr_array([b.ptr for b in IDs])
        tables, _t = L_.ptr_array([b.ptr for b in TBs])
        dms, _d = L_.int_array(list(dims))
        cls, _c = L_.int_array(cols)
        rws, _r = L_.long_array(cards)
        call(a, "t4r_seq_features_fwd", stream(), len(dims), kinds, inputs, tables, dms, cls, rws, agg, -1, B, L, L, W, 0,
             None, None, O.ptr, ER.ptr)
        if not keeps:
            torch.cuda.synchronize()
            assert bool((O.t[:, :left] == 0).all()) and bool((O.t[:, left + width:] == 0).all()), "uncovered columns must be written 0"
        tol = None if agg == 0 else dict(rtol=2e-5, atol=1e-6)
        t = "test_kernels_gpu.py::test_seq_features_concat_and_mask_modes (copy) / test_seq_features_sum_and_item_multi (atol 1e-6)"
        return [Out(O, ref, tol, t), Out(ER, torch.zeros(1, dtype=I32), None, "no id out of range")]
    return fn


for _B, _L in ((1, 1), (3, 21), (13, 20)):
    case("input", f"seq_features_concat-{_B}-{_L}", ["t4r_seq_features_fwd"])(_seq_features(_B, _L, (64, 24, 8), 0, 4, 4))
    # widths / offsets that are no multiple of 4: the generic kernel, which zero-fills the columns no feature covers
    case("input", f"seq_features_concat_odd-{_B}-{_L}", ["t4r_seq_features_fwd"])(_seq_features(_B, _L, (5, 3, 6), 0, 3, 3))
    case("input", f"seq_features_concat_w-{_B}-{_L}", ["t4r_seq_features_fwd"])(_seq_features(_B, _L, (64, 24, 9), 0, 4, 2))
    case("input", f"seq_features_sum-{_B}-{_L}", ["t4r_seq_features_fwd"])(_seq_features(_B, _L, (24, 24, 24), 1, 0, 0))


def _embedding_bwd(ntok, W, col, dim, rows, ids_div, sorted_):
    def fn(a, key):
        lib = _lib().load()
        g = gen(ntok + W + col + dim + rows + ids_div)
        n = ntok // ids_div
        ids = torch.randint(0, rows, (n,), generator=g)
        ids[0] = 0                                                  # padding_idx 0: no gradient
        dout = rn(g, ntok, dim)
        ref = torch.ones(rows, dim, dtype=torch.float64)
        src = dout.double().view(n, ids_div, dim).sum(1)
        live = ids != 0
        ref.index_add_(0, ids[live], src[live])
        DO = a.new("dout", "in", F32, (ntok, W), col, dim).set(dout)
        DO.t[:, :col] = 7.0                                         # live neighbours: other features' gradient columns
        DO.t[:, col + dim:] = 9.0
        ID = a.new("ids", "in", I64, n).set(ids)
        # include/t4r_hip.h: "d_table[id, :] += dout[tok, col:col+dim] ... d_table accumulated"
        DT = a.new("d_table", "inout", F32, (rows, dim)).set(1.0)
        if not sorted_:
            call(a, "t4r_embedding_bwd", stream(), DO.ptr, ID.ptr, DT.ptr, ntok, W, col, dim, rows, 0, ids_div)
            return [Out(DT, ref, dict(rtol=2e-5, atol=1e-4), "test_kernels_gpu.py::test_seq_features_concat_and_mask_modes (d table)",
                        atomic=True)]
        KS, PM = a.new("keys_sorted", "out", I32, n), a.new("perm", "out", I32, n)
        nb = lib.t4r_sort_ids_ws_bytes(n)
        WS = a.ws("sort_ws", nb)
        WS2 = a.ws("bwd_ws", 4 * lib.t4r_embedding_bwd_sorted_ws_floats(n, dim))
        call(a, "t4r_sort_ids", stream(), ID.ptr, n, rows, 0, KS.ptr, PM.ptr, WS.ptr, nb)
        call(a, "t4r_embedding_bwd_sorted", stream(), DO.ptr, KS.ptr, PM.ptr, DT.ptr, n, W, col, dim, rows, ids_div, WS2.ptr)
        keys = torch.where(ids == 0, torch.full_like(ids, rows), ids)
        order = torch.sort(keys, stable=True)
        t = "test_kernels_gpu.py::test_embedding_bwd_sorted_is_exact_and_deterministic"
        return [Out(KS, order.values.to(I32), None, t), Out(PM, order.indices.to(I32), None, t),
                Out(DT, ref, dict(rtol=2e-5, atol=1e-4), t)]
    return fn


for _nt, _W, _c, _d, _r, _div in ((1, 12, 4, 4, 3, 1), (63, 40, 4, 24, 50, 1), (260, 76, 8, 64, 17, 1), (60, 20, 4, 8, 9, 20),
                                  (1025, 16, 4, 8, 300, 1)):
    case("input", f"embedding_bwd-{_nt}-{_W}-{_c}-{_d}-{_r}-div{_div}", ["t4r_embedding_bwd"])(_embedding_bwd(_nt, _W, _c, _d, _r, _div, False))
    case("input", f"embedding_bwd_sorted-{_nt}-{_W}-{_c}-{_d}-{_r}-div{_div}",
         ["t4r_sort_ids", "t4r_embedding_bwd_sorted"])(_embedding_bwd(_nt, _W, _c, _d, _r, _div, True))


def _sort_multi(n, F):
    def fn(a, key):
        lib = _lib().load()
        g = gen(n * 10 + F)
        rows = [20 + 13 * f for f in range(F)]
        pads = [0 if f % 2 == 0 else -1 for f in range(F)]
        ids = [torch.randint(0, r + 3, (n,), generator=g) for r in rows]      # ids >= rows are out of range: they sort last
        IDs = [a.new(f"ids{f}", "in", I64, n).set(i) for f, i in enumerate(ids)]
        KS, PM = a.new("keys_sorted", "out", I32, F * n), a.new("perm", "out", I32, F * n)
        nb = lib.t4r_sort_ids_multi_ws_bytes(n, F)
        WS = a.ws("ws", nb)
        L_ = _lib()
        parr, _k0 = L_.ptr_array([b.ptr for b in IDs])
        rws, _k1 = L_.long_array(rows)
        pds, _k2 = L_.int_array(pads)
        call(a, "t4r_sort_ids_multi", stream(), parr, F, n, rws, pds, KS.ptr, PM.ptr, WS.ptr, nb)
        ks, pm = [], []
        for i, r, p in zip(ids, rows, pads):
            k = torch.where((i == p) | (i >= r), torch.full_like(i, r), i)
            o = torch.sort(k, stable=True)
            ks.append(o.values)
            pm.append(o.indices)
        t = "integer output (test_round5_gpu.py: sort_ids_multi equals sort_ids per feature)"
        return [Out(KS, torch.cat(ks).to(I32), None, t), Out(PM, torch.cat(pm).to(I32), None, t)]
    return fn


for _n, _F in ((1, 1), (255, 3), (1025, 4), (300, 16)):
    case("input", f"sort_ids_multi-{_n}-{_F}", ["t4r_sort_ids_multi"])(_sort_multi(_n, _F))


def _bag(n_bags, dim, ragged, combiner, ld, col, fixed_k=3):
    def fn(a, key):
        g = gen(n_bags * 10 + dim + combiner + int(ragged))
        rows = 37
        table = rn(g, rows, dim)
        if ragged:
            lens = torch.randint(0, 5, (n_bags,), generator=g)
            lens[n_bags // 2] = 0                                  # an empty bag: a zero row
            offs = lens.cumsum(0) - lens
            nv = int(lens.sum())
        else:
            lens = torch.full((n_bags,), fixed_k)
            offs, nv = None, n_bags * fixed_k
        vals = torch.randint(0, rows, (max(nv, 1),), generator=g)[:nv]
        bag_of = torch.repeat_interleave(torch.arange(n_bags), lens)
        dout = rn(g, n_bags, dim)
        scale = {0: torch.ones(n_bags, dtype=torch.float64), 1: 1 / lens.clamp(min=1).double(),
                 2: 1 / lens.clamp(min=1).double().sqrt()}[combiner]
        ref = torch.zeros(n_bags, dim, dtype=torch.float64)
        ref.index_add_(0, bag_of, table.double()[vals])
        ref = ref * scale[:, None]
        ref_rows = dout.double()[bag_of] * scale[bag_of][:, None]
        TB = a.new("table", "in", F32, (rows, dim)).set(table)
        VL = a.new("values", "in", I64, nv).set(vals)
        OF = a.new("offsets", "in", I64, n_bags).set(offs) if ragged else None
        O = a.new("out", "out", F32, (n_bags, ld), col, dim)
        O.t[:, :col] = 7.0
        O.t[:, col + dim:] = 9.0
        ER = a.new("err", "inout", I32, 1).set(0)
        DO = a.new("dout", "in", F32, (n_bags, ld), col, dim).set(dout)
        DO.t[:, :col] = 7.0
        DO.t[:, col + dim:] = 9.0
        RO = a.new("rows_out", "out", F32, (nv, dim))
        fk = 0 if ragged else fixed_k
        ofp = OF.ptr if ragged else None
        call(a, "t4r_embedding_bag_fwd", stream(), TB.ptr, rows, dim, VL.ptr, ofp, n_bags, nv, fk, combiner, O.ptr, ld, col, ER.ptr)
        call(a, "t4r_embedding_bag_bwd_rows", stream(), DO.ptr, ld, col, dim, ofp, n_bags, nv, fk, combiner, RO.ptr)
        t = "test_round4_gpu.py (embedding bag vs torch.nn.EmbeddingBag, atol 1e-5)"
        return [Out(O, ref, dict(rtol=2e-5, atol=1e-5), t), Out(RO, ref_rows, dict(rtol=2e-5, atol=1e-5), t),
                Out(ER, torch.zeros(1, dtype=I32), None, "no id out of range")]
    return fn


for _nb, _dim, _rag, _cmb, _ld, _col in ((1, 4, False, 0, 12, 4), (7, 24, True, 1, 40, 8), (65, 64, True, 2, 72, 4),
                                         (257, 10, False, 1, 20, 6), (33, 8, True, 0, 8, 0)):
    case("input", f"embedding_bag-{_nb}-{_dim}-{'ragged' if _rag else 'matrix'}-c{_cmb}",
         ["t4r_embedding_bag_fwd", "t4r_embedding_bag_bwd_rows"])(_bag(_nb, _dim, _rag, _cmb, _ld, _col))


def _soft_ref(x, pw, pb, tab, lw, lb, eps, dout):
    ps = [t.double().clone().requires_grad_() for t in (pw, pb, tab)] + ([lw.double().clone().requires_grad_(),
                                                                        lb.double().clone().requires_grad_()] if lw is not None else [])
    s = x.double()[:, None] * ps[0][None] + ps[1][None]
    e = torch.softmax(s, 1) @ ps[2]
    if lw is not None:
        mu = e.mean(1, keepdim=True)
        e = (e - mu) / torch.sqrt(((e - mu) ** 2).mean(1, keepdim=True) + eps) * ps[3] + ps[4]
    e.backward(dout.double())
    return e.detach(), [p.grad for p in ps]


def _soft_embedding(ntok, K, D, ln, W, col):
    def fn(a, key):
        lib = _lib().load()
        g = gen(ntok + K * 10 + D)
        x, pw, pb, tab = rn(g, ntok), rn(g, K), rn(g, K), rn(g, K, D)
        lw, lb = (1 + 0.1 * rn(g, D), 0.1 * rn(g, D)) if ln else (None, None)
        dout = rn(g, ntok, D)
        out_ref, grads = memo(key, lambda: _soft_ref(x, pw, pb, tab, lw, lb, 1e-5, dout))
        X, PW, PB = a.new("x", "in", F32, ntok).set(x), a.new("proj_w", "in", F32, K).set(pw), a.new("proj_b", "in", F32, K).set(pb)
        TB = a.new("table", "in", F32, (K, D)).set(tab)
        LW = a.new("ln_w", "in", F32, D).set(lw) if ln else None
        LB = a.new("ln_b", "in", F32, D).set(lb) if ln else None
        O = a.new("out", "out", F32, (ntok, D))
        DO = a.new("dout", "in", F32, (ntok, W), col, D).set(dout)
        DO.t[:, :col] = 7.0
        DO.t[:, col + D:] = 9.0
        # include/t4r_hip.h: "Backward accumulates all parameter gradients"
        DPW, DPB = a.new("d_proj_w", "inout", F32, K).set(1.0), a.new("d_proj_b", "inout", F32, K).set(1.0)
        DTB = a.new("d_table", "inout", F32, (K, D)).set(1.0)
        DLW = a.new("d_ln_w", "inout", F32, D).set(1.0) if ln else None
        DLB = a.new("d_ln_b", "inout", F32, D).set(1.0) if ln else None
        WS = a.ws("ws", 4 * lib.t4r_soft_embedding_bwd_ws_floats(ntok, K, D))
        P = lambda b: None if b is None else b.ptr
        call(a, "t4r_soft_embedding_fwd", stream(), X.ptr, PW.ptr, PB.ptr, TB.ptr, P(LW), P(LB), O.ptr, ntok, K, D, 1e-5)
        call(a, "t4r_soft_embedding_bwd", stream(), DO.ptr, X.ptr, PW.ptr, PB.ptr, TB.ptr, P(LW), DPW.ptr, DPB.ptr, DTB.ptr,
             P(DLW), P(DLB), ntok, W, col, K, D, 1e-5, WS.ptr)
        t = "test_kernels_gpu.py::test_soft_embedding_fwd_bwd"
        tb = dict(rtol=1e-4, atol=2e-4)
        outs = [Out(O, out_ref, dict(rtol=2e-5, atol=1e-5), t), Out(DPW, grads[0] + 1, tb, t), Out(DPB, grads[1] + 1, tb, t),
                Out(DTB, grads[2] + 1, tb, t)]
        if ln:
            outs += [Out(DLW, grads[3] + 1, tb, t), Out(DLB, grads[4] + 1, tb, t)]
        return outs
    return fn


# soft_embedding kernels: one thread per token, 256 per workgroup; the exact (K, D) = (10, 8) instance and the generic ones
for _nt, _K, _D, _ln, _W, _c in ((1, 10, 8, True, 16, 4), (255, 10, 8, False, 8, 0), (257, 5, 12, True, 20, 4), (300, 32, 32, True, 40, 4)):
    case("input", f"soft_embedding-{_nt}-{_K}-{_D}-ln{int(_ln)}", ["t4r_soft_embedding_fwd", "t4r_soft_embedding_bwd"])(
        _soft_embedding(_nt, _K, _D, _ln, _W, _c))


def _copy_cols(rows, ldw, col, dim, B, L):
    def fn(a, key):
        g = gen(rows + ldw + col + dim)
        wide, narrow = rn(g, rows, ldw), rn(g, rows, dim)
        WI = a.new("wide_in", "in", F32, (rows, ldw)).set(wide)
        NO = a.new("narrow_out", "out", F32, (rows, dim))
        NI = a.new("narrow_in", "in", F32, (rows, dim)).set(narrow)
        WO = a.new("wide_out", "out", F32, (rows, ldw), col, dim)
        WO.t[:, :col] = 7.0
        WO.t[:, col + dim:] = 9.0
        SO = a.new("seq_sum", "out", F32, (B, dim))
        call(a, "t4r_copy_cols", stream(), WI.ptr, ldw, col, NO.ptr, dim, rows, 0)
        call(a, "t4r_copy_cols", stream(), WO.ptr, ldw, col, NI.ptr, dim, rows, 1)
        call(a, "t4r_seq_sum_cols", stream(), WI.ptr, ldw, col, SO.ptr, dim, B, L)
        return [Out(NO, wide[:, col:col + dim], None, "copy: exact"), Out(WO, narrow, None, "copy: exact"),
                Out(SO, wide.double()[:, col:col + dim].view(B, L, dim).sum(1), dict(rtol=2e-5, atol=1e-5),
                    "no direct test: L <= 21 fp32 additions of O(1) values, 21 * 2^-24 * |sum| < 1e-5")]
    return fn


for _B, _L, _ldw, _c, _d in ((1, 1, 6, 1, 1), (3, 21, 40, 8, 24), (5, 13, 9, 3, 5), (33, 8, 72, 4, 64)):
    case("input", f"copy_cols-{_B}-{_L}-{_ldw}-{_c}-{_d}", ["t4r_copy_cols", "t4r_seq_sum_cols"])(_copy_cols(_B * _L, _ldw, _c, _d, _B, _L))


def _swap_noise(B, L, eb, per_session):
    def fn(a, key):
        lib = _lib().load()
        g = gen(B * 100 + L + eb)
        ids, lens = _session_ids(g, B, L)
        n = B if per_session else B * L
        x = torch.randint(1, 1000, (n,), generator=g) if eb == 8 else rn(g, n)
        nonpad = (ids[:, 0] != 0) if per_session else (ids.view(-1) != 0)
        bern = torch.rand(n, generator=g) < 0.4
        nn_ = int(nonpad.sum())
        perm = torch.randperm(nn_, generator=g)
        masked = x[nonpad]
        rep = (nonpad & bern).nonzero().view(-1)
        ref = x.clone()
        ref[rep] = masked[perm[:rep.numel()]]
        X = a.new("x", "in", I64 if eb == 8 else F32, n).set(x)
        O = a.new("out", "out", I64 if eb == 8 else F32, n)
        ID = a.new("item_ids", "in", I64, (B, L)).set(ids)
        BE, PM = a.new("bern", "in", U8, n).set(bern), a.new("perm", "in", I64, nn_).set(perm)
        nb = lib.t4r_swap_noise_ws_bytes(n)
        WS = a.ws("ws", nb)
        call(a, "t4r_swap_noise", stream(), X.ptr, O.ptr, eb, n, ID.ptr, 0, L if per_session else 1, 0.4, BE.ptr, PM.ptr, 0, 0, WS.ptr, nb)
        return [Out(O, ref, None, "copy: exact (test_kernels_gpu.py::test_swap_noise_replays_reference_draws)")]
    return fn


def _swap_noise_device(B, L):
    def fn(a, key):
        lib = _lib().load()
        g = gen(B * 100 + L)
        ids, lens = _session_ids(g, B, L)
        n = B * L
        x = ids.view(-1).clone()
        X, O, ID = a.new("x", "in", I64, n).set(x), a.new("out", "out", I64, n), a.new("item_ids", "in", I64, (B, L)).set(ids)
        nb = lib.t4r_swap_noise_ws_bytes(n)
        WS = a.ws("ws", nb)
        call(a, "t4r_swap_noise", stream(), X.ptr, O.ptr, 8, n, ID.ptr, 0, 1, 0.4, None, None, 7, 3, WS.ptr, nb)
        torch.cuda.synchronize()
        got = O.win.cpu()
        # device draws: pads stay, and a replaced element receives one of the non-pad values (the k-th replaced one takes
        # masked[perm[k]]: a draw from the non-pad values, not a rearrangement of the replaced ones)
        assert torch.equal(got[x == 0], x[x == 0]) and bool(torch.isin(got[x != 0], x[x != 0]).all())
        return [Out(O)]
    return fn


for _B, _L, _eb, _ps in ((1, 1, 8, False), (5, 20, 8, False), (13, 20, 4, False), (70, 20, 8, True), (33, 31, 4, False)):
    case("input", f"swap_noise-{_B}-{_L}-e{_eb}-{'session' if _ps else 'seq'}", ["t4r_swap_noise"])(_swap_noise(_B, _L, _eb, _ps))
case("input", "swap_noise_device-13-20", ["t4r_swap_noise"])(_swap_noise_device(13, 20))


# ================================================================================================================ training head
def _ce_ref(logits64, y, eps, gout):
    lg = logits64.clone().requires_grad_()
    rows = torch.nn.functional.cross_entropy(lg, y, label_smoothing=eps, reduction="none")
    (rows.mean() * gout).backward()
    return rows.detach(), torch.logsumexp(logits64, 1), lg.grad


def _softmax_ce(N, V, ld, eps):
    def fn(a, key):
        g = gen(N * 7 + V)
        logits, y, gout = 3 * rn(g, N, V), torch.randint(0, V, (N,), generator=g), 1.7
        rows, lse, dl = memo(key, lambda: _ce_ref(logits.double(), y, eps, gout))
        LG = a.new("logits", "in", F32, (N, ld), 0, V).set(logits)
        Y, GO = a.new("labels", "in", I64, N).set(y), a.new("grad_out", "in", F32, 1).set(gout)
        LR, LS, LM = a.new("loss_rows", "out", F32, N), a.new("lse", "out", F32, N), a.new("loss_mean", "out", F32, 1)
        # include/t4r_hip.h: "bwd: dlogits = ..., pad columns V..ld-1 written 0": the one documented pad write of this entry
        DL = a.new("dlogits", "out", F32, (N, ld), 0, V).allow(V, ld)
        call(a, "t4r_softmax_ce_fwd", stream(), LG.ptr, Y.ptr, LR.ptr, LS.ptr, LM.ptr, N, V, ld, eps)
        call(a, "t4r_softmax_ce_bwd", stream(), LG.ptr, Y.ptr, LS.ptr, GO.ptr, DL.ptr, N, V, ld, eps)
        torch.cuda.synchronize()
        assert float(DL.t[:, V:].abs().sum()) == 0.0 and not bool(torch.isnan(DL.t[:, V:]).any()), "pad columns of dlogits must be 0"
        t = "test_kernels_gpu.py::test_softmax_ce_fwd_bwd"
        return [Out(LR, rows, dict(rtol=2e-5, atol=1e-5), t), Out(LS, lse, dict(rtol=2e-5, atol=1e-5), t),
                Out(LM, rows.mean().view(1), dict(rtol=2e-5, atol=1e-5), t), Out(DL, dl, dict(rtol=1e-4, atol=1e-7), t)]
    return fn


# softmax_ce kernels: one workgroup per row (fwd), 1024 columns per workgroup (bwd), float4 columns
for _N, _V, _ld, _eps in ((1, 33, 36, 0.0), (5, 129, 192, 0.1), (3, 1023, 1024, 0.0), (2, 1025, 1088, 0.1), (4, 1001, 1004, 0.0)):
    case("head", f"softmax_ce-{_N}-{_V}-ld{_ld}-e{_eps}", ["t4r_softmax_ce_fwd", "t4r_softmax_ce_bwd"])(_softmax_ce(_N, _V, _ld, _eps))


def _topk(N, V, ld, k):
    def fn(a, key):
        g = gen(N + V + k)
        s = rn(g, N, V)
        rv, ri = memo(key, lambda: torch.topk(s, k, dim=-1))
        S = a.new("scores", "in", F32, (N, ld), 0, V).set(s)
        OV, OI = a.new("out_val", "out", F32, (N, k)), a.new("out_idx", "out", I64, (N, k))
        call(a, "t4r_topk", stream(), S.ptr, N, V, ld, k, OV.ptr, OI.ptr)
        t = "test_kernels_gpu.py::test_topk (bit-exact)"
        return [Out(OV, rv, None, t), Out(OI, ri, None, t)]
    return fn


for _N in (1, 33):
    for _V, _ld in ((7, 8), (129, 132), (1000, 1024)):
        for _k in sorted({1, min(20, _V), min(_V, 256)}):
            case("serving", f"topk-{_N}-{_V}-k{_k}", ["t4r_topk"])(_topk(_N, _V, _ld, _k))


def _sampled_ref(x, y, W, neg, q, dl):
    x_, W_ = x.double().clone().requires_grad_(), W.double().clone().requires_grad_()
    pos = (x_ * W_[y]).sum(1, keepdim=True) - torch.log(q.double()[y] + 1e-16)[:, None]
    ng = x_ @ W_[neg].t() - torch.log(q.double()[neg] + 1e-16)[None]
    hit = neg[None, :] == y[:, None]
    ng = torch.where(hit, torch.full((), -65504.0 / 100.0, dtype=torch.float64), ng)
    out = torch.cat([pos, ng], 1)
    out.backward(dl.double())
    return out.detach(), x_.grad, W_.grad, hit


def _sampled(N, D, S, V, with_ws, rows_form):
    def fn(a, key):
        g = gen(N * 13 + D + S)
        x, W = rn(g, N, D, scale=0.5), rn(g, V, D, scale=0.5)
        y = torch.randint(1, V, (N,), generator=g)
        pool = torch.randperm(V - 1, generator=g) + 1                # unique negatives (the scatter of d W_neg relies on it) ...
        neg = torch.cat([y[:1], pool[pool != y[0]][:S - 1]])         # ... the first one an accidental hit of row 0
        q = torch.rand(V, generator=g) + 0.01
        q = q / q.sum()
        dl = rn(g, N, S + 1)
        out, dx, dW, hit = memo(key, lambda: _sampled_ref(x, y, W, neg, q, dl))
        X, Wt = a.new("x", "in", F32, (N, D)).set(x), a.new("W", "in", F32, (V, D)).set(W)
        Y, NG, Q = a.new("labels", "in", I64, N).set(y), a.new("neg_samples", "in", I64, S).set(neg), a.new("dist", "in", F32, V).set(q)
        O = a.new("out", "out", F32, (N, S + 1))
        # include/t4r_hip.h: "ws: n_neg * D floats (...); NULL: row-wise"
        WS = a.ws("fwd_ws", 4 * S * D) if with_ws else None
        DL = a.new("dlogits", "inout", F32, (N, S + 1)).set(dl)       # "dlogits is modified in place (accidental-hit entries zeroed)"
        DX = a.new("dx", "out", F32, (N, D))
        WS2 = a.ws("bwd_ws", 4 * 2 * S * D)                          # "ws = 2 * n_neg * D floats of scratch"
        call(a, "t4r_sampled_logits_fwd", stream(), X.ptr, Y.ptr, Wt.ptr, NG.ptr, Q.ptr, O.ptr, N, D, S, 1.0, None if WS is None else WS.ptr)
        t = "test_kernels_gpu.py::test_sampled_logits_golden (atol 1e-4)"
        tol = dict(rtol=2e-5, atol=1e-4)
        dl_ref = dl.clone()
        dl_ref[:, 1:][hit] = 0
        outs = [Out(O, out, tol, t), Out(DL, dl_ref, None, "copy with zeroed hits: exact")]
        if rows_form:
            RO = a.new("rows_out", "out", F32, (N + S, D))
            call(a, "t4r_sampled_logits_bwd_rows", stream(), DL.ptr, X.ptr, Y.ptr, Wt.ptr, NG.ptr, DX.ptr, RO.ptr, WS2.ptr, N, D, S, 1.0)
            g0 = dl.double()[:, :1]
            gn = dl_ref.double()[:, 1:]
            ref_rows = torch.cat([g0 * x.double(), gn.t() @ x.double()], 0)
            outs += [Out(DX, dx, tol, t), Out(RO, ref_rows, tol, t, atomic=True)]
        else:
            # csrc/head.hip: "the weight gradient is accumulated into the dense dW[V, D]"; stated in include/t4r_hip.h
            DW = a.new("dW", "inout", F32, (V, D)).set(1.0)
            call(a, "t4r_sampled_logits_bwd", stream(), DL.ptr, X.ptr, Y.ptr, Wt.ptr, NG.ptr, DX.ptr, DW.ptr, WS2.ptr, N, D, S, 1.0)
            outs += [Out(DX, dx, tol, t), Out(DW, dW + 1, tol, t, atomic=True)]
        return outs
    return fn


for _N, _D, _S, _V, _ws in ((1, 4, 1, 9, False), (5, 64, 3, 40, True), (33, 64, 20, 300, True), (65, 100, 67, 300, True), (9, 32, 4, 50, False)):
    case("head", f"sampled_logits-{_N}-{_D}-{_S}-ws{int(_ws)}", ["t4r_sampled_logits_fwd", "t4r_sampled_logits_bwd"])(
        _sampled(_N, _D, _S, _V, _ws, False))
    case("head", f"sampled_logits_rows-{_N}-{_D}-{_S}-ws{int(_ws)}", ["t4r_sampled_logits_fwd", "t4r_sampled_logits_bwd_rows"])(
        _sampled(_N, _D, _S, _V, _ws, True))


def _log_uniform(n, lo, hi):
    def fn(a, key):
        O = a.new("out", "out", I64, n)
        call(a, "t4r_log_uniform_sample", stream(), O.ptr, n, lo, hi, 17, 3)
        torch.cuda.synchronize()
        got = O.win.cpu()
        assert bool(((got >= lo) & (got < hi)).all()), "log_uniform_sample: an id outside [min_id, max_id)"
        return [Out(O)]        # the distribution is test_kernels_gpu.py::test_log_uniform_device_sampler_...'s subject; here: where it writes
    return fn


for _n in (1, 255, 256, 257, 1000):
    case("head", f"log_uniform-{_n}", ["t4r_log_uniform_sample"])(_log_uniform(_n, 1, 5000))


def _linear_ce(N, V, D, chunk, eps, ldx, ldw):
    def fn(a, key):
        lib = _lib().load()
        g = gen(N * 11 + V + D)
        x, W, y = rn(g, N, D, scale=0.5), rn(g, V, D, scale=0.5), torch.randint(0, V, (N,), generator=g)
        alpha, gout = 1 / 0.7, 1.3

        def mk():
            x_, W_ = x.double().clone().requires_grad_(), W.double().clone().requires_grad_()
            lg = alpha * x_ @ W_.t()
            rows = torch.nn.functional.cross_entropy(lg, y, label_smoothing=eps, reduction="none")
            (rows.mean() * gout).backward()
            return rows.detach(), torch.logsumexp(lg.detach(), 1), x_.grad, W_.grad
        rows, lse, dx, dW = memo(key, mk)
        X, Wt = a.new("X", "in", F32, (N, ldx), 0, D).set(x), a.new("W", "in", F32, (V, ldw), 0, D).set(W)
        Y, GO = a.new("labels", "in", I64, N).set(y), a.new("grad_out", "in", F32, 1).set(gout)
        CH = a.ws("chunk_buf", 4 * lib.t4r_linear_softmax_ce_chunk_floats(N, chunk))
        ST = a.ws("stats", 4 * 4 * N)                                # include/t4r_hip.h: "stats: 4*N floats scratch"
        LR, LS, LM = a.new("loss_rows", "out", F32, N), a.new("lse", "out", F32, N), a.new("loss_mean", "out", F32, 1)
        DX = a.new("dX", "out", F32, (N, ldx), 0, D)                 # "dX[N,D] = alpha * dlogits @ W (overwritten)"
        DW = a.new("dW", "inout", F32, (V, ldw), 0, D).set(1.0)      # "dW[V,D] += alpha * dlogits^T @ X"
        call(a, "t4r_linear_softmax_ce_fwd", stream(), X.ptr, ldx, Wt.ptr, ldw, Y.ptr, N, V, D, alpha, eps, chunk, CH.ptr, ST.ptr,
             LR.ptr, LS.ptr, LM.ptr)
        call(a, "t4r_linear_softmax_ce_bwd", stream(), X.ptr, ldx, Wt.ptr, ldw, Y.ptr, LS.ptr, GO.ptr, N, V, D, alpha, eps, chunk,
             CH.ptr, DX.ptr, ldx, DW.ptr, ldw)
        t = "test_kernels_gpu.py::test_linear_softmax_ce_fused_fwd_bwd"
        return [Out(LR, rows, dict(rtol=1e-6, atol=2e-6), t), Out(LS, lse, dict(rtol=1e-6, atol=2e-6), t),
                Out(LM, rows.mean().view(1), dict(rtol=1e-6, atol=2e-6), t),
                Out(DX, dx, dict(rtol=1e-4, atol=1e-6), t, atomic=True), Out(DW, dW + 1, dict(rtol=1e-4, atol=2e-6), t)]
    return fn


# chunks that do not divide V, V below one chunk, row pitches wider than D
for _N, _V, _D, _ch, _eps, _ldx, _ldw in ((1, 33, 32, 64, 0.0, 32, 32), (37, 129, 32, 64, 0.1, 36, 36), (33, 257, 64, 100, 0.0, 68, 64),
                                          (65, 1001, 128, 256, 0.1, 128, 132)):
    case("head", f"linear_softmax_ce-{_N}-{_V}-{_D}-c{_ch}", ["t4r_linear_softmax_ce_fwd", "t4r_linear_softmax_ce_bwd"])(
        _linear_ce(_N, _V, _D, _ch, _eps, _ldx, _ldw))


# ================================================================================================================ GEMM
def _round_to(x, mode):
    if mode == "bf16":
        return x.to(torch.bfloat16).float()
    if mode == "fp16":
        return x.to(torch.float16).float()
    return x


def _pitch(w, pad):
    """logical width + the smallest pad that keeps rows 16-byte loadable (+4 floats past the next multiple of 4); pad 1: an
    odd pitch (scalar loads, fp32 form)"""
    return w + 1 if pad == 1 else (w + 3) // 4 * 4 + 4


def _gemm_layouts(mode, M, N, K, pad):
    def fn(a, key):
        ops = _ops()
        g = gen(M * 7 + N * 3 + K)
        outs = []
        with ops.precision(mode):
            for ta in (0, 1):
                for tb in (0, 1):
                    A, B = rn(g, *((K, M) if ta else (M, K))), rn(g, *((N, K) if tb else (K, N)))
                    half = mode in ("bf16", "fp16") and pad != 1        # 16-byte loadable operands: the half-precision form runs
                    Ar, Br = (_round_to(A, mode), _round_to(B, mode)) if half else (A, B)
                    ref = memo((key, ta, tb), lambda: 0.5 * ((Ar.t() if ta else Ar).double() @ (Br.t() if tb else Br).double()))
                    Ab = a.new(f"A{ta}{tb}", "in", F32, (A.shape[0], _pitch(A.shape[1], pad)), 0, A.shape[1]).set(A)
                    Bb = a.new(f"B{ta}{tb}", "in", F32, (B.shape[0], _pitch(B.shape[1], pad)), 0, B.shape[1]).set(B)
                    Cb = a.new(f"C{ta}{tb}", "out", F32, (M, _pitch(N, pad)), 0, N)
                    outs.append((Ab, Bb, Cb, ta, tb, ref))
            a.seal()
            for Ab, Bb, Cb, ta, tb, ref in outs:
                ops.gemm(Ab.win, Bb.win, bool(ta), bool(tb), alpha=0.5, out=Cb.win)
        t = "test_kernels_gpu.py::test_gemm_layouts / test_gemm_precision_modes_layouts"
        return [Out(Cb, ref, dict(rtol=1e-5, atol=1e-4), t) for _, _, Cb, _, _, ref in outs]
    return fn


_GEMM_SHAPES = ((1, 1, 1), (63, 65, 17), (64, 64, 16), (65, 127, 33), (129, 3, 40))
for _mode in ("fp32", "fp32_bf16x3", "bf16", "fp16", "auto"):
    for _M, _N, _K in _GEMM_SHAPES:
        case("gemm", f"gemm-{_mode}-{_M}-{_N}-{_K}", ["t4r_gemm_f32"])(_gemm_layouts(_mode, _M, _N, _K, 4))
for _mode in ("fp32", "auto"):
    case("gemm", f"gemm-{_mode}-63-65-17-oddpitch", ["t4r_gemm_f32"])(_gemm_layouts(_mode, 63, 65, 17, 1))


def _gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def _gemm_epilogues(mode, M, N, K, p):
    def fn(a, key):
        import device_rng as R
        ops = _ops()
        g = gen(M + N + K)
        A, W, bias, res = rn(g, M, K), rn(g, N, K), rn(g, N), rn(g, M, N)
        seed, ctr = 2, ops.dropout_ctr_hi(1, 0, ops.SITE_FF_OUT)
        pf = float(torch.tensor(p, dtype=F32))
        Ar, Wr = _round_to(A, mode), _round_to(W, mode)
        pre = memo((key, "pre"), lambda: Ar.double() @ Wr.double().t() + bias.double())
        keep = memo((key, "keep"), lambda: torch.from_numpy(R.dropout_keep(seed, ctr, M * N, p).copy()).view(M, N).double() / (1 - pf)) \
            if p > 0 else 1.0
        lda, ldw, ldc = _pitch(K, 4), _pitch(K, 4), _pitch(N, 4)
        Ab, Wb = a.new("A", "in", F32, (M, lda), 0, K).set(A), a.new("W", "in", F32, (N, ldw), 0, K).set(W)
        Bi = a.new("bias", "in", F32, N).set(bias)
        Rs = a.new("residual", "in", F32, (M, ldc), 0, N).set(res)
        C1, C2, C3, C4 = (a.new(f"C_{n}", "out", F32, (M, ldc), 0, N) for n in ("bias", "gelu", "relu", "resid"))
        AUX = a.new("aux_preact", "out", F32, (M, ldc), 0, N)
        ACC = a.new("C_acc", "inout", F32, (M, ldc), 0, N).set(1.0)     # include/t4r_hip.h: "accumulate: C += result"
        a.seal()
        with ops.precision(mode):
            ops.gemm(Ab.win, Wb.win, False, True, bias=Bi.t, epilogue=ops.EPI_BIAS, out=C1.win)
            ops.gemm(Ab.win, Wb.win, False, True, bias=Bi.t, epilogue=ops.EPI_BIAS_GELU, out=C2.win, aux=AUX.win, drop=(p, seed, ctr))
            ops.gemm(Ab.win, Wb.win, False, True, bias=Bi.t, epilogue=ops.EPI_BIAS_RELU, out=C3.win)
            ops.gemm(Ab.win, Wb.win, False, True, bias=Bi.t, epilogue=ops.EPI_BIAS_RESID, out=C4.win, aux=Rs.win, drop=(p, seed, ctr))
            ops.gemm(Ab.win, Wb.win, False, True, out=ACC.win, accumulate=True)
        t = ("test_kernels_gpu.py::test_gemm_epilogues_splitk_accumulate (fp32: atol 1e-4) / test_gemm_precision_modes_features "
             "(rtol 1e-4, atol 2e-4)")
        tol = dict(rtol=2e-5, atol=1e-4) if mode in ("fp32", "auto") else dict(rtol=1e-4, atol=2e-4)
        return [Out(C1, pre, tol, t), Out(AUX, pre, tol, t), Out(C2, _gelu64(pre) * keep, tol, t), Out(C3, torch.relu(pre), tol, t),
                Out(C4, pre * keep + res.double(), tol, t), Out(ACC, pre - bias.double() + 1, tol, t)]
    return fn


for _mode in ("fp32", "fp32_bf16x3", "bf16", "fp16", "auto"):
    for _M, _N, _K, _p in ((65, 127, 33, 0.0), (64, 64, 16, 0.3), (63, 65, 17, 0.3)):
        case("gemm", f"gemm_epilogues-{_mode}-{_M}-{_N}-{_K}-p{_p}", ["t4r_gemm_f32"])(_gemm_epilogues(_mode, _M, _N, _K, _p))


def _gemm_splitk(mode, M, N, K, splitk):
    def fn(a, key):
        ops = _ops()
        g = gen(M + N + K + splitk)
        A, B = rn(g, K, M), rn(g, K, N)
        Ar, Br = _round_to(A, mode), _round_to(B, mode)
        ref = memo(key, lambda: Ar.double().t() @ Br.double())
        Ab, Bb = a.new("A", "in", F32, (K, _pitch(M, 4)), 0, M).set(A), a.new("B", "in", F32, (K, _pitch(N, 4)), 0, N).set(B)
        t = "test_kernels_gpu.py::test_gemm_epilogues_splitk_accumulate (rtol 1e-4, atol 2e-3)"
        tol = dict(rtol=1e-4, atol=2e-3)
        C = a.new("C", "out", F32, (M, _pitch(N, 4)), 0, N)
        ACC = a.new("C_acc", "inout", F32, (M, _pitch(N, 4)), 0, N).set(1.0)
        a.seal()
        with ops.precision(mode):
            ops.gemm(Ab.win, Bb.win, True, False, splitk=splitk, out=C.win)       # "C zeroed first unless accumulate"
            ops.gemm(Ab.win, Bb.win, True, False, splitk=splitk, accumulate=True, out=ACC.win)
        return [Out(C, ref, tol, t, atomic=splitk != 1), Out(ACC, ref + 1, tol, t, atomic=splitk != 1)]
    return fn


def _gemm_wgrad(mode, M, N, K, ws):
    """t4r_gemm_wgrad_f32: the deterministic split-K weight gradient in one call, dense C (ldc == N).  ws "query": the workspace
    is what t4r_gemm_wgrad_ws_floats returns; "one_split": M * N floats, room for one split only (at K = 700 the rule gives two:
    the product must say so in *bypassed and use atomics); "null": none at all (K = 304 is 19 k-tiles: one split, nothing parked)"""
    def fn(a, key):
        ops = _ops()
        g = gen(M + N + K - 1)      # (the operands of the gemm_splitk_sink cases as they always were: seed M + N + K + splitk)
        A, B = rn(g, K, M), rn(g, K, N)
        Ar, Br = _round_to(A, mode), _round_to(B, mode)
        ref = memo(key, lambda: Ar.double().t() @ Br.double())
        Ab, Bb = a.new("A", "in", F32, (K, _pitch(M, 4)), 0, M).set(A), a.new("B", "in", F32, (K, _pitch(N, 4)), 0, N).set(B)
        t = "test_kernels_gpu.py::test_gemm_epilogues_splitk_accumulate (rtol 1e-4, atol 2e-3)"
        tol = dict(rtol=1e-4, atol=2e-3)
        C = a.new("C", "inout", F32, (M, N)).set(1.0)
        floats = {"query": _lib().load().t4r_gemm_wgrad_ws_floats(M, N, K), "one_split": M * N, "null": 0}[ws]
        WS = a.ws("sink_ws", 4 * floats) if floats else None
        bypassed = ctypes.c_int(-1)
        with ops.precision(mode):
            call(a, "t4r_gemm_wgrad_f32", stream(), M, N, K, Ab.ptr, Ab.win.stride(0), Bb.ptr, Bb.win.stride(0), C.ptr,
                 WS.ptr if WS else None, floats, ctypes.addressof(bypassed))
        assert bypassed.value == (1 if ws == "one_split" else 0)
        return [Out(C, ref + 1, tol, t, atomic=ws == "one_split")]
    return fn


for _mode in ("fp32", "auto", "bf16"):
    for _sk in (1, 3, -1):
        case("gemm", f"gemm_splitk-{_mode}-65-47-700-s{_sk}", ["t4r_gemm_f32"])(_gemm_splitk(_mode, 65, 47, 700, _sk))
    # (t4r_gemm_f32 is named so that, as before, this case is what runs between the two runs of the atomic split-K case above:
    # after the deterministic product nothing is left armed that a later t4r_gemm_f32(splitk = -1) could find)
    case("gemm", f"gemm_splitk_sink-{_mode}-64-48-700", ["t4r_gemm_f32", "t4r_gemm_wgrad_f32"])(_gemm_wgrad(_mode, 64, 48, 700, "query"))
case("gemm", "gemm_wgrad_bypass-fp32-64-48-700", ["t4r_gemm_wgrad_f32"])(_gemm_wgrad("fp32", 64, 48, 700, "one_split"))
case("gemm", "gemm_wgrad_nosplit-fp32-64-48-304", ["t4r_gemm_wgrad_f32"])(_gemm_wgrad("fp32", 64, 48, 304, "query"))
case("gemm", "gemm_wgrad_nosplit_nullws-fp32-64-48-304", ["t4r_gemm_wgrad_f32"])(_gemm_wgrad("fp32", 64, 48, 304, "null"))


def _gemm_softmax_grad(N, V, D, eps, mode):
    def fn(a, key):
        ops = _ops()
        g = gen(N + V + D)
        x, W, y = rn(g, N, D), rn(g, V, D, scale=0.3), torch.randint(0, V, (N,), generator=g)
        logits = (x @ W.t())
        gout, alpha = 1.7, 0.9

        def mk():
            lg = logits.double()
            dl = (torch.softmax(lg, 1) * 1.0 - (1 - eps) * torch.nn.functional.one_hot(y, V).double() - eps / V) * gout / N
            return torch.logsumexp(lg, 1), alpha * dl @ W.double(), alpha * dl.t() @ x.double()
        lse, dx, dW = memo(key, mk)
        ld = ops.pad_ld(V)
        LG = a.new("logits", "in", F32, (N, ld), 0, V).set(logits)
        LS, Y, GO = a.new("lse", "in", F32, N).set(lse), a.new("labels", "in", I64, N).set(y), a.new("grad_out", "in", F32, 1).set(gout)
        Wb, Xb = a.new("W", "in", F32, (V, _pitch(D, 4)), 0, D).set(W), a.new("X", "in", F32, (N, _pitch(D, 4)), 0, D).set(x)
        DX = a.new("dX", "out", F32, (N, _pitch(D, 4)), 0, D)
        DW = a.new("dW", "inout", F32, (V, _pitch(D, 4)), 0, D).set(1.0)
        a.seal()
        with ops.precision(mode):
            ops.gemm_softmax_grad(LG.win, LS.t, Y.t, GO.t, V, Wb.win, False, alpha=alpha, label_smoothing=eps, out=DX.win)
            ops.gemm_softmax_grad(LG.win, LS.t, Y.t, GO.t, V, Xb.win, True, alpha=alpha, label_smoothing=eps, out=DW.win, accumulate=True)
        t = "test_kernels_gpu.py::test_gemm_softmax_grad_fused (fp32-accurate) / test_gemm_precision_modes_features (half modes)"
        if mode in ("bf16", "fp16"):
            tx = tw = dict(rtol=2e-2, atol=2e-5)
        else:
            tx, tw = dict(rtol=1e-4, atol=1e-6), dict(rtol=1e-4, atol=2e-6)
        return [Out(DX, dx, tx, t), Out(DW, dW + 1, tw, t)]
    return fn


for _mode in ("fp32", "auto", "fp16"):
    for _N, _V, _D, _eps in ((37, 129, 32, 0.1), (1, 33, 32, 0.0)):
        case("gemm", f"gemm_softmax_grad-{_mode}-{_N}-{_V}-{_D}", ["t4r_gemm_softmax_grad_f32"])(_gemm_softmax_grad(_N, _V, _D, _eps, _mode))


def _tok_gemm(M, N, K, tb):
    def fn(a, key):
        ops = _ops()
        g = gen(M + N + K + int(tb))
        A, B, c0 = rn(g, M, K), rn(g, *((N, K) if tb else (K, N)), scale=0.2), rn(g, M, N)
        ref = memo(key, lambda: A.double() @ (B.double().t() if tb else B.double()))
        scale = float(ref.abs().max())
        Ab = a.new("A", "in", F32, (M, K + 4), 0, K).set(A)
        Bb = a.new("B", "in", F32, (B.shape[0], B.shape[1] + 4), 0, B.shape[1]).set(B)
        C = a.new("C", "out", F32, (M, N + 4), 0, N)
        ACC = a.new("C_acc", "inout", F32, (M, N + 32), 0, N).set(c0)
        a.seal()
        with ops.tok_gemm_min_rows(1):          # csrc/tok_gemm.hip: 128 token rows per workgroup
            ops.gemm(Ab.win, Bb.win, False, tb, alpha=0.7, out=C.win)
            ops.gemm(Ab.win, Bb.win, False, tb, out=ACC.win, accumulate=True)
        t = "test_kernels_gpu.py::test_tok_gemm_matches_fp64 (rtol 1e-5, atol 2e-5 * max |ref|)"
        tol = dict(rtol=1e-5, atol=2e-5 * scale)
        return [Out(C, 0.7 * ref, tol, t), Out(ACC, c0.double() + ref, tol, t)]
    return fn


for _M in (1, 127, 128, 129):
    for _N, _K, _tb in ((64, 32, True), (32, 128, False)):
        case("gemm", f"tok_gemm-{_M}-{_N}-{_K}-tb{int(_tb)}", ["t4r_gemm_f32"])(_tok_gemm(_M, _N, _K, _tb))


# ================================================================================================================ split head
def _amax_tol(c, ref):
    return dict(rtol=0, atol=c * float(ref.abs().max()))


def _head_bwd_ref(lg, lse, y, V, yoff, smooth, gout, N, alpha, W64, x64):
    """fp64 backward products formed from the GIVEN fp32 logits (the kernels' input), as test_head_split_products_match_fp64"""
    Vc = lg.shape[1]
    p = torch.exp(lg.double() - lse.double()[:, None])
    onehot = torch.zeros(N, V, dtype=torch.float64)
    onehot[torch.arange(N), y] = 1.0
    G = (gout / N) * (p - (1 - smooth) * onehot[:, yoff:yoff + Vc] - smooth / V)
    return alpha * (G @ W64[yoff:yoff + Vc]), alpha * (G.t() @ x64)


def _head_split(N, V, D, smooth, form):
    """form: "mat" prepare -> logits -> logits_ce -> dw, dx | "fdx" prepare -> logits_ce_dx -> dw | "fdx_amax" the same through
    logits_ce_dx_amax (the table maximum from the caller's partials) | "rc" prepare -> prepare_rc -> ce -> dw_rc, dx_rc |
    "chunk" prepare -> logits -> dx, dw on the columns [yoff, yoff + Vc)"""
    def fn(a, key):
        ops = _ops()
        lib = _lib().load()
        g = gen(N + V + D)
        x, W, y = rn(g, N, D), rn(g, V, D, scale=0.3), torch.randint(0, V, (N,), generator=g)
        alpha, gout = 0.5, 1.7
        x64, W64 = x.double(), W.double()
        lg64 = memo((key, "lg"), lambda: alpha * x64 @ W64.t())
        ldx, ldw, ldc = D + 4, D + 4, ops.pad_ld(V)
        X, Wb = a.new("X", "in", F32, (N, ldx), 0, D).set(x), a.new("W", "in", F32, (V, ldw), 0, D).set(W)
        Y, GO = a.new("labels", "in", I64, N).set(y), a.new("grad_out", "in", F32, 1).set(gout)
        nb = lib.t4r_head_split_ws_bytes(N, V, D)
        assert nb > 0
        WS = a.ws("ws", nb)
        note = (ctypes.c_ulonglong * 8)()                 # "Zero it before the forward product": host, caller-owned
        nptr = ctypes.addressof(note)
        LR, LS, LM = a.new("loss_rows", "out", F32, N), a.new("lse", "out", F32, N), a.new("loss_mean", "out", F32, 1)
        DX = a.new("dX", "out", F32, (N, ldx), 0, D)
        t = "test_kernels_gpu.py::test_head_split_products_match_fp64"
        call(a, "t4r_head_split_prepare", stream(), X.ptr, ldx, N, D, V, WS.ptr)
        if form == "mat":
            C1 = a.new("logits", "out", F32, (N, ldc), 0, V)
            call(a, "t4r_head_split_logits", stream(), WS.ptr, Wb.ptr, ldw, C1.ptr, ldc, N, V, D, alpha, nptr)
            outs = [Out(C1, lg64, _amax_tol(2e-6, lg64), t)]
            C2 = a.new("logits_ce", "out", F32, (N, ldc), 0, V)
            DW = a.new("dW", "inout", F32, (V, ldw), 0, D).set(1.0)
            DWN = a.new("dW_overwritten", "out", F32, (V, ldw), 0, D)
            ctypes.memset(nptr, 0, 64)
            call(a, "t4r_head_split_logits_ce", stream(), WS.ptr, Wb.ptr, ldw, C2.ptr, ldc, Y.ptr, LR.ptr, LS.ptr, LM.ptr, N, V, D, alpha,
                 smooth, nptr)
            call(a, "t4r_head_split_dw", stream(), WS.ptr, C2.ptr, ldc, LS.ptr, Y.ptr, GO.ptr, smooth, DW.ptr, ldw, N, V, V, 0, D, alpha, 1, nptr)
            call(a, "t4r_head_split_dw", stream(), WS.ptr, C2.ptr, ldc, LS.ptr, Y.ptr, GO.ptr, smooth, DWN.ptr, ldw, N, V, V, 0, D, alpha, 0, nptr)
            call(a, "t4r_head_split_dx", stream(), WS.ptr, C2.ptr, ldc, LS.ptr, Y.ptr, GO.ptr, smooth, Wb.ptr, ldw, DX.ptr, ldx, N, V, V, 0, D,
                 alpha, 0, nptr)
            torch.cuda.synchronize()
            lg2, lse2 = C2.win.cpu(), LS.win.cpu()
            rows = torch.nn.functional.cross_entropy(lg2.double(), y, reduction="none", label_smoothing=smooth)
            dX64, dW64 = _head_bwd_ref(lg2, lse2, y, V, 0, smooth, gout, N, alpha, W64, x64)
            t1e5 = dict(rtol=0, atol=1e-5)
            outs += [Out(C2, lg64, _amax_tol(4e-6, lg64), t), Out(LR, rows, t1e5, t), Out(LS, torch.logsumexp(lg2.double(), 1), t1e5, t),
                     Out(LM, rows.mean().view(1), t1e5, t), Out(DX, dX64, _amax_tol(5e-6, dX64), t),
                     Out(DWN, dW64, _amax_tol(5e-6, dW64), t), Out(DW, dW64 + 1, _amax_tol(1e-5, dW64), t)]
            return outs
        if form == "chunk":
            # one vocabulary-chunk call: logits hold the columns [yoff, yoff + Vc) of the [N, V] problem, W points at row yoff
            yoff, Vc = 32, V - 40
            ldk = ops.pad_ld(Vc)
            lse64 = torch.logsumexp(lg64, 1)
            chunk = lg64[:, yoff:yoff + Vc].float()
            CH = a.new("logits_chunk", "in", F32, (N, ldk), 0, Vc).set(chunk)
            LSI = a.new("lse_in", "in", F32, N).set(lse64)
            DWC = a.new("dW_chunk", "out", F32, (Vc, ldw), 0, D)
            call(a, "t4r_head_split_dx", stream(), WS.ptr, CH.ptr, ldk, LSI.ptr, Y.ptr, GO.ptr, smooth, Wb.ptr + 4 * yoff * ldw, ldw, DX.ptr,
                 ldx, N, Vc, V, yoff, D, alpha, 0, None)
            call(a, "t4r_head_split_dw", stream(), WS.ptr, CH.ptr, ldk, LSI.ptr, Y.ptr, GO.ptr, smooth, DWC.ptr, ldw, N, Vc, V, yoff, D, alpha,
                 0, None)
            dX64, dW64 = _head_bwd_ref(chunk, lse64.float(), y, V, yoff, smooth, gout, N, alpha, W64, x64)
            tc = "test_kernels_gpu.py::test_head_split_vocabulary_chunk"
            return [Out(DX, dX64, dict(rtol=1e-4, atol=1e-7), tc), Out(DWC, dW64, dict(rtol=1e-4, atol=1e-7), tc)]
        if form in ("fdx", "fdx_amax"):
            C3 = a.new("logits", "out", F32, (N, ldc), 0, V)
            WSUM = a.new("wsum", "in", F32, D).set(W.double().sum(0)) if smooth > 0 else None
            DW = a.new("dW", "inout", F32, (V, ldw), 0, D).set(1.0)
            fdx_args = (stream(), WS.ptr, X.ptr, ldx, Wb.ptr, ldw, C3.ptr, ldc, Y.ptr, LR.ptr, LS.ptr, LM.ptr,
                        DX.ptr, ldx, None if WSUM is None else WSUM.ptr, N, V, D, alpha, smooth, nptr)
            if form == "fdx_amax":
                # host-computed per-slot maxima over exactly W's elements (what t4r_adam_step_amax leaves), five slots: max |W| is
                # exact whichever way it is reduced, so the expected outputs are the fdx case's
                part = torch.stack([c.abs().max() for c in W.chunk(5)])
                PART = a.new("w_amax_part", "in", F32, part.numel()).set(part)
                call(a, "t4r_head_split_logits_ce_dx_amax", *fdx_args, PART.ptr, part.numel())
            else:
                call(a, "t4r_head_split_logits_ce_dx", *fdx_args)
            call(a, "t4r_head_split_dw", stream(), WS.ptr, C3.ptr, ldc, LS.ptr, Y.ptr, GO.ptr, smooth, DW.ptr, ldw, N, V, V, 0, D, alpha, 1, nptr)

            def mk():
                x_, W_ = x64.clone().requires_grad_(), W64.clone().requires_grad_()
                z = alpha * x_ @ W_.t()
                rows = torch.nn.functional.cross_entropy(z, y, label_smoothing=smooth, reduction="none")
                rows.mean().backward()
                return rows.detach(), torch.logsumexp(z.detach(), 1), x_.grad, W_.grad
            rows, lse, gx, gW = memo((key, "fdx"), mk)
            t5 = "test_round5_gpu.py (one-pass head against fp64: 3e-6 relative to the largest entry; d W rows 2e-5 of the row's own)"
            scale = max(1.0, float(rows.abs().max()))
            return [Out(C3, lg64, _amax_tol(3e-6, lg64), t5), Out(LS), Out(LR),
                    Out(LM, rows.mean().view(1), dict(rtol=0, atol=3e-6 * max(1.0, abs(float(rows.mean())))), t5),
                    Out(DX, gx, _amax_tol(3e-6, gx), t5), Out(DW, gout * gW + 1, _amax_tol(2e-5, gW * gout), t5)]
        # form == "rc"
        DW = a.new("dW", "inout", F32, (V, ldw), 0, D).set(1.0)
        DWN = a.new("dW_overwritten", "out", F32, (V, ldw), 0, D)
        call(a, "t4r_head_split_prepare_rc", stream(), X.ptr, ldx, N, D, V, WS.ptr)
        call(a, "t4r_head_split_ce", stream(), WS.ptr, Wb.ptr, ldw, Y.ptr, LR.ptr, LS.ptr, LM.ptr, N, V, D, alpha, smooth, nptr)
        call(a, "t4r_head_split_dw_rc", stream(), WS.ptr, Wb.ptr, ldw, LS.ptr, Y.ptr, GO.ptr, smooth, DW.ptr, ldw, N, V, D, alpha, 1, nptr)
        call(a, "t4r_head_split_dw_rc", stream(), WS.ptr, Wb.ptr, ldw, LS.ptr, Y.ptr, GO.ptr, smooth, DWN.ptr, ldw, N, V, D, alpha, 0, nptr)
        call(a, "t4r_head_split_dx_rc", stream(), WS.ptr, X.ptr, ldx, Wb.ptr, ldw, LS.ptr, Y.ptr, GO.ptr, smooth, DX.ptr, ldx, N, V, D, alpha,
             0, nptr)
        rows = torch.nn.functional.cross_entropy(lg64, y, reduction="none", label_smoothing=smooth)
        lse64 = torch.logsumexp(lg64, 1)
        dX64, dW64 = _head_bwd_ref(lg64, lse64, y, V, 0, smooth, gout, N, alpha, W64, x64)
        t4 = "test_round4_gpu.py (recomputing head against fp64: rows 2e-5, d X / d W 5e-6 and 1e-5 of the largest entry)"
        return [Out(LR, rows, dict(rtol=0, atol=2e-5), t4), Out(LS, lse64, dict(rtol=0, atol=2e-5), t4),
                Out(LM, rows.mean().view(1), dict(rtol=0, atol=2e-5), t4), Out(DX, dX64, _amax_tol(5e-6, dX64), t4),
                Out(DWN, dW64, _amax_tol(5e-6, dW64), t4), Out(DW, dW64 + 1, _amax_tol(1e-5, dW64), t4)]
    return fn


def _head_supported(form, D):
    lib = _lib().load()
    if not lib.t4r_head_split_supported(D):
        return False
    if form in ("fdx", "fdx_amax"):
        return bool(lib.t4r_head_split_fdx_supported(D))
    if form == "rc":
        return bool(lib.t4r_head_split_recompute_supported(D))
    return True


_HEAD_FORMS = {"mat": ["t4r_head_split_prepare", "t4r_head_split_logits", "t4r_head_split_logits_ce", "t4r_head_split_dw", "t4r_head_split_dx"],
               "fdx": ["t4r_head_split_prepare", "t4r_head_split_logits_ce_dx", "t4r_head_split_dw"],
               "fdx_amax": ["t4r_head_split_prepare", "t4r_head_split_logits_ce_dx_amax", "t4r_head_split_dw"],
               "rc": ["t4r_head_split_prepare", "t4r_head_split_prepare_rc", "t4r_head_split_ce", "t4r_head_split_dw_rc", "t4r_head_split_dx_rc"],
               "chunk": ["t4r_head_split_prepare", "t4r_head_split_dw", "t4r_head_split_dx"]}
# csrc/head_split.hip: 128-row x 128-column tiles; V = 33 / 129 / 257 / 1001 are one tile, one tile + 1, two + 1 and a ragged last tile
for _N, _V, _D, _sm in ((1, 33, 32, 0.0), (33, 129, 64, 0.1), (77, 257, 96, 0.0), (130, 1001, 128, 0.1), (129, 129, 64, 0.0)):
    # fdx_amax: at the fdx form's two small shapes (the table maximum does not depend on the tiling)
    for _form in ("mat", "fdx", "rc") + (("chunk",) if _V >= 129 else ()) + (("fdx_amax",) if _V <= 129 and _N <= 33 else ()):
        if _head_supported(_form, _D):        # "the recompute forms ... where *_supported says they exist" (pure host queries)
            case("head", f"head_split_{_form}-{_N}-{_V}-{_D}-e{_sm}", _HEAD_FORMS[_form])(_head_split(_N, _V, _D, _sm, _form))


# ================================================================================================================ serving heads
# Inputs are small dyadic rationals (multiples of 1/8 in [-3/8, 3/8]): exact in fp16 and bf16, every product a multiple of 1/64
# and every sum of up to 512 of them exact in fp32 -- so the scores have ONE correct value whatever the summation order, the fp64
# reference gives its bits, real ties occur (D = 1: seven distinct products) and "ties to the lower index" is checked exactly.
def dy(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).float() / 8


def _rank_rule(S, y):
    t = torch.gather(S, 1, y[:, None])
    cols = torch.arange(S.shape[1])[None, :]
    return t[:, 0], ((S > t) | ((S == t) & (cols < y[:, None]))).sum(1).to(I32)


def _topk_rule(S, k):
    o = torch.sort(S, dim=1, descending=True, stable=True)
    return o.values[:, :k], o.indices[:, :k]


def _item_topk_f32(n, V, D, k):
    def fn(a, key):
        lib = _lib().load()
        g = gen(n * 3 + V + D)
        x, W, y = dy(g, n, D), dy(g, V, D), torch.randint(0, V, (n,), generator=g)
        alpha = 0.5
        S = memo((key, "S"), lambda: alpha * x.double() @ W.double().t())
        rv, ri = _topk_rule(S, k)
        tgt, rank = _rank_rule(S, y)
        ldx, ldw = D + 4, D + 4
        X, Wb = a.new("X", "in", F32, (n, ldx), 0, D).set(x), a.new("W", "in", F32, (V, ldw), 0, D).set(W)
        OV, OI = a.new("out_val", "out", F32, (n, k)), a.new("out_idx", "out", I64, (n, k))
        nb = lib.t4r_item_topk_ws_bytes(n, V, D, k)
        WS = a.ws("workspace", nb)
        Y, TG = a.new("labels", "in", I64, n).set(y), a.new("target_score", "in", F32, n).set(tgt)
        RK = a.new("rank", "out", I32, n)
        st = (ctypes.c_long * 8)()
        call(a, "t4r_item_topk_f32", stream(), n, V, D, alpha, X.ptr, ldx, Wb.ptr, ldw, k, OV.ptr, OI.ptr, WS.ptr, nb,
             ctypes.cast(st, ctypes.c_void_p))
        call(a, "t4r_rank_of_target_f32", stream(), n, V, D, alpha, X.ptr, ldx, Wb.ptr, ldw, TG.ptr, Y.ptr, RK.ptr)
        t = "test_item_topk_gpu.py / test_kernels_gpu.py::test_rank_of_target_matches_topk_and_sort (bit for bit; exact inputs)"
        return [Out(OV, rv, None, t), Out(OI, ri, None, t), Out(RK, rank, None, t)]
    return fn


def _item_h16(n, V, D, k, dtype):
    def fn(a, key):
        lib = _lib().load()
        td, code = (torch.float16, 3) if dtype == "fp16" else (torch.bfloat16, 2)
        g = gen(n * 5 + V + D + code)
        x, W, y = dy(g, n, D), dy(g, V, D), torch.randint(0, V, (n,), generator=g)
        alpha = 0.5
        S = memo((key, "S"), lambda: alpha * x.double() @ W.double().t())
        rv, ri = _topk_rule(S, k)
        tgt, rank = _rank_rule(S, y)
        ild = lib.t4r_item_table_image_ld(D)
        ldx, ldw, ldp, ldc = D + 4, D + 4, ild + 8, (V + 3) // 4 * 4 + 4
        X, Wb = a.new("X", "in", F32, (n, ldx), 0, D).set(x), a.new("W", "in", F32, (V, ldw), 0, D).set(W)
        # include/t4r_hip.h: "W fp32 [V, D] (row pitch ldw) -> image [V, ldp], round to nearest even, pad columns zero" -- a wider
        # pitch is zero-filled to its end: the documented pad write of this entry
        IM = a.new("image", "out", td, (V, ldp), 0, D).allow(D, ldp)
        C = a.new("C", "out", F32, (n, ldc), 0, V)
        WS1 = a.ws("scores_ws", n * ild * 2)                          # "workspace: n_rows * t4r_item_table_image_ld(D) * 2 bytes"
        OV, OI = a.new("out_val", "out", F32, (n, k)), a.new("out_idx", "out", I64, (n, k))
        nb2 = lib.t4r_item_topk_h16_ws_bytes(n, V, D, k)
        WS2 = a.ws("topk_ws", nb2)
        Y = a.new("labels", "in", I64, n).set(y)
        LSE, TG, SS, RK = (a.new("lse", "out", F32, n), a.new("target", "out", F32, n), a.new("score_sum", "out", F32, n),
                           a.new("rank", "out", I32, n))
        nb3 = lib.t4r_item_eval_h16_ws_bytes(n, V, D)
        WS3 = a.ws("eval_ws", nb3)
        st = (ctypes.c_long * 8)()
        call(a, "t4r_item_table_pack_h16", stream(), Wb.ptr, ldw, V, D, code, IM.ptr, ldp)
        call(a, "t4r_item_scores_h16", stream(), n, V, D, alpha, X.ptr, ldx, IM.ptr, ldp, code, C.ptr, ldc, WS1.ptr, n * ild * 2)
        call(a, "t4r_item_topk_h16", stream(), n, V, D, alpha, X.ptr, ldx, IM.ptr, ldp, code, k, OV.ptr, OI.ptr, WS2.ptr, nb2,
             ctypes.cast(st, ctypes.c_void_p))
        call(a, "t4r_item_eval_h16", stream(), n, V, D, alpha, X.ptr, ldx, IM.ptr, ldp, code, Y.ptr, LSE.ptr, TG.ptr, SS.ptr, RK.ptr,
             WS3.ptr, nb3)
        torch.cuda.synchronize()
        assert bool((IM.t[:, D:] == 0).all()), "pad columns of the serving image must be zero to the end of the pitch"
        t = "test_item_topk_h16_gpu.py / test_item_eval_gpu.py (bit for bit; lse: LSE_TOL 2e-5)"
        return [Out(IM, W, None, t), Out(C, S, None, t), Out(OV, rv, None, t), Out(OI, ri, None, t),
                Out(LSE, torch.logsumexp(S, 1), dict(rtol=0, atol=2e-5), t), Out(TG, tgt, None, t), Out(SS, S.sum(1), None, t),
                Out(RK, rank, None, t)]
    return fn


_H16_ENTRIES = ["t4r_item_table_pack_h16", "t4r_item_scores_h16", "t4r_item_topk_h16", "t4r_item_eval_h16"]
_i = 0
for _n in (1, 33):
    for _V in (7, 129, 1000):
        for _k in sorted({1, min(20, _V), min(_V, 256)}):
            for _D in (1, 512):                                       # the smallest and the largest width the 16-bit head takes
                _i += 1
                case("serving", f"item_topk_f32-{_n}-{_V}-{_D}-k{_k}", ["t4r_item_topk_f32", "t4r_rank_of_target_f32"])(
                    _item_topk_f32(_n, _V, _D, _k))
                _dt = "fp16" if _i % 2 else "bf16"
                case("serving", f"item_h16-{_dt}-{_n}-{_V}-{_D}-k{_k}", _H16_ENTRIES)(_item_h16(_n, _V, _D, _k, _dt))
for _dt in ("fp16", "bf16"):
    case("serving", f"item_h16-{_dt}-33-129-20-k20", _H16_ENTRIES)(_item_h16(33, 129, 20, 20, _dt))
case("serving", "item_topk_f32-33-129-20-k20", ["t4r_item_topk_f32", "t4r_rank_of_target_f32"])(_item_topk_f32(33, 129, 20, 20))


# ================================================================================================================ attention
def _keep(seed, ctr, shape, p):
    import device_rng as R
    n = 1
    for s in shape:
        n *= s
    pf = float(torch.tensor(p, dtype=F32))
    return torch.from_numpy(R.dropout_keep(seed, ctr, n, p).copy()).view(*shape).double() / (1 - pf)


def _xlnet_attn_ref(q, k, v, kr, rw, rr, dout, per_b, keep, key_len):
    B, L, n, dh = q.shape
    q_, k_, v_, kr_, rw_, rr_ = (t.double().clone().requires_grad_() for t in (q, k, v, kr, rw, rr))
    ac = torch.einsum("bind,bjnd->bnij", q_ + rw_, k_)
    bd_full = torch.einsum("bind,bpnd->bnip", q_ + rr_, kr_) if per_b else torch.einsum("bind,pnd->bnip", q_ + rr_, kr_)
    idx = torch.arange(L)[None, :] + L - torch.arange(L)[:, None]
    bd = torch.gather(bd_full, 3, idx[None, None].expand(B, n, L, L))
    s = (ac + bd) / dh ** 0.5
    if key_len is not None:
        j, i = torch.arange(L)[None, None, None, :], torch.arange(L)[None, None, :, None]
        s = s - 1e30 * ((j >= key_len[:, None, None, None]) & (i != j)).double()
    prob = torch.softmax(s, 3)
    if keep is not None:
        prob = prob * keep
    out = torch.einsum("bnij,bjnd->bind", prob, v_)
    out.backward(dout.double())
    return out.detach(), [t.grad for t in (q_, k_, v_, kr_, rw_, rr_)]


def _xlnet_attn(B, L, D, n, per_b, p, use_kl):
    def fn(a, key):
        ops = _ops()
        lib = _lib().load()
        g = gen(B * L + D + int(per_b))
        dh = D // n
        q, k, v = (rn(g, B, L, n, dh) for _ in range(3))
        kr = rn(g, B, 2 * L, n, dh) if per_b else rn(g, 2 * L, n, dh)
        rw, rr, dout = rn(g, n, dh, scale=0.5), rn(g, n, dh, scale=0.5), rn(g, B, L, n, dh)
        kl = torch.randint(1, L + 1, (B,), generator=g) if use_kl else None
        seed, ctr = 5, ops.dropout_ctr_hi(3, 1, ops.SITE_PROB)
        out, grads = memo(key, lambda: _xlnet_attn_ref(q, k, v, kr, rw, rr, dout, per_b,
                                                       _keep(seed, ctr, (B, n, L, L), p) if p > 0 else None, kl))
        T = B * L
        mk = lambda name, t: a.new(name, "in", F32, (t.numel() // D, D)).set(t.reshape(-1, D))
        Q, K, V, KR, DO = mk("q", q), mk("k", k), mk("v", v), mk("k_r", kr), mk("dout", dout)
        RW, RR = a.new("r_w_bias", "in", F32, D).set(rw.reshape(-1)), a.new("r_r_bias", "in", F32, D).set(rr.reshape(-1))
        KL = a.new("key_len", "in", I32, B).set(kl) if use_kl else None
        O, LSE = a.new("out", "out", F32, (T, D)), a.new("lse", "out", F32, B * n * L)
        DQ, DK, DV = a.new("dq", "out", F32, (T, D)), a.new("dk", "out", F32, (T, D)), a.new("dv", "out", F32, (T, D))
        DKR = a.new("dk_r", "out", F32, (KR.shape[0], D))
        # include/t4r_hip.h: "backward: d_r_w_bias / d_r_r_bias accumulated, the rest overwritten"
        DRW, DRR = a.new("d_r_w_bias", "inout", F32, D).set(1.0), a.new("d_r_r_bias", "inout", F32, D).set(1.0)
        WS = a.ws("workspace", 4 * lib.t4r_xlnet_attn_bwd_ws_floats(B, L, D, n))
        klp = KL.ptr if use_kl else None
        call(a, "t4r_xlnet_attn_fwd", stream(), Q.ptr, K.ptr, V.ptr, KR.ptr, RW.ptr, RR.ptr, O.ptr, LSE.ptr, B, L, n, dh, int(per_b),
             p, seed, ctr, klp)
        call(a, "t4r_xlnet_attn_bwd", stream(), Q.ptr, K.ptr, V.ptr, KR.ptr, RW.ptr, RR.ptr, O.ptr, LSE.ptr, DO.ptr, DQ.ptr, DK.ptr,
             DV.ptr, DKR.ptr, DRW.ptr, DRR.ptr, WS.ptr, B, L, n, dh, int(per_b), p, seed, ctr, klp)
        plain = not per_b and p == 0
        t = ("test_kernels_gpu.py::test_xlnet_attention_core" if plain else
             "test_kernels_gpu.py::test_xlnet_attention_dropout_per_session_kr")
        tl = lambda at: dict(rtol=2e-5, atol=at)
        to, td, tb = (2e-5, 1e-4, 3e-4) if plain else (3e-5, 2e-4, 5e-4)
        return [Out(O, out, tl(to), t), Out(LSE), Out(DQ, grads[0], tl(td), t), Out(DK, grads[1], tl(td), t), Out(DV, grads[2], tl(td), t),
                Out(DKR, grads[3], tl(2e-4), t), Out(DRW, grads[4].reshape(-1) + 1, tl(tb), t), Out(DRR, grads[5].reshape(-1) + 1, tl(tb), t)]
    return fn


# one-wave kernels (MFMA for L <= 32, d_head 16 / 32; VALU up to 64 positions), the general kernels beyond, a head width that
# is no multiple of 4 (25), a head count the heads-per-block does not divide (3), L = 1
for _B, _L, _D, _n in ((3, 20, 64, 4), (2, 65, 32, 2), (2, 70, 50, 2), (3, 33, 96, 3), (2, 1, 64, 2)):
    case("attention", f"xlnet_attn-{_B}-{_L}-{_D}-{_n}-shared", ["t4r_xlnet_attn_fwd", "t4r_xlnet_attn_bwd"])(
        _xlnet_attn(_B, _L, _D, _n, False, 0.0, False))
    case("attention", f"xlnet_attn-{_B}-{_L}-{_D}-{_n}-persession-p0.3-keylen", ["t4r_xlnet_attn_fwd", "t4r_xlnet_attn_bwd"])(
        _xlnet_attn(_B, _L, _D, _n, True, 0.3, True))


def _mha_ref(qkv, dout, B, L, n, causal, keep, key_len):
    D = qkv.shape[1] // 3
    dh = D // n
    r = qkv.double().clone().requires_grad_()
    q, k, v = (r[:, i * D:(i + 1) * D].view(B, L, n, dh).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / dh ** 0.5
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
    if key_len is not None:
        s = s.masked_fill(torch.arange(L)[None, None, None, :] >= key_len[:, None, None, None], float("-inf"))
    prob = torch.softmax(s, -1)
    if keep is not None:
        prob = prob * keep
    out = (prob @ v).transpose(1, 2).reshape(B * L, D)
    out.backward(dout.double())
    return out.detach(), r.grad


def _mha(B, L, D, n, causal, p, fused, use_kl):
    def fn(a, key):
        ops = _ops()
        g = gen(B + L + D + int(causal))
        dh, T = D // n, B * L
        qkv, dout = rn(g, T, 3 * D), rn(g, T, D)
        kl = torch.randint(1, L + 1, (B,), generator=g) if use_kl else None
        seed, ctr = 5, ops.dropout_ctr_hi(3, 1, ops.SITE_PROB)
        out, dqkv = memo(key, lambda: _mha_ref(qkv, dout, B, L, n, causal, _keep(seed, ctr, (B, n, L, L), p) if p > 0 else None, kl))
        ldo = D + 4
        DO = a.new("dout", "in", F32, (T, ldo), 0, D).set(dout)
        O, LSE = a.new("out", "out", F32, (T, ldo), 0, D), a.new("lse", "out", F32, B * n * L)
        KL = a.new("key_len", "in", I32, B).set(kl) if use_kl else None
        klp = KL.ptr if use_kl else None
        tl = lambda rt, at: dict(rtol=rt, atol=at)
        t = "test_kernels_gpu.py::test_mha_fwd_bwd / test_mha_padding_mask"
        if fused:        # GPT-2's fused c_attn output: q | k | v are column blocks of one [T, 3D] buffer, and so are dq | dk | dv
            QKV = a.new("qkv", "in", F32, (T, 3 * D)).set(qkv)
            DQKV = a.new("dqkv", "out", F32, (T, 3 * D))
            qp, kp, vp, ld = QKV.ptr, QKV.ptr + 4 * D, QKV.ptr + 8 * D, 3 * D
            dqp, dkp, dvp, ldd = DQKV.ptr, DQKV.ptr + 4 * D, DQKV.ptr + 8 * D, 3 * D
            outs = [Out(DQKV, dqkv, tl(1e-4, 2e-4), t)]
        else:
            ld = ldd = D + 4
            Q, K, V = (a.new(nm, "in", F32, (T, ld), 0, D).set(qkv[:, i * D:(i + 1) * D]) for i, nm in enumerate(("q", "k", "v")))
            DQ, DK, DV = (a.new(nm, "out", F32, (T, ldd), 0, D) for nm in ("dq", "dk", "dv"))
            qp, kp, vp, dqp, dkp, dvp = Q.ptr, K.ptr, V.ptr, DQ.ptr, DK.ptr, DV.ptr
            outs = [Out(b, dqkv[:, i * D:(i + 1) * D], tl(1e-4, 2e-4), t) for i, b in enumerate((DQ, DK, DV))]
        call(a, "t4r_mha_fwd", stream(), qp, kp, vp, ld, O.ptr, ldo, LSE.ptr, B, L, n, dh, int(causal), p, seed, ctr, klp)
        call(a, "t4r_mha_bwd", stream(), qp, kp, vp, ld, O.ptr, DO.ptr, ldo, LSE.ptr, dqp, dkp, dvp, ldd, B, L, n, dh, int(causal), p,
             seed, ctr, klp)
        return [Out(O, out, tl(2e-5, 3e-5), t), Out(LSE)] + outs
    return fn


# LDS / MFMA kernels up to 128 positions with d_head 16 | 32 | 64, the general kernels beyond (L = 129) and for d_head 25
for _B, _L, _D, _n in ((3, 33, 64, 4), (2, 129, 64, 2), (2, 30, 100, 4), (2, 1, 32, 2)):
    case("attention", f"mha-{_B}-{_L}-{_D}-{_n}-causal-fused", ["t4r_mha_fwd", "t4r_mha_bwd"])(_mha(_B, _L, _D, _n, True, 0.0, True, False))
    case("attention", f"mha-{_B}-{_L}-{_D}-{_n}-p0.3-separate-keylen", ["t4r_mha_fwd", "t4r_mha_bwd"])(
        _mha(_B, _L, _D, _n, False, 0.3, False, True))
    case("attention", f"mha-{_B}-{_L}-{_D}-{_n}-causal-keylen-fused", ["t4r_mha_fwd", "t4r_mha_bwd"])(_mha(_B, _L, _D, _n, True, 0.0, True, True))


# ================================================================================================================ XLNet layer
ORDER = ("q", "k", "v", "o", "r", "r_w_bias", "r_r_bias", "ln_w", "ln_b", "w1", "b1", "w2", "b2", "ff_ln_w", "ff_ln_b")
_XL_SHAPES = ((3, 20, 64, 4), (5, 17, 128, 4), (1, 1, 32, 2))      # T = 60, 85, 1: multiples of neither the 16- nor the 80-row tile


def _xl_params(g, D, n, scale=0.1):
    dh = D // n
    r = lambda *s: scale * torch.randn(*s, generator=g)
    return dict(q=r(D, n, dh), k=r(D, n, dh), v=r(D, n, dh), o=r(D, n, dh), r=r(D, n, dh), r_w_bias=r(n, dh), r_r_bias=r(n, dh),
                ln_w=1 + r(D), ln_b=r(D), w1=r(4 * D, D), b1=r(4 * D), w2=r(D, 4 * D), b2=r(D), ff_ln_w=1 + r(D), ff_ln_b=r(D))


def _xl_param_bufs(a, p, tag=""):
    return [a.new(f"param{tag}_{k}", "in", F32, p[k].numel()).set(p[k].reshape(-1)) for k in ORDER]


def _rel(c, ref):
    """the existing tests' rel_err(a, ref) < c: |a - ref| <= c * max |ref|"""
    return dict(rtol=0, atol=c * max(float(ref.abs().max()), 1e-30))


def _xlnet_pieces(T, D, n, p):
    def fn(a, key):
        ops = _ops()
        lib = _lib().load()
        g = gen(T * 3 + D)
        prm = _xl_params(g, D, n)
        h, av, dy, dy2, h1in = (rn(g, T, D) for _ in range(5))
        dqkv, base, pos = rn(g, 3, T, D), rn(g, T, D), rn(g, 53, D)
        seed, c_out, c_act, c_ffo = 77, 12345, 4004, 5005
        eps = 0.03

        def mk():
            P = {k: v.double().clone().requires_grad_() for k, v in prm.items()}
            r = {}
            for z, nm in enumerate("qkv"):
                r[nm] = h.double() @ P[nm].detach().reshape(D, D)
            r["kr"] = pos.double() @ P["r"].detach().reshape(D, D)
            av_, h_ = av.double().clone().requires_grad_(), h.double().clone().requires_grad_()
            m = _keep(seed, c_out, (T, D), p) if p > 0 else torch.ones(T, D, dtype=torch.float64)
            ao = av_ @ P["o"].detach().reshape(D, D).t()
            x = ao * m + h_
            y1 = torch.nn.functional.layer_norm(x, (D,), P["ln_w"], P["ln_b"], eps)
            y1.backward(dy.double())
            r.update(ao=ao.detach(), h1=y1.detach(), mean=x.detach().mean(-1), dh=h_.grad, dav=av_.grad, dao=h_.grad * m,
                     dg1=P["ln_w"].grad, db1_=P["ln_b"].grad)
            r["dh_acc"] = base.double() + sum(dqkv[z].double() @ P[nm].detach().reshape(D, D).t() for z, nm in enumerate("qkv"))
            h1_ = h1in.double().clone().requires_grad_()
            ma = _keep(seed, c_act, (T, 4 * D), p) if p > 0 else 1.0
            mo = _keep(seed, c_ffo, (T, D), p) if p > 0 else 1.0
            pre = h1_ @ P["w1"].t() + P["b1"]
            act = torch.nn.functional.gelu(pre) * ma
            ffo = act @ P["w2"].t() + P["b2"]
            y2 = torch.nn.functional.layer_norm(ffo * mo + h1_, (D,), P["ff_ln_w"], P["ff_ln_b"], eps)
            y2.backward(dy2.double())
            r.update(pre=pre.detach(), act=act.detach(), ffo=ffo.detach(), hout=y2.detach(), dh1=h1_.grad, gb1=P["b1"].grad,
                     gb2=P["b2"].grad, gg2=P["ff_ln_w"].grad, gbe2=P["ff_ln_b"].grad, gw1=P["w1"].grad, gw2=P["w2"].grad)
            return r
        R = memo(key, mk)
        PB = _xl_param_bufs(a, prm)
        pb = dict(zip(ORDER, PB))
        PL = a.ws("planes", 4 * lib.t4r_xlnet_layer_planes_floats(D))
        PF = a.ws("ff_planes", 4 * lib.t4r_xlnet_ff_planes_floats(D))
        mkin = lambda nm, t: a.new(nm, "in", F32, tuple(t.shape) if t.dim() <= 2 else (t.shape[0] * t.shape[1], t.shape[2])).set(t.reshape(-1, t.shape[-1]))
        H, AV, DY, DY2, H1I, DQKV, POS = (mkin(nm, t) for nm, t in (("h", h), ("av", av), ("dy", dy), ("dy2", dy2), ("h1_in", h1in),
                                                                     ("dqkv", dqkv), ("pos", pos)))
        QKV, KR = a.new("qkv", "out", F32, (3 * T, D)), a.new("kr", "out", F32, (53, D))
        AO, MU, RS, H1 = a.new("ao", "out", F32, (T, D)), a.new("mean", "out", F32, T), a.new("rstd", "out", F32, T), a.new("h1", "out", F32, (T, D))
        DH, DAO, DAV = (a.new(nm, "out", F32, (T, D)) for nm in ("dh", "dao", "dav"))
        # include/t4r_hip.h: "d_gamma, d_beta ACCUMULATED; part: t4r_xlnet_ln1_bwd_part_floats(T, D) floats"
        DG1, DB1 = a.new("d_gamma1", "inout", F32, D).set(1.0), a.new("d_beta1", "inout", F32, D).set(1.0)
        PART1 = a.ws("ln1_part", 4 * lib.t4r_xlnet_ln1_bwd_part_floats(T, D))
        DHA = a.new("dh_acc", "inout", F32, (T, D)).set(base)            # "dh [T, D] += d q @ W_q^T + d k @ W_k^T + d v @ W_v^T"
        FPRE, FACT = a.new("ffpre", "out", F32, (T, 4 * D)), a.new("ffact", "out", F32, (T, 4 * D))
        FOUT, MU2, RS2, HOUT = a.new("ffout", "out", F32, (T, D)), a.new("mean2", "out", F32, T), a.new("rstd2", "out", F32, T), a.new("hout", "out", F32, (T, D))
        HINF = a.new("hout_inference", "out", F32, (T, D))
        DH1, DFO, DPRE = a.new("dh1", "out", F32, (T, D)), a.new("dffout", "out", F32, (T, D)), a.new("dpre", "out", F32, (T, 4 * D))
        # "d_gamma, d_beta, d_b2 [D], d_b1 [4D] are ACCUMULATED ... part: t4r_xlnet_ff_bwd_part_floats(T, D) floats of scratch"
        DG2, DBE2, DB2 = (a.new(nm, "inout", F32, D).set(1.0) for nm in ("d_gamma2", "d_beta2", "d_b2"))
        DB1F = a.new("d_b1", "inout", F32, 4 * D).set(1.0)
        PART2 = a.ws("ff_part", 4 * lib.t4r_xlnet_ff_bwd_part_floats(T, D))
        parr, _k = _lib().ptr_array([b.ptr for b in PB])
        s = stream()
        call(a, "t4r_xlnet_layer_prepare", s, parr, D, PL.ptr)
        call(a, "t4r_xlnet_ff_prepare", s, pb["w1"].ptr, pb["b1"].ptr, pb["w2"].ptr, D, PF.ptr)
        call(a, "t4r_xlnet_qkv_proj", s, H.ptr, PL.ptr, QKV.ptr, T, D)
        call(a, "t4r_xlnet_kr_proj", s, POS.ptr, PL.ptr, KR.ptr, 53, D)
        call(a, "t4r_xlnet_oproj_ln", s, AV.ptr, H.ptr, PL.ptr, pb["ln_w"].ptr, pb["ln_b"].ptr, AO.ptr, MU.ptr, RS.ptr, H1.ptr, T, D, eps,
             p, seed, c_out)
        call(a, "t4r_xlnet_ln1_bwd", s, DY.ptr, AO.ptr, H.ptr, MU.ptr, RS.ptr, pb["ln_w"].ptr, PL.ptr, DH.ptr, DAO.ptr, DAV.ptr, DG1.ptr,
             DB1.ptr, PART1.ptr, T, D, p, seed, c_out)
        call(a, "t4r_xlnet_dh", s, DQKV.ptr, PL.ptr, DHA.ptr, T, D)
        # the feed-forward pair on the planes t4r_xlnet_ff_prepare cut ("the feed-forward planes only (same buffer layout)")
        call(a, "t4r_xlnet_ff_fwd", s, H1I.ptr, PF.ptr, pb["b1"].ptr, pb["b2"].ptr, pb["ff_ln_w"].ptr, pb["ff_ln_b"].ptr, FPRE.ptr, FACT.ptr,
             FOUT.ptr, MU2.ptr, RS2.ptr, HOUT.ptr, T, D, eps, p, seed, c_act, c_ffo)
        call(a, "t4r_xlnet_ff_bwd", s, DY2.ptr, FOUT.ptr, H1I.ptr, MU2.ptr, RS2.ptr, pb["ff_ln_w"].ptr, FPRE.ptr, PF.ptr, DH1.ptr, DFO.ptr,
             DPRE.ptr, DG2.ptr, DBE2.ptr, DB2.ptr, DB1F.ptr, PART2.ptr, T, D, p, seed, c_act, c_ffo)
        if p == 0:      # "Inference form: all five NULL"
            call(a, "t4r_xlnet_ff_fwd", s, H1I.ptr, PL.ptr, pb["b1"].ptr, pb["b2"].ptr, pb["ff_ln_w"].ptr, pb["ff_ln_b"].ptr, None, None, None,
                 None, None, HINF.ptr, T, D, eps, 0.0, 0, 0, 0)
        t = "test_fused_gpu.py (rel_err bounds of the same outputs)"
        acc = lambda ref, c: dict(rtol=0, atol=c * max(float(ref.abs().max()), 1e-30))
        qkv_ref = torch.stack([R["q"], R["k"], R["v"]]).reshape(3 * T, D)
        outs = [Out(QKV, qkv_ref, dict(rtol=0, atol=3e-6 * min(float(R[nm].abs().max()) for nm in "qkv")), t), Out(KR, R["kr"], _rel(3e-6, R["kr"]), t),
                Out(AO, R["ao"], _rel(3e-6, R["ao"]), t), Out(H1, R["h1"], _rel(5e-6, R["h1"]), t),
                Out(MU, R["mean"], dict(rtol=1e-5, atol=1e-6), t), Out(RS),
                Out(DH, R["dh"], _rel(2e-5, R["dh"]), t), Out(DAV, R["dav"], _rel(2e-5, R["dav"]), t), Out(DAO, R["dao"], _rel(2e-5, R["dao"]), t),
                Out(DG1, R["dg1"] + 1, acc(R["dg1"], 3e-5), t), Out(DB1, R["db1_"] + 1, acc(R["db1_"], 3e-5), t),
                Out(DHA, R["dh_acc"], _rel(3e-6, R["dh_acc"]), t),
                Out(FPRE, R["pre"], _rel(3e-6, R["pre"]), t), Out(FACT, R["act"], _rel(3e-6, R["act"]), t), Out(FOUT, R["ffo"], _rel(5e-6, R["ffo"]), t),
                Out(HOUT, R["hout"], _rel(1e-5, R["hout"]), t), Out(MU2), Out(RS2),
                Out(DH1, R["dh1"], _rel(3e-5, R["dh1"]), t), Out(DB1F, R["gb1"] + 1, acc(R["gb1"], 3e-5), t), Out(DB2, R["gb2"] + 1, acc(R["gb2"], 3e-5), t),
                Out(DG2, R["gg2"] + 1, acc(R["gg2"], 3e-5), t), Out(DBE2, R["gbe2"] + 1, acc(R["gbe2"], 3e-5), t),
                # the rows the two weight gradients contract over: d W2 = dffout^T @ ffact, d W1 = dpre^T @ h1
                Out(DFO), Out(DPRE),
                Out(DFO, R["gw2"], _rel(3e-5, R["gw2"]), t, sel=lambda v: v.double().t().cpu() @ R["act"]),
                Out(DPRE, R["gw1"], _rel(3e-5, R["gw1"]), t, sel=lambda v: v.double().t().cpu() @ h1in.double())]
        if p == 0:
            outs.append(Out(HINF, R["hout"], _rel(1e-5, R["hout"]), t))
        return outs
    return fn


_XL_PIECES = ["t4r_xlnet_layer_prepare", "t4r_xlnet_ff_prepare", "t4r_xlnet_qkv_proj", "t4r_xlnet_kr_proj", "t4r_xlnet_oproj_ln",
              "t4r_xlnet_ln1_bwd", "t4r_xlnet_dh", "t4r_xlnet_ff_fwd", "t4r_xlnet_ff_bwd"]
for _B, _L, _D, _n in _XL_SHAPES:
    for _p in (0.0, 0.3):
        if _lib().load().t4r_xlnet_fused_supported(_D):
            case("xlnet", f"xlnet_pieces-{_B * _L}-{_D}-{_n}-p{_p}", _XL_PIECES)(_xlnet_pieces(_B * _L, _D, _n, _p))


def _xlnet_layer(B, L, D, n, p, defer, stack):
    def fn(a, key):
        import t4r_oracle as Orc
        ops = _ops()
        lib = _lib().load()
        g = gen(B + L + D)
        prm = _xl_params(g, D, n)
        h, dout = rn(g, B, L, D), rn(g, B, L, D)
        seed, offset, layer, eps = 99, 7, 2, 0.03
        pos = Orc.xlnet_pos_emb(L, D)

        def mk():
            P = {k: v.double().clone().requires_grad_() for k, v in prm.items()}
            hr = h.double().clone().requires_grad_()
            if p > 0:
                Cc = lambda site: ops.dropout_ctr_hi(offset, layer, site)
                masks = dict(pos=_keep(seed, ops.dropout_ctr_hi(offset, 255, ops.SITE_POS), (B, 2 * L, D), p),
                             prob=_keep(seed, Cc(ops.SITE_PROB), (B, n, L, L), p), attn_out=_keep(seed, Cc(ops.SITE_ATTN_OUT), (B, L, D), p),
                             ff_act=_keep(seed, Cc(ops.SITE_FF_ACT), (B, L, 4 * D), p), ff_out=_keep(seed, Cc(ops.SITE_FF_OUT), (B, L, D), p))
                masks = {k: (v != 0).double() for k, v in masks.items()}      # the oracle takes 0 / 1 masks and scales by 1 / (1 - p) itself
                ref = Orc.xlnet_layer_dropout(hr, P, n, eps, masks, p)
            else:
                ref = Orc.xlnet_layer(hr, P, n, eps)
            ref.backward(dout.double())
            return ref.detach(), hr.grad, {k: P[k].grad for k in ORDER}
        out, dh, gr = memo(key, mk)
        T = B * L
        PB = _xl_param_bufs(a, prm)
        # include/t4r_hip.h conventions: "'accumulated' outputs are read-modify-write (parameter gradients)"
        GB = [a.new(f"grad_{k}", "inout", F32, prm[k].numel()).set(1.0) for k in ORDER]
        H, DO, PE = a.new("h", "in", F32, (T, D)).set(h.reshape(T, D)), a.new("dh_out", "in", F32, (T, D)).set(dout.reshape(T, D)), \
            a.new("pos_emb", "in", F32, (2 * L, D)).set(pos)
        WS = a.ws("ws", 4 * lib.t4r_xlnet_layer_ws_floats(B, L, D, n, int(p > 0)))
        BWS = a.ws("bws", 4 * lib.t4r_xlnet_layer_bwd_ws_floats(B, L, D, n, int(p > 0)))
        HO, DHI = a.new("h_out", "out", F32, (T, D)), a.new("dh_in", "out", F32, (T, D))
        parr, _k1 = _lib().ptr_array([b.ptr for b in PB])
        garr, _k2 = _lib().ptr_array([b.ptr for b in GB])
        s = stream()
        if stack:
            po, ko = ctypes.c_long(0), ctypes.c_long(0)
            call(a, "t4r_xlnet_layer_ws_offsets", B, L, D, n, int(p > 0), ctypes.addressof(po), ctypes.addressof(ko))
            planes, _k3 = _lib().ptr_array([WS.ptr + 4 * po.value])
            kr, _k4 = _lib().ptr_array([WS.ptr + 4 * ko.value])
            call(a, "t4r_xlnet_stack_prepare", s, parr, 1, D, planes, PE.ptr, 2 * L, kr)
        # the options are bits of layer_idx (include/t4r_hip.h: T4R_LAYER_STACK_PREPARED, T4R_LAYER_DEFER_JOIN), each given to
        # the one call it is meant for
        call(a, "t4r_xlnet_layer_fwd", s, H.ptr, PE.ptr, parr, WS.ptr, HO.ptr, B, L, D, n, eps, p, seed, offset,
             layer | (ops.LAYER_STACK_PREPARED if stack else 0), None, None)
        call(a, "t4r_xlnet_layer_bwd", s, H.ptr, PE.ptr, parr, garr, WS.ptr, BWS.ptr, DO.ptr, DHI.ptr, B, L, D, n, eps, p, seed, offset,
             layer | (ops.LAYER_DEFER_JOIN if defer else 0), None, None)
        if defer:
            call(a, "t4r_xlnet_layer_bwd_join", s)          # "calls t4r_xlnet_layer_bwd_join(stream) before the gradients are read"
        t = "test_kernels_gpu.py::test_xlnet_layer_fwd_bwd" if p == 0 else "test_kernels_gpu.py::test_xlnet_layer_dropout_fwd_bwd"
        ao, ad, ag = (3e-5, 2e-4, 5e-4) if p == 0 else (5e-5, 3e-4, 8e-4)
        return [Out(HO, out.reshape(T, D), dict(rtol=2e-5, atol=ao), t), Out(DHI, dh.reshape(T, D), dict(rtol=1e-4, atol=ad), t)] + \
               [Out(b, gr[k].reshape(-1) + 1, dict(rtol=1e-4, atol=ag), t) for k, b in zip(ORDER, GB)]
    return fn


for _B, _L, _D, _n in _XL_SHAPES:
    for _p, _defer, _stack in ((0.0, False, False), (0.3, False, False), (0.0, True, False), (0.0, False, True)):
        _ents = ["t4r_xlnet_layer_fwd", "t4r_xlnet_layer_bwd"] + (["t4r_xlnet_layer_bwd_join"] if _defer else []) + \
                (["t4r_xlnet_stack_prepare"] if _stack else [])
        if _stack and not _lib().load().t4r_xlnet_fused_supported(_D):
            continue
        case("xlnet", f"xlnet_layer-{_B}-{_L}-{_D}-{_n}-p{_p}" + ("-deferred" if _defer else "") + ("-stack" if _stack else ""), _ents)(
            _xlnet_layer(_B, _L, _D, _n, _p, _defer, _stack))


def _stack_prepare_drop(n_layers):
    """t4r_xlnet_stack_prepare_drop: the stack prologue that makes the dropped positional rows itself.  `dropped` must be, bit
    for bit, what t4r_dropout gives over the expanded encoding with the same key, and every kr[l], bit for bit, what
    t4r_xlnet_stack_prepare gives over those dropped rows (the two-call form it replaces).  The prologue projects four layers per
    launch: n_layers = 5 crosses the group boundary."""
    B, L, D, n, p = 2, 5, 32, 2, 0.3

    def fn(a, key):
        import t4r_oracle as Orc
        ops = _ops()
        lib = _lib().load()
        g = gen(1000 + n_layers)
        prms = [_xl_params(g, D, n) for _ in range(n_layers)]
        pos = Orc.xlnet_pos_emb(L, D).to(F32)
        period, rows = 2 * L, B * 2 * L
        seed, ctr = 99, ops.dropout_ctr_hi(7, 255, ops.SITE_POS)
        npl = lib.t4r_xlnet_layer_planes_floats(D)

        def mk():       # the two-call form, on plain device tensors
            flat = [pr[k].to(DEV, F32).contiguous() for pr in prms for k in ORDER]
            pl = [torch.empty(npl, device=DEV, dtype=F32) for _ in prms]
            krs = [torch.empty(rows, D, device=DEV, dtype=F32) for _ in prms]
            src, dropped = pos.to(DEV).contiguous(), torch.empty(rows, D, device=DEV, dtype=F32)
            parr, _k0 = _lib().ptr_array([t.data_ptr() for t in flat])
            planes, _k1 = _lib().ptr_array([t.data_ptr() for t in pl])
            kr, _k2 = _lib().ptr_array([t.data_ptr() for t in krs])
            _lib().call("t4r_dropout", stream(), src.data_ptr(), dropped.data_ptr(), None, rows * D, period * D, p, seed, ctr)
            _lib().call("t4r_xlnet_stack_prepare", stream(), parr, n_layers, D, planes, dropped.data_ptr(), rows, kr)
            torch.cuda.synchronize()
            return dropped.cpu(), [t.cpu() for t in krs]
        dropped_ref, kr_ref = memo(key, mk)
        PB = [b for l, pr in enumerate(prms) for b in _xl_param_bufs(a, pr, tag=str(l))]
        POS = a.new("pos", "in", F32, (period, D)).set(pos)
        PL = [a.ws(f"planes{l}", 4 * npl) for l in range(n_layers)]
        KR = [a.new(f"kr{l}", "out", F32, (rows, D)) for l in range(n_layers)]
        DR = a.new("dropped", "out", F32, (rows, D))
        parr, _k0 = _lib().ptr_array([b.ptr for b in PB])
        planes, _k1 = _lib().ptr_array([b.ptr for b in PL])
        kr, _k2 = _lib().ptr_array([b.ptr for b in KR])
        call(a, "t4r_xlnet_stack_prepare_drop", stream(), parr, n_layers, D, planes, POS.ptr, rows, kr, p, seed, ctr, period, DR.ptr)
        torch.cuda.synchronize()
        t = "bit for bit the two-call form: t4r_dropout, then t4r_xlnet_stack_prepare over its rows"
        for b, ref in [(DR, dropped_ref)] + list(zip(KR, kr_ref)):
            assert _bits_equal(b.win.cpu(), ref), f"{key}: '{b.name}' is not {t}"
        assert float((dropped_ref == 0).float().mean()) > 0.1, "the dropout mask must drop something for the comparison to mean anything"
        return [Out(DR, dropped_ref, None, t)] + [Out(b, ref, None, t) for b, ref in zip(KR, kr_ref)]
    return fn


if _lib().load().t4r_xlnet_fused_supported(32):
    for _nl in (1, 5):
        case("xlnet", f"stack_prepare_drop-2-5-32-p0.3-layers{_nl}", ["t4r_xlnet_stack_prepare_drop"])(_stack_prepare_drop(_nl))


def _attn_block(B, L, D, n, p, use_kl):
    def fn(a, key):
        import t4r_oracle as Orc
        ops = _ops()
        lib = _lib().load()
        g = gen(B * 7 + L + D)
        prm = _xl_params(g, D, n)
        dh, T, eps = D // n, B * L, 0.03
        h = rn(g, T, D)
        kl = torch.randint(1, L + 1, (B,), generator=g) if use_kl else None
        seed, c_prob, c_out = 31, ops.dropout_ctr_hi(2, 1, ops.SITE_PROB), ops.dropout_ctr_hi(2, 1, ops.SITE_ATTN_OUT)
        kr = (Orc.xlnet_pos_emb(L, D).double() @ prm["r"].double().reshape(D, D)).float()

        def mk():
            P = {k: v.double() for k, v in prm.items()}
            q, k, v = (h.double() @ P[nm].reshape(D, D) for nm in "qkv")
            r4 = lambda t: t.reshape(B, L, n, dh)
            ac = torch.einsum("bind,bjnd->bnij", r4(q) + P["r_w_bias"], r4(k))
            bd_full = torch.einsum("bind,pnd->bnip", r4(q) + P["r_r_bias"], kr.double().reshape(2 * L, n, dh))
            idx = torch.arange(L)[None, :] + L - torch.arange(L)[:, None]
            s = (ac + torch.gather(bd_full, 3, idx[None, None].expand(B, n, L, L))) / dh ** 0.5
            if kl is not None:
                j, i = torch.arange(L)[None, None, None, :], torch.arange(L)[None, None, :, None]
                s = s - 1e30 * ((j >= kl[:, None, None, None]) & (i != j)).double()
            lse = torch.logsumexp(s, 3)
            prob = torch.softmax(s, 3)
            if p > 0:
                prob = prob * _keep(seed, c_prob, (B, n, L, L), p)
            av = torch.einsum("bnij,bjnd->bind", prob, r4(v)).reshape(T, D)
            ao = av @ P["o"].reshape(D, D).t()
            x = (ao * _keep(seed, c_out, (T, D), p) if p > 0 else ao) + h.double()
            h1 = torch.nn.functional.layer_norm(x, (D,), P["ln_w"], P["ln_b"], eps)
            return dict(qkv=torch.cat([q, k, v]), av=av, lse=lse.reshape(-1), ao=ao, h1=h1)
        R = memo(key, mk)
        PB = _xl_param_bufs(a, prm)
        pb = dict(zip(ORDER, PB))
        PL = a.ws("planes", 4 * lib.t4r_xlnet_layer_planes_floats(D))
        H, KR = a.new("h", "in", F32, (T, D)).set(h), a.new("kr", "in", F32, (2 * L, D)).set(kr)
        KL = a.new("key_len", "in", I32, B).set(kl) if use_kl else None
        QKV, AV, LSE = a.new("qkv", "out", F32, (3 * T, D)), a.new("av", "out", F32, (T, D)), a.new("lse", "out", F32, B * n * L)
        AO, MU, RS, H1 = a.new("ao", "out", F32, (T, D)), a.new("mean", "out", F32, T), a.new("rstd", "out", F32, T), a.new("h1", "out", F32, (T, D))
        parr, _k = _lib().ptr_array([b.ptr for b in PB])
        call(a, "t4r_xlnet_layer_prepare", stream(), parr, D, PL.ptr)
        call(a, "t4r_xlnet_attn_block_fwd", stream(), H.ptr, PL.ptr, pb["o"].ptr, KR.ptr, 0, pb["r_w_bias"].ptr, pb["r_r_bias"].ptr,
             pb["ln_w"].ptr, pb["ln_b"].ptr, QKV.ptr, AV.ptr, LSE.ptr, AO.ptr, MU.ptr, RS.ptr, H1.ptr, B, L, D, n, eps, p, seed, c_prob,
             c_out, KL.ptr if use_kl else None)
        t = "test_attn_block_gpu.py::test_attn_block_forward_matches_fp64 (rel_err < 6e-6)"
        return [Out(QKV, R["qkv"], _rel(6e-6, R["qkv"]), t), Out(AV, R["av"], _rel(6e-6, R["av"]), t),
                Out(LSE, R["lse"], dict(rtol=0, atol=6e-6 * max(1.0, float(R["lse"].abs().max()))), t), Out(AO, R["ao"], _rel(6e-6, R["ao"]), t),
                Out(H1, R["h1"], _rel(6e-6, R["h1"]), t), Out(MU), Out(RS)]
    return fn


for _B, _L, _D, _n in _XL_SHAPES + ((4, 32, 32, 2),):
    if _lib().load().t4r_xlnet_attn_block_supported(_L, _D, _n):
        case("xlnet", f"attn_block-{_B}-{_L}-{_D}-{_n}-p0", ["t4r_xlnet_layer_prepare", "t4r_xlnet_attn_block_fwd"])(_attn_block(_B, _L, _D, _n, 0.0, False))
        case("xlnet", f"attn_block-{_B}-{_L}-{_D}-{_n}-p0.3-keylen", ["t4r_xlnet_layer_prepare", "t4r_xlnet_attn_block_fwd"])(
            _attn_block(_B, _L, _D, _n, 0.3, True))


# ================================================================================================================ runner
BY_ID = {c.id: c for c in CASES}


def _run(c, fill):
    a = Arena(fill, DEV, capacity=getattr(c, "capacity", 24 << 20))
    outs = c.fn(a, c.id)
    torch.cuda.synchronize()
    v = a.check()
    assert v is None, f"{c.id} under fill {fill:#04x}: {v}"
    return a, outs


def _values(outs):
    return [o.value().detach().clone() for o in outs]


def _bits_equal(x, y):
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]
    return torch.equal(x.contiguous().view(it), y.contiguous().view(it))


def _against(o, got, ref, what):
    if o.tol is None:
        assert torch.equal(got.cpu(), ref.to(got.dtype).reshape(got.shape).cpu()), f"{what}: '{o.buf.name}' not exact ({o.cite})"
    else:
        torch.testing.assert_close(got.double().cpu(), ref.double().reshape(got.shape).cpu(), **o.tol,
                                   msg=lambda m: f"{what}: '{o.buf.name}' ({o.cite}): {m}")


def _sibling(c):
    fam = [x for x in CASES if x.family == c.family and set(x.entries) & set(c.entries) and x.id != c.id]
    fam = fam or [x for x in CASES if x.family == c.family and x.id != c.id]
    i = [x.id for x in CASES].index(c.id)
    later = [x for x in fam if [y.id for y in CASES].index(x.id) > i]
    return (later or fam)[0]


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_redzone(cid):
    c = BY_ID[cid]
    # 1. fill 0x00
    a0, outs0 = _run(c, 0x00)
    v0 = _values(outs0)
    for o, got in zip(outs0, v0):
        if got.dtype.is_floating_point:
            assert bool(torch.isfinite(got).all()), f"{cid}: non-finite value in '{o.buf.name}' under fill 0x00"
        if o.ref is not None:
            _against(o, got, o.ref, f"{cid} fill 0x00")
    del a0
    # 2. fill 0xFF
    a1, outs1 = _run(c, 0xFF)
    for o, o0, got, first in zip(outs1, outs0, _values(outs1), v0):
        if got.dtype.is_floating_point:
            bad = (~torch.isfinite(got)).nonzero()
            assert bad.numel() == 0, (f"{cid}: non-finite value in '{o.buf.name}' at {tuple(int(i) for i in bad[0])} "
                                      "under fill 0xFF: something outside the entry's inputs was read")
        if o.atomic:
            if o0.ref is not None:
                _against(o0, got, o0.ref, f"{cid} fill 0xFF")
        else:
            assert _bits_equal(got, first), f"{cid}: '{o.buf.name}' differs between fill 0x00 and fill 0xFF"
    del a1
    # 3. another case of the family in between, then the same case again
    sib = _sibling(c)
    _run(sib, 0x00)
    a2, outs2 = _run(c, 0x00)
    for o, o0, got, first in zip(outs2, outs0, _values(outs2), v0):
        if o.atomic:
            if o0.ref is not None:
                _against(o0, got, o0.ref, f"{cid} rerun")
        else:
            assert _bits_equal(got, first), f"{cid}: '{o.buf.name}' changed after running {sib.id} in between"


def test_harness_sees_a_real_device_store():
    """t4r_mul with n = 9 into an `out` registered as 8 floats: the ninth float is the first 4 bytes of the trailing guard
    (byte 32 from the buffer's start), inside the arena -- nothing faults, check() must name it"""
    for fill in (0x00, 0xFF):
        a = Arena(fill, DEV, capacity=1 << 20)
        x = a.new("a", "in", F32, 9).set(torch.full((9,), 1.2345))      # 0x3F9E0419: no byte equals either fill
        y = a.new("b", "in", F32, 9).set(torch.full((9,), 1.0))
        o = a.new("out", "out", F32, 8)
        call(a, "t4r_mul", stream(), x.ptr, y.ptr, o.ptr, 9)
        torch.cuda.synchronize()
        v = a.check()
        assert v is not None and v.buffer == "out" and v.region == "trailing guard", v
        assert v.offset == 0 and v.payload_offset == 32, v
        assert torch.equal(o.win.cpu(), torch.full((8,), 1.2345))
