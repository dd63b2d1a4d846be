"""t4r_gemm_wgrad_f32 (include/t4r_hip.h): the deterministic split-K weight gradient as ONE call -- the sink of the partial tiles
lives on that call's stack, so nothing is armed before it and nothing stays armed after it.  Its red-zone cases (workspace
sized by the query, one split too small, null) are in test_abi_redzone_gpu.py; here: values, bits, the warning of
ops.gemm_wgrad, and that neither a failed nor a successful call changes what the NEXT call on the thread does.

Shapes: M 64, N 48; K 700 is 44 k-tiles of 16 and the launcher's rule (at least 20 per split) gives 2 splits, K 304 is 19
k-tiles and one split.  Tolerances: rtol 1e-4 / atol 2e-3 as test_kernels_gpu.py::test_gemm_epilogues_splitk_accumulate, and
test_add_layernorm_fwd_bwd's atol 1e-4 for d gamma / d beta."""
import ctypes
import warnings

import pytest
import torch

import t4r_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
M, N = 64, 48
TOL = dict(rtol=1e-4, atol=2e-3)


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def operands():
    """K -> (A [K, M], B [K, N] on the device, fp64 A^T B on the host): made once, never written"""
    out = {}
    for K in (700, 304):
        g = torch.Generator().manual_seed(K)
        A, B = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
        out[K] = (A.to(DEV), B.to(DEV), A.double().t() @ B.double())
    return out


def close(a, b, **tol):
    torch.testing.assert_close(a.double().cpu(), b, **tol)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _wgrad(A, B, C, ws, ws_floats):
    """the entry itself -> (rc, *bypassed)"""
    from transformers4rec_amd import _lib

    K = B.shape[0]
    bypassed = ctypes.c_int(-1)
    rc = _lib.load().t4r_gemm_wgrad_f32(_stream(), M, N, K, None if A is None else A.data_ptr(), M, B.data_ptr(), N, C.data_ptr(),
                                        None if ws is None else ws.data_ptr(), ws_floats, ctypes.addressof(bypassed))
    return rc, bypassed.value


def test_gemm_wgrad_is_right_and_bit_reproducible(ops, operands):
    from transformers4rec_amd import _lib

    A, B, ref = operands[700]
    assert _lib.load().t4r_gemm_wgrad_ws_floats(M, N, 700) == M * N * 3      # the launcher's bound K / 320 + 1; it uses 2
    outs = []
    with ops.precision("fp32"), warnings.catch_warnings():
        warnings.simplefilter("error")
        for _ in range(2):
            outs.append(ops.gemm_wgrad(A, B, torch.ones(M, N, device=DEV)))
    torch.cuda.synchronize()
    close(outs[0], ref + 1, **TOL)
    assert torch.equal(outs[0], outs[1])


def test_gemm_wgrad_without_room_says_so(ops, operands, monkeypatch):
    A, B, ref = operands[700]
    with ops.precision("fp32"):
        C = torch.ones(M, N, device=DEV)
        rc, bypassed = _wgrad(A, B, C, torch.empty(M * N, device=DEV), M * N)
        assert rc == 0 and bypassed == 1
        close(C, ref + 1, **TOL)
        monkeypatch.setattr(ops, "_gemm_wgrad_ws_floats", lambda m, n, k: m * n)
        with pytest.warns(RuntimeWarning, match="not bit-reproducible"):
            C2 = ops.gemm_wgrad(A, B, torch.ones(M, N, device=DEV))
        close(C2, ref + 1, **TOL)


@pytest.mark.parametrize("null_ws", [False, True])
def test_gemm_wgrad_one_split(ops, operands, null_ws):
    from transformers4rec_amd import _lib

    A, B, ref = operands[304]
    floats = _lib.load().t4r_gemm_wgrad_ws_floats(M, N, 304)
    assert floats == M * N
    with ops.precision("fp32"):
        C = torch.ones(M, N, device=DEV)
        rc, bypassed = _wgrad(A, B, C, None if null_ws else torch.empty(floats, device=DEV), 0 if null_ws else floats)
    assert rc == 0 and bypassed == 0
    close(C, ref + 1, **TOL)


def test_nothing_stays_armed(ops, operands):
    """after a call that fails its argument check, and after one that succeeds, the next launches of the thread are their own:
    an accumulating split-K product holds its complete sum after a sync (nothing was parked for a flush that never comes), and
    so do the d gamma / d beta of a LayerNorm backward (their second stage ran, on this stream)"""
    A, B, ref = operands[700]
    with ops.precision("fp32"):
        C = torch.ones(M, N, device=DEV)
        ws = torch.empty(M * N * 3, device=DEV)
        rc, _ = _wgrad(None, B, C, ws, ws.numel())
        assert rc != 0
        ops.gemm(A, B, True, False, splitk=-1, accumulate=True, out=C)
        torch.cuda.synchronize()
        close(C, ref + 1, **TOL)

        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ops.gemm_wgrad(A, B, torch.ones(M, N, device=DEV))
    rows, D = 32, 64
    g = torch.Generator().manual_seed(rows + D)
    a, b, dy = (torch.randn(rows, D, generator=g) for _ in range(3))
    gam, bet = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    g_, be_ = gam.double().requires_grad_(), bet.double().requires_grad_()
    O.layer_norm(a.double() + b.double(), g_, be_, 0.03).backward(dy.double())
    cu = lambda t: t.to(DEV)
    _, mean, rstd = ops.add_layernorm_fwd(cu(a), cu(b), cu(gam), cu(bet), 0.03)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    ops.add_layernorm_bwd(cu(a), cu(b), cu(gam), mean, rstd, cu(dy), dg, db)
    torch.cuda.synchronize()
    close(dg, g_.grad, rtol=2e-5, atol=1e-4)
    close(db, be_.grad, rtol=2e-5, atol=1e-4)
