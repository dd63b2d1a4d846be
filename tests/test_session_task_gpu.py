"""The session-level tasks on the GPU: the kernels (csrc/seq_task.hip, include/t4r_hip_seqtask.h) against float64
(tests/session_task_restatement.py) under derived bounds, saturated rows, the output contract, bit-reproducibility and red zones
around every buffer; the registered operators against the ctypes calls; the task modules; the reference's fixtures
(tests/golden/session_tasks_*.npz, tools/make_session_task_golden.py) replayed through Model; and the gradient plumbing of a
multi-task model (autograd-visible gradients, the fused optimizer).

Where the figures go: every numeric test prints the largest observed error / bound ratio; with T4R_RATIO_LOG set to a path the
maxima over the run are also written there as JSON (DESIGN.md 4.11 quotes them)."""
import atexit
import json
import os

import pytest
import torch

import golden_utils as gu
import session_task_restatement as R
import transformers4rec_amd as tr
from abi_arena import FILLS, Arena
from transformers4rec_amd import _lib, ops, torch_ops  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, I32 = torch.float32, torch.int32
U = R.U
CLICK, DWELL = "click/binary_classification_task", "dwell/regression_task"
TD = "heads.0.prediction_task_dict."
PAIRS = ((1, R.BCE), (0, R.MSE))            # (act, loss_kind): the binary task's and the regression task's

RATIOS = {}


def _note(what, ratio):
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))


@atexit.register
def _dump_ratios():
    path = os.environ.get("T4R_RATIO_LOG")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def raw_fwd(x, lengths, w, b, target, summary, act, loss_kind, s=None, pred=None, loss=None, ws=None):
    """the C entry itself, every buffer the caller's (pre-filled with NaN by default) -> (s, pred, loss, ws)"""
    B, L, D = x.shape
    nan = float("nan")
    s = torch.full((B, D), nan, device=DEV) if s is None else s
    pred = torch.full((B,), nan, device=DEV) if pred is None else pred
    loss = torch.full((1,), nan, device=DEV) if loss is None else loss
    ws = torch.full((max(1, _lib.load().t4r_seq_task_ws_floats(B, D)),), nan, device=DEV) if ws is None else ws
    _lib.call("t4r_seq_task_fwd", _stream(), _ptr(x), _ptr(lengths), B, L, D, summary, _ptr(w), _ptr(b), act, loss_kind, _ptr(target),
              _ptr(s), _ptr(pred), _ptr(loss), _ptr(ws))
    return s, pred, loss, ws


def raw_bwd(g, pred, target, s, lengths, L, w, summary, act, loss_kind, d_w=None, d_b=None, dx=None, ws=None):
    B, D = s.shape
    nan = float("nan")
    dx = torch.full((B, L, D), nan, device=DEV) if dx is None else dx
    ws = torch.full((max(1, _lib.load().t4r_seq_task_ws_floats(B, D)),), nan, device=DEV) if ws is None else ws
    _lib.call("t4r_seq_task_bwd", _stream(), _ptr(g), _ptr(pred), _ptr(target), _ptr(s), _ptr(lengths), B, L, D, summary, _ptr(w), act,
              loss_kind, _ptr(dx), _ptr(d_w), _ptr(d_b), _ptr(ws))
    return dx, ws


def _lengths(B, L, g):
    """0, 1, L and values above L (and a negative one) among the sessions"""
    lens = torch.randint(0, L + 3, (B,), generator=g, dtype=torch.int32)
    special = [0, 1, L, L + 2, -1]
    for i in range(min(B, len(special))):
        lens[(i * 7) % B if B > len(special) else i] = special[i]
    return lens


def _case(B, L, D):
    """x, w, bias, lengths, targets: w scaled so that |z| <= 8 under every summary, with and without lengths"""
    g = torch.Generator().manual_seed(B * 100000 + L * 1000 + D)
    x = torch.randn((B, L, D), generator=g)
    w = (torch.rand((D,), generator=g) * 2 - 1)
    bias = (torch.rand((1,), generator=g) * 2 - 1)
    lens = _lengths(B, L, g)
    zmax = max(float(R.logits(R.summary_of(x, m, ln), w).abs().max()) for m in (0, 1, 2) for ln in (None, lens))
    w = (w * (7.0 / max(zmax, 1e-30))).float() if zmax > 7.0 else w
    t_bin = torch.randint(0, 2, (B,), generator=g).float()
    t_reg = torch.randn((B,), generator=g)
    return dict(x=x, w=w, bias=bias, lens=lens, t={R.BCE: t_bin, R.MSE: t_reg})


def _check_case(k, B, L, D, x_dev, tag):
    """every summary x pair x bias x lengths of one shape against float64 under the derived bounds"""
    w_dev, b_dev, g_dev = k["w"].to(DEV), k["bias"].to(DEV), torch.tensor([0.75], device=DEV)
    for lens in (None, k["lens"]):
        lens_dev = None if lens is None else lens.to(DEV)
        for summary in (R.FIRST, R.LAST, R.MEAN):
            s64 = R.summary_of(k["x"], summary, lens)
            zb = R.z_bound(k["x"], k["w"], summary, lens)
            for act, kind in PAIRS:
                t = k["t"][kind]
                t_dev = t.to(DEV)
                for bias in (None, k["bias"]):
                    what = f"{tag} B={B} L={L} D={D} summary={summary} act={act} bias={bias is not None} len={lens is not None}"
                    s, pred, loss, ws = raw_fwd(x_dev, lens_dev, w_dev, None if bias is None else b_dev, t_dev, summary, act, kind)
                    rows = ws[:B].cpu()
                    s, pred, loss = s.cpu(), pred.cpu(), loss.cpu()
                    assert bool(torch.isfinite(s).all() and torch.isfinite(pred).all() and torch.isfinite(loss).all()), what
                    # s: one rounding per added position and one for the divide
                    es = (s.double() - s64).abs()
                    bs = (L + 2) * U * (R.coef(B, L, summary, lens)[:, :, None] * k["x"].double().abs()).sum(1)
                    assert bool((es <= bs).all()), what
                    if summary != R.MEAN:
                        assert torch.equal(s.double(), s64), what            # a copied row
                    # z / pred against float64 from the inputs
                    p64 = R.predictions(R.logits(s64, k["w"], bias), act)
                    bound = zb + 8 * U * p64.abs()
                    ep = (pred.double() - p64).abs()
                    _note("pred", (ep / bound.clamp_min(1e-300)).max())
                    assert bool((ep <= bound).all()), (what, float((ep / bound.clamp_min(1e-300)).max()))
                    # row losses and the mean against float64 from the kernel's own pred
                    r64 = R.row_losses(pred, t, kind)
                    er = (rows.double() - r64).abs()
                    _note("row loss", (er / (8 * U * r64.abs()).clamp_min(1e-300)).max() if bool((er > 0).any()) else 0.0)
                    assert bool((er <= 8 * U * r64.abs()).all()), what
                    el = abs(float(loss.double()) - float(r64.mean()))
                    bl = (8 + B) * U * float(r64.abs().mean())
                    _note("loss", el / max(bl, 1e-300))
                    assert el <= bl, what
                    # backward
                    d_w = torch.zeros(D, device=DEV)
                    d_b = torch.zeros(1, device=DEV)
                    dx, ws2 = raw_bwd(g_dev, pred.to(DEV), t_dev, s.to(DEV), lens_dev, L, w_dev, summary, act, kind, d_w, d_b)
                    dz = ws2[:B].cpu()
                    dx, d_w, d_b = dx.cpu(), d_w.cpu(), d_b.cpu()
                    assert bool(torch.isfinite(dx).all() and torch.isfinite(d_w).all() and torch.isfinite(d_b).all()), what
                    dz64 = R.dz_of(pred, t, 0.75, act, kind)
                    ez = (dz.double() - dz64).abs()
                    _note("dz", (ez / (8 * U * dz64.abs()).clamp_min(1e-300)).max() if bool((ez > 0).any()) else 0.0)
                    assert bool((ez <= 8 * U * dz64.abs()).all()), what
                    dx64, dw64, db64 = R.backward(dz, s, k["w"], L, summary, lens)
                    ex = (dx.double() - dx64).abs()
                    _note("dx", (ex / ((B + 4) * U * dx64.abs()).clamp_min(1e-300)).max() if bool((ex > 0).any()) else 0.0)
                    assert bool((ex <= (B + 4) * U * dx64.abs()).all()), what        # zero outside the summary's positions, exactly
                    bw = (B + 4) * U * (dz.double().abs()[:, None] * s.double().abs()).sum(0)
                    ew = (d_w.double() - dw64).abs()
                    _note("d_w", (ew / bw.clamp_min(1e-300)).max() if bool((ew > 0).any()) else 0.0)
                    assert bool((ew <= bw).all()), what
                    bb = (B + 4) * U * float(dz.double().abs().sum())
                    eb = abs(float(d_b.double()) - float(db64))
                    _note("d_b", eb / max(bb, 1e-300))
                    assert eb <= bb, what


@pytest.mark.parametrize("D", [1, 6, 64, 100, 130, 1024])
@pytest.mark.parametrize("L", [1, 2, 7, 33])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_kernels_against_float64(B, L, D):
    k = _case(B, L, D)
    _check_case(k, B, L, D, k["x"].to(DEV), "aligned")
    print(f"B={B} L={L} D={D}: largest error / bound so far {json.dumps({n: round(v, 3) for n, v in RATIOS.items()})}")


@pytest.mark.parametrize("B,L", [(3, 7), (65, 33)])
def test_scalar_path_at_a_base_address_off_by_four_bytes(B, L):
    """D = 64 with x four bytes off a 16-byte boundary: the 4-byte path runs; the same bounds, and the bits of the 16-byte path"""
    D = 64
    k = _case(B, L, D)
    flat = torch.zeros(B * L * D + 1, device=DEV)
    x_off = flat[1:].view(B, L, D)
    x_off.copy_(k["x"])
    assert x_off.data_ptr() % 16 == 4 and x_off.is_contiguous()
    _check_case(k, B, L, D, x_off, "offset")
    x_al, w, t = k["x"].to(DEV), k["w"].to(DEV), k["t"][R.BCE].to(DEV)
    for summary in (0, 1, 2):
        a = raw_fwd(x_al, None, w, None, t, summary, 1, R.BCE)
        b = raw_fwd(x_off, None, w, None, t, summary, 1, R.BCE)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_saturated_rows():
    """z = +-40 and +-200 against targets 0 and 1.  fp32 sigmoid is exactly 1 at +40 and +200 and exactly 0 at -200: the row loss
    is exactly 0 or 100 (the -100 clamp) and dz exactly 0.  At z = -40 the fp32 sigmoid is 4.2e-18, not 0 -- in torch as well --,
    so that row follows the formulas at that value: checked against float64 from the kernel's own pred, tiny and finite."""
    zs = torch.tensor([40.0, 40.0, 200.0, 200.0, -200.0, -200.0, -40.0, -40.0])
    t = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0])
    x = torch.zeros(8, 1, 2)
    x[:, 0, 0] = zs
    w = torch.tensor([1.0, 0.0])
    s, pred, loss, ws = raw_fwd(x.to(DEV), None, w.to(DEV), None, t.to(DEV), R.FIRST, 1, R.BCE)
    rows, pred = ws[:8].cpu(), pred.cpu()
    assert pred[:6].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert rows[:6].tolist() == [0.0, 100.0, 0.0, 100.0, 100.0, 0.0]
    assert 0.0 < float(pred[6]) < 1e-17 and float(pred[6]) == float(pred[7])
    assert abs(float(pred[6]) - float(torch.sigmoid(torch.tensor(-40.0, dtype=torch.float64)))) <= 8 * U * float(pred[6])
    r64 = R.row_losses(pred[6:], t[6:], R.BCE)
    assert bool(((rows[6:].double() - r64).abs() <= 8 * U * r64.abs()).all()) and 39.9 < float(rows[6]) < 40.1 and float(rows[7]) < 1e-17
    d_w, d_b = torch.zeros(2, device=DEV), torch.zeros(1, device=DEV)
    dx, ws2 = raw_bwd(torch.ones(1, device=DEV), pred.to(DEV), t.to(DEV), s, None, 1, w.to(DEV), R.FIRST, 1, R.BCE, d_w, d_b)
    dz = ws2[:8].cpu()
    assert dz[:6].tolist() == [0.0] * 6 and float(dx[:6].abs().max()) == 0.0
    dz64 = R.dz_of(pred, t, 1.0, 1, R.BCE)[6:]
    assert bool(((dz[6:].double() - dz64).abs() <= 8 * U * dz64.abs()).all()) and float(dz[6:].abs().max()) < 1e-5
    for v in (s, pred, loss, rows, dx, dz, d_w, d_b):
        assert bool(torch.isfinite(v).all())


def test_contract_full_writes_accumulation_nulls_and_reruns():
    B, L, D = 65, 7, 100
    k = _case(B, L, D)
    x, w, b, lens = k["x"].to(DEV), k["w"].to(DEV), k["bias"].to(DEV), k["lens"].to(DEV)
    g = torch.tensor([1.5], device=DEV)
    for (act, kind), summary in zip(PAIRS + PAIRS[:1], (0, 1, 2)):
        t = k["t"][kind].to(DEV)
        s, pred, loss, ws = raw_fwd(x, lens, w, b, t, summary, act, kind)              # NaN pre-fills
        assert bool(torch.isfinite(s).all() and torch.isfinite(pred).all() and torch.isfinite(loss).all())
        s2, pred2, loss2, _ = raw_fwd(x, lens, w, b, t, summary, act, kind)
        assert torch.equal(s, s2) and torch.equal(pred, pred2) and torch.equal(loss, loss2)     # two runs: the same bits
        # inference: target NULL, loss and ws NULL -- s and pred as with a target, loss untouched
        s3, pred3 = torch.full_like(s, float("nan")), torch.full_like(pred, float("nan"))
        _lib.call("t4r_seq_task_fwd", _stream(), x.data_ptr(), lens.data_ptr(), B, L, D, summary, w.data_ptr(), b.data_ptr(), act, kind,
                  None, s3.data_ptr(), pred3.data_ptr(), None, None)
        assert torch.equal(s3, s) and torch.equal(pred3, pred)
        keep = torch.tensor([-7.0], device=DEV)
        raw_fwd(x, lens, w, None, None, summary, act, kind, loss=keep)
        assert float(keep) == -7.0
        # backward: NaN-filled dx fully written; d_w / d_b accumulate; NULLs accepted; reruns equal
        d_w0, d_b0 = torch.zeros(D, device=DEV), torch.zeros(1, device=DEV)
        dx, _ = raw_bwd(g, pred, t, s, lens, L, w, summary, act, kind, d_w0, d_b0)
        assert bool(torch.isfinite(dx).all())
        pre_w = torch.arange(D, device=DEV, dtype=F32) * 0.125 - 3.0
        pre_b = torch.tensor([0.625], device=DEV)
        d_w1, d_b1 = pre_w.clone(), pre_b.clone()
        dx1, _ = raw_bwd(g, pred, t, s, lens, L, w, summary, act, kind, d_w1, d_b1)
        assert torch.equal(dx1, dx) and torch.equal(d_w1, pre_w + d_w0) and torch.equal(d_b1, pre_b + d_b0)
        d_w2 = torch.zeros(D, device=DEV)
        dx2, _ = raw_bwd(g, pred, t, s, lens, L, w, summary, act, kind, d_w2, None)
        d_b3 = torch.zeros(1, device=DEV)
        dx3, _ = raw_bwd(g, pred, t, s, lens, L, w, summary, act, kind, None, d_b3)
        dx4, _ = raw_bwd(g, pred, t, s, lens, L, w, summary, act, kind, None, None)
        assert torch.equal(dx2, dx) and torch.equal(dx3, dx) and torch.equal(dx4, dx)
        assert torch.equal(d_w2, d_w0) and torch.equal(d_b3, d_b0)
        # sessions without items: summary 0, no gradient into x
        empty = (k["lens"] <= 0).to(DEV)
        assert bool(empty.any()) and float(s[empty].abs().max()) == 0.0 and float(dx[empty].abs().max()) == 0.0
    # B = 0: returns 0, nothing is written
    z = torch.zeros(0, L, D, device=DEV)
    keep = torch.tensor([-7.0], device=DEV)
    s, pred, loss, ws = raw_fwd(z, None, w, b, torch.zeros(0, device=DEV), 2, 1, R.BCE, loss=keep, ws=torch.full((4,), 5.0, device=DEV))
    assert float(keep) == -7.0 and ws.tolist() == [5.0] * 4
    d_w = torch.full((D,), 2.0, device=DEV)
    raw_bwd(g, pred, torch.zeros(0, device=DEV), s, None, L, w, 2, 1, R.BCE, d_w, None, ws=ws)
    assert float(d_w.min()) == 2.0 == float(d_w.max()) and ws.tolist() == [5.0] * 4


@pytest.mark.parametrize("L,D", [(7, 100), (33, 130), (2, 64)])
def test_a_session_gives_the_same_bits_alone_and_inside_a_batch(L, D):
    """row 40 of B = 65 against the same session as B = 1.  dx depends on B through the one factor g / B, formed first: the lone
    run takes g = fl(1 / 65) where the batch takes g = 1"""
    B = 65
    k = _case(B, L, D)
    x, w, b, lens = k["x"].to(DEV), k["w"].to(DEV), k["bias"].to(DEV), k["lens"].to(DEV)
    lens[40] = max(1, L - 1)
    one, g_one = torch.ones(1, device=DEV), torch.tensor([1.0], device=DEV) / torch.tensor([65.0], device=DEV)
    for (act, kind), summary in ((a, m) for a in PAIRS for m in (0, 1, 2)):
        t = k["t"][kind].to(DEV)
        s, pred, _, _ = raw_fwd(x, lens, w, b, t, summary, act, kind)
        dx, _ = raw_bwd(one, pred, t, s, lens, L, w, summary, act, kind)
        s1, pred1, _, _ = raw_fwd(x[40:41].contiguous(), lens[40:41].contiguous(), w, b, t[40:41].contiguous(), summary, act, kind)
        dx1, _ = raw_bwd(g_one, pred1, t[40:41].contiguous(), s1, lens[40:41].contiguous(), L, w, summary, act, kind)
        assert torch.equal(s1[0], s[40]) and torch.equal(pred1[0], pred[40]) and torch.equal(dx1[0], dx[40]), (summary, act)
        assert float(dx[40].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ red zones
@pytest.mark.parametrize("fill", FILLS, ids=["zeros", "ones"])
@pytest.mark.parametrize("B,L,D", [(3, 7, 6), (65, 33, 130)])
def test_red_zones_around_every_buffer(fill, B, L, D):
    lib = _lib.load()
    k = _case(B, L, D)
    for (act, kind), summary in zip(PAIRS + PAIRS[:1], (2, 1, 0)):
        a = Arena(fill, DEV, capacity=16 << 20)
        xb = a.new("x", "in", F32, B * L * D).set(k["x"])
        lb = a.new("len", "in", I32, B).set(k["lens"])
        wb = a.new("w", "in", F32, D).set(k["w"])
        bb = a.new("b", "in", F32, 1).set(k["bias"])
        tb = a.new("target", "in", F32, B).set(k["t"][kind])
        sb = a.new("s", "out", F32, B * D)
        pb = a.new("pred", "out", F32, B)
        lo = a.new("loss", "out", F32, 1)
        ws = a.ws("ws", 4 * lib.t4r_seq_task_ws_floats(B, D))
        a.seal()
        for _ in range(2):          # and a rerun over its own outputs
            rc = lib.t4r_seq_task_fwd(_stream(), xb.ptr, lb.ptr, B, L, D, summary, wb.ptr, bb.ptr, act, kind, tb.ptr, sb.ptr, pb.ptr,
                                      lo.ptr, ws.ptr)
            assert rc == 0, lib.t4r_last_error()
            torch.cuda.synchronize()
            v = a.check()
            assert v is None, str(v)
            assert a.nonfinite() is None
        want = ops.seq_task_fwd(k["x"].to(DEV), k["lens"].to(DEV), k["w"].to(DEV), k["bias"].to(DEV), k["t"][kind].to(DEV), summary,
                                act, kind)
        assert torch.equal(sb.t.view(B, D), want[0]) and torch.equal(pb.t, want[1]) and torch.equal(lo.t, want[2])
        gb = a.new("g", "in", F32, 1).set(1.25)
        dxb = a.new("dx", "out", F32, B * L * D)
        dwb = a.new("d_w", "inout", F32, D).set(0.5)
        dbb = a.new("d_b", "inout", F32, 1).set(-0.25)
        ws2 = a.ws("ws2", 4 * lib.t4r_seq_task_ws_floats(B, D))
        a.seal()
        fwd_bits = (sb.bits(), pb.bits(), lo.bits())
        rc = lib.t4r_seq_task_bwd(_stream(), gb.ptr, pb.ptr, tb.ptr, sb.ptr, lb.ptr, B, L, D, summary, wb.ptr, act, kind, dxb.ptr,
                                  dwb.ptr, dbb.ptr, ws2.ptr)
        assert rc == 0, lib.t4r_last_error()
        torch.cuda.synchronize()
        v = a.check()
        assert v is None, str(v)
        assert a.nonfinite() is None
        assert all(torch.equal(x, y) for x, y in zip(fwd_bits, (sb.bits(), pb.bits(), lo.bits())))
        d_w, d_b = torch.full((D,), 0.5, device=DEV), torch.full((1,), -0.25, device=DEV)
        dx = ops.seq_task_bwd_(torch.tensor([1.25], device=DEV), want[1], k["t"][kind].to(DEV), want[0], k["lens"].to(DEV), L,
                               k["w"].to(DEV), summary, act, kind, d_w, d_b)
        assert torch.equal(dxb.t.view(B, L, D), dx) and torch.equal(dwb.t, d_w) and torch.equal(dbb.t, d_b)


# ------------------------------------------------------------------------------------------------ operators
def test_operators_give_the_bits_of_the_ctypes_calls():
    B, L, D = 65, 7, 100
    k = _case(B, L, D)
    x, w, b, lens = k["x"].to(DEV), k["w"].to(DEV), k["bias"].to(DEV), k["lens"].to(DEV)
    g = torch.tensor([0.5], device=DEV)
    for (act, kind), summary, bias in ((PAIRS[0], 2, None), (PAIRS[1], 1, b), (PAIRS[0], 0, None)):
        t = k["t"][kind].to(DEV)
        s, pred, loss, _ = raw_fwd(x, lens, w, bias, t, summary, act, kind)
        so, po, lo = torch.ops.t4r_hip.seq_task_fwd(x, lens, w.view(1, D), bias, t, summary, act, kind)
        assert torch.equal(so, s) and torch.equal(po, pred) and torch.equal(lo, loss)
        si, pi, li = torch.ops.t4r_hip.seq_task_fwd(x, lens, w, bias, None, summary, act, kind)
        assert torch.equal(si, s) and torch.equal(pi, pred) and li.shape == (0,)
        d_w, d_b = torch.zeros(D, device=DEV), torch.zeros(1, device=DEV)
        dx, _ = raw_bwd(g, pred, t, s, lens, L, w, summary, act, kind, d_w, d_b if bias is not None else None)
        dxo, dwo, dbo = torch.ops.t4r_hip.seq_task_bwd(g, pred, t, s, lens, L, w.view(1, D), bias is not None, summary, act, kind)
        assert torch.equal(dxo, dx) and torch.equal(dwo.view(-1), d_w) and dwo.shape == (1, D)
        assert torch.equal(dbo, d_b) if bias is not None else dbo.shape == (0,)
    with pytest.raises(_lib.T4RHipError):
        ops.seq_task_fwd(x.cpu(), None, w.cpu(), None, None, 0, 1, 1)


# ------------------------------------------------------------------------------------------------ modules
def _features(L=6, V=50, D=64, masking=None):
    return tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking=masking, aggregation="concat",
                                                  embedding_dims={"item_id": D})


@pytest.mark.parametrize("cls,summary", [(tr.BinaryClassificationTask, "mean"), (tr.BinaryClassificationTask, "cls_index"),
                                         (tr.RegressionTask, "last"), (tr.RegressionTask, "first")])
def test_task_forward_and_backward_equal_the_restatement(cls, summary):
    B, L, D = 9, 7, 100
    torch.manual_seed(5)
    task = cls("y", summary_type=summary).build(body=None, input_size=(-1, L, D)).to(DEV)
    act, kind = (1, R.BCE) if cls is tr.BinaryClassificationTask else (0, R.MSE)
    mode = {"cls_index": 1}.get(summary, ops.SUMMARY.get(summary))
    g = torch.Generator().manual_seed(6)
    x = torch.randn((B, L, D), generator=g)
    t = torch.randint(0, 2, (B,), generator=g).float() if kind == R.BCE else torch.randn((B,), generator=g)
    lin = task.pre[0]
    w, b = lin.weight.detach().cpu().view(-1), None if lin.bias is None else lin.bias.detach().cpu()
    xd = x.to(DEV).requires_grad_(True)
    out = task(xd, targets=t.to(DEV), training=True)
    assert set(out) == {"loss", "labels", "predictions"} and out["loss"].shape == () and out["predictions"].shape == (B,)
    assert torch.equal(out["labels"].cpu(), t)
    r = R.forward(x, w, b, t, mode, act, kind)
    pred = out["predictions"].detach().cpu()
    assert bool(((pred.double() - r["pred"]).abs() <= R.z_bound(x, w, mode) + 8 * U * r["pred"].abs()).all())
    r64 = R.row_losses(pred, t, kind)
    assert abs(float(out["loss"].detach()) - float(r64.mean())) <= (8 + B) * U * float(r64.abs().mean())
    (out["loss"] * 2.0).backward()
    dz64 = R.dz_of(pred, t, 2.0, act, kind)
    dx64, dw64, db64 = R.backward(dz64, R.summary_of(x, mode), w, L, mode)
    slack = (B + 12) * U
    assert bool(((xd.grad.cpu().double() - dx64).abs() <= slack * dx64.abs()).all())
    bw = slack * (dz64.abs()[:, None] * R.summary_of(x, mode).abs()).sum(0) + (L + 2) * U * dw64.abs()
    assert bool(((lin.weight.grad.cpu().view(-1).double() - dw64).abs() <= bw).all())
    if b is not None:
        assert abs(float(lin.bias.grad) - float(db64)) <= slack * float(dz64.abs().sum())
    # evaluation returns the same dict, inference the bare predictions: the same bits
    with torch.no_grad():
        ev = task(xd.detach(), targets=t.to(DEV), testing=True)
        inf = task(xd.detach())
    assert torch.equal(ev["predictions"], out["predictions"]) and torch.equal(inf, out["predictions"]) and torch.equal(ev["loss"], out["loss"])
    # a frozen weight keeps .grad untouched
    before = lin.weight.grad.clone()
    lin.weight.requires_grad_(False)
    xd2 = x.to(DEV).requires_grad_(True)
    task(xd2, targets=t.to(DEV), training=True)["loss"].backward()
    assert torch.equal(lin.weight.grad, before) and torch.equal(xd2.grad * 2.0, xd.grad)


def test_mask_padding_differs_exactly_on_the_padded_sessions():
    d = gu.load("session_tasks_train")
    ids = gu.t(d["in2/item_id"]).to(DEV)
    padded = (ids == 0).any(dim=1).cpu()
    assert bool(padded.any()) and not bool(padded.all()) and bool(padded[2])
    hidden = gu.t(d["out2/hidden"]).to(DEV)
    for cls, summary in ((tr.BinaryClassificationTask, "mean"), (tr.RegressionTask, "last")):
        preds = {}
        for mp in (False, True):
            feats = _features().to(DEV)
            torch.manual_seed(1)
            task = cls("y", summary_type=summary, mask_padding=mp).build(body=None, input_size=(-1, 6, 64), inputs=feats).to(DEV)
            feats({"item_id": ids}, training=False)          # the input module sees the batch: item_seq
            preds[mp] = task(hidden).cpu()
        diff = preds[True] != preds[False]
        assert torch.equal(diff, padded), (summary, diff, padded)
        lens = (ids != 0).sum(1).to(torch.int32).cpu()
        lin = task.pre[0]
        r = R.forward(hidden.cpu(), lin.weight.detach().cpu().view(-1), None if lin.bias is None else lin.bias.detach().cpu(), None,
                      ops.SUMMARY[summary], 1 if cls is tr.BinaryClassificationTask else 0, 0, lens)
        torch.testing.assert_close(preds[True].double(), r["pred"], rtol=1e-5, atol=1e-6)
    # first is the same either way
    a = tr.RegressionTask("y", mask_padding=True).build(body=None, input_size=(-1, 6, 64), inputs=feats).to(DEV)
    bsame = tr.RegressionTask("y").build(body=None, input_size=(-1, 6, 64)).to(DEV)
    bsame.load_state_dict(a.state_dict())
    assert torch.equal(a(hidden), bsame(hidden))


# ------------------------------------------------------------------------------------------------ fixtures
TOL = dict(rtol=1e-4, atol=5e-5)            # tests/test_e2e_gpu.py's bounds for the same quantities: the body dominates the error
GTOL = dict(rtol=2e-4, atol=1e-4)


def _close(a, b, **kw):
    torch.testing.assert_close(a.detach().cpu().float(), b.detach().cpu().float(), **kw)


def _fixture_model(d, multi):
    L, Vt, D = int(d["meta/L"]), int(d["meta/V"]), int(d["meta/d_model"])
    feats = _features(L, Vt - 1, D, masking="clm" if multi else None)
    cfg = tr.XLNetConfig.build(dropout=0.0, d_model=D, n_head=int(d["meta/n_head"]), n_layer=int(d["meta/n_layer"]), total_seq_length=L)
    if multi:
        tasks = [tr.NextItemPredictionTask(weight_tying=True), tr.BinaryClassificationTask("click", summary_type="first"),
                 tr.RegressionTask("dwell", summary_type="mean")]
        weights = None
    else:
        tasks = [tr.BinaryClassificationTask("click", summary_type="mean"), tr.RegressionTask("dwell", summary_type="last")]
        weights = [1.0, 0.5]
    model = cfg.to_torch_model(feats, *tasks, task_weights=weights)
    sd, own = gu.section(d, "p/"), model.state_dict()
    missing = [k for k in sd if k not in own]
    assert not missing, missing
    with torch.no_grad():
        for k, v in sd.items():
            assert own[k].shape == v.shape, k
            own[k].copy_(v)
    return model.to(DEV)


def _inputs(d, prefix="in/"):
    x = {k[len(prefix):]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith(prefix) and "/targets/" not in k}
    tg = {k[len(prefix + "targets/"):]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith(prefix + "targets/")}
    return x, tg


@pytest.mark.parametrize("name", ["session_tasks_train", "session_tasks_multi_train"])
def test_training_fixture_replayed_through_model(name):
    d = gu.load(name)
    multi = name == "session_tasks_multi_train"
    model = _fixture_model(d, multi)
    model.train()
    x, tg = _inputs(d)
    cap = {}
    model.transformer_block.register_forward_hook(lambda m, i, o: cap.__setitem__("hidden", o.detach().clone()))
    out = model(x, targets=tg, training=True)
    names = list(model.heads[0].prediction_task_dict.keys())
    assert list(out["predictions"].keys()) == names == list(out["labels"].keys())
    _close(cap["hidden"], gu.t(d["out/hidden"]), **TOL)
    _close(out["loss"], gu.t(d["out/loss"]), **TOL)
    for n in names:
        _close(out["predictions"][n], gu.t(d["out/predictions/" + n]), **(dict(rtol=1e-4, atol=2e-4) if n == "next-item" else TOL))
        assert torch.equal(out["labels"][n].cpu().to(torch.float64), gu.t(d["out/labels/" + n]).to(torch.float64))
    out["loss"].backward()
    g = gu.section(d, "g/")
    named = dict(model.named_parameters())
    assert sum("binary_classification_task" in k or "regression_task" in k for k in g) == 3
    for k, ref in g.items():
        assert named[k].grad is not None, k
        _close(named[k].grad, ref, **GTOL, msg=lambda m, k=k: f"{k}: {m}")
    # the step's loss is the reduction of the weighted task losses, one task at a time over the same body output
    tasks = model.heads[0].prediction_task_dict
    with torch.no_grad():
        one = []
        for n, task in tasks.items():
            o = task(cap["hidden"], targets=None if n == "next-item" else tg[task.target_name], training=True)
            _close(o["loss"], gu.t(d["out/loss/" + n]), **TOL)
            one.append(o["loss"].reshape(()) * model.heads[0].task_weight(n))
    _close(torch.stack(one).mean(), out["loss"], rtol=1e-6, atol=1e-7)
    if not multi:
        # the second batch: row 2 one item short.  Without mask_padding the reference's numbers; with it, only row 2 moves
        x2, _ = _inputs(d, "in2/")
        with torch.no_grad():
            o2 = model(x2, targets=tg, training=True)
        for n in names:
            _close(o2["predictions"][n], gu.t(d["out2/predictions/" + n]), **TOL)
        return
    # the next-item predictions equal those of the same weights as a single-task model: the body is unchanged
    feats = _features(int(d["meta/L"]), int(d["meta/V"]) - 1, int(d["meta/d_model"]), masking="clm")
    cfg = tr.XLNetConfig.build(dropout=0.0, d_model=int(d["meta/d_model"]), n_head=int(d["meta/n_head"]), n_layer=1, total_seq_length=int(d["meta/L"]))
    single = cfg.to_torch_model(feats, tr.NextItemPredictionTask(weight_tying=True))
    own = single.state_dict()
    with torch.no_grad():
        for k, v in gu.section(d, "p/").items():
            if k in own:
                own[k].copy_(v)
    single = single.to(DEV).train()
    so = single(x, training=True)
    assert torch.equal(so["labels"], out["labels"]["next-item"])
    _close(so["predictions"], out["predictions"]["next-item"], rtol=1e-5, atol=1e-6)
    _close(so["loss"], gu.t(d["out/loss/next-item"]), **TOL)


def test_inference_fixture_replayed_through_model():
    d = gu.load("session_tasks_infer")
    model = _fixture_model(d, False).eval()
    x, _ = _inputs(d)
    with torch.no_grad():
        out = model(x)
    assert list(out.keys()) == [CLICK, DWELL]
    for n in out:
        assert out[n].shape == (8,)
        _close(out[n], gu.t(d["out/predictions/" + n]), **TOL)
    # metrics over all tasks
    tg = {CLICK: torch.ones(8, device=DEV), DWELL: torch.zeros(8, device=DEV)}
    got = model.calculate_metrics(out, tg)
    assert set(got) == {CLICK + "/precision", CLICK + "/recall", CLICK + "/accuracy", DWELL + "/mean_squared_error"}
    assert abs(float(got[DWELL + "/mean_squared_error"]) - float((out[DWELL].double() ** 2).mean())) < 1e-6
    assert abs(float(model.compute_metrics()[CLICK + "/recall"]) - float((out[CLICK] >= 0.5).float().mean())) < 1e-6
    model.reset_metrics()


# ------------------------------------------------------------------------------------------------ gradient plumbing
def test_autograd_visible_gradients_equal_the_fast_path():
    d = gu.load("session_tasks_multi_train")
    x, tg = _inputs(d)
    grads = {}
    for visible in (False, True):
        model = _fixture_model(d, True).train()
        if visible:
            tr.enable_autograd_gradients(model)
        model(x, targets=tg, training=True)["loss"].backward()
        grads[visible] = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    # the carrier hands every parameter a buffer: those the path never touches (XLNet's unused ones) come back as zeros
    assert set(grads[False]) <= set(grads[True]) and sum("_task.pre.0" in k for k in grads[False]) == 3
    assert all(float(grads[True][k].abs().max()) == 0.0 for k in set(grads[True]) - set(grads[False]))
    for k in grads[False]:
        if "_task.pre.0" in k:
            assert torch.equal(grads[True][k], grads[False][k]), k
        else:
            _close(grads[True][k], grads[False][k], rtol=1e-5, atol=1e-7, msg=lambda m, k=k: f"{k}: {m}")


def test_fused_adam_steps_the_session_tasks_parameters():
    d = gu.load("session_tasks_train")
    model = _fixture_model(d, False).train()
    x, tg = _inputs(d)
    dense, tables = tr.flatten_model(model)
    opt = tr.FusedAdam([b for b in (dense, tables) if b is not None], lr=1e-2)
    named = dict(model.named_parameters())
    keys = [TD + CLICK + ".pre.0.weight", TD + DWELL + ".pre.0.weight", TD + DWELL + ".pre.0.bias"]
    before = {k: named[k].detach().clone() for k in keys}
    model(x, targets=tg, training=True)["loss"].backward()
    opt.step()
    torch.cuda.synchronize()
    for k in keys:
        moved = (named[k].detach() - before[k]).abs()
        assert float(moved.max()) > 1e-3 and bool(torch.isfinite(named[k]).all()), k      # Adam's first step: lr per element
