"""GRU body on the GPU: the kernels (csrc/gru.hip, include/t4r_hip_gru.h) against float64 (tests/gru_restatement.py) under its
per-element bounds, the forward step by step from the device's own h_{t-1} of every layer (a lower layer's h is the output of the
same call with fewer layers: the same kernels on the same arguments), the backward with the bounds carried along the dh chain;
saturated gates; inference = training bits, row independence, the scalar path of unaligned operands, determinism and
accumulation, NULL outputs and B = 0, red zones around every buffer with exact workspaces; the registered operators; and the
block inside a Model: one training step against the reference's fixtures (tests/golden/gru_body_*_train.npz,
tools/make_gru_golden.py) at the tolerances tests/test_mlp_block_gpu.py uses for its fixtures, the restated block in training,
evaluation and inference, the fused optimizer, the replay of the masks.

Every numeric test prints the largest observed error / bound ratio; with T4R_RATIO_LOG set to a path the maxima over the run are
also written there as text: profiles/gru_margins.txt is that file."""
import atexit
import os

import numpy as np
import pytest
import torch

import gru_restatement as R
import transformers4rec_amd as tr
from abi_arena import FILLS, Arena
from transformers4rec_amd import _lib, ops, torch_ops  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
SEED, OFFSET = 0x5EED1234ABCD, 3
# (B, L, K0, H, n, bias, p, h0 given, forward only): the hazard each reaches is named in test_entries_against_float64
SHAPES = [(1, 1, 8, 8, 1, True, 0.0, False, False), (3, 2, 5, 12, 1, False, 0.0, False, False), (17, 20, 65, 33, 1, True, 0.0, False, False),
          (33, 21, 48, 64, 2, True, 0.3, False, False), (65, 20, 128, 128, 1, True, 0.0, True, False),
          (5, 100, 24, 100, 3, True, 0.1, False, False), (2, 1023, 16, 16, 1, True, 0.0, False, True)]
NAMES = ("W_ih", "W_hh", "b_ih", "b_hh")
RATIOS = {}


def _note(what, ratio):
    RATIOS[what] = max(RATIOS.get(what, 0.0), float(ratio))


MARGINS_HEAD = """GRU body (csrc/gru.hip): worst error / bound per quantity on an MI355X
Written by tests/test_gru_gpu.py:  T4R_RATIO_LOG=profiles/gru_margins.txt pytest -m gpu tests/test_gru_gpu.py
Kernel level (h<k>/, dx/, W_ih<k>/, W_hh<k>/, b_ih<k>/, b_hh<k>/ by shape B x L x K0 x H x n): the bounds of tests/gru_restatement.py;
every layer's h step by step against the restatement of the device's own h_{t-1}, the gradients with the bounds carried along dh.
saturated/: inputs scaled until the pre-activations pass +-30.
model/: the Model with the block against the restated block of its own input, same bounds.
fixture/<name>/<quantity>: the Model with the block against the reference's training step (tests/golden/gru_body_*_train.npz),
|got - want| / (atol + rtol |want|) with the tolerances tests/test_mlp_block_gpu.py applies to its fixtures.
A ratio of 0 is bit equality.
"""


@atexit.register
def _dump_ratios():
    path = os.environ.get("T4R_RATIO_LOG")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write(MARGINS_HEAD + "\n")
            for k in sorted(RATIOS):
                f.write(f"{k:<60s} {RATIOS[k]:.4f}\n")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tag(s):
    return "x".join(str(v) for v in s[:5]) + ("" if s[5] else "/nob") + (f"/p{s[6]}" if s[6] else "") + ("/h0" if s[7] else "")


def _dev(k):
    mv = lambda v: None if v is None else v.to(DEV)      # noqa: E731
    out = {}
    for n, v in k.items():
        if isinstance(v, dict):
            out[n] = {a: (None if b is None else [mv(t) for t in b]) for a, b in v.items()}
        else:
            out[n] = [mv(t) for t in v] if isinstance(v, list) else mv(v)
    return out


def _device_h(d, n, drop):
    """the device's own h of every layer: layer k's is the output of the same call with k + 1 layers -> host list"""
    hs = []
    for k in range(n):
        cut = lambda lst: None if lst is None else lst[:k + 1]  # noqa: E731
        h0 = None if d["h0"] is None else d["h0"][:k + 1].contiguous()
        hs.append(ops.gru_fwd(d["x"], d["W_ih"][:k + 1], d["W_hh"][:k + 1], cut(d["b_ih"]), cut(d["b_hh"]), h0, drop).cpu())
    return hs


def _run(k, n, p, accumulate=False, want_dx=True, backward=True):
    """training forward and backward of one case through ops -> (out, dict dx, W_ih, ...), host tensors"""
    d = _dev(k)
    drop = (p, SEED, OFFSET)
    out, saved = ops.gru_fwd(d["x"], d["W_ih"], d["W_hh"], d["b_ih"], d["b_hh"], d["h0"], drop, save=True)
    if not backward:
        return out.cpu(), None
    g = {name: (None if d["g0"][name] is None else [t.clone() if accumulate else torch.zeros_like(t) for t in d["g0"][name]])
         for name in NAMES}
    dx = ops.gru_bwd_(d["dout"], d["x"], d["W_ih"], d["W_hh"], out, saved, d["h0"], drop, g["W_ih"], g["W_hh"], g["b_ih"], g["b_hh"],
                      want_dx=want_dx)
    grads = {name: (None if v is None else [t.cpu() for t in v]) for name, v in g.items()}
    grads["dx"] = None if dx is None else dx.cpu()
    return out.cpu(), grads


def _check(tag, k, n, p, out, grads, h_dev, accumulate=False):
    B, L, H = out.shape
    keeps = R.keep_masks(SEED, OFFSET, B, L, H, n, p)
    assert torch.equal(h_dev[-1], out), (tag, "the n-layer call and the call cut after the last layer differ")
    f = R.forward(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], k["h0"], p, keeps, h_dev=h_dev)
    worst = {}
    for i in range(n):
        worst[f"h{i}"] = r = R.ratio(h_dev[i], f[i]["h"], f[i]["Bh"])
        _note(f"h{i}/{tag}", r)
        assert r <= 1.0 and bool(torch.isfinite(h_dev[i]).all()), (tag, f"h{i}", r)
    if grads is None:
        return worst
    ref = R.backward(k["dout"], k["x"], k["W_ih"], k["W_hh"], k["h0"], h_dev, f, p, keeps, k["g0"] if accumulate else None)
    if grads["dx"] is not None:
        worst["dx"] = r = R.ratio(grads["dx"], *ref["dx"])
        _note(f"dx/{tag}", r)
        assert r <= 1.0, (tag, "dx", r)
    for name in NAMES:
        if grads[name] is None:
            continue
        for i in range(n):
            worst[f"{name}{i}"] = r = R.ratio(grads[name][i], *ref[name][i])
            _note(f"{name}{i}/{tag}", r)
            assert r <= 1.0, (tag, name, i, r)
            assert float(grads[name][i].abs().max()) > 0 or float(ref[name][i][0].abs().max()) == 0, (tag, name, i, "all zero")
    return worst


# ------------------------------------------------------------------------------------------------ entries against float64
@pytest.mark.parametrize("shape", SHAPES, ids=[_tag(s) for s in SHAPES])
def test_entries_against_float64(shape):
    """1x1x8x8: one step, one session.  3x2x5x12 without biases: odd widths.  17x20x65x33: nothing divisible, B straddles a
    session tile.  33x21x48x64x2 p 0.3: two layers with dropout between them.  65x20x128x128 with h0: the tutorial's width, the
    on-chip W_hh limit.  5x100x24x100x3 p 0.1: a long session, three layers.  2x1023x16x16, forward only: the longest session."""
    B, L, K0, H, n, bias, p, with_h0, fwd_only = shape
    k = R.make_case(B, L, K0, H, n, bias=bias, with_h0=with_h0)
    out, grads = _run(k, n, p, backward=not fwd_only)
    h_dev = _device_h(_dev(k), n, (p, SEED, OFFSET))
    worst = _check(_tag(shape), k, n, p, out, grads, h_dev)
    print(f"{_tag(shape)}: " + ", ".join(f"{a} {v:.3f}" for a, v in worst.items()))


def test_saturated_gates_stay_finite_and_exact():
    """inputs scaled until the pre-activations pass +-30: finite outputs within the bounds; where float64 says the update gate is
    1 and the candidate is +-1 once rounded to fp32 (sig: v >= 17.4; tanh: |v| >= 9.1, past the rounding tie at 9.011), the
    device's gates are exactly those: h_t = fl(n + fl(h_{t-1} - n)) bit for bit; backward finite"""
    B, L, K0, H = 17, 6, 33, 33
    k = R.make_case(B, L, K0, H, 1, x_scale=40.0)
    out, grads = _run(k, 1, 0.0)
    h_dev = [out]
    keeps = R.keep_masks(SEED, OFFSET, B, L, H, 1, 0.0)
    f = R.forward(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], None, 0.0, keeps, h_dev=h_dev)[0]
    assert float(f["pz"].abs().max()) > 30 and float(f["pn"].abs().max()) > 30 and float(f["pr"].abs().max()) > 30
    r = R.ratio(out, f["h"], f["Bh"])
    _note("saturated/h0", r)
    assert r <= 1.0 and bool(torch.isfinite(out).all())
    exact = (f["pz"] >= 17.4) & (f["pn"].abs() >= 9.1)
    assert int(exact.sum()) > 50
    hprev = torch.cat([torch.zeros(B, 1, H), out[:, :-1]], 1)
    nn = torch.sign(f["pn"]).float()
    want = nn + (hprev - nn)                                 # fp32: z = 1 exactly, n = +-1 exactly
    assert torch.equal(out[exact], want[exact])
    off = f["pz"] <= -104.0                                  # sig rounds to 0 in fp32 only below the smallest subnormal: h = n
    assert torch.equal(out[off & (f["pn"].abs() >= 9.1)], nn[off & (f["pn"].abs() >= 9.1)])
    for name in NAMES:
        assert bool(torch.isfinite(grads[name][0]).all()), name
    assert bool(torch.isfinite(grads["dx"]).all())
    ref = R.backward(k["dout"], k["x"], k["W_ih"], k["W_hh"], None, h_dev, [f], 0.0, keeps)
    _note("saturated/dx", R.ratio(grads["dx"], *ref["dx"]))
    assert R.ratio(grads["dx"], *ref["dx"]) <= 1.0


# ------------------------------------------------------------------------------------------------ bit identity and accumulation
@pytest.mark.parametrize("B,L,K0,H,n,p", [(17, 20, 65, 33, 1, 0.0), (33, 21, 48, 64, 2, 0.3), (5, 9, 24, 100, 3, 0.1)])
def test_inference_out_is_the_training_forms_output(B, L, K0, H, n, p):
    k = _dev(R.make_case(B, L, K0, H, n, with_h0=True))
    for drop in ((0.0, 0, 0), (p, SEED, OFFSET)):
        out = ops.gru_fwd(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], k["h0"], drop)
        assert out.shape == (B, L, H)
        assert torch.equal(out, ops.gru_fwd(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], k["h0"], drop, save=True)[0])


@pytest.mark.parametrize("H,n", [(33, 2), (128, 1)])
def test_a_session_has_the_same_bits_alone_and_in_a_batch(H, n):
    """p = 0 (the mask of a row depends on its index by definition): a session's h and its dx, alone, at another place in the
    launch, and inside the batch at sessions 0, 16 and 36 (tile edges and the tail tile)"""
    B, L, K0 = 37, 7, 24
    k = _dev(R.make_case(B, L, K0, H, n, with_h0=True))
    args = (k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"])
    out, saved = ops.gru_fwd(k["x"], *args, k["h0"], save=True)
    dx = ops.gru_bwd_(k["dout"], k["x"], k["W_ih"], k["W_hh"], out, saved, k["h0"])
    for b in (0, 16, 36):
        x1, d1, h1 = k["x"][b:b + 1].contiguous(), k["dout"][b:b + 1].contiguous(), k["h0"][:, b:b + 1].contiguous()
        o1, s1 = ops.gru_fwd(x1, *args, h1, save=True)
        assert torch.equal(o1[0], out[b])
        assert torch.equal(ops.gru_bwd_(d1, x1, k["W_ih"], k["W_hh"], o1, s1, h1)[0], dx[b])
        lo = b - b % 5
        sub = ops.gru_fwd(k["x"][lo:b + 1].contiguous(), *args, k["h0"][:, lo:b + 1].contiguous())
        assert torch.equal(sub[-1], out[b])


def test_a_right_padded_sessions_real_positions_do_not_depend_on_its_padding():
    k = _dev(R.make_case(5, 12, 24, 33, 2))
    args = (k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"])
    full = ops.gru_fwd(k["x"], *args)
    other = k["x"].clone()
    other[:, 7:] = 3.0
    assert torch.equal(ops.gru_fwd(other, *args)[:, :7], full[:, :7])
    assert torch.equal(ops.gru_fwd(k["x"][:, :7].contiguous(), *args), full[:, :7])


def _shift(t):
    flat = torch.empty(t.numel() + 1, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("which", ["x", "W_ih0", "W_hh1", "b_ih0", "b_hh1", "dout", "h0"])
def test_a_view_at_a_4_byte_offset_takes_the_scalar_path_with_the_same_bits(which):
    k = _dev(R.make_case(19, 9, 48, 64, 2, with_h0=True))
    drop = (0.3, SEED, OFFSET)

    def run(kk):
        out, saved = ops.gru_fwd(kk["x"], kk["W_ih"], kk["W_hh"], kk["b_ih"], kk["b_hh"], kk["h0"], drop, save=True)
        g = [[torch.zeros_like(t) for t in k[name]] for name in NAMES]
        dx = ops.gru_bwd_(kk["dout"], kk["x"], kk["W_ih"], kk["W_hh"], out, saved, kk["h0"], drop, *g)
        return [out, dx] + [t for lst in g for t in lst]

    shifted = dict(k, **{name: list(k[name]) for name in NAMES})
    if which in ("x", "dout", "h0"):
        shifted[which] = _shift(k[which])
    else:
        shifted[which[:-1]][int(which[-1])] = _shift(k[which[:-1]][int(which[-1])])
    for a, b in zip(run(k), run(shifted)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("bias,p", [(True, 0.3), (False, 0.0)])
def test_two_runs_give_the_same_bits_and_gradients_accumulate(bias, p):
    B, L, K0, H, n = 33, 21, 48, 64, 2
    k = R.make_case(B, L, K0, H, n, bias=bias, seed=1)
    names = NAMES if bias else NAMES[:2]
    o1, g1 = _run(k, n, p)
    o2, g2 = _run(k, n, p)
    assert torch.equal(o1, o2) and torch.equal(g1["dx"], g2["dx"])
    for name in names:
        for x, y in zip(g1[name], g2[name]):
            assert torch.equal(x, y), name
    # accumulated: the batch sum is formed first, then added once to what the buffers held
    o3, g3 = _run(k, n, p, accumulate=True)
    for name in names:
        for i in range(n):
            assert torch.equal(g3[name][i], k["g0"][name][i] + g1[name][i]), (name, i)
    assert torch.equal(g3["dx"], g1["dx"])                                   # overwritten, not accumulated
    _check("accumulate", k, n, p, o3, g3, _device_h(_dev(k), n, (p, SEED, OFFSET)), accumulate=True)
    # a second backward into the same buffers adds exactly its gradients: x + x is exact
    d = _dev(k)
    drop = (p, SEED, OFFSET)
    out, saved = ops.gru_fwd(d["x"], d["W_ih"], d["W_hh"], d["b_ih"], d["b_hh"], None, drop, save=True)
    dW = [torch.zeros_like(w) for w in d["W_hh"]]
    for _ in range(2):
        ops.gru_bwd_(d["dout"], d["x"], d["W_ih"], d["W_hh"], out, saved, None, drop, None, dW, None, None, want_dx=False)
    for i in range(n):
        assert torch.equal(dW[i].cpu(), g1["W_hh"][i] + g1["W_hh"][i])


def test_null_outputs_and_no_sessions():
    B, L, K0, H, n = 19, 9, 48, 64, 2
    k = _dev(R.make_case(B, L, K0, H, n))
    drop = (0.3, SEED, OFFSET)
    Wi, Wh = k["W_ih"], k["W_hh"]
    out, saved = ops.gru_fwd(k["x"], Wi, Wh, k["b_ih"], k["b_hh"], None, drop, save=True)
    full = [[torch.zeros_like(t) for t in k[name]] for name in NAMES]
    dx = ops.gru_bwd_(k["dout"], k["x"], Wi, Wh, out, saved, None, drop, *full)
    assert torch.equal(ops.gru_bwd_(k["dout"], None, Wi, Wh, out, saved, None, drop), dx)            # dx only: x is not read
    w1 = torch.zeros_like(Wh[1])
    assert ops.gru_bwd_(k["dout"], None, Wi, Wh, out, saved, None, drop, None, [None, w1], want_dx=False) is None
    assert torch.equal(w1, full[1][1])
    b0 = torch.zeros_like(k["b_ih"][0])
    assert ops.gru_bwd_(k["dout"], k["x"], Wi, Wh, out, saved, None, drop, None, None, [b0, None], None, want_dx=False) is None
    assert torch.equal(b0, full[2][0])
    bh0 = torch.zeros_like(k["b_hh"][0])
    assert torch.equal(ops.gru_bwd_(k["dout"], None, Wi, Wh, out, saved, None, drop, None, None, None, [bh0, None]), dx)
    assert torch.equal(bh0, full[3][0])
    assert ops.gru_bwd_(k["dout"], None, Wi, Wh, out, saved, None, drop, want_dx=False) is None      # nothing asked: nothing launches
    # no biases: the same as biases of zeros
    zeros = [torch.zeros_like(b) for b in k["b_ih"]]
    assert torch.equal(ops.gru_fwd(k["x"], Wi, Wh, None, None, None, drop), ops.gru_fwd(k["x"], Wi, Wh, zeros, zeros, None, drop))
    assert torch.equal(ops.gru_fwd(k["x"], Wi, Wh, [None, k["b_ih"][1]], None, None, drop),
                       ops.gru_fwd(k["x"], Wi, Wh, [zeros[0], k["b_ih"][1]], zeros, None, drop))
    empty = ops.gru_fwd(k["x"][:0], Wi, Wh, k["b_ih"], k["b_hh"])
    assert empty.shape == (0, L, H)
    e_out, e_saved = ops.gru_fwd(k["x"][:0], Wi, Wh, k["b_ih"], k["b_hh"], save=True)
    assert ops.gru_bwd_(k["dout"][:0], k["x"][:0], Wi, Wh, e_out, e_saved).shape == (0, L, K0)


# ------------------------------------------------------------------------------------------------ buffer discipline
@pytest.mark.parametrize("fill", FILLS, ids=["zeros", "ones"])
@pytest.mark.parametrize("B,L,K0,H,n,p", [(17, 20, 65, 33, 1, 0.0), (33, 21, 48, 64, 2, 0.3)])
def test_red_zones_around_every_buffer(B, L, K0, H, n, p, fill):
    """guards around every buffer, saved and the workspaces exactly as large as the size queries say, under both fills, each call
    twice"""
    lib = _lib.load()
    k = R.make_case(B, L, K0, H, n, with_h0=True)
    Ks = [K0] + [H] * (n - 1)
    T = B * L
    a = Arena(fill, DEV, capacity=32 << 20)
    x = a.new("x", "in", F32, T * K0).set(k["x"])
    h0 = a.new("h0", "in", F32, n * B * H).set(k["h0"])
    Wi = [a.new(f"W_ih{i}", "in", F32, 3 * H * Ks[i]).set(k["W_ih"][i]) for i in range(n)]
    Wh = [a.new(f"W_hh{i}", "in", F32, 3 * H * H).set(k["W_hh"][i]) for i in range(n)]
    bi = [a.new(f"b_ih{i}", "in", F32, 3 * H).set(k["b_ih"][i]) for i in range(n)]
    bh = [a.new(f"b_hh{i}", "in", F32, 3 * H).set(k["b_hh"][i]) for i in range(n)]
    out = a.new("out", "out", F32, T * H)
    n_fws = lib.t4r_gru_fwd_ws_floats(B, L, n, K0, H)
    n_saved = lib.t4r_gru_saved_floats(B, L, n, K0, H)
    n_bws = lib.t4r_gru_bwd_ws_floats(B, L, n, K0, H)
    assert n_fws > 0 and n_saved > 0 and n_bws > 0
    fws = a.ws("fwd_ws", 4 * n_fws)
    a.seal()
    ptrs = lambda bufs: _lib.ptr_array([b.ptr for b in bufs])  # noqa: E731
    (Ip, k1), (Hp, k2), (Bi, k3), (Bh, k4) = ptrs(Wi), ptrs(Wh), ptrs(bi), ptrs(bh)
    d = _dev(k)
    want, _ = ops.gru_fwd(d["x"], d["W_ih"], d["W_hh"], d["b_ih"], d["b_hh"], d["h0"], (p, SEED, OFFSET), save=True)
    for _ in range(2):              # inference form: out only
        rc = lib.t4r_gru_fwd(_stream(), x.ptr, h0.ptr, Ip, Hp, Bi, Bh, out.ptr, None, fws.ptr, B, L, n, K0, H, p, SEED, OFFSET)
        assert rc == 0, lib.t4r_last_error()
        torch.cuda.synchronize()
        v = a.check()
        assert v is None, str(v)
        assert torch.equal(out.t.view(B, L, H), want)
    saved = a.ws("saved", 4 * n_saved)
    a.seal()
    for _ in range(2):              # training form
        rc = lib.t4r_gru_fwd(_stream(), x.ptr, h0.ptr, Ip, Hp, Bi, Bh, out.ptr, saved.ptr, fws.ptr, B, L, n, K0, H, p, SEED, OFFSET)
        assert rc == 0, lib.t4r_last_error()
        torch.cuda.synchronize()
        v = a.check()
        assert v is None, str(v)
        assert torch.equal(out.t.view(B, L, H), want)
    # ---- backward: the exact workspace
    dyb = a.new("dout", "in", F32, T * H).set(k["dout"])
    dx = a.new("dx", "out", F32, T * K0)
    g = {name: [a.new(f"d_{name}{i}", "inout", F32, k[name][i].numel()).set(0) for i in range(n)] for name in NAMES}
    bws = a.ws("bwd_ws", 4 * n_bws)
    a.seal()
    G = [ptrs(g[name]) for name in NAMES]
    first = None
    for _ in range(2):
        for name in NAMES:
            for t in g[name]:
                t.t.zero_()
        rc = lib.t4r_gru_bwd(_stream(), dyb.ptr, x.ptr, h0.ptr, Ip, Hp, out.ptr, saved.ptr, dx.ptr, G[0][0], G[1][0], G[2][0], G[3][0],
                             bws.ptr, B, L, n, K0, H, p, SEED, OFFSET)
        assert rc == 0, lib.t4r_last_error()
        torch.cuda.synchronize()
        v = a.check()
        assert v is None, str(v)
        assert a.nonfinite() is None
        got = [dx.bits()] + [t.bits() for name in NAMES for t in g[name]]
        if first is None:
            first = got
        for p0, p1 in zip(first, got):
            assert torch.equal(p0, p1)
    grads = {name: [g[name][i].t.view(k[name][i].shape).cpu() for i in range(n)] for name in NAMES}
    grads["dx"] = dx.t.view(B, L, K0).cpu()
    _check("arena", k, n, p, out.t.view(B, L, H).cpu(), grads, _device_h(d, n, (p, SEED, OFFSET)))


# ------------------------------------------------------------------------------------------------ registered operators
@pytest.mark.parametrize("bias,p", [(True, 0.3), (False, 0.0)])
def test_registered_operators_equal_the_ctypes_calls_and_differentiate(bias, p):
    B, L, K0, H, n = 9, 7, 24, 33, 2
    k = _dev(R.make_case(B, L, K0, H, n, bias=bias))
    x = k["x"].clone().requires_grad_()
    Wi, Wh = [w.clone().requires_grad_() for w in k["W_ih"]], [w.clone().requires_grad_() for w in k["W_hh"]]
    bi = [b.clone().requires_grad_() for b in k["b_ih"]] if bias else []
    bh = [b.clone().requires_grad_() for b in k["b_hh"]] if bias else []
    out = torch.ops.t4r_hip.gru_fwd(x, Wi, Wh, bi, bh, p, SEED, OFFSET)
    drop = (p, SEED, OFFSET)
    want, saved = ops.gru_fwd(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], None, drop, save=True)
    assert torch.equal(out, want)
    out.backward(k["dout"])
    g = [[torch.zeros_like(t) for t in k[name]] if k[name] is not None else None for name in NAMES]
    dx = ops.gru_bwd_(k["dout"], k["x"], k["W_ih"], k["W_hh"], want, saved, None, drop, *g)
    assert torch.equal(x.grad, dx)
    for i in range(n):
        assert torch.equal(Wi[i].grad, g[0][i]) and torch.equal(Wh[i].grad, g[1][i])
        if bias:
            assert torch.equal(bi[i].grad, g[2][i]) and torch.equal(bh[i].grad, g[3][i])


# ------------------------------------------------------------------------------------------------ module level
V, L, D_ITEM, D, B = 50, 20, 48, 64, 13


def _model(dims=(96, 64), n=2, masking="clm", seed=0, dropout=0.0, whh=0.25):
    """items 48 wide, the MLP stack, the GRU block 64 -> 64, L 20, tied head.  whh: the factor on the drawn W_hh (see
    gru_restatement.make_case: 0.25 takes U(-1/8, 1/8) to U(-2/64, 2/64), where the backward's carried bound says something)"""
    torch.manual_seed(seed)
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking=masking,
                                                   aggregation="concat", embedding_dims={"item_id": D_ITEM})
    blk = tr.GRUBlock(D, D, num_layers=n, dropout=dropout)
    with torch.no_grad():
        for i in range(n):
            getattr(blk.module, f"weight_hh_l{i}").mul_(whh)
    model = tr.Model(feats, blk, tr.NextItemPredictionTask(weight_tying=True), mlp_block=tr.MLPBlock(list(dims)))
    return model.to(DEV)


def _batch(n=B):
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(5, L + 1, (n,), generator=g)
    lens[0] = L
    m = torch.arange(L)[None] < lens[:, None]
    return {"item_id": (torch.randint(1, V + 1, (n, L), generator=g) * m).to(DEV)}


def _watch(model, seen, with_grad=True):
    blk = model.transformer_block

    def pre(_mod, args):
        a = args[0]
        seen["x"] = a.detach().clone()
        if with_grad and a.requires_grad:
            a.register_hook(lambda g: seen.__setitem__("dx", g.detach().clone()))

    def post(_mod, _inp, out):
        if with_grad and out.requires_grad:
            out.register_hook(lambda g: seen.__setitem__("dout", g.detach().clone()))
        seen["out"] = out.detach().clone()

    return [blk.register_forward_pre_hook(pre), blk.register_forward_hook(post)]


def _block_case(blk, seen):
    Wi, Wh, bi, bh = blk._params()
    host = lambda ts: None if ts is None else [t.cpu() for t in ts]  # noqa: E731
    k = dict(x=seen["x"].cpu(), W_ih=host(Wi), W_hh=host(Wh), b_ih=host(bi), b_hh=host(bh), h0=None, g0=None,
             dout=seen["dout"].cpu() if "dout" in seen else None)
    return k


def _check_block_output(tag, blk, seen, drop):
    """the block's output is the ops call's bits on its input, and every layer's h is within its bound of the restatement on the
    device's own h_{t-1} -> (case, device h)"""
    k = _block_case(blk, seen)
    d = _dev(dict(k, g0={}))
    n = blk.num_layers
    h_dev = _device_h(d, n, drop)
    assert torch.equal(h_dev[-1], seen["out"].cpu()) and seen["out"].shape == seen["x"].shape[:2] + (blk.hidden_size,)
    Bm, Lm, H = h_dev[-1].shape
    keeps = R.keep_masks(drop[1], drop[2], Bm, Lm, H, n, drop[0])
    f = R.forward(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], None, drop[0], keeps, h_dev=h_dev)
    for i in range(n):
        r = R.ratio(h_dev[i], f[i]["h"], f[i]["Bh"])
        _note(f"model/{tag}/h{i}", r)
        assert r <= 1.0, (tag, i, r)
    return k, h_dev, f, keeps


def test_a_training_step_equals_the_restated_block_of_its_inputs():
    """dropout 0.3 between the two layers: the MLP stack's output through the restated block (float64, the device's masks) at the
    block's output, the block's gradients and its input's gradient from the gradient that arrives there; the loss is finite"""
    model = _model(dropout=0.3).train()
    blk = model.transformer_block
    seen = {}
    hooks = _watch(model, seen)
    out = model(_batch(), training=True)
    assert bool(torch.isfinite(out["loss"])) and blk._drop_offset == 1
    out["loss"].backward()
    for h in hooks:
        h.remove()
    assert seen["x"].shape == (B, L, D) and seen["out"].shape == (B, L, D) and "dout" in seen and "dx" in seen
    drop = (0.3, blk.seed, 1)
    k, h_dev, f, keeps = _check_block_output("train", blk, seen, drop)
    ref = R.backward(k["dout"], k["x"], k["W_ih"], k["W_hh"], None, h_dev, f, 0.3, keeps)
    r = R.ratio(seen["dx"].cpu(), *ref["dx"])
    _note("model/train/dx", r)
    assert r <= 1.0
    for mine, theirs in (("W_ih", "weight_ih"), ("W_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
        for i in range(2):
            got = getattr(blk.module, f"{theirs}_l{i}").grad
            r = R.ratio(got.cpu(), *ref[mine][i])
            _note(f"model/train/{mine}{i}", r)
            assert r <= 1.0 and float(got.abs().max()) > 0, (mine, i, r)
    assert float(model.mlp_block[0][0].weight.grad.abs().max()) > 0
    assert float(model.input_features.item_embedding_table.weight.grad.abs().max()) > 0


def test_fast_path_and_autograd_visible_gradients_are_equal():
    x = _batch()
    grads = {}
    for visible in (False, True):
        model = _model(dropout=0.3).train()
        if visible:
            tr.enable_autograd_gradients(model)
        model(x, training=True)["loss"].backward()
        grads[visible] = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    keys = {f"heads.0.body.2.module.{n}_l{i}" for i in (0, 1) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    assert keys <= set(grads[False]) <= set(grads[True])
    for k in grads[False]:
        assert torch.equal(grads[True][k], grads[False][k]), k


@pytest.mark.parametrize("masking", ["clm", "mlm"])
def test_evaluation_and_topk_inference_equal_the_restated_composition(masking):
    model = _model(masking=masking, dropout=0.3).eval()
    model.top_k = 5
    blk = model.transformer_block
    x = _batch()
    with torch.no_grad():
        seen = {}
        hooks = _watch(model, seen, with_grad=False)
        ev = model(x, testing=True)
        assert bool(torch.isfinite(ev["loss"])) and ev["predictions"].shape[0] == ev["labels"].shape[0]
        _check_block_output(f"eval/{masking}", blk, seen, ops.NO_DROP)                   # evaluation: no dropout
        scores, items = model(x)
        for h in hooks:
            h.remove()
        assert scores.shape == (B, 5) and items.shape == (B, 5) and blk._drop_offset == 0
        assert seen["x"].shape == (B, L + 1 if masking == "mlm" else L, D)               # MLM inference: one more position
        _check_block_output(f"infer/{masking}", blk, seen, ops.NO_DROP)


def test_one_fused_adam_step_moves_every_gru_parameter_and_the_reducer_sees_them():
    model = _model(dropout=0.1).train()
    dense, tables = tr.flatten_model(model)
    opt = tr.FusedAdam([b for b in (dense, tables) if b is not None], lr=1e-2)
    named = dict(model.named_parameters())
    keys = [f"heads.0.body.2.module.{n}_l{i}" for i in (0, 1) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    hip = {id(p) for p in tr.hip_parameters(model)}
    assert {id(named[k]) for k in keys} <= hip
    assert set(keys) <= {name for name, _, _ in dense.entries}
    before = {k: named[k].detach().clone() for k in keys}
    model(_batch(), training=True)["loss"].backward()
    # the gradients landed in the flat buffer the reducer exchanges: views of it, non-zero
    lo, hi = dense.grad.data_ptr(), dense.grad.data_ptr() + 4 * dense.grad.numel()
    for k in keys:
        assert lo <= named[k].grad.data_ptr() < hi and float(named[k].grad.abs().max()) > 0, k
    reducer = tr.GradReducer(dense.grad, None if tables is None else tables.grad)
    assert reducer.dense is dense.grad and reducer.world == 1
    opt.step()
    torch.cuda.synchronize()
    for k in keys:
        moved = (named[k].detach() - before[k]).abs()
        assert float(moved.max()) > 1e-3 and bool(torch.isfinite(named[k]).all()), k      # Adam's first step: lr per element


def test_rng_state_replays_the_blocks_masks():
    model = _model(dropout=0.3).train()
    x = _batch()
    seen = {}
    hooks = _watch(model, seen, with_grad=False)
    with torch.no_grad():
        model(x, training=True)
        state = tr.get_rng_state(model)
        assert state["heads.0.body.2"]["_drop_offset"] == 1
        model(x, training=True)
        second = seen["out"].clone()
        model(x, training=True)
        third = seen["out"].clone()
        tr.set_rng_state(model, state)
        model(x, training=True)
    for h in hooks:
        h.remove()
    assert torch.equal(seen["out"], second) and not torch.equal(second, third)


# ------------------------------------------------------------------------------------------------ against the reference's step
FIXTURES = ("gru_body_clm_train", "gru_body_2layer_clm_train")


def _fixture_model(d):
    """the mirror of tools/make_gru_golden.py's reference model, with the reference's parameters"""
    import test_e2e_gpu as e2e

    Lf, Vf, dm = int(d["meta/L"]), int(d["meta/V"]), int(d["meta/d_model"])
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(Vf - 1, Lf), max_sequence_length=Lf, masking="clm",
                                                   aggregation="concat", embedding_dims={"item_id": int(d["meta/d_item"])})
    gru = torch.nn.GRU(dm, dm, num_layers=int(d["meta/num_layers"]), batch_first=True)
    mlp = tr.MLPBlock([int(v) for v in str(d["meta/dimensions"]).split(",")])
    model = tr.Model(feats, tr.Block(gru, [None, Lf, dm]), tr.NextItemPredictionTask(weight_tying=True), mlp_block=mlp)
    e2e.load_reference_state(model, d)
    return model.to(DEV)


def _tol_ratio(got, want, tol):
    got, want = got.detach().cpu().double(), want.double()
    return float(((got - want).abs() / (tol["atol"] + tol["rtol"] * want.abs())).max())


@pytest.mark.parametrize("name", FIXTURES)
def test_train_step_matches_the_reference_fixture(name):
    """the GRU's input and output, loss, labels, predictions and the gradients the fixture stores (the GRU, the stack, the
    masked-item vector, the item table, the task projection) against the reference's own step, with the tolerances
    tests/test_mlp_block_gpu.py::test_train_step_matches_the_reference_fixture applies, unchanged"""
    import golden_utils as gu
    import test_e2e_gpu as e2e

    d = gu.load(name)
    model = _fixture_model(d).train()
    assert sorted(model.state_dict().keys()) == sorted(str(d["meta/state_dict_keys"]).split("\n"))
    x = {k[3:]: gu.t(v).to(DEV) for k, v in d.items() if k.startswith("in/")}
    seen = {}
    hooks = _watch(model, seen)
    out = model(x, training=True)
    masking = model.input_features.masking
    assert torch.equal(masking.mask_schema.cpu(), gu.t(d["out/mask_schema"]))
    assert torch.equal(masking.masked_targets.cpu(), gu.t(d["out/masked_targets"]))
    assert torch.equal(out["labels"].cpu(), gu.t(d["out/labels"]))
    grad_tol = dict(rtol=2e-4, atol=1e-4)
    for mine, theirs in (("x", "gru_in"), ("out", "gru_out")):
        _note(f"fixture/{name}/{theirs}", _tol_ratio(seen[mine], gu.t(d["out/" + theirs]), e2e.TOL))
        e2e.close(seen[mine], gu.t(d["out/" + theirs]))
    _note(f"fixture/{name}/predictions", _tol_ratio(out["predictions"], gu.t(d["out/predictions"]), e2e.TOL))
    _note(f"fixture/{name}/loss", _tol_ratio(out["loss"], gu.t(d["out/loss"]), e2e.TOL))
    e2e.close(out["predictions"], gu.t(d["out/predictions"]))
    e2e.close(out["loss"], gu.t(d["out/loss"]))
    assert abs(float(out["loss"]) - float(d["out/loss"])) < 1e-3
    assert float((out["predictions"].cpu() - gu.t(d["out/predictions"])).abs().max()) < 1e-3
    out["loss"].backward()
    for h in hooks:
        h.remove()
    for mine, theirs in (("dx", "gru_in_grad"), ("dout", "gru_out_grad")):
        _note(f"fixture/{name}/{theirs}", _tol_ratio(seen[mine], gu.t(d["out/" + theirs]), grad_tol))
        e2e.close(seen[mine], gu.t(d["out/" + theirs]), **grad_tol)
    g = gu.section(d, "g/")
    named = dict(model.named_parameters())
    need = ["heads.0.body.2.module.weight_ih_l0", "heads.0.body.2.module.weight_hh_l0", "heads.0.body.2.module.bias_ih_l0",
            "heads.0.body.2.module.bias_hh_l0", "heads.0.body.1.0.0.weight", "heads.0.body.0._masking.masked_item_embedding",
            "heads.0.body.0.to_merge.categorical_module.embedding_tables.item_id.weight",
            "heads.0.prediction_task_dict.next-item.task_block.0.0.weight"]
    assert set(need) <= set(g), sorted(set(need) - set(g))
    for k, ref in g.items():
        assert k in named and named[k].grad is not None, k
        short = k.replace("heads.0.body.", "").replace("heads.0.prediction_task_dict.", "")
        r = _tol_ratio(named[k].grad, ref, grad_tol)
        _note(f"fixture/{name}/g/{short}", r)
        print(f"{name} {short}: {r:.3f}")
        e2e.close(named[k].grad, ref, msg=lambda m, k=k: f"{k}: {m}", **grad_tol)
    assert len(g) >= 10
    assert np.isfinite(float(out["loss"]))
