"""Host half of the GRU body: the feature header (include/t4r_hip_gru.h) and its binding through _lib.FEATURE_HEADERS, the size
queries and the argument limits (refused before any launch), the float64 restatement (tests/gru_restatement.py) against a live
torch.nn.GRU in float64, against the committed fixtures and against planted faults at the GPU test's shapes, the registered
operators' fakes, the module's names and initialisation, Block(...)'s conversion and refusals, the Model's state-dict keys
against the fixture's.  Nothing here needs a GPU."""
import ctypes
import os
import re

import pytest
import torch

import gru_restatement as R
import transformers4rec_amd as tr
from transformers4rec_amd import _lib, ops, torch_ops  # noqa: F401
from transformers4rec_amd.block import Block, GRUBlock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = "t4r_hip_gru.h"
SIX = ["t4r_gru_bwd", "t4r_gru_bwd_ws_floats", "t4r_gru_fwd", "t4r_gru_fwd_ws_floats", "t4r_gru_saved_floats", "t4r_gru_supported"]
SEED, OFFSET = 0x5EED1234ABCD, 3
# the shapes of tests/test_gru_gpu.py: (B, L, K0, H, n, bias, p, h0 given, forward only)
SHAPES = [(1, 1, 8, 8, 1, True, 0.0, False, False), (3, 2, 5, 12, 1, False, 0.0, False, False), (17, 20, 65, 33, 1, True, 0.0, False, False),
          (33, 21, 48, 64, 2, True, 0.3, False, False), (65, 20, 128, 128, 1, True, 0.0, True, False),
          (5, 100, 24, 100, 3, True, 0.1, False, False), (2, 1023, 16, 16, 1, True, 0.0, False, True)]


# ---------------------------------------------------------------------------------------------------------- header and binding
def test_header_parses_and_is_bound_through_the_feature_tuple():
    assert _lib.FEATURE_HEADERS == ("t4r_hip_postfusion.h", HEADER, "t4r_hip_mlpblock.h")
    assert _lib.FEATURE_HEADERS[-1] == "t4r_hip_mlpblock.h"
    assert HEADER not in _lib.HEADERS and HEADER not in _lib.EXTENSION_HEADERS
    assert _lib.header_symbols(HEADER) == SIX
    feat = _lib.feature_signatures()
    assert set(SIX) <= set(feat)
    assert not set(feat) & set(_lib.signatures()) and not set(feat) & set(_lib.extension_signatures())
    others = [n for h in _lib.FEATURE_HEADERS if h != HEADER for n in _lib.header_symbols(h)]
    assert not set(SIX) & set(others)
    assert feat["t4r_gru_supported"] == ("i", "iiii")
    for name in ("t4r_gru_saved_floats", "t4r_gru_fwd_ws_floats", "t4r_gru_bwd_ws_floats"):
        assert feat[name] == ("l", "liiii")
    assert feat["t4r_gru_fwd"] == ("i", "p" * 10 + "l" + "iiii" + "f" + "QQ")
    assert feat["t4r_gru_bwd"] == ("i", "p" * 14 + "l" + "iiii" + "f" + "QQ")
    lib = _lib.load()
    for name in SIX:
        fn = getattr(lib, name)
        ret, args = feat[name]
        assert fn.restype is _lib._C[ret] and list(fn.argtypes) == [_lib._C[a] for a in args], name
    text = open(_lib.header_path(HEADER)).read()
    for entry in ("int t4r_gru_fwd(void* stream", "int t4r_gru_bwd(void* stream"):
        decl = text[: text.index(entry)]
        comment = decl[decl.rindex("/*"):]
        assert "replaces:" in comment and "torch.nn.GRU" in comment and "block/base.py:87-106" in comment and "launch" in comment, entry
    assert "expf" in text and "1 / (1 + expf(-v))" in text and "1 - 2 / (1 + expf(2 v))" in text     # how sig and tanh are evaluated
    decls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in decls, f"{word} leaked into the C ABI"
    build = open(os.path.join(ROOT, "transformers4rec_amd", "build.py")).read()
    assert HEADER in build and '"gru.hip"' in build
    sites = (ops.SITE_INPUT, ops.SITE_POS, ops.SITE_PROB, ops.SITE_ATTN_OUT, ops.SITE_FF_ACT, ops.SITE_FF_OUT, ops.SITE_FINAL,
             ops.SITE_GUMBEL, ops.SITE_MLP_BLOCK)
    assert ops.SITE_GRU == R.SITE == 9 and ops.SITE_GRU not in sites
    assert torch_ops.OPERATORS[-2:] == ("gru_fwd", "gru_bwd") and len(torch_ops.OPERATORS) == 50
    assert len(set(torch_ops.OPERATORS)) == len(torch_ops.OPERATORS)


# ---------------------------------------------------------------------------------------------------------- limits
BUF = ctypes.c_void_p(1 << 20)        # never dereferenced: every failing case below is refused before any launch


def _ptrs(n, p=BUF):
    return (ctypes.c_void_p * n)(*([p.value] * n))


def _fwd(lib, B=3, L=5, n=2, K0=8, H=12, p=0.0, x=BUF, W="ok", Wh="ok", out=BUF, ws=BUF, saved=None, h0=None):
    return lib.t4r_gru_fwd(None, x, h0, _ptrs(max(n, 1)) if W == "ok" else W, _ptrs(max(n, 1)) if Wh == "ok" else Wh, None, None, out,
                           saved, ws, B, L, n, K0, H, p, 1, 2)


def _bwd(lib, B=3, L=5, n=2, K0=8, H=12, p=0.0, x=BUF, W="ok", Wh="ok", out=BUF, ws=BUF, saved=BUF, h0=None, dout=BUF, dW=None):
    return lib.t4r_gru_bwd(None, dout, x, h0, _ptrs(max(n, 1)) if W == "ok" else W, _ptrs(max(n, 1)) if Wh == "ok" else Wh, out, saved,
                           BUF, dW, None, None, None, ws, B, L, n, K0, H, p, 1, 2)


def test_supported_agrees_with_the_documented_limits():
    lib = _lib.load()
    cases = [((1, 1, 1, 1), 1), ((4, 1024, 128, 1023), 1), ((1, 128, 128, 20), 1), ((2, 65, 33, 21), 1), ((0, 8, 8, 4), 0),
             ((5, 8, 8, 4), 0), ((1, 0, 8, 4), 0), ((1, 1025, 8, 4), 0), ((1, 8, 0, 4), 0), ((1, 8, 129, 4), 0), ((1, 8, 8, 0), 0),
             ((1, 8, 8, 1024), 0)]
    for (n, K0, H, L), want in cases:
        assert lib.t4r_gru_supported(n, K0, H, L) == want, (n, K0, H, L)
        assert ops.gru_supported(n, K0, H, L) == bool(want)
    assert (ops.GRU_MAX_LAYERS, ops.GRU_MAX_K0, ops.GRU_MAX_H, ops.GRU_MAX_L) == (4, 1024, 128, 1023)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    for call in (_fwd, _bwd):
        for kw, word in ((dict(n=0), b"layers"), (dict(n=5), b"layers"), (dict(K0=0), b"K0"), (dict(K0=1025), b"K0"), (dict(H=0), b"H"),
                         (dict(H=129), b"H"), (dict(L=0), b"L"), (dict(L=1024), b"L"), (dict(B=-1), b"B"),
                         (dict(B=(1 << 31) // (5 * 36) + 1), b"2^31"), (dict(p=1.0), b"drop_p"), (dict(p=-0.1), b"drop_p"),
                         (dict(W=None), b"null"), (dict(Wh=None), b"null"), (dict(W=_ptrs(2, ctypes.c_void_p(0))), b"null"),
                         (dict(Wh=_ptrs(2, ctypes.c_void_p(0))), b"null"), (dict(W=_ptrs(2, ctypes.c_void_p((1 << 20) + 2))), b"aligned"),
                         (dict(out=None), b"null"), (dict(ws=None), b"null"), (dict(x=ctypes.c_void_p((1 << 20) + 1)), b"aligned"),
                         (dict(h0=ctypes.c_void_p((1 << 20) + 3)), b"aligned")):
            assert call(lib, **kw) != 0, (call.__name__, kw)
            assert word in lib.t4r_last_error(), (call.__name__, kw, lib.t4r_last_error())
    assert _fwd(lib, x=None) != 0 and b"null" in lib.t4r_last_error()
    assert _bwd(lib, dout=None) != 0 and b"null" in lib.t4r_last_error()
    assert _bwd(lib, saved=None) != 0 and b"null" in lib.t4r_last_error()
    assert _bwd(lib, dW=_ptrs(2), x=None) != 0 and b"d_W_ih[0]" in lib.t4r_last_error()
    # B = 0: nothing launches, nothing is looked at but the sizes
    assert lib.t4r_gru_fwd(None, None, None, None, None, None, None, None, None, None, 0, 5, 2, 8, 12, 0.0, 0, 0) == 0
    assert lib.t4r_gru_bwd(None, None, None, None, None, None, None, None, None, None, None, None, None, None, 0, 5, 2, 8, 12, 0.3, 0, 0) == 0
    x, Wi, Wh = torch.zeros(2, 3, 8), [torch.zeros(36, 8)], [torch.zeros(36, 12)]
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.gru_fwd(x, Wi, Wh)
    with pytest.raises(_lib.T4RHipError, match="GPU"):
        ops.gru_bwd_(torch.zeros(2, 3, 12), x, Wi, Wh, torch.zeros(2, 3, 12), torch.zeros(1))


def test_size_queries_are_pure_monotone_and_zero_outside_the_limits():
    lib = _lib.load()
    for f in (lib.t4r_gru_saved_floats, lib.t4r_gru_fwd_ws_floats, lib.t4r_gru_bwd_ws_floats):
        for args in ((0, 5, 1, 8, 8), (-3, 5, 1, 8, 8), (1 << 31, 5, 1, 8, 8), (4, 0, 1, 8, 8), (4, 1024, 1, 8, 8), (4, 5, 0, 8, 8),
                     (4, 5, 5, 8, 8), (4, 5, 1, 0, 8), (4, 5, 1, 1025, 8), (4, 5, 1, 8, 0), (4, 5, 1, 8, 129),
                     ((1 << 31) // (5 * 24) + 1, 5, 1, 8, 8)):
            assert f(*args) == 0, args
        for L, n, K0, H in ((1, 1, 1, 1), (20, 1, 128, 128), (21, 2, 48, 64), (100, 3, 24, 100), (1023, 4, 1024, 128)):
            top = ((1 << 31) - 1) // (L * max(K0, 3 * H))
            Bs = [b for b in (1, 2, 15, 16, 17, 33, 1024, 100000) if b <= top] + [top]
            got = [f(B, L, n, K0, H) for B in Bs]
            assert got == [f(B, L, n, K0, H) for B in Bs] and got == sorted(got) and got[0] > 0, (L, n, K0, H, got)
    assert lib.t4r_gru_saved_floats(8, 20, 2, 64, 64) >= 8 * 20 * 64 * 5          # the gate values of two layers and one output


# ---------------------------------------------------------------------------------------------------------- the restatement
def _torch_gru(k, n, bias, H, K0):
    gru = torch.nn.GRU(K0, H, num_layers=n, bias=bias, batch_first=True).double()
    with torch.no_grad():
        for i in range(n):
            getattr(gru, f"weight_ih_l{i}").copy_(k["W_ih"][i])
            getattr(gru, f"weight_hh_l{i}").copy_(k["W_hh"][i])
            if bias:
                getattr(gru, f"bias_ih_l{i}").copy_(k["b_ih"][i])
                getattr(gru, f"bias_hh_l{i}").copy_(k["b_hh"][i])
    return gru


@pytest.mark.parametrize("n,bias", [(1, True), (1, False), (3, True), (3, False)])
def test_restatement_is_torch_gru_in_float64(n, bias):
    B, L, K0, H = 4, 7, 5, 6
    k = R.make_case(B, L, K0, H, n, bias=bias, with_h0=True, whh_scale=1.0 / H ** 0.5)
    gru = _torch_gru(k, n, bias, H, K0)
    x = k["x"].double().requires_grad_()
    out, _ = gru(x, k["h0"].double())
    out.backward(k["dout"].double())
    keeps = R.keep_masks(SEED, OFFSET, B, L, H, n, 0.0)
    f = R.forward(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], k["h0"], 0.0, keeps)
    assert (f[-1]["h"] - out.detach()).abs().max() < 1e-12
    hs = [lay["h"] for lay in f]
    g = R.backward(k["dout"], k["x"], k["W_ih"], k["W_hh"], k["h0"], hs, f, 0.0, keeps)
    assert (g["dx"][0] - x.grad).abs().max() < 1e-12
    for i in range(n):
        names = [("W_ih", "weight_ih"), ("W_hh", "weight_hh")] + ([("b_ih", "bias_ih"), ("b_hh", "bias_hh")] if bias else [])
        for mine, theirs in names:
            assert (g[mine][i][0] - getattr(gru, f"{theirs}_l{i}").grad).abs().max() < 1e-12, (mine, i)


def _case(shape, h0=None, p=None, n=None):
    B, L, K0, H, n0, bias, p0, h00, _ = shape
    n, p, h0 = n0 if n is None else n, p0 if p is None else p, h00 if h0 is None else h0
    k = R.make_case(B, L, K0, H, n, bias=bias, with_h0=h0)
    return k, n, p


def _worst_forward(k, n, p, keeps, h_dev, fault=None, fault_keeps=None):
    f = R.forward(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], k["h0"], p, fault_keeps or keeps, fault=fault, h_dev=h_dev)
    return max(R.ratio(h_dev[i], f[i]["h"], f[i]["Bh"]) for i in range(n))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] <= 100], ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_planted_faults_exceed_their_bounds(shape):
    """each planted fault lies outside the bounds at the GPU test's shapes with L <= 100, against a stand-in for the device (the
    float64 restatement rounded to fp32); the case is given what the fault needs to show (h0, a second layer with p >= 0.3, the
    biases), and a fault that cannot be expressed at a shape is not asked there: the time chain at L = 1, the transposed mask of
    a single token row"""
    B, L, K0, H = shape[:4]
    n, p = max(shape[4], 2), max(shape[6], 0.3)
    k = R.make_case(B, L, K0, H, n, bias=True, with_h0=True)
    keeps = R.keep_masks(SEED, OFFSET, B, L, H, n, p)
    h_dev = R.fp32_standin(k, p, keeps)
    assert _worst_forward(k, n, p, keeps, h_dev) < 1.0
    for fault in ("gates_zr", "bhn_outside", "blend_swapped", "h0_ignored"):
        assert _worst_forward(k, n, p, keeps, h_dev, fault=fault) > 10.0, fault
    if L > 1:
        assert _worst_forward(k, n, p, keeps, h_dev, fault="drop_state") > 10.0
    assert _worst_forward(k, n, p, keeps, h_dev, fault_keeps=R.keep_masks(SEED, OFFSET, B, L, H, n, p, fault="mask_prev_layer")) > 10.0
    if B * L > 1:
        assert _worst_forward(k, n, p, keeps, h_dev, fault_keeps=R.keep_masks(SEED, OFFSET, B, L, H, n, p, fault="mask_transposed")) > 10.0
    f = R.forward(k["x"], k["W_ih"], k["W_hh"], k["b_ih"], k["b_hh"], k["h0"], p, keeps, h_dev=h_dev)
    good = R.backward(k["dout"], k["x"], k["W_ih"], k["W_hh"], k["h0"], h_dev, f, p, keeps, k["g0"])

    def worst(bad, names):
        out = 0.0
        for name in names:
            pairs = [(good[name], bad[name])] if name == "dx" else zip(good[name], bad[name])
            for (want, _), (got, bound) in pairs:
                out = max(out, R.ratio(want.float(), got, bound))
        return out
    every = ("dx", "W_ih", "W_hh", "b_ih", "b_hh")
    assert worst(good, every) < 1.0                                    # fp32 rounding of the right values is inside
    if L > 1:
        bad = R.backward(k["dout"], k["x"], k["W_ih"], k["W_hh"], k["h0"], h_dev, f, p, keeps, k["g0"], fault="bptt_truncated")
        assert worst(bad, ("dx", "W_ih", "b_ih")) > 10.0
    bad = R.backward(k["dout"], k["x"], k["W_ih"], k["W_hh"], k["h0"], h_dev, f, p, keeps, k["g0"], fault="dbhh_n_from_dbih")
    assert worst(bad, ("b_hh",)) > 10.0 and worst(bad, ("dx", "W_ih", "W_hh", "b_ih")) < 1.0
    bad = R.backward(k["dout"], k["x"], k["W_ih"], k["W_hh"], k["h0"], h_dev, f, p, keeps, k["g0"], fault="grad_overwritten")
    for name in ("W_ih", "W_hh", "b_ih", "b_hh"):
        assert worst(bad, (name,)) > 10.0, name
    assert set(R.FAULTS) == {"gates_zr", "bhn_outside", "blend_swapped", "drop_state", "mask_prev_layer", "mask_transposed",
                             "h0_ignored", "bptt_truncated", "dbhh_n_from_dbih", "grad_overwritten"}


def test_allowances_are_the_derived_ones():
    assert (R.EPS, R.U_SIG, R.U_TANH) == (2.0 ** -24, 12.0, 25.0)


# ---------------------------------------------------------------------------------------------------------- fixtures
FIXTURES = [("gru_body_clm_train", 1, [64]), ("gru_body_2layer_clm_train", 2, [96, 64])]
GRU = "heads.0.body.2.module."


def _load(name):
    import golden_utils as gu

    assert os.path.exists(os.path.join(GOLDEN, name + ".npz")), f"{name}.npz is missing (tools/make_gru_golden.py writes it)"
    return gu.load(name)


@pytest.mark.parametrize("name,n,dims", FIXTURES)
def test_restatement_reproduces_the_fixture_within_fp32_bounds(name, n, dims):
    """the reference's fp32 torch.nn.GRU on the CPU: its recorded output and gradients against the restatement on its recorded
    input.  One layer: within the restatement's bounds, step by step from the recorded output (torch's CPU kernels evaluate sig
    and tanh with other expressions of comparable accuracy; the allowances hold for them).  Two layers: the fixture has the last
    layer's output only, so the lower layer is the restated one and the comparison is 1e-5 of the largest magnitude (fp32 sums of
    at most 160 terms); that tolerance is asserted for one layer as well."""
    import golden_utils as gu

    d = _load(name)
    t = gu.t
    W_ih, W_hh = [t(d[f"p/{GRU}weight_ih_l{i}"]) for i in range(n)], [t(d[f"p/{GRU}weight_hh_l{i}"]) for i in range(n)]
    b_ih, b_hh = [t(d[f"p/{GRU}bias_ih_l{i}"]) for i in range(n)], [t(d[f"p/{GRU}bias_hh_l{i}"]) for i in range(n)]
    x, out, dout = t(d["out/gru_in"]), t(d["out/gru_out"]), t(d["out/gru_out_grad"])
    B, L, H = out.shape
    assert (B, L, H) == (8, 20, 64) and x.shape == (8, 20, 64) and int(d["meta/num_layers"]) == n
    keeps = R.keep_masks(0, 0, B, L, H, n, 0.0)
    f = R.forward(x, W_ih, W_hh, b_ih, b_hh, None, 0.0, keeps)
    tol = lambda want: 1e-5 * float(want.abs().max()) + 1e-9  # noqa: E731
    assert (out.double() - f[-1]["h"]).abs().max() < tol(f[-1]["h"])
    if n == 1:
        f = R.forward(x, W_ih, W_hh, b_ih, b_hh, None, 0.0, keeps, h_dev=[out])
        assert R.ratio(out, f[0]["h"], f[0]["Bh"]) < 1.0
    hs = [lay["h"] for lay in f[:-1]] + [out]
    g = R.backward(dout, x, W_ih, W_hh, None, hs, f, 0.0, keeps)
    assert (t(d["out/gru_in_grad"]).double() - g["dx"][0]).abs().max() < tol(g["dx"][0])
    if n == 1:
        assert R.ratio(t(d["out/gru_in_grad"]), *g["dx"]) < 1.0
    for i in range(n):
        for mine, theirs in (("W_ih", "weight_ih"), ("W_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh")):
            got = t(d[f"g/{GRU}{theirs}_l{i}"])
            if n == 1:
                assert R.ratio(got, *g[mine][i]) < 1.0, (mine, i)
            assert (got.double() - g[mine][i][0]).abs().max() < tol(g[mine][i][0]), (mine, i)
            assert float(got.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------- module and model
def _model(n, dims, V=50, width=48, L=20):
    feats = tr.TabularSequenceFeatures.from_schema(tr.session_schema(V, L), max_sequence_length=L, masking="clm",
                                                   aggregation="concat", embedding_dims={"item_id": width})
    return tr.Model(feats, GRUBlock(dims[-1], 64, num_layers=n), tr.NextItemPredictionTask(weight_tying=True),
                    mlp_block=tr.MLPBlock(dims))


@pytest.mark.parametrize("name,n,dims", FIXTURES)
def test_state_dict_keys_of_a_model_equal_the_fixtures(name, n, dims):
    d = _load(name)
    want = str(d["meta/state_dict_keys"]).split("\n")
    model = _model(n, dims)
    own = model.state_dict()
    assert sorted(own.keys()) == sorted(want)
    assert "heads.0.body.2.module.weight_ih_l0" in want
    for key, v in own.items():
        if "p/" + key in d:                                  # a tensor under several names is stored once
            assert tuple(v.shape) == tuple(d["p/" + key].shape), key
    assert all("p/" + key in d for key in own if ".body.2." in key or ".body.1." in key)
    assert model.transformer_block is model.heads[0].body[2] and isinstance(model.transformer_block, GRUBlock)
    from transformers4rec_amd.model import last_rows_gate
    assert last_rows_gate(model, True, 8, 20, n_labels=4) is None


def test_names_shapes_and_initialisation():
    torch.manual_seed(5)
    b = GRUBlock(48, 100, num_layers=3, bias=True, dropout=0.2)
    torch.manual_seed(5)
    ref = torch.nn.GRU(48, 100, num_layers=3, bias=True, batch_first=True, dropout=0.2)
    assert [k for k, _ in b.module.named_parameters()] == [k for k, _ in ref.named_parameters()]
    for (k, p), (_, q) in zip(b.module.named_parameters(), ref.named_parameters()):
        assert p.shape == q.shape and torch.equal(p, q), k                 # torch's order of creation and of draws
        assert 0.09 < float(p.detach().abs().max()) <= 0.1, k
    assert list(b.state_dict().keys())[0] == "module.weight_ih_l0"
    assert b._t4r_hip and b.seed != tr.MLPBlock([4]).build([1, 1, 4]).seed and b._drop_offset == 0
    assert b.output_size([8, 20, 48]) == torch.Size([8, 20, 100])
    assert not GRUBlock(8, 8, bias=False).state_dict().keys() & {"module.bias_ih_l0", "module.bias_hh_l0"}
    assert {id(p) for p in tr.hip_parameters(b)} == {id(p) for p in b.parameters()}
    for kw in (dict(hidden_size=129), dict(hidden_size=0), dict(num_layers=5), dict(num_layers=0), dict(input_size=1025)):
        args = dict(input_size=8, hidden_size=8, num_layers=1)
        args.update(kw)
        with pytest.raises(NotImplementedError, match="fused recurrence"):
            GRUBlock(**args)
    with pytest.raises(ValueError, match="dropout"):
        GRUBlock(8, 8, dropout=1.0)


def test_block_converts_a_gru_and_refuses_what_has_no_hip_path():
    gru = torch.nn.GRU(12, 16, num_layers=2, batch_first=True, dropout=0.25)
    blk = Block(gru, [None, 20, 16])
    assert isinstance(blk, GRUBlock) and (blk.input_size, blk.hidden_size, blk.num_layers, blk.bias, blk.dropout) == (12, 16, 2, True, 0.25)
    for name, p in gru.named_parameters():
        assert torch.equal(getattr(blk.module, name), p) and getattr(blk.module, name) is not p
    assert tr.Block is Block and tr.GRUBlock is GRUBlock
    with pytest.raises(NotImplementedError, match="batch_first"):
        Block(torch.nn.GRU(12, 16), [None, 20, 16])
    with pytest.raises(NotImplementedError, match="future"):
        Block(torch.nn.GRU(12, 16, batch_first=True, bidirectional=True))
    with pytest.raises(NotImplementedError, match="only torch.nn.GRU"):
        Block(torch.nn.LSTM(12, 16, batch_first=True))
    with pytest.raises(NotImplementedError, match="only torch.nn.GRU"):
        Block(torch.nn.Linear(12, 16))
    fake = torch.nn.GRU(12, 16, batch_first=True)
    fake.proj_size = 4
    with pytest.raises(NotImplementedError, match="proj_size"):
        Block(fake)


def test_model_refusals_and_the_functional_guard():
    def feats():
        return tr.TabularSequenceFeatures.from_schema(tr.session_schema(50, 20), max_sequence_length=20, masking="mlm",
                                                      aggregation="concat", embedding_dims={"item_id": 64})
    model = tr.Model(feats(), GRUBlock(64, 32), tr.NextItemPredictionTask(weight_tying=False))     # any masking, no MLP stack
    assert [k for k in model.state_dict() if ".body.1." in k][0] == "heads.0.body.1.module.weight_ih_l0"
    from transformers4rec_amd import functional
    with pytest.raises(NotImplementedError, match="GRUBlock"):
        functional.config_of(model)
    with pytest.raises(NotImplementedError, match="post_context_module"):
        tr.Model(feats(), GRUBlock(64, 32), tr.NextItemPredictionTask(weight_tying=False), post_context_module=feats())
    with pytest.raises(ValueError, match="mlp_block maps"):
        tr.Model(feats(), GRUBlock(32, 32), tr.NextItemPredictionTask(weight_tying=False), mlp_block=tr.MLPBlock([48]))


# ---------------------------------------------------------------------------------------------------------- operators
def test_operator_fakes_give_the_right_shapes():
    for name in ("gru_fwd", "gru_bwd"):
        assert name in torch_ops.OPERATORS
        assert str(getattr(torch.ops.t4r_hip, name).default._schema).startswith(f"t4r_hip::{name}(")
    H, K0, n = 12, 5, 2
    with torch._subclasses.FakeTensorMode():
        x = torch.empty(3, 7, K0)
        Wi, Wh = [torch.empty(3 * H, K0), torch.empty(3 * H, H)], [torch.empty(3 * H, H) for _ in range(n)]
        bi, bh = [torch.empty(3 * H) for _ in range(n)], [torch.empty(3 * H) for _ in range(n)]
        out = torch.ops.t4r_hip.gru_fwd(x, Wi, Wh, bi, bh, 0.1, 1, 2)
        assert tuple(out.shape) == (3, 7, H)
        assert tuple(torch.ops.t4r_hip.gru_fwd(x, Wi, Wh, [], [], 0.0, 0, 0).shape) == (3, 7, H)
        g = torch.ops.t4r_hip.gru_bwd(out, x, Wi, Wh, bi, bh, 0.1, 1, 2)
        assert [tuple(t.shape) for t in g] == [(3, 7, K0)] + [tuple(w.shape) for w in Wi + Wh + bi + bh]
        assert len(torch.ops.t4r_hip.gru_bwd(out, x, Wi, Wh, [], [], 0.0, 0, 0)) == 1 + 2 * n
