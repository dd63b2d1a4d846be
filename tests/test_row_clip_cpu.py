"""Host half of global-norm clipping across dense buckets and row-sparse tables: the tenth C-ABI header
(include/t4r_hip_rowclip.h), its count query and argument checks, and what ops.row_adam_reduce_ / row_adam_apply_ and the linked
pair optim.FusedAdam(...).link(optim.RowSparseAdam) do without a device.  Nothing here needs a GPU."""
import ctypes
import os
import re

import pytest
import torch

from transformers4rec_amd import _lib, ops, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = (1e-3, 0.9, 0.999, 1e-8, 0.01)
NAMES = ["t4r_row_adam_apply", "t4r_row_adam_reduce", "t4r_row_grad_sumsq_parts"]


# ---------------------------------------------------------------------------------------------------------- header and ABI
def test_rowclip_header_library_and_prototypes_agree():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_rowclip.h")
    assert syms == NAMES
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_rowclip.h but not exported"
    text = open(_lib.header_path("t4r_hip_rowclip.h")).read()
    for name, ret, words in (("t4r_row_adam_reduce", "int", ("clip_grad_norm_", "trainer.py")),
                             ("t4r_row_adam_apply", "int", ("torch.optim.AdamW.step", "trainer.py"))):
        decl = text[: text.index(f"{ret} {name}(void* stream")]
        comment = decl[decl.rindex("/*"):]
        assert "replaces:" in comment and all(w in comment for w in words), name
    decls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in decls, f"{word} leaked into the C ABI"


def test_parts_is_pure_monotone_and_capped():
    lib = _lib.load()
    f = lib.t4r_row_grad_sumsq_parts
    assert [f(n, 64) for n in (-3, 0)] == [0, 0]
    assert f(100, 0) == 0 and f(100, -1) == 0
    for D in (1, 3, 4, 130, 256):
        ns = [1, 2, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 5000, 65_536, 1 << 20, (1 << 20) + 1, 3_000_000, (1 << 31) - 2]
        got = [f(n, D) for n in ns]
        assert got == [f(n, D) for n in ns]                                    # the same answer when asked again
        assert got == sorted(got) and got[0] == 1 and got[-1] <= 2048, (D, got)
        assert got == [lib.t4r_grad_sumsq_parts(n * D) for n in ns]            # the count of a flat bucket of n * D elements
    assert f(65_536, 128) == 2048 and f(65_535, 128) == 2048
    dense = [f(n, 20) for n in range(1, 3000, 7)]
    assert dense == sorted(dense)
    assert ops.row_grad_sumsq_parts(5000, 130) == f(5000, 130) == (5000 * 130 // 4 + 255) // 256


def test_argument_errors_come_back_as_messages():
    lib = _lib.load()
    err = lib.t4r_last_error
    one = ctypes.c_void_p(256)                # non-null, never dereferenced: every call below returns before any launch

    def reduce(V=10, D=4, keys=one, perm=one, rows=one, ld=4, n=8, ws=one, ws_bytes=1 << 30, part=one):
        return lib.t4r_row_adam_reduce(None, V, D, keys, perm, rows, ld, n, ws, ws_bytes, part)

    def apply(p=one, m=one, v=one, V=10, D=4, n=8, t=1, coef=None, ws=one, ws_bytes=1 << 30):
        return lib.t4r_row_adam_apply(None, p, m, v, V, D, n, t, *HP, 0, 1.0, coef, ws, ws_bytes)

    need = lib.t4r_row_adam_ws_bytes(8, 4)
    assert reduce(n=-1) < 0 and b"row_adam_reduce: n must not be negative" in err()
    assert reduce(D=0) < 0 and b"row_adam_reduce: D must be at least 1" in err()
    assert reduce(V=0) < 0 and b"row_adam_reduce: V must be at least 1" in err()
    assert reduce(n=0, D=0) < 0 and reduce(n=0, V=0) < 0                          # checked even when there is nothing to do
    assert reduce(keys=None, perm=None, rows=None, ws=None, part=None, n=0) == 0   # n = 0: nothing launches
    for which in ("keys", "perm", "rows", "ws", "part"):
        assert reduce(**{which: None}) < 0 and b"row_adam_reduce: null pointer" in err(), which
    assert reduce(ld=3) < 0 and b"ld_grad must be at least D" in err()
    assert reduce(rows=ctypes.c_void_p(258)) < 0 and b"grad_rows must be 4-byte aligned" in err()
    assert reduce(ws=ctypes.c_void_p(264)) < 0 and b"row_adam_reduce: the workspace must be 16-byte aligned" in err()
    assert reduce(part=ctypes.c_void_p(260)) < 0 and b"row_adam_reduce: part must be 8-byte aligned" in err()
    assert reduce(ws_bytes=need - 1) < 0 and b"row_adam_reduce: workspace too small" in err()
    assert reduce(n=(1 << 31) - 1) < 0 and b"n must fit 31 bits" in err()

    assert apply(n=-1) < 0 and b"row_adam_apply: n must not be negative" in err()
    assert apply(D=0) < 0 and b"row_adam_apply: D must be at least 1" in err()
    assert apply(V=0) < 0 and b"row_adam_apply: V must be at least 1" in err()
    assert apply(t=0) < 0 and b"row_adam_apply: step is 1-based" in err()
    assert apply(n=0, D=0) < 0 and apply(n=0, V=0) < 0 and apply(n=0, t=0) < 0
    assert apply(None, None, None, ws=None, n=0) == 0
    for which in ("p", "m", "v", "ws"):
        assert apply(**{which: None}) < 0 and b"row_adam_apply: null pointer" in err(), which
    assert apply(p=ctypes.c_void_p(258)) < 0 and b"row_adam_apply: buffers must be 4-byte aligned" in err()
    assert apply(coef=ctypes.c_void_p(258)) < 0 and b"row_adam_apply: clip_coef must be 4-byte aligned" in err()
    assert apply(ws=ctypes.c_void_p(264)) < 0 and b"row_adam_apply: the workspace must be 16-byte aligned" in err()
    assert apply(ws_bytes=need - 1) < 0 and b"row_adam_apply: workspace too small" in err()
    assert apply(ws_bytes=0) < 0 and b"workspace too small" in err()
    assert apply(n=(1 << 31) - 1) < 0 and b"n must fit 31 bits" in err()


# ---------------------------------------------------------------------------------------------------------- host layer
def _table(V=12, D=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.Parameter(torch.randn(V, D, generator=g))


def _dense(n=8):
    return optim.FlatParams([("w", torch.nn.Parameter(torch.ones(n)))])


def test_host_tensors_raise():
    p = _table()
    m, v = torch.zeros_like(p.data), torch.zeros_like(p.data)
    part = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(_lib.T4RHipError):
        ops.row_adam_reduce_(torch.tensor([1, 2]), torch.ones(2, 4), 12, -1, part)
    with pytest.raises(_lib.T4RHipError):
        ops.row_adam_apply_(p.data, m, v, ops.RowAdamReduced(None, 0, 0, 12, 4), 1)
    opt_s = optim.RowSparseAdam([p])
    opt_d = optim.FusedAdam([_dense()], max_grad_norm=1.0).link(opt_s)
    opt_s.add_rows(p, torch.tensor([1, 2]), torch.ones(2, 4))
    before = p.detach().clone()
    with pytest.raises(_lib.T4RHipError):
        opt_d.step()
    assert torch.equal(p.detach(), before)


def test_a_linked_row_sparse_step_raises_and_the_link_is_checked():
    a, b = _table(), _table(seed=1)
    opt_s = optim.RowSparseAdam([a, b])
    assert opt_s._linked is None
    opt_d = optim.FusedAdam([_dense()], max_grad_norm=1.0).link(opt_s)
    assert opt_d.row_sparse is opt_s and opt_s._linked is opt_d
    with pytest.raises(RuntimeError, match="stepped through the FusedAdam"):
        opt_s.step()
    assert opt_s.step_count == 0                                  # nothing advanced
    assert opt_d.link(opt_s) is opt_d                             # its own again: fine
    other = optim.FusedAdam([_dense()])
    with pytest.raises(RuntimeError):
        other.link(opt_s)                                         # one FusedAdam per RowSparseAdam
    assert other.row_sparse is None and opt_s._linked is opt_d
    with pytest.raises(RuntimeError):
        opt_d.link(optim.RowSparseAdam([b]))                      # ... and one RowSparseAdam per FusedAdam
    for bad in (None, object(), "tables", [opt_s], other, a):
        with pytest.raises(TypeError):
            optim.FusedAdam([_dense()], max_grad_norm=1.0).link(bad)
    assert optim.FusedAdam([_dense()]).row_sparse is None         # the default: nothing linked, step() as ever


def test_linked_step_advances_both_counts_and_schedules():
    """nothing pending and no clip: no kernel of the tables is launched, yet both step counts and both schedules advance --
    each object its own"""
    p = _table()
    opt_s = optim.RowSparseAdam([p], lr=1.0).set_schedule(optim.warmup_schedule("constant_with_warmup", 4))
    opt_s.step_count = 2
    opt_d = optim.FusedAdam([_dense()], lr=3.0).link(opt_s)
    assert opt_d.max_grad_norm is None
    try:
        opt_d.step()
    except _lib.T4RHipError:                                      # the dense bucket's launch: there is no CPU path
        pass
    assert opt_d.step_count == 1 and opt_s.step_count == 3 and opt_s.lr == 0.5 and opt_d.lr == 3.0


def test_state_dicts_stay_separate_and_round_trip():
    a = _table()
    opt_s = optim.RowSparseAdam([a], lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1, decoupled_weight_decay=True)
    opt_d = optim.FusedAdam([_dense()], lr=5e-3, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=0.5).link(opt_s)
    opt_s.add_rows(a, torch.tensor([1]), torch.ones(1, 4))
    opt_s.state[0][0].fill_(0.5)
    opt_d.state[0][1].fill_(0.25)
    opt_s.step_count, opt_d.step_count = 17, 19
    sd_s, sd_d = opt_s.state_dict(), opt_d.state_dict()
    assert sorted(sd_s) == sorted(sd_d) == ["hyper", "state", "step_count"]           # neither pending rows nor the link
    assert sd_s["hyper"] == {"lr": 2e-3, "betas": (0.8, 0.99), "eps": 1e-6, "weight_decay": 0.1, "decoupled_weight_decay": True}
    assert sd_d["hyper"] == {"lr": 5e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.01, "max_grad_norm": 0.5,
                             "decoupled_weight_decay": True}
    assert len(sd_d["state"]) == 1 and sd_d["state"][0]["exp_avg"].shape == (8,) and sd_s["state"][0]["exp_avg"].shape == (12, 4)
    fresh_s = optim.RowSparseAdam([a])
    fresh_d = optim.FusedAdam([_dense()]).link(fresh_s)
    fresh_s.load_state_dict(sd_s)
    fresh_d.load_state_dict(sd_d)
    assert fresh_s.step_count == 17 and fresh_d.step_count == 19 and fresh_d.max_grad_norm == 0.5 and fresh_s.base_lr == 2e-3
    assert torch.equal(fresh_s.state[0][0], sd_s["state"][0]["exp_avg"]) and torch.equal(fresh_d.state[0][1], sd_d["state"][0]["exp_avg_sq"])
    assert fresh_s._pending == [] and fresh_s._linked is fresh_d and fresh_d.row_sparse is fresh_s       # the link survives a load
    unlinked = optim.RowSparseAdam([a])
    unlinked.load_state_dict(sd_s)
    assert unlinked._linked is None                                                   # ... and does not come with one


# ---------------------------------------------------------------------------------------------------------- documents
def test_documents_name_the_new_surface():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "the 3 row-sparse clipping entry points of `include/t4r_hip_rowclip.h`" in readme
    assert readme.count("t4r_hip_rowclip.h") >= 2                                     # the first paragraph and the layout list
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in NAMES + ["t4r_hip_rowclip.h", "row_adam_reduce_", "row_adam_apply_", ".link(opt_s)", "t4r_row_adam_ws_bytes"]:
        assert word in integ, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.10" in design and "row_sumsq_kernel" in design and "sumsq_kernel.h" in design and "t4r_hip_rowclip.h" in design
    doc = optim.RowSparseAdam.__doc__
    assert ".link(" in doc and "max_grad_norm" in doc and "No gradient clipping" not in doc
    doc = optim.FusedAdam.__doc__
    assert "link(opt_s)" in doc and "reduce_all" in doc and "same coefficient bits" in doc
    assert "t4r_hip_rowclip.h" in open(os.path.join(ROOT, "transformers4rec_amd", "build.py")).read()
