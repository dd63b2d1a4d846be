"""Host half of the row-sparse (lazy) Adam step: the eighth C-ABI header (include/t4r_hip_rowadam.h), its size query and
argument checks, and what ops.row_adam_step_, optim.RowSparseAdam and optim.row_sparse_tables do without a device.  Nothing here
needs a GPU."""
import ctypes
import os
import re

import pytest
import torch

from transformers4rec_amd import _lib, ops, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = (1e-3, 0.9, 0.999, 1e-8, 0.01)


# ---------------------------------------------------------------------------------------------------------- header and ABI
def test_rowadam_header_library_and_prototypes_agree():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_rowadam.h")
    assert syms == ["t4r_row_adam_step", "t4r_row_adam_ws_bytes"]
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_rowadam.h but not exported"
    text = open(_lib.header_path("t4r_hip_rowadam.h")).read()
    decl = text[: text.index("int t4r_row_adam_step(void* stream")]
    comment = decl[decl.rindex("/*"):]
    assert "replaces:" in comment and "torch.optim.Adam.step" in comment and "Model.fit" in comment
    decls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in decls, f"{word} leaked into the C ABI"


def test_ws_bytes_is_pure_and_monotone():
    lib = _lib.load()
    assert [lib.t4r_row_adam_ws_bytes(n, 64) for n in (-3, 0)] == [0, 0]
    assert lib.t4r_row_adam_ws_bytes(100, 0) == 0 and lib.t4r_row_adam_ws_bytes(100, -1) == 0
    for D in (1, 6, 64, 256, 300):
        ns = [1, 2, 15, 16, 17, 255, 256, 257, 5000, 66_200, 131_071, 131_072, 262_143, 262_144, 262_145, 1 << 20, (1 << 20) + 1,
              3_000_000]
        got = [lib.t4r_row_adam_ws_bytes(n, D) for n in ns]
        assert got == [lib.t4r_row_adam_ws_bytes(n, D) for n in ns]                 # the same answer when asked again
        assert got == sorted(got) and got[0] > 0, (D, got)
        # room for the compact [n, D] gradient and the four index arrays at the least
        assert all(b >= n * D * 4 + 4 * n * 4 for n, b in zip(ns, got))
    dense = [lib.t4r_row_adam_ws_bytes(n, 20) for n in range(1, 3000, 7)]
    assert dense == sorted(dense)


def test_argument_errors_come_back_as_messages():
    lib = _lib.load()
    err = lib.t4r_last_error
    one = ctypes.c_void_p(256)                # non-null, never dereferenced: every call below returns before any launch

    def step(p=one, m=one, v=one, V=10, D=4, keys=one, perm=one, rows=one, ld=4, n=8, t=1, ws=one, ws_bytes=1 << 30):
        return lib.t4r_row_adam_step(None, p, m, v, V, D, keys, perm, rows, ld, n, t, *HP, 0, 1.0, ws, ws_bytes)

    assert step(n=-1) < 0 and b"row_adam: n must not be negative" in err()
    assert step(D=0) < 0 and b"row_adam: D must be at least 1" in err()
    assert step(V=0) < 0 and b"row_adam: V must be at least 1" in err()
    assert step(t=0) < 0 and b"row_adam: step is 1-based" in err()
    assert step(n=0, D=0) < 0 and step(n=0, V=0) < 0 and step(n=0, t=0) < 0       # checked even when there is nothing to do
    assert step(None, None, None, keys=None, perm=None, rows=None, ws=None, n=0) == 0          # n = 0: nothing launches
    for which in ("p", "m", "v", "keys", "perm", "rows", "ws"):
        assert step(**{which: None}) < 0 and b"row_adam: null pointer" in err(), which
    assert step(ld=3) < 0 and b"ld_grad must be at least D" in err()
    assert step(p=ctypes.c_void_p(258)) < 0 and b"4-byte aligned" in err()
    assert step(ws=ctypes.c_void_p(264)) < 0 and b"workspace must be 16-byte aligned" in err()
    need = lib.t4r_row_adam_ws_bytes(8, 4)
    assert step(ws_bytes=need - 1) < 0 and b"row_adam: workspace too small" in err()
    assert step(ws_bytes=0) < 0 and b"workspace too small" in err()
    assert step(n=(1 << 31) - 1) < 0 and b"n must fit 31 bits" in err()


# ---------------------------------------------------------------------------------------------------------- host layer
def _table(V=12, D=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.Parameter(torch.randn(V, D, generator=g))


def test_host_tensors_raise():
    p = _table()
    m, v = torch.zeros_like(p.data), torch.zeros_like(p.data)
    with pytest.raises(_lib.T4RHipError):
        ops.row_adam_step_(p.data, m, v, torch.tensor([1, 2]), torch.ones(2, 4), 1)
    opt = optim.RowSparseAdam([p])
    opt.add_rows(p, torch.tensor([1, 2]), torch.ones(2, 4))
    before = p.detach().clone()
    with pytest.raises(_lib.T4RHipError):
        opt.step()
    assert torch.equal(p.detach(), before)


def test_constructor_refuses_what_is_not_a_table():
    with pytest.raises(ValueError):
        optim.RowSparseAdam([])
    with pytest.raises(ValueError):
        optim.RowSparseAdam([torch.nn.Parameter(torch.zeros(5))])
    with pytest.raises(ValueError):
        optim.RowSparseAdam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError):
        optim.RowSparseAdam([torch.nn.Parameter(torch.zeros(4, 6, dtype=torch.float64))])
    p = _table()
    assert len(optim.RowSparseAdam([p, p]).params) == 1


def test_attach_detach_and_a_second_sink():
    from transformers4rec_amd.distributed import SparseRowExchange

    a, b = _table(), _table(seed=1)
    opt = optim.RowSparseAdam([a, b])
    assert opt.attach() is opt and a._t4r_sparse_sink is opt and b._t4r_sparse_sink is opt
    opt.attach()                                                 # its own tables again: fine
    opt.detach()
    assert not hasattr(a, "_t4r_sparse_sink") and not hasattr(b, "_t4r_sparse_sink")
    other = SparseRowExchange(apply_fn=lambda *a: None).attach(b)
    with pytest.raises(RuntimeError):
        opt.attach()
    assert not hasattr(a, "_t4r_sparse_sink") and b._t4r_sparse_sink is other      # nothing half-attached
    opt.detach()
    assert b._t4r_sparse_sink is other                           # detach removes only its own
    SparseRowExchange.detach(b)


def test_add_and_add_rows_collect_and_zero_grad_clears():
    p = _table(V=12, D=4)
    opt = optim.RowSparseAdam([p])
    ids = torch.tensor([[1, 0, 3], [3, 5, 0]])
    rows = torch.arange(24.0).view(6, 4)
    opt.add(p, ids, rows, 0, 4, 1, 0)                            # W == dim, ids_div 1: the rows as they are, no kernel needed
    opt.add_rows(p, torch.tensor([7, 7]), torch.ones(2, 4))
    assert len(opt._pending) == 2
    tab, i0, r0, pad0 = opt._pending[0]
    assert tab is p and i0.tolist() == [1, 0, 3, 3, 5, 0] and r0 is rows and pad0 == 0
    assert opt._pending[1][3] == -1
    with pytest.raises(ValueError):
        opt.add_rows(_table(seed=3), torch.tensor([1]), torch.ones(1, 4))
    opt.zero_grad()
    assert opt._pending == [] and opt.step_count == 0
    opt.step()                                                   # nothing pending: nothing to launch, the step still counts
    assert opt.step_count == 1


def test_state_dict_round_trip():
    a, b = _table(), _table(V=5, D=3, seed=1)
    opt = optim.RowSparseAdam([a, b], lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1, decoupled_weight_decay=True)
    opt.set_schedule(optim.warmup_schedule("constant_with_warmup", 4))
    opt.state[0][0].fill_(0.5)
    opt.state[1][1].fill_(0.25)
    opt.step_count = 17
    sd = opt.state_dict()
    assert sd["step_count"] == 17 and sd["hyper"] == {"lr": 2e-3, "betas": (0.8, 0.99), "eps": 1e-6, "weight_decay": 0.1,
                                                      "decoupled_weight_decay": True}
    assert sd["state"][0]["exp_avg"].data_ptr() != opt.state[0][0].data_ptr()        # copies, not views
    opt.state[0][0].zero_()
    assert float(sd["state"][0]["exp_avg"][0, 0]) == 0.5
    fresh = optim.RowSparseAdam([a, b])
    fresh.load_state_dict(sd)
    assert fresh.step_count == 17 and fresh.base_lr == fresh.lr == 2e-3 and fresh.betas == (0.8, 0.99) and fresh.eps == 1e-6
    assert fresh.weight_decay == 0.1 and fresh.decoupled_weight_decay is True
    assert torch.equal(fresh.state[0][0], sd["state"][0]["exp_avg"]) and torch.equal(fresh.state[1][1], sd["state"][1]["exp_avg_sq"])
    assert fresh.state[0][0].data_ptr() != sd["state"][0]["exp_avg"].data_ptr()
    with pytest.raises(ValueError):
        optim.RowSparseAdam([a]).load_state_dict(sd)
    with pytest.raises(ValueError):
        optim.RowSparseAdam([b, a]).load_state_dict(sd)
    # the schedule scales the constructor's lr as FusedAdam's does: the step that makes step_count t runs at base_lr * f(t - 1)
    sch = optim.RowSparseAdam([a], lr=1.0).set_schedule(optim.warmup_schedule("constant_with_warmup", 4))
    seen = []
    for _ in range(6):
        sch.step()
        seen.append(sch.lr)
    assert seen == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0]


def test_world_one_exchange_delivers_into_the_pending_list():
    from transformers4rec_amd.distributed import GradReducer, SparseRowExchange

    p = _table(V=9, D=3)
    opt = optim.RowSparseAdam([p])
    ex = SparseRowExchange(grad_of=lambda tab: tab, apply_fn=lambda tab, ids, rows, pad: opt.add_rows(tab, ids, rows, pad))
    ex.attach(p)
    with pytest.raises(RuntimeError):
        opt.attach()                                             # the exchange is the table's sink; the optimizer is behind it
    ids1, rows1 = torch.tensor([1, 0, 1, 8]), torch.ones(4, 3)
    ids2, rows2 = torch.tensor([2]), torch.full((1, 3), 2.0)
    ex.add_rows(p, ids1, rows1, padding_idx=0)
    ex.add_rows(p, ids2, rows2)
    assert opt._pending == []
    GradReducer(torch.zeros(2), None, sparse=ex).reduce_all()
    assert [(t is p, i.tolist(), pad) for t, i, r, pad in opt._pending] == [(True, [1, 0, 1, 8], 0), (True, [2], -1)]
    assert torch.equal(opt._pending[0][2], rows1) and torch.equal(opt._pending[1][2], rows2)
    assert p.grad is None                                        # nothing dense was created on the way
    SparseRowExchange.detach(p)


# ---------------------------------------------------------------------------------------------------------- which tables
def _model(weight_tying, sampled, cats=()):
    import transformers4rec_amd as tr

    V, L = 50, 6
    schema = tr.session_schema(V - 1, L, cats, ())
    torch.manual_seed(0)
    inputs = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="clm", aggregation="concat",
                                                    embedding_dim_default=16, d_output=16 if cats else None)
    cfg = tr.GPT2Config.build(dropout=0.0, d_model=16, n_head=2, n_layer=1, total_seq_length=L)
    return cfg.to_torch_model(inputs, tr.NextItemPredictionTask(weight_tying=weight_tying, sampled_softmax=sampled, max_n_samples=10))


def test_row_sparse_tables_leaves_out_what_gets_a_dense_gradient():
    def names(model):
        return [n for n, _ in optim.row_sparse_tables(model)]

    def all_tables(model):
        return [n for n, p in model.named_parameters() if optim._is_table(n, p)]

    tied_full = _model(True, False, cats=(("category", 7),))
    item = [n for n in all_tables(tied_full) if "item_id" in n]
    assert len(item) == 1 and len(all_tables(tied_full)) == 2
    assert names(tied_full) == [n for n in all_tables(tied_full) if n not in item]          # the tied item table is out
    tied_sampled = _model(True, True, cats=(("category", 7),))
    assert names(tied_sampled) == all_tables(tied_sampled) and len(names(tied_sampled)) == 2
    untied_full = _model(False, False)
    assert [n for n in all_tables(untied_full) if n.endswith("output_layer")] and not [n for n in names(untied_full) if n.endswith("output_layer")]
    assert [n for n in names(untied_full) if "item_id" in n]                                # its item table only feeds lookups
    untied_sampled = _model(False, True)
    assert names(untied_sampled) == all_tables(untied_sampled) and any(n.endswith("output_layer") for n in names(untied_sampled))
    # the recipe of the class docstring: the two sets partition the parameters, and flatten_model's table bucket is the union
    sparse = dict(optim.row_sparse_tables(tied_sampled))
    dense = optim.FlatParams((n, p) for n, p in tied_sampled.named_parameters() if n not in sparse)
    assert not {n for n, _, _ in dense.entries} & set(sparse)
    assert len(dense.entries) + len(sparse) == len(list(tied_sampled.named_parameters()))


# ---------------------------------------------------------------------------------------------------------- documents
def test_documents_name_the_new_surface():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "t4r_hip_rowadam.h" in readme and re.search(r"\b2 row-sparse optimizer entry points", readme)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("t4r_row_adam_step", "t4r_row_adam_ws_bytes", "RowSparseAdam", "row_sparse_tables", "t4r_hip_rowadam.h", "lazy",
                 "opt.add_rows(tab, ids, rows, pad)"):
        assert word in integ, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.8" in design and "row_adam.hip" in design and "seg_sum_kernel.h" in design
    doc = optim.RowSparseAdam.__doc__
    assert "row_sparse_tables(model)" in doc and "max_grad_norm" in doc and "out of scope" in doc
    assert "row_adam.hip" in open(os.path.join(ROOT, "transformers4rec_amd", "build.py")).read()
