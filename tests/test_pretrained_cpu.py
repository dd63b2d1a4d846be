"""CPU checks of the pretrained-embedding feature: the fifth header against the library, the pure size queries, the argument
limits (refused before any launch: these run without a GPU), the module mirror's construction and refusals, and its state-dict
names against the reference classes built live (oracle/ref_standins.py)."""
import ctypes
import os

import pytest
import torch

import transformers4rec_amd as tr
from transformers4rec_amd import _lib, features as F, ops

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_header_symbols_match_the_ctypes_table_and_are_exported():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_pretrained.h")
    assert len(syms) == 4
    for s in syms:
        assert hasattr(lib, s), s
    assert not set(syms) & set(_lib.header_symbols()), "the pretrained entries stay out of t4r_hip.h"


def test_workspace_queries_are_pure_and_monotone():
    lib = _lib.load()
    f, g = lib.t4r_pretrained_proj_ws_bytes, lib.t4r_pretrained_proj_bwd_ws_floats
    assert f(768, 64) == f(768, 64) == 256 + 2 * 48 * 2048
    assert f(1, 1) == 256 + 2048 and f(1024, 256) == 256 + 8 * 64 * 2048
    assert f(0, 8) == 0 and f(1025, 8) == 0 and f(8, 257) == 0 and f(8, 0) == 0
    prev = 0
    for E in (1, 15, 16, 17, 40, 272, 768, 1024):
        assert f(E, 64) >= prev
        prev = f(E, 64)
    prev = 0
    for P in (1, 24, 32, 33, 64, 256):
        assert f(768, P) >= prev
        prev = f(768, P)
    assert g(300, 40, 24) == g(300, 40, 24) == 5 * 32 * 128 + 300 * 24 + 5 * 6 * 24
    assert g(20480, 768, 64) == 128 * 64 * 768 + 20480 * 64 + 128 * 6 * 64
    for args in ((0, 40, 24), (1, 40, 24)):
        assert g(*args) > 0
    assert g(10, 0, 24) == 0 and g(10, 40, 257) == 0 and g(-1, 40, 24) == 0
    prev = 0
    for T in (0, 1, 63, 64, 65, 129, 300, 2000, 2048, 2049, 20480, 100000):
        assert g(T, 272, 64) >= prev, T
        prev = g(T, 272, 64)
    for a, b in (((300, 40, 24), (300, 41, 24)), ((300, 40, 24), (300, 40, 25)), ((300, 128, 32), (300, 129, 33))):
        assert g(*a) <= g(*b)


def _fwd(lib, E, P, dtype=3, image=1 << 20, ldp=None, T=4):
    ldp = (E + 15) // 16 * 16 if ldp is None else ldp
    buf = 1 << 20       # never dereferenced: every case below is refused before any launch
    return lib.t4r_pretrained_proj_fwd(None, dtype, image, ldp, 10, buf, T, 1, buf, buf, None, None, 1e-5, E, P, buf, P, 0, None,
                                       None, buf, None)


def _bwd(lib, E, P, dtype=3, image=1 << 20, ldp=None, T=4):
    ldp = (E + 15) // 16 * 16 if ldp is None else ldp
    buf = 1 << 20
    return lib.t4r_pretrained_proj_bwd(None, dtype, image, ldp, 10, buf, T, 1, buf, P, 0, None, None, None, E, P, buf, buf, None,
                                       None, buf)


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_argument_limits_are_refused_before_any_launch(call):
    lib = _lib.load()
    for kw, word in ((dict(E=0, P=8), b"E <= 1024"), (dict(E=1025, P=8), b"E <= 1024"), (dict(E=40, P=257), b"P <= 256"),
                     (dict(E=40, P=0), b"P <= 256"), (dict(E=40, P=8, dtype=2), b"bf16"), (dict(E=40, P=8, dtype=0), b"dtype"),
                     (dict(E=40, P=8, image=(1 << 20) + 8), b"16-byte aligned"), (dict(E=40, P=8, ldp=40), b"16-byte aligned"),
                     (dict(E=40, P=8, ldp=52), b"16-byte aligned"), (dict(E=40, P=8, T=-1), b"T")):
        rc = call(lib, **kw)
        assert rc < 0, kw
        assert word in lib.t4r_last_error(), (kw, lib.t4r_last_error())


def test_ops_wrappers_refuse_cpu_tensors():
    image = torch.zeros(8, 48, dtype=torch.float16)[:, :40]
    ids = torch.zeros(4, dtype=torch.int64)
    W, b = torch.zeros(8, 40), torch.zeros(8)
    with pytest.raises(_lib.T4RHipError):
        ops.pretrained_proj_fwd(image, ids, W, b)
    with pytest.raises(_lib.T4RHipError):
        ops.pretrained_proj_bwd(torch.zeros(4, 8), image, ids, None, None, None, torch.zeros(8, 40), torch.zeros(8))


def _schema(L=10, V=50, E=40):
    return tr.session_schema(V, L, categoricals=(("category", 7),)) + tr.Schema(
        [tr.ColumnSchema("item_vec", [tr.Tags.EMBEDDING, tr.Tags.LIST], embedding_dim=E)])


def test_module_construction_order_offsets_and_sizes():
    pt = tr.PretrainedEmbeddingFeatures(["txt", "img"], {"txt": 40, "img": 16}, pretrained_output_dims={"txt": 24},
                                        normalizer="layer-norm")
    assert pt.features == ["txt", "img"] and pt.pretrained_output_dims == {"txt": 24}
    assert list(pt.projection) == ["txt"] and pt.output_dim("txt") == 24 and pt.output_dim("img") == 16
    assert sorted(pt.state_dict()) == sorted(
        ["projection.txt.weight", "projection.txt.bias"] + [f"post.feature_layer_norm.{n}.{w}" for n in ("txt", "img")
                                                              for w in ("weight", "bias")])
    assert pt.projection["txt"].weight.shape == (24, 40)
    sizes = pt.forward_output_size({"txt": torch.Size([-1, 10, 40]), "img": torch.Size([-1, 10, 16])})
    assert sizes == {"txt": torch.Size([-1, 10, 24]), "img": torch.Size([-1, 10, 16])}
    assert tr.PretrainedEmbeddingFeatures(["a"], 12).state_dict() == {}
    cat = tr.SequenceEmbeddingFeatures({"item_id": (51, 16), "category": (8, 4)}, item_id="item_id")
    f = tr.TabularSequenceFeatures(cat, None, "concat", 32, pretrained_embedding_module=pt)
    assert list(f.to_merge) == ["categorical_module", "pretrained_embedding_module"] and f.pretrained_module is pt
    assert f._feature_order == ["category", "img", "item_id", "txt"]
    assert f._cols == {"category": 0, "img": 4, "item_id": 20, "txt": 36} and f._agg_width == 60
    assert f._dims["txt"] == 24 and f.output_size()[-1] == 32
    with pytest.raises(ValueError, match="same dimension"):
        tr.TabularSequenceFeatures(tr.SequenceEmbeddingFeatures({"item_id": (51, 16)}, item_id="item_id"), None, "element-wise-sum",
                                   pretrained_embedding_module=tr.PretrainedEmbeddingFeatures(["a"], 12, 24))
    g = tr.TabularSequenceFeatures(tr.SequenceEmbeddingFeatures({"item_id": (51, 24)}, item_id="item_id"), None, "element-wise-sum",
                                   pretrained_embedding_module=tr.PretrainedEmbeddingFeatures(["a"], 12, 24))
    assert g._agg_width == 24 and g._cols == {"a": 0, "item_id": 0}


def test_from_schema_reads_the_embedding_tag():
    f = tr.TabularSequenceFeatures.from_schema(_schema(), max_sequence_length=10, masking="mlm", d_output=32,
                                               embedding_dim_default=16, pretrained_output_dims=24, normalizer="layer-norm")
    pt = f.pretrained_module
    assert pt.features == ["item_vec"] and pt.input_dims == {"item_vec": 40} and f._dims["item_vec"] == 24
    assert f._feature_order == ["category", "item_id", "item_vec"]
    # a schema without such columns builds exactly what it built before
    plain = tr.TabularSequenceFeatures.from_schema(tr.session_schema(50, 10), max_sequence_length=10, masking="mlm", d_output=32)
    assert plain.pretrained_module is None and list(plain.to_merge) == ["categorical_module"]
    off = tr.TabularSequenceFeatures.from_schema(_schema(), max_sequence_length=10, pretrained_embeddings_tags=None)
    assert off.pretrained_module is None
    with pytest.raises(ValueError, match="no input width"):
        tr.TabularSequenceFeatures.from_schema(
            tr.session_schema(50, 10) + tr.Schema([tr.ColumnSchema("v", [tr.Tags.EMBEDDING])]), max_sequence_length=10)


def test_refusals():
    with pytest.raises(NotImplementedError, match="sequence_combiner"):
        tr.PretrainedEmbeddingFeatures(["a"], 8, sequence_combiner="mean")
    for kw in (dict(pre="ssn"), dict(post="layer-norm"), dict(aggregation="concat")):
        with pytest.raises(NotImplementedError):
            tr.PretrainedEmbeddingFeatures(["a"], 8, **kw)
    with pytest.raises(NotImplementedError):
        tr.PretrainedEmbeddingFeatures(["a"], 8, normalizer="batch-norm")
    with pytest.raises(NotImplementedError):
        tr.TabularSequenceFeatures.from_schema(_schema(), max_sequence_length=10, pretrained_input_dims=40, post="layer-norm")
    pt = tr.PretrainedEmbeddingFeatures(["a", "b"], 8, pretrained_output_dims={"a": 4})
    with pytest.raises(ValueError, match="needs a projection"):
        pt.attach_table("b", torch.zeros(5, 8))
    with pytest.raises(KeyError):
        pt.attach_table("c", torch.zeros(5, 8))
    with pytest.raises(_lib.T4RHipError):          # the image is packed on the device: no CPU path
        pt.attach_table("a", torch.zeros(5, 8))
    # the registered-operator path keeps refusing
    from transformers4rec_amd import functional

    f = tr.TabularSequenceFeatures.from_schema(_schema(), max_sequence_length=10, masking="mlm", pretrained_output_dims=24)
    model = type("M", (), {"input_features": f})()
    with pytest.raises(NotImplementedError, match="pretrained"):
        functional.input_block_of(model)


def test_new_parameters_are_ordinary_dense_parameters():
    """they land in the flat `dense` bucket (FusedAdam) and among the parameters GradCarrier / DDP carry"""
    f = tr.TabularSequenceFeatures.from_schema(_schema(), max_sequence_length=10, masking="mlm", d_output=32,
                                               pretrained_output_dims=24, normalizer="layer-norm")
    dense, tables = tr.flatten_model(f)
    names = [n for n, _p, _o in dense.entries]
    want = ["to_merge.pretrained_embedding_module." + k for k in
            ("projection.item_vec.weight", "projection.item_vec.bias", "post.feature_layer_norm.item_vec.weight",
             "post.feature_layer_norm.item_vec.bias")]
    assert all(w in names for w in want), names
    assert not any("pretrained" in n for n, _p, _o in tables.entries)
    for _n, p, o in dense.entries:
        assert p.grad.data_ptr() == dense.grad.data_ptr() + 4 * o
    carried = {id(p) for p in tr.hip_parameters(f)}
    assert all(id(p) in carried for p in f.pretrained_module.parameters())
    tr.enable_autograd_gradients(f)
    assert {id(p) for p in f.__dict__["_t4r_carrier_params"]} >= {id(p) for p in f.pretrained_module.parameters()}


# ------------------------------------------------------------------------------------------------ against the reference, live
def _reference():
    import ref_standins as rs

    if not os.path.isdir(rs.REFERENCE_ROOT):
        pytest.skip("the reference tree is not on this machine")
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_pretrained_golden", os.path.join(ROOT, "tools", "make_pretrained_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return rs.import_reference(), mod


def _mirror(mod):
    schema = tr.session_schema(mod.V, mod.L) + tr.Schema(
        [tr.ColumnSchema(mod.FEATURE, [tr.Tags.EMBEDDING, tr.Tags.LIST], embedding_dim=mod.E)])
    return tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=mod.L, masking="mlm", d_output=mod.D_MODEL,
                                                  embedding_dim_default=mod.D_ITEM, pretrained_output_dims=mod.P,
                                                  normalizer="layer-norm")


def test_state_dict_keys_equal_the_reference_classes():
    ref_tr, mod = _reference()
    ref = mod.build_reference(ref_tr).heads[0].body[0]
    ours = _mirror(mod)
    ref_pt = ref.to_merge["pretrained_embedding_module"]
    assert _shapes(ours.pretrained_module) == _shapes(ref_pt)
    assert sorted(_shapes(ours)) == sorted(_shapes(ref))
    assert _shapes(ours) == _shapes(ref)


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_dropin_shadow_builds_and_ties():
    ref_tr, mod = _reference()
    from transformers4rec_amd import dropin

    ref = mod.build_reference(ref_tr).heads[0].body[0]
    sh = dropin.shadow_features(ref)
    assert isinstance(sh.pretrained_module, F.PretrainedEmbeddingFeatures)
    assert sh._feature_order == ["item_id", mod.FEATURE] and sh._dims[mod.FEATURE] == mod.P
    ref_params = dict(ref.named_parameters())
    n = 0
    for name, p in sh.named_parameters():
        assert p is ref_params[name], name
        n += "pretrained" in name
    assert n == 4
    assert "pretrained" not in dropin.__doc__.split("Configurations off the hot path")[1].split("raise NotImplementedError")[0]
