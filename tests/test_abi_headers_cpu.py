"""The C ABI has one statement, the headers under include/: the ctypes prototypes are derived from them (_lib.signatures()).  This
checks the parser on the hard cases, then the twelve headers against the loaded library, then the relations between entries that
the feature tests state in words.  Nothing here needs a GPU."""
import ctypes
import re

import pytest

from transformers4rec_amd import _lib

COUNTS = {"t4r_hip.h": 125, "t4r_hip_sampling.h": 6, "t4r_hip_filter.h": 7, "t4r_hip_optim.h": 4, "t4r_hip_pretrained.h": 4,
          "t4r_hip_attn.h": 2, "t4r_hip_rows.h": 5, "t4r_hip_rowadam.h": 2, "t4r_hip_contproj.h": 4, "t4r_hip_rowclip.h": 3,
          "t4r_hip_seqtask.h": 4, "t4r_hip_rtd.h": 4}
CTYPES = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "Q": ctypes.c_ulonglong,
          "s": ctypes.c_char_p, "v": None}

SYNTHETIC = """
/* a block comment with a declaration inside: int t4r_not_this(int a); */
#ifndef X_H
#define X_H
#ifdef __cplusplus
extern "C" {
#endif
typedef struct x_note { unsigned long long w[8]; } x_note;
int x_version(void);
const char* x_last_error(void);
unsigned long long x_ctr(unsigned long long seed, long row, int layer);     // a line comment: void x_nor_this(float f);
long x_ws_bytes(long n, int D);
void x_set(int v);
int x_gather(void* stream, const long* const* ids, const int* n, x_note* note, float scale,
             unsigned long long lo /* inside the list, with a comma, and (parentheses) */,
             long ld);
#define X_FLAG 0x100
#define X_LONG(a) \\
    ((a) + 1)
long x_after_define(int B, const float* const w);
int
x_split(
    int a);
#ifdef __cplusplus
}
#endif
#endif /* X_H */
"""


# ---------------------------------------------------------------------------------------------------------- the parser
def test_parser_on_the_hard_cases():
    got = _lib.parse_header(SYNTHETIC, "x.h")
    assert list(got.items()) == [
        ("x_version", ("i", "")), ("x_last_error", ("s", "")), ("x_ctr", ("Q", "Qli")), ("x_ws_bytes", ("l", "li")),
        ("x_set", ("v", "i")), ("x_gather", ("i", "ppppfQl")), ("x_after_define", ("l", "ip")), ("x_split", ("i", "i"))]
    assert _lib.parse_header("int f(const unsigned long long a, unsigned long long, long, const long b);") == {"f": ("i", "QQll")}
    assert _lib.parse_header("") == {} and _lib.parse_header("/* only a comment */\n#define A 1\n") == {}


@pytest.mark.parametrize("decl", [
    "int f(double x);", "int f(int a, size_t n);", "int f(unsigned n);", "int f(x_note note);", "int f(int (*cb)(int));",
    "int f(int a, ...);", "int f(long long n);", "int f(short a);", "int f(float v[4]);", "int f();",
    "double f(int a);", "float f(int a);", "size_t f(void);", "unsigned f(void);", "char* f(void);", "int* f(void);", "x_note f(void);",
    "int f(int a); int f(long a);", "int f(int a)", "int f(int a) { return a; }", "static int x = 3;", "struct s { int a; };"])
def test_parser_refuses_what_it_cannot_map(decl):
    with pytest.raises(_lib.T4RHipError, match=r"x\.h"):
        _lib.parse_header(decl, "x.h")


def test_a_name_in_two_headers_and_a_missing_header_are_errors(monkeypatch, tmp_path):
    (tmp_path / "a.h").write_text("int f(int a);\nint g(void);\n")
    (tmp_path / "b.h").write_text("long h(long n);\nint f(int a);\n")
    monkeypatch.setattr(_lib, "header_path", lambda name: str(tmp_path / name))
    monkeypatch.setattr(_lib, "_lib", None)
    try:
        for headers, words in ((("a.h", "b.h"), ("`f`", "a.h", "b.h")), (("a.h", "c.h"), (str(tmp_path / "c.h"), "missing"))):
            monkeypatch.setattr(_lib, "HEADERS", headers)
            for fn in (_lib.signatures, _lib.load):                            # load() reports the same, before it opens the library
                _lib.signatures.cache_clear()
                with pytest.raises(_lib.T4RHipError) as e:
                    fn()
                assert all(w in str(e.value) for w in words), str(e.value)
        assert _lib.header_symbols("a.h") == ["f", "g"]
    finally:
        _lib.signatures.cache_clear()
        _lib._header_signatures.cache_clear()


# ---------------------------------------------------------------------------------------------------------- the twelve headers
def test_headers_counts_and_disjoint_names():
    assert _lib.HEADERS == tuple(COUNTS) and _lib.HEADER_PATH == _lib.header_path("t4r_hip.h")
    per_header = {h: _lib.header_symbols(h) for h in _lib.HEADERS}
    assert {h: len(v) for h, v in per_header.items()} == COUNTS
    assert _lib.header_symbols() == per_header["t4r_hip.h"] == sorted(per_header["t4r_hip.h"])
    sigs = _lib.signatures()
    assert len(sigs) == sum(COUNTS.values()) == 170                             # pairwise disjoint: the union loses nothing
    assert list(sigs) == [n for h in _lib.HEADERS for n in _lib.parse_header(open(_lib.header_path(h)).read(), h)]
    assert all(n.startswith("t4r_") for n in sigs)
    # what the names-only scan of the text finds is what the parser finds: no declaration is passed over
    for h in _lib.HEADERS:
        text = re.sub(r"/\*.*?\*/", "", open(_lib.header_path(h)).read(), flags=re.S)
        assert sorted(set(re.findall(r"\b(t4r_\w+)\s*\(", text))) == per_header[h], h


def test_loaded_library_has_the_parsed_prototypes():
    lib = _lib.load()
    for name, (ret, args) in _lib.signatures().items():
        assert hasattr(lib, name), f"{name} is declared in a header but not exported"
        fn = getattr(lib, name)
        assert fn.restype is CTYPES[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [CTYPES[a] for a in args], name
    # a few prototypes written out by hand from the headers: every code, Q next to l, the s and v returns, a comment inside the
    # parameter list (t4r_apply_mask_bwd), the declaration after the #define block, t4r_head_note*
    sigs = _lib.signatures()
    assert sigs["t4r_last_error"] == ("s", "") and sigs["t4r_set_precision"] == ("v", "i") and sigs["t4r_abi_version"] == ("i", "")
    assert sigs["t4r_dropout_ctr_hi"] == ("Q", "Qii") and sigs["t4r_dropout"] == ("i", "pppp" + "llfQQ")
    assert sigs["t4r_apply_mask_bwd"] == ("i", "ppppiiii" + "p") and sigs["t4r_xlnet_layer_ws_floats"] == ("l", "iiiii")
    assert sigs["t4r_head_note_dw_form"] == ("i", "p") and sigs["t4r_mask_targets"] == ("i", "ppiiil" + "ppp" + "fQQ" + "ppp")
    assert sigs["t4r_row_adam_step"] == ("i", "pppp" + "li" + "ppp" + "lli" + "fffff" + "if" + "pl")


def test_no_torch_types_in_any_header():
    for h in _lib.HEADERS:
        decls = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(_lib.header_path(h)).read(), flags=re.S)
        for word in ("at::", "torch", "Tensor", "std::", "c10"):
            assert word not in decls, f"{word} leaked into the C ABI ({h})"


# ---------------------------------------------------------------------------------------------------------- relations
def test_structural_relations_between_entries():
    sigs = _lib.signatures()
    # include/t4r_hip_rows.h: the plain entry + the map (rows, n) (+ the compact h1 rows of the feed-forward backward)
    for plain, tail in (("t4r_xlnet_ff_fwd", "pi"), ("t4r_xlnet_ff_bwd", "pip"), ("t4r_xlnet_layer_fwd", "pi"),
                        ("t4r_xlnet_layer_bwd", "pi")):
        assert sigs[plain + "_rows"] == ("i", sigs[plain][1] + tail), plain
    # include/t4r_hip_filter.h: the unfiltered entry + allow_bits, excl, n_excl, ld_excl
    for plain in ("t4r_item_topk_f32", "t4r_item_topk_h16", "t4r_item_sample_f32", "t4r_item_sample_h16"):
        filtered = plain.replace("_f32", "_filtered_f32").replace("_h16", "_filtered_h16")
        assert sigs[filtered] == ("i", sigs[plain][1] + "ppil"), plain
    assert sigs["t4r_item_mask_f32"] == ("i", "pp" + "iili" + "ppil")
    # include/t4r_hip_attn.h: + prob in the forward; out, lse -> prob and no key_len in the backward
    fwd, fwd_p = sigs["t4r_xlnet_attn_block_fwd"][1], sigs["t4r_xlnet_attn_block_fwd_prob"][1]
    assert len(fwd_p) == len(fwd) + 1 and fwd_p.replace("p", "") == fwd.replace("p", "")
    bwd, bwd_p = sigs["t4r_xlnet_attn_bwd"][1], sigs["t4r_xlnet_attn_bwd_prob"][1]
    assert len(bwd_p) == len(bwd) - 2 and bwd_p.replace("p", "") == bwd.replace("p", "")
    # include/t4r_hip_rowadam.h and t4r_hip_rowclip.h: the argument counts the feature tests call with
    assert len(sigs["t4r_row_adam_step"][1]) == 21
    assert [len(sigs[n][1]) for n in ("t4r_row_grad_sumsq_parts", "t4r_row_adam_reduce", "t4r_row_adam_apply")] == [2, 11, 18]
