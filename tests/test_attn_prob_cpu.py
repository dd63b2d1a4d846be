"""Host half of the attention probabilities' hand-over: the sixth C-ABI header (include/t4r_hip_attn.h) against the library and
the derived prototypes, and the layer workspace that carries the probabilities.  Nothing here needs a GPU."""
import ctypes
import re

from transformers4rec_amd import _lib


def test_sixth_header_library_and_prototypes_agree():
    lib = _lib.load()
    syms = _lib.header_symbols("t4r_hip_attn.h")
    assert syms == ["t4r_xlnet_attn_block_fwd_prob", "t4r_xlnet_attn_bwd_prob"]
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/t4r_hip_attn.h but not exported"
    # the two entries are their t4r_hip.h counterparts plus / minus the documented pointers: tests/test_abi_headers_cpu.py
    text = re.sub(r"/\*.*?\*/", "", open(_lib.header_path("t4r_hip_attn.h")).read(), flags=re.S)
    for word in ("at::", "torch", "Tensor", "std::", "c10"):
        assert word not in text, f"{word} leaked into the C ABI"


def test_layer_workspace_carries_the_probabilities():
    lib = _lib.load()
    B, L, D, n = 1024, 20, 128, 4
    T = B * L
    w0, w1 = lib.t4r_xlnet_layer_ws_floats(B, L, D, n, 0), lib.t4r_xlnet_layer_ws_floats(B, L, D, n, 1)
    # the slot has the same size with and without dropout (tests/test_abi.py pins the difference of the two carves) ...
    assert w1 == w0 + (B - 1) * 2 * L * D + B * 2 * L * D + T * D
    # ... and holds B n L L floats behind everything the layer kept before
    saved = 3 * T * D + 2 * L * D + T * D + B * n * L + T * D + 2 * T + T * D + 8 * T * D + T * D + 2 * T
    assert w0 >= saved + B * n * L * L
    # per session it grows by the saved rows, lse and n L L probabilities
    per_token = 3 * D + D + D + 2 + D + 8 * D + D + 2                  # qkv, av, ao, mean1 / rstd1, h1, ffpre / ffact, ffout, mean2 / rstd2
    c, d = lib.t4r_xlnet_layer_ws_floats(8, L, D, n, 0), lib.t4r_xlnet_layer_ws_floats(16, L, D, n, 0)
    assert d - c >= 8 * (L * per_token + n * L + n * L * L)
    # the offsets query stays consistent with the carve: planes and k_r where they were, inside the workspace
    po, ko = ctypes.c_long(), ctypes.c_long()
    assert lib.t4r_xlnet_layer_ws_offsets(B, L, D, n, 1, ctypes.byref(po), ctypes.byref(ko)) == 0
    assert ko.value == 3 * T * D and 0 < po.value < w1
    assert lib.t4r_xlnet_attn_bwd_ws_floats(8, 20, 64, 4) == 8 * (2 * 20 * 64 + 2 * 64)
