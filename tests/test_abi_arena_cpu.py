"""CPU checks of the red-zone harness (tests/abi_arena.py) and the completeness check of tests/test_abi_redzone_gpu.py.

The harness is proved on CPU tensors with fake "kernels" written in torch: every kind of stray store or poisoned read the GPU
cases rely on it to see must be reported with the right buffer and offset, and a clean call must pass.
"""
import re

import pytest
import torch

import abi_arena
from abi_arena import GUARD, Arena

F32 = torch.float32


def _setup(fill, rows=5, N=6, ld=8, col=0):
    """x [rows, ld] pitched input with N logical columns; out = the window [col, col + N) of a [rows, ld_out] row buffer with a
    live neighbour on each side; y [rows] a dense output; ws 40 bytes"""
    a = Arena(fill, "cpu", capacity=2 << 20)
    x = a.new("x", "in", F32, (rows, ld), 0, N).set(torch.arange(rows * N, dtype=F32).view(rows, N) + 1)
    wide = a.new("wide", "out", F32, (rows, 4 + N + 4), 4, N)
    wide.t[:, :4] = 7.0                 # live neighbours: another feature's columns
    wide.t[:, 4 + N:] = 9.0
    y = a.new("y", "out", F32, rows)
    ws = a.ws("ws", 40)
    return a, x, wide, y, ws


def _clean_kernel(x, wide, y, ws, N=6):
    wide.t[:, 4:4 + N] = 2 * x.t[:, :N]
    y.t[:] = x.t[:, :N].sum(1)
    ws.t[:] = 3


@pytest.mark.parametrize("fill", abi_arena.FILLS)
def test_clean_call_passes(fill):
    a, x, wide, y, ws = _setup(fill)
    a.seal()
    _clean_kernel(x, wide, y, ws)
    assert a.check() is None
    assert a.nonfinite() is None
    assert torch.equal(y.win, (torch.arange(30, dtype=F32).view(5, 6) + 1).sum(1))


def test_layout_alignment_guards_and_fill():
    a, x, wide, y, ws = _setup(0xFF)
    for b in (x, wide, y, ws):
        assert b.ptr % 256 == 0                                  # payloads start as torch's own allocations do
    assert ws.nbytes == 40 and y.nbytes == 20                    # no rounding: the guard starts at the last byte plus one
    starts = sorted((b.start, b.nbytes) for b in a.bufs)
    assert starts[0][0] >= GUARD
    for (s0, n0), (s1, _) in zip(starts, starts[1:]):
        assert s1 - (s0 + n0) >= 2 * GUARD                       # a trailing and a leading guard between two payloads
    assert a.mem.numel() - (starts[-1][0] + starts[-1][1]) >= GUARD
    assert bool(torch.isnan(y.t).all()) and bool(torch.isnan(x.t[:, 6:]).all())      # 0xFF is NaN in fp32 ...
    assert bool(torch.isnan(a.new("h", "out", torch.float16, 4).t).all())
    assert bool(torch.isnan(a.new("bf", "out", torch.bfloat16, 4).t).all())
    assert bool((a.new("i", "out", torch.int64, 4).t == -1).all())                   # ... and -1 in the integer types
    assert bool((a.new("j", "out", torch.int32, 4).t == -1).all())
    with pytest.raises(AssertionError):
        y.set(0.0)                                               # an `out` buffer keeps the fill until the kernel writes


@pytest.mark.parametrize("fill", abi_arena.FILLS)
def test_one_element_past_the_end(fill):
    a, x, wide, y, ws = _setup(fill)
    a.seal()
    _clean_kernel(x, wide, y, ws)
    a.mem[y.start:y.start + y.nbytes + 4].view(F32)[5] = 1.2345   # y[5] of a 5-element buffer (0x3F9E0419: no 0x00 / 0xFF byte)
    v = a.check()
    assert v is not None and (v.buffer, v.region, v.offset, v.payload_offset) == ("y", "trailing guard", 0, 20), v


@pytest.mark.parametrize("fill", abi_arena.FILLS)
def test_one_element_before_the_start(fill):
    a, x, wide, y, ws = _setup(fill)
    a.seal()
    _clean_kernel(x, wide, y, ws)
    a.mem[ws.start - 1] = 0x5A                                   # ws[-1]
    v = a.check()
    assert v is not None and (v.buffer, v.region, v.offset, v.payload_offset) == ("ws", "leading guard", 1, -1), v


@pytest.mark.parametrize("fill", abi_arena.FILLS)
def test_workspace_overrun_by_a_tile(fill):
    a, x, wide, y, ws = _setup(fill)
    a.seal()
    _clean_kernel(x, wide, y, ws)
    a.mem[ws.start + 40:ws.start + 64] = 0x11                    # a kernel that rounds the 40 bytes up to 64
    v = a.check()
    assert v is not None and (v.buffer, v.region, v.offset) == ("ws", "trailing guard", 0), v


@pytest.mark.parametrize("fill", abi_arena.FILLS)
def test_write_into_a_pad_column(fill):
    a, x, wide, y, ws = _setup(fill)
    pitched = a.new("logits", "out", F32, (5, 8), 0, 6)
    a.seal()
    _clean_kernel(x, wide, y, ws)
    pitched.t[:, :6] = 1.0
    assert a.check() is None
    pitched.t[3, 6] = 0.5                                        # a vector store that runs to the pitch
    v = a.check()
    assert v is not None and (v.buffer, v.region, v.row, v.col) == ("logits", "outside window", 3, 6), v
    assert v.payload_offset // 4 == 3 * 8 + 6


@pytest.mark.parametrize("fill", abi_arena.FILLS)
def test_documented_pad_write_is_allowed_and_only_that(fill):
    a = Arena(fill, "cpu", capacity=1 << 20)
    img = a.new("image", "out", torch.float16, (4, 16), 0, 5).allow(5, 16)      # "a wider pitch is zero-filled to its end"
    a.seal()
    img.t[:, :5] = 1.0
    img.t[:, 5:] = 0.0
    assert a.check() is None
    assert bool((img.t[:, 5:] == 0).all())


@pytest.mark.parametrize("fill", abi_arena.FILLS)
def test_write_into_a_neighbours_column_window(fill):
    a, x, wide, y, ws = _setup(fill)
    a.seal()
    _clean_kernel(x, wide, y, ws)
    wide.t[2, 10] = 2.5                                          # first column of the right-hand neighbour
    v = a.check()
    assert v is not None and (v.buffer, v.region, v.row, v.col) == ("wide", "outside window", 2, 10), v
    wide.t[2, 10] = 9.0
    wide.t[4, 3] = -1.0                                          # last column of the left-hand neighbour
    v = a.check()
    assert v is not None and (v.buffer, v.row, v.col) == ("wide", 4, 3), v


@pytest.mark.parametrize("fill", abi_arena.FILLS)
def test_write_into_an_input(fill):
    a, x, wide, y, ws = _setup(fill)
    a.seal()
    _clean_kernel(x, wide, y, ws)
    x.t[1, 2] += 1
    v = a.check()
    assert v is not None and (v.buffer, v.region, v.row, v.col) == ("x", "input", 1, 2), v


def test_nan_read_from_a_pad_column_is_reported():
    """a kernel that sums the whole pitch instead of the logical width: invisible under 0x00, a NaN under 0xFF"""
    for fill, want in ((0x00, None), (0xFF, ("y", (0,)))):
        a, x, wide, y, ws = _setup(fill)
        a.seal()
        _clean_kernel(x, wide, y, ws)
        y.t[:] = x.t.sum(1)                                      # reads columns 6, 7: the pad
        assert a.check() is None                                 # nothing was written out of place ...
        assert a.nonfinite() == want                             # ... the poison shows in the result
    a, x, wide, y, ws = _setup(0xFF)
    a.seal()
    _clean_kernel(x, wide, y, ws)
    wide.t[3, 4 + 2] = x.t[3, 7]                                 # one poisoned element in a column window
    assert a.nonfinite() == ("wide", (3, 2))


@pytest.mark.parametrize("fill", abi_arena.FILLS)
def test_buffers_carved_between_two_calls(fill):
    """a case of several calls carves more buffers after the first call: the earlier snapshot stays, and a store of the first
    call far beyond what existed then is still reported"""
    a, x, wide, y, ws = _setup(fill)
    a.seal()
    _clean_kernel(x, wide, y, ws)
    z = a.new("z", "in", F32, 4).set(torch.ones(4))
    out2 = a.new("out2", "out", F32, 4)
    assert not a.sealed
    a.seal()
    out2.t[:] = z.t * y.t[:4]
    assert a.check() is None
    y.t[0] = 5.0
    assert a.check() is None                                     # y is still the kernel's
    x.t[0, 0] = -3.0
    v = a.check()
    assert v is not None and (v.buffer, v.region) == ("x", "input"), v
    a, x, wide, y, ws = _setup(fill)
    a.seal()
    a.mem[a.cursor + 1000] = 0x5A                                # a wild store of "call 1" past everything carved so far
    z = a.new("z", "in", F32, 4).set(torch.ones(4))
    a.seal()
    assert a.check() is not None


def test_a_stray_store_of_the_fill_value_needs_the_other_fill():
    """why every case runs under both fills: a stray 0 is invisible on 0x00, a stray NaN / -1 on 0xFF"""
    seen = {}
    for fill in abi_arena.FILLS:
        a, x, wide, y, ws = _setup(fill)
        a.seal()
        _clean_kernel(x, wide, y, ws)
        a.mem[y.start + 20:y.start + 24] = 0                     # y[5] = 0.0f
        seen[fill] = a.check()
    assert seen[0x00] is None and seen[0xFF] is not None and seen[0xFF].buffer == "y"


# ------------------------------------------------------------------------------------------------ completeness
# Entries of include/t4r_hip.h that need no red-zone case, each with the reason: nothing is launched on the device.
EXEMPT = {
    "t4r_abi_version": "constant query: nothing launches",
    "t4r_last_error": "host string getter: nothing launches",
    "t4r_sort_ids_ws_bytes": "size query: nothing launches (its value sizes the workspace of the t4r_sort_ids cases)",
    "t4r_sort_ids_multi_ws_bytes": "size query: nothing launches (sizes the workspace of the t4r_sort_ids_multi cases)",
    "t4r_embedding_bwd_sorted_ws_floats": "size query: nothing launches (sizes the workspace of the t4r_embedding_bwd_sorted cases)",
    "t4r_apply_mask_bwd_ws_floats": "size query: nothing launches (sizes the workspace of the t4r_apply_mask_bwd cases)",
    "t4r_soft_embedding_bwd_ws_floats": "size query: nothing launches",
    "t4r_gemm_wgrad_ws_floats": "size query: nothing launches",
    "t4r_set_precision": "setter: nothing launches",
    "t4r_get_precision": "getter: nothing launches",
    "t4r_set_tok_gemm_min_rows": "setter: nothing launches",
    "t4r_get_tok_gemm_min_rows": "getter: nothing launches",
    "t4r_head_note_dw_form": "reads the caller's host note: nothing launches",
    "t4r_head_split_supported": "capability query: nothing launches",
    "t4r_head_split_fwd_products": "capability query: nothing launches",
    "t4r_head_split_ws_bytes": "size query: nothing launches",
    "t4r_head_split_fdx_supported": "capability query: nothing launches",
    "t4r_head_split_recompute_supported": "capability query: nothing launches",
    "t4r_linear_softmax_ce_chunk_floats": "size query: nothing launches",
    "t4r_dropout_ctr_hi": "host arithmetic: nothing launches",
    "t4r_colreduce_ws_floats": "size query: nothing launches (sizes the workspaces of the column-reduction cases)",
    "t4r_xlnet_attn_bwd_ws_floats": "size query: nothing launches",
    "t4r_xlnet_fused_supported": "capability query: nothing launches",
    "t4r_xlnet_fused_products": "capability query: nothing launches",
    "t4r_xlnet_layer_planes_floats": "size query: nothing launches",
    "t4r_xlnet_ff_planes_floats": "size query: nothing launches",
    "t4r_xlnet_ln1_bwd_part_floats": "size query: nothing launches",
    "t4r_xlnet_set_cu_budget": "setter: nothing launches",
    "t4r_xlnet_get_cu_budget": "getter: nothing launches",
    "t4r_device_cus": "device attribute query: nothing launches",
    "t4r_experimental_build": "build-flag query: nothing launches",
    "t4r_xlnet_attn_block_supported": "capability query: nothing launches",
    "t4r_xlnet_ff_bwd_part_floats": "size query: nothing launches",
    "t4r_xlnet_layer_ws_floats": "size query: nothing launches",
    "t4r_xlnet_layer_bwd_ws_floats": "size query: nothing launches",
    "t4r_xlnet_layer_ws_offsets": "offset query into host longs: nothing launches",
    "t4r_item_topk_ws_bytes": "size query: nothing launches",
    "t4r_item_table_image_ld": "pitch query: nothing launches",
    "t4r_item_topk_h16_supported": "capability query: nothing launches",
    "t4r_item_topk_h16_ws_bytes": "size query: nothing launches",
    "t4r_item_eval_h16_ws_bytes": "size query: nothing launches",
    "t4r_swap_noise_ws_bytes": "size query: nothing launches",
}


def _header_entries():
    from transformers4rec_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)       # as tests/test_abi.py / _lib.header_symbols
    names = sorted(set(re.findall(r"\b(t4r_\w+)\s*\(", text)))
    assert names == _lib.header_symbols() and len(names) >= 100
    return names


def test_every_entry_point_has_a_redzone_case_or_an_exemption():
    import test_abi_redzone_gpu as rz

    names = _header_entries()
    cased = set(rz.cased_entries())
    assert cased <= set(names), f"cases name entries the header does not declare: {sorted(cased - set(names))}"
    assert not (set(EXEMPT) - set(names)), f"exemptions for entries the header does not declare: {sorted(set(EXEMPT) - set(names))}"
    for n, why in EXEMPT.items():
        assert why and "\n" not in why, n
    missing = [n for n in names if n not in cased and n not in EXEMPT]
    assert not missing, ("entry points of include/t4r_hip.h with neither a red-zone case in tests/test_abi_redzone_gpu.py nor "
                         f"an exemption with a reason here: {missing}")


def test_case_table_is_well_formed():
    import test_abi_redzone_gpu as rz

    ids = [c.id for c in rz.CASES]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    fams = {}
    for c in rz.CASES:
        fams.setdefault(c.family, []).append(c.id)
        assert c.entries, c.id
    for f, members in fams.items():
        assert len(members) >= 2, f"family {f} needs a second case for the state-leak rerun"
