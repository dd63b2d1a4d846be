"""One case per large-tile form of the general GEMM (csrc/gemm_f32.hip: launch_layout; DESIGN.md lists the forms).

test_kernels_gpu.py reaches the 64 x 64 forms and the one-plane 128 x 128 form; no small shape reaches the fp32 128 x 128 tile or
the three-plane 128 x 64 tile.  A test cannot observe which kernel ran: the shapes below are derived from the selection rule
    fp32 128 x 128 x 16     NT, M >= 1024, N >= 32768, no epilogue, and the launch stays fp32
                            (default mode below the 2 GFLOP auto-split floor, or operands that are not 16-byte loadable)
    three-plane 128 x 64    mode fp32_bf16x3, no feature, M >= 1024, N >= 512, 2 M N K >= 2e10
and sit just past each threshold, off every tile multiple.

Operands are integers from {-3 ... 3} held in fp32: every product and every partial sum is exact in every form (three-plane
included: such a value is its own high bf16 plane), so the result must EQUAL the fp64 product cast to fp32."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from transformers4rec_amd import ops as _ops

    return _ops


def _ints(shape, g):
    return torch.randint(-3, 4, shape, generator=g).float()


# K = 12: rows of 48 bytes, 16-byte loadable (the VEC instantiation); 2 * 1028 * 32772 * 12 = 0.8 GFLOP < 2 GFLOP: stays fp32.
# K = 13: contiguous rows of 13 floats are not 16-byte loadable (the non-VEC instantiation), which also forces fp32.
@pytest.mark.parametrize("K", [12, 13])
@pytest.mark.parametrize("data", ["ints", "randn"])
def test_fp32_128x128_tile(ops, K, data):
    M, N = 1028, 32772
    g = torch.Generator().manual_seed(100 + K)
    if data == "ints":
        A, B = _ints((M, K), g), _ints((N, K), g)
    else:
        A, B = torch.randn((M, K), generator=g), torch.randn((N, K), generator=g)
    ref = (0.5 * (A.double() @ B.double().t())).float()
    with ops.precision("auto"):
        out = ops.gemm(A.to(DEV), B.to(DEV), False, True, alpha=0.5).cpu()
    if data == "ints":
        assert torch.equal(out, ref)
    else:       # test_kernels_gpu.py: test_gemm_layouts' own tolerance
        torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-4)


# 2 * 1028 * 516 * 18852 = 2.0002e10 FLOP, just over the 2e10 threshold; K is a multiple of 4 (16-byte loadable in every layout)
# but not of 32 (the k-tail runs); |sum| <= 9 * 18852 < 2^24
_M, _N, _K = 1028, 516, 18852


@pytest.fixture(scope="module")
def three_plane_case():
    g = torch.Generator().manual_seed(7)
    A, B = _ints((_M, _K), g), _ints((_K, _N), g)
    return A, B, (A.double() @ B.double()).float()


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_three_plane_128x64_tile(ops, three_plane_case, ta, tb):
    A, B, ref = three_plane_case
    assert 2.0 * _M * _N * _K >= 2e10 and _K % 4 == 0 and _K % 32 != 0 and 9 * _K < 2 ** 24
    a = (A.t() if ta else A).contiguous().to(DEV)
    b = (B.t() if tb else B).contiguous().to(DEV)
    with ops.precision("fp32_bf16x3"):
        out = ops.gemm(a, b, bool(ta), bool(tb)).cpu()
    assert torch.equal(out, ref)
