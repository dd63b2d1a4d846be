// bf16 / fp16 matrix-core instantiations of the GEMM kernel (gemm_kernel.h, PREC = 1, 2, 3), in their own
// translation unit so that they compile next to the fp32 ones.  Selected by gemm_f32.hip: launch_layout.
//   PREC 1: fp32-accurate products by the exact three-way bf16 split (six v_mfma_f32_32x32x16_bf16 per K = 16)
//   PREC 4: fp32-class products by the two-way fp16 split (three v_mfma_f32_32x32x16_f16 per K = 16), operands positioned by
//           powers of two from their maxima (the weight gradients of the fused XLNet layer)
//   PREC 2 / 3: mixed precision (bf16 / fp16 operands, fp32 accumulation) -- the reference's AMP mode,
//               transformers4rec/torch/trainer.py:363-367, model/prediction_task.py:430
// Tiles (BK = kBkHalf = 32 throughout; gemm_f32.hip: launch_layout chooses, DESIGN.md 4.1.2 lists the forms):
//   64 x 64    every precision, layout and feature (three-plane images: 52 KB of LDS, three workgroups per CU)
//   128 x 64   PREC 1, plain launches of >= 2e10 FLOP, all four layouts
//   128 x 128  PREC 2 / 3, the plain NT logits product (the three-plane images of such a tile would take 101 KB of LDS)
#include "gemm_kernel.h"
#include "t4r_internal.h"

// the 64 x 64 forms: the A-operand transform or epilogue of the launch picks FEAT.  The layout error is a guard kept on purpose
// (gemm_f32.hip: launch_cfg says why): launch_layout sends a softmax-gradient launch with transB = 1 to fp32.
template <bool TA, bool TB, int PREC>
static int half_cfg(const GemmParams& p, int batch, hipStream_t stream) {
    if (p.sg_lse) {
        if constexpr (!TB) return launch_vec<64, 64, kBkHalf, TA, false, 1, true, PREC>(p, batch, stream);
        t4r_set_error("gemm (half): softmax-grad operand needs transB = 0");
        return -1;
    }
    if (p.drop.p > 0.f && (p.epilogue == EPI_BIAS_GELU || p.epilogue == EPI_BIAS_RESID))
        return launch_vec<64, 64, kBkHalf, TA, TB, 2, true, PREC>(p, batch, stream);
    return launch_vec<64, 64, kBkHalf, TA, TB, 0, true, PREC>(p, batch, stream);
}

// bm, bn: launch_layout's tile.  It asks for 128 x 64 only at PREC 1 and for 128 x 128 only at PREC 2 / 3 in the NT layout, both
// without a feature, so each large tile has exactly the instantiations below.
template <bool TA, bool TB>
static int half_layout(const GemmParams& p, int batch, int bm, int bn, int prec, hipStream_t stream) {
    if (bm == 128 && bn == 64) return launch_vec<128, 64, kBkHalf, TA, TB, 0, true, 1>(p, batch, stream);
    if constexpr (!TA && TB) {
        if (bm == 128 && bn == 128)
            return prec == 2 ? launch_vec<128, 128, kBkHalf, false, true, 0, true, 2>(p, batch, stream)
                             : launch_vec<128, 128, kBkHalf, false, true, 0, true, 3>(p, batch, stream);
    }
    if (prec == 1) return half_cfg<TA, TB, 1>(p, batch, stream);
    if (prec == 2) return half_cfg<TA, TB, 2>(p, batch, stream);
    if (prec == 3) return half_cfg<TA, TB, 3>(p, batch, stream);
    if (prec == 4) {        // two-way fp16 split with operand scales (plain launches only: the layer's weight gradients)
        if (p.sg_lse || p.drop.p > 0.f || !p.amaxA || !p.amaxB) { t4r_set_error("gemm (fp16 split): plain products with operand maxima only"); return -1; }
        return launch_vec<64, 64, kBkHalf, TA, TB, 0, true, 4>(p, batch, stream);
    }
    t4r_set_error("gemm (half): unknown precision");
    return -1;
}

int t4r_gemm_half_dispatch(const GemmParams& p, int batch, int ta, int tb, int bm, int bn, int prec, hipStream_t stream) {
    if (ta) return tb ? half_layout<true, true>(p, batch, bm, bn, prec, stream) : half_layout<true, false>(p, batch, bm, bn, prec, stream);
    return tb ? half_layout<false, true>(p, batch, bm, bn, prec, stream) : half_layout<false, false>(p, batch, bm, bn, prec, stream);
}
