"""TEST INFRASTRUCTURE ONLY.  Records tests/golden/contproj_regression.npz: the output and every parameter gradient of two input
blocks that do NOT project their continuous columns -- plain ContinuousFeatures (width-1 pass-through columns) and
SoftEmbeddingFeatures -- on the GPU, so that tests/test_cont_proj_gpu.py can hold later commits to the same bits.  It was run on
the commit BEFORE `continuous_projection` existed; run it again only to re-baseline on purpose.

    python tools/make_contproj_regression.py [--out DIR]

Parameters and inputs come from CPU generators with fixed seeds; every kernel on these paths sums in a fixed order."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "contproj_regression"
B, L, V = 6, 7, 30
CATS = (("category", 5),)
CONTS = ("price", "age_days")
CASES = {"plain": False, "soft": True}


def build(tr, soft):
    schema = tr.session_schema(V, L, CATS, CONTS)
    torch.manual_seed(0)
    f = tr.TabularSequenceFeatures.from_schema(schema, max_sequence_length=L, masking="clm", aggregation="concat", d_output=16,
                                               embedding_dim_default=8, continuous_soft_embeddings=soft)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in f.named_parameters():
            if "layer_norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return f


def inputs():
    g = torch.Generator().manual_seed(6)
    lens = torch.randint(2, L + 1, (B,), generator=g)
    lens[0] = L
    m = torch.arange(L)[None] < lens[:, None]
    x = {"item_id": torch.randint(1, V + 1, (B, L), generator=g) * m,
         "category": torch.randint(1, 6, (B, L), generator=g) * m}
    for n in CONTS:
        x[n] = torch.rand((B, L), generator=g) * m
    return x


def run(tr, soft, device="cuda"):
    """-> {"out": ..., "g/<parameter>": ...} as host tensors"""
    f = build(tr, soft).to(device)
    f.train()
    x = {k: v.to(device) for k, v in inputs().items()}
    out = f(x, training=True)
    (out * out).sum().backward()
    d = {"out": out.detach().cpu()}
    for n, p in f.named_parameters():
        if p.grad is not None:
            d["g/" + n] = p.grad.detach().cpu()
    return d


def main():
    import transformers4rec_amd as tr

    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    d = {}
    for case, soft in CASES.items():
        for k, v in run(tr, soft).items():
            d[f"{case}/{k}"] = v.numpy()
    path = os.path.join(out_dir, NAME + ".npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes,", len(d), "arrays from", os.path.dirname(tr.__file__))


if __name__ == "__main__":
    main()
