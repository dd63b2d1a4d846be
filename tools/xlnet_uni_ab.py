"""A/B timing of one XLNet layer, forward + backward, with the causal core of attn_type='uni' (csrc/xlnet_attn_uni.hip, through
ops.xlnet_layer_fwd / _bwd(causal=True)) against the bi layer (causal=False) on the same GPU tensors, on one GPU in one
process, the two alternating.

    python tools/xlnet_uni_ab.py [--reps 200] [--inner 5] [--out profiles/xlnet_uni_ab.json]

Shapes (B, L, D, heads): (1024, 20, 128, 4), the benchmark's configs[1], and (256, 100, 128, 4).  The bi kernels are the ones
the library had before the causal core was added, so the bi figure stands for the layer as it was.  The attention cores alone
(ops.xlnet_attn_fwd + _bwd against ops.xlnet_attn_uni_fwd + _bwd on the layer's q | k | v layout) are timed the same way.
Each sample times `inner` forward + backward pairs between two device events; the figure is the median over `reps` (>= 200)
samples after a warm-up; the spread of a figure is its interquartile range (min and max are recorded too).  Dropout 0.
Fails without a GPU."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1024, 20, 128, 4), (256, 100, 128, 4)]


def _arg(name, default, cast):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner        # microseconds per call


def _stats(v, unit):
    q = statistics.quantiles(v, n=4)
    return {f"{unit}": statistics.median(v), f"{unit}_iqr": q[2] - q[0], f"{unit}_min": min(v), f"{unit}_max": max(v)}


def _alternate(fa, fb, reps, inner):
    for fn in (fa, fb):           # warm-up
        for _ in range(3):
            _timed(fn, inner)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_timed(fa, inner))
        tb.append(_timed(fb, inner))
    return ta, tb


def layer_ab(reps, inner):
    from transformers4rec_amd import ops
    from transformers4rec_amd.transformer import relative_positional_encoding

    dev = "cuda"
    rows = []
    for B, L, D, n in SHAPES:
        dh = D // n
        g = torch.Generator().manual_seed(B + L + D)
        r = lambda *s: (0.1 * torch.randn(*s, generator=g)).to(dev)
        params = [r(D, n, dh), r(D, n, dh), r(D, n, dh), r(D, n, dh), r(D, n, dh), r(n, dh), r(n, dh), 1 + r(D), r(D),
                  r(4 * D, D), r(4 * D), r(D, 4 * D), r(D), 1 + r(D), r(D)]
        h = torch.randn(B * L, D, generator=g).to(dev)
        dout = (torch.randn(B * L, D, generator=g) / (B * L)).to(dev)
        pos = relative_positional_encoding(L, D).to(dev).contiguous()
        grads = [torch.zeros_like(t) for t in params]
        ws = torch.empty(ops.xlnet_layer_ws_floats(B, L, D, n), device=dev)
        bws = torch.empty(ops.xlnet_layer_bwd_ws_floats(B, L, D, n), device=dev)

        def layer(causal):
            def run():
                _out, w = ops.xlnet_layer_fwd(h, pos, params, B, L, n, 0.03, ws=ws, causal=causal)
                return ops.xlnet_layer_bwd(h, pos, params, grads, w, dout, B, L, n, 0.03, bws=bws, causal=causal)
            return run

        # the cores alone, on planes of one [3, T, D] buffer as the layer holds them
        qkv = torch.randn(3, B * L, D, generator=g).to(dev)
        kr, rw, rr = torch.randn(2 * L, D, generator=g).to(dev), r(D), r(D)
        g_av = torch.randn(B * L, D, generator=g).to(dev)
        d_rw, d_rr = torch.zeros(D, device=dev), torch.zeros(D, device=dev)

        def core(fwd, bwd):
            def run():
                out, lse = fwd(qkv[0], qkv[1], qkv[2], kr, rw, rr, B, L, n)
                return bwd(qkv[0], qkv[1], qkv[2], kr, rw, rr, out, lse, g_av, d_rw, d_rr, B, L, n)
            return run

        row = dict(B=B, L=L, D=D, n_head=n)
        for tag, fu, fb in (("layer", layer(True), layer(False)),
                            ("core", core(ops.xlnet_attn_uni_fwd, ops.xlnet_attn_uni_bwd), core(ops.xlnet_attn_fwd, ops.xlnet_attn_bwd))):
            tu, tb = _alternate(fu, fb, reps, inner)
            row.update({f"{tag}_uni_" + k: v for k, v in _stats(tu, "us").items()})
            row.update({f"{tag}_bi_" + k: v for k, v in _stats(tb, "us").items()})
            row[f"{tag}_uni_over_bi"] = row[f"{tag}_uni_us"] / row[f"{tag}_bi_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("xlnet_uni_ab: no GPU visible; a timing needs one")
    reps, inner = _arg("--reps", 200, int), _arg("--inner", 5, int)
    path = _arg("--out", os.path.join(ROOT, "profiles", "xlnet_uni_ab.json"), str)
    assert reps >= 200, "each figure is the median over at least 200 samples"
    res = dict(device=torch.cuda.get_device_name(0), reps=reps, inner=inner,
               method="median over reps of device-event time per forward + backward pair of one layer (and of the attention core "
                      "alone), uni and bi alternating in one process; spread = interquartile range; dropout 0",
               shapes=layer_ab(reps, inner))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
