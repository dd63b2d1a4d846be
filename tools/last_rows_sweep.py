"""Crossover of the row-mapped last layer (include/t4r_hip_rows.h): one XLNet layer forward + backward through the plain and
through the mapped entry at T = 20 480 tokens, d_model 128, with n / T in {1/16, 1/8, 1/4, 1/2, 3/4, 1} mapped rows, in ONE
process with interleaved legs, timed with device events on the launch stream (the weight-gradient streams are joined inside
the timed region).

    python tools/last_rows_sweep.py [--legs 5] [--iters 20] [--json OUT]

Prints one line per fraction: ms per forward + backward of both entries (median, min, max over the legs) and whether the
mapped form is faster by more than the spread of the legs.  transformer._LAST_ROWS_MAX_FRACTION is the largest fraction at
which it is."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from transformers4rec_amd import ops  # noqa: E402
from transformers4rec_amd.transformer import relative_positional_encoding  # noqa: E402

B, L, D, NH, EPS, P = 1024, 20, 128, 4, 0.03, 0.3
FRACTIONS = (1 / 16, 1 / 8, 1 / 4, 1 / 2, 3 / 4, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    T = B * L
    g = torch.Generator().manual_seed(0)
    dh = D // NH
    r = lambda *s: (0.1 * torch.randn(*s, generator=g)).to(dev)
    params = [r(D, NH, dh), r(D, NH, dh), r(D, NH, dh), r(D, NH, dh), r(D, NH, dh), r(NH, dh), r(NH, dh), 1 + r(D), r(D),
              r(4 * D, D), r(4 * D), r(D, 4 * D), r(D), 1 + r(D), r(D)]
    grads = [torch.zeros_like(t) for t in params]
    h = torch.randn(T, D, generator=g).to(dev)
    pos = relative_positional_encoding(L, D).to(dev).contiguous()
    ws = torch.empty(ops.xlnet_layer_ws_floats(B, L, D, NH, True), device=dev)
    bws = torch.empty(ops.xlnet_layer_bwd_ws_floats(B, L, D, NH, True), device=dev)
    kw = dict(drop_p=P, seed=7, offset=1, layer_idx=3 | ops.LAYER_FUSE_FINAL)

    def leg(rows, n, dout):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            _, w = ops.xlnet_layer_fwd(h, pos, params, B, L, NH, EPS, ws=ws, rows=rows, n_rows=n, **kw)
            ops.xlnet_layer_bwd(h, pos, params, grads, w, dout, B, L, NH, EPS, bws=bws, rows=rows, n_rows=n, **kw)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    table = []
    for f in FRACTIONS:
        n = max(1, int(round(f * T)))
        idx = torch.randperm(T, generator=g)[:n].sort().values.to(dev)
        rows = idx.to(torch.int32).contiguous()
        dout = torch.zeros(T, D, device=dev)
        dout[idx] = torch.randn(n, D, generator=g).to(dev)
        leg(None, None, dout), leg(rows, n, dout)      # heat
        full, mapped = [], []
        for _ in range(args.legs):
            full.append(leg(None, None, dout))
            mapped.append(leg(rows, n, dout))
        spread = max(max(full) - min(full), max(mapped) - min(mapped))
        gain = statistics.mean(full) - statistics.mean(mapped)
        row = dict(fraction=round(f, 4), n=n, full_ms=dict(median=round(statistics.median(full), 4), min=round(min(full), 4),
                                                           max=round(max(full), 4)),
                   mapped_ms=dict(median=round(statistics.median(mapped), 4), min=round(min(mapped), 4), max=round(max(mapped), 4)),
                   gain_us=round(1e3 * gain, 1), spread_us=round(1e3 * spread, 1), mapped_faster=bool(gain > spread))
        table.append(row)
        print(json.dumps(row), flush=True)
    ok = [t["fraction"] for t in table if t["mapped_faster"]]
    out = dict(what="one XLNet layer forward + backward, plain vs row-mapped entry, T = 20480, d_model 128, dropout 0.3, "
                    f"{args.legs} interleaved legs of {args.iters} iterations, device events", table=table,
               largest_fraction_mapped_faster=max(ok) if ok else None)
    print(json.dumps({"largest_fraction_mapped_faster": out["largest_fraction_mapped_faster"]}))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
