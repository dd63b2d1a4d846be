"""Table of the worst error / bound ratios printed by tests/test_body_split_gpu.py (profiles/body_split_margins.txt):
    python -m pytest tests/test_body_split_gpu.py -q -s | python tools/body_split_margins.py
Rows: kernel and output; columns: input family (A global magnitudes, B per-row magnitudes, C in-row range, D loose activation
bound, E zero operand); entries: worst per-row error / bound over the shapes, and in brackets the worst tensor-relative error as a
fraction of its limit."""
import re
import sys
from collections import defaultdict

ROW = re.compile(r"(ff|proj|oproj|attn_block) (\w+) .*? (\w+):(?: tensor-relative error (\S+) \(limit (\S+)\))?"
                 r"(?: worst error / bound (\S+) \((\d+) rows left out\))?$")
TOK = re.compile(r"tok_gemm (\w+) \S+ tb=\w+: worst error / limit (\S+), tensor-relative (\S+) \(general kernel (\S+)\)")
LAYER = re.compile(r"layer B=(\d+) L=\d+ D=(\d+) p=(\S+) a=(\S+) g=(\S+): worst error / limit (\S+), worst error / e32 (\S+)")
FAMS = "ABCDE"


def main():
    bound, rel, left = defaultdict(float), defaultdict(float), 0
    tok, layer, stale = defaultdict(lambda: [0.0, 0.0]), defaultdict(lambda: [0.0, 0.0]), []
    for line in sys.stdin:
        line = line.rstrip("\n")
        m = ROW.search(line)
        if m:
            key = (m.group(1), m.group(3), m.group(2)[0])
            if m.group(4):
                rel[key] = max(rel[key], float(m.group(4)) / float(m.group(5)))
            if m.group(6):
                bound[key] = max(bound[key], float(m.group(6)))
                left += int(m.group(7))
            continue
        m = TOK.search(line)
        if m:
            t = tok[m.group(1)[0]]
            t[0], t[1] = max(t[0], float(m.group(2))), max(t[1], float(m.group(3)))
            continue
        m = LAYER.search(line)
        if m:
            t = layer[(m.group(2), m.group(3))]
            t[0], t[1] = max(t[0], float(m.group(6))), max(t[1], float(m.group(7)))
            continue
        if "stale maxima" in line:
            stale.append(line[line.index("stale maxima"):])
    print("worst per-row error / bound [worst tensor-relative error / its limit], by kernel output and input family")
    print(f"{'kernel output':<22}" + "".join(f"{f:>16}" for f in FAMS))
    for kern, out in sorted({k[:2] for k in list(bound) + list(rel)}, key=lambda k: (("ff", "proj", "oproj", "attn_block").index(k[0]), k[1])):
        cells = []
        for f in FAMS:
            k = (kern, out, f)
            if k not in bound and k not in rel:
                cells.append(f"{'-':>16}")
                continue
            b = f"{bound[k]:.3f}" if k in bound else "  -  "
            r = f"[{rel[k]:.2f}]" if k in rel else ""
            cells.append(f"{b + ' ' + r:>16}")
        print(f"{kern + ' ' + out:<22}" + "".join(cells))
    print(f"rows left out (fp64 result outside fp32's normal range): {left}")
    print()
    print("token-stationary GEMM (three bf16 planes): worst per-row error / max(bound, 3 e_gen), worst tensor-relative error")
    for f in sorted(tok):
        print(f"  family {f}: {tok[f][0]:.3f}, {tok[f][1]:.2e}")
    print()
    print("whole layer, 15 parameter gradients + out + d h: worst tensor-relative error / max(L0, 4 e32), worst error / e32")
    for (d, p) in sorted(layer):
        print(f"  D={d} p={p}: {layer[(d, p)][0]:.3f}, {layer[(d, p)][1]:.2f}")
    print()
    print("stale maxima (as the whole-layer rows above: the weight-gradient GEMMs forced into the split form that reads the "
          "producers' maxima, ops.precision(\"fp32_bf16x3\"); each test shows it by bits that differ from the fp32 form's)")
    for s in stale:
        print(s)


if __name__ == "__main__":
    main()
