"""Table of the worst error / bound ratios printed by tests/test_attn_core_gpu.py (profiles/attn_core_margins.txt):
    python -m pytest tests/test_attn_core_gpu.py -q -s -m gpu | python tools/attn_core_margins.py
Rows: kernel group and output; columns: input family (M: key_len edges on U and on O-; /drop: dropout 0.3); entries: the worst
|error| / bound over every element of every shape of the group.  Below the table: the smallest C_EXP that puts each kernel group
at <= 0.5 of its bound on the unit-scale family."""
import re
import sys
from collections import defaultdict

ROW = re.compile(r"attn_core (\S+) (\S+) B=.*? ((?:fused |separate |prob-path )?[\w-]+): worst error / bound (\S+)$")
CEXP = re.compile(r"attn_core (\S+) U B=.*?((?: fused| separate| prob-path)?) smallest C_EXP for 0\.5: (.+)$")
FAMS = ("U", "P", "A+", "A-", "O+", "O-", "E", "Z1", "Z2", "M/U", "M/O-", "U/drop", "P/drop", "S70", "M/S70")


def main():
    worst, cexp = defaultdict(float), defaultdict(int)
    for line in sys.stdin:
        line = line.strip()
        m = ROW.search(line)
        if m:
            key = (m.group(1), m.group(3), m.group(2))
            worst[key] = max(worst[key], float(m.group(4)))
            continue
        m = CEXP.search(line)
        if m:
            key = m.group(1) + m.group(2)
            cexp[key] = max(cexp[key], 65 if m.group(3).startswith("above") else int(m.group(3)))
    fams = [f for f in FAMS if any(k[2] == f for k in worst)]
    print("worst |error| / bound over every element, by kernel group, output and input family")
    print(f"{'kernel group, output':<34}" + "".join(f"{f:>8}" for f in fams))
    for group, out in sorted({k[:2] for k in worst}):
        cells = "".join(f"{worst[(group, out, f)]:>8.3f}" if (group, out, f) in worst else f"{'-':>8}" for f in fams)
        print(f"{group + ' ' + out:<34}" + cells)
    print()
    print("smallest C_EXP that puts every output of the unit-scale family at <= 0.5 of its bound")
    for key in sorted(cexp):
        print(f"  {key:<24} {cexp[key] if cexp[key] < 65 else 'above 64'}")
    print(f"overall worst ratio: {max(worst.values()):.3f}")


if __name__ == "__main__":
    main()
