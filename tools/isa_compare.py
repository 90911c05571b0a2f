"""Compare the kernels of two device-assembly files (hipcc -S --cuda-device-only), symbol by symbol.

    python tools/isa_compare.py OLD.s NEW.s

Prints one line per kernel: symbol, instruction count, and same / DIFFERENT / removed / ADDED.  "same" = identical
instruction stream (labels renumbered per function, comments dropped) and identical .amdhsa_ directives.
Exit status 1 if a kernel differs or exists only in NEW."""
import re
import sys


def kernels(path):
    """symbol -> (instructions, .amdhsa_ directives)"""
    out, body, hsa, cur, in_hsa = {}, {}, {}, None, None
    for raw in open(path):
        line = raw.split(";")[0].strip()
        if not line:
            continue
        if line.startswith(".amdhsa_kernel "):
            in_hsa = line.split()[1]
            hsa[in_hsa] = []
        elif line == ".end_amdhsa_kernel":
            in_hsa = None
        elif in_hsa:
            hsa[in_hsa].append(line)
        elif re.fullmatch(r"\.Lfunc_end\d+:", line):
            cur = None
        elif re.fullmatch(r"[A-Za-z_][\w$.]*:", line) and not line.startswith(".L"):
            cur = line[:-1]
            body[cur] = []
        elif cur is not None and not (line.startswith(".") and not line.startswith(".LBB")):
            body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    for sym, directives in hsa.items():
        out[sym] = (body[sym], directives)          # block labels stay in the stream: a moved label is a difference
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in new:
            verdict = "removed"
        elif sym not in old:
            verdict, bad = "ADDED", 1
        elif old[sym] == new[sym]:
            verdict = "same"
        else:
            verdict, bad = "DIFFERENT", 1
        count = sum(not i.endswith(":") for i in (old.get(sym) or new[sym])[0])
        print(f"{sym}  {count}  {verdict}")
    print(f"# {len(old)} kernels before, {len(new)} after")
    return bad


if __name__ == "__main__":
    sys.exit(main())
