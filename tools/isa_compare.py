"""Compare the kernels of two device-assembly files (hipcc -S --cuda-device-only), symbol by symbol.

    python tools/isa_compare.py [--map OLD_SYMBOL=NEW_SYMBOL | --map FILE]... [--diff] OLD.s NEW.s

Prints one line per kernel: symbol, instruction count, and same / DIFFERENT / removed / ADDED.  "same" = identical
instruction stream (labels renumbered per function, comments dropped) and identical .amdhsa_ directives.
--map: a kernel that was renamed (a hand-written kernel that became a template instantiation) is compared under its old symbol
and printed as "OLD -> NEW"; FILE holds one OLD=NEW pair per line.  --diff: the differing lines of every DIFFERENT kernel.
Exit status 1 if a kernel differs or exists only in NEW."""
import difflib
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
    args, renamed, show = sys.argv[1:], {}, False
    while args and args[0].startswith("--"):
        if args[0] == "--diff":
            show, args = True, args[1:]
            continue
        if args[0] != "--map" or len(args) < 2:
            sys.exit(f"{args[0]}: unknown option, or --map without a value\n{__doc__}")
        pairs = [args[1]] if "=" in args[1] else [ln.strip() for ln in open(args[1]) if ln.strip()]
        for pair in pairs:
            if pair.count("=") != 1:
                sys.exit(f"--map: {pair!r} is not OLD_SYMBOL=NEW_SYMBOL")
            renamed.update([pair.split("=")])
        args = args[2:]
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = kernels(args[0]), kernels(args[1])
    for was, now in renamed.items():          # the new kernel is compared in the old one's place, its own name in the stream rewritten too
        if was in old and now in new:
            new[was] = tuple([line.replace(now, was) for line in part] for part in new.pop(now))
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
        name = f"{sym} -> {renamed[sym]}" if sym in renamed and sym in old and sym in new else sym
        print(f"{name}  {count}  {verdict}")
        if show and verdict == "DIFFERENT":
            for part, what in zip(zip(old[sym], new[sym]), ("instructions", ".amdhsa_ directives")):
                for line in difflib.unified_diff(*part, "before", "after", n=0, lineterm=""):
                    print(f"    {what}: {line}" if line.startswith("@@") else f"    {line}")
    print(f"# {len(old)} kernels before, {len(new)} after")
    return bad


if __name__ == "__main__":
    sys.exit(main())
