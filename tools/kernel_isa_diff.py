"""Compare the device code of two builds of the engine, kernel by kernel, without a GPU.

    hipcc --offload-arch=gfx950 <the flags of rmf_crowdsim_amd/_native.py> --cuda-device-only -S -o a.s csrc/crowdstep_hip.hip
    (the same for the other tree, -o b.s)
    python tools/kernel_isa_diff.py a.s b.s

Every function of a.s (from its label to its .Lfunc_end) is compared with the function of the same name in b.s, line
for line, after dropping comments and renumbering local labels (they are numbered through the whole file, so a function
added in front shifts them).  Prints the functions that differ, that exist on one side only, and one summary line; exit
status 1 if a function that both have differs."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";")[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*$", line)
        if m and name is None and not line.startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.strip().startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            body.append(line)
    return out


def canonical(body):
    """local labels by order of first appearance"""
    seen = {}

    def sub(m):
        return seen.setdefault(m.group(0), f".L{len(seen)}")
    return [re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", sub, ln) for ln in body if not ln.strip().startswith((".loc", ".file", ".cfi"))]


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    differ = [n for n in a if n in b and canonical(a[n]) != canonical(b[n])]
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    for n in differ:
        print("DIFFERS", n)
    for n in only_a:
        print("only in", sys.argv[1], n)
    for n in only_b:
        print("only in", sys.argv[2], n)
    same = len([n for n in a if n in b]) - len(differ)
    print(f"{same} functions identical ({sum(len(a[n]) for n in a if n in b and n not in differ)} lines), {len(differ)} differ, "
          f"{len(only_a)} only in the first, {len(only_b)} only in the second")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
