"""Compare two device-assembly files function by function.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include [-DENFLOW_NFMAX=16] \
        --cuda-device-only -S -o OLD.s enflow_amd/csrc/enflow_backward.hip      (on the parent)
    ... the same on this tree -> NEW.s
    python tools/asm_functions_diff.py OLD.s NEW.s [--json OUT.json]

A function is everything from its ``.type NAME,@function`` line to its
``; -- End function`` line: the instructions, the ``.amdhsa_kernel`` descriptor
(VGPR / SGPR / scratch / LDS figures) and the ``.set NAME.*`` resource symbols.
A kernel added ahead of another shifts the function index inside the block
labels of those that follow (``.LBB16_3`` becomes ``.LBB20_3``, ``.Lfunc_end16``
``.Lfunc_end20``); that index is masked, nothing else.  Prints the functions
only one side has and those whose masked text differs; exit status 1 if any
function present on both sides differs.
"""
import hashlib
import json
import re
import sys

BEGIN = re.compile(r"^\s*\.type\s+(\S+),@function")
END = re.compile(r";\s*-- End function")
MASK = re.compile(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin|\bBB)\d+")     # labels, and the loop comments that name them
DESC = re.compile(r"^\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size|"
                  r"private_segment_fixed_size)\s+(\S+)")


def functions(path):
    out, name, lines = {}, None, []
    with open(path) as fh:
        for line in fh:
            if name is None:
                m = BEGIN.match(line)
                if m:
                    name, lines = m.group(1), [line]
                continue
            lines.append(line)
            if END.search(line):
                out[name] = [MASK.sub(r"\1#", x.rstrip()) for x in lines]
                name = None
    return out


def summary(lines):
    d = {}
    for x in lines:
        m = DESC.match(x)
        if m:
            d[m.group(1)] = m.group(2)
    d["lines"] = len(lines)
    d["sha256"] = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
    return d


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    old, new = functions(args[0]), functions(args[1])
    common = [k for k in old if k in new]
    differ = [k for k in common if old[k] != new[k]]
    added = [k for k in new if k not in old]
    removed = [k for k in old if k not in new]
    print(f"{len(old)} functions in {args[0]}, {len(new)} in {args[1]}")
    print(f"{len(common) - len(differ)} of {len(common)} common functions identical (block-label index masked)")
    for k in differ:
        print(f"DIFFERS: {k}: {summary(old[k])} -> {summary(new[k])}")
    for k in removed:
        print(f"REMOVED: {k}")
    for k in added:
        print(f"ADDED:   {k}: {summary(new[k])}")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump({"old_functions": len(old), "new_functions": len(new), "common": len(common),
                       "identical": len(common) - len(differ), "differ": differ, "removed": removed,
                       "added": {k: summary(new[k]) for k in added},
                       "common_functions": {k: summary(new[k]) for k in common}}, fh, indent=1)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
