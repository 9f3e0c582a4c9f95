"""Compare the resource figures of kernels in two device-assembly files.

    python tools/asm_resources_diff.py OLD.s NEW.s [NAME_SUBSTRING ...]

Reads the ``amdhsa.kernels`` metadata at the end of each file (hipcc
--cuda-device-only -S) and prints, for every kernel of OLD.s whose name holds one
of the substrings (default: all), its VGPR / AGPR / SGPR counts, VGPR and SGPR
spill counts, scratch (private segment) and LDS (group segment) sizes, and what
they became in NEW.s.  Exit status 1 if any figure changed or a kernel is missing.
"""
import re
import sys

KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path):
    out, cur, in_md = [], None, False
    with open(path) as fh:
        for line in fh:
            if "amdhsa.kernels:" in line:
                in_md = True
            if not in_md:
                continue
            m = re.match(r"  (?:- |  )(\.[a-z_]+):\s*(\S+)", line)
            if not m:
                continue
            if line.startswith("  - "):
                cur = {}
                out.append(cur)
            if cur is not None and (m.group(1) in KEYS or m.group(1) == ".name"):
                cur[m.group(1)] = m.group(2)
    return {d[".name"]: d for d in out if ".name" in d}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    subs = sys.argv[3:]
    bad = 0
    for name in sorted(old):
        if subs and not any(s in name for s in subs):
            continue
        o, n = old[name], new.get(name)
        fig = " ".join(f"{k[1:]}={o.get(k)}" for k in KEYS)
        if n is None:
            bad += 1
            print("MISSING", name, fig)
        elif all(o.get(k) == n.get(k) for k in KEYS):
            print("same   ", name, fig)
        else:
            bad += 1
            print("CHANGED", name, fig, "->", " ".join(f"{k[1:]}={n.get(k)}" for k in KEYS))
    print(f"{bad} kernel(s) with changed resource figures")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
