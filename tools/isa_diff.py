"""Per-kernel comparison of two builds' gfx950 assembly (hipcc --cuda-device-only -S): the resource
figures the compiler records for each kernel and whether the instruction streams are equal once
symbol and label names are normalised.

    python tools/isa_diff.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...] old_substr=new_substr ...

Each pair names one kernel in the old and in the new files by a substring of its mangled name
(the first kernel containing it).  Prints one table row per pair.
"""
import difflib
import re
import sys

FIELDS = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("scratch", "ScratchSize"), ("lds", "LDSByteSize"),
          ("occ", "Occupancy"))


def kernels(paths):
    """{mangled name: (normalised instruction list, resource dict)} of the kernels in the files."""
    out = {}
    for path in paths.split(","):
        text = open(path).read()
        # a kernel's body runs from its label to .Lfunc_end; its "Kernel info" comment block follows
        for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:(.*?); Occupancy: (\d+)", text, re.S | re.M):
            name, body, info, _ = m.groups()
            info = m.group(3) + m.group(0)[-20:]
            if "; Kernel info:" not in info:
                continue
            ins = []
            for line in body.split("\n"):
                line = line.split(";")[0].strip()
                if not line or line.startswith((".p2align", ".loc", ".file", ".cfi")):
                    continue
                line = re.sub(r"\.LBB\d+_", ".LBB_", line)
                line = re.sub(r"_Z\w+", "SYM", line)
                ins.append(line)
            res = {k: int(re.search(rf"; {key}: (\d+)", info).group(1)) for k, key in FIELDS}
            out[name] = (ins, res)
    return out


def find(ks, sub):
    for name in ks:
        if sub in name:
            return ks[name]
    raise SystemExit(f"no kernel containing {sub!r}")


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    print(f"{'kernel (old = new)':58s} {'vgpr':>9s} {'agpr':>9s} {'scratch':>7s} {'lds':>15s} {'occ':>5s} {'instr':>11s}  ISA")
    for pair in sys.argv[3:]:
        a, b = pair.split("=")
        (ia, ra), (ib, rb) = find(old, a), find(new, b)
        sm = difflib.SequenceMatcher(None, ia, ib, autojunk=False)
        same = sum(bl.size for bl in sm.get_matching_blocks())
        verdict = "identical" if ia == ib else f"differs ({len(ia) - same} old / {len(ib) - same} new lines unmatched)"
        col = lambda k: f"{ra[k]}/{rb[k]}"  # noqa: E731
        print(f"{a + ' = ' + b:58s} {col('vgpr'):>9s} {col('agpr'):>9s} {col('scratch'):>7s} {col('lds'):>15s} "
              f"{col('occ'):>5s} {len(ia):5d}/{len(ib):<5d}  {verdict}")


if __name__ == "__main__":
    main()
