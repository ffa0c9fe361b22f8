"""Per-kernel comparison of two builds' gfx950 assembly (hipcc --cuda-device-only -S): the resource
figures the compiler records for each kernel and whether the instruction streams are equal once
symbol and label names are normalised.

    python tools/isa_diff.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...] old_substr=new_substr ...

Each pair names one kernel in the old and in the new files by a substring of its mangled name
(the first kernel containing it).  Prints one table row per pair.

    python tools/isa_diff.py --all OLD.s[,...] NEW.s[,...]

pairs every kernel of the two file lists by equal (file stem, mangled name), prints one row per pair and
the kernels present on one side only; exits 1 if there is such a kernel or any column of a row differs.
"""
import difflib
import os
import re
import sys

FIELDS = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("scratch", "ScratchSize"), ("lds", "LDSByteSize"),
          ("occ", "Occupancy"))


def kernels(paths, by_file=False):
    """{mangled name: (normalised instruction list, resource dict)} of the kernels in the files; with
    by_file the key is "file stem:mangled name" (template kernels are emitted in every file that uses them)."""
    out = {}
    for path in paths.split(","):
        stem = os.path.splitext(os.path.basename(path))[0] + ":" if by_file else ""
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
            out[stem + name] = (ins, res)
    return out


def find(ks, sub):
    for name in ks:
        if sub in name:
            return ks[name]
    raise SystemExit(f"no kernel containing {sub!r}")


def main():
    every = sys.argv[1] == "--all"
    args = sys.argv[2:] if every else sys.argv[1:]
    old, new = kernels(args[0], every), kernels(args[1], every)
    print(f"{'kernel (old = new)':58s} {'vgpr':>9s} {'agpr':>9s} {'scratch':>7s} {'lds':>15s} {'occ':>5s} {'instr':>11s}  ISA")
    bad = 0
    for pair in sorted(set(old) & set(new)) if every else args[2:]:
        a, b = (pair, pair) if every else pair.split("=")
        (ia, ra), (ib, rb) = (old[a], new[b]) if every else (find(old, a), find(new, b))
        sm = difflib.SequenceMatcher(None, ia, ib, autojunk=False)
        same = sum(bl.size for bl in sm.get_matching_blocks())
        verdict = "identical" if ia == ib else f"differs ({len(ia) - same} old / {len(ib) - same} new lines unmatched)"
        col = lambda k: f"{ra[k]}/{rb[k]}"  # noqa: E731
        bad += ia != ib or ra != rb
        print(f"{a if every else a + ' = ' + b:58s} {col('vgpr'):>9s} {col('agpr'):>9s} {col('scratch'):>7s} {col('lds'):>15s} "
              f"{col('occ'):>5s} {len(ia):5d}/{len(ib):<5d}  {verdict}")
    if every:
        for side, only in (("old", set(old) - set(new)), ("new", set(new) - set(old))):
            for name in sorted(only):
                print(f"only in {side}: {name}")
            bad += len(only)
        print(f"{len(set(old) & set(new))} kernels paired, {bad} differing or unpaired")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
