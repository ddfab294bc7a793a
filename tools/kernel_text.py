"""Compare the device code of two builds function by function, as text.

    hipcc <the Makefile's FLAGS> --offload-device-only -S old/pm_x.hip -o A.s
    hipcc <the Makefile's FLAGS> --offload-device-only -S new/pm_x.hip -o B.s
    python tools/kernel_text.py A.s B.s
    python tools/kernel_text.py A.s --union B1.s B2.s ...   (several files as one side: a split unit)

Per function: the instruction count on each side, VGPR / AGPR / SGPR, LDS bytes, scratch, occupancy
and kernel-argument bytes from the function's metadata, and IDENTICAL or DIFFER with the number of
differing lines. The text is normalised as the records under profiles/ did by hand: directives,
comments, blank lines and label definitions are dropped, and every .L reference becomes one token.
Exit status 1 if a function present on both sides differs (text or resources) or a function of A is
missing from B. No compiler and no GPU is used: a kernel's timing here moves with how it is compiled,
so this comparison comes before any measurement (DESIGN.md "The self-play learner's units").
"""
import argparse
import difflib
import re
import sys

FIELDS = ("VGPR", "AGPR", "SGPR", "LDS", "scratch", "occupancy", "kernarg")
_META = {"NumVgprs": "VGPR", "NumAgprs": "AGPR", "TotalNumSgprs": "SGPR", "NumSgprs": "SGPR",
         "LDSByteSize": "LDS", "ScratchSize": "scratch", "Occupancy": "occupancy"}
_TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_LREF = re.compile(r"\.L[\w.$]+")
_INFO = re.compile(r"^;\s*(\w+)\s*[:=]\s*(\d+)")
_KERNARG = re.compile(r"^\s*\.amdhsa_kernarg_size\s+(\d+)")


class Function:
    def __init__(self):
        self.text = []  # normalised instruction lines
        self.res = {}   # FIELDS -> int, where the metadata has them


def parse(asm):
    """{function name: Function} of one `-S` output."""
    out, names, cur, info = {}, set(), None, None
    for raw in asm.splitlines():
        m = _TYPE.match(raw)
        if m:
            names.add(m.group(1))
            continue
        lab = _LABEL.match(raw)
        if lab and lab.group(1) in names and lab.group(1) not in out:
            cur = info = out[lab.group(1)] = Function()
            continue
        if cur is not None:  # inside a body
            if lab and lab.group(1).startswith(".Lfunc_end"):
                cur = None
                continue
            m = _KERNARG.match(raw)
            if m:
                cur.res["kernarg"] = int(m.group(1))
            line = raw.split(";", 1)[0].strip()
            if not line or line.startswith(".") or _LABEL.match(line):
                continue  # blank / comment, directive, label definition
            cur.text.append(_LREF.sub(".L", " ".join(line.split())))
        elif info is not None:  # the metadata comment block after a body
            m = _INFO.match(raw)
            if m and m.group(1) in _META:
                info.res.setdefault(_META[m.group(1)], int(m.group(2)))
    return out


def parse_union(texts):
    """Several outputs as one side; a function defined in more than one keeps its first definition."""
    out = {}
    for t in texts:
        for name, f in parse(t).items():
            out.setdefault(name, f)
    return out


def differing_lines(a, b):
    """Lines that an alignment of the two texts leaves unmatched (the longer side of every changed run)."""
    lo = 0
    while lo < len(a) and lo < len(b) and a[lo] == b[lo]:
        lo += 1
    hi = 0
    while hi < len(a) - lo and hi < len(b) - lo and a[len(a) - 1 - hi] == b[len(b) - 1 - hi]:
        hi += 1
    a, b = a[lo:len(a) - hi], b[lo:len(b) - hi]
    ops = difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


def compare(fa, fb):
    """Rows (name, n_a, n_b, res_a, res_b, verdict) for every function of A, then B's extras; and the exit status."""
    rows, bad = [], 0
    for name, a in fa.items():
        b = fb.get(name)
        if b is None:
            rows.append((name, len(a.text), None, a.res, {}, "MISSING in B"))
            bad = 1
            continue
        if a.text != b.text:
            verdict = f"DIFFER ({differing_lines(a.text, b.text)} lines)"
        elif a.res != b.res:
            verdict = "RESOURCES DIFFER"
        else:
            verdict = "IDENTICAL"
        bad |= verdict != "IDENTICAL"
        rows.append((name, len(a.text), len(b.text), a.res, b.res, verdict))
    for name, b in fb.items():
        if name not in fa:
            rows.append((name, None, len(b.text), {}, b.res, "only in B"))
    return rows, bad


def _res(r):
    return " ".join("-" if k not in r else str(r[k]) for k in FIELDS)


def report(rows, out=sys.stdout):
    print("function | instructions A B | " + " ".join(FIELDS) + " (A) | (B) | verdict", file=out)
    for name, na, nb, ra, rb, verdict in rows:
        print(f"{name} | {'-' if na is None else na} {'-' if nb is None else nb} | {_res(ra)} | {_res(rb)} | {verdict}",
              file=out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a", help="side A: one --offload-device-only -S output")
    ap.add_argument("b", nargs="?", help="side B: one output")
    ap.add_argument("--union", nargs="+", metavar="B.s", help="side B: several outputs taken as one")
    args = ap.parse_args(argv)
    if (args.b is None) == (args.union is None):
        ap.error("give side B as one file or as --union files")
    with open(args.a) as f:
        fa = parse(f.read())
    texts = []
    for path in [args.b] if args.b else args.union:
        with open(path) as f:
            texts.append(f.read())
    rows, bad = compare(fa, parse_union(texts))
    report(rows)
    return bad


if __name__ == "__main__":
    sys.exit(main())
