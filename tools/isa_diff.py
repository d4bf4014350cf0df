#!/usr/bin/env python3
"""Compare the device assembly of two builds, kernel by kernel.

    python3 tools/isa_diff.py DIR_A DIR_B [--diff-lines N] [--rename REGEX REPL]...

DIR_A and DIR_B hold the `hipcc --cuda-device-only -S` output of the same translation units (any *.s below them).  Per function symbol
the tool reports: equal text in both, different text (with a short unified diff), only in A, only in B.  "Text" is the function body
from its label to its .Lfunc_end label plus its .amdhsa_kernel ... .end_amdhsa_kernel descriptor.  Local labels that carry the index of
the function inside its file (.LBB<i>_<n>, .LJTI<i>_<n>, .Ltmp<n>, .Lfunc_end<i>) are renumbered by order of first appearance inside
the function, so a kernel compares equal when kernels in front of it came or went; the blanks in front of a comment count as one (the
compiler pads a label's comment to a column, so the padding moves with the width of the index).  __hip_cuid_* is ignored.  --rename REGEX REPL (may
be repeated) is re.sub applied to every line of A, symbols included, before anything is compared: a kernel that lost a template argument
has another mangled name in B, and compares equal to its form in A once A's name is rewritten.  The comparison is of text alone.  Exit
status 1 when a symbol differs or exists in B only.
"""
import argparse
import difflib
import pathlib
import re
import sys

TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
DESC_BEGIN = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
DESC_END = re.compile(r"^\s*\.end_amdhsa_kernel")
PAD = re.compile(r"[ \t]+;")
LOCAL = re.compile(r"(?:\.L|\b)(BB|JTI)\d+_(\d+)|\.L(tmp)(\d+)|\.L(func_end)\d+")      # the compiler's loop comments say BB<i>_<n> without .L


def renumber(lines):
    seen = {}

    def sub(m):
        kind = m.group(1) or m.group(3) or m.group(5)
        if kind == "func_end":
            return ".Lfunc_end"
        key = (kind, m.group(2) or m.group(4))
        if key not in seen:
            seen[key] = sum(1 for k in seen if k[0] == kind)
        return "%s%s_%d" % (".L" if m.group(0).startswith(".L") else "", kind, seen[key])

    return [PAD.sub(" ;", LOCAL.sub(sub, ln)) for ln in lines]


def functions(text):
    """{symbol: [lines]} of one assembly file."""
    body, desc = {}, {}
    pending, cur, in_desc = set(), None, None
    for ln in text.splitlines():
        ln = ln.rstrip()
        m = TYPE.match(ln)
        if m:
            pending.add(m.group(1))
        m = DESC_BEGIN.match(ln)
        if m:
            in_desc = m.group(1)
            desc[in_desc] = []
        if in_desc is not None:
            desc[in_desc].append(ln)
            if DESC_END.match(ln):
                in_desc = None
            continue
        if cur is None:
            name = ln.split(":", 1)[0] if ":" in ln else None
            if name in pending and not name.startswith("__hip_cuid_"):
                pending.discard(name)
                cur = name
                body[cur] = [ln]
        else:
            body[cur].append(ln)
            if FUNC_END.match(ln):
                cur = None
    return {name: renumber(lines + desc.get(name, [])) for name, lines in body.items()}


def rename(text, renames):
    for pattern, repl in renames:
        text = re.sub(pattern, repl, text)
    return text


def load(root, renames=()):
    out = {}
    for path in sorted(pathlib.Path(root).rglob("*.s")):
        for name, lines in functions(rename(path.read_text(), renames)).items():
            out["%s: %s" % (path.relative_to(root), name)] = lines      # per file: several units may instantiate the same template
    return out


def compare(a, b):
    equal = sorted(n for n in a if n in b and a[n] == b[n])
    differ = sorted(n for n in a if n in b and a[n] != b[n])
    return equal, differ, sorted(set(a) - set(b)), sorted(set(b) - set(a))


def report(a, b, diff_lines=40, out=sys.stdout):
    equal, differ, only_a, only_b = compare(a, b)
    print("equal: %d  different: %d  only in A: %d  only in B: %d" % (len(equal), len(differ), len(only_a), len(only_b)), file=out)
    for n in differ:
        print("DIFFERENT %s" % n, file=out)
        for ln in list(difflib.unified_diff(a[n], b[n], "A", "B", lineterm="", n=1))[:diff_lines]:
            print("    " + ln, file=out)
    for n in only_a:
        print("ONLY IN A %s" % n, file=out)
    for n in only_b:
        print("ONLY IN B %s" % n, file=out)
    return 1 if differ or only_b else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--diff-lines", type=int, default=40)
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    args = ap.parse_args()
    sys.exit(report(load(args.dir_a, args.rename), load(args.dir_b), args.diff_lines))
