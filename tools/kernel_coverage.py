#!/usr/bin/env python3
"""Which of the library's __global__ instantiations a traced run launched.

    kernel_coverage.py static [objects dir] [-o list.txt]
        the built instantiations: the `__device_stub__` host stubs of the in-tree build's objects (nm -C), one normalised
        name per line, sorted
    kernel_coverage.py report <static list> <rocpd .db> [more .db ...] [--label L] [--commit C] [--command CMD]
        the union of the kernel names in `rocprofv3 --kernel-trace` databases (one per traced process: pass them all) against that list: launched / built per family, the launched values of every template parameter per family, every built name with its
        mark (`L` launched, `-` never launched)

Both sides are normalised the same way (normalise()): `void `, the argument list, `__device_stub__` and a `.kd` suffix go;
namespaces and template arguments stay as the demangler spelt them; whitespace collapses to single blanks.
"""
import argparse
import os
import re
import sqlite3
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ_DIR = os.path.join(ROOT, "hashgan_amd", "_lib", "obj", "prod")
ANON = "(anonymous namespace)"
STUB = "__device_stub__"


def _cut_arguments(name):
    """The name up to the `(` that opens the argument list: the first one outside every `<...>` that is not `(anonymous namespace)`
    (a cast inside template arguments, `(unsigned long)5`, sits inside `<...>`)."""
    depth = 0
    i = 0
    while i < len(name):
        ch = name[i]
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(":
            if name.startswith(ANON, i):
                i += len(ANON)
                continue
            if depth == 0:
                return name[:i]
        i += 1
    return name


def normalise(name):
    name = " ".join(name.split())
    if name.endswith(".kd"):
        name = name[:-3]
    if name.startswith("void "):
        name = name[5:]
    name = _cut_arguments(name).strip()
    return name.replace(STUB, "")


def family(name):
    return name.split("<", 1)[0]


def template_args(name):
    """The top-level template arguments of the kernel itself (the last `<...>` group at depth 0), as the demangler spelt them."""
    if not name.endswith(">"):
        return []
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        if name[i] == ">":
            depth += 1
        elif name[i] == "<":
            depth -= 1
            if depth == 0:
                inner = name[i + 1:-1]
                break
    else:
        return []
    args, depth, cur = [], 0, ""
    for ch in inner:
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    args.append(cur.strip())
    return args


def static_names(obj_dir=OBJ_DIR):
    objs = sorted(os.path.join(obj_dir, f) for f in os.listdir(obj_dir) if f.endswith(".o"))
    if not objs:
        raise RuntimeError("no objects under %s: build the library first (python -m hashgan_amd.build)" % obj_dir)
    out = subprocess.run(["nm", "-C"] + objs, capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        if STUB not in line:
            continue
        m = re.match(r"^(?:[0-9a-fA-F]+)?\s+[A-Za-z]\s+(.*)$", line)
        if m:
            names.add(normalise(m.group(1)))
    return sorted(names)


def traced_names(dbs):
    names = set()
    for path in dbs:
        c = sqlite3.connect(path)
        try:
            rows = c.execute("select distinct name from kernels").fetchall()
        except sqlite3.Error:
            try:
                rows = c.execute("select name from top_kernels").fetchall()
            except sqlite3.Error as e:
                print("# %s: no `kernels` / `top_kernels` view (%s): a process that launched nothing" % (path, e))
                rows = []
        c.close()
        names.update(normalise(r[0]) for r in rows if r[0])
    return names


def _key(v):
    return (0, int(v), "") if re.fullmatch(r"-?\d+", v) else (1, 0, v)


def report_text(built, launched, label="", commit="", command="", ndb=0):
    built = sorted(set(built))
    hit = [n for n in built if n in launched]
    miss = [n for n in built if n not in launched]
    fams = {}
    for n in built:
        fams.setdefault(family(n), []).append(n)
    out = []
    out.append("== kernel coverage%s" % (": " + label if label else ""))
    if commit:
        out.append("# commit: %s" % commit)
    if command:
        out.append("# command: %s" % command)
    out.append("# databases: %d   built: %d   launched: %d   never launched: %d   traced names outside the list: %d" % (
        ndb, len(built), len(hit), len(miss), len(launched - set(built))))
    out.append("-- families (launched / built)")
    for f in sorted(fams, key=lambda f: (-len(fams[f]), f)):
        out.append("%-44s %3d / %3d" % (f, sum(n in launched for n in fams[f]), len(fams[f])))
    out.append("-- template parameters (family [position]: launched values | built values never launched)")
    for f in sorted(fams, key=lambda f: (-len(fams[f]), f)):
        rows = [template_args(n) for n in fams[f]]
        width = max(len(r) for r in rows)
        for p in range(width):
            bv = {r[p] for r in rows if len(r) > p}
            lv = {template_args(n)[p] for n in fams[f] if n in launched and len(template_args(n)) > p}
            out.append("%s [%d]: %s | %s" % (f, p, " ".join(sorted(lv, key=_key)) or "-", " ".join(sorted(bv - lv, key=_key)) or "-"))
    # the rescore kernels' KP x slices product (reported, not required): one row per first argument
    for f in sorted(fams):
        if f.endswith("_rescore") and all(len(template_args(n)) == 2 for n in fams[f]):
            out.append("-- %s: second argument launched per first argument" % f)
            firsts = sorted({template_args(n)[0] for n in fams[f]}, key=_key)
            for a in firsts:
                lv = sorted((template_args(n)[1] for n in fams[f] if n in launched and template_args(n)[0] == a), key=_key)
                out.append("%s <%s, .>: %s" % (f, a, " ".join(lv) or "-"))
    out.append("-- names (L launched, - never launched)")
    for n in built:
        out.append("%s %s" % ("L" if n in launched else "-", n))
    out.append("-- never launched: %d" % len(miss))
    out.extend(miss)
    extra = sorted(n for n in launched - set(built) if "hg::" in n)
    out.append("-- traced names in the library's namespace that the list lacks (a spelling the normaliser misses): %d" % len(extra))
    out.extend(extra)
    out.append("== end")
    return "\n".join(out) + "\n"


def parse_report(text, label=None):
    """{name: launched?} of the report whose header carries `label` (the last report of the text if None)."""
    blocks = re.split(r"(?m)^== kernel coverage", text)[1:]
    if label is not None:
        blocks = [b for b in blocks if b.splitlines()[0].strip().lstrip(": ").startswith(label)]
    if not blocks:
        raise ValueError("no report%s in the text" % (" labelled " + label if label else ""))
    marks = {}
    on = False
    for line in blocks[-1].splitlines():
        if line.startswith("-- "):
            on = line.startswith("-- names")
        elif line.startswith("== end"):
            break
        elif on and line[:2] in ("L ", "- "):
            marks[line[2:]] = line[0] == "L"
    return marks


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("static")
    s.add_argument("obj_dir", nargs="?", default=OBJ_DIR)
    s.add_argument("-o", "--output")
    r = sub.add_parser("report")
    r.add_argument("static_list")
    r.add_argument("db", nargs="+")
    r.add_argument("--label", default="")
    r.add_argument("--commit", default="")
    r.add_argument("--command", default="")
    a = ap.parse_args(argv)
    if a.cmd == "static":
        text = "\n".join(static_names(a.obj_dir)) + "\n"
        if a.output:
            with open(a.output, "w") as f:
                f.write(text)
        else:
            sys.stdout.write(text)
        return 0
    built = [ln.strip() for ln in open(a.static_list) if ln.strip() and not ln.startswith("#")]
    sys.stdout.write(report_text(built, traced_names(a.db), a.label, a.commit, a.command, len(a.db)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
