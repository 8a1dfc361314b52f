#!/usr/bin/env python3
"""Merge gcov's JSON output (one document per object of the emulation build, tools/emu_coverage.sh) into the text report
profiles/emu_coverage.txt:

  1. per source file of gnark_amd/csrc, the lines that no object executed;
  2. per device header and per object, the lines inside kernels and device functions that this object compiled and never executed.
     A template is instantiated per curve and group, and the lazy bounds (tools/lazy_bounds.py) are proved per field, so a line that
     ran for another field did not run for this one.  Host functions are left out of part 2: the inline host helpers of a header
     are compiled into every object and called from one.

A line counts as executed when any of its instantiations has a non-zero count.  Ranges bridge the lines gcov has no counter for
(comments, braces), never an executed line.

  emu_coverage_merge.py <csrc directory> <directory of *.json> [headline]"""
import bisect
import json
import os
import re
import sys


def ranges(lines, executed):
    """'137-142, 380' for the sorted line numbers `lines`; two lines join when no executed line lies between them"""
    out, lines = [], sorted(lines)
    ex = sorted(executed)
    i = 0
    while i < len(lines):
        j = i
        while j + 1 < len(lines) and not ex_between(ex, lines[j], lines[j + 1]):
            j += 1
        out.append(str(lines[i]) if i == j else "%d-%d" % (lines[i], lines[j]))
        i = j + 1
    return ", ".join(out)


def ex_between(ex, lo, hi):
    return ex[bisect.bisect_right(ex, lo):bisect.bisect_left(ex, hi)]


def device_spans(path):
    """[(first line, last line)] of the bodies of the functions of `path` declared __global__ or __device__, from the source text (an
    always-inline device function has no function record of its own in gcov's output: its lines are counted in the kernels that
    inline it).  Lambdas inside a kernel lie within its span."""
    try:
        text = open(path, errors="replace").read()
    except OSError:
        return []
    # comments are blanked (line breaks kept) before braces are counted; the headers hold no string literal with a brace in it
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
    spans = []
    for m in re.finditer(r"__global__|__device__", text):
        if spans and m.start() < spans[-1][2]:
            continue
        k, depth = m.end(), 0
        while k < len(text) and not (text[k] == "{" and depth == 0):   # the body's brace: the first one outside the parameter list
            if text[k] == ";" and depth == 0:
                break                                                  # a declaration only
            depth += text[k] == "("
            depth -= text[k] == ")"
            k += 1
        if k >= len(text) or text[k] != "{":
            continue
        e, depth = k, 0
        while e < len(text):
            depth += text[e] == "{"
            depth -= text[e] == "}"
            if depth == 0:
                break
            e += 1
        spans.append((text.count("\n", 0, m.start()) + 1, text.count("\n", 0, e) + 1, e))
    return [(a, b) for a, b, _ in spans]


def main():
    csrc, jdir = os.path.realpath(sys.argv[1]), sys.argv[2]
    headline = re.sub(r"\s+in [0-9.]+s.*$", "", sys.argv[3].strip("= \n")) if len(sys.argv) > 3 else ""
    objs = sorted(f[:-5] for f in os.listdir(jdir) if f.endswith(".json"))
    hit, seen = {}, {}                       # file -> lines executed / instrumented, in any object
    per_obj = {}                             # (file, object) -> (instrumented, executed)
    for o in objs:
        doc = json.load(open(os.path.join(jdir, o + ".json")))
        for fr in doc["files"]:
            path = os.path.realpath(os.path.join(csrc, fr["file"]))
            if os.path.dirname(path) != csrc:
                continue
            name = os.path.basename(path)
            ins = {l["line_number"] for l in fr["lines"]}
            exe = {l["line_number"] for l in fr["lines"] if l["count"] > 0}
            seen.setdefault(name, set()).update(ins)
            hit.setdefault(name, set()).update(exe)
            a, b = per_obj.setdefault((name, o), (set(), set()))
            a.update(ins)
            b.update(exe)
    total = sum(len(v) for v in seen.values())
    done = sum(len(v) for v in hit.values())
    print("# Lines of gnark_amd/csrc that the CPU suite executes on the emulation build (tools/emu_coverage.sh)")
    if headline:
        print("# suite: " + headline)
    print("# %d objects, %d of %d instrumented lines executed in at least one object (%.2f %%)" % (len(objs), done, total, 100.0 * done / max(1, total)))
    print()
    print("## 1. per source file: lines never executed in any object")
    for name in sorted(seen):
        miss = seen[name] - hit[name]
        if miss:
            print("%s (%d of %d): %s" % (name, len(miss), len(seen[name]), ranges(miss, hit[name])))
    print()
    print("## 2. per device header and object: lines inside kernels and device functions never executed in that object")
    print("##    (lines of part 1 are not repeated)")
    for name in sorted(seen):
        if name.endswith(".hip"):
            continue
        spans = device_spans(os.path.join(csrc, name))
        inside = lambda n: any(s <= n <= e for s, e in spans)
        rows = []
        for o in objs:
            if (name, o) not in per_obj:
                continue
            ins, exe = per_obj[(name, o)]
            miss = {n for n in ins - exe if n in hit[name] and inside(n)}
            if miss:
                rows.append("  %s (%d): %s" % (o, len(miss), ranges(miss, exe)))
        if rows:
            print(name)
            print("\n".join(rows))


if __name__ == "__main__":
    main()
