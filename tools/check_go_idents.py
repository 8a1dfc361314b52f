#!/usr/bin/env python3
"""Resolve every package-qualified identifier of the Go shim (go/**) without a Go toolchain (there is none in the build image).

For every `alias.Ident` in a .go file whose alias is an import of
  * github.com/consensys/gnark/<path>     -> the identifier must be DECLARED (func / type / const / var, exported) in a non-test
                                             .go file of the reference's <path>, or of go/<path> for the shim's own packages;
  * github.com/consensys/gnark-crypto/... -> the module is not in the reference (go.mod dependency): the same `pkg.Ident`
                                             must be USED somewhere in the reference with the same import path (gnark itself
                                             compiles against it, so the name exists in the pinned version);
  * the standard library                   -> checked against a small allow-list of the packages the shim uses;
  * "C"                                    -> `C.ga_*` must be a prototype of include/gnark_amd.h with the SAME NUMBER of
                                             arguments at the call site; `C.GA_*` must be a #define of the header; a handful of
                                             cgo built-ins (C.int, C.GoString, ...) are allowed.
Methods and struct fields (x.Method() on values) are out of reach of a textual check and are not claimed.
Every hunk of a patch shipped under go/** (prove.patch, internal/fixtures/groth16_rs_*.patch) must also find the lines it replaces
exactly where it says, in the reference file it names: the patch applies without offset or fuzz.

"The reference" is the gnark source tree go/** is written against.  With `--reference DIR` the check reads that tree; without it, it
reads tests/golden/reference_go_index.json, the part of the tree the check needs (package names, the exported declarations of the
packages the shim imports, the gnark-crypto identifiers the tree uses, a SHA-256 of the lines every patch hunk replaces), which
`--reference DIR --write-index tests/golden/reference_go_index.json` regenerates.

  python tools/check_go_idents.py            # prints a report, exit code 1 on any unresolved identifier or stale patch hunk
  python tools/check_go_idents.py --json go/IDENTS.json   # also writes the resolved table (committed, reviewed by the test)
"""
import argparse
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX = os.path.join(ROOT, "tests", "golden", "reference_go_index.json")
GNARK = "github.com/consensys/gnark/"
CRYPTO = "github.com/consensys/gnark-crypto/"
SHIM_PREFIX = "backend/accelerated/mi355x"

STDLIB = {
    "fmt": {"Errorf", "Sprintf", "Println", "Printf", "Sprint", "Fprintf"}, "errors": {"New", "Is", "As"},
    "os": {"Open", "File", "Getenv", "Create", "Remove", "CreateTemp", "ReadFile", "WriteFile", "MkdirAll"}, "slices": {"Equal", "Clone", "Concat", "Sort", "Compact", "Contains"},
    "sync": {"Mutex", "RWMutex", "Once", "WaitGroup"}, "time": {"Now", "Since", "Duration"}, "unsafe": {"Pointer", "Sizeof", "SliceData", "Slice", "Add"},
    "runtime": {"Pinner", "KeepAlive", "LockOSThread", "UnlockOSThread", "NumCPU"}, "math/big": {"Int", "NewInt"}, "io": {"Reader", "Writer", "ReaderFrom", "WriterTo"},
    "bytes": {"Buffer", "NewReader", "Equal"}, "testing": {"T", "B", "Short"}, "math/bits": {"Len64", "TrailingZeros64"}, "hash": {"Hash"},
    "context": {"Context", "Background"}, "strings": {"Join", "Split", "HasPrefix"}, "sort": {"Slice", "Ints"}, "path/filepath": {"Join"},
    "encoding/json": {"MarshalIndent", "Marshal"},
    "crypto/sha256": {"New", "Sum256"}, "encoding/binary": {"BigEndian", "LittleEndian", "Write", "Read"},
}
CGO_BUILTINS = {"int", "uint", "uint32_t", "uint64_t", "int32_t", "size_t", "char", "uchar", "GoString", "CString", "free", "malloc", "calloc", "GoBytes",
                "uint8_t", "uintptr_t", "longlong", "ulonglong", "ulong", "long", "double", "float", "uint16_t", "int64_t", "schar", "short", "ushort"}


def go_files(top):
    for d, _, fs in os.walk(top):
        for f in fs:
            if f.endswith(".go"):
                yield os.path.join(d, f)


def strip_comments_and_strings(src):
    src = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r'`[^`]*`', '""', src)
    src = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', src)
    return src


def imports_of(src):
    """alias -> import path"""
    out = {}
    block = re.search(r"^import\s*\((.*?)^\)", src, flags=re.S | re.M)
    lines = block.group(1).splitlines() if block else []
    lines += re.findall(r'^import\s+((?:\w+\s+)?"[^"]+")', src, flags=re.M)
    for ln in lines:
        m = re.match(r'\s*(?:(\w+|\.|_)\s+)?"([^"]+)"', ln)
        if m:
            path = m.group(2)
            alias = m.group(1) or default_alias(path)
            out[alias] = path
    return out


_PKG_NAME_CACHE = {}


def default_alias(path):
    """package name of an import path: the `package x` clause when the directory is known (reference / shim), else the last element"""
    if path in _PKG_NAME_CACHE:
        return _PKG_NAME_CACHE[path]
    name = path.rsplit("/", 1)[-1]
    d = None
    if path.startswith(GNARK):
        rel = path[len(GNARK):]
        if os.path.isdir(os.path.join(ROOT, "go", rel)):
            d = os.path.join(ROOT, "go", rel)
        elif REF.package_name(rel):
            name = REF.package_name(rel)
    if d:
        name = package_clause(d) or name
    _PKG_NAME_CACHE[path] = name
    return name


def package_clause(d):
    for f in sorted(os.listdir(d)):
        if f.endswith(".go") and not f.endswith("_test.go"):
            m = re.search(r"^package\s+(\w+)", open(os.path.join(d, f)).read(), flags=re.M)
            if m:
                return m.group(1)
    return None


_DECL_CACHE = {}


def declared_in(dirpath):
    """exported top-level identifiers declared in the non-test .go files of a package directory"""
    if dirpath in _DECL_CACHE:
        return _DECL_CACHE[dirpath]
    names = set()
    if os.path.isdir(dirpath):
        for f in os.listdir(dirpath):
            if not f.endswith(".go") or f.endswith("_test.go"):
                continue
            src = strip_comments_and_strings(open(os.path.join(dirpath, f)).read())
            names |= set(re.findall(r"^func\s+([A-Z]\w*)\s*[\(\[]", src, flags=re.M))
            names |= set(re.findall(r"^type\s+([A-Z]\w*)\b", src, flags=re.M))
            names |= set(re.findall(r"^(?:var|const)\s+([A-Z]\w*)\b", src, flags=re.M))
            for blk in re.findall(r"^(?:var|const|type)\s*\((.*?)^\)", src, flags=re.S | re.M):
                names |= set(re.findall(r"^\s*([A-Z]\w*)\b", blk, flags=re.M))
    _DECL_CACHE[dirpath] = names
    return names


def declared_by_patches():
    """exported identifiers ADDED to a reference package by a patch shipped under go/** (prove.patch: the PLONK Accelerator hooks;
    internal/fixtures/groth16_rs_*.patch: the test-only TestingHooks of the Groth16 prover): package dir -> {ident: patch}"""
    out = {}
    for d, _, fs in os.walk(os.path.join(ROOT, "go")):
        for f in fs:
            if not f.endswith(".patch"):
                continue
            pkg = None
            for line in open(os.path.join(d, f)):
                if line.startswith("+++ "):
                    m = re.match(r"\+\+\+ [ab]/(\S+)", line)
                    pkg = os.path.dirname(m.group(1)) if m else None
                elif pkg and line.startswith("+") and not line.startswith("+++"):
                    m = re.match(r"\+(?:func|type|var|const)\s+([A-Z]\w*)\b", line)
                    if m:
                        out.setdefault(pkg, {})[m.group(1)] = os.path.relpath(os.path.join(d, f), ROOT)
    return out


def used_in_reference(import_path, ident):
    """is `<alias>.<ident>` used in a reference file that imports import_path (under whatever alias)?"""
    return ident in REF.crypto_uses(import_path)


def patch_hunks(path):
    """(target file, old start line, old line count, the old lines) of every hunk of a unified diff"""
    out, target, lines = [], None, open(path).read().split("\n")
    i = 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("--- "):
            target = re.sub(r"^a/", "", ln[4:].split("\t")[0].strip())
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@", ln)
        if m:
            start, count = int(m.group(1)), int(m.group(2) or "1")
            old, j = [], i + 1
            while len(old) < count and j < len(lines):
                if lines[j][:1] in (" ", "-"):
                    old.append(lines[j][1:])
                elif lines[j][:1] != "+" and not lines[j].startswith("\\"):
                    break
                j += 1
            out.append((target, start, count, old))
            i = j
            continue
        i += 1
    return out


def text_sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


class TreeReference:
    """the reference source tree itself; records what it was asked, which is the index (write_index)"""

    def __init__(self, top):
        self.top = top
        self.names, self.decls, self.uses, self.hunks = {}, {}, {}, {}

    def package_name(self, rel):
        if rel not in self.names:
            d = os.path.join(self.top, rel)
            self.names[rel] = package_clause(d) if os.path.isdir(d) else None
        return self.names[rel]

    def declared(self, pkg):
        if pkg not in self.decls:
            self.decls[pkg] = declared_in(os.path.join(self.top, pkg))
        return self.decls[pkg]

    def crypto_uses(self, import_path):
        if import_path not in self.uses:
            uses = set()
            for f in go_files(self.top):
                try:
                    raw = open(f).read()
                except OSError:
                    continue
                if '"%s"' % import_path not in raw:
                    continue
                src = strip_comments_and_strings(raw)
                for alias, path in imports_of(raw).items():
                    if path == import_path:
                        uses |= set(re.findall(r"\b%s\.([A-Z]\w*)" % re.escape(alias), src))
            self.uses[import_path] = uses
        return self.uses[import_path]

    def hunk_sha(self, target, start, count):
        """SHA-256 of lines [start, start + count) of the reference file `target` (None if the file is missing or too short)"""
        key = "%s:%d,%d" % (target, start, count)
        if key not in self.hunks:
            f = os.path.join(self.top, target)
            lines = open(f).read().split("\n") if os.path.isfile(f) else []
            self.hunks[key] = text_sha(lines[start - 1:start - 1 + count]) if start - 1 + count <= len(lines) else None
        return self.hunks[key]

    def write_index(self, path):
        idx = {"package_names": {k: v for k, v in sorted(self.names.items()) if v},
               "declared": {k: sorted(v) for k, v in sorted(self.decls.items())},
               "crypto_uses": {k: sorted(v) for k, v in sorted(self.uses.items())},
               "patch_hunk_sha256": {k: v for k, v in sorted(self.hunks.items()) if v}}
        with open(path, "w") as f:
            json.dump(idx, f, indent=0, sort_keys=True)
            f.write("\n")


class IndexReference:
    """the committed index of the reference tree (tests/golden/reference_go_index.json)"""

    def __init__(self, path):
        idx = json.load(open(path))
        self.names, self.hunks = idx["package_names"], idx["patch_hunk_sha256"]
        self.decls = {k: set(v) for k, v in idx["declared"].items()}
        self.uses = {k: set(v) for k, v in idx["crypto_uses"].items()}

    def package_name(self, rel):
        return self.names.get(rel)

    def declared(self, pkg):
        return self.decls.get(pkg, set())

    def crypto_uses(self, import_path):
        return self.uses.get(import_path, set())

    def hunk_sha(self, target, start, count):
        return self.hunks.get("%s:%d,%d" % (target, start, count))


REF = None


def check_patch(path):
    """the hunks of one patch whose replaced lines are not where the hunk says in the reference: [(hunk header, reason)]"""
    bad = []
    for target, start, count, old in patch_hunks(path):
        where = "%s @@ -%d,%d" % (target, start, count)
        if len(old) != count:
            bad.append((where, "the hunk holds %d old lines, its header says %d" % (len(old), count)))
            continue
        want = REF.hunk_sha(target, start, count)
        if want is None:
            bad.append((where, "the reference has no such lines"))
        elif text_sha(old) != want:
            bad.append((where, "the lines the hunk replaces differ from the reference's"))
    return bad


def header_symbols():
    h = open(os.path.join(ROOT, "include", "gnark_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(ga_\w+)\s*\(([^;{]*?)\)\s*;", h, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    defines = set(re.findall(r"^#define\s+(GA_\w+)", h, flags=re.M))
    types = set(re.findall(r"\btypedef\s+struct\s+\w*\s*(?:\{[^}]*\})?\s*(ga_\w+)\s*;", h, flags=re.S)) | set(re.findall(r"\}\s*(ga_\w+)\s*;", h))
    return protos, defines, types


def call_arity(src, pos):
    """number of top-level arguments of the call whose '(' is at src[pos]"""
    depth, n, i, seen = 0, 0, pos, False
    while i < len(src):
        ch = src[i]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                return n + (1 if seen else 0)
        elif ch == "," and depth == 1:
            n += 1
        elif depth >= 1 and not ch.isspace():
            seen = True
        i += 1
    return -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reference", metavar="DIR", help="the gnark source tree to resolve against (default: the committed index)")
    ap.add_argument("--write-index", metavar="FILE", help="with --reference: write what the check read from the tree (the committed index)")
    args = ap.parse_args()
    global REF
    if args.reference:
        if not os.path.isdir(args.reference):
            print("reference tree not present at %s: nothing to resolve against" % args.reference)
            return 2
        REF = TreeReference(args.reference)
    elif args.write_index:
        ap.error("--write-index needs --reference")
    else:
        REF = IndexReference(INDEX)
    protos, defines, ctypes = header_symbols()
    patched = declared_by_patches()
    table, bad = [], []
    for f in sorted(go_files(os.path.join(ROOT, "go"))):
        raw = open(f).read()
        imps = imports_of(raw)
        src = strip_comments_and_strings(raw)
        rel = os.path.relpath(f, ROOT)
        has_c = re.search(r'^import\s+"C"', raw, flags=re.M) is not None
        if has_c:
            for m in re.finditer(r"\bC\.(\w+)", src):
                name = m.group(1)
                if name.startswith("ga_") and name in protos:
                    after = src[m.end():m.end() + 1]
                    if after == "(":
                        got = call_arity(src, m.end())
                        if got != protos[name]:
                            bad.append((rel, "C." + name, "called with %d arguments, header declares %d" % (got, protos[name])))
                            continue
                    table.append((rel, "C." + name, "include/gnark_amd.h prototype (%d args)" % protos[name]))
                elif name.startswith("GA_") and name in defines:
                    table.append((rel, "C." + name, "include/gnark_amd.h #define"))
                elif name in ctypes or name.startswith("struct_") or name in CGO_BUILTINS:
                    table.append((rel, "C." + name, "cgo / header type"))
                else:
                    bad.append((rel, "C." + name, "not in include/gnark_amd.h"))
        for alias, path in imps.items():
            if alias in ("_", ".", "C"):
                continue
            idents = set(re.findall(r"(?<![\w.])%s\.([A-Za-z_]\w*)" % re.escape(alias), src))
            for ident in sorted(idents):
                if path.startswith(GNARK):
                    pkg = path[len(GNARK):]
                    shim = pkg.startswith(SHIM_PREFIX)
                    if ident in (declared_in(os.path.join(ROOT, "go", pkg)) if shim else REF.declared(pkg)):
                        # named relative to its tree, so that the table does not depend on where either tree is checked out
                        where = "go/" + pkg if shim else "the reference's " + pkg
                        table.append((rel, "%s.%s" % (alias, ident), "declared in %s" % where))
                    elif ident in patched.get(pkg, {}):
                        table.append((rel, "%s.%s" % (alias, ident), "added to %s by %s" % (pkg, patched[pkg][ident])))
                    else:
                        bad.append((rel, "%s.%s" % (alias, ident), "not declared in %s" % ("go/" + pkg if shim else "the reference's " + pkg)))
                elif path.startswith(CRYPTO):
                    if used_in_reference(path, ident):
                        table.append((rel, "%s.%s" % (alias, ident), "gnark-crypto [EXT]: used by the reference with import %s" % path))
                    else:
                        bad.append((rel, "%s.%s" % (alias, ident), "gnark-crypto %s: no use of this identifier anywhere in the reference" % path))
                elif path in STDLIB:
                    if ident in STDLIB[path]:
                        table.append((rel, "%s.%s" % (alias, ident), "standard library"))
                    else:
                        bad.append((rel, "%s.%s" % (alias, ident), "not in the allow-list for standard package %s" % path))
                else:
                    bad.append((rel, "%s.%s" % (alias, ident), "import %s is neither gnark, gnark-crypto nor an allow-listed standard package" % path))
    patches = sorted(os.path.relpath(f, ROOT) for d, _, fs in os.walk(os.path.join(ROOT, "go")) for f in
                     (os.path.join(d, x) for x in fs if x.endswith(".patch")))
    stale = [(p,) + b for p in patches for b in check_patch(os.path.join(ROOT, p))]
    print("%d package-qualified identifiers resolved, %d unresolved" % (len(table), len(bad)))
    for r in bad:
        print("UNRESOLVED  %s: %s -- %s" % r)
    print("%d patches checked against the reference, %d stale hunks" % (len(patches), len(stale)))
    for r in stale:
        print("STALE  %s: %s -- %s" % r)
    if args.json:
        json.dump({"resolved": sorted(set(table)), "unresolved": bad}, open(args.json, "w"), indent=0)
    if args.write_index:
        REF.write_index(args.write_index)
    return 1 if bad or stale else 0


if __name__ == "__main__":
    sys.exit(main())
