"""Is the device code of avec_amd/csrc/*.hip the same as at a git revision?   python tools/isa_diff.py [REV, default HEAD~1]

The acceptance test of a refactor of kernel sources: every .hip file of REV (from `git archive`, in a temporary directory) and of the working tree is compiled to
gfx950 assembly with build.FLAGS + --cuda-device-only -S, the text is cut at every symbol (`.type NAME,@function|@object`) and the pieces are compared as text.
Two things are normalised and nothing else: the __hip_cuid_<hash> symbol (a hash of the source text) and the name and linkage of the LDS-DMA zero page
(\\w*zero16): its .globl / .weak / .protected / .addrsig_sym directives and the section it is defined in.  How kernels ADDRESS it (pc-relative literal or GOT) is code and is
compared.  Prints one line per file and per kernel; exits 1 if anything differs."""
import concurrent.futures as cf
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("avec_build", os.path.join(ROOT, "avec_amd", "build.py"))     # (by path: the package itself imports torch)
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)


def asm(src, csrc, inc, out):
    flags = [f for f in build.FLAGS if not f.startswith("-I")] + ["-I" + inc, "-I" + csrc, "--cuda-device-only", "-S"]
    r = subprocess.run(["hipcc"] + flags + [src, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", open(out).read())
    text = re.sub(r"\b\w*zero16\b[ \t]*", "zero16 ", text)        # (the padding in front of the `; @name` comments depends on the name's length)
    text = re.sub(r"(?m)^\s*\.(globl|protected|hidden|local|weak|addrsig_sym)\s+zero16\b.*\n", "", text)
    text = re.sub(r'(\.type\s+__hip_cuid,@object.*\n)\s*\.section\s+\.bss,"aw",@nobits\n', r"\1", text)      # (the switch back to .bss behind that group)
    pieces, name = {"(preamble)": []}, "(preamble)"
    for line in text.splitlines():
        m = re.match(r"\s*\.type\s+(\S+?)\s*,@(function|object)", line)
        if m:
            name = m.group(1)
            pieces[name] = []
        pieces[name].append(line)
    if "zero16" in pieces:      # its section is linkage too: .bss for a plain global, a comdat group of its own (and a switch back to .bss behind it) for an inline variable
        pieces["zero16"] = [l for l in pieces["zero16"] if not re.match(r"\s*\.section\s", l)]
    return pieces


def tree(csrc, inc, tmp, tag):
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        return dict(zip(srcs, ex.map(lambda f: asm(os.path.join(csrc, f), csrc, inc, os.path.join(tmp, tag + "_" + f[:-4] + ".s")), srcs)))


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD~1"
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "avec_amd/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        old = tree(os.path.join(tmp, "avec_amd", "csrc"), os.path.join(tmp, "include"), tmp, "old")
        new = tree(build.CSRC, build.INC, tmp, "new")
    for f in sorted(set(old) | set(new)):
        a, b = old.get(f, {}), new.get(f, {})
        names = list(a) + [n for n in b if n not in a]
        diff = [n for n in names if a.get(n) != b.get(n)] + (["(order of symbols)"] if list(a) != list(b) else [])
        kernels = [n for n in names if "@function" in (a.get(n) or b.get(n))[0]]
        print("%-22s %3d kernels, %6d lines: %s" % (f, len(kernels), sum(map(len, b.values())), "DIFFERS" if diff else "identical"))
        for n in kernels:
            print("    %-9s %s" % ("DIFFERS" if n in diff else "identical", n))
        for n in diff:
            if n not in kernels:
                print("    DIFFERS   %s" % n)
        bad += len(diff)
    print("%d piece(s) differ from %s" % (bad, rev) if bad else "all device code identical to %s" % rev)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
