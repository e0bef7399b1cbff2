#!/usr/bin/env python
"""Do two sets of HIP sources compile to the same kernels?  For a change that only MOVES kernels between files (no GPU needed).

  git archive <parent> online-continual-learning_amd/csrc include | tar -x -C /tmp/parent
  python scripts/kernel_text_equal.py /tmp/parent/online-continual-learning_amd/csrc small_ops.hip optim.hip loader.hip \\
      -- online-continual-learning_amd/csrc buffer_rows.hip loader.hip optim.hip cosine.hip row_losses.hip supcon.hip aser.hip ncm.hip \\
         augment.hip gemm_small.hip small_ops.hip

Every file of either side is compiled with the Makefile's CXXFLAGS plus `-S --cuda-device-only` into a temporary directory.  Of every
`_Z...` kernel symbol (one with an `.amdhsa_kernel` block) two parts are taken:
  text  the lines from `<sym>:` to its `.Lfunc_end`, `;` comments stripped, the per-file counter in block labels (`.LBB<n>_`) normalised
  desc  its `.amdhsa_kernel ... .end_amdhsa_kernel` block: registers, LDS, scratch, every other field of the kernel descriptor
One line per symbol: name, the file it came from on either side, a hash of each part, and `same` or `DIFFERS`.  The exit status is
non-zero if a symbol differs, is on one side only, or is defined by two files of one side.  Equality of text is all that is tested:
what the instructions are is nobody's business here."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
MAKEFILE = os.path.join(os.path.dirname(HERE), "online-continual-learning_amd", "csrc", "Makefile")


def makefile_var(name, text):
    return re.search(r"(?m)^%s\s*\??=\s*(.*)$" % name, text).group(1).strip()


def compile_flags():
    text = open(MAKEFILE).read()
    arch = os.environ.get("ARCH") or makefile_var("ARCH", text)
    flags = makefile_var("CXXFLAGS", text).replace("$(ARCH)", arch).split()
    return os.environ.get("HIPCC") or makefile_var("HIPCC", text), flags


def kernels_of(asm):
    """symbol -> (text, desc) of every kernel of one assembly file."""
    lines = asm.split("\n")
    out = {}
    for sym in re.findall(r"(?m)^\s*\.amdhsa_kernel\s+(_Z\S+)\s*$", asm):
        beg = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == sym + ":")
        end = next(i for i in range(beg, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].rstrip()) for l in lines[beg:end]]
        d0 = next(i for i, l in enumerate(lines) if l.split() == [".amdhsa_kernel", sym])
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        desc = [l.strip() for l in lines[d0:d1 + 1]]
        assert sym not in out, sym
        out[sym] = ("\n".join(l for l in body if l.strip()), "\n".join(desc))
    return out


def side(src_dir, files, tmp, tag):
    """symbol -> (file, text, desc) over the files of one side; symbols that two files define are returned apart."""
    hipcc, flags = compile_flags()
    syms, twice = {}, []
    for f in files:
        asm = os.path.join(tmp, "%s_%s.s" % (tag, os.path.splitext(f)[0]))
        subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(src_dir, f), "-o", asm])
        for sym, parts in kernels_of(open(asm).read()).items():
            if sym in syms:
                twice.append("%s: %s and %s" % (sym, syms[sym][0], f))
            syms[sym] = (f,) + parts
    return syms, twice


def h(s):
    return hashlib.sha256(s.encode()).hexdigest()[:16]


def main(argv):
    if "--" not in argv or len(argv) < 5:
        sys.exit(__doc__)
    cut = argv.index("--")
    (dir_a, files_a), (dir_b, files_b) = (argv[0], argv[1:cut]), (argv[cut + 1], argv[cut + 2:])
    with tempfile.TemporaryDirectory() as tmp:
        a, twice_a = side(dir_a, files_a, tmp, "a")
        b, twice_b = side(dir_b, files_b, tmp, "b")
    bad = 0
    for sym in sorted(set(a) | set(b)):
        fa, ta, da = a.get(sym, ("-", "", ""))
        fb, tb, db = b.get(sym, ("-", "", ""))
        ok = sym in a and sym in b and ta == tb and da == db
        bad += not ok
        print("%-7s %-15s text %s %s  desc %s %s  %-15s %s" % ("same" if ok else "DIFFERS", fa, h(ta), h(tb), h(da), h(db), fb, sym))
    for t in twice_a + twice_b:
        print("TWICE   " + t)
    print("%d kernel symbols, %d differ or are missing on a side, %d defined twice" % (len(set(a) | set(b)), bad, len(twice_a + twice_b)))
    return 1 if bad or twice_a or twice_b else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
