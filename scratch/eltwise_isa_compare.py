"""Compares the device code of the trunk's epilogue family between two trees, kernel by kernel (profiles/eltwise_unify_isa.txt).

    python scratch/eltwise_isa_compare.py PARENT_TREE NEW_TREE > table.txt

Both trees' dib_eltwise.hip and dib_eltwise_bf16.hip are compiled with csrc/Makefile's flags (--cuda-device-only -S,
-Rpass-analysis=kernel-resource-usage).  A kernel's instruction stream is what is left of its function after dropping
directives, comments and labels, with `.LBB<k>_<n>` renamed to `.LBB_<n>`.  Kernels are paired by stem, lane type and template
flags, so `bias_act_vec4_kernel<1,1,0>` meets `bias_act_kernel<F32Lane,1,1,0>`.  CPU only: nothing is run.
"""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]
RES = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def compile_tree(tree, tmp):
    funcs, res = {}, {}
    for f in ("dib_eltwise.hip", "dib_eltwise_bf16.hip"):
        src = os.path.join(tree, "detectinblur_amd", "csrc", f)
        asm = os.path.join(tmp, f + ".s")
        p = subprocess.run([HIPCC] + FLAGS + [src, "-o", asm], capture_output=True, text=True, check=True)
        cur = None
        for line in p.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = res.setdefault(m.group(1), {})
            m = re.search(r"remark:\s+(%s): (\d+)" % "|".join(re.escape(r) for r in RES), line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
        name = None
        for line in open(asm):
            s = line.split(";")[0].strip()
            m = re.match(r"(_Z\w+):$", s)
            if m and name is None:
                name = m.group(1)
                funcs[name] = []
            elif s.startswith(".Lfunc_end"):
                name = None
            elif name and s and not s.startswith(".") and not s.endswith(":"):
                funcs[name].append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", " ".join(s.split())))
    demangled = subprocess.run(["c++filt"] + list(funcs), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for mangled, d in zip(funcs, demangled):
        m = re.match(r"(?:void )?dib::(\w+?)(_vec4|_bf16)?_kernel(?:<(.*?)>)?\(", d)
        args = [a.strip() for a in (m.group(3) or "").split(",") if a.strip()]
        lane = "bf16" if (m.group(2) == "_bf16" or "dib::Bf16Lane" in args) else "fp32"
        flags = ",".join("1" if a == "true" else "0" for a in args if a in ("true", "false"))
        out["%s<%s%s>" % (m.group(1), lane, "," + flags if flags else "")] = (funcs[mangled], res[mangled])
    return out


def mem_counts(insts):
    c = collections.Counter(i.split()[0] for i in insts if re.match(r"(global|flat|buffer|scratch)_", i))
    return " ".join("%s=%d" % kv for kv in sorted(c.items()))


def main():
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        old, new = compile_tree(sys.argv[1], t1), compile_tree(sys.argv[2], t2)
    assert sorted(old) == sorted(new), (sorted(set(old) ^ set(new)))
    fmt = lambda r: "/".join(str(r[k]) for k in RES)
    print("resources: " + " / ".join(RES))
    print("%-34s %6s %6s  %-9s %-22s %-22s" % ("kernel", "before", "after", "identical", "resources before", "resources after"))
    diffs = []
    for k in sorted(old):
        (a, ra), (b, rb) = old[k], new[k]
        print("%-34s %6d %6d  %-9s %-22s %-22s" % (k, len(a), len(b), "yes" if a == b else "NO", fmt(ra), fmt(rb)))
        if a != b:
            diffs.append((k, a, b))
    print("\n%d kernels, %d identical, %d with resources unchanged" % (len(old), len(old) - len(diffs), sum(old[k][1] == new[k][1] for k in old)))
    for k, a, b in diffs:
        print("\n--- %s: memory instructions before: %s\n--- %s: memory instructions after:  %s" % (k, mem_counts(a), k, mem_counts(b)))
        print("\n".join(difflib.unified_diff(a, b, "before", "after", lineterm="", n=1)))


if __name__ == "__main__":
    main()
