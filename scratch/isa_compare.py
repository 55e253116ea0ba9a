"""Compares the device code of csrc/ sources between two trees, kernel by kernel (profiles/roi_sampling_isa.txt,
profiles/eltwise_unify_isa.txt).

    python scratch/isa_compare.py PARENT_TREE NEW_TREE dib_roi.hip > table.txt
    python scratch/isa_compare.py --pair epilogue PARENT_TREE NEW_TREE dib_eltwise.hip dib_eltwise_bf16.hip > table.txt
    python scratch/isa_compare.py --pair sliced_sum PARENT_TREE NEW_TREE dib_deblur_train.hip dib_deblur_adv.hip > table.txt

The named files of both trees' detectinblur_amd/csrc are compiled with csrc/Makefile's flags (--cuda-device-only -S,
-Rpass-analysis=kernel-resource-usage).  A kernel's instruction stream is what is left of its function after dropping
directives, comments and labels, with `.LBB<k>_<n>` renamed to `.LBB_<n>`.  Kernels are paired by demangled name without the
parameter list (`roi_align_fwd_nhwc_sr_kernel<2>`); `--pair epilogue` pairs the trunk's epilogue family by stem, lane type and
template flags instead, so `bias_act_vec4_kernel<1,1,0>` meets `bias_act_kernel<F32Lane,1,1,0>`; `--pair sliced_sum` pairs the
trainer's scalar losses, so `l1_partial_kernel` meets `sliced_sum_partial_kernel<L1Term>` and `adv_bce_final_kernel` meets
`sliced_sum_final_kernel<BceTerm>` (profiles/deblur_trainer_unify_isa.txt).  CPU only: nothing is run.
"""
import argparse
import collections
import difflib
import os
import re
import subprocess
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]
RES = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def pair_by_name(demangled):
    return re.sub(r"^void ", "", demangled.split("(")[0]).replace("dib::", "")


def pair_epilogue(demangled):
    m = re.match(r"(?:void )?dib::(\w+?)(_vec4|_bf16)?_kernel(?:<(.*?)>)?\(", demangled)
    args = [a.strip() for a in (m.group(3) or "").split(",") if a.strip()]
    lane = "bf16" if (m.group(2) == "_bf16" or "dib::Bf16Lane" in args) else "fp32"
    flags = ",".join("1" if a == "true" else "0" for a in args if a in ("true", "false"))
    return "%s<%s%s>" % (m.group(1), lane, "," + flags if flags else "")


def pair_sliced_sum(demangled):
    name = pair_by_name(demangled)
    m = re.match(r"(l1|adv_bce)_(partial|final)_kernel$", name)
    if m:
        return "sliced_sum_%s_kernel<%s>" % (m.group(2), {"l1": "L1Term", "adv_bce": "BceTerm"}[m.group(1)])
    return name


PAIRINGS = {"name": pair_by_name, "epilogue": pair_epilogue, "sliced_sum": pair_sliced_sum}


def compile_tree(tree, files, pair, tmp):
    funcs, res = {}, {}
    for f in files:
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
    return {pair(d): (funcs[mangled], res[mangled]) for mangled, d in zip(funcs, demangled)}


def mem_counts(insts):
    c = collections.Counter(i.split()[0] for i in insts if re.match(r"(global|flat|buffer|scratch)_", i))
    return " ".join("%s=%d" % kv for kv in sorted(c.items()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pair", choices=sorted(PAIRINGS), default="name", help="how kernels of the two trees are matched")
    ap.add_argument("parent_tree")
    ap.add_argument("new_tree")
    ap.add_argument("files", nargs="+", help="source files under detectinblur_amd/csrc, e.g. dib_roi.hip")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        old = compile_tree(a.parent_tree, a.files, PAIRINGS[a.pair], t1)
        new = compile_tree(a.new_tree, a.files, PAIRINGS[a.pair], t2)
    assert sorted(old) == sorted(new), (sorted(set(old) ^ set(new)))
    fmt = lambda r: "/".join(str(r[k]) for k in RES)
    print("resources: " + " / ".join(RES))
    print("%-34s %6s %6s  %-9s %-22s %-22s" % ("kernel", "before", "after", "identical", "resources before", "resources after"))
    diffs = []
    for k in sorted(old):
        (x, rx), (y, ry) = old[k], new[k]
        print("%-34s %6d %6d  %-9s %-22s %-22s" % (k, len(x), len(y), "yes" if x == y else "NO", fmt(rx), fmt(ry)))
        if x != y:
            diffs.append((k, x, y))
    print("\n%d kernels, %d identical, %d with resources unchanged" % (len(old), len(old) - len(diffs), sum(old[k][1] == new[k][1] for k in old)))
    for k, x, y in diffs:
        print("\n--- %s: memory instructions before: %s\n--- %s: memory instructions after:  %s" % (k, mem_counts(x), k, mem_counts(y)))
        print("\n".join(difflib.unified_diff(x, y, "before", "after", lineterm="", n=1)))


if __name__ == "__main__":
    main()
