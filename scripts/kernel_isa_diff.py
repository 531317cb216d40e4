"""Compare the gfx950 instruction streams of two builds of libfq_hip.so, kernel by kernel.

    python scripts/kernel_isa_diff.py OLD.so NEW.so

Unbundles the gfx950 code object of each library (clang-offload-bundler), disassembles it with llvm-objdump and compares
every kernel symbol present in both builds.  Kernel-argument offsets (s_load offsets off the kernarg pointer) and
branch targets differ whenever a parameter struct grows at its end, so each instruction is compared with its
immediate offsets masked; a type that moved or was renamed changes the mangled names of the kernels instantiated on it, so
the symbols are matched by their demangled names (c++filt) after the MOVED substitutions; the script prints how many
kernels match exactly, how many match after masking, which differ,
and which symbols exist in one build only.  Needs no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
# kernels that became one instantiation of a template: old symbol -> new symbol
RENAMED = {
    "_ZN2fq21linear_i8_wave_kernelEPKaS1_PKfPfNS_10ConvParamsE": "_ZN2fq21linear_i8_wave_kernelILb0EEEvPKaS2_PKfPfNS_10ConvParamsE",
}
# types that moved between namespaces or were renamed, applied in order to the demangled symbol names of both builds
MOVED = [
    (r"\(anonymous namespace\)::(?:Dwf|Gf)?NoStat\b", "NoStat"),            # the five NoStat of the float convolutions -> fq::NoStat
    (r"\(anonymous namespace\)::(?:Dwf|Gf)HistTag\b", "HistTag"),           # -> fq::HistTag
    (r"\(anonymous namespace\)::(?:Dwf|Gf)StatArgs\b", "ProducerStatArgs"), # -> fq::ProducerStatArgs
    # the two concat kernels became the MAXSRC = 8 and MAXSRC = 2 instantiations of one template
    (r"concat_n_i8_kernel<(\w+), (\w+)>\(signed char\*, fq::CatNParams\)", r"concat_i8_kernel<8, \1, \2>(signed char*, fq::CatParams<8>)"),
    (r"concat_i8_kernel<(true|false), (\w+)>\(signed char\*, fq::CatParams\)", r"concat_i8_kernel<2, \1, \2>(signed char*, fq::CatParams<2>)"),
    # ... and with the re-quantising kernel the two element policies of one skeleton
    (r"concat_i8_kernel<(\d), (\w+), (\w+)>\(signed char\*, fq::CatParams<\d>\)",
     r"concat_kernel<fq::CatMove, \1, \2, \3>(signed char*, fq::CatParams<fq::CatMove, \1>)"),
    (r"concat_rq_i8_kernel<(\w+), (\w+)>\(signed char\*, fq::CrqParams\)",
     r"concat_kernel<fq::CatRequant, 8, \1, \2>(signed char*, fq::CatParams<fq::CatRequant, 8>)"),
]


def normalised(syms):
    """The kernels keyed by their demangled names with the MOVED substitutions applied."""
    names = sorted(syms)
    plain = subprocess.check_output(["c++filt"], input="\n".join(names) + "\n", text=True).splitlines()
    assert len(plain) == len(names)
    out = {}
    for name, text in zip(names, plain):
        for pat, rep in MOVED:
            text = re.sub(pat, rep, text)
        assert text not in out, text
        out[text] = syms[name]
    return out


def code_objects(so, tmp):
    """The gfx950 code objects of a library: its .hip_fatbin section holds one offload bundle per source file."""
    blob = os.path.join(tmp, os.path.basename(so) + ".fatbin")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, blob])
    data = open(blob, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)] + [len(data)]
    out = []
    for i in range(len(starts) - 1):
        part = os.path.join(tmp, "%s.%d.bundle" % (os.path.basename(so), i))
        with open(part, "wb") as fh:
            fh.write(data[starts[i]:starts[i + 1]])
        co = part + ".co"
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                               "--output=" + co, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        out.append(co)
    return out


def kernels(cos):
    out, name = {}, None
    for co in cos:
        text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                       text=True)
        out.update(_symbols(text))
    return out


def _symbols(text):
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(.+)>:\s*$", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        line = line.split("//")[0].strip()
        if name and line:
            out[name].append(line)
    for v in out.values():                           # alignment padding behind the last function of a code object
        while v and (v[-1] == "..." or v[-1] == "s_nop 0"):
            v.pop()
    return {k: v for k, v in out.items() if v}


def masked(ins):
    """Only the kernel-argument offset of a scalar load is masked (s_load_* sdst, s[0:1], OFFSET); every other operand, literal
    and branch target is compared as is."""
    ins = re.sub(r"<[^+>]*(\+0x[0-9a-f]+)?>", r"<\1>", ins)      # a branch target's annotation: its offset, not the symbol's name
    return re.sub(r"^(s_load_dword\S*\s+s\[?[0-9:]+\]?,\s*s\[0:1\],\s*)0x[0-9a-f]+$", r"\1X", ins)


def renamed(name):
    """A kernel template that gained a trailing `bool kPcs = false` parameter: its per-tensor instantiation's new symbol."""
    return re.sub(r"Lb0EEEv", "EEv", name, count=1) if "Lb0EEEv" in name else name


def main(old_so, new_so):
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(code_objects(old_so, tmp)), kernels(code_objects(new_so, tmp))
    for a, b in RENAMED.items():
        if a in old and b in new and a not in new:
            new[a] = new.pop(b)
    for b in list(new):
        a = renamed(b)
        if a != b and a in old and a not in new:
            new[a] = new.pop(b)
    old, new = normalised(old), normalised(new)
    same = exact = 0
    diff = []
    for k in sorted(set(old) & set(new)):
        if old[k] == new[k]:
            exact += 1
        elif [masked(i) for i in old[k]] == [masked(i) for i in new[k]]:
            same += 1
        else:
            diff.append(k)
    print("symbols in both builds: %d; identical: %d; identical up to s_load kernel-argument offsets: %d; different: %d"
          % (len(set(old) & set(new)), exact, same, len(diff)))
    for k in diff:
        print("  DIFFERENT", k, len(old[k]), "->", len(new[k]), "instructions")
        for a, b in [(a, b) for a, b in zip(old[k], new[k]) if masked(a) != masked(b)][:3]:
            print("      -", a, "\n      +", b)
    for k in sorted(set(old) - set(new)):
        print("  only in", old_so, k)
    only_new = sorted(set(new) - set(old))
    print("symbols only in %s: %d" % (new_so, len(only_new)))
    for k in only_new:
        print("  +", k)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
