"""Device assembly of two builds, compared kernel by kernel: the text is cut at every .section directive and at every
kernel entry of the metadata, and the two multisets of pieces must be equal (the order of kernels in the code object
follows the order in which host code first names them).

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/tgnx_tgn.hip -o <a.s | b.s>   # at each commit
    python tools/device_asm_equal.py a.s b.s"""
import re, sys, collections
def pieces(p):
    s = open(p).read()
    s = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", s)
    s = re.sub(r"BB\d+_", "BB_", s)                      # basic-block labels carry the function's ordinal
    s = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", s)
    out = []
    for sec in re.split(r"(?m)^(?=\t\.section\t)", s):
        if ".amdgpu_metadata" in sec:
            out += re.split(r"(?m)^(?=  - \.agpr_count:)", sec)
        else:
            out.append(sec)
    return out
a, b = pieces(sys.argv[1]), pieces(sys.argv[2])
ca, cb = collections.Counter(a), collections.Counter(b)
print("pieces", len(a), len(b), "equal multisets:", ca == cb, "same order:", a == b)
for k in (ca - cb): print("only in A:", k[:300].replace("\n", " | "))
for k in (cb - ca): print("only in B:", k[:300].replace("\n", " | "))
