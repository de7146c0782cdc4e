"""Per-kernel ISA figures of one HIP source, for comparing two revisions of a hand-scheduled kernel without a GPU.

    python scripts/isa_table.py colxlip_amd/csrc/gemm_bf16_nt8p.hip [more.hip ...] [--prefix _Z21gemm_bf16_nt8p_kernel]

Compiles with the line tests/test_isa_guards.py uses and prints, per kernel symbol: VGPRs, SGPRs, scratch bytes/lane, occupancy,
static LDS, instructions, and the counts of v_mfma, ds_read_b128, LDS-DMA loads, s_barrier, s_waitcnt with vmcnt(0), v_writelane.
`kloop` lists, per k-step body in the text (from the first fragment read of a burst to the last MFMA that follows it), how many
v_writelane / v_readlane / scratch_* / vmcnt(0) instructions sit inside it: all zeros = nothing spilled or drained in the loop.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BAD_IN_LOOP = ("v_writelane", "v_readlane", "scratch_")


def compile_asm(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", out,
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr[-3000:])
        with open(out) as f:
            return f.read(), r.stderr


def instructions(body):
    lines = [l.split(";")[0].strip() for l in body.split("\n")]
    return [l for l in lines if l and not l.startswith((".", "//")) and not l.endswith(":")]


def kloop_regions(ins):
    """[first fragment read of a k-step .. last MFMA before the next k-step's first read]"""
    reads = [i for i, l in enumerate(ins) if l.startswith("ds_read_b128")]
    mfmas = [i for i, l in enumerate(ins) if l.startswith("v_mfma")]
    starts = [i for k, i in enumerate(reads) if k == 0 or any(reads[k - 1] < m < i for m in mfmas)]
    out = []
    for k, s in enumerate(starts):
        nxt = starts[k + 1] if k + 1 < len(starts) else len(ins)
        inside = [m for m in mfmas if s < m < nxt]
        if inside:
            out.append((s, inside[-1]))
    return out


def table(src, prefix):
    asm, remarks = compile_asm(src)
    res = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", remarks, re.S):
        def num(key, body=m.group(2)):
            s = re.search(re.escape(key) + r": (\d+)", body)
            return int(s.group(1)) if s else -1
        res[m.group(1)] = (num("VGPRs"), num("SGPRs"), num("ScratchSize [bytes/lane]"), num("Occupancy [waves/SIMD]"),
                           num("LDS Size [bytes/block]"))
    rows = []
    for m in re.finditer(r"^(%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % prefix, asm, re.S | re.M):
        name, ins = m.group(1), instructions(m.group(2))
        cnt = lambda p: sum(1 for l in ins if l.startswith(p))
        vm0 = lambda seq: sum(1 for l in seq if l.startswith("s_waitcnt") and "vmcnt(0)" in l)
        dma = sum(1 for l in ins if l.startswith("buffer_load_dword") and l.endswith(" lds"))
        kl = ["%d" % (sum(1 for l in ins[a:b + 1] if l.startswith(BAD_IN_LOOP)) + vm0(ins[a:b + 1])) for a, b in kloop_regions(ins)]
        targs = re.search(r"Li(\d+)ELi(\d+)EEv", name)
        short = "<%s,%s>" % (targs.group(1), targs.group(2)) if targs else name
        rows.append((short,) + res.get(name, (-1,) * 5) + (len(ins), cnt("v_mfma"), cnt("ds_read_b128"), dma, cnt("s_barrier"),
                                                           vm0(ins), cnt("v_writelane"), "/".join(kl)))
    head = ("kernel", "vgpr", "sgpr", "scr", "occ", "lds", "instr", "mfma", "dsr128", "dma", "sbar", "vm0", "wlane", "kloop")
    print("# %s  (%d kernels)" % (os.path.basename(src), len(rows)))
    print(" ".join("%8s" % h for h in head))
    for r in sorted(rows):
        print(" ".join("%8s" % (v,) for v in r))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--prefix", default="_Z", help="kernel symbol prefix")
    a = ap.parse_args()
    for s in a.sources:
        table(s, a.prefix)
