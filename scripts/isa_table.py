"""Per-kernel ISA figures of one HIP source, for comparing two revisions of a hand-scheduled kernel without a GPU.

    python scripts/isa_table.py colxlip_amd/csrc/gemm_bf16_nt8p.hip [more.hip ...] [--prefix _Z21gemm_bf16_nt8p_kernel]

Compiles with the line tests/test_isa_guards.py uses and prints, per kernel symbol: VGPRs, SGPRs, scratch bytes/lane, occupancy,
static LDS, instructions, and the counts of v_mfma, ds_read_b128, LDS-DMA loads, s_barrier, s_waitcnt with vmcnt(0), v_writelane.
`kloop` lists, per k-step body in the text (from the first fragment read of a burst to the last MFMA that follows it), how many
v_writelane / v_readlane / scratch_* / vmcnt(0) instructions sit inside it: all zeros = nothing spilled or drained in the loop.

    python scripts/isa_table.py colxlip_amd/csrc/attention.hip --identical-to colxlip_amd/csrc/attention_parent.hip

compares a refactored source with an earlier revision of it (saved beside it, so that its includes resolve): per kernel symbol
VGPRs, scratch, occupancy, instructions and whether the instruction stream is the other revision's (comments and directives
dropped, .LBB labels numbered by first appearance), then the symbols that only the other revision has.
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


def stream(body):
    lines = [l.split(";")[0].strip() for l in body.split("\n")]
    text = "\n".join(l for l in lines if l and not l.startswith("//") and (not l.startswith(".") or l.endswith(":")))
    labels = {}
    return re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), text)


def identity(src, other, prefix):
    def load(path):
        asm, remarks = compile_asm(path)
        res = {m.group(1): tuple(int(re.search(re.escape(k) + r": (\d+)", m.group(2)).group(1))
                                 for k in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"))
               for m in re.finditer(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", remarks, re.S)}
        return res, {m.group(1): stream(m.group(2)) for m in re.finditer(r"^(%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % prefix, asm, re.S | re.M)}
    res, new = load(src)
    old_res, old = load(other)
    same = sum(1 for n in new if old.get(n) == new[n])
    print("# %s against %s: %d kernels, %d with the other revision's instruction stream" % (os.path.basename(src), os.path.basename(other), len(new), same))
    print("%-84s %5s %5s %4s %6s %s" % ("kernel", "vgpr", "scr", "occ", "instr", "identical"))
    for n in sorted(new):
        print("%-84s %5d %5d %4d %6d %s" % ((n,) + res[n] + (len(instructions(new[n])), "yes" if old.get(n) == new[n] else "NO")))
    for n in sorted(set(old) - set(new)):
        print("only in %s: %-60s vgpr %d scr %d occ %d" % ((os.path.basename(other), n) + old_res[n]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--prefix", default="_Z", help="kernel symbol prefix")
    ap.add_argument("--identical-to", help="an earlier revision of the (one) source: compare instruction streams instead")
    a = ap.parse_args()
    for s in a.sources:
        identity(s, a.identical_to, a.prefix) if a.identical_to else table(s, a.prefix)
