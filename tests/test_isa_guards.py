"""Compile-time guards on the hand-scheduled GEMM kernels (no GPU needed: hipcc cross-compiles gfx950 here).

The k-loops keep three LDS-DMA items in flight and wait for them with COUNTED s_waitcnt vmcnt(N).  The compiler adds
a blanket `s_waitcnt vmcnt(0)` in front of the loop's first LDS read / register write whenever it believes a VMEM load
may still be pending (a load inside the loop, a load whose use was sunk into a predicated block, LDS reads it can
see next to LDS-DMA); that drains the operand ring every k-step and silently costs 15-40 %.  It came and went with
unrelated edits, so the absence of that instruction -- and of register spills -- is asserted here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "colxlip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


_ASM_CACHE = {}


def _asm(src, tmp_path=None):
    """(device assembly, resource-usage remarks) of one source file; compiled once per test session."""
    if src not in _ASM_CACHE:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, src + ".s")
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", os.path.join(CSRC, src),
                   "-o", out, "-Rpass-analysis=kernel-resource-usage"]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stderr[-2000:]
            with open(out) as f:
                _ASM_CACHE[src] = (f.read(), r.stderr)
    return _ASM_CACHE[src]


def _kernels(asm, prefix):
    """name -> body for every kernel symbol starting with `prefix`"""
    out = {}
    # the whole function (an early-exit s_endpgm may come before the loop): up to its .Lfunc_end label
    for m in re.finditer(r"^(%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % prefix, asm, re.S | re.M):
        out[m.group(1)] = m.group(2)
    return out


def _read_burst_heads(body, read_mnemonic, window=8):
    """the `window` instructions in front of every burst of LDS fragment reads (a burst starts at a read whose preceding
    instruction is not one): where the compiler puts the blanket wait when it guards the reads.  Independent of how the loop
    is laid out in the text (rotated, peeled or not)."""
    lines = [l.strip() for l in body.split("\n")]
    lines = [l for l in lines if l and not l.startswith((";", ".", "//"))]
    heads = []
    for i, l in enumerate(lines):
        if l.startswith(read_mnemonic) and (i == 0 or not lines[i - 1].startswith(read_mnemonic)):
            heads.append(lines[max(0, i - window):i])
    assert heads, "no fragment reads found"
    return heads


# bytes/lane of scratch that an instantiation had when its kernel came under the guard below (see its docstring); an upper bound
_KNOWN_SCRATCH = {"_Z20gemm_fp8_nt8p_kernelIDF16bLi25ELi1E": 8, "_Z20gemm_fp8_nt8p_kernelIDF16bLi73ELi1E": 24}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src,prefix,read", [("gemm_bf16_nt.hip", "_Z19gemm_bf16_nt_kernel", "ds_read_b128"),
                                             ("gemm_bf16_tn.hip", "_Z19gemm_bf16_tn_kernel", "ds_read_b64_tr_b16"),
                                             ("gemm_bf16_nt8p.hip", "_Z21gemm_bf16_nt8p_kernel", "ds_read_b128"),
                                             ("gemm_fp8_nt8p.hip", "_Z20gemm_fp8_nt8p_kernel", "ds_read_b128"),
                                             ("gemm_bf16_tn.hip", "_Z22gemm_bf16_tn_pp_kernel", "ds_read_b64_tr_b16"),
                                             ("gemm_bf16_tn.hip", "_Z23gemm_bf16_tn_ppg_kernel", "ds_read_b64_tr_b16")])
def test_no_ring_drain_and_no_spills(src, prefix, read, tmp_path):
    """No compiler-inserted vmcnt(0) in front of the fragment reads, and no scratch.  A recorded finding, not a licence: two fp8
    ping-pong instantiations already spilled when this guard was extended to that kernel -- <bf16, 25, 1> (bias + GELU +
    pre-activation) 8 bytes/lane and <bf16, 73, 1> (bias + GELU + eight-bit GELU', the training c_fc under fp8_mfma) 24 bytes/lane.
    _KNOWN_SCRATCH pins them at those figures until they are fixed; every other instantiation stays at 0."""
    asm, remarks = _asm(src, tmp_path)
    kernels = _kernels(asm, prefix)
    assert kernels, "no kernels found"
    for name, body in kernels.items():
        for head in _read_burst_heads(body, read):
            assert not any(h.startswith("s_waitcnt") and "vmcnt(0)" in h for h in head), \
                f"{name}: compiler-inserted vmcnt(0) in front of the fragment reads drains the LDS-DMA ring each k-step"
    # spills: only the everything-at-once epilogue used by the kernel tests (flags 27) may touch scratch
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", remarks, re.S):
        name, scratch = m.group(1), int(m.group(2))
        if name.startswith(prefix) and "Li27E" not in name:
            allowed = next((b for k, b in _KNOWN_SCRATCH.items() if name.startswith(k)), 0)
            assert scratch <= allowed, f"{name} spills {scratch} bytes/lane (allowed: {allowed})"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_attention_kernels_of_the_train_step_do_not_spill(tmp_path):
    """The MFMA attention kernels run at the register budget that their waves-per-SIMD hint allows; a wider scheduling window
    (round 4: the mask-free backward without its per-tile scheduling barriers) spilled 228 bytes per lane and ran 2.5x slower
    with every parity test still green.  No scratch in the forms the train step launches: the whole-sequence forward and
    four-image backward at every tile count, and the non-causal online-softmax kernels (the causal ones are coverage paths:
    no tower of the configs launches them)."""
    _, remarks = _asm("attention.hip", tmp_path)
    seen = 0
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", remarks, re.S):
        name, scratch = m.group(1), int(m.group(2))
        hot = (name.startswith("_Z20attn_bf16_fwd_kernel") or name.startswith("_Z21attn_bf16_bwd4_kernel")
               or name.startswith("_Z25attn_bf16_long_fwd_kernelILi64ELb0E") or name.startswith("_Z25attn_bf16_long_fwd_kernelILi80ELb0E")
               or re.match(r"_Z25attn_bf16_long_bwd_kernelILi(64|80)ELb1ELb0E", name))
        if hot:
            seen += 1
            assert scratch == 0, f"{name} spills {scratch} bytes/lane"
    assert seen == 36, seen        # 16 forward + 16 four-image backward (NT = 2, 4, 6, 8) + 2 + 2 online-softmax


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pipelined_nt_kernel_keeps_its_accumulators(tmp_path):
    """gemm_bf16_nt5.hip keeps all 256 accumulators in AGPRs that only its inline asm names.  The register allocator
    does not know they are live between asm statements: under pressure it spills VGPRs INTO them (v_accvgpr_write) or to
    scratch (whose reloads in the k-loop are VMEM loads that drain the LDS-DMA queue).  Both must be absent, and the
    compiler must not have added any vmcnt wait of its own to the variants with the deferred epilogue."""
    asm, remarks = _asm("gemm_bf16_nt5.hip", tmp_path)
    kernels = _kernels(asm, "_Z20gemm_bf16_nt5_kernel")
    assert len(kernels) >= 9, sorted(kernels)
    for name, body in kernels.items():
        assert "v_accvgpr_write" not in body, f"{name}: the compiler wrote into an accumulator AGPR"
        assert "scratch_" not in body, f"{name}: spills"
        deferred = not re.search(r"ELi0EEv", name)            # third template argument (parked tuples per k-step) != 0
        if deferred:
            own = re.sub(r";;#ASMSTART.*?;;#ASMEND", "", body, flags=re.S)
            assert not re.search(r"s_waitcnt[^\n]*vmcnt", own), f"{name}: compiler-inserted vmcnt wait"
    for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", remarks, re.S):
        if m.group(1).startswith("_Z20gemm_bf16_nt5_kernel"):
            assert int(m.group(2)) == 0, f"{m.group(1)} spills {m.group(2)} bytes/lane"


_LOSS_WALKS = {"loss_fused.hip": "_Z19ce_fused_bwd_kernel", "loss_sigmoid.hip": "_Z15sig_walk_kernel",
               "loss_distill.hip": "_Z18distill_bwd_kernel"}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src,min_kernels", [("loss_fused.hip", 13), ("loss_sigmoid.hip", 10), ("loss_distill.hip", 17)])
def test_kernel_compiles_without_scratch_or_spills(src, min_kernels, tmp_path):
    """The three fused losses on the tile engine of loss_tile.h: no scratch, no spills, at most 80 KiB of LDS per block, and the
    backward walks at the waves per SIMD their launch bounds ask for: 2 up to NE = 32 (E = 512), 1 for the AGPR-resident
    NE = 40, 48, 64 (E = 640, 768, 1024); 3 for the loss-only sigmoid walk (NE = 0)."""
    _, remarks = _asm(src, tmp_path)
    found = walks = 0
    for m in re.finditer(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", remarks, re.S):
        name, body = m.group(1), m.group(2)
        found += 1
        s = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body)
        assert s is not None and int(s.group(1)) == 0, f"{name} uses scratch"
        for kind in ("VGPRs", "SGPRs"):
            s = re.search(r"%s Spill: (\d+)" % kind, body)
            assert s is None or int(s.group(1)) == 0, f"{name} spills {kind}"
        lds = re.search(r"LDS Size \[bytes/block\]: (\d+)", body)
        assert lds is None or int(lds.group(1)) <= 80 * 1024, f"{name} uses {lds.group(1)} bytes of LDS"
        ne = re.match(r"%sILi(\d+)E" % _LOSS_WALKS[src], name)
        if ne:
            walks += 1
            ne = int(ne.group(1))
            want = 3 if ne == 0 else (2 if ne <= 32 else 1)
            occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", body).group(1))
            assert occ == want, f"{name}: {occ} waves/SIMD, want {want}"
    assert found >= min_kernels, found     # the walk for 9 embed dims (+ sigmoid's loss-only walk), forward, merge, sums, dense
    assert walks == (10 if src == "loss_sigmoid.hip" else 9), walks


# ---------------------------------------------------------------------------------------------------------------------------
# SGPR written by a VALU instruction, read as an address by a VMEM instruction inside INLINE ASM (round-3 GPU fault).
_VALU_SGPR_WRITERS = ("v_readlane_b32", "v_readfirstlane_b32")
_VMEM_PREFIXES = ("global_load", "global_store", "global_atomic", "buffer_load", "buffer_store", "buffer_atomic", "flat_load",
                  "flat_store", "flat_atomic", "scratch_load", "scratch_store")


def _sgprs(operand_text):
    """indices of every scalar register named in an operand list: s7, s[4:7]"""
    out = set()
    for m in re.finditer(r"\bs\[(\d+):(\d+)\]|\bs(\d+)\b", operand_text):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def sgpr_vmem_hazards(body, wait_states=5):
    """(writer line, reader line) pairs: a v_readlane / v_readfirstlane result used by a VMEM instruction fewer than `wait_states`
    wait states later (every instruction in between counts one, `s_nop N` counts N + 1; a label ends the look-ahead, as the
    hazard recogniser's own analysis does at block ends)."""
    lines = [l.split(";")[0].split("//")[0].strip() for l in body.split("\n")]
    lines = [l for l in lines if l and not l.startswith(".") or (l and l.startswith(".L"))]
    found = []
    for i, l in enumerate(lines):
        if not l.startswith(_VALU_SGPR_WRITERS):
            continue
        dst = _sgprs(l.split(None, 1)[1].split(",")[0])
        waited, k = 0, i + 1
        while k < len(lines) and waited < wait_states:
            n = lines[k]
            if n.endswith(":"):
                break
            if n.startswith(_VMEM_PREFIXES) and dst & _sgprs(n.split(None, 1)[1] if " " in n else ""):
                found.append((l, n))
            m = re.match(r"s_nop\s+(\d+)", n)
            waited += (int(m.group(1)) + 1) if m else 1
            k += 1
    return found


def test_sgpr_hazard_scanner_sees_the_round3_pattern():
    """The scanner on the pattern that faulted in round 3 (profiles/r03_ablation_early_bias.txt: an inline-asm VMEM load reading an
    SGPR pair that v_readlane_b32 had just restored from a spill lane), and on its fix."""
    bad = "v_readlane_b32 s2, v255, 4\nv_readlane_b32 s3, v255, 5\nglobal_load_dword v7, v6, s[2:3]\n"
    assert len(sgpr_vmem_hazards(bad)) == 2
    assert not sgpr_vmem_hazards("v_readlane_b32 s2, v255, 4\nv_readlane_b32 s3, v255, 5\ns_nop 4\nglobal_load_dword v7, v6, s[2:3]\n")
    assert not sgpr_vmem_hazards("v_readfirstlane_b32 s9, v3\nglobal_load_dword v7, v6, s[2:3]\n")
    assert sgpr_vmem_hazards("v_readfirstlane_b32 s9, v3\nv_add_u32 v1, v2, v3\nbuffer_load_dword v7, v6, s[8:11], s20 offen\n")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_no_valu_written_sgpr_feeds_vmem_within_five_wait_states():
    """Every shipped kernel: no VMEM instruction reads an SGPR that v_readlane_b32 / v_readfirstlane_b32 wrote fewer than 5 wait
    states earlier.  The compiler's hazard recogniser guarantees this for instructions it emits and cannot see into inline asm;
    the disassembly is checked whole, so a hand-written load or store placed behind a spill reload is caught at build time
    instead of as a memory access fault on the GPU."""
    from concurrent.futures import ThreadPoolExecutor
    from colxlip_amd.build import SOURCES
    with ThreadPoolExecutor(max_workers=4) as pool:
        list(pool.map(_asm, SOURCES))
    bad = []
    for src in SOURCES:
        asm, _ = _asm(src)
        for name, body in _kernels(asm, "_Z").items():
            for w, r in sgpr_vmem_hazards(body):
                bad.append(f"{src}:{name[:60]}: `{w}` -> `{r}`")
    assert not bad, "\n".join(bad[:20])
