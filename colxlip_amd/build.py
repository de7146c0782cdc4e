"""Build libclipx_hip.so (hand-written HIP for gfx950) in-tree with hipcc.

    python -m colxlip_amd.build          # incremental
    python -m colxlip_amd.build --force
"""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libclipx_hip.so")
SOURCES = ["elementwise.hip", "gemm_f32.hip", "gemm_bf16_nt.hip", "gemm_bf16_nt5.hip", "gemm_bf16_nt8p.hip", "gemm_fp8_nt8p.hip", "gemm_bf16_tn.hip", "linear.hip", "attention.hip", "attention_pooled.hip", "colbert.hip", "maxsim_pairs.hip", "topk.hip", "loss_fused.hip", "loss_sigmoid.hip", "loss_distill.hip", "patch_dropout.hip", "image_transform.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result"] + os.environ.get("CLIPX_EXTRA_FLAGS", "").split()


def _stamp() -> str:
    h = hashlib.sha256()
    for name in sorted(os.listdir(CSRC)) + ["../../include/clipx.h"]:
        p = os.path.join(CSRC, name)
        if os.path.isfile(p):
            with open(p, "rb") as f:
                h.update(name.encode())
                h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def build(force: bool = False, verbose: bool = True) -> str:
    stamp_path = LIB + ".stamp"
    stamp = _stamp()
    if not force and os.path.exists(LIB) and os.path.exists(stamp_path):
        with open(stamp_path) as f:
            if f.read().strip() == stamp:
                return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    procs = []
    for src in SOURCES:
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        cmd = [hipcc, *FLAGS, "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, obj, subprocess.Popen(cmd)))
    objs = []
    for src, obj, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
        objs.append(obj)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    # a kernel template whose host-side stub was not emitted links fine and only fails at dlopen: check now
    import ctypes
    try:
        ctypes.CDLL(LIB)
    except OSError as e:
        raise RuntimeError(f"{LIB} was built but does not load: {e}") from e
    with open(stamp_path, "w") as f:
        f.write(stamp)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
