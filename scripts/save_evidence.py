"""Copy what scripts/collect_round.sh left under gpurun_out/final_<round>/ into profiles/ (round-tagged names), refresh
profiles/pmc_traffic.json and write profiles/<round>_summary.md FROM those files (scripts/profile_summary.py).
    ROUND=r03 python scripts/save_evidence.py"""
import glob
import json
import os
import shutil
import subprocess
import sys

sys.path.insert(0, ".")
import bench  # noqa: E402

R = os.environ.get("ROUND", "r04")
F = f"gpurun_out/final_{R}"


def last_json(path):
    return json.loads(open(path).read().strip().splitlines()[-1])


e = json.load(open(f"gpurun_out/pmc_{R}_traffic_entry.json"))
t = json.load(open("profiles/pmc_traffic.json"))
ent = e["traffic_entry"]
if ent:
    ent["round"] = int(R[1:])
    ent["algorithmic_bytes_per_launch"] = last_json(f"{F}/bench_default.json")["roofline"]["algorithmic_bytes_per_launch"]
    t["ViT-B-32/b4096/bf16/packed"] = ent
    json.dump(t, open("profiles/pmc_traffic.json", "w"), indent=1)
    print("kernel_rev now", bench.nt_kernel_rev(), "entry", ent["kernel_rev"], "ratio",
          round(ent["traffic_bytes_per_launch"] / ent["algorithmic_bytes_per_launch"], 3))
cp = {f"{F}/bench_default.json": f"profiles/{R}_bench_default.json",
      f"{F}/bench_forcedist.json": f"profiles/{R}_bench_forcedist_1rank_rccl.json",
      f"{F}/kstats.txt": f"profiles/{R}_bench_serial_towers_kstats.txt",
      f"{F}/kstats_b512.txt": f"profiles/{R}_bench_b512_serial_towers_kstats.txt",
      f"{F}/timeline_two_streams.txt": f"profiles/{R}_timeline_two_streams.txt",
      f"{F}/gemm_vs_hipblaslt.txt": f"profiles/{R}_gemm_vs_hipblaslt.txt",
      f"{F}/epilogue_variants.txt": f"profiles/{R}_epilogue_variants.txt",
      f"{F}/colclip.txt": f"profiles/{R}_colclip.txt",
      f"gpurun_out/pmc_{R}_sq.txt": f"profiles/{R}_pmc_sq_bench_step.txt",
      f"gpurun_out/pmc_{R}_fetch.txt": f"profiles/{R}_pmc_fetch_bench_step.txt",
      f"gpurun_out/pmc_{R}_write.txt": f"profiles/{R}_pmc_write_bench_step.txt",
      f"gpurun_out/pmc_{R}_traffic_entry.json": f"profiles/{R}_pmc_mfma_util_and_traffic.json"}
for b in (2048, 1024, 512):
    cp[f"{F}/bench_b{b}.json"] = f"profiles/{R}_bench_b{b}.json"
for p in ("bf16", "fp8", "fp8_mfma"):
    cp[f"{F}/bench_h14_{p}_b128.json"] = f"profiles/{R}_bench_vit_h14_{p}_b128.json"
for tag in ("b16_b512", "l14_336_b1024_ckpt", "h14_b2048_fp8_mfma_ckpt", "colxlip_b16_b512"):
    cp[f"{F}/bench_{tag}.json"] = f"profiles/{R}_bench_{tag}.json"
    cp[f"{F}/kstats_{tag}.txt"] = f"profiles/{R}_kstats_{tag}.txt"
for s, d in cp.items():
    if os.path.exists(s):
        if s.endswith(".json") and "bench_" in s:         # keep the JSON line only (library banners may precede it)
            open(d, "w").write(json.dumps(last_json(s)) + "\n")
        else:
            shutil.copy(s, d)
    else:
        print("missing", s)
with open(f"profiles/{R}_attention_bwd4.txt", "w") as f:
    f.write("scripts/bench_attn.py (b = 4096): four-image backward\n")
    if os.path.exists(f"{F}/attention.txt"):
        f.write("".join(l for l in open(f"{F}/attention.txt") if "TB/s" in l))
with open(f"profiles/{R}_attention_other_models.txt", "w") as f:
    f.write("scripts/bench_attn.py 256 {h14,long,b16}: the online-softmax kernels at the other BASELINE models' shapes (end of the round)\n")
    for name in ("attention_h14.txt", "attention_l14.txt", "attention_b16.txt"):
        if os.path.exists(f"{F}/{name}"):
            f.write("".join(l for l in open(f"{F}/{name}") if l.startswith("ViT-")))
for sub, dst in (("prof", f"profiles/{R}_bench_serial_towers_kernel_stats.csv"), ("prof512", f"profiles/{R}_bench_b512_serial_towers_kernel_stats.csv")):
    found = glob.glob(f"{F}/{sub}/**/*_kernel_stats.csv", recursive=True)
    if found:          # gpurun merges into gpurun_out/ without deleting: an earlier collection's files may still be there
        shutil.copy(max(found, key=os.path.getmtime), dst)
for tag in ("b16_b512", "l14_336_b1024_ckpt", "h14_b2048_fp8_mfma_ckpt", "colxlip_b16_b512"):
    found = glob.glob(f"{F}/prof_{tag}/**/*_kernel_stats.csv", recursive=True)
    if found:
        shutil.copy(max(found, key=os.path.getmtime), f"profiles/{R}_kernel_stats_{tag}.csv")
benches = [f"profiles/{R}_bench_default.json"] + [f"profiles/{R}_bench_b{b}.json" for b in (2048, 1024, 512)] + \
          [f"profiles/{R}_bench_vit_h14_{p}_b128.json" for p in ("bf16", "fp8", "fp8_mfma")] + [f"profiles/{R}_bench_b16_b512.json"] + \
          [f"profiles/{R}_bench_forcedist_1rank_rccl.json"]
with open(f"profiles/{R}_summary.md", "w") as f:
    f.write(f"# {R}: numbers derived from the files in this directory by scripts/profile_summary.py (nothing typed by hand)\n\n")
    f.write(subprocess.run([sys.executable, "scripts/profile_summary.py", f"profiles/{R}_bench_serial_towers_kernel_stats.csv", "12"] + benches,
                           capture_output=True, text=True).stdout)
    f.write("\n\n")
    f.write(subprocess.run([sys.executable, "scripts/profile_summary.py", f"profiles/{R}_bench_b512_serial_towers_kernel_stats.csv", "27"],
                           capture_output=True, text=True).stdout)
    for tag, steps in (("b16_b512", 12), ("l14_336_b1024_ckpt", 5), ("h14_b2048_fp8_mfma_ckpt", 4), ("colxlip_b16_b512", 12)):
        if os.path.exists(f"profiles/{R}_kernel_stats_{tag}.csv"):
            f.write(f"\n\n## {tag}\n\n")
            f.write(subprocess.run([sys.executable, "scripts/profile_summary.py", f"profiles/{R}_kernel_stats_{tag}.csv", str(steps),
                                    f"profiles/{R}_bench_{tag}.json"], capture_output=True, text=True).stdout)
print(open(f"profiles/{R}_summary.md").read()[:3000])
