"""Numbers for profiles/README.md and DESIGN.md section 5, computed FROM the committed files (no hand-typed figures):
    python scripts/profile_summary.py profiles/r03_bench_serial_towers_kernel_stats.csv 12 [bench.json ...] > profiles/r03_summary.md
Kernel families are matched on the (demangled or mangled) kernel name; per-step = TotalDurationNs / steps."""
import csv
import json
import re
import sys

FAMILIES = [
    ("NT plain  <0,0>", r"gemm_bf16_nt8p_kernel.*(Li0ELi0E|, 0, 0>)"),
    ("NT bias  <1,0>", r"gemm_bf16_nt8p_kernel.*(Li1ELi0E|, 1, 0>)"),
    ("NT bias+residual  <3,0>", r"gemm_bf16_nt8p_kernel.*(Li3ELi0E|, 3, 0>)"),
    ("NT x GELU'(u)  <4,1>", r"gemm_bf16_nt8p_kernel.*(Li4ELi1E|, 4, 1>)"),
    ("NT bias+GELU+preact  <25,1>", r"gemm_bf16_nt8p_kernel.*(Li25ELi1E|, 25, 1>)"),
    ("NT bias+GELU+8-bit GELU'  <73,1>", r"gemm_bf16_nt8p_kernel.*(Li73ELi1E|, 73, 1>)"),
    ("NT x 8-bit GELU' factor  <128,0>", r"gemm_bf16_nt8p_kernel.*(Li128ELi0E|, 128, 0>)"),
    ("NT MaxSim epilogue  <32,0>", r"gemm_bf16_nt8p_kernel.*(Li32ELi0E|, 32, 0>)"),
    ("NT other ping-pong", r"gemm_bf16_nt8p_kernel"),
    ("NT pipelined (nt5)", r"gemm_bf16_nt5_kernel"),
    ("NT one-barrier", r"gemm_bf16_nt_kernel"),
    ("NT fp8", r"gemm_fp8_nt8p_kernel"),
    ("TN wgrad", r"gemm_bf16_tn"),
    ("TN slab / partial reduce", r"slab_reduce_(group_)?kernel|reduce_partials"),
    ("attention fwd", r"attn_\w*fwd"),
    ("attention bwd", r"attn_\w*bwd"),
    ("LayerNorm fwd", r"ln_fwd"),
    ("LayerNorm bwd", r"ln_bwd"),
    ("loss", r"ce_fused|ce_rows|ce_cols|ce_grad"),
    ("MaxSim pack / finish / scatter", r"maxsim_"),
    ("AdamW + weight casts", r"adamw_multi|cast_weight|quant_weight"),
    ("row quantiser (fp8)", r"quant_rows"),
]


def main():
    path, steps = sys.argv[1], float(sys.argv[2])
    rows = list(csv.DictReader(open(path)))
    fam = {name: [0.0, 0] for name, _ in FAMILIES}
    fam["everything else"] = [0.0, 0]
    total = 0.0
    for r in rows:
        ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
        total += ns
        for name, pat in FAMILIES:
            if re.search(pat, r["Name"]):
                fam[name][0] += ns
                fam[name][1] += calls
                break
        else:
            fam["everything else"][0] += ns
            fam["everything else"][1] += calls
    print(f"### `{path}` ({int(steps)} steps profiled)\n")
    print("| kernel family | launches / step | ms / step | avg us / launch | share |")
    print("|---|---|---|---|---|")
    for name, (ns, calls) in fam.items():
        if calls:
            print(f"| {name} | {calls / steps:.1f} | {ns / 1e6 / steps:.2f} | {ns / 1e3 / calls:.1f} | {100 * ns / total:.1f} % |")
    nt = [v for k, v in fam.items() if k.startswith("NT ") and "fp8" not in k]
    nt_ns, nt_calls = sum(v[0] for v in nt), sum(v[1] for v in nt)
    print(f"| **all bf16 NT launches** | {nt_calls / steps:.1f} | {nt_ns / 1e6 / steps:.2f} | {nt_ns / 1e3 / max(nt_calls, 1):.1f} | {100 * nt_ns / total:.1f} % |")
    print(f"| **total kernel time** | {sum(int(r['Calls']) for r in rows) / steps:.0f} | {total / 1e6 / steps:.1f} | | |")
    for b in sys.argv[3:]:
        try:
            d = json.loads(open(b).read().strip().splitlines()[-1])
        except (OSError, ValueError, IndexError) as e:
            print(f"\n`{b}`: unreadable ({e})")
            continue
        rf = d.get("roofline", {})
        print(f"\n`{b}`: {d['ms_per_step']} ms/step, {d['value']} {d['unit']}; {rf.get('kernel', '')[:60]}: {rf.get('achieved')} {rf.get('unit')} "
              f"= {rf.get('frac')} of {rf.get('peak')}, {rf.get('launches_per_step')} launches of {rf.get('avg_launch_us')} us; "
              f"traffic/algorithmic {rf.get('traffic_over_algorithmic')}; dense text rows {d.get('dense_text_rows')}; "
              f"cpu_baseline {d.get('cpu_baseline', {}).get('value')} on {d.get('cpu_baseline', {}).get('cores')} cores")


if __name__ == "__main__":
    main()
