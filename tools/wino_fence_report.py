"""The conditioning fence's measurements as a table: every row of tests/test_wino_fence_gpu.py (kernel x shape x operand family, the direct
kernel as the control) run once through the test module's own measuring function -- the kernel's and the float32 model's E and S against
float64 and both ratios.  Nothing is asserted here.  Writes profiles/wino_fence.json.

    timeout -k 10 900 python tools/wino_fence_report.py [--out profiles/wino_fence.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wino_fence.json"))
    args = ap.parse_args()
    import torch
    import test_wino_fence_gpu as T
    from vspbfr_amd import hip_ops as H
    torch.set_grad_enabled(False)
    rows = []
    for case, family, epi in T.ROWS:
        r = T.measure(H, case, family, epi)
        rows.append(r)
        print(f"{case.id:48s} {family:9s}{'+epi' if epi else '    '} E {r['E_kernel']:.3e} / {r['E_model']:.3e} = {r['E_ratio']:5.2f}x   "
              f"S {r['S_kernel']:7.2f} / {r['S_model']:7.2f} = {r['S_ratio']:5.2f}x   E / max|ref| {r['E_kernel_of_range']:.2e}", flush=True)
    worst = max(rows, key=lambda r: max(r["E_ratio"], r["S_ratio"]))
    out = dict(device=torch.cuda.get_device_name(0), factor=T.FACTOR, rows=rows,
               worst=dict(kernel=worst["kernel"], shape=worst["shape"], dilations=worst["dilations"], family=worst["family"],
                          epilogue=worst["epilogue"], E_ratio=worst["E_ratio"], S_ratio=worst["S_ratio"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "rows:", len(rows), "worst:", out["worst"])


if __name__ == "__main__":
    main()
