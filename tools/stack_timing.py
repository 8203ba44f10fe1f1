"""Timing of the spanwise stacking kernel (k_stack_planes, K11) beside the export transpose (k_soa_planes, K8) -- the closest existing
kernel: the same transposition with one input and two output streams.

Workload: 8 resident cuts of 2048^2 (config 5: amplitude 0.05 + 0.001 c, one handle per cut), cubic, planar, 16 layers, one
tm_stack_smoothers call per window of k_count = 4; tm_smoother_export_soa of cut 0 in the same run.  Kernel times come from ONE profiler
run of this tool with kernel tracing and statistics only (no counters in that run):

    rocprofv3 --kernel-trace --stats -d <dir> -o stack -- python tools/stack_timing.py            (needs the MI355X)
    python tools/stack_timing.py --report <dir>/.../stack_kernel_stats.csv [--out profiles/stack_timing.txt]   (no GPU: reads the CSV)
    python tools/stack_timing.py --cli-wall     wall time of the T106 three-cut CLI job with and without --stack (needs the MI355X)

Bytes per node: K11 reads 16 K and writes 24 k_count (here 16 * 8 + 24 * 4 = 224); K8 reads 16 and writes 16."""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CUTS, LAYERS, WINDOW, REPEATS = 2048, 8, 16, 4, 3


def workload(n, repeats):
    import numpy as np

    from turbomesh_amd import _capi, configs, stack
    from turbomesh_amd.smoothing import smooth, solver

    handles = [smooth.Smoother(configs.single_block(n, n, amplitude=0.05 + 0.001 * c), solver.Option.hip(inner=solver.Inner.relax)) for c in range(CUTS)]
    try:
        for h in handles:
            h.iterate(3)
        z = np.arange(CUTS, dtype=np.float64)
        st = stack.Stack(z, stack.layers_from(z, LAYERS), "cubic", "planar")
        x, y = np.empty(n * n), np.empty(n * n)
        t0 = time.perf_counter()
        for _ in range(repeats + 1):   # the first round warms the code objects
            for k in range(0, LAYERS, WINDOW):
                st.block(handles, 0, k, WINDOW)
            _capi.check(_capi.lib().tm_smoother_export_soa(handles[0]._h, 0, _capi.f64ptr(x), _capi.f64ptr(y), None, None))
        print(f"stack_timing: {repeats + 1} rounds of {LAYERS // WINDOW} windows of {WINDOW} layers from {CUTS} cuts of {n}^2, {time.perf_counter() - t0:.2f} s wall "
              "(device-to-host copies of the planes included)")
    finally:
        for h in handles:
            h.close()


def report(stats_csv, out, n):
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            for key in ("k_stack_planes", "k_soa_planes"):
                if key in r["Name"]:
                    rows[key] = r
    if "k_stack_planes" not in rows or "k_soa_planes" not in rows:
        sys.exit(f"{stats_csv}: no k_stack_planes / k_soa_planes rows")
    nodes = float(n) * n

    def line(key, bytes_per_node, what):
        r = rows[key]
        avg_us, min_us, max_us = float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3
        rate = lambda us: bytes_per_node * nodes / (us * 1e-6) / 1e12   # noqa: E731
        return (f"  {key:15s} {int(r['Calls']):3d} calls  average {avg_us:9.1f} us  min {min_us:9.1f}  max {max_us:9.1f}   "
                f"{rate(avg_us):.3f} TB/s of {bytes_per_node} B/node ({what}); best launch {rate(min_us):.3f} TB/s"), rate(avg_us)

    l11, r11 = line("k_stack_planes", 16 * CUTS + 24 * WINDOW, f"16 x {CUTS} read + 24 x {WINDOW} written")
    l8, r8 = line("k_soa_planes", 32, "16 read + 16 written")
    text = "\n".join([
        f"K11 k_stack_planes beside K8 k_soa_planes on {n}^2 blocks: {CUTS} resident cuts, cubic, planar, windows of {WINDOW} layers; kernel times of one "
        "rocprofv3 --kernel-trace --stats run of tools/stack_timing.py (no counters), every launch of the run averaged, the warm-up round included",
        l11, l8,
        f"  per byte, K11 / K8 = {r11 / r8:.2f} (aim: parity, 1.00)" + ("" if r11 >= r8 else f": K11 falls short of K8 by {100 * (1 - r11 / r8):.0f} %"),
    ]) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def cli_wall():
    gold = os.path.join(ROOT, "tests", "golden")
    base = json.load(open(os.path.join(gold, "examples", "T106", "T106.json")))
    with tempfile.TemporaryDirectory() as tmp:
        files = [os.path.join(gold, "examples", "T106", "T106.json")]
        for c, f in ((1, 1.03), (2, 1.06)):
            d = json.loads(json.dumps(base))
            d["geometry"]["pitch"] = base["geometry"]["pitch"] * f
            for k in ("down_csv_path", "up_csv_path"):
                d["geometry"]["profile"]["csv"][k] = os.path.join(gold, base["geometry"]["profile"]["csv"][k])
            files.append(os.path.join(tmp, f"T106_cut{c}.json"))
            json.dump(d, open(files[-1], "w"))
        env = dict(os.environ, PYTHONPATH=ROOT)
        common = ["--hip", "--iterations", "10"]

        def run(argv):
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "turbomesh_amd"] + argv, cwd=gold, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(r.stderr[-2000:])
            return time.perf_counter() - t0

        run([files[0]] + common + ["--output", os.path.join(tmp, "warm.xyz")])   # first start of the interpreter and the library
        separate = sum(run([f] + common + ["--output", os.path.join(tmp, f"cut{c}.xyz")]) for c, f in enumerate(files))
        stacked = run([files[0]] + common + ["--stack", files[1], files[2], "--span", "0,0.05,0.1", "--layers", "33", "--output", os.path.join(tmp, "blade.xyz")])
        print(f"T106, three cuts, --hip --iterations 10: three separate jobs (2-D files) {separate:.2f} s wall; one job with --stack, 33 layers (3-D file) {stacked:.2f} s wall")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--report", metavar="KERNEL_STATS_CSV")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cli-wall", action="store_true")
    ap.add_argument("--size", type=int, default=N)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.size)
    elif args.cli_wall:
        cli_wall()
    else:
        workload(args.size, args.repeats)


if __name__ == "__main__":
    main()
