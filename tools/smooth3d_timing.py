"""Timing of the 3-D elliptic smoothing kernels (K22: k_s3_sweep, k_s3_control_faces, k_s3_control_blend) beside a device-to-device copy
of the same three planes and K11's launch for the same block.

Workload: 8 resident cuts of 2049^2 (config 5: amplitude 0.05 + 0.001 c, one handle per cut), cubic, planar, 33 layers -- one block of
138.5 M nodes, stacked on the device and smoothed there (tm_stack_smoothers_smooth), SWEEPS Laplace sweeps and SWEEPS Thomas-Middlecoff
sweeps; tm_stream_probe with 24 B per node and array in the same run: its copy kernel (k_stream<0>) moves the compulsory 24 + 24 B/node
of a sweep and nothing else.

    python tools/smooth3d_timing.py --all        every GPU step under its own `timeout`, stopping at the first failure: ONE
                                                 `rocprofv3 --kernel-trace --stats --output-format csv` run of the workload (no counters in it), then the
                                                 report into profiles/smooth3d_timing.txt and the statistics into
                                                 profiles/smooth3d_kernel_stats.csv                                    (needs the MI355X)
    python tools/smooth3d_timing.py              the workload alone (what the profiler runs)
    python tools/smooth3d_timing.py --report KERNEL_STATS_CSV [--out FILE]      no GPU: reads the CSV

Bytes per node and sweep: 24 read + 24 written, + 24 of field with a control function.  Aim, recorded and not asserted: a Laplace sweep
within 2 x the copy."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, CUTS, LAYERS, SWEEPS = 2049, 8, 33, 4
KERNELS = [   # (label, substrings that must all occur in the kernel's name, bytes per node of the block, what they are)
    ("k_s3_sweep<false>", ("k_s3_sweep", "false"), 48, "Laplace sweep: 24 read + 24 written"),
    ("k_s3_sweep<true>", ("k_s3_sweep", "true"), 72, "Thomas-Middlecoff sweep: 24 + 24 of field read, 24 written"),
    ("k_s3_control_faces", ("k_s3_control_faces",), None, "line formula on the faces"),
    ("k_s3_control_blend", ("k_s3_control_blend",), 24, "transfinite blend: 24 written"),
    ("k_s3_finalize", ("k_s3_finalize",), None, "record of a sweep, one wave"),
    ("k_stream<0>", ("k_stream<0",), 48, "device-to-device copy of three planes: 24 read + 24 written"),
    ("k_stack_planes", ("k_stack_planes",), 24, "K11, all 33 layers in one launch: 16 x 8 / 33 read + 24 written"),
]


def workload(n, sweeps):
    import ctypes as C

    import numpy as np

    from turbomesh_amd import _capi, configs, stack
    from turbomesh_amd.smoothing import smooth, solver

    handles = [smooth.Smoother(configs.single_block(n, n, amplitude=0.05 + 0.001 * c), solver.Option.hip(inner=solver.Inner.relax)) for c in range(CUTS)]
    try:
        for h in handles:
            h.iterate(3)
        z = np.arange(CUTS, dtype=np.float64)
        st = stack.Stack(z, stack.layers_from(z, LAYERS), "cubic", "planar")
        for algorithm in ("laplace", "thomas-middlecoff"):
            t0 = time.perf_counter()
            *_, info = st.smooth(handles, 0, sweeps, algorithm)
            print(f"smooth3d_timing: {algorithm}: {info.line('block')}; {time.perf_counter() - t0:.2f} s wall (the planes to the host included)")
        copy, triad = C.c_double(), C.c_double()
        _capi.check(_capi.lib().tm_stream_probe(24 * n * n * LAYERS, 5, C.byref(copy), C.byref(triad)))
        print(f"smooth3d_timing: tm_stream_probe at 24 B/node: copy {copy.value:.0f} GB/s triad {triad.value:.0f} GB/s")
    finally:
        for h in handles:
            h.close()


def report(stats_csv, out, n):
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            for label, needles, _, _ in KERNELS:
                name = r["Name"]
                if all(s in name for s in needles):
                    rows.setdefault(label, r)
    if "k_s3_sweep<false>" not in rows:
        sys.exit(f"{stats_csv}: no k_s3_sweep rows")
    nodes = float(n) * n * LAYERS
    lines = [f"K22 on one block of {n} x {n} x {LAYERS} = {nodes / 1e6:.1f} M nodes stacked from {CUTS} resident cuts (cubic, planar): kernel times of one "
             f"rocprofv3 --kernel-trace --stats run of tools/smooth3d_timing.py (no counters), every launch of the run averaged; {SWEEPS} sweeps per algorithm"]
    avg = {}
    for label, _, bpn, what in KERNELS:
        r = rows.get(label)
        if r is None:
            lines.append(f"  {label:20s} not in the trace")
            continue
        a, lo, hi = float(r["AverageNs"]) / 1e6, float(r["MinNs"]) / 1e6, float(r["MaxNs"]) / 1e6
        avg[label] = a
        rate = f"  {bpn * nodes / (a * 1e-3) / 1e12:.2f} TB/s of {bpn} B/node" if bpn else ""
        lines.append(f"  {label:20s} {int(r['Calls']):3d} calls  average {a:9.3f} ms  min {lo:9.3f}  max {hi:9.3f}{rate}  ({what})")
    if "k_stream<0>" in avg:
        for label in ("k_s3_sweep<false>", "k_s3_sweep<true>"):
            if label in avg:
                lines.append(f"  {label} / copy = {avg[label] / avg['k_stream<0>']:.2f}" + (" (aim: <= 2)" if "false" in label else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def run_all(n, sweeps):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "smooth3d", "--", sys.executable, os.path.abspath(__file__),
               "--size", str(n), "--sweeps", str(sweeps)]
        r = subprocess.run(cmd, cwd=ROOT)
        if r.returncode != 0:
            sys.exit(f"the profiled workload ended with status {r.returncode}: nothing further is run")
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            sys.exit("rocprofv3 wrote no kernel statistics")
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        shutil.copy(found[0], os.path.join(ROOT, "profiles", "smooth3d_kernel_stats.csv"))
    report(os.path.join(ROOT, "profiles", "smooth3d_kernel_stats.csv"), os.path.join(ROOT, "profiles", "smooth3d_timing.txt"), n)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--report", metavar="KERNEL_STATS_CSV")
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=N)
    ap.add_argument("--sweeps", type=int, default=SWEEPS)
    args = ap.parse_args()
    if args.report:
        report(args.report, args.out, args.size)
    elif args.all:
        run_all(args.size, args.sweeps)
    else:
        workload(args.size, args.sweeps)


if __name__ == "__main__":
    main()
