"""Timing of the mesh quality pass (tm_smoother_quality: one k_quality launch per block + one finalize launch + the copy of the
records) on the 4096^2 bench block and on the T106 example mesh, beside one single-sweep pass of the relaxation kernel (K2,
TM_OPT_SINGLE_SWEEP) on the same handle in the same run -- the yardstick: the quality pass reads 16 B/node, a sweep moves 32.
An event pair per repeat around the call; the sweep by the handle's own event pairs (Smoother.profile / profile_read).

    python tools/quality_timing.py [--repeats 7] [--size 4096] [--out profiles/quality_timing.txt]      (needs the MI355X)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from turbomesh_amd import configs  # noqa: E402
from turbomesh_amd.input import Input  # noqa: E402
from turbomesh_amd.smoothing import smooth, solver  # noqa: E402


def spread(v):
    v = np.asarray(v)
    return f"median {np.median(v):9.4f}  min {v.min():9.4f}  max {v.max():9.4f}"


def time_handle(sm, repeats):
    """(ms per quality call by event pairs, wall ms per call, ms per single sweep) on a warm handle."""
    sm.quality()   # allocates the records, warms the code object
    sm.iterate(2)
    ev, wall, sweep = [], [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        sm.quality()
        e1.record()
        e1.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(e0.elapsed_time(e1))
        sm.profile(1)
        sm.iterate(1)
        ms, _, _ = sm.profile_read()
        sm.profile(0)
        sweep.append(ms)   # every K2 launch of the sweep bracketed: their sum (one launch on a single block)
    return ev, wall, sweep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join("profiles", "quality_timing.txt"))
    args = ap.parse_args()
    opt = solver.Option.hip(inner=solver.Inner.relax, single_sweep=True)
    lines = [f"mesh quality pass (tm_smoother_quality) beside one single-sweep relaxation pass (K2) of the same handle, ms, {args.repeats} repeats "
             "after a warm-up (tools/quality_timing.py)"]
    n = args.size
    gold = os.path.join(ROOT, "tests", "golden")
    inp = Input.parse(open(os.path.join(gold, "examples", "T106", "T106.json")).read())
    cases = [(f"{n}^2 bench block ({(n - 1) ** 2} cells)", configs.single_block(n, n, perturb=0.25)),
             ("T106 (8 blocks, 25118 nodes)", inp.template.run(inp.geometry(gold)))]
    for label, mesh in cases:
        nodes = sum(b.points.size[0] * b.points.size[1] for b in mesh.blocks)
        with smooth.Smoother(mesh, opt) as sm:
            ev, wall, sweep = time_handle(sm, args.repeats)
            per, total = sm.quality()
        lines.append(f"  {label}")
        lines.append(f"    quality, event pair around the call   {spread(ev)}   {16.0 * nodes / (1e-3 * np.median(ev)) / 1e9:8.1f} GB/s of 16 B/node")
        lines.append(f"    quality, wall time of the call        {spread(wall)}")
        lines.append(f"    single sweep pass (K2 event pairs)    {spread(sweep)}   {32.0 * nodes / (1e-3 * np.median(sweep)) / 1e9:8.1f} GB/s of 32 B/node")
        lines.append(f"    quality / sweep (medians) {np.median(ev) / np.median(sweep):.2f}; report: inverted {total.inverted} degenerate {total.degenerate} "
                     f"min scaled jacobian {total.min_scaled_jacobian:.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
