"""The driver's contract with bench.py: ONE JSON line on stdout with the agreed keys (task description, "Measurement")."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"}
ROOFLINE = {"bound", "achieved", "peak", "unit", "frac", "traffic"}
BASELINE = {"value", "unit", "cores", "kind", "sample"}


def test_cpu_baseline_leg_runs_on_the_host_alone():
    # the only place outside tests/ and smoke() that may use the oracle; bounded sample, no GPU involved
    sys.path.insert(0, ROOT)
    import bench

    b = bench.cpu_baseline(129, budget_s=0.3, with_t106=False)
    assert BASELINE <= set(b) and b["kind"] == "port" and b["cores"] == 1 and b["value"] > 0
    # the reference's path stage by stage (fill, BiCGStab-diagonal, GMRES+ILU0, residual + copy-back), sizes stated
    st = b["stages"]
    assert {"tfi", "init", "fill", "bicgstab_diag", "gmres30_ilu0", "residual_copyback"} <= set(st)
    assert st["bicgstab_diag"]["iterations"] == 3 and st["gmres30_ilu0"]["iterations"] == 4
    assert all(st[k]["seconds"] > 0 for k in ("fill", "bicgstab_diag", "gmres30_ilu0", "residual_copyback"))
    m = b["mirror_sweep"]
    assert m["cores"] == 1 and m["value"] > 0 and m["all_threads"]["cores"] >= 1 and m["all_threads"]["value"] > 0


def test_t106_json_as_written_cpu_leg():
    sys.path.insert(0, ROOT)
    import bench

    t = bench.t106_cpu()   # BASELINE configs[0]: 10 iterations, GMRES + ILU0, white
    assert t["outer_iterations"] == 10 and t["nodes"] == 25118 and t["cpu_seconds"] > 0


def test_self_launch_command_line(monkeypatch):
    # `python bench.py --gpus N` without a launcher starts N ranks as a CHILD process and relays rank 0's JSON line
    sys.path.insert(0, ROOT)
    import bench

    seen = {}

    class R:
        returncode = 0
        stdout = b'noise\n{"metric": "x", "n_gpus": 4}\n'

    def fake_run(cmd, stdout=None, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return R()

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "7"] and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_dump_outputs_float64_within_64_mb_and_a_fixed_sample(tmp_path, monkeypatch):
    # --dump-outputs on host arrays: every owned node when they fit, else the same seeded sample every time; float64 only, <= 64 MB
    sys.path.insert(0, ROOT)
    import numpy as np

    import bench

    class _Points:
        def __init__(self, a):
            self.data = a

    class _Block:
        def __init__(self, a):
            self.points = _Points(a)

    class _Mesh:
        def __init__(self, arrays):
            self.blocks = [_Block(a) for a in arrays]

    assert bench.DUMP_MAX_NODES * 2 * 8 <= 64 * 2**20
    rng = np.random.default_rng(1)
    mesh = _Mesh([rng.random((7, 9, 2)), rng.random((5, 4, 2)), rng.random((3, 3, 2))])
    whole = np.concatenate([mesh.blocks[b].points.data.reshape(-1, 2) for b in (0, 1)])
    bench.dump_outputs(str(tmp_path / "all"), mesh, [0, 1], {"last_residual": 0.125}, 0, 1)
    assert sorted(os.listdir(tmp_path / "all")) == ["coords.npy", "residual.npy"]
    xy = np.load(tmp_path / "all" / "coords.npy")
    assert xy.dtype == np.float64 and np.array_equal(xy, whole)
    res = np.load(tmp_path / "all" / "residual.npy")
    assert res.dtype == np.float64 and res.tolist() == [0.125]

    monkeypatch.setattr(bench, "DUMP_MAX_NODES", 16)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), mesh, [0, 1], {"last_residual": 0.125}, 0, 1)
    a, b = (np.load(tmp_path / d / "coords.npy") for d in ("s1", "s2"))
    assert a.shape == (16, 2) and np.array_equal(a, b)
    rows = [int(np.flatnonzero((whole == p).all(axis=1))[0]) for p in a]   # sampled nodes of the owned blocks, in node order
    assert rows == sorted(set(rows))

    bench.dump_outputs(str(tmp_path / "r1"), mesh, [0, 1], {"last_residual": 0.5}, 1, 2)   # rank 1 of 2: its own files, half the budget
    assert sorted(os.listdir(tmp_path / "r1")) == ["coords_rank1.npy", "residual_rank1.npy"]
    assert np.load(tmp_path / "r1" / "coords_rank1.npy").shape == (8, 2)


def _bench_line(args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_its_dumped_outputs_repeat(tmp_path):
    # a plain run: the timed steps and the line, none of the --full reports; the same arguments give the same outputs, bit for bit
    import numpy as np

    from tests.conftest import oracle_tfi
    from turbomesh_amd import configs

    for d in ("a", "b"):
        j = _bench_line(["--size", "256", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / d)])
        c = j["config"]
        assert j["steps"] == 7 and j["warmup"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0 and c["full"] is False
        assert "cpu_baseline" not in j and "solve_to_1e-8" not in c and "krylov" not in j["roofline"]
        assert j["roofline"]["stream_ceiling_GBps"] is None and j["roofline"]["single_sweep_reference"] is None
        assert c["cold_ms_per_step"] is None and c["cold_value"] is None            # no W + K steps timed before the settling
        assert c["settle_steps"] > 0 and c["sweeps_before_timed"] == c["settle_steps"] + 2
        assert np.load(tmp_path / d / "residual.npy").tolist() == [c["residual_last"]]   # the last timed step's residual, as the line reports it
    a, b = ({f: np.load(tmp_path / d / f) for f in ("coords.npy", "residual.npy")} for d in ("a", "b"))
    assert a["coords.npy"].shape == (256 * 256, 2) and a["coords.npy"].dtype == np.float64 and np.isfinite(a["coords.npy"]).all()
    assert a["residual.npy"].shape == (1,) and a["residual.npy"][0] > 0
    assert all(np.array_equal(a[f], b[f]) for f in a)
    seed = configs.single_block(256, 256, tfi=oracle_tfi).blocks[0].points.data.reshape(-1, 2)   # the TFI seed (bit-exact on the GPU, smoke())
    assert not np.array_equal(a["coords.npy"], seed)                              # the smoothed state was downloaded, not the seed


@pytest.mark.gpu
def test_bench_full_adds_the_untimed_reports():
    j = _bench_line(["--size", "256", "--steps", "6", "--warmup", "2", "--full", "--no-cpu-baseline"], timeout=600)
    c = j["config"]
    assert c["full"] is True and j["steps"] == 6 and j["ms_per_step"] > 0
    assert c["cold_ms_per_step"] > 0 and c["sweeps_before_timed"] == c["settle_steps"] + 2 + 6 + 2   # cold W + K, settling, W
    assert j["roofline"]["stream_ceiling_GBps"] > 0 and "krylov" in j["roofline"]
    assert j["config"]["solve_to_1e-8"]["outer_iterations"] >= 1 and "solve_to_converged" in j["config"]


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--size", "512", "--steps", "6", "--warmup", "2", "--no-cpu-baseline", "--no-solve"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert KEYS <= set(j) and ROOFLINE <= set(j["roofline"])
    assert j["n_gpus"] == 1 and j["steps"] == 6 and j["warmup"] == 2 and j["higher_is_better"] is True and j["scaling"] == "weak"
    assert j["dtype"] == "f64" and j["data"] == "synthetic" and j["vs_baseline"] is None and "workload" in j["config"]
    assert j["value"] > 0 and j["roofline"]["bound"] == "hbm" and j["roofline"]["peak"] == 8000.0
    assert 0 < j["roofline"]["frac"] <= 1.0 and j["roofline"]["launches_timed"] >= 1   # a bandwidth fraction, never above the peak


@pytest.mark.gpu
@pytest.mark.parametrize("pair_sync", ["counters", "events", "triples"])
def test_bench_gpus4_config4_rehearsal_on_one_gpu_is_bit_identical_to_one_handle(pair_sync):
    # `python bench.py --gpus 4 --config 4` launches its own ranks; rehearsed on ONE GPU with the gloo transport (halo rows staged
    # through the host; RCCL refuses two ranks on one device): strong scaling of the 8-block strip, 2 blocks per rank, and after
    # 4+21 sweeps every rank's blocks equal the single-handle run of the whole strip bit for bit.  4 ranks + this process <= 6.
    # Both forms of the cross-queue ordering inside a sweep pair: one-wave signal / wait kernels on device-memory counters (the
    # default for one multi-rank handle per process) and hipEvent record / wait (TM_PAIR_SYNC=events).
    env = dict(os.environ, TM_BENCH_SAME_DEVICE="1", TM_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    env.pop("TM_PAIR_SYNC", None)
    if pair_sync == "events":
        env["TM_PAIR_SYNC"] = "events"
    env["TM_TRIPLES_MIN_NODES"] = "-1"   # the PAIR schedule (since round 4 the default is triples at every size)
    if pair_sync == "triples":   # sweep triples across ranks (depth-3 halo, one exchange per triple): the threshold lowered to these 96^2 blocks
        env["TM_TRIPLES_MIN_NODES"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--config", "4", "--size", "96", "--steps", "21", "--warmup", "4",
                        "--verify", "--transport", "torch", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 4 and j["scaling"] == "strong" and j["config"]["nodes_total"] == 8 * 96 * 96 and j["config"]["nodes_per_gpu"] == 2 * 96 * 96
    assert j["config"]["verified_against_single_handle"] is True
    assert 0 < j["roofline"]["frac"] <= 1.0
