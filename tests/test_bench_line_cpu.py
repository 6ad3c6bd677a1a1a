"""The ONE stdout line of bench.py must stay something the driver can parse (round-5 verdict: it had grown to 23.5 KB and
`BENCH_r05.json` recorded `parsed: null`).  Held here, for the N = 1 and the N > 1 emitters alike: the line is one JSON object
below 8 KB with every contract key, `roofline` and `cpu_baseline` as objects of numbers, and `roofline.frac` follows from `value`
(same clock).  The GPU legs are stubbed (tests/stubs/bench_stub.py); record building, compaction and emission are the real code."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config")
ROOFLINE = ("bound", "achieved", "peak", "unit", "frac", "traffic")
CPU = ("value", "unit", "cores", "kind", "sample")


def _run(cmd, tmp_path, extra_env=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update({"EMX_BENCH_STUB": "tests.stubs.bench_stub", "EMX_BENCH_STUB_DIR": str(tmp_path), "PYTHONPATH": ROOT,
                "EMX_BENCH_DETAIL": os.path.join(str(tmp_path), "bench_detail.json")})
    env.update(extra_env or {})
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    return r, [ln for ln in r.stdout.splitlines() if ln.strip()]


def _check_line(text):
    assert len(text) < 8192, "the bench line is %d bytes" % len(text)
    line = json.loads(text)
    for k in CONTRACT:
        assert k in line, k
    assert "workload" in line["config"]
    return line


def test_n1_line_is_compact_and_roofline_follows_from_value(tmp_path):
    r, lines = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"], tmp_path, {"EMX_BENCH_STUB_SINGLE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, r.stdout[:2000]
    line = _check_line(lines[0])
    assert line["n_gpus"] == 1 and line["steps"] == 20 and line["warmup"] == 5 and line["dtype"] == "f64" and line["vs_baseline"] is None
    rl, cpu = line["roofline"], line["cpu_baseline"]
    for k in ROOFLINE:
        assert k in rl, k
    for k in CPU:
        assert k in cpu, k
    assert rl["bound"] == "hbm" and rl["unit"] == "GB/s" and rl["peak"] == 8000.0
    # ONE clock: frac == value x (24 D + 17) / 8e12 to three digits, and the event clock's figure is a separate key
    assert rl["algorithmic_bytes_per_walker_update"] == 1553
    assert rl["frac"] == pytest.approx(line["value"] * 1553 / 8e12, rel=1e-3)
    assert rl["achieved"] == pytest.approx(line["value"] * 1553 / 1e9, rel=1e-3)
    assert rl["frac_event_clock"] == pytest.approx(rl["frac"] / 0.977, rel=1e-3)
    assert line["value"] == pytest.approx(65536 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert rl["avg_halfstep_us"] == pytest.approx(line["ms_per_step"] * 1e3 / 2 * 0.977, rel=1e-3)         # hipEvent time per half-step
    # one small object per further configuration, every one with the fraction on its own wall clock
    assert set(line["configs"]) == {"c3_262144x32_rosen", "c4_de_snooker", "c5_16384x1024_diag", "c2_store", "hbm_1048576x64_dense",
                                    "hbm_262144x1024_diag", "wide_65536x512_dense", "dense_65536x128_fused"}
    for name, c in line["configs"].items():
        assert set(c) <= {"nwalkers", "ndim", "ms_per_step", "wu_per_s", "accept_frac", "device_status", "bound", "frac", "frac_event_clock",
                          "frac_traffic", "algorithmic_bytes_per_walker_update", "algorithmic_flops_per_walker_update",
                          "mfma_f64_frac_wall_clock", "frac_kernel", "frac_of_achievable_6300"}, name
        per = c.get("algorithmic_bytes_per_walker_update")
        if c["bound"] == "hbm":
            assert c["frac"] == pytest.approx(c["wu_per_s"] * per / 8e12, rel=1e-3), name
    assert {"c2", "c3", "mid_ms_per_step"} <= set(line["exact_mode"]) and "ms_per_step" in line["exact_mode"]["c2"]
    assert line["quality"]["within_2pct"] is True
    assert cpu["kind"] == "reference" and cpu["cores"] == 16 and len(cpu["modes"]) == 3
    # no paragraph survives in the line; the full record is beside it
    assert max(len(v) for v in _strings(line)) <= 300
    detail = json.load(open(os.path.join(str(tmp_path), "bench_detail.json")))
    assert "note" in detail["roofline"] and "pipeline_stage_us_per_step" in detail["exact_mode"]
    assert detail["value"] == pytest.approx(line["value"], rel=1e-5)
    assert "[bench-detail] {" in r.stderr


def _single_calls(tmp_path):
    with open(os.path.join(str(tmp_path), "single.log")) as f:
        return [json.loads(ln) for ln in f]


def test_n1_plain_run_times_exactly_k_steps_of_the_headline_and_nothing_else(tmp_path):
    r, lines = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], tmp_path, {"EMX_BENCH_STUB_SINGLE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1, r.stdout[:2000]
    line = _check_line(lines[0])
    assert line["steps"] == 20 and line["warmup"] == 5 and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["unit"] == "walker-updates/s" and line["metric"].startswith("walker-updates/sec")
    assert line["value"] == pytest.approx(65536 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["roofline"]["frac"] == pytest.approx(line["value"] * 1553 / 8e12, rel=1e-3)
    # one measurement: the headline, one block of exactly K steps after W, from the seeded inputs, no kernel pass
    calls = _single_calls(tmp_path)
    assert calls == [{"key": "c2", "N": 65536, "K": 20, "W": 5, "single_block": True, "want_kernel": False, "restart": True, "outputs": False}]
    assert line["timing"] == "one K-step block"
    for k in ("configs", "exact_mode", "quality"):
        assert k not in line, k
    assert line["cpu_baseline"] is None


def test_n1_dump_outputs_writes_the_last_step_and_repeats(tmp_path):
    got = []
    for i in range(2):
        d = tmp_path / ("out%d" % i)
        r, lines = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(d)], tmp_path,
                        {"EMX_BENCH_STUB_SINGLE": "1"})
        assert r.returncode == 0, r.stderr[-3000:]
        assert len(lines) == 1 and _check_line(lines[0])["steps"] == 7
        names = sorted(os.listdir(str(d)))
        assert names == ["accepted.npy", "coords.npy", "log_prob.npy"]
        arrs = {n: np.load(os.path.join(str(d), n)) for n in names}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert sum(os.path.getsize(os.path.join(str(d), n)) for n in names) <= 64 << 20
        assert arrs["coords.npy"].shape == (65536, 64) and arrs["log_prob.npy"].shape == (65536,)
        got.append(arrs)
    assert all(np.array_equal(got[0][n], got[1][n]) for n in got[0])
    assert _single_calls(tmp_path)[0]["outputs"] is True


def test_dump_outputs_is_refused_beyond_one_gpu(tmp_path):
    r, lines = _run([sys.executable, "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--config", "c2",
                     "--dump-outputs", str(tmp_path / "out")], tmp_path)
    assert r.returncode != 0
    line = json.loads(lines[-1])
    assert line["value"] is None and "--dump-outputs" in line["error"]
    assert not os.path.exists(str(tmp_path / "out"))


def test_multi_gpu_plain_run_measures_the_headline_configuration_alone(tmp_path):
    r, lines = _run([sys.executable, "bench.py", "--gpus", "2", "--steps", "5", "--warmup", "1"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1
    line = _check_line(lines[0])
    assert line["n_gpus"] == 2 and line["value"] > 0
    assert set(line["multi_gpu"]) == {"c2_weak_65536_per_gpu"}


def _strings(o):
    if isinstance(o, str):
        yield o
    elif isinstance(o, dict):
        for v in o.values():
            yield from _strings(v)
    elif isinstance(o, list):
        for v in o:
            yield from _strings(v)


@pytest.mark.parametrize("world", [2, 8])
def test_multi_gpu_line_is_compact(tmp_path, world):
    r, lines = _run([sys.executable, "bench.py", "--gpus", str(world), "--steps", "5", "--warmup", "1", "--full"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1
    line = _check_line(lines[0])
    assert line["n_gpus"] == world and line["rccl_ranks"] == world and line["distinct_devices"] == world
    assert line["roofline"]["frac"] == pytest.approx(line["value"] * 1553 / 8e12 / world, rel=1e-3)        # per GPU
    assert line["cpu_baseline"] is None
    multi = line["multi_gpu"]
    assert set(multi) == {"c2_weak_65536_per_gpu", "c3_262144x32_rosen_sharded", "c5_16384x1024_strong", "wide_65536x512_dense_weak"}
    for name, e in multi.items():
        # measured and predicted side by side, one number per protocol
        assert e["ms_per_step"] > 0 and e["predicted_us_per_step"] > 0 and e["reported"] in e["us_per_step_by_exchange"], name
        assert all(isinstance(v, float) for v in e["us_per_step_by_exchange"].values())
    assert line["time_budget"]["time_budget_s"] == 840.0
    detail = json.load(open(os.path.join(str(tmp_path), "bench_detail.json")))
    assert "xgmi_bytes_per_walker_update" in detail["multi_gpu"]["c2_weak_65536_per_gpu"]["exchange"]["pull"]


def test_the_round5_record_compacts_below_the_limit():
    """the 23.5 KB record the driver could not parse, through the compactor"""
    from tools.benchkit.emit import LINE_LIMIT, compact
    path = os.path.join(ROOT, "profiles", "r05", "bench_n1.json")
    rec = json.loads(open(path).read())
    assert len(json.dumps(rec)) > 20000
    line = compact(rec)
    text = json.dumps(line)
    assert len(text) <= LINE_LIMIT
    for k in CONTRACT:
        assert k in line
    assert line["roofline"]["frac"] > 0 and line["cpu_baseline"]["kind"] == "reference"
    assert set(line["configs"]) == set(rec["configs"])


def test_an_oversized_record_still_fits():
    """whatever a future section adds: optional sections are replaced by a pointer to the detail file, the contract keys stay"""
    from tools.benchkit.emit import LINE_LIMIT, compact
    rec = {"metric": "m", "value": 1.0, "unit": "u", "n_gpus": 1, "steps": 1, "warmup": 0, "ms_per_step": 1.0, "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic", "config": {"workload": "w" * 5000},
           "roofline": {"bound": "hbm", "achieved": 1.0, "peak": 8000.0, "unit": "GB/s", "frac": 1.0 / 8000, "traffic": None, "note": "n" * 9000},
           "cpu_baseline": {"value": 1.0, "unit": "u", "cores": 1, "kind": "port", "sample": "s" * 4000},
           "configs": {"cfg%d" % i: {"ms_per_step": 1.0, "wu_per_s": 1.0, "roofline": {"bound": "hbm", "frac": 0.5}} for i in range(200)}}
    text = json.dumps(compact(rec))
    assert len(text) <= LINE_LIMIT
    line = json.loads(text)
    assert line["configs"].startswith("see ") and line["roofline"]["frac"] == 1.0 / 8000 and line["cpu_baseline"]["kind"] == "port"
