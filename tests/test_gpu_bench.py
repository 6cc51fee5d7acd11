"""bench.py's output contract on the GPU box: exactly ONE line on stdout — the JSON record — whether the process is the
single-GPU bench or spawns its own ranks (`--gpus 2` on a one-GPU box = rehearsal mode: both ranks on cuda:0, gloo + host
copies, which makes gloo print its connection banner to the C stdout), with the keys the driver reads."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
        "config", "roofline"}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("extra,n", [([], 1), (["--gpus", "2"], 2), (["--gpus", "3", "--width", "960", "--height", "544"], 3)])
def test_bench_prints_one_json_line(extra, n):
    cmd = ["timeout", "-k", "10", "500", sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--settle", "5", "--no-cpu-baseline"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, lines[:5]
    rec = json.loads(lines[0])
    assert KEYS <= set(rec) and rec["n_gpus"] == n and rec["steps"] == 3 and rec["warmup"] == 1 and rec["value"] > 0
    assert rec["config"]["clock_settle_frames"] == 5 and "workload" in rec["config"]
    assert rec["roofline"]["bound"] in ("hbm", "mfma") and rec["roofline"]["achieved"] > 0
    assert "roughness" in rec["config"]["workload"] and "attenuation preset" in rec["config"]["workload"]     # the headline says what it timed
    fr = rec["roofline"]["frame"]
    assert rec["roofline"]["kernel_limited_by"] == "valu" and fr["bytes"] > 0 and 0 < fr["frac"] < 1 and abs(fr["GBps"] * rec["ms_per_step"] * 1e6 - fr["bytes"]) < 1e-2 * fr["bytes"]
    if n == 1:
        ab = rec["shade_ms_by_path"]
        assert set(ab) >= {"as_shipped", "roughness_0_255", "two_attenuation_presets", "roughness_0_255_and_two_presets"}, ab
        lp = {k: v["mean_lights_per_pixel"] for k, v in ab.items() if isinstance(v, dict)}
        assert max(lp.values()) - min(lp.values()) < 0.02, lp      # the variants differ in the walk instantiation, not in the work
        box = rec["roofline"]["box"]                                   # the normalisers come from THIS box, in this run
        assert box["plain_v_mul_f32"]["Ginst_s"] > 100 and 0.5 < box["packed_v_pk_fma_f32"]["clock_GHz"] < 3.0 and box["hbm_read_GBps"] > 1000
        assert box["shade_simd_cycles_per_pixel"] > 10
        if "valu" in rec["roofline"]:                                  # (needs a committed counter profile of this very shade.hip)
            assert rec["roofline"]["valu"]["shade_simd_cycles_per_pixel"] > 0
        # round 6: every single-GPU BASELINE config and the reference's own operating point in the same line (no CPU legs here: --no-cpu-baseline)
        cf = rec["configs"]
        assert "error" not in cf, cf
        assert cf["cfg1_brdf_lut"]["lut256"]["ms"] > 0 and cf["cfg1_brdf_lut"]["lut512"]["Msamples_per_s"] > 1e4
        c2 = cf["cfg2_1080p_1_light"]
        assert 0 < c2["shade_ms"] < 1 and c2["unit"] == "Mpixel/s" and abs(c2["value"] * c2["shade_ms"] * 1e3 / (1920 * 1080) - 1.0) < 1e-2   # (both are rounded in the record)
        r2 = c2["roofline"]
        assert r2["bound"] == "hbm" and r2["algorithmic_bytes"] == 25 * 1920 * 1080 and abs(r2["frac"] - r2["achieved"] / r2["peak"]) < 1e-3
        assert r2["traffic"] is None or r2["traffic"] > r2["algorithmic_bytes"]      # (None: no counter profile of this very shade.hip committed)
        c3 = cf["cfg3_prefilter_sh9"]
        assert c3["prefilter_fp32_source"]["ms"] > c3["prefilter_half_representable_source"]["ms"] > 0 and c3["sh9"]["ms"] > 0
        rp = cf["reference_operating_point"]
        assert "error" not in rp and rp["dispatch_by_dispatch"]["dispatches_per_frame"] == 23 and rp["fused_passes"]["dispatches_per_frame"] == 7
        assert rp["dispatch_by_dispatch"]["ms_per_frame"] >= rp["fused_passes"]["ms_per_frame"] > 0
    if n > 1:
        # the multi-rank orchestration, rehearsed on the one GPU (gloo + host copies): the grid, the cfg5 sub-record with its single-GPU
        # denominator, and the C++ pass graph leg (loopback halo transport) all come back in the one record.  (Three ranks, not four: the
        # pool kills a job with more than 6 processes holding the card, and this test runs inside a pytest process that holds it too,
        # next to torch.distributed.run's agent; the 2x2 rehearsal is kept as profiles/r05_p_rehearsal4.json)
        assert "rehearsal" in rec and rec["config"]["layout_rows_x_cols"] == {2: "1x2", 3: "1x3"}[n], rec["config"]
        c5 = rec["config"]["cfg5"]
        assert "error" not in c5 and c5["single_gpu_ms_per_step"] > 0 and c5["ms_per_step"] > 0 and c5["speedup_vs_single_gpu"] > 0, c5
        hg = rec["host_graph"]
        assert "error" not in hg and hg["fused_throughput_ms"] > 0 and "rehearsal" in hg, hg
        assert "error" not in c5["host_graph"] and c5["host_graph"]["fused_throughput_ms"] > 0, c5["host_graph"]


@pytest.mark.timeout(600)
def test_bench_dump_outputs_is_reproducible(tmp_path):
    """`--dump-outputs DIR`: the last timed frame's outputs (bench.frame_outputs) as float32 .npy files within 64 MB; two runs with the same
    arguments render the same inputs and dump the same arrays, bit for bit (no atomics on floats anywhere in the frame)."""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        cmd = ["timeout", "-k", "10", "250", sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--settle", "3",
               "--no-cpu-baseline", "--no-kernel-timing", "--no-host-graph", "--no-shade-paths", "--no-configs", "--no-tail-overlap", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        rec = json.loads(r.stdout.splitlines()[-1])
        assert rec["steps"] == 4 and rec["ms_per_step"] > 0
        assert sorted(os.listdir(d)) == ["avg_luminance.npy", "hdr.npy", "ldr.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = dumps
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["hdr"].shape == a["ldr"].shape == (1 << 20, 4) and a["avg_luminance"].shape == (1,)
    assert np.isfinite(a["hdr"]).all() and (a["hdr"][:, :3] >= 0).all() and a["hdr"][:, :3].max() > 0 and a["avg_luminance"][0] > 0
    assert (a["ldr"] >= 0).all() and (a["ldr"] <= 255).all() and a["ldr"][:, :3].max() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k
