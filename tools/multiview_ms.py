"""Multi-view frames: ms per view of B camera views rendered as ONE chain of launches (pipeline.MultiViewFrame, the pbr_*_views
entry points) against B sequential DeferredFrame.render() calls, for B in {1, 2, 4, 8, 16}:
  * 1440x960 / 8 lights: the reference's operating point (App.h:77-78; the 8 light records of Asset/Scene/main.json from
    tests/golden/scene_lights.npz, reference camera with the yaw varied per view);
  * 1920x1080 / 1 light (the reference scene light).
Both back to back (K batches, one fence at the end) and with a fence per batch (the reference's frame loop waits on its fence).
Three rounds, every (size, round) in a fresh child process under its own `timeout`; batched and sequential runs interleave inside
a child; medians over the rounds.
python tools/multiview_ms.py [--rounds 3] [--frames 40] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = (1, 2, 4, 8, 16)
CONFIGS = ((1440, 960, "scene8"), (1920, 1080, "one"))


def child(W, H, lights_kind, frames):
    import numpy as np
    import torch

    import bench
    from direct12pbrrenderer_amd import scene, synth
    from direct12pbrrenderer_amd.api import PbrContext
    from direct12pbrrenderer_amd.pipeline import DeferredFrame, MultiViewFrame, TileSpec

    ctx = PbrContext(0)
    lut, env, sh = bench.build_ibl(ctx)
    if lights_kind == "scene8":
        recs = np.load(os.path.join(ROOT, "tests", "golden", "scene_lights.npz"))
        lights = np.concatenate([scene.make_lights(recs["translation"][i], recs["color"][i], float(recs["radius"][i]), float(recs["intensity"][i]))
                                 for i in range(len(recs["radius"]))])
    else:
        lights = synth.reference_scene_light()
    gb = synth.gbuffer_tile(0, 0, W, H, W, H)

    def cam_global(v):
        cam = scene.Camera.reference_default(W, H)
        cam.rotate(0.0, 0.2 * v, 0.0)
        return scene.make_global(cam, W, H, sh_pack=sh, delta_time=1.0 / 60.0)

    nmax = max(BATCHES)
    singles = []
    for v in range(nmax):
        fr = DeferredFrame(ctx, TileSpec(0, 0, W, H, W, H, 0), cam_global(v), lights, lut, 512, env, 512, 5)
        fr.upload_gbuffer(gb)
        fr.set_prev_luminance(0.18)
        singles.append(fr)
    multis = {}
    for b in BATCHES:
        mv = MultiViewFrame(ctx, W, H, [cam_global(v) for v in range(b)], [lights] * b, lut, 512, env, 512, 5)
        mv.upload_gbuffers([gb] * b)
        mv.set_prev_luminance(0.18)
        multis[b] = mv

    def batched(b):
        multis[b].render()

    def sequential(b):
        for fr in singles[:b]:
            fr.render()

    def b2b(fn, b):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            fn(b)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (frames * b)

    def fenced(fn, b):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            fn(b)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (frames * b)

    for b in BATCHES:   # warm-up (clocks, one-shot allocations)
        for _ in range(5):
            batched(b)
            sequential(b)
    torch.cuda.synchronize()
    out = {}
    for b in BATCHES:
        r = {}
        for _ in range(2):   # interleaved: batched, sequential, batched, sequential
            for key, fn in (("batched", batched), ("sequential", sequential)):
                r.setdefault(key + "_b2b", []).append(b2b(fn, b))
                r.setdefault(key + "_fenced", []).append(fenced(fn, b))
        out[str(b)] = {k: min(v) for k, v in r.items()}
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child (one size, one round)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), a.child[2], a.frames)
        return 0
    runs = {f"{W}x{H}": [] for W, H, _ in CONFIGS}
    for rnd in range(a.rounds):
        for W, H, kind in CONFIGS:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--child", str(W), str(H), kind]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                print(f"round {rnd} {W}x{H}: child failed with status {p.returncode}; stopping", file=sys.stderr)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            runs[f"{W}x{H}"].append(json.loads(line[7:]))
    report = {"tool": "tools/multiview_ms.py", "rounds": a.rounds, "frames_per_run": a.frames,
              "unit": "ms per view (median over rounds of the best of two interleaved runs)", "configs": {}}
    lines = []
    for W, H, kind in CONFIGS:
        key = f"{W}x{H}"
        cfg = {}
        lines.append(f"{key} / {'8 lights (main.json)' if kind == 'scene8' else '1 light'}:   B   batched b2b  seq b2b  gain   |  batched fenced  seq fenced  gain")
        for b in BATCHES:
            med = {k: statistics.median(r[str(b)][k] for r in runs[key]) for k in runs[key][0][str(b)]}
            med["gain_b2b"] = med["sequential_b2b"] / med["batched_b2b"]
            med["gain_fenced"] = med["sequential_fenced"] / med["batched_fenced"]
            cfg[str(b)] = {k: round(v, 4) for k, v in med.items()}
            lines.append(f"{'':>28}{b:>3}   {med['batched_b2b']:.4f}      {med['sequential_b2b']:.4f}   {med['gain_b2b']:.2f}x  |  "
                         f"{med['batched_fenced']:.4f}          {med['sequential_fenced']:.4f}      {med['gain_fenced']:.2f}x")
        report["configs"][key] = cfg
    text = "\n".join(lines)
    print(text)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n\n" + json.dumps(report, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
