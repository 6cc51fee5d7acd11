"""The sky resolve of B views: ms per view of ONE pbr_skybox_views / pbr_skybox_bc6h_views call against B sequential pbr_skybox /
pbr_skybox_bc6h calls, for B in {1, 2, 4, 8, 16} at 1440x960 and 3840x2160.  Every pixel is sky (stencil 0: the resolve's worst
case); the fp32 sky is synth.env_cube(256) with its mips, the resident one tests/golden/sky_bc6h.npz's smooth file; the reference
camera with the yaw varied per view.  K calls back to back between two events.  Three rounds, every (size, round) in a fresh child
process under its own `timeout`; batched and sequential runs interleave inside a child; medians over the rounds, and the spread
(max - min over the rounds) of the sequential figure beside them.
python tools/multiview_sky_ms.py [--rounds 3] [--calls 50] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = (1, 2, 4, 8, 16)
SIZES = ((1440, 960), (3840, 2160))
KINDS = ("f32", "bc6h")
SKY_SIZE = 256


def child(W, H, calls):
    import numpy as np
    import torch

    from direct12pbrrenderer_amd import host, scene, synth
    from direct12pbrrenderer_amd.api import PbrContext
    from direct12pbrrenderer_amd.structs import Tile, View

    ctx = PbrContext(0)
    mips = SKY_SIZE.bit_length()
    cube = ctx.upload(synth.env_cube(SKY_SIZE))
    ctx.cube_gen_mips(cube, SKY_SIZE, mips)
    data = np.load(os.path.join(ROOT, "tests", "golden", "sky_bc6h.npz"), allow_pickle=False)["smooth_file"]
    bsize, bmips, offsets, _ = host.parse_cubemap_file(data.tobytes())
    staged = ctx.upload(data.copy())
    faces = [staged.data_ptr() + o for o in offsets]
    nmax = max(BATCHES)
    tile = Tile(0, 0, W, H, W, H)
    stencil = ctx.zeros((H, W), torch.uint8)
    hdrs = [ctx.zeros((H, W, 4), torch.float16) for _ in range(nmax)]
    globals_ = []
    for v in range(nmax):
        cam = scene.Camera.reference_default(W, H)
        cam.rotate(0.0, 0.2 * v, 0.0)
        globals_.append(scene.make_global(cam, W, H))
    views = (View * nmax)()
    for v in range(nmax):
        views[v].g = globals_[v]
        views[v].gb.stencil, views[v].gb.pitch = stencil.data_ptr(), W
        views[v].hdr, views[v].hdr_pitch = hdrs[v].data_ptr(), W

    def batched(kind, b):
        if kind == "f32":
            ctx.skybox_views(views, b, W, H, cube, SKY_SIZE, mips)
        else:
            ctx.skybox_bc6h_views(views, b, W, H, faces, bsize, bmips)

    def sequential(kind, b):
        for v in range(b):
            if kind == "f32":
                ctx.skybox(globals_[v], tile, cube, SKY_SIZE, mips, stencil, W, hdrs[v], W)
            else:
                ctx.skybox_bc6h(globals_[v], tile, faces, bsize, bmips, stencil, W, hdrs[v], W)

    def timed(fn, kind, b):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn(kind, b)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (calls * b)

    for kind in KINDS:   # warm-up (clocks, code objects)
        for b in BATCHES:
            for _ in range(3):
                batched(kind, b)
                sequential(kind, b)
    torch.cuda.synchronize()
    out = {}
    for kind in KINDS:
        for b in BATCHES:
            r = {"batched": [], "sequential": []}
            for _ in range(2):   # interleaved: batched, sequential, batched, sequential
                r["batched"].append(timed(batched, kind, b))
                r["sequential"].append(timed(sequential, kind, b))
            out[f"{kind}/{b}"] = {k: min(v) for k, v in r.items()}
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=200, help="seconds per child (one size, one round)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), a.calls)
        return 0
    runs = {f"{W}x{H}": [] for W, H in SIZES}
    for rnd in range(a.rounds):
        for W, H in SIZES:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--calls", str(a.calls), "--child", str(W), str(H)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                print(f"round {rnd} {W}x{H}: child failed with status {p.returncode}; stopping", file=sys.stderr)
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            runs[f"{W}x{H}"].append(json.loads(line[7:]))
    report = {"tool": "tools/multiview_sky_ms.py", "rounds": a.rounds, "calls_per_run": a.calls,
              "unit": "ms per view (median over rounds of the best of two interleaved runs); spread = max - min of the sequential figure over the rounds",
              "configs": {}}
    lines = []
    for W, H in SIZES:
        key = f"{W}x{H}"
        cfg = {}
        for kind in KINDS:
            lines.append(f"{key} / {'fp32 cube 256^2' if kind == 'f32' else 'BC6H-resident 32^2'}:   B   one call  sequential  (spread)   ratio")
            for b in BATCHES:
                rows = [r[f"{kind}/{b}"] for r in runs[key]]
                bat = statistics.median(x["batched"] for x in rows)
                seq = statistics.median(x["sequential"] for x in rows)
                spread = max(x["sequential"] for x in rows) - min(x["sequential"] for x in rows)
                cfg[f"{kind}/{b}"] = {"batched": round(bat, 5), "sequential": round(seq, 5), "sequential_spread": round(spread, 5), "ratio": round(seq / bat, 3)}
                lines.append(f"{'':>36}{b:>3}   {bat:.5f}   {seq:.5f}    ({spread:.5f})  {seq / bat:.2f}x")
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
