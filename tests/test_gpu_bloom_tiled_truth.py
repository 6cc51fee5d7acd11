"""pbr_bloom_tiled (csrc/bloom.hip), the multi-GPU path of the bloom, under the float64 interval truth of tests/bloom_truth.py
(tiled_chain): the up-pass on shrinking rectangles, the merge of merge_rect alone, its histogram, buf_origin and the first tile in the
fused kernels — at small extended tiles off every tile size and at the benchmark's own rank shapes, where k_blur_up_poly and the
32-row k_blur_hv run with a rectangle.  The poison protocol is test_gpu_bloom_truth's: guards around every plane, chain B and every
level of chain A but the given level 1 poisoned, each call once per poison with the same bits required.  Which kernel ran is read
from the launch log and held to bloom_truth.tiled_kernels.  The knobs build's PBR_BLOOM_SHRINK=0 (the up-pass on whole levels)
runs the big cases in a child process under the same check.  tests/test_bloom_truth_cpu.py proves what the tiling rests on (the
rectangles' margins, the apron) and that the check rejects wrong tiled passes.  `-s` prints the measured figures."""
import os
import tempfile

import numpy as np
import pytest
import torch

import bloom_truth as bt
import common
from test_gpu_bloom_truth import GUARD, POISONS, Plane

pytestmark = pytest.mark.gpu


def run_tiled(ctx, case, level1, hdr, poison):
    """one pbr_bloom_tiled call between poison: (HDR buffer before, after [rows, hdr_pitch, 4] uint16, the histogram or None,
    pbr_lum_histogram of the merged window or None, the labels of the call's launches)"""
    from direct12pbrrenderer_amd.structs import bloom_chain_texels, bloom_level_offset
    (hx, hy, hw, hh), (mx, my, mw, mh) = case.hdr_rect, case.merge_rect
    n = bloom_chain_texels(case.ew, case.eh)
    ca, cb = Plane(ctx, poison, texels=n), Plane(ctx, poison, texels=n)
    o = GUARD + bloom_level_offset(case.ew, case.eh, 1)
    ca.t[o:o + level1.shape[0] * level1.shape[1]] = ctx.upload(np.ascontiguousarray(level1).view(np.uint16).reshape(-1, 4))
    before = np.full((hh, case.hdr_pitch, 4), poison, dtype=np.uint16)          # the pitch padding is poison too
    before[:, :hw] = hdr.view(np.uint16)
    buf = Plane(ctx, poison, before.view(np.float16))
    hist = ctx.zeros((256,), torch.int32) if case.hist else None
    ctx.set_bloom_shader_order(case.shader_order)
    try:
        labels = ctx.launches_of(lambda: ctx.bloom_tiled(buf.ptr, case.hdr_pitch, case.hdr_rect, case.ew, case.eh, ca.ptr, cb.ptr, case.merge_rect, hist))
    finally:
        ctx.set_bloom_shader_order(False)
    plain = None
    if case.hist:
        plain = ctx.zeros((256,), torch.int32)
        ctx.lum_histogram(buf.ptr + 8 * ((my - hy) * case.hdr_pitch + (mx - hx)), mw, mh, case.hdr_pitch, plain)
        hist, plain = (t.cpu().numpy().view(np.uint32) for t in (hist, plain))
    ctx.sync()
    ca.bits(), cb.bits()                                                         # the guards around the two chains
    return before, buf.bits().reshape(hh, case.hdr_pitch, 4), hist, plain, labels


def run_twice(ctx, case, level1, hdr):
    """run_tiled once per poison: the same bits in hdr_rect, the same histogram and the same kernels both times"""
    a, b = (run_tiled(ctx, case, level1, hdr, p) for p in POISONS)
    hw = case.hdr_rect[2]
    assert np.array_equal(a[1][:, :hw], b[1][:, :hw]), "the result depends on what the buffers held before"
    assert a[4] == b[4] and (a[2] is None or np.array_equal(a[2], b[2]))
    for before, after, *_ in (a, b):
        assert np.array_equal(after[:, hw:], before[:, hw:]), "the pitch padding changed"
    return a


def check(case, run, lo, hi, shrink=True):
    """bloom_truth.check_tiled on one run, the tail's histogram against pbr_lum_histogram on the merged window, and the four 2x-up
    launches against the kernels launch_hv's restated rule gives them"""
    before, after, hist, plain, labels = run
    r = bt.check_tiled(case, before, after, hist, lo, hi, case.id)
    if case.hist:
        assert np.array_equal(hist, plain), "the tail's histogram differs from pbr_lum_histogram on the merged window"
    want = bt.tiled_kernels(case.merge_rect, case.ew, case.eh, case.shader_order, shrink)
    assert list(labels[-4:]) == [k[1] for k in want] and len(labels) == 7, (labels, want)
    print(f"{case.id}{'' if shrink else ' (whole up-pass)'}: interval at most {r['width']} wide, {1 - r['degenerate']:.4%} undecided; levels 3 .. 0 ran "
          + ", ".join(f"{k[1]} ({k[3]} tiles from {k[2]})" for k in want)
          + (f"; histogram: {r['ambiguous']} of {case.merge_rect[2] * case.merge_rect[3]} pixels within the truth's band of a bin edge, "
             f"{r['other side']} counted on the other side of it than float64, every other pixel in its bin" if case.hist else ""))
    return r


@pytest.mark.parametrize("case", bt.TILED_SMALL, ids=lambda c: c.id)
def test_tiled_small(ctx, case):
    level1, hdr = case.inputs()
    check(case, run_twice(ctx, case, level1, hdr), *bt.tiled_chain(level1, hdr, case.hdr_rect, case.merge_rect))


# ------------------------------------------------------------------------------------------------------ the benchmark's rank shapes
def _key(case):
    return (case.ew, case.eh, case.hdr_rect, case.merge_rect, case.kind)


@pytest.fixture(scope="module")
def big_truth():
    """(level 1, hdr, lo, hi) per big case, computed once per module and shared by the cases that differ in the switch alone"""
    cache = {}

    def get(case):
        if _key(case) not in cache:
            level1, hdr = case.inputs()
            cache[_key(case)] = (level1, hdr, *bt.tiled_chain(level1, hdr, case.hdr_rect, case.merge_rect))
        return cache[_key(case)]
    return get


@pytest.fixture(scope="module")
def big_product(ctx, big_truth):
    """the product library's run of every big case, once per module"""
    cache = {}

    def get(i):
        if i not in cache:
            level1, hdr = big_truth(bt.TILED_BIG[i])[:2]
            cache[i] = run_twice(ctx, bt.TILED_BIG[i], level1, hdr)
        return cache[i]
    return get


_WHOLE_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import bloom_truth as bt
from direct12pbrrenderer_amd.api import PbrContext
from test_gpu_bloom_tiled_truth import run_twice
ctx = PbrContext(0)
for i, case in enumerate(bt.TILED_BIG):
    before, after, hist, plain, labels = run_twice(ctx, case, *case.inputs())
    np.savez(%r %% i, before=before, after=after, hist=hist, plain=plain, labels=np.array(labels))
ctx.close()
print("whole up-pass ran")
"""


@pytest.fixture(scope="module")
def big_whole():
    """every big case on the knobs build with PBR_BLOOM_SHRINK=0, in one child process (knobs are read once per process): the same
    poison protocol there, the runs handed back in files and checked here against the truth this module already has"""
    with tempfile.TemporaryDirectory() as d:
        r = common.run_child(_WHOLE_CHILD % (common.ROOT, os.path.join(common.ROOT, "tests"), os.path.join(d, "case%d.npz")),
                             {"PBR_BLOOM_SHRINK": "0"}, clear=("PBR_BLOOM_SHRINK", "PBR_BLOOM_WIDE", "PBR_BLOOM_HIST_BLOCKS"), timeout_s=300)
        assert r.returncode == 0 and "whole up-pass ran" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        runs = []
        for i in range(len(bt.TILED_BIG)):
            z = np.load(os.path.join(d, "case%d.npz" % i))
            runs.append((z["before"], z["after"], z["hist"], z["plain"], [str(s) for s in z["labels"]]))
    return runs


BIG = list(range(len(bt.TILED_BIG)))
BIG_IDS = [c.id for c in bt.TILED_BIG]


@pytest.mark.parametrize("i", BIG, ids=BIG_IDS)
def test_tiled_big(big_truth, big_product, i):
    """the shrunk up-pass of the product library: k_blur_up_poly<DUAL, TAIL 0> on a rectangle with a first tile other than (0, 0)
    (3232 x 3312), k_blur_hv/16 where the whole level would take the polyphase kernel (2432 x 2672), the 32-row k_blur_hv on a
    rectangle (shader order), k_blur_up_poly<TAIL 2> with a merge rectangle at every one"""
    check(bt.TILED_BIG[i], big_product(i), *big_truth(bt.TILED_BIG[i])[2:])


@pytest.mark.parametrize("i", BIG, ids=BIG_IDS)
def test_tiled_big_with_the_whole_up_pass(big_truth, big_whole, i):
    check(bt.TILED_BIG[i], big_whole[i], *big_truth(bt.TILED_BIG[i])[2:], shrink=False)


@pytest.mark.parametrize("i", BIG, ids=BIG_IDS)
def test_shrunk_and_whole_up_pass_agree_where_they_run_the_same_kernels(big_truth, big_product, big_whole, i):
    """Whole tiles are computed either way, so a texel is the same function of the same inputs wherever both runs give every level
    the same kernel: equal bits, histogram included.  Where the choice differs (2432 x 2672: level 1 is k_blur_hv/16 on the
    rectangle and k_blur_up_poly on the whole level) the two may differ — only at texels where the chain interval is not
    degenerate, and both inside it (which the two tests above assert)."""
    case = bt.TILED_BIG[i]
    lo, hi = big_truth(case)[2:]
    (hx, hy, hw, hh), (mx, my, mw, mh) = case.hdr_rect, case.merge_rect
    a, b = big_product(i), big_whole[i]
    same = [k[1] for k in bt.tiled_kernels(case.merge_rect, case.ew, case.eh, case.shader_order)] == \
           [k[1] for k in bt.tiled_kernels(case.merge_rect, case.ew, case.eh, case.shader_order, shrink=False)]
    assert same == (i != 0)                                                     # the table of the case set: row 1 alone differs
    differ = a[1][:, :hw] != b[1][:, :hw]
    if same:
        assert not differ.any() and np.array_equal(a[2], b[2]), f"{int(differ.sum())} values differ between the shrunk and the whole up-pass"
    else:
        inside = differ[my - hy:my - hy + mh, mx - hx:mx - hx + mw]
        assert int(inside.sum()) == int(differ.sum())
        assert (bt.half_width(lo, hi)[inside] > 0).all(), "the two up-passes differ where the truth leaves no freedom"
        d = common.half_ulp_diff(a[1].view(np.float16), b[1].view(np.float16))
        print(f"{case.id}: {int(differ.sum())} of {inside.size} values differ between the shrunk and the whole up-pass (at most {int(d[:, :hw][differ].max()) if differ.any() else 0} "
              f"half steps), all where the interval is not degenerate; histograms {'equal' if np.array_equal(a[2], b[2]) else 'differ'}")


# ------------------------------------------------------------------------------------------------------ the launch log itself
def test_launch_log_keeps_the_last_64_labels_in_order(ctx):
    """pbr_launch_log: the count runs on, the ring keeps the last 64 labels oldest first, a smaller cap gives the newest ones"""
    w, h = 8, 4
    hdr, src = (Plane(ctx, POISONS[0], bt.plane("smooth", w, h, seed=s)) for s in (3, 4))
    out = Plane(ctx, POISONS[0], texels=w * h)
    start = ctx.launch_log(0)[0]
    for _ in range(70):
        ctx.bloom_merge(hdr.ptr, w, src.ptr, w, h)
    ctx.blur_v(src.ptr, w, h, out.ptr, w, h)
    ctx.sync()
    total, labels = ctx.launch_log()
    assert total == start + 71 and labels == ["k_bloom_merge"] * 63 + ["k_blur_v"]
    assert ctx.launch_log(2) == (total, ["k_bloom_merge", "k_blur_v"]) and ctx.launch_log(0) == (total, [])
    assert ctx.launches_of(lambda: ctx.blur_v(src.ptr, w, h, out.ptr, w, h)) == ["k_blur_v"]
