"""Instruction-class counts of k_deferred_shade<true, 257, false, NoViews> (the 4K / 256-light instantiation) from the compiler's
gfx950 ISA.  No GPU needed.
    python tools/isa_phase_count.py [out.md] [--phases] [--fold | --tabled] [--prologue] [--src shade.hip]
--prologue adds the prologue rows (below) to the report of the sampled or the folded kernel.
--tabled measures k_deferred_shade_tabled<257> (pbr_deferred_shade with tables: the folded-LUT kernel with its prologue read from the shade tables).
--fold measures k_deferred_shade<true, 257, false, NoViews, true>, the instantiation that reads the LUT from its x-folded table
(pbr_deferred_shade with lut_fold), and adds the static v_* count of its LUT phase (the kernel minus its -DPBR_EXP_NOLUT build).
Reported:
  * the kernel's footer: occupancy, scratch bytes per lane, VGPRs;
  * every light-walk loop (innermost loops that carry the per-light arithmetic): v_* per TRIP (a trip = one pair of lights = four
    transcendentals, so an unrolled body is divided by transcendentals / 4), of them packed and transcendental;
  * the pixel-row body (the loop over a block's rows that encloses the walks): its static v_* count minus the walk loops and minus
    the rare exact-slice path (sized with -DPBR_EXP_NOEXACT), and from it the executed VALU instructions per pixel row at 16 trips
    of the as-shipped walk (the cheapest instantiation: attenuation floor hoisted, rough wave, one polynomial).  Every walk
    instantiation's few instructions outside its loop are in the static count although one runs: an upper bound, alike on both
    sides of a comparison;
  * the prologue: the v_* and s_barrier the kernel holds outside the row loop (static; what a block runs once, before it);
  * with --phases, per-phase counts: shade.hip compiled once per PBR_EXP_* switch that removes one phase of shade_pixel; the
    difference of the kernels' static v_* counts is that phase.
Only instruction CLASSES are counted (v_*, v_pk_*, the transcendental unit's, moves, ds_*, global_*, s_waitcnt, s_barrier, other s_*).
    python tools/isa_phase_count.py --bloom parent_bloom.hip [out.md] [--src gbuffer_raster.hip] [--flags "-ffp-contract=off"] [--also-with PBR_DEBUG_KNOBS]
compares every kernel instantiation of a translation unit (bloom.hip unless --src names another; --flags: what the Makefile adds for
it, bloom.hip's by default) with those of another copy of the source, which includes the headers that lie beside it (see bloom_report
below); --also-with adds the same table for the build with that macro defined.
    python tools/isa_phase_count.py --shade parent_shade.hip [out.md]
the same for shade.hip, product and knobs build (shade_report below)."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "direct12pbrrenderer_amd", "csrc")
SRC = os.path.join(CSRC, "shade.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# k_deferred_shade<true, 257, false, ...>: the template-argument prefix of the mangled name; the last argument (the view table's
# type) and the parameter list follow it
PREFIX = "_Z16k_deferred_shadeILb1ELi257ELb0E"
VIEWS = "NoViews"
FOLD_ARG = {False: "NoViewsELb0E", True: "NoViewsELb1E"}   # ... NoViews, LUTFOLD>: the sampled-LUT and the folded-LUT instantiation
TABLED_PREFIX = "_Z23k_deferred_shade_tabledILi257EE"   # k_deferred_shade_tabled<257>
TRIPS = 16   # pairs of lights of a capped (32-entry) list


def compile_isa(defines=(), src=SRC, flags=()):
    """flags: what the Makefile adds for this translation unit (bloom.hip: -ffp-contract=off)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-Wno-unused-function", "-Wno-unused-variable",
               "-Wno-unused-but-set-variable", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, src, "-o", os.path.join(d, "shade.s")] + ["-D" + x for x in defines] + list(flags)
        subprocess.run(cmd, check=True, capture_output=True)
        return open(os.path.join(d, "shade.s")).read()


def kernel(text, prefix=PREFIX, views=VIEWS, fold=False):
    """(mangled name, code lines, footer {Occupancy, ScratchSize, NumVgprs, TotalNumSgprs, LDSByteSize}) of the instantiation whose
    name starts with prefix (fold: the folded-LUT one; a source from before that template argument has only the sampled one)"""
    names = [m.group(1) for m in re.finditer(r"^(" + re.escape(prefix) + r"\w*):", text, re.M)]
    if fold and not any(FOLD_ARG[True] in n for n in names):
        raise SystemExit(f"no folded-LUT instantiation of {prefix}* in the ISA")
    names = [n for n in names if n == prefix] or [n for n in names if FOLD_ARG[fold] in n] or [n for n in names if views in n] or names
    if not names:
        raise SystemExit(f"no kernel named {prefix}* in the ISA")
    name = names[0]
    a = text.index(name + ":")
    b = text.index(".end_amdhsa_kernel", a)
    code = text[a:text.index(".amdhsa_kernel", a)].splitlines()
    info = text.index("; Kernel info:", b)
    foot = {k: int(v) for k, v in re.findall(r"^; (Occupancy|ScratchSize|NumVgprs|TotalNumSgprs|LDSByteSize): (\d+)", text[info:info + 1000], re.M)[:5]}
    return name, code, foot


def count(lines):
    ops = [ln.split()[0] for ln in lines if re.match(r"\s+[a-z]", ln)]
    valu = [o for o in ops if o.startswith("v_")]
    return {"valu": len(valu), "trans": sum(1 for v in valu if re.match(r"v_(rcp|rsq|log|exp|sqrt|sin|cos)_", v)),
            "packed": sum(1 for v in valu if v.startswith("v_pk_")), "moves": sum(1 for v in valu if v.startswith("v_mov_") or v.startswith("v_pk_mov")),
            "ds": sum(1 for o in ops if o.startswith("ds_")), "global": sum(1 for o in ops if o.startswith("global_")),
            "waitcnt": ops.count("s_waitcnt"), "barrier": ops.count("s_barrier"),
            "salu": sum(1 for o in ops if o.startswith("s_") and o not in ("s_waitcnt", "s_barrier"))}


def blocks(lines):
    """basic blocks of a kernel: (label, the compiler's loop annotation of the block, its lines)"""
    out = []
    for ln in lines:
        m = re.match(r"(?:\.L|; %)(BB\d+_\d+|bb\.\d+):\s*(;.*)?$", ln)
        if m:
            out.append([m.group(1), m.group(2) or "", []])
        elif out and re.match(r"\s+;", ln) and not out[-1][2]:
            out[-1][1] += ln   # the annotation goes on over comment-only lines
        elif out:
            out[-1][2].append(ln)
    return out


def walks_and_row(lines):
    """From the compiler's loop annotations: the walk loops (innermost loops with the per-light arithmetic: >= 40 packed
    instructions), as (label, lines), and the lines of the row loop around them (its child loops included)."""
    bl = blocks(lines)
    heads = [(lb, len(re.findall(r"Child Loop", an))) for lb, an, _ in bl if "This Loop Header: Depth=1" in an]
    if not heads:
        return [], []
    row_head = max(heads, key=lambda h: h[1])[0]
    member = re.compile(r"(Header=|Parent Loop )" + row_head + r"\b")
    row, inner = [], {}
    for lb, an, body in bl:
        if lb == row_head or member.search(an):
            row += body
            m = re.search(r"Header=(BB\d+_\d+) Depth=2", an)
            own = lb if "This Inner Loop Header: Depth=2" in an else (m.group(1) if m else None)
            if own:
                inner.setdefault(own, []).extend(body)
    return [(lb, body) for lb, body in inner.items() if count(body)["packed"] >= 40], row


def prologue(lines):
    """instruction classes of what the kernel holds outside its row loop (the Depth=1 loop that encloses the walks): a block runs that once,
    before the loop — nothing but s_endpgm follows it"""
    whole, row = count(lines), count(walks_and_row(lines)[1])
    return {k: whole[k] - row[k] for k in whole}


def measure(src=SRC, fold=False, lut_phase=False, prefix=PREFIX):
    """lut_phase: also the static v_* of the LUT phase (one more compile, -DPBR_EXP_NOLUT); prefix: the kernel (TABLED_PREFIX: the tabled one)"""
    builds = [(), ("PBR_EXP_NOEXACT",)] + ([("PBR_EXP_NOLUT",)] if lut_phase else [])
    with ThreadPoolExecutor(len(builds)) as ex:
        shipped, noexact, *nolut = ex.map(lambda d: kernel(compile_isa(d, src), prefix, fold=fold), builds)
    name, code, foot = shipped
    walks, row = walks_and_row(code)
    if not walks or not row:
        raise SystemExit("no light walk / row loop found in " + name)
    res = {"name": name, "occupancy": foot["Occupancy"], "scratch": foot["ScratchSize"], "vgprs": foot["NumVgprs"], "kernel": count(code), "walks": []}
    for lb, body in walks:
        c = count(body)
        unroll = max(c["trans"] // 4, 1)
        res["walks"].append({"label": lb, "unroll": unroll, "body": c, "valu_per_trip": c["valu"] / unroll,
                             "packed_per_trip": c["packed"] / unroll, "trans_per_trip": c["trans"] / unroll})
    hot = min(res["walks"], key=lambda w: w["valu_per_trip"])
    in_walks = sum(w["body"]["valu"] for w in res["walks"])
    res["row_static"] = count(row)["valu"]
    # the exact-slice path: the row body of the build without it, walks taken out alike
    code_n = noexact[1]
    walks_n, row_n = walks_and_row(code_n)
    res["surround"] = count(row_n)["valu"] - sum(count(b)["valu"] for _, b in walks_n)
    res["exact_path"] = res["row_static"] - in_walks - res["surround"]
    res["hot_trip"] = hot["valu_per_trip"]
    res["row_executed"] = res["surround"] + TRIPS * hot["valu_per_trip"]
    pro = prologue(code)
    res["prologue"], res["prologue_barriers"] = pro["valu"], pro["barrier"]
    if nolut:
        res["lut_phase"] = res["kernel"]["valu"] - count(nolut[0][1])["valu"]
    return res


METRICS = [("occupancy", "occupancy (waves per SIMD)"), ("scratch", "scratch bytes per lane"), ("hot_trip", "v_* per trip, as-shipped walk"),
           ("surround", "v_* per pixel row around the walk (row body - walk loops - exact-slice path)"),
           ("row_executed", f"executed v_* per pixel row at {TRIPS} trips, as-shipped walk")]
LUT_METRIC = ("lut_phase", "v_* of the split-sum LUT phase (kernel - its PBR_EXP_NOLUT build, static)")
PROLOGUE_METRICS = [("prologue", "v_* of the prologue (the kernel outside its row loop, static)"), ("prologue_barriers", "s_barrier of the prologue")]


def report(res, with_prologue=False):
    k = res["kernel"]
    title = "k_deferred_shade_tabled<257>" if res["name"].startswith(TABLED_PREFIX) else "k_deferred_shade<true, 257, false, NoViews" + (", true" if FOLD_ARG[True] in res["name"] else "") + ">"
    doc = ["# " + title + ": instruction classes of the gfx950 ISA (static counts)", "", f"`{res['name']}`", "",
           f"whole kernel: {k['valu']} v_* ({k['packed']} packed, {k['trans']} transcendental, {k['moves']} moves), {k['ds']} ds_*, {k['global']} global_*; {res['vgprs']} VGPRs", "",
           "| metric | value |", "|---|---|"]
    doc += [f"| {text} | {res[key]:g} |" for key, text in METRICS + [LUT_METRIC] + (PROLOGUE_METRICS if with_prologue else []) if key in res]
    doc += ["", f"row body: {res['row_static']} v_* static, of them {sum(w['body']['valu'] for w in res['walks'])} in the walk loops and {res['exact_path']} on the exact-slice path", "",
            "light walks (one of them runs per pixel; a trip = one pair of lights):", "",
            "| loop | trips per body | v_* per trip | packed per trip | transcendental per trip | moves per body | ds_* per body |", "|---|---|---|---|---|---|---|"]
    for w in res["walks"]:
        doc.append(f"| {w['label']} | {w['unroll']} | {w['valu_per_trip']:g} | {w['packed_per_trip']:g} | {w['trans_per_trip']:g} | {w['body']['moves']} | {w['body']['ds']} |")
    return doc


def parse_metrics(md_text):
    """{metric key: value} of a report written by this tool"""
    by_text = {text: key for key, text in METRICS + [LUT_METRIC] + PROLOGUE_METRICS}
    out = {}
    for m in re.finditer(r"^\| (.+?) \| ([-0-9.e+]+) \|$", md_text, re.M):
        if m.group(1) in by_text:
            out[by_text[m.group(1)]] = float(m.group(2))
    return out


def phases(src=SRC, fold=False):
    variants = [("light walk (cluster index + every instantiation of the list walk + the sums' zeroing)", "PBR_EXP_NOLOOP"),
                ("IBL specular: reflection vector, cube face, two trilinear levels from the footprint layout, their lerps", "PBR_EXP_NOENV"),
                ("split-sum LUT fetch + bilinear", "PBR_EXP_NOLUT"), ("SH9 irradiance (EnvironmentDiffuse)", "PBR_EXP_NOSH"),
                ("all of the IBL specular term (env + LUT)", "PBR_EXP_NOIBL")]
    with ThreadPoolExecutor(3) as ex:
        cs = list(ex.map(lambda d: count(kernel(compile_isa(d, src), fold=fold)[1]), [()] + [(v[1],) for v in variants]))
    t = cs[0]
    doc = ["", "phases (static v_* of the whole kernel, every path):", "", "| phase removed (-D switch) | v_* removed | of them packed | transcendental | moves |", "|---|---|---|---|---|"]
    for (nm, d), c in zip(variants, cs[1:]):
        doc.append(f"| {nm} (`{d}`) | {t['valu'] - c['valu']} | {t['packed'] - c['packed']} | {t['trans'] - c['trans']} | {t['moves'] - c['moves']} |")
    return doc


# ---- bloom.hip, or the unit --src names: resources and instruction classes of EVERY kernel instantiation, for a change that must leave the
# generated code as it is (profiles/bloom_isa_resources.md, tests/test_bloom_isa_cpu.py; profiles/raster_isa_resources.md):
#   python tools/isa_phase_count.py --bloom parent_bloom.hip [out.md]
BLOOM_SRC = os.path.join(CSRC, "bloom.hip")
BLOOM_FLAGS = ("-ffp-contract=off",)   # the Makefile's flags of bloom.o
BLOOM_COLS = [("valu", "v_*"), ("ds", "ds_*"), ("global", "global_*"), ("waitcnt", "s_waitcnt"), ("barrier", "s_barrier"), ("salu", "other s_*"),
              ("vgprs", "VGPR"), ("sgprs", "SGPR"), ("lds", "LDS bytes"), ("scratch", "scratch"), ("occupancy", "occupancy")]


def kernel_table(text):
    """{mangled name: ({column: value}, the kernel's instructions with block labels renumbered)} of every kernel of the ISA"""
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\w+)", text, re.M):
        _, code, foot = kernel(text, name)
        row = {k: v for k, v in count(code).items() if k in dict(BLOOM_COLS)}
        row.update(vgprs=foot["NumVgprs"], sgprs=foot["TotalNumSgprs"], lds=foot["LDSByteSize"], scratch=foot["ScratchSize"], occupancy=foot["Occupancy"])
        out[name] = (row, [re.sub(r"BB\d+_", "BB_", ln) for ln in code if re.match(r"\s+[a-z]", ln)])
    return out


def exceeds(new, ref):
    """the columns in which `new` breaks the condition against `ref`: LDS and occupancy equal, scratch (none in bloom.hip; k_rs_setup's
    clip arrays in gbuffer_raster.hip), registers and the counts of v_*, ds_*, global_*, s_waitcnt and s_barrier no higher (scalar-ALU
    counts may move)"""
    return ([c for c in ("lds", "occupancy") if new[c] != ref[c]] +
            [c for c in ("scratch", "vgprs", "sgprs", "valu", "ds", "global", "waitcnt", "barrier") if new[c] > ref[c]])


def bloom_report(parent_src, new_src=BLOOM_SRC, flags=BLOOM_FLAGS, defines=()):
    with ThreadPoolExecutor(2) as ex:
        parent, new = ex.map(lambda s: kernel_table(compile_isa(defines, s, flags)), [parent_src, new_src])
    same = [n for n in new if n in parent and new[n][1] == parent[n][1]]
    unit = os.path.basename(new_src)
    doc = [f"# {unit}{''.join(' -D' + d for d in defines)}: every kernel instantiation of the gfx950 ISA, parent commit and this tree (static counts)", "",
           f"{len(new)} kernels, {len(same)} with the parent's instruction stream byte for byte (`same` below); " +
           f"kernels of the parent that are gone: {sorted(set(parent) - set(new)) or 'none'}", ""]
    if unit == "bloom.hip":
        doc += ["Mangled template arguments: `k_blur_hv<MODE (1 M_DOWN, 2 M_UP), DUAL, TAIL, TH, NT, views>`, `k_blur_up_poly<DUAL, TAIL, TH, views>`, " +
                "`Lb0E` / `Lb1E` = false / true, `LiNE` = N.", ""]
    doc += ["| kernel | side | " + " | ".join(t for _, t in BLOOM_COLS) + " | same |", "|---" * (len(BLOOM_COLS) + 3) + "|"]
    for n, (row, _) in new.items():
        for side, r in (("parent", parent.get(n, (None,))[0]), ("new", row)):
            if r:
                note = "yes" if n in same else ("no" if n in parent else "-")
                doc.append(f"| `{n}` | {side} | " + " | ".join(str(r[k]) for k, _ in BLOOM_COLS) + f" | {note} |")
    bad = {n: exceeds(new[n][0], parent[n][0]) for n in new if n in parent and exceeds(new[n][0], parent[n][0])}
    doc += ["", "condition (LDS and occupancy equal, scratch / VGPR / SGPR / v_* / ds_* / global_* / s_waitcnt / s_barrier no higher): " +
            ("held by every kernel" if not bad else f"BROKEN by {bad}")]
    return doc, bad


SHADE_BUILDS = ((), ("PBR_DEBUG_KNOBS",))   # the Makefile's shade.o and shade.k.o: no flags of the unit's own


def shade_report(parent_src):
    """bloom_report for shade.hip (profiles/shade_isa_resources.md, tests/test_shade_isa_resources_cpu.py): the product build's table,
    then the knobs build's"""
    doc, bad = [], {}
    for defines in SHADE_BUILDS:
        more, bad_more = bloom_report(parent_src, SRC, (), defines)
        doc += ([""] if doc else []) + more
        bad.update({n + "".join(" -D" + d for d in defines): c for n, c in bad_more.items()})
    return doc, bad


def parse_bloom_rows(md_text, side="new"):
    """{mangled name: {column: value}} of the `side` rows of a report written by bloom_report"""
    out = {}
    for m in re.finditer(r"^\| `(\w+)` \| " + side + r" \| (.+?) \| \S+ \|$", md_text, re.M):
        out[m.group(1)] = {k: int(v) for (k, _), v in zip(BLOOM_COLS, m.group(2).split(" | "))}
    return out


def main(argv):
    if "--shade" in argv:   # python tools/isa_phase_count.py --shade parent_shade.hip [out.md]
        rest = [a for a in argv if a != "--shade"]
        doc, bad = shade_report(rest[0])
        text = "\n".join(doc) + "\n"
        print(text)
        if len(rest) > 1:
            open(rest[1], "w").write(text)
        sys.exit(1 if bad else 0)
    if "--bloom" in argv:
        rest = [a for a in argv if a != "--bloom"]
        opt = {}
        for name in ("--src", "--flags", "--also-with"):
            if name in rest:
                k = rest.index(name)
                opt[name] = rest[k + 1]
                del rest[k:k + 2]
        src, flags = opt.get("--src", BLOOM_SRC), tuple(opt["--flags"].split()) if "--flags" in opt else BLOOM_FLAGS
        doc, bad = bloom_report(rest[0], src, flags)
        if "--also-with" in opt:
            more, bad_more = bloom_report(rest[0], src, flags, (opt["--also-with"],))
            doc, bad = doc + [""] + more, dict(bad, **{n + " -D" + opt["--also-with"]: c for n, c in bad_more.items()})
        text = "\n".join(doc) + "\n"
        print(text)
        if len(rest) > 1:
            open(rest[1], "w").write(text)
        sys.exit(1 if bad else 0)
    args = [a for a in argv if not a.startswith("--")]
    src = SRC
    if "--src" in argv:
        src = argv[argv.index("--src") + 1]
        args.remove(src)
    fold = "--fold" in argv
    if "--tabled" in argv:   # the tabled kernel, and the prologue of the folded one it replaces beside it
        with ThreadPoolExecutor(2) as ex:
            tabled, folded = ex.map(lambda a: measure(src, **a), [dict(prefix=TABLED_PREFIX), dict(fold=True)])
        doc = report(tabled, with_prologue=True)
        doc += ["", f"the untabled folded kernel `{folded['name']}`: prologue {folded['prologue']} v_*, {folded['prologue_barriers']} s_barrier"]
    else:
        doc = report(measure(src, fold=fold, lut_phase=fold), with_prologue="--prologue" in argv)
    if "--phases" in argv:
        doc += phases(src, fold)
    text = "\n".join(doc) + "\n"
    print(text)
    if args:
        open(args[0], "w").write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
