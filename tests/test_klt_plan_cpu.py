"""The trackers' launch plan (csrc/klt_plan.h) on the CPU: klt_plan() is a pure function of values, so which kernel form a call runs,
with how many waves per feature, how many features per workgroup and how much LDS is checked here without a device, through
host/build/klt_plan_cli.  Properties the kernels rely on over a grid of cases, and a handful of cases pinned to what the launchers
did before the plan existed (recorded from the parent commit's fill_klt_params + launchers, not from klt_plan)."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "klt_plan_cli")

BASIC, AFFINE, LSSD = 0, 1, 2
INVERSE, DIRECT, FAST, NEON = 0, 1, 2, 4
NOT_SET = -1
KB = 1024


def plan(cases):
    """cases: dicts with model, method, half (rows, cols), n and optionally max_extent, lum, tree, long_tail, waves, group, chunked, spill."""
    assert os.path.exists(EXE), "host layer not built (python -c 'import __graft_entry__ as g; g.build()')"
    lines = []
    for c in cases:
        lines.append(" ".join(str(v) for v in (
            c["model"], c["method"], c["half"][0], c["half"][1], c["n"], c.get("max_extent", 640), c.get("lum", 0), c.get("tree", 0), c.get("long_tail", 0),
            c.get("waves", NOT_SET), c.get("group", NOT_SET), c.get("chunked", NOT_SET), c.get("spill", NOT_SET))))
    r = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        d = {}
        for kv in line.split():
            k, v = kv.split("=")
            d[k] = int(v) if v.lstrip("-").isdigit() else v
        out.append(d)
    assert len(out) == len(cases)
    return out


HALVES = [(0, 0), (0, 1), (1, 1), (4, 4), (5, 5), (6, 6), (6, 5), (7, 7), (10, 10), (15, 15), (16, 16), (20, 20), (32, 32), (33, 33), (40, 40), (150, 150),
          (1023, 1023)]


def grid_cases():
    cases = []
    for model, method, lum, half, n, tree, long_tail in itertools.product((BASIC, AFFINE, LSSD), (INVERSE, DIRECT, FAST, NEON), (0, 1), HALVES,
                                                                           (1, 300, 512, 4096, 4097, 16000, 70000), (0, 1), (0, 1)):
        cases.append(dict(model=model, method=method, lum=lum, half=half, n=n, tree=tree, long_tail=long_tail))
    overrides = [dict(waves=w) for w in (1, 2, 3, 4)] + [dict(waves=1, group=g) for g in (1, 2, 3, 4)] + [dict(group=3), dict(chunked=0), dict(waves=1, chunked=0),
                 dict(spill=1), dict(spill=2), dict(spill=0), dict(max_extent=1 << 23), dict(max_extent=1 << 23, waves=1)]
    for ov, model, method, lum, half, n, tree in itertools.product(overrides, (BASIC, AFFINE, LSSD), (INVERSE, DIRECT, FAST), (0, 1),
                                                                   ((0, 0), (5, 5), (6, 6), (6, 5), (10, 10), (20, 20), (33, 33), (150, 150)), (1, 512, 4097, 70000), (0, 1)):
        cases.append(dict(model=model, method=method, lum=lum, half=half, n=n, tree=tree, **ov))
    return cases


def test_plan_properties_hold_over_the_case_grid():
    cases = grid_cases()
    plans = plan(cases)
    seen_forms = set()
    for c, p in zip(cases, plans):
        what = f"{c} -> {p}"
        assert p["rc"] == 0 and p["kernel"] == 1, what
        assert p["stable"] == 1, what  # the same plan when asked twice: no state
        # exactly one form, and the argument block's flags say the same
        assert p["form"] in ("pipelined", "one_wave_fast", "generic", "generic_spill"), what
        assert (p["pb_enabled"], p["fk_enabled"], p["spill"]) == (int(p["form"] == "pipelined"), int(p["form"] == "one_wave_fast"), int(p["form"] == "generic_spill")), what
        assert p["family"] == {"pipelined": "pipelined", "one_wave_fast": "fast", "generic": "generic", "generic_spill": "generic"}[p["form"]], what
        seen_forms.add((p["form"], p["lssd_chunked"], p["k_lum"]))
        waves, group = p["waves_per_feature"], p["features_per_group"]
        assert 1 <= waves <= 4 and 1 <= group <= 4, what
        assert p["lds_bytes"] <= 160 * KB, what
        if p["form"] == "one_wave_fast":
            assert p["lds_bytes"] <= 64 * KB and waves == 1 and p["group_lds_stride"] <= 40 * KB, what
        if waves > 1:
            assert group == 1, what
        if waves == 1 and group > 1:  # one-wave features share a workgroup: their carves tile its LDS
            assert p["group_lds_stride"] % 16 == 0 and group * p["group_lds_stride"] == p["lds_bytes"], what
        if p["form"] == "generic_spill":
            assert waves >= 2 and p["tree"] == 0 and p["lssd_chunked"] == 0 and p["spill_stride_floats"] > 0 and p["k_spill"] == 1, what
        else:
            assert p["spill_stride_floats"] == 0 and p["k_spill"] == 0, what
            assert p["tree"] == c.get("tree", 0), what
        if c.get("tree", 0):
            assert p["form"] != "one_wave_fast", what
        assert p["k_tree"] == p["tree"] and p["solo"] == int(waves == 1), what
        if c.get("max_extent", 640) >= 1 << 23:  # coordinates would not be exact in fp32: the generic kernel
            assert p["form"] in ("generic", "generic_spill"), what
        assert p["block"] == 64 * waves * group, what
        assert p["grid"] == (c["n"] + group - 1) // group, what
        assert p["quad_chain"] == int(c["n"] <= 4096) and p["long_tail"] == c.get("long_tail", 0), what
        if p["k_lum"]:
            assert p["lssd_chunked"] == 1 and c["lum"] == 1 and c["model"] == LSSD and p["P"] <= 512, what
        if c.get("spill", NOT_SET) == 2:
            assert (p["rwin_rows"], p["rwin_cols"], p["cwin_rows"], p["cwin_cols"]) == (1, 0, 1, 0), what
    # the grid walks every form, the chunked LSSD levels with and without luminance
    assert {f for f, _, _ in seen_forms} == {"pipelined", "one_wave_fast", "generic", "generic_spill"}
    assert ("generic", 1, 0) in seen_forms and ("generic", 1, 1) in seen_forms


def expect(p, **want):
    got = {k: p[k] for k in want}
    assert got == want, f"{p}"


def test_pinned_plans():
    """What the launchers did at the commit before the plan existed (its fill_klt_params + launch_variant / klt_fast_launch /
    klt_basic_pipelined_launch, run on the CPU with the kernel launch intercepted), for the cases DESIGN.md and the planner's
    comments name."""
    c = [
        dict(model=BASIC, method=FAST, half=(6, 6), n=2000),              # 0: the policy's one wave -> the one-wave fast kernel <BASIC, 6, 6>
        dict(model=BASIC, method=INVERSE, half=(6, 6), n=2000),           # 1: pipelined <6, 6>, two waves
        dict(model=BASIC, method=INVERSE, half=(6, 6), n=25000),          # 2: pipelined solo form, four features per workgroup
        dict(model=LSSD, method=FAST, half=(6, 6), n=10000, waves=1),     # 3: generic, chunked
        dict(model=LSSD, method=FAST, half=(6, 6), n=10000, waves=1, lum=1),      # 4: chunked with luminance
        dict(model=LSSD, method=FAST, half=(6, 6), n=10000, waves=1, chunked=0),  # 5: FTK_LSSD_CHUNKED=0
        dict(model=BASIC, method=FAST, half=(20, 20), n=300),             # 6: 41 x 41 still fits the generic kernel's LDS on four waves
        dict(model=BASIC, method=FAST, half=(31, 31), n=300),             # 7: 63 x 63 does not: spill
        dict(model=BASIC, method=INVERSE, half=(31, 31), n=300),          # 8: ... the pipelined kernel holds it
        dict(model=BASIC, method=INVERSE, half=(32, 32), n=300),          # 9: ... up to 64 rows
        dict(model=AFFINE, method=INVERSE, half=(17, 17), n=300),         # 10: 35 x 35 fits
        dict(model=AFFINE, method=INVERSE, half=(18, 18), n=300),         # 11: 37 x 37: spill
        dict(model=BASIC, method=FAST, half=(6, 6), n=300, spill=1),      # 12: forced
        dict(model=BASIC, method=FAST, half=(6, 6), n=300, spill=2),      # 13: forced, windows disabled
        dict(model=BASIC, method=FAST, half=(6, 6), n=2000, tree=1),      # 14: no one-wave fast kernel in the throughput mode
        dict(model=AFFINE, method=FAST, half=(6, 6), n=2000),             # 15: the policy's three waves: generic <6>
        dict(model=BASIC, method=INVERSE, half=(10, 10), n=2000, tree=1), # 16: pipelined <10, 10>, throughput mode
        dict(model=AFFINE, method=INVERSE, half=(6, 6), n=2000),          # 17: axis tables in the head of the product groups
    ]
    p = plan(c)
    expect(p[0], form="one_wave_fast", family="fast", half=6, grid=500, block=256, lds_bytes=35456, waves_per_feature=1, features_per_group=4, group_lds_stride=8864,
           px_floats=3, terms_floats=0, a0_floats=312)
    expect(p[1], form="pipelined", family="pipelined", half=6, solo=0, k_tree=0, grid=2000, block=128, lds_bytes=10992, waves_per_feature=2, features_per_group=1,
           group_lds_stride=0)
    expect(p[2], form="pipelined", half=6, solo=1, grid=6250, block=256, lds_bytes=37568, waves_per_feature=1, features_per_group=4, group_lds_stride=9392, quad_chain=0)
    expect(p[3], form="generic", half=6, solo=1, k_lum=0, lssd_chunked=1, grid=5000, block=128, lds_bytes=17568, features_per_group=2, group_lds_stride=8784, px_floats=6,
           terms_floats=612, a0_floats=0)
    expect(p[4], form="generic", half=6, solo=1, k_lum=1, lssd_chunked=1, grid=5000, block=128, lds_bytes=17568, px_floats=6, terms_floats=612, a0_floats=0)
    expect(p[5], form="generic", half=6, solo=1, k_lum=0, lssd_chunked=0, lds_bytes=23616, group_lds_stride=11808, px_floats=3, terms_floats=0, a0_floats=312)
    expect(p[6], form="generic", half=0, solo=0, grid=300, block=256, lds_bytes=74096, waves_per_feature=4, a0_floats=1852)
    expect(p[7], form="generic_spill", k_spill=1, block=256, lds_bytes=19472, waves_per_feature=4, spill_stride_floats=38220)
    expect(p[8], form="pipelined", half=0, lds_bytes=83728, waves_per_feature=4)
    expect(p[9], form="generic_spill", lds_bytes=20032, waves_per_feature=4, spill_stride_floats=40660)
    expect(p[10], form="generic", lds_bytes=152640, waves_per_feature=4, px_floats=4, terms_floats=30800, a0_floats=0)
    expect(p[11], form="generic_spill", k_spill=1, grid=300, block=256, lds_bytes=7488, waves_per_feature=4, px_floats=4, terms_floats=34400, a0_floats=1524,
           spill_stride_floats=42220)
    expect(p[12], form="generic_spill", block=192, lds_bytes=1728, waves_per_feature=3, spill_stride_floats=1888, rwin_rows=16, rwin_cols=16)
    expect(p[13], form="generic_spill", block=192, lds_bytes=416, waves_per_feature=3, spill_stride_floats=1888, rwin_rows=1, rwin_cols=0, cwin_rows=1, cwin_cols=0)
    expect(p[14], form="generic", half=0, k_tree=1, solo=0, block=192, lds_bytes=8992, waves_per_feature=3, tree=1)
    expect(p[15], form="generic", half=6, solo=0, block=192, lds_bytes=22368, waves_per_feature=3)
    expect(p[16], form="pipelined", half=10, k_tree=1, solo=0, block=128, lds_bytes=18352, waves_per_feature=2, tree=1)
    expect(p[17], form="generic", half=6, solo=0, block=192, lds_bytes=22528, px_floats=4, terms_floats=4400, a0_floats=0)
