"""The matchers' and the direct method's launch plans (csrc/match_plan.h) on the CPU: hamming_plan, cosine_plan and direct_plan are pure
functions of values, so which kernel, grid and workspace a call gets is checked here without a device, through
host/build/match_plan_cli.  Properties the kernels rely on over grids of cases, and cases pinned to what the entry points and launchers
did before the plans existed (recorded from the parent commit's decision code, extracted and run on the CPU, not from the plans)."""
import itertools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "feature_tracker_amd", "host", "build", "match_plan_cli")

NOT_SET = "-"
DIRECT, INVERSE, FAST = 1, 0, 2
MB = 1 << 20
HAMMING_FIELDS = ("n_ref", "n_cur", "n_words", "n_bits", "nearby", "keys_given", "small", "kernel")
COSINE_FIELDS = ("n_ref", "n_cur", "dim", "nearby", "aligned16", "small", "chunked", "splits")
DIRECT_FIELDS = ("n_problems", "max_features", "patch_rows", "patch_cols", "method", "tree", "spread_allowed", "resident", "capturing", "held", "spread",
                 "resident_cap", "poison", "min_terms")
DEFAULTS = dict(nearby=0, keys_given=0, small=NOT_SET, kernel=NOT_SET, aligned16=1, chunked=NOT_SET, splits=NOT_SET, method=DIRECT, tree=0, spread_allowed=1,
                resident=2048, capturing=0, held=0, spread=NOT_SET, resident_cap=NOT_SET, poison=NOT_SET, min_terms=NOT_SET)
FIELDS = dict(hamming=HAMMING_FIELDS, cosine=COSINE_FIELDS, direct=DIRECT_FIELDS)


def case_line(kind, c):
    return " ".join([kind] + [str(c.get(f, DEFAULTS.get(f))) for f in FIELDS[kind]])


def plan(kind, cases):
    assert os.path.exists(EXE), "host layer not built (python -c 'import __graft_entry__ as g; g.build()')"
    r = subprocess.run([EXE], input="\n".join(case_line(kind, c) for c in cases) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        d = {}
        for kv in line.split():
            k, v = kv.split("=")
            if re.fullmatch(r"\d+x\d+", v):  # a grid or block: x x y
                d[k] = tuple(int(t) for t in v.split("x"))
            else:
                d[k] = int(v) if v.lstrip("-").isdigit() else v
        out.append(d)
    assert len(out) == len(cases)
    return out


def cdiv(a, b):
    return -(-a // b)


# ---- Hamming matcher ----

def hamming_cases():
    cases = []
    for n_ref, n_cur, n_words, bits, nearby, keys in itertools.product((1, 300, 512, 513, 2000, 10000, 70000),
                                                                       (1, 63, 64, 300, 2047, 2048, 3000, 24576, 24577, 60000),
                                                                       (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 32), ("zero", "one", "full"), (0, 1), (0, 1)):
        n_bits = {"zero": 0, "one": 1, "full": 32 * n_words}[bits]
        cases.append(dict(n_ref=n_ref, n_cur=n_cur, n_words=n_words, n_bits=n_bits, nearby=nearby, keys_given=keys))
    for ov, n_ref, n_cur, n_words, nearby in itertools.product((dict(small=0), dict(small=1), dict(kernel=1), dict(kernel=0), dict(small=0, kernel=0)),
                                                               (1, 300, 2048, 2049, 10000), (300, 1536, 2048, 3000, 33554431, 33554432), (1, 3, 8, 16, 24), (0, 1)):
        cases.append(dict(n_ref=n_ref, n_cur=n_cur, n_words=n_words, n_bits=32 * n_words, nearby=nearby, **ov))
    return cases


def test_hamming_plan_properties():
    cases = hamming_cases()
    seen = set()
    for c, p in zip(cases, plan("hamming", cases)):
        what = f"{c} -> {p}"
        n_ref, n_cur, n_bits = c["n_ref"], c["n_cur"], c["n_bits"]
        nw = p["dev_words"]
        seen.add(p["form"])
        # the padded width: a supported width, or n_words itself above 16
        assert (nw in (1, 2, 4, 8, 16) and nw >= c["n_words"] and nw < 2 * c["n_words"]) if c["n_words"] <= 16 else nw == c["n_words"], what
        assert p["pad"] == int(nw != c["n_words"]) and p["keys_clean"] == 1 - c.get("keys_given", 0), what
        small_rule = (c.get("small") != 0 and nw <= 16 and n_bits > 0 and n_cur < 0xFFFFF and n_cur * nw <= 24576 and n_ref * n_cur * nw <= 32 * MB)
        assert (p["form"] == "small") == small_rule, what
        mfma_rule = n_bits > 0 and nw in (8, 16) and n_cur * nw * 4 < 2 ** 31 and c.get("kernel", NOT_SET) in (NOT_SET, 1)
        assert p["matrix_cores"] == int(mfma_rule), what
        if p["form"] == "matrix_cores":
            assert mfma_rule and p["cur_per_block"] % 32 == 0 and p["cur_per_block"] // 32 <= 1024, what
        elif p["form"] == "popcount":
            assert p["cur_per_block"] % 64 == 0, what
        if p["form"] in ("popcount", "plain", "generic"):
            assert not mfma_rule or p["form"] != "popcount", what
            assert p["cur_per_block"] % 64 == 0, what
        assert p["form"] == "generic" if nw > 16 else p["form"] != "generic", what
        assert (p["form"] == "plain") == (n_bits == 0 and nw <= 16), what
        # boxes: NearbyMatch, n_bits > 0, n_cur >= 2048 only; launched only by the popcount and matrix-core scans
        assert (p["n_boxes"] > 0) == (c.get("nearby", 0) == 1 and n_bits > 0 and n_cur >= 2048), what
        splits = cdiv(n_cur, p["cur_per_block"])
        if p["form"] == "small":
            assert p["scan_grid"] == (cdiv(n_ref, 4), 1) and p["scan_block"] == (256, 1) and p["box_grid"][0] == 0 and p["epilogue_grid"][0] == 0, what
            continue
        assert p["scan_grid"][1] == splits and splits * p["cur_per_block"] >= n_cur > (splits - 1) * p["cur_per_block"], what  # the splits cover every candidate
        rows_per_group = {"popcount": 512, "matrix_cores": 64, "plain": 256, "generic": 256}[p["form"]]
        assert p["scan_grid"][0] * rows_per_group >= n_ref > (p["scan_grid"][0] - 1) * rows_per_group, what
        assert p["scan_block"] == ((64, 1) if p["form"] == "matrix_cores" else (256, 1)), what
        assert p["epilogue_grid"] == (cdiv(n_ref, 256), 1), what
        if p["box_grid"][0]:
            assert p["form"] in ("popcount", "matrix_cores") and p["n_boxes"] == p["box_grid"][0] == cdiv(n_ref, 512) + splits, what
        else:
            assert p["n_boxes"] == 0 or p["form"] in ("plain", "generic"), what
    assert seen == {"small", "plain", "popcount", "matrix_cores", "generic"}


def expect(p, **want):
    got = {k: p[k] for k in want}
    assert got == want, f"{p}"


def test_hamming_pinned():
    c = [
        dict(n_ref=300, n_cur=300, n_words=8, n_bits=256),                          # 0: BRIEF-256, the reference's sizes: one launch
        dict(n_ref=300, n_cur=300, n_words=8, n_bits=256, small=0),                 # 1: FTK_MATCH_SMALL=0: the matrix-core scan
        dict(n_ref=300, n_cur=300, n_words=8, n_bits=256, small=0, kernel=0),       # 2: ... FTK_MATCH_KERNEL=scalar: popcount
        dict(n_ref=10000, n_cur=10000, n_words=8, n_bits=256, nearby=1),            # 3: matrix cores with boxes
        dict(n_ref=10000, n_cur=10000, n_words=4, n_bits=128, nearby=1),            # 4: popcount with boxes
        dict(n_ref=10000, n_cur=2047, n_words=4, n_bits=128, nearby=1),             # 5: one candidate short of boxes
        dict(n_ref=2048, n_cur=2048, n_words=8, n_bits=256),                        # 6: exactly kSmallMatchWork
        dict(n_ref=2049, n_cur=2048, n_words=8, n_bits=256),                        # 7: one row more
        dict(n_ref=1, n_cur=24576, n_words=1, n_bits=32),                           # 8: exactly kSmallMatchRowWork
        dict(n_ref=1, n_cur=24577, n_words=1, n_bits=32),                           # 9: one more
        dict(n_ref=300, n_cur=300, n_words=3, n_bits=96, small=0),                  # 10: padded to 4 words
        dict(n_ref=300, n_cur=300, n_words=24, n_bits=768),                         # 11: generic width
        dict(n_ref=300, n_cur=300, n_words=8, n_bits=0),                            # 12: plain scan
        dict(n_ref=1, n_cur=33554431, n_words=16, n_bits=512),                      # 13: the last 32-bit offset
        dict(n_ref=1, n_cur=33554432, n_words=16, n_bits=512),                      # 14: one beyond: popcount
        dict(n_ref=131072, n_cur=10000000, n_words=8, n_bits=256),                  # 15: the 1024-tile cap
        dict(n_ref=300, n_cur=300, n_words=8, n_bits=256, keys_given=1, small=0),   # 16: caller's keys
        dict(n_ref=10000, n_cur=2048, n_words=4, n_bits=128, nearby=1),             # 17: the first candidate count with boxes
        dict(n_ref=300, n_cur=300, n_words=8, n_bits=256, small=0, kernel=1),       # 18: FTK_MATCH_KERNEL=mfma
        dict(n_ref=300, n_cur=300, n_words=4, n_bits=128, small=0, kernel=1),       # 19: ... has no matrix-core scan at 4 words
    ]
    p = plan("hamming", c)
    expect(p[0], form="small", matrix_cores=1, cur_per_block=32, scan_grid=(75, 1), scan_block=(256, 1), box_grid=(0, 1), epilogue_grid=(0, 1))
    expect(p[1], form="matrix_cores", cur_per_block=32, scan_grid=(5, 10), scan_block=(64, 1), epilogue_grid=(2, 1))
    expect(p[2], form="popcount", matrix_cores=0, cur_per_block=64, scan_grid=(1, 5), scan_block=(256, 1))
    expect(p[3], form="matrix_cores", cur_per_block=800, n_boxes=33, box_grid=(33, 1), scan_grid=(157, 13), epilogue_grid=(40, 1))
    expect(p[4], form="popcount", cur_per_block=64, n_boxes=177, box_grid=(177, 1), scan_grid=(20, 157))
    expect(p[5], form="popcount", n_boxes=0, box_grid=(0, 1), cur_per_block=64, scan_grid=(20, 32))
    expect(p[6], form="small", scan_grid=(512, 1))
    expect(p[7], form="matrix_cores", cur_per_block=64, scan_grid=(33, 32))
    expect(p[8], form="small", scan_grid=(1, 1))
    expect(p[9], form="popcount", cur_per_block=64, scan_grid=(1, 385))
    expect(p[10], form="popcount", dev_words=4, pad=1, cur_per_block=64, scan_grid=(1, 5))
    expect(p[11], form="generic", dev_words=24, pad=0, matrix_cores=0, cur_per_block=64, scan_grid=(2, 5))
    expect(p[12], form="plain", matrix_cores=0, cur_per_block=64, scan_grid=(2, 5))
    expect(p[13], form="matrix_cores", cur_per_block=16384, scan_grid=(1, 2048))
    expect(p[14], form="popcount", matrix_cores=0, cur_per_block=8192, scan_grid=(1, 4096))
    expect(p[15], form="matrix_cores", cur_per_block=32768, scan_grid=(2048, 306))
    expect(p[16], form="matrix_cores", keys_clean=0)
    expect(p[17], form="popcount", cur_per_block=64, n_boxes=52, box_grid=(52, 1), scan_grid=(20, 32))
    expect(p[18], form="matrix_cores", matrix_cores=1, cur_per_block=32, scan_grid=(5, 10), scan_block=(64, 1))
    expect(p[19], form="popcount", matrix_cores=0, cur_per_block=64, scan_grid=(1, 5), scan_block=(256, 1))


# ---- cosine matcher ----

def cosine_cases():
    cases = []
    for n_ref, n_cur, dim, nearby, aligned in itertools.product((1, 300, 512, 513, 2000, 4096, 4097, 10000), (1, 64, 300, 384, 385, 2047, 2048, 2049, 5000, 20000),
                                                                (1, 63, 64, 100, 128, 192, 256, 257, 512, 4096), (0, 1), (0, 1)):
        cases.append(dict(n_ref=n_ref, n_cur=n_cur, dim=dim, nearby=nearby, aligned16=aligned))
    overrides = [dict(small=0), dict(small=1), dict(chunked=1), dict(chunked=0), dict(splits=1), dict(splits=7), dict(splits=1000), dict(splits=0),
                 dict(chunked=1, splits=3), dict(small=0, chunked=1)]
    for ov, n_ref, n_cur, dim, nearby in itertools.product(overrides, (1, 300, 2000, 10000), (64, 300, 2048, 5000), (64, 128, 200, 256, 512), (0, 1)):
        cases.append(dict(n_ref=n_ref, n_cur=n_cur, dim=dim, nearby=nearby, **ov))
    return cases


REGIONS = ("ref_h", "cur_h", "ref_norm", "cur_norm", "cur_bias", "cur_info", "tile_box", "ref_irregular", "row_max", "cand_count", "irregular_count", "cand",
           "cand_score", "irregular_list")


def region_bytes(p):
    nr, nc, d = p["n_ref_pad"], p["n_cur_pad"], p["dim_pad"]
    return dict(ref_h=2 * nr * d, cur_h=2 * nc * d, ref_norm=4 * nr, cur_norm=4 * nc, cur_bias=4 * nc, cur_info=16 * nc, tile_box=16 * (nc // 64 + 1),
                ref_irregular=nr, row_max=4 * nr, cand_count=4 * nr, irregular_count=4, cand=4 * nr * 64, cand_score=4 * nr * 64 if p["ref_stationary"] else 0,
                irregular_list=4 * 64)


COSINE_MARGIN = 0.00150000001  # 1.5e-3f as the CLI prints it (%.9g)


def cosine_margin(dim_pad):
    """kCosineMargin + kCosineMarginPerK * (dim_pad - 256) in fp32, as the CLI prints it."""
    import numpy as np
    return float("%.9g" % (np.float32(1.5e-3) + np.float32(1.75e-7) * np.float32(dim_pad - 256)))


def test_cosine_plan_properties():
    cases = cosine_cases()
    seen = set()
    for c, p in zip(cases, plan("cosine", cases)):
        what = f"{c} -> {p}"
        n_ref, n_cur, dim = c["n_ref"], c["n_cur"], c["dim"]
        seen.add(p["form"])
        assert p["dim_pad"] == cdiv(dim, 64) * 64, what
        rs = p["dim_pad"] <= 256 and c.get("chunked") != 1  # register-stationary exactly when dim_pad <= 256 and chunked is not forced
        assert p["ref_stationary"] == int(rs), what
        small_rule = c.get("small") != 0 and dim in (64, 128, 256) and n_ref <= 4096 and n_cur <= (2048 if c["nearby"] else 384)
        assert (p["form"] == "small") == small_rule, what
        if not small_rule:
            assert p["form"] == ("register_stationary" if rs else "chunked"), what
        cur_tile, row_group = (64, 512) if rs else (128, 128)
        assert p["n_ref_pad"] == cdiv(n_ref, row_group) * row_group and p["n_cur_pad"] == cdiv(n_cur, cur_tile) * cur_tile, what
        tiles = p["n_cur_pad"] // cur_tile
        assert 1 <= p["splits"] <= tiles and p["tiles_per_split"] == cdiv(tiles, p["splits"]), what
        if rs and c.get("splits", NOT_SET) == NOT_SET and tiles >= 2:
            assert p["tiles_per_split"] >= 2, what
        # the workspace: regions 256-byte aligned, in order, not overlapping, inside the total
        sizes = region_bytes(p)
        used = [r for r in REGIONS if sizes[r] > 0]
        assert p["ref_h"] == 0 and all(p[r] % 256 == 0 for r in used), what
        for a, b in zip(used, used[1:]):
            assert p[a] + sizes[a] <= p[b], what
        assert p[used[-1]] + sizes[used[-1]] <= p["ws_bytes"], what
        # the clear range is exactly row_max | cand_count | irregular_count
        assert p["cand_count"] == p["row_max"] + cdiv(sizes["row_max"], 256) * 256 and p["irregular_count"] == p["cand_count"] + cdiv(sizes["cand_count"], 256) * 256, what
        assert p["clear_end"] == p["irregular_count"] + 256, what
        assert p["use_tile_box"] == int(c["nearby"] == 1 and p["n_cur_pad"] // 64 >= 32), what
        # the shortlist margin: today's constant wherever the register-stationary kernel (which compiles it in) can run, growing with
        # dim_pad beyond, whatever the form, the sizes and the switches
        assert float(p["margin"]) == (COSINE_MARGIN if p["dim_pad"] <= 256 else cosine_margin(p["dim_pad"])), what
        if p["form"] == "small":
            assert p["grid"] == (cdiv(n_ref, 4), 1) and p["block"] == (256, 1) and p["lds"] == 0, what
            assert p["prep_grid"][0] == p["box_grid"][0] == p["recheck_grid"][0] == 0, what
            continue
        assert p["packet_prep"] == int(dim % 8 == 0 and c.get("aligned16", 1) == 1), what
        assert p["recheck_grid"] == (cdiv(n_ref * 8, 256), 1) and p["prep_grid"][1] == 2, what
        if rs:
            assert p["grid"] == (p["n_ref_pad"] // 512 * p["splits"], 1) and p["block"] == (512, 1) and p["lds"] > 0, what
            assert p["box_grid"][0] == (p["n_cur_pad"] // 64 if p["use_tile_box"] and not p["packet_prep"] else 0), what
        else:
            assert p["grid"] == (p["n_ref_pad"] // 128, cdiv(tiles, p["tiles_per_split"])) and p["block"] == (256, 1) and p["lds"] == 0, what
            assert p["box_grid"][0] == 0, what
    assert seen == {"small", "register_stationary", "chunked"}


def test_cosine_pinned():
    c = [
        dict(n_ref=300, n_cur=300, dim=256, nearby=1),               # 0: one launch
        dict(n_ref=300, n_cur=300, dim=256, nearby=0),               # 1: ForceMatch within its 384 candidates
        dict(n_ref=300, n_cur=385, dim=256, nearby=0),               # 2: one candidate beyond the ForceMatch bound
        dict(n_ref=300, n_cur=2049, dim=128, nearby=1),              # 3: beyond the NearbyMatch bound, tile boxes
        dict(n_ref=4097, n_cur=300, dim=128, nearby=1),              # 4: beyond kCosineSmallRefMax
        dict(n_ref=2000, n_cur=2000, dim=256, small=0),              # 5: FTK_COSINE_SMALL=0: register-stationary
        dict(n_ref=2000, n_cur=2000, dim=256, small=0, aligned16=0), # 6: misaligned: the octet prep
        dict(n_ref=2000, n_cur=2000, dim=256, small=0, nearby=1, aligned16=0),  # 7: ... and the tile-box launch
        dict(n_ref=2000, n_cur=2000, dim=256, chunked=1),            # 8: FTK_COSINE_CHUNKED=1
        dict(n_ref=2000, n_cur=2000, dim=512),                       # 9: dim_pad > 256: chunked
        dict(n_ref=2000, n_cur=2000, dim=256, splits=7),             # 10: FTK_COSINE_SPLITS
        dict(n_ref=2000, n_cur=2000, dim=100),                       # 11: odd width
        dict(n_ref=2000, n_cur=2000, dim=256),                       # 12: the widest register-stationary descriptor
        dict(n_ref=2000, n_cur=2000, dim=257),                       # 13: one more: chunked
    ]
    p = plan("cosine", c)
    expect(p[0], form="small", grid=(75, 1), block=(256, 1), ws_bytes=703232)
    expect(p[1], form="small", grid=(75, 1))
    expect(p[2], form="register_stationary", splits=3, tiles_per_split=3, n_cur_pad=448, grid=(3, 1), block=(512, 1), lds=80032, packet_prep=1, prep_grid=(4, 2),
           recheck_grid=(10, 1))
    expect(p[3], form="register_stationary", use_tile_box=1, box_grid=(0, 1), splits=16, tiles_per_split=3, grid=(16, 1))
    expect(p[4], form="register_stationary", n_ref_pad=4608, splits=2, grid=(18, 1))
    expect(p[5], form="register_stationary", splits=16, tiles_per_split=2, grid=(64, 1), row_max=2157312, clear_end=2173952, cand=2173952, cand_score=2698240,
           irregular_list=3222528, ws_bytes=3222784)
    expect(p[6], form="register_stationary", packet_prep=0, prep_grid=(64, 2))
    expect(p[7], form="register_stationary", use_tile_box=1, box_grid=(32, 1))
    expect(p[8], form="chunked", ref_stationary=0, n_ref_pad=2048, n_cur_pad=2048, splits=16, tiles_per_split=1, grid=(16, 16), block=(256, 1), lds=0, cand_score=0)
    expect(p[9], form="chunked", dim_pad=512, splits=16, grid=(16, 16))
    expect(p[10], form="register_stationary", splits=7, tiles_per_split=5, grid=(28, 1))
    expect(p[11], form="register_stationary", dim_pad=128, packet_prep=0)
    expect(p[12], form="register_stationary", ref_stationary=1, dim_pad=256, splits=16, tiles_per_split=2, grid=(64, 1), block=(512, 1), lds=80032)
    expect(p[13], form="chunked", ref_stationary=0, dim_pad=320, splits=16, tiles_per_split=1, grid=(16, 16), block=(256, 1), lds=0)
    # the margin: 1.5e-3 up to dim_pad 256 (also under the chunked pair, case 8), 1.75e-7 more per component beyond
    assert [q["margin"] for k, q in enumerate(p) if k not in (9, 13)] == ["0.00150000001"] * 12
    assert abs(float(p[9]["margin"]) - (1.5e-3 + 256 * 1.75e-7)) < 1e-9 and abs(float(p[13]["margin"]) - (1.5e-3 + 64 * 1.75e-7)) < 1e-9


# ---- direct method ----

def direct_cases():
    cases = []
    for n, feats, patch, method, tree, allowed, resident, capturing, held in itertools.product(
            (1, 2, 6, 7, 74, 75, 112, 113), (0, 1, 100, 300, 768, 769, 2000), (1, 3, 13, 127), (INVERSE, DIRECT, FAST), (0, 1), (0, 1), (0, 32, 256),
            (0, 1), (0, 1 << 40)):
        cases.append(dict(n_problems=n, max_features=feats, patch_rows=patch, patch_cols=patch, method=method, tree=tree, spread_allowed=allowed,
                          resident=resident, capturing=capturing, held=held))
    overrides = [dict(spread=0), dict(spread=1), dict(spread=2), dict(spread=8), dict(spread=300), dict(spread=-1), dict(resident_cap=16), dict(resident_cap=40),
                 dict(poison=1), dict(poison=0), dict(min_terms=0), dict(min_terms=1), dict(min_terms=1 << 31), dict(spread=1, resident_cap=6)]
    for ov, n, feats, patch, capturing in itertools.product(overrides, (1, 2, 6, 75, 112), (1, 300, 768), (1, 13, 127), (0, 1)):
        cases.append(dict(n_problems=n, max_features=feats, patch_rows=patch, patch_cols=patch, capturing=capturing, **ov))
    return cases


def test_direct_plan_properties():
    cases = direct_cases()
    spreads = 0
    for c, p in zip(cases, plan("direct", cases)):
        what = f"{c} -> {p}"
        d = dict(DEFAULTS, **c)
        n, feats = d["n_problems"], d["max_features"]
        assert p["ask_resident"] == 0 and p["ask_capturing"] == 0, what  # every input known
        assert p["feat_in_global"] == int(feats > 768) and p["feat_bytes"] == (cdiv(64 * feats, 256) * 256 if feats > 768 else 0), what
        assert p["poison"] == int(d["poison"] not in (NOT_SET, 0)), what
        assert p["block"] == (512, 1), what
        if p["producers"] == 0:
            assert p["grid"] == (n, 1) and p["ws_stride"] == 0 and p["clear_bytes"] == 0, what
            continue
        spreads += 1
        terms = feats * d["patch_rows"] * d["patch_cols"]
        min_terms = 64 * 256 if d["min_terms"] == NOT_SET else d["min_terms"]
        # a spread only under today's conditions
        assert d["method"] == DIRECT and d["tree"] == 0 and d["spread_allowed"] == 1 and feats <= 768 and n <= 112, what
        assert min_terms <= terms < 2 ** 31, what
        resident = d["resident"] if d["resident_cap"] == NOT_SET else min(d["resident"], d["resident_cap"])
        usable = resident - resident // 8
        fit = usable // n - 1
        assert p["producers"] >= 2 or (d["spread"] != NOT_SET and p["producers"] == min(d["spread"], fit) >= 1), what
        assert p["producers"] <= (32 if d["spread"] == NOT_SET else min(d["spread"], 200)), what
        assert n * (1 + p["producers"]) <= usable and p["grid"] == (n * (1 + p["producers"]), 1), what
        assert p["ws_stride"] % 256 == 0 and p["ws_stride"] * n <= 512 * MB and 0 < p["clear_bytes"] <= p["ws_stride"], what
        assert not (d["capturing"] and p["ws_stride"] * n > d["held"]), what  # no growth while capturing
    assert spreads > 100


def test_direct_plan_asks_only_when_it_decides():
    base = dict(n_problems=1, max_features=300, patch_rows=13, patch_cols=13)
    p = plan("direct", [dict(base, resident=NOT_SET, capturing=NOT_SET), dict(base, resident=2048, capturing=NOT_SET),
                        dict(base, resident=2048, capturing=NOT_SET, held=1 << 40), dict(base, method=FAST, resident=NOT_SET, capturing=NOT_SET),
                        dict(base, spread_allowed=0, resident=NOT_SET, capturing=NOT_SET), dict(base, spread=0, resident=NOT_SET, capturing=NOT_SET)])
    expect(p[0], ask_resident=1, ask_capturing=0)
    expect(p[1], ask_resident=0, ask_capturing=1)
    expect(p[2], ask_resident=0, ask_capturing=0, producers=32)
    for q in p[3:]:
        expect(q, ask_resident=0, ask_capturing=0, producers=0)


def test_direct_pinned():
    c = [
        dict(n_problems=1, max_features=300, patch_rows=13, patch_cols=13),                     # 0: one problem spread, 32 producers
        dict(n_problems=1, max_features=300, patch_rows=13, patch_cols=13, spread_allowed=0),   # 1: the re-run of a poisoned launch
        dict(n_problems=6, max_features=300, patch_rows=13, patch_cols=13, resident=256),       # 2: 256 resident: 36 fit a problem
        dict(n_problems=75, max_features=300, patch_rows=13, patch_cols=13, resident=256),      # 3: two producers no longer fit
        dict(n_problems=74, max_features=300, patch_rows=13, patch_cols=13, resident=256),      # 4: ... they still do
        dict(n_problems=113, max_features=300, patch_rows=13, patch_cols=13),                   # 5: beyond kDirectSpreadMaxProblems
        dict(n_problems=1, max_features=300, patch_rows=13, patch_cols=13, tree=1),             # 6: throughput mode
        dict(n_problems=1, max_features=769, patch_rows=13, patch_cols=13),                     # 7: features in device memory
        dict(n_problems=1, max_features=96, patch_rows=13, patch_cols=13),                      # 8: below the 16 384 terms
        dict(n_problems=1, max_features=96, patch_rows=13, patch_cols=13, min_terms=0),         # 9: FTK_DIRECT_SPREAD_MIN_TERMS=0
        dict(n_problems=1, max_features=300, patch_rows=13, patch_cols=13, spread=1),           # 10: FTK_DIRECT_SPREAD=1 is honoured
        dict(n_problems=1, max_features=300, patch_rows=13, patch_cols=13, spread=0),           # 11: FTK_DIRECT_SPREAD=0
        dict(n_problems=2, max_features=300, patch_rows=13, patch_cols=13, resident_cap=4),     # 12: FTK_DIRECT_SPREAD_RESIDENT=4: one producer fits
        dict(n_problems=2, max_features=300, patch_rows=13, patch_cols=13, resident_cap=4, spread=1),  # 13: ... asked for: honoured
        dict(n_problems=1, max_features=300, patch_rows=13, patch_cols=13, capturing=1),        # 14: growth while capturing
        dict(n_problems=1, max_features=300, patch_rows=13, patch_cols=13, capturing=1, held=1 << 30),  # 15: ... no growth
        dict(n_problems=2, max_features=768, patch_rows=127, patch_cols=127),                   # 16: beyond 512 MB
        dict(n_problems=1, max_features=300, patch_rows=13, patch_cols=13, poison=1),           # 17: FTK_DIRECT_SPREAD_POISON=1
        dict(n_problems=112, max_features=300, patch_rows=13, patch_cols=13, resident=4096),    # 18: kDirectSpreadMaxProblems, where two producers fit
        dict(n_problems=113, max_features=300, patch_rows=13, patch_cols=13, resident=4096),    # 19: one more
        dict(n_problems=1, max_features=768, patch_rows=13, patch_cols=13),                     # 20: the last feature count in LDS
    ]
    p = plan("direct", c)
    expect(p[0], producers=32, grid=(33, 1), ws_stride=1424640, clear_bytes=3584, lds=122400)
    expect(p[1], producers=0, grid=(1, 1), lds=122400)
    expect(p[2], producers=32, grid=(198, 1))
    expect(p[3], producers=0, grid=(75, 1))
    expect(p[4], producers=2, grid=(222, 1))
    expect(p[5], producers=0, grid=(113, 1))
    expect(p[6], producers=0)
    expect(p[7], producers=0, feat_in_global=1, feat_bytes=49408, lds=103200)
    expect(p[8], producers=0)
    expect(p[9], producers=32, grid=(33, 1), ws_stride=456448, clear_bytes=1280)
    expect(p[10], producers=1, grid=(2, 1))
    expect(p[11], producers=0)
    expect(p[12], producers=0, grid=(2, 1))
    expect(p[13], producers=1, grid=(4, 1))
    expect(p[14], producers=0, grid=(1, 1))
    expect(p[15], producers=32, grid=(33, 1))
    expect(p[16], producers=0, grid=(2, 1))
    expect(p[17], producers=32, poison=1)
    expect(p[18], producers=31, grid=(3584, 1))
    expect(p[19], producers=0, grid=(113, 1))
    expect(p[20], producers=32, grid=(33, 1), feat_in_global=0, lds=152352)
