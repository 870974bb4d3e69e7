"""The host's route decision (csrc/kad_route.h route_schedule / route_grids) through kad_route_eval: no GPU.

Every expected value below is written out from a reading of the launchers this decision replaced
(schedule_locked's flags, launch_prep, launch_schedule, launch_rows, launch_defer_pass), not computed by the
library: the kernel names per (chunks, snapshot class, score set), the LDS sizes from the layouts' byte
counts (a wide wave region is 5248 B, a lean one 768 / 1408 / 2048 / 2688 B at 1 / 2 / 3 / 4-or-dynamic
position groups), and the rules' asymmetries — the wide branch's may_defer ignores TW and snap_negative,
<16, 0, SM_LEAST> needs fold && fitfold while <8, 8, SM_DEFAULT> does not, and nine to twelve chunks
(C = 513 .. 768) have three prep lanes per unit, no power of two, so no early rows.

A relaxed snapshot reaches the decision as clean with fold and fitfold set (kad_api.hip res_clean admits it
only folded); strict ones are clean with any fold state; generic ones are not clean.
"""

import itertools

import pytest

from kubeadmiral_amd import build, runtime

TT, AFF, BAL, LEAST, MOST = 1, 4, 5, 6, 7  # KAD_PL_* ids of the score plugins (include/kad_sched.h)
SM_LEAST = 1 << LEAST                                                 # C2 / C3
SM_DEFAULT = (1 << TT) | (1 << BAL) | (1 << LEAST) | (1 << AFF)        # C4 / C5
SCORE_SETS = {"least": SM_LEAST, "default": SM_DEFAULT, "none": 0, "most_tt": (1 << MOST) | (1 << TT)}
FILTER_DEFAULT = 0b11111  # APIResources, TaintToleration, ClusterResourcesFit, PlacementFilter, ClusterAffinity

CS = (1, 64, 65, 256, 257, 449, 512, 513, 960, 961, 1024, 1025, 3136, 3137, 4096, 4097, 8192, 8193, 12288, 12289, 16384, 16385,
      32768, 32769, 65535)
# per C: chunks, prep kernel, prep_kernel lanes per unit (ceil(chunks / 4))
FACTS = {1: (1, "PREP", 1), 64: (1, "PREP", 1), 65: (2, "PREP", 1), 256: (4, "PREP", 1), 257: (5, "PREP", 2),
         449: (8, "PREP", 2), 512: (8, "PREP", 2), 513: (9, "PREP", 3), 960: (15, "PREP", 4), 961: (16, "PREP", 4),
         1024: (16, "PREP", 4), 1025: (17, "PREP", 5), 3136: (49, "PREP", 13), 3137: (50, "PREP", 13), 4096: (64, "PREP", 16), 4097: (65, "PREP_WAVE2", 17),
         8192: (128, "PREP_WAVE2", 32), 8193: (129, "PREP_WAVE3", 33), 12288: (192, "PREP_WAVE3", 48),
         12289: (193, "PREP_WAVE4", 49), 16384: (256, "PREP_WAVE4", 64), 16385: (257, "PREP", 65),
         32768: (512, "PREP", 128), 32769: (513, "PREP", 129), 65535: (1024, "PREP", 256)}
LEAN_WAVE_BYTES = {1: 768, 2: 1408, 3: 2048, 4: 2688}
N_CU, PER_CU, ROW_PER_CU = 256, 2, 2


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build()
    return runtime.load_library()


def expected(C, clean, fold, fitfold, TW, neg, W, cur, zero, bdefer, many, fmask, smask, dbg, side, no_inline):
    nch, prep, lanes = FACTS[C]
    e = {"prep": prep, "prep_lanes": lanes}
    wide = bool(clean) and 5 <= nch <= 16
    e["use_rows"] = int(clean and fold and fitfold and 1 <= C <= 12288)
    e["early_rows"] = int(e["use_rows"] and wide and lanes in (2, 4) and not dbg)
    e["cache_ne"] = int(bool(fmask & (1 << TT)) and cur)
    e["cache_pn"] = (smask >> TT) & 1
    e["row_variant"] = "ROW_DEFAULT" if smask == SM_DEFAULT else "ROW"
    # schedule_kernel's per-wave rows (20 B per padded cluster + 32 B per chunk + 128 + 1024, 16-B rounded) in 64 KB
    e["full_variant"] = "FULL_LDS" if C <= 3136 else "FULL_GSCR"  # 49 chunks: 65 440 B
    Cp = 64 * nch
    if wide:
        e["family"] = "WIDE"
        e["may_defer"] = int(bdefer or dbg or not e["early_rows"] or (many and bool(smask & (1 << AFF))))
        e["cache_zs"] = int(bool(smask & ((1 << LEAST) | (1 << MOST) | (1 << BAL))) and zero)
        e["wpb"], e["threads"], e["wave_bytes"] = 16, 1024, 5248
        e["lds"] = Cp * (56 + 8 * e["cache_ne"] + 8 * e["cache_pn"] + 4 * e["cache_zs"]) + 16 * 5248
        base = ("WIDE_LEAST" if fold and fitfold and nch == 16 and smask == SM_LEAST else
                "WIDE8_DEFAULT" if nch == 8 and smask == SM_DEFAULT else "WIDE")
        e["variant"] = base + ("_ZR" if e["cache_zs"] else "")
        # the row body's LDS (at most 21 104 B at 16 chunks) always fits below the 16 wave regions
        if e["early_rows"]:
            e["rows"] = "INLINE" if not no_inline else ("BESIDE" if side else "AFTER")
        else:
            e["rows"] = "AFTER" if e["use_rows"] else "NONE"
        e["defer_pass"] = e["may_defer"]
        grid = min(N_CU, -(-W // 16))
        if W:
            e["grid"], e["batch"] = grid, 3 if -(-W // (grid * 16)) < 64 else 4
    else:
        e["family"] = "LEAN"
        e["may_defer"] = int(bdefer or neg or TW > 1 or dbg)
        e["cache_zs"] = 0
        cl = bool(clean) and nch <= 4
        e["wpb"], e["threads"], e["wave_bytes"] = 4, 256, LEAN_WAVE_BYTES[nch if nch <= 4 else 4]
        e["lds"] = 4 * e["wave_bytes"] + (8 * Cp * (6 + e["cache_ne"] + e["cache_pn"] + cl) if nch <= 4 else 0)
        if nch <= 3:
            e["variant"] = f"LEAN{nch}" + ("_CLEAN" if cl else "")
        elif nch == 4:
            e["variant"] = ("LEAN4_CLEAN_LEAST" if smask == SM_LEAST else "LEAN4_CLEAN") if cl else "LEAN4"
        else:
            e["variant"] = "LEAN0_DEFAULT" if smask == SM_DEFAULT else "LEAN0"
        e["rows"] = "AFTER" if nch > 4 and e["use_rows"] else "NONE"
        e["defer_pass"] = int(nch > 4 or e["may_defer"])
        grid = min(N_CU * PER_CU, -(-W // 4))
        if W:
            e["grid"], e["batch"] = grid, min(4, max(1, -(-W // (grid * 4)) // 6))
    if W:
        e["row_grid"] = min(N_CU * ROW_PER_CU, 1024, W) if e["rows"] in ("AFTER", "BESIDE") else 0
    return e


def check_invariants(r):
    assert r["lds"] <= 160 * 1024 and r["wpb"] >= 1, r
    assert r["use_rows"] or not r["early_rows"], r
    assert r["rows"] != "INLINE" or r["wpb"] >= 2, r
    assert r["threads"] == 64 * r["wpb"], r


SNAPSHOTS = [(clean, fold, fitfold, neg) for clean, fold, fitfold in itertools.product((1, 0), repeat=3)
             for neg in ((0,) if clean else (0, 1))]


@pytest.mark.parametrize("C", CS)
def test_route_at_every_boundary(C):
    n = 0
    for (clean, fold, fitfold, neg), TW, (_, smask), zero, cur, dbg, side, no_inline, W in itertools.product(
            SNAPSHOTS, (1, 2), SCORE_SETS.items(), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (90, 125000)):
        if fitfold and C > 16384:
            continue  # FITFOLD_MAX_C: no such snapshot
        bdefer, many = (n >> 1) & 1, n & 1  # (the two batch facts alternate over the product)
        n += 1
        got = runtime.route_eval(PER_CU, ROW_PER_CU, C=C, clean=clean, fold=fold, fitfold=fitfold, TW=TW,
                                 snap_negative=neg, W=W, has_current=cur, zero_req=zero, batch_defer=bdefer,
                                 batch_many_terms=many, filter_mask=FILTER_DEFAULT, score_mask=smask, debug_capture=dbg,
                                 side_stream=side, rows_no_inline=no_inline, n_cu=N_CU)
        want = expected(C, clean, fold, fitfold, TW, neg, W, cur, zero, bdefer, many, FILTER_DEFAULT, smask, dbg, side,
                        no_inline)
        assert {k: got[k] for k in want} == want, (C, clean, fold, fitfold, neg, TW, smask, zero, cur, dbg, side,
                                                   no_inline, W)
        check_invariants(got)
    assert n > 0


# One row on each side of every boundary, every figure by hand from the parent's launchers: W = 125 000 units on
# 256 CUs, two lean (and row) blocks per CU, no CurrentClusters, requests present, TW = 1 unless said.
# (C, snapshot (clean, fold, fitfold), TW, score set) -> (variant, prep, defer-pass kernel, use_rows, early_rows,
#  may_defer, rows, defer_pass, waves per block, LDS bytes, batch, row grid)
F, G, U = (1, 1, 1), (0, 1, 1), (1, 0, 0)  # folded clean; generic; clean, nothing folded
LITERAL = {
    (1, F, 1, "default"): ("LEAN1_CLEAN", "PREP", "FULL_LDS", 1, 0, 0, "NONE", 0, 4, 7168, 4, 0),
    (64, F, 1, "default"): ("LEAN1_CLEAN", "PREP", "FULL_LDS", 1, 0, 0, "NONE", 0, 4, 7168, 4, 0),
    (65, F, 1, "default"): ("LEAN2_CLEAN", "PREP", "FULL_LDS", 1, 0, 0, "NONE", 0, 4, 13824, 4, 0),
    (256, F, 1, "default"): ("LEAN4_CLEAN", "PREP", "FULL_LDS", 1, 0, 0, "NONE", 0, 4, 27136, 4, 0),
    (256, F, 1, "least"): ("LEAN4_CLEAN_LEAST", "PREP", "FULL_LDS", 1, 0, 0, "NONE", 0, 4, 25088, 4, 0),
    (256, F, 2, "default"): ("LEAN4_CLEAN", "PREP", "FULL_LDS", 1, 0, 1, "NONE", 1, 4, 27136, 4, 0),
    (256, G, 1, "default"): ("LEAN4", "PREP", "FULL_LDS", 0, 0, 0, "NONE", 0, 4, 25088, 4, 0),
    (257, F, 1, "default"): ("WIDE", "PREP", "FULL_LDS", 1, 1, 0, "INLINE", 0, 16, 104448, 3, 0),
    (257, F, 2, "default"): ("WIDE", "PREP", "FULL_LDS", 1, 1, 0, "INLINE", 0, 16, 104448, 3, 0),
    (257, G, 1, "default"): ("LEAN0_DEFAULT", "PREP", "FULL_LDS", 0, 0, 0, "NONE", 1, 4, 10752, 4, 0),
    (449, F, 1, "default"): ("WIDE8_DEFAULT", "PREP", "FULL_LDS", 1, 1, 0, "INLINE", 0, 16, 116736, 3, 0),
    (449, U, 1, "default"): ("WIDE8_DEFAULT", "PREP", "FULL_LDS", 0, 0, 1, "NONE", 1, 16, 116736, 3, 0),
    (512, F, 1, "default"): ("WIDE8_DEFAULT", "PREP", "FULL_LDS", 1, 1, 0, "INLINE", 0, 16, 116736, 3, 0),
    (513, F, 1, "default"): ("WIDE", "PREP", "FULL_LDS", 1, 0, 1, "AFTER", 1, 16, 120832, 3, 512),
    (960, F, 1, "default"): ("WIDE", "PREP", "FULL_LDS", 1, 1, 0, "INLINE", 0, 16, 145408, 3, 0),
    (960, F, 1, "least"): ("WIDE", "PREP", "FULL_LDS", 1, 1, 0, "INLINE", 0, 16, 137728, 3, 0),
    (961, F, 1, "least"): ("WIDE_LEAST", "PREP", "FULL_LDS", 1, 1, 0, "INLINE", 0, 16, 141312, 3, 0),
    (961, U, 1, "least"): ("WIDE", "PREP", "FULL_LDS", 0, 0, 1, "NONE", 1, 16, 141312, 3, 0),
    (1024, F, 1, "least"): ("WIDE_LEAST", "PREP", "FULL_LDS", 1, 1, 0, "INLINE", 0, 16, 141312, 3, 0),
    (1024, F, 1, "default"): ("WIDE", "PREP", "FULL_LDS", 1, 1, 0, "INLINE", 0, 16, 149504, 3, 0),
    (1024, G, 1, "default"): ("LEAN0_DEFAULT", "PREP", "FULL_LDS", 0, 0, 0, "NONE", 1, 4, 10752, 4, 0),
    (1025, F, 1, "default"): ("LEAN0_DEFAULT", "PREP", "FULL_LDS", 1, 0, 0, "AFTER", 1, 4, 10752, 4, 512),
    (1025, F, 1, "least"): ("LEAN0", "PREP", "FULL_LDS", 1, 0, 0, "AFTER", 1, 4, 10752, 4, 512),
    (3136, F, 1, "default"): ("LEAN0_DEFAULT", "PREP", "FULL_LDS", 1, 0, 0, "AFTER", 1, 4, 10752, 4, 512),
    (3137, F, 1, "default"): ("LEAN0_DEFAULT", "PREP", "FULL_GSCR", 1, 0, 0, "AFTER", 1, 4, 10752, 4, 512),
    (4096, F, 1, "default"): ("LEAN0_DEFAULT", "PREP", "FULL_GSCR", 1, 0, 0, "AFTER", 1, 4, 10752, 4, 512),
    (4097, F, 1, "default"): ("LEAN0_DEFAULT", "PREP_WAVE2", "FULL_GSCR", 1, 0, 0, "AFTER", 1, 4, 10752, 4, 512),
    (8192, F, 1, "default"): ("LEAN0_DEFAULT", "PREP_WAVE2", "FULL_GSCR", 1, 0, 0, "AFTER", 1, 4, 10752, 4, 512),
    (8193, F, 1, "default"): ("LEAN0_DEFAULT", "PREP_WAVE3", "FULL_GSCR", 1, 0, 0, "AFTER", 1, 4, 10752, 4, 512),
    (12288, F, 1, "default"): ("LEAN0_DEFAULT", "PREP_WAVE3", "FULL_GSCR", 1, 0, 0, "AFTER", 1, 4, 10752, 4, 512),
    (12289, F, 1, "default"): ("LEAN0_DEFAULT", "PREP_WAVE4", "FULL_GSCR", 0, 0, 0, "NONE", 1, 4, 10752, 4, 0),
    (16384, F, 1, "default"): ("LEAN0_DEFAULT", "PREP_WAVE4", "FULL_GSCR", 0, 0, 0, "NONE", 1, 4, 10752, 4, 0),
    (16385, (1, 1, 0), 1, "default"): ("LEAN0_DEFAULT", "PREP", "FULL_GSCR", 0, 0, 0, "NONE", 1, 4, 10752, 4, 0),
    (32768, (1, 1, 0), 1, "default"): ("LEAN0_DEFAULT", "PREP", "FULL_GSCR", 0, 0, 0, "NONE", 1, 4, 10752, 4, 0),
    (32769, (1, 1, 0), 1, "none"): ("LEAN0", "PREP", "FULL_GSCR", 0, 0, 0, "NONE", 1, 4, 10752, 4, 0),
    (65535, (1, 1, 0), 1, "default"): ("LEAN0_DEFAULT", "PREP", "FULL_GSCR", 0, 0, 0, "NONE", 1, 4, 10752, 4, 0),
}
LITERAL_KEYS = ("variant", "prep", "full_variant", "use_rows", "early_rows", "may_defer", "rows", "defer_pass", "wpb", "lds",
                "batch", "row_grid")


@pytest.mark.parametrize("key", LITERAL, ids=lambda k: f"C{k[0]}-{'clean%d-fold%d-fitfold%d' % k[1]}-TW{k[2]}-{k[3]}")
def test_literal_routes(key):
    C, (clean, fold, fitfold), TW, sm = key
    got = runtime.route_eval(PER_CU, ROW_PER_CU, C=C, clean=clean, fold=fold, fitfold=fitfold, TW=TW, W=125000,
                             filter_mask=FILTER_DEFAULT, score_mask=SCORE_SETS[sm], n_cu=N_CU)
    assert tuple(got[k] for k in LITERAL_KEYS) == LITERAL[key], got
    assert C in CS
    check_invariants(got)


def test_empty_batch_launches_prep_alone():
    for C in (0, 1, 1000, 10000):
        r = runtime.route_eval(C=C, clean=1, fold=1, fitfold=1, W=0, score_mask=SM_DEFAULT)
        assert r["grid"] == 0 and r["batch"] == 0 and r["row_grid"] == 0 and r["prep"].startswith("PREP"), r
        check_invariants(r)


def test_no_side_stream_runs_the_rows_after_the_wide_kernel():
    """ROWS_BESIDE needs the row body not to fit inside the wide kernel, which no C <= 1024 reaches; with
    inlining tuned off (KAD_ROWS_NO_INLINE) the side stream decides between beside and after."""
    base = dict(C=1000, clean=1, fold=1, fitfold=1, W=125000, score_mask=SM_LEAST, filter_mask=FILTER_DEFAULT)
    assert runtime.route_eval(**base)["rows"] == "INLINE"
    assert runtime.route_eval(**base, rows_no_inline=1, side_stream=1)["rows"] == "BESIDE"
    r = runtime.route_eval(2, 2, **base, rows_no_inline=1, side_stream=0)
    assert r["rows"] == "AFTER" and r["early_rows"] == 1 and r["row_grid"] == 512, r
    assert runtime.route_eval(**base, rows_after=1)["early_rows"] == 0
    assert runtime.route_eval(**base, no_rows=1)["use_rows"] == 0
    assert runtime.route_eval(**dict(base, C=200), wide_min_nch=1)["family"] == "WIDE"
    assert runtime.route_eval(**dict(base, C=8192), prep_wave=0)["prep"] == "PREP"
    assert runtime.route_eval(1, 1, **dict(base, C=200), lean_blocks_per_cu=3)["grid"] == 768


def test_bench_profiles():
    """The flagship configurations, every figure by hand: C2 (256 clusters, LeastAllocated), C3 (1000, the same),
    C4 (500, the default set), C5 (10 000, the default set, four taint words)."""
    c2 = runtime.route_eval(2, 1, C=256, clean=1, fold=1, fitfold=1, W=100000, score_mask=SM_LEAST, filter_mask=FILTER_DEFAULT)
    assert (c2["variant"], c2["lds"], c2["grid"], c2["batch"], c2["rows"], c2["defer_pass"]) == \
        ("LEAN4_CLEAN_LEAST", 4 * 2688 + 7 * 8 * 256, 512, 4, "NONE", 0), c2
    c3 = runtime.route_eval(C=1000, clean=1, fold=1, fitfold=1, W=1000000, score_mask=SM_LEAST, filter_mask=FILTER_DEFAULT)
    assert (c3["variant"], c3["lds"], c3["grid"], c3["batch"], c3["rows"], c3["defer_pass"], c3["wpb"]) == \
        ("WIDE_LEAST", 141312, 256, 4, "INLINE", 0, 16), c3
    c4 = runtime.route_eval(C=500, clean=1, fold=1, fitfold=1, W=125000, score_mask=SM_DEFAULT, filter_mask=FILTER_DEFAULT)
    assert (c4["variant"], c4["lds"], c4["batch"], c4["cache_pn"]) == ("WIDE8_DEFAULT", 512 * 64 + 83968, 3, 1), c4
    c5 = runtime.route_eval(2, 2, C=10000, clean=1, fold=1, fitfold=1, TW=4, W=100000, score_mask=SM_DEFAULT,
                            filter_mask=FILTER_DEFAULT)
    assert (c5["variant"], c5["prep"], c5["row_variant"], c5["rows"], c5["defer_pass"], c5["full_variant"], c5["lds"],
            c5["row_grid"]) == ("LEAN0_DEFAULT", "PREP_WAVE3", "ROW_DEFAULT", "AFTER", 1, "FULL_GSCR", 10752, 512), c5


def test_rejects_inputs_outside_the_abi():
    for bad in (dict(C=-1), dict(C=65536), dict(W=-1), dict(n_cu=0)):
        with pytest.raises(ValueError):
            runtime.route_eval(**bad)
