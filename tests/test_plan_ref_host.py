"""CPU checks of the planner's row reference (plan_ref.py) and of the rows the GPU tests send
(plan_cases.py): the reference is pinned to the oracle's planner.Plan, every row is admissible input, and the
rows reach both sides of each width switch of kad_plan.h (plan_ref.classify).

Admissible input is non-negative and cannot wrap: all of weight, minimum, maximum, capacity, current and total
>= 0, total * max(weight) + sum(weight) < 2^62, and the reference ends within its round guard. Go's own loop
need not end once ``distribute * weight`` wraps or a weight is negative, and a kernel given such a row would spin
on a shared GPU; the negative-value branches of desired_narrow and of the clamp scans stay untested for that
reason.
"""
import collections
import random

import pytest

import plan_cases as PC
import plan_ref as PR
from golden_util import case_id, load
from kubeadmiral_amd import k8s
from oracle import kad_oracle as O

PLANNER = load("planner.json")


def ref_plan(rsp, replicas, clusters, existing, est, key, avoid, keep):
    """planner.Plan's signature (oracle.kad_oracle.plan) on plan_ref.plan_row."""
    prefs = [(c, rsp.get(c, rsp.get("*"))) for c in clusters]
    prefs = [(c, p) for c, p in prefs if p is not None]
    elems = [{"hash": k8s.fnv1_32((n + key).encode()), "weight": p.weight, "min": p.min_replicas,
              "max": p.max_replicas, "cap": (est or {}).get(n), "current": (existing or {}).get(n, 0)} for n, p in prefs]
    plan, over = PR.plan_row(elems, replicas, avoid, keep)
    return ({n: v for (n, _), v in zip(prefs, plan)}, {n: v for (n, _), v in zip(prefs, over) if v is not None})


def test_plan_ref_equals_oracle_on_golden_cases():
    """Every call of planner_test.go's convergence driver on the 192 golden cases: plan_ref == oracle.plan."""
    from test_oracle_golden import run_planner_case
    calls = 0

    def both(*a):
        nonlocal calls
        calls += 1
        got, want = ref_plan(*a), O.plan(*a)
        assert got == want, a
        return want

    assert len(PLANNER) == 192
    for c in PLANNER:
        converged, plan, over = run_planner_case(c, both)
        assert converged, case_id(c)
    assert calls >= len(PLANNER)


def test_plan_ref_equals_oracle_on_random_named_rows():
    """400 random named rows (K up to 40, so both of Go's sort regimes; minimums, maximums, capacities, current
    replicas, all four avoid / keep combinations) without (weight, hash) ties: the restated avoid-disruption half
    equals the oracle's scale_up / scale_down."""
    rng = random.Random(5)
    branches = collections.Counter()
    over_n = 0
    for i in range(400):
        K = rng.choice((rng.randrange(1, 13), rng.randrange(13, 41)))
        names = [f"cluster-{rng.randrange(10_000):04d}-{j}" for j in range(K)]
        key = f"ns{i % 5}/unit-{i}"
        rsp = {n: O.ClusterPreferences(rng.randrange(0, 6) if rng.random() < 0.3 else 0,
                                       rng.randrange(0, 200) if rng.random() < 0.3 else None,
                                       rng.randrange(0, 5 if rng.random() < 0.4 else 1000)) for n in names}
        assert len({(p.weight, k8s.fnv1_32((n + key).encode())) for n, p in rsp.items()}) == K  # no ties
        existing = {n: rng.randrange(0, 400) for n in names if rng.random() < 0.5}
        est = {n: rng.randrange(0, 300) for n in names if rng.random() < 0.25}
        avoid, keep = PC.COMBOS[i % 4]
        args = (rsp, rng.randrange(0, 20_000), names, existing, est, key, avoid, keep)
        got, want = ref_plan(*args), O.plan(*args)
        assert got == want, (i, args)
        over_n += bool(want[1])
        if avoid:
            des = sum(O.plan(*args[:6], False, keep)[0].values())
            cur = sum(min(v, est.get(n, v)) for n, v in existing.items())
            branches["up" if cur < des else "down" if cur > des else "equal"] += 1
    assert branches["up"] > 20 and branches["down"] > 20 and over_n > 50, (branches, over_n)


@pytest.mark.parametrize("name", list(PC.FAMILIES))
def test_every_row_is_admissible(name):
    """Non-negative fields, no wrap, and the reference within its round guard (each getDesiredPlan call at most
    m + 2 rounds, and itself inside the no-wrap condition): for every row that goes to a GPU."""
    rows, want = PC.family(name)
    assert len(rows) == len(want)
    for i, r in enumerate(rows):
        assert PR.valid_row(r), (name, i)
        _, _, rounds = PR.plan_row_rounds(r["elems"], r["total"], r["avoid"], r["keep"])  # raises past the guard
        assert max(rounds) <= len(r["elems"]) + 2, (name, i, rounds)


def test_row_budget():
    assert sum(len(PC.family(n)[0]) for n in PC.FAMILIES) <= 2000


def test_round_guard_and_input_condition_raise():
    """The guards themselves: a wrapping product is refused before the oracle runs, and a call that keeps
    modifying (a negative maximum hands replicas back every round) stops at its cap."""
    with pytest.raises(PR.InputError):
        PR.plan_row([PC.E(1, 1 << 40), PC.E(2, 1)], 1 << 30, False, False)
    with pytest.raises(PR.InputError):
        PR.plan_row([PC.E(1, -1), PC.E(2, 5)], 10, False, False)
    calls = PR._Calls()
    prefs = [PR._Pref(0, 1, 0, None, 1, calls)]
    calls.rounds.append(0)
    calls.cap = 1
    for _ in range(2):
        prefs[0].weight
    with pytest.raises(PR.RoundGuard):
        prefs[0].weight
    assert not PR.valid_row(PC.row([PC.E(1, 1, mn=-1)], 5)) and not PR.valid_row(PC.row([PC.E(1, 1 << 40)], 1 << 30))


def names_of(rows):
    cnt = collections.Counter()
    for r in rows:
        cnt.update(PR.classify(r))
    return cnt


SWITCHES = {
    "narrow_bounds": [("narrow", "wide")],
    "scan_bound": [("min_scan32", "min_scan64"), ("round_scan32", "round_scan64")],
    "rank_key": [("rank_key", "rank_compare"), ("ws_rank_key", "ws_rank_compare")],
    "quotient": [("quot_f64", "quot_godiv")],
    "shapes": [("narrow", "wide")],
    "shapes_long": [("min_scan32", "min_scan64")],
    "pairs": [("narrow", "wide")],
    "random_1": [(a, b) for a, b in zip(sorted(PR.ALL_NAMES)[0::2], sorted(PR.ALL_NAMES)[1::2])],
    "random_2": [("narrow", "wide"), ("rank_key", "rank_compare"), ("quot_f64", "quot_godiv")],
}


@pytest.mark.parametrize("name", list(SWITCHES))
def test_family_reaches_both_sides_of_its_switch(name):
    cnt = names_of(PC.family(name)[0])
    for a, b in SWITCHES[name]:
        if name == "random_1" and a.startswith("ws_"):
            continue  # (rows of K <= 64 with weights below 2^31: the workspace key only)
        assert cnt[a] >= 4 and cnt[b] >= 4, (name, a, b, dict(cnt))


def test_every_classification_occurs():
    cnt = collections.Counter()
    for n in PC.FAMILIES:
        cnt.update(names_of(PC.family(n)[0]))
    assert set(cnt) == PR.ALL_NAMES, dict(cnt)


def test_narrow_bounds_sit_on_the_bounds():
    """Per K: the 13 rows at bound - 1 (total; weight, minimum, maximum, capacity at three positions) and the 3
    rows with minimum = maximum are narrow, every row at or past a bound and with minimum = maximum + 1 is wide."""
    rows, _ = PC.family("narrow_bounds")
    cnt = names_of(rows)
    assert cnt["narrow"] == 2 * 4 * (13 + 3) and cnt["wide"] == len(rows) - cnt["narrow"]
    for field, bound in (("weight", PC.B20), ("min", PC.B18), ("max", PC.B24), ("cap", PC.B24)):
        for v in (bound - 1, bound, bound + 1):
            hit = [r for r in rows if any(e[field] == v for e in r["elems"])]
            assert {i for r in hit for i, e in enumerate(r["elems"]) if e[field] == v} >= {0, len(hit[0]["elems"]) // 2}
            assert all(("narrow" in PR.classify(r)) == (v < bound) for r in hit if r["total"] < PC.B24), (field, v)
    assert {r["total"] for r in rows} >= {PC.B24 - 1, PC.B24, PC.B24 + 1}


def test_scan_bound_rows():
    rows, _ = PC.family("scan_bound")
    kinds = collections.Counter()
    for r in rows:
        n = PR.classify(r)
        if r["total"] >= PC.B24 and "round_scan32" in n:
            kinds["R below 2^24 only after the minimum pass"] += 1
        fc = PR.first_call(r)
        if r["total"] < PC.B24 and max(fc["min_steps"]) >= PC.B24:
            assert "min_scan64" in n
            kinds["a step at 2^24 under R < 2^24"] += 1
        if r["total"] < PC.B24 and max(fc["min_steps"]) == PC.B24 - 1:
            assert "min_scan32" in n
            kinds["a step at 2^24 - 1"] += 1
    assert len(kinds) == 3 and min(kinds.values()) >= 4, kinds


def test_quotient_rows_need_the_correction():
    """The f64 side of ceil_extra on the quotient family, evaluated here without its corrections:

    * ``int(nd * (1.0 / sd))`` (ceil_extra_inv, and the int32 planner's inline form) is one short of the integer
      quotient on rows of every weight-sum class (near 2^20, 2^26, 2^31), so the ``r >= sd`` correction fires;
    * no estimate is ever above the quotient, and ``int(nd / sd)`` (ceil_extra) is never off: for a numerator below
      2^52 the correctly rounded quotient cannot reach the next integer from below (the gap 1 / sd is more than
      half a unit in the last place of the quotient), so the ``r < 0`` correction and a second step have no
      admissible input that reaches them. Asserted here as what the inputs show, not assumed.

    Exact multiples of the weight sum, one less and one more all occur, on both sides of the switch."""
    rows, _ = PC.family("quotient")
    short = collections.Counter()
    residues = collections.Counter()
    sides = collections.Counter()
    for r in rows:
        rd = PR.first_call(r)["round"]
        if rd is None:
            continue
        D, S = rd["D"], rd["wsum"]
        cls = [b for b, s in PC.S_NEAR.items() if s == S]
        for e, num in zip(PR.first_call(r)["sorted"], rd["nums"]):
            f64 = PR.quotient_is_f64(D, e["weight"], S, num)
            if cls and num % S in (0, 1, S - 1):
                residues[cls[0], num % S, f64] += 1
            if D in (PC.B26 - 1, PC.B26) and e["weight"] in (PC.B26 - 1, PC.B26):
                sides[D, e["weight"], num >= PC.B52, f64] += 1
            if not f64:
                continue
            q, nd, sd = num // S, float(num), float(S)
            assert int(nd / sd) == q, (D, e["weight"], S)
            d = int(nd * (1.0 / sd)) - q
            assert d in (0, -1), (D, e["weight"], S)
            if d == -1 and cls:
                short[cls[0]] += 1
    assert all(short[b] >= 2 for b in (20, 26, 31)), short
    for b in (20, 26, 31):
        for res in (0, 1, PC.S_NEAR[b] - 1):
            assert residues[b, res, True] >= 2 and residues[b, res, False] >= 1, (b, res, residues)
    # D = w = 2^26 - 1: the numerator 2^52 - 1 takes the f64 quotient, 2^52 go_div; D or w at 2^26: go_div
    assert sides[PC.B26 - 1, PC.B26 - 1, False, True] and sides[PC.B26 - 1, PC.B26 - 1, True, False], sides
    assert not any(f for (D, w, _, f) in sides if PC.B26 in (D, w)) and len({(D, w) for D, w, _, _ in sides}) == 4
    nums = {num for r in rows if (rd := PR.first_call(r)["round"]) for num in rd["nums"]}
    assert {PC.B52 - 1, PC.B52} <= nums
    assert any(r["total"] >= 1 << 40 and max(e["weight"] for e in r["elems"]) <= 512 for r in rows)
    assert any(r["total"] >= 1 << 30 and max(e["weight"] for e in r["elems"]) >= 1 << 25 for r in rows)


def test_rank_rows_tie_and_bound():
    rows, _ = PC.family("rank_key")
    ws = {e["weight"] for r in rows for e in r["elems"]}
    assert {PC.B25 - 1, PC.B25, PC.B31 - 1, PC.B31} <= ws
    full_ties = [r for r in rows if len({(e["weight"], e["hash"]) for e in r["elems"]}) == 1 and len(r["elems"]) > 1]
    assert {len(r["elems"]) <= 12 for r in full_ties} == {True, False}
    assert any({0, 1, 0xFFFFFFFF} <= {e["hash"] for e in r["elems"]} and len({e["weight"] for e in r["elems"]}) == 1
               for r in rows)


def test_shapes_and_long_rows():
    assert {len(r["elems"]) for r in PC.family("shapes")[0]} == set(PC.SHAPE_KS)
    assert {len(r["elems"]) for r in PC.family("shapes_long")[0]} == {65, 100}
    assert max(len(r["elems"]) for r in PC.family("long_257")[0]) == 257
    ks = [len(r["elems"]) for r in PC.family("slab")[0]]
    assert max(ks) == PC.SLAB_K and PC.layout_bytes(PC.SLAB_K) > 64 * 1024 >= PC.layout_bytes(PC.SLAB_K - 1)
    for name in ("shapes", "shapes_long", "long_257", "slab"):  # several rounds: the active list shrinks
        rows, _ = PC.family(name)
        multi = [max(PR.plan_row_rounds(r["elems"], r["total"], r["avoid"], r["keep"])[2]) for r in rows]
        assert sum(m >= 3 for m in multi) >= len(rows) // 3, (name, multi)


def test_pairs_pair_what_they_claim():
    """plan_force_workspace(2) plans rows 2 i and 2 i + 1 together when both hold at most 32 elements: the
    family's fixed order puts PAIR_BLOCK's pairs there."""
    rows, _ = PC.family("pairs")
    assert len(rows) % 2 == 1  # the last row has no partner
    n = 2 * len(PC.PAIR_BLOCK)
    assert (len(rows) - 1) % n == 0
    want_k = [(10, 10), (10, 10), (32, 1), (5, 0), (0, 7), (33, 20), (20, 33), (12, 16), (16, 12)]
    mixed_avoid = 0
    for b in range(0, len(rows) - 1, n):
        blk = rows[b:b + n]
        pairs = [(blk[2 * i], blk[2 * i + 1]) for i in range(len(PC.PAIR_BLOCK))]
        assert [(len(a["elems"]), len(c["elems"])) for a, c in pairs] == want_k
        cls = [("narrow" in PR.classify(a), "narrow" in PR.classify(c)) for a, c in pairs[:2]]
        assert cls == [(True, False), (False, True)]
        for one, many in (pairs[7], pairs[8][::-1]):  # frozen lanes: one round beside sixteen
            assert PR.plan_row_rounds(one["elems"], one["total"], False, False)[2] == [1]
            assert PR.plan_row_rounds(many["elems"], many["total"], False, False)[2] == [16]
        mixed_avoid += any(a["avoid"] != c["avoid"] for a, c in pairs)
        # neighbouring K <= 32 are planned as a pair, K = 33 beside K = 20 falls back to one row per wave
        assert [max(len(a["elems"]), len(c["elems"])) <= 32 for a, c in pairs] == [True] * 5 + [False] * 2 + [True] * 2
    assert mixed_avoid == 2


def test_avoid_rows_take_their_branch():
    for i, (want, r) in enumerate(PC.avoid_cases()):
        desired, _ = PR.plan_row(r["elems"], r["total"], False, False)
        cur = sum(min(e["current"], e["cap"]) if e["cap"] is not None else e["current"] for e in r["elems"])
        got = "up" if cur < sum(desired) else "down" if cur > sum(desired) else "equal"
        assert got == want, (i, cur, desired)
    cases = [r for _, r in PC.avoid_cases()]
    # scale-up stopped by max - current: the capped preference ends at its maximum with the shortfall elsewhere
    plan, _ = PR.plan_row(cases[8]["elems"], cases[8]["total"], True, False)
    assert plan[0] == 4 and sum(plan) == 8
    # the current replicas capped by capacity
    plan, _ = PR.plan_row(cases[6]["elems"], cases[6]["total"], True, False)
    assert plan[0] <= 2
    # keep = false trims the overflow to the replicas that remain, and drops the entry when none remain
    assert PR.plan_row(cases[10]["elems"], 9, True, False)[1] == [6, None]
    assert PR.plan_row(cases[10]["elems"], 9, True, True)[1] == [11, None]  # 7 of the minimum + (8 + 2 - 1) // 2
    assert PR.plan_row(cases[11]["elems"], 9, True, False)[1] == [None, None]
    assert PR.plan_row(cases[11]["elems"], 9, True, True)[1][0] > 0


def test_schedule_units_are_admissible_and_c_oracle_equals_plan_ref():
    """The Divide units of the schedule-path test: admissible rows, every placement size, values inside int32
    (so the batch takes the i32 preference columns), and the C oracle's result rows equal plan_ref's plan +
    overflow (zeros dropped, ascending cluster id) — the two references of the GPU tests agree on them."""
    from gpu_util import c_oracle, default_framework
    from kubeadmiral_amd import pack
    clusters, units, named = PC.schedule_case()
    assert {len(r["elems"]) for r in named} == set(PC.SCHEDULE_KS)
    assert {r["total"] for r in named} >= {PC.B24 - 1, PC.B24, PC.B24 + 1, PC.I64_MAX}
    assert {r["avoid"] for r in named} == {False, True}
    cnt = names_of(named)
    assert all(cnt[n] >= 4 for n in ("narrow", "wide", "rank_key", "rank_compare", "quot_f64", "quot_godiv")), cnt
    snap = pack.Snapshot(clusters)
    fwk = default_framework()
    batch = pack.Batch(snap, fwk, units)
    assert pack.header_of(batch.blob, pack.BatchHeader).flags == pack.BATCH_NARROW_PREFS
    want = c_oracle(snap, batch, fwk)
    for w, (su, r) in enumerate(zip(units, named)):
        assert PC.admissible(r), w
        plan, over = PR.plan_row(r["elems"], r["total"], r["avoid"], r["keep"])
        ids = sorted(snap.name_id[n] for n in su.cluster_names)
        pairs = [(c, p + (o or 0)) for c, p, o in zip(ids, plan, over) if p + (o or 0) != 0]
        assert want.row(w) == (pack.ST_OK, pairs), (w, want.row(w), pairs)
