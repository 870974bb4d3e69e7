"""Planner rows for kad_plan_rows, in families that each straddle one width switch of kad_plan.h (the bounds
of desired_narrow, clamp_narrow, the sort keys and ceil_extra), the lane shapes of the DPP scans, the pair
planner's row pairing and the avoid-disruption branches. tests/test_plan_ref_host.py checks on the CPU that the
rows are valid input and reach both sides of every switch (plan_ref.classify); tests/test_gpu_plan_rows.py
runs them on the GPU against plan_ref.plan_row.

Every row has non-negative fields and total * max(weight) + sum(weight) < 2^62, and passes the reference
within its round guard (plan_ref): Go's own loop need not end on a wrapped product or a negative weight, and
a kernel given such a row would spin on a shared GPU. The negative-value branches of desired_narrow and of the
clamp scans therefore stay untested.
"""
import functools
import math
import random

import plan_ref

B18, B20, B24, B25, B26, B31, B52 = (1 << b for b in (18, 20, 24, 25, 26, 31, 52))
COMBOS = ((False, False), (False, True), (True, False), (True, True))  # (avoid, keep)

# kad_k_plan.h plan_layout: twelve i64 and eight 32-bit arrays of Kp = K rounded up to 64 elements, each a
# multiple of 16 bytes: 12 * 8 * Kp + 8 * 4 * Kp = 128 * Kp bytes. The launch's LDS budget is 64 KiB = 128 * 512,
# so K = 512 (Kp = 512, 65 536 bytes) is the last row in LDS and K = 513 (Kp = 576, 73 728 bytes) the smallest
# whose workspace goes to the global slab (plan_rows_kernel<true>).
SLAB_K = 513


def layout_bytes(K):
    return 128 * ((K + 63) & ~63)


assert layout_bytes(SLAB_K - 1) <= 64 * 1024 < layout_bytes(SLAB_K)


def E(h, w, mn=0, mx=None, cap=None, cur=0):
    return {"hash": h, "weight": w, "min": mn, "max": mx, "cap": cap, "current": cur}


def row(elems, total, avoid=False, keep=False):
    return {"elems": elems, "total": total, "avoid": avoid, "keep": keep}


def x4(rows):
    """Every row under the four (avoid, keep) combinations."""
    return [row([dict(e) for e in r["elems"]], r["total"], a, k) for r in rows for a, k in COMBOS]


def _h(i):
    return (i * 2654435761 + 12345) & 0xFFFFFFFF


def base_elems(K, seed):
    """A narrow row's elements: weights below 2^10, some small minimums, maximums, capacities and current
    replicas, so that several rounds, both bounds and the overflow come into play."""
    rng = random.Random(seed)
    es = []
    for i in range(K):
        es.append(E(_h(seed * 1000 + i), rng.randrange(1, 1000), rng.randrange(0, 40) if rng.random() < 0.3 else 0,
                    rng.randrange(50, 400_000) if rng.random() < 0.3 else None,
                    rng.randrange(20, 300_000) if rng.random() < 0.25 else None,
                    rng.randrange(0, 300_000) if rng.random() < 0.5 else 0))
    return es


# ------------------------------------------------------------------ narrow bounds, one at a time
def narrow_bounds():
    """An otherwise narrow row (K = 64 and K = 32: the last lane of a wave and of a half-wave segment) with one
    field at bound - 1, bound, bound + 1; the offending element first, in the middle and last."""
    rows = []
    for K in (64, 32):
        for d in (-1, 0, 1):
            rows.append(row(base_elems(K, 1), B24 + d))
            for pos in (0, K // 2, K - 1):
                for field, bound in (("weight", B20), ("min", B18), ("max", B24), ("cap", B24)):
                    es = base_elems(K, 2)
                    es[pos][field] = bound + d
                    if field == "min":
                        es[pos]["max"] = None
                    rows.append(row(es, B24 - 1000))
        for pos in (0, K // 2, K - 1):
            for d in (0, 1):  # minimum = maximum (narrow), minimum = maximum + 1 (wide)
                es = base_elems(K, 3)
                es[pos]["max"] = 77
                es[pos]["min"] = 77 + d
                rows.append(row(es, 50_000))
    return x4(rows)


# ------------------------------------------------------------------ scan bound (clamp_narrow)
def scan_bound():
    """R crosses 2^24 between the minimum pass and the first round, and a single step reaches 2^24."""
    rows = []
    for K in (8, 40):
        for short in (100, 400 * K):  # minimums of 50 each: R falls below 2^24 only when 50 K > short
            es = base_elems(K, 4)
            for e in es:
                e["min"], e["max"] = 50, None
            rows.append(row(es, B24 + short - 50 * K))
        for d in (-1, 0, 1):  # one minimum-pass step min(minimum, capacity) at 2^24 - 1, 2^24, 2^24 + 1
            for capped in (False, True):
                es = base_elems(K, 5)
                es[K // 2]["min"], es[K // 2]["max"] = (B24 + 5 if capped else B24 + d), None
                es[K // 2]["cap"] = B24 + d if capped else None
                rows.append(row(es, B24 - 1))
                rows.append(row(es, B24 + 100_000))
    return x4(rows)


# ------------------------------------------------------------------ rank keys
def rank_key():
    rows = []
    for K in (5, 20, 40):
        for bound in (B25, B31):  # lane_sort_rank / pair_sort_rank's key; sort_by_weight_hash's (workspace)
            for d in (-1, 0):
                for pos in (0, K - 1):
                    es = base_elems(K, 6)
                    es[pos]["weight"] = bound + d
                    rows.append(row(es, 1_000_003))
                es = [E(_h(i) & 3, bound + d) for i in range(K)]  # every weight at the bound, tie-heavy hashes
                rows.append(row(es, 5 * K + 3))
    for K in (3, 8, 20, 40):
        hs = [0, 1, 0xFFFFFFFF]
        for rot in range(3):  # equal weights: the hash decides, the extremes of u32 in every row position
            rows.append(row([E(hs[(i + rot) % 3] if i < 3 else _h(i), 7) for i in range(K)], K + 1))
        # full (weight, hash) ties: the row position decides
        rows.append(row([E(9, 7) for _ in range(K)], K + 2))
        rows.append(row([E(9 if i % 3 else 4, 7 if i % 2 else 8) for i in range(K)], 2 * K + 3))
        rows.append(row([E(0xFFFFFFFF, B25 - 1) for _ in range(K)], K // 2 + 1))
        rows.append(row([E(0, B25) for _ in range(K)], K // 2 + 1))
    return x4(rows)


# ------------------------------------------------------------------ quotient (ceil_extra)
# Weight sums near 2^20 / 2^26 / 2^31: composite (so that D * w can be a multiple), no power of two, and chosen so
# that the f64 reciprocal 1.0 / S lies almost a whole unit in the last place below 1 / S: then int(nd * (1.0 / S))
# is one short of the quotient on most exact multiples and ceil_extra_inv's correction has to fire
# (test_plan_ref_host.py evaluates it).
S_FACTORS = {20: (1002, 1045), 26: (8173, 8205), 31: (46322, 46358)}
S_NEAR = {b: x * y for b, (x, y) in S_FACTORS.items()}


def _residue_pairs(bits, r, n, lim=B26):
    """n pairs (D, w), both below lim, with D * w = r (mod S): D * w + S - 1 is then a multiple of S (r = 1),
    one less (r = 0) or one more (r = 2)."""
    S = S_NEAR[bits]
    a, b = S_FACTORS[bits]
    out = []
    rng = random.Random(bits * 10 + r)
    while len(out) < n:
        if r == 0:
            D, w = a * rng.randrange(2, lim // a // 4), b * rng.randrange(2, min(lim // b // 4, a))  # (w < S)
        else:
            D = rng.randrange(lim // 8, lim)
            if math.gcd(D, S) != 1:
                continue
            w = r * pow(D, -1, S) % S
        if 0 < w < lim and D * w > S:
            out.append((D, w))
    return out


def _with_sum(w, S, extra=0):
    """Elements whose weights sum to S, the first of weight w (the others split the rest, none above 2^30)."""
    rest, ws = S - w, []
    while rest > 0:
        ws.append(min(rest, (1 << 30) - 1 - 7 * len(ws)))
        rest -= ws[-1]
    return [E(_h(extra), w)] + [E(_h(extra + 1 + i), x) for i, x in enumerate(ws)]


def quotient():
    rows = []
    # D and w at 2^26 - 1 / 2^26; (2^26 - 1)^2 + (2^27 - 1) - 1 = 2^52 - 1: the numerator just below and at 2^52
    for D in (B26 - 1, B26):
        for w in (B26 - 1, B26):
            for s2 in (B26 - 1, B26, 0):
                es = [E(1, w), E(2, s2)] if s2 else [E(1, w)]
                for one in (0, 1, 2):
                    rows.append(row(es + [E(3 + i, 1) for i in range(one)], D))
    # exact multiples of the weight sum, one less, one more
    for bits in (20, 26, 31):
        for r in (1, 0, 2):
            for j, (D, w) in enumerate(_residue_pairs(bits, r, 6)):
                rows.append(row(_with_sum(w, S_NEAR[bits], j), D))
            # the same residues with D past 2^26 (go_div)
            for j, (D, w) in enumerate(_residue_pairs(bits, r, 2, lim=1 << 30)):
                rows.append(row(_with_sum(w, S_NEAR[bits], 50 + j), D))
    rng = random.Random(77)
    for K in (3, 17, 40, 64):
        for _ in range(3):  # totals up to 2^36 with weights up to 2^26
            es = [E(_h(rng.randrange(1 << 20)), rng.randrange(0, B26 + 1), mx=rng.choice((None, rng.randrange(1 << 34))))
                  for _ in range(K)]
            rows.append(row(es, rng.randrange(1 << 30, (1 << 35))))
        for _ in range(3):  # totals up to 2^52 with weights <= 2^9
            es = [E(_h(rng.randrange(1 << 20)), rng.randrange(0, 513), mx=rng.choice((None, rng.randrange(1 << 50))),
                    cap=rng.choice((None, None, rng.randrange(1 << 50)))) for _ in range(K)]
            rows.append(row(es, rng.randrange(1 << 40, B52)))
    out = []
    for i, r in enumerate(rows):  # keep stays as the planner sets it without avoid; avoid only where its own
        out.append(r)             # getDesiredPlan calls stay within the input condition (totals below 2^30)
        if r["total"] < (1 << 30) and max(e["weight"] for e in r["elems"]) <= B26:
            out.append(row(r["elems"], r["total"], True, bool(i & 1)))
    return out


# ------------------------------------------------------------------ shapes
def staggered(K, total, seed=0):
    """A row of K preferences that takes K rounds: weights 2^(K-1) .. 1 and, on all but the lightest, a maximum
    equal to what the preference holds when it heads the list, so each round fills exactly the heaviest."""
    w = [1 << (K - 1 - i) for i in range(K)]
    plan, mx, R = [0] * K, [None] * K, total
    for first in range(K - 1):
        S = sum(w[first:])
        D = R
        mx[first] = plan[first]
        for i in range(first + 1, K):
            extra = min((D * w[i] + S - 1) // S, R)
            plan[i] += extra
            R -= extra
    return row([E(_h(seed + i), w[i], mx=mx[i]) for i in range(K)], total)


def multi_round(K, seed, wide=False):
    """K preferences of which many fill in different rounds (maximums and capacities spread over the shares)."""
    rng = random.Random(seed)
    total = (B24 + 12345) if wide else 40 * K + 17
    es = []
    for i in range(K):
        share = total // K
        es.append(E(_h(seed * 7919 + i), rng.randrange(1, 50), rng.randrange(0, 3),
                    rng.randrange(2, 2 * share + 3) if rng.random() < 0.5 else None,
                    rng.randrange(0, 2 * share + 3) if rng.random() < 0.3 else None, rng.randrange(0, 3 * share + 1)))
    return row(es, total)


SHAPE_KS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64)


def shapes():
    return x4([multi_round(K, 10 + K, wide) for K in SHAPE_KS for wide in (False, True)])


def shapes_long():
    """K = 65 and 100: the workspace planner as routed (two 64-element scans per pass)."""
    return x4([multi_round(K, 20 + K, wide) for K in (65, 100) for wide in (False, True)])


def long_257():
    rows = [multi_round(257, 31), multi_round(257, 32, True), multi_round(5, 33), multi_round(64, 34), multi_round(65, 35)]
    return [row(r["elems"], r["total"], a, k) for r, (a, k) in zip(rows + rows[:3], COMBOS * 2)]


def slab():
    """One row whose workspace exceeds the LDS budget (SLAB_K), so the launch takes plan_rows_kernel<true> on the
    global slab, beside shorter rows of the same launch (K <= 64 in registers, K = 65 on the slab)."""
    rows = [multi_round(SLAB_K, 41), multi_round(5, 42), multi_round(64, 43, True), multi_round(65, 44),
            multi_round(SLAB_K, 45, True)]
    return [row(r["elems"], r["total"], a, k) for r, (a, k) in zip(rows, COMBOS + COMBOS[3:])]


# ------------------------------------------------------------------ pair composition
PAIR_BLOCK = ("narrow|wide", "wide|narrow", "K32|K1", "K5|empty", "empty|K7", "K33|K20", "K20|K33",
              "one round|K rounds", "K rounds|one round")


def pair_block(avoid_a, keep_a, avoid_b, keep_b, seed):
    """Eighteen rows, paired (2 i, 2 i + 1) by plan_force_workspace(2) as PAIR_BLOCK names them."""
    narrow, wide = multi_round(10, seed + 1), multi_round(10, seed + 2, True)
    one = row([E(_h(i), 3) for i in range(12)], 36)  # finishes in its first round
    many = staggered(16, 1 << 22, seed)
    empty = row([], 0)
    pairs = [(narrow, wide), (wide, narrow), (multi_round(32, seed + 3), multi_round(1, seed + 4)),
             (multi_round(5, seed + 5), empty), (empty, multi_round(7, seed + 6)),
             (multi_round(33, seed + 7), multi_round(20, seed + 8)), (multi_round(20, seed + 9), multi_round(33, seed + 10)),
             (one, many), (many, one)]
    out = []
    for a, b in pairs:
        out.append(row(a["elems"], a["total"], avoid_a, keep_a))
        out.append(row(b["elems"], b["total"], avoid_b, keep_b))
    return out


def pairs():
    """Blocks of eighteen rows (an even count, so every block pairs alike) and a last row without a partner:
    the four (avoid, keep) combinations on both rows, then avoid on one row of the pair only."""
    out = []
    for i, (a, k) in enumerate(COMBOS):
        out += pair_block(a, k, a, k, 100 * i)
    out += pair_block(True, False, False, True, 500)
    out += pair_block(False, False, True, True, 600)
    out.append(multi_round(9, 700))
    return out


# ------------------------------------------------------------------ avoid-disruption
def avoid_cases():
    """(name, row): each branch of planner.Plan's second half, by the current replicas."""
    eq = [E(1, 1), E(2, 1), E(3, 1)]
    c = []
    c.append(("down", row([E(1, 1, cur=5), E(2, 1, cur=5), E(3, 1, cur=5)], 6)))
    c.append(("down", row([E(1, 3, cur=0), E(2, 1, cur=9), E(3, 1, cur=4)], 7)))
    c.append(("up", row([E(1, 1, cur=1), E(2, 1), E(3, 1)], 9)))
    c.append(("up", row([E(1, 5, cur=1), E(2, 1, cur=2), E(3, 1)], 20)))
    c.append(("equal", row([E(1, 1, cur=1), E(2, 1, cur=2), E(3, 1, cur=3)], 6)))
    c.append(("equal", row([dict(e) for e in eq], 0)))
    # the current replicas capped by capacity: 10 counts as 2, so the row scales up, not down
    c.append(("up", row([E(1, 1, cap=2, cur=10), E(2, 1), E(3, 1)], 6)))
    c.append(("down", row([E(1, 1, cap=2, cur=10), E(2, 1, cur=7), E(3, 1)], 6)))
    # scale-up stopped by max - current: the first preference may take one more, the shortfall goes on
    c.append(("up", row([E(1, 4, mx=4, cur=3), E(2, 1, cur=0), E(3, 1, cur=0)], 8)))
    c.append(("up", row([E(1, 4, mx=6, cur=5), E(2, 1, mx=1, cur=0), E(3, 1, cur=1)], 9)))
    # overflow: minimum 8 over capacity 1 leaves 7, the round adds its share; the second preference fills at its
    # maximum, so replicas remain and keep = false trims the overflow to them; with no maximum none remain and
    # the entry is dropped
    c.append(("up", row([E(1, 1, mn=8, cap=1), E(2, 1, mx=2)], 9)))
    c.append(("up", row([E(1, 1, mn=8, cap=1), E(2, 1)], 9)))
    c.append(("down", row([E(1, 1, mn=8, cap=1, cur=1), E(2, 1, mx=2, cur=6)], 9)))
    return c


def avoid():
    return x4([r for _, r in avoid_cases()])


# ------------------------------------------------------------------ randomised rows
def _draw(rng, classes):
    lo, hi = rng.choice(classes)
    return rng.randrange(lo, hi)


def random_row(rng):
    """Every field draws its magnitude class (below or above its bound) independently; one row in four draws
    from the classes below the bounds only, so that narrow rows are not left to chance."""
    tame = rng.random() < 0.25
    K = rng.choice((rng.randrange(1, 33), rng.randrange(1, 33), rng.randrange(33, 65), rng.choice(SHAPE_KS)))
    avoid, keep = rng.random() < 0.5, rng.random() < 0.5
    # a row that avoids disruption plans the shortfall or surplus with itself as the weights: total^2 stays
    # below 2^60 and the current replicas below 2^24
    t_cls = [(0, 20_000), (B24 - 50_000, B24), (B24, B24 + 50_000)] + ([(B24, 1 << 29)] if avoid else [(B24, 1 << 35)])
    total = _draw(rng, t_cls[:2] if tame else t_cls)
    w_cls = rng.choice(([(0, 5)], [(0, 1000)], [(0, B20)], [(B20 - 3, B20 + 3), (0, 1000)], [(B20, B25)],
                        [(B25 - 3, B25 + 3), (0, B20)], [(B25, B26 + 1)])[:3 if tame else 7])
    h_cls = rng.choice(([(0, 4)], [(0, 1 << 32)]))
    mn_cls = rng.choice(([(0, 1)], [(0, 6), (0, 1)], [(0, B18), (0, 1)], [(B18, B20), (0, 1), (0, 1)])[:3 if tame else 4])
    mx_cls = rng.choice(([(0, 200)], [(0, B24)], [(B24, 1 << 30)], [(B24 - 2, B24 + 2)])[:2 if tame else 4])
    cap_cls = rng.choice(([(0, 300)], [(0, B24)], [(B24, 1 << 30)], [(B24 - 2, B24 + 2)])[:2 if tame else 4])
    cur_cls = rng.choice(([(0, 1)], [(0, 400), (0, 1)], [(0, B24), (0, 1)]))
    es = []
    for _ in range(K):
        mn = _draw(rng, mn_cls)
        mx = _draw(rng, mx_cls) if rng.random() < 0.3 else None
        if mx is not None and mx < mn and rng.random() < 0.8:
            mx = mn + rng.randrange(0, 2)
        es.append(E(_draw(rng, h_cls), _draw(rng, w_cls), mn, mx, _draw(rng, cap_cls) if rng.random() < 0.25 else None,
                    _draw(rng, cur_cls)))
    return row(es, total, avoid, keep)


def admissible(r):
    """The condition under which a row may go to a GPU: non-negative, no wrap, and the reference ends within
    its round guard with every getDesiredPlan call inside the input condition."""
    if not plan_ref.valid_row(r):
        return False
    try:
        plan_ref.plan_row(r["elems"], r["total"], r["avoid"], r["keep"])
    except (plan_ref.RoundGuard, plan_ref.InputError):
        return False
    return True


def random_rows(seed, n=300):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        r = random_row(rng)
        if admissible(r):
            out.append(r)
    return out


# ------------------------------------------------------------------ rows for the schedule path
SCHEDULE_KS = (1, 32, 33, 64, 65, 100)  # placements: one cluster, a half-wave, one past; a wave, one past; all
I64_MAX = (1 << 63) - 1


def schedule_rows():
    """Rows that tests turn into Divide units (one element per placed cluster, the hashes then come from the
    cluster names): per placement size the bounds of desired_narrow one at a time, desired replicas around 2^24,
    the rank key's bound and weights up to 2^26, each with and without avoid-disruption; then the largest
    desired replicas: INT64_MAX with zero weights (the minimums alone are planned) and 2^62 - K - 1 with weights
    of one (the largest total the input condition admits with a positive weight), without avoid-disruption."""
    rows = []
    for K in SCHEDULE_KS:
        base = [multi_round(K, 60 + K), multi_round(K, 70 + K, True)]
        for d in (-1, 0, 1):
            base.append(row(base_elems(K, 8), B24 + d))
            for field, bound in (("weight", B20), ("min", B18), ("max", B24), ("cap", B24)):
                es = base_elems(K, 9)
                es[K // 2][field] = bound + d
                if field == "min":
                    es[K // 2]["max"] = None
                base.append(row(es, B24 - 1000))
        for wt in (B25 - 1, B25, B26):
            es = base_elems(K, 11)
            es[K // 2]["weight"] = wt
            base.append(row(es, B26 - 1))
        for i, r in enumerate(base):
            rows.append(row(r["elems"], r["total"], False, bool(i & 1)))
            rows.append(row(r["elems"], r["total"], True, not (i & 1)))
        es = base_elems(K, 12)
        for e in es:
            e["weight"], e["max"], e["cap"] = 0, None, None
        rows.append(row(es, I64_MAX))
        es = base_elems(K, 13)
        for e in es:
            e["weight"], e["max"], e["cap"] = 1, None, None
        rows.append(row(es, (1 << 62) - K - 1, False, True))
    return rows


@functools.lru_cache(maxsize=None)
def schedule_case():
    """(clusters, units, named rows): 100 plain clusters (no taints, Deployments served everywhere) and one Divide
    unit per row of schedule_rows(), placed on K consecutive clusters with static weights, MinReplicas,
    MaxReplicas, estimated capacities and current replicas from the row's elements. The named rows are the
    planner's view of the units (elements by ascending cluster id, hash = FNV-1 of name ‖ unit key)."""
    import numpy as np

    import gpu_util as G
    from kubeadmiral_amd import k8s, synth
    from kubeadmiral_amd import types as T

    clusters = synth.gen_clusters(np.random.default_rng(4242), 100, n_taints=0)
    G.serve_deployments(clusters)
    names = sorted(c.name for c in clusters)
    units, named = [], []
    for i, r in enumerate(schedule_rows()):
        es = r["elems"]
        place = sorted(names[(7 * i + j) % 100] for j in range(len(es)))
        caps = {n: e["cap"] for n, e in zip(place, es) if e["cap"] is not None}
        su = T.SchedulingUnit(
            group="apps", version="v1", kind="Deployment", resource="deployments", namespace="default",
            name=f"plan-{i}", desired_replicas=r["total"], scheduling_mode=T.SCHEDULING_MODE_DIVIDE,
            avoid_disruption=r["avoid"], cluster_names=set(place),
            tolerations=[T.Toleration(operator=T.TOLERATION_OP_EXISTS)],
            weights={n: e["weight"] for n, e in zip(place, es)}, min_replicas={n: e["min"] for n, e in zip(place, es)},
            max_replicas={n: e["max"] for n, e in zip(place, es) if e["max"] is not None} or None,
            current_clusters={n: e["current"] for n, e in zip(place, es) if e["current"] > 0} or None,
            auto_migration=T.AutoMigrationSpec(caps, r["keep"]) if (caps or r["keep"]) else None)
        units.append(su)
        named.append(row([dict(e, hash=k8s.fnv1_32((n + su.key()).encode())) for n, e in zip(place, es)],
                         r["total"], r["avoid"], r["keep"]))
    return clusters, units, named


# ------------------------------------------------------------------ the families
FAMILIES = {
    "narrow_bounds": narrow_bounds, "scan_bound": scan_bound, "rank_key": rank_key, "quotient": quotient,
    "shapes": shapes, "shapes_long": shapes_long, "long_257": long_257, "slab": slab, "pairs": pairs, "avoid": avoid,
    "random_1": lambda: random_rows(1), "random_2": lambda: random_rows(2),
}
DEFAULT_ROUTING_ONLY = ("long_257", "slab")  # (their long rows take one route whatever is forced)


@functools.lru_cache(maxsize=None)
def family(name):
    """(rows, reference results) of one family; computed once and shared by the tests."""
    rows = FAMILIES[name]()
    return rows, plan_ref.plan_rows(rows)
