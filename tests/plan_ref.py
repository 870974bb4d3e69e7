"""Row-level reference of planner.Plan for kad_plan_rows, on the oracle's own getDesiredPlan.

``plan_row`` takes the row dicts of ``Context.plan_rows`` (elements with hash, weight, min, max, cap, current;
total, avoid, keep) and returns (plan list, overflow list with None). The order of the preferences is the
project's rule for the planner: weight descending, hash ascending, row position ascending (on a
(weight, hash) tie the reference's own order depends on Go's map order; kad_plan.h sort_by_weight_hash breaks it
by position). ``getDesiredPlan`` is ``oracle.kad_oracle.get_desired_plan`` itself, called with the sorted
preference objects; the avoid-disruption half of planner.Plan (planner.go:134-177, 306-366) is restated here
over the given hashes, because the oracle's scale_up / scale_down derive the hashes from cluster names.
Python integers with gosem.wrap64 throughout, no numpy.

Two guards keep a row that Go itself would not finish away from a GPU (a wrapped ``distribute * weight`` or a
negative weight can keep planner.go:216-220's loop modifying for ever):

* ``RoundGuard``: every getDesiredPlan call counts its rounds and raises past m + 2 (m preferences). With
  non-negative values and no wrap a round that leaves replicas over has filled (and dropped) a preference, so
  m + 1 rounds are the most a valid call takes.
* ``InputError``: a getDesiredPlan call with a negative weight or total, or with
  total * max(weight) + sum(weight) >= 2^62 (the products and the numerator of planner.go:249 could wrap).

``valid_row`` states the conditions on the row's own fields; ``classify`` restates kad_plan.h's width switches on
the host for the row's first getDesiredPlan call, to show that a set of inputs reaches both sides of each.
"""
from oracle import kad_oracle as O
from oracle.gosem import wrap64

NO_WRAP = 1 << 62


class RoundGuard(Exception):
    """A getDesiredPlan call took more than m + 2 rounds."""


class InputError(Exception):
    """A getDesiredPlan call outside the no-wrap, non-negative input condition."""


class _Calls:
    """Round counts of the getDesiredPlan calls of one plan_row (the last entry is the call in progress)."""

    def __init__(self):
        self.rounds = []
        self.cap = 0


class _Pref:
    """A named preference for oracle.get_desired_plan. Every round reads the weight of each preference still
    listed exactly twice (the weight sum, then planner.go:249), and nothing else reads it: a preference's odd
    reads number the rounds it is listed in."""

    __slots__ = ("name", "hash", "min_replicas", "max_replicas", "_w", "_reads", "_calls")

    def __init__(self, name, hsh, mn, mx, w, calls):
        self.name, self.hash, self.min_replicas, self.max_replicas = name, hsh, mn, mx
        self._w, self._reads, self._calls = w, 0, calls

    @property
    def weight(self):
        self._reads += 1
        rnd = (self._reads + 1) // 2
        c = self._calls
        if rnd > c.rounds[-1]:
            c.rounds[-1] = rnd
            if rnd > c.cap:
                raise RoundGuard(f"getDesiredPlan: round {rnd} of a call with cap {c.cap}")
        return self._w


def _order(prefs):
    return sorted(prefs, key=lambda p: (-p._w, p.hash, p.name))


def _desired(prefs, capacity, total, keep, calls):
    ws = [p._w for p in prefs]
    if total < 0 or any(w < 0 for w in ws) or total * max(ws, default=0) + sum(ws) >= NO_WRAP:
        raise InputError(f"getDesiredPlan: total {total}, weights up to {max(ws, default=0)}, sum {sum(ws)}")
    calls.rounds.append(0)
    calls.cap = len(prefs) + 2
    return O.get_desired_plan(_order(prefs), capacity, total, keep)


def plan_row_rounds(elems, total, avoid, keep):
    """(plan, overflow, rounds of each getDesiredPlan call) of one row."""
    calls = _Calls()
    K = len(elems)
    prefs = [_Pref(i, e["hash"], e["min"], e.get("max"), e["weight"], calls) for i, e in enumerate(elems)]
    cap = {i: e["cap"] for i, e in enumerate(elems) if e.get("cap") is not None}
    if not avoid:  # planner.go:112-114
        keep = True
    desired, over = _desired(prefs, cap, total, keep, calls)
    overflow = [over.get(i) for i in range(K)]
    if not avoid:
        return [desired[i] for i in range(K)], overflow, calls.rounds
    # currentPlan, capped by capacity (planner.go:134-146)
    cur, cur_total, des_total = [], 0, 0
    for i, e in enumerate(elems):
        r = e["current"]
        if i in cap and cap[i] < r:
            r = cap[i]
        cur.append(r)
        cur_total = wrap64(cur_total + r)
        des_total = wrap64(des_total + desired[i])
    if cur_total == des_total:
        return cur, overflow, calls.rounds
    if cur_total > des_total:  # scaleDown (planner.go:340-366): weight = the surplus, at most the current replicas
        named = [_Pref(i, elems[i]["hash"], 0, cur[i], cur[i] - desired[i], calls)
                 for i in range(K) if desired[i] < cur[i]]
        down, _ = _desired(named, None, cur_total - des_total, False, calls)
        for i, n in down.items():
            cur[i] = wrap64(cur[i] - n)
        return cur, overflow, calls.rounds
    # scaleUp (planner.go:306-338): weight = the shortfall, at most max - current
    named = []
    for i in range(K):
        if desired[i] > cur[i]:
            mx = elems[i].get("max")
            named.append(_Pref(i, elems[i]["hash"], 0, None if mx is None else mx - cur[i], desired[i] - cur[i], calls))
    up, _ = _desired(named, None, des_total - cur_total, False, calls)
    for i, n in up.items():
        cur[i] = wrap64(cur[i] + n)
    return cur, overflow, calls.rounds


def plan_row(elems, total, avoid, keep):
    plan, overflow, _ = plan_row_rounds(elems, total, avoid, keep)
    return plan, overflow


def plan_rows(rows):
    return [plan_row(r["elems"], r["total"], r["avoid"], r["keep"]) for r in rows]


def valid_row(row):
    """The conditions on a row's own fields: every value >= 0 and total * max(weight) + sum(weight) < 2^62."""
    vals = [row["total"]]
    for e in row["elems"]:
        vals += [e["weight"], e["min"], e["current"]] + [e[k] for k in ("max", "cap") if e.get(k) is not None]
    ws = [e["weight"] for e in row["elems"]]
    return all(v >= 0 for v in vals) and row["total"] * max(ws, default=0) + sum(ws) < NO_WRAP


# ------------------------------------------------------------------ kad_plan.h's switches, restated
def first_call(row):
    """The first getDesiredPlan call of a valid row in sorted order, as far as the switches look: the
    minimum pass's clamp steps and the first weighted round's D, weight sum, numerators and clamp steps
    (None when no round runs)."""
    es = sorted(enumerate(row["elems"]), key=lambda ie: (-ie[1]["weight"], ie[1]["hash"], ie[0]))
    es = [e for _, e in es]
    R = row["total"]
    min_steps, start = [], []
    for e in es:
        cap = e.get("cap")
        min_steps.append(min(e["min"], cap) if cap is not None else e["min"])
        mt = min(e["min"], R)
        if cap is not None and cap < mt:
            mt = cap
        start.append(mt)
        R -= mt
    out = {"sorted": es, "min_steps": min_steps, "after_min": R, "round": None}
    wsum = sum(e["weight"] for e in es)
    if R > 0 and wsum > 0:
        nums = [R * e["weight"] + wsum - 1 for e in es]
        steps = []
        for e, s, num in zip(es, start, nums):
            bounds = [b for b in (e.get("max"), e.get("cap")) if b is not None]
            ee = num // wsum
            steps.append(min(ee, min(bounds) - s) if bounds else ee)
        out["round"] = {"D": R, "wsum": wsum, "nums": nums, "steps": steps}
    return out


def _scan_names(prefix, R, steps, names):
    """clamp_narrow per 64-element scan: R at the scan's start in [0, 2^24) and every step |s| < 2^24."""
    for a in range(0, len(steps), 64):
        chunk = steps[a:a + 64]
        names.add(prefix + ("32" if 0 <= R < (1 << 24) and all(abs(s) < (1 << 24) for s in chunk) else "64"))
        for s in chunk:
            R = max(R - s, 0) if s >= 0 else R - s


def quotient_is_f64(D, w, wsum, num):
    """ceil_extra / ceil_extra_inv take the corrected f64 quotient (else go_div)."""
    return 0 <= D < (1 << 26) and 0 <= w < (1 << 26) and 0 < wsum < (1 << 52) and 0 <= num < (1 << 52)


def classify(row):
    """Which side of each width switch the row's first getDesiredPlan call takes (a set of names):

    * ``narrow`` / ``wide``: desired_narrow / desired_plan_pair_any (the int32 getDesiredPlan of rows of K <= 64);
    * ``rank_key`` / ``rank_compare``: lane_sort_rank / pair_sort_rank's packed u64 key (every weight < 2^25);
    * ``ws_rank_key`` / ``ws_rank_compare``: sort_by_weight_hash's key of the workspace planner (K <= 64 and every
      weight < 2^31; longer rows always compare);
    * ``quot_f64`` / ``quot_godiv``: ceil_extra's quotient of each preference in the first weighted round;
    * ``min_scan32`` / ``min_scan64``, ``round_scan32`` / ``round_scan64``: clamp_narrow of the minimum pass's and
      the first round's scans (the int64 getDesiredPlan: wide rows, and every row of the workspace planner).
    """
    es = row["elems"]
    if not es:
        return set()
    names = set()

    def elem_narrow(e):
        mx, cap = e.get("max"), e.get("cap")
        return (0 <= e["weight"] < (1 << 20) and 0 <= e["min"] < (1 << 18)
                and (mx is None or (0 <= mx < (1 << 24) and e["min"] <= mx))
                and (cap is None or 0 <= cap < (1 << 24)))

    names.add("narrow" if 0 <= row["total"] < (1 << 24) and all(elem_narrow(e) for e in es) else "wide")
    names.add("rank_key" if all(0 <= e["weight"] < (1 << 25) for e in es) else "rank_compare")
    names.add("ws_rank_key" if len(es) <= 64 and all(0 <= e["weight"] < (1 << 31) for e in es) else "ws_rank_compare")
    fc = first_call(row)
    _scan_names("min_scan", row["total"], fc["min_steps"], names)
    rd = fc["round"]
    if rd is not None:
        for e, num in zip(fc["sorted"], rd["nums"]):
            names.add("quot_f64" if quotient_is_f64(rd["D"], e["weight"], rd["wsum"], num) else "quot_godiv")
        _scan_names("round_scan", rd["D"], rd["steps"], names)
    return names


ALL_NAMES = {"narrow", "wide", "rank_key", "rank_compare", "ws_rank_key", "ws_rank_compare", "quot_f64", "quot_godiv",
             "min_scan32", "min_scan64", "round_scan32", "round_scan64"}
