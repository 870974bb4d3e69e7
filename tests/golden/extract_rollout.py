#!/usr/bin/env python3
"""Extract the rollout planner's unit-test cases into tests/golden/rolloutplan.json.

    python tests/golden/extract_rollout.py

Reads pkg/controllers/util/rolloutplan_test.go of the reference AS TEXT (``KAD_REFERENCE``, at extraction time only)
and walks the statements of its eight test functions: each builds PlanTestSuits statement by statement
(``s.Targets = Targets{newTarget(...), ...}``, ``s.Plans = RolloutPlans{...}``, ``tests = append(tests, s)``) and
then runs every suit collected so far through a ``&RolloutPlanner{...}`` literal, whose fields are either the
suit's or constants (TestPlanCreation leaves Replicas out, TestPlanEmptyTargets fixes all three). One case is
written per (loop, suit), with the three target constructors expanded to the full twelve fields. Data only.
"""

from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from goliteral import find_func_body, tokenize  # noqa: E402

REF = os.environ.get("KAD_REFERENCE", "/root/reference")
REL = "pkg/controllers/util/rolloutplan_test.go"
FUNCS = ("TestPlanWholeProcessWithMaxUnavailable", "TestPlanWholeProcessWithBoth", "TestPlanWholeProcessWithSurge",
         "TestPlanCreation", "TestPlanScale", "TestPlanEmptyTargets", "TestPlanUnexceptedCases", "TestPlanActualCases")
PLAN_FIELDS = ("Replicas", "MaxSurge", "MaxUnavailable", "OnlyPatchReplicas")
PLAN_KEYS = ("replicas", "max_surge", "max_unavailable", "only_patch_replicas")


def target(kind, a):
    """newTarget / newTargetWithActualInfo / newTargetWithAllInfo (rolloutplan_test.go:37-135)."""
    name, updated, replicas, desired, upd, upd_avail = a[:6]
    if kind == "newTarget":
        ms, mu = a[6:]
        actual = available = replicas
    elif kind == "newTargetWithActualInfo":
        actual, available, ms, mu = a[6:]
    if kind == "newTargetWithAllInfo":
        cur_new, cur_new_avail, actual, available, ms, mu = a[6:]
    else:
        cur_new = upd if updated else replicas
        cur_new_avail = cur_new
    return {"name": name, "updated": updated, "replicas": replicas, "actual": actual, "available": available,
            "updated_replicas": upd, "updated_available": upd_avail, "current_new": cur_new,
            "current_new_available": cur_new_avail, "max_surge": ms, "max_unavailable": mu, "desired": desired}


class Walk:
    def __init__(self, toks, env=None):
        self.t, self.i, self.env = toks, 0, env or {}

    def peek(self, k=0):
        return self.t[self.i + k].val

    def next(self):
        self.i += 1
        return self.t[self.i - 1]

    def expect(self, v):
        tok = self.next()
        if tok.val != v:
            raise SyntaxError(f"expected {v!r}, got {tok.val!r} at {tok.pos}")

    def at(self, *vals):
        return all(self.peek(k) == v for k, v in enumerate(vals))

    def scalar(self):
        """A number, a string, true / false / nil, a variable of the function, ptr(x)."""
        tok = self.next()
        if tok.val == "-":
            return -self.scalar()
        if tok.kind == "num":
            return int(tok.val)
        if tok.kind == "str":
            return json.loads(tok.val)
        if tok.val in ("true", "false"):
            return tok.val == "true"
        if tok.val == "nil":
            return None
        if tok.val == "ptr":
            self.expect("(")
            v = self.scalar()
            self.expect(")")
            return v
        if tok.kind == "ident" and tok.val in self.env:
            return self.env[tok.val]
        raise SyntaxError(f"unsupported value {tok.val!r} at {tok.pos}")

    def fields(self, names):
        """``{a, b}`` or ``{X: a}`` after the opening brace → dict by names (absent: the zero value None)."""
        out, pos = {}, 0
        while self.peek() != "}":
            if self.t[self.i].kind == "ident" and self.peek(1) == ":":
                key = self.next().val
                self.next()
            else:
                key = names[pos]
                pos += 1
            if key not in names:
                raise SyntaxError(f"unknown field {key}")
            out[key] = self.scalar()
            if self.peek() == ",":
                self.next()
        self.next()
        return out

    def skip_block(self):
        depth = 0
        while True:
            v = self.next().val
            depth += v == "{"
            depth -= v == "}"
            if depth == 0 and v == "}":
                return


def planner_literal(toks, i, env):
    """The fields of the ``RolloutPlanner{...}`` literal that starts at token i + 1 ('{'): ('suit', field), a number or a
    variable of the function."""
    out, i = {}, i + 2
    while toks[i].val != "}":
        key = toks[i].val
        assert toks[i + 1].val == ":", key
        i += 2
        if toks[i].val == "test":
            out[key] = ("suit", toks[i + 2].val)
            i += 3
        else:
            out[key] = env[toks[i].val] if toks[i].val in env else int(toks[i].val)
            i += 1
        if toks[i].val == ",":
            i += 1
    return out


def extract_func(src, fn):
    toks = find_func_body(src, fn)
    w = Walk(toks)
    suits, suit, cases = [], None, []
    while w.peek() != "":
        if w.at("var") and w.peek(1) != "tests":  # var a, b, c int32 = 1, 2, 3
            w.next()
            names = [w.next().val]
            while w.peek() == ",":
                w.next()
                names.append(w.next().val)
            w.next()  # the type
            w.expect("=")
            for k, n in enumerate(names):
                w.env[n] = w.scalar()
                if k + 1 < len(names):
                    w.expect(",")
        elif w.at("var", "tests"):
            while w.peek() != "PlanTestSuit":
                w.next()
            w.next()
        elif w.at("s", ":=") or w.at("s", "="):
            w.next(), w.next()
            w.expect("PlanTestSuit")
            w.expect("{")
            f = w.fields(("Name", "Targets", "Plans", "MaxSurge", "MaxUnavailable", "Replicas"))
            suit = {"Name": "", "Targets": [], "Plans": {}, "MaxSurge": 0, "MaxUnavailable": 0, "Replicas": 0, **f}
        elif w.at("s", ".", "Name", "="):
            w.i += 4
            suit["Name"] = w.scalar()
        elif w.at("s", ".", "Targets", "="):
            w.i += 4
            w.expect("Targets")
            w.expect("{")
            ts = []
            while w.peek() != "}":
                kind = w.next().val
                w.expect("(")
                args = []
                while w.peek() != ")":
                    args.append(w.scalar())
                    if w.peek() == ",":
                        w.next()
                w.next()
                ts.append(target(kind, args))
                if w.peek() == ",":
                    w.next()
            w.next()
            suit["Targets"] = ts
        elif w.at("s", ".", "Plans", "="):
            w.i += 4
            w.expect("RolloutPlans")
            w.expect("{")
            plans = {}
            while w.peek() != "}":
                name = w.scalar()
                w.expect(":")
                w.expect("{")
                f = w.fields(PLAN_FIELDS)
                plans[name] = {k: (f.get(n) if n != "OnlyPatchReplicas" else bool(f.get(n))) for n, k in zip(PLAN_FIELDS, PLAN_KEYS)}
                if w.peek() == ",":
                    w.next()
            w.next()
            suit["Plans"] = plans
        elif w.at("tests", "=", "append"):
            while w.peek() != ")":
                w.next()
            w.next()
            suits.append(dict(suit))
        elif w.at("for"):
            start = w.i
            while w.peek() != "{":
                w.next()
            w.skip_block()
            lit = [k for k in range(start, w.i) if toks[k].val == "RolloutPlanner" and toks[k + 1].val == "{"]
            assert len(lit) == 1, fn
            pl = planner_literal(toks, lit[0], w.env)
            for s in suits:
                val = lambda key, zero: (s[pl[key][1]] if isinstance(pl[key], tuple) else pl[key]) if key in pl else zero  # noqa: E731
                cases.append({"func": fn, "name": s["Name"], "replicas": val("Replicas", 0), "max_surge": val("MaxSurge", 0),
                              "max_unavailable": val("MaxUnavailable", 0), "targets": val("Targets", []), "plans": s["Plans"]})
        else:
            raise SyntaxError(f"{fn}: unsupported statement at token {w.peek()!r} ({toks[w.i].pos})")
    return cases


def main():
    with open(os.path.join(REF, REL)) as f:
        src = f.read()
    assert tokenize  # (goliteral's tokenizer, through find_func_body)
    cases = [c for fn in FUNCS for c in extract_func(src, fn)]
    doc = {"source": REL + " (the eight Test* functions), as data: every suit as the RolloutPlanner literal of its "
                     "t.Run loop sees it; targets expanded from newTarget / newTargetWithActualInfo / "
                     "newTargetWithAllInfo; a nil plan field is null",
           "cases": cases}
    out = os.path.join(HERE, "rolloutplan.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(out, len(cases), "cases")


if __name__ == "__main__":
    main()
