"""Shapes for kad_rollout_plan's tests: batches as the call's arrays, built directly (no Kubernetes objects), so that
the host tests and the GPU tests walk the same ones. Objects are (replicas, max_surge, max_unavailable, targets,
error) with targets as dicts of rollout_ref.FIELDS plus ``updated`` / ``exists`` / ``to_delete``."""
import json
import os

import numpy as np

import rollout_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
BIG = 2 ** 31 - 1


def golden():
    with open(os.path.join(HERE, "golden", "rolloutplan.json")) as f:
        return json.load(f)["cases"]


def tgt(replicas=0, desired=0, updated=False, new=None, new_avail=None, actual=None, available=None, ms=0, mu=0,
        upd_r=None, upd_a=None, exists=True, to_delete=False):
    """A target the way the reference's newTarget* build one: the new replica set holds ``new`` (``new_avail``
    available) replicas, which count as updated when the template is."""
    new = (0 if updated else replicas) if new is None else new
    new_avail = new if new_avail is None else new_avail
    return {"replicas": replicas, "actual": replicas if actual is None else actual,
            "available": replicas if available is None else available,
            "updated_replicas": (new if updated else 0) if upd_r is None else upd_r,
            "updated_available": (new_avail if updated else 0) if upd_a is None else upd_a, "current_new": new,
            "current_new_available": new_avail, "max_surge": ms, "max_unavailable": mu, "desired": desired,
            "updated": updated, "exists": exists, "to_delete": to_delete}


def obj(replicas, max_surge, max_unavailable, targets, error=False):
    return (replicas, max_surge, max_unavailable, list(targets), error)


def from_golden(c):
    ts = sorted(c["targets"], key=lambda t: t["name"].encode())
    return obj(c["replicas"], c["max_surge"], c["max_unavailable"], [dict(t, exists=True, to_delete=False) for t in ts])


def pack(objs):
    """→ the keyword arguments of Context.rollout_plan / rollout_ref.run."""
    ts = [t for o in objs for t in o[3]]
    off = np.zeros(len(objs) + 1, np.int32)
    off[1:] = np.cumsum([len(o[3]) for o in objs])
    vals = np.array([[t[f] for t in ts] for f in R.FIELDS], np.int64).reshape(len(R.FIELDS), len(ts))
    flags = [(R.UPDATED if t["updated"] else 0) | (R.EXISTS if t["exists"] else 0) | (R.TO_DELETE if t["to_delete"] else 0) for t in ts]
    return {"obj_tgt_off": off, "obj_replicas": np.array([o[0] for o in objs], np.int64).astype(np.int32),
            "obj_max_surge": np.array([o[1] for o in objs], np.int64).astype(np.int32),
            "obj_max_unavailable": np.array([o[2] for o in objs], np.int64).astype(np.int32),
            "obj_flags": np.array([R.OBJ_ERROR if o[4] else 0 for o in objs], np.uint8),
            "tgt_vals": vals.astype(np.int32), "tgt_flags": np.array(flags, np.uint8)}


def random_obj(rng, n, wild=False):
    """n targets in every state a rollout passes through; ``wild``: values near the ends of int32."""
    ts = []
    for _ in range(n):
        if rng.random() < 0.08:  # no member object yet
            ts.append(tgt(0, int(rng.integers(1, 30)), exists=False))
            continue
        d = int(rng.integers(0, 40))
        r = d if rng.random() < 0.5 else int(rng.integers(0, 40))
        updated = bool(rng.random() < 0.5)
        new = int(rng.integers(0, r + 1)) if updated or rng.random() < 0.2 else r
        new_avail = max(0, new - int(rng.integers(0, 3)))
        actual = max(0, r + int(rng.integers(-1, 3))) if rng.random() < 0.3 else r
        available = max(0, min(actual, r) - int(rng.integers(0, 3))) if rng.random() < 0.3 else r
        t = tgt(r, d, updated, new, new_avail, actual, available, int(rng.integers(0, 6)), int(rng.integers(0, 6)))
        if rng.random() < 0.05:
            t.update(desired=0, to_delete=True)
        if wild:
            for f in R.FIELDS:
                if rng.random() < 0.3 and not (f == "desired" and t["to_delete"]):
                    t[f] = int(rng.choice([BIG, -BIG - 1, BIG - 7, -BIG + 3, 2 ** 30, -2 ** 30]))
        ts.append(t)
    total = sum(t["desired"] for t in ts if not wild)
    pct = [(0, 25), (25, 0), (25, 25), (10, 5)][int(rng.integers(0, 4))]
    ms, mu = -(-pct[0] * total // 100), pct[1] * total // 100
    if ms == 0 and mu == 0:
        mu = 1
    rep = total + int(rng.integers(-2, 3)) * int(rng.random() < 0.2)
    if wild:
        rep, ms, mu = (int(rng.choice([BIG, -BIG, 5, 0, 2 ** 30])) for _ in range(3))
    return obj(rep, ms, mu, ts)


def batch(lens, seed=0, wild=False):
    rng = np.random.default_rng([seed, 0x524F])
    return pack([random_obj(rng, int(n), wild) for n in lens])


def lengths(long_min):
    return list(range(0, 66)) + [63, 64, 65, long_min - 1, long_min, long_min + 1, 3 * 256 + 5]


def named():
    """name → object, each built to take one path; the tests assert that on the checker's answer."""
    steady = [tgt(10, 10, True, 10) for _ in range(2)]
    unit = dict(replicas=10, desired=10, updated=True, new=9)  # offers 1 to each budget in pass 3
    return {
        "ok": obj(30, 5, 0, [tgt(10, 10, True, 4, ms=2), tgt(10, 10), tgt(10, 10)]),
        "scale": obj(25, 0, 5, steady + [tgt(0, 5, exists=False)]),
        "invalid": obj(100, 0, 1, [tgt(5, 5), tgt(5, 5)]),
        "error": obj(0, 0, 0, [tgt(0, 0, exists=True), tgt(0, 0, exists=False)], error=True),
        # pass 1 gives the fenceposts, pass 4 the replicas
        "pass1+4": obj(20, 5, 0, [tgt(5, 10, True, 3), tgt(10, 10, True, 10)]),
        # pass 2 scales in with OnlyPatchReplicas, pass 5 adds the fenceposts and clears it
        "pass2+5": obj(15, 0, 5, [tgt(10, 5, True, 4, mu=2), tgt(10, 10, True, 10)]),
        "pass2-only": obj(25, 0, 5, [tgt(10, 5), tgt(10, 10), tgt(10, 10)]),
        "pass3": obj(20, 0, 5, [tgt(10, 10, True, 5, mu=3), tgt(10, 10)]),
        # a cluster without the object yet: created with the replicas pass 4 allows
        "pass4-only": obj(12, 5, 0, [tgt(0, 2, exists=False), tgt(10, 10, True, 5)]),
        # the surge budget is 64 and every target takes 1: it reaches zero after 64 targets, a chunk boundary of
        # every width
        "zero-at-64": obj(1300, 64, 0, [tgt(**unit) for _ in range(130)]),
        # both budgets negative before the first target
        "negative": obj(1300, 3, 2, [tgt(10, 10, True, 9, actual=11, available=9) for _ in range(130)]),
        "to-delete": obj(10, 0, 5, [tgt(10, 10, True, 10), tgt(5, 0, to_delete=True), tgt(0, 0, to_delete=True)]),
        "empty": obj(0, 0, 25, []),
    }


def shapes_case(long_min):
    """One batch with every length of ``lengths``, the named objects, ERROR objects (short and long) and objects
    that may wrap (short, of more than one chunk, long) between live ones → (arrays, marks: name → object index)."""
    rng = np.random.default_rng(0xC0FFEE)
    objs, marks = [], {}
    for n in lengths(long_min):
        objs.append(random_obj(rng, n))
    for name, o in named().items():
        marks[name] = len(objs)
        objs.append(o)
    for name, n in (("error-long", long_min + 9), ("wild", 5), ("wild-chunks", 70), ("wild-long", long_min + 3)):
        marks[name] = len(objs)
        o = random_obj(rng, n, wild=name.startswith("wild"))
        objs.append(obj(o[0], o[1], o[2], o[3], error=name.startswith("error")))
        objs.append(random_obj(rng, 7))
    for k in range(6):
        objs.append(random_obj(rng, int(rng.integers(1, 9)), wild=True))
        objs.append(random_obj(rng, int(rng.integers(1, 9))))
    return pack(objs), marks
