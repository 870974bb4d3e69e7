"""Object-by-object checker for rollout planning, restated from the reference (pkg/controllers/util/rolloutplan.go:
58-867, pkg/controllers/sync/dispatch/managed.go:219-249): the serial walk over an object's targets in Go's wrapping
int32, with plain Python integers. Two levels: ``plan`` takes one planner (targets as dicts) and returns the
reference's RolloutPlans as a dict; ``run`` walks kad_rollout_plan's columns. Shares no code with
kubeadmiral_amd/rollout.py."""

UPDATED, EXISTS, TO_DELETE = 1, 2, 4
PLANNED, HAS_REPLICAS, HAS_SURGE, HAS_UNAVAILABLE, ONLY_PATCH_REPLICAS = 1, 2, 4, 8, 16
KEEP_TEMPLATE_PATCH, NONE, DELETE, CREATE, PATCH_REPLICAS, UPDATE = range(6)
OK, SCALE, INVALID, ERROR = range(4)
OBJ_ERROR = 1
FIELDS = ("replicas", "actual", "available", "updated_replicas", "updated_available", "current_new",
          "current_new_available", "max_surge", "max_unavailable", "desired")  # the rows of tgt_vals


def w32(v):
    """Go's int32 result of an exact integer."""
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


class Target:
    """TargetInfo (:179-362)."""

    def __init__(self, t):
        self.name = t.get("name", "")
        self.updated = bool(t["updated"])
        for f in FIELDS:
            setattr(self, f, int(t[f]))

    def to_update(self):
        return max(w32(self.replicas - self.updated_replicas), 0)

    def to_updated_available(self):
        return max(w32(self.replicas - self.updated_available), 0)

    def to_update_currently(self):
        return max(w32(self.replicas - self.current_new), 0)

    def to_updated_available_currently(self):
        return max(w32(self.replicas - self.current_new_available), 0)

    def during_updating(self):
        if self.current_new < self.replicas:
            return True
        return self.updated and self.to_update() > 0

    def update_completed(self):
        return self.to_update() == 0

    def is_surge(self):
        return self.max_surge != 0 and self.max_unavailable == 0

    def flip(self, default_is_surge):
        return self.is_surge() and not default_is_surge and self.to_updated_available() > 0

    def least_surge(self):
        res = max(w32(self.actual - self.replicas), 0)
        if not self.during_updating():
            return res
        return max(res, min(self.max_surge, w32(res + self.to_update_currently())))

    def least_unavailable(self):
        res = max(w32(self.replicas - self.available), 0)
        if not self.during_updating():
            return res
        return max(res, min(self.max_unavailable, self.to_updated_available_currently()))

    def fence_surge(self, m, least):
        res = max(min(w32(m + least), self.to_update()), 0)
        more = max(w32(res - least), 0)
        if m < 0 and least > self.max_surge and res > self.max_surge:
            res = self.max_surge
        return res, more

    def fence_unavailable(self, m, least):
        res = max(min(w32(m + least), self.to_updated_available()), 0)
        more = max(w32(res - least), 0)
        if m < 0 and least > self.max_unavailable and res > self.max_unavailable:
            res = self.max_unavailable
        return res, more

    def scale_out(self, m, least):
        res = max(min(w32(m + least), w32(self.desired - self.replicas)), 0)
        return res, max(w32(res - least), 0)

    def scale_in(self, m, least):
        res = min(w32(m + least), w32(self.replicas - self.desired))
        if res > self.replicas:
            res = self.replicas
        res = max(res, 0)
        return res, max(w32(res - least), 0)

    def skip_update(self, s, u):
        return (s <= 0 and u <= 0 and not self.updated and not self.during_updating() and self.least_surge() <= 0
                and self.least_unavailable() <= 0)

    def skip_update_scale_in(self, s, u, least_unavailable):
        if s <= 0 and u <= 0 and not self.updated and not self.during_updating():
            if least_unavailable > 0:
                return False
            least_surge = self.least_surge()
            if self.desired < self.replicas:
                least_surge = 0
            return not least_surge > 0
        return False


def _correct(p, t, default_is_surge):
    """correctFencepost (:93-112)."""
    if t.update_completed() and not t.flip(default_is_surge):
        p["max_surge"] = p["max_unavailable"] = None
    elif p["max_surge"] == 0 and p["max_unavailable"] == 0:
        if t.is_surge():
            p["max_surge"] = 1
        else:
            p["max_unavailable"] = 1


def _new(replicas=None, only=False):
    return {"replicas": replicas, "max_surge": None, "max_unavailable": None, "only_patch_replicas": only}


def plan_status(replicas, max_surge, max_unavailable, targets):
    """RolloutPlanner.Plan (:569-695) → (plans by position in the sorted order, status). ``targets`` sorted by name."""
    ts = [Target(t) for t in targets]
    change = [w32(t.desired - t.replicas) for t in ts]
    to_update = [i for i, c in enumerate(change) if c == 0]
    to_out = [i for i, c in enumerate(change) if c > 0]
    to_in = [i for i, c in enumerate(change) if c < 0]
    p_surge = max_surge != 0 and max_unavailable == 0
    if bool(to_out) != bool(to_in) and all(t.update_completed() and not t.flip(p_surge) for t in ts):
        return {i: _new() for i in range(len(ts))}, SCALE
    cur = occ_s = occ_u = 0
    for t in ts:
        cur = w32(cur + t.replicas)
        occ_s = w32(occ_s + t.least_surge())
        occ_u = w32(occ_u + t.least_unavailable())
    s = w32(w32(max_surge - w32(cur - replicas)) - occ_s)
    u = w32(w32(max_unavailable - w32(replicas - cur)) - occ_u)
    plans = {}

    def fenceposts(i, p, s, u, lu):
        t = ts[i]
        p["max_surge"], sm = t.fence_surge(s, t.least_surge())
        p["max_unavailable"], um = t.fence_unavailable(u, lu)
        _correct(p, t, p_surge)
        plans[i] = p
        return w32(s - sm), w32(u - um)

    for i in to_out:
        if not ts[i].skip_update(s, u):
            s, u = fenceposts(i, _new(ts[i].replicas), s, u, ts[i].least_unavailable())
    for i in to_in:
        t = ts[i]
        if u <= 0 and t.least_unavailable() <= 0:
            continue
        scale, more = t.scale_in(u, 0 if t.during_updating() else t.least_unavailable())
        u = w32(u - more)
        plans[i] = _new(w32(t.replicas - scale), True)
    for i in to_update:
        if not ts[i].skip_update(s, u):
            s, u = fenceposts(i, _new(), s, u, ts[i].least_unavailable())
    for i in to_out:
        t = ts[i]
        if s <= 0 and t.least_surge() <= 0:
            continue
        if not t.updated and t.replicas != 0:
            continue
        scale, more = t.scale_out(s, 0 if t.during_updating() else t.least_surge())
        s = w32(s - more)
        plans.setdefault(i, _new())["replicas"] = w32(t.replicas + scale)
    for i in to_in:
        t = ts[i]
        p = plans.get(i) or _new(t.replicas)
        lu = t.least_unavailable()
        if not t.during_updating():
            lu = max(w32(lu - w32(t.replicas - p["replicas"])), 0)
        if t.skip_update_scale_in(s, u, lu):
            continue
        p["only_patch_replicas"] = False
        s, u = fenceposts(i, p, s, u, lu)
    # validatePlans (:831-867)
    planned = desired = 0
    for i, t in enumerate(ts):
        desired = w32(desired + t.desired)
        r = t.replicas
        if i in plans:
            r = plans[i]["replicas"] if plans[i]["replicas"] is not None else t.desired
        planned = w32(planned + r)
    lo, hi = (cur, desired) if desired > cur else (desired, cur)
    if w32(replicas - desired) > max_unavailable or w32(lo - planned) > max_unavailable or w32(planned - hi) > max_surge:
        return {}, INVALID
    return plans, OK


def plan(replicas, max_surge, max_unavailable, targets):
    """The reference's RolloutPlans by cluster name; the targets in any order."""
    ts = sorted(targets, key=lambda t: t["name"].encode())
    plans, _ = plan_status(replicas, max_surge, max_unavailable, ts)
    return {ts[i]["name"]: p for i, p in plans.items()}


def action(flags, p):
    """managed.go:219-249 for one cluster; p is its plan or None."""
    if p is None:
        return KEEP_TEMPLATE_PATCH if flags & EXISTS else NONE
    if flags & TO_DELETE and (p["replicas"] is None or p["replicas"] == 0):
        return DELETE
    if not flags & EXISTS:
        return CREATE
    if p["only_patch_replicas"] and p["replicas"] is not None:
        return PATCH_REPLICAS
    return UPDATE


def run(obj_tgt_off, obj_max_surge, obj_max_unavailable, obj_replicas, obj_flags, tgt_vals, tgt_flags):
    """kad_rollout_plan's outputs from its columns, as lists."""
    T = len(tgt_flags)
    vals = [[int(v) for v in row] for row in tgt_vals] if T else [[] for _ in FIELDS]
    out = {k: [0] * T for k in ("replicas", "max_surge", "max_unavailable", "plan_flags", "action")}
    out["status"] = []
    for o in range(len(obj_flags)):
        lo, hi = int(obj_tgt_off[o]), int(obj_tgt_off[o + 1])
        if int(obj_flags[o]) & OBJ_ERROR:
            plans, st = {}, ERROR
        else:
            ts = [dict({f: vals[k][i] for k, f in enumerate(FIELDS)}, updated=int(tgt_flags[i]) & UPDATED) for i in range(lo, hi)]
            plans, st = plan_status(int(obj_replicas[o]), int(obj_max_surge[o]), int(obj_max_unavailable[o]), ts)
        out["status"].append(st)
        for i in range(lo, hi):
            p = plans.get(i - lo)
            out["action"][i] = action(int(tgt_flags[i]), p)
            if p is None:
                continue
            f = PLANNED | (ONLY_PATCH_REPLICAS if p["only_patch_replicas"] else 0)
            for key, bit in (("replicas", HAS_REPLICAS), ("max_surge", HAS_SURGE), ("max_unavailable", HAS_UNAVAILABLE)):
                if p[key] is not None:
                    f |= bit
                    out[key][i] = p[key]
            out["plan_flags"][i] = f
    return out
